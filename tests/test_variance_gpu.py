"""The streaming pair statistics (dv_pairstat_accum_f32), their host module (dualvar_amd/utils/variance.py) and
`classifier.py --retrieval --variance` against float64 references written here from include/dualvar_pairstat.h.

Conventions (those of tests/test_loss_gemm_optim_gpu.py; the helpers are tests/checks.py's): the state sits in buffers filled with a NaN
bit pattern no kernel produces and larger than needed (a fourth row behind hist / sums / ext, ldh = bins + 3, 64 bytes behind the
workspace): after every call everything beyond hist[c][0..bins], sums [3][4] and ext [3][2] must still hold it.  The similarity
carries NaN in sim[:, n_cols:ld).  Three layouts: ld = n_cols on an aligned base (16-byte loads iff n_cols % 4 == 0),
ld = n_cols + 3 on a base 4 bytes off alignment (always the 4-byte path), ld = the next multiple of 4 above n_cols, plus 4, on an
aligned base (always 16-byte loads, the last quad of a row partly padding).

Reference (state_ref): categories and self pairs from the ids in int64; bins from the header's fp32 expression in torch on the
host, (s + 1.0f) * (0.5f * bins) then floor and clamp, every step one IEEE operation; sums in float64 of the exact argument
x = (s - 1) * 2t (math.fsum up to 4096 terms, torch.sum beyond).  hist (with the non-finite column) and ext must match as bits in
every case.  Bounds, u64 = 2^-53, u = 2^-24, N_c = the finite pairs of the category:
  sum s, sum s^2:  |err| <= (N_c - 1) u64 sum|term|      (any order of N_c - 1 additions; s and s*s are exact in double)
  sum w:           |err| <= sum w_i (E_EXPF + 2u |x_i|) + (N_c - 1) u64 sum w      (two fp32 roundings in x_i, then expf)
all times mult.  pair_statistics is compared with float64 products of the normalised features taken to float64 (the fp32 rows
the library's own centring and dv_l2norm_fwd formed, as tests/test_knn_gpu.py does for knn_eval: gemm_bound is a statement about
the product of those rows): |s_i - s64_i| <= g_i = gemm_bound, hence |d mean|, |d std|, |d min|, |d max| <= max g,
|d w_i| <= w_i (E_EXPF + 2u |x_i| + expm1(2t g_i)), and the histogram is compared cumulatively: a pair within g_i + 4u of a bin
edge may fall on either side (4u: the two fp32 roundings of the bin expression on |s + 1| <= 2).
Each case prints (-s) err / bound.  Largest err / bound measured on an MI355X: accum sum s 0.000 (fp32 values of like magnitude
add exactly in double), sum s^2 0.296, sum w 0.407 (R = 1, n = 63; 0.06 on the 130 x 1000 blocks); pair_statistics mean 0.003,
std 0.001, min 0.057, max 0.046, sum w 0.004; 10 of 16 770 pairs undecidable at a bin edge with centring, 0 without, 1 of 3 900
in the cross case.  The whole file takes 17 s, 11 s of it the two classifier.py children; every other test is below 0.5 s.
"""
import functools
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from tests import checks  # noqa: E402
from tests.chains import E_EXPF, gemm_bound, gemm_chain  # noqa: E402
from tests.checks import U, Ratios, child as _child, f32, is_sent, sent  # noqa: E402
from tests.dataset_support import write_dataset  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
U64 = 2.0 ** -53
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
NO_SELF = -(1 << 40)
RATIO = Ratios()                   # cleared per test: each prints its own figures
within = RATIO.within
# bit for bit against float64: the reference must be an fp32 number; + 0.0 on both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)


# --------------------------------------------------------------------------------------------------------------- reference
def categories(rv, rc, cv, cc):
    """[R, n] category of every pair, ids compared in int64"""
    same_v = rv.long()[:, None] == cv.long()[None, :]
    same_c = rc.long()[:, None] == cc.long()[None, :]
    return torch.where(same_v, 0, torch.where(same_c, 1, 2))


def kept(R, n, diag):
    """[R, n] False on the self pairs j == r + diag"""
    return torch.arange(n)[None, :] != torch.arange(R)[:, None] + diag


def bin_ref(s, bins):
    """the header's bin of fp32 values, in fp32 on the host, each step a single IEEE operation; bins for a non-finite value"""
    assert s.dtype == torch.float32 and not s.is_cuda
    fin = torch.isfinite(s)
    x = (torch.where(fin, s, torch.zeros_like(s)) + 1.0) * (0.5 * bins)
    assert x.dtype == torch.float32
    return torch.where(fin, torch.floor(x).clamp(0, bins - 1).long(), torch.full(s.shape, bins))


def exact_sum(v):
    return math.fsum(v.tolist()) if v.numel() <= 4096 else float(v.sum())


def state_ref(s, ids, diag, mult, t, bins):
    """s [R, n] fp32 on the host, ids = (row_vid, row_cls, col_vid, col_cls) -> {'hist' [3, bins + 1] i64, 'ext' [3, 2] f64,
    'sums' [3, 4] f64, 'bound' [3, 4] f64, 'n' [3]} of the header comment"""
    R, n = s.shape
    cat, keep, fin = categories(*ids), kept(R, n, diag), torch.isfinite(s)
    hist = torch.bincount((cat * (bins + 1) + bin_ref(s, bins))[keep], minlength=3 * (bins + 1)).view(3, bins + 1) * mult
    s64 = s.double()
    x64 = (s64 - 1.0) * (2.0 * f32(t))
    sums, bound, ext, cnt = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64), []
    for c in range(3):
        m = keep & fin & (cat == c)
        N = int(m.sum())
        cnt.append(N)
        sv, xv = s64[m], x64[m]
        wv = torch.exp(xv)
        chain = max(N - 1, 0) * U64
        a1, a2, aw = exact_sum(sv.abs()), exact_sum(sv * sv), exact_sum(wv)
        sums[c] = torch.tensor([exact_sum(sv), a2, aw, 0.0], dtype=torch.float64) * mult
        bound[c] = torch.tensor([chain * a1, chain * a2, exact_sum(wv * (E_EXPF + 2 * U * xv.abs())) + chain * aw, 0.0], dtype=torch.float64) * mult
        ext[c] = torch.tensor([float(sv.min()), float(sv.max())] if N else [INF, -INF], dtype=torch.float64)
    return {'hist': hist, 'ext': ext, 'sums': sums, 'bound': bound, 'n': cnt}


def add_refs(refs):
    """the reference of a sequence of calls: counts and sums add (so do their bounds: the chain bound of the union is no smaller
    than the sum of the parts'), extrema fold"""
    out = {'hist': sum(r['hist'] for r in refs), 'sums': sum(r['sums'] for r in refs), 'n': [sum(r['n'][c] for r in refs) for c in range(3)]}
    out['ext'] = torch.stack([torch.stack([r['ext'][:, 0] for r in refs]).min(0).values, torch.stack([r['ext'][:, 1] for r in refs]).max(0).values], 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ harness
class State:
    """hist [3][ldh] u64, sums [3][4] f64, ext [3][2] f32 inside sentinel buffers with one more row and ldh = bins + 3"""

    def __init__(self, bins, dev):
        self.bins, self.ldh = bins, bins + 3
        self.hist = sent((4, 2 * self.ldh), dev, torch.int32).view(torch.int64)
        self.sums = sent((4, 8), dev, torch.int32).view(torch.float64)
        self.ext = sent((4, 2), dev)
        assert self.hist.shape == (4, self.ldh) and self.sums.shape == (4, 4)

    def frame_ok(self):
        """(the 8-byte words hold the int32 sentinel twice: they are checked through int32 views)"""
        w32 = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
        return (is_sent(w32(self.hist[3:])) and is_sent(w32(self.hist[:3, self.bins + 1:])) and is_sent(w32(self.sums[3:]))
                and is_sent(self.ext[3:]))

    def bits(self):
        """the whole state as integers, for bit comparisons"""
        return (self.hist[:3, :self.bins + 1].clone(), self.sums[:3].clone().view(torch.int64), self.ext[:3].clone().view(torch.int32))

    def check_exact(self, ref, what):
        assert self.frame_ok(), what + ': wrote outside the state'
        got = self.hist[:3, :self.bins + 1].cpu()
        assert torch.equal(got, ref['hist']), '%s: hist differs\n got %s\nwant %s' % (what, got.tolist(), ref['hist'].tolist())
        same_bits(self.ext[:3].cpu(), ref['ext'], what + ' ext')
        assert bool((self.sums[:3, 3] == 0).all()), what + ': sums[c][3] is not 0'

    def check(self, ref, what):
        self.check_exact(ref, what)
        got = self.sums[:3, :3].cpu()
        for k, name in enumerate(('sum_s', 'sum_s2', 'sum_w')):
            within(got[:, k], ref['sums'][:, k], ref['bound'][:, k], 'accum.%s %s' % (name, what), key='accum.' + name, quiet=True)


def layout(s, kind, dev):
    """s [R, n] on the host -> (device tensor that owns the memory, pointer of element (0, 0), ld); NaN everywhere else"""
    R, n = s.shape
    ld, off = {'tight': (n, 0), 'odd': (n + 3, 1), 'quad': ((n + 3) // 4 * 4 + 4, 0)}[kind]
    flat = torch.full((off + R * ld + 4,), float('nan'), dtype=torch.float32, device=dev)
    flat[off:off + R * ld].view(R, ld)[:, :n] = s.to(dev)
    ptr = flat.data_ptr() + 4 * off
    assert flat.data_ptr() % 16 == 0 and (ptr % 16 == 0) == (kind != 'odd')
    return flat, ptr, ld


def accum(st, ptr, ld, R, n, ids_dev, diag, mult, t, first, r0=0, c0=0):
    """one dv_pairstat_accum_f32 call on rows [r0, r0 + R) x columns [c0, c0 + n) of the block at ptr; diag is the block's"""
    lib = _lib.load()
    nbytes = lib.dv_pairstat_workspace(R, n)
    assert nbytes > 0 and nbytes % 96 == 0
    ws = sent((nbytes // 4 + 16,), st.hist.device, torch.int32)
    rv, rc, cv, cc = ids_dev
    ops.call('dv_pairstat_accum_f32', ptr + 4 * (r0 * ld + c0), ld, R, n, rv.data_ptr() + 4 * r0, rc.data_ptr() + 4 * r0,
             cv.data_ptr() + 4 * c0, cc.data_ptr() + 4 * c0, diag + r0 - c0, mult, t, st.bins, st.sums, st.ext, st.hist, st.ldh, ws, first)
    assert is_sent(ws[nbytes // 4:]), 'wrote behind the workspace'
    assert st.frame_ok(), 'wrote outside the state'


# --------------------------------------------------------------------------------------------------------------------- data
def make_ids(kind, R, n, gen):
    """(row_vid, row_cls, col_vid, col_cls) int32 on the host"""
    if kind == 'mixed':                  # a handful of videos over three classes: all three categories occur in larger blocks
        rv, cv = torch.randint(0, 6, (R,), generator=gen), torch.randint(0, 6, (n,), generator=gen)
        ids = (rv, rv % 3, cv, cv % 3)
    elif kind == 'one_video':            # every pair is same-video
        ids = (torch.full((R,), 7), torch.full((R,), 1), torch.full((n,), 7), torch.full((n,), 2))
    elif kind == 'all_distinct':         # no two ids alike: categories 0 and 1 stay empty
        ids = (torch.arange(R), torch.arange(R) + 50000, torch.arange(n) + 100000, torch.arange(n) + 150000)
    else:                                # 'extreme': negative ids and the ends of int32
        pool_v = torch.tensor([-5, INT32_MAX, INT32_MIN, 0, -1])
        pool_c = torch.tensor([-1, INT32_MAX, INT32_MIN])
        rv, cv = torch.randint(0, 5, (R,), generator=gen), torch.randint(0, 5, (n,), generator=gen)
        ids = (pool_v[rv], pool_c[rv % 3], pool_v[cv], pool_c[cv % 3])
    return tuple(v.to(torch.int32) for v in ids)


def make_sim(kind, R, n, gen, cat=None, keep=None):
    """[R, n] fp32 on the host"""
    if kind == 'grid':                   # multiples of 1/32 in [-1, 1]: every value on a bin edge at 64 bins, s = 1 included
        return torch.randint(-32, 33, (R, n), generator=gen).float() / 32
    if kind == 'outside':                # the ends, and values just and well beyond them
        pool = torch.tensor([1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, 1.25, -1.25, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24, 0.0, -0.0])
        return pool[torch.randint(0, pool.numel(), (R, n), generator=gen)]
    x = torch.randn((R, n), generator=gen)
    s = (x / x.abs().max()).float()      # Gaussian, scaled into [-1, 1]
    if kind == 'nonfinite':              # NaN, +inf, -inf planted in each category (as far as it has pairs)
        for c in range(3):
            at = ((cat == c) & keep).nonzero()
            for q, v in enumerate((float('nan'), INF, -INF, float('nan'))):
                if q < at.shape[0]:
                    r, j = at[(q * 7919) % at.shape[0]].tolist()
                    s[r, j] = v
    return s


def diag_of(kind, R, n, i):
    if kind == 'zero':
        return 0
    if kind == 'positive':               # inside the block (0 for a single column)
        return min(2, n - 1)
    if kind == 'negative':
        return -min(2, R - 1)
    return (n + 5, -(R + 5), 1 << 40, NO_SELF)[i % 4]                       # 'outside': no self pair


SIM_KINDS = ('grid', 'outside', 'gauss', 'nonfinite')
ID_KINDS = ('mixed', 'one_video', 'all_distinct', 'extreme')
DIAG_KINDS = ('zero', 'positive', 'negative', 'outside')
SHAPES = [(R, n) for R in (1, 3, 67, 130) for n in (1, 63, 65, 257, 1000)]


# ------------------------------------------------------------------------------------------- 1. one call, every shape and path
@pytest.mark.parametrize('R,n', SHAPES, ids=['R%d-n%d' % s for s in SHAPES])
def test_accum_one_call(gpu, R, n):
    """(R, n) x {ld = n, ld = n + 3 misaligned, ld a multiple of 4 with padding} x bins {1, 2, 64, 256} x the four diag kinds x
    mult {1, 2}; the data kind and the id pattern rotate so that each meets every bins / diag / mult / layout"""
    gen = torch.Generator().manual_seed(1000 * R + n)
    RATIO.clear()
    i = 0
    empty_seen = False
    for lay in ('tight', 'odd', 'quad'):
        for bins in (1, 2, 64, 256):
            for dk in DIAG_KINDS:
                for mult in (1, 2):
                    sim_kind, id_kind = SIM_KINDS[(i + i // 4) % 4], ID_KINDS[(i // 2 + i // 16) % 4]
                    diag = diag_of(dk, R, n, i)
                    t = (2.0, 0.0, 0.5, 7.0)[(i // 8) % 4]
                    ids = make_ids(id_kind, R, n, gen)
                    s = make_sim(sim_kind, R, n, gen, categories(*ids), kept(R, n, diag))
                    ref = state_ref(s, ids, diag, mult, t, bins)
                    what = 'R=%d n=%d %s bins=%d diag=%s(%d) mult=%d %s %s t=%g' % (R, n, lay, bins, dk, diag, mult, sim_kind, id_kind, t)
                    # what the header promises about the reference itself
                    n_self = int((~kept(R, n, diag)).sum())
                    assert int(ref['hist'].sum()) == mult * (R * n - n_self), what
                    assert (n_self > 0) == (dk != 'outside'), what
                    if id_kind == 'one_video':
                        assert ref['n'][1] == ref['n'][2] == 0 and int(ref['hist'][1:].sum()) == 0
                    if id_kind == 'all_distinct':
                        assert ref['n'][0] == ref['n'][1] == 0 and bool((ref['ext'][:2] == torch.tensor([INF, -INF])).all())
                        assert bool((ref['sums'][:2] == 0).all())
                        empty_seen = True
                    if sim_kind == 'nonfinite' and R * n - n_self >= 3:
                        assert int(ref['hist'][:, bins].sum()) >= 3 * mult, what
                    if sim_kind == 'grid' and bins == 64:                    # on the edges: the value IS its bin's lower edge
                        assert torch.equal(bin_ref(s, 64), ((s.double() + 1) * 32).long().clamp(max=63))
                    st = State(bins, gpu)
                    keepalive, ptr, ld = layout(s, lay, gpu)
                    accum(st, ptr, ld, R, n, tuple(v.to(gpu) for v in ids), diag, mult, t, 1)
                    st.check(ref, what)
                    i += 1
    assert empty_seen and i == 96
    print('    R=%d n=%d: %d calls, largest err / bound %s' % (R, n, i, ', '.join('%s %.3f' % kv for kv in sorted(RATIO.items()))))


def test_bin_edges_and_clamp(gpu):
    """every multiple of 1/32 in [-1, 1] lands in the bin whose lower edge it is, 1.0 in the last; values outside in the end bins"""
    vals = torch.cat([torch.arange(-32, 33).float() / 32, torch.tensor([1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, 3.0e38, -3.0e38, 100.0, -7.5])])
    n = vals.numel()
    ids = make_ids('one_video', 1, n, None)
    st = State(64, gpu)
    keepalive, ptr, ld = layout(vals[None, :], 'odd', gpu)
    accum(st, ptr, ld, 1, n, tuple(v.to(gpu) for v in ids), NO_SELF, 1, 0.0, 1)
    want = torch.zeros(3, 65, dtype=torch.int64)
    want[0, :64] = 1
    want[0, 63] += 1 + 3                                                    # 1.0, and the three values above it
    want[0, 0] += 3
    assert torch.equal(st.hist[:3, :65].cpu(), want)
    same_bits(st.ext[:1].cpu(), torch.tensor([[-3.0e38, 3.0e38]]).float().double(), 'ext of the clamp case')
    assert torch.equal(torch.bincount(bin_ref(vals, 64), minlength=65), want[0])      # the reference agrees with the hand count


# ----------------------------------------------------------------------------------- 2. accumulation over calls, determinism
def accumulation_case(gpu):
    R, n = 67, 300
    gen = torch.Generator().manual_seed(77)
    ids = make_ids('mixed', R, n, gen)
    diag = 3
    s = make_sim('nonfinite', R, n, gen, categories(*ids), kept(R, n, diag))
    return R, n, ids, diag, s


@pytest.mark.parametrize('mult', [1, 2])
def test_accumulation_over_calls(gpu, mult):
    """one call over [R, n] against the same block walked in column chunks of 1, 7 and 64 (`first` on the first chunk only) and
    split by rows with diag adjusted: hist and ext identical, sums within the bounds of the whole"""
    R, n, ids, diag, s = accumulation_case(gpu)
    t, bins = 2.0, 64
    ref = state_ref(s, ids, diag, mult, t, bins)
    assert min(ref['n']) > 100 and int(ref['hist'][:, bins].sum()) >= 9 * mult and int((~kept(R, n, diag)).sum()) == R
    ids_dev = tuple(v.to(gpu) for v in ids)
    RATIO.clear()
    for lay in ('tight', 'odd'):
        keepalive, ptr, ld = layout(s, lay, gpu)
        whole = State(bins, gpu)
        accum(whole, ptr, ld, R, n, ids_dev, diag, mult, t, 1)
        whole.check(ref, 'whole %s' % lay)
        for m in (1, 7, 64):
            st = State(bins, gpu)
            for k, c0 in enumerate(range(0, n, m)):
                accum(st, ptr, ld, R, min(m, n - c0), ids_dev, diag, mult, t, int(k == 0), c0=c0)
            st.check(ref, 'column chunks of %d %s' % (m, lay))
            assert torch.equal(st.bits()[0], whole.bits()[0]) and torch.equal(st.bits()[2], whole.bits()[2])
        for cuts in ((0, 30, R), (0, 1, 2, 66, R)):
            st = State(bins, gpu)
            for k in range(len(cuts) - 1):
                accum(st, ptr, ld, cuts[k + 1] - cuts[k], n, ids_dev, diag, mult, t, int(k == 0), r0=cuts[k])
            st.check(ref, 'row cuts %s %s' % (cuts, lay))
            assert torch.equal(st.bits()[0], whole.bits()[0]) and torch.equal(st.bits()[2], whole.bits()[2])
    # the parts' references add up to the whole's (the reference of a chunked walk is the reference of the block)
    parts = add_refs([state_ref(s[:, c0:c0 + 64], (ids[0], ids[1], ids[2][c0:c0 + 64], ids[3][c0:c0 + 64]), diag - c0, mult, t, bins)
                      for c0 in range(0, n, 64)])
    assert torch.equal(parts['hist'], ref['hist']) and torch.equal(parts['ext'], ref['ext']) and parts['n'] == ref['n']
    print('    accumulation mult=%d: largest err / bound %s' % (mult, ', '.join('%s %.3f' % kv for kv in sorted(RATIO.items()))))


def test_same_calls_same_bits(gpu):
    """the same sequence of calls, run twice, leaves the same bits in the whole state (no floating-point atomics; the partials
    are folded in workgroup order).  Two runs, not a hunt."""
    R, n, ids, diag, s = accumulation_case(gpu)
    big = torch.Generator().manual_seed(5)
    sb = make_sim('gauss', 130, 5000, big)                                  # several tiles per row of tiles, more than one workgroup
    idb = make_ids('mixed', 130, 5000, big)
    runs = []
    for _ in range(2):
        st, stb = State(64, gpu), State(256, gpu)
        keepalive, ptr, ld = layout(s, 'odd', gpu)
        ids_dev = tuple(v.to(gpu) for v in ids)
        accum(st, ptr, ld, R, n, ids_dev, diag, 2, 2.0, 1)
        for c0 in range(0, n, 7):
            accum(st, ptr, ld, R, min(7, n - c0), ids_dev, diag, 1, 2.0, 0, c0=c0)
        keepb, ptrb, ldb = layout(sb, 'tight', gpu)
        accum(stb, ptrb, ldb, 130, 5000, tuple(v.to(gpu) for v in idb), 0, 1, 2.0, 1)
        runs.append(st.bits() + stb.bits())
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    stb.check(state_ref(sb, idb, 0, 1, 2.0, 256), 'R=130 n=5000 tight')


# --------------------------------------------------------------------------------------------------- 3. pair_statistics
CACHE = {}


def clip_case(gpu):
    """130 clips = 13 videos x 10 clips over 4 classes, D = 64: class centre + video centre + clip noise"""
    if 'clips' not in CACHE:
        gen = torch.Generator().manual_seed(2025)
        n_video, num_seq, D = 13, 10, 64
        label = torch.arange(n_video) % 4
        feat = (torch.randn((4, D), generator=gen)[label][:, None, :] + 0.8 * torch.randn((n_video, 1, D), generator=gen)
                + 0.6 * torch.randn((n_video, num_seq, D), generator=gen))
        vid = torch.arange(n_video).repeat_interleave(num_seq)
        CACHE['clips'] = (feat.to(gpu), label, vid.int(), label.repeat_interleave(num_seq).int())
    return CACHE['clips']


def pairs_ref64(zq, zb, ids, diag, t, bins):
    """zq [R, D], zb [n, D] float64 (the normalised fp32 rows) on the host -> the float64 pair values per category with their
    gemm bounds, and the report figures they give"""
    R, n = zq.shape[0], zb.shape[0]
    s64 = zq @ zb.t()
    g = gemm_bound(zq, zb, 1.0, gemm_chain(R, n, zq.shape[1], 'tile4'))     # every block of these walks takes the tile4 form
    cat, keep = categories(*ids), kept(R, n, diag)
    out = {'s': [], 'g': [], 'n': []}
    for c in range(3):
        m = keep & (cat == c)
        out['s'].append(s64[m])
        out['g'].append(g[m])
        out['n'].append(int(m.sum()))
    return out


def check_against_float64(state, ref, t, bins, what):
    from dualvar_amd.utils.variance import CATEGORIES, report_from_state
    sums, ext, hist = state
    assert sums.shape == (3, 4) and sums.dtype == torch.float64 and ext.shape == (3, 2) and ext.dtype == torch.float32
    assert hist.shape == (3, bins + 1) and hist.dtype == torch.int64 and not sums.is_cuda
    rep = report_from_state(sums, ext, hist, bins, t)
    und_total, pairs_total, worst = 0, 0, {}
    edges = -1.0 + 2.0 * torch.arange(1, bins, dtype=torch.float64) / bins
    for c, name in enumerate(CATEGORIES):
        s, g, N = ref['s'][c], ref['g'][c], ref['n'][c]
        got = rep['categories'][name]
        assert got['count'] == N and got['skipped'] == 0 and int(hist[c].sum()) == N, (what, name)       # from the ids alone
        assert N > 0
        gmax = float(g.max())
        mean64, std64 = float(s.mean()), float(s.std(unbiased=False))
        for key, v64 in (('mean', mean64), ('std', std64), ('min', float(s.min())), ('max', float(s.max()))):
            r = abs(got[key] - v64) / (gmax + 1e-12)
            worst['pair_statistics.' + key] = max(worst.get('pair_statistics.' + key, 0.0), r)
            assert r <= 1.0, (what, name, key, got[key], v64, gmax)
        # sum s, sum s^2: every term moves by at most g (s^2: 2|s| g + g^2), plus the chain of the double sum
        chain = (N - 1) * U64
        b1 = float(g.sum()) + chain * float(s.abs().sum())
        b2 = float((2 * s.abs() * g + g * g).sum()) + chain * float((s * s).sum())
        assert abs(float(sums[c, 0]) - float(s.sum())) <= b1 and abs(float(sums[c, 1]) - float((s * s).sum())) <= b2, (what, name)
        x = (s - 1.0) * (2.0 * f32(t))
        w = torch.exp(x)
        bw = float((w * (E_EXPF + 2 * U * x.abs() + torch.expm1(2.0 * f32(t) * g))).sum()) + chain * float(w.sum())
        r = abs(float(sums[c, 2]) - float(w.sum())) / bw
        worst['pair_statistics.sum_w'] = max(worst.get('pair_statistics.sum_w', 0.0), r)
        assert r <= 1.0, (what, name, 'sum w', r)
        # histogram, cumulatively: pairs at or above each edge, undecidable within g + 4u of it
        above = (s[None, :] >= edges[:, None]).sum(1)                      # [bins - 1]
        und = ((s[None, :] - edges[:, None]).abs() <= (g + 4 * U)[None, :]).sum(1)
        got_above = hist[c, :bins].flip(0).cumsum(0).flip(0)[1:]            # pairs in bins >= k, k = 1 .. bins - 1
        assert bool(((got_above - above).abs() <= und).all()), (what, name, (got_above - above).abs().max(), und.max())
        und_total, pairs_total = und_total + int(und.sum()), pairs_total + N
    assert und_total <= 0.01 * pairs_total, 'more than 1 %% of the pairs lie within their bound of a bin edge: take another seed (%d of %d)' % (und_total, pairs_total)
    # the derived figures: 1 - mean moves by at most max g of the pairs behind it
    g01 = max(float(ref['g'][1].max()), float(ref['g'][2].max()))
    m12 = float(torch.cat([ref['s'][1], ref['s'][2]]).mean())
    want = {'var_intra_video': (1 - float(ref['s'][0].mean()), float(ref['g'][0].max())), 'var_inter_video': (1 - m12, g01),
            'var_intra_class': (1 - float(ref['s'][1].mean()), float(ref['g'][1].max())),
            'var_inter_class': (1 - float(ref['s'][2].mean()), float(ref['g'][2].max()))}
    for key, (v, b) in want.items():
        assert abs(rep[key] - v) <= b + 1e-12, (what, key, rep[key], v, b)
    for key, a, b in (('ratio_video', 'var_intra_video', 'var_inter_video'), ('ratio_class', 'var_intra_class', 'var_inter_class')):
        (va, ba), (vb, bb) = want[a], want[b]
        assert abs(rep[key] - va / vb) <= (ba + va / vb * bb) / (vb - bb) + 1e-12, (what, key)
    assert abs(rep['alignment'] - 2 * want['var_intra_video'][0]) <= 2 * want['var_intra_video'][1] + 1e-12
    s_all, g_all = torch.cat(ref['s']), torch.cat(ref['g'])
    x = (s_all - 1.0) * (2.0 * f32(t))
    w = torch.exp(x)
    rel = float((w * (E_EXPF + 2 * U * x.abs() + torch.expm1(2.0 * f32(t) * g_all))).sum() / w.sum()) + s_all.numel() * U64
    assert abs(rep['uniformity'] - math.log(float(w.mean()))) <= -math.log1p(-rel), (what, 'uniformity')
    print('    %s: undecidable %d of %d pairs; largest err / bound %s' % (what, und_total, pairs_total, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    return rep


@pytest.mark.parametrize('centre', [True, False])
def test_pair_statistics_against_float64(gpu, centre):
    """row_block = 48, chunk = 40 on n = 130: three row blocks (the last ragged, 34 rows), every diagonal square cut into two
    column chunks, blocks to its right of 40 columns and a ragged last one"""
    from dualvar_amd.utils import features as F
    from dualvar_amd.utils import variance as V
    feat, label, vid, cls = clip_case(gpu)
    x = feat.reshape(130, 64)
    t, bins = 2.0, 64
    z = F.normalise(x, centre)
    z64 = x.double() - x.double().mean(0) if centre else x.double()
    z64 = z64 / z64.norm(dim=1, keepdim=True)
    assert float((z.double() - z64).abs().max()) < 1e-5                     # the library's rows ARE the normalised features
    zh = z.double().cpu()
    ref = pairs_ref64(zh, zh, (vid, cls, vid, cls), 0, t, bins)
    assert ref['n'] == [13 * 10 * 9, sum(k * (k - 1) for k in (4, 3, 3, 3)) * 100, 130 * 129 - 1170 - sum(k * (k - 1) for k in (4, 3, 3, 3)) * 100]
    sym = V.pair_statistics(x, vid, cls, bins=bins, t=t, centre=centre, symmetric=True, row_block=48, chunk=40)
    check_against_float64(sym, ref, t, bins, 'pair_statistics symmetric centre=%s' % centre)
    full = V.pair_statistics(x, vid, cls, bins=bins, t=t, centre=centre, symmetric=False, row_block=48, chunk=40)
    check_against_float64(full, ref, t, bins, 'pair_statistics full walk centre=%s' % centre)
    assert torch.equal(sym[2], full[2]), 'symmetric and full walk differ in hist'
    assert torch.equal(sym[1].view(torch.int32), full[1].view(torch.int32)), 'symmetric and full walk differ in ext'
    one = V.pair_statistics(x, vid, cls, bins=bins, t=t, centre=centre)     # the defaults: one 130 x 130 block
    check_against_float64(one, ref, t, bins, 'pair_statistics one block centre=%s' % centre)
    assert torch.equal(one[2], full[2]) and torch.equal(one[1].view(torch.int32), full[1].view(torch.int32))


def test_pair_statistics_cross(gpu):
    from dualvar_amd.utils import features as F
    from dualvar_amd.utils import variance as V
    feat, label, vid, cls = clip_case(gpu)
    bank = feat.reshape(130, 64)
    gen = torch.Generator().manual_seed(11)
    q = (bank[torch.randint(0, 130, (30,), generator=gen).to(gpu)] + 0.5 * torch.randn((30, 64), generator=gen).to(gpu)).contiguous()
    q_vid = torch.tensor([0, 1, 2] * 10, dtype=torch.int32)                # three of the bank's videos: all categories occur
    q_cls = (q_vid % 4).int()
    t, bins = 2.0, 64
    zq, zb = F.normalise(q, True).double().cpu(), F.normalise(bank, True).double().cpu()
    ref = pairs_ref64(zq, zb, (q_vid, q_cls, vid, cls), NO_SELF, t, bins)
    assert sum(ref['n']) == 30 * 130 and ref['n'][0] == 30 * 10 and min(ref['n']) > 0
    for rb, ch in ((7, 33), (None, None)):
        state = V.pair_statistics_cross(q, q_vid, q_cls, bank, vid, cls, bins=bins, t=t, row_block=rb, chunk=ch)
        check_against_float64(state, ref, t, bins, 'pair_statistics_cross row_block=%s chunk=%s' % (rb, ch))


# ----------------------------------------------------------------------------------------------------- 4. variance_eval
def test_variance_eval_is_the_report_of_the_state(gpu):
    from dualvar_amd.utils import variance as V
    feat, label, vid, cls = clip_case(gpu)
    rep = V.variance_eval(feat, label, bins=32, t=1.5)
    state = V.pair_statistics(feat.reshape(130, 64), vid, cls, bins=32, t=1.5)
    assert rep == V.report_from_state(*state, 32, 1.5)
    assert [rep['categories'][n]['count'] for n in V.CATEGORIES] == [1170, 3000, 130 * 129 - 4170]
    json.dumps(rep)


def test_variance_eval_known_by_construction(gpu):
    """clips = a video centre + small noise: same-video clips lie closer than clips of different videos (ratio < 1); with the
    scales swapped (tiny centres, large noise) the video no longer matters and, the centring removing what is common, same-video
    pairs are no closer than the rest: the ratio is not below 1"""
    from dualvar_amd.utils import variance as V
    gen = torch.Generator().manual_seed(3)
    n_video, num_seq, D = 13, 10, 64
    centre, noise = torch.randn((n_video, 1, D), generator=gen), torch.randn((n_video, num_seq, D), generator=gen)
    label = torch.arange(n_video) % 4
    tight = V.variance_eval((centre + 0.05 * noise).to(gpu), label)
    assert tight['var_intra_video'] < tight['var_inter_video'] and tight['ratio_video'] < 1
    assert tight['var_intra_video'] < 0.01 and tight['alignment'] == 2 * tight['var_intra_video']
    # every clip its own direction, one shared offset per video scaled down to nothing, pushed apart within a video
    spread = V.variance_eval((0.05 * centre + noise - noise.mean(1, keepdim=True)).to(gpu), label)
    assert spread['var_intra_video'] > spread['var_inter_video'] and spread['ratio_video'] > 1
    print('    ratio_video: centre + small noise %.4f, small centre + noise %.4f' % (tight['ratio_video'], spread['ratio_video']))


# --------------------------------------------------------------------------------------------------- 5. the driver, two children
def test_cli_retrieval_with_variance(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp('variance_cli')
    split, frame = write_dataset(str(d / 'data'), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
    os.makedirs(str(d / 'run' / 'model'))
    base = [os.path.join(ROOT, 'classifier.py'), '--test', str(d / 'run' / 'model' / 'none.pth.tar'), '--retrieval', '--num_seq', '10',
            '--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
            '--split_root', split, '--frame_root', frame]
    out = _child(base + ['--variance', '--var_bins', '16', '--var_t', '1.5'], str(d), 600)
    fdir = str(d / 'run' / 'model' / 'feature')
    assert out.count('Variance report on ucf101') == 2 and 'intra-video = ' in out and 'uniformity = ' in out, out[-2000:]
    for split_name in ('test', 'train'):
        with open(os.path.join(fdir, 'ucf101_%s_variance.json' % split_name)) as fp:
            rep = json.load(fp)
        label = torch.load(os.path.join(fdir, 'ucf101_%s_label.pth.tar' % split_name), map_location='cpu', weights_only=True)
        per = torch.load(os.path.join(fdir, 'ucf101_%s_per_feature.pth.tar' % split_name), map_location='cpu', weights_only=True)
        n_video = label.numel()
        assert per.shape[:2] == (n_video, 10) and n_video == (3 if split_name == 'test' else 30)
        n = 10 * n_video
        same_class_videos = sum(int((label == c).sum()) * (int((label == c).sum()) - 1) for c in label.unique().tolist())
        want = [n_video * 10 * 9, same_class_videos * 100]
        want.append(n * (n - 1) - sum(want))
        cats = [rep['categories'][k] for k in ('same_video', 'same_class', 'diff_class')]
        assert [c['count'] + c['skipped'] for c in cats] == want, (split_name, want)
        assert all(sum(c['hist']) == c['count'] and len(c['hist']) == 16 for c in cats)
        assert rep['bins'] == 16 and rep['t'] == 1.5
        for key in ('var_intra_video', 'var_inter_video', 'var_intra_class', 'var_inter_class', 'alignment'):
            assert rep[key] is None or 0.0 <= rep[key] <= 2.0 + 1e-5, (key, rep[key])
    out2 = _child(base + ['--dirname', 'feature_plain'], str(d), 600)
    assert 'Variance report' not in out2
    plain = os.listdir(str(d / 'run' / 'model' / 'feature_plain'))
    assert plain and not [f for f in plain if 'variance' in f], plain
