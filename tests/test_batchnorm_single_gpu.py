"""The single-tensor BatchNorm entries (dv_bn_reduce_stats, dv_bn_stats_finalize, dv_bn_finalize, dv_bn_apply, dv_bn_bwd_reduce
in its ordered and atomic forms, dv_bn_bwd_apply) and the helpers around them (dv_bn_eval_coeffs, dv_addcmul_f32,
dv_bn_rows_partials_f32, dv_fill_cols_f32) against a plain float64 reference of the same operation.

engine.BNGroupOp.launches gives these entries to every lone member: the residual-closing and ReLU-free BatchNorms of the
ResNets, the stems and separable pairs of S3D-G, every eval-mode layer and the classifier head's BatchNorm1d.  The kernel bodies
are those of the multi-tensor entries (tests/test_batchnorm_multi_gpu.py; the Member / check_* helpers of tests/bn_support.py
and the sentinel discipline of tests/checks.py serve both files); what is pinned here is what the single-tensor wrappers decide
themselves, at the rows of tests/bn_cases.py: 1024-thread statistics from 2048 tiles, reduce grids whose trailing blocks own no rows, the atomic form and
its replicas, the second trip of the capped grid-stride loops, the LDS limit of dv_bn_bwd_apply, dv_bn_finalize inside a wider
gathered row.  Two kinds of data, as in the sibling file:

  (A) exactly representable: S, count, sum g, sum g*xhat (ordered; in the atomic form every replica, which must hold exactly
      the blocks bid % n_rep sends to it), y, dres, dbeta / dgamma equal float64 BIT FOR BIT, in fp32 and bf16.
  (B) Gaussian data against float64 with derived bounds (u = 2^-24, 2^-8 more for a bf16 store); the chains that differ from
      the multi-tensor launches:
        statistics      ceil(n_tiles / threads) + 6 + threads / 64, threads = 1024 from 2048 tiles
        atomic reduce   column_chain of one block + the ceil(blocks / n_rep) atomics that meet in a replica; the n_rep - 1
                        additions of dv_bn_bwd_apply's fold of the replicas enter its k2 / k3 / dgamma / dbeta bounds
        finalize        R sequential additions for count, S and M2
        rows_partials   M sequential additions per pass, two roundings per squared term
        eval_coeffs     the finalize's roundings, rsqrtf allowed the same 2 ulp
        addcmul         three roundings of |y| + |alpha a b|
      A chain of launches is checked stage by stage: every stage against float64 of the values the stage before it STORED
      (the statistics against float64 of x), so no bound has to carry another stage's error; the formulas composed are those
      tests/test_abi_and_host.py compares with torch's float64 autograd.

Every launch goes through the C ABI on explicit tensors: NaN outside input views and junk in the input pad lanes [C, CP);
sentinel bits outside output views, output pad lanes exactly 0; per-channel outputs past C untouched (dv_bn_eval_coeffs
writes zeros up to CP); the reduce workspace's row area holds NaN before a launch (a block that stores no row shows), its
ticket words are zero after every ordered launch, and two ordered launches give the same bits.

Measured on the MI355X (Gaussian data, the largest over the cases; -s prints every figure).  err / bound: statistics S 0.13,
M2 0.13 (from x through the stored partials: 0.14 / 0.15); dv_bn_finalize mean 0.58; atomic replicas sum g 0.18, sum g*xhat
0.19; dv_bn_rows_partials_f32 sums 0.43, M2 0.15; dv_bn_eval_coeffs scale 0.35, shift 0.38, shift + scale * bias 0.46, the eval
chain against the float64 layer 0.31 (fp32) / 0.99 (bf16: the store's half ulp); dv_addcmul_f32 0.45; the all-reduced SyncBN
sums 0.0006.  In units of u * sum|terms|, as the sibling file prints them: ordered sums 1.9 / 2.2 (chain 15 - 45), SyncBN 0.5 /
0.7, dx 3.6 of the 12 u allowed through the ordered sums and 14.4 behind four atomic replicas (M = 220 000: the 12 u plus the
three additions of the fold, which weigh on k3 where sum g cancels).  Every (A) quantity is bit-equal.  The file takes 13 s
(174 tests, the longest 0.3 s).

Four launch rules changed one at a time in a scratch build of what is now csrc/batchnorm.hip, and what noticed:
  an empty reduce block stores no row      test_backward_against_float64[m20481_c8_r2-*] and [m300033_c8-*] (NaN in the sums)
  bid % n_rep -> 0 in the atomic form      test_backward_against_float64[m33_c83_accum-*] and [m2048_c3-*] (a replica is not
                                           the sum of its blocks; the total alone would not tell)
  the grid-stride step of bn_apply_body    test_apply_against_float64[overcap_m220000_c40-*], the one row with a second trip
    doubled
  1024 -> 512 threads in both statistics   no GPU test: block_sum folds blockDim / 64 wave sums, so 512 threads give correct
    launches                               sums by another order, inside the same bounds; the quoted launch rule of
                                           tests/bn_cases.py no longer matches the source and
                                           tests/test_abi_and_host.py::test_bn_case_table_blocks_and_coverage fails"""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L  # noqa: E402
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_F32  # noqa: E402
from tests import bn_cases as T  # noqa: E402
from tests import bn_reference as REF  # noqa: E402
from tests import bn_support as MU  # noqa: E402
from tests.bn_support import DTYPES, EPS, MOM, Member  # noqa: E402
from tests.chains import bwd_reduce_chain, column_chain, m2_bound, stats_chain  # noqa: E402
from tests.checks import BF16_U, U, ceil_div, chan, cp8, equal_bits, is_sent, launch, sent, vec, within  # noqa: E402

KINDS = [pytest.param(True, id='exact'), pytest.param(False, id='gauss')]
NAN = float('nan')


def ids(cases):
    return [c.name for c in cases]


def ratio(what, err, bound):
    """err / bound, the largest over the values (printed with -s; the bound itself is the assertion)"""
    r = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'    {what:<44s} max err / bound = {r:7.4f}')
    return r


def twin(make):
    """two members with the same data: one for each of two launch forms whose outputs are compared bit for bit"""
    return make(), make()


# ----------------------------------------------------------------------------------------------------------- launches
def stats_finalize(m, local, out=None, rm=None, rv=None):
    o = m.o if out is None else out
    rm, rv = (m.rm, m.rv) if rm is None else (rm, rv)
    launch('dv_bn_stats_finalize', m.partials_ptr(), m.n_tiles, m.tile_rows, m.pitch, m.M, m.C, local.data_ptr(),
           m.p['gamma'].data_ptr(), m.p['beta'].data_ptr(), EPS, MOM, rm.data_ptr(), rv.data_ptr(),
           *(o[k].data_ptr() for k in ('mean', 'invstd', 'scale', 'shift')))


def finalize(stats_ptr, R, stride, m, out, rm, rv):
    launch('dv_bn_finalize', stats_ptr, R, stride, m.C, m.p['gamma'].data_ptr(), m.p['beta'].data_ptr(), EPS, MOM,
           rm.data_ptr() if rm is not None else 0, rv.data_ptr() if rv is not None else 0,
           *(out[k].data_ptr() for k in ('mean', 'invstd', 'scale', 'shift')))


def apply(m, scale=None, shift=None):
    sc = m.p['scale'] if scale is None else scale
    sh = m.p['shift'] if shift is None else shift
    launch('dv_bn_apply', m.dtype, m.x.ptr, m.x.ld, sc.data_ptr(), sh.data_ptr(), m.res.ptr if m.res else 0,
           m.res.ld if m.res else 0, m.y.ptr, m.y.ld, m.M, m.C, m.fwd_flags)


def bwd_reduce(m, sums, n_rep, ws):
    """(the reduce writes no dres: without DV_ACCUM, as the engine launches it; without a mask y is not passed at all)"""
    launch('dv_bn_bwd_reduce', m.dtype, m.dy.ptr, m.dy.ld, m.y.ptr if m.relu else 0, m.y.ld if m.relu else 0, m.x.ptr, m.x.ld,
           m.p['mean'].data_ptr(), m.p['invstd'].data_ptr(), m.M, m.C, m.bwd_flags & ~DV_ACCUM, sums.data_ptr(), n_rep,
           ws.data_ptr() if ws is not None else 0)


def bwd_apply(m, sums, n_rep, inv_count, dparams=True):
    launch('dv_bn_bwd_apply', m.dtype, m.dy.ptr, m.dy.ld, m.y.ptr if m.relu else 0, m.y.ld if m.relu else 0, m.x.ptr, m.x.ld,
           m.p['mean'].data_ptr(), m.p['invstd'].data_ptr(), m.p['gamma'].data_ptr(), sums.data_ptr(), n_rep, inv_count, m.dscale,
           m.dgamma.data_ptr() if dparams else 0, m.dbeta.data_ptr() if dparams else 0, m.dx.ptr, m.dx.ld,
           m.dres.ptr if m.dres else 0, m.dres.ld if m.dres else 0, m.M, m.C, m.bwd_flags)


def adopt(m, out):
    """the stored statistics `out` (mean / invstd / scale / shift as a launch wrote them, sentinel NaN past C) become the
    member's parameters: what the later stages read, and -- as float64 -- what their references are formed from"""
    C_ = m.C
    for k in ('mean', 'invstd', 'scale', 'shift'):
        m.p[k] = out[k]
    m.mean, m.invstd, m.scale, m.shift = (out[k][:C_].double() for k in ('mean', 'invstd', 'scale', 'shift'))


def poison_rows(m):
    """NaN in the row and group-row area of the ordered reduce's workspace (ticket words stay zero): a block that does not
    store its row leaves NaN in the sums"""
    nblk = MU.n_blocks(L.load(), 'red', m.M, m.C, m.dtype)
    m.red_ws[:(nblk + ceil_div(nblk, 32)) * 2 * m.CP] = NAN


def forward_for_backward(m, what):
    """y as dv_bn_apply stores it (checked), junk in its pad lanes afterwards; (g, xhat) of the backward"""
    apply(m)
    torch.cuda.synchronize()
    MU.check_apply(m, what)
    y_in = m.y.val()
    m.y.buf[:, m.y.off + m.C:m.y.off + m.CP] = MU.JUNK
    g, xhat = MU.backward_terms(m, y_in)
    MU.assert_exact_data_fits(m, g, xhat)
    return g, xhat


def ordered_reduce_twice(m, g, xhat, what):
    for k in range(2):
        poison_rows(m)
        bwd_reduce(m, m.sums[k], 1, m.red_ws)
        torch.cuda.synchronize()
        MU.check_ticket_area(m, f'{what} launch {k}')
    assert equal_bits(m.sums[0], m.sums[1]), f'{what}: two ordered reduces: the two forms differ'
    MU.check_reduce(m, m.sums[0], g, xhat, 0, what)


# ----------------------------------------------------------------------------------------------------------- statistics
def stats_member(dev, c, exact, seed=5):
    m = Member(dev, DV_F32, T.stats_rows(c), c.C, seed, exact=exact, relu=False, tile_rows=c.tile_rows,
               part_pitch_extra=c.pitch_extra)
    assert m.n_tiles == c.n_tiles and float(m.tile_n[-1]) == c.last_rows
    return m


def fresh_outputs(m, dev):
    return ({k: sent((m.CP,), dev) for k in ('mean', 'invstd', 'scale', 'shift')}, chan(m.rm0, m.CP, dev),
            chan(m.rv0, m.CP, dev))


@pytest.mark.parametrize('exact', KINDS)
@pytest.mark.parametrize('case', T.STATS_CASES, ids=ids(T.STATS_CASES))
def test_stats_finalize_against_float64(gpu, case, exact):
    """dv_bn_stats_finalize against float64 of the stored partials (S bit for bit with exact data), with the chain of the block
    size the row names; dv_bn_reduce_stats + dv_bn_finalize(R = 1) gives the same bits on both sides of 2048 tiles; below it a
    one-member dv_bn_stats_multi does too"""
    c, w = case, f'stats {case.name}'
    assert T.stats_threads(c.n_tiles) == c.threads
    m = stats_member(gpu, c, exact)
    print(f'\n  {w}: M={m.M} C={m.C} tiles={m.n_tiles} threads={c.threads}')
    local = sent((2 * m.C + 1 + 8,), gpu)
    stats_finalize(m, local)
    torch.cuda.synchronize()
    S, M2, dS, dM2, sabs = MU.stats_reference(m, c.threads)
    MU.check_local(m, local, S, M2, dS, dM2, sabs, w)
    row = local[:2 * m.C].double()
    if not exact:
        ratio(f'{w} S', (row[:m.C] - S).abs(), dS)
    ratio(f'{w} M2', (row[m.C:] - M2).abs(), dM2)
    assert is_sent(local[2 * m.C + 1:]), f'{w}: wrote behind the local row'
    assert all(is_sent(t[m.C:]) for t in m.o.values()), f'{w}: outputs past C'
    assert bool((m.rm[m.C:] == 0.625).all()) and bool((m.rv[m.C:] == 0.625).all()), f'{w}: running statistics past C'
    MU.check_finalized(m, m.o, S, M2, m.M, dS, dM2, m.rm, m.rv, w)
    # the exchange form: reduce_stats, then finalize over the one row
    local2 = sent((2 * m.C + 1 + 8,), gpu)
    o2, rm2, rv2 = fresh_outputs(m, gpu)
    launch('dv_bn_reduce_stats', m.partials_ptr(), m.n_tiles, m.tile_rows, m.pitch, m.M, m.C, local2.data_ptr())
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in o2.values()), f'{w}: reduce_stats wrote the affine map'
    finalize(local2.data_ptr(), 1, 2 * m.C + 1, m, o2, rm2, rv2)
    torch.cuda.synchronize()
    for a, b, n in [(local, local2, 'local row'), (m.rm, rm2, 'running_mean'), (m.rv, rv2, 'running_var')] + \
                   [(m.o[k], o2[k], k) for k in m.o]:
        assert equal_bits(a, b), f'{w} stats_finalize vs reduce_stats + finalize: {n}: the two forms differ'
    if c.threads == 256:                            # the multi-tensor launch always runs 256 threads: the same grid
        m3 = stats_member(gpu, c, exact)
        loc3, _ = MU.group_local([m3], gpu)
        tab, ends = MU.make_table([m3], L.load(), gpu, DV_F32, stats_outputs=True)
        launch('dv_bn_stats_multi', tab.data_ptr(), 1, 1, ends['stats'])
        torch.cuda.synchronize()
        for a, b, n in [(local[:2 * m.C + 1], loc3, 'local row'), (m.rm, m3.rm, 'running_mean'), (m.rv, m3.rv, 'running_var')] + \
                       [(m.o[k], m3.o[k], k) for k in m.o]:
            assert equal_bits(a, b), f'{w} single vs multi: {n}: the two forms differ'


# ----------------------------------------------------------------------------------------------------------- finalize
def finalize_bounds(S_r, Q_r, n_r, dS_r=None, dQ_r=None):
    """float64 (count, S, M2) of the ranks' stored rows and the bounds of dv_bn_finalize's fp32 evaluation of them: R
    sequential additions for count (exact: integers), S and M2; a rank's mean S_r / n_r one rounding"""
    R = S_r.shape[0]
    dS_r = torch.zeros_like(S_r) if dS_r is None else dS_r
    dQ_r = torch.zeros_like(Q_r) if dQ_r is None else dQ_r
    cnt, S, mean, M2 = REF.combine(S_r, Q_r, n_r)
    n = n_r.double()[:, None]
    dS = dS_r.sum(0) + R * U * (S_r.abs() + dS_r).sum(0)
    a = S_r / n
    dM2 = m2_bound(n, dS_r / n + U * a.abs(), a - mean, Q_r, dQ_r, dS / cnt + U * mean.abs(), R)
    return cnt, S, M2, dS, dM2


@pytest.mark.parametrize('case', T.FINALIZE_CASES, ids=ids(T.FINALIZE_CASES))
def test_finalize_against_float64(gpu, case):
    """dv_bn_finalize over R rows of unequal counts, the member's row at `base` inside a [R][stride] table that holds NaN
    everywhere else"""
    c, w = case, f'finalize {case.name}'
    C_, R = c.C, len(c.counts)
    assert c.blocks == ceil_div(C_, 128)
    stride = 2 * C_ + 1 + c.stride_extra
    gen = torch.Generator(device=gpu).manual_seed(31 + C_)
    n_r = torch.tensor(c.counts, dtype=torch.float64, device=gpu)
    mu = 0.5 * torch.randn(C_, generator=gen, device=gpu, dtype=torch.float64)
    S_r = (n_r[:, None] * (mu + 0.3 * torch.randn((R, C_), generator=gen, device=gpu, dtype=torch.float64))).float()
    Q_r = ((n_r[:, None] - 1) * (0.25 + torch.rand((R, C_), generator=gen, device=gpu, dtype=torch.float64))).float()
    Q_r[:, 0] = 0                                                 # a constant channel
    table = torch.full((R * stride + 8,), NAN, dtype=torch.float32, device=gpu)
    rows = table[:R * stride].view(R, stride)
    rows[:, c.base:c.base + C_] = S_r
    rows[:, c.base + C_:c.base + 2 * C_] = Q_r
    rows[:, c.base + 2 * C_] = n_r.float()
    m = SimpleNamespace(C=C_, p={'gamma': (1 + 0.2 * torch.randn(C_, generator=gen, device=gpu)),
                                 'beta': 0.1 * torch.randn(C_, generator=gen, device=gpu)},
                        rm0=torch.randint(-8, 9, (C_,), generator=gen, device=gpu).float() / 8,
                        rv0=0.5 + torch.randint(0, 9, (C_,), generator=gen, device=gpu).float() / 8)
    out = {k: sent((C_ + 8,), gpu) for k in ('mean', 'invstd', 'scale', 'shift')}
    rm, rv = (chan(m.rm0, C_ + 8, gpu), chan(m.rv0, C_ + 8, gpu)) if c.running else (None, None)
    finalize(table.data_ptr() + 4 * c.base, R, stride, m, out, rm, rv)
    torch.cuda.synchronize()
    cnt, S, M2, dS, dM2 = finalize_bounds(S_r.double(), Q_r.double(), n_r)
    assert cnt == sum(c.counts)
    print(f'\n  {w}: R={R} C={C_} stride={stride} base={c.base}')
    MU.check_finalized(m, out, S, M2, cnt, dS, dM2, rm, rv, w)
    ratio(f'{w} mean', (out['mean'][:C_].double() - S / cnt).abs(), dS / cnt + U * (S / cnt).abs())
    assert all(is_sent(t[C_:]) for t in out.values()), f'{w}: outputs past C'
    if c.running:
        assert bool((rm[C_:] == 0.625).all()) and bool((rv[C_:] == 0.625).all()), f'{w}: running statistics past C'


# per-rank row counts of the three rank tables below: unequal, one of them a single row (its M2 is 0)
FORM_COUNTS = {1: (37,), 2: (120, 1), 3: (64, 1, 300)}


@pytest.mark.parametrize('running', [True, False], ids=['running', 'norunning'])
@pytest.mark.parametrize('C_', [3, 83, 130])
def test_finalize_forms_agree_bit_for_bit(gpu, C_, running):
    """the finalize is one expression: on one seeded [R][stride] table dv_bn_finalize and dv_bn_finalize_multi (the table as a
    one-item group) leave the same bytes in mean / invstd / scale / shift / running_mean / running_var, for R = 1, 2, 3;
    and dv_bn_stats_finalize leaves the bytes of dv_bn_reduce_stats + dv_bn_finalize(R = 1) on the same partials (several
    tiles with a one-row tail, and the single row whose count is 1).  C = 130 crosses the 128-channel block."""
    gen = torch.Generator(device=gpu).manual_seed(1000 + C_)
    CP, keys = cp8(C_), ('mean', 'invstd', 'scale', 'shift')
    m = SimpleNamespace(C=C_, p={'gamma': chan(1 + 0.2 * torch.randn(C_, generator=gen, device=gpu), CP, gpu),
                                 'beta': chan(0.1 * torch.randn(C_, generator=gen, device=gpu), CP, gpu)})
    rm0 = torch.randint(-8, 9, (C_,), generator=gen, device=gpu).float() / 8
    rv0 = 0.5 + torch.randint(0, 9, (C_,), generator=gen, device=gpu).float() / 8

    def outputs():
        return {k: sent((CP,), gpu) for k in keys}, (chan(rm0, CP, gpu) if running else None), (chan(rv0, CP, gpu) if running else None)

    def same(a, b, what):
        (oa, rma, rva), (ob, rmb, rvb) = a, b
        assert not is_sent(oa['mean'][:C_]) and all(is_sent(t[C_:]) for t in list(oa.values()) + list(ob.values())), what
        for k in keys:
            assert equal_bits(oa[k], ob[k]), f'{what}: {k}: the two forms differ'
        if running:
            assert not torch.equal(rma[:C_], rm0) and equal_bits(rma, rmb) and equal_bits(rva, rvb), f'{what}: running statistics'

    for R, counts in FORM_COUNTS.items():
        stride = 2 * C_ + 1 + 5
        n_r = torch.tensor(counts, dtype=torch.float64, device=gpu)
        table = torch.full((R, stride), NAN, dtype=torch.float32, device=gpu)
        table[:, :C_] = (n_r[:, None] * (0.5 + 0.3 * torch.randn((R, C_), generator=gen, device=gpu, dtype=torch.float64))).float()
        table[:, C_:2 * C_] = ((n_r[:, None] - 1) * (0.25 + torch.rand((R, C_), generator=gen, device=gpu, dtype=torch.float64))).float()
        table[:, 2 * C_] = n_r.float()
        single, multi = outputs(), outputs()
        finalize(table.data_ptr(), R, stride, m, *single)
        arr = (L.BnItem * 1)()
        it = arr[0]
        it.C, it.local_stats, it.eps, it.momentum = C_, table.data_ptr(), EPS, MOM
        it.gamma, it.beta = m.p['gamma'].data_ptr(), m.p['beta'].data_ptr()
        it.running_mean, it.running_var = (multi[1].data_ptr(), multi[2].data_ptr()) if running else (0, 0)
        it.mean, it.invstd, it.scale, it.shift = (multi[0][k].data_ptr() for k in keys)
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(gpu)
        launch('dv_bn_finalize_multi', tab.data_ptr(), 1, ceil_div(C_, 128), table.data_ptr(), table.data_ptr(), R, stride)
        torch.cuda.synchronize()
        same(single, multi, f'finalize vs finalize_multi, C={C_} R={R}')

    for n_tiles, tile_rows, M in [(5, 8, 33), (1, 4, 1)]:
        rows = torch.full((n_tiles,), float(tile_rows), dtype=torch.float64, device=gpu)
        rows[-1] = M - (n_tiles - 1) * tile_rows
        part = torch.empty((2, C_, n_tiles), dtype=torch.float32, device=gpu)
        part[0] = (rows * (0.5 + 0.3 * torch.randn((C_, n_tiles), generator=gen, device=gpu, dtype=torch.float64))).float()
        part[1] = ((rows - 1) * (0.25 + torch.rand((C_, n_tiles), generator=gen, device=gpu, dtype=torch.float64))).float()
        fused, split = outputs(), outputs()
        loc_f, loc_s = sent((2 * C_ + 1,), gpu), sent((2 * C_ + 1,), gpu)
        launch('dv_bn_stats_finalize', part.data_ptr(), n_tiles, tile_rows, C_, M, C_, loc_f.data_ptr(), m.p['gamma'].data_ptr(),
               m.p['beta'].data_ptr(), EPS, MOM, *(t.data_ptr() if t is not None else 0 for t in fused[1:]),
               *(fused[0][k].data_ptr() for k in keys))
        launch('dv_bn_reduce_stats', part.data_ptr(), n_tiles, tile_rows, C_, M, C_, loc_s.data_ptr())
        finalize(loc_s.data_ptr(), 1, 2 * C_ + 1, m, *split)
        torch.cuda.synchronize()
        assert equal_bits(loc_f, loc_s) and float(loc_f[2 * C_]) == M, f'local row, C={C_} M={M}'
        same(fused, split, f'stats_finalize vs reduce_stats + finalize, C={C_} M={M}')


# ----------------------------------------------------------------------------------------------------------- apply
def apply_member(dev, dtype, c, exact, seed=3):
    return Member(dev, dtype, c.M, c.C, seed, exact=exact, relu=c.relu, res=c.res, views=c.views)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('exact', KINDS)
@pytest.mark.parametrize('case', T.APPLY_CASES, ids=ids(T.APPLY_CASES))
def test_apply_against_float64(gpu, dtype, case, exact):
    """dv_bn_apply (y bit for bit with exact data; the over-cap row takes a second grid-stride trip in both dtypes), and a
    one-member dv_bn_apply_multi gives the same bits"""
    c, w = case, f'apply {case.name}'
    v = vec(dtype)
    assert T.stride_trip(c.M, c.C, v, T.APPLY_CAP) == (c.trip[v == 8], c.wraps[v == 8])
    m, m2 = twin(lambda: apply_member(gpu, dtype, c, exact))
    apply(m)
    torch.cuda.synchronize()
    MU.check_apply(m, w)
    tab, ends = MU.make_table([m2], L.load(), gpu, dtype)
    assert ends['apply'] * 256 == c.trip[v == 8]
    launch('dv_bn_apply_multi', dtype, tab.data_ptr(), 1, ends['apply'])
    torch.cuda.synchronize()
    assert equal_bits(m.y.buf, m2.y.buf), f'{w} single vs multi: y: the two forms differ'


# ----------------------------------------------------------------------------------------------------------- backward
def bwd_member(dev, dtype, c, exact, seed=9):
    return Member(dev, dtype, c.M, c.C, seed, exact=exact, relu=c.relu, res=c.res is not None, accum=c.res == 'accum',
                  views=c.views, dscale=1.0 / c.R, R=c.R)


def atomic_chain(c, dtype):
    """longest chain of fp32 additions behind one value of a replica: column_chain over the rows of one block, then the float
    atomics of the ceil(blocks / n_rep) blocks that bid % n_rep sends there"""
    blocks, rpb = c.red[0], c.red[1]
    return column_chain(rpb, cp8(c.C), dtype, 2, ceil_div(blocks, c.n_rep))


def check_atomic(m, c, rep, g, xhat, what):
    """every replica against float64 of the rows of the blocks it owns; columns [C, CP) and the replica behind the last untouched"""
    C_, CP, n_rep = m.C, m.CP, c.n_rep
    blocks, rpb = c.red[0], c.red[1]
    owner = (torch.arange(m.M, device=g.device) // rpb) % n_rep
    assert int(owner.max()) < n_rep and ceil_div(m.M, rpb) <= blocks
    zero = torch.zeros((n_rep, C_), dtype=torch.float64, device=g.device)
    gx = g * xhat
    sg, sgx = zero.clone().index_add_(0, owner, g), zero.clone().index_add_(0, owner, gx)
    ag, agx = zero.clone().index_add_(0, owner, g.abs()), zero.clone().index_add_(0, owner, gx.abs())
    r = rep.view(n_rep + 1, 2, CP)
    assert is_sent(r[n_rep]) and is_sent(r[:n_rep, :, C_:]), f'{what}: wrote outside its replicas'
    got_g, got_gx = r[:n_rep, 0, :C_].double(), r[:n_rep, 1, :C_].double()
    chain = atomic_chain(c, m.dtype)
    if m.exact:
        assert torch.equal(got_g, sg) and torch.equal(got_gx, sgx), f'{what}: a replica is not the exact sum of its blocks'
        assert torch.equal(got_g.sum(0), g.sum(0)) and torch.equal(got_gx.sum(0), gx.sum(0)), f'{what}: replicas do not add up'
    within(got_g, sg, chain * U * ag, f'{what} replica sum g', quiet=True)
    within(got_gx, sgx, (chain + 3) * U * agx, f'{what} replica sum g*xhat', quiet=True)
    if not m.exact:
        ratio(f'{what} sum g (L={chain})', (got_g - sg).abs(), chain * U * ag)
        ratio(f'{what} sum g*xhat', (got_gx - sgx).abs(), (chain + 3) * U * agx)
    # what dv_bn_bwd_apply is given: the replicas; its reference: their float64 total, and what its fp32 fold may lose
    total = torch.full((2 * CP,), NAN, dtype=torch.float64, device=g.device)
    total[:C_], total[CP:CP + C_] = got_g.sum(0), got_gx.sum(0)
    dsums = ((n_rep - 1) * U * got_g.abs().sum(0), (n_rep - 1) * U * got_gx.abs().sum(0))
    return total, dsums


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('exact', KINDS)
@pytest.mark.parametrize('case', T.BWD_CASES, ids=ids(T.BWD_CASES))
def test_backward_against_float64(gpu, dtype, case, exact):
    """dv_bn_bwd_reduce, ordered (twice: same bits, tickets zero, NaN-poisoned rows) and atomic with the row's n_rep, then
    dv_bn_bwd_apply over the replicas (n_rep > 1) or the ordered sums"""
    c, w = case, f'bwd {case.name}'
    lib = L.load()
    blocks, rpb, ne, last, grp = c.red
    assert (blocks, rpb) == (int(lib.dv_bn_bwd_blocks(c.M, c.C)), ceil_div(c.M, blocks))
    m = bwd_member(gpu, dtype, c, exact)
    print(f'\n  {w}: M={m.M} C={m.C} blocks={blocks} ({ne} non-empty, the last {last} rows) n_rep={c.n_rep}')
    g, xhat = forward_for_backward(m, w)
    ordered_reduce_twice(m, g, xhat, f'{w} ordered')
    rep = torch.zeros((c.n_rep + 1) * 2 * m.CP, dtype=torch.float32, device=gpu)
    r = rep.view(c.n_rep + 1, 2, m.CP)
    r[c.n_rep] = sent((2 * m.CP,), gpu).view(2, m.CP)
    r[:c.n_rep, :, m.C:] = sent((c.n_rep * 2 * (m.CP - m.C),), gpu).view(c.n_rep, 2, m.CP - m.C)
    bwd_reduce(m, rep, c.n_rep, None)
    torch.cuda.synchronize()
    total, dsums = check_atomic(m, c, rep, g, xhat, f'{w} atomic')
    v = vec(dtype)
    assert T.stride_trip(c.M, c.C, v, T.BAPPLY_CAP) == (c.bapply[0][v == 8], c.bapply[1][v == 8])
    inv_count = 1.0 / (c.R * c.M)
    if c.n_rep > 1:
        bwd_apply(m, rep, c.n_rep, inv_count, c.dparams)
        sums_in = total
    else:
        bwd_apply(m, m.sums[0], 1, inv_count, c.dparams)
        sums_in, dsums = m.sums[0], None
    torch.cuda.synchronize()
    MU.check_bwd_apply(m, g, sums_in, inv_count, w, dsums=dsums, dparams=c.dparams)


SAME_GRID = [c for c in T.BWD_CASES if cp8(c.C) <= 3072]        # (dv_bn_bwd_apply_multi keeps 5 CP floats of LDS: C <= 3072)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', SAME_GRID, ids=ids(SAME_GRID))
def test_backward_single_equals_multi(gpu, dtype, case):
    """the engine's block rules give a one-member multi-tensor launch the grid of the single-tensor entry: apply, the ordered
    reduce and bwd_apply give the same bits (Gaussian data)"""
    c, w = case, f'single == multi {case.name}'
    a, b = twin(lambda: bwd_member(gpu, dtype, c, False))
    inv_count = 1.0 / (c.R * c.M)
    apply(a)
    bwd_reduce(a, a.sums[0], 1, a.red_ws)
    bwd_apply(a, a.sums[0], 1, inv_count)
    tab, ends = MU.make_table([b], L.load(), gpu, dtype)
    assert ends['red'] == c.red[0]
    launch('dv_bn_apply_multi', dtype, tab.data_ptr(), 1, ends['apply'])
    launch('dv_bn_bwd_reduce_multi', dtype, tab.data_ptr(), 1, ends['red'])
    launch('dv_bn_bwd_apply_multi', dtype, tab.data_ptr(), 1, ends['bapply'], c.C)
    torch.cuda.synchronize()
    pairs = [(a.y.buf, b.y.buf, 'y'), (a.sums[0], b.sums[0], 'ordered sums'), (a.dx.buf, b.dx.buf, 'dx'),
             (a.dgamma, b.dgamma, 'dgamma'), (a.dbeta, b.dbeta, 'dbeta')]
    if a.dres:
        pairs.append((a.dres.buf, b.dres.buf, 'dres'))
    for x, y, n in pairs:
        assert equal_bits(x, y), f'{w}: {n}: the two forms differ'
    assert not bool(torch.isnan(a.dx.val()).any())


# ----------------------------------------------------------------------------------------------------------- chains
TRAIN = [pytest.param(1000, 83, 256, id='m1000_c83_t4'), pytest.param(2049 * 64 - 63, 8, 64, id='m131073_c8_t2049')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M,C_,tile_rows', TRAIN)
def test_train_chain_against_float64(gpu, dtype, M, C_, tile_rows):
    """a lone training-mode BatchNorm3d + residual + ReLU as the engine launches it: dv_bn_stats_finalize -> dv_bn_apply ->
    ordered dv_bn_bwd_reduce (mask from the y the forward stored) -> dv_bn_bwd_apply, on both sides of 2048 tiles.  The
    statistics against float64 of x; each later stage against float64 of the stored statistics."""
    w = f'train M={M} C={C_}'
    m = Member(gpu, dtype, M, C_, 23, exact=False, relu=True, res=True, accum=True, views=True, tile_rows=tile_rows)
    threads = T.stats_threads(m.n_tiles)
    print(f'\n  {w}: tiles={m.n_tiles} threads={threads}')
    local = sent((2 * C_ + 1,), gpu)
    stats_finalize(m, local)
    torch.cuda.synchronize()
    # float64 of x itself: the partials the member stores are float64 tile sums rounded once
    x = m.x.val()
    S = x.sum(0)
    mean = S / M
    M2 = ((x - mean) ** 2).sum(0)
    ps, pq, n = m.ps(), m.pq(), m.tile_n[:, None]
    chain = stats_chain(m.n_tiles, threads)
    dps = U * ps.abs()
    dS = dps.sum(0) + chain * U * ps.abs().sum(0)
    a = ps / n
    dM2 = m2_bound(n, dps / n + U * a.abs(), a - mean, pq, U * pq, dS / M + U * mean.abs(), chain)
    row = local.double()
    assert float(row[2 * C_]) == M
    within(row[:C_], S, dS, f'{w} S')
    within(row[C_:2 * C_], M2, dM2, f'{w} M2')
    MU.check_finalized(m, m.o, S, M2, M, dS, dM2, m.rm, m.rv, w)
    adopt(m, m.o)
    g, xhat = forward_for_backward(m, w)
    ordered_reduce_twice(m, g, xhat, w)
    bwd_apply(m, m.sums[0], 1, 1.0 / M)
    torch.cuda.synchronize()
    MU.check_bwd_apply(m, g, m.sums[0], 1.0 / M, w)


@pytest.mark.parametrize('dtype', DTYPES)
def test_reduce_stats_then_finalize_is_syncbn(gpu, dtype):
    """three ranks with different row counts run dv_bn_reduce_stats into their row of a wider gathered table; dv_bn_finalize
    (stride = the table's width, the pointer at the member's offset) matches float64 statistics of the pooled rows.  The
    backward runs with the all-reduced ordered sums, inv_count = 1 / sum M and dparam_scale = 1 / 3."""
    R, C_, base, width = 3, 83, 24, 24 + 2 * 83 + 1 + 40
    Ms = (1000, 2049 * 64, 333)
    ranks = [Member(gpu, dtype, M, C_, 41 + 7 * r, exact=False, relu=True, res=r == 1, R=R, dscale=1.0 / R,
                    tile_rows=64 if r == 1 else 256, part_pitch_extra=16 * (r == 2)) for r, M in enumerate(Ms)]
    gathered = torch.full((R, width), NAN, dtype=torch.float32, device=gpu)
    for r, m in enumerate(ranks):
        launch('dv_bn_reduce_stats', m.partials_ptr(), m.n_tiles, m.tile_rows, m.pitch, m.M, C_,
               gathered[r].data_ptr() + 4 * base)
    torch.cuda.synchronize()
    per = [MU.stats_reference(m, T.stats_threads(m.n_tiles)) for m in ranks]
    for r, (m, (S, M2, dS, dM2, sabs)) in enumerate(zip(ranks, per)):
        m.loff = base
        MU.check_local(m, gathered[r], S, M2, dS, dM2, sabs, f'syncbn rank {r}')
        assert bool(torch.isnan(gathered[r, :base]).all()) and bool(torch.isnan(gathered[r, base + 2 * C_ + 1:]).all())
    me = ranks[0]
    finalize(gathered.data_ptr() + 4 * base, R, width, me, me.o, me.rm, me.rv)
    torch.cuda.synchronize()
    # float64 over the pooled rows (of the partials every rank stored); the finalize works on the ranks' fp32 rows
    ps = torch.cat([m.ps() for m in ranks])
    pq = torch.cat([m.pq() for m in ranks])
    nn = torch.cat([m.tile_n for m in ranks])[:, None]
    cnt = sum(Ms)
    S = ps.sum(0)
    M2 = (pq + nn * (ps / nn - S / cnt) ** 2).sum(0)
    n_r = torch.tensor(Ms, dtype=torch.float64, device=gpu)
    cnt2, _, _, dS, dM2 = finalize_bounds(torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), n_r,
                                             torch.stack([p[2] for p in per]), torch.stack([p[3] for p in per]))
    assert cnt2 == cnt
    MU.check_finalized(me, me.o, S, M2, cnt, dS, dM2, me.rm, me.rv, 'syncbn fwd')
    # backward: every rank reads the global statistics and rank 0's parameters
    for m in ranks:
        adopt(m, me.o)
        for k in ('gamma', 'beta'):
            m.p[k] = me.p[k]
        m.gamma, m.beta = me.gamma, me.beta
    gx = [forward_for_backward(m, f'syncbn rank {r}') for r, m in enumerate(ranks)]
    for r, m in enumerate(ranks):
        ordered_reduce_twice(m, *gx[r], f'syncbn bwd rank {r}')
    total = ranks[0].sums[0] + ranks[1].sums[0] + ranks[2].sums[0]                 # the all-reduce, fp32
    g_all = torch.cat([g for g, _ in gx])
    gx_all = torch.cat([g * xh for g, xh in gx])
    chain = max(bwd_reduce_chain(m.M, C_, dtype, MU.n_blocks(L.load(), 'red', m.M, C_, dtype)) for m in ranks) + R
    t = total.double()
    CP = cp8(C_)
    within(t[:C_], g_all.sum(0), chain * U * g_all.abs().sum(0), 'syncbn sum g')
    within(t[CP:CP + C_], gx_all.sum(0), (chain + 3) * U * gx_all.abs().sum(0), 'syncbn sum g*xhat')
    for r, m in enumerate(ranks):
        bwd_apply(m, total, 1, 1.0 / cnt)
    torch.cuda.synchronize()
    for r, m in enumerate(ranks):
        MU.check_bwd_apply(m, gx[r][0], total, 1.0 / cnt, f'syncbn bwd rank {r}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C_', [1, 3, 127, 128, 129, 250, 257])
def test_eval_chain_against_float64(gpu, dtype, C_):
    """an eval-mode layer behind a biased conv: dv_bn_eval_coeffs (zeros in [C, CP), nothing past CP; blocks of 128 channels),
    dv_addcmul_f32 (shift += scale * b) and dv_bn_apply, against float64 (x + b - rm) / sqrt(rv + eps) * gamma + beta; every
    fourth channel has running_var = 0"""
    w, M, CP = f'eval C={C_}', 37, cp8(C_)
    m = Member(gpu, dtype, M, C_, 61 + C_, exact=False, relu=False, views=True)
    gen = torch.Generator(device=gpu).manual_seed(C_)
    b = 0.3 * torch.randn(C_, generator=gen, device=gpu)
    rm, rv = m.rm0.clone(), m.rv0.clone()
    rv[::4] = 0
    gamma, beta = m.p['gamma'][:C_].clone(), m.p['beta'][:C_].clone()                # (exactly C floats: nothing behind is read)
    scale, shift = sent((CP + 8,), gpu), sent((CP + 8,), gpu)
    launch('dv_bn_eval_coeffs', gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, C_, scale.data_ptr(),
           shift.data_ptr())
    torch.cuda.synchronize()
    for t in (scale, shift):
        assert bool((t[C_:CP] == 0).all()) and is_sent(t[CP:]), f'{w}: pad lanes / behind CP'
    g64, b64, rm64, rv64, bias64 = (t.double() for t in (gamma, beta, rm, rv, b))
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    inv = (rv64 + eps).rsqrt()
    rel_inv = 0.5 * (U * (rv64 + eps) + U * eps) / (rv64 + eps) + 4 * U           # (+ eps rounded; rsqrtf: 2 ulp allowed)
    sc = g64 * inv
    dsc = sc.abs() * (rel_inv + U) * (1 + 2 * U)
    sh = b64 - rm64 * sc
    dsh = (rm64.abs() * dsc + U * (rm64 * sc).abs() + U * sh.abs()) * (1 + 2 * U)
    print(f'\n  {w}')
    within(scale[:C_].double(), sc, dsc, f'{w} scale')
    within(shift[:C_].double(), sh, dsh, f'{w} shift')
    sc_k, sh_k = scale[:C_].double(), shift[:C_].double()                           # as stored
    launch('dv_addcmul_f32', shift.data_ptr(), scale.data_ptr(), b.data_ptr(), 1.0, C_)
    torch.cuda.synchronize()
    assert bool((shift[C_:CP] == 0).all()) and is_sent(shift[CP:]), f'{w}: addcmul wrote past n'
    shp = sh_k + sc_k * bias64
    dadd = 3 * U * (sh_k.abs() + (sc_k * bias64).abs())
    within(shift[:C_].double(), shp, dadd, f'{w} shift + scale * bias')
    # apply, against float64 of the stored coefficients ...
    m.scale, m.shift = sc_k, shift[:C_].double()
    apply(m, scale, shift)
    torch.cuda.synchronize()
    MU.check_apply(m, w)
    # ... and the chain against the float64 eval-mode layer: x (sc + dsc) + (sh + dsh) + bias (sc + dsc), the addcmul's and
    # the apply's three roundings each
    x = m.x.val()
    ref = REF.eval_reference(x, bias64, rm64, rv64, g64, b64, eps)
    dshp = dsh + bias64.abs() * dsc + 3 * U * (sh.abs() + dsh + (bias64 * sc).abs() + bias64.abs() * dsc)
    bound = x.abs() * dsc + dshp + 3 * U * (x.abs() * (sc.abs() + dsc) + (sh + bias64 * sc).abs() + dshp)
    if dtype == DV_BF16:
        bound = bound * (1 + BF16_U) + BF16_U * ref.abs()
    within(m.y.val(), ref, bound, f'{w} y against the float64 layer')


@pytest.mark.parametrize('n', [1, 255, 256, 257, 2048])
def test_addcmul_bias_fixup(gpu, n):
    """the train-mode fix-up of a biased conv, running_mean += momentum * b (b == NULL form), blocks of 256; the floats behind n
    stay; exact with dyadic data and alpha = 1/2"""
    gen = torch.Generator(device=gpu).manual_seed(n)
    for exact in (True, False):
        if exact:
            y0 = torch.randint(-64, 65, (n,), generator=gen, device=gpu).float() / 16
            a = torch.randint(-64, 65, (n,), generator=gen, device=gpu).float() / 8
            alpha = 0.5
        else:
            y0, a, alpha = torch.randn(n, generator=gen, device=gpu), torch.randn(n, generator=gen, device=gpu), MOM
        y = sent((n + 8,), gpu)
        y[:n] = y0
        launch('dv_addcmul_f32', y.data_ptr(), a.data_ptr(), 0, alpha, n)
        torch.cuda.synchronize()
        assert is_sent(y[n:]), 'addcmul wrote past n'
        al = float(torch.tensor(alpha, dtype=torch.float32))
        ref = y0.double() + al * a.double()
        if exact:
            assert torch.equal(y[:n].double(), ref)
        else:
            print()
            within(y[:n].double(), ref, 3 * U * (y0.double().abs() + (al * a.double()).abs()), f'addcmul n={n}')


HEAD = [(c.tile_rows, c.C) for c in T.STATS_CASES if c.name.startswith('bn1d')]


@pytest.mark.parametrize('M,C_', HEAD, ids=['m%d_c%d' % h for h in HEAD])
def test_head_batchnorm1d_chain(gpu, M, C_):
    """the classifier head's BatchNorm1d: dv_bn_rows_partials_f32 (ldx > C) -> dv_bn_stats_finalize(n_tiles = 1, tile_rows = M)
    -> dv_bn_apply -> ordered dv_bn_bwd_reduce (DV_NO_RELU_MASK) -> dv_bn_bwd_apply, against float64 training-mode
    BatchNorm1d, running statistics included"""
    w = f'head M={M} C={C_}'
    m = Member(gpu, DV_F32, M, C_, 71, exact=False, relu=False, views=True, tile_rows=M)
    assert m.n_tiles == 1 and m.x.ld > C_
    part = sent((2 * C_ + 8,), gpu)
    launch('dv_bn_rows_partials_f32', m.x.ptr, m.x.ld, M, C_, part.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(part[2 * C_:]), f'{w}: partials past [2][C]'
    x = m.x.val()
    ref = REF.bn1d_reference(x, m.gamma, m.beta, m.rm0.double(), m.rv0.double(), m.dy.val(), EPS, MOM)
    S, M2 = ref['S'], ref['M2']
    mean = S / M
    dps = M * U * x.abs().sum(0)                                                   # M sequential additions
    ones = torch.ones((M, 1), dtype=torch.float64, device=gpu)
    dpq = m2_bound(ones, torch.zeros_like(x), x - mean, torch.zeros_like(x), torch.zeros_like(x), dps / M + U * mean.abs(), M)
    print(f'\n  {w}')
    within(part[:C_].double(), S, dps, f'{w} partial sums')
    within(part[C_:2 * C_].double(), M2, dpq, f'{w} partial M2')
    m.part, m.coff, m.pitch = part[:2 * C_].view(2, C_, 1), 0, C_
    local = sent((2 * C_ + 1,), gpu)
    stats_finalize(m, local)
    torch.cuda.synchronize()
    chain = stats_chain(1)
    dS = dps + chain * U * (S.abs() + dps)
    n1 = torch.full((1, 1), float(M), dtype=torch.float64, device=gpu)
    a = m.ps() / M
    dM2 = m2_bound(n1, dps[None] / M + U * a.abs(), a - mean, m.pq(), dpq[None], dS / M + U * mean.abs(), chain)
    MU.check_finalized(m, m.o, S, M2, M, dS, dM2, m.rm, m.rv, w)
    adopt(m, m.o)
    g, xhat = forward_for_backward(m, w)
    ordered_reduce_twice(m, g, xhat, w)
    bwd_apply(m, m.sums[0], 1, 1.0 / M)
    torch.cuda.synchronize()
    MU.check_bwd_apply(m, g, m.sums[0], 1.0 / M, w)


FILL = [(1, 1, 1, 0), (51, 5, 9, 4), (257, 1, 3, 0), (85, 3, 3, 0), (300000, 4, 7, 2)]


@pytest.mark.parametrize('rows,ncols,pitch,col0', FILL, ids=['r%d_n%d_p%d_c%d' % f for f in FILL])
def test_fill_cols(gpu, rows, ncols, pitch, col0):
    """dv_fill_cols_f32: only columns [col0, col0 + ncols) of a sentinel [rows][pitch] buffer change (rows * ncols = 1, 255,
    257, and past one trip of the 4096-block grid; col0 = 0 and col0 + ncols = pitch included)"""
    buf = sent((rows * pitch + 8,), gpu)
    launch('dv_fill_cols_f32', buf.data_ptr(), rows, pitch, col0, ncols, -1.25)
    torch.cuda.synchronize()
    v = buf[:rows * pitch].view(rows, pitch)
    assert bool((v[:, col0:col0 + ncols] == -1.25).all()), 'a column of the range was not filled'
    assert is_sent(v[:, :col0]) and is_sent(v[:, col0 + ncols:]) and is_sent(buf[rows * pitch:])
    if rows == 300000:
        assert rows * ncols > 4096 * 256
