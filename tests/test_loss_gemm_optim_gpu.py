"""The loss, fp32 GEMM and optimizer entries (csrc/loss.hip; dv_sgd_momentum, dv_ema, dv_cast_arena of csrc/optim.hip; dv_mean_f32,
dv_colsum_f32 of csrc/elementwise.hip) against plain float64 references of the same operations, written here from include/dualvar_hip.h.

Every entry is called through the C ABI on explicit tensors.  Inputs sit in buffers whose gaps (pitch padding, the float in
front of an offset base) hold NaN, outputs in buffers filled with a NaN bit pattern no kernel produces (SENT): a read or a
write outside the stated range shows as a NaN in the result or as a changed sentinel.  Two kinds of data:

  (A) exactly representable: operands are integers in [-2, 2] / 4, alpha / inv_T / bias / lr / mu / wd / grad_scale powers of
      two (or sums of two).  The host asserts sum|terms| < 2^24 units of the terms' common dyadic unit, so every fp32 sum is exact in
      any order and the plain, four-wave, grouped and split-K (atomic and ordered) GEMMs, the reference-ordered logits, rank0,
      the margin logits and the SGD / EMA arithmetic must equal float64 BIT FOR BIT (compared as int32 after adding +0.0, which
      only folds -0 into +0).  Ties between a negative and the positive are frequent on this data (asserted from the float64
      reference), which pins the strict `>` of rank0.  dq of InfoNCE is exact only on one-hot data (see
      test_infonce_ordered_splitk_exact_onehot): there the ordered and the atomic split-K must give the same bits.
  (B) Gaussian data at the training shapes against float64 with DERIVED bounds.  u = 2^-24.  Notation: b(x) the bound on x.
      Device functions (no accuracy figure ships with the compiler's headers; measured on gfx950 against float64 over 2^20
      arguments per range by a standalone device program, and taken with a factor 2):
        __expf(x), x in [-87, 45]:  measured rel. error <= max(2.10, 2.04 |x|) u   -> E_EXP(x) = (4.2 + 4.1 |x|) u
                                    (v_exp_f32 of x * log2(e): the product's rounding is scaled by |x|)
        expf(x),  x in [-87, 0]:    measured 1.39 u -> 2.8 u;    logf(x), x in [1, 8192]: measured 2.68 u -> E_LOG = 5.4 u
        log1pf(x), x in [1e-38, 1e19]: measured 1.05 u -> E_LOG1P = 2.1 u
        1.f / x: measured exactly u (correctly rounded IEEE division) -> u, like every other single operation
      test_device_function_figures re-measures what the ABI lets one isolate (__expf on both signs, the reciprocal)
      and asserts it stays under half of E_EXP.  Where __expf may flush to 0 (below 2^-126) the bounds carry that as an
      absolute term (TINY).
      GEMM element:  b = (L + 2) u |alpha| sum_k |a_k b_k|, L the longest chain of sequential fp32 additions of the form taken
                     (gemm_chain: K for the one-wave kernel; 16 ceil(ceil(K/16)/4) + 3 for the four-wave kernels, the 3 being the
                     LDS fold; for split-K that of one slice plus the number of slices), + 2 for the product and alpha.
      NT-Xent:       b(s_rc) the GEMM bound with L(D);  logits: b(s).
                     lse_r:  max_c b(s_rc)  [lse is 1-Lipschitz in max-norm]  + (L_se + 1) u  [chain of the sum of exp:
                             ceil(2N/64) + 6, relative, all terms positive; + 1: the max term]  + sum_c p_c (E_EXP(x_c) + u |x_c|)
                             [x_c = s_c - max: one rounding, then __expf]  + E_LOG |log se| + u |lse|
                     loss_r: b(lse_r) + b(s_r,pos) + u |loss_r|
                     dsim:   g [p (E_EXP(x) + b(s) + b(lse) + u |x|) + u |p - 1_pos|] + 2u |dsim|,  x = s - lse, g = inv_T / R
                     rank0:  #{c: s_c - s_pos > b(s_c) + b(s_pos)} <= rank0 <= #{c: s_c - s_pos >= -(b(s_c) + b(s_pos))}
                     drows / dcols: the GEMM bound on the computed dsim + b(dsim) carried through |cols| / |rows|
      InfoNCE:       as NT-Xent with L(l0) = ceil(D/256) + 10, L_se = ceil(K/256) + 11;  dq adds the axpy's two roundings.
      rank margin:   b(S_ij) = (D + 1) u sum|f_i f_j|;  z = (lo - hi) / theta: b(z) = (b(lo) + b(hi)) / theta + 2u |z|;
                     softplus term: b(z) + (E_EXP(z) sigmoid(z) + E_LOG1P) softplus(z)  [d log1p(e) / de * e = sigmoid];  the row
                     sum, wave fold, weight / count and the sum over samples add (2s + 8 + ceil(Bn/256) + 11) u |loss|.
                     dfeats: b(sigmoid) = sigmoid (1 - sigmoid) b(z) + sigmoid (E_EXP(z) + 2u); dz has 3 more roundings; dS chains of
                     2s - 2; df = (dS + dS^T) f with a chain of 2s + 2.  No |z - clip| may be below b(z) (asserted: data property).
      softmax CE / rows, group mean, mean, colsum: the same constructions; see the functions.
      SGD:           per step  b(d) = u (|g gs| + |wd p| + |d|) + wd b(p);  b(buf') = mu b(buf) + u |mu buf| + b(d) + u |buf'|;
                     b(p') = b(p) + lr b(buf') + u |lr buf'| + u |p'|, accumulated over the steps against float64 carried in
                     float64.  lr, mu, wd, grad_scale are taken as the fp32 values the entry receives.
      Each case prints (-s) err / bound.  Largest err / bound measured on an MI355X, per quantity:
        ntxent   logits 0.16  loss_rows 0.30  dsim 0.35  drows 0.07  dcols 0.16      (rank0 inside its interval in every row;
                 the interval is 0 wide in 78 - 100 % of the rows, at most 3 wide at N = 2048)
        infonce  logits 0.07  loss_rows 0.24  dlogits 0.34  dq 0.09 (plain, atomic and ordered)
        margin   logits 0.05  loss 0.05  dfeats 0.05         sigmoid epilogue 0.69
        softmax_ce loss 0.56  dlogits 0.48   softmax_rows 0.29   group_mean 0.54 / 0.67 (bwd)   mean 0.91   colsum 0.15
        sgd      p 1.00 (0.997: single operations reach their half ulp)  buf 0.63
      The whole file takes about 9 s on an MI355X.
Finding (test_ntxent_drows_splitk_is_atomic): drows of NT-Xent at 2N >= 4096 and <= 64 output tiles goes through dv_gemm_f32's
atomic split-K: inside the bound (<= 0.005), but about 70 % of the 32 768 elements differ in bits between two launches.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_F32, DV_RELU, DV_SIGMOID  # noqa: E402
from tests import checks  # noqa: E402
from tests.chains import E_EXPF, E_LOG, E_LOG1P, TINY, e_exp, gemm_bound, gemm_chain, gemm_form, splitk_plan  # noqa: E402
from tests.checks import F64, U, Ratios, ceil_div, f32, is_sent, report_fixture, sent  # noqa: E402
from tests.optim_support import arena, check_copy, copy_buffer  # noqa: E402

RATIO = Ratios()                  # quantity -> largest err / bound of the run
within = RATIO.within
_report = report_fixture(RATIO, 34)
# bit for bit against float64: the reference must be an fp32 number; + 0.0 on both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)


# ----------------------------------------------------------------------------------------------------------- helpers
def grid(gen, shape, dev, density=1.0):
    """integers in [-2, 2] / 4 as float64 on the device"""
    v = torch.randint(-2, 3, shape, generator=gen, dtype=torch.int64)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=gen) < density)
    return (v.double() / 4).to(dev)


class Mat:
    """[rows][K] values stored k-contiguous (row pitch K + pe) or k-strided ([K][rows + pe]) at `off` floats from an aligned
    base; every gap holds NaN"""

    def __init__(self, vals64, kcontig, pe=0, off=0):
        rows, K = vals64.shape
        shape = (rows, K + pe) if kcontig else (K, rows + pe)
        n = shape[0] * shape[1]
        self.flat = torch.full((off + n + 4,), float('nan'), dtype=torch.float32, device=vals64.device)
        v = self.flat[off:off + n].view(shape)
        if kcontig:
            v[:, :K] = vals64.float()
            self.srow, self.sk = K + pe, 1
        else:
            v[:, :rows] = vals64.t().float()
            self.srow, self.sk = 1, rows + pe
        self.ptr = self.flat.data_ptr() + 4 * off
        self.vals = vals64


class Out:
    """[M][N] result inside a sentinel buffer of M + 2 rows and pitch N + pe, optionally holding C0"""

    def __init__(self, M, N, pe, dev, c0=None):
        self.M, self.N, self.ld = M, N, N + pe
        self.buf = sent((M + 2, self.ld), dev)
        if c0 is not None:
            self.buf[:M, :N] = c0.float()

    @property
    def val(self):
        return self.buf[:self.M, :self.N]

    def frame_ok(self):
        return is_sent(self.buf[:self.M, self.N:]) and is_sent(self.buf[self.M:])


# ----------------------------------------------------------------------------------------------------------- GEMM plan
def splitk_ws_bytes(M, N, K):
    tiles, splits, _ = splitk_plan(M, N, K)
    return (splits * tiles * 1024 + ((tiles + 7) & ~7)) * 4 if splits else 0


def assert_exact_sum(A64, B64t, alpha, extra=None):
    """every partial sum of alpha * A.B (+ extra) is an integer below 2^24 in units of the operands' common dyadic unit"""
    unit = min(abs(alpha), 1.0) / 16 / 2
    tot = abs(alpha) * (A64.abs() @ B64t.abs().t())
    if extra is not None:
        tot = tot + extra
    assert float(tot.max()) / unit < 2 ** 24


def run_gemm(dev, gen, M, N, K, a_kc, b_kc, pe, off, alpha, acc, cpe=3):
    A64 = grid(gen, (M, K), dev, min(1.0, 2048 / K))
    B64 = grid(gen, (N, K), dev, min(1.0, 2048 / K))
    C0 = grid(gen, (M, N), dev) * 4 if acc else None
    assert_exact_sum(A64, B64, alpha, C0.abs() if acc else None)
    a, b, c = Mat(A64, a_kc, pe, off), Mat(B64, b_kc, pe, off), Out(M, N, cpe, dev, C0)
    ops.call('dv_gemm_f32', M, N, K, a.ptr, a.srow, a.sk, b.ptr, b.sk, b.srow, c.buf, c.ld, alpha, int(acc))
    ref = alpha * (A64 @ B64.t())
    if acc:
        ref = ref + C0
    what = f'dv_gemm_f32 {M}x{N}x{K} {gemm_form(M, N, K)} a_kc={a_kc} b_kc={b_kc} pe={pe} off={off} alpha={alpha} acc={acc}'
    same_bits(c.val, ref, what)
    assert c.frame_ok(), what + ': wrote outside [M][N]'
    return c


SWEEP = [  # plain: K < 64 or more than 1024 tiles
    (1, 1, 1), (5, 31, 2), (33, 5, 3), (31, 33, 15), (32, 32, 16), (65, 64, 17), (128, 65, 63), (257, 4200, 40), (257, 4200, 8),
    (257, 4200, 64), (1025, 1024, 64), (1025, 1024, 65),
    # four waves per tile: <= 1024 tiles, K >= 64, not split
    (1, 5, 64), (33, 31, 65), (64, 128, 127), (5, 257, 255), (128, 128, 256), (65, 33, 257), (31, 64, 832), (128, 1024, 1024),
    (1024, 1024, 64), (257, 257, 4096), (257, 256, 4097), (257, 257, 5000), (64, 64, 4095), (128, 257, 4095), (1, 1, 4095),
    # split-K: <= 64 tiles, K >= 4096
    (256, 256, 4096), (64, 64, 4096), (128, 257, 4096), (32, 128, 4097), (1, 1, 5000), (33, 65, 5000), (5, 31, 4096),
    (32, 128, 65536), (128, 128, 65536), (1, 5, 65536)]
ALPHAS = [1.0, -1.0, 0.5, 2.0, 16.0, -0.5]
PES = [0, 4, 3, 8, 1]


def test_sweep_reaches_every_form_and_threshold():
    """the shape list puts at least three shapes on each side of each rule of launch_gemm_f32 / gemm_splitk_plan"""
    forms = [gemm_form(*s) for s in SWEEP]
    assert min(forms.count(f) for f in ('plain', 'tile4', 'split')) >= 7
    t = lambda s: ceil_div(s[0], 32) * ceil_div(s[1], 32)  # noqa: E731
    assert sum(1 for s in SWEEP if s[2] >= 4096 and t(s) <= 64) >= 3 and sum(1 for s in SWEEP if s[2] >= 4096 and t(s) > 64) >= 3
    assert sum(1 for s in SWEEP if t(s) <= 64 and 4000 <= s[2] < 4096) >= 3
    assert sum(1 for s in SWEEP if t(s) > 1024) >= 3 and sum(1 for s in SWEEP if t(s) == 1024) >= 1
    assert sum(1 for s in SWEEP if s[2] < 64) >= 3 and sum(1 for s in SWEEP if 64 <= s[2] < 4096 and t(s) <= 1024) >= 3
    plans = [splitk_plan(*s) for s in SWEEP if gemm_form(*s) == 'split']
    assert any(sp * ks > s[2] for (_, sp, ks), s in zip(plans, [s for s in SWEEP if gemm_form(*s) == 'split']))   # ragged slice
    assert any(sp == 1024 // tl for tl, sp, _ in plans) and any(sp < 1024 // tl for tl, sp, _ in plans)
    assert splitk_plan(1, 1, 5000) == (1, 16, 320) and splitk_plan(32, 128, 4097) == (4, 13, 320)


@pytest.mark.parametrize('i', range(len(SWEEP)), ids=['%dx%dx%d' % s for s in SWEEP])
def test_gemm_f32_exact(gpu, i):
    M, N, K = SWEEP[i]
    gen = torch.Generator().manual_seed(100 + i)
    for rep in range(2):                      # two layouts per shape, every (a, b) storage pair over the sweep
        j = 2 * i + rep
        run_gemm(gpu, gen, M, N, K, a_kc=(j & 1) == 0, b_kc=(j >> 1) & 1 == 0, pe=PES[j % 5], off=(j // 3) & 1,
                 alpha=ALPHAS[j % 6], acc=j % 3 == 1)


@pytest.mark.parametrize('a_kc', [True, False])
@pytest.mark.parametrize('b_kc', [True, False])
def test_gemm_f32_operand_switch(gpu, a_kc, b_kc):
    """the vectorised / strided operand switch of the four-wave body: stride 1, pitch % 4, base % 16, all twelve states"""
    gen = torch.Generator().manual_seed(7)
    for pe in (0, 4, 3):
        for off in (0, 1):
            for (M, N, K) in ((33, 65, 100), (64, 32, 832)):
                run_gemm(gpu, gen, M, N, K, a_kc, b_kc, pe, off, alpha=0.5, acc=off == 1)


def atomic_vs_two_launches(dev, M, N, K):
    gen = torch.Generator().manual_seed(11)
    c1 = run_gemm(dev, gen, M, N, K, True, False, 0, 0, 1.0, False)
    gen = torch.Generator().manual_seed(11)
    c2 = run_gemm(dev, gen, M, N, K, True, False, 0, 0, 1.0, False)
    assert torch.equal(c1.buf.view(torch.int32), c2.buf.view(torch.int32))


def test_gemm_splitk_atomic_exact_repeat(gpu):
    atomic_vs_two_launches(gpu, 256, 128, 4096)


# ------------------------------------------------------------------------------------------------- dv_gemm_f32_ex / grouped
def make_desc(dev, gen, M, N, K, flags, alpha, bias, a_kc, b_kc, pe, off, cpe=2):
    A64 = grid(gen, (M, K), dev, min(1.0, 2048 / K))
    B64 = grid(gen, (N, K), dev, min(1.0, 2048 / K))
    bias64 = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0, 16.0], dtype=F64)[torch.randint(0, 6, (N,), generator=gen)].to(dev) if bias else None
    C0 = grid(gen, (M, N), dev) * 4 if flags & DV_ACCUM else None
    extra = torch.zeros((M, N), dtype=F64, device=dev)
    if bias:
        extra = extra + bias64.abs()
    if C0 is not None:
        extra = extra + C0.abs()
    assert_exact_sum(A64, B64, alpha, extra)
    a, b, c = Mat(A64, a_kc, pe, off), Mat(B64, b_kc, pe, off), Out(M, N, cpe, dev, C0)
    bias_buf = None
    if bias:
        bias_buf = torch.full((N + 1,), float('nan'), dtype=torch.float32, device=dev)
        bias_buf[:N] = bias64.float()
    d = L.GemmDesc()
    d.A, d.B, d.C, d.bias = a.ptr, b.ptr, c.buf.data_ptr(), bias_buf.data_ptr() if bias else None
    d.sam, d.sak, d.sbk, d.sbn, d.ldc = a.srow, a.sk, b.sk, b.srow, c.ld
    d.M, d.N, d.K, d.flags, d.tile_end, d.alpha = M, N, K, flags, 0, alpha
    pre = alpha * (A64 @ B64.t())
    if bias:
        pre = pre + bias64
    if C0 is not None:
        pre = pre + C0
    return d, dict(a=a, b=b, c=c, c0=C0, bias=bias_buf, pre=pre, flags=flags,
                   what=f'{M}x{N}x{K} flags={flags} alpha={alpha} bias={bias}')


def check_desc_result(k):
    c, pre, flags = k['c'], k['pre'], k['flags']
    if flags & DV_SIGMOID:
        sg = torch.sigmoid(pre)             # 1 / (1 + e), e = __expf(-pre): E_EXP e / (1 + e), the add, the division
        within(c.val, sg, sg * (e_exp(pre) * (1 - sg) + 2 * U) + TINY, 'sigmoid ' + k['what'], quiet=True)
    else:
        same_bits(c.val, pre.clamp_min(0) if flags & DV_RELU else pre, 'gemm_desc ' + k['what'])
    assert c.frame_ok(), k['what'] + ': wrote outside [M][N]'


EX_K = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 255, 256, 257, 832, 1024, 4097]
EX_MN = [(1, 1), (5, 33), (31, 64), (32, 5), (33, 31), (64, 65), (65, 128), (128, 1), (257, 32)]
EX_FLAGS = [0, DV_RELU, DV_ACCUM, DV_ACCUM | DV_RELU, DV_SIGMOID, DV_SIGMOID | DV_ACCUM]


@pytest.mark.parametrize('K', EX_K)
def test_gemm_f32_ex_exact(gpu, K):
    gen = torch.Generator().manual_seed(300 + K)
    ki = EX_K.index(K)
    for r in range(6):
        j = 6 * ki + r
        M, N = EX_MN[j % 9]
        flags = EX_FLAGS[j % 6]
        args = dict(alpha=ALPHAS[(j // 2) % 6], bias=j % 4 != 3, a_kc=(j & 1) == 0, b_kc=(j >> 1) & 1 == 0, pe=PES[j % 5],
                    off=(j // 3) & 1)
        gs = gen.get_state()
        d, k = make_desc(gpu, gen, M, N, K, flags & ~DV_SIGMOID, **args)      # the pre-activation, bit for bit
        ops.call('dv_gemm_f32_ex', d)
        check_desc_result(k)
        if flags & DV_SIGMOID:
            gen.set_state(gs)
            d, k = make_desc(gpu, gen, M, N, K, flags, **args)
            ops.call('dv_gemm_f32_ex', d)
            check_desc_result(k)


GROUP_SHAPES = [(33, 65, 832), (1, 5, 3), (64, 64, 64), (5, 31, 17), (128, 33, 256), (32, 32, 16), (65, 1, 1024), (31, 257, 65),
                (257, 5, 127), (5, 5, 2), (64, 128, 255), (33, 33, 15), (1, 64, 63)]


@pytest.mark.parametrize('n_groups', [1, 8, 9, 13])
def test_gemm_f32_grouped_exact(gpu, n_groups):
    """mixed sizes; one descriptor (two from nine on: one in the first eight, one in the walked part) with an empty tile
    range; three surplus workgroups"""
    gen = torch.Generator().manual_seed(500 + n_groups)
    empty = {1: (), 8: (2,), 9: (2, 8), 13: (0, 10)}[n_groups]
    descs, keep, end = (L.GemmDesc * n_groups)(), [], 0
    for g in range(n_groups):
        M, N, K = GROUP_SHAPES[g]
        d, k = make_desc(gpu, gen, M, N, K, [0, DV_RELU, DV_ACCUM, DV_ACCUM | DV_RELU][g % 4], ALPHAS[g % 6], g % 3 != 2,
                         (g & 1) == 0, (g >> 1) & 1 == 0, PES[g % 5], (g // 3) & 1)
        if g not in empty:
            end += ceil_div(M, 32) * ceil_div(N, 32)
        d.tile_end = end
        descs[g] = d
        keep.append(k)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(gpu)
    ops.call('dv_gemm_f32_grouped', table, n_groups, end + 3)
    for g, k in enumerate(keep):
        if g in empty:
            c = k['c']
            if k['flags'] & DV_ACCUM:
                assert c.frame_ok() and bool((c.val.double() == k['c0']).all()), f'group {g} has no tiles but its C changed'
            else:
                assert is_sent(c.buf), f'group {g} has no tiles but its C was written'
        else:
            check_desc_result(k)


# ----------------------------------------------------------------------------------------------------------- NT-Xent
def ntxent_ref(rows, cols, n_local, N, row_index0, inv_T):
    """float64, from include/dualvar_hip.h: s = rows.cols^T * inv_T; row r is global index gi, its positive (gi + N) % 2N;
    logits = [positive, the others in index order without self and positive]; loss = logsumexp(logits) - positive;
    rank0 = #{negatives > positive}; dsim = (softmax - onehot) * inv_T / R, 0 at self"""
    R, C2 = rows.shape[0], 2 * N
    dev = rows.device
    r = torch.arange(R, device=dev)
    gi = row_index0 + (r // n_local) * N + r % n_local
    pos = (gi + N) % C2
    s = (rows @ cols.t()) * inv_T
    c = torch.arange(C2, device=dev)[None, :]
    is_self, is_pos = c == gi[:, None], c == pos[:, None]
    neg = ~(is_self | is_pos)
    sp = s[r, pos]
    logits = torch.cat([sp[:, None], s[neg].view(R, C2 - 2)], 1)
    lse = torch.logsumexp(logits, 1)
    rank = (neg & (s > sp[:, None])).sum(1)
    p = torch.exp(s - lse[:, None])
    g = f32(f32(inv_T) / np.float32(R))
    dsim = torch.where(is_self, torch.zeros_like(p), (p - is_pos.double()) * g)
    return dict(s=s, gi=gi, pos=pos, sp=sp, neg=neg, is_self=is_self, is_pos=is_pos, logits=logits, lse=lse, loss=lse - sp,
                rank=rank, p=torch.where(is_self, torch.zeros_like(p), p), dsim=dsim, g=g)


def run_ntxent(dev, rows, cols, n_local, N, row_index0, inv_T, exact, tag):
    R, D = rows.shape
    C2 = 2 * N
    rows32, cols32 = rows.float().contiguous(), cols.float().contiguous()
    rows, cols = rows32.double(), cols32.double()
    logits, loss, dsim = sent((R + 1, C2 - 1), dev), sent((R + 8,), dev), sent((R + 1, C2), dev)
    rank0 = sent((R + 8,), dev, torch.int32)
    ops.call('dv_ntxent_fwd', rows32, cols32, R, n_local, N, D, row_index0, inv_T, logits, loss, rank0, dsim)
    torch.cuda.synchronize()
    assert is_sent(logits[R:]) and is_sent(loss[R:]) and is_sent(rank0[R:]) and is_sent(dsim[R:]), tag + ': wrote past its rows'
    ref = ntxent_ref(rows, cols, n_local, N, row_index0, f32(inv_T))
    rr = torch.arange(R, device=dev)
    chain = gemm_chain(R, C2, D)
    if exact:
        assert_exact_sum(rows, cols, inv_T)
        spread = float((ref['logits'].max(1).values - ref['logits'].min(1).values).max())
        assert spread < 40, spread
        b = torch.zeros_like(ref['s'])
        same_bits(logits[:R], ref['logits'], tag + ' logits')
        assert torch.equal(rank0[:R].long(), ref['rank']), tag + ': rank0 differs from #{negatives > positive}'
        tie = (ref['neg'] & (ref['s'] == ref['sp'][:, None])).any(1).double().mean().item()
        print(f'    {tag}: rows with a negative tying the positive {tie:.2f}, logit spread {spread:.1f}')
        if N >= 37:
            assert tie >= 0.5
    else:
        b = gemm_bound(rows, cols, inv_T, chain)
        bl = torch.cat([b[rr, ref['pos']][:, None], b[ref['neg']].view(R, C2 - 2)], 1)
        within(logits[:R], ref['logits'], bl, f'ntxent.logits {tag}')
        bb = b + b[rr, ref['pos']][:, None]
        diff = ref['s'] - ref['sp'][:, None]
        lo, hi = (ref['neg'] & (diff > bb)).sum(1), (ref['neg'] & (diff >= -bb)).sum(1)
        got = rank0[:R].long()
        assert bool(((got >= lo) & (got <= hi)).all()), tag + ': rank0 outside the interval the similarity bound allows'
        print(f'    {tag}: rank0 median {int(got.median())} max {int(got.max())}; interval width 0 in {float((hi == lo).double().mean()):.2f}'
              f' of rows, max {int((hi - lo).max())}')
    # loss and gradient
    mask = ~ref['is_self']
    mx = torch.where(mask, ref['s'], torch.full_like(ref['s'], -1e300)).max(1).values
    x = torch.where(mask, ref['s'] - mx[:, None], torch.zeros_like(ref['s']))
    b_in = torch.where(mask, b, torch.zeros_like(b)).max(1).values
    b_lse = b_in + (ceil_div(C2, 64) + 6 + 1) * U + (ref['p'] * (e_exp(x) + U * x.abs())).sum(1) + E_LOG * (ref['lse'] - mx).abs() \
        + U * ref['lse'].abs()
    within(loss[:R], ref['loss'], b_lse + b[rr, ref['pos']] + U * ref['loss'].abs(), f'ntxent.loss_rows {tag}')
    xl = ref['s'] - ref['lse'][:, None]
    b_d = ref['g'] * (ref['p'] * (e_exp(xl) + b + b_lse[:, None] + U * xl.abs()) + U * (ref['p'] - ref['is_pos'].double()).abs() + TINY) \
        + 2 * U * ref['dsim'].abs()
    b_d = torch.where(mask, b_d, torch.zeros_like(b_d))
    within(dsim[:R], ref['dsim'], b_d, f'ntxent.dsim {tag}')
    return ref, dsim, b_d, rows32, cols32


NTXENT_CASES = [(6, 6, 0, 128), (37, 37, 0, 48), (64, 64, 0, 128), (128, 128, 0, 128), (1024, 128, 0, 128), (1024, 128, 384, 128),
                (1024, 128, 896, 64), (2048, 256, 1792, 128), (2049, 1, 2048, 20)]
NT_IDS = ['N%d-n%d-r%d-D%d' % c for c in NTXENT_CASES]


def local_rows(cols, n_local, N, row_index0):
    return torch.cat([cols[row_index0:row_index0 + n_local], cols[N + row_index0:N + row_index0 + n_local]], 0)


@pytest.mark.parametrize('case', NTXENT_CASES, ids=NT_IDS)
def test_ntxent_grid_exact(gpu, case):
    N, n_local, row_index0, D = case
    gen = torch.Generator().manual_seed(N + D)
    cols = grid(gen, (2 * N, D), gpu)
    run_ntxent(gpu, local_rows(cols, n_local, N, row_index0), cols, n_local, N, row_index0, 2.0 if D >= 100 else 4.0, True,
               'grid ' + NT_IDS[NTXENT_CASES.index(case)])


def test_ntxent_grid_exact_rows_differ_from_cols(gpu):
    """the tc head passes series means: rows are not rows of cols"""
    gen = torch.Generator().manual_seed(5)
    N, n_local, row_index0, D = 1024, 128, 640, 128
    cols = grid(gen, (2 * N, D), gpu)
    run_ntxent(gpu, grid(gen, (2 * n_local, D), gpu), cols, n_local, N, row_index0, 2.0, True, 'grid rows!=cols')


def gauss_views(gen, N, D, dev):
    """L2-normalised, the two views of a sample weakly correlated (0.12 a + b): rank0 spreads over its whole range"""
    a = torch.randn((N, D), generator=gen, dtype=F64)
    f = torch.cat([0.12 * a + torch.randn((N, D), generator=gen, dtype=F64) for _ in range(2)], 0)
    return torch.nn.functional.normalize(f, dim=1).to(dev)


@pytest.mark.parametrize('T', [0.07, 0.5])
@pytest.mark.parametrize('case', NTXENT_CASES + [(64, 64, 0, 128)], ids=NT_IDS + ['headline-128-clips'])
def test_ntxent_gaussian_bounds(gpu, case, T):
    N, n_local, row_index0, D = case
    gen = torch.Generator().manual_seed(N * 3 + D)
    cols = gauss_views(gen, N, D, gpu)
    rows = local_rows(cols, n_local, N, row_index0)
    tag = f'T={T} ' + 'N%d-n%d-r%d-D%d' % case
    ref, dsim, b_d, rows32, cols32 = run_ntxent(gpu, rows, cols, n_local, N, row_index0, 1.0 / T, False, tag)
    # the two products of functional._NTXentFn.backward, on the kernel's own dsim
    R, C2 = rows.shape[0], 2 * N
    ds = dsim[:R].contiguous()
    drows, dcols = Out(R, D, 1, gpu), Out(C2, D, 1, gpu)
    ops.call('dv_gemm_f32', R, D, C2, ds, C2, 1, cols32, D, 1, drows.buf, drows.ld, 1.0, 0)
    ops.call('dv_gemm_f32', C2, D, R, ds, 1, C2, rows32, D, 1, dcols.buf, dcols.ld, 1.0, 0)
    c64, r64 = cols32.double(), rows32.double()
    within(drows.val, ref['dsim'] @ c64, (gemm_chain(R, D, C2) + 2) * U * (ds.double().abs() @ c64.abs()) + b_d @ c64.abs(),
           f'ntxent.drows {tag} {gemm_form(R, D, C2)}')
    within(dcols.val, ref['dsim'].t() @ r64, (gemm_chain(C2, D, R) + 2) * U * (ds.double().abs().t() @ r64.abs()) + b_d.t() @ r64.abs(),
           f'ntxent.dcols {tag} {gemm_form(C2, D, R)}')
    assert drows.frame_ok() and dcols.frame_ok()


def test_ntxent_drows_splitk_is_atomic(gpu):
    """R = 256, D = 128, 2N = 4096: 32 tiles and K >= 4096, so dv_gemm_f32 splits K, and without a workspace argument it adds the
    slices with float atomics.  Each launch is held to the float64 bound; two launches are compared and the outcome printed.
    Their bits may differ (the order of the atomic additions is not fixed), so equality is NOT asserted: run-to-run identical
    drows at this shape needs an entry that takes a workspace."""
    gen = torch.Generator().manual_seed(9)
    N, n_local, D = 2048, 128, 128
    R, C2 = 2 * n_local, 2 * N
    assert gemm_form(R, D, C2) == 'split'
    cols = gauss_views(gen, N, D, gpu)
    ds64 = torch.randn((R, C2), generator=gen, dtype=F64).to(gpu) * 1e-3
    ds, c32 = ds64.float().contiguous(), cols.float().contiguous()
    outs = []
    for _ in range(2):
        o = Out(R, D, 0, gpu)
        ops.call('dv_gemm_f32', R, D, C2, ds, C2, 1, c32, D, 1, o.buf, o.ld, 1.0, 0)
        within(o.val, ds.double() @ c32.double(), gemm_bound(ds.double(), c32.double().t().contiguous(), 1.0, gemm_chain(R, D, C2)),
               'gemm.splitk_atomic drows 256x128x4096')
        outs.append(o.val.clone())
    n_diff = int((outs[0].view(torch.int32) != outs[1].view(torch.int32)).sum())
    print(f'    atomic split-K drows: {n_diff} of {outs[0].numel()} elements differ in bits between two launches')


# ----------------------------------------------------------------------------------------------------------- InfoNCE
INFONCE_CASES = [(1, 20, 96), (5, 128, 96), (32, 128, 4095), (32, 128, 4096), (40, 100, 4097), (128, 128, 65536), (256, 256, 65536)]


def infonce_ref(q, k, queue, inv_T):
    B = q.shape[0]
    l0 = (q * k).sum(1) * inv_T
    ln = (q @ queue) * inv_T
    logits = torch.cat([l0[:, None], ln], 1)
    lse = torch.logsumexp(logits, 1)
    g = f32(f32(inv_T) / np.float32(B))
    p = torch.exp(logits - lse[:, None])
    dl = p * g
    dl[:, 0] -= g
    dq = dl[:, 1:] @ queue.t() + dl[:, :1] * k
    return dict(logits=logits, lse=lse, loss=lse - l0, rank=(ln > l0[:, None]).sum(1), p=p, dl=dl, dq=dq, g=g)


def run_infonce(dev, q, k, queue, inv_T, exact, tag, form):
    """form: 'none' (no workspace passed), 'ordered' (workspace of dv_infonce_workspace bytes)"""
    B, D = q.shape
    K = queue.shape[1]
    q32, k32, qu32 = q.float().contiguous(), k.float().contiguous(), queue.float().contiguous()
    q, k, queue = q32.double(), k32.double(), qu32.double()
    lib = L.load()
    ws_bytes = int(lib.dv_infonce_workspace(B, D, K))
    # the plan of dq = dlogits . queue^T (M = B, N = D over K): split when it has <= 64 tiles of 32 x 32 and K >= 4096
    assert (ws_bytes > 0) == (ceil_div(B, 32) * ceil_div(D, 32) <= 64 and K >= 4096) and ws_bytes == splitk_ws_bytes(B, D, K)
    logits, dlog = sent((B + 1, K + 1), dev), sent((B + 1, K + 1), dev)
    loss, rank0, dq = sent((B + 8,), dev), sent((B + 8,), dev, torch.int32), sent((B + 1, D), dev)
    ws = None
    if form == 'ordered' and ws_bytes:
        ws = torch.zeros(ws_bytes // 4 + 8, dtype=torch.float32, device=dev)
        ws[ws_bytes // 4:] = float('nan')
    ops.call('dv_infonce_fwd', q32, k32, qu32, B, D, K, inv_T, logits, loss, rank0, dlog, dq, ws, ws_bytes if ws is not None else 0)
    torch.cuda.synchronize()
    assert is_sent(logits[B:]) and is_sent(dlog[B:]) and is_sent(loss[B:]) and is_sent(rank0[B:]) and is_sent(dq[B:]), \
        tag + ': wrote past its rows'
    if ws is not None:
        tiles, splits, _ = splitk_plan(B, D, K)
        assert bool((ws[splits * tiles * 1024:ws_bytes // 4].view(torch.int32) == 0).all()), \
            tag + ': ticket words not zero after the launch'
        assert bool(torch.isnan(ws[ws_bytes // 4:]).all()), tag + ': wrote past the workspace'
    ref = infonce_ref(q, k, queue, f32(inv_T))
    if exact:
        assert_exact_sum(q, queue.t().contiguous(), inv_T)
        same_bits(logits[:B], ref['logits'], tag + ' logits')
        assert torch.equal(rank0[:B].long(), ref['rank']), tag + ': rank0'
        b = torch.zeros_like(ref['logits'])
    else:
        b = torch.cat([((ceil_div(D, 256) + 10 + 2) * U * f32(inv_T) * (q * k).abs().sum(1))[:, None],
                       gemm_bound(q, queue.t().contiguous(), inv_T, gemm_chain(B, K, D))], 1)
        within(logits[:B], ref['logits'], b, f'infonce.logits {tag}')
        bb = b[:, 1:] + b[:, :1]
        diff = ref['logits'][:, 1:] - ref['logits'][:, :1]
        got = rank0[:B].long()
        assert bool(((got >= (diff > bb).sum(1)) & (got <= (diff >= -bb).sum(1))).all()), tag + ': rank0 outside its interval'
    mx = ref['logits'].max(1).values
    x = ref['logits'] - mx[:, None]
    b_lse = b.max(1).values + (ceil_div(K, 256) + 11 + 1) * U + (ref['p'] * (e_exp(x) + U * x.abs())).sum(1) \
        + E_LOG * (ref['lse'] - mx).abs() + U * ref['lse'].abs()
    within(loss[:B], ref['loss'], b_lse + b[:, 0] + U * ref['loss'].abs(), f'infonce.loss_rows {tag}')
    xl = ref['logits'] - ref['lse'][:, None]
    b_dl = ref['g'] * (ref['p'] * (e_exp(xl) + b + b_lse[:, None] + U * xl.abs()) + TINY) + 2 * U * ref['dl'].abs()
    b_dl[:, 0] += ref['g'] * U * (ref['p'][:, 0] - 1).abs()
    within(dlog[:B], ref['dl'], b_dl, f'infonce.dlogits {tag}')
    dl = dlog[:B].double()
    b_dq = (gemm_chain(B, D, K) + 2) * U * (dl[:, 1:].abs() @ queue.abs().t()) + b_dl[:, 1:] @ queue.abs().t() + b_dl[:, :1] * k.abs() \
        + U * (dl[:, :1] * k).abs() + U * ref['dq'].abs()
    within(dq[:B], ref['dq'], b_dq, f'infonce.dq {tag} {gemm_form(B, D, K)}-{form}')
    return dict(logits=logits, dlog=dlog, dq=dq, loss=loss, rank0=rank0, ref=ref)


@pytest.mark.parametrize('case', INFONCE_CASES, ids=['B%d-D%d-K%d' % c for c in INFONCE_CASES])
def test_infonce_grid_exact(gpu, case):
    B, D, K = case
    gen = torch.Generator().manual_seed(B + K)
    q, k, queue = grid(gen, (B, D), gpu), grid(gen, (B, D), gpu), grid(gen, (D, K), gpu)
    run_infonce(gpu, q, k, queue, 2.0 if D >= 100 else 4.0, True, 'grid B%d-D%d-K%d' % case, 'ordered')


SPLIT_CASES = [c for c in INFONCE_CASES if c[2] >= 4096]


@pytest.mark.parametrize('case', SPLIT_CASES, ids=['B%d-D%d-K%d' % c for c in SPLIT_CASES])
def test_infonce_ordered_splitk_exact_onehot(gpu, case):
    """Data on which dq itself is exact: every query equals one queue column (logit 4 D, the rest at least 200 lower), so
    every other softmax weight underflows to 0 and that one is exactly 1: dlogits = g * (onehot(jmax) - onehot(0)), dq = g *
    (queue[:, jmax] - k).  jmax of row b is the last column of split-K slice b % splits (the ragged one included).  dq is bit
    for bit float64 in the ordered and in the atomic form, the two equal each other, two ordered launches give the same bits."""
    B, D, K = case
    gen = torch.Generator().manual_seed(B)
    tiles, splits, kslice = splitk_plan(B, D, K)
    q = (torch.randint(0, 2, (B, D), generator=gen).double() - 0.5)[torch.arange(B) % splits].to(gpu)   # equal where jmax is
    k = grid(gen, (B, D), gpu, 0.25).sign() / 2            # 0, +-1/2: g * (queue - k) stays one rounding-free product
    queue = grid(gen, (D, K), gpu, 0.25)
    jmax = torch.tensor([min(K, (b % splits + 1) * kslice) - 1 for b in range(B)], device=gpu)
    queue[:, jmax] = q.t()
    inv_T = 16.0
    lg = infonce_ref(q, k, queue, inv_T)['logits']
    rest = lg.clone()
    rest[torch.arange(B), jmax + 1] = -1e9
    assert bool((lg[torch.arange(B), jmax + 1] == 4 * D).all()) and float(rest.max()) <= 4 * D - 200
    g = f32(np.float32(inv_T) / np.float32(B))
    want = g * (queue[:, jmax].t() - k)
    outs = {}
    for form in ('ordered', 'none', 'ordered'):
        o = run_infonce(gpu, q, k, queue, inv_T, True, f'onehot B{B}-D{D}-K{K}', form)
        same_bits(o['dq'][:B], want, f'dq {form}')
        dl = torch.zeros((B, K + 1), dtype=F64, device=gpu)
        dl[torch.arange(B), jmax + 1] = g
        dl[:, 0] = -g
        same_bits(o['dlog'][:B], dl, f'dlogits {form}')
        outs.setdefault(form, []).append(o['dq'].clone())
    assert torch.equal(outs['ordered'][0].view(torch.int32), outs['ordered'][1].view(torch.int32))
    assert torch.equal(outs['ordered'][0].view(torch.int32), outs['none'][0].view(torch.int32))


@pytest.mark.parametrize('T', [0.07, 0.5])
@pytest.mark.parametrize('case', INFONCE_CASES, ids=['B%d-D%d-K%d' % c for c in INFONCE_CASES])
def test_infonce_gaussian_bounds(gpu, case, T):
    B, D, K = case
    gen = torch.Generator().manual_seed(B * 7 + K)
    nrm = torch.nn.functional.normalize
    a = torch.randn((B, D), generator=gen, dtype=F64)
    q = nrm(0.12 * a + torch.randn((B, D), generator=gen, dtype=F64), dim=1).to(gpu)
    k = nrm(0.12 * a + torch.randn((B, D), generator=gen, dtype=F64), dim=1).to(gpu)
    queue = nrm(torch.randn((D, K), generator=gen, dtype=F64), dim=0).to(gpu)
    tag = f'T={T} B{B}-D{D}-K{K}'
    o1 = run_infonce(gpu, q, k, queue, 1.0 / T, False, tag, 'ordered')
    o2 = run_infonce(gpu, q, k, queue, 1.0 / T, False, tag, 'ordered')
    assert torch.equal(o1['dq'].view(torch.int32), o2['dq'].view(torch.int32)), 'two ordered launches differ'
    if K >= 4096:
        run_infonce(gpu, q, k, queue, 1.0 / T, False, tag, 'none')       # the atomic form: to the bound only


# ----------------------------------------------------------------------------------------------------------- rank margin
def rank_margin_ref(f, s, theta, clip, weight):
    """feats [Bn][2s][D]; row i's highest is its pair (i + s) % 2s, the others j != i, pair in index order.  Returns logits
    [Bn][2s][2s-1], z [Bn][2s][2s-2], loss = weight * mean softplus(min(z, clip)), dfeats"""
    Bn, n2, D = f.shape
    S = f @ f.transpose(1, 2)
    i = torch.arange(n2, device=f.device)
    pr = (i + s) % n2
    oth = torch.stack([torch.tensor([j for j in range(n2) if j != a and j != (a + s) % n2], device=f.device) for a in range(n2)])
    hi = S[:, i, pr]
    lo = torch.gather(S, 2, oth[None].expand(Bn, -1, -1))
    z = (lo - hi[:, :, None]) / theta
    zc = z.clamp_max(clip) if clip > 0 else z
    count = Bn * n2 * (n2 - 2)
    return dict(S=S, oth=oth, pr=pr, hi=hi, lo=lo, z=z, zc=zc, count=count, logits=torch.cat([hi[:, :, None], lo], 2),
                loss=weight * torch.nn.functional.softplus(zc, threshold=1e9).sum() / count)


def run_rank_margin(dev, f64, s, theta, clip, weight, tag):
    Bn, n2, D = f64.shape
    f32t = f64.float().contiguous()
    f = f32t.double().requires_grad_(True)
    th, cl, w = f32(theta), f32(clip), f32(weight)
    logits, loss, df, scratch = sent((Bn * n2 + 1, n2 - 1), dev), sent((8,), dev), sent((Bn * n2 + 1, D), dev), sent((Bn + 8,), dev)
    ops.call('dv_rank_margin', f32t, Bn, s, D, theta, clip, weight, logits, loss, df, scratch)
    torch.cuda.synchronize()
    assert is_sent(logits[Bn * n2:]) and is_sent(loss[1:]) and is_sent(df[Bn * n2:]) and is_sent(scratch[Bn:]), \
        tag + ': wrote past its range'
    ref = rank_margin_ref(f, s, th, cl, w)
    ref['loss'].backward()
    fd, fa = f.detach(), f.detach().abs()
    bS = (D + 1) * U * (fa @ fa.transpose(1, 2))
    z, zc = ref['z'].detach(), ref['zc'].detach()
    i = torch.arange(n2, device=dev)
    b_hi = bS[:, i, ref['pr']]
    b_lo = torch.gather(bS, 2, ref['oth'][None].expand(Bn, -1, -1))
    within(logits[:Bn * n2].view(Bn, n2, n2 - 1), ref['logits'].detach(), torch.cat([b_hi[:, :, None], b_lo], 2), f'margin.logits {tag}')
    bz = (b_lo + b_hi[:, :, None]) / th + 2 * U * z.abs()
    if clip > 0:
        n_hi, n_lo = int((z > cl).sum()), int((z <= cl).sum())
        print(f'    {tag}: {n_hi} pairs above the clip, {n_lo} below')
        assert n_hi > 0 and n_lo > 0 and bool(((z - cl).abs() > bz).all()), 'test data: a pair sits on the clip'
    sp = torch.nn.functional.softplus(zc, threshold=1e9)
    sg = torch.sigmoid(zc)
    b_term = bz + (e_exp(zc) * sg + E_LOG1P) * sp
    scale = w / ref['count']
    b_loss = scale * b_term.sum() + (n2 + 8 + ceil_div(Bn, 256) + 11) * U * float(ref['loss'].detach().abs())
    within(loss[:1], ref['loss'].detach().view(1), b_loss.view(1), f'margin.loss {tag}')
    # gradient: dz = weight / count * sigmoid * pass / theta into dS[i][j] and -dS[i][pair]
    passed = (z <= cl).double() if clip > 0 else torch.ones_like(z)
    dz = scale * sg * passed / th
    b_dz = passed * scale / th * (sg * (1 - sg) * bz + sg * (e_exp(zc) + 2 * U)) + 3 * U * dz
    dS, bdS = torch.zeros((Bn, n2, n2), dtype=F64, device=dev), torch.zeros((Bn, n2, n2), dtype=F64, device=dev)
    idx = ref['oth'][None].expand(Bn, -1, -1)
    dS.scatter_(2, idx, dz)
    bdS.scatter_(2, idx, b_dz + U * dz)
    dS[:, i, ref['pr']] = -dz.sum(2)
    bdS[:, i, ref['pr']] = b_dz.sum(2) + (n2 - 2) * U * dz.sum(2)
    sym, bsym = dS + dS.transpose(1, 2), bdS + bdS.transpose(1, 2) + U * (dS.abs() + dS.transpose(1, 2).abs())
    within(df[:Bn * n2].view(Bn, n2, D), f.grad, bsym @ fa + (n2 + 2) * U * (sym.abs() @ fa), f'margin.dfeats {tag}')
    assert bool(((sym @ fd) - f.grad).abs().max() <= 1e-12 * (1 + f.grad.abs().max())), \
        'the hand-written gradient disagrees with autograd'


@pytest.mark.parametrize('clip', [0.0, 5.0])
@pytest.mark.parametrize('Bn', [1, 6, 64])
@pytest.mark.parametrize('s', [2, 3, 4, 8])
def test_rank_margin_grid_exact(gpu, s, Bn, clip):
    gen = torch.Generator().manual_seed(s * 100 + Bn)
    f = grid(gen, (Bn, 2 * s, 32), gpu)
    # theta = 1/4: z = 4 (lo - hi) reaches about +-15, so both sides of clip = 5 occur
    run_rank_margin_exact(gpu, f, s, clip)


def run_rank_margin_exact(dev, f, s, clip):
    Bn, n2, D = f.shape
    ref = rank_margin_ref(f, s, 0.25, clip, 1.0)
    logits, loss, df, scratch = sent((Bn * n2 + 1, n2 - 1), dev), sent((8,), dev), sent((Bn * n2 + 1, D), dev), sent((Bn + 8,), dev)
    f32t = f.float().contiguous()
    ops.call('dv_rank_margin', f32t, Bn, s, D, 0.25, clip, 1.0, logits, loss, df, scratch)
    assert float((f.abs() @ f.abs().transpose(1, 2)).max()) * 16 < 2 ** 24
    same_bits(logits[:Bn * n2].view(Bn, n2, n2 - 1), ref['logits'], f'margin grid s={s} Bn={Bn} logits')
    assert is_sent(logits[Bn * n2:]) and is_sent(loss[1:]) and is_sent(df[Bn * n2:]) and is_sent(scratch[Bn:])
    # loss with exact z: the softplus terms alone
    zc = ref['zc']
    sp = torch.nn.functional.softplus(zc, threshold=1e9)
    b_loss = ((e_exp(zc) * torch.sigmoid(zc) + E_LOG1P) * sp).sum() / ref['count'] \
        + (n2 + 8 + ceil_div(Bn, 256) + 11) * U * ref['loss'].abs()
    within(loss[:1], ref['loss'].view(1), b_loss.view(1), f'margin.loss grid s={s} Bn={Bn} clip={clip}')
    if clip > 0 and Bn > 1:
        assert bool((ref['z'] > clip).any()) and bool((ref['z'] < clip).any())


@pytest.mark.parametrize('clip', [0.0, 5.0])
@pytest.mark.parametrize('s', [2, 3, 4, 5, 6, 7, 8])
def test_rank_margin_gaussian_bounds(gpu, s, clip):
    gen = torch.Generator().manual_seed(s)
    Bn, D = 8, 64           # cosines spread by about 1/8: z = (lo - hi) / 0.05 by about 3.5, so some pairs pass the clip of 5
    base = torch.randn((Bn, 1, D), generator=gen, dtype=F64)
    f = torch.nn.functional.normalize(0.3 * base + torch.randn((Bn, 2 * s, D), generator=gen, dtype=F64), dim=2).to(gpu)
    run_rank_margin(gpu, f, s, 0.05, clip, 0.5, f's={s} clip={clip}')


# ------------------------------------------------------------------------------------- softmax CE, softmax rows, kNN rank
ROWS, CLASSES = [1, 5, 130], [1, 2, 63, 64, 65, 101, 400, 1000]


@pytest.mark.parametrize('K', CLASSES)
@pytest.mark.parametrize('R', ROWS)
def test_softmax_ce_and_rows(gpu, R, K):
    gen = torch.Generator().manual_seed(R * 1000 + K)
    ld = K + 3
    lg = torch.full((R, ld), float('nan'), dtype=torch.float32, device=gpu)
    lg[:, :K] = (torch.randn((R, K), generator=gen) * 4).to(gpu)
    labels = torch.randint(0, K, (R,), generator=gen, dtype=torch.int32).to(gpu)
    x64 = lg[:, :K].double()
    lse = torch.logsumexp(x64, 1)
    ly = x64[torch.arange(R), labels.long()]
    mx = x64.max(1).values
    p = torch.exp(x64 - lse[:, None])
    xm = x64 - mx[:, None]
    b_lse = (ceil_div(K, 64) + 6 + 1) * U + (p * (e_exp(xm) + U * xm.abs())).sum(1) + E_LOG * (lse - mx).abs() + U * lse.abs()
    onehot = torch.nn.functional.one_hot(labels.long(), K).double()
    gs = f32(np.float32(1.0) / np.float32(R))
    xl = x64 - lse[:, None]
    b_dl = gs * (p * (e_exp(xl) + b_lse[:, None] + U * xl.abs()) + U * (p - onehot).abs() + TINY) + U * (gs * (p - onehot)).abs()
    for with_grad in (True, False):
        loss, rank0 = sent((R + 8,), gpu), sent((R + 8,), gpu, torch.int32)
        dl = sent((R + 1, K + 2), gpu)
        ops.call('dv_softmax_ce_fwd', lg, ld, R, K, labels, loss, dl if with_grad else None, K + 2, rank0)
        within(loss[:R], lse - ly, b_lse + U * (lse - ly).abs(), f'softmax_ce.loss R={R} K={K}', quiet=True)
        assert torch.equal(rank0[:R].long(), (x64 > ly[:, None]).sum(1)) and is_sent(loss[R:]) and is_sent(rank0[R:])
        if with_grad:
            within(dl[:R, :K], gs * (p - onehot), b_dl, f'softmax_ce.dlogits R={R} K={K}', quiet=True)
            assert is_sent(dl[:R, K:]) and is_sent(dl[R:])
        else:
            assert is_sent(dl), 'dlogits = NULL but something was written'
    # softmax rows: expf(x - max) / sum: expf, the sum's chain, the reciprocal, the product
    probs = sent((R + 1, K + 5), gpu)
    ops.call('dv_softmax_rows_f32', lg, ld, R, K, probs, K + 5)
    pm = torch.softmax(x64, 1)
    within(probs[:R, :K], pm, pm * ((ceil_div(K, 64) + 6 + 2) * U + 2 * (E_EXPF + U * xm.abs()).max(1).values[:, None] + U * xm.abs()),
           f'softmax_rows R={R} K={K}', quiet=True)
    assert is_sent(probs[:R, K:]) and is_sent(probs[R:])


@pytest.mark.parametrize('Nt', [1, 63, 64, 65, 400, 1000])
@pytest.mark.parametrize('R', ROWS)
def test_knn_rank_exact_with_ties(gpu, R, Nt):
    """grid similarities (multiples of 1/4 in [-2, 2]: nearly every row has train samples tying its best same-label one),
    labels from 0..5 with label 5 absent from the train set: rank = #{sim > best same-label} strictly, Nt if the label is absent"""
    gen = torch.Generator().manual_seed(R + Nt)
    ld = Nt + 2
    sim = torch.full((R, ld), float('nan'), dtype=torch.float32, device=gpu)
    sim[:, :Nt] = (torch.randint(-8, 9, (R, Nt), generator=gen).float() / 4).to(gpu)
    trl = torch.randint(0, 5, (Nt,), generator=gen, dtype=torch.int32).to(gpu)
    tel = torch.randint(0, 6, (R,), generator=gen, dtype=torch.int32).to(gpu)
    rank = sent((R + 8,), gpu, torch.int32)
    ops.call('dv_knn_rank', sim, ld, R, Nt, trl, tel, rank)
    s = sim[:, :Nt].double()
    same = trl[None, :] == tel[:, None]
    best = torch.where(same, s, torch.full_like(s, -math.inf)).max(1).values
    want = torch.where(same.any(1), (s > best[:, None]).sum(1), torch.full((R,), Nt, device=gpu))
    assert torch.equal(rank[:R].long(), want) and is_sent(rank[R:])
    if Nt >= 400 and R >= 5:
        assert bool((same.any(1) & ((s == best[:, None]) & ~same).any(1)).any()), 'no tie in the test data'


# ----------------------------------------------------------------------------------- group mean, mean, column sums
@pytest.mark.parametrize('G', [1, 2, 3, 8])
def test_group_mean_fwd_bwd(gpu, G):
    gen = torch.Generator().manual_seed(G)
    for R, D in ((1, 1), (5, 100), (130, 128)):
        x = torch.randn((R, G, D), generator=gen).to(gpu)
        y, dx = sent((R * D + 8,), gpu), sent((R * G * D + 8,), gpu)
        ops.call('dv_group_mean_f32', x, R, G, D, y)
        x64 = x.double()
        within(y[:R * D].view(R, D), x64.mean(1), (G + 1) * U * x64.abs().sum(1) / G, f'group_mean G={G}', quiet=True)
        dy = torch.randn((R, D), generator=gen).to(gpu)
        ops.call('dv_group_mean_bwd_f32', dy, R, G, D, dx)
        want = (dy.double() / G)[:, None, :].expand(R, G, D)
        within(dx[:R * G * D].view(R, G, D), want, U * want.abs(), f'group_mean_bwd G={G}', quiet=True)
        assert is_sent(y[R * D:]) and is_sent(dx[R * G * D:])
        # exact data: integers, G a power of two -> bit for bit
        if G in (1, 2, 8):
            xi = torch.randint(-8, 9, (R, G, D), generator=gen).float().to(gpu)
            ops.call('dv_group_mean_f32', xi, R, G, D, y)
            same_bits(y[:R * D].view(R, D), xi.double().mean(1), f'group_mean exact G={G}')


@pytest.mark.parametrize('n', [1, 63, 256, 257, 1000, 4096 + 5])
def test_mean_f32(gpu, n):
    gen = torch.Generator().manual_seed(n)
    x = torch.full((n + 4,), float('nan'), dtype=torch.float32, device=gpu)
    x[:n] = (torch.randn((n,), generator=gen) + 3).to(gpu)
    out = sent((8,), gpu)
    ops.call('dv_mean_f32', x, n, out)
    x64 = x[:n].double()
    within(out[:1], x64.mean().view(1), ((ceil_div(n, 256) + 6 + 4 + 1) * U * x64.abs().sum() / n).view(1), f'mean n={n}', quiet=True)
    assert is_sent(out[1:])
    xi = torch.randint(-8, 9, (n,), generator=gen).float().to(gpu)
    ops.call('dv_mean_f32', xi, n, out)
    within(out[:1], xi.double().mean().view(1), (U * xi.double().mean().abs()).view(1), f'mean exact-sum n={n}', quiet=True)


@pytest.mark.parametrize('R', [1, 7, 8, 9, 31, 32, 33, 130, 1000])
def test_colsum_f32(gpu, R):
    """out[c] += sum_r x[r][c]: four accumulators per thread over rows r, r + 8, r + 16, r + 24 (+32 per trip), their pairwise
    sum, eight row groups in a row, the add into out"""
    gen = torch.Generator().manual_seed(R)
    for Cc in (1, 31, 32, 33, 100):
        ld = Cc + 3
        x = torch.full((R, ld), float('nan'), dtype=torch.float32, device=gpu)
        xi = torch.randint(-8, 9, (R, Cc), generator=gen).float().to(gpu)
        out0 = torch.randint(-8, 9, (Cc,), generator=gen).float().to(gpu)
        x[:, :Cc] = xi
        out = sent((Cc + 8,), gpu)
        out[:Cc] = out0
        ops.call('dv_colsum_f32', x, ld, R, Cc, out)
        same_bits(out[:Cc], out0.double() + xi.double().sum(0), f'colsum exact R={R} C={Cc}')
        assert is_sent(out[Cc:])
        xg = torch.randn((R, Cc), generator=gen).to(gpu)
        x[:, :Cc] = xg
        out[:Cc] = out0
        ops.call('dv_colsum_f32', x, ld, R, Cc, out)
        ref = out0.double() + xg.double().sum(0)
        within(out[:Cc], ref, (ceil_div(R, 32) + 2 + 8 + 1) * U * (out0.double().abs() + xg.double().abs().sum(0)), f'colsum R={R}',
               quiet=True)


# ------------------------------------------------------------------------------------------------ SGD, EMA, arena cast
NS = [1, 3, 4, 5, 1003, 2 ** 20 + 3, 2 ** 21 + 4099]       # the last: 2048 blocks x 256 threads x 4 elements, then a second trip


def assert_f32(t, what):
    assert bool((t.float().double() == t).all()), f'{what} is not exact in fp32 (test data)'


def sgd_ref(p, g, buf, lr, mu, wd, gs, exact):
    d = g * gs + wd * p
    nb = mu * buf + d
    lb = lr * nb
    npar = p - lb
    if exact:
        for name, t in (('g*gs', g * gs), ('wd*p', wd * p), ('d', d), ('mu*buf', mu * buf), ('buf', nb), ('lr*buf', lb), ('p', npar)):
            assert_f32(t, name)
    return npar, nb


COPY_CASES = [(n, c) for n in NS for c in ('bf16', 'f32', 'none')] + [(n, 'bf16-odd') for n in (5, 1003)]


@pytest.mark.parametrize('n,copy', COPY_CASES)
def test_sgd_exact(gpu, n, copy):
    """lr 2^-8, mu 1/2, wd 2^-10, grad_scale 1/4, integer p, g, buf: one step with weight decay, three without, bit for bit"""
    gen = torch.Generator().manual_seed(n)
    for wd, steps in ((2.0 ** -10, 1), (0.0, 3)):
        ri = lambda: torch.randint(-8, 9, (n,), generator=gen).double().to(gpu)  # noqa: E731
        p64, b64 = ri(), ri()
        p, buf = arena(p64), arena(b64)
        dt, code, whole, cp = copy_buffer(n, copy, gpu)
        for step in range(steps):
            g64 = ri()
            g = arena(g64)
            ops.call('dv_sgd_momentum', p, g, buf, n, 2.0 ** -8, 0.5, wd, 0.25, code, cp if dt is not None else None)
            p64, b64 = sgd_ref(p64, g64, b64, 2.0 ** -8, 0.5, wd, 0.25, True)
            same_bits(p[:n], p64, f'sgd p n={n} wd={wd} step {step}')
            same_bits(buf[:n], b64, f'sgd buf n={n} wd={wd} step {step}')
            assert is_sent(p[n:]) and is_sent(buf[n:]) and is_sent(g[n:])
            check_copy(cp, p, n, dt, f'sgd n={n} {copy}')
            assert is_sent(whole[:whole.numel() - cp.numel()]), f'sgd n={n} {copy}: copy written in front of its start'


TIE_BITS = [0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0x3f817fff, 0x3f818001, 0xbf808000, 0xbf818000, 0x00008000, 0x00018000,
            0x7f7e8000, 0x3fffffff, 0x3fff8000, 0x80008000, 0x3f800000, 0x00000000]


def tie_values(n, gen, dev):
    """Gaussian values with every 5th replaced by a value exactly half-way between two bf16 numbers or one unit off it"""
    v = torch.randn((n,), generator=gen)
    t = torch.tensor(np.array(TIE_BITS, dtype=np.uint32).view(np.float32))
    idx = torch.arange(0, n, 5)
    v[idx] = t[torch.arange(idx.numel()) % len(TIE_BITS)]
    return v.to(dev)


@pytest.mark.parametrize('n', [1, 5, 1003, 2 ** 20 + 3])
def test_bf16_copies_round_to_nearest_even(gpu, n):
    """dv_cast_arena, dv_sgd_momentum (lr = 0: p unchanged) and dv_ema (m = 1) on Gaussian values and exact rounding ties; then
    one ordinary Gaussian SGD step and EMA: the copy is the cast of the NEW fp32 value"""
    gen = torch.Generator().manual_seed(n)
    v = tie_values(n, gen, gpu)
    src = arena(v.double())
    for code, dt in ((DV_BF16, torch.bfloat16), (DV_F32, torch.float32)):
        dst = sent((n + 8,), gpu, dt)
        ops.call('dv_cast_arena', code, src, dst, n)
        check_copy(dst, src, n, dt, f'cast_arena n={n}')
        assert torch.equal(src[:n].view(torch.int32), v.view(torch.int32)) and is_sent(src[n:])
        p, g = arena(v.double()), arena(torch.randn((n,), generator=gen).double().to(gpu))
        buf, cp = arena(torch.zeros(n, dtype=F64, device=gpu)), sent((n + 8,), gpu, dt)
        ops.call('dv_sgd_momentum', p, g, buf, n, 0.0, 0.9, 0.0, 1.0, code, cp)
        assert torch.equal(p[:n], v)
        check_copy(cp, p, n, dt, f'sgd lr=0 n={n}')
        ops.call('dv_sgd_momentum', p, g, buf, n, 0.003, 0.9, 1e-4, 1.0, code, cp)
        check_copy(cp, p, n, dt, f'sgd gaussian n={n}')
        k, q, cp = arena(v.double()), arena(torch.randn((n,), generator=gen).double().to(gpu)), sent((n + 8,), gpu, dt)
        ops.call('dv_ema', k, q, n, 1.0, code, cp)
        assert torch.equal(k[:n], v)
        check_copy(cp, k, n, dt, f'ema m=1 n={n}')
        ops.call('dv_ema', k, q, n, 0.999, code, cp)
        check_copy(cp, k, n, dt, f'ema gaussian n={n}')
        assert is_sent(k[n:]) and is_sent(p[n:]) and is_sent(buf[n:])


@pytest.mark.parametrize('m', [0.5, 0.75])
@pytest.mark.parametrize('n', NS[:-1])
def test_ema_exact(gpu, n, m):
    gen = torch.Generator().manual_seed(n + 1)
    k64 = torch.randint(-8, 9, (n,), generator=gen).double().to(gpu)
    k = arena(k64)
    for code, dt in ((DV_BF16, torch.bfloat16), (DV_F32, torch.float32), (DV_F32, None)):
        cp = sent((n + 8,), gpu, dt or torch.float32)
        for step in range(3):
            q64 = torch.randint(-8, 9, (n,), generator=gen).double().to(gpu)
            ops.call('dv_ema', k, arena(q64), n, m, code, cp if dt is not None else None)
            k64 = k64 * m + q64 * (1 - m)
            same_bits(k[:n], k64, f'ema n={n} m={m} step {step}')
            check_copy(cp, k, n, dt, f'ema n={n}')
            assert is_sent(k[n:])
        k64 = torch.round(k64)          # back to integers: the dyadic unit must not shrink over the nine steps
        k[:n] = k64.float()


@pytest.mark.parametrize('gs', [1.0, 1.0 / 128])
@pytest.mark.parametrize('n', [5, 1003, 2 ** 20 + 3])
def test_sgd_gaussian_three_steps(gpu, n, gs):
    gen = torch.Generator().manual_seed(n)
    lr, mu, wd, gsf = f32(0.003), f32(0.9), f32(1e-4), f32(gs)
    p32 = (torch.randn((n,), generator=gen) * 0.05).to(gpu)
    p, buf = arena(p32.double()), arena(torch.zeros(n, dtype=F64, device=gpu))
    p64, b64 = p32.double(), torch.zeros(n, dtype=F64, device=gpu)
    bp, bb = torch.zeros_like(p64), torch.zeros_like(p64)
    for step in range(3):
        g32 = (torch.randn((n,), generator=gen) * 0.01 / gs).to(gpu)
        g64 = g32.double()
        ops.call('dv_sgd_momentum', p, arena(g64), buf, n, 0.003, 0.9, 1e-4, gs, DV_F32, None)
        d = g64 * gsf + wd * p64
        bd = U * ((g64 * gsf).abs() + (wd * p64).abs() + d.abs()) + wd * bp
        nb = mu * b64 + d
        bb = mu * bb + U * (mu * b64).abs() + bd + U * nb.abs()
        npar = p64 - lr * nb
        bp = bp + lr * bb + U * (lr * nb).abs() + U * npar.abs()
        p64, b64 = npar, nb
        within(p[:n], p64, bp, f'sgd.p step {step} n={n} gs={gs:g}', quiet=step < 2)
        within(buf[:n], b64, bb, f'sgd.buf step {step} n={n} gs={gs:g}', quiet=step < 2)
    rel = (p[:n].double() - p64).abs() / p64.abs().clamp_min(1e-30)
    print(f'    sgd n={n} gs={gs:g}: after 3 steps |p_fp32 - p_float64| / |p|: median {float(rel.median()):.2e}, '
          f'max |p_fp32 - p_float64| {float((p[:n].double() - p64).abs().max()):.2e}')


# ------------------------------------------------------------------------------------------- the device-function figures
def test_device_function_figures(gpu):
    """What E_EXP rests on, re-measured through the ABI where an entry isolates the function:
      __expf(x), x <= 0: dv_softmax_ce_fwd on rows [0, t] with the label on the 0 returns lse as loss_rows (lse - 0 is exact) and
                 dlogits[r][1] = __expf(fl(t - lse)) / R, R a power of two: argument and value are both observable.
      __expf(x), x > 0 and the reciprocal: DV_SIGMOID on a K = 1 product, 1 / (1 + __expf(-v)): two more roundings (<= 2u).
    Both must stay under HALF of E_EXP (the figure is a measurement taken with a factor 2)."""
    R = 4096                                        # gs = 1 / R is a power of two: the product with it is exact
    lg = torch.zeros((R, 2), dtype=torch.float32, device=gpu)
    lg[:, 1] = torch.linspace(-80.0, 12.0, R, device=gpu)
    labels = torch.zeros((R,), dtype=torch.int32, device=gpu)
    loss, dl = sent((R,), gpu), sent((R, 2), gpu)
    ops.call('dv_softmax_ce_fwd', lg, 2, R, 2, labels, loss, dl, 2, None)
    arg = (lg[:, 1] - loss).double()                # fl32(logit - lse), as the kernel forms it
    got = dl[:, 1].double() * R
    rel = (got - torch.exp(arg)).abs() / torch.exp(arg)
    r1 = float((rel / e_exp(arg)).max())
    v = torch.linspace(-40.0, 0.0, 2048, device=gpu)
    a = torch.ones((1, 1), dtype=torch.float32, device=gpu)
    out = sent((1, 2048), gpu)
    d = L.GemmDesc()
    d.A, d.B, d.C, d.bias = a.data_ptr(), v.data_ptr(), out.data_ptr(), None
    d.sam, d.sak, d.sbk, d.sbn, d.ldc = 1, 1, 1, 1, 2048
    d.M, d.N, d.K, d.flags, d.tile_end, d.alpha = 1, 2048, 1, DV_SIGMOID, 0, 1.0
    ops.call('dv_gemm_f32_ex', d)
    v64 = v.double()
    sg = torch.sigmoid(v64)
    rel2 = ((out[0].double() - sg).abs() / sg - 2 * U).clamp_min(0)
    r2 = float((rel2 / (e_exp(v64) * (1 - sg))).max())
    print(f'    __expf: measured / E_EXP  {r1:.3f} (x <= 0), {r2:.3f} (x > 0, through the sigmoid)')
    assert r1 <= 0.5 and r2 <= 0.5
