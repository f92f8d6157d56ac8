"""The convolution kernels (csrc/conv_gemm.hpp, conv_wgrad.hip, conv_tap.hip, conv_tap_wgrad.hip; host layer csrc/conv.hip) against a float64 reference, on the route
each row of tests/conv_cases.py names.  Every entry is called through the C ABI / dualvar_amd.ops on explicit tensors.

Reference: a plain float64 convolution (`ref_fwd`, `ref_dgrad`, `ref_wgrad` of tests/conv_reference.py): a loop over the kernel taps, each
a shifted, zero-padded, strided slice of the NDHWC input times the [Cin, Cout] weight slice, summed in float64 on the GPU by
torch; the same loop over |x|, |w| gives S = sum|terms| per element and over ones the number of terms `cnt`.  Three small
cases check it against torch.nn.functional.conv3d / autograd in float64 on the CPU.  It never calls the library under test.

Frames: every input lives in a buffer of NaN (rows behind the tensor, lanes outside the view) with zeros in its pad lanes
[C, cpitch); every output in a buffer of a NaN sentinel pattern, of which only the view's lanes [0, cp8(C)) of rows < M may
change, the pad lanes [C, cp8(C)) to zero.  Small rows run as channel slices at offset 8 of a wider buffer (ld > cpitch).

(A) EXACT DATA: bit equality with float64 (`same_bits`: int32 views after + 0.0).  The host asserts from the reference alone
    that S of every element is below 2^24 units of the data's dyadic unit, so every partial sum of every summation order is an
    fp32 number; a case that fails this is a test-data error.
    G1  integers in [-2, 2] / 4 in both operands, dense (unit 1/16): gathers, taps, padding, strides, parity classes, tile and
        split boundaries, trimmed windows, the K-split fold, the slab reduce.  8-bit data: only the hi*hi product is non-zero.
    G2  both operands +-(a 2^8 + b), a in {1,2,3}, b in {1,3} (unit 1): hi is the value rounded to 8 bits, mid the rest; the
        host split (`planes`) asserts mid != 0 and lo == 0 for EVERY value under the rounding split3 and the truncating split3w.
        The four partial products hh, hm, mh, mm are all among the six kept ones, so the result is exact and each of those
        MFMAs is pinned.  A product is < 2^19.2, the second operand is sparse (at most 24 non-zeros per output element).
    G3  operand A with all three planes populated (24-bit integers 2^23 <= |v| < 2^24, scaled 2^-20; asserted: mid != 0 and
        lo != 0 in at least half of them) against operand P = signed powers of two, ONE non-zero term per output element
        (asserted with the `cnt` loop over the non-zero masks): pins hi*lo / lo*hi in the in-kernel splits and the planes of
        dv_pack_w3.  Run with A = activations, P = weights and with the roles swapped.  With one term the result is the
        product itself: an identity / shift convolution returns its fp32 input bit for bit.
    DV_BF16: G1 with integers in [-8, 8] / 4 (sums of the [-2, 2] grid never reach 9 significant bits at these K) and the
        expected output = round-to-nearest-even bf16 of the exact sum; ties are asserted to occur.
    DV_ACCUM / `dw +=`: the old contents are G1 data and count into S.
(B) GAUSSIAN DATA at the table's shapes (x post-ReLU Gaussian, w Gaussian * fan_in^-1/2, dy Gaussian): every element inside
      b = gamma(n_add - 1 + c) (1 + 2^-7) S + d S,        gamma(n) = n u / (1 - n u),  u = 2^-24
    split mode: n_add = 6 cnt (six partial products per term, each counted as one sequential fp32 addition: an upper bound
    for any order inside and between the MFMAs; exact zeros of padding add nothing), c = the additions that follow: 3 for the
    4-wave fold of conv_gemm_ks, `splits` slab additions of wgrad_reduce_kernel, 1 for `+=` into dw.  (1 + 2^-7) >= the sum of
    the six |partial products| over |x w| ((1 + 2^-8)^2: |hi| <= (1 + 2^-8)|v|).  d = the three dropped products: |mid| <=
    2^-8 |v| (2^-9 rounded), |lo| <= 2^-17 |v| -> mid*lo + lo*mid + lo*lo <= 2^-24 |x w| for split3; the truncated mid of
    split3w (weight gradients) leaves |lo| <= 2^-16 |v|: d = 2^-23.
    DV_BF16: products of two bf16 are exact, n_add = cnt, d = 0, plus half a bf16 ulp of the result for activations
    (8 significant bits: half an ulp is at most 2^-8 of the value): 2^-8 (|ref| + b).
    Every (B) case also prints rms(err) / (u rms(ref)) for the kernel and, on the smaller shapes, for torch's fp32 CPU conv on
    the same data, and asserts kernel <= 4 x torch (the project's factor of test_fp32_conv_at_headline_tile_sizes_against_
    cpu_conv3d, moved from the maximum to the rms).
DV_STATS: the statistics are of the values as stored.  On G1 data the stored values equal float64, so each tile's sum must
    equal the float64 sum bit for bit (S_tile < 2^24 units asserted); M2 (fp32: two passes about fl(s / rows_here)) within
      sum_i [2 |d_i| e_i + e_i^2 + u d_i^2] + gamma(rows + 2) sum_i d_i^2,   e_i = u (|mu| + |d_i|) + u |mu|
    (mu's rounding, the subtraction's, the square's, then the chain over the tile's rows and the folds).  bf16 outputs use a
    shifted sums about a centre c (a stored value of the tile) and a pairwise merge: every term |y - c| <= |y| + max|y|, so
    the sum is held to gamma(rows + 8) (sum|y| + rows max|y|) and M2 to gamma(rows + 8) 2 (sum y^2 + rows max y^2).
    The partial last tile (rows_here < rows per tile) is part of every row whose M is not a multiple of its tile.
Epilogue flags (DV_BIAS, DV_RELU, DV_SIGMOID): bias is G1 data, so relu(conv + bias) is exact; sigmoid s = 1 / (1 + exp(-v))
    of an exact v: b = s ((1 - s) E_EXP(v) + 2u) with E_EXP = (4.2 + 4.1 |v|) u as measured (with its factor 2) in
    tests/test_loss_gemm_optim_gpu.py, and 2u for the addition and the division.

NOT COVERED YET (tests/conv_cases.py: NOT_COVERED_YET says the same to the CPU test): the kernels only a DUALVAR_* switch
reaches (DUALVAR_F32_EXACT=1, DUALVAR_WGRAD_F32S, DUALVAR_CONV_TAP_GRID=1 small ragged tap shapes, DUALVAR_CONV_TAP_BM128)
and the multi-plane grids G2 / G3 for DV_BF16 (its rows run G1 with ties and Gaussian data).  The fp8 pair (the 24 fp8
conv_gemm kernels) is covered by tests/test_fp8_float64_gpu.py over tests/fp8_cases.py.

Each case prints (-s) err / bound; the module prints the largest err / bound per quantity and route at the end.
The measured figures (largest err / bound per quantity and route, the rms figures next to torch fp32's, the mutants) are in
DESIGN.md section 2.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_BIAS, DV_F32, DV_RELU, DV_SIGMOID, DV_STATS, DV_W3  # noqa: E402
from tests import checks  # noqa: E402
from tests import conv_cases as T  # noqa: E402
from tests.chains import e_exp, gamma  # noqa: E402
from tests.checks import F64, TDT, U, Ratios, dev_gen, is_sent, sent  # noqa: E402
from tests.conv_reference import gauss_bound, ref_dgrad, ref_fwd, ref_wgrad  # noqa: E402

RATIO = Ratios()                  # quantity -> largest err / bound of the run
within = RATIO.within
# bit for bit against float64 (bf16: against its round-to-nearest-even bf16): the reference must be an fp32 number; + 0.0 on
# both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)
RMS = {}                          # quantity -> (kernel rms figure, torch fp32 figure or None)
CPU_REF_MAX_FLOPS = 2.5e10        # torch's fp32 CPU conv is taken where 2 M K Cout stays below this: every fp32 row of the table


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    RATIO.report(44)
    print('rms(err) / (u rms(ref)):  kernel   torch fp32 (CPU)')
    for k in sorted(RMS):
        a, b = RMS[k]
        print(f'  {k:44s} {a:7.3f}   {"-" if b is None else "%.3f" % b}')


def rms_figure(got64, ref64):
    return float(((got64 - ref64) ** 2).mean().sqrt() / (U * (ref64 ** 2).mean().sqrt()))


def test_reference_against_torch_float64_on_the_cpu():
    """the loops above against torch.nn.functional.conv3d and its autograd, float64, CPU: a slip in the reference cannot hide
    a slip in a kernel"""
    g = torch.Generator().manual_seed(11)
    for (N, Ci, Tt, H, W, Co, k3, s3, p3) in [(2, 5, 4, 7, 6, 3, (3, 3, 3), (2, 2, 2), (1, 1, 1)), (1, 3, 5, 9, 8, 4, (1, 7, 4), (1, 2, 1), (0, 0, 0)),
                                              (2, 4, 1, 3, 5, 6, (3, 1, 3), (1, 1, 2), (1, 0, 2))]:
        x = torch.randn(N, Ci, Tt, H, W, generator=g, dtype=F64, requires_grad=True)
        w = torch.randn(Co, Ci, *k3, generator=g, dtype=F64, requires_grad=True)
        y = F.conv3d(x, w, None, s3, p3)
        gy = torch.randn(y.shape, generator=g, dtype=F64)
        y.backward(gy)
        xl, wl, gl = x.detach().permute(0, 2, 3, 4, 1).contiguous(), w.detach().permute(0, 2, 3, 4, 1).contiguous(), gy.permute(0, 2, 3, 4, 1).contiguous()
        tol = 1e-12
        assert float((ref_fwd(xl, wl, s3, p3) - y.detach().permute(0, 2, 3, 4, 1)).abs().max()) < tol
        assert float((ref_dgrad(gl, wl, (Tt, H, W), s3, p3) - x.grad.permute(0, 2, 3, 4, 1)).abs().max()) < tol
        assert float((ref_wgrad(xl, gl, k3, s3, p3) - w.grad.permute(0, 2, 3, 4, 1)).abs().max()) < tol


# -------------------------------------------------------------------------------------------------------------- frames
class Frame:
    """an NDHWC view of C channels (pitch cpitch) at channel offset `off` of a [rows + guard, ld] buffer.  Inputs: NaN
    everywhere outside the view (`put` writes the data and the zero pad lanes); outputs: the sentinel pattern everywhere."""

    def __init__(self, dev, dims, C_, cpitch, dtype, wide=False, out=False, guard=37):
        N, Tt, H, W = dims
        self.rows, self.C, self.cpitch, self.dims = N * Tt * H * W, C_, cpitch, dims
        self.off, self.ld = (8, cpitch + 24) if wide else (0, cpitch)
        shape = (self.rows + guard, self.ld)
        self.buf = sent(shape, dev, TDT[dtype]) if out else torch.full(shape, float('nan'), dtype=TDT[dtype], device=dev)
        self.act = ops.Act(self.buf, N, Tt, H, W, C_, self.ld, self.off, dtype, cpitch)
        self.wcols = min(cpitch, ops.cp8(C_))          # lanes a kernel writes: [0, cp8(C)) (the 4-lane RGB input is never an output)

    def put(self, v64):
        self.buf[:self.rows, self.off:self.off + self.cpitch] = 0
        self.buf[:self.rows, self.off:self.off + self.C] = v64.reshape(self.rows, self.C).to(self.buf.dtype)
        return self

    def get(self):
        return self.buf[:self.rows, self.off:self.off + self.C].reshape(self.dims + (self.C,))

    def check_frame(self, what):
        """pad lanes zero, everything outside the written lanes still the sentinel"""
        b, o = self.buf, self.off
        assert float(b[:self.rows, o + self.C:o + self.wcols].float().abs().max() if self.wcols > self.C else 0.0) == 0.0, what + ': pad lanes'
        assert is_sent(b[self.rows:]), what + ': rows behind the tensor written'
        assert is_sent(b[:self.rows, :o]) and is_sent(b[:self.rows, o + self.wcols:]), what + ': lanes outside the view written'


# ---------------------------------------------------------------------------------------------------------------- data
def g1(gen, shape, dev, r=2):
    return torch.randint(-r, r + 1, shape, generator=gen, device=dev).double() / 4


def g2(gen, shape, dev):
    a = torch.randint(1, 4, shape, generator=gen, device=dev)
    b = torch.randint(0, 2, shape, generator=gen, device=dev) * 2 + 1
    sg = torch.randint(0, 2, shape, generator=gen, device=dev) * 2 - 1
    return (sg * (a * 256 + b)).double()


def g3a(gen, shape, dev):
    v = torch.randint(2 ** 23, 2 ** 24, shape, generator=gen, device=dev)
    sg = torch.randint(0, 2, shape, generator=gen, device=dev) * 2 - 1
    return (sg * v).double() * 2.0 ** -20


def g3p(gen, shape, dev):
    e = torch.randint(-3, 4, shape, generator=gen, device=dev)
    sg = torch.randint(0, 2, shape, generator=gen, device=dev) * 2 - 1
    return sg.double() * torch.pow(torch.tensor(2.0, dtype=F64, device=dev), e.double())


def keep_per_row(gen, t2, n):
    """t2 [R, K]: keep at most n entries per row (random positions), zero the rest"""
    R, K = t2.shape
    if K <= n:
        return t2
    idx = torch.randint(0, K, (R, n), generator=gen, device=t2.device)
    m = torch.zeros(R, K, dtype=torch.bool, device=t2.device)
    m.scatter_(1, idx, True)
    return t2 * m


def planes(v64, trunc):
    """the three bf16 planes of fp32 values as split3 (trunc = False) / split3w (mid truncated) form them, in float64"""
    v = v64.to(torch.float32)
    hi = v.to(torch.bfloat16).float()
    r1 = v - hi
    if trunc:
        mid = (r1.view(torch.int32) & -65536).view(torch.float32)
        lo = r1 - mid
    else:
        mid = r1.to(torch.bfloat16).float()
        lo = (r1 - mid).to(torch.bfloat16).float()
    assert bool((hi.double() + mid.double() + lo.double() == v.double()).all()), 'hi + mid + lo != v (test data)'
    return hi, mid, lo


def assert_planes(kind, v64, trunc, what):
    nz = v64 != 0
    if not bool(nz.any()):
        return
    hi, mid, lo = planes(v64[nz], trunc)
    if kind == 'G2':
        assert bool((mid != 0).all()) and bool((lo == 0).all()), what + ': G2 must populate hi and mid only'
    if kind == 'G3A':
        assert float((mid != 0).double().mean()) >= 0.5 and float((lo != 0).double().mean()) >= 0.5, what + ': G3 planes degenerate'


def make_data(c, kind, mode, dev, seed, g1_range=None):
    """-> (x, w, dy) float64 NDHWC / [Cout,kt,kh,kw,Cin], the operand that is not used by `mode` left None; `unit`"""
    gen = dev_gen(dev, seed)
    To, Ho, Wo = T.out_dims(c)
    xs, ws, ys = (c.N, c.T, c.H, c.W, c.Cin), (c.Cout,) + c.k + (c.Cin,), (c.N, To, Ho, Wo, c.Cout)
    K = c.k[0] * c.k[1] * c.k[2]
    x = w = dy = None
    if kind == 'G1':
        r = g1_range or (2 if c.dtype == DV_F32 else 8)         # (bf16: 5-bit integers, so that sums of 9 significant bits -- ties -- occur)
        x, w, dy = g1(gen, xs, dev, r), g1(gen, ws, dev, r), g1(gen, ys, dev, r)
        unit = 1.0 / 16
    elif kind == 'B':
        x = torch.randn(xs, generator=gen, device=dev, dtype=F64).clamp_min(0)
        w = torch.randn(ws, generator=gen, device=dev, dtype=F64) * (c.Cin * K) ** -0.5
        dy = torch.randn(ys, generator=gen, device=dev, dtype=F64)
        x, w, dy = (t.to(torch.float32).to(TDT[c.dtype]).double() for t in (x, w, dy))     # the values the kernels receive
        unit = None
    else:
        n = 24 if kind == 'G2' else 1
        dense, sparse = (g2, g2) if kind == 'G2' else (g3a, g3p) if kind == 'G3' else (g3p, g3a)
        if mode == 'fwd':
            x = dense(gen, xs, dev)
            w = keep_per_row(gen, sparse(gen, ws, dev).reshape(c.Cout, -1), n).reshape(ws)
        elif mode == 'dgrad':
            dy = dense(gen, ys, dev)
            wt = sparse(gen, ws, dev).permute(4, 1, 2, 3, 0).reshape(c.Cin, -1)            # [Cin, taps * Cout]
            w = keep_per_row(gen, wt, n).reshape(c.Cin, *c.k, c.Cout).permute(4, 1, 2, 3, 0).contiguous()
        else:
            x = dense(gen, xs, dev)
            dyt = sparse(gen, ys, dev).reshape(-1, c.Cout).t().contiguous()                 # [Cout, M]
            dy = keep_per_row(gen, dyt, n).t().reshape(ys).contiguous()
        unit = 1.0 if kind == 'G2' else None
        first, second = (x, w) if mode == 'fwd' else (dy, w) if mode == 'dgrad' else (x, dy)
        # the weight-gradient kernels split both operands with split3w; the others split3 (dv_pack_w3 and in the kernels)
        for t, pk in ((first, 'G2' if kind == 'G2' else 'G3A' if kind == 'G3' else 'P'),
                      (second, 'G2' if kind == 'G2' else 'P' if kind == 'G3' else 'G3A')):
            assert_planes(pk, t, mode == 'wgrad', '%s %s %s' % (c.name, kind, mode))
    return x, w, dy, unit


def assert_exact(S, cnt, unit, kind, what):
    """the 2^24 rule, from the float64 reference alone"""
    if kind in ('G3', 'G3S'):
        assert float(cnt.max()) <= 1.0, what + ': more than one term per element (test data)'
    else:
        assert float(S.max()) < 2.0 ** 24 * unit, what + ': sum|terms| leaves the exact range (test data)'


# ------------------------------------------------------------------------------------------------------- the launches
def master_weight(w, cinp):
    """[Cout,kt,kh,kw,Cin] float64 -> fp32 master layout [Cout, taps, CinP]"""
    Co, Ci = w.shape[0], w.shape[4]
    wp = torch.zeros(Co, w.shape[1] * w.shape[2] * w.shape[3], cinp, dtype=torch.float32, device=w.device)
    wp[:, :, :Ci] = w.reshape(Co, -1, Ci).to(torch.float32)
    return wp


def dgrad_weight(w, coutp):
    Co, Ci = w.shape[0], w.shape[4]
    wd = torch.zeros(Ci, w.shape[1] * w.shape[2] * w.shape[3], coutp, dtype=torch.float32, device=w.device)
    wd[:, :, :Co] = w.reshape(Co, -1, Ci).permute(2, 1, 0).to(torch.float32)
    return wd


def is_wide(c):
    """small rows run as channel slices of a wider buffer; the pixel-pair forms need ldx == 8"""
    return c.N * c.T * c.H * c.W < 20000 and c.k != (1, 7, 4) and not c.cinp


def fwd_desc(c, xa, ya, flags):
    return ops.conv_desc(c.dtype, xa.act, ya.act, c.k, c.s, c.p, flags=flags | (DV_W3 if c.w3 else 0))


def run_fwd(c, dev, x, w, flags=0, bias=None, expect_route=True):
    """-> (output Frame, stats [2, Cout, tiles] or None, desc)"""
    To, Ho, Wo = T.out_dims(c)
    wide = is_wide(c)
    xa = Frame(dev, (c.N, c.T, c.H, c.W), c.Cin, T.cin_pitch(c), c.dtype, wide=wide).put(x)
    ya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype, wide=wide, out=True)
    d = fwd_desc(c, xa, ya, flags)
    route = T.query_fwd(d)
    if expect_route:
        assert route == c.fwd, (c.name, route, c.fwd)
    wp = master_weight(w, T.cin_pitch(c))
    wk = ops.pack_w3(wp.view(c.Cout, -1)) if c.w3 else wp.to(TDT[c.dtype])
    stats = sent((2, c.Cout, route.tiles), dev) if flags & DV_STATS else None
    ops.conv_fwd(d, xa.act, wk, bias, ya.act, stats)
    torch.cuda.synchronize()
    return ya, stats, route


def run_dgrad(c, dev, dy, w, old=None):
    To, Ho, Wo = T.out_dims(c)
    wide = is_wide(c)
    dya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype, wide=wide).put(dy)
    dxa = Frame(dev, (c.N, c.T, c.H, c.W), c.Cin, T.cin_pitch(c), c.dtype, wide=wide, out=True)
    if old is not None:
        dxa.put(old)
    d = ops.conv_desc(c.dtype, dxa.act, dya.act, c.k, c.s, c.p, flags=(DV_W3 if c.dgrad.w3 else 0) | (DV_ACCUM if old is not None else 0))
    assert T.query_dgrad(d) == c.dgrad, (c.name, T.query_dgrad(d), c.dgrad)
    wd = dgrad_weight(w, ops.cp8(c.Cout))
    wk = ops.pack_w3(wd.view(c.Cin, -1)) if c.dgrad.w3 else wd.to(TDT[c.dtype])
    ops.conv_dgrad(d, dya.act, wk, dxa.act)
    torch.cuda.synchronize()
    return dxa


def run_wgrad(c, dev, x, dy, old):
    """dw (+)= x^T dy into `old` ([Cout,kt,kh,kw,Cin] float64) -> (dw [Cout, taps, CinP] fp32, the sentinel tail behind it)"""
    To, Ho, Wo = T.out_dims(c)
    wide = is_wide(c)
    xa = Frame(dev, (c.N, c.T, c.H, c.W), c.Cin, T.cin_pitch(c), c.dtype, wide=wide).put(x)
    dya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype, wide=wide).put(dy)
    d = ops.conv_desc(c.dtype, xa.act, dya.act, c.k, c.s, c.p)
    assert T.query_wgrad(d) == c.wgrad, (c.name, T.query_wgrad(d), c.wgrad)
    n = c.Cout * c.k[0] * c.k[1] * c.k[2] * T.cin_pitch(c)
    buf = sent((n + 64,), dev)
    buf[:n] = master_weight(old, T.cin_pitch(c)).reshape(-1)
    need = ops.wgrad_workspace_bytes(d)
    ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device=dev)       # NaN words: every slab word that is read was written
    ops.conv_wgrad(d, xa.act, dya.act, buf, workspace=ws)
    torch.cuda.synchronize()
    assert is_sent(buf[n:]), c.name + ': written behind dw'
    return buf[:n].reshape(c.Cout, -1, T.cin_pitch(c))


def cpu_fp32_figures(c, x, w, dy, mode):
    """torch's fp32 CPU conv3d (mode 'fwd') or its autograd for the one gradient asked for, on the same data, as float64 NDHWC; None
    where the shape is too large for the CPU.  Operands the mode does not use may be None."""
    To, Ho, Wo = T.out_dims(c)
    if 2.0 * c.N * To * Ho * Wo * c.k[0] * c.k[1] * c.k[2] * c.Cin * c.Cout > CPU_REF_MAX_FLOPS:
        return None
    nc = lambda t, shape: (torch.zeros(shape) if t is None else t.cpu().float()).permute(0, 4, 1, 2, 3).contiguous()      # noqa: E731
    xc = nc(x, (c.N, c.T, c.H, c.W, c.Cin)).requires_grad_(mode == 'dgrad')
    wc = nc(w, (c.Cout,) + c.k + (c.Cin,)).requires_grad_(mode == 'wgrad')
    with torch.set_grad_enabled(mode != 'fwd'):
        y = F.conv3d(xc, wc, None, c.s, c.p)
    if mode == 'fwd':
        return y.permute(0, 2, 3, 4, 1).double()
    y.backward(nc(dy, (c.N, To, Ho, Wo, c.Cout)))
    return (xc.grad if mode == 'dgrad' else wc.grad).permute(0, 2, 3, 4, 1).double()


def route_key(c, mode):
    r = {'fwd': c.fwd, 'dgrad': c.dgrad}.get(mode)
    dt = 'f32' if c.dtype == DV_F32 else 'bf16'
    if mode == 'wgrad':
        return 'wgrad:%s:%dx%d' % (dt, c.wgrad.rows, c.wgrad.cols)
    path = r.path + (str(r.kind) if r.path in ('TAP', 'TAP_CLASSES') else '')
    form = ('' if c.dtype != DV_F32 else ':w3' if (c.w3 if mode == 'fwd' else r.w3) else ':split')
    return '%s:%s:%s%s' % (mode, dt, path, form)


# ------------------------------------------------------------------------------------------------------ the main sweep
IDS = [c.name for c in T.CASES]


def _kinds(c):
    out = []
    for k in c.data.split():
        out += ['G3', 'G3S'] if k == 'G3' else [k]
    return out


def _stats_check(c, dev, y_ref, stats, route, exact, what, unit=1.0 / 16):
    """per-tile sums and M2 of the stored values against float64"""
    M, Co = y_ref.numel() // c.Cout, c.Cout
    rows, tiles = route.rows, route.tiles
    assert tiles * rows >= M > (tiles - 1) * rows
    yp = torch.zeros(tiles * rows, Co, dtype=F64, device=dev)
    if route.kind == 2:        # the temporal LDS-staged form: a tile is rows / T pixels (n, h, w) x all T frames
        To = T.out_dims(c)[0]
        yp[:M] = y_ref.reshape(c.N, To, -1, Co).permute(0, 2, 1, 3).reshape(M, Co)
    else:
        yp[:M] = y_ref.reshape(M, Co)
    yt = yp.reshape(tiles, rows, Co)
    valid = (torch.arange(tiles * rows, device=dev) < M).reshape(tiles, rows, 1)
    nrow = valid.sum(1).double()                                     # [tiles, 1]
    s = yt.sum(1)
    mu = s / nrow
    dlt = torch.where(valid, yt - mu[:, None, :], torch.zeros_like(yt))
    m2 = (dlt ** 2).sum(1)
    got_s, got_m2 = stats[0].t().double(), stats[1].t().double()     # [tiles, Cout]
    assert bool(torch.isfinite(stats).all()), what + ': statistics not written'
    amax = yt.abs().amax(1)
    if exact:      # (bf16 too: the shifted form n c + s1 of grid data is exact)
        assert float(yt.abs().sum(1).max() + rows * amax.max()) < 2.0 ** 24 * unit, what + ': tile sums leave the exact range (test data)'
        same_bits(stats[0].t(), s, what + ' tile sums')
    elif c.dtype == DV_F32:
        within(got_s, s, gamma(rows + 8) * yt.abs().sum(1), 'stats_sum:' + what)
    else:      # sums about a centre c (a stored value): every term |y - c| <= |y| + max|y|, then s = n c + s1
        within(got_s, s, gamma(rows + 8) * (yt.abs().sum(1) + rows * amax), 'stats_sum:' + what)
    if c.dtype == DV_F32:
        e = U * (mu.abs()[:, None, :] + dlt.abs()) + U * mu.abs()[:, None, :]
        b = torch.where(valid, 2 * dlt.abs() * e + e * e + U * dlt ** 2, torch.zeros_like(yt)).sum(1) + gamma(rows + 2) * m2
    else:
        b = gamma(rows + 8) * 2 * ((yt ** 2).sum(1) + rows * amax ** 2)
    within(got_m2, m2, b, 'stats_m2:' + what)


@pytest.mark.parametrize('case', T.CASES, ids=IDS)
def test_conv_fwd(gpu, case):
    """dv_conv3d_fwd (+ DV_STATS) on the row's route: exact grids bit for bit, Gaussian data inside the bound, frames intact,
    two launches the same bits"""
    c, dev = case, gpu
    for kind in _kinds(c):
        x, w, _, unit = make_data(c, kind, 'fwd', dev, 100)
        ref = ref_fwd(x, w, c.s, c.p)
        S = ref_fwd(x.abs(), w.abs(), c.s, c.p)
        cnt = ref_fwd((x != 0).double(), (w != 0).double(), c.s, c.p)
        what = '%s %s %s' % (route_key(c, 'fwd'), c.name, kind)
        ya, stats, route = run_fwd(c, dev, x, w, flags=DV_STATS)
        ya.check_frame(what)
        got = ya.get()
        if kind == 'B':
            within(got, ref, gauss_bound(c, 'fwd', S, cnt, ref), what)
            ya2, stats2, _ = run_fwd(c, dev, x, w, flags=DV_STATS)
            assert torch.equal(ya2.get(), got) and torch.equal(stats2, stats), what + ': two launches differ'
            _stats_check(c, dev, got.double(), stats, route, False, what)
            if c.dtype == DV_F32:
                cpu = cpu_fp32_figures(c, x, w, None, 'fwd')
                fig, cfig = rms_figure(got.double(), ref), (rms_figure(cpu.to(dev), ref) if cpu is not None else None)
                key = route_key(c, 'fwd')
                RMS[key] = max(RMS.get(key, (0, None)), (fig, cfig), key=lambda t: t[0])
                print(f'    {what}: rms figure {fig:.3f}  torch fp32 {cfig}')
                if cfig is not None:
                    assert fig <= 4 * cfig, f'{what}: rms figure {fig:.3f} > 4 x torch fp32 {cfig:.3f}'
        else:
            assert_exact(S, cnt, unit, kind, what)
            same_bits(got, ref, what)
            if kind == 'G1':
                if c.dtype == DV_BF16:
                    r32 = ref.to(torch.float32)
                    assert bool(((r32.view(torch.int32) & 0xFFFF) == 0x8000).any()), what + ': no bf16 tie in the data'
                _stats_check(c, dev, got.double(), stats, route, True, what)


@pytest.mark.parametrize('case', [c for c in T.CASES if c.dgrad is not None], ids=[c.name for c in T.CASES if c.dgrad is not None])
def test_conv_dgrad(gpu, case):
    """dv_conv3d_dgrad on the row's route, plain and with DV_ACCUM onto grid data (positions no output window reaches read 0 /
    keep their old value)"""
    c, dev = case, gpu
    xd = (c.T, c.H, c.W)
    for kind in _kinds(c):
        _, w, dy, unit = make_data(c, kind, 'dgrad', dev, 200)
        ref = ref_dgrad(dy, w, xd, c.s, c.p)
        S = ref_dgrad(dy.abs(), w.abs(), xd, c.s, c.p)
        cnt = ref_dgrad((dy != 0).double(), (w != 0).double(), xd, c.s, c.p)
        what = '%s %s %s' % (route_key(c, 'dgrad'), c.name, kind)
        dxa = run_dgrad(c, dev, dy, w)
        dxa.check_frame(what)
        got = dxa.get()
        if kind == 'B':
            within(got, ref, gauss_bound(c, 'dgrad', S, cnt, ref), what)
            assert torch.equal(run_dgrad(c, dev, dy, w).get(), got), what + ': two launches differ'
            if c.dtype == DV_F32:
                cpu = cpu_fp32_figures(c, None, w, dy, 'dgrad')
                fig, cfig = rms_figure(got.double(), ref), (rms_figure(cpu.to(dev), ref) if cpu is not None else None)
                key = route_key(c, 'dgrad')
                RMS[key] = max(RMS.get(key, (0, None)), (fig, cfig), key=lambda t: t[0])
                print(f'    {what}: rms figure {fig:.3f}  torch fp32 {cfig}')
                if cfig is not None:
                    assert fig <= 4 * cfig, f'{what}: rms figure {fig:.3f} > 4 x torch fp32 {cfig:.3f}'
        else:
            assert_exact(S, cnt, unit, kind, what)
            same_bits(got, ref, what)
        if kind == 'G1':
            old = g1(dev_gen(dev, 201), ref.shape, dev)
            assert float((S + old.abs()).max()) < 2.0 ** 24 / 16
            if c.dtype == DV_BF16:                                   # the old value and the new one are each a bf16 number; their
                want = (ref.to(torch.float32).to(torch.bfloat16).double() + old)   # sum is rounded once more
            else:
                want = ref + old
            dxo = run_dgrad(c, dev, dy, w, old=old)
            dxo.check_frame(what + ' accum')
            same_bits(dxo.get(), want, what + ' accum')


@pytest.mark.parametrize('case', T.CASES, ids=IDS)
def test_conv_wgrad(gpu, case):
    """dv_conv3d_wgrad on the row's kernel and row split: dw += x^T dy onto grid data, NaN in the workspace"""
    c, dev = case, gpu
    for kind in _kinds(c):
        x, _, dy, unit = make_data(c, kind, 'wgrad', dev, 300)
        ref = ref_wgrad(x, dy, c.k, c.s, c.p)
        S = ref_wgrad(x.abs(), dy.abs(), c.k, c.s, c.p)
        cnt = ref_wgrad((x != 0).double(), (dy != 0).double(), c.k, c.s, c.p)
        what = '%s %s %s' % (route_key(c, 'wgrad'), c.name, kind)
        old = g1(dev_gen(dev, 301), ref.shape, dev) if kind in ('G1', 'B') else torch.zeros_like(ref)
        dw = run_wgrad(c, dev, x, dy, old)
        got = dw[:, :, :c.Cin].reshape(ref.shape)
        assert float(dw[:, :, c.Cin:].abs().max() if dw.shape[2] > c.Cin else 0.0) == 0.0, what + ': pad lanes of dw'
        if kind == 'B':
            within(got, ref + old, gauss_bound(c, 'wgrad', S, cnt, ref) + U * (ref + old).abs(), what)
            assert torch.equal(run_wgrad(c, dev, x, dy, old), dw), what + ': two launches differ'
            if c.dtype == DV_F32:
                cpu = cpu_fp32_figures(c, x, None, dy, 'wgrad')
                fig = rms_figure(got.double() - old, ref)
                cfig = rms_figure(cpu.to(dev), ref) if cpu is not None else None
                key = route_key(c, 'wgrad')
                RMS[key] = max(RMS.get(key, (0, None)), (fig, cfig), key=lambda t: t[0])
                print(f'    {what}: rms figure {fig:.3f}  torch fp32 {cfig}')
                if cfig is not None:
                    assert fig <= 4 * cfig, f'{what}: rms figure {fig:.3f} > 4 x torch fp32 {cfig:.3f}'
        else:
            assert_exact(S + old.abs(), cnt, unit, kind, what)
            same_bits(got, ref + old, what)


# ------------------------------------------------------------------------------------------------- the epilogue flags
FLAG_ROWS = ['pw_c64_m294', 'pw_c24_m16384', 'ks32_m72', 'c144_c230_sp3', 'tap_sp_m12544', 'pair_stem_pp', 'now3_sp3_c24', 'now3_pw_s2', 'now3_sp3_s2_c83', 'c40_c3_sp3',
             'bf_sp3_c24']
FLAG_SETS = [DV_BIAS, DV_RELU, DV_BIAS | DV_RELU, DV_SIGMOID, DV_BIAS | DV_SIGMOID, DV_BIAS | DV_RELU | DV_SIGMOID]


@pytest.mark.parametrize('name', FLAG_ROWS)
def test_conv_fwd_epilogue_flags(gpu, name):
    """DV_BIAS / DV_RELU / DV_SIGMOID of dv_conv3d_fwd, alone and combined, with DV_STATS: conv_gemm's direct-store path (full
    tiles) and its staged path (the partial last tile of M = 294 and of the ragged rows), conv_gemm_ks, and the fall-back
    of the rows that run on the LDS-staged kernel / the pixel-pair form without flags (those kernels refuse them) to one that
    honours them."""
    c, dev = T.BY_NAME[name], gpu
    x, w, _, _ = make_data(c, 'G1', 'fwd', dev, 400, g1_range=2)
    conv = ref_fwd(x, w, c.s, c.p)
    S = ref_fwd(x.abs(), w.abs(), c.s, c.p)
    bias64 = g1(dev_gen(dev, 401), (c.Cout,), dev) * 8                       # multiples of 2 in [-4, 4]: moves the means
    assert float(S.max()) + 4 < 2.0 ** 24 / 16
    bias = torch.full((ops.cp8(c.Cout) + 8,), float('nan'), device=dev)      # NaN behind the Cout values
    bias[:c.Cout] = bias64.float()
    for fl in FLAG_SETS:
        v = conv + (bias64 if fl & DV_BIAS else 0)
        if fl & DV_RELU:
            v = v.clamp_min(0)
        ya, stats, route = run_fwd(c, dev, x, w, flags=fl | DV_STATS, bias=bias if fl & DV_BIAS else None, expect_route=False)
        assert route.kind == 0, (name, route)                               # flags never run on the LDS-staged / pixel-pair kernels
        if c.fwd.kind == 0:
            assert route == c.fwd, (name, route)                            # ... and do not move any other row
        what = 'fwd_flags:%s:%s %s flags %d' % ('f32' if c.dtype == DV_F32 else 'bf16', route.path, c.name, fl)
        ya.check_frame(what)
        got = ya.get()
        if fl & DV_SIGMOID:
            s = torch.sigmoid(v)
            b = s * ((1 - s) * e_exp(v) + 2 * U)
            if c.dtype == DV_BF16:
                b = b + 2.0 ** -8 * (s + b)
            within(got, s, b, what)
            _stats_check(c, dev, got.double(), stats, route, False, what)
        else:
            same_bits(got, v, what)
            _stats_check(c, dev, got.double(), stats, route, True, what)


# ------------------------------------------------------------------------------------------ packed weight layouts
def test_pack_w3_planes_and_dgrad_layout_bit_exact(gpu):
    """dv_pack_w3 against the host split (bf16 round-to-nearest residues) in its documented layout [K tile][k half][rows
    padded to 128][hi|mid|lo][8], and dv_pack_dgrad_weights against the host permutation: bit for bit"""
    dev = gpu
    gen = dev_gen(dev, 500)
    for rows, ktot in [(24, 64), (83, 72), (130, 16 * 9 + 8), (1, 8)]:
        w = torch.randn(rows, ktot, generator=gen, device=dev)
        w[0, 0] = 2.0 ** -20 * (2 ** 23 + 12345)
        out = ops.pack_w3(w)
        kt, npad = (ktot + 15) // 16, (rows + 127) // 128 * 128
        assert out.numel() == kt * 2 * npad * 48 == L.load().dv_w3_bytes(rows, ktot)
        got = out.view(torch.bfloat16).reshape(kt, 2, npad, 3, 8)
        wpad = torch.zeros(npad, kt * 16, device=dev)
        wpad[:rows, :ktot] = w
        hi, mid, lo = planes(wpad.double(), False)
        want = torch.stack([p.reshape(npad, kt, 2, 8).permute(1, 2, 0, 3) for p in (hi, mid, lo)], dim=3).to(torch.bfloat16)
        assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), (rows, ktot)
    shapes = [(64, 32, 9), (83, 64, 3), (48, 16, 1), (230, 144, 9)]
    master, descs, bmap, soff, doff = [], [], [], 0, 0
    for i, (O, I, taps) in enumerate(shapes):
        cinp, coutp = ops.cp8(I), ops.cp8(O)
        w = torch.randn(O, taps, cinp, generator=gen, device=dev)
        w[:, :, I:] = 0
        master.append(w)
        descs.append((soff, doff, O, I, taps, cinp, coutp))
        bmap += [(i, r) for r in range(I)]
        soff += w.numel()
        doff += I * taps * coutp
    m = torch.cat([w.reshape(-1) for w in master])
    darr = (L.PackDesc * len(descs))()
    for j, t in enumerate(descs):
        darr[j].src_off, darr[j].dst_off, darr[j].Cout, darr[j].Cin, darr[j].taps, darr[j].cin_pitch, darr[j].cout_pitch = t
    dbytes = torch.frombuffer(bytearray(bytes(darr)), dtype=torch.uint8).to(dev)
    bm = torch.tensor(bmap, dtype=torch.int32).to(dev)
    for dtype in (DV_F32, DV_BF16):
        dst = sent((doff + 16,), dev, TDT[dtype])
        ops.call('dv_pack_dgrad_weights', dtype, m, dst, dbytes, bm, len(bmap))
        torch.cuda.synchronize()
        assert is_sent(dst[doff:])
        for (so, do, O, I, taps, cinp, coutp), w in zip(descs, master):
            want = torch.zeros(I, taps, coutp, device=dev)
            want[:, :, :O] = w[:, :, :I].permute(2, 1, 0)
            same_bits(dst[do:do + I * taps * coutp].reshape(I, taps, coutp), want.double(), 'pack_dgrad %d' % dtype)


# ------------------------------------------------------------------------------------------ the fused BatchNorm forms
def _pow2_affine(gen, C_, dev):
    """power-of-two scale, quarter-integer shift: x * scale + shift of grid data is exact"""
    cp = ops.cp8(C_)
    scale, shift = torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)
    scale[:C_] = g3p(gen, (C_,), dev).float().clamp(-2, 2)
    shift[:C_] = g1(gen, (C_,), dev).float()
    return scale, shift


@pytest.mark.parametrize('name', ['tap_tm_m12544', 'tap_tm_t2', 'stem_tm7_m131072'])
@pytest.mark.parametrize('relu', [True, False])
def test_conv_bn_on_load_against_float64(gpu, name, relu):
    """dv_conv3d_fwd_bn_in / dv_conv3d_wgrad_bn_in on grid data against float64 directly: y = conv([relu](x scale + shift), w)
    with the conv's zero padding applied to the BatchNorm's OUTPUT, the pad lanes of x_bn poisoned"""
    c, dev = T.BY_NAME[name], gpu
    lib = L.load()
    gen = dev_gen(dev, 600)
    x, w, dy, _ = make_data(c, 'G1', 'fwd', dev, 601)
    scale, shift = _pow2_affine(gen, c.Cin, dev)
    act = x * scale[:c.Cin].double() + shift[:c.Cin].double()
    if relu:
        act = act.clamp_min(0)
    ref = ref_fwd(act, w, c.s, c.p)
    S = ref_fwd(act.abs(), w.abs(), c.s, c.p)
    assert float(S.max()) < 2.0 ** 24 / 128                # unit: x scale in 1/32, times w in 1/4
    To, Ho, Wo = T.out_dims(c)
    xa = Frame(dev, (c.N, c.T, c.H, c.W), c.Cin, T.cin_pitch(c), c.dtype).put(x)
    ya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype, out=True)
    d = ops.conv_desc(c.dtype, xa.act, ya.act, c.k, c.s, c.p, flags=DV_W3 | DV_STATS)
    assert lib.dv_conv3d_bn_in_ok(C.byref(d)) == c.bn_in > 0
    route = T.query_fwd(d)
    stats = sent((2, c.Cout, route.tiles), dev)
    bn = ops.bn_in_desc(scale, shift, relu)
    ops.conv_fwd_bn_in(d, xa.act, bn, ops.pack_w3(master_weight(w, T.cin_pitch(c)).view(c.Cout, -1)), ya.act, stats)
    torch.cuda.synchronize()
    what = 'fwd_bn_in %s relu %d' % (name, relu)
    ya.check_frame(what)
    same_bits(ya.get(), ref, what)
    _stats_check(c, dev, ya.get().double(), stats, route, True, what, unit=1.0 / 128)
    # the weight gradient with the same operand formed on load
    refw = ref_wgrad(act, dy, c.k, c.s, c.p)
    Sw = ref_wgrad(act.abs(), dy.abs(), c.k, c.s, c.p)
    assert float(Sw.max()) < 2.0 ** 24 / 128
    dya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype).put(dy)
    dwd = ops.conv_desc(c.dtype, xa.act, dya.act, c.k, c.s, c.p)
    dw = torch.zeros(c.Cout, c.k[0] * c.k[1] * c.k[2], T.cin_pitch(c), device=dev)
    need = ops.wgrad_workspace_bytes(dwd)
    ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device=dev)
    ops.conv_wgrad_bn_in(dwd, xa.act, bn, dya.act, dw, workspace=ws)
    torch.cuda.synchronize()
    same_bits(dw[:, :, :c.Cin].reshape(refw.shape), refw, 'wgrad_bn_in %s relu %d' % (name, relu))


@pytest.mark.parametrize('name', ['tap_sp_m12544', 'tap_tm_m12544', 'stem_tm7_m12544', 'sp3_c40_m16384'])
def test_conv_dgrad_bn_ordered_against_float64(gpu, name):
    """dv_conv3d_dgrad_bn_ws (the ordered form on the LDS-staged kernel) on grid data with power-of-two mean / invstd / scale /
    shift: dx equal to float64 bit for bit, both sums equal to float64 bit for bit, `+=` into the caller's sums, ticket words
    left zero, two launches the same bits.  dv_conv3d_dgrad_bn (the atomic form) on the same data: same dx, sums exact too
    (every partial sum of exact data is exact in any order)."""
    c, dev = T.BY_NAME[name], gpu
    lib = L.load()
    gen = dev_gen(dev, 700)
    _, w, dy, _ = make_data(c, 'G1', 'dgrad', dev, 701)
    xd = (c.T, c.H, c.W)
    ref = ref_dgrad(dy, w, xd, c.s, c.p)
    Ci, cp = c.Cin, ops.cp8(c.Cin)
    xbn = g1(gen, ref.shape, dev)
    scale, shift = _pow2_affine(gen, Ci, dev)
    mean, invstd = torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)
    mean[:Ci] = g1(gen, (Ci,), dev).float()
    invstd[:Ci] = g3p(gen, (Ci,), dev).float().abs().clamp(0.5, 2)
    To, Ho, Wo = T.out_dims(c)
    for bflag in (0, L.DV_NO_RELU_MASK):
        act = xbn * scale[:Ci].double() + shift[:Ci].double()
        gmask = ref if bflag else torch.where(act > 0, ref, torch.zeros_like(ref))
        xhat = (xbn - mean[:Ci].double()) * invstd[:Ci].double()
        want = torch.stack([gmask.reshape(-1, Ci).sum(0), (gmask * xhat).reshape(-1, Ci).sum(0)])
        # unit: dx in 1/16, xhat = (x - mean) invstd in 1/8
        assert float((gmask * xhat).abs().reshape(-1, Ci).sum(0).max()) < 2.0 ** 24 / 128, 'sums leave the exact range (test data)'
        dya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype).put(dy)
        xb = Frame(dev, (c.N,) + xd, Ci, T.cin_pitch(c), c.dtype).put(xbn)
        wk = ops.pack_w3(dgrad_weight(w, ops.cp8(c.Cout)).view(Ci, -1))
        runs = []
        # (a strided data gradient takes pre-split weights on the LDS-staged kernel only: no atomic form there)
        for form in ('ordered', 'ordered') + (('atomic',) if max(c.s) == 1 else ()):
            dxa = Frame(dev, (c.N,) + xd, Ci, T.cin_pitch(c), c.dtype, out=True)
            d = ops.conv_desc(c.dtype, dxa.act, dya.act, c.k, c.s, c.p, flags=DV_W3)
            need = int(lib.dv_conv3d_dgrad_bn_workspace(C.byref(d)))
            assert need == c.dgrad_bn_ws > 0
            n_rep = 1 if form == 'ordered' else 3
            sums = torch.ones(n_rep, 2, cp, device=dev) if form == 'ordered' else torch.zeros(n_rep, 2, cp, device=dev)
            r = ops.bn_reduce_desc(xb.act, mean, invstd, scale, shift, sums, n_rep, bflag)
            if form == 'ordered':
                ws = torch.zeros(need // 4 + 16, device=dev)
                L.check(lib.dv_conv3d_dgrad_bn_ws(C.byref(d), dya.act.ptr, wk.data_ptr(), dxa.act.ptr, C.byref(r), ws.data_ptr(), need,
                                                  ops.stream_ptr()), 'dv_conv3d_dgrad_bn_ws')
                torch.cuda.synchronize()
                assert float(ws[:16384].abs().max()) == 0.0, 'ticket words not left zero'
                got = sums[0].double() - 1.0
            else:
                ops.conv_dgrad_bn(d, dya.act, wk, dxa.act, r)
                torch.cuda.synchronize()
                got = sums.double().sum(0)
            what = 'dgrad_bn_%s %s flag %d' % (form, name, bflag)
            dxa.check_frame(what)
            same_bits(dxa.get(), ref, what + ' dx')
            same_bits(got[:, :Ci].float(), want, what + ' sums')
            assert float(got[:, Ci:].abs().max() if cp > Ci else 0.0) == 0.0
            runs.append((dxa.get().clone(), sums.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------- scaling and the edge of the split
SCALE_ROWS = [('pw_c64_m294', 'fwd'), ('pw_c64_m294', 'dgrad'), ('now3_sp3_c24', 'fwd'), ('now3_sp3_c24', 'dgrad'), ('ks32_m72', 'fwd'),
              ('ks32_m72', 'dgrad'), ('tap_sp_m12544', 'fwd'), ('tap_tm_m12544', 'dgrad'), ('stem_tm7_m12544', 'dgrad'),
              ('pw_c64_m294', 'wgrad'), ('tap_tm_m12544', 'wgrad'), ('w1x9x9_c16', 'wgrad')]


@pytest.mark.parametrize('name,mode', SCALE_ROWS, ids=['%s-%s' % r for r in SCALE_ROWS])
@pytest.mark.parametrize('e', [40, -40])
def test_conv_exact_grids_scaled_by_powers_of_two(gpu, name, mode, e):
    """one G2 and one G3 case per kernel family with BOTH operands scaled by 2^e: the bits must be the scaled bits (the split
    and the six products are scale free inside the exponent range; products move by 2^(2e))"""
    c, dev = T.BY_NAME[name], gpu
    sc = 2.0 ** e
    for kind in ('G2', 'G3'):
        x, w, dy, unit = make_data(c, kind, mode, dev, 800)
        x, w, dy = (None if t is None else t * sc for t in (x, w, dy))
        what = 'scaled %s %s %s 2^%d' % (name, mode, kind, e)
        if mode == 'fwd':
            ref, S, cnt = (ref_fwd(a, b, c.s, c.p) for a, b in ((x, w), (x.abs(), w.abs()), ((x != 0).double(), (w != 0).double())))
            got = run_fwd(c, dev, x, w)[0].get()
        elif mode == 'dgrad':
            xd = (c.T, c.H, c.W)
            ref, S, cnt = (ref_dgrad(a, b, xd, c.s, c.p) for a, b in ((dy, w), (dy.abs(), w.abs()), ((dy != 0).double(), (w != 0).double())))
            got = run_dgrad(c, dev, dy, w).get()
        else:
            ref, S, cnt = (ref_wgrad(a, b, c.k, c.s, c.p) for a, b in ((x, dy), (x.abs(), dy.abs()), ((x != 0).double(), (dy != 0).double())))
            got = run_wgrad(c, dev, x, dy, torch.zeros_like(ref))[:, :, :c.Cin].reshape(ref.shape)
        assert_exact(S, cnt, None if unit is None else unit * sc * sc, kind, what)
        assert float(ref.abs().max()) > 0
        same_bits(got, ref, what)


def test_split_exactness_range_on_the_matrix_cores(gpu):
    """hi + mid + lo == v needs the lowest bit of lo, 2^-23 |v|, to be a bf16 number.  Host emulation (bf16 round to nearest,
    every 24-bit mantissa pattern sampled): with bf16 denormals every normal |v| >= 2^-110 splits exactly (2^-133 is bf16's
    smallest denormal); if bf16 denormals were flushed, only |v| >= 2^-103 would.  gfx950 keeps them, in the conversion and on
    the matrix cores (the lo * 1.0 partial products at 2^-110 are fp32 denormals, 2^-127 .. 2^-133, and the accumulator keeps
    them), so this asserts that an identity convolution returns its input bit for bit at |v| in [2^-90, 2^-89), [2^-103,
    2^-102) and [2^-110, 2^-109): the documented edge (csrc/conv_common.hpp, include/dualvar_hip.h).  Below the edge the
    fraction of elements that come back exact is only printed, nothing is asserted."""
    c, dev = T.BY_NAME['pw_c64_m294'], gpu
    gen = dev_gen(dev, 900)
    w = torch.zeros((c.Cout, 1, 1, 1, c.Cin), dtype=F64, device=dev)
    for o in range(c.Cout):
        w[o, 0, 0, 0, (5 * o) % c.Cin] = 1.0
    for e in (-90, -103, -110, -114, -120):
        x = g3a(gen, (c.N, c.T, c.H, c.W, c.Cin), dev) * 2.0 ** (e - 3)          # g3a: 8 <= |v| < 16
        assert float(x.abs().min()) >= 2.0 ** e and float(x.abs().max()) < 2.0 ** (e + 1)
        ref = ref_fwd(x, w, c.s, c.p)
        got = run_fwd(c, dev, x, w)[0].get()
        frac = float((got.double() == ref).double().mean())
        print(f'    identity conv at |v| in [2^{e}, 2^{e + 1}): {100 * frac:.2f} % of the elements returned bit for bit')
        if e >= -110:
            same_bits(got, ref, 'identity conv at 2^%d' % e)


# ------------------------------------------------------------------------------- the fused BatchNorm-backward weight gradient
WGRAD_BN_ROWS = ['pw_c64_m294', 'pw_c24_m16384', 'rgb_stem_sp7', 'ks32_m72', 'c144_c230_sp3', 'pair_stem_pp']


def _wgrad_bn_call(c, dev, x, g, y, gamma_, mean, invstd, scale, shift, sums, inv_count, relu, dw, dgamma, dbeta):
    """-> return code of dv_conv3d_wgrad_bn on dense frames (bn->x must have the pitch of g)"""
    lib = L.load()
    To, Ho, Wo = T.out_dims(c)
    xa = Frame(dev, (c.N, c.T, c.H, c.W), c.Cin, T.cin_pitch(c), c.dtype).put(x)
    ga = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype).put(g)
    ya = Frame(dev, (c.N, To, Ho, Wo), c.Cout, ops.cp8(c.Cout), c.dtype).put(y)
    d = ops.conv_desc(c.dtype, xa.act, ga.act, c.k, c.s, c.p)
    assert T.query_wgrad(d) == c.wgrad, (c.name, T.query_wgrad(d), c.wgrad)
    r = L.BnBwd()
    r.x, r.ldx = ya.act.ptr, ya.ld
    r.mean, r.invstd, r.gamma, r.scale, r.shift = (t.data_ptr() for t in (mean, invstd, gamma_, scale, shift))
    r.sums, r.n_rep, r.flags = sums.data_ptr(), sums.shape[0], (0 if relu else L.DV_NO_RELU_MASK)
    r.dgamma, r.dbeta, r.inv_count, r.dparam_scale = dgamma.data_ptr(), dbeta.data_ptr(), inv_count, 0.5
    need = ops.wgrad_workspace_bytes(d)
    ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device=dev)
    rc = lib.dv_conv3d_wgrad_bn(C.byref(d), xa.act.ptr, ga.act.ptr, dw.data_ptr(), ws.data_ptr(), need, C.byref(r), ops.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('name', WGRAD_BN_ROWS)
@pytest.mark.parametrize('relu', [True, False])
def test_conv_wgrad_bn_against_float64(gpu, name, relu):
    """dv_conv3d_wgrad_bn on grid data against float64 directly: dw += x^T (k1 g' + k2 y + k3) with g' = g masked by
    (y scale + shift > 0), k1 = gamma invstd, k2 = -k1 invstd sum(g xhat) inv_count, k3 = -k1 sum(g) inv_count - k2 mean
    (dv_bn_bwd_apply's expression).  gamma (+-1, +-2), invstd (1, 2), scale and inv_count (1) are powers of two, mean, shift and the two sums (any
    sums will do: the entry takes them as given, here over three replicas) quarter integers, so every step of the expression
    is exact -- asserted by forming it in fp32 in the kernel's order on the host -- and dw, dgamma, dbeta must equal float64
    bit for bit.  Rows: conv_wgrad_dma_kernel's shared-split form with one and with many row splits, ragged channel counts,
    the RGB input, and the pixel-pair stem form."""
    c, dev = T.BY_NAME[name], gpu
    assert c.wgrad.bn_ok == 1
    gen = dev_gen(dev, 1000)
    Co, cp = c.Cout, ops.cp8(c.Cout)
    x, _, g, _ = make_data(c, 'G1', 'fwd', dev, 1001)
    y = g1(gen, g.shape, dev)                                    # the BatchNorm's input = the conv's forward output
    scale, shift = _pow2_affine(gen, Co, dev)
    pad = lambda t: torch.cat([t.float(), torch.zeros(cp - Co, device=dev)])       # noqa: E731
    gamma_ = pad(g3p(gen, (Co,), dev).sign() * g3p(gen, (Co,), dev).abs().clamp(1, 2))      # +-1, +-2
    invstd = pad(g3p(gen, (Co,), dev).abs().clamp(1, 2))
    mean = pad(g1(gen, (Co,), dev))
    sums = torch.zeros(3, 2, cp, device=dev)
    sums[:, :, :Co] = g1(gen, (3, 2, Co), dev, 1).float()
    inv_count = 1.0
    sg, sgx = sums[:, 0, :Co].double().sum(0), sums[:, 1, :Co].double().sum(0)
    k1 = gamma_[:Co].double() * invstd[:Co].double()
    k2 = -k1 * invstd[:Co].double() * sgx * inv_count
    k3 = -k1 * sg * inv_count - k2 * mean[:Co].double()
    act = y * scale[:Co].double() + shift[:Co].double()
    gm = torch.where(act > 0, g, torch.zeros_like(g)) if relu else g
    dly = k1 * gm + k2 * y + k3
    # the same in fp32, in the kernel's order (no fma): exact data makes the two agree exactly
    f = lambda t: t.float()      # noqa: E731
    k1f = gamma_[:Co] * invstd[:Co]
    k2f = -k1f * invstd[:Co] * f(sgx) * inv_count
    k3f = -k1f * f(sg) * inv_count - k2f * mean[:Co]
    assert bool(((k1f * f(gm) + k2f * f(y) + k3f).double() == dly).all()), 'the expression is not exact in fp32 (test data)'
    ref = ref_wgrad(x, dly, c.k, c.s, c.p)
    S = ref_wgrad(x.abs(), dly.abs(), c.k, c.s, c.p)
    old = g1(gen, ref.shape, dev)
    unit = 2.0 ** -6                                             # dL/dy in 1/16 (k2 y, k2 mean), x in 1/4
    assert bool((dly * 16 == (dly * 16).round()).all())
    assert float((S + old.abs()).max()) < 2.0 ** 24 * unit, 'sum|terms| leaves the exact range (test data)'
    n = Co * c.k[0] * c.k[1] * c.k[2] * T.cin_pitch(c)
    buf = sent((n + 64,), dev)
    buf[:n] = master_weight(old, T.cin_pitch(c)).reshape(-1)
    dgamma, dbeta = torch.ones(cp, device=dev), torch.ones(cp, device=dev)
    rc = _wgrad_bn_call(c, dev, x, g, y, gamma_, mean, invstd, scale, shift, sums, inv_count, relu, buf, dgamma, dbeta)
    assert rc == 0, rc
    what = 'wgrad_bn %s relu %d' % (name, relu)
    assert is_sent(buf[n:]), what + ': written behind dw'
    dw = buf[:n].reshape(Co, -1, T.cin_pitch(c))
    same_bits(dw[:, :, :c.Cin].reshape(ref.shape), ref + old, what)
    assert float(dw[:, :, c.Cin:].abs().max() if dw.shape[2] > c.Cin else 0.0) == 0.0, what + ': pad lanes of dw'
    same_bits(dgamma[:Co], 1.0 + 0.5 * sgx, what + ' dgamma')
    same_bits(dbeta[:Co], 1.0 + 0.5 * sg, what + ' dbeta')


def test_conv_wgrad_bn_is_refused_where_the_plan_cannot_carry_it(gpu):
    """a row on the LDS-staged temporal weight gradient (dv_conv3d_wgrad_bn_ok == 0): DV_EUNSUPPORTED, dw untouched"""
    c, dev = T.BY_NAME['tap_tm_m12544'], gpu
    assert c.wgrad.bn_ok == 0
    gen = dev_gen(dev, 1100)
    Co, cp = c.Cout, ops.cp8(c.Cout)
    x, _, g, _ = make_data(c, 'G1', 'fwd', dev, 1101)
    one, zero = torch.ones(cp, device=dev), torch.zeros(cp, device=dev)
    n = Co * c.k[0] * c.k[1] * c.k[2] * T.cin_pitch(c)
    buf = sent((n,), dev)
    rc = _wgrad_bn_call(c, dev, x, g, g1(gen, g.shape, dev), one, zero, one, one, zero, torch.zeros(1, 2, cp, device=dev), 1.0, True, buf,
                        zero.clone(), zero.clone())
    assert rc == -3, rc
    assert is_sent(buf)
