"""The pooling (csrc/pool.hip), self-gating and spatial-mean (csrc/gate.hip), small fp32 helper and ingest kernels (csrc/elementwise.hip) against plain float64
restatements of include/dualvar_hip.h, through the C ABI on explicit tensors, on every launch route of tests/pool_cases.py
(tests/test_abi_and_host.py::test_pool_case_table_routes_and_coverage pins each row to its route without a GPU).

Conventions (those of tests/test_batchnorm_multi_gpu.py; the helpers are tests/checks.py's): gaps of input buffers -- pitch padding,
columns outside a channel slice, the stride between ingest samples, the slack in front of an offset idx -- hold NaN (0xff
bytes for idx); pad lanes [C, CP) of input activations hold zeros, the stated convention for activations; outputs start as a
NaN bit pattern no kernel produces, and after a call everything outside the stated range keeps those bits while pad lanes of
written views are 0.

(A) exactly representable data: every assertion is BIT FOR BIT.
    pool forward      values and uint8 taps == F.max_pool3d(float64, return_indices) with the flat index converted to the tap
                      (dt*kh + dh)*kw + dw, on integers in [-3, 3] whose channels cycle through constant (all taps tie: the
                      first valid tap), all negative, post-ReLU and +-inf (with windows that are entirely -inf), and on
                      Gaussian data (a forward is a selection).  No NaN data: the routes legitimately differ there (the
                      per-element kernels propagate any NaN, the staged keys only rank a NaN with the sign bit clear above
                      +inf, and which of several NaNs is reported differs).
    pool backward     integer gy in [-4, 4] (sum |terms| < 2^8 asserted: exact in bf16 too), plain and DV_ACCUM
    tap order         Gaussian gy: dx == the host's fp32 sum of the contributions in ascending tap order (DV_ACCUM: starting
                      from the old value), rounded once to bf16 in bf16, on the gather, quad and staged routes
    BN+ReLU+pool      forward: values and taps == the pool reference applied to the fp32 operation-by-operation restatement
                      max(x*scale + shift, 0) rounded to storage; dyadic scale (negative and zero channels) and shift (<= 0
                      channels); also on Gaussian data, where the values are in addition bounded against pure float64.
                      backward: sums (replicas added on the host, n_rep 1 and 4), dgamma, dbeta exact; dx exact where M is a
                      power of two.  The ReLU mask is the sign of the fp32 restatement: the forward's definition.
                      fp32, one block: sums, dx, dgamma, dbeta == the two-pass form's (dv_maxpool3d_bwd, then the multi-tensor
                      reduce and apply with DV_MASK_FROM_X), which the fused passes share their arithmetic with.
    means and gates   integer data, S a power of two, dyadic g: exact on every chunk layout and on both rowscale paths (the
                      scalar one forced by C % V != 0 and by a g / dmean table at a 4-byte offset); S = 127 is bounded (1 / S).
    helpers, ingest   dv_relu_bwd_f32, dv_l2norm_fwd on rows of power-of-two norm, the ingest copies: exact.
(B) Gaussian data, derived bounds, u = 2^-24 (bf16 store: + 2^-8 |ref|):
    column sums       |err| <= (L + r) u sum|terms|: L = column_chain() (next to bwd_reduce_chain in
                      tests/chains.py), the longest chain of sequential fp32 additions
                      column_reduce forms (rows per thread + ceil(log2 rg) + blocks per replica for the atomic form), r the
                      roundings inside one term
    dx of dv_bn_bwd_apply_maxpool   the kernel's own expression k1*g + k2*x + k3, k3 = -k1*sg/M - k2*mean:
                      u [(w + 3)|k1| G + 8 |k2| (|x| + |mean|) + 6 |k1 sg / M|], G = sum |gathered gy|, w its windows;
                      one case is ill-centred (|mean| ~ 30 std): the bound carries |k2|(|x| + |mean|), not |k2 (x - mean)|
    elementwise       the stated count of roundings x u x the term magnitudes
    dv_l2norm_*       chain ceil(D / 64) + 6 for the wave sum.  No accuracy figure for sqrtf ships with the project: it is
                      measured here on the device against float64 (norms of two-element rows, 65 536 arguments,
                      2^-40 <= s <= 2^43: test_sqrtf_accuracy_on_the_device).  Measured on the MI355X:
                      max |sqrtf(s) - sqrt(s)| = 0.9999 u sqrt(s) (half an ulp of the result: correctly rounded).  Recorded as
                      SQRT_MEASURED = 1.0 and taken with a factor 2: e_sqrt = 2 u; the test fails above 1.0.

Signed zeros (documented behaviour, include/dualvar_hip.h): the per-element kernels compare values, -0.0 and +0.0 tie and the
first wins; the staged forward orders -0.0 below +0.0 and reports the first +0.0.  test_signed_zeros pins both.

Largest err / bound per quantity, measured on the MI355X (printed by the module fixture under -s), fp32 / bf16:
    bn_apply_maxpool y vs float64 0.425 / 0.981; bn_bwd_reduce_maxpool sum g 0.058 / 0.000 (bf16 gy: exact sums), sum g xhat
    0.042 / 0.034; bn_bwd_apply_maxpool dbeta 0.479, dgamma 0.363, dx 0.395 / 0.993, ill-centred 0.201 / 0.989;
    spatial_mean 0.105 / 0.120; gate_bwd_reduce x_is_output=0 0.109 / 0.097, =1 0.082 / 0.076; gate_scale 1.000 / 0.996;
    gate_bwd_apply 0.987 / 0.996, DV_ACCUM 0.978 / 0.996; spatial_mean_bwd 0.509 / 0.996, DV_ACCUM 0.996 / 0.996;
    dv_ingest_ncdhw normalised 0.707 / 0.892, dv_ingest_ncdhw_pad 0.781 / 0.969; l2norm_fwd norm 0.183, y 0.292; l2norm_bwd dx
    0.614, zero row 0.000 (dy * 2^20 is exact).
    The ratios next to 1 are elementwise outputs whose bound is one to three roundings (or the bf16 store's half ulp) and is
    met on mantissas next to a power of two; the column sums stay an order below their chain bounds.
Seeded faults, each built into a scratch copy of the kernels and run against this file on the MI355X (failing tests):
    `>=` for `>` in maxpool_fwd_kernel's compare: test_pool_forward_values_and_taps (33 cases), test_signed_zeros (2);
    `>=` for `>` in the staged forward's 3x3 compare of one plane: test_pool_forward_values_and_taps (15), test_signed_zeros (2);
    the quad kernel's tap + 1: test_pool_backward_exact_and_in_tap_order (10), test_pool_with_idx_at_a_4_byte_offset (2);
    the channel-chunk grid without its partial last chunk: test_means_and_gates_on_every_chunk_layout (8), and
        test_pool_case_table_routes_and_coverage on the host;
    rowscale_kernel's scalar path without `if (c0 + e >= C) r = 0`: test_scalar_path_writes_zero_pad_lanes_whatever_the_inputs_hold
        (2; with zeros in the inputs' pad lanes the masked table reads alone give the same zeros);
    bn_apply_maxpool_kernel pooling x before the affine map: test_bn_relu_pool_forward (8).
"""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_F32  # noqa: E402
from tests import pool_cases as T  # noqa: E402
from tests.bn_support import DTYPES, Member, make_table  # noqa: E402
from tests.chains import column_chain  # noqa: E402
from tests import checks  # noqa: E402
from tests.checks import (BF16_U, U, Ratios, View, bits, ceil_div, chan, cp8, equal_bits, is_sent, launch,  # noqa: E402
                          report_fixture, sent, vec)
from tests.pool_reference import ref_pool_bwd, ref_pool_fwd  # noqa: E402

IDX_SENT = 0xEE                    # idx bytes before a launch: no tap is that large (kt*kh*kw <= 27 here)
SQRT_MEASURED = 1.0                # max |sqrtf(s) - sqrt(s)| / (u sqrt(s)) on the MI355X: 0.9999 measured (see the docstring)
RATIOS = Ratios()
# bit for bit against float64: the reference must be a number of the storage dtype, and -0 is not +0
same_bits = functools.partial(checks.same_bits, ref_exact_in='storage', signed_zeros=True)


_report = report_fixture(RATIOS, 44)


def tdt(dtype):
    return ops.TORCH_DTYPE[dtype]


def store_u(dtype):
    return 0.0 if dtype == DV_F32 else BF16_U


def rc_of(name, *args):
    return getattr(L.load(), name)(*args, ops.stream_ptr())


def bounded(got, ref, bound, name):
    """the shared bound check, recorded under the whole name"""
    RATIOS.within(got, ref, bound, name, key=name)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def padded(v5, CP):
    """[.., C] -> [.., CP] with zero pad lanes"""
    out = torch.zeros(v5.shape[:-1] + (CP,), dtype=v5.dtype)
    out[..., :v5.shape[-1]] = v5
    return out


class IdxBuf:
    """uint8 [M][CP] tap indices with `lead` bytes in front (0: 8-byte aligned; 4: the misaligned case) and 16 behind"""

    def __init__(self, M, CP, dev, lead=0, taps=None):
        self.n = M * CP
        self.lead = lead
        self.raw = torch.full((8 + self.n + 16,), IDX_SENT if taps is None else 0xFF, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 8 == 0
        if taps is not None:
            self.view()[:] = taps.reshape(-1).to(dev)

    def view(self):
        return self.raw[self.lead:self.lead + self.n]

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lead

    def check_frame(self, what, fill=IDX_SENT):
        assert bool((self.raw[:self.lead] == fill).all()) and bool((self.raw[self.lead + self.n:] == fill).all()), \
            what + ': idx written outside [M][CP]'


def pool_x(c, kind, seed):
    """[N, T, H, W, C] float64 test data (CPU)"""
    g = gen(seed)
    shape = (c.N, c.T, c.H, c.W, c.C)
    if kind == 'gauss':
        return torch.randn(shape, generator=g, dtype=torch.float64)
    x = torch.randint(-3, 4, shape, generator=g).double()
    ch = torch.arange(c.C)
    x[..., ch % 4 == 0] = 2.0                                              # constant: every tap ties
    neg = -torch.randint(1, 4, shape, generator=g).double()
    x[..., ch % 4 == 1] = neg[..., ch % 4 == 1]                            # all negative: -inf padding must lose, 0 must not appear
    x[..., ch % 4 == 2] = x[..., ch % 4 == 2].clamp_min(0)                 # post-ReLU: many ties at 0
    r = torch.rand(shape, generator=g)
    inf = torch.where(r < 0.15, float('inf'), torch.where(r > 0.6, -float('inf'), 0.0)).double()
    m3 = (ch % 4 == 3)
    x[..., m3] = torch.where(inf[..., m3] != 0, inf[..., m3], x[..., m3])
    x[0, ..., ch % 8 == 3] = -float('inf')                                 # sample 0: windows that are entirely -inf
    return x


def run_pool_fwd(c, dtype, dev, x5, what):
    """x5: [N, T, H, W, C] values representable in dtype.  Launch dv_maxpool3d_fwd, check the frames, return (y, idx, refs)"""
    CP = cp8(c.C)
    M_in, M_out = c.N * c.T * c.H * c.W, c.N * math.prod(T.out_dims(c))
    x = View.sliced(dtype, M_in, c.C, dev, c.sliced, x5.reshape(M_in, c.C))
    y = View.sliced(dtype, M_out, c.C, dev, c.sliced)
    idx = IdxBuf(M_out, CP, dev)
    d = T.desc(c, dtype, x.ld, y.ld)
    launch('dv_maxpool3d_fwd', C.byref(d), x.ptr, y.ptr, idx.ptr)
    torch.cuda.synchronize()
    y.check_frame(what)
    idx.check_frame(what)
    return y, idx


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('c', T.POOL_CASES, ids=lambda c: c.name)
def test_pool_forward_values_and_taps(gpu, dtype, kind, c):
    CP = cp8(c.C)
    x5 = pool_x(c, kind, 11).to(tdt(dtype)).double()
    yr, tr = ref_pool_fwd(padded(x5, CP), c)
    yr[..., c.C:] = 0
    y, idx = run_pool_fwd(c, dtype, gpu, x5, c.name)
    if kind == 'int':
        assert bool(torch.isinf(yr[..., :c.C]).any()) or c.C < 4
        assert bool((yr[0][..., 3] == -float('inf')).all()) if c.C > 3 else True
    same_bits(y.cols(), yr.reshape(-1, CP), c.name + ' pooled values')
    got = idx.view().view(-1, CP).cpu()
    ok = got == tr.reshape(-1, CP)
    assert bool(ok.all()), '%s: %d taps differ, first at %s' % (c.name, int((~ok).sum()), (~ok).nonzero()[0].tolist())


def pool_bwd_inputs(c, dtype, kind, seed):
    """taps from the reference forward of Gaussian data (every tap occurs), gy [.., CP] with zero pad lanes, old dx"""
    CP = cp8(c.C)
    g = gen(seed)
    x5 = padded(torch.randn((c.N, c.T, c.H, c.W, c.C), generator=g, dtype=torch.float64), CP)
    x5[..., ::5] = 1.0                                                     # constant channels: first-valid-tap windows
    _, tap = ref_pool_fwd(x5, c)
    oshape = (c.N,) + T.out_dims(c) + (c.C,)
    ishape = (c.N, c.T, c.H, c.W, c.C)
    if kind == 'int':
        gy = torch.randint(-4, 5, oshape, generator=g).double()
        old = torch.randint(-3, 4, ishape, generator=g).double()
    else:
        gy = torch.randn(oshape, generator=g, dtype=torch.float64).to(tdt(dtype)).double()
        old = torch.randn(ishape, generator=g, dtype=torch.float64).to(tdt(dtype)).double()
    return tap, padded(gy, CP), padded(old, CP)


def run_pool_bwd(c, dtype, dev, tap, gy, old, lead=0):
    """dv_maxpool3d_bwd plain (old is None) or DV_ACCUM onto old; returns the dx view"""
    CP = cp8(c.C)
    M_in, M_out = c.N * c.T * c.H * c.W, c.N * math.prod(T.out_dims(c))
    dy = View.sliced(dtype, M_out, c.C, dev, c.sliced, gy.reshape(M_out, CP))
    dx = View.sliced(dtype, M_in, c.C, dev, c.sliced, None if old is None else old.reshape(M_in, CP))
    idx = IdxBuf(M_out, CP, dev, lead, tap)
    d = T.desc(c, dtype, dx.ld, dy.ld)
    launch('dv_maxpool3d_bwd', C.byref(d), dy.ptr, idx.ptr, dx.ptr, 0 if old is None else DV_ACCUM)
    torch.cuda.synchronize()
    dx.check_frame(c.name + ' dx')
    idx.check_frame(c.name, 0xFF)
    return dx


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', T.POOL_CASES, ids=lambda c: c.name)
def test_pool_backward_exact_and_in_tap_order(gpu, dtype, c):
    CP = cp8(c.C)
    # (A) integers: exact whatever the order
    tap, gy, old = pool_bwd_inputs(c, dtype, 'int', 5)
    zero = torch.zeros_like(old)
    ref, cnt, mag = ref_pool_bwd(gy, tap, c, zero)
    lim = 2.0 ** 8 if dtype == DV_BF16 else 2.0 ** 24
    assert float((mag + old.abs()).max()) < lim
    assert int(cnt.max()) >= 1
    if c.name == 'g_222_odd':
        assert int(cnt[:, -1].max()) == 0 and int(cnt[:, :, -1].max()) == 0 and int(cnt[:, :, :, -1].max()) == 0
    same_bits(run_pool_bwd(c, dtype, gpu, tap, gy, None).cols(), ref.reshape(-1, CP), c.name + ' dx')
    ref_acc, _, _ = ref_pool_bwd(gy, tap, c, old)
    same_bits(run_pool_bwd(c, dtype, gpu, tap, gy, old).cols(), ref_acc.reshape(-1, CP), c.name + ' dx (DV_ACCUM)')
    # tap order: the fp32 sum in ascending tap order, rounded once to the storage type
    tap, gy, old = pool_bwd_inputs(c, dtype, 'gauss', 6)
    for o, what in ((None, ' dx, tap order'), (old, ' dx, tap order (DV_ACCUM)')):
        want, _, _ = ref_pool_bwd(gy, tap, c, zero if o is None else o, torch.float32)
        want = want.to(tdt(dtype)).double()
        same_bits(run_pool_bwd(c, dtype, gpu, tap, gy, o).cols(), want.reshape(-1, CP), c.name + what)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [c for c in T.POOL_CASES if c.idx4], ids=lambda c: c.name)
def test_pool_with_idx_at_a_4_byte_offset(gpu, dtype, c):
    """a misaligned idx sends the backward to the gather kernel, which must give the bits of the aligned call (quad / staged);
    the forward refuses it with DV_EALIGN and writes nothing"""
    CP = cp8(c.C)
    assert T.query(c, dtype, 1)[0] in (T.QUAD, T.TILE)
    tap, gy, old = pool_bwd_inputs(c, dtype, 'gauss', 8)
    for o in (None, old):
        a = run_pool_bwd(c, dtype, gpu, tap, gy, o, lead=0)
        b = run_pool_bwd(c, dtype, gpu, tap, gy, o, lead=4)
        assert torch.equal(bits(a.buf), bits(b.buf))
        assert bool(torch.isfinite(a.cols().float()).all()) and float(a.cols().float().abs().max()) > 0
    M_in, M_out = c.N * c.T * c.H * c.W, c.N * math.prod(T.out_dims(c))
    x = View.sliced(dtype, M_in, c.C, gpu, False, pool_x(c, 'gauss', 1).reshape(M_in, c.C))
    y = View.sliced(dtype, M_out, c.C, gpu)
    idx = IdxBuf(M_out, CP, gpu, lead=4)
    d = T.desc(c, dtype, x.ld, y.ld)
    assert rc_of('dv_maxpool3d_fwd', C.byref(d), x.ptr, y.ptr, idx.ptr) == -2
    torch.cuda.synchronize()
    assert is_sent(y.buf) and bool((idx.raw == IDX_SENT).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_signed_zeros(gpu, dtype):
    """-0.0 and +0.0 in one window (include/dualvar_hip.h, MaxPool3d): values compare numerically on every route; the gather
    kernel reports the first zero of either sign, as PyTorch does; the staged forward orders -0.0 below +0.0 and reports the
    first +0.0 -- the DOCUMENTED behaviour of that route (the pools read post-ReLU data, which holds no -0.0)."""
    staged, gather = T.POOL_CASES[0], T.POOL_CASES[1]
    assert T.query(staged, dtype, 0)[0] == T.TILE and T.query(gather, dtype, 0)[0] == T.GATHER
    for c in (staged, gather):
        CP = cp8(c.C)
        x5 = torch.full((c.N, c.T, c.H, c.W, c.C), -0.0, dtype=torch.float64)
        x5[..., 1::2] = -1.0                                # odd channels: -1 everywhere but the two zeros below
        x5[0, 0, 1, 1, :] = -0.0
        x5[0, c.T - 1, 2, 3, :] = 0.0                       # the only +0.0, later in scan order than a -0.0 in every window
        y, idx = run_pool_fwd(c, dtype, gpu, x5, c.name)
        yv = y.cols()[:, :c.C].double().cpu()
        _, first = ref_pool_fwd(padded(x5, CP), c)                             # -0.0 == +0.0: the first of them
        keyed = torch.where((x5 == 0) & torch.signbit(x5), torch.full_like(x5, -1e-300), x5)
        _, plus = ref_pool_fwd(padded(keyed, CP), c)                           # -0.0 below +0.0
        assert not torch.equal(first, plus)
        yr, _ = ref_pool_fwd(padded(x5, CP), c)
        assert torch.equal(yv, yr.reshape(-1, CP)[:, :c.C]), 'values must be numerically equal'
        got = idx.view().view(-1, CP).cpu()
        want = plus if c is staged else first
        assert torch.equal(got[:, :c.C], want.reshape(-1, CP)[:, :c.C]), c.name


# ------------------------------------------------------------------------------------------------------------ BN + ReLU + pool
class BnPool:
    """dv_bn_apply_maxpool / dv_bn_bwd_reduce_maxpool / dv_bn_bwd_apply_maxpool on one case"""

    def __init__(self, c, dtype, dev, exact, seed, ill=False, sliced=True):
        self.sliced = sliced
        self.c, self.dtype, self.dev, self.exact = c, dtype, dev, exact
        g = gen(seed)
        C_, CP = c.C, cp8(c.C)
        self.M = c.N * c.T * c.H * c.W
        self.Mo = c.N * math.prod(T.out_dims(c))
        shape = (c.N, c.T, c.H, c.W, C_)
        pick = lambda vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (C_,), generator=g)]  # noqa: E731
        if exact:
            x = torch.randint(-3, 4, shape, generator=g).double()
            mean = torch.randint(-4, 5, (C_,), generator=g).double() / 4
            invstd = pick([0.5, 1.0, 2.0])
            gamma = pick([-1.5, -0.5, 0.0, 0.5, 1.0, 2.0])
            gamma[:3] = torch.tensor([-0.5, 0.0, 1.0])                    # a negative, a zero and a positive scale at least
            beta = torch.randint(-6, 3, (C_,), generator=g).double() / 4
            mean[2], beta[2] = 0.0, -1.0                                  # a shift <= 0 under a positive scale
            gy = torch.randint(-4, 5, (c.N,) + T.out_dims(c) + (C_,), generator=g).double()
        else:
            sd = 0.5 + torch.rand(C_, generator=g, dtype=torch.float64) * 1.5
            mu = 0.5 * torch.randn(C_, generator=g, dtype=torch.float64) + (30.0 * sd if ill else 0.0)
            x = (torch.randn(shape, generator=g, dtype=torch.float64) * sd + mu).to(tdt(dtype)).double()
            xm = x.reshape(-1, C_)
            mean = xm.mean(0).float().double()
            invstd = (xm.var(0, unbiased=False) + 1e-5).rsqrt().float().double()
            gamma = (1 + 0.3 * torch.randn(C_, generator=g, dtype=torch.float64)).float().double()
            gamma[:2] = torch.tensor([-0.75, 0.0])
            beta = (0.3 * torch.randn(C_, generator=g, dtype=torch.float64)).float().double()
            gy = torch.randn((c.N,) + T.out_dims(c) + (C_,), generator=g, dtype=torch.float64).to(tdt(dtype)).double()
        scale = (gamma * invstd).float().double()
        shift = (beta - mean * scale).float().double()
        if exact:
            assert torch.equal(scale, gamma * invstd) and torch.equal(shift, beta - mean * scale)
            assert bool((scale < 0).any()) and bool((scale == 0).any()) and bool((shift <= 0).any())
        self.x5, self.gy5 = x, gy
        self.mean, self.invstd, self.gamma, self.scale, self.shift = mean, invstd, gamma, scale, shift
        self.x = View.sliced(dtype, self.M, C_, dev, sliced, x.reshape(self.M, C_))
        self.p = {k: chan(v, CP, dev) for k, v in (('mean', mean), ('invstd', invstd), ('gamma', gamma), ('scale', scale),
                                                   ('shift', shift))}
        # the fp32 restatement, one operation at a time (torch on the CPU: two roundings), over the CP lanes the kernel sees
        sc_p, sh_p = (torch.full((CP,), 0.625, dtype=torch.float32) for _ in range(2))
        sc_p[:C_], sh_p[:C_] = scale.float(), shift.float()
        xp = padded(x, CP).float()
        self.pre = xp * sc_p + sh_p                                       # fp32: its sign is the ReLU mask
        self.act = self.pre.clamp_min(0).to(tdt(dtype)).double()         # what dv_bn_apply would have stored
        self.yr, self.tap = ref_pool_fwd(self.act, c)
        self.yr[..., C_:] = 0

    def desc(self, ldy):
        return T.desc(self.c, self.dtype, self.x.ld, ldy)

    def forward(self):
        c, CP = self.c, cp8(self.c.C)
        y = View.sliced(self.dtype, self.Mo, c.C, self.dev, self.sliced)
        idx = IdxBuf(self.Mo, CP, self.dev)
        launch('dv_bn_apply_maxpool', C.byref(self.desc(y.ld)), self.x.ptr, self.p['scale'].data_ptr(), self.p['shift'].data_ptr(),
               y.ptr, idx.ptr)
        torch.cuda.synchronize()
        y.check_frame(c.name)
        idx.check_frame(c.name)
        return y, idx

    def gathered(self):
        """dL/dy at the input elements in float64, the windows per element and sum |gy|; the mask of the restatement"""
        CP = cp8(self.c.C)
        g, cnt, mag = ref_pool_bwd(padded(self.gy5, CP), self.tap, self.c, torch.zeros(self.pre.shape, dtype=torch.float64))
        mask = self.pre > 0
        zero = torch.zeros((), dtype=torch.float64)                       # (+0.0 where masked, as the kernels' gg = 0.f)
        C_ = self.c.C
        return (torch.where(mask, g, zero)[..., :C_].reshape(-1, C_), cnt[..., :C_].reshape(-1, C_),
                torch.where(mask, mag, zero)[..., :C_].reshape(-1, C_))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['exact', 'gauss'])
@pytest.mark.parametrize('c', T.BN_POOL_CASES, ids=lambda c: c.name)
def test_bn_relu_pool_forward(gpu, dtype, kind, c):
    """against the pool of the fp32 restatement -- NOT against a pool of x followed by the affine map, which agrees only for
    scale > 0 (negative and zero scales are in every case)"""
    b = BnPool(c, dtype, gpu, kind == 'exact', 21)
    CP = cp8(c.C)
    y, idx = b.forward()
    same_bits(y.cols(), b.yr.reshape(-1, CP), c.name + ' pooled values')
    got = idx.view().view(-1, CP).cpu()
    assert torch.equal(got, b.tap.reshape(-1, CP)), '%s: %d taps differ' % (c.name, int((got != b.tap.reshape(-1, CP)).sum()))
    # a pool of x mapped afterwards would differ: the data must be able to tell
    wrong, _ = ref_pool_fwd(padded(b.x5, CP), c)
    wrong = (wrong[..., :c.C] * b.scale + b.shift).clamp_min(0)
    assert not torch.equal(wrong.to(tdt(dtype)).double(), b.yr[..., :c.C])
    if kind == 'gauss':
        # against pure float64: x*scale rounds (u |x scale|), the sum rounds (u |y|, y >= 0 the larger of the two), bf16 store
        a64 = (b.x5 * b.scale + b.shift).clamp_min(0)
        y64, _ = ref_pool_fwd(padded(a64, CP), c)
        xs = ref_pool_fwd(padded((b.x5 * b.scale).abs(), CP), c)[0]          # the largest |x scale| of the window: an upper bound
        bound = 2 * U * (xs + y64) + store_u(dtype) * y64
        bounded(y.cols()[:, :c.C].double().cpu(), y64.reshape(-1, CP)[:, :c.C], bound.reshape(-1, CP)[:, :c.C],
                'bn_apply_maxpool y vs float64 [%s]' % ('fp32' if dtype == DV_F32 else 'bf16'))


def run_bn_pool_backward(b, n_rep, dscale, what):
    c, dtype, dev = b.c, b.dtype, b.dev
    C_, CP, M = c.C, cp8(c.C), b.M
    lib = L.load()
    dyp = View.sliced(dtype, b.Mo, C_, dev, b.sliced, b.gy5.reshape(b.Mo, C_))
    idx = IdxBuf(b.Mo, CP, dev, 0, b.tap)
    sums = torch.zeros(n_rep * 2 * CP, dtype=torch.float32, device=dev)
    d = b.desc(dyp.ld)
    launch('dv_bn_bwd_reduce_maxpool', C.byref(d), dyp.ptr, idx.ptr, b.x.ptr, b.p['mean'].data_ptr(), b.p['invstd'].data_ptr(),
           b.p['scale'].data_ptr(), b.p['shift'].data_ptr(), sums.data_ptr(), n_rep)
    torch.cuda.synchronize()
    g, cnt, mag = b.gathered()
    x = b.x5.reshape(-1, C_)
    xhat = (x - b.mean) * b.invstd
    got = sums.view(n_rep, 2, CP).double().sum(0).cpu()                   # the replicas, added on the host
    assert bool((sums.view(n_rep, 2, CP)[:, :, C_:] == 0).all()), what + ': pad lanes of sums written'
    ref = torch.stack([g.sum(0), (g * xhat).sum(0)])
    nblk = int(lib.dv_bn_bwd_blocks(M, C_))
    rpb = ceil_div(M, nblk)
    if b.exact:
        assert float(mag.sum(0).max()) * 64 < 2 ** 24                     # unit of g*xhat: 1/8
        assert torch.equal(got[:, :C_], ref), what + ': sums'
    else:
        w = int(cnt.max())
        Lc = column_chain(rpb, CP, dtype, 2, ceil_div(nblk, n_rep))
        name = 'bn_bwd_reduce_maxpool %s [%s]' % ('%s', 'fp32' if dtype == DV_F32 else 'bf16')
        bounded(got[0, :C_], ref[0], (Lc + w - 1) * U * mag.sum(0), name % 'sum g')
        # one term g * (x - mean) * invstd: the w - 1 additions of the gather, the subtraction, two products.  The subtraction
        # rounds relative to |x - mean| because x and mean are fp32 numbers (Sterbenz or not, one rounding of the difference)
        bounded(got[1, :C_], ref[1], (Lc + w - 1 + 3) * U * (mag * xhat.abs()).sum(0), name % 'sum g xhat')
    # ---- apply: the device's own sums are the input (as for the multi-tensor suite)
    dg0 = torch.arange(C_, dtype=torch.float64) / 4 - 1
    db0 = 2 - torch.arange(C_, dtype=torch.float64) / 8
    dgamma, dbeta = chan(dg0, CP, dev), chan(db0, CP, dev)
    dx = View.sliced(dtype, M, C_, dev, b.sliced)
    inv_count = 1.0 / M
    launch('dv_bn_bwd_apply_maxpool', C.byref(d), dyp.ptr, idx.ptr, b.x.ptr, b.p['mean'].data_ptr(), b.p['invstd'].data_ptr(),
           b.p['gamma'].data_ptr(), b.p['scale'].data_ptr(), b.p['shift'].data_ptr(), sums.data_ptr(), n_rep, inv_count, dscale,
           dgamma.data_ptr(), dbeta.data_ptr(), dx.ptr, dx.ld)
    torch.cuda.synchronize()
    dx.check_frame(what + ' dx')
    assert bool((dgamma[C_:] == 0.625).all()) and bool((dbeta[C_:] == 0.625).all())
    sg, sgx = got[0, :C_], got[1, :C_]
    ic = float(torch.tensor(inv_count, dtype=torch.float32))
    k1 = b.gamma * b.invstd
    k2 = -k1 * b.invstd * sgx * ic
    a = k1 * sg * ic
    k3 = -a - k2 * b.mean
    ref_dx = k1 * g + k2 * x + k3
    got_dx = dx.cols()[:, :C_].double().cpu()
    pow2 = (M & (M - 1)) == 0
    if b.exact:
        assert torch.equal(dbeta[:C_].double().cpu(), db0 + dscale * sg) and torch.equal(dgamma[:C_].double().cpu(), dg0 + dscale * sgx)
    else:
        # the replicas are added in fp32 on the device (n_rep - 1 roundings), the product and the sum round once each
        for nm, t, t0, s in (('dbeta', dbeta, db0, sg), ('dgamma', dgamma, dg0, sgx)):
            rs = sums.view(n_rep, 2, CP)[:, 0 if nm == 'dbeta' else 1, :C_].double().abs().sum(0).cpu()
            bounded(t[:C_], t0 + dscale * s, U * ((n_rep + 1) * dscale * rs + (t0 + dscale * s).abs()), 'bn_bwd_apply_maxpool %s' % nm)
    if b.exact and pow2:
        # every product and sum of the kernel's expression is exact on this data: one rounding, the bf16 store
        same_bits(dx.cols()[:, :C_], ref_dx.to(tdt(dtype)).double(), what + ' dx')
    else:
        w = int(cnt.max())
        rep = (n_rep - 1)                                                  # fp32 additions of the replicas inside sg / sgx
        bound = U * ((w + 3) * k1.abs() * mag + 8 * k2.abs() * (x.abs() + b.mean.abs()) + 6 * a.abs()) + \
            store_u(dtype) * ref_dx.abs()
        if rep:                                                            # sg / sgx as the kernel adds them: sum |replica| scales it
            rs = sums.view(n_rep, 2, CP).double().abs().sum(0).cpu()[:, :C_]
            bound = bound + U * rep * (k1.abs() * rs[0] * ic + (k1 * b.invstd).abs() * rs[1] * ic * (x.abs() + b.mean.abs()))
        bounded(got_dx, ref_dx, bound,
                'bn_bwd_apply_maxpool dx [%s]%s' % ('fp32' if dtype == DV_F32 else 'bf16', ' ill-centred' if 'ill' in what else ''))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n_rep', [1, 4])
@pytest.mark.parametrize('c', T.BN_POOL_CASES, ids=lambda c: c.name)
def test_bn_relu_pool_backward_exact(gpu, dtype, n_rep, c):
    b = BnPool(c, dtype, gpu, True, 31)
    for dscale in (1.0, 0.5):
        run_bn_pool_backward(b, n_rep, dscale, '%s n_rep %d' % (c.name, n_rep))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ill', [False, True], ids=['centred', 'ill-centred'])
@pytest.mark.parametrize('c', T.BN_POOL_CASES, ids=lambda c: c.name)
def test_bn_relu_pool_backward_bounds(gpu, dtype, ill, c):
    b = BnPool(c, dtype, gpu, False, 41, ill=ill)
    for n_rep in (1, 4):
        run_bn_pool_backward(b, n_rep, 1.0, '%s%s n_rep %d' % (c.name, ' ill' if ill else '', n_rep))


# M = 32 rows: dv_bn_bwd_blocks gives one block, so the atomics of both forms add onto zero once and no order is left open
_ONE_BLOCK = [T._pc('bnp_133_one_block', 1, 2, 4, 4, 5, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
              T._pc('bnp_333s2_one_block', 1, 2, 4, 4, 5, T.K333, (2, 2, 2), T.P1)]


@pytest.mark.parametrize('c', _ONE_BLOCK, ids=lambda c: c.name)
def test_pooled_bn_backward_equals_two_pass_bits(gpu, c):
    """dv_bn_bwd_reduce_maxpool + dv_bn_bwd_apply_maxpool against the two passes they replace, bit for bit: dv_maxpool3d_bwd into
    a dy buffer, then dv_bn_bwd_reduce_multi + dv_bn_bwd_apply_multi over one DV_MASK_FROM_X member with red_ws = NULL.  fp32
    only: there the pool's gradient is stored unrounded, summed in the same ascending tap order (bf16 would round dy between)."""
    dtype, lib = DV_F32, L.load()
    C_, CP = c.C, cp8(c.C)
    M, Mo = c.N * c.T * c.H * c.W, c.N * math.prod(T.out_dims(c))
    assert M <= 32 and int(lib.dv_bn_bwd_blocks(M, C_)) == 1 and C_ % 8
    m = Member(gpu, dtype, M, C_, 51, exact=False, from_x=True)
    m.red_ws = torch.empty(0, dtype=torch.float32, device=gpu)               # the item's red_ws = NULL: sums by atomics
    assert m.red_ws.data_ptr() == 0
    m.sums[0].zero_()
    dyp = View.sliced(dtype, Mo, C_, gpu, False, torch.randn((Mo, C_), generator=gen(52), dtype=torch.float64))
    # taps of the fused forward on the member's own x
    y, idx = View.sliced(dtype, Mo, C_, gpu), IdxBuf(Mo, CP, gpu)
    par = {k: m.p[k].data_ptr() for k in m.p}
    launch('dv_bn_apply_maxpool', C.byref(T.desc(c, dtype, m.x.ld, y.ld)), m.x.ptr, par['scale'], par['shift'], y.ptr, idx.ptr)
    # fused (first: the two-pass form below adds onto the same dgamma / dbeta values)
    sums = torch.zeros(2 * CP, dtype=torch.float32, device=gpu)
    dgamma, dbeta = m.dgamma.clone(), m.dbeta.clone()
    dx = View.sliced(dtype, M, C_, gpu)
    d = T.desc(c, dtype, m.x.ld, dyp.ld)
    launch('dv_bn_bwd_reduce_maxpool', C.byref(d), dyp.ptr, idx.ptr, m.x.ptr, par['mean'], par['invstd'], par['scale'], par['shift'],
           sums.data_ptr(), 1)
    launch('dv_bn_bwd_apply_maxpool', C.byref(d), dyp.ptr, idx.ptr, m.x.ptr, par['mean'], par['invstd'], par['gamma'], par['scale'],
           par['shift'], sums.data_ptr(), 1, 1.0 / M, m.dscale, dgamma.data_ptr(), dbeta.data_ptr(), dx.ptr, dx.ld)
    # two passes
    launch('dv_maxpool3d_bwd', C.byref(T.desc(c, dtype, m.dy.ld, dyp.ld)), dyp.ptr, idx.ptr, m.dy.ptr, 0)
    tab, ends = make_table([m], lib, gpu, dtype)
    assert ends['red'] == 1 and ends['bapply'] == 1
    launch('dv_bn_bwd_reduce_multi', dtype, tab.data_ptr(), 1, 1)
    launch('dv_bn_bwd_apply_multi', dtype, tab.data_ptr(), 1, 1, C_)
    torch.cuda.synchronize()
    idx.check_frame(c.name)
    for v, what in ((m.dy, 'two-pass dy'), (m.dx, 'two-pass dx'), (dx, 'fused dx')):
        v.check_frame('%s %s' % (c.name, what))                               # zeros in the pad lanes
    # the data can tell: gathered gradient passes the mask in every channel (a pool picks a masked element only from a window
    # of zeros, so little is dropped), and both sums of every channel are nonzero
    s2, act = m.sums[0], m.x.val() * m.scale + m.shift
    assert bool(((m.dy.val() != 0) & (act > 0)).any(0).all()) and bool((s2[:C_] != 0).all()) and bool((s2[CP:CP + C_] != 0).all())
    for got, want, what in ((sums, s2, 'sums'), (dx.cols(), m.dx.cols(), 'dx'), (dgamma, m.dgamma, 'dgamma'), (dbeta, m.dbeta, 'dbeta')):
        assert equal_bits(got, want), '%s: %s of the fused and the two-pass form differ' % (c.name, what)
    assert bool((sums.view(2, CP)[:, C_:] == 0).all()), c.name + ': pad lanes of the sums'
    assert bool((dgamma[C_:] == 0.625).all()) and bool((dbeta[C_:] == 0.625).all()), c.name + ': pad lanes of dgamma / dbeta'
    assert not torch.equal(dgamma[:C_], chan(m.dg0, CP, gpu)[:C_])


# ------------------------------------------------------------------------------------------------------------ means and gates
def gate_data(N, S, C_, dtype, exact, seed):
    g = gen(seed)
    M = N * S
    if exact:
        x = torch.randint(-2, 3, (M, C_), generator=g).double()
        dy = torch.randint(-2, 3, (M, C_), generator=g).double()
        old = torch.randint(-2, 3, (M, C_), generator=g).double()
        gate = torch.randint(0, 5, (N, C_), generator=g).double() / 4
        dm = torch.randint(-4, 5, (N, C_), generator=g).double() * (S / 4 if S & (S - 1) == 0 else 1.0)
    else:
        x, dy, old = (torch.randn((M, C_), generator=g, dtype=torch.float64).to(tdt(dtype)).double() for _ in range(3))
        gate = torch.sigmoid(torch.randn((N, C_), generator=g, dtype=torch.float64)).float().double()
        dm = (4 * torch.randn((N, C_), generator=g, dtype=torch.float64)).float().double()
    return x, dy, old, gate, dm


def table(vals, dev, lead=0):
    """a [N][C] fp32 table, pitch C, `lead` floats of NaN in front (1: a 4-byte offset) and 8 behind; returns (tensor, ptr)"""
    t = torch.full((lead + vals.numel() + 8,), float('nan'), dtype=torch.float32, device=dev)
    t[lead:lead + vals.numel()] = vals.reshape(-1).float().to(dev)
    return t, t.data_ptr() + 4 * lead


def run_means_and_gates(dev, dtype, N, S, C_, exact, lead, tag, nan_pads=False):
    """all five entries on one layout; exact: bit for bit when S is a power of two, else (and for Gaussian data) bounded.
    nan_pads: the pad lanes [C, CP) of the INPUT views hold NaN instead of zeros (see the test that sets it)"""
    M, CP = N * S, cp8(C_)
    pow2 = S & (S - 1) == 0
    bit = exact and pow2
    dn = 'fp32' if dtype == DV_F32 else 'bf16'
    x, dy, old, gate, dm = gate_data(N, S, C_, dtype, exact, 3 + N + S + C_)
    rows = torch.arange(M) // S
    xv, dyv = View.sliced(dtype, M, C_, dev, True, x), View.sliced(dtype, M, C_, dev, False, dy, pitch_pad=8)
    if nan_pads:
        xv.buf[:, xv.off + C_:xv.off + CP] = float('nan')
        dyv.buf[:, dyv.off + C_:dyv.off + CP] = float('nan')
    lead_g, lead_dm = lead if isinstance(lead, tuple) else (lead, lead)
    gt, gp = table(gate, dev, lead_g)
    dt_, dp = table(dm, dev, lead_dm)
    su = store_u(dtype)
    invS = float(torch.tensor(1.0, dtype=torch.float32) / S)
    # a chunk is ceil(CV / chunks) vectors wide and the last one may be narrower: the longer chain of the two widths
    CV, chunks = CP // vec(dtype), int(L.load().dv_spatial_chunks(dtype, N, S, C_))
    ccv = ceil_div(CV, chunks)
    Lc = max(column_chain(S, w * vec(dtype), dtype, 1) for w in {ccv, CV - (chunks - 1) * ccv} if w > 0)

    def out_table():
        return sent((N * C_ + 8,), dev)

    def elementwise(name, got_view, ref, bound):
        got_view.check_frame(name)
        if bit:
            same_bits(got_view.cols()[:, :C_], ref, '%s %s' % (tag, name))
        else:
            bounded(got_view.cols()[:, :C_], ref, bound + su * ref.abs(), '%s [%s]' % (name, dn))

    def tab(name, got, ref, bound):
        assert is_sent(got[N * C_:]), name + ': wrote behind the [N][C] table'
        if bit:
            same_bits(got[:N * C_].view(N, C_), ref, '%s %s' % (tag, name))
        else:
            bounded(got[:N * C_].view(N, C_), ref, bound, '%s [%s]' % (name, dn))

    # dv_spatial_mean: the sum, then * fl(1 / S)
    out = out_table()
    launch('dv_spatial_mean', dtype, xv.ptr, xv.ld, N, S, C_, out.data_ptr())
    torch.cuda.synchronize()
    xs = x.view(N, S, C_)
    tab('spatial_mean', out, xs.mean(1), ((0 if exact else Lc) + 2) * U * xs.abs().mean(1))
    # dv_gate_bwd_reduce, both forms
    for xio in (0, 1):
        out = out_table()
        launch('dv_gate_bwd_reduce', dtype, dyv.ptr, dyv.ld, xv.ptr, xv.ld, gp, N, S, C_, out.data_ptr(), xio)
        torch.cuda.synchronize()
        prod = (dy * x).view(N, S, C_)
        f = (1 - gate) if xio else gate * (1 - gate)
        # one rounding per product, the chain, then 1 - g, (g * .), the final product
        tab('gate_bwd_reduce x_is_output=%d' % xio, out, prod.sum(1) * f, (Lc + 1 + 3) * U * prod.abs().sum(1) * f.abs())
    # dv_gate_scale
    y = View.sliced(dtype, M, C_, dev, True)
    launch('dv_gate_scale', dtype, xv.ptr, xv.ld, gp, N, S, C_, y.ptr, y.ld)
    torch.cuda.synchronize()
    elementwise('gate_scale', y, x * gate[rows], U * (x * gate[rows]).abs())
    # dv_gate_bwd_apply and dv_spatial_mean_bwd, plain and DV_ACCUM
    for o in (None, old):
        fl = 0 if o is None else DV_ACCUM
        sfx = '' if o is None else ' (DV_ACCUM)'
        dx = View.sliced(dtype, M, C_, dev, True, o)
        launch('dv_gate_bwd_apply', dtype, dyv.ptr, dyv.ld, gp, dp, N, S, C_, dx.ptr, dx.ld, fl)
        torch.cuda.synchronize()
        t1, t2 = dy * gate[rows], dm[rows] / S
        r = t1 + t2
        bnd = U * (2 * t1.abs() + 3 * t2.abs()) + (0 if o is None else U * (o.abs() + r.abs()))
        elementwise('gate_bwd_apply' + sfx, dx, r if o is None else o + r, bnd)
        dx = View.sliced(dtype, M, C_, dev, False, o, pitch_pad=8)
        launch('dv_spatial_mean_bwd', dtype, dp, N, S, C_, dx.ptr, dx.ld, fl)
        torch.cuda.synchronize()
        elementwise('spatial_mean_bwd' + sfx, dx, t2 if o is None else o + t2, 2 * U * t2.abs() + (0 if o is None else U * (o.abs() + t2.abs())))
    assert abs(invS * S - 1) < 1e-6


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'gauss'])
@pytest.mark.parametrize('cc', T.CHUNK_CASES, ids=lambda c: c.name)
def test_means_and_gates_on_every_chunk_layout(gpu, dtype, exact, cc):
    C_ = cc.C[0 if dtype == DV_F32 else 1]
    assert int(L.load().dv_spatial_chunks(dtype, cc.N, cc.S, C_)) == cc.chunks
    run_means_and_gates(gpu, dtype, cc.N, cc.S, C_, exact, 0, cc.name)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lead', [(1, 1), (1, 0), (0, 1)], ids=['g+dmean', 'g-only', 'dmean-only'])
def test_gate_tables_at_a_4_byte_offset_take_the_scalar_path(gpu, dtype, lead):
    """C % V == 0 but g and / or dmean are not 16-byte aligned: rowscale_kernel's scalar path, same exact results.  Each
    table is also offset alone: dv_gate_bwd_apply reads both, and either alignment clause alone selects the scalar reads"""
    cc = [c for c in T.CHUNK_CASES if c.tag == 'CV<=16'][0]
    C_ = cc.C[0 if dtype == DV_F32 else 1]
    assert C_ % vec(dtype) == 0
    run_means_and_gates(gpu, dtype, cc.N, cc.S, C_, True, lead, cc.name + ' +4 bytes %s' % (lead,))


@pytest.mark.parametrize('dtype', DTYPES)
def test_scalar_path_writes_zero_pad_lanes_whatever_the_inputs_hold(gpu, dtype):
    """C % V != 0 with NaN in the pad lanes of x and dy: rowscale_kernel's scalar path masks its table reads AND its results
    by c0 + e < C, so the pad lanes of y / dx are still zeros and the reductions still write columns [0, C) only.  (With the
    conventional zeros in the inputs' pad lanes either of the two masks hides the loss of the other.)"""
    cc = [c for c in T.CHUNK_CASES if c.tag == 'C%V!=0'][0]
    C_ = cc.C[0 if dtype == DV_F32 else 1]
    assert C_ % vec(dtype) != 0
    run_means_and_gates(gpu, dtype, cc.N, cc.S, C_, True, 0, cc.name + ' NaN pads', nan_pads=True)


def bn_items(members, dev):
    arr = (L.BnItem * len(members))()
    for it, m in zip(arr, members):
        it.x, it.ldx, it.y, it.ldy = m['x'].ptr, m['x'].ld, m['y_ptr'], m['ldy']
        it.scale, it.shift, it.C, it.M = m['scale'].data_ptr(), m['shift'].data_ptr(), m['C'], m['M']
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gate_fold_level_against_float64(gpu, dtype):
    """dv_gate_mean_bn / dv_gate_scale_bn on the Ct = 256 level (chunked: grid.y = 4 / 2) against float64 of the header's
    definition -- tests/test_gate_fold_gpu.py compares them with kernels that share column_reduce"""
    gl = T.GATE_LEVEL
    N, S, Ct = gl['N'], gl['S'], gl['Ct']
    M = N * S
    assert int(L.load().dv_spatial_chunks(dtype, N, S, Ct)) == gl['chunks'][0 if dtype == DV_F32 else 1] > 1
    g = gen(77)
    cat = sent((M, Ct + 16), gpu, dtype)
    members, refs, off = [], [], 0
    for k, w in enumerate(gl['widths']):
        x = torch.randint(-3, 4, (M, w), generator=g).double()
        scale = torch.tensor([-1.0, 0.0, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 5, (w,), generator=g)]
        shift = torch.randint(-4, 5, (w,), generator=g).double() / 4
        members.append(dict(x=View.sliced(dtype, M, w, gpu, k in gl['sliced'], x), scale=chan(scale, w, gpu), shift=chan(shift, w, gpu),
                            C=w, M=M, y_ptr=cat.data_ptr() + off * cat.element_size(), ldy=cat.shape[1]))
        refs.append((x * scale + shift).clamp_min(0))
        off += w
    act = torch.cat(refs, 1)
    offs = [sum(gl['widths'][:k]) for k in range(4)]
    gate_off = torch.tensor(offs, dtype=torch.int32, device=gpu)
    tab = bn_items(members, gpu)
    mean = sent((N * Ct + 8,), gpu)
    launch('dv_gate_mean_bn', dtype, tab.data_ptr(), 4, gate_off.data_ptr(), N, S, Ct, mean.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(cat) and is_sent(mean[N * Ct:])
    same_bits(mean[:N * Ct].view(N, Ct), act.view(N, S, Ct).mean(1), 'gate_mean_bn')
    gate = torch.randint(0, 5, (N, Ct), generator=g).double() / 4
    gt = gate.float().to(gpu)
    launch('dv_gate_scale_bn', dtype, tab.data_ptr(), 4, gate_off.data_ptr(), gt.data_ptr(), N, S, Ct)
    torch.cuda.synchronize()
    assert is_sent(cat[:, Ct:])
    same_bits(cat[:, :Ct], act * gate[torch.arange(M) // S], 'gate_scale_bn')


# ------------------------------------------------------------------------------------------------------------ small helpers
def test_sqrtf_accuracy_on_the_device(gpu):
    """the figure the l2norm bounds take.  The norm of a two-element row is sqrtf(s) with s = fl(fl(a*a) + fl(b*b)) -- the other
    lanes of the wave sum add zeros, so the host forms the same s with three fp32 operations -- against float64 sqrt(s)"""
    g = gen(5)
    R = 1 << 16
    x = (torch.rand((R, 2), generator=g, dtype=torch.float64) + 1) * 2.0 ** torch.randint(-20, 21, (R, 2), generator=g).double()
    x = x.float()
    sq = x * x
    s = (sq[:, 0] + sq[:, 1]).double()
    xd = x.to(gpu)
    y, nrm = sent((2 * R,), gpu), sent((R,), gpu)
    launch('dv_l2norm_fwd', xd.data_ptr(), R, 2, 1e-12, y.data_ptr(), nrm.data_ptr())
    torch.cuda.synchronize()
    rel = ((nrm.double().cpu() - s.sqrt()).abs() / (U * s.sqrt())).max()
    print('\n    sqrtf on the device: max |err| / (u sqrt(s)) = %.4f over %d arguments in [2^-40, 2^43]' % (float(rel), R))
    RATIOS['sqrtf measured / SQRT_MEASURED'] = float(rel) / SQRT_MEASURED
    assert float(rel) <= SQRT_MEASURED, 'sqrtf is less accurate than the figure the l2norm bounds were derived with'


L2_SHAPES = [(R, D) for R in (1, 10, 11) for D in (7, 64, 100, 2048)]


@pytest.mark.parametrize('R,D', L2_SHAPES)
def test_l2norm(gpu, R, D):
    eps = 2.0 ** -20
    g = gen(R * 31 + D)
    Lc = ceil_div(D, 64) + 6
    e_sqrt = 2 * SQRT_MEASURED * U
    # (A) rows of power-of-two norm: 4^k entries of one power of two; row 0 is zero
    k = {7: 1, 64: 3, 100: 3, 2048: 5}[D]
    x = torch.zeros(R, D, dtype=torch.float64)
    for r in range(1, R):
        pos = torch.randperm(D, generator=g)[:4 ** k]
        sgn = torch.randint(0, 2, (4 ** k,), generator=g).double() * 2 - 1
        x[r, pos] = sgn * 2.0 ** (r % 5 - 3)
    xd = x.float().to(gpu)
    y, nrm = sent((R * D + 8,), gpu), sent((R + 8,), gpu)
    launch('dv_l2norm_fwd', xd.data_ptr(), R, D, eps, y.data_ptr(), nrm.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(y[R * D:]) and is_sent(nrm[R:])
    n_ref = x.pow(2).sum(1).sqrt().clamp_min(eps)
    assert all(math.frexp(float(v))[0] == 0.5 for v in n_ref)
    same_bits(nrm[:R], n_ref, 'l2norm_fwd norm')
    same_bits(y[:R * D].view(R, D), x / n_ref[:, None], 'l2norm_fwd y')
    assert float(nrm[0]) == eps and not bool(y[:D].any())
    # the zero row backward: finite, dy * (1 / eps) within 2u
    dy = torch.randn(R, D, generator=g, dtype=torch.float64).float().double()
    dx = sent((R * D + 8,), gpu)
    dyd = dy.float().to(gpu)
    launch('dv_l2norm_bwd', dyd.data_ptr(), y.data_ptr(), nrm.data_ptr(), R, D, dx.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(dx[R * D:]) and bool(torch.isfinite(dx[:R * D]).all())
    bounded(dx[:D], dy[0] / eps, 2 * U * (dy[0] / eps).abs(), 'l2norm_bwd zero row')
    # (B) Gaussian rows
    x = torch.randn(R, D, generator=g, dtype=torch.float64).float().double() * 2.0 ** torch.randint(-3, 4, (R, 1), generator=g).double()
    xd = x.float().to(gpu)
    y, nrm = sent((R * D,), gpu), sent((R,), gpu)
    launch('dv_l2norm_fwd', xd.data_ptr(), R, D, eps, y.data_ptr(), nrm.data_ptr())
    torch.cuda.synchronize()
    n_ref = x.pow(2).sum(1).sqrt()
    # s: one rounding per square + the chain, all terms positive: relative (Lc + 1) u; sqrt halves it and adds its own error
    rel_n = (Lc + 1) * U / 2 + e_sqrt
    bounded(nrm, n_ref, rel_n * n_ref, 'l2norm_fwd norm')
    bounded(y.view(R, D), x / n_ref[:, None], (rel_n + U) * (x / n_ref[:, None]).abs(), 'l2norm_fwd y')
    # backward on the device's own y and norm: s = <dy, y>, inv = 1 / norm, dx = (dy - y*s) * inv
    yv, nv = y.view(R, D).double().cpu(), nrm.double().cpu()
    s = (dy * yv).sum(1, keepdim=True)
    sa = (dy * yv).abs().sum(1, keepdim=True)
    ys = (yv * s).abs()
    ref = (dy - yv * s) / nv[:, None]
    bound = (yv.abs() * (Lc + 1) * U * sa + U * ys + 3 * U * (dy.abs() + ys)) / nv[:, None]
    dx = sent((R * D,), gpu)
    launch('dv_l2norm_bwd', dyd.data_ptr(), y.data_ptr(), nrm.data_ptr(), R, D, dx.data_ptr())
    torch.cuda.synchronize()
    bounded(dx.view(R, D), ref, bound, 'l2norm_bwd dx')


def test_relu_bwd_small(gpu):
    g = gen(9)
    n = 1000
    dy = torch.randn(n, generator=g)
    y = torch.randn(n, generator=g).clamp_min(0)
    y[::7] = -0.0
    dx = sent((n + 8,), gpu)
    dyd, yd = dy.to(gpu), y.to(gpu)
    launch('dv_relu_bwd_f32', dyd.data_ptr(), yd.data_ptr(), n, dx.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(dx[n:])
    same_bits(dx[:n], torch.where(y > 0, dy, torch.zeros(())).double(), 'relu_bwd')


# ------------------------------------------------------------------------------------------------------------ ingest
INGEST_CASES = [
    # C, ldy, pad, n_seg (0: no perm), extra stride, mean
    (3, 4, 0, 0, 0, False), (3, 8, 3, 2, 5, False), (1, 4, 3, 4, 0, False), (1, 8, 0, 1, 7, False),
    (3, 4, 3, 4, 3, True), (1, 8, 0, 2, 0, True),
]


def run_ingest(dev, dtype, N, C_, T_, H, W, ldy, pad, n_seg, extra, with_mean, seed, padded_entry):
    g = gen(seed)
    sxn = C_ * T_ * H * W + extra
    xbuf = torch.full((N * sxn + 4,), float('nan'), dtype=torch.float32)
    x = torch.randn(N, C_, T_, H, W, generator=g)
    for n in range(N):
        xbuf[n * sxn:n * sxn + C_ * T_ * H * W] = x[n].reshape(-1)
    xd = xbuf.to(dev)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    y = sent((N * T_, Hp, Wp, ldy), dev, dtype)
    perm = None
    src = x
    if n_seg:
        perm = torch.stack([torch.roll(torch.arange(n_seg), n + 1) for n in range(N)]).to(torch.int32)
        seg = T_ // n_seg
        ts = (perm.long()[:, torch.arange(T_) // seg] * seg + torch.arange(T_) % seg)
        src = torch.stack([x[n][:, ts[n]] for n in range(N)])
        assert n_seg == 1 or not torch.equal(src, x)
    mean = istd = None
    ref = src.double()
    bound = torch.zeros_like(ref)
    if with_mean:
        mean, istd = torch.tensor([0.4, -0.3, 0.2, 9.0]), torch.tensor([2.1, 0.7, 1.3, 9.0])
        m, s = mean[:C_].double().view(1, C_, 1, 1, 1), istd[:C_].double().view(1, C_, 1, 1, 1)
        bound = 2 * U * (ref.abs() + m.abs()) * s.abs()
        ref = (ref - m) * s
    pd = perm.to(dev) if perm is not None else None
    md, sd = (mean.to(dev), istd.to(dev)) if with_mean else (None, None)
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    args = (dtype, xd.data_ptr(), y.data_ptr(), N, C_, T_, H, W, sxn, ldy, p(md), p(sd), p(pd), n_seg)
    if padded_entry:
        launch('dv_ingest_ncdhw_pad', *args, pad)
    else:
        assert pad == 0
        launch('dv_ingest_ncdhw', *args)
    torch.cuda.synchronize()
    inner = y[:, pad:pad + H, pad:pad + W]
    got = inner[..., :C_].reshape(N, T_, H, W, C_).permute(0, 4, 1, 2, 3)
    name = 'ingest' + ('_pad' if padded_entry else '')
    if with_mean:
        bounded(got, ref, bound + store_u(dtype) * ref.abs(), '%s normalised [%s]' % (name, 'fp32' if dtype == DV_F32 else 'bf16'))
    else:
        want = src.to(tdt(dtype))                          # fp32: the bits; bf16: torch's round-to-nearest-even cast
        assert torch.equal(bits(got.contiguous().cpu()), bits(want.contiguous())), name + ': not a bit-exact copy / RNE cast'
    assert bool((inner[..., C_:4] == 0).all()), name + ': lanes [C, 4) not zero'
    assert is_sent(inner[..., 4:]), name + ': lanes [4, ldy) written'
    if pad:
        border = torch.ones((Hp, Wp), dtype=torch.bool, device=dev)
        border[pad:pad + H, pad:pad + W] = False
        assert is_sent(y[:, border]), name + ': the border was written'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', INGEST_CASES, ids=lambda c: 'c%d_ld%d_pad%d_seg%d_x%d_%s' % (c[:5] + ('mean' if c[5] else 'copy',)))
def test_ingest(gpu, dtype, case):
    C_, ldy, pad, n_seg, extra, with_mean = case
    N, T_, H, W = 2, 4, 5, 7
    assert n_seg in (0, 1, 2, T_)
    run_ingest(gpu, dtype, N, C_, T_, H, W, ldy, pad, n_seg, extra, with_mean, 13, True)
    if pad == 0:
        run_ingest(gpu, dtype, N, C_, T_, H, W, ldy, 0, n_seg, extra, with_mean, 13, False)


def test_ingest_refuses_segments_that_do_not_divide_t(gpu):
    x = torch.zeros(2 * 3 * 4 * 5 * 7, device=gpu)
    y = sent((8, 5, 7, 4), gpu, DV_F32)
    perm = torch.zeros(2, 3, dtype=torch.int32, device=gpu)
    args = (DV_F32, x.data_ptr(), y.data_ptr(), 2, 3, 4, 5, 7, 3 * 4 * 5 * 7, 4, 0, 0, perm.data_ptr(), 3)
    assert rc_of('dv_ingest_ncdhw', *args) == -1 and rc_of('dv_ingest_ncdhw_pad', *args, 0) == -1
    torch.cuda.synchronize()
    assert is_sent(y)


# ------------------------------------------------------------------------------------------------------------ grid wrap
def _over_cap(name):
    assert T.wrap_items(name) > T.WRAP_CAPS[name] * 256


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_grid_wrap_rowscale(gpu, mode):
    """more vectors than 4096 blocks x 256 threads: the grid-stride loop wraps, with a ragged last pass"""
    _over_cap('rowscale%d' % mode)
    w = T.WRAP_ROWSCALE
    N, S, C_ = w['N'], w['S'], w['C']
    M = N * S
    x, dy, old, gate, dm = gate_data(N, S, C_, DV_F32, True, 50 + mode)
    rows = torch.arange(M) // S
    gt, dmt = gate.float().to(gpu), dm.float().to(gpu)
    a = View.sliced(DV_F32, M, C_, gpu, False, x)
    o = View.sliced(DV_F32, M, C_, gpu, False, old if mode else None)
    if mode == 0:
        launch('dv_gate_scale', DV_F32, a.ptr, a.ld, gt.data_ptr(), N, S, C_, o.ptr, o.ld)
        ref = x * gate[rows]
    elif mode == 1:
        launch('dv_gate_bwd_apply', DV_F32, a.ptr, a.ld, gt.data_ptr(), dmt.data_ptr(), N, S, C_, o.ptr, o.ld, DV_ACCUM)
        ref = old + x * gate[rows] + dm[rows] / S
    else:
        launch('dv_spatial_mean_bwd', DV_F32, dmt.data_ptr(), N, S, C_, o.ptr, o.ld, DV_ACCUM)
        ref = old + dm[rows] / S
    torch.cuda.synchronize()
    same_bits(o.buf, ref, 'rowscale mode %d over the cap' % mode)


def test_grid_wrap_relu_bwd(gpu):
    _over_cap('relu_bwd')
    n = T.WRAP_RELU_N
    g = gen(3)
    dy = torch.randint(-4, 5, (n,), generator=g).float()
    y = torch.randint(-1, 2, (n,), generator=g).float()
    dx = sent((n + 8,), gpu)
    dyd, yd = dy.to(gpu), y.to(gpu)
    launch('dv_relu_bwd_f32', dyd.data_ptr(), yd.data_ptr(), n, dx.data_ptr())
    torch.cuda.synchronize()
    assert is_sent(dx[n:])
    same_bits(dx[:n], torch.where(y > 0, dy, torch.zeros(())).double(), 'relu_bwd over the cap')


def test_grid_wrap_ingest(gpu):
    _over_cap('ingest')
    w = T.WRAP_INGEST
    run_ingest(gpu, DV_F32, w['N'], w['C'], w['T'], w['H'], w['W'], 4, 0, 0, 0, False, 17, False)
    run_ingest(gpu, DV_F32, w['N'], w['C'], w['T'], w['H'], w['W'], 4, 0, 2, 0, False, 18, True)


def _int_pool_x(c, seed):
    return torch.randint(-3, 4, (c.N, c.T, c.H, c.W, c.C), generator=gen(seed)).double()


def test_grid_wrap_pool_forward_gather(gpu):
    _over_cap('pool_fwd_gather')
    c = T.WRAP_POOLS['pool_fwd_gather']
    assert T.query(c, DV_F32, 0)[0] == T.GATHER
    x5 = _int_pool_x(c, 1)
    yr, tr = ref_pool_fwd(x5, c)
    y, idx = run_pool_fwd(c, DV_F32, gpu, x5, c.name)
    same_bits(y.buf, yr.reshape(-1, c.C), c.name)
    assert torch.equal(idx.view().cpu(), tr.reshape(-1))


@pytest.mark.parametrize('name', ['pool_bwd_gather', 'pool_bwd_quad'])
def test_grid_wrap_pool_backward(gpu, name):
    _over_cap(name)
    c = T.WRAP_POOLS[name]
    assert T.query(c, DV_F32, 1)[0] == (T.GATHER if name == 'pool_bwd_gather' else T.QUAD)
    g = gen(2)
    _, tap = ref_pool_fwd(_int_pool_x(c, 2), c)
    gy = torch.randint(-4, 5, tap.shape, generator=g).double()
    # float64 scatter: input element of each (window, tap)
    To, Ho, Wo = T.out_dims(c)
    tp = tap.long()
    dt, dh, dw = tp // (c.k[1] * c.k[2]), (tp // c.k[2]) % c.k[1], tp % c.k[2]
    it = torch.arange(To).view(1, To, 1, 1, 1) * c.s[0] - c.p[0] + dt
    ih = torch.arange(Ho).view(1, 1, Ho, 1, 1) * c.s[1] - c.p[1] + dh
    iw = torch.arange(Wo).view(1, 1, 1, Wo, 1) * c.s[2] - c.p[2] + dw
    flat = (((torch.arange(c.N).view(c.N, 1, 1, 1, 1) * c.T + it) * c.H + ih) * c.W + iw) * c.C + torch.arange(c.C)
    ref = torch.zeros(c.N * c.T * c.H * c.W * c.C, dtype=torch.float64).index_add_(0, flat.reshape(-1), gy.reshape(-1))
    dx = run_pool_bwd(c, DV_F32, gpu, tap, gy, None)
    same_bits(dx.buf, ref.view(-1, c.C), c.name)


def test_grid_wrap_bn_relu_pool_forward(gpu):
    _over_cap('bn_apply_maxpool')
    b = BnPool(T.WRAP_POOLS['bn_apply_maxpool'], DV_F32, gpu, True, 61, sliced=False)
    y, idx = b.forward()
    same_bits(y.cols(), b.yr.reshape(-1, 8), 'bn_apply_maxpool over the cap')
    assert torch.equal(idx.view().cpu(), b.tap.reshape(-1))


def test_grid_wrap_bn_relu_pool_backward_apply(gpu):
    _over_cap('bn_bwd_apply_maxpool')
    b = BnPool(T.WRAP_POOLS['bn_bwd_apply_maxpool'], DV_F32, gpu, True, 62, sliced=False)
    run_bn_pool_backward(b, 1, 1.0, 'bn_bwd_apply_maxpool over the cap')
