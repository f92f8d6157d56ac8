"""The fp8 path -- dv_quantize_fp8, dv_conv3d_fwd_fp8, dv_conv3d_dgrad_fp8 (compute mode `fp8pw`) -- against the float64
references of tests/fp8_reference.py (OCP e4m3fn / e5m2 from the bit layout, rounding by sorted midpoints, a float64 GEMM of
the decoded bytes), over the tables of tests/fp8_cases.py.  Every entry is called through the C ABI / dualvar_amd.ops on explicit
tensors.  tests/test_fp8_host.py checks the references against torch's float8 types, the conditions stated here before a
launch, the table against the host queries (all 24 conv_gemm members of `fp8_impl`) and the refusals, on the CPU.

dv_quantize_fp8 (DV_F32 / DV_BF16 x e4m3 / e5m2).  Frames: x is a channel slice at offset 16 of a wider NaN buffer, q sits in a
    buffer of 0x7F bytes with ldq > C and rows behind it, scale_out is one float of a sentinel array, the workspace is +inf.
    EXACT GRID  amax = FMAX 2^k planted (k = -3, 0, 5): scale_out == 2^k bit for bit and EVERY byte equals `ref_quantize` --
        every finite code, every midpoint (ties to the lower and to the upper neighbour and subnormal codes asserted from the
        reference), the fp32 neighbours of the midpoints, half the smallest subnormal, +-0.
    GAUSSIAN  scale_out == fl32(amax / FMAX) bit for bit; every byte equals ref_quantize(x, scale_out) except the AMBIGUOUS
        ones (the byte changes somewhere in r (1 +- 4u), r = x / scale), which equal one of their two candidates; at most
        max(4, 1e-4 M C) elements may be ambiguous, asserted from the reference before the launch.  Shapes: one block; the
        blocks cap; second trips of both grid-stride loops with a ragged end; the negative amax element in the first vector,
        the last one, and one only a second trip reads.
    EDGES  all-zero tensor: scale 1, bytes 0.  TINY AMAX (2^-120 fp32, 2^-118 bf16: the scale is an fp32 subnormal and its
        reciprocal is +inf): scale finite and > 0, zeros stay 0x00 / 0x80, every byte the reference's, +-amax dequantise to
        within half an fp8 step.  The kernel divides (x / scale) since this test: with the reciprocal it stored 0xFE / 0xFB
        for zeros (0 * inf = NaN -> fmaxf -> -FMAX) and +-FMAX for everything else.
dv_conv3d_fwd_fp8 / dv_conv3d_dgrad_fp8.  Frames: the fp8 operand in a buffer of NaN codes (0x7F e4m3 / 0x7E e5m2) behind its
    rows and, on the small rows, beyond its pitch (ld > pitch, offset 16), zeros in its pad lanes [C, pitch); NaN codes behind
    the weights; the bf16 output in the NaN-sentinel frame of tests/test_conv_float64_gpu.py (offset 8 of a wider buffer on
    the small rows): only lanes [0, pitch) of rows < M change, the pad lanes to zero.
    (A) EXACT  G1: integers in [-8, 8] / 4 in both operands (numbers of both formats), scales 2^-3 and 2^5: the output is the
        round-to-nearest-even bf16 of the exact sum (S < 2^24 units asserted; ties asserted to occur); with DV_STATS each
        tile's sum equals float64 bit for bit and M2 stays inside the bf16-output bound of the conv file, rows per tile from
        dv_conv3d_tile_rows with the ragged last tile; DV_ACCUM of the data gradient onto G1 data.
        ALL CODES: operand A holds every finite code in every K position, operand P one signed power of two per output element
        (cnt <= 1 asserted; subnormal powers included) on a permutation of two K tiles: the output is the product itself.
        Four ways: A = activations / weights, forward / data gradient (e5m2 dy against e4m3 w).
    (B) GAUSSIAN at every row: operands are `ref_quantize` bytes of post-ReLU / fan_in^-1/2 / Gaussian data, scales the fp32
        amax / FMAX; every element inside
            b = (gamma(cnt + 2) S + 15 * 2^-13 G) |sc_a sc_b| + 2^-8 (|ref| + that),    gamma(n) = n u / (1 - n u), u = 2^-24
        gamma(cnt + 2) S: products of fp8 numbers are exact in fp32; cnt - 1 additions, the product of the scales and the
        multiplication by it.  2^-8 (..): half a bf16 ulp of the result.  15 * 2^-13 G, G = sum over the groups of 16
        consecutive K positions of max|a| max|b| (`group_term`), is what the first run of this file FOUND: the bound without it
        (the form of the conv file's DV_BF16 row) was missed by up to 54.7x (K = 16; 38 / 31 / 12.7 / 4.3 / 2.3x at K = 16 / 32 /
        64 / 128 / 192, met at K = 512) while every exact case held.  The 64-wide fp8 matrix instruction does not add its
        products as fp32 numbers: the 16 products of one 16-byte group are aligned to the exponent E of the group's largest
        one and each is truncated (towards zero) below 2^-13 E; group sums and the accumulator then add like fp32, rounded to
        nearest.  test_fp8_mfma_group_alignment_as_measured pins both facts on exact data; the worst Gaussian element was
        1200 + 13824 - 14976 - 48.75 = -0.75 in one group, returned as 0 (-48.75 -> -48 below 2^-13 * 2^13).  G1 data spans
        2^6 per group and is untouched.  Derived, not fitted: each of the at most 15 other terms of a group loses less than
        2^-13 max_g <= 2^-13 max|a| max|b|.  The statistics stay inside the conv file's bf16 bounds.

Each case prints (-s) err / bound; the module prints the largest err / bound and rms(err) / (2^-8 rms(ref)) per mode, tile and
gather at the end.  Measured figures and the mutants: DESIGN.md section 2.  Of six arithmetic changes seeded into a scratch build
five fail this file (the data gradient's format selector: every dgrad row and the two dgrad all-codes cases; a lane's two K
halves swapped: every GEMM test; one scale dropped: every row and all-codes case; e4m3 FMAX 240: the e4m3 grids and Gaussian
rows; truncation instead of rounding: every quantiser grid and Gaussian row); halving amax_partials_kernel's grid stride still
computes the maximum and fails nothing.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import ops  # noqa: E402
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_F32, DV_STATS  # noqa: E402
from tests import fp8_cases as T  # noqa: E402
from tests import fp8_reference as R  # noqa: E402
from tests import checks  # noqa: E402
from tests.chains import gamma  # noqa: E402
from tests.checks import F64, TDT, Ratios, dev_gen, is_sent, sent  # noqa: E402

E4, E5 = R.E4M3, R.E5M2
RATIO, RMS, AMBIG = Ratios(), {}, {}
within = RATIO.within
# bit for bit against float64 (bf16: against its round-to-nearest-even bf16): the reference must be an fp32 number; + 0.0 on
# both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nlargest err / bound, rms(err) / (2^-8 rms(ref)):')
    for k in sorted(RATIO):
        print(f'  {k:40s} {RATIO[k]:.3f}   {"" if k not in RMS else "%.3f" % RMS[k]}')
    print('ambiguous elements (of which took the other candidate) / elements:')
    for k in sorted(AMBIG):
        print(f'  {k:40s} {AMBIG[k][0]} ({AMBIG[k][1]}) / {AMBIG[k][2]}')


# ================================================================================================ dv_quantize_fp8
def run_quantize(dev, x, dtype, fmt):
    """x [M, C] of the input format -> (bytes [M, C], scale_out as a Python float); the frames are checked here"""
    M, C_ = x.shape
    ld, off, ldq = C_ + 32, 16, C_ + 16
    wide = torch.full((M + 3, ld), float('nan'), dtype=TDT[dtype], device=dev)
    wide[:M, off:off + C_] = x.to(dev)
    qbuf = torch.full((M + 5, ldq), 0x7F, dtype=torch.uint8, device=dev)
    sarr = sent((8,), dev)
    ws = torch.full((T.K_AMAX_BLOCKS,), float('inf'), dtype=torch.float32, device=dev)      # an unwritten partial that is read shows
    ops.quantize_fp8(wide[:, off:], M, C_, ld, fmt, dtype, q=qbuf, scale=sarr[3:4], workspace=ws)
    torch.cuda.synchronize()
    assert bool((qbuf[:M, C_:] == 0x7F).all()) and bool((qbuf[M:] == 0x7F).all()), 'bytes outside [M, C] written'
    assert is_sent(sarr[:3]) and is_sent(sarr[4:]), 'scale_out: a neighbour changed'
    return qbuf[:M, :C_], float(sarr[3])


@pytest.mark.parametrize('k', [-3, 0, 5])
@pytest.mark.parametrize('fmt', [E4, E5])
@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
def test_quantize_exact_grid(gpu, dtype, fmt, k):
    """scale = 2^k exactly, x / scale exact: every byte is the reference's, ties and subnormals included, no allowance"""
    x, is_mid = R.exact_grid(fmt, k, TDT[dtype])
    assert R.grid_properties(x, is_mid, fmt, k) == (True, True, True)
    q, scale = run_quantize(gpu, x, dtype, fmt)
    assert scale == 2.0 ** k, (scale, 2.0 ** k)
    ref = R.ref_quantize(x.double(), 2.0 ** k, fmt).to(gpu)
    bad = q != ref
    assert not bool(bad.any()), (f'{int(bad.sum())} of {bad.numel()} bytes differ; first: x / scale = '
                                 f'{float(x.double().to(gpu)[bad][0]) / 2.0 ** k!r} got {int(q[bad][0]):#x} want {int(ref[bad][0]):#x}')


def check_bytes(q, x64, scale, fmt, key):
    """every non-ambiguous byte equals ref_quantize(x, scale); an ambiguous one equals one of its two candidates"""
    lo, mid, hi = R.candidates(x64, scale, fmt)
    amb = (lo != mid) | (mid != hi)
    ok = torch.where(amb, (q == lo) | (q == hi), q == mid)
    other = int((amb & (q != mid)).sum())
    AMBIG[key] = (int(amb.sum()), other, q.numel())
    assert bool(ok.all()), (f'{key}: {int((~ok).sum())} of {ok.numel()} bytes differ ({int((~ok & amb).sum())} of them ambiguous); first: x / scale = '
                            f'{float((x64 / scale)[~ok][0])!r} got {int(q[~ok][0]):#x} want {int(mid[~ok][0]):#x}')
    return amb


@pytest.mark.parametrize('fmt', [E4, E5])
@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
@pytest.mark.parametrize('row', T.Q_ROWS, ids=[q.name for q in T.Q_ROWS])
def test_quantize_gaussian(gpu, row, dtype, fmt):
    x = R.gauss_input(row.M, row.C, TDT[dtype], T.amax_index(row))
    x64 = x.double().to(gpu)
    want = R.expected_scale(R.GAUSS_AMAX, fmt)
    n_amb = int(R.ambiguous(x64, want, fmt).sum())
    assert n_amb <= max(4, 1e-4 * row.M * row.C), f'{n_amb} ambiguous elements (test data)'
    q, scale = run_quantize(gpu, x, dtype, fmt)
    assert scale == want, f'scale_out {scale!r} is not fl32(amax / FMAX) = {want!r}'
    check_bytes(q, x64, scale, fmt, 'quantize:%s:%s:%s' % (row.name, 'f32' if dtype == DV_F32 else 'bf16', 'e4m3' if fmt == E4 else 'e5m2'))


@pytest.mark.parametrize('fmt', [E4, E5])
@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
def test_quantize_all_zero_and_tiny_amax(gpu, dtype, fmt):
    """the edges of the scale: an all-zero tensor (scale 1), and an amax whose scale is an fp32 subnormal"""
    z = torch.zeros(64, 16, dtype=TDT[dtype])
    z[5, 3] = -0.0
    q, scale = run_quantize(gpu, z, dtype, fmt)
    assert scale == 1.0 and int(q[5, 3]) == 0x80 and int((q != 0).sum()) == 1
    x = R.tiny_input(TDT[dtype])
    x64 = x.double().to(gpu)
    amax = R.TINY_AMAX[TDT[dtype]]
    q, scale = run_quantize(gpu, x, dtype, fmt)
    print(f'    tiny amax {amax!r}: scale_out {scale!r} (fl32(amax / FMAX) = {R.expected_scale(amax, fmt)!r})')
    assert scale == scale and 0 < scale < float('inf'), scale
    zero = x64 == 0
    want0 = torch.signbit(x64[zero]).to(torch.uint8) << 7
    assert torch.equal(q[zero], want0), f'zeros became {sorted(set(q[zero].tolist()))}'
    check_bytes(q, x64, scale, fmt, 'quantize:tiny:%s:%s' % ('f32' if dtype == DV_F32 else 'bf16', 'e4m3' if fmt == E4 else 'e5m2'))
    pos, _ = R._positive(fmt, gpu)
    half_step = float(pos[-1] - pos[-2]) / 2
    top = x64.abs() == amax
    assert bool(top.any()) and bool(((R.decode(q, fmt) * scale - x64).abs()[top] <= half_step * scale).all())


# ============================================================================== dv_conv3d_fwd_fp8 / dv_conv3d_dgrad_fp8
class Op8:
    """an fp8 operand [rows, C] with channel pitch `pitch` (bytes) in a buffer of NaN codes: rows behind it and, when wide, lanes
    around it (row pitch ld > pitch, offset 16); pad lanes [C, pitch) zero"""

    def __init__(self, dev, b8, pitch, fmt, wide, guard=37):
        rows, C_ = b8.shape
        self.ld, self.off = (pitch + 32, 16) if wide else (pitch, 0)
        self.buf = torch.full((rows + guard, self.ld), R.NAN_BYTE[fmt], dtype=torch.uint8, device=dev)
        self.buf[:rows, self.off:self.off + pitch] = 0
        self.buf[:rows, self.off:self.off + C_] = b8
        self.view = self.buf[:, self.off:]


def weight8(dev, b8, pitch, fmt):
    """[rows, C] bytes -> the dense [rows][pitch] weight operand (pad lanes zero) with NaN codes behind it"""
    rows, C_ = b8.shape
    buf = torch.full((rows * pitch + 512,), R.NAN_BYTE[fmt], dtype=torch.uint8, device=dev)
    w = buf[:rows * pitch].view(rows, pitch)
    w[:] = 0
    w[:, :C_] = b8
    return buf


class Out16:
    """the bf16 output [rows, C] (pitch `pitch`) in a buffer of the NaN sentinel, at channel offset 8 of a wider one when wide"""

    def __init__(self, dev, r, C_, pitch, wide, old=None, guard=37):
        self.rows, self.C, self.pitch = T.rows_of(r), C_, pitch
        self.off, self.ld = (8, pitch + 24) if wide else (0, pitch)
        self.buf = sent((self.rows + guard, self.ld), dev, torch.bfloat16)
        self.act = ops.Act(self.buf, r.N, r.T, r.H, r.W, C_, self.ld, self.off, DV_BF16, pitch)
        if old is not None:
            self.buf[:self.rows, self.off:self.off + pitch] = 0
            self.buf[:self.rows, self.off:self.off + C_] = old.to(torch.bfloat16)

    def get(self):
        return self.buf[:self.rows, self.off:self.off + self.C]

    def check_frame(self, what):
        b, o = self.buf, self.off
        if self.pitch > self.C:
            pad = b[:self.rows, o + self.C:o + self.pitch]
            assert bool(((pad.contiguous().view(torch.int16) & 0x7FFF) == 0).all()), what + ': pad lanes [C, pitch) are not zero'
        assert is_sent(b[self.rows:]), what + ': rows behind the tensor written'
        assert is_sent(b[:self.rows, :o]) and is_sent(b[:self.rows, o + self.pitch:]), what + ': lanes outside the view written'


def scalar(dev, v):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def run_fwd(r, dev, x8, w8, sx, sw, flags=0):
    """x8 [M, Cin], w8 [Cout, Cin] e4m3 bytes -> (output frame, stats [2, Cout, tiles] or None, rows per tile)"""
    wide = T.rows_of(r) < T.SMALL_ROWS
    xa = Op8(dev, x8, r.cinp, E4, wide)
    ya = Out16(dev, r, r.Cout, r.coutp, wide)
    d = T.make_desc(r, flags=flags, ld_src=xa.ld, ld_out=ya.ld)
    if r.fwd is not None:
        assert T.query(d, False) == r.fwd, (r.name, T.query(d, False), r.fwd)
    tiles, rows_t = ops.stat_tiles(d), ops.tile_rows(d)
    stats = sent((2, r.Cout, tiles), dev) if flags & DV_STATS else None
    ops.conv_fwd_fp8(d, xa.view, weight8(dev, w8, r.cinp, E4), scalar(dev, sx), scalar(dev, sw), ya.act, stats)
    torch.cuda.synchronize()
    return ya, stats, rows_t


def run_dgrad(r, dev, dy8, wd8, sdy, sw, old=None):
    """dy8 [M, Cout] e5m2, wd8 [Cin, Cout] e4m3 (the dgrad layout) -> the dx frame"""
    wide = T.rows_of(r) < T.SMALL_ROWS
    dya = Op8(dev, dy8, r.coutp, E5, wide)
    dxa = Out16(dev, r, r.Cin, r.cinp, wide, old=old)
    d = T.make_desc(r, flags=DV_ACCUM if old is not None else 0, ld_src=dya.ld, ld_out=dxa.ld, dgrad=True)
    if r.dgrad is not None:
        assert T.query(d, True) == r.dgrad, (r.name, T.query(d, True), r.dgrad)
    ops.conv_dgrad_fp8(d, dya.view, weight8(dev, wd8, r.coutp, E4), scalar(dev, sdy), scalar(dev, sw), dxa.act)
    torch.cuda.synchronize()
    return dxa


def g1_bytes(gen, shape, dev, fmt, rng=8):
    """integers in [-rng, rng] / 4 as bytes of `fmt` (asserted to decode to themselves)"""
    v = torch.randint(-rng, rng + 1, shape, generator=gen, device=dev).double() / 4
    b = R.ref_quantize(v, 1.0, fmt)
    assert bool((R.decode(b, fmt) == v).all()), 'a grid value is not a number of the format (test data)'
    return b


def gauss_bytes(gen, shape, dev, fmt, relu=False, mul=1.0):
    """(bytes, scale) of Gaussian data rounded to fp32 and quantised by the reference with scale = fl32(amax / FMAX)"""
    v = torch.randn(shape, generator=gen, device=dev, dtype=F64) * mul
    v = (v.clamp_min(0) if relu else v).to(torch.float32).double()
    s = R.expected_scale(float(v.abs().max()), fmt)
    return R.ref_quantize(v, s, fmt), s


def key_of(mode, form):
    return '%s:%dx%d:%s' % (mode, form.bm, form.bn, form.gather)


def gauss_bound(S, cnt, ref, sc, G):
    b = (gamma(cnt + 2) * S + (R.GROUP - 1) * 2.0 ** -R.GROUP_BITS * G) * abs(sc)
    return b + 2.0 ** -8 * (ref.abs() + b)


def rms_figure(got64, ref64, key):
    fig = float(((got64 - ref64) ** 2).mean().sqrt() / (2.0 ** -8 * (ref64 ** 2).mean().sqrt()))
    RMS[key] = max(RMS.get(key, 0.0), fig)
    return fig


def has_bf16_tie(ref64):
    r32 = ref64.to(torch.float32)
    return bool(((r32.view(torch.int32) & 0xFFFF) == 0x8000).any())


def stats_check(dev, y64, stats, rows_t, exact, unit, key, what):
    """per-tile sums and M2 of the stored values y64 [M, Cout] against float64: sums bit for bit on grid data, else -- and M2
    always -- inside the bf16-output bounds of tests/test_conv_float64_gpu.py (shifted sums about a stored value c and a
    pairwise merge: every term |y - c| <= |y| + max|y|)"""
    M, Co = y64.shape
    tiles = stats.shape[2]
    assert tiles * rows_t >= M > (tiles - 1) * rows_t and M % rows_t != 0          # the last tile is ragged
    assert bool(torch.isfinite(stats).all()), what + ': statistics not written'
    yp = torch.zeros(tiles * rows_t, Co, dtype=F64, device=dev)
    yp[:M] = y64
    yt = yp.reshape(tiles, rows_t, Co)
    valid = (torch.arange(tiles * rows_t, device=dev) < M).reshape(tiles, rows_t, 1)
    s = yt.sum(1)
    mu = s / valid.sum(1).double()
    dlt = torch.where(valid, yt - mu[:, None, :], torch.zeros_like(yt))
    m2 = (dlt ** 2).sum(1)
    amax = yt.abs().amax(1)
    if exact:
        assert float(yt.abs().sum(1).max() + rows_t * amax.max()) < 2.0 ** 24 * unit, what + ': tile sums leave the exact range (test data)'
        same_bits(stats[0].t(), s, what + ' tile sums')
    else:
        within(stats[0].t().double(), s, gamma(rows_t + 8) * (yt.abs().sum(1) + rows_t * amax), what + ' tile sums', key='stats_sum:' + key)
    within(stats[1].t().double(), m2, gamma(rows_t + 8) * 2 * ((yt ** 2).sum(1) + rows_t * amax ** 2), what + ' tile M2', key='stats_m2:' + key)


SA, SB = 2.0 ** -3, 2.0 ** 5            # the scales of the exact cases: powers of two, not both 1
IDS = [r.name for r in T.ROWS]


@pytest.mark.parametrize('row', T.ROWS, ids=IDS)
def test_fp8_gemm_fwd(gpu, row):
    """dv_conv3d_fwd_fp8 + DV_STATS on the row's tile and gather: G1 bit for bit, Gaussian data inside the bound, frames intact"""
    r, dev, M = row, gpu, T.rows_of(row)
    key = key_of('fwd', r.fwd)
    gen = dev_gen(dev, 300)
    # (A) G1
    x8, w8 = g1_bytes(gen, (M, r.Cin), dev, E4), g1_bytes(gen, (r.Cout, r.Cin), dev, E4)
    ref, S, _ = R.ref_gemm(x8, E4, w8, E4, SA, SB)
    assert float(S.max()) < 2.0 ** 24 / 16, 'sum|terms| leaves the exact range (test data)'
    assert has_bf16_tie(ref), 'no bf16 tie in the data'
    what = '%s %s G1' % (key, r.name)
    ya, stats, rows_t = run_fwd(r, dev, x8, w8, SA, SB, flags=DV_STATS)
    assert rows_t == r.fwd.bm
    ya.check_frame(what)
    same_bits(ya.get(), ref, what)
    stats_check(dev, ya.get().double(), stats, rows_t, True, SA * SB / 16, key, what)
    # (B) Gaussian
    x8, sx = gauss_bytes(gen, (M, r.Cin), dev, E4, relu=True)
    w8, sw = gauss_bytes(gen, (r.Cout, r.Cin), dev, E4, mul=r.Cin ** -0.5)
    ref, S, cnt = R.ref_gemm(x8, E4, w8, E4, sx, sw)
    what = '%s %s B' % (key, r.name)
    ya, stats, rows_t = run_fwd(r, dev, x8, w8, sx, sw, flags=DV_STATS)
    ya.check_frame(what)
    got = ya.get().double()
    within(got, ref, gauss_bound(S, cnt, ref, sx * sw, R.group_term(x8, E4, w8, E4)), what, key=key)
    print(f'    {what}: rms figure {rms_figure(got, ref, key):.3f}')
    stats_check(dev, got, stats, rows_t, False, None, key, what)
    ya2, _, _ = run_fwd(r, dev, x8, w8, sx, sw)                                  # without DV_STATS: the same bits, stats untouched
    assert torch.equal(ya2.get(), ya.get()), what + ': the output depends on DV_STATS'


@pytest.mark.parametrize('row', T.ROWS, ids=IDS)
def test_fp8_gemm_dgrad(gpu, row):
    """dv_conv3d_dgrad_fp8 (e5m2 dy, e4m3 w in the dgrad layout), plain and DV_ACCUM onto grid data"""
    r, dev, M = row, gpu, T.rows_of(row)
    key = key_of('dgrad', r.dgrad)
    gen = dev_gen(dev, 400)
    dy8, wd8 = g1_bytes(gen, (M, r.Cout), dev, E5), g1_bytes(gen, (r.Cin, r.Cout), dev, E4)
    ref, S, _ = R.ref_gemm(dy8, E5, wd8, E4, SA, SB)
    assert has_bf16_tie(ref), 'no bf16 tie in the data'
    what = '%s %s G1' % (key, r.name)
    dxa = run_dgrad(r, dev, dy8, wd8, SA, SB)
    dxa.check_frame(what)
    same_bits(dxa.get(), ref, what)
    old = torch.randint(-8, 9, ref.shape, generator=gen, device=dev).double() / 4
    assert float((S * SA * SB + old.abs()).max()) < 2.0 ** 24 / 16, 'sum|terms| leaves the exact range (test data)'
    want = ref.to(torch.float32).to(torch.bfloat16).double() + old              # both are bf16 numbers; their sum is rounded once more
    dxo = run_dgrad(r, dev, dy8, wd8, SA, SB, old=old)
    dxo.check_frame(what + ' accum')
    same_bits(dxo.get(), want, what + ' accum')
    # (B) Gaussian
    dy8, sdy = gauss_bytes(gen, (M, r.Cout), dev, E5)
    wd8, sw = gauss_bytes(gen, (r.Cin, r.Cout), dev, E4, mul=r.Cin ** -0.5)
    ref, S, cnt = R.ref_gemm(dy8, E5, wd8, E4, sdy, sw)
    what = '%s %s B' % (key, r.name)
    dxa = run_dgrad(r, dev, dy8, wd8, sdy, sw)
    dxa.check_frame(what)
    got = dxa.get().double()
    within(got, ref, gauss_bound(S, cnt, ref, sdy * sw, R.group_term(dy8, E5, wd8, E4)), what, key=key)
    print(f'    {what}: rms figure {rms_figure(got, ref, key):.3f}')


P_EXP = {E4: (-9, -8, -6, -2, 0, 3, 8), E5: (-16, -15, -14, -3, 0, 6, 15)}      # signed powers of two of P, subnormal ones first
K_ALL = 128                                                                     # two K tiles of 64 bytes


def all_codes(dev, fmt):
    """A [n_finite, 128]: every finite code of `fmt` in every K position (column k is a rotation of the code list)"""
    _, finite = R.decode_table(fmt)
    codes = torch.arange(256)[finite].to(dev)
    n = codes.numel()
    i, k = torch.arange(n, device=dev)[:, None], torch.arange(K_ALL, device=dev)[None, :]
    a = codes[(i + 37 * k) % n].to(torch.uint8)
    for col in (0, 63, 64, 127):
        assert sorted(a[:, col].tolist()) == sorted(codes.tolist())
    val = R.decode(a, fmt)
    sub = ((a & 0x7F) >> R.MBITS[fmt] == 0) & ((a & 0x7F) != 0)
    for cls in (sub, val == R.FMAX[fmt], val == -R.FMAX[fmt], a == 0x00, a == 0x80):
        assert bool(cls.any(0).all()), 'a class of codes misses a K position (test data)'
    return a


def one_per_row(dev, fmt, rows=K_ALL):
    """P [rows, 128]: one signed power of two per row, on a permutation of the K positions"""
    j = torch.arange(rows, device=dev)
    pi = (j * 37 + 11) % K_ALL
    assert sorted(pi.tolist()) == list(range(K_ALL))                            # every position of both K tiles
    p2 = torch.tensor([2.0 ** e for e in P_EXP[fmt]], dtype=F64, device=dev)[j % len(P_EXP[fmt])]     # (exact: no pow on the device)
    v = torch.zeros(rows, K_ALL, dtype=F64, device=dev)
    v[j, pi] = torch.where(j % 3 == 1, -p2, p2)
    b = R.ref_quantize(v, 1.0, fmt)
    assert bool((R.decode(b, fmt) == v).all())
    return b


@pytest.mark.parametrize('mode,a_is', [('fwd', 'act'), ('fwd', 'w'), ('dgrad', 'act'), ('dgrad', 'w')])
def test_fp8_gemm_every_code_against_one_power_of_two(gpu, mode, a_is):
    """One term per output element: the output is decode(A) * P * sc_a * sc_b, exact in bf16.  Pins the decode of every code
    (subnormals, maxima, signed zeros), the format selectors (e5m2 dy against e4m3 w), the lane -> k mapping and the LDS swizzle."""
    dev = gpu
    fmt_src = E4 if mode == 'fwd' else E5                                       # the format of the activation-side operand
    if a_is == 'act':
        src8, w8 = all_codes(dev, fmt_src), one_per_row(dev, E4)
    else:
        src8, w8 = one_per_row(dev, fmt_src), all_codes(dev, E4)
    M, Nw = src8.shape[0], w8.shape[0]
    H = 2 if M % 2 == 0 else 1
    cw = (Nw + 15) // 16 * 16
    if mode == 'fwd':
        r = T.Row('all_codes', 1, 1, H, M // H, K_ALL, Nw, K_ALL, cw, None, None)
    else:
        r = T.Row('all_codes', 1, 1, H, M // H, Nw, K_ALL, cw, K_ALL, None, None)
    sa, sb = 2.0 ** 3, 2.0 ** -1
    ref, _, cnt = R.ref_gemm(src8, fmt_src, w8, E4, sa, sb)
    assert float(cnt.max()) == 1.0 and float(cnt.min()) == 0.0 and float((cnt == 1).double().mean()) > 0.95, 'one term per element (test data)'
    assert bool((ref.to(torch.bfloat16).double() == ref).all()), 'a product is not a bf16 number (test data)'
    assert float(ref.abs()[ref != 0].min()) <= 2.0 ** -16 and float(ref.abs().max()) >= 2.0 ** 15
    what = 'all codes %s A=%s' % (mode, a_is)
    out = run_fwd(r, dev, src8, w8, sa, sb)[0] if mode == 'fwd' else run_dgrad(r, dev, src8, w8, sa, sb)
    out.check_frame(what)
    same_bits(out.get(), ref, what)


def _probe(dev, K, k_big, k_small, k_neg):
    """out[i, j] = B - B + s_ij with B = 256 * 256 at k_big, -B at k_neg and s_ij = 1.75 * 2^x_i * 2^y_j at k_small -> (got, s)"""
    M, N = 64, 32
    r = T.Row('probe', 1, 1, 1, M, K, N, K, N, None, None)
    i, j = torch.arange(M, device=dev), torch.arange(N, device=dev)
    a = torch.zeros(M, K, dtype=F64, device=dev)
    b = torch.zeros(N, K, dtype=F64, device=dev)
    a[:, k_big], a[:, k_neg], b[:, k_big], b[:, k_neg] = 256.0, -256.0, 256.0, 256.0
    a[:, k_small] = 1.75 * torch.tensor([2.0 ** (-6 + int(v) % 15) for v in i], dtype=F64, device=dev)
    b[:, k_small] = torch.tensor([2.0 ** (-9 + int(v) % 18) for v in j], dtype=F64, device=dev)
    a8, b8 = R.ref_quantize(a, 1.0, E4), R.ref_quantize(b, 1.0, E4)
    assert bool((R.decode(a8, E4) == a).all()) and bool((R.decode(b8, E4) == b).all())
    out = run_fwd(r, dev, a8, b8, 1.0, 1.0)[0]
    out.check_frame('probe')
    return out.get().double(), a[:, k_small:k_small + 1] * b[:, k_small][None, :]


def test_fp8_mfma_group_alignment_as_measured(gpu):
    """What gauss_bound's group term rests on, on exact data.  A small product s = 1.75 * 2^e next to B = 2^16, with -B in the
    next K tile: in ANOTHER 16-byte group of the same tile (k 5 / 17, 5 / 40) the result is fl32(B + s) - B, fp32 addition
    rounded to nearest even; in the SAME group (k 5 / 6) s is truncated towards zero below 2^-13 B = 8 before it is added."""
    Bv = 2.0 ** 16
    for k_small in (17, 40):
        got, s = _probe(gpu, 128, 5, k_small, 64 + 5)
        want = (torch.tensor(Bv, dtype=F64, device=gpu) + s).to(torch.float32).double() - Bv
        assert bool((s < 2.0 ** -9 * Bv).any()) and bool((want != s).any()) and bool((want == 0).any())
        same_bits(got.to(torch.bfloat16), want, 'another group, k 5 / %d' % k_small)
    got, s = _probe(gpu, 128, 5, 6, 64 + 5)
    unit = 2.0 ** -R.GROUP_BITS * Bv
    want = torch.floor(s / unit) * unit
    assert bool(((want != s) & (want != 0)).any()) and bool((want == 0).any())
    same_bits(got.to(torch.bfloat16), want, 'the same group, k 5 / 6')
