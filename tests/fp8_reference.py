"""float64 references of the fp8 path (dv_quantize_fp8, dv_conv3d_fwd_fp8, dv_conv3d_dgrad_fp8), written from the OCP 8-bit
floating point layouts and from the header's contract.  torch float64 on whatever device the inputs live on; it never calls
the library under test and never uses torch's float8 casts (tests/test_fp8_host.py compares it WITH them on the CPU).

  e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN: 254 finite codes, max 448,
          smallest subnormal 2^-9.
  e5m2:   1 sign, 5 exponent (bias 15), 2 mantissa bits; exponent 31 is inf / NaN: 248 finite codes, max 57344, smallest
          subnormal 2^-16.
"""
import torch

F64 = torch.float64
E4M3, E5M2 = 0, 1
FMAX = {E4M3: 448.0, E5M2: 57344.0}
MBITS = {E4M3: 3, E5M2: 2}
BIAS = {E4M3: 7, E5M2: 15}
NAN_BYTE = {E4M3: 0x7F, E5M2: 0x7E}          # a NaN code of each format: the filling of the operand frames
U = 2.0 ** -24


def decode_table(fmt):
    """-> (values float64 [256] with NaN at the non-finite codes, finite bool [256]) from the bit layout"""
    code = torch.arange(256, dtype=torch.int64)
    mb, bias = MBITS[fmt], BIAS[fmt]
    sign = (code >> 7) & 1
    e = (code >> mb) & ((1 << (7 - mb)) - 1)
    m = code & ((1 << mb) - 1)
    two = torch.tensor(2.0, dtype=F64)
    sub = m.double() * 2.0 ** (1 - bias - mb)
    nrm = (1.0 + m.double() / (1 << mb)) * torch.pow(two, (e - bias).double())
    val = torch.where(e == 0, sub, nrm)
    val = torch.where(sign == 1, -val, val)
    finite = ~((e == 15) & (m == 7)) if fmt == E4M3 else e != 31
    return torch.where(finite, val, torch.full_like(val, float('nan'))), finite


def _positive(fmt, dev):
    """the non-negative finite values in code order (code i has value pos[i]) and the midpoints between neighbours"""
    val, finite = decode_table(fmt)
    n = int(finite[:128].sum())
    assert bool(finite[:n].all())
    pos = val[:n].to(dev)
    assert bool((pos[1:] > pos[:-1]).all()) and float(pos[-1]) == FMAX[fmt]
    return pos, (pos[1:] + pos[:-1]) / 2


def quantize_ratio(r64, fmt):
    """the byte of the float64 number r: nearest code value, ties to the code with an even mantissa (= even code), saturating at
    +-FMAX; the sign bit is r's (so -0.0 -> 0x80)"""
    pos, mid = _positive(fmt, r64.device)
    a = r64.abs()
    idx = torch.searchsorted(mid, a.contiguous(), right=False)                 # the number of midpoints below |r|
    tie = (idx < mid.numel()) & (mid[idx.clamp_max(mid.numel() - 1)] == a)
    idx = torch.where(tie & (idx % 2 == 1), idx + 1, idx)                      # a tie sits between codes idx and idx + 1
    return (idx | (torch.signbit(r64).to(torch.int64) << 7)).to(torch.uint8)


def ref_quantize(x64, s, fmt):
    """fp8_rne(x / s): x float64 (holding fp32 or bf16 numbers), s the fp32 scale as a Python float -> uint8"""
    return quantize_ratio(x64 / float(s), fmt)


def candidates(x64, s, fmt):
    """the bytes of r (1 - 4u), r, r (1 + 4u), r = x / s, u = 2^-24"""
    r = x64 / float(s)
    return quantize_ratio(r * (1 - 4 * U), fmt), quantize_ratio(r, fmt), quantize_ratio(r * (1 + 4 * U), fmt)


def ambiguous(x64, s, fmt):
    """elements whose byte may legitimately be either neighbour under an fp32 evaluation of x / s (a reciprocal multiply, or a
    division followed by the second rounding to fp8): the byte changes somewhere in r (1 +- 4u)"""
    lo, mid, hi = candidates(x64, s, fmt)
    return (lo != mid) | (mid != hi)


def decode(b, fmt):
    """uint8 tensor -> float64 values (NaN for the non-finite codes)"""
    val, _ = decode_table(fmt)
    return val.to(b.device)[b.long()]


def ref_gemm(a8, fmt_a, b8, fmt_b, sc_a, sc_b):
    """a8 [M, K], b8 [N, K] bytes -> (ref [M, N] = (sum_k a b) sc_a sc_b in float64, S = sum_k |a b| (unscaled), cnt = the
    number of non-zero terms)"""
    a, b = decode(a8, fmt_a), decode(b8, fmt_b)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), 'non-finite code in an operand (test data)'
    ref = (a @ b.t()) * (float(sc_a) * float(sc_b))
    S = a.abs() @ b.abs().t()
    cnt = (a != 0).double() @ (b != 0).double().t()
    return ref, S, cnt


GROUP = 16                # K positions whose products the matrix instruction adds in one aligned group (a 16-byte register quad)
GROUP_BITS = 13           # bits kept below the exponent of the group's largest product


def group_term(a8, fmt_a, b8, fmt_b):
    """[M, N]: sum over the groups g of GROUP consecutive K positions of max_k|a| max_k|b| -- an upper bound of the sum of the
    groups' largest |products|.  v_mfma_f32_32x32x64_f8f6f4 aligns the 16 products of a group to the exponent E of the largest
    one and TRUNCATES each below 2^-13 E before it adds them (measured, tests/test_fp8_float64_gpu.py::
    test_fp8_mfma_group_alignment_as_measured); the group sums and the accumulator then add as fp32 numbers, rounded to
    nearest.  So each of the at most GROUP - 1 other terms of a group loses less than 2^-GROUP_BITS max_g."""
    a, b = decode(a8, fmt_a).abs(), decode(b8, fmt_b).abs()
    K = a.shape[1]
    pad = -K % GROUP
    if pad:
        a = torch.cat([a, a.new_zeros(a.shape[0], pad)], 1)
        b = torch.cat([b, b.new_zeros(b.shape[0], pad)], 1)
    return a.reshape(a.shape[0], -1, GROUP).amax(2) @ b.reshape(b.shape[0], -1, GROUP).amax(2).t()


# ------------------------------------------------------------------------------------------- inputs of the quantiser tests
def expected_scale(amax, fmt):
    """fl32(amax / FMAX): the float64 quotient rounded once is the correctly rounded fp32 quotient"""
    return float(torch.tensor(float(amax) / FMAX[fmt], dtype=F64).to(torch.float32))


def _next_up(t):
    """the next number of t's own format above each positive element"""
    it = torch.int32 if t.dtype == torch.float32 else torch.int16
    return (t.contiguous().view(it) + 1).view(t.dtype)


GAUSS_AMAX = 24.0 * (1 + 2.0 ** -6)      # planted: a bf16 number; amax / FMAX is then no power of two (ties belong to the grid)


def gauss_input(M, C_, tdt, at, seed=5):
    """randn * 3 clamped to +-20 in the tensor's own format, with -GAUSS_AMAX planted at `at` = (row, column): -> [M, C] of tdt"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C_, generator=g) * 3).clamp(-20, 20).to(tdt)
    x[at[0], at[1]] = -GAUSS_AMAX
    assert float(x.double().abs().max()) == GAUSS_AMAX and float(x[at[0], at[1]]) == -GAUSS_AMAX
    return x


def exact_grid(fmt, k, tdt, C_=48):
    """The exact grid of dv_quantize_fp8: 2^k times every finite code value, every midpoint between adjacent codes (both signs;
    the first one is half the smallest subnormal), for fp32 the neighbours one ulp below and above each midpoint, the number
    just above FMAX's lower midpoint, and +-0, padded with zeros to [M, C].  amax = FMAX 2^k is among them, so scale = 2^k and
    x / scale is exact.  -> (x [M, C] of tdt, is_mid bool [M, C] marking the exact midpoints)"""
    val, finite = decode_table(fmt)
    pos, mid = _positive(fmt, 'cpu')
    sc = 2.0 ** k
    codes = val[finite] * sc
    mids = torch.cat([mid, -mid]) * sc
    parts, marks = [codes, mids], [torch.zeros_like(codes, dtype=torch.bool), torch.ones_like(mids, dtype=torch.bool)]
    m_t = mids.to(tdt)
    assert bool((m_t.double() == mids).all()), 'a midpoint is not a number of the input format (test data)'
    if tdt == torch.float32:
        pm = (mid * sc).to(tdt)
        up, dn = torch.nextafter(pm, torch.full_like(pm, float('inf'))), torch.nextafter(pm, torch.zeros_like(pm))
        near = torch.cat([up, dn, -up, -dn]).double()
    else:
        top = (mid[-1:] * sc).to(tdt)
        near = torch.cat([_next_up(top), -_next_up(top)]).double()
    parts.append(near)
    marks.append(torch.zeros_like(near, dtype=torch.bool))
    zeros = torch.tensor([0.0, -0.0], dtype=F64)
    parts.append(zeros)
    marks.append(torch.zeros(2, dtype=torch.bool))
    v, mk = torch.cat(parts), torch.cat(marks)
    M = -(-v.numel() // C_)
    x = torch.zeros(M * C_, dtype=F64)
    x[:v.numel()] = v
    is_mid = torch.zeros(M * C_, dtype=torch.bool)
    is_mid[:mk.numel()] = mk
    xt = x.to(tdt)
    assert bool((xt.double() == x).all()) and float(x.abs().max()) == FMAX[fmt] * sc
    return xt.reshape(M, C_), is_mid.reshape(M, C_)


def grid_properties(x, is_mid, fmt, k):
    """from the reference alone: the grid holds ties that go to the lower and to the upper neighbour, and subnormal codes"""
    b = ref_quantize(x.double(), 2.0 ** k, fmt).long()
    r = x.double().abs() / 2.0 ** k
    _, mid = _positive(fmt, 'cpu')
    lower = torch.searchsorted(mid, r[is_mid].contiguous())          # a midpoint sits between codes `lower` and `lower + 1`
    mag = b[is_mid] & 0x7F
    assert bool(((mag == lower) | (mag == lower + 1)).all())
    sub = ((b & 0x7F) >> MBITS[fmt] == 0) & ((b & 0x7F) != 0)
    return bool((mag == lower).any()), bool((mag == lower + 1).any()), bool(sub.any())


TINY_AMAX = {torch.float32: 2.0 ** -120, torch.bfloat16: 2.0 ** -118}


def tiny_input(tdt, M=40, C_=32):
    """zeros of both signs, +-amax, amax / 2, amax / 3 (rounded to the format) with amax below FMAX 2^-128 of both formats: the
    scale amax / FMAX is an fp32 subnormal and its reciprocal overflows"""
    a = TINY_AMAX[tdt]
    pat = torch.tensor([0.0, -0.0, a, -a, a / 2, a / 3, -a / 2, -a / 3, 0.0, a / 2, -0.0], dtype=F64)
    x = pat.repeat(-(-M * C_ // pat.numel()))[:M * C_].to(tdt).reshape(M, C_)
    assert float(x.double().abs().max()) == a
    return x
