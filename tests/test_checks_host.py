"""CPU: tests/checks.py and tests/chains.py themselves.  Every float64 suite now stands on one bound check, one bit check, one
sentinel pattern table and one set of summation-order models, so each is pinned here on CPU tensors, without a GPU and without
loading the library: what must be refused is refused, what must pass passes, and the chain models keep the values they had
when the suites' bounds were derived (the rows are the shapes where a row-group count or a fold changes)."""
import numpy as np
import pytest
import torch

from dualvar_amd._lib import DV_BF16, DV_F32
from tests import chains, checks
from tests.checks import F64, Ratios, View, equal_bits, is_sent, same_bits, sent, within

CPU = torch.device('cpu')
ULP32 = 2.0 ** -23                 # spacing of fp32 at 1.0
ULP16 = 2.0 ** -7                  # spacing of bf16 at 1.0


def t64(*v):
    return torch.tensor(v, dtype=F64)


# -------------------------------------------------------------------------------------------------------------- bound check
def test_bound_check_refuses_what_any_suite_refused():
    ref, bound = t64(1.0, 2.0, 3.0), t64(0.5, 0.5, 0.5)
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(AssertionError, match='non-finite'):
            within(t64(1.0, bad, 3.0), ref, bound, 'q non-finite', quiet=True)
    above = float(np.nextafter(0.5, 1.0))                       # one ulp above the bound, in one element
    assert above - 0.5 == 2.0 ** -53
    with pytest.raises(AssertionError, match='1 of 3 values outside'):
        within(t64(1.0, above, 3.0), t64(1.0, 0.0, 3.0), bound, 'q one ulp', quiet=True)
    with pytest.raises(AssertionError, match='outside the bound'):
        within(t64(1.0, 2.0, 3.0 + 2.0 ** -40), ref, t64(0.5, 0.5, 0.0), 'q zero bound', quiet=True)
    with pytest.raises(AssertionError, match='outside the bound'):
        within(t64(1.0, 2.0, 3.0), ref, t64(0.5, float('nan'), 0.5), 'q nan bound', quiet=True)
    with pytest.raises(AssertionError, match='outside the bound'):
        within(t64(1.0, 2.0, 3.0), t64(1.0, float('nan'), 3.0), bound, 'q nan reference', quiet=True)
    with pytest.raises(AssertionError, match='outside the bound'):
        within(t64(1.0, 2.1, 3.0), ref, t64(0.5, -0.5, 0.5), 'q negative bound', quiet=True)
    with pytest.raises(AssertionError, match='outside the bound'):          # the error-only form: inf under an infinite bound
        checks.err_within(t64(float('inf')), t64(float('inf')), 'q inf')


def test_bound_check_passes_and_records():
    r = Ratios()
    assert within(torch.zeros(0), torch.zeros(0, dtype=F64), torch.zeros(0, dtype=F64), 'empty case', r) == 0.0
    assert r == {'empty': 0.0}
    # err == bound exactly, and an exact element under a zero bound
    assert within(t64(1.5, 2.0, 3.25), t64(1.0, 2.0, 3.0), t64(0.5, 0.0, 1.0), 'q.x step 3 n=5', r, quiet=True) == 1.0
    assert r['q.x'] == 1.0
    assert r.within(t64(1.25), t64(1.0), t64(1.0), 'q.x again') == 0.25 and r['q.x'] == 1.0          # the largest is kept
    assert r.within(t64(1.25), t64(1.0), t64(1.0), 'a name with blanks [fp32]', key='a name with blanks [fp32]') == 0.25
    assert r.ratio(np.array([0.5, 0.25]), [1.0, 1.0], 'err.only case') == 0.5                          # arrays and lists
    assert set(r) == {'empty', 'q.x', 'a name with blanks [fp32]', 'err.only'}
    assert within(t64(1.0), t64(1.0), t64(0.0), 'no recorder', quiet=True) == 0.0                        # ratios = None
    # an fp32 result against a float64 reference on a broadcast bound
    got = torch.tensor([1.0, 1.0 + ULP32], dtype=torch.float32)
    assert within(got, t64(1.0, 1.0), ULP32, 'broadcast', quiet=True) == 1.0


def test_report_prints_every_key(capsys):
    r = Ratios({'b.y': 0.5, 'a.x': 0.12345})
    r.report(12)
    assert capsys.readouterr().out == '\nlargest err / bound per quantity:\n  a.x          0.123\n  b.y          0.500\n'


# ---------------------------------------------------------------------------------------------------------------- bit check
FOLD = dict(ref_exact_in=torch.float32, signed_zeros=False)        # the conv / loss / optimizer suites
STRICT = dict(ref_exact_in='storage', signed_zeros=True)           # the pool / gate suite


def test_bit_check_one_ulp_and_representability():
    ref = t64(1.0, -2.5, 0.375)
    same_bits(ref.float(), ref, 'fp32', **FOLD)
    same_bits(ref.float(), ref, 'fp32', **STRICT)
    same_bits(ref.bfloat16(), ref, 'bf16', **FOLD)
    off32 = ref.float().clone()
    off32[1] = float(np.nextafter(np.float32(-2.5), np.float32(0)))
    off16 = ref.bfloat16().clone()
    off16[0] = 1.0 + ULP16
    for kw in (FOLD, STRICT):
        with pytest.raises(AssertionError, match='1 of 3 elements differ'):
            same_bits(off32, ref, 'fp32 one ulp', **kw)
        with pytest.raises(AssertionError, match='1 of 3 elements differ'):
            same_bits(off16, ref, 'bf16 one ulp', **kw)
    # a reference that is no fp32 number / no number of the storage dtype
    with pytest.raises(AssertionError, match='not representable'):
        same_bits(torch.ones(1), t64(1.0 + 2.0 ** -30), 'fp32 ref', **FOLD)
    with pytest.raises(AssertionError, match='not representable'):
        same_bits(torch.ones(1, dtype=torch.bfloat16), t64(1.0 + ULP32), 'bf16 storage ref', **STRICT)
    # ... while ref_exact_in = fp32 holds a bf16 result to the round-to-nearest-even bf16 of an fp32 reference (a tie: to even)
    same_bits(torch.ones(1, dtype=torch.bfloat16), t64(1.0 + ULP16 / 2), 'bf16 tie', **FOLD)
    with pytest.raises(AssertionError, match='elements differ'):
        same_bits(torch.tensor([1.0 + ULP16], dtype=torch.bfloat16), t64(1.0 + ULP16 / 2), 'bf16 tie up', **FOLD)
    # infinities are numbers of every format
    same_bits(torch.tensor([float('inf'), -float('inf')]), t64(float('inf'), -float('inf')), 'inf', **STRICT)


def test_bit_check_signed_zeros_as_the_argument_says():
    pz, nz = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    ref_p, ref_n = t64(0.0, 1.0), t64(-0.0, 1.0)
    for got, ref in ((pz, ref_n), (nz, ref_p)):
        same_bits(got, ref, 'folded', **FOLD)
        with pytest.raises(AssertionError, match='1 of 2 elements differ'):
            same_bits(got, ref, 'told apart', **STRICT)
        with pytest.raises(AssertionError, match='1 of 2 elements differ'):
            same_bits(got.bfloat16(), ref, 'told apart bf16', **STRICT)
    same_bits(nz, ref_n, 'same sign', **STRICT)
    with pytest.raises(TypeError):                               # no default: a call site has to say which it means
        same_bits(pz, ref_p, 'no arguments')
    assert equal_bits(nz, nz.clone()) and not equal_bits(pz, nz)
    nan2 = torch.tensor([0x7fc00000, 0x7fc00001], dtype=torch.int32).view(torch.float32)
    assert not equal_bits(nan2[:1], nan2[1:]) and equal_bits(nan2, nan2.clone())
    assert equal_bits(torch.arange(6.0).view(2, 3).t(), torch.arange(6.0).view(2, 3).t().contiguous())      # not contiguous


# ---------------------------------------------------------------------------------------------------------------- sentinels
@pytest.mark.parametrize('dtype,code', [(torch.float32, DV_F32), (torch.bfloat16, DV_BF16), (torch.float64, None), (torch.int32, None)])
def test_sentinels_detect_one_changed_element(dtype, code):
    t = sent((5, 7), CPU, dtype)
    assert t.dtype == dtype and is_sent(t) and is_sent(t[:0]) and is_sent(t[:, 7:]) and is_sent(t.t())
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    if code is not None:
        assert equal_bits(sent((5, 7), CPU, code), t)
    keep = torch.ones(5, 7, dtype=torch.bool)
    keep[3, 4] = False
    for v in (0, 1):
        t = sent((5, 7), CPU, dtype)
        t[3, 4] = v
        assert not is_sent(t) and not is_sent(t[3]) and is_sent(t[:3]) and is_sent(t, keep) and not is_sent(t, ~keep)
    if dtype == torch.float32:                                   # another NaN is not the sentinel
        t = sent((4,), CPU)
        t[2] = float('nan')
        assert not is_sent(t)


def test_sentinel_bits_are_the_ones_the_suites_were_written_with():
    assert int(checks.bits(sent((1,), CPU))[0]) == 0x7fb12345
    assert int(checks.bits(sent((1,), CPU, torch.bfloat16))[0]) == 0x7fb1
    assert int(checks.bits(sent((1,), CPU, F64))[0]) == 0x7ff8123456789abc
    assert int(sent((1,), CPU, torch.int32)[0]) == 0x7fb12345


@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
def test_view_frames(dtype):
    M, C_ = 6, 5                                                  # CP = 8: three pad lanes
    vals = torch.arange(M * C_, dtype=F64).view(M, C_)
    out = View(dtype, M, C_, 8, 32, CPU)
    assert out.untouched() and out.CP == 8 and out.ptr == out.buf.data_ptr() + 8 * out.buf.element_size()
    with pytest.raises(AssertionError, match='pad lanes'):        # an output nobody wrote: its pad lanes are not 0
        out.check_frame('unwritten')
    out.set(vals, pad=0)
    out.check_frame('written')
    assert not out.untouched() and torch.equal(out.val(), vals) and out.cols().shape == (M, 8)
    for r, c, msg in ((0, 7, 'outside the view'), (M - 1, 16, 'outside the view'), (2, 8 + C_, 'pad lanes'), (5, 15, 'pad lanes')):
        v = View(dtype, M, C_, 8, 32, CPU, vals, pad=0)
        v.check_frame('clean')
        v.buf[r, c] = 1.0
        with pytest.raises(AssertionError, match=msg):
            v.check_frame('poked')
    inp = View(dtype, M, C_, 0, 8, CPU, vals, pad=3.0)            # an input with junk pad lanes; pad=None leaves them
    assert bool((inp.cols()[:, C_:] == 3.0).all())
    inp.set(vals + 1, pad=None)
    assert bool((inp.cols()[:, C_:] == 3.0).all()) and torch.equal(inp.val(), vals + 1)
    for r, c in ((0, 0), (M - 1, 31), (3, 8 + C_)):               # any write at all
        v = View(dtype, M, C_, 8, 32, CPU)
        v.buf[r, c] = 0.0
        assert not v.untouched()
    s = View.sliced(dtype, M, C_, CPU, True, vals)
    assert (s.off, s.ld) == (8, 32) and bool((s.cols()[:, C_:] == 0).all()) and is_sent(s.buf[:, :8]) and is_sent(s.buf[:, 16:])
    d = View.sliced(dtype, M, C_, CPU, False, vals, pitch_pad=8)
    assert (d.off, d.ld) == (0, 16)
    with pytest.raises(AssertionError):
        View(dtype, M, C_, 4, 32, CPU)                            # offsets are multiples of 8


# ------------------------------------------------------------------------------------------------------------- chain models
F, B = DV_F32, DV_BF16
COLUMN = [  # (rows, CP, dtype) -> chain, the same for one and two sums per column at these widths
    ((1, 8, F), 8), ((4097, 8, F), 40), ((1, 8, B), 9), ((4097, 8, B), 25),
    ((1, 1032, F), 8), ((4097, 1032, F), 4097), ((1, 1032, B), 1), ((4097, 1032, B), 4097)]
BWD_REDUCE = [  # (M, C, dtype, nblk) -> chain
    ((1, 3, F, 1), 10), ((1, 3, F, 32), 41), ((1, 3, F, 33), 42), ((4097, 3, F, 1), 42), ((4097, 3, F, 32), 42), ((4097, 3, F, 33), 42),
    ((1, 3, B, 1), 11), ((1, 3, B, 32), 42), ((1, 3, B, 33), 43), ((4097, 3, B, 1), 27), ((4097, 3, B, 32), 42), ((4097, 3, B, 33), 43),
    ((1, 1030, F, 1), 10), ((1, 1030, F, 32), 41), ((1, 1030, F, 33), 42), ((4097, 1030, F, 1), 4099), ((4097, 1030, F, 32), 162),
    ((4097, 1030, F, 33), 159),
    ((1, 1030, B, 1), 3), ((1, 1030, B, 32), 34), ((1, 1030, B, 33), 35), ((4097, 1030, B, 1), 4099), ((4097, 1030, B, 32), 162),
    ((4097, 1030, B, 33), 159)]
STATS = [((1, 256), 11), ((256, 256), 11), ((257, 256), 12), ((2048, 1024), 24), ((2049, 1024), 25)]
GEMM = [  # (M, N, K) -> (form, chain)
    ((1, 1, 1), ('plain', 2)), ((5, 31, 2), ('plain', 2)), ((257, 4200, 64), ('plain', 64)), ((1025, 1024, 65), ('plain', 66)),
    ((1, 5, 64), ('tile4', 19)), ((33, 31, 65), ('tile4', 35)), ((257, 257, 4096), ('tile4', 1027)), ((64, 64, 4095), ('tile4', 1027)),
    ((256, 256, 4096), ('split', 83)), ((32, 128, 4097), ('split', 96)), ((1, 1, 5000), ('split', 99)), ((128, 128, 65536), ('split', 323))]


def test_chain_models_keep_their_values():
    for args, want in COLUMN:
        assert chains.column_chain(*args, 1) == chains.column_chain(*args, 2) == want, args
        assert chains.column_chain(*args, 2, extra=5) == want + 5
    for args, want in BWD_REDUCE:
        assert chains.bwd_reduce_chain(*args) == want, args
    for args, want in STATS:
        assert chains.stats_chain(*args) == want, args
    assert chains.stats_chain(300) == chains.stats_chain(300, 256) == 12
    for args, (form, want) in GEMM:
        assert (chains.gemm_form(*args), chains.gemm_chain(*args)) == (form, want), args
    assert chains.splitk_plan(1, 1, 5000) == (1, 16, 320) and chains.splitk_plan(32, 128, 4097) == (4, 13, 320)
    assert chains.gemm_chain(64, 64, 4096, 'plain') == 4096 and chains.gemm_chain(64, 64, 4095, 'plain') == 4096


def test_error_figures_keep_their_values():
    u = 2.0 ** -24
    assert (checks.U, checks.BF16_U) == (u, 2.0 ** -8)
    assert (chains.E_LOG, chains.E_LOG1P, chains.E_EXPF, chains.TINY) == (5.4 * u, 2.1 * u, 2.8 * u, 2.0 ** -126)
    assert chains.e_exp(t64(0.0, -2.0, 10.0)).tolist() == [4.2 * u, (4.2 + 8.2) * u, (4.2 + 41.0) * u]
    assert chains.gamma(0) == 0.0 and chains.gamma(7) == 7 * u / (1 - 7 * u)
    a, b = t64(1.0, -2.0).view(1, 2), t64(3.0, 0.5).view(1, 2)
    assert chains.gemm_bound(a, b, -0.5, 6).tolist() == [[8 * u * 0.5 * 4.0]]
    one = t64(1.0).view(1, 1)
    zero = torch.zeros(1, 1, dtype=F64)
    # one term, d = 0, Q = 1 exact: only the roundings of Q + n d^2 and the fold are left
    assert chains.m2_bound(one, zero, zero, one, zero, zero, 3).tolist() == [u + 3 * u]
    assert (checks.cp8(1), checks.cp8(8), checks.cp8(9), checks.ceil_div(9, 8), checks.ceil_div(8, 8)) == (8, 8, 16, 2, 1)
    assert (checks.vec(DV_F32), checks.vec(DV_BF16), checks.f32(0.1)) == (4, 8, float(np.float32(0.1)))
