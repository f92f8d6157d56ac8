"""CPU: what tests/test_fp8_float64_gpu.py rests on, checked without a device.

* tests/fp8_reference.py against torch's own OCP float8 types: the decode tables on every finite code, `ref_quantize` against
  torch's cast on Gaussian data and on the exact grid (where nothing is ambiguous);
* the conditions the GPU test states BEFORE it launches: the ambiguity cap of every Gaussian quantiser case, the ties and
  subnormal codes of the exact grids, the launch shapes of the quantiser rows;
* tests/fp8_cases.py against the host-side queries: every row runs the tile and gather it names, the table reaches all 24
  conv_gemm members of `fp8_impl`, every row ends in a ragged row tile;
* the refusals of dv_conv3d_fwd_fp8 / dv_conv3d_dgrad_fp8 / dv_quantize_fp8 (nothing is launched, nothing written).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fp8_cases as T
from tests import fp8_reference as R

T8 = {R.E4M3: torch.float8_e4m3fn, R.E5M2: torch.float8_e5m2}
TDTS = (torch.float32, torch.bfloat16)


@pytest.mark.parametrize('fmt', [R.E4M3, R.E5M2])
def test_decode_table_against_torch(fmt):
    val, finite = R.decode_table(fmt)
    n, fmax, tiny = {R.E4M3: (254, 448.0, 2.0 ** -9), R.E5M2: (248, 57344.0, 2.0 ** -16)}[fmt]
    assert int(finite.sum()) == n and float(val[finite].max()) == fmax == R.FMAX[fmt] and float(val[finite].min()) == -fmax
    assert float(val[finite & (val > 0)].min()) == tiny and float(val[1]) == tiny
    assert float(val[0]) == 0.0 and float(val[128]) == 0.0 and bool(torch.signbit(val[128]))
    assert not bool(finite[R.NAN_BYTE[fmt]])                     # the filling of the operand frames decodes to NaN
    t = torch.arange(256, dtype=torch.uint8).view(T8[fmt]).double()
    assert bool((t[finite] == val[finite]).all()) and not bool(torch.isfinite(t[~finite]).any())
    assert bool((torch.signbit(t[finite]) == torch.signbit(val[finite])).all())


@pytest.mark.parametrize('fmt', [R.E4M3, R.E5M2])
def test_ref_quantize_against_torch_cast(fmt):
    """the sorted-midpoint rounding against torch's cast of the fp32 quotient: equal wherever the quotient's own rounding cannot
    matter (every non-ambiguous element), and on the whole exact grid"""
    fmax = R.FMAX[fmt]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(40000, generator=g) * 3
    s = R.expected_scale(float(x.abs().max()), fmt)
    mine = R.ref_quantize(x.double(), s, fmt)
    theirs = (x / s).clamp(-fmax, fmax).to(T8[fmt]).view(torch.uint8)
    amb = R.ambiguous(x.double(), s, fmt)
    assert int(amb.sum()) <= 4
    assert torch.equal(mine[~amb], theirs[~amb])
    lo, _, hi = R.candidates(x.double(), s, fmt)
    assert bool(((theirs == lo) | (theirs == hi))[amb].all())
    assert int(mine.long().bincount(minlength=256)[R.NAN_BYTE[fmt]]) == 0
    for tdt in TDTS:
        for k in (-3, 0, 5):
            xg, _ = R.exact_grid(fmt, k, tdt)
            sc = 2.0 ** k
            mine = R.ref_quantize(xg.double(), sc, fmt)
            theirs = (xg.float() / sc).clamp(-fmax, fmax).to(T8[fmt]).view(torch.uint8)
            assert torch.equal(mine, theirs), (fmt, tdt, k)
            assert R.expected_scale(float(xg.double().abs().max()), fmt) == sc
    # saturation and the sign of zero
    edge = torch.tensor([fmax * 4, -fmax * 4, fmax, -fmax, 0.0, -0.0], dtype=torch.float64)
    top = {R.E4M3: 0x7E, R.E5M2: 0x7B}[fmt]
    assert R.ref_quantize(edge, 1.0, fmt).tolist() == [top, top | 0x80, top, top | 0x80, 0x00, 0x80]


@pytest.mark.parametrize('fmt', [R.E4M3, R.E5M2])
def test_exact_grids_hold_ties_both_ways_and_subnormal_codes(fmt):
    for tdt in TDTS:
        for k in (-3, 0, 5):
            x, is_mid = R.exact_grid(fmt, k, tdt)
            assert R.grid_properties(x, is_mid, fmt, k) == (True, True, True), (fmt, tdt, k)
            assert int(is_mid.sum()) == 2 * (int(R.decode_table(fmt)[1][:128].sum()) - 1)
            half_tiny = 2.0 ** k * {R.E4M3: 2.0 ** -10, R.E5M2: 2.0 ** -17}[fmt]     # half the smallest subnormal ties to zero
            at = x.double() == half_tiny
            assert bool(at.any()) and bool((R.ref_quantize(x.double(), 2.0 ** k, fmt)[at] == 0).all())


def test_quantiser_rows_have_the_launch_shapes_they_name():
    for q in T.Q_ROWS:
        vecs = q.M * (q.C // 16)
        if q.name == 'one_block':
            assert T.q_blocks(q) == 1
        if q.name == 'm43606_blocks_cap':
            assert vecs // 256 + 1 == T.K_AMAX_BLOCKS == T.q_blocks(q)
        if q.M == 70001:
            assert 2 * T.K_AMAX_BLOCKS * 256 < vecs < 3 * T.K_AMAX_BLOCKS * 256 and vecs % 256 != 0
        r, c = T.amax_index(q)
        assert 0 <= r < q.M and 0 <= c < q.C
        if q.amax_at == 'second_trip':
            assert r * (q.C // 16) + c // 16 >= 2 * T.K_AMAX_BLOCKS * 256
        if q.amax_at == 'last':
            assert r * (q.C // 16) + c // 16 == vecs - 1
    assert {q.amax_at for q in T.Q_ROWS if q.M == 70001} == {'first', 'last', 'second_trip'}


Q_SHAPES = sorted({(q.M, q.C) for q in T.Q_ROWS})


@pytest.mark.parametrize('shape', Q_SHAPES, ids=['%dx%d' % s for s in Q_SHAPES])
def test_ambiguity_caps_of_the_gaussian_quantiser_cases(shape):
    """the condition of the Gaussian test: at most max(4, 1e-4 M C) elements may take either of two bytes; the planted amax keeps
    the scale away from a power of two.  (One placement of the amax element per shape: the rows of a shape share every other
    element, and the GPU test asserts the cap of its own row before it launches.)"""
    M, C_ = shape
    for tdt in TDTS:
        x = R.gauss_input(M, C_, tdt, (0, 3)).double()
        for fmt in (R.E4M3, R.E5M2):
            s = R.expected_scale(R.GAUSS_AMAX, fmt)
            assert np.frexp(s)[0] != 0.5, 'the scale is a power of two (test data)'
            n = int(R.ambiguous(x, s, fmt).sum())
            print(f'{M} x {C_} {tdt} fmt {fmt}: {n} ambiguous of {x.numel()}')
            assert n <= max(4, 1e-4 * M * C_), (shape, tdt, fmt, n)


def test_tiny_amax_inputs_leave_the_reciprocals_range():
    """amax = 2^-120 (fp32) / 2^-118 (bf16): the scale is an fp32 subnormal in both formats, and its fp32 reciprocal is +inf for
    amax < FMAX 2^-128 -- both formats in fp32, e5m2 in bf16"""
    overflow = []
    for tdt in TDTS:
        x = R.tiny_input(tdt)
        a = float(x.double().abs().max())
        assert a == R.TINY_AMAX[tdt] and bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any())
        for fmt in (R.E4M3, R.E5M2):
            s = R.expected_scale(a, fmt)
            assert 0 < s < 2.0 ** -126                               # an fp32 subnormal
            with np.errstate(over='ignore', divide='ignore'):
                inf = bool(np.isinf(np.float32(1.0) / np.float32(s)))
            assert inf == (a < R.FMAX[fmt] * 2.0 ** -128)
            overflow.append(inf)
    assert overflow == [True, True, False, True]


def test_case_table_against_the_queries_and_all_24_members():
    seen = set()
    for r in T.ROWS:
        M = T.rows_of(r)
        assert r.cinp % 16 == 0 and r.coutp % 16 == 0 and r.Cin <= r.cinp and r.Cout <= r.coutp
        wide = M < T.SMALL_ROWS
        for dgrad, form in ((False, r.fwd), (True, r.dgrad)):
            d = T.make_desc(r, dgrad=dgrad)
            assert T.query(d, dgrad) == form, (r.name, 'dgrad' if dgrad else 'fwd', T.query(d, dgrad), form)
            if wide:       # the pitches of the frames do not move the row
                kp, op = (r.coutp, r.cinp) if dgrad else (r.cinp, r.coutp)
                assert T.query(T.make_desc(r, ld_src=kp + 32, ld_out=op + 24, dgrad=dgrad), dgrad) == form
            assert M % form.bm != 0, (r.name, 'the last row tile is full')
        seen.update(T.members(r))
    assert sorted(seen) == sorted(T.REQUIRED) and len(T.REQUIRED) == 24, sorted(set(T.REQUIRED) - seen)
    kp = {p for r in T.ROWS for p in (r.cinp, r.coutp)}
    assert {64, 128, 16, 48, 80, 144} <= kp
    # the statistics layout of the forward follows the same tile
    lib = __import__('dualvar_amd._lib', fromlist=['load']).load()
    for r in T.ROWS:
        d = T.make_desc(r, flags=T.DV_STATS)
        assert lib.dv_conv3d_tile_rows(C.byref(d)) == r.fwd.bm
        assert lib.dv_conv3d_stat_tiles(C.byref(d)) == -(-T.rows_of(r) // r.fwd.bm)


@pytest.mark.skipif(torch.cuda.is_available(), reason='a library without the check would launch: CPU-only hosts only')
def test_fp8_entries_refuse_bad_arguments():
    """every refusal that launches nothing: in each call every other argument is valid, so the named one is the only reason
    (-1 DV_EINVAL, -2 DV_EALIGN, -3 DV_EUNSUPPORTED).  y, dx, stats, q and scale_out point at host sentinels that must not change."""
    from dualvar_amd import _lib as L
    lib = L.load()
    r = T.BY_NAME['s196_k64_n48']
    p = 1 << 20                                     # non-null, 16-byte aligned; never dereferenced
    sentinel = np.full(4096 + 16, 0x5A, dtype=np.uint8)
    out = (sentinel.ctypes.data + 15) & ~15         # a 16-byte aligned host address for every output

    def fwd(edit=None, x=p, w=p, sx=p, sw=p, y=None, stats=None, flags=0):
        d = T.make_desc(r, flags=flags)
        if edit:
            edit(d)
        return lib.dv_conv3d_fwd_fp8(C.byref(d), x, w, sx, sw, out if y is None else y, stats, None)

    def dgr(edit=None, dy=p, w=p, sdy=p, sw=p, dx=None, flags=0):
        d = T.make_desc(r, flags=flags, dgrad=True)
        if edit:
            edit(d)
        return lib.dv_conv3d_dgrad_fp8(C.byref(d), dy, w, sdy, sw, out if dx is None else dx, None)

    def ed(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    def quant(dtype=L.DV_F32, x=p, M=64, C_=32, ld=32, fmt=0, q=None, ldq=32, scale=None, ws=p):
        return lib.dv_quantize_fp8(dtype, x, M, C_, ld, fmt, out if q is None else q, ldq, out + 1024 if scale is None else scale, ws, None)

    unsupported = [
        fwd(ed(kt=3, pt=1)), dgr(ed(kt=3, pt=1)), fwd(ed(kh=3, ph=1)), fwd(ed(kw=3, pw=1)),            # not pointwise
        fwd(ed(sh=2, Ho=7)), dgr(ed(sh=2, Ho=7)), fwd(ed(sw=2, Wo=7)),                                 # a stride
        fwd(ed(dtype=L.DV_F32)), dgr(ed(dtype=L.DV_F32)), fwd(ed(dtype=7)),                            # the bf16 side must be DV_BF16
        quant(dtype=7),
    ]
    assert all(rc == -3 for rc in unsupported), unsupported
    align = [
        fwd(ed(cin_pitch=72, ldx=80)), fwd(ed(cout_pitch=56, ldy=56)), dgr(ed(cin_pitch=72, ldx=72)), dgr(ed(cout_pitch=56, ldy=64)),
        fwd(x=p + 4), fwd(w=p + 8), fwd(y=out + 4), dgr(dy=p + 4), dgr(w=p + 2), dgr(dx=out + 8),        # pointers
        fwd(ed(ldx=68)), dgr(ed(ldy=52)), fwd(ed(ldy=52)), dgr(ed(ldx=68)),                            # row pitches in bytes
        quant(x=p + 4), quant(q=out + 4), quant(ld=34), quant(dtype=L.DV_BF16, ld=36),
    ]
    assert all(rc == -2 for rc in align), align
    inval = [
        fwd(sx=None), fwd(sw=None), dgr(sdy=None), dgr(sw=None),                                       # null scales
        fwd(x=None), fwd(w=None), dgr(dy=None), dgr(w=None),
        lib.dv_conv3d_fwd_fp8(C.byref(T.make_desc(r)), p, p, p, p, None, None, None),
        lib.dv_conv3d_dgrad_fp8(C.byref(T.make_desc(r, dgrad=True)), p, p, p, p, None, None),
        lib.dv_conv3d_fwd_fp8(None, p, p, p, p, out, None, None), lib.dv_conv3d_dgrad_fp8(None, p, p, p, p, out, None),
        fwd(flags=T.DV_STATS),                                                                          # DV_STATS without stats
        fwd(ed(cin_pitch=48)), fwd(ed(ldx=48)), fwd(ed(N=0)),
        quant(x=None), quant(M=0), quant(C_=0), quant(C_=24, ld=24, ldq=32), quant(ld=16), quant(ldq=16), quant(ldq=40), quant(fmt=2),
        quant(ws=None), lib.dv_quantize_fp8(L.DV_F32, p, 64, 32, 32, 0, None, 32, out, p, None),
        lib.dv_quantize_fp8(L.DV_F32, p, 64, 32, 32, 0, out, 32, None, p, None),
    ]
    assert all(rc == -1 for rc in inval), [i for i, rc in enumerate(inval) if rc != -1]
    assert lib.dv_quantize_fp8_workspace() == T.K_AMAX_BLOCKS * 4
    assert bool((sentinel == 0x5A).all()), 'a refused call wrote to its output'
