"""The case table of tests/test_conv_float64_gpu.py and of the CPU route test in tests/test_abi_and_host.py.

Every row is one convolution problem with the kernels it is EXPECTED to run on, written out as literals: the forward's and
the data gradient's route (`route_conv` of csrc/conv.hip: path, GEMM tile, LDS-staged kind and rows, K-split columns, rows
and number of the BatchNorm partial tiles) and the weight gradient's plan (`plan_wgrad`, the one decision its launch and
its queries read: tile, row splits, workspace, and whether the fused BatchNorm forms take it).  The expectations are read back through the host-side queries of
include/dualvar_hip.h (no device needed), so

* the CPU test proves on any machine that every row still runs where it was written for (a routing threshold that moves a
  case is named there, not found by accident as `ks64` was), and that the table as a whole reaches every member of
  the list written out in that test;
* the GPU test asserts the same row before it launches, so a number in its output belongs to the kernel the row names.

Forms that no query reports (gather kind, LDS stages, plain or pre-split weights, BatchNorm on load) are named by the
property that selects them in `gemm_form` -- channel pitch, taps, grid size, DV_W3 -- and derived here by `members`.

No torch and no GPU in this file: ctypes and the library's host code only.
"""
import ctypes as C
from collections import namedtuple

from tests.checks import cp8

F32, BF16 = 0, 1
DV_BIAS, DV_RELU, DV_SIGMOID, DV_ACCUM, DV_STATS, DV_W3 = 1, 2, 4, 8, 16, 128

Fwd = namedtuple('Fwd', 'path bm bn kind tap_rows ks rows tiles')
Dgrad = namedtuple('Dgrad', 'path bm bn kind tap_rows ks w3')
Wgrad = namedtuple('Wgrad', 'rows cols splits workspace bn_ok')
Case = namedtuple('Case', 'name N Cin T H W Cout k s p dtype w3 cinp data fwd dgrad wgrad bn_in dgrad_bn_ws')


def out_dims(c):
    return tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((c.T, c.H, c.W), c.k, c.s, c.p))


def cin_pitch(c):
    return c.cinp if c.cinp else cp8(c.Cin)


def make_desc(c, flags=0, ldx=None, ldy=None):
    """dv_conv_desc of the row (dense pitches unless given); `flags` are added to the row's DV_W3"""
    from dualvar_amd import _lib as L
    d = L.ConvDesc()
    d.dtype, d.N, d.Ti, d.Hi, d.Wi, d.Cin = c.dtype, c.N, c.T, c.H, c.W, c.Cin
    d.To, d.Ho, d.Wo = out_dims(c)
    d.Cout = c.Cout
    d.kt, d.kh, d.kw = c.k
    d.st, d.sh, d.sw = c.s
    d.pt, d.ph, d.pw = c.p
    d.cin_pitch, d.cout_pitch = cin_pitch(c), cp8(c.Cout)
    d.ldx, d.ldy = ldx or d.cin_pitch, ldy or d.cout_pitch
    d.flags = flags | (DV_W3 if c.w3 else 0)
    return d


def _path(d, dgrad, kind, ks):
    """the ROUTE_* member of route_conv from what the queries report; the strided-data-gradient condition is route_conv's own
    (strides <= 2, every parity class has a tap)"""
    strided = max(d.st, d.sh, d.sw) > 1
    classes = (dgrad and strided and max(d.st, d.sh, d.sw) <= 2 and d.kt >= d.st and d.kh >= d.sh and d.kw >= d.sw)
    if kind == 3:
        return 'PP'
    if kind:
        return 'TAP_CLASSES' if classes else 'TAP'
    if ks:
        return 'KS'
    return 'GEMM_CLASSES' if classes else 'GEMM'


def query_fwd(d):
    from dualvar_amd import _lib as L
    lib = L.load()
    r, cc = C.c_int32(), C.c_int32()
    assert lib.dv_conv3d_tile_shape(C.byref(d), 0, C.byref(r), C.byref(cc)) == 0
    kind, ks = lib.dv_conv3d_tap_kind(C.byref(d), 0), lib.dv_conv3d_ksplit_cols(C.byref(d), 0)
    return Fwd(_path(d, 0, kind, ks), r.value, cc.value, kind, lib.dv_conv3d_tap_rows(C.byref(d), 0), ks,
               lib.dv_conv3d_tile_rows(C.byref(d)), lib.dv_conv3d_stat_tiles(C.byref(d)))


def query_dgrad(d):
    """A strided data gradient takes pre-split weights on the LDS-staged kernel only (route_conv: every parity class there,
    or DV_EUNSUPPORTED); elsewhere the caller hands over the plain dgrad layout.  `w3` says which the row uses."""
    from dualvar_amd import _lib as L
    lib = L.load()
    if (d.flags & DV_W3) and max(d.st, d.sh, d.sw) > 1 and not lib.dv_conv3d_tap_kind(C.byref(d), 1):
        d.flags &= ~DV_W3
    r, cc = C.c_int32(), C.c_int32()
    assert lib.dv_conv3d_tile_shape(C.byref(d), 1, C.byref(r), C.byref(cc)) == 0
    kind, ks = lib.dv_conv3d_tap_kind(C.byref(d), 1), lib.dv_conv3d_ksplit_cols(C.byref(d), 1)
    return Dgrad(_path(d, 1, kind, ks), r.value, cc.value, kind, lib.dv_conv3d_tap_rows(C.byref(d), 1), ks, bool(d.flags & DV_W3))


def query_wgrad(d):
    from dualvar_amd import _lib as L
    lib = L.load()
    r, cc, sp = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.dv_conv3d_wgrad_tile(C.byref(d), C.byref(r), C.byref(cc), C.byref(sp)) == 0
    return Wgrad(r.value, cc.value, sp.value, int(lib.dv_conv3d_wgrad_workspace(C.byref(d))), lib.dv_conv3d_wgrad_bn_ok(C.byref(d)))


def query_extras(d):
    from dualvar_amd import _lib as L
    lib = L.load()
    return lib.dv_conv3d_bn_in_ok(C.byref(d)), int(lib.dv_conv3d_dgrad_bn_workspace(C.byref(d)))


def query(c):
    """(fwd, dgrad, wgrad, bn_in_ok, dgrad_bn_workspace) as the library reports them for the row.  The weight gradient takes
    no DV_W3 (its operands are activations); the RGB input has no data gradient."""
    d = make_desc(c)
    dw = make_desc(c)
    dw.flags = 0
    bn_in, bn_ws = query_extras(d)
    return query_fwd(d), (None if c.Cin <= 4 else query_dgrad(make_desc(c))), query_wgrad(dw), bn_in, bn_ws


# ---------------------------------------------------------------------------------------------------------------- the table
# name, N, Cin, T, H, W, Cout, k, s, p, dtype, DV_W3, channel pitch of x (None: cp8(Cin)), data kinds the GPU test runs
# (G1 G2 G3: the exact grids, B: Gaussian data inside the derived bound), then the expectations:
#   Fwd(path, GEMM tile rows, cols, tap kind, tap rows, K-split cols, rows per BatchNorm partial tile, partial tiles)
#   Dgrad(path, GEMM tile rows, cols, tap kind, tap rows, K-split cols, weights pre-split)     (None: the RGB / one-channel input has none)
#   Wgrad(tile rows, cols, row splits, workspace bytes, dv_conv3d_wgrad_bn_ok), dv_conv3d_bn_in_ok, dv_conv3d_dgrad_bn_workspace
# (dv_conv3d_tile_shape reports pick_tile's answer on every path; it is the launched tile on GEMM only.)
CASES = [
    Case('pw_c64_m294', 3, 64, 2, 7, 7, 24, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 5), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 2, 12288, 1), 0, 0),
    Case('pw_c24_m16384', 4, 24, 4, 32, 32, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 64, 0, 0, 0, 64, 256), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 64, 393216, 1), 0, 0),
    Case('sp3_c40_m16384', 4, 40, 4, 32, 32, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 128, 0, 0, 0, 64, 256), Dgrad('TAP', 64, 64, 1, 128, 0, True), Wgrad(64, 128, 64, 11796480, 1), 0, 133120),
    Case('sp3_c128_c40_m16384', 4, 128, 4, 32, 32, 40, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('TAP', 64, 64, 1, 128, 0, 128, 128), Dgrad('GEMM', 64, 128, 0, 0, 0, True), Wgrad(64, 128, 52, 9584640, 1), 0, 0),
    Case('pw_c24_m131072', 8, 24, 4, 64, 64, 24, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0, True, None, 'G1 B',
         Fwd('GEMM', 128, 32, 0, 0, 0, 128, 1024), Dgrad('GEMM', 128, 32, 0, 0, 0, True), Wgrad(64, 128, 512, 1179648, 1), 0, 0),
    Case('pw_c256_m65536', 4, 256, 4, 64, 64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 128, 128, 0, 0, 0, 128, 512), Dgrad('GEMM', 128, 128, 0, 0, 0, True), Wgrad(128, 128, 128, 33554432, 0), 0, 0),
    Case('pw_c64_m131072', 8, 64, 4, 64, 64, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), 0, True, None, 'G1 G3 B',
         Fwd('GEMM', 256, 64, 0, 0, 0, 256, 512), Dgrad('GEMM', 256, 64, 0, 0, 0, True), Wgrad(64, 128, 512, 8388608, 1), 0, 0),
    Case('rgb_stem_sp7', 2, 3, 4, 30, 30, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 0, True, 4, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 29), None, Wgrad(64, 128, 8, 401408, 1), 0, 0),
    Case('w5x7x7_c8', 1, 8, 6, 12, 12, 32, (5, 7, 7), (1, 1, 1), (2, 3, 3), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 14), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 4, 1003520, 1), 0, 0),
    Case('tap_sp_m12544', 4, 64, 4, 28, 28, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 G3 B',
         Fwd('TAP', 64, 32, 1, 128, 0, 128, 98), Dgrad('TAP', 64, 32, 1, 128, 0, True), Wgrad(64, 128, 49, 7225344, 1), 0, 117760),
    Case('tap_tm_m12544', 4, 64, 4, 28, 28, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('TAP', 64, 32, 2, 128, 0, 128, 98), Dgrad('TAP', 64, 32, 2, 128, 0, True), Wgrad(64, 192, 22, 1081344, 0), 1, 117760),
    Case('tap_sp_m50176', 4, 64, 4, 56, 56, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 G3 B',
         Fwd('TAP', 64, 64, 1, 128, 0, 128, 392), Dgrad('TAP', 64, 64, 1, 128, 0, True), Wgrad(64, 192, 98, 14450688, 0), 0, 272896),
    Case('tap_sp_c192_m100352', 8, 64, 4, 56, 56, 192, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 B',
         Fwd('TAP', 256, 64, 1, 256, 0, 256, 392), Dgrad('TAP', 64, 64, 1, 128, 0, True), Wgrad(64, 192, 83, 36716544, 0), 0, 479744),
    Case('tap_tm_t2', 8, 64, 2, 32, 32, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('TAP', 64, 64, 2, 128, 0, 128, 128), Dgrad('TAP', 64, 64, 2, 128, 0, True), Wgrad(64, 192, 32, 1572864, 0), 1, 133120),
    Case('tap_tm_t8', 2, 32, 8, 28, 28, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 B',
         Fwd('TAP', 64, 32, 2, 256, 0, 256, 49), Dgrad('TAP', 64, 32, 2, 256, 0, True), Wgrad(64, 128, 49, 1204224, 1), 0, 117760),
    Case('ks32_m72', 8, 192, 1, 3, 3, 384, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 G3 B',
         Fwd('KS', 64, 32, 0, 0, 32, 64, 2), Dgrad('KS', 64, 32, 0, 0, 32, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('ks64_m6080', 4, 96, 4, 20, 19, 96, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('KS', 64, 32, 0, 0, 64, 64, 95), Dgrad('KS', 64, 32, 0, 0, 64, True), Wgrad(64, 128, 24, 7962624, 1), 0, 0),
    Case('ks_trim_t', 4, 384, 1, 3, 3, 384, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 B',
         Fwd('KS', 64, 32, 0, 0, 32, 64, 1), Dgrad('KS', 64, 32, 0, 0, 32, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('ks_trim_hw', 16, 256, 2, 1, 1, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('KS', 64, 32, 0, 0, 32, 64, 1), Dgrad('KS', 64, 32, 0, 0, 32, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('gemm_trim_t', 3, 64, 1, 3, 3, 96, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 1), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('gemm_trim_hw', 4, 48, 1, 1, 5, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 1), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('stem_tm7_m12544', 4, 64, 8, 28, 28, 64, (7, 1, 1), (2, 1, 1), (3, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 196), Dgrad('TAP_CLASSES', 64, 64, 2, 256, 0, True), Wgrad(64, 224, 22, 2523136, 0), 0, 169472),
    Case('stem_tm7_m131072', 8, 64, 8, 64, 64, 64, (7, 1, 1), (2, 1, 1), (3, 0, 0), 0, True, None, 'G1 B',
         Fwd('GEMM', 256, 64, 0, 0, 0, 256, 512), Dgrad('TAP_CLASSES', 256, 64, 2, 256, 0, True), Wgrad(64, 224, 205, 23511040, 0), 2, 1146880),
    Case('pair_stem_pp', 5, 6, 8, 117, 59, 64, (1, 7, 4), (1, 2, 1), (0, 0, 0), 0, True, None, 'G1 G2 G3 B',
         Fwd('PP', 64, 64, 3, 224, 0, 224, 560), Dgrad('GEMM_CLASSES', 128, 32, 0, 0, 0, False), Wgrad(64, 224, 280, 16056320, 1), 0, 0),
    Case('pair_stem_small', 2, 8, 4, 20, 22, 64, (1, 7, 4), (1, 2, 1), (0, 0, 0), 0, True, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 17), Dgrad('GEMM_CLASSES', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 5, 286720, 1), 0, 0),
    Case('c83_tm3', 1, 83, 4, 6, 6, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 3), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('c144_c230_sp3', 2, 144, 2, 7, 7, 230, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('KS', 64, 32, 0, 0, 32, 64, 4), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('c1_c1_sp3', 2, 1, 2, 5, 5, 1, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 2), None, Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('c40_c3_sp3', 2, 40, 2, 5, 5, 3, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, True, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 2), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('w1x9x9_c16', 1, 16, 2, 12, 12, 32, (1, 9, 9), (1, 1, 1), (0, 4, 4), 0, True, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 5), Dgrad('GEMM', 64, 32, 0, 0, 0, True), Wgrad(64, 128, 2, 331776, 0), 0, 0),
    Case('now3_stem_tm7', 2, 64, 8, 9, 9, 64, (7, 1, 1), (2, 1, 1), (3, 0, 0), 0, False, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 11), Dgrad('GEMM_CLASSES', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 3, 344064, 1), 0, 0),
    Case('now3_full3_s2', 2, 32, 4, 8, 8, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), 0, False, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 1), Dgrad('GEMM_CLASSES', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('now3_sp3_s2_c83', 1, 64, 2, 8, 8, 83, (1, 3, 3), (1, 2, 2), (0, 1, 1), 0, False, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 1), Dgrad('GEMM_CLASSES', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('now3_full3_s2_t1', 2, 32, 1, 8, 8, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), 0, False, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 1), Dgrad('GEMM_CLASSES', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('now3_pw_s2', 2, 64, 4, 8, 8, 42, (1, 1, 1), (1, 2, 2), (0, 0, 0), 0, False, None, 'G1 G2 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 2), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('now3_sp3_c24', 2, 24, 2, 7, 7, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 0, False, None, 'G1 G2 G3 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 4), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 1, 0, 1), 0, 0),
    Case('bf_rgb_stem', 2, 3, 4, 30, 30, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 1, False, 4, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 29), None, Wgrad(64, 128, 8, 401408, 0), 0, 0),
    Case('bf_sp3_c24', 2, 24, 2, 7, 7, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 4), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(128, 128, 1, 0, 0), 0, 0),
    Case('bf_sp3_c64', 2, 64, 2, 7, 7, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 4), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(128, 128, 1, 0, 0), 0, 0),
    Case('bf_pw_c64_m131072', 8, 64, 4, 64, 64, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), 1, False, None, 'G1 B',
         Fwd('GEMM', 128, 64, 0, 0, 0, 128, 1024), Dgrad('GEMM', 128, 64, 0, 0, 0, False), Wgrad(128, 128, 512, 8388608, 0), 0, 0),
    Case('bf_sp3_c192_m100352', 8, 64, 4, 56, 56, 192, (1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False, None, 'G1 B',
         Fwd('GEMM', 128, 64, 0, 0, 0, 128, 784), Dgrad('GEMM', 64, 64, 0, 0, 0, False), Wgrad(192, 256, 85, 37601280, 0), 0, 0),
    Case('bf_sp3_c320_m3136', 4, 160, 4, 14, 14, 320, (1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 49), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(128, 256, 9, 16588800, 0), 0, 0),
    Case('bf_pw_c512_m1568', 4, 512, 2, 14, 14, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 25), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(128, 128, 7, 7340032, 0), 0, 0),
    Case('bf_sp3_c64_m25088', 8, 64, 4, 28, 28, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 64, 0, 0, 0, 64, 392), Dgrad('GEMM', 64, 64, 0, 0, 0, False), Wgrad(64, 256, 79, 11649024, 0), 0, 0),
    Case('bf_w1x9x9_c16', 1, 16, 2, 12, 12, 32, (1, 9, 9), (1, 1, 1), (0, 4, 4), 1, False, None, 'G1 B',
         Fwd('GEMM', 64, 32, 0, 0, 0, 64, 5), Dgrad('GEMM', 64, 32, 0, 0, 0, False), Wgrad(64, 128, 2, 331776, 0), 0, 0),
]
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------- what the table covers
def _live(k, odim, idim, stride, pad):
    """taps of one axis that reach the tensor for at least one output position (trim_dead_taps, forward form)"""
    return [d for d in range(k) if any(0 <= o * stride - pad + d < idim for o in range(odim))]


def _classes(c):
    """(parity classes of the strided data gradient that have positions, whether one has none): dgrad_classes"""
    n = empty = 0
    for rt in range(c.s[0]):
        for rh in range(c.s[1]):
            for rw in range(c.s[2]):
                first = [((r - p) % s + s) % s for r, p, s in zip((rt, rh, rw), c.p, c.s)]
                if any(f >= dim for f, dim in zip(first, (c.T, c.H, c.W))):
                    empty += 1
                else:
                    n += 1
    return n, empty > 0


def _gemm_members(c, mode, bm, bn, M, NP, cp, classes, w3):
    """the conv_gemm form gemm_form picks, named by the properties that select it"""
    out = []
    taps = c.k[0] * c.k[1] * c.k[2]
    if not classes:
        out.append('%s:tile:%dx%d' % (mode, bm, bn))
    if c.dtype == F32:
        if not w3:
            out.append('f32:plain-split')
        elif cp % 16 == 0 and taps <= 32:
            out.append('f32:w3:uniform-tap')
        else:
            out.append('f32:w3:generic:' + ('taps>32' if taps > 32 and cp % 16 == 0 else 'cp%d' % cp))
            if taps > 32:
                out.append('f32:w3:generic:taps>32')
    else:
        out.append('bf16:gather%d' % (16 if cp % 8 == 0 else 8))
        if cp % 8 == 0:
            out.append('bf16:cp%32==0' if cp % 32 == 0 else 'bf16:cp%32!=0')
        if not classes:
            grid = -(-NP // bn) * -(-M // bm)
            out.append('bf16:stages4' if cp % 8 == 0 and bm == 64 and grid <= 512 else 'bf16:stages2')
    return out


def members(c):
    """the coverage members (tests/test_abi_and_host.py: CONV_REQUIRED) this row reaches, from its geometry and its EXPECTED route (the literals of the table)"""
    out = ['row:' + c.name]
    To, Ho, Wo = out_dims(c)
    Mo, Mi = c.N * To * Ho * Wo, c.N * c.T * c.H * c.W
    f, g, w = c.fwd, c.dgrad, c.wgrad
    strided = max(c.s) > 1
    trim = ''
    if not strided:       # (stride 1: the live taps of the data gradient are the forward's, mirrored)
        lt, lh, lw = (_live(k, o, i, 1, p) for k, o, i, p in zip(c.k, (To, Ho, Wo), (c.T, c.H, c.W), c.p))
        trim = ('t' if len(lt) < c.k[0] else '') + ('hw' if len(lh) < c.k[1] or len(lw) < c.k[2] else '')
    for mode, r, M, NP, cp in (('fwd', f, Mo, cp8(c.Cout), cin_pitch(c)), ('dgrad', g, Mi, cin_pitch(c), cp8(c.Cout))):
        if r is None:
            continue
        out.append('%s:path:%s' % (mode, r.path))
        if r.path in ('GEMM', 'GEMM_CLASSES'):
            out += _gemm_members(c, mode, r.bm, r.bn, M, NP, cp, r.path == 'GEMM_CLASSES', c.w3 if mode == 'fwd' else r.w3)
        if r.path == 'KS':
            out.append('%s:ks%d' % (mode, r.ks))
        if r.path in ('TAP', 'TAP_CLASSES'):
            out += ['tap:kind%d' % r.kind, 'tap:rows%d' % r.tap_rows]
        w3_mode = c.w3 if mode == 'fwd' else r.w3          # trim_dead_taps: not on the generic-gather pre-split-weight path
        if trim and r.path in ('GEMM', 'KS') and not (w3_mode and (cp % 16 != 0 or c.k[0] * c.k[1] * c.k[2] > 32)):
            out += ['trim:%s:%s' % (ax, r.path) for ax in (('t', 'hw') if trim == 'thw' else (trim,))]
        if mode == 'dgrad' and r.path in ('GEMM_CLASSES', 'TAP_CLASSES'):
            n, empty = _classes(c)
            out += ['dgrad:classes:%d' % n, 'dgrad:classes:' + ('w3' if r.w3 else 'no-w3')]
            if empty:
                out.append('dgrad:classes:empty-class')
    if strided and g is not None and g.path == 'GEMM':
        out.append('dgrad:strided-generic(k<s)')
    if c.bn_in:
        out.append('bn-on-load:%d' % c.bn_in)
    # the weight gradient: the LDS-staged forms by their geometry (wgrad_tm_kind), else the DMA kernel's table row, else conv_wgrad_kernel
    tm = {(64, 192, (3, 1, 1)): 1, (64, 224, (7, 1, 1)): 2, (64, 192, (1, 3, 3)): 3, (64, 224, (1, 7, 4)): 4}
    dt = 'f32' if c.dtype == F32 else 'bf16'
    if c.dtype == F32 and (w.rows, w.cols, c.k) in tm:
        out.append('wgrad:tm%d' % tm[(w.rows, w.cols, c.k)])
    elif (c.dtype == BF16 and cin_pitch(c) % 8 != 0) or max(c.k) > 8:
        out.append('wgrad:%s:conv_wgrad_kernel:%s' % (dt, 'window>8' if max(c.k) > 8 else 'no-16-byte-gather'))
    else:
        out.append('wgrad:%s:dma:%dx%d' % (dt, w.rows, w.cols))
    out.append('wgrad:splits=1' if w.splits == 1 else 'wgrad:splits>1')
    if w.bn_ok:
        out.append('wgrad:bn-ok')
    if c.dgrad_bn_ws:
        out.append('dgrad-bn:ordered')
    for ch in (c.Cin, c.Cout):
        if ch in (1, 3, 24, 40, 83, 144, 230):
            out.append('channels:%d' % ch)
    return out


# Members only a DUALVAR_* switch reaches (read once per process: a child pytest each).  NOT COVERED YET: the table has no rows
# for them and tests/test_conv_float64_gpu.py starts no child process.  (Said here in words; nothing asserts on it.)  The fp8
# pair has a table and a float64 file of its own: tests/fp8_cases.py, tests/test_fp8_float64_gpu.py.
NOT_COVERED_YET = {
    'DUALVAR_CONV_TAP_GRID=1': 'the LDS-staged kernels on small ragged shapes (tools/tap_check.py runs them against torch float64)',
    'DUALVAR_WGRAD_F32S=0|2': 'conv_wgrad_f32s_kernel, the opt-in second fp32 weight-gradient form (conv_experiments.hip)',
    'DUALVAR_F32_EXACT=1': 'the f32-input MFMA kernels (tests/test_ops_gpu.py runs them against torch fp32 in its A/B mode)',
    'DUALVAR_CONV_TAP_BM128': 'the LDS-staged kernel with its 128-row tiles switched off',
    'bf16:G2,G3': 'DV_BF16 rows run G1 (with ties) and Gaussian data only; the multi-plane grids are not bf16 numbers as written',
    'route:NONE': 'refused calls (DV_EUNSUPPORTED) launch nothing; tests/test_abi_and_host.py checks the refusals',
}
