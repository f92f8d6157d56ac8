"""The case tables of tests/test_fp8_float64_gpu.py and of the CPU test tests/test_fp8_host.py.

GEMM rows: one pointwise (1x1x1, stride 1) problem each, with the conv_gemm tile and the gather form its forward
(dv_conv3d_fwd_fp8) and its data gradient (dv_conv3d_dgrad_fp8) are EXPECTED to run, as literals.  `fp8_impl` of csrc/conv.hip
takes the tile from `pick_tile(DV_BF16, M, NP)` -- what dv_conv3d_tile_shape reports for the bf16 descriptor -- and the
uniform-tap gather iff the K-side channel pitch is a multiple of the 64-byte K tile.  Forward: NP = cout_pitch, K side =
cin_pitch; data gradient: the roles swap.  The CPU test reads every literal back through the query and proves that the table
reaches all 24 members {64x32, 64x64, 64x128, 128x32, 128x64, 128x128} x {uniform, generic} x {fwd, dgrad}; the GPU test asserts
the row before it launches.

How the shapes follow from pick_bn / pick_bm / pick_tile: columns 32 / 64 / 128 by least padding of NP; 128 rows once
ceil(M / 128) * ceil(NP / bn) >= 1024, else 64 rows, narrowed towards 32 columns while the grid has fewer than 256 workgroups.
  64x32    any small problem (M = 196)
  64x64    NP = 64 / 48 / 144 with 256 row tiles: M = 16 330 (last tile 10 rows)
  64x128   NP = 128 / 80 at the same M
  128x128  NP = 512 (4 column tiles): M >= 32 641
  128x64   NP = 192 (3 column tiles): M >= 43 649;  NP = 64: M >= 130 945
  128x32   NP = 32 / 16: M >= 130 945
Every M leaves a ragged last row tile.  K-side pitches: 64, 128, 192, 512 (uniform) and 16, 32, 48, 80, 144 (generic: the last
64-byte K tile lies partly beyond the pitch and must read as zero).

Quantiser rows: the launch shapes of dv_quantize_fp8 (`blocks = min(vecs / 256 + 1, kAmaxBlocks = 512)`, the second kernel on
2 * blocks) with the place of the planted, negative amax element.

No torch and no GPU in this file: ctypes and the library's host code only.
"""
import ctypes as C
from collections import namedtuple

BF16 = 1
DV_ACCUM, DV_STATS = 8, 16
UNIFORM, GENERIC = 'uniform', 'generic'

Form = namedtuple('Form', 'bm bn gather')
Row = namedtuple('Row', 'name N T H W Cin Cout cinp coutp fwd dgrad')

ROWS = [
    # small: both directions on the narrowed 64x32 tile
    Row('s196_k64_n48', 1, 1, 14, 14, 61, 40, 64, 48, Form(64, 32, UNIFORM), Form(64, 32, GENERIC)),
    Row('s196_k48_n64', 1, 1, 14, 14, 45, 64, 48, 64, Form(64, 32, GENERIC), Form(64, 32, UNIFORM)),
    # 256 row tiles of 64 rows, the last one 10 rows
    Row('m16330_k64_n128', 1, 2, 115, 71, 64, 128, 64, 128, Form(64, 128, UNIFORM), Form(64, 64, UNIFORM)),
    Row('m16330_k128_n64', 1, 2, 115, 71, 128, 59, 128, 64, Form(64, 64, UNIFORM), Form(64, 128, UNIFORM)),
    Row('m16330_k48_n80', 1, 2, 115, 71, 48, 77, 48, 80, Form(64, 128, GENERIC), Form(64, 64, GENERIC)),
    Row('m16330_k80_n144', 1, 2, 115, 71, 75, 144, 80, 144, Form(64, 64, GENERIC), Form(64, 128, GENERIC)),
    # 128x128: 256 row tiles x 4 column tiles, the last row tile 10 rows
    Row('m32650_k64_n512', 1, 2, 25, 653, 64, 512, 64, 512, Form(128, 128, UNIFORM), Form(64, 64, UNIFORM)),
    Row('m32650_k16_n512', 2, 1, 25, 653, 16, 505, 16, 512, Form(128, 128, GENERIC), Form(64, 32, UNIFORM)),
    Row('m32650_k512_n64', 1, 2, 25, 653, 512, 64, 512, 64, Form(64, 64, UNIFORM), Form(128, 128, UNIFORM)),
    Row('m32650_k512_n16', 2, 1, 25, 653, 500, 16, 512, 16, Form(64, 32, UNIFORM), Form(128, 128, GENERIC)),
    # 128x64 by three column tiles: 342 row tiles, the last one 12 rows
    Row('m43660_k64_n192', 1, 1, 148, 295, 64, 192, 64, 192, Form(128, 64, UNIFORM), Form(64, 64, UNIFORM)),
    Row('m43660_k192_n48', 1, 1, 148, 295, 192, 43, 192, 48, Form(64, 64, UNIFORM), Form(128, 64, GENERIC)),
    Row('m43660_k192_n64', 1, 1, 148, 295, 185, 64, 192, 64, Form(64, 64, UNIFORM), Form(128, 64, UNIFORM)),
    # 1024 row tiles of 128 rows, the last one 6 rows
    Row('m130950_k64_n32', 1, 2, 675, 97, 64, 32, 64, 32, Form(128, 32, UNIFORM), Form(128, 64, GENERIC)),
    Row('m130950_k16_n32', 1, 2, 675, 97, 16, 27, 16, 32, Form(128, 32, GENERIC), Form(128, 32, GENERIC)),
    Row('m130950_k32_n64', 1, 2, 675, 97, 32, 64, 32, 64, Form(128, 64, GENERIC), Form(128, 32, UNIFORM)),
]
BY_NAME = {r.name: r for r in ROWS}
SMALL_ROWS = 20000            # rows below this run as channel slices of wider buffers (ld > pitch)

REQUIRED = ['%s:%dx%d:%s' % (mode, bm, bn, g) for mode in ('fwd', 'dgrad') for bm in (64, 128) for bn in (32, 64, 128)
            for g in (UNIFORM, GENERIC)]


def rows_of(r):
    return r.N * r.T * r.H * r.W


def gather(k_pitch):
    return UNIFORM if k_pitch % 64 == 0 else GENERIC


def make_desc(r, flags=0, ld_src=None, ld_out=None, dgrad=False):
    """the bf16-side descriptor of the row: pitches of the bf16 tensor in elements, ldx / ldy of the fp8 operand in BYTES"""
    from dualvar_amd import _lib as L
    d = L.ConvDesc()
    d.dtype, d.N, d.Ti, d.Hi, d.Wi, d.Cin = BF16, r.N, r.T, r.H, r.W, r.Cin
    d.To, d.Ho, d.Wo, d.Cout = r.T, r.H, r.W, r.Cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.pt = d.ph = d.pw = 0
    d.cin_pitch, d.cout_pitch = r.cinp, r.coutp
    if dgrad:
        d.ldx, d.ldy = ld_out or r.cinp, ld_src or r.coutp
    else:
        d.ldx, d.ldy = ld_src or r.cinp, ld_out or r.coutp
    d.flags = flags
    return d


def query(d, dgrad):
    """the Form the library will run for descriptor d: the tile through dv_conv3d_tile_shape, the gather from the K-side pitch"""
    from dualvar_amd import _lib as L
    lib = L.load()
    bm, bn = C.c_int32(), C.c_int32()
    assert lib.dv_conv3d_tile_shape(C.byref(d), 1 if dgrad else 0, C.byref(bm), C.byref(bn)) == 0
    return Form(bm.value, bn.value, gather(d.cout_pitch if dgrad else d.cin_pitch))


def members(r):
    return ['fwd:%dx%d:%s' % r.fwd, 'dgrad:%dx%d:%s' % r.dgrad]


# ---- dv_quantize_fp8: (name, M, C, where the amax element sits)
QRow = namedtuple('QRow', 'name M C amax_at')
K_AMAX_BLOCKS = 512
Q_ROWS = [
    QRow('one_block', 5, 16, 'first'),
    QRow('m700_first', 700, 48, 'first'),
    QRow('m700_last', 700, 48, 'last'),
    QRow('m43606_blocks_cap', 43606, 48, 'last'),                   # vecs / 256 + 1 == kAmaxBlocks
    QRow('m70001_first', 70001, 64, 'first'),                       # more than 2 * 512 * 256 vectors: second trips, ragged end
    QRow('m70001_last', 70001, 64, 'last'),
    QRow('m70001_second_trip', 70001, 64, 'second_trip'),
]


def q_blocks(q):
    vecs = q.M * (q.C // 16)
    return min(vecs // 256 + 1, K_AMAX_BLOCKS)


def amax_index(q):
    """(row, column) of the planted amax element: the first vector, the last vector of the last row, or a vector that only the
    second trip of both grid-stride loops reads (vector index in [2 * 512 * 256, vecs))"""
    if q.amax_at == 'first':
        return 0, 3
    if q.amax_at == 'last':
        return q.M - 1, q.C - 2
    vpr = q.C // 16
    vec = 2 * K_AMAX_BLOCKS * 256 + 4321
    assert vec < q.M * vpr
    return vec // vpr, (vec % vpr) * 16 + 5
