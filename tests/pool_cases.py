"""The case tables of tests/test_pool_gate_float64_gpu.py: MaxPool3d problems, per-sample column reductions and the capped
grid-stride launches of csrc/pool.hip, csrc/gate.hip and csrc/elementwise.hip.  Every row names the launch route it was written for; the host-side queries
(dv_maxpool3d_route, dv_spatial_chunks) are compared with those literals by
tests/test_abi_and_host.py::test_pool_case_table_routes_and_coverage, without a GPU, so a threshold that moves a case away
from its route is named there.  The shapes are the smallest that still reach each behaviour."""
import ctypes as C
from collections import namedtuple

from dualvar_amd import _lib as L
from dualvar_amd._lib import DV_BF16, DV_F32
from tests.checks import cp8

GATHER, QUAD, TILE = 0, 1, 2
K333, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)

# fwd / bwd: expected dv_maxpool3d_route per dtype as (route, tile_w, chunk_vecs) for (fp32, bf16); tile_w / chunk_vecs 0
# off route 2.  sliced: x, y, dy, dx are channel slices (offset 8) of wider buffers.  idx4: also run with idx offset by 4 bytes.
PoolCase = namedtuple('PoolCase', 'name N T H W C k s p fwd bwd sliced idx4')
_G = ((GATHER, 0, 0), (GATHER, 0, 0))


def _pc(name, N, T, H, W, C_, k, s, p, fwd=_G, bwd=_G, sliced=False, idx4=False):
    return PoolCase(name, N, T, H, W, C_, k, s, p, fwd, bwd, sliced, idx4)


_T7 = ((TILE, 7, 4), (TILE, 7, 4))             # staged forward, 7-wide tile, 4 vectors per chunk in both dtypes
_T7B = ((TILE, 7, 4), (TILE, 7, 2))            # staged backward: 4 vectors in fp32, 2 in bf16
_Q = ((QUAD, 0, 0), (QUAD, 0, 0))

POOL_CASES = [
    # ---- LDS-staged 3x3x3 / 1 / 1 (Hi*Wi >= 25)
    _pc('st_5x5_t2_c4', 1, 2, 5, 5, 4, K333, S1, P1, _T7, _T7B, idx4=True),        # boundary 25, one ragged tile, cpv < CV
    _pc('g_4x6_t2', 1, 2, 4, 6, 8, K333, S1, P1),                                 # 24 pixels: below the boundary -> gather
    _pc('st_8x15_t1_c36', 1, 1, 8, 15, 36, K333, S1, P1, ((TILE, 14, 4), (TILE, 7, 4)), _T7B),  # TW 14 + 1-wide last tile (fp32 fwd)
    _pc('st_15x8_t5_c72_n3', 3, 5, 15, 8, 72, K333, S1, P1, ((TILE, 14, 4), (TILE, 7, 4)), _T7B),            # tiles along H, groups % 8 != 0, 3-slot ring wraps
    _pc('st_6x6_t2_sliced', 2, 2, 6, 6, 12, K333, S1, P1, _T7, _T7B, sliced=True),
    # ---- 2x2-quad backward (3x3 / stride 2 / padding 1 in h, w); the forward is the gather kernel
    _pc('q_133_7x8', 2, 2, 7, 8, 20, (1, 3, 3), (1, 2, 2), (0, 1, 1), _G, _Q, idx4=True),
    _pc('q_133_1x2', 1, 3, 1, 2, 20, (1, 3, 3), (1, 2, 2), (0, 1, 1), _G, _Q),
    _pc('q_333s2_8x7', 1, 5, 8, 7, 20, K333, (2, 2, 2), P1, _G, _Q),
    _pc('q_333s122_2x1', 2, 3, 2, 1, 20, K333, (1, 2, 2), P1, _G, _Q),
    _pc('q_333s122_7x7', 1, 2, 7, 7, 20, K333, (1, 2, 2), P1, _G, _Q, sliced=True),
    # ---- gather both ways
    _pc('g_222_odd', 2, 3, 5, 7, 12, (2, 2, 2), (2, 2, 2), (0, 0, 0)),             # trailing rows belong to no window
    _pc('g_311_s2', 1, 5, 3, 4, 8, (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    _pc('g_333_p0', 1, 4, 5, 6, 20, K333, S1, (0, 0, 0)),
]

# the fused BatchNorm + ReLU + pool entries run one kernel whatever the geometry: the two stem pools, M a power of two / not
BN_POOL_CASES = [
    _pc('bnp_133_pow2', 1, 2, 8, 8, 12, (1, 3, 3), (1, 2, 2), (0, 1, 1), _G, _Q),
    _pc('bnp_333s2_odd', 2, 3, 7, 5, 20, K333, (2, 2, 2), P1, _G, _Q),
]

# (name, N, S, C per dtype (fp32, bf16), expected dv_spatial_chunks, tag)
ChunkCase = namedtuple('ChunkCase', 'name N S C chunks tag')
CHUNK_CASES = [
    ChunkCase('s127_one_chunk', 2, 127, (196, 392), 1, 'S<128'),
    ChunkCase('s128_partial_last', 2, 128, (196, 392), 4, 'partial-last-chunk'),   # 49 vectors: 13 + 13 + 13 + 10
    ChunkCase('s128_capped_by_n', 400, 128, (196, 392), 3, 'capped-by-N'),         # ceil(1024 / 400) = 3 < ceil(49 / 16) = 4
    ChunkCase('s128_narrow', 3, 128, (64, 128), 1, 'CV<=16'),
    ChunkCase('s128_c50_scalar', 2, 128, (50, 50), 1, 'C%V!=0'),                   # rowscale's scalar path by C % V != 0
]
# the gate-fold level: widths, Ct, S, N; members 1 and 3 read x from slices
GATE_LEVEL = dict(widths=(64, 96, 32, 64), Ct=256, S=128, N=3, sliced=(1, 3), chunks=(4, 2))

# capped grid-stride launches: (entry, blocks cap); each wrap case has cap * 256 work items plus a ragged remainder
WRAP_CAPS = {
    'rowscale0': 4096, 'rowscale1': 4096, 'rowscale2': 4096, 'relu_bwd': 4096, 'ingest': 4096,
    'pool_fwd_gather': 16384, 'pool_bwd_gather': 16384, 'pool_bwd_quad': 16384, 'bn_apply_maxpool': 16384,
    'bn_bwd_apply_maxpool': 2048,
}
# fp32 problems just over each cap (work items = 16-byte vectors, or pixels for ingest / floats for relu_bwd)
WRAP_ROWSCALE = dict(N=16387, S=32, C=8)                                            # 16387 * 32 * 2 = 4096 * 256 + 192
WRAP_RELU_N = 4096 * 256 + 77
WRAP_INGEST = dict(N=1, C=3, T=2, H=724, W=725)                                     # 1 049 800 pixels
WRAP_POOLS = {
    'pool_fwd_gather': _pc('wrap_fwd_311', 1, 2097152 // 4 + 5, 2, 2, 8, (3, 1, 1), S1, (1, 0, 0)),
    'pool_bwd_gather': _pc('wrap_bwd_311', 1, 2097152 // 4 + 5, 2, 2, 8, (3, 1, 1), S1, (1, 0, 0)),
    'pool_bwd_quad': _pc('wrap_quad_333s2', 1, 2097152 + 19, 1, 2, 8, K333, (2, 2, 2), P1, _G, _Q),
    'bn_apply_maxpool': _pc('wrap_bnp_311', 1, 2097152 // 4 + 5, 2, 2, 8, (3, 1, 1), S1, (1, 0, 0)),
    'bn_bwd_apply_maxpool': _pc('wrap_bnpb_133', 1, 2200, 8, 15, 8, (1, 3, 3), (1, 2, 2), (0, 1, 1), _G, _Q),
}


def out_dims(c):
    return tuple((i + 2 * p - k) // s + 1 for i, k, s, p in zip((c.T, c.H, c.W), c.k, c.s, c.p))


def desc(c, dtype, ldx=None, ldy=None):
    d = L.PoolDesc()
    d.dtype = dtype
    d.N, d.Ti, d.Hi, d.Wi, d.C = c.N, c.T, c.H, c.W, c.C
    d.To, d.Ho, d.Wo = out_dims(c)
    d.kt, d.kh, d.kw = c.k
    d.st, d.sh, d.sw = c.s
    d.pt, d.ph, d.pw = c.p
    d.ldx = ldx if ldx is not None else cp8(c.C)
    d.ldy = ldy if ldy is not None else cp8(c.C)
    return d


def query(c, dtype, bwd):
    """(route, tile_w, chunk_vecs) as the library reports it"""
    tw, cv = C.c_int32(0), C.c_int32(0)
    r = L.load().dv_maxpool3d_route(C.byref(desc(c, dtype)), int(bwd), C.byref(tw), C.byref(cv))
    return (r, tw.value, cv.value)


def wrap_items(name, c=None):
    """work items of a wrap case's launch, as the host entry counts them (fp32: 4-channel vectors)"""
    if name.startswith('rowscale'):
        w = WRAP_ROWSCALE
        return w['N'] * w['S'] * (cp8(w['C']) // 4)
    if name == 'relu_bwd':
        return WRAP_RELU_N
    if name == 'ingest':
        w = WRAP_INGEST
        return w['N'] * w['T'] * w['H'] * w['W']
    c = WRAP_POOLS[name]
    cv = cp8(c.C) // 4
    To, Ho, Wo = out_dims(c)
    if name in ('pool_fwd_gather', 'bn_apply_maxpool'):
        return c.N * To * Ho * Wo * cv
    if name == 'pool_bwd_quad':
        return c.N * c.T * ((c.H + 1) // 2) * ((c.W + 1) // 2) * cv
    return c.N * c.T * c.H * c.W * cv


def members(c):
    """what a pool row covers, for the coverage test (derived from the row's literals)"""
    out = ['row:' + c.name]
    names = ('fwd', 'bwd')
    for which, exp in zip(names, (c.fwd, c.bwd)):
        for dt, (r, tw, cv) in zip(('f32', 'bf16'), exp):
            out.append('%s:%s:route%d' % (which, dt, r))
            if r == TILE:
                out.append('%s:%s:tw%d' % (which, dt, tw))
                cpv = cp8(c.C) // (4 if dt == 'f32' else 8)
                nth, ntw = -(-c.H // 7), -(-c.W // tw)
                ncc = -(-cpv // cv)
                if cpv < cv:
                    out.append('tile:cpv<CV')
                if cpv % cv and cpv > cv:
                    out.append('tile:partial-last-chunk')
                if (c.N * nth * ntw * ncc) % 8:
                    out.append('tile:groups%8!=0')
                if tw == 14 and c.W % 14 == 1:
                    out.append('tile:tw14-one-pixel-last-tile')
                if ntw >= 3:
                    out.append('tile:three-tiles-w')
                if nth >= 2:
                    out.append('tile:tiles-along-h')
                if c.H * c.W == 25:
                    out.append('tile:boundary25')
                out.append('tile:T%d' % c.T)
    if c.fwd[1][0] == TILE and c.bwd[1][0] == TILE:
        cpv = cp8(c.C) // 8
        if -(-cpv // c.fwd[1][2]) != -(-cpv // c.bwd[1][2]):
            out.append('tile:bf16-chunks-differ-fwd-bwd')
    if c.k == K333 and c.s == S1 and c.p == P1 and c.H * c.W < 25:
        out.append('staged-shape:below25->gather')
    if c.bwd[0][0] == QUAD:
        out.append('quad:k%d%d%d/s%d%d%d' % (c.k + c.s))
        out += ['quad:H%d' % c.H, 'quad:W%d' % c.W]
        if c.C % 8:
            out.append('quad:pad-lanes')
    if c.bwd[0][0] == GATHER and c.fwd[0][0] == GATHER:
        out.append('gather:k%d%d%d/s%d%d%d/p%d%d%d' % (c.k + c.s + c.p))
    if c.sliced:
        out.append('sliced:route%d' % c.bwd[0][0])
    if c.idx4:
        out.append('idx+4:route%d' % c.bwd[0][0])
    return out
