"""The case tables of tests/test_batchnorm_single_gpu.py: the single-tensor BatchNorm entries (dv_bn_reduce_stats,
dv_bn_stats_finalize, dv_bn_finalize, dv_bn_apply, dv_bn_bwd_reduce, dv_bn_bwd_apply) at the shapes where their wrappers in
csrc/batchnorm.hip decide something on their own.  Every row writes out as literals what it was written to hit; the reduce
literals are read back through dv_bn_bwd_blocks / dv_bn_bwd_reduce_workspace and the others recomputed from the launch rules
quoted below by tests/test_abi_and_host.py::test_bn_case_table_blocks_and_coverage, without a GPU, so a retune that moves a
row off its edge is named there.  The shapes are the smallest that reach each edge; C stays small wherever M is large.

The launch rules, as csrc/batchnorm.hip has them (column_reduce and ordered_fold: csrc/streaming.hpp):
  dv_bn_reduce_stats / dv_bn_stats_finalize   grid C, block n_tiles >= 2048 ? 1024 : 256; the last tile holds M - (n_tiles-1) tile_rows rows
  dv_bn_finalize                              grid ceil(C / 128), block 128
  dv_bn_apply                                 total = M * (CP / V) vectors, grid min(4096, ceil(total / 256)), block 256, grid-stride
  dv_bn_bwd_reduce                            grid dv_bn_bwd_blocks(M, C), rows per block ceil(M / grid); column_reduce walks the
                                              CV = CP / V channel vectors 256 at a time; ordered_fold groups 32 blocks
  dv_bn_bwd_apply                             as dv_bn_apply with a cap of 2048 blocks; 3 CP floats of LDS <= 60 KiB (C <= 5120)
(CP = C rounded up to 8, V = 4 fp32 / 8 bf16 values per 16-byte vector)"""
from collections import namedtuple

from dualvar_amd import _lib as L
from tests.checks import ceil_div, cp8

STATS_WIDE_FROM = 2048          # n_tiles from which the statistics launch runs 1024 threads
APPLY_CAP, BAPPLY_CAP = 4096, 2048
BLOCK = 256
FOLD_GROUP = 32
BAPPLY_MAX_C = 5120


# the rules above as csrc spells them: (text, {file it lives in: occurrences there}).  The case-table test finds each in its
# home as often as quoted and in none of the other files it lists, so a block size, cap or limit that is retuned there has to
# be retuned in this file's rules (and rows) too.
QUOTED_RULES = [
    ('constexpr int kThreads = 256;', {'streaming.hpp': 1}),
    ('static inline int grid_for(int64_t work_items, int max_blocks = 4096) {', {'common.hpp': 1}),   # shared with optim.hip
    ('int64_t b = (work_items + 255) / 256;', {'common.hpp': 1}),                  # ... in blocks of kThreads
    ('dim3(C), dim3(n_tiles >= 2048 ? 1024 : kThreads)', {'batchnorm.hip': 2}),    # dv_bn_reduce_stats, dv_bn_stats_finalize
    ('hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 127) / 128), dim3(128)', {'batchnorm.hip': 1}),
    ('hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(grid_for(total)), dim3(kThreads)', {'batchnorm.hip': 1}),
    ('int grid = grid_for(total, 2048);', {'batchnorm.hip': 1}),                   # dv_bn_bwd_apply
    ('if (3 * CP * 4 > 60 * 1024) return DV_EUNSUPPORTED;', {'batchnorm.hip': 1}),
    ('const int64_t rpb = (M + blocks - 1) / blocks;', {'batchnorm.hip': 1, 'pool.hip': 1}),   # dv_bn_bwd_reduce; its max-pool twin
    ('constexpr int kFoldGroup = 32;', {'ordered_fold.hpp': 1}),                    # shared with the other ordered folds
    ('for (int cvb = 0; cvb < CV; cvb += kThreads) {', {'streaming.hpp': 1}),      # column_reduce
]

# ------------------------------------------------------------------------------------------------------------ statistics
# M = (n_tiles - 1) * tile_rows + last_rows.  pitch_extra > 0: the partials are channels [8, 8 + C) of a [2][C + 8 + extra][tiles]
# table.  threads: the block size the launch is expected to use.
StatsCase = namedtuple('StatsCase', 'name n_tiles tile_rows last_rows C pitch_extra threads')
STATS_CASES = [
    StatsCase('t1_r64_full', 1, 64, 64, 3, 0, 256),
    StatsCase('t255_r128_one', 255, 128, 1, 8, 0, 256),
    StatsCase('t257_r256_full', 257, 256, 256, 1, 0, 256),
    StatsCase('t257_r224_one_sliced', 257, 224, 1, 3, 5, 256),
    StatsCase('t2047_r224_one', 2047, 224, 1, 3, 0, 256),
    StatsCase('t2047_r64_full_sliced', 2047, 64, 64, 8, 3, 256),
    StatsCase('t2048_r64_full', 2048, 64, 64, 8, 0, 1024),
    StatsCase('t2048_r224_one_sliced', 2048, 224, 1, 3, 5, 1024),
    StatsCase('t2049_r128_one', 2049, 128, 1, 1, 0, 1024),
    StatsCase('t5000_r64_full_sliced', 5000, 64, 64, 3, 2, 1024),
    StatsCase('t5000_r64_one', 5000, 64, 1, 8, 0, 1024),
    # BatchNorm1d of the classifier head: one tile that holds every row
    StatsCase('bn1d_m2_c8', 1, 2, 2, 8, 0, 256),
    StatsCase('bn1d_m7_c136', 1, 7, 7, 136, 0, 256),
    StatsCase('bn1d_m128_c128', 1, 128, 128, 128, 0, 256),
    StatsCase('bn1d_m7_c512', 1, 7, 7, 512, 0, 256),
]

# ------------------------------------------------------------------------------------------------------------ finalize
# counts: rows of each rank (unequal); stride = 2C + 1 + stride_extra, the member's row at `base` floats inside it;
# blocks: ceil(C / 128)
FinalizeCase = namedtuple('FinalizeCase', 'name counts C stride_extra base running blocks')
FINALIZE_CASES = [
    FinalizeCase('r1_c1', (37,), 1, 0, 0, True, 1),
    FinalizeCase('r2_c127', (120, 77), 127, 0, 0, True, 1),
    FinalizeCase('r3_c128_wide', (1000, 1097, 1194), 128, 37, 11, False, 1),
    FinalizeCase('r8_c129_wide', (64, 65, 1, 300, 2, 128, 77, 5), 129, 5, 3, True, 2),
    FinalizeCase('r3_c230', (12544, 12641, 333), 230, 0, 0, False, 2),
    FinalizeCase('r2_c2048_wide', (40, 9), 2048, 64, 32, True, 16),
]

# ------------------------------------------------------------------------------------------------------------ apply
# trip: (fp32, bf16) vectors one grid-stride trip covers (grid * 256); wraps: whether a second trip happens
ApplyCase = namedtuple('ApplyCase', 'name M C relu res views trip wraps')
APPLY_CASES = [
    ApplyCase('c1', 77, 1, True, False, False, (256, 256), (False, False)),
    ApplyCase('c3_res_views', 300, 3, True, True, True, (768, 512), (False, False)),
    ApplyCase('c24_norelu_res', 129, 24, False, True, False, (1024, 512), (False, False)),
    ApplyCase('c83_views', 64, 83, True, False, True, (1536, 768), (False, False)),
    ApplyCase('c230_norelu', 50, 230, False, False, False, (3072, 1536), (False, False)),
    ApplyCase('c2048_res', 9, 2048, True, True, False, (4608, 2304), (False, False)),
    ApplyCase('overcap_m220000_c40', 220000, 40, True, True, True, (1048576, 1048576), (True, True)),
]

# ------------------------------------------------------------------------------------------------------------ backward
# One table for dv_bn_bwd_reduce and dv_bn_bwd_apply.  res: None / 'plain' / 'accum' (dres absent / written / DV_ACCUM);
# n_rep: replicas of the atomic form (every row also runs the ordered form); R: ranks (inv_count = 1 / (R M),
# dparam_scale = 1 / R); dparams: False passes dgamma = dbeta = NULL.
# red: (blocks, rows per block, non-empty blocks, rows of the last non-empty block, fold groups);
# bapply: ((fp32, bf16) vectors per trip, (fp32, bf16) second trip)
BwdCase = namedtuple('BwdCase', 'name M C relu res views n_rep R dparams red bapply')
BWD_CASES = [
    BwdCase('m1_c3', 1, 3, True, None, False, 1, 1, True, (1, 1, 1, 1, 1), ((256, 256), (False, False))),
    BwdCase('m31_c8_nomask', 31, 8, False, 'plain', True, 4, 1, True, (1, 31, 1, 31, 1), ((256, 256), (False, False))),
    BwdCase('m33_c83_accum', 33, 83, True, 'accum', True, 8, 1, True, (2, 17, 2, 16, 1), ((768, 512), (False, False))),
    BwdCase('m2048_c3', 2048, 3, True, None, False, 4, 1, True, (64, 32, 64, 32, 2), ((4096, 2048), (False, False))),
    BwdCase('m2049_c8_nomask_noparams', 2049, 8, False, None, False, 1, 1, False, (33, 63, 33, 33, 2),
            ((4352, 2304), (False, False))),
    BwdCase('m20480_c83', 20480, 83, True, 'plain', False, 4, 1, True, (320, 64, 320, 64, 10), ((450560, 225280), (False, False))),
    BwdCase('m20481_c8_r2', 20481, 8, True, 'accum', True, 8, 2, True, (320, 65, 316, 6, 10), ((41216, 20736), (False, False))),
    BwdCase('m300000_c3_nomask', 300000, 3, False, None, False, 1, 1, True, (1024, 293, 1024, 261, 32),
            ((524288, 300032), (True, False))),
    BwdCase('m300033_c8', 300033, 8, True, 'plain', False, 4, 2, True, (1024, 294, 1021, 153, 32),
            ((524288, 300288), (True, False))),
    BwdCase('c2048_m300', 300, 2048, True, None, False, 1, 1, True, (10, 30, 10, 30, 1), ((153600, 76800), (False, False))),
    BwdCase('overcap_bwd_m220000_c40', 220000, 40, True, 'accum', False, 4, 1, True, (320, 688, 320, 528, 10),
            ((524288, 524288), (True, True))),
    BwdCase('c5120_m40_nomask_noparams', 40, 5120, False, None, False, 1, 1, False, (2, 20, 2, 20, 1),
            ((51200, 25600), (False, False))),
]


# ------------------------------------------------------------------------------------------------------------ the rules
def stats_rows(c):
    return (c.n_tiles - 1) * c.tile_rows + c.last_rows


def stats_threads(n_tiles):
    return 1024 if n_tiles >= STATS_WIDE_FROM else BLOCK


def stride_trip(M, C_, v, cap):
    """(vectors one trip of the capped grid covers, whether a second trip happens) for M rows of CP / v vectors"""
    total = M * (cp8(C_) // v)
    grid = max(1, min(cap, ceil_div(total, BLOCK)))
    return grid * BLOCK, total > grid * BLOCK


def reduce_query(M, C_):
    """(blocks, rows per block, non-empty blocks, rows of the last non-empty block, fold groups, workspace bytes) as the
    library's host queries give them"""
    lib = L.load()
    b = int(lib.dv_bn_bwd_blocks(M, C_))
    rpb = ceil_div(M, b)
    ne = ceil_div(M, rpb)
    return b, rpb, ne, M - (ne - 1) * rpb, ceil_div(b, FOLD_GROUP), int(lib.dv_bn_bwd_reduce_workspace(M, C_))


def workspace_bytes(blocks, C_):
    """ordered_fold_floats (on ordered_fold.hpp's layout functions): [blocks][2 CP] rows, [groups][2 CP] group rows, groups + 1
    ticket words rounded up to 8"""
    g = ceil_div(blocks, FOLD_GROUP)
    return 4 * ((blocks + g) * 2 * cp8(C_) + ((g + 1 + 7) & ~7))


# ------------------------------------------------------------------------------------------------------------ coverage
def members(c):
    """the features a row reaches, derived from the row's literals"""
    out = ['row:' + c.name]
    if isinstance(c, StatsCase):
        M = stats_rows(c)
        out += ['stats:threads%d' % c.threads, 'stats:tiles%d' % c.n_tiles, 'stats:tile_rows%d' % c.tile_rows, 'stats:C%d' % c.C]
        if c.n_tiles > 1:
            out.append('stats:last-tile-one-row' if c.last_rows == 1 else 'stats:last-tile-full' if c.last_rows == c.tile_rows
                       else 'stats:last-tile-ragged')
        if c.pitch_extra:
            out.append('stats:pitch>C:first-channel>0')
        if c.n_tiles == 1 and c.tile_rows == M:
            out += ['bn1d:M%d' % M, 'bn1d:C%d' % c.C]
    elif isinstance(c, FinalizeCase):
        out += ['fin:R%d' % len(c.counts), 'fin:C%d' % c.C, 'fin:blocks%d' % c.blocks,
                'fin:running' if c.running else 'fin:running-null']
        out.append('fin:stride>2C+1:base>0' if c.stride_extra and c.base else 'fin:stride==2C+1' if not c.stride_extra
                   else 'fin:stride>2C+1')
        if len(set(c.counts)) == len(c.counts) and len(c.counts) > 1:
            out.append('fin:unequal-counts')
    elif isinstance(c, ApplyCase):
        out += ['apply:C%d' % c.C, 'apply:relu' if c.relu else 'apply:no-relu']
        if c.res:
            out.append('apply:residual-own-pitch-offset' if c.views else 'apply:residual')
        for dt, w in zip(('f32', 'bf16'), c.wraps):
            out.append('apply:%s:%s' % (dt, 'second-trip' if w else 'one-trip'))
    elif isinstance(c, BwdCase):
        b, rpb, ne, last, grp = c.red
        out += ['red:M%d' % c.M, 'red:C%d' % c.C, 'red:mask-from-y' if c.relu else 'red:no-relu-mask', 'red:ordered',
                'red:atomic:n_rep%d' % c.n_rep, 'bapply:n_rep%d' % c.n_rep, 'bapply:dres-%s' % (c.res or 'absent')]
        if ne < b:
            out.append('red:empty-trailing-blocks')
        if last == 1:
            out.append('red:last-block-one-row')
        if grp > 1:
            out.append('red:fold-groups>1')
        if b % FOLD_GROUP and grp > 1:
            out.append('red:ragged-last-group')
        if b == 320 and c.M < 300000:
            out.append('red:cap320')
        if b == 1024:
            out.append('red:cap1024')
        for dt, v in (('f32', 4), ('bf16', 8)):
            passes = ceil_div(cp8(c.C) // v, BLOCK)
            if passes > 1:
                out.append('red:%s:column-passes%d' % (dt, passes))
        if c.R > 1:
            out.append('bapply:inv_count=1/(R*M):dparam_scale=1/R')
        if not c.dparams:
            out.append('bapply:dgamma-dbeta-null')
        if cp8(c.C) == BAPPLY_MAX_C:
            out.append('bapply:lds-limit')
        for dt, w in zip(('f32', 'bf16'), c.bapply[1]):
            out.append('bapply:%s:%s' % (dt, 'second-trip' if w else 'one-trip'))
    return out


# what the tables as a whole must reach
REQUIRED = (
    ['stats:threads256', 'stats:threads1024', 'stats:last-tile-one-row', 'stats:last-tile-full', 'stats:pitch>C:first-channel>0'] +
    ['stats:tiles%d' % t for t in (1, 255, 257, 2047, 2048, 2049, 5000)] +
    ['stats:tile_rows%d' % r for r in (64, 128, 256, 224)] + ['stats:C%d' % ch for ch in (1, 3, 8)] +
    ['bn1d:M%d' % m for m in (2, 7, 128)] + ['bn1d:C%d' % ch for ch in (8, 128, 136, 512)] +
    ['fin:R%d' % r for r in (1, 2, 3, 8)] + ['fin:C%d' % ch for ch in (1, 127, 128, 129, 230, 2048)] +
    ['fin:unequal-counts', 'fin:stride==2C+1', 'fin:stride>2C+1:base>0', 'fin:running', 'fin:running-null', 'fin:blocks1',
     'fin:blocks2', 'fin:blocks16'] +
    ['apply:C%d' % ch for ch in (1, 3, 24, 83, 230, 2048)] +
    ['apply:relu', 'apply:no-relu', 'apply:residual', 'apply:residual-own-pitch-offset', 'apply:f32:one-trip',
     'apply:bf16:one-trip', 'apply:f32:second-trip', 'apply:bf16:second-trip'] +
    ['red:M%d' % m for m in (1, 31, 33, 2048, 2049, 20480, 20481, 300000, 300033)] + ['red:C%d' % ch for ch in (3, 8, 83)] +
    ['red:mask-from-y', 'red:no-relu-mask', 'red:ordered', 'red:atomic:n_rep1', 'red:atomic:n_rep4', 'red:atomic:n_rep8',
     'red:empty-trailing-blocks', 'red:fold-groups>1', 'red:ragged-last-group', 'red:cap320', 'red:cap1024',
     'red:last-block-one-row', 'red:f32:column-passes2', 'red:f32:column-passes5', 'red:bf16:column-passes3'] +
    ['bapply:n_rep1', 'bapply:n_rep4', 'bapply:dres-absent', 'bapply:dres-plain', 'bapply:dres-accum',
     'bapply:inv_count=1/(R*M):dparam_scale=1/R', 'bapply:dgamma-dbeta-null', 'bapply:lds-limit', 'bapply:f32:second-trip',
     'bapply:bf16:second-trip', 'bapply:f32:one-trip', 'bapply:bf16:one-trip'])
