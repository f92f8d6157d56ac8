"""Models of the kernels' summation orders and of the device functions' intrinsic error: what the derived bounds of the
float64 suites and of tests/plan_audit.py are built from.  Each function names the kernel it models; a kernel that
changes its order changes its model here, and tests/test_checks_host.py pins the values at the shapes where a row-group
count or a fold changes."""
import math

from tests.checks import U, ceil_div, cp8, vec

# Device functions (measured on gfx950 against float64 over 2^20 arguments per range and taken with a factor 2; the
# derivation and the re-measurement are in tests/test_loss_gemm_optim_gpu.py): relative errors
E_LOG, E_LOG1P, E_EXPF = 5.4 * U, 2.1 * U, 2.8 * U
TINY = 2.0 ** -126                # below it __expf may flush to 0: an absolute term next to the relative E_EXP


def e_exp(x):
    """__expf(x): v_exp_f32 of x * log2(e), the product's rounding scaled by |x|"""
    return (4.2 + 4.1 * x.abs()) * U


def gamma(n):
    """n sequential fp32 roundings: n u / (1 - n u)"""
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------- csrc/streaming.hpp, csrc/batchnorm.hip
def column_chain(rows, CP, dtype, NS, extra=0):
    """longest chain of sequential fp32 additions column_reduce (streaming.hpp) forms over `rows` rows of CP columns with NS
    sums per column: rows per thread, then ceil(log2 rg) for the pairwise fold of the rg row groups; `extra` is what the caller
    adds behind it (block folds, or the blocks that add to one replica with float atomics; 0: every output has one owner)"""
    V, CV = vec(dtype), CP // vec(dtype)
    chain = 0
    for cvb in range(0, CV, 256):
        cvc = min(256, CV - cvb)
        rg = 256 // cvc
        while rg > 1 and rg * cvc * V * NS > 4096:
            rg >>= 1
        chain = max(chain, ceil_div(rows, rg) + math.ceil(math.log2(rg)))
    return chain + extra


def bwd_reduce_chain(M, C_, dtype, nblk):
    """longest chain of sequential fp32 additions of bn_bwd_reduce_body + ordered_fold (streaming.hpp): column_chain over
    the rows of one block, the fold of a group of <= 32 block rows, the fold of the groups"""
    return column_chain(ceil_div(M, nblk), cp8(C_), dtype, 2, min(32, nblk) + ceil_div(nblk, 32))


def stats_chain(n_tiles, threads=256):
    """bn_reduce_stats_body with `threads` threads: tiles per thread, the 64-lane shuffle tree, the threads / 64 wave sums in a
    row (256 threads: 4; the single-tensor launch runs 1024 from 2048 tiles: 16)"""
    return ceil_div(n_tiles, threads) + 6 + threads // 64


def m2_bound(n, da, d, Q, dQ, dmean, chain):
    """error bound of the fp32 M2 = sum_i (Q_i + n_i d_i^2), d_i = a_i - mean, evaluated term by term ([terms][C]):
    a_i carries da_i, mean dmean, Q_i dQ_i; then d (1 rounding), n*d*d (2), Q + n d^2 (1), and a fold of `chain` additions"""
    dd = da + dmean + U * (d.abs() + da + dmean)
    ad = d.abs() + dd
    term = Q + dQ + n * ad * ad
    e = dQ + n * (2 * d.abs() * dd + dd * dd) + 2 * U * n * ad * ad + U * term
    return e.sum(0) + chain * U * term.sum(0)


# ------------------------------------------------------------------------------------------------- dv_gemm_f32, csrc/loss.hip
def splitk_plan(M, N, K):
    """gemm_splitk_plan of loss.hip: (tiles, splits, kslice); splits 0 = not split"""
    tiles = ceil_div(M, 32) * ceil_div(N, 32)
    splits = kslice = 0
    if tiles <= 64 and K >= 4096:
        splits = min(1024 // tiles, K // 256)
        kslice = ceil_div(ceil_div(K, splits), 64) * 64
        splits = ceil_div(K, kslice)
    return tiles, splits, kslice


def gemm_form(M, N, K):
    """launch_gemm_f32 of loss.hip: the one-wave kernel, four waves per tile, or split-K"""
    tiles, splits, _ = splitk_plan(M, N, K)
    if splits:
        return 'split'
    return 'tile4' if tiles <= 1024 and K >= 64 else 'plain'


def gemm_chain(M, N, K, form=None):
    """longest chain of sequential fp32 additions of the form taken: K for the one-wave kernel; 16 ceil(ceil(K/16)/4) + 3 for
    the four-wave kernels, the 3 being the LDS fold; for split-K that of one slice plus the number of slices"""
    form = form or gemm_form(M, N, K)
    if form == 'plain':
        return K + (K & 1)
    if form == 'tile4':
        return 16 * ceil_div(ceil_div(K, 16), 4) + 3
    _, splits, kslice = splitk_plan(M, N, K)
    return 16 * ceil_div(ceil_div(kslice, 16), 4) + 3 + splits


def gemm_bound(A64, B64t, alpha, chain):
    """A64 [M][K], B64t [N][K]: (chain + 2) u |alpha| sum_k |a_k b_k|, the + 2 for the product and alpha"""
    return (chain + 2) * U * abs(alpha) * (A64.abs() @ B64t.abs().t())
