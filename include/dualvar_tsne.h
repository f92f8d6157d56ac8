/* t-SNE of libdualvar_hip.so (csrc/tsne.hip): the feature map of the clip features, with sparse attraction over neighbour lists
 * and the exact repulsion over all ordered pairs (no tree, no grid), beside dualvar_select.h and dualvar_pairstat.h.  Same
 * conventions: plain C, device pointers, the stream last, 0 on success, DV_E* (< 0) for refused arguments before anything is
 * launched, a hipError_t (> 0) for a failed launch.  There are no floating-point atomics: every sum below has one stated order,
 * so the same inputs give the same bits.  The library is built with -ffp-contract=off: every fp32 expression below is evaluated
 * as written, one IEEE operation per operator, unless a different unit is named (expf, logf, log1pf, the hardware reciprocal).
 * "Wave fold" of per-lane values v[0..64): for o = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l ^ o] (a fixed tree; all lanes end equal).
 * ctypes mirror: dualvar_amd/_lib.py TSNE_SIGNATURES (tests/test_tsne_host.py compares the two). */
#ifndef DUALVAR_TSNE_H
#define DUALVAR_TSNE_H
#include "dualvar_hip.h"
#include "dualvar_select.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_TSNE_BETA_START 1.0f      /* first beta of the bisection */
#define DV_TSNE_MAX_STEPS 100        /* entropy evaluations per row at most */
#define DV_TSNE_ENTROPY_TOL 1e-5f    /* the bisection stops at |H - log(perplexity)| <= this, H as evaluated in fp32 */
#define DV_TSNE_ROWS 256             /* dv_tsne_repulse_f32: rows per workgroup (one per thread) */
#define DV_TSNE_TILE 256             /* dv_tsne_repulse_f32: columns staged in LDS at a time */

/* Conditional affinities p_{j|r} from neighbour lists as dv_topk_merge_f32 leaves them (dot products of unit-norm rows, so
 * |z_r - z_j|^2 = 2 - 2 s).  Row r < n has the slots j < k1 of top_val / top_idx [n][ldk].
 * Slot j is EXCLUDED iff top_idx[r][j] < 0 or top_idx[r][j] == row0 + r (the point itself, in whichever slot it is).
 * For an included slot, in fp32:  d_j = fmaxf(2.0f - 2.0f * s_j, 0.0f)  (a NaN s_j gives 0),  m = min d_j,
 * e_j = d_j == m ? 0 : d_j - m.
 * Entropy at beta, in fp32:  x_j = beta * e_j,  w_j = expf(-x_j),  S = sum w_j,  A = sum (w_j > 0 ? w_j * e_j : 0),
 * H = logf(S) + (beta * A) / S.  Both sums: lane l adds its slots l, l + 64, l + 128, l + 192 in that order (excluded slots
 * add 0), then the wave fold.
 * Bisection: target = (float) log((double) perplexity); beta = DV_TSNE_BETA_START, lo = 0, hi = +inf; at most
 * DV_TSNE_MAX_STEPS times: evaluate H; stop if |H - target| <= DV_TSNE_ENTROPY_TOL; if H > target: lo = beta and
 * beta = hi == +inf ? beta * 2 : (beta + hi) * 0.5f; else hi = beta and beta = (lo + beta) * 0.5f.  After the last allowed
 * evaluation beta is left as evaluated.  If perplexity is not below the number of included slots the target cannot be met:
 * beta then halves DV_TSNE_MAX_STEPS - 1 times and the row comes out uniform to fp32.
 * Written: p[r][j] = w_j / S at the final beta (w_j, S re-evaluated there as above) for included slots, exactly 0 for excluded
 * slots, for j < k1 only; beta[r].  A row with no included slot: p = 0 and beta = 0.  A row whose d_j are all equal: the
 * bisection is skipped, beta = DV_TSNE_BETA_START and p_j = 1 / (included slots).  No output is ever NaN.
 * One wavefront per row.  p[r][k1..ldk) and rows >= n are never touched.
 * DV_EINVAL: null pointers, n <= 0, k1 < 1, k1 > DV_TOPK_MAX_K, ldk < k1, n * (int64) ldk > 2^31 - 1, row0 < 0,
 * row0 + n overflowing int32, perplexity < 1 or not finite. */
int dv_tsne_perplexity_f32(const float* top_val, const int32_t* top_idx, int32_t ldk, int32_t n, int32_t k1, int32_t row0,
                           float perplexity, float* p, float* beta, void* stream);

/* Attractive force and cross-entropy term of row i < n of the symmetrised affinity P_ij = (p_{j|i} + p_{i|j}) / 2n, which is
 * never formed: row i walks its forward list and then its reverse list, each edge with weight c = p_edge * (0.5f / (float) n).
 * Forward edges: slots s < k1 of row i with p[i][s] > 0 and 0 <= top_idx[i][s] < n; the other point is j = top_idx[i][s].
 * Reverse edges: positions f = rev_edge[e], rev_ptr[i] <= e < rev_ptr[i + 1] (clipped to [0, E]), with 0 <= f < n * ldk and
 * p[f] > 0; the other point is j = f / ldk (the row that lists i).  rev_ptr [n + 1], rev_edge [E] are int32.
 * Per edge, in fp32:  dx = y[i][0] - y[j][0], dy likewise, d2 = dx * dx + dy * dy, q = 1.0f / (1.0f + d2) (IEEE division),
 *   tx = (c * q) * dx,  ty = (c * q) * dy,  tc = c * log1pf(d2).
 * Sums: each term is converted to double; lane l adds the forward slots l, l + 64, ... and then the reverse edges
 * rev_ptr[i] + l, + 64, ... in that order in double; wave fold in double.
 * Written: fa[i][0..2) = (float) of the two sums, ce_row[i] = (float) of the third.  If ce_sum is not null a second launch of
 * one workgroup writes *ce_sum (double) = sum of ce_row: thread t < 256 adds the rows t, t + 256, ... in ascending order in
 * double, the 256 values are folded wave by wave (wave fold) and the four wave totals added in ascending order.
 * One wavefront per row; y (8 n bytes) is gathered and stays in L2.
 * DV_EINVAL: null pointers (ce_sum may be null), n <= 0, n > 2^24 ((float) n must be exact), k1 < 1, k1 > DV_TOPK_MAX_K,
 * ldk < k1, n * (int64) ldk > 2^31 - 1, E < 0.  DV_EALIGN: y or fa not 8-byte aligned, ce_sum not 8-byte aligned. */
int dv_tsne_attract_f32(const float* y, const int32_t* top_idx, const float* p, int32_t ldk, int32_t n, int32_t k1,
                        const int32_t* rev_ptr, const int32_t* rev_edge, int32_t E,
                        float* fa, float* ce_row, double* ce_sum, void* stream);

/* Parts S the columns of dv_tsne_repulse_f32 are split into, a function of n only (written to *parts when not null), and the
 * bytes of its workspace: 24 n S + 8 ceil(n / DV_TSNE_ROWS).  With T = ceil(n / DV_TSNE_TILE) column tiles and
 * B = ceil(n / DV_TSNE_ROWS) row blocks, S = min(T, ceil(1024 / B)): about four workgroups per CU once n allows it.
 * < 0 (DV_EINVAL) for n <= 0. */
int64_t dv_tsne_repulse_workspace(int32_t n, int32_t* parts);

/* Exact repulsion over all ordered pairs:  fr[i][0..2) = sum_{j != i} q_ij^2 (y_i - y_j),  *Z = sum_{i != j} q_ij.
 * Per pair, in fp32:  dx = y[i][0] - y[j][0], dy likewise, t = 1.0f + (dx * dx + dy * dy), q = the hardware reciprocal of t
 * (v_rcp_f32: within 1 ulp of 1 / t, not the IEEE quotient), q2 = q * q, terms q, q2 * dx, q2 * dy.  The pair j == i is
 * skipped: it contributes to neither sum (a duplicate point j != i contributes q = 1 to Z and 0 to fr).  q_ij = q_ji is not
 * exploited: every row walks every column.
 * Order.  A thread owns row i; the columns are walked in tiles of DV_TSNE_TILE staged in LDS.  Within a tile each of the three
 * sums runs in fp32 as two chains, the tile's even columns (c0, c0 + 2, ...) and its odd columns, each in ascending order from
 * 0.0f; the tile's value is even + odd in fp32: at most DV_TSNE_TILE / 2 additions lie above any term.  Tile values are
 * converted to double and added in double in ascending tile order within a part; part s of S takes the tiles
 * [s T / S, (s + 1) T / S) (integer division) and writes its three doubles per row to the workspace.  A second launch adds the
 * parts of a row in ascending s in double, writes fr[i] = (float) of the two sums, and folds the rows' Z of each block of 256
 * rows (wave fold in double, then the four wave totals in ascending order) into the workspace; a third launch of one workgroup
 * adds those block values: thread t adds the blocks t, t + 256, ... in ascending order, then the same fold, and writes *Z.
 * Only fr[0..2n) and *Z are written.
 * DV_EINVAL: null pointers, n <= 0.  DV_EALIGN: y or fr not 8-byte aligned, Z or workspace not 8-byte aligned. */
int dv_tsne_repulse_f32(const float* y, int32_t n, float* fr, double* Z, void* workspace, void* stream);

/* One gradient step with gains and momentum, elementwise over the m = 2n coordinates, in fp32 unless said otherwise:
 *   r    = (float) ((double) fr / *Z)                        (one IEEE double division, rounded to fp32)
 *   g    = 4.0f * (exaggeration * fa - r)
 *   gain = ((g > 0) != (vel > 0)) ? gain + 0.2f : gain * 0.8f;   gain = fmaxf(gain, min_gain)
 *   vel  = momentum * vel - (lr * gain) * g
 *   y    = y + vel
 * *Z is read from the device, so a loop of iterations needs no host synchronisation.  y, vel and gain are updated in place;
 * fa, fr and *Z are only read.
 * DV_EINVAL: null pointers, m <= 0, m > 256 (2^31 - 1), exaggeration, momentum, lr or min_gain not finite, lr < 0, momentum < 0,
 * min_gain < 0.
 * DV_EALIGN: Z not 8-byte aligned. */
int dv_tsne_update_f32(float* y, float* vel, float* gain, const float* fa, const float* fr, const double* Z, int64_t m,
                       float exaggeration, float momentum, float lr, float min_gain, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_TSNE_H */
