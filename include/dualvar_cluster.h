/* Spherical k-means of libdualvar_hip.so (csrc/cluster.hip): the three steps of Lloyd's algorithm on cosine similarity with
 * k-means++ seeding, beside dualvar_select.h, dualvar_pairstat.h and dualvar_tsne.h.  The similarities themselves come from
 * dv_gemm_f32 in row blocks; these entries take the arg-max of a block, rebuild the centroids and draw the next seed.  Same
 * conventions: plain C, device pointers, the stream last, 0 on success, DV_E* (< 0) for refused arguments before anything is
 * launched, a hipError_t (> 0) for a failed launch.  There are no floating-point atomics: every sum below has one stated order,
 * so the same inputs give the same bits.  The library is built with -ffp-contract=off: every expression below is evaluated as
 * written, one IEEE operation per operator.
 * "Block fold" of 256 per-thread doubles: within each wavefront, for o = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l ^ o]; then the
 * four wavefront totals are added in ascending order.
 * ctypes mirror: dualvar_amd/_lib.py CLUSTER_SIGNATURES (tests/test_cluster_host.py compares the two). */
#ifndef DUALVAR_CLUSTER_H
#define DUALVAR_CLUSTER_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_KMEANS_MAX_K 4096         /* the most clusters */
#define DV_KMEANS_PART 64            /* dv_kmeans_update_f32: members of a cluster that one partial sum takes */
#define DV_KMEANS_SORT_ROWS 512      /* dv_kmeans_update_f32: rows per block of the stable counting sort */
#define DV_KMEANS_SEED_BLOCK 256     /* dv_kmeans_seed_f32: rows per block partial */

/* Arg-max of the rows of a row-major block of similarities, sim [R][ld], over the columns j < K.
 * A column is SELECTABLE iff its value is not NaN (-inf and +inf are).  assign[r] = the lowest selectable column holding the
 * row's largest selectable value under the IEEE comparison (so -0.0 equals +0.0 and the lower column wins between them),
 * best[r] = sim[r][assign[r]] as stored.  A row with no selectable column gets assign = -1 and best = -inf.
 * sim[r][K..ld) is never read; rows >= R of assign / best are never touched.
 * *changed (uint64 on the device) is increased, by integer atomics only, by the number of rows r < R whose new assign[r] differs
 * from the value assign[r] held on entry: the host zeroes it once per iteration and the row blocks of that iteration add up to
 * one count.  assign is therefore read before it is written and must be initialised (-1 before the first iteration).
 * Ownership: a row is owned by a group of G adjacent lanes, G = the smallest power of two >= min(K, 64) (1, 2, 4, ..., 64), a
 * workgroup of 256 threads by 256 / G rows (128 rows at K = 2, 4 rows - one wavefront each - from K = 33 on).  Lane g of the
 * group walks the columns g, g + G, g + 2G, ... in ascending order, consecutive lanes reading consecutive addresses, and keeps
 * its first largest; the G candidates are merged over the group in log2 G exchanges (larger value, then lower column).
 * DV_EINVAL: null pointers, R <= 0, K < 1, K > DV_KMEANS_MAX_K, ld < K.  DV_EALIGN: changed not 8-byte aligned. */
int dv_kmeans_assign_f32(const float* sim, int64_t ld, int32_t R, int32_t K, int32_t* assign, float* best, uint64_t* changed,
                         void* stream);

/* Bytes of the workspace of dv_kmeans_update_f32, a function of (n, D, K) only.  With B = ceil(n / DV_KMEANS_SORT_ROWS) sort
 * blocks and P = n / DV_KMEANS_PART + K (integer division; no assignment has more parts):
 *   8 (P D + P + K D)  +  4 (B K + 2 (K + 1) + n),  rounded up to a multiple of 8.
 * < 0 (DV_EINVAL) for n <= 0, D <= 0, K < 1 or K > DV_KMEANS_MAX_K. */
int64_t dv_kmeans_update_workspace(int32_t n, int32_t D, int32_t K);

/* The centroid step.  z [n][ldz] fp32 rows, assign / best [n] as dv_kmeans_assign_f32 leaves them.  For cluster k < K with the
 * members M_k = {r < n : assign[r] == k}, m_0 < m_1 < ... in ascending row order:
 *   counts[k] = |M_k| (int32),   within[k] = sum_{r in M_k} best[r] (double),   s_k[d] = sum_{r in M_k} z[r][d] (double),
 *   cent_out[k][d] = (float) (s_k[d] / sqrt(sum_d s_k[d]^2))      for d < D: a double division, rounded once to fp32.
 * A cluster that is empty, or whose norm is 0 or not finite, gets cent_out[k][0..D) = cent_in[k][0..D) bit for bit; it still
 * reports its count (and its within).  cent_in and cent_out may be the same array.  Rows with assign < 0 or >= K belong to no
 * cluster: neither their z nor their best is read.
 * Order of every sum, a function of (n, D, K, assign) alone.  Part j of cluster k holds the members m_{jL} ... m_{jL + L - 1},
 * L = DV_KMEANS_PART (the last part is short).  A part's sums start at 0.0 and add its members in ascending row order, each
 * fp32 term converted to double first; s_k[d] and within[k] start at 0.0 and add the cluster's parts in ascending j.  The norm:
 * thread t < 256 starts at 0.0 and adds s_k[d] * s_k[d] for d = t, t + 256, ... in ascending order, then the block fold.
 * How the members are found: a stable counting sort of the row indices by cluster.  Blocks of DV_KMEANS_SORT_ROWS rows are
 * counted per cluster (integer LDS atomics), the counts are scanned over blocks and clusters, and one wavefront per block hands
 * out the ranks 64 rows at a time in row order (match by ballot, rank = the equal keys in lower lanes), so the sorted list is
 * the same whichever workgroup runs first.
 * Ownership: a workgroup of 256 threads owns (one part, 256 adjacent columns), a thread one column: each member row is read
 * once, coalesced along D, so a cluster holding every row spreads over n / L workgroups per 256 columns.  The fold of a cluster's
 * parts is owned by (cluster, 256 columns), the norm and the division by one workgroup per cluster.  Seven launches.
 * Only cent_out[k][0..D) for k < K (pitch ldc), counts[0..K) and within[0..K) are written, besides the workspace.
 * DV_EINVAL: null pointers, n <= 0, D <= 0, K < 1, K > DV_KMEANS_MAX_K, ldz < D, ldc < D.
 * DV_EALIGN: within or workspace not 8-byte aligned. */
int dv_kmeans_update_f32(const float* z, int64_t ldz, int32_t n, int32_t D, const int32_t* assign, const float* best, int32_t K,
                         const float* cent_in, float* cent_out, int64_t ldc, int32_t* counts, double* within, void* workspace,
                         void* stream);

/* Similarity of every row to ONE centre, the input of a seeding step:  s[r] = sum_{d < D} z[r][d] * c[d]  for r < n, in fp32.
 * (dv_gemm_f32 at one output column computes the same product, but its 32 x 32 tiles then carry 31 idle columns: measured at
 * n = 37 830, D = 512 it takes 65 us against the 77 MB this entry reads once.)
 * Order.  The elements go in groups of four, group g = d / 4.  Lane l of the row's wavefront owns the groups l, l + 64, ...; it
 * starts at 0.0f and takes its elements in ascending d:  acc = acc + z[r][d] * c[d]  (a product and a sum, each rounded); then
 * the wave fold in fp32: for o = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l ^ o].
 * Ownership: one wavefront per row, four rows per workgroup; 16-byte loads when z and c are 16-byte aligned and ldz and D are
 * multiples of 4, 4-byte loads otherwise - the same order and the same bits either way.
 * Only s[0..n) is written.  DV_EINVAL: null pointers, n <= 0, D <= 0, ldz < D. */
int dv_kmeans_dot_f32(const float* z, int64_t ldz, int32_t n, int32_t D, const float* c, float* s, void* stream);

/* Bytes of the workspace of dv_kmeans_seed_f32: 8 ceil(n / DV_KMEANS_SEED_BLOCK).  < 0 (DV_EINVAL) for n <= 0. */
int64_t dv_kmeans_seed_workspace(int32_t n);

/* One k-means++ step on unit-norm rows.  s[r], r < n, is the similarity of row r to the centre chosen last.  In fp32:
 *   d_r = fmaxf(2.0f - 2.0f * s[r], 0.0f)        (a NaN s[r] gives +0: the squared distance |z_r - c|^2, clamped)
 *   mind[r] = first ? d_r : fminf(mind[r], d_r)  (first != 0: mind is not read)
 * Order.  Block b holds the rows [b W, min(n, (b + 1) W)), W = DV_KMEANS_SEED_BLOCK.  The in-block prefix p_r starts at 0.0 and
 * adds (double) mind of the block's rows in ascending order up to and including r; the block partial is p of its last row.
 * T_0 = 0.0, T_{b+1} = T_b + partial_b in ascending b;  *total (double) = T of the last block;  cum_r = T_b + p_r.
 * *pick (int32) = the first row r, in ascending order, with cum_r > u * total (one double multiplication), where 0 <= u < 1 comes
 * from the host.  cum is non-decreasing and a row with mind[r] == 0 repeats the value before it, so such a row is never picked.
 * total == 0 (every row at distance 0): *pick = -1 and the host draws uniformly.  If total > 0 and no row qualifies (u * total
 * rounds up to total, or total is not finite) *pick = the last row with mind[r] > 0.
 * Ownership: first launch, a thread owns a row and thread 0 of each workgroup of W rows adds the block in order from LDS;
 * second launch, one workgroup stages the partials in LDS and its thread 0 walks them twice (total, then the block) and the
 * chosen block once.
 * DV_EINVAL: null pointers, n <= 0, u < 0, u >= 1 or NaN.  DV_EALIGN: total or workspace not 8-byte aligned. */
int dv_kmeans_seed_f32(const float* s, int32_t n, float* mind, int32_t first, double u, int32_t* pick, double* total,
                       void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_CLUSTER_H */
