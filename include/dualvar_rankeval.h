/* Full-ranking retrieval figures of libdualvar_hip.so (csrc/rankeval.hip): the rank of every positive of every query in the
 * full ordering of the bank, from a streaming count and without a sort of the bank, and from the ranks the average precision,
 * hits@k, R-precision's numerator and the first positive's rank.  Beside the training ABI of dualvar_hip.h and the evaluation
 * entries of dualvar_select.h / dualvar_pairstat.h.  Same conventions: plain C, device pointers, the stream last, 0 on success,
 * DV_E* (< 0) for refused arguments before anything is launched, a hipError_t (> 0) for a failed launch.
 * ctypes mirror: dualvar_amd/_lib.py RANKEVAL_SIGNATURES (tests/test_rankeval_host.py compares the two).
 *
 * Items and order.  A block is a row-major [R][n_cols] piece of similarities, element (r, j) = sim[r*ld + j], exactly as in
 * dv_pairstat_accum_f32; sim[r][n_cols..ld) is never read.  Column j is the bank item col0 + j; the column id pointers are those
 * of the block's first column.  For row r, item j is VALID unless excluded:
 *   exclude == 0  nothing is excluded
 *   exclude == 1  the self pair j == r + diag is excluded (a diag that no (r, j) satisfies disables it)
 *   exclude == 2  every pair with row_vid[r] == col_vid[j] is excluded
 * row_vid and col_vid are read only when exclude == 2 (they may be null otherwise); diag is read only when exclude == 1.
 * Excluded items appear in no list and no count.  The key of an item is its similarity with NaN replaced by -inf and -0.0 by
 * +0.0; +inf and -inf are ordinary values (unlike dv_topk_merge_f32, a -inf item is valid and ranks last).  Valid items are in
 * the total order of dualvar_select.h: a precedes b iff key_a > key_b, or the keys are equal and idx_a < idx_b (idx = the bank
 * index).  The 1-based position of an item in this order is its RANK.  A valid item is a POSITIVE of r iff
 * col_cls[j] == row_cls[r] (ids are compared for equality only; any int32 is allowed).
 *
 * The chain, per block of rows:  gather over every column chunk -> sort -> count over the same column chunks -> finish.
 * The column ranges of successive gather calls (and of successive count calls) must be disjoint and the same set; their order
 * does not matter.  With p_0 .. p_{P-1} the sorted positives of r, the count adds, for every valid item j (the positives
 * included), one to hist[r][b_j], b_j = #{i : p_i precedes j or p_i is j}; then rank(p_i) = 1 + sum_{b <= i} hist[r][b] and
 * sum_{b <= P} hist[r][b] is the number of valid items.  Everything is integer or a fixed sequence of IEEE operations: the same
 * inputs give the same bits however the columns are cut and in whatever order the chunks arrive.  There are no floating-point
 * atomics. */
#ifndef DUALVAR_RANKEVAL_H
#define DUALVAR_RANKEVAL_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_RANKEVAL_MAX_POS 4096

/* Appends the block's positives (key, col0 + j) to the rows' lists  pos_val f32 [R][ldp], pos_idx i32 [R][ldp].
 * first != 0: the lists are empty on entry (pos_cnt is not read); first == 0: they are what earlier calls left.
 * pos_cnt[r] counts every positive found, also beyond ldp; an entry is written only to a slot < ldp, so nothing is written
 * beyond the pitch and pos_cnt[r] > ldp tells the host that the list overflowed.  Slots are handed out by an integer atomic:
 * the order of a list's entries is not defined until dv_rankeval_sort has run.
 * Written: pos_cnt[0..R), and the slots [old count, min(new count, ldp)) of each row of pos_val / pos_idx.  Nothing else.
 * DV_EINVAL: null pointers (sim, row_cls, col_cls, pos_val, pos_idx, pos_cnt; row_vid or col_vid when exclude == 2), R <= 0,
 * n_cols <= 0, ld < n_cols, ldp < 1, ldp > DV_RANKEVAL_MAX_POS, exclude outside 0..2, col0 < 0, col0 + n_cols overflowing
 * int32. */
int dv_rankeval_gather_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0,
                           const int32_t* row_cls, const int32_t* col_cls, const int32_t* row_vid, const int32_t* col_vid,
                           int32_t exclude, int64_t diag,
                           float* pos_val, int32_t* pos_idx, int32_t ldp, int32_t* pos_cnt, int32_t first, void* stream);

/* Sorts the first min(pos_cnt[r], ldp) entries of each row's list in place in the order above (one workgroup per row, a
 * bitonic network in LDS).  The indices of a list are distinct, so the result does not depend on the order gather left.
 * Only those entries are written; pos_cnt is read only.
 * DV_EINVAL: null pointers, R <= 0, ldp < 1, ldp > DV_RANKEVAL_MAX_POS. */
int dv_rankeval_sort(float* pos_val, int32_t* pos_idx, int32_t ldp, const int32_t* pos_cnt, int32_t R, void* stream);

/* Counts the block's valid items against the sorted lists:  hist u32 [R][ldh], hist[r][b_j] += 1 (b_j above, found by one
 * binary search of the list; with n = min(pos_cnt[r], ldp) entries in the list, 0 <= b_j <= n).
 * first != 0: hist[r][0..n] is zeroed first (in the same stream); first == 0: hist is what earlier calls left.
 * A workgroup stages its row's list and a histogram in LDS (12 bytes per list slot, sized from ldp), streams a span of the row's
 * columns and flushes its non-zero buckets with 32-bit integer atomic adds, which commute.  Rows are read with 16-byte loads
 * when sim is 16-byte aligned and ld is a multiple of 4, with 4-byte loads otherwise; the result is the same either way.
 * Written: hist[r][0..n] of rows r < R.  pos_val, pos_idx and pos_cnt are read only.
 * DV_EINVAL: null pointers (sim, pos_val, pos_idx, pos_cnt, hist; row_vid or col_vid when exclude == 2), R <= 0, n_cols <= 0,
 * ld < n_cols, ldp < 1, ldp > DV_RANKEVAL_MAX_POS, ldh < ldp + 1, exclude outside 0..2, col0 < 0, col0 + n_cols overflowing
 * int32. */
int dv_rankeval_count_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0,
                          const int32_t* row_vid, const int32_t* col_vid, int32_t exclude, int64_t diag,
                          const float* pos_val, const int32_t* pos_idx, int32_t ldp, const int32_t* pos_cnt,
                          uint32_t* hist, int32_t ldh, int32_t first, void* stream);

/* The per-query figures from the counts.  With P = min(pos_cnt[r], ldp) and the ranks rho_0 < rho_1 < ... of row r:
 *   rank[r][i] = rho_i = 1 + sum_{b <= i} hist[r][b], i < P          rank i32 [R][ldp]; [P..ldp) is not written
 *   ap[r] = (sum over ascending i of (double)(i + 1) / (double)rho_i) / (double)P, every operation in IEEE double in that
 *           order, uncontracted;  P == 0: ap[r] = -1.0 (a sentinel the host leaves out)
 *   first_rank[r] = rho_0 (0 when P == 0)
 *   hits[r][q] = #{i : rho_i <= ks[q]}, q < n_k                      hits i32 [R][n_k], dense
 *   rhits[r] = #{i : rho_i <= P}    (the numerator of R-precision)
 *   n_valid[r] = sum_{b <= P} hist[r][b]    (the number of valid items of the row)
 * ks i32 [n_k] lives on the device and is not validated here: an entry < 1 gives hits 0.  n_k == 0: ks and hits are not
 * touched (they may be null).  hist and pos_cnt are read only.
 * DV_EINVAL: null pointers (hist, pos_cnt, rank, ap, first_rank, rhits, n_valid; ks or hits when n_k > 0), R <= 0, ldp < 1,
 * ldp > DV_RANKEVAL_MAX_POS, ldh < ldp + 1, n_k outside 0..16.
 * DV_EALIGN: ap not 8-byte aligned. */
int dv_rankeval_finish(const uint32_t* hist, int32_t ldh, const int32_t* pos_cnt, int32_t ldp, int32_t R,
                       const int32_t* ks, int32_t n_k,
                       int32_t* rank, double* ap, int32_t* first_rank, int32_t* hits, int32_t* rhits, int32_t* n_valid,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_RANKEVAL_H */
