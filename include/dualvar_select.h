/* Nearest-neighbour selection and the weighted k-NN vote of libdualvar_hip.so (csrc/select.hip): the evaluation entries that
 * stand beside the training ABI of dualvar_hip.h.  Same conventions: plain C, device pointers, the stream last, 0 on success,
 * DV_E* (< 0) for refused arguments before anything is launched, a hipError_t (> 0) for a failed launch.
 * ctypes mirror: dualvar_amd/_lib.py SELECT_SIGNATURES (tests/test_knn_host.py compares the two). */
#ifndef DUALVAR_SELECT_H
#define DUALVAR_SELECT_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_TOPK_MAX_K 256

/* Streaming top-k over the columns of a row-major block of similarities: the similarity arrives in column chunks and only the
 * [R][k] state is kept, so the full [n_test][n_train] matrix never has to exist.
 * State: top_val [R][ldk] f32, top_idx [R][ldk] i32, ldk >= k.  Total order: a precedes b iff
 * val_a > val_b, or val_a == val_b and idx_a < idx_b  (-0.0 == +0.0; it is returned as +0.0).
 * first != 0: the state is not read (empty on entry).  first == 0: the state is what an earlier call left.
 * After the call, row r holds in that order the k first of  state(r) U {(sim[r*ld + j], col0 + j) : 0 <= j < n_cols};
 * slots that could not be filled hold (-inf, -1).  A column whose value is NaN or -inf is never selected.
 * Only top_val[r][0..k) and top_idx[r][0..k) of rows r < R are written; sim[r][n_cols..ld) is never read.
 * The column ranges of successive calls must be disjoint; their order does not matter.
 * One wavefront per row (few rows use little of the GPU); repeated launches give the same bits.
 * DV_EINVAL: null pointers, R <= 0, n_cols <= 0, n_cols > 2^31 - 513 (the kernel walks a row in steps of 256 columns with
 * int32 indices), ld < n_cols, k < 1, k > DV_TOPK_MAX_K, ldk < k, col0 < 0, col0 + n_cols overflowing int32. */
int dv_topk_merge_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0, int32_t k,
                      float* top_val, int32_t* top_idx, int32_t ldk, int32_t first, void* stream);

/* Weighted k-NN vote (the InstDisc / MoCo protocol: k = 200, T = 0.07) over neighbour lists in the order above.  For row r,
 * with the valid neighbours V = {i < k : top_idx[r][i] >= 0 and 0 <= bank_labels[top_idx[r][i]] < n_class}:
 *   w_i = expf((top_val[r][i] - top_val[r][0]) * inv_T)            (inv_T == 0: every w_i = 1, plain majority)
 *   score[r][c] = (sum_{i in V, label_i == c} w_i) / (sum_{i in V} w_i),   sums taken in ascending i
 *   pred[r] = the lowest c with the largest score;  V empty: score row = 0, pred = -1.
 * The lists are expected as dv_topk_merge_f32 leaves them (top_val[r][0] finite and the row's largest wherever a slot is valid).
 * Lists that break this can make the total 0, infinite or NaN (every weight underflows; top_val[r][0] = -inf before valid slots):
 * such a row is treated as V empty (score row = 0, pred = -1), never NaN.
 * score [R][lds], lds >= n_class; only [0..n_class) of rows < R is written.  No float atomics: run-to-run identical bits.
 * DV_EINVAL: null pointers, R <= 0, k < 1, k > DV_TOPK_MAX_K, ldk < k, n_bank <= 0, n_class < 1, n_class > 4096,
 * lds < n_class, inv_T < 0 or not finite.  An index >= n_bank is treated as invalid (not read). */
int dv_knn_vote(const float* top_val, const int32_t* top_idx, int32_t ldk, int32_t R, int32_t k,
                const int32_t* bank_labels, int32_t n_bank, int32_t n_class, float inv_T,
                float* score, int32_t lds, int32_t* pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_SELECT_H */
