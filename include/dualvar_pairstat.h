/* Pair statistics of libdualvar_hip.so (csrc/pairstat.hip): the streaming accumulation behind the inter- / intra-video variance
 * report, beside the training ABI of dualvar_hip.h and the selection entries of dualvar_select.h.  Same conventions: plain C,
 * device pointers, the stream last, 0 on success, DV_E* (< 0) for refused arguments before anything is launched, a hipError_t
 * (> 0) for a failed launch.
 * ctypes mirror: dualvar_amd/_lib.py PAIRSTAT_SIGNATURES (tests/test_variance_host.py compares the two). */
#ifndef DUALVAR_PAIRSTAT_H
#define DUALVAR_PAIRSTAT_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_PAIRSTAT_MAX_BINS 256

/* Bytes of `workspace` for one dv_pairstat_accum_f32 call of this R and n_cols (at most 96 KiB); < 0 (DV_EINVAL) for R <= 0 or
 * n_cols <= 0. */
int64_t dv_pairstat_workspace(int32_t R, int32_t n_cols);

/* Streaming statistics over the pairs of a row-major block of similarities: the similarity arrives block by block and only a
 * small state is kept, so the full [n][n] matrix never has to exist.
 *
 * Pairs.  Element (r, j), r < R, j < n_cols, has the value s = sim[r*ld + j].  It is a SELF pair iff j == r + diag; self pairs
 * are skipped (they appear nowhere in the state).  A diag that no (r, j) satisfies disables this (test x train).
 * sim[r][n_cols..ld) is never read.
 * Category of a pair (ids are compared for equality only; any int32 is allowed):
 *   0  same video               row_vid[r] == col_vid[j]
 *   1  same class, other video  the vids differ and row_cls[r] == col_cls[j]
 *   2  different class          the vids and the classes differ
 * A non-finite s (NaN, +inf, -inf) is accumulated nowhere; it is counted in hist[c][bins].
 * Bin of a finite s, all in fp32 and uncontracted (the library is built with -ffp-contract=off):
 *   b = (int)floorf((s + 1.0f) * (0.5f * (float)bins)),  clamped to [0, bins - 1]
 * so values outside [-1, 1] land in the end bins and s = 1 in the last one.
 *
 * State, additive over calls (c = category):
 *   hist  uint64 [3][ldh], ldh >= bins + 1:  hist[c][b] += mult for each pair in bin b, hist[c][bins] += mult for a non-finite one
 *   sums  double [3][4]:  {sum s, sum s^2, sum w, 0}, every term times mult, over the finite pairs;
 *         w = expf((s - 1.0f) * (2.0f * t)), the argument formed in fp32, expf and not __expf (on unit vectors
 *         w = exp(-t |z_i - z_j|^2)); s is converted to double and s*s formed in double, where both are exact
 *   ext   float [3][2]:  {min, max} over the finite pairs; an empty category holds (+inf, -inf)
 * mult is 1 or 2: the host may walk only the blocks on or above the diagonal of a symmetric problem and count the blocks
 * strictly above it twice.
 * first != 0: the state is not read (empty on entry).  first == 0: the state is what earlier calls left.
 * Only hist[c][0..bins], sums and ext are written.
 *
 * Order of summation.  There are no floating-point atomics.  Counts go through integer atomics (an LDS histogram per
 * workgroup, flushed into hist with 64-bit integer adds), which commute.  The call runs G = workspace bytes / 96 workgroups
 * (a function of R and n_cols only); workgroup g takes the 64-row x 1024-column tiles g, g + G, ... (column tiles fastest),
 * every lane keeps nine double sums and six extrema in registers, a workgroup folds its lanes in a fixed tree and writes its
 * partials to workspace[g]; a second launch of ONE workgroup adds the partials in ascending g and adds that total into sums
 * (min / max into ext).  The same sequence of calls therefore gives the same bits.
 *
 * Rows are read with 16-byte loads when sim is 16-byte aligned and ld is a multiple of 4, with 4-byte loads otherwise; the
 * result is the same sum in another association (hist and ext do not depend on it).
 *
 * DV_EINVAL: null pointers (sim, the four id arrays, sums, ext, hist, workspace), R <= 0, n_cols <= 0, ld < n_cols, bins < 1,
 * bins > DV_PAIRSTAT_MAX_BINS, ldh < bins + 1, mult not 1 or 2, t < 0 or not finite, R * (int64) n_cols > 2^32 - 1 (a
 * workgroup counts its pairs in 32-bit LDS counters, which one call of at most 2^32 - 1 pairs cannot overflow; rows, columns
 * and tiles are indexed in unsigned 32 bits, element addresses in 64).
 * DV_EALIGN: sums, hist or workspace not 8-byte aligned. */
int dv_pairstat_accum_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols,
                          const int32_t* row_vid, const int32_t* row_cls, const int32_t* col_vid, const int32_t* col_cls,
                          int64_t diag, int32_t mult, float t, int32_t bins,
                          double* sums, float* ext, uint64_t* hist, int32_t ldh,
                          void* workspace, int32_t first, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_PAIRSTAT_H */
