/* Feature spectrum of libdualvar_hip.so (csrc/spectrum.hip): the covariance of the clip features from the augmented Gram matrix
 * of dualvar_ridge.h, and its eigen-decomposition by a parallel-ordered one-sided Jacobi method in double, beside
 * dualvar_select.h, dualvar_pairstat.h, dualvar_tsne.h, dualvar_cluster.h and dualvar_ridge.h.  Same conventions: plain C,
 * device pointers, the stream last, 0 on success, DV_E* (< 0) for refused arguments before anything is launched, a hipError_t
 * (> 0) for a failed launch.  There are no atomics of any kind and no hand-off between workgroups but the launch boundary: every
 * sum below has one stated order, so the same inputs give the same bits.  The library is built with -ffp-contract=off: every
 * product, quotient, sum and square root below is rounded on its own.
 * ctypes mirror: dualvar_amd/_lib.py SPECTRUM_SIGNATURES (tests/test_spectrum_host.py compares the two).
 *
 * THE DOT PRODUCT of two rows x, y of length n, used by every entry below ("the stated order"): thread t of the 256 of a
 * workgroup starts at 0.0 and adds the rounded products x[i] * y[i] for i = t, t + 256, t + 512, ... < n in ascending order; the
 * 256 partials are then folded by the tree  for s = 128, 64, ..., 1: part[t] = part[t] + part[t + s] (t < s); part[0] is the
 * result.
 *
 * THE METHOD.  For a symmetric A [n][n], W starts as A (row p of W = row p of A) and V as the identity.  A rotation of the row
 * pair (p, q) replaces (w_p, w_q) and (v_p, v_q) by an orthogonal combination that makes w_p and w_q orthogonal, so W = V A
 * holds throughout and V stays orthogonal.  When all rows of W are mutually orthogonal, W W^T = V A^2 V^T is diagonal: the rows
 * of V are eigenvectors of A^2, and of A itself when A is positive semi-definite (a covariance; a pair of eigenvalues +l, -l of
 * an indefinite matrix is not separated), with the eigenvalue lambda_j = v_j . w_j / v_j . v_j.  A sweep visits every pair once, in
 * dv_spectrum_rounds(n) rounds of disjoint pairs (below); the rounds are launches, the pairs of a round are workgroups that own
 * their two rows of W and V and their two words of stat and touch nothing else. */
#ifndef DUALVAR_SPECTRUM_H
#define DUALVAR_SPECTRUM_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_SPECTRUM_MAX_D 4096       /* the largest matrix order n (the widest feature row) */
#define DV_SPECTRUM_MAX_SWEEPS 64    /* the host's cap on sweeps: 22 to 29 were needed at condition numbers of 1e8 to 1e12 */
#define DV_SPECTRUM_BLOCK 256        /* threads of a workgroup: the stride of the dot product above */

/* mean and covariance (divisor n) of the rows whose augmented Gram matrix G [D + 1][ldg] dv_ridge_gram_f64 formed with C = 1
 * and every label 0: s_j = G[D][j] (the column sums), n = G[D][D] (the rows).
 *   mean[j]   = s_j / n
 *   Cov[i][j] = (G[i][j] - (s_i * s_j) / n) / n        a product, a quotient, a difference and a quotient, each rounded, in
 *                                                      that order
 * One thread per element of Cov; both triangles are written and, G being symmetric bit for bit, are equal bit for bit.  Only
 * Cov[i][0..D) for i < D and mean[0..D) are written.
 * DV_EINVAL: null pointers, D < 1, D > DV_SPECTRUM_MAX_D, ldg < D + 1, ldc < D.  DV_EALIGN: G, Cov or mean not 8-byte aligned. */
int dv_spectrum_cov_f64(const double* G, int64_t ldg, int32_t D, double* Cov, int64_t ldc, double* mean, void* stream);

/* The rounds of a sweep over n rows: m - 1 with m = n rounded up to even; 0 for n == 1.  DV_EINVAL for n < 1 or
 * n > DV_SPECTRUM_MAX_D. */
int dv_spectrum_rounds(int32_t n);

/* The pair of slot k (0 <= k < m / 2) of round `round` (0 <= round < m - 1), the round-robin (circle) schedule:
 *   slot 0:       (m - 1, round)
 *   slot k >= 1:  ((round + k) mod (m - 1), (round - k) mod (m - 1))
 * returned with *p < *q.  The slots of a round are disjoint and cover 0 .. m - 1; every unordered pair occurs in exactly one
 * round.  A pair with *q >= n (odd n: the partner of index m - 1 = n) is the bye: the kernel skips it.  The kernel and this
 * query call one function.  DV_EINVAL: null pointers, n < 1, n > DV_SPECTRUM_MAX_D, round or k out of range. */
int dv_spectrum_pair(int32_t n, int32_t round, int32_t k, int32_t* p, int32_t* q);

/* W[p][0..n) = A[p][0..n) for p < n (A symmetric; its pitch lda), V = the n x n identity, and
 * scale[0] = the Frobenius norm of A = sqrt(sum), by ONE workgroup: thread t starts at 0.0 and adds the rounded squares of the
 * elements e = t, t + 256, ... < n * n in ascending order, e counting the elements row by row (element e is A[e / n][e % n]);
 * the 256 partials are folded by the tree of the dot product above; one square root.
 * Only W[p][0..n), V[p][0..n) for p < n and scale[0] are written.
 * DV_EINVAL: null pointers, n < 1, n > DV_SPECTRUM_MAX_D, lda < n, ldw < n, ldv < n.  DV_EALIGN: A, W, V or scale not 8-byte
 * aligned. */
int dv_spectrum_init_f64(const double* A, int64_t lda, int32_t n, double* W, int64_t ldw, double* V, int64_t ldv, double* scale,
                         void* stream);

/* The rounds [round_lo, round_hi) of a sweep, one launch each, one workgroup of DV_SPECTRUM_BLOCK threads per pair slot.  With
 * (p, q) of dv_spectrum_pair (nothing is done for the bye), a = w_p . w_p, b = w_q . w_q, c = w_p . w_q in the stated order,
 * ra = sqrt(a), rb = sqrt(b), eps = DBL_EPSILON:
 *   above   = min(ra, rb) > eps * scale[0]                       (the floor: a row that has shrunk to round-off is left alone;
 *                                                                 without it the null rows of a rank-deficient matrix keep
 *                                                                 rotating against each other and the sweeps never end)
 *   rotated = above and |c| > (eps * ra) * rb
 *   zeta = (b - a) / (2 c);  t = copysign(1, zeta) / (|zeta| + sqrt(1 + zeta * zeta));  cs = 1 / sqrt(1 + t * t);  sn = cs * t
 *          (zeta * zeta overflowing to infinity gives t = 0, which is correct)
 *   w_p' = cs * w_p - sn * w_q,  w_q' = sn * w_p + cs * w_q   element by element (two products and a sum or difference, each
 *   rounded), and likewise v_p, v_q.
 * stat [m] doubles (m = n rounded up to even); slot k owns stat[2k] and stat[2k + 1] across rounds, ordered by the launch
 * boundary:
 *   stat[2k]     = max(stat[2k], |c| / (ra * rb)) if above, else unchanged; NaN if a, b or c is NaN (and stays NaN)
 *   stat[2k + 1] = stat[2k + 1] + 1 if rotated.
 * round_lo == 0 clears stat [m] first (a launch of its own), so after rounds [0, dv_spectrum_rounds(n)) the sum of the odd
 * words is the number of rotations of the sweep and the largest even word its largest cosine between two rows.
 * Only rows p < n, columns < n of W and V and stat[0..m) are written; scale is read.
 * DV_EINVAL: null pointers, n < 1, n > DV_SPECTRUM_MAX_D, ldw < n, ldv < n, round_lo < 0, round_lo > round_hi,
 * round_hi > dv_spectrum_rounds(n).  DV_EALIGN: W, V, scale or stat not 8-byte aligned. */
int dv_spectrum_rounds_f64(double* W, int64_t ldw, double* V, int64_t ldv, int32_t n, int32_t round_lo, int32_t round_hi,
                           const double* scale, double* stat, void* stream);

/* lambda[j] = (v_j . w_j) / (v_j . v_j) for j < n, both dot products in the stated order and one division, one workgroup per
 * j: the Rayleigh quotient of v_j, since w_j = A v_j.  The divisor is 1 up to the rounding of the rotations, and exactly 1 for a
 * row of V no rotation has touched (the quotient is then v_j . w_j bit for bit); dividing by it takes the drift of |v_j|^2 out
 * of the eigenvalue.  That drift has one sign over all rows (about +50 eps after 14 sweeps at n = 64), so without the division
 * the sum of the eigenvalues misses the trace by about n / 4 times the error of one eigenvalue.
 * DV_EINVAL: null pointers, n < 1, n > DV_SPECTRUM_MAX_D, ldw < n, ldv < n.  DV_EALIGN: W, V or lambda not 8-byte aligned. */
int dv_spectrum_values_f64(const double* W, int64_t ldw, const double* V, int64_t ldv, int32_t n, double* lambda, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_SPECTRUM_H */
