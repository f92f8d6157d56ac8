/* Closed-form ridge probe of libdualvar_hip.so (csrc/ridge.hip): the normal equations of multi-class ridge regression onto
 * one-hot targets, formed and solved in double precision, beside dualvar_select.h, dualvar_pairstat.h, dualvar_tsne.h and
 * dualvar_cluster.h.  Same conventions: plain C, device pointers, the stream last, 0 on success, DV_E* (< 0) for refused
 * arguments before anything is launched, a hipError_t (> 0) for a failed launch.  There are no floating-point atomics and no
 * hand-off between workgroups but the launch boundary: every sum below has one stated order, so the same inputs give the same
 * bits.  The library is built with -ffp-contract=off; the only fused operation is the one the f64 MFMA
 * (v_mfma_f64_16x16x4_f64) performs itself.
 * ctypes mirror: dualvar_amd/_lib.py RIDGE_SIGNATURES (tests/test_ridge_host.py compares the two). */
#ifndef DUALVAR_RIDGE_H
#define DUALVAR_RIDGE_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DV_RIDGE_MAX_D 4096          /* the widest feature row (without the constant column) */
#define DV_RIDGE_MAX_C 4096          /* the most classes / right-hand sides */
#define DV_RIDGE_SLAB 512            /* dv_ridge_gram_f64: rows of a slab */
#define DV_RIDGE_MAX_SLABS 8         /* dv_ridge_gram_f64: the most slab partials; beyond it a slab takes a multiple of DV_RIDGE_SLAB rows */
#define DV_RIDGE_TILE 64             /* edge of a tile of G, and the block size of the factorisation */

/* The slabs of n rows: with S = ceil(n / DV_RIDGE_SLAB) and q = ceil(S / DV_RIDGE_MAX_SLABS), a slab holds R = q DV_RIDGE_SLAB
 * adjacent rows (the last one is short) and there are P = ceil(n / R) <= DV_RIDGE_MAX_SLABS of them: R = DV_RIDGE_SLAB up to
 * n = DV_RIDGE_MAX_SLABS * DV_RIDGE_SLAB rows.
 * Bytes of the workspace of dv_ridge_gram_f64 (the slab partials), a function of (n, D, C) only.  With Da = D + 1 and
 * T = ceil(Da / DV_RIDGE_TILE):
 *   8 P (T (T + 1) / 2 * DV_RIDGE_TILE^2  +  C Da)
 * (the lower-triangle tiles of G, then the class sums).  < 0 (DV_EINVAL) for n <= 0, D < 1, D > DV_RIDGE_MAX_D, C < 1 or
 * C > DV_RIDGE_MAX_C. */
int64_t dv_ridge_gram_workspace(int32_t n, int32_t D, int32_t C);

/* The normal equations of the rows z [n][ldz] (fp32) with an implicit constant column: zt_r = (z_r[0..D), 1), Da = D + 1.
 * A row is LIVE iff 0 <= label[r] < C; any other row is skipped whole: its z is loaded at most, never multiplied or added, so
 * a NaN in it does not reach the output.
 *   G[i][j] (+)= sum_{live r} zt_r[i] zt_r[j]              for i, j < Da (pitch ldg; both triangles are written and are equal
 *                                                          bit for bit; G[D][D] = the live rows, G[D][j] = the column sums)
 *   B[i][c] (+)= sum_{live r, label[r] == c} zt_r[i]       for i < Da, c < C (pitch ldb; B[D][c] = the rows of class c)
 * accumulate == 0: G and B are overwritten (and not read).  accumulate != 0: the new sum is added to what they hold,
 * G[i][j] = G[i][j] + sum: two disjoint row sets become one system in two calls.
 * Arithmetic: every fp32 value is converted to double first, so every product is exact (48 bits) and only the additions round.
 * Order of every sum, a function of (n, D, C) alone.  A slab's partial starts at 0.0 and takes its rows in ascending order: for
 * G four rows at a time on the f64 MFMA (one instruction adds the products of rows 4s .. 4s + 3 to the accumulator it was
 * handed; a skipped row and a row beyond the slab enter as 0.0, which changes nothing), for B one addition per live row of the
 * class.  The sum over the slabs starts at 0.0 and adds the partials in ascending slab order in a second launch; with
 * accumulate that sum is then added to the old value.
 * Ownership.  G: a workgroup of 256 threads owns (slab, one 64 x 64 tile on or below the diagonal), a wavefront 32 x 32 of it
 * in four 16 x 16 accumulators; 32 rows of both operand columns are staged in LDS as doubles per step.  The tiles above the
 * diagonal are never computed: the fold writes G[j][i] from the partial of G[i][j].  B: one wavefront owns (slab, 64 columns
 * i, 64 classes), a lane one column, the accumulators in LDS.  The fold kernels own one element of G or B per thread.
 * Only G[i][0..Da), B[i][0..C) for i < Da and the workspace are written.
 * DV_EINVAL: null pointers, n <= 0, D < 1, D > DV_RIDGE_MAX_D, C < 1, C > DV_RIDGE_MAX_C, ldz < D, ldg < Da, ldb < C.
 * DV_EALIGN: G, B or workspace not 8-byte aligned. */
int dv_ridge_gram_f64(const float* z, int64_t ldz, int32_t n, int32_t D, const int32_t* label, int32_t C,
                      double* G, int64_t ldg, double* B, int64_t ldb, int32_t accumulate, void* workspace, void* stream);

/* W = A^-1 B for A = G + lambda diag(1 x n_pen, 0 x (Da - n_pen)), by a blocked Cholesky factorisation A = L L^T and two
 * triangular solves, all in double.  Only the lower triangle of G [Da][ldg] is read.  L is written to the lower triangle of
 * chol [Da][ldc]; its strict upper triangle is left as found.  B [Da][ldb] holds C right-hand sides; W [Da][ldw] receives the
 * solution, columns c < C of rows i < Da only.  chol may be G itself (A then replaces its lower triangle); W may be B.
 * *info (int32 on the device) = 0 on success, otherwise the 1-based index of the first pivot that is not a finite positive
 * number; W and the rest of chol are then unspecified and the call still returns 0.
 * Order.  A[i][i] = G[i][i] + lambda (one addition, i < n_pen).  Block columns of b = DV_RIDGE_TILE, k = 0, 1, ...:
 *   1. the diagonal block in LDS, column by column: l_jj = sqrt(a_jj); l_ij = a_ij / l_jj; a_ic = a_ic - l_ij * l_cj
 *      (j < c <= i; a product and a difference, each rounded);
 *   2. the panel below it by substitution, row by row: for j ascending x_j = a_j / l_jj, then a_m = a_m - x_j * l_mj for
 *      m > j (64 rows per workgroup, the updates of a step shared by its four wavefronts).  No block is inverted;
 *   3. the trailing lower triangle, A22 = A22 - L21 L21^T, a 64 x 64 tile per workgroup on the f64 MFMA, the 64 products of an
 *      element in ascending column order, four per instruction, starting from the old value.
 * Then L Y = B block by block downwards (the diagonal block by substitution as in 2., 64 right-hand sides per workgroup, then
 * the rows below updated as in 3.), and L^T W = Y upwards in the same way.  The steps are ordered by launches
 * (about 3 Da / 64 for the factor and 4 Da / 64 for the solves).
 * DV_EINVAL: null pointers, Da < 1, Da > DV_RIDGE_MAX_D + 1, n_pen < 0, n_pen > Da, lambda negative or not finite, C < 1,
 * C > DV_RIDGE_MAX_C, ldg < Da, ldc < Da, ldb < C, ldw < C.  DV_EALIGN: G, B, W or chol not 8-byte aligned, info not 4-byte
 * aligned. */
int dv_ridge_solve_f64(const double* G, int64_t ldg, int32_t Da, int32_t n_pen, double lambda,
                       const double* B, int64_t ldb, int32_t C, double* W, int64_t ldw,
                       double* chol, int64_t ldc, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALVAR_RIDGE_H */
