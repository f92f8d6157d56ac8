// Closed-form ridge probe (include/dualvar_ridge.h: dv_ridge_gram_workspace, dv_ridge_gram_f64, dv_ridge_solve_f64).
//
// The normal equations of ridge regression onto one-hot targets in double: the Gram matrix of the fp32 rows (with a constant
// column) and the class sums in slab partials folded by a second launch, then a blocked Cholesky factorisation and two blocked
// triangular solves.  The matrix products (the Gram tiles, the trailing update, the updates of the right-hand sides) run on
// v_mfma_f64_16x16x4_f64; the diagonal blocks are factored and substituted in LDS.  Every sum has a fixed order, there are no
// atomics of any kind and the only hand-off between workgroups is the launch boundary: DESIGN.md, §6g.
#include "common.hpp"
#include "../../include/dualvar_ridge.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define RG_TILE DV_RIDGE_TILE
#define RG_KC 32                                 // rows (Gram) / columns (updates) of the two operands staged in LDS per step
#define RG_PITCH 65                              // doubles per staged LDS row: a transposed store walks the banks two by two
#define RG_BC 64                                 // classes per workgroup of the class sums

static_assert(RG_TILE == 64, "a workgroup of four wavefronts owns 64 x 64, a wavefront 32 x 32");
static_assert(RG_KC % 4 == 0 && (RG_KC * RG_TILE) % 256 == 0, "the MFMA takes four at a time, 256 threads stage a chunk");
static_assert(DV_RIDGE_SLAB % RG_KC == 0, "a slab is a whole number of staged chunks");

// ------------------------------------------------------------------------------------------------------ the MFMA tile
// acc[mb][nb] += A^T B over one staged chunk: sA [RG_KC][RG_PITCH] holds A[k][m], sB holds B[k][n].  Operand maps of
// v_mfma_f64_16x16x4_f64: lane l gives A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; register g of the result is
// (row (l >> 4) + 4 g, column l & 15) -- not the f32 map.  k ascends through the chunk.
__device__ __forceinline__ void rg_mma_chunk(const double* sA, const double* sB, f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* pa = sA + (lane >> 4) * RG_PITCH + (w >> 1) * 32 + (lane & 15);
  const double* pb = sB + (lane >> 4) * RG_PITCH + (w & 1) * 32 + (lane & 15);
#pragma unroll
  for (int kk = 0; kk < RG_KC / 4; ++kk) {
    const double a0 = pa[kk * 4 * RG_PITCH], a1 = pa[kk * 4 * RG_PITCH + 16];
    const double b0 = pb[kk * 4 * RG_PITCH], b1 = pb[kk * 4 * RG_PITCH + 16];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}
// the element of the 64 x 64 tile that acc[mb][nb][g] of this thread is
__device__ __forceinline__ int rg_row(int mb, int g) { return (int)(threadIdx.x >> 7) * 32 + mb * 16 + (int)((threadIdx.x & 63) >> 4) + 4 * g; }
__device__ __forceinline__ int rg_col(int nb) { return (int)((threadIdx.x >> 6) & 1) * 32 + nb * 16 + (int)(threadIdx.x & 15); }

// ---------------------------------------------------------------------------------------------------------------- Gram
struct rg_slabs {
  int rows, P;                                   // rows per slab, slabs
};
static inline rg_slabs rg_cut(int64_t n) {
  const int64_t S = cdiv64(n, DV_RIDGE_SLAB), q = cdiv64(S, DV_RIDGE_MAX_SLABS);
  rg_slabs s;
  s.rows = (int)(q * DV_RIDGE_SLAB);
  s.P = (int)cdiv64(n, s.rows);
  return s;
}
static inline int64_t rg_tiles(int64_t Da) {
  const int64_t T = cdiv64(Da, RG_TILE);
  return T * (T + 1) / 2;
}

// column i of the row with the constant column, as a double: z[i] for i < D, 1 at i == D, 0 beyond
__device__ __forceinline__ double rg_elem(const float* __restrict__ zr, int i, int D) {
  return i < D ? (double)zr[i] : (i == D ? 1.0 : 0.0);
}

// grid (T, T, P), the blocks above the diagonal leave at once: the partial of one slab over one tile, rows ascending
__global__ void __launch_bounds__(256) ridge_gram_part_kernel(const float* __restrict__ z, long long ldz, int n, int D,
                                                              const int* __restrict__ label, int C, int slab_rows,
                                                              double* __restrict__ part) {
  const int tj = blockIdx.x, ti = blockIdx.y, p = blockIdx.z;
  if (tj > ti) return;                           // uniform over the workgroup
  __shared__ double sA[RG_KC * RG_PITCH], sB[RG_KC * RG_PITCH];
  const long long r_begin = (long long)p * slab_rows;
  const long long r_end = min((long long)n, r_begin + slab_rows);
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (long long r0 = r_begin; r0 < r_end; r0 += RG_KC) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RG_KC * RG_TILE / 256; ++u) {
      const int e = threadIdx.x + 256 * u, k = e >> 6, c = e & 63;
      const long long r = r0 + k;
      double va = 0.0, vb = 0.0;
      if (r < r_end) {
        const int lab = label[r];
        if (lab >= 0 && lab < C) {               // a skipped row stays 0.0: nothing of it is read
          const float* zr = z + (size_t)r * (size_t)ldz;
          va = rg_elem(zr, ti * RG_TILE + c, D);
          vb = rg_elem(zr, tj * RG_TILE + c, D);
        }
      }
      sA[k * RG_PITCH + c] = va;
      sB[k * RG_PITCH + c] = vb;
    }
    __syncthreads();
    rg_mma_chunk(sA, sB, acc);
  }
  const size_t tile = (size_t)ti * (ti + 1) / 2 + tj;
  double* dst = part + ((size_t)p * ((size_t)gridDim.y * (gridDim.y + 1) / 2) + tile) * (RG_TILE * RG_TILE);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) dst[rg_row(mb, g) * RG_TILE + rg_col(nb)] = acc[mb][nb][g];
}

// one element of G per thread: the slabs in ascending order; an element above the diagonal reads its mirror image
__global__ void __launch_bounds__(256) ridge_gram_fold_kernel(const double* __restrict__ part, int P, int Da, double* __restrict__ G,
                                                              long long ldg, int accumulate) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Da * Da) return;
  const int i = (int)(idx / Da), j = (int)(idx % Da);
  const int a = max(i, j), b = min(i, j);
  const size_t T = (size_t)(Da + RG_TILE - 1) / RG_TILE, tiles = T * (T + 1) / 2;
  const size_t at = ((size_t)(a >> 6) * ((a >> 6) + 1) / 2 + (b >> 6)) * (RG_TILE * RG_TILE) + (size_t)(a & 63) * RG_TILE + (b & 63);
  double acc = 0.0;
  for (int p = 0; p < P; ++p) acc += part[(size_t)p * tiles * (RG_TILE * RG_TILE) + at];
  double* g = G + (size_t)i * (size_t)ldg + j;
  *g = accumulate ? *g + acc : acc;
}

// grid (ceil(Da / 64), ceil(C / RG_BC), P), one wavefront: lane = column i, the sums of RG_BC classes in LDS, rows ascending
__global__ void __launch_bounds__(64) ridge_class_part_kernel(const float* __restrict__ z, long long ldz, int n, int D,
                                                              const int* __restrict__ label, int C, int slab_rows,
                                                              double* __restrict__ partB) {
  __shared__ double acc[RG_BC * 64];
  const int lane = threadIdx.x, i = blockIdx.x * 64 + lane, c0 = blockIdx.y * RG_BC, p = blockIdx.z, Da = D + 1;
  for (int c = 0; c < RG_BC; ++c) acc[c * 64 + lane] = 0.0;        // a lane touches its own column of acc only: no barrier
  const long long r_begin = (long long)p * slab_rows;
  const long long r_end = min((long long)n, r_begin + slab_rows);
  for (long long r0 = r_begin; r0 < r_end; r0 += 8) {
    int lc[8];
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      lc[u] = -1;
      v[u] = 0.f;
      if (r0 + u < r_end) {
        const int lab = label[r0 + u];           // the same for every lane
        if (lab >= 0 && lab < C && lab >= c0 && lab < c0 + RG_BC) {
          lc[u] = lab - c0;
          if (i < D) v[u] = z[(size_t)(r0 + u) * (size_t)ldz + i];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (lc[u] >= 0) acc[lc[u] * 64 + lane] += (i == D) ? 1.0 : (double)v[u];
  }
  if (i < Da)
    for (int c = 0; c < RG_BC && c0 + c < C; ++c) partB[((size_t)p * C + c0 + c) * Da + i] = acc[c * 64 + lane];
}

__global__ void __launch_bounds__(256) ridge_class_fold_kernel(const double* __restrict__ partB, int P, int Da, int C,
                                                               double* __restrict__ B, long long ldb, int accumulate) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Da * C) return;
  const int i = (int)(idx / C), c = (int)(idx % C);
  double acc = 0.0;
  for (int p = 0; p < P; ++p) acc += partB[((size_t)p * C + c) * Da + i];
  double* b = B + (size_t)i * (size_t)ldb + c;
  *b = accumulate ? *b + acc : acc;
}

extern "C" int64_t dv_ridge_gram_workspace(int32_t n, int32_t D, int32_t C) {
  if (n <= 0 || D < 1 || D > DV_RIDGE_MAX_D || C < 1 || C > DV_RIDGE_MAX_C) return DV_EINVAL;
  const int64_t Da = (int64_t)D + 1;
  return 8 * (int64_t)rg_cut(n).P * (rg_tiles(Da) * RG_TILE * RG_TILE + (int64_t)C * Da);
}

extern "C" int dv_ridge_gram_f64(const float* z, int64_t ldz, int32_t n, int32_t D, const int32_t* label, int32_t C, double* G,
                                 int64_t ldg, double* B, int64_t ldb, int32_t accumulate, void* workspace, void* stream) {
  if (!z || !label || !G || !B || !workspace || n <= 0 || D < 1 || D > DV_RIDGE_MAX_D || C < 1 || C > DV_RIDGE_MAX_C || ldz < D ||
      ldg < (int64_t)D + 1 || ldb < C)
    return DV_EINVAL;
  if (((uintptr_t)G | (uintptr_t)B | (uintptr_t)workspace) & 7) return DV_EALIGN;
  hipStream_t st = ST(stream);
  const int Da = D + 1, T = (int)cdiv64(Da, RG_TILE);
  const rg_slabs s = rg_cut(n);
  double* partG = (double*)workspace;
  double* partB = partG + (size_t)s.P * (size_t)rg_tiles(Da) * (RG_TILE * RG_TILE);
  hipLaunchKernelGGL(ridge_gram_part_kernel, dim3(T, T, s.P), dim3(256), 0, st, z, (long long)ldz, n, D, label, C, s.rows, partG);
  hipLaunchKernelGGL(ridge_class_part_kernel, dim3(T, (unsigned)cdiv64(C, RG_BC), s.P), dim3(64), 0, st, z, (long long)ldz, n, D,
                     label, C, s.rows, partB);
  hipLaunchKernelGGL(ridge_gram_fold_kernel, dim3((unsigned)cdiv64((int64_t)Da * Da, 256)), dim3(256), 0, st, partG, s.P, Da, G,
                     (long long)ldg, accumulate);
  hipLaunchKernelGGL(ridge_class_fold_kernel, dim3((unsigned)cdiv64((int64_t)Da * C, 256)), dim3(256), 0, st, partB, s.P, Da, C, B,
                     (long long)ldb, accumulate);
  return dv_launch_status();
}

// --------------------------------------------------------------------------------------------------------------- solve
// chol (lower triangle) = G + lambda on the first n_pen diagonal entries;  W = B;  *info = 0
__global__ void __launch_bounds__(256) ridge_init_kernel(const double* G, long long ldg, int Da, int n_pen, double lambda,
                                                         const double* B, long long ldb, int C, double* W, long long ldw,
                                                         double* chol, long long ldc, int* info) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nG = (long long)Da * Da;
  if (idx == 0) *info = 0;
  if (idx < nG) {
    const int i = (int)(idx / Da), j = (int)(idx % Da);
    if (j <= i) {
      double v = G[(size_t)i * (size_t)ldg + j];
      if (i == j && i < n_pen) v = v + lambda;
      chol[(size_t)i * (size_t)ldc + j] = v;
    }
  } else if (idx < nG + (long long)Da * C) {
    const long long e = idx - nG;
    const int i = (int)(e / C), c = (int)(e % C);
    W[(size_t)i * (size_t)ldw + c] = B[(size_t)i * (size_t)ldb + c];
  }
}

// one workgroup: the diagonal block [k0, k0 + nb) in LDS, column by column
__global__ void __launch_bounds__(256) ridge_potrf_kernel(double* __restrict__ chol, long long ldc, int k0, int nb, int* __restrict__ info) {
  __shared__ double a[RG_TILE * RG_PITCH];
  const int t = threadIdx.x;
  for (int e = t; e < nb * nb; e += 256) {
    const int i = e / nb, j = e % nb;
    if (j <= i) a[i * RG_PITCH + j] = chol[(size_t)(k0 + i) * (size_t)ldc + k0 + j];
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const double d2 = a[j * RG_PITCH + j];
    __syncthreads();                             // every thread holds the pivot before it is replaced
    const double d = sqrt(d2);
    if (t == 0) {
      if (!(d2 > 0.0 && d2 < (double)INFINITY) && *info == 0) *info = k0 + j + 1;
      a[j * RG_PITCH + j] = d;
    }
    for (int i = j + 1 + t; i < nb; i += 256) a[i * RG_PITCH + j] = a[i * RG_PITCH + j] / d;
    __syncthreads();
    const int m = nb - j - 1;
    for (int e = t; e < m * m; e += 256) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) a[i * RG_PITCH + c] = a[i * RG_PITCH + c] - a[i * RG_PITCH + j] * a[c * RG_PITCH + j];
    }
    __syncthreads();
  }
  for (int e = t; e < nb * nb; e += 256) {
    const int i = e / nb, j = e % nb;
    if (j <= i) chol[(size_t)(k0 + i) * (size_t)ldc + k0 + j] = a[i * RG_PITCH + j];
  }
}

// Substitution against the diagonal block L = chol[k0 .. k0 + nb)^2 for 64 right-hand sides per workgroup:
// X(j, c) = X[j * sj + c * sc], j < nb, c < ncols.  upper == 0: L x = b (j ascending); upper != 0: L^T x = b (j descending).
// The panel of the factorisation is the first form on the rows below the block, read as columns.  Lane c of each of the four
// wavefronts works on right-hand side c: at step j all four form x_j = b_j / l_jj (the same division), wavefront q updates the
// rows j + 1 + q, j + 5 + q, ... (upper: q, q + 4, ... below j) and wavefront 0 stores x_j once the step's barrier has passed,
// when nobody reads row j any more.  An element takes its updates in the order of j, as one thread per right-hand side would
// apply them.
__global__ void __launch_bounds__(256) ridge_trsm_kernel(const double* L, long long ldl, int nb, double* X, long long sj,
                                                         long long sc, int ncols, int upper) {
  __shared__ double l[RG_TILE * RG_TILE], s[RG_TILE * RG_TILE];      // 64 KiB together; l is read by broadcast, s along the lanes
  const int t = threadIdx.x, c0 = blockIdx.x * 64;
  for (int e = t; e < nb * nb; e += 256) {
    const int i = e / nb, j = e % nb;
    if (j <= i) l[i * RG_TILE + j] = L[(size_t)i * (size_t)ldl + j];
  }
  for (int e = t; e < nb * 64; e += 256) {
    const int j = (sj == 1) ? e % nb : e / 64, c = (sj == 1) ? e / nb : e % 64;      // the contiguous index goes with the lanes
    if (c0 + c < ncols) s[j * RG_TILE + c] = X[(size_t)j * (size_t)sj + (size_t)(c0 + c) * (size_t)sc];
  }
  __syncthreads();
  const int c = t & 63, q = t >> 6;             // a column beyond ncols works on whatever LDS holds and is never stored
  if (!upper) {
    for (int j = 0; j < nb; ++j) {
      const double x = s[j * RG_TILE + c] / l[j * RG_TILE + j];
      for (int m = j + 1 + q; m < nb; m += 4) s[m * RG_TILE + c] = s[m * RG_TILE + c] - x * l[m * RG_TILE + j];
      __syncthreads();
      if (q == 0) s[j * RG_TILE + c] = x;
    }
  } else {
    for (int j = nb - 1; j >= 0; --j) {
      const double x = s[j * RG_TILE + c] / l[j * RG_TILE + j];
      for (int m = q; m < j; m += 4) s[m * RG_TILE + c] = s[m * RG_TILE + c] - x * l[j * RG_TILE + m];
      __syncthreads();
      if (q == 0) s[j * RG_TILE + c] = x;
    }
  }
  __syncthreads();
  for (int e = t; e < nb * 64; e += 256) {
    const int j = (sj == 1) ? e % nb : e / 64, c = (sj == 1) ? e / nb : e % 64;
    if (c0 + c < ncols) X[(size_t)j * (size_t)sj + (size_t)(c0 + c) * (size_t)sc] = s[j * RG_TILE + c];
  }
}

// Cm[m][n] = Cm[m][n] - sum_{k < K} A(m, k) B(k, n), m < M, n < N, K <= 64: A(m, k) = A[m * sam + k * sak],
// B(k, n) = B[k * sbk + n * sbn].  grid (ceil(N / 64), ceil(M / 64)).  lower != 0: only the tiles on or below the diagonal
// run and only the elements m >= n are stored.  A is negated as it is staged (exact), so the MFMA starts from the old value
// and adds.
__global__ void __launch_bounds__(256) ridge_gemm_sub_kernel(double* Cm, long long ldcm, int M, int N, const double* A,
                                                             long long sam, long long sak, const double* B, long long sbk,
                                                             long long sbn, int K, int lower) {
  if (lower && blockIdx.x > blockIdx.y) return;  // uniform over the workgroup
  __shared__ double sA[RG_KC * RG_PITCH], sB[RG_KC * RG_PITCH];
  const int m0 = blockIdx.y * RG_TILE, n0 = blockIdx.x * RG_TILE;
  f64x4 acc[2][2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = m0 + rg_row(mb, g), n = n0 + rg_col(nb);
        acc[mb][nb][g] = (m < M && n < N && (!lower || m >= n)) ? Cm[(size_t)m * (size_t)ldcm + n] : 0.0;
      }
  for (int k0 = 0; k0 < K; k0 += RG_KC) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RG_KC * RG_TILE / 256; ++u) {
      const int e = threadIdx.x + 256 * u;
      {
        const int k = (sak == 1) ? e % RG_KC : e / RG_TILE, m = (sak == 1) ? e / RG_KC : e % RG_TILE;
        sA[k * RG_PITCH + m] = (m0 + m < M && k0 + k < K) ? -A[(size_t)(m0 + m) * (size_t)sam + (size_t)(k0 + k) * (size_t)sak] : 0.0;
      }
      {
        const int k = (sbk == 1) ? e % RG_KC : e / RG_TILE, nn = (sbk == 1) ? e / RG_KC : e % RG_TILE;
        sB[k * RG_PITCH + nn] = (n0 + nn < N && k0 + k < K) ? B[(size_t)(k0 + k) * (size_t)sbk + (size_t)(n0 + nn) * (size_t)sbn] : 0.0;
      }
    }
    __syncthreads();
    rg_mma_chunk(sA, sB, acc);
  }
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = m0 + rg_row(mb, g), n = n0 + rg_col(nb);
        if (m < M && n < N && (!lower || m >= n)) Cm[(size_t)m * (size_t)ldcm + n] = acc[mb][nb][g];
      }
}

extern "C" int dv_ridge_solve_f64(const double* G, int64_t ldg, int32_t Da, int32_t n_pen, double lambda, const double* B,
                                  int64_t ldb, int32_t C, double* W, int64_t ldw, double* chol, int64_t ldc, int32_t* info,
                                  void* stream) {
  if (!G || !B || !W || !chol || !info || Da < 1 || Da > DV_RIDGE_MAX_D + 1 || n_pen < 0 || n_pen > Da || !(lambda >= 0.0) ||
      !(lambda < (double)INFINITY) || C < 1 || C > DV_RIDGE_MAX_C || ldg < Da || ldc < Da || ldb < C || ldw < C)
    return DV_EINVAL;
  if ((((uintptr_t)G | (uintptr_t)B | (uintptr_t)W | (uintptr_t)chol) & 7) || ((uintptr_t)info & 3)) return DV_EALIGN;
  hipStream_t st = ST(stream);
  const long long lc = ldc, lw = ldw;
  const unsigned cb = (unsigned)cdiv64(C, 64);
  hipLaunchKernelGGL(ridge_init_kernel, dim3((unsigned)cdiv64((int64_t)Da * Da + (int64_t)Da * C, 256)), dim3(256), 0, st, G,
                     (long long)ldg, Da, n_pen, lambda, B, (long long)ldb, C, W, lw, chol, lc, info);
  for (int k0 = 0; k0 < Da; k0 += RG_TILE) {     // A = L L^T
    const int nb = min(RG_TILE, Da - k0), below = Da - k0 - nb;
    double* diag = chol + (size_t)k0 * (size_t)ldc + k0;
    hipLaunchKernelGGL(ridge_potrf_kernel, dim3(1), dim3(256), 0, st, chol, lc, k0, nb, info);
    if (below > 0) {
      double* panel = diag + (size_t)nb * (size_t)ldc;                       // [below][nb]: a row is a right-hand side
      double* trail = panel + nb;
      const unsigned tb = (unsigned)cdiv64(below, RG_TILE);
      hipLaunchKernelGGL(ridge_trsm_kernel, dim3(tb), dim3(256), 0, st, diag, lc, nb, panel, 1ll, lc, below, 0);
      hipLaunchKernelGGL(ridge_gemm_sub_kernel, dim3(tb, tb), dim3(256), 0, st, trail, lc, below, below, panel, lc, 1ll, panel, 1ll,
                         lc, nb, 1);
    }
  }
  for (int k0 = 0; k0 < Da; k0 += RG_TILE) {     // L Y = B
    const int nb = min(RG_TILE, Da - k0), below = Da - k0 - nb;
    const double* diag = chol + (size_t)k0 * (size_t)ldc + k0;
    double* wk = W + (size_t)k0 * (size_t)ldw;
    hipLaunchKernelGGL(ridge_trsm_kernel, dim3(cb), dim3(256), 0, st, diag, lc, nb, wk, lw, 1ll, C, 0);
    if (below > 0)
      hipLaunchKernelGGL(ridge_gemm_sub_kernel, dim3(cb, (unsigned)cdiv64(below, RG_TILE)), dim3(256), 0, st,
                         wk + (size_t)nb * (size_t)ldw, lw, below, C, diag + (size_t)nb * (size_t)ldc, lc, 1ll, wk, lw, 1ll, nb, 0);
  }
  for (int k0 = (Da - 1) / RG_TILE * RG_TILE; k0 >= 0; k0 -= RG_TILE) {      // L^T W = Y
    const int nb = min(RG_TILE, Da - k0);
    const double* diag = chol + (size_t)k0 * (size_t)ldc + k0;
    double* wk = W + (size_t)k0 * (size_t)ldw;
    hipLaunchKernelGGL(ridge_trsm_kernel, dim3(cb), dim3(256), 0, st, diag, lc, nb, wk, lw, 1ll, C, 1);
    if (k0 > 0)                                  // rows above: A(m, k) = L[k0 + k][m]
      hipLaunchKernelGGL(ridge_gemm_sub_kernel, dim3(cb, (unsigned)cdiv64(k0, RG_TILE)), dim3(256), 0, st, W, lw, k0, C,
                         chol + (size_t)k0 * (size_t)ldc, 1ll, lc, wk, lw, 1ll, nb, 0);
  }
  return dv_launch_status();
}
