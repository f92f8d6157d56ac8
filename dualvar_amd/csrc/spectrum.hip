// Feature spectrum (include/dualvar_spectrum.h: dv_spectrum_cov_f64, dv_spectrum_rounds, dv_spectrum_pair, dv_spectrum_init_f64,
// dv_spectrum_rounds_f64, dv_spectrum_values_f64).
//
// The covariance of the clip features from the augmented Gram matrix of ridge.hip, and its eigen-decomposition by a
// parallel-ordered one-sided Jacobi method in double.  A workgroup owns one pair of rows of W and V for one round: it reads them
// twice (the three dot products, then the rotation; the second read comes from the cache), writes them once and touches nothing
// else, so the only hand-off between workgroups is the launch boundary between two rounds.  Every sum has a fixed order and
// there are no read-modify-write operations on shared words of any kind: DESIGN.md, §6h.
#include <float.h>
#include "common.hpp"
#include "../../include/dualvar_spectrum.h"

#define SP_BLOCK DV_SPECTRUM_BLOCK

static_assert(SP_BLOCK == 256, "the fold tree below starts at 128");

// the round-robin (circle) schedule over m (even) indices: the one function behind dv_spectrum_pair and the kernel
__host__ __device__ __forceinline__ void sp_pair(int m, int round, int k, int* p, int* q) {
  int a, b;
  if (k == 0) {
    a = m - 1;
    b = round;
  } else {
    a = (round + k) % (m - 1);
    b = (round - k + (m - 1)) % (m - 1);         // k < m / 2 <= m - 1: the sum is not negative
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// part[0..256) -> part[0]: for s = 128, 64, ..., 1: part[t] = part[t] + part[t + s] (t < s).  Ends on a barrier.
__device__ __forceinline__ void sp_fold(double* part) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int s = SP_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) part[t] = part[t] + part[t + s];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------- covariance
__global__ void __launch_bounds__(256) spectrum_cov_kernel(const double* __restrict__ G, long long ldg, int D,
                                                           double* __restrict__ Cov, long long ldc, double* __restrict__ mean) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)D * D) return;
  const int i = (int)(idx / D), j = (int)(idx % D);
  const double* sums = G + (size_t)D * (size_t)ldg;
  const double n = sums[D], si = sums[i], sj = sums[j];
  const double prod = si * sj;
  const double quot = prod / n;
  const double diff = G[(size_t)i * (size_t)ldg + j] - quot;
  Cov[(size_t)i * (size_t)ldc + j] = diff / n;
  if (i == 0) mean[j] = sj / n;
}

extern "C" int dv_spectrum_cov_f64(const double* G, int64_t ldg, int32_t D, double* Cov, int64_t ldc, double* mean, void* stream) {
  if (!G || !Cov || !mean || D < 1 || D > DV_SPECTRUM_MAX_D || ldg < (int64_t)D + 1 || ldc < D) return DV_EINVAL;
  if (((uintptr_t)G | (uintptr_t)Cov | (uintptr_t)mean) & 7) return DV_EALIGN;
  hipLaunchKernelGGL(spectrum_cov_kernel, dim3((unsigned)cdiv64((int64_t)D * D, 256)), dim3(256), 0, ST(stream), G, (long long)ldg,
                     D, Cov, (long long)ldc, mean);
  return dv_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ schedule
extern "C" int dv_spectrum_rounds(int32_t n) {
  if (n < 1 || n > DV_SPECTRUM_MAX_D) return DV_EINVAL;
  return n == 1 ? 0 : n + (n & 1) - 1;
}

extern "C" int dv_spectrum_pair(int32_t n, int32_t round, int32_t k, int32_t* p, int32_t* q) {
  if (!p || !q || n < 1 || n > DV_SPECTRUM_MAX_D) return DV_EINVAL;
  const int m = n + (n & 1);
  if (round < 0 || round >= dv_spectrum_rounds(n) || k < 0 || k >= m / 2) return DV_EINVAL;
  int pp, qq;
  sp_pair(m, round, k, &pp, &qq);
  *p = pp;
  *q = qq;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- init
// blocks 0 .. gridDim.x - 2 copy A to W and write the identity to V, one element per thread; the last block alone forms the norm
__global__ void __launch_bounds__(256) spectrum_init_kernel(const double* __restrict__ A, long long lda, int n, double* __restrict__ W,
                                                            long long ldw, double* __restrict__ V, long long ldv,
                                                            double* __restrict__ scale) {
  __shared__ double part[SP_BLOCK];
  const int t = threadIdx.x;
  const long long total = (long long)n * n;
  if (blockIdx.x + 1 < gridDim.x) {
    const long long e = (long long)blockIdx.x * 256 + t;
    if (e >= total) return;
    const int i = (int)(e / n), j = (int)(e % n);
    W[(size_t)i * (size_t)ldw + j] = A[(size_t)i * (size_t)lda + j];
    V[(size_t)i * (size_t)ldv + j] = i == j ? 1.0 : 0.0;
    return;
  }
  double acc = 0.0;
  int i = t / n, j = t % n;                      // element e = t, t + 256, ...: (i, j) advanced without a division per step
  const int di = 256 / n, dj = 256 % n;
  for (long long e = t; e < total; e += 256) {
    const double x = A[(size_t)i * (size_t)lda + j];
    acc = acc + x * x;
    i += di;
    j += dj;
    if (j >= n) {
      j -= n;
      ++i;
    }
  }
  part[t] = acc;
  sp_fold(part);
  if (t == 0) scale[0] = sqrt(part[0]);
}

extern "C" int dv_spectrum_init_f64(const double* A, int64_t lda, int32_t n, double* W, int64_t ldw, double* V, int64_t ldv,
                                    double* scale, void* stream) {
  if (!A || !W || !V || !scale || n < 1 || n > DV_SPECTRUM_MAX_D || lda < n || ldw < n || ldv < n) return DV_EINVAL;
  if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)V | (uintptr_t)scale) & 7) return DV_EALIGN;
  hipLaunchKernelGGL(spectrum_init_kernel, dim3((unsigned)cdiv64((int64_t)n * n, 256) + 1), dim3(256), 0, ST(stream), A,
                     (long long)lda, n, W, (long long)ldw, V, (long long)ldv, scale);
  return dv_launch_status();
}

// -------------------------------------------------------------------------------------------------------------- rounds
__global__ void __launch_bounds__(256) spectrum_clear_kernel(double* __restrict__ stat, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) stat[i] = 0.0;
}

__global__ void __launch_bounds__(256) spectrum_round_kernel(double* __restrict__ W, long long ldw, double* __restrict__ V,
                                                             long long ldv, int n, int m, int round,
                                                             const double* __restrict__ scale, double* __restrict__ stat) {
  __shared__ double pa[SP_BLOCK], pb[SP_BLOCK], pc[SP_BLOCK];
  const int t = threadIdx.x, k = blockIdx.x;
  int p, q;
  sp_pair(m, round, k, &p, &q);
  if (q >= n) return;                            // the bye of an odd n: the whole workgroup leaves
  double* wp = W + (size_t)p * (size_t)ldw;
  double* wq = W + (size_t)q * (size_t)ldw;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = t; i < n; i += SP_BLOCK) {
    const double x = wp[i], y = wq[i];
    a = a + x * x;
    b = b + y * y;
    c = c + x * y;
  }
  pa[t] = a;
  pb[t] = b;
  pc[t] = c;
  __syncthreads();
#pragma unroll
  for (int s = SP_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) {
      pa[t] = pa[t] + pa[t + s];
      pb[t] = pb[t] + pb[t + s];
      pc[t] = pc[t] + pc[t + s];
    }
    __syncthreads();
  }
  a = pa[0];
  b = pb[0];
  c = pc[0];
  // every thread decides from the same three numbers
  const double ra = sqrt(a), rb = sqrt(b);
  const bool bad = a != a || b != b || c != c;
  const bool above = fmin(ra, rb) > DBL_EPSILON * scale[0];
  const bool rotated = above && fabs(c) > (DBL_EPSILON * ra) * rb;
  if (t == 0) {
    double s0 = stat[2 * k];
    if (bad)
      s0 = a + b + c;                            // NaN
    else if (above && s0 == s0)
      s0 = fmax(s0, fabs(c) / (ra * rb));
    stat[2 * k] = s0;
    if (rotated) stat[2 * k + 1] = stat[2 * k + 1] + 1.0;
  }
  if (!rotated) return;
  const double zeta = (b - a) / (2.0 * c);
  const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + tn * tn);
  const double sn = cs * tn;
  double* vp = V + (size_t)p * (size_t)ldv;
  double* vq = V + (size_t)q * (size_t)ldv;
  for (int i = t; i < n; i += SP_BLOCK) {
    const double x = wp[i], y = wq[i];
    wp[i] = cs * x - sn * y;
    wq[i] = sn * x + cs * y;
    const double u = vp[i], v = vq[i];
    vp[i] = cs * u - sn * v;
    vq[i] = sn * u + cs * v;
  }
}

extern "C" int dv_spectrum_rounds_f64(double* W, int64_t ldw, double* V, int64_t ldv, int32_t n, int32_t round_lo, int32_t round_hi,
                                      const double* scale, double* stat, void* stream) {
  if (!W || !V || !scale || !stat || n < 1 || n > DV_SPECTRUM_MAX_D || ldw < n || ldv < n || round_lo < 0 || round_lo > round_hi ||
      round_hi > dv_spectrum_rounds(n))
    return DV_EINVAL;
  if (((uintptr_t)W | (uintptr_t)V | (uintptr_t)scale | (uintptr_t)stat) & 7) return DV_EALIGN;
  hipStream_t st = ST(stream);
  const int m = n + (n & 1);
  if (round_lo == 0) hipLaunchKernelGGL(spectrum_clear_kernel, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, st, stat, m);
  for (int r = round_lo; r < round_hi; ++r)
    hipLaunchKernelGGL(spectrum_round_kernel, dim3(m / 2), dim3(SP_BLOCK), 0, st, W, (long long)ldw, V, (long long)ldv, n, m, r,
                       scale, stat);
  return dv_launch_status();
}

// -------------------------------------------------------------------------------------------------------------- values
__global__ void __launch_bounds__(256) spectrum_values_kernel(const double* __restrict__ W, long long ldw,
                                                              const double* __restrict__ V, long long ldv, int n,
                                                              double* __restrict__ lambda) {
  __shared__ double num[SP_BLOCK], den[SP_BLOCK];
  const int t = threadIdx.x, j = blockIdx.x;
  const double* w = W + (size_t)j * (size_t)ldw;
  const double* v = V + (size_t)j * (size_t)ldv;
  double vw = 0.0, vv = 0.0;
  for (int i = t; i < n; i += SP_BLOCK) {
    const double x = v[i];
    vw = vw + x * w[i];
    vv = vv + x * x;
  }
  num[t] = vw;
  den[t] = vv;
  sp_fold(num);
  sp_fold(den);
  if (t == 0) lambda[j] = num[0] / den[0];
}

extern "C" int dv_spectrum_values_f64(const double* W, int64_t ldw, const double* V, int64_t ldv, int32_t n, double* lambda,
                                      void* stream) {
  if (!W || !V || !lambda || n < 1 || n > DV_SPECTRUM_MAX_D || ldw < n || ldv < n) return DV_EINVAL;
  if (((uintptr_t)W | (uintptr_t)V | (uintptr_t)lambda) & 7) return DV_EALIGN;
  hipLaunchKernelGGL(spectrum_values_kernel, dim3(n), dim3(SP_BLOCK), 0, ST(stream), W, (long long)ldw, V, (long long)ldv, n, lambda);
  return dv_launch_status();
}
