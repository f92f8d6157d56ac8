// Spherical k-means (include/dualvar_cluster.h: dv_kmeans_assign_f32, dv_kmeans_update_workspace, dv_kmeans_update_f32,
// dv_kmeans_dot_f32, dv_kmeans_seed_workspace, dv_kmeans_seed_f32).
//
// The similarities of an iteration come from dv_gemm_f32; these kernels are the rest of it.  All are bound by memory: the
// arg-max reads the [R, K] block once, the centroid step reads the n rows of z once (coalesced along D, gathered through a
// stable counting sort of the rows by cluster), a seeding step reads z once against one centre (the row dot) and then reads and
// writes n floats.  Every sum has a fixed order (no
// floating-point atomics; the integer atomics are counts, which commute): DESIGN.md, §6f.
#include "common.hpp"
#include "../../include/dualvar_cluster.h"

#define KM_PART DV_KMEANS_PART
#define KM_SORT_ROWS DV_KMEANS_SORT_ROWS
#define KM_SEED_BLOCK DV_KMEANS_SEED_BLOCK
#define KM_STAGE 1024                            // block partials the seeding's second launch stages in LDS at a time

static_assert(KM_SEED_BLOCK == 256, "a thread owns a row of its seed block");
static_assert(KM_SORT_ROWS % 256 == 0 && KM_SORT_ROWS % 64 == 0, "the sort blocks are walked by 256 threads and by one wavefront");
static_assert(KM_PART <= 256, "a part's row indices are staged by one pass of the workgroup");

// --------------------------------------------------------------------------------------------------------------- assign
// G lanes per row, 256 / G rows per workgroup
template <int G>
__global__ void __launch_bounds__(256) kmeans_assign_kernel(const float* __restrict__ sim, long long ld, int R, int K,
                                                            int* __restrict__ assign, float* __restrict__ best,
                                                            unsigned long long* __restrict__ changed) {
  __shared__ int sh[4];
  const int row = blockIdx.x * (256 / G) + (int)threadIdx.x / G;
  const int g = threadIdx.x % G;
  const bool valid = row < R;                    // the same for all lanes of a group
  float bv = -INFINITY;
  int bi = -1;
  if (valid) {
    const float* p = sim + (size_t)row * (size_t)ld;
#pragma unroll 4
    for (int j = g; j < K; j += G) {
      const float v = p[j];
      if (v > bv || (bi < 0 && v == v)) {        // strictly larger, or the first column that is not NaN
        bv = v;
        bi = j;
      }
    }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
      bv = ov;
      bi = oi;
    }
  }
  bool diff = false;
  if (valid && g == 0) {
    diff = assign[row] != bi;
    assign[row] = bi;
    best[row] = bv;
  }
  const int cnt = __popcll(__ballot(diff));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = sh[0] + sh[1] + sh[2] + sh[3];
    if (c) atomicAdd(changed, (unsigned long long)c);
  }
}

template <int G>
static void launch_assign(const float* sim, int64_t ld, int R, int K, int* assign, float* best, uint64_t* changed, hipStream_t st) {
  const int rows = 256 / G;
  hipLaunchKernelGGL(kmeans_assign_kernel<G>, dim3((unsigned)cdiv64(R, rows)), dim3(256), 0, st, sim, (long long)ld, R, K, assign,
                     best, (unsigned long long*)changed);
}

extern "C" int dv_kmeans_assign_f32(const float* sim, int64_t ld, int32_t R, int32_t K, int32_t* assign, float* best,
                                    uint64_t* changed, void* stream) {
  if (!sim || !assign || !best || !changed || R <= 0 || K < 1 || K > DV_KMEANS_MAX_K || ld < K) return DV_EINVAL;
  if ((uintptr_t)changed & 7) return DV_EALIGN;
  hipStream_t st = ST(stream);
  if (K <= 1) launch_assign<1>(sim, ld, R, K, assign, best, changed, st);
  else if (K <= 2) launch_assign<2>(sim, ld, R, K, assign, best, changed, st);
  else if (K <= 4) launch_assign<4>(sim, ld, R, K, assign, best, changed, st);
  else if (K <= 8) launch_assign<8>(sim, ld, R, K, assign, best, changed, st);
  else if (K <= 16) launch_assign<16>(sim, ld, R, K, assign, best, changed, st);
  else if (K <= 32) launch_assign<32>(sim, ld, R, K, assign, best, changed, st);
  else launch_assign<64>(sim, ld, R, K, assign, best, changed, st);
  return dv_launch_status();
}

// --------------------------------------------------------------------------------------------------------------- update
static inline int64_t km_sort_blocks(int64_t n) { return cdiv64(n, KM_SORT_ROWS); }
static inline int64_t km_max_parts(int64_t n, int64_t K) { return n / KM_PART + K; }

// the workspace, doubles first
struct km_ws {
  double* part_sum;      // [P][D]
  double* part_within;   // [P]
  double* s;             // [K][D]
  int* hist;             // [B][K]: counts per (sort block, cluster), then their exclusive scan over the blocks
  int* offset;           // [K + 1]: first position of a cluster in `sorted`
  int* partoff;          // [K + 1]: first part of a cluster
  int* sorted;           // [n]: row indices, by cluster, ascending within a cluster
  int64_t bytes;
};
static inline km_ws km_layout(void* base, int64_t n, int64_t D, int64_t K) {
  const int64_t P = km_max_parts(n, K), B = km_sort_blocks(n);
  km_ws w;
  w.part_sum = (double*)base;
  w.part_within = w.part_sum + P * D;
  w.s = w.part_within + P;
  w.hist = (int*)(w.s + K * D);
  w.offset = w.hist + B * K;
  w.partoff = w.offset + (K + 1);
  w.sorted = w.partoff + (K + 1);
  w.bytes = (8 * (P * D + P + K * D) + 4 * (B * K + 2 * (K + 1) + n) + 7) & ~(int64_t)7;
  return w;
}

__device__ __forceinline__ int km_key(const int* __restrict__ assign, long long r, int n, int K) {
  if (r >= n) return K;
  const int a = assign[r];
  return (a < 0 || a >= K) ? K : a;               // K: no cluster
}

// counts per (sort block, cluster): an LDS histogram, integer atomics only
__global__ void __launch_bounds__(256) kmeans_count_kernel(const int* __restrict__ assign, int n, int K, int* __restrict__ hist) {
  __shared__ int h[DV_KMEANS_MAX_K];
  for (int k = threadIdx.x; k < K; k += 256) h[k] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * KM_SORT_ROWS;
  for (int i = threadIdx.x; i < KM_SORT_ROWS; i += 256) {
    const int key = km_key(assign, r0 + i, n, K);
    if (key < K) atomicAdd(&h[key], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) hist[(size_t)blockIdx.x * K + k] = h[k];
}

// per cluster: exclusive scan of its counts over the sort blocks in place; the total into cnt[k]
__global__ void __launch_bounds__(256) kmeans_scan_blocks_kernel(int* __restrict__ hist, int B, int K, int* __restrict__ cnt) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  int run = 0;
  for (int b = 0; b < B; ++b) {
    const int v = hist[(size_t)b * K + k];
    hist[(size_t)b * K + k] = run;
    run += v;
  }
  cnt[k] = run;
}

// one workgroup: cnt[0..K) -> offset[0..K] (exclusive scan of the counts) and partoff[0..K] (of ceil(count / KM_PART));
// cnt and offset may be the same array (a thread reads its run of clusters before anything is written)
__global__ void __launch_bounds__(256) kmeans_scan_clusters_kernel(const int* cnt, int K, int* offset, int* __restrict__ partoff) {
  __shared__ int so[257], sp[257];
  const int per = (K + 255) / 256;
  const int k0 = threadIdx.x * per, k1 = min(K, k0 + per);
  int c[DV_KMEANS_MAX_K / 256];
  int a = 0, b = 0;
#pragma unroll
  for (int i = 0; i < DV_KMEANS_MAX_K / 256; ++i) {
    c[i] = (k0 + i < k1) ? cnt[k0 + i] : 0;
    a += c[i];
    b += (c[i] + KM_PART - 1) / KM_PART;
  }
  so[threadIdx.x + 1] = a;
  sp[threadIdx.x + 1] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    so[0] = sp[0] = 0;
    for (int t = 1; t <= 256; ++t) {
      so[t] += so[t - 1];
      sp[t] += sp[t - 1];
    }
    offset[K] = so[256];
    partoff[K] = sp[256];
  }
  __syncthreads();
  a = so[threadIdx.x];
  b = sp[threadIdx.x];
#pragma unroll
  for (int i = 0; i < DV_KMEANS_MAX_K / 256; ++i) {
    if (k0 + i < k1) {
      offset[k0 + i] = a;
      partoff[k0 + i] = b;
    }
    a += c[i];
    b += (c[i] + KM_PART - 1) / KM_PART;
  }
}

// one wavefront per sort block: the stable ranks, 64 rows at a time in row order
__global__ void __launch_bounds__(64) kmeans_scatter_kernel(const int* __restrict__ assign, int n, int K, int bits,
                                                            const int* __restrict__ hist, const int* __restrict__ offset,
                                                            int* __restrict__ sorted) {
  __shared__ int next[DV_KMEANS_MAX_K];          // the position the next member of cluster k in this block goes to
  const int lane = threadIdx.x;
  for (int k = lane; k < K; k += 64) next[k] = offset[k] + hist[(size_t)blockIdx.x * K + k];
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * KM_SORT_ROWS;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int step = 0; step < KM_SORT_ROWS / 64; ++step) {
    const long long r = r0 + step * 64 + lane;
    const int key = km_key(assign, r, n, K);
    unsigned long long same = ~0ull;             // the lanes holding this lane's key
    for (int bit = 0; bit < bits; ++bit) {
      const bool one = (key >> bit) & 1;
      const unsigned long long m = __ballot(one);
      same &= one ? m : ~m;
    }
    const int rank = __popcll(same & below), total = __popcll(same);
    int base = 0;
    if (key < K) {
      base = next[key];
      sorted[base + rank] = (int)r;
    }
    __syncthreads();                             // every lane has read next[] before the group's last lane moves it on
    if (key < K && rank == total - 1) next[key] = base + total;
    __syncthreads();
  }
}

// the cluster of part q: the k with partoff[k] <= q < partoff[k + 1]
__device__ __forceinline__ int km_cluster_of_part(const int* __restrict__ partoff, int K, int q) {
  int lo = 0, hi = K;                            // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (partoff[mid] <= q) lo = mid; else hi = mid;
  }
  return lo;
}

// grid (P, ceil(D / 256)): the sums of one part over 256 columns, members in ascending row order
__global__ void __launch_bounds__(256) kmeans_part_kernel(const float* __restrict__ z, long long ldz, int D,
                                                          const float* __restrict__ best, int K, const int* __restrict__ offset,
                                                          const int* __restrict__ partoff, const int* __restrict__ sorted,
                                                          double* __restrict__ part_sum, double* __restrict__ part_within) {
  __shared__ int rows[KM_PART];
  const int q = blockIdx.x;
  if (q >= partoff[K]) return;                   // uniform over the workgroup
  const int k = km_cluster_of_part(partoff, K, q);
  const int c0 = offset[k] + (q - partoff[k]) * KM_PART;
  const int m = min(KM_PART, offset[k + 1] - c0);
  if ((int)threadIdx.x < m) rows[threadIdx.x] = sorted[c0 + threadIdx.x];
  __syncthreads();
  const int d = blockIdx.y * 256 + threadIdx.x;
  if (d < D) {
    double acc = 0.0;
    int i = 0;
    for (; i + 8 <= m; i += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = z[(size_t)rows[i + u] * (size_t)ldz + d];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; i < m; ++i) acc += (double)z[(size_t)rows[i] * (size_t)ldz + d];
    part_sum[(size_t)q * D + d] = acc;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    double w = 0.0;
    for (int i = 0; i < m; ++i) w += (double)best[rows[i]];
    part_within[q] = w;
  }
}

// grid (K, ceil(D / 256)): s_k over 256 columns, the cluster's parts in ascending order
__global__ void __launch_bounds__(256) kmeans_fold_kernel(const double* __restrict__ part_sum, const int* __restrict__ partoff,
                                                          int D, double* __restrict__ s) {
  const int k = blockIdx.x;
  const int d = blockIdx.y * 256 + threadIdx.x;
  if (d >= D) return;
  const int q0 = partoff[k], q1 = partoff[k + 1];
  double acc = 0.0;
  int q = q0;
  for (; q + 8 <= q1; q += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part_sum[(size_t)(q + u) * D + d];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; q < q1; ++q) acc += part_sum[(size_t)q * D + d];
  s[(size_t)k * D + d] = acc;
}

// one workgroup per cluster: the norm, the division, counts and within
__global__ void __launch_bounds__(256) kmeans_centroid_kernel(const double* __restrict__ s, int D, const int* __restrict__ offset,
                                                              const int* __restrict__ partoff,
                                                              const double* __restrict__ part_within, const float* cent_in,
                                                              float* cent_out, long long ldc, int* __restrict__ counts,
                                                              double* __restrict__ within) {
  __shared__ double sh[4];
  const int k = blockIdx.x;
  const int count = offset[k + 1] - offset[k];
  const double* sk = s + (size_t)k * D;
  double ss = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) {
    const double v = sk[d];
    ss += v * v;
  }
  const double nrm = sqrt(block_sum_f64(ss, sh));
  const bool ok = count > 0 && nrm > 0.0 && nrm < (double)INFINITY;
  for (int d = threadIdx.x; d < D; d += 256) {
    const size_t at = (size_t)k * (size_t)ldc + d;
    cent_out[at] = ok ? (float)(sk[d] / nrm) : cent_in[at];
  }
  if (threadIdx.x == 0) {
    double w = 0.0;
    for (int q = partoff[k]; q < partoff[k + 1]; ++q) w += part_within[q];
    counts[k] = count;
    within[k] = w;
  }
}

extern "C" int64_t dv_kmeans_update_workspace(int32_t n, int32_t D, int32_t K) {
  if (n <= 0 || D <= 0 || K < 1 || K > DV_KMEANS_MAX_K) return DV_EINVAL;
  return km_layout(nullptr, n, D, K).bytes;
}

extern "C" int dv_kmeans_update_f32(const float* z, int64_t ldz, int32_t n, int32_t D, const int32_t* assign, const float* best,
                                    int32_t K, const float* cent_in, float* cent_out, int64_t ldc, int32_t* counts,
                                    double* within, void* workspace, void* stream) {
  if (!z || !assign || !best || !cent_in || !cent_out || !counts || !within || !workspace || n <= 0 || D <= 0 || K < 1 ||
      K > DV_KMEANS_MAX_K || ldz < D || ldc < D)
    return DV_EINVAL;
  if (((uintptr_t)within | (uintptr_t)workspace) & 7) return DV_EALIGN;
  hipStream_t st = ST(stream);
  const km_ws w = km_layout(workspace, n, D, K);
  const int B = (int)km_sort_blocks(n), P = (int)km_max_parts(n, K), DB = (int)cdiv64(D, 256);
  int bits = 0;
  while ((1 << bits) <= K) ++bits;               // the keys 0 .. K (K: no cluster) differ within these bits
  hipLaunchKernelGGL(kmeans_count_kernel, dim3(B), dim3(256), 0, st, assign, n, K, w.hist);
  hipLaunchKernelGGL(kmeans_scan_blocks_kernel, dim3((unsigned)cdiv64(K, 256)), dim3(256), 0, st, w.hist, B, K, w.offset);
  hipLaunchKernelGGL(kmeans_scan_clusters_kernel, dim3(1), dim3(256), 0, st, w.offset, K, w.offset, w.partoff);
  hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(B), dim3(64), 0, st, assign, n, K, bits, w.hist, w.offset, w.sorted);
  hipLaunchKernelGGL(kmeans_part_kernel, dim3(P, DB), dim3(256), 0, st, z, (long long)ldz, D, best, K, w.offset, w.partoff,
                     w.sorted, w.part_sum, w.part_within);
  hipLaunchKernelGGL(kmeans_fold_kernel, dim3(K, DB), dim3(256), 0, st, w.part_sum, w.partoff, D, w.s);
  hipLaunchKernelGGL(kmeans_centroid_kernel, dim3(K), dim3(256), 0, st, w.s, D, w.offset, w.partoff, w.part_within, cent_in,
                     cent_out, (long long)ldc, counts, within);
  return dv_launch_status();
}

// ----------------------------------------------------------------------------------------------------------------- seed
// one wavefront per row; lane l owns the groups of four elements l, l + 64, ...; VEC: 16-byte loads (D % 4 == 0)
template <bool VEC>
__global__ void __launch_bounds__(256) kmeans_dot_kernel(const float* __restrict__ z, long long ldz, int n, int D,
                                                         const float* __restrict__ c, float* __restrict__ s) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;                          // a whole wavefront; the kernel has no barrier
  const float* p = z + (size_t)row * (size_t)ldz;
  const int groups = (D + 3) >> 2;
  float acc = 0.f;
  if (VEC) {
#pragma unroll 2
    for (int g = lane; g < groups; g += 64) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * (size_t)g);
      const f32x4 b = *reinterpret_cast<const f32x4*>(c + 4 * (size_t)g);
      acc = acc + a.x * b.x;
      acc = acc + a.y * b.y;
      acc = acc + a.z * b.z;
      acc = acc + a.w * b.w;
    }
  } else {
    for (int g = lane; g < groups; g += 64) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = 4 * g + e;
        if (d < D) acc = acc + p[d] * c[d];
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s[row] = acc;
}

extern "C" int dv_kmeans_dot_f32(const float* z, int64_t ldz, int32_t n, int32_t D, const float* c, float* s, void* stream) {
  if (!z || !c || !s || n <= 0 || D <= 0 || ldz < D) return DV_EINVAL;
  const bool vec = aligned16(z) && aligned16(c) && ldz % 4 == 0 && D % 4 == 0;
  const dim3 grid((unsigned)cdiv64(n, 4));
  if (vec) hipLaunchKernelGGL(kmeans_dot_kernel<true>, grid, dim3(256), 0, ST(stream), z, (long long)ldz, n, D, c, s);
  else hipLaunchKernelGGL(kmeans_dot_kernel<false>, grid, dim3(256), 0, ST(stream), z, (long long)ldz, n, D, c, s);
  return dv_launch_status();
}

__global__ void __launch_bounds__(KM_SEED_BLOCK) kmeans_seed_dist_kernel(const float* __restrict__ s, int n, float* __restrict__ mind,
                                                                         int first, double* __restrict__ partial) {
  __shared__ float sm[KM_SEED_BLOCK];
  const long long r = (long long)blockIdx.x * KM_SEED_BLOCK + threadIdx.x;
  float m = 0.f;
  if (r < n) {
    const float d = fmaxf(2.0f - 2.0f * s[r], 0.0f);
    m = first ? d : fminf(mind[r], d);
    mind[r] = m;
  }
  sm[threadIdx.x] = m;                           // rows beyond n add +0 after the block's last row: the partial is unchanged
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = 0.0;
    for (int i = 0; i < KM_SEED_BLOCK; ++i) p += (double)sm[i];
    partial[blockIdx.x] = p;
  }
}

__global__ void __launch_bounds__(256) kmeans_seed_pick_kernel(const double* __restrict__ partial, int NB,
                                                               const float* __restrict__ mind, int n, double u,
                                                               int* __restrict__ pick, double* __restrict__ total) {
  __shared__ double sh[KM_STAGE];
  __shared__ float sm[KM_SEED_BLOCK];
  __shared__ int s_blk;
  const int t = threadIdx.x;
  double T = 0.0;                                // thread 0's alone
  for (int c0 = 0; c0 < NB; c0 += KM_STAGE) {
    const int nc = min(KM_STAGE, NB - c0);
    __syncthreads();
    for (int i = t; i < nc; i += 256) sh[i] = partial[c0 + i];
    __syncthreads();
    if (t == 0)
      for (int i = 0; i < nc; ++i) T += sh[i];
  }
  const double target = u * T;
  double Tb = 0.0, run = 0.0;
  int blk = -1;
  for (int c0 = 0; c0 < NB; c0 += KM_STAGE) {
    const int nc = min(KM_STAGE, NB - c0);
    if (NB > KM_STAGE) {                         // otherwise the partials are still staged
      __syncthreads();
      for (int i = t; i < nc; i += 256) sh[i] = partial[c0 + i];
      __syncthreads();
    }
    if (t == 0 && blk < 0)
      for (int i = 0; i < nc; ++i) {
        const double nxt = run + sh[i];
        if (nxt > target) {
          blk = c0 + i;
          Tb = run;
          break;
        }
        run = nxt;
      }
  }
  if (t == 0) {
    *total = T;
    s_blk = blk;
  }
  __syncthreads();
  const int b = s_blk;
  if (b >= 0) {                                  // uniform: s_blk is shared
    const long long r = (long long)b * KM_SEED_BLOCK + t;
    sm[t] = r < n ? mind[r] : 0.f;
  }
  __syncthreads();
  if (t != 0) return;
  int chosen = -1;
  if (b >= 0) {
    double p = 0.0;
    for (int i = 0; i < KM_SEED_BLOCK; ++i) {
      p += (double)sm[i];
      if (Tb + p > target) {
        chosen = (int)((long long)b * KM_SEED_BLOCK + i);
        break;
      }
    }
  } else if (!(T == 0.0)) {                      // u * total rounded up to total, or total not finite: the last row off the centres
    for (long long r = (long long)n - 1; r >= 0; --r)
      if (mind[r] > 0.f) {
        chosen = (int)r;
        break;
      }
  }
  *pick = chosen;
}

extern "C" int64_t dv_kmeans_seed_workspace(int32_t n) {
  if (n <= 0) return DV_EINVAL;
  return 8 * cdiv64(n, KM_SEED_BLOCK);
}

extern "C" int dv_kmeans_seed_f32(const float* s, int32_t n, float* mind, int32_t first, double u, int32_t* pick, double* total,
                                  void* workspace, void* stream) {
  if (!s || !mind || !pick || !total || !workspace || n <= 0 || !(u >= 0.0) || !(u < 1.0)) return DV_EINVAL;
  if (((uintptr_t)total | (uintptr_t)workspace) & 7) return DV_EALIGN;
  const int NB = (int)cdiv64(n, KM_SEED_BLOCK);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(kmeans_seed_dist_kernel, dim3(NB), dim3(KM_SEED_BLOCK), 0, ST(stream), s, n, mind, first, partial);
  hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, ST(stream), partial, NB, mind, n, u, pick, total);
  return dv_launch_status();
}
