// Streaming pair statistics (include/dualvar_pairstat.h: dv_pairstat_workspace, dv_pairstat_accum_f32).
//
// One pass over a [R][n_cols] block of similarities, read once: memory-bound.  At most PS_MAX_GRID workgroups of 256 threads walk
// the 64 x 1024 tiles of the block with a fixed stride, so which workgroup sees which element depends on (R, n_cols) only.  A lane
// owns four columns of a tile (their ids stay in registers for the tile's 64 rows, the rows' ids are staged in LDS), keeps nine
// double sums and six extrema in registers and counts into the workgroup's LDS histogram.  Partials go to the workspace; the
// fold kernel (one workgroup) adds them in ascending workgroup order.  No floating-point atomics.
#include "common.hpp"
#include "../../include/dualvar_pairstat.h"

#define PS_THREADS 256
#define PS_TR 64                                // rows of a tile
#define PS_TC (4 * PS_THREADS)                  // columns of a tile: four per lane
#define PS_ROWS_IN_FLIGHT 4                     // rows a lane loads before it works on them
#define PS_HS (DV_PAIRSTAT_MAX_BINS + 1)        // pitch of the LDS histogram: the bins and the non-finite counter
#define PS_MAX_GRID 1024                        // four workgroups per CU
#define PS_SUMS 9                               // 3 categories x {s, s^2, w}
#define PS_EXTS 6                               // 3 categories x {min, max}
#define PS_SLOT_BYTES (PS_SUMS * 8 + PS_EXTS * 4)
#define PS_FOLD_CHUNK 256                       // workgroup partials the fold kernel stages in LDS at a time

static inline int64_t pairstat_tiles(int32_t R, int32_t n_cols) { return cdiv64(R, PS_TR) * cdiv64(n_cols, PS_TC); }
static inline int pairstat_grid(int32_t R, int32_t n_cols) {
  const int64_t tiles = pairstat_tiles(R, n_cols);
  return (int)(tiles < PS_MAX_GRID ? tiles : PS_MAX_GRID);
}

__global__ void __launch_bounds__(PS_THREADS) pairstat_zero_kernel(unsigned long long* __restrict__ hist, int ldh, int bins) {
  for (int i = threadIdx.x; i < 3 * (bins + 1); i += PS_THREADS) hist[(size_t)(i / (bins + 1)) * ldh + i % (bins + 1)] = 0ull;
}

// VEC: lane `tid` owns the columns c0 + 4 tid + u (one 16-byte load per row); otherwise c0 + tid + 256 u (four coalesced 4-byte loads)
template <bool VEC>
__global__ void __launch_bounds__(PS_THREADS)
pairstat_kernel(const float* __restrict__ sim, int ld, uint32_t R, uint32_t n_cols, const int* __restrict__ row_vid,
                const int* __restrict__ row_cls, const int* __restrict__ col_vid, const int* __restrict__ col_cls, long long diag,
                int mult, float t2, float half_bins, int bins, unsigned long long* __restrict__ hist, int ldh,
                double* __restrict__ ws_sum, float* __restrict__ ws_ext, uint32_t gx, uint32_t n_tiles) {
  __shared__ unsigned int lh[3 * PS_HS];
  __shared__ int srv[PS_TR], src[PS_TR];
  __shared__ double wsum[PS_THREADS / 64][PS_SUMS];
  __shared__ float wext[PS_THREADS / 64][PS_EXTS];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 3 * PS_HS; i += PS_THREADS) lh[i] = 0u;
  double acc[PS_SUMS];
  float mn[3], mx[3];
#pragma unroll
  for (int i = 0; i < PS_SUMS; ++i) acc[i] = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mn[c] = INFINITY;
    mx[c] = -INFINITY;
  }
  const float top = (float)(bins - 1);

  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t ty = tile / gx, tx = tile - ty * gx;
    const uint32_t r0 = ty * PS_TR, c0 = tx * PS_TC;
    __syncthreads();                     // the histogram is zeroed; the previous tile's row ids are no longer read
    if (tid < PS_TR) {
      const uint32_t r = r0 + tid;
      srv[tid] = r < R ? row_vid[r] : 0;
      src[tid] = r < R ? row_cls[r] : 0;
    }
    uint32_t j[4];
    int cv[4], cc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      j[u] = c0 + (VEC ? 4 * tid + u : tid + PS_THREADS * u);
      cv[u] = j[u] < n_cols ? col_vid[j[u]] : 0;
      cc[u] = j[u] < n_cols ? col_cls[j[u]] : 0;
    }
    __syncthreads();
    const uint32_t nr = R - r0 < PS_TR ? R - r0 : PS_TR;
    for (uint32_t rb = 0; rb < nr; rb += PS_ROWS_IN_FLIGHT) {
      float v[PS_ROWS_IN_FLIGHT][4];
#pragma unroll
      for (int q = 0; q < PS_ROWS_IN_FLIGHT; ++q) {
        const float* p = sim + (size_t)(r0 + rb + q) * ld;
        const bool row = rb + q < nr;
        if (VEC && row && j[3] < n_cols) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(p + j[0]);
          v[q][0] = x.x; v[q][1] = x.y; v[q][2] = x.z; v[q][3] = x.w;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[q][u] = (row && j[u] < n_cols) ? p[j[u]] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < PS_ROWS_IN_FLIGHT; ++q) {
        const uint32_t rr = rb + q;      // <= 63: rb is a multiple of PS_ROWS_IN_FLIGHT below nr <= 64
        const bool row = rr < nr;
        const int rv = srv[rr], rc = src[rr];
        const long long dj = diag + (long long)(r0 + rr);
        const uint32_t self = (dj >= 0 && dj < (long long)n_cols) ? (uint32_t)dj : 0xffffffffu;    // no column has that index
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float s = v[q][u];
          const bool valid = row && j[u] < n_cols && j[u] != self;
          const int cat = rv == cv[u] ? 0 : (rc == cc[u] ? 1 : 2);
          const bool fin = fabsf(s) < INFINITY;                             // false for NaN and the infinities
          const float fb = fminf(fmaxf(floorf((s + 1.0f) * half_bins), 0.f), top);
          const int key = valid ? cat * PS_HS + (fin ? (int)fb : bins) : -1;
          // similarities crowd into a few bins: the lanes that share the first lane's counter add once, the rest one by one
          const int k0 = __builtin_amdgcn_readfirstlane(key);
          const unsigned long long same = __ballot(key == k0);
          if (key == k0) {
            if (k0 >= 0 && lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&lh[k0], (unsigned int)__popcll(same));
          } else if (key >= 0) {
            atomicAdd(&lh[key], 1u);
          }
          const bool use = valid && fin;
          const double ds = (double)s;
          const double d2 = ds * ds;
          const double dw = (double)expf((s - 1.0f) * t2);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const bool sel = use && cat == c;
            acc[3 * c + 0] += sel ? ds : 0.0;
            acc[3 * c + 1] += sel ? d2 : 0.0;
            acc[3 * c + 2] += sel ? dw : 0.0;
            mn[c] = sel ? fminf(mn[c], s) : mn[c];
            mx[c] = sel ? fmaxf(mx[c], s) : mx[c];
          }
        }
      }
    }
  }

  // lanes -> wavefront (xor butterfly: a fixed tree) -> workgroup (wavefronts in ascending order) -> workspace[blockIdx.x]
#pragma unroll
  for (int i = 0; i < PS_SUMS; ++i) acc[i] = wave_sum_f64(acc[i]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mn[c] = wave_min(mn[c]);
    mx[c] = wave_max(mx[c]);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < PS_SUMS; ++i) wsum[tid >> 6][i] = acc[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wext[tid >> 6][2 * c] = mn[c];
      wext[tid >> 6][2 * c + 1] = mx[c];
    }
  }
  __syncthreads();                       // also: every LDS count of the workgroup has landed
  if (tid < PS_SUMS) {
    double s = wsum[0][tid];
    for (int w = 1; w < PS_THREADS / 64; ++w) s += wsum[w][tid];
    ws_sum[(size_t)blockIdx.x * PS_SUMS + tid] = s * (double)mult;          // mult is 1 or 2: exact
  } else if (tid < PS_SUMS + PS_EXTS) {
    const int e = tid - PS_SUMS;
    float x = wext[0][e];
    for (int w = 1; w < PS_THREADS / 64; ++w) x = (e & 1) ? fmaxf(x, wext[w][e]) : fminf(x, wext[w][e]);
    ws_ext[(size_t)blockIdx.x * PS_EXTS + e] = x;
  }
  for (int i = tid; i < 3 * PS_HS; i += PS_THREADS) {
    const int c = i / PS_HS, b = i - c * PS_HS;
    const unsigned int n = lh[i];
    if (b <= bins && n) atomicAdd(&hist[(size_t)c * ldh + b], (unsigned long long)n * (unsigned long long)mult);
  }
}

// One workgroup: the G partials in ascending order (staged through LDS, coalesced), then the total into the state.
__global__ void __launch_bounds__(PS_THREADS) pairstat_fold_kernel(const double* __restrict__ ws_sum, const float* __restrict__ ws_ext,
                                                                   int G, double* __restrict__ sums, float* __restrict__ ext, int first) {
  __shared__ double sd[PS_FOLD_CHUNK * PS_SUMS];
  __shared__ float se[PS_FOLD_CHUNK * PS_EXTS];
  const int tid = threadIdx.x;
  const int e = tid - PS_SUMS;
  double a = 0.0;
  float x = (e & 1) ? -INFINITY : INFINITY;
  for (int base = 0; base < G; base += PS_FOLD_CHUNK) {
    const int n = G - base < PS_FOLD_CHUNK ? G - base : PS_FOLD_CHUNK;
    __syncthreads();
    for (int i = tid; i < n * PS_SUMS; i += PS_THREADS) sd[i] = ws_sum[(size_t)base * PS_SUMS + i];
    for (int i = tid; i < n * PS_EXTS; i += PS_THREADS) se[i] = ws_ext[(size_t)base * PS_EXTS + i];
    __syncthreads();
    if (tid < PS_SUMS) {
      for (int g = 0; g < n; ++g) a += sd[g * PS_SUMS + tid];
    } else if (e < PS_EXTS) {
      for (int g = 0; g < n; ++g) x = (e & 1) ? fmaxf(x, se[g * PS_EXTS + e]) : fminf(x, se[g * PS_EXTS + e]);
    }
  }
  if (tid < PS_SUMS) {
    const int at = 4 * (tid / 3) + tid % 3;                                 // sums [3][4]
    sums[at] = first ? a : sums[at] + a;
  } else if (e < PS_EXTS) {
    ext[e] = first ? x : ((e & 1) ? fmaxf(ext[e], x) : fminf(ext[e], x));
  } else if (first && e < PS_EXTS + 3) {
    sums[4 * (e - PS_EXTS) + 3] = 0.0;
  }
}

extern "C" int64_t dv_pairstat_workspace(int32_t R, int32_t n_cols) {
  if (R <= 0 || n_cols <= 0) return DV_EINVAL;
  return (int64_t)pairstat_grid(R, n_cols) * PS_SLOT_BYTES;
}

extern "C" int dv_pairstat_accum_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, const int32_t* row_vid,
                                     const int32_t* row_cls, const int32_t* col_vid, const int32_t* col_cls, int64_t diag,
                                     int32_t mult, float t, int32_t bins, double* sums, float* ext, uint64_t* hist, int32_t ldh,
                                     void* workspace, int32_t first, void* stream) {
  // R * n_cols <= 2^32 - 1: no 32-bit LDS counter of a workgroup can overflow within one call
  if (!sim || !row_vid || !row_cls || !col_vid || !col_cls || !sums || !ext || !hist || !workspace || R <= 0 || n_cols <= 0 ||
      ld < n_cols || bins < 1 || bins > DV_PAIRSTAT_MAX_BINS || ldh < bins + 1 || (mult != 1 && mult != 2) || !(t >= 0.f) ||
      !(t < INFINITY) || (int64_t)R * n_cols > 0xffffffffLL)
    return DV_EINVAL;
  if (((uintptr_t)sums | (uintptr_t)hist | (uintptr_t)workspace) & 7) return DV_EALIGN;
  const int G = pairstat_grid(R, n_cols);
  const uint32_t gx = (uint32_t)cdiv64(n_cols, PS_TC), n_tiles = (uint32_t)pairstat_tiles(R, n_cols);
  double* ws_sum = (double*)workspace;
  float* ws_ext = (float*)((char*)workspace + (size_t)G * PS_SUMS * 8);
  unsigned long long* h = (unsigned long long*)hist;
  if (first) hipLaunchKernelGGL(pairstat_zero_kernel, dim3(1), dim3(PS_THREADS), 0, ST(stream), h, ldh, bins);
  const float t2 = 2.0f * t, half_bins = 0.5f * (float)bins;
  if (aligned16(sim) && ld % 4 == 0)
    hipLaunchKernelGGL(pairstat_kernel<true>, dim3(G), dim3(PS_THREADS), 0, ST(stream), sim, ld, (uint32_t)R, (uint32_t)n_cols,
                       row_vid, row_cls, col_vid, col_cls, (long long)diag, mult, t2, half_bins, bins, h, ldh, ws_sum, ws_ext, gx,
                       n_tiles);
  else
    hipLaunchKernelGGL(pairstat_kernel<false>, dim3(G), dim3(PS_THREADS), 0, ST(stream), sim, ld, (uint32_t)R, (uint32_t)n_cols,
                       row_vid, row_cls, col_vid, col_cls, (long long)diag, mult, t2, half_bins, bins, h, ldh, ws_sum, ws_ext, gx,
                       n_tiles);
  hipLaunchKernelGGL(pairstat_fold_kernel, dim3(1), dim3(PS_THREADS), 0, ST(stream), ws_sum, ws_ext, G, sums, ext, first);
  return dv_launch_status();
}
