// t-SNE with sparse attraction and exact repulsion (include/dualvar_tsne.h: dv_tsne_perplexity_f32, dv_tsne_attract_f32,
// dv_tsne_repulse_workspace, dv_tsne_repulse_f32, dv_tsne_update_f32).
//
// The repulsion is the hot path: n^2 pairs of 2-D points per iteration, about a dozen fp32 operations and one v_rcp_f32 each,
// compute-bound.  A thread owns a row, a workgroup of TS_ROWS rows walks its part of the columns in tiles of TS_TILE points
// staged in LDS (every lane reads the same address: a broadcast), and (row, part) partials go to the workspace in double.  The
// perplexity search and the attraction run one wavefront per row over lists of at most 256 entries.  Every sum has a fixed
// order (no floating-point atomics): DESIGN.md, §6e.
#include "common.hpp"
#include "../../include/dualvar_tsne.h"

#define TS_ROWS DV_TSNE_ROWS
#define TS_TILE DV_TSNE_TILE
#define TS_SLOTS (DV_TOPK_MAX_K / 64)           // list slots a lane holds in registers
#define TS_TARGET_WGS 1024                      // four workgroups per CU

static_assert(TS_ROWS == TS_TILE, "the tile that holds a workgroup's own rows is found as tile == blockIdx.x");
static_assert(TS_ROWS == 256, "block_sum_f64 folds four wavefronts");

// ---------------------------------------------------------------------------------------------------------- perplexity
__global__ void __launch_bounds__(64) tsne_perplexity_kernel(const float* __restrict__ top_val, const int* __restrict__ top_idx,
                                                             int ldk, int k1, int row0, float target, float* __restrict__ p,
                                                             float* __restrict__ beta_out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* tv = top_val + (size_t)r * ldk;
  const int* ti = top_idx + (size_t)r * ldk;
  float d[TS_SLOTS], w[TS_SLOTS];
  bool in[TS_SLOTS];
  float m = INFINITY;
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < TS_SLOTS; ++u) {
    const int j = lane + 64 * u;
    in[u] = false;
    d[u] = 0.f;
    if (j < k1) {
      const int idx = ti[j];
      in[u] = idx >= 0 && idx != row0 + r;
      d[u] = fmaxf(2.0f - 2.0f * tv[j], 0.0f);
    }
    if (in[u]) {
      m = fminf(m, d[u]);
      ++cnt;
    }
  }
  m = wave_min(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  float emax = 0.f;
#pragma unroll
  for (int u = 0; u < TS_SLOTS; ++u) {
    d[u] = (in[u] && d[u] != m) ? d[u] - m : 0.f;        // e_j from here on
    emax = fmaxf(emax, d[u]);
  }
  emax = wave_max(emax);
  float beta = cnt > 0 ? DV_TSNE_BETA_START : 0.f;
  float lo = 0.f, hi = INFINITY, S = 1.f;
  const int steps = (cnt > 0 && emax > 0.f) ? DV_TSNE_MAX_STEPS : 1;      // all distances equal: one evaluation, no search
  for (int step = 0; step < steps; ++step) {
    float s = 0.f, a = 0.f;
#pragma unroll
    for (int u = 0; u < TS_SLOTS; ++u) {
      const float x = beta * d[u];
      w[u] = in[u] ? expf(-x) : 0.f;
      s += w[u];
      a += w[u] > 0.f ? w[u] * d[u] : 0.f;
    }
    S = wave_sum(s);
    const float A = wave_sum(a);
    const float diff = (logf(S) + (beta * A) / S) - target;
    if (fabsf(diff) <= DV_TSNE_ENTROPY_TOL || step == steps - 1) break;      // S, A are equal on all lanes: uniform
    if (diff > 0.f) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0f : (beta + hi) * 0.5f;
    } else {
      hi = beta;
      beta = (lo + beta) * 0.5f;
    }
  }
#pragma unroll
  for (int u = 0; u < TS_SLOTS; ++u) {
    const int j = lane + 64 * u;
    if (j < k1) p[(size_t)r * ldk + j] = (in[u] && cnt > 0) ? w[u] / S : 0.f;
  }
  if (lane == 0) beta_out[r] = beta;
}

extern "C" int dv_tsne_perplexity_f32(const float* top_val, const int32_t* top_idx, int32_t ldk, int32_t n, int32_t k1,
                                      int32_t row0, float perplexity, float* p, float* beta, void* stream) {
  if (!top_val || !top_idx || !p || !beta || n <= 0 || k1 < 1 || k1 > DV_TOPK_MAX_K || ldk < k1 ||
      (int64_t)n * ldk > 0x7fffffffLL || row0 < 0 || (int64_t)row0 + n > 0x7fffffffLL || !(perplexity >= 1.f) ||
      !(perplexity < INFINITY))
    return DV_EINVAL;
  const float target = (float)log((double)perplexity);
  hipLaunchKernelGGL(tsne_perplexity_kernel, dim3(n), dim3(64), 0, ST(stream), top_val, top_idx, ldk, k1, row0, target, p, beta);
  return dv_launch_status();
}

// ---------------------------------------------------------------------------------------------------------- attraction
struct ts_acc3 {
  double x, y, c;
};

__device__ __forceinline__ void tsne_edge(const float* __restrict__ y, float yix, float yiy, int j, float c, ts_acc3& acc) {
  const float dx = yix - y[2 * (size_t)j], dy = yiy - y[2 * (size_t)j + 1];
  const float d2 = dx * dx + dy * dy;
  const float cq = c * (1.0f / (1.0f + d2));
  acc.x += (double)(cq * dx);
  acc.y += (double)(cq * dy);
  acc.c += (double)(c * log1pf(d2));
}

__global__ void __launch_bounds__(64) tsne_attract_kernel(const float* __restrict__ y, const int* __restrict__ top_idx,
                                                          const float* __restrict__ p, int ldk, int n, int k1,
                                                          const int* __restrict__ rev_ptr, const int* __restrict__ rev_edge, int E,
                                                          float* __restrict__ fa, float* __restrict__ ce_row) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const float yix = y[2 * (size_t)i], yiy = y[2 * (size_t)i + 1];
  const float inv2n = 0.5f / (float)n;
  const int total = n * ldk;                    // <= 2^31 - 1 (checked by the host)
  ts_acc3 acc = {0.0, 0.0, 0.0};
  for (int s = lane; s < k1; s += 64) {
    const float pe = p[(size_t)i * ldk + s];
    const int j = top_idx[(size_t)i * ldk + s];
    if (pe > 0.f && j >= 0 && j < n) tsne_edge(y, yix, yiy, j, pe * inv2n, acc);
  }
  int e0 = rev_ptr[i], e1 = rev_ptr[i + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > E ? E : e1;
  for (int e = e0 + lane; e < e1; e += 64) {
    const int f = rev_edge[e];
    if (f >= 0 && f < total) {
      const float pe = p[f];
      if (pe > 0.f) tsne_edge(y, yix, yiy, f / ldk, pe * inv2n, acc);
    }
  }
  acc.x = wave_sum_f64(acc.x);
  acc.y = wave_sum_f64(acc.y);
  acc.c = wave_sum_f64(acc.c);
  if (lane == 0) {
    fa[2 * (size_t)i] = (float)acc.x;
    fa[2 * (size_t)i + 1] = (float)acc.y;
    ce_row[i] = (float)acc.c;
  }
}

// one workgroup: thread t adds v[t], v[t + 256], ... in ascending order, then the block fold
template <typename T>
__global__ void __launch_bounds__(256) tsne_total_kernel(const T* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)v[i];
  a = block_sum_f64(a, sh);
  if (threadIdx.x == 0) *out = a;
}

extern "C" int dv_tsne_attract_f32(const float* y, const int32_t* top_idx, const float* p, int32_t ldk, int32_t n, int32_t k1,
                                   const int32_t* rev_ptr, const int32_t* rev_edge, int32_t E, float* fa, float* ce_row,
                                   double* ce_sum, void* stream) {
  if (!y || !top_idx || !p || !rev_ptr || !rev_edge || !fa || !ce_row || n <= 0 || n > (1 << 24) || k1 < 1 ||
      k1 > DV_TOPK_MAX_K || ldk < k1 || (int64_t)n * ldk > 0x7fffffffLL || E < 0)
    return DV_EINVAL;
  if (((uintptr_t)y | (uintptr_t)fa | (uintptr_t)ce_sum) & 7) return DV_EALIGN;
  hipLaunchKernelGGL(tsne_attract_kernel, dim3(n), dim3(64), 0, ST(stream), y, top_idx, p, ldk, n, k1, rev_ptr, rev_edge, E, fa,
                     ce_row);
  if (ce_sum) hipLaunchKernelGGL(tsne_total_kernel<float>, dim3(1), dim3(256), 0, ST(stream), ce_row, n, ce_sum);
  return dv_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ repulsion
static inline int tsne_row_blocks(int32_t n) { return (int)cdiv64(n, TS_ROWS); }
static inline int tsne_tiles(int32_t n) { return (int)cdiv64(n, TS_TILE); }
static inline int tsne_parts(int32_t n) {
  const int T = tsne_tiles(n), want = (int)cdiv64(TS_TARGET_WGS, tsne_row_blocks(n));
  return T < want ? T : want;
}

struct ts_pair_acc {
  float x, y, z;
};

// one column against the thread's row; SELF: the tile holds the row itself, whose pair is skipped
template <bool SELF>
__device__ __forceinline__ void tsne_pair(float yix, float yiy, float cx, float cy, bool self, ts_pair_acc& a) {
  const float dx = yix - cx, dy = yiy - cy;
  const float t = 1.0f + (dx * dx + dy * dy);
  float q = __builtin_amdgcn_rcpf(t);
  if (SELF) q = self ? 0.f : q;
  const float q2 = q * q;
  a.z += q;
  a.x += q2 * dx;
  a.y += q2 * dy;
}

template <bool SELF>
__device__ __forceinline__ void tsne_tile(const float2* __restrict__ tile, int nc, float yix, float yiy, int self_col, double& sx,
                                          double& sy, double& sz) {
  ts_pair_acc ev = {0.f, 0.f, 0.f}, od = {0.f, 0.f, 0.f};
  int c = 0;
#pragma unroll 4
  for (; c + 1 < nc; c += 2) {
    const float4 two = *reinterpret_cast<const float4*>(tile + c);          // c is even: 16-byte aligned
    tsne_pair<SELF>(yix, yiy, two.x, two.y, c == self_col, ev);
    tsne_pair<SELF>(yix, yiy, two.z, two.w, c + 1 == self_col, od);
  }
  if (c < nc) {
    const float2 one = tile[c];
    tsne_pair<SELF>(yix, yiy, one.x, one.y, c == self_col, ev);
  }
  sx += (double)(ev.x + od.x);
  sy += (double)(ev.y + od.y);
  sz += (double)(ev.z + od.z);
}

// grid (row blocks, parts); ws [parts][3][n] doubles
__global__ void __launch_bounds__(TS_ROWS) tsne_repulse_kernel(const float2* __restrict__ y, int n, int T, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float2 tile[TS_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * TS_ROWS + tid;
  const int S = gridDim.y, s = blockIdx.y;
  const int t0 = (int)((long long)s * T / S), t1 = (int)((long long)(s + 1) * T / S);
  const float2 yi = i < n ? y[i] : make_float2(0.f, 0.f);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * TS_TILE;
    const int nc = n - c0 < TS_TILE ? n - c0 : TS_TILE;
    __syncthreads();                     // the previous tile is no longer read
    if (tid < nc) tile[tid] = y[c0 + tid];
    __syncthreads();
    if (t == (int)blockIdx.x)            // uniform over the workgroup: its own rows are this tile's columns
      tsne_tile<true>(tile, nc, yi.x, yi.y, tid, sx, sy, sz);
    else
      tsne_tile<false>(tile, nc, yi.x, yi.y, -1, sx, sy, sz);
  }
  if (i < n) {
    double* w = ws + (size_t)s * 3 * n;
    w[i] = sx;
    w[(size_t)n + i] = sy;
    w[2 * (size_t)n + i] = sz;
  }
}

// parts in ascending order per row; fr; the block's Z into zblock[blockIdx.x]
__global__ void __launch_bounds__(TS_ROWS) tsne_repulse_fold_kernel(const double* __restrict__ ws, int n, int S, float* __restrict__ fr,
                                                                    double* __restrict__ zblock) {
  __shared__ double sh[4];
  const int i = blockIdx.x * TS_ROWS + threadIdx.x;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (i < n) {
    for (int s = 0; s < S; ++s) {
      const double* w = ws + (size_t)s * 3 * n;
      sx += w[i];
      sy += w[(size_t)n + i];
      sz += w[2 * (size_t)n + i];
    }
    fr[2 * (size_t)i] = (float)sx;
    fr[2 * (size_t)i + 1] = (float)sy;
  }
  sz = block_sum_f64(sz, sh);
  if (threadIdx.x == 0) zblock[blockIdx.x] = sz;
}

extern "C" int64_t dv_tsne_repulse_workspace(int32_t n, int32_t* parts) {
  if (n <= 0) return DV_EINVAL;
  const int S = tsne_parts(n);
  if (parts) *parts = S;
  return (int64_t)24 * n * S + (int64_t)8 * tsne_row_blocks(n);
}

extern "C" int dv_tsne_repulse_f32(const float* y, int32_t n, float* fr, double* Z, void* workspace, void* stream) {
  if (!y || !fr || !Z || !workspace || n <= 0) return DV_EINVAL;
  if (((uintptr_t)y | (uintptr_t)fr | (uintptr_t)Z | (uintptr_t)workspace) & 7) return DV_EALIGN;
  const int B = tsne_row_blocks(n), T = tsne_tiles(n), S = tsne_parts(n);
  double* ws = (double*)workspace;
  double* zblock = ws + (size_t)3 * n * S;
  hipLaunchKernelGGL(tsne_repulse_kernel, dim3(B, S), dim3(TS_ROWS), 0, ST(stream), (const float2*)y, n, T, ws);
  hipLaunchKernelGGL(tsne_repulse_fold_kernel, dim3(B), dim3(TS_ROWS), 0, ST(stream), ws, n, S, fr, zblock);
  hipLaunchKernelGGL(tsne_total_kernel<double>, dim3(1), dim3(256), 0, ST(stream), zblock, B, Z);
  return dv_launch_status();
}

// --------------------------------------------------------------------------------------------------------------- update
__global__ void __launch_bounds__(256) tsne_update_kernel(float* __restrict__ y, float* __restrict__ vel, float* __restrict__ gain,
                                                          const float* __restrict__ fa, const float* __restrict__ fr,
                                                          const double* __restrict__ Z, long long m, float exaggeration,
                                                          float momentum, float lr, float min_gain) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float r = (float)((double)fr[i] / *Z);
  const float g = 4.0f * (exaggeration * fa[i] - r);
  const float v = vel[i];
  float gn = gain[i];
  gn = ((g > 0.f) != (v > 0.f)) ? gn + 0.2f : gn * 0.8f;
  gn = fmaxf(gn, min_gain);
  const float vn = momentum * v - (lr * gn) * g;
  gain[i] = gn;
  vel[i] = vn;
  y[i] = y[i] + vn;
}

extern "C" int dv_tsne_update_f32(float* y, float* vel, float* gain, const float* fa, const float* fr, const double* Z, int64_t m,
                                  float exaggeration, float momentum, float lr, float min_gain, void* stream) {
  const float inf = INFINITY;
  if (!y || !vel || !gain || !fa || !fr || !Z || m <= 0 || !(fabsf(exaggeration) < inf) || !(momentum >= 0.f) ||
      !(momentum < inf) || !(lr >= 0.f) || !(lr < inf) || !(min_gain >= 0.f) || !(min_gain < inf) || cdiv64(m, 256) > 0x7fffffffLL)
    return DV_EINVAL;
  if ((uintptr_t)Z & 7) return DV_EALIGN;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, ST(stream), y, vel, gain, fa, fr, Z,
                     (long long)m, exaggeration, momentum, lr, min_gain);
  return dv_launch_status();
}
