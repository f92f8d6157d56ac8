// S3D-G self gating and the spatial mean on gfx950: per-sample column sums, the gate's scale and its gradients, and the forms
// that apply the BatchNorm + ReLU in front of the gate on load.  (The gated BatchNorm backward is in batchnorm.hip.)
#include "streaming.hpp"

namespace {

// ------------------------------------------------------------------ spatial mean / gating
// Per-sample column sums over the S positions.  Large levels are split over CHANNEL chunks (grid.y, `ccv` 16-byte vectors =
// >= 256 bytes of a row each), not over positions: every output element has one owner, so there are no float atomics and no
// memset in front -- the results do not depend on the order workgroups finish in.
template <typename T>
__global__ void spatial_mean_kernel(const T* __restrict__ x, int ldx, int S, int C, int CP, int ccv, float* __restrict__ out) {
  constexpr int V = DT<T>::VEC;
  const int n = blockIdx.x;
  const float inv = 1.f / (float)S;
  const int cb = (int)blockIdx.y * ccv * V, cpl = min(ccv * V, CP - cb);
  if (cpl <= 0) return;
  column_reduce<V, 1>(
      (int64_t)n * S, (int64_t)(n + 1) * S, cpl,
      [&](int64_t r, int c0, float(&acc)[1][V]) {
        float v[V];
        Pack16<T>::load(x + r * ldx + cb + c0, v);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0][e] += v[e];
      },
      [&](int c0, float(&acc)[1][V]) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (cb + c0 + e < C) out[(size_t)n * C + cb + c0 + e] = acc[0][e] * inv;
      });
}

template <typename T>
__global__ void gate_bwd_reduce_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x, int ldx,
                                       const float* __restrict__ g, int S, int C, int CP, int ccv, float* __restrict__ dpre,
                                       int x_is_output) {
  constexpr int V = DT<T>::VEC;
  const int n = blockIdx.x;
  const int cb = (int)blockIdx.y * ccv * V, cpl = min(ccv * V, CP - cb);
  if (cpl <= 0) return;
  column_reduce<V, 1>(
      (int64_t)n * S, (int64_t)(n + 1) * S, cpl,
      [&](int64_t r, int c0, float(&acc)[1][V]) {
        float a[V], b[V];
        Pack16<T>::load(dy + r * lddy + cb + c0, a);
        Pack16<T>::load(x + r * ldx + cb + c0, b);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0][e] += a[e] * b[e];
      },
      [&](int c0, float(&acc)[1][V]) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (cb + c0 + e < C) {
            const float gg = g[(size_t)n * C + cb + c0 + e];
            dpre[(size_t)n * C + cb + c0 + e] = x_is_output ? acc[0][e] * (1.f - gg) : acc[0][e] * gg * (1.f - gg);
          }
      });
}

// Self gating with the BatchNorm + ReLU in front of it applied on load (engine.FUSE_GATE): the un-gated concat is never written.
// The gated members of a level are `items` (x, ldx, scale, shift, C; y, ldy for the scale), gate_off[k] is member k's first column
// in the level's [N][Ct] tables (-1: not a gated member, skipped); widths and offsets are multiples of 8 channels, so a 16-byte
// channel vector never straddles two members.
//
// gate_mean_bn_kernel is spatial_mean_kernel over the VIRTUAL concat: same grid, same channel chunks, same column_reduce
// decomposition as the launch over the real concat buffer -- the same additions in the same order, applied to the values
// bn_apply_multi would have stored.
template <typename T>
__global__ void gate_mean_bn_kernel(const dv_bn_item* __restrict__ items, int n, const int32_t* __restrict__ gate_off, int S, int Ct,
                                    int ccv, float* __restrict__ out) {
  constexpr int V = DT<T>::VEC;
  const int nn = blockIdx.x;
  const float inv = 1.f / (float)S;
  const int cb = (int)blockIdx.y * ccv * V, cpl = min(ccv * V, Ct - cb);
  if (cpl <= 0) return;
  const T* xp;                                     // the owning member's x at this thread's channel vector
  int ldx = 0;
  float sc[V], sh[V];
  column_reduce<V, 1>(
      (int64_t)nn * S, (int64_t)(nn + 1) * S, cpl,
      [&](int64_t r, int c0, float(&acc)[1][V]) {
        float v[V];
        Pack16<T>::load(xp + r * ldx, v);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0][e] += bn_relu_stored<T>(v[e], sc[e], sh[e]);
      },
      [&](int c0, float(&acc)[1][V]) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (cb + c0 + e < Ct) out[(size_t)nn * Ct + cb + c0 + e] = acc[0][e] * inv;
      },
      [&](int c0) {
        const int c = cb + c0;
        // (a vector no member owns -- the members do not tile [0, Ct) -- reads member 0 with a zero map: relu(0) = 0.  No test of
        // xp in the row loop: a branch there keeps the unrolled rows' loads from being in flight together, 12 -> 24 us.)
        xp = (const T*)items[0].x;
        ldx = items[0].ldx;
#pragma unroll
        for (int e = 0; e < V; ++e) sc[e] = sh[e] = 0.f;
        for (int k = 0; k < n; ++k) {
          const int off = gate_off[k];
          if (off >= 0 && c >= off && c < off + items[k].C) {
            xp = (const T*)items[k].x + (c - off);
            ldx = items[k].ldx;
            load_params<V>(items[k].scale, c - off, sc);
            load_params<V>(items[k].shift, c - off, sh);
          }
        }
      });
}

// blocks of one member in gate_scale_bn_kernel: four vectors per thread, at most 1024 blocks.  (bn_apply_multi's one vector per
// thread puts three dependent table reads in front of every 16 bytes moved: the 12 544-row levels took 19 us against
// rowscale's 12.)
constexpr uint32_t kGateScaleMaxBlocks = 1024;
__host__ __device__ inline uint32_t gate_scale_blocks(uint32_t vecs) {
  const uint32_t b = (vecs + 1023u) / 1024u;
  return b < 1u ? 1u : b > kGateScaleMaxBlocks ? kGateScaleMaxBlocks : b;
}

// y = relu(x*scale + shift) * g[n][off + c] into the members' concat slices: bn_apply_multi and rowscale_kernel<T, 0> in one
// pass.  Every block derives the members' block counts from the table (n <= 8), so the host needs no prefix.
template <typename T>
__global__ void gate_scale_bn_kernel(const dv_bn_item* __restrict__ items, int n, const int32_t* __restrict__ gate_off,
                                     const float* __restrict__ g, uint32_t M, FastDiv fS, int ldg) {
  constexpr int V = DT<T>::VEC;
  uint32_t bid = blockIdx.x, nblk = 0, start = 0;
  int i = -1;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t b = (k < n && gate_off[k] >= 0) ? gate_scale_blocks(M * (uint32_t)(items[k].C / V)) : 0u;
    if (i < 0 && bid < start + b) { i = k; nblk = b; bid -= start; }
    start += b;
  }
  if (i < 0) return;                               // (the host's grid is an upper bound of the sum)
  const dv_bn_item& it = items[i];
  const T* __restrict__ x = (const T*)it.x;
  T* __restrict__ y = (T*)it.y;
  const int ldx = it.ldx, ldy = it.ldy;
  const float* __restrict__ scale = it.scale;
  const float* __restrict__ shift = it.shift;
  const float* __restrict__ gi = g + gate_off[i];
  const FastDiv fcv = make_fastdiv((uint32_t)(it.C / V));
  const uint32_t CV = fcv.d, total = M * CV;
  for (uint32_t j = bid * blockDim.x + threadIdx.x; j < total; j += nblk * blockDim.x) {
    const uint32_t row = fd_div(j, fcv);
    const int c0 = (int)(j - row * CV) * V;
    float v[V], sc[V], sh[V], gv[V];
    Pack16<T>::load(x + (size_t)row * ldx + c0, v);
    load_params<V>(scale, c0, sc);
    load_params<V>(shift, c0, sh);
    load_params<V>(gi + (size_t)fd_div(row, fS) * ldg, c0, gv);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = bn_relu_stored<T>(v[e], sc[e], sh[e]) * gv[e];
    Pack16<T>::store(y + (size_t)row * ldy + c0, v);
  }
}

// MODE 0: y = x*g[n][c]          (gate_scale)
// MODE 1: dx (+)= dy*g + dmean/S  (gate_bwd_apply)
// MODE 2: dx (+)= dout[n][c]/S    (spatial_mean_bwd)
template <typename T, int MODE>
__global__ void rowscale_kernel(const T* __restrict__ a, int lda, const float* __restrict__ g,
                                const float* __restrict__ dm, uint32_t total, FastDiv fcv, FastDiv fS, int C,
                                T* __restrict__ o, int ldo, int accumulate) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = fcv.d;
  const float invS = 1.f / (float)fS.d;
  // 16-byte reads of the [N][C] tables only when a row of them is whole vectors up to CP: with C % V == 0 but C < CP (fp32,
  // C = 4 mod 8) the pad vector of the LAST sample would be read from behind the table
  const bool vec = (int)CV * V == C && (MODE == 2 || ((uintptr_t)g & 15) == 0) && (MODE == 0 || ((uintptr_t)dm & 15) == 0);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t row = fd_div(i, fcv);
    const int c0 = (int)(i - row * CV) * V;
    const int n = (int)fd_div(row, fS);
    float v[V], old[V];
    if (MODE != 2) Pack16<T>::load(a + (size_t)row * lda + c0, v);
    if (accumulate) Pack16<T>::load(o + (size_t)row * ldo + c0, old);
    float gv[V], dv[V];
    if (vec) {                                     // C == CP: the [N][C] fp32 rows are read as float4s
      if (MODE != 2) load_params<V>(g + (size_t)n * C, c0, gv);
      if (MODE != 0) load_params<V>(dm + (size_t)n * C, c0, dv);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const bool in = c0 + e < C;
        gv[e] = (MODE != 2 && in) ? g[(size_t)n * C + c0 + e] : 0.f;
        dv[e] = (MODE != 0 && in) ? dm[(size_t)n * C + c0 + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float r;
      if (MODE == 0) r = v[e] * gv[e];
      else if (MODE == 1) r = gate_grad(v[e], gv[e], dv[e], invS);
      else r = dv[e] * invS;
      if (!vec && c0 + e >= C) r = 0.f;
      v[e] = accumulate ? old[e] + r : r;
    }
    Pack16<T>::store(o + (size_t)row * ldo + c0, v);
  }
}

}  // namespace

// channel chunks per sample (16-byte vectors per chunk): ~1024 workgroups in all, at least 16 vectors (256 bytes of a row) each,
// and one chunk when a sample has fewer than 128 positions (the row groups of one workgroup cover it)
static int c_chunk_vecs(int N, int S, int CV) {
  int chunks = (1024 + N - 1) / N;
  const int cap = (CV + 15) / 16;
  if (chunks > cap) chunks = cap;
  if (chunks < 1 || S < 128) chunks = 1;
  return (CV + chunks - 1) / chunks;
}
// grid.y of the three per-sample column reductions: the launches and dv_spatial_chunks both take it from here
static int spatial_grid_y(int N, int S, int CV, int& ccv) {
  ccv = c_chunk_vecs(N, S, CV);
  return (CV + ccv - 1) / ccv;
}

extern "C" int dv_spatial_chunks(int32_t dtype, int32_t N, int32_t S, int32_t C) {
  if ((dtype != DV_F32 && dtype != DV_BF16) || N <= 0 || S <= 0 || C <= 0) return DV_EINVAL;
  int ccv;
  return spatial_grid_y(N, S, cp8(C) / (dtype == DV_F32 ? 4 : 8), ccv);
}

extern "C" int dv_spatial_mean(int32_t dtype, const void* x, int32_t ldx, int32_t N, int32_t S, int32_t C, float* out,
                               void* stream) {
  const int CP = cp8(C);
  if (!x || !out || N <= 0 || S <= 0 || C <= 0 || ldx < CP) return DV_EINVAL;
  if (!aligned16(x)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    if (ldx % DT<T>::VEC) return DV_EALIGN;
    int ccv;
    const int gy = spatial_grid_y(N, S, CP / DT<T>::VEC, ccv);
    hipLaunchKernelGGL((spatial_mean_kernel<T>), dim3(N, gy), dim3(kThreads), 0, ST(stream), (const T*)x, ldx, S,
                       C, CP, ccv, out);
  });
  return dv_launch_status();
}

extern "C" int dv_spatial_mean_bwd(int32_t dtype, const float* dout, int32_t N, int32_t S, int32_t C, void* dx,
                                   int32_t lddx, int32_t flags, void* stream) {
  const int CP = cp8(C);
  if (!dout || !dx || N <= 0 || S <= 0 || C <= 0 || lddx < CP) return DV_EINVAL;
  if (!aligned16(dx)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (lddx % V) return DV_EALIGN;
    const int64_t total = (int64_t)N * S * (CP / V);
    if (total >= (1ll << 31)) return DV_EINVAL;
    hipLaunchKernelGGL((rowscale_kernel<T, 2>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream),
                       (const T*)nullptr, 0, (const float*)nullptr, dout, (uint32_t)total, make_fastdiv((uint32_t)(CP / V)),
                       make_fastdiv((uint32_t)S), C, (T*)dx, lddx, (flags & DV_ACCUM) ? 1 : 0);
  });
  return dv_launch_status();
}

extern "C" int dv_gate_scale(int32_t dtype, const void* x, int32_t ldx, const float* g, int32_t N, int32_t S, int32_t C,
                             void* y, int32_t ldy, void* stream) {
  const int CP = cp8(C);
  if (!x || !g || !y || N <= 0 || S <= 0 || C <= 0 || ldx < CP || ldy < CP) return DV_EINVAL;
  if (!aligned16(x) || !aligned16(y)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (ldx % V || ldy % V) return DV_EALIGN;
    const int64_t total = (int64_t)N * S * (CP / V);
    if (total >= (1ll << 31)) return DV_EINVAL;
    hipLaunchKernelGGL((rowscale_kernel<T, 0>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream),
                       (const T*)x, ldx, g, (const float*)nullptr, (uint32_t)total, make_fastdiv((uint32_t)(CP / V)),
                       make_fastdiv((uint32_t)S), C, (T*)y, ldy, 0);
  });
  return dv_launch_status();
}

extern "C" int dv_gate_bwd_reduce(int32_t dtype, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* g,
                                  int32_t N, int32_t S, int32_t C, float* dpre, int32_t x_is_output, void* stream) {
  const int CP = cp8(C);
  if (!dy || !x || !g || !dpre || N <= 0 || S <= 0 || C <= 0 || lddy < CP || ldx < CP) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(x)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    if (lddy % DT<T>::VEC || ldx % DT<T>::VEC) return DV_EALIGN;
    int ccv;
    const int gy = spatial_grid_y(N, S, CP / DT<T>::VEC, ccv);
    hipLaunchKernelGGL((gate_bwd_reduce_kernel<T>), dim3(N, gy), dim3(kThreads), 0, ST(stream), (const T*)dy,
                       lddy, (const T*)x, ldx, g, S, C, CP, ccv, dpre, x_is_output);
  });
  return dv_launch_status();
}

extern "C" int dv_gate_bwd_apply(int32_t dtype, const void* dy, int32_t lddy, const float* g, const float* dmean, int32_t N,
                                 int32_t S, int32_t C, void* dx, int32_t lddx, int32_t flags, void* stream) {
  const int CP = cp8(C);
  if (!dy || !g || !dmean || !dx || N <= 0 || S <= 0 || C <= 0 || lddy < CP || lddx < CP) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(dx)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (lddy % V || lddx % V) return DV_EALIGN;
    const int64_t total = (int64_t)N * S * (CP / V);
    if (total >= (1ll << 31)) return DV_EINVAL;
    hipLaunchKernelGGL((rowscale_kernel<T, 1>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream),
                       (const T*)dy, lddy, g, dmean, (uint32_t)total, make_fastdiv((uint32_t)(CP / V)),
                       make_fastdiv((uint32_t)S), C, (T*)dx, lddx, (flags & DV_ACCUM) ? 1 : 0);
  });
  return dv_launch_status();
}

static int gate_fold_args(const dv_bn_item* items, int32_t n, const int32_t* gate_off, int32_t N, int32_t S, int32_t Ct) {
  if (!items || !gate_off || n <= 0 || n > 8 || N <= 0 || S <= 0 || Ct <= 0 || Ct % 8) return DV_EINVAL;
  if ((int64_t)N * S * (Ct / 4) >= (1ll << 31)) return DV_EINVAL;
  return DV_OK;
}

extern "C" int dv_gate_mean_bn(int32_t dtype, const dv_bn_item* items, int32_t n, const int32_t* gate_off, int32_t N, int32_t S,
                               int32_t Ct, float* mean, void* stream) {
  if (int rc = gate_fold_args(items, n, gate_off, N, S, Ct)) return rc;
  if (!mean) return DV_EINVAL;
  DISPATCH_T(dtype, {
    int ccv;
    const int gy = spatial_grid_y(N, S, Ct / DT<T>::VEC, ccv);
    hipLaunchKernelGGL((gate_mean_bn_kernel<T>), dim3(N, gy), dim3(kThreads), 0, ST(stream), items, n, gate_off,
                       S, Ct, ccv, mean);
  });
  return dv_launch_status();
}

extern "C" int dv_gate_scale_bn(int32_t dtype, const dv_bn_item* items, int32_t n, const int32_t* gate_off, const float* g,
                                int32_t N, int32_t S, int32_t Ct, void* stream) {
  if (int rc = gate_fold_args(items, n, gate_off, N, S, Ct)) return rc;
  if (!g) return DV_EINVAL;
  if (!aligned16(g)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    const uint32_t M = (uint32_t)N * (uint32_t)S, vecs = M * (uint32_t)(Ct / DT<T>::VEC);
    // sum_k min(cap, ceil(v_k / 1024)) <= min(cap n, ceil(sum_k v_k / 1024) + n); blocks past the members' sum return at once
    uint32_t grid = (vecs + 1023u) / 1024u + (uint32_t)n;
    if (grid > kGateScaleMaxBlocks * (uint32_t)n) grid = kGateScaleMaxBlocks * (uint32_t)n;
    hipLaunchKernelGGL((gate_scale_bn_kernel<T>), dim3(grid), dim3(kThreads), 0, ST(stream), items, n, gate_off, g, M,
                       make_fastdiv((uint32_t)S), Ct);
  });
  return dv_launch_status();
}
