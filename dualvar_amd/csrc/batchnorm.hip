// BatchNorm on gfx950: forward statistics and finalize, apply (+residual, +ReLU), backward reduce and apply -- each as a
// single-tensor launch and as one launch over a group's dv_bn_item table, the backward also with self gating taken on load.
// (The backward's two bodies are in streaming.hpp: pool.hip instantiates them over the pooled gradient.)
#include "streaming.hpp"

namespace {

// ------------------------------------------------------------------ BN forward statistics
struct BnFinalize {
  const float* gamma; const float* beta; float eps, momentum;
  float* running_mean; float* running_var; float* mean; float* invstd; float* scale; float* shift;
};
// THE finalize: channel c's mean, M2 about it and count -> mean / invstd / scale / shift / running statistics.  One expression
// for the fused single-rank form (bn_reduce_stats_body) and the two cross-rank kernels, which therefore agree bit for bit.
// F: a BnFinalize, or the dv_bn_item itself (the same member names), read where it lies.
template <typename F>
__device__ __forceinline__ void bn_finalize_channel(const F& f, int c, float mean, float M2, float cnt) {
  const float var = M2 / cnt;
  const float invstd = rsqrtf(var + f.eps);
  f.mean[c] = mean;
  f.invstd[c] = invstd;
  const float sc = f.gamma[c] * invstd;
  f.scale[c] = sc;
  f.shift[c] = f.beta[c] - mean * sc;
  if (f.running_mean) {
    f.running_mean[c] = (1.f - f.momentum) * f.running_mean[c] + f.momentum * mean;
    const float unbiased = cnt > 1.f ? M2 / (cnt - 1.f) : var;
    f.running_var[c] = (1.f - f.momentum) * f.running_var[c] + f.momentum * unbiased;
  }
}
// the cross-rank combine: the gathered [R][stride] table of local rows [sum C | M2 C | count] -> channel c's mean, M2, count
__device__ __forceinline__ void bn_combine_ranks(const float* stats, int R, int stride, int C, int c, float& mean, float& M2, float& cnt) {
  float n = 0.f, S = 0.f;
  for (int r = 0; r < R; ++r) { n += stats[r * stride + 2 * C]; S += stats[r * stride + c]; }
  const float mu = S / n;
  float q = 0.f;
  for (int r = 0; r < R; ++r) {
    float n_r = stats[r * stride + 2 * C];
    float d = stats[r * stride + c] / n_r - mu;
    q += stats[r * stride + C + c] + n_r * d * d;
  }
  mean = mu; M2 = q; cnt = n;
}
// one block per channel: partials [2][P][tiles] (a channel's tiles contiguous: coalesced) -> local [2C+1]; with `fin` set (single rank) the block also
// finalises the channel (mean / invstd / scale / shift / running statistics), saving a launch per BN layer
__device__ __forceinline__ void bn_reduce_stats_body(const float* __restrict__ part, int n_tiles, int tile_rows, int P,
                                                     int64_t M, int C, float* __restrict__ out, int fin,
                                                     const BnFinalize& f, int c) {
  __shared__ float sh[32];
  float s = 0.f;
  const float* ps = part + (size_t)c * n_tiles;                 // sums of channel c, one per tile
  const float* pq = part + ((size_t)P + c) * n_tiles;           // M2 about the tile mean
  for (int i = threadIdx.x; i < n_tiles; i += blockDim.x) s += ps[i];
  const float S = block_sum(s, sh);
  const float mean = S / (float)M;
  float m2 = 0.f;
  for (int i = threadIdx.x; i < n_tiles; i += blockDim.x) {
    int64_t left = M - (int64_t)i * tile_rows;
    float n_i = (float)(left < tile_rows ? left : tile_rows);
    float d = ps[i] / n_i - mean;
    m2 += pq[i] + n_i * d * d;
  }
  const float M2 = block_sum(m2, sh + 16);
  if (threadIdx.x == 0) {
    out[c] = S;
    out[C + c] = M2;
    if (c == 0) out[2 * C] = (float)M;
    if (fin) bn_finalize_channel(f, c, mean, M2, (float)M);
  }
}

__global__ void bn_reduce_stats_kernel(const float* __restrict__ part, int n_tiles, int tile_rows, int P, int64_t M, int C,
                                       float* __restrict__ out, int fin, BnFinalize f) {
  bn_reduce_stats_body(part, n_tiles, tile_rows, P, M, C, out, fin, f, blockIdx.x);
}

// locate the item a block of a multi-tensor launch belongs to: `end` is the running block-count prefix
// (the first eight prefixes are fetched with independent loads: a `while` over them is a chain of dependent global
// loads, ~1 us each, in front of every block of these latency-bound launches)
template <typename GetEnd>
__device__ __forceinline__ int find_item(int n, uint32_t& bid, uint32_t& nblk, GetEnd end) {
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = k < n ? (uint32_t)end(k) : 0xffffffffu;
  int i = 0;
  uint32_t start = 0, endv = e[0];
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (k < n - 1 && bid >= e[k]) { start = e[k]; i = k + 1; endv = e[k + 1]; }
  if (n > 8 && i == 7) {
    while (i < n - 1 && bid >= (uint32_t)end(i)) { start = (uint32_t)end(i); ++i; }
    endv = (uint32_t)end(i);
  }
  nblk = endv - start;
  bid -= start;
  return i;
}

__global__ void bn_stats_multi_kernel(const dv_bn_item* __restrict__ items, int n, int fin) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_stats; });
  const dv_bn_item& it = items[i];
  BnFinalize f = {it.gamma, it.beta, it.eps, it.momentum, it.running_mean, it.running_var, it.mean, it.invstd, it.scale, it.shift};
  bn_reduce_stats_body(it.partials, it.n_tiles, it.tile_rows, it.pitch, it.M, it.C, it.local_stats, fin, f, (int)bid);
}

__global__ void bn_finalize_kernel(const float* __restrict__ stats, int R, int stride, int C, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean,
                                   float* running_var, float* mean_o, float* invstd_o, float* scale_o,
                                   float* shift_o) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float mean, M2, cnt;
  bn_combine_ranks(stats, R, stride, C, c, mean, M2, cnt);
  bn_finalize_channel(BnFinalize{gamma, beta, eps, momentum, running_mean, running_var, mean_o, invstd_o, scale_o, shift_o}, c, mean, M2, cnt);
}

// the members of a group in ONE launch: item i's rows sit in the gathered [R][stride] table at the offset its
// local_stats has inside the group's local row; 128 channels per block, blocks of item i follow those of item i-1
__global__ void bn_finalize_multi_kernel(const dv_bn_item* __restrict__ items, int n, const float* __restrict__ local_base,
                                         const float* __restrict__ gathered, int R, int stride) {
  int bid = blockIdx.x, i = 0;
  while (i < n - 1 && bid >= (items[i].C + 127) / 128) { bid -= (items[i].C + 127) / 128; ++i; }
  const dv_bn_item& it = items[i];
  const int c = bid * 128 + threadIdx.x, C = it.C;
  if (c >= C) return;
  float mean, M2, cnt;
  bn_combine_ranks(gathered + (it.local_stats - local_base), R, stride, C, c, mean, M2, cnt);
  bn_finalize_channel(it, c, mean, M2, cnt);
}

// ------------------------------------------------------------------ BN apply (+residual) (+ReLU)
// i (vector index) -> (row, first channel) with one mulhi; parameters as 16-byte vector loads (the per-channel
// arrays are padded to a multiple of 8 floats)
template <typename T>
__device__ __forceinline__ void bn_apply_body(const T* __restrict__ x, int ldx, const float* __restrict__ scale,
                                              const float* __restrict__ shift, const T* __restrict__ res, int ldr,
                                              T* __restrict__ y, int ldy, uint32_t total, int C, const FastDiv& fcv,
                                              int flags, uint32_t bid, uint32_t nblk) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = fcv.d;
  for (uint32_t i = bid * blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
    const uint32_t row = fd_div(i, fcv);
    const int c0 = (int)(i - row * CV) * V;
    float v[V], r[V], sc[V], sh[V];
    Pack16<T>::load(x + (size_t)row * ldx + c0, v);
    if (res) Pack16<T>::load(res + (size_t)row * ldr + c0, r);
    load_params<V>(scale, c0, sc);
    load_params<V>(shift, c0, sh);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float o = bn_affine(v[e], sc[e], sh[e]);
      if (res) o += r[e];
      if (flags & DV_RELU) o = fmaxf(o, 0.f);
      v[e] = (c0 + e < C) ? o : 0.f;
    }
    Pack16<T>::store(y + (size_t)row * ldy + c0, v);
  }
}

template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ scale,
                                const float* __restrict__ shift, const T* __restrict__ res, int ldr,
                                T* __restrict__ y, int ldy, uint32_t total, int C, FastDiv fcv, int flags) {
  bn_apply_body<T>(x, ldx, scale, shift, res, ldr, y, ldy, total, C, fcv, flags, blockIdx.x, gridDim.x);
}

template <typename T>
__global__ void bn_apply_multi_kernel(const dv_bn_item* __restrict__ items, int n) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_apply; });
  const dv_bn_item& it = items[i];
  constexpr int V = DT<T>::VEC;
  const int CP = (it.C + 7) & ~7;
  bn_apply_body<T>((const T*)it.x, it.ldx, it.scale, it.shift, (const T*)it.residual, it.ldr, (T*)it.y, it.ldy,
                   (uint32_t)(it.M * (CP / V)), it.C, make_fastdiv((uint32_t)(CP / V)), it.fwd_flags, bid, nblk);
}

// Self gating folded into the BatchNorm backward of the gated members: g / dm point at the item's first column of the level's
// [N][ldg] gate tables (nullptr: this item is not gated -- block-uniform, a launch may mix both kinds), fS divides a row by S.
struct GateOnLoad {
  const float* g; const float* dm; FastDiv fS; int ldg; float invS;
};

// dL/dy as it lies in memory
template <typename T>
struct PlainDy {
  static constexpr int V = DT<T>::VEC, kRows = 0;
  static constexpr bool kPooled = false;
  struct Pend {};
  const T* dy; int lddy;
  __device__ __forceinline__ void load(int64_t r, int c0, float (&g)[V], Pend&) const { Pack16<T>::load(dy + r * lddy + c0, g); }
  __device__ __forceinline__ void finish(int64_t, int, float (&)[V], Pend&) const {}
};

// dL/dy behind a self-gating scale, as gate_bwd_apply would have left it in dy (ga.g == nullptr: the plain dy).
// (half the rows in flight -- two more vectors per row -- which keeps the registers at the plain kernel's occupancy; measured,
// 2 / 3 / 4 rows in flight run the step's gated reduces in 601 / 611 / 611 us)
// ROW_FIRST (the reduce): the gate's row is issued before dy -- these loads hit in L1 / L2 and come back at once; issued behind
// dy and x they cost 15 us more per step.  The apply issues them last, where they are not held across its other loads.
template <typename T, bool ROW_FIRST>
struct GatedDy {
  static constexpr int V = DT<T>::VEC, kRows = V == 4 ? 2 : 1;
  static constexpr bool kPooled = false;
  struct Pend { float gv[V], dv[V]; };
  const T* dy; int lddy; GateOnLoad ga;
  __device__ __forceinline__ void gate_row(int64_t r, int c0, Pend& p) const {
    const size_t go = (size_t)fd_div((uint32_t)r, ga.fS) * ga.ldg;
    load_params<V>(ga.g + go, c0, p.gv);
    load_params<V>(ga.dm + go, c0, p.dv);
  }
  __device__ __forceinline__ void load(int64_t r, int c0, float (&g)[V], Pend& p) const {
    if (ROW_FIRST && ga.g) gate_row(r, c0, p);
    Pack16<T>::load(dy + r * lddy + c0, g);
  }
  __device__ __forceinline__ void finish(int64_t r, int c0, float (&g)[V], Pend& p) const {
    if (!ga.g) return;
    if (!ROW_FIRST) gate_row(r, c0, p);
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = as_stored<T>(gate_grad(g[e], p.gv[e], p.dv[e], ga.invS));
  }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ y, int ldy,
                                     const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                                     const float* __restrict__ invstd, int64_t M, int C, int CP, int flags,
                                     int64_t rows_per_block, float* __restrict__ sums_all, int n_rep, float* __restrict__ ws) {
  bn_bwd_reduce_body<T>(PlainDy<T>{dy, lddy}, y, ldy, x, ldx, mean, invstd, M, C, CP, flags, rows_per_block, sums_all, n_rep,
                        blockIdx.x, nullptr, nullptr, ws, gridDim.x);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_multi_kernel(const dv_bn_item* __restrict__ items, int n) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_red; });
  const dv_bn_item& it = items[i];
  const int CP = (it.C + 7) & ~7;
  const int64_t rpb = (it.M + nblk - 1) / nblk;
  bn_bwd_reduce_body<T>(PlainDy<T>{(const T*)it.dy, it.lddy}, (const T*)it.y, it.ldy, (const T*)it.x, it.ldx, it.mean,
                        it.invstd, it.M, it.C, CP, it.bwd_flags, rpb, it.sums, it.n_rep, bid, it.scale, it.shift, it.red_ws, nblk);
}

__device__ __forceinline__ GateOnLoad gate_of_item(const int32_t* __restrict__ gate_off, int i, const float* g, const float* dm,
                                                   const FastDiv& fS, int ldg) {
  const int off = gate_off[i];
  GateOnLoad ga;
  ga.g = off >= 0 ? g + off : nullptr;
  ga.dm = off >= 0 ? dm + off : nullptr;
  ga.fS = fS; ga.ldg = ldg; ga.invS = 1.f / (float)fS.d;
  return ga;
}

// the same launch for a group that holds gated members (GateGroupOp, engine.FUSE_GATE): an instantiation of its own, so the
// plain kernel above keeps its registers
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_multi_gated_kernel(const dv_bn_item* __restrict__ items, int n,
                                                                            const int32_t* __restrict__ gate_off,
                                                                            const float* __restrict__ g, const float* __restrict__ dm,
                                                                            FastDiv fS, int ldg) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_red; });
  const dv_bn_item& it = items[i];
  const int CP = (it.C + 7) & ~7;
  const int64_t rpb = (it.M + nblk - 1) / nblk;
  bn_bwd_reduce_body<T>(GatedDy<T, true>{(const T*)it.dy, it.lddy, gate_of_item(gate_off, i, g, dm, fS, ldg)}, (const T*)it.y, it.ldy,
                        (const T*)it.x, it.ldx, it.mean, it.invstd, it.M, it.C, CP, it.bwd_flags, rpb, it.sums, it.n_rep, bid,
                        it.scale, it.shift, it.red_ws, nblk);
}

template <typename T>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ y, int ldy,
                                    const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                    const float* __restrict__ sums_g, int rep_g, float inv_count, float dscale,
                                    float* dgamma, float* dbeta, T* __restrict__ dx, int lddx,
                                    T* __restrict__ dres, int lddres, uint32_t total, int C, int CP, FastDiv fcv,
                                    int flags) {
  bn_bwd_apply_body<T>(PlainDy<T>{dy, lddy}, y, ldy, x, ldx, mean, invstd, gamma, sums_g, rep_g, inv_count, dscale, dgamma,
                       dbeta, dx, lddx, dres, lddres, total, C, CP, fcv, flags, blockIdx.x, gridDim.x, nullptr, nullptr);
}

template <typename T>
__global__ void bn_bwd_apply_multi_kernel(const dv_bn_item* __restrict__ items, int n) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_bapply; });
  const dv_bn_item& it = items[i];
  constexpr int V = DT<T>::VEC;
  const int CP = (it.C + 7) & ~7;
  bn_bwd_apply_body<T>(PlainDy<T>{(const T*)it.dy, it.lddy}, (const T*)it.y, it.ldy, (const T*)it.x, it.ldx, it.mean, it.invstd,
                       it.gamma, it.sums, it.n_rep, it.inv_count, it.dparam_scale, it.dgamma, it.dbeta, (T*)it.dx, it.lddx,
                       (T*)it.dres, it.lddres, (uint32_t)(it.M * (CP / V)), it.C, CP, make_fastdiv((uint32_t)(CP / V)),
                       it.bwd_flags, bid, nblk, it.scale, it.shift);
}

template <typename T>
__global__ void bn_bwd_apply_multi_gated_kernel(const dv_bn_item* __restrict__ items, int n, const int32_t* __restrict__ gate_off,
                                                const float* __restrict__ g, const float* __restrict__ dm, FastDiv fS, int ldg) {
  uint32_t bid = blockIdx.x, nblk;
  const int i = find_item(n, bid, nblk, [&](int k) { return items[k].blk_bapply; });
  const dv_bn_item& it = items[i];
  constexpr int V = DT<T>::VEC;
  const int CP = (it.C + 7) & ~7;
  bn_bwd_apply_body<T>(GatedDy<T, false>{(const T*)it.dy, it.lddy, gate_of_item(gate_off, i, g, dm, fS, ldg)}, (const T*)it.y, it.ldy,
                       (const T*)it.x, it.ldx, it.mean, it.invstd, it.gamma, it.sums, it.n_rep, it.inv_count, it.dparam_scale,
                       it.dgamma, it.dbeta, (T*)it.dx, it.lddx, (T*)it.dres, it.lddres, (uint32_t)(it.M * (CP / V)), it.C, CP,
                       make_fastdiv((uint32_t)(CP / V)), it.bwd_flags, bid, nblk, it.scale, it.shift);
}

}  // namespace

// eval-mode BatchNorm (running statistics): scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale;
// arrays are written up to round_up(C, 8) (pad lanes zero) for the 16-byte loads of dv_bn_apply
__global__ void bn_eval_coeffs_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv, float eps, int C, int CP,
                                      float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP) return;
  float sc = 0.f, sh = 0.f;
  if (c < C) {
    sc = gamma[c] * rsqrtf(rv[c] + eps);
    sh = beta[c] - rm[c] * sc;
  }
  scale[c] = sc;
  shift[c] = sh;
}

extern "C" int dv_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                 float eps, int32_t C, float* scale, float* shift, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || C <= 0) return DV_EINVAL;
  const int CP = cp8(C);
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((CP + 127) / 128), dim3(128), 0, ST(stream), gamma, beta, running_mean,
                     running_var, eps, C, CP, scale, shift);
  return dv_launch_status();
}

// BatchNorm partials of a small fp32 [M][C] matrix (BatchNorm1d of the classifier head, M = batch): one thread per
// channel, ONE tile: partials [2][C][1] = (sum, M2 about the mean), the format dv_bn_stats_finalize consumes
__global__ void bn_rows_partials_kernel(const float* __restrict__ x, int ldx, int M, int C, float* __restrict__ part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int r = 0; r < M; ++r) s += x[(size_t)r * ldx + c];
  const float mu = s / (float)M;
  float q = 0.f;
  for (int r = 0; r < M; ++r) { const float d = x[(size_t)r * ldx + c] - mu; q += d * d; }
  part[c] = s;
  part[C + c] = q;
}

extern "C" int dv_bn_rows_partials_f32(const float* x, int32_t ldx, int32_t M, int32_t C, float* partials, void* stream) {
  if (!x || !partials || M <= 0 || C <= 0 || ldx < C) return DV_EINVAL;
  hipLaunchKernelGGL(bn_rows_partials_kernel, dim3((C + 127) / 128), dim3(128), 0, ST(stream), x, ldx, M, C, partials);
  return dv_launch_status();
}

extern "C" int dv_bn_reduce_stats(const float* partials, int32_t n_tiles, int32_t tile_rows, int32_t pitch, int64_t M,
                                  int32_t C, float* local_stats, void* stream) {
  if (!partials || !local_stats || n_tiles <= 0 || C <= 0 || M <= 0 || pitch < C) return DV_EINVAL;
  BnFinalize f = {};
  hipLaunchKernelGGL(bn_reduce_stats_kernel, dim3(C), dim3(n_tiles >= 2048 ? 1024 : kThreads), 0, ST(stream), partials, n_tiles,
                     tile_rows, pitch, M, C, local_stats, 0, f);
  return dv_launch_status();
}

extern "C" int dv_bn_stats_finalize(const float* partials, int32_t n_tiles, int32_t tile_rows, int32_t pitch, int64_t M,
                                    int32_t C, float* local_stats, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                                    float* shift, void* stream) {
  if (!partials || !local_stats || n_tiles <= 0 || C <= 0 || M <= 0 || pitch < C) return DV_EINVAL;
  if (!gamma || !beta || !mean || !invstd || !scale || !shift) return DV_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return DV_EINVAL;
  BnFinalize f = {gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift};
  hipLaunchKernelGGL(bn_reduce_stats_kernel, dim3(C), dim3(n_tiles >= 2048 ? 1024 : kThreads), 0, ST(stream), partials, n_tiles,
                     tile_rows, pitch, M, C, local_stats, 1, f);
  return dv_launch_status();
}

extern "C" int dv_bn_stats_multi(const dv_bn_item* items, int32_t n, int32_t finalize, int32_t total_blocks, void* stream) {
  if (!items || n <= 0 || total_blocks <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(bn_stats_multi_kernel, dim3(total_blocks), dim3(kThreads), 0, ST(stream), items, n, finalize);
  return dv_launch_status();
}
extern "C" int dv_bn_finalize_multi(const dv_bn_item* items, int32_t n, int32_t total_blocks, const float* local_base,
                                    const float* gathered, int32_t R, int32_t stride, void* stream) {
  if (!items || n <= 0 || total_blocks <= 0 || !local_base || !gathered || R <= 0 || stride <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(bn_finalize_multi_kernel, dim3(total_blocks), dim3(128), 0, ST(stream), items, n, local_base, gathered, R,
                     stride);
  return dv_launch_status();
}
extern "C" int dv_bn_apply_multi(int32_t dtype, const dv_bn_item* items, int32_t n, int32_t total_blocks, void* stream) {
  if (!items || n <= 0 || total_blocks <= 0) return DV_EINVAL;
  DISPATCH_T(dtype, hipLaunchKernelGGL((bn_apply_multi_kernel<T>), dim3(total_blocks), dim3(kThreads), 0, ST(stream), items, n));
  return dv_launch_status();
}
extern "C" int dv_bn_bwd_reduce_multi(int32_t dtype, const dv_bn_item* items, int32_t n, int32_t total_blocks, void* stream) {
  if (!items || n <= 0 || total_blocks <= 0) return DV_EINVAL;
  DISPATCH_T(dtype, hipLaunchKernelGGL((bn_bwd_reduce_multi_kernel<T>), dim3(total_blocks), dim3(kThreads), 0, ST(stream), items, n));
  return dv_launch_status();
}
extern "C" int dv_bn_bwd_apply_multi(int32_t dtype, const dv_bn_item* items, int32_t n, int32_t total_blocks, int32_t max_c,
                                     void* stream) {
  if (!items || n <= 0 || total_blocks <= 0 || max_c <= 0) return DV_EINVAL;
  const int CP = cp8(max_c);
  if (5 * CP * 4 > 60 * 1024) return DV_EUNSUPPORTED;
  DISPATCH_T(dtype, hipLaunchKernelGGL((bn_bwd_apply_multi_kernel<T>), dim3(total_blocks), dim3(kThreads), 5 * CP * sizeof(float),
                                       ST(stream), items, n));
  return dv_launch_status();
}

extern "C" int dv_bn_finalize(const float* stats, int32_t R, int32_t stride, int32_t C, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                              float* scale, float* shift, void* stream) {
  if (!stats || R <= 0 || C <= 0 || stride < 2 * C + 1 || !gamma || !beta || !mean || !invstd || !scale || !shift) return DV_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return DV_EINVAL;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 127) / 128), dim3(128), 0, ST(stream), stats, R, stride, C, gamma, beta, eps,
                     momentum, running_mean, running_var, mean, invstd, scale, shift);
  return dv_launch_status();
}

extern "C" int dv_bn_apply(int32_t dtype, const void* x, int32_t ldx, const float* scale, const float* shift,
                           const void* residual, int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C, int32_t flags,
                           void* stream) {
  const int CP = cp8(C);
  if (!x || !y || !scale || !shift || M <= 0 || C <= 0 || ldx < CP || ldy < CP || (residual && ldr < CP)) return DV_EINVAL;
  if (!aligned16(x) || !aligned16(y) || (residual && !aligned16(residual))) return DV_EALIGN;
  if (!aligned16(scale) || !aligned16(shift)) return DV_EALIGN;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (ldx % V || ldy % V || (residual && ldr % V)) return DV_EALIGN;
    const int64_t total = M * (CP / V);
    if (total >= (1ll << 31)) return DV_EINVAL;
    hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream), (const T*)x,
                       ldx, scale, shift, (const T*)residual, ldr, (T*)y, ldy, (uint32_t)total, C,
                       make_fastdiv((uint32_t)(CP / V)), flags);
  });
  return dv_launch_status();
}

extern "C" int dv_bn_bwd_blocks(int64_t M, int32_t C) {
  (void)C;
  // Every workgroup ends with an LDS fold and 2*C atomics, so fewer, longer workgroups win as soon as there are enough of
  // them to cover the chip (measured in the S3D-G step: 100k-row layers 83 -> 43 us going from 1024 to 320 workgroups,
  // 12.5k-row layers 25 -> 18 us with 64 instead of 32 rows each); the >= 300k-row layers keep 1024.
  const int rpb = M <= 2048 ? 32 : 64;
  const int cap = M >= 300000 ? 1024 : 320;       // (2048 on the >= 1M-row layers: 105 -> 127 us, 208 -> 216 us)
  int64_t b = (M + rpb - 1) / rpb;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

extern "C" int dv_bn_bwd_reduce(int32_t dtype, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* x,
                                int32_t ldx, const float* mean, const float* invstd, int64_t M, int32_t C, int32_t flags,
                                float* sums, int32_t n_rep, float* ws, void* stream) {
  const int CP = cp8(C);
  const bool mask = !(flags & DV_NO_RELU_MASK);
  // DV_MASK_FROM_X needs the affine map (scale / shift) that only the multi-tensor item carries
  if (mask && (flags & DV_MASK_FROM_X)) return DV_EINVAL;
  if (!dy || !x || (mask && !y) || !mean || !invstd || !sums || M <= 0 || C <= 0 || n_rep <= 0) return DV_EINVAL;
  if (ws && (reinterpret_cast<uintptr_t>(ws) & 3)) return DV_EALIGN;
  if (lddy < CP || ldx < CP || (mask && ldy < CP)) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(x) || (mask && !aligned16(y)) || !aligned16(mean) || !aligned16(invstd)) return DV_EALIGN;
  const int blocks = dv_bn_bwd_blocks(M, C);
  const int64_t rpb = (M + blocks - 1) / blocks;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (lddy % V || ldx % V || (mask && ldy % V)) return DV_EALIGN;
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T>), dim3(blocks), dim3(kThreads), 0, ST(stream), (const T*)dy, lddy,
                       (const T*)y, ldy, (const T*)x, ldx, mean, invstd, M, C, CP, flags, rpb, sums, n_rep, ws);
  });
  return dv_launch_status();
}

extern "C" int64_t dv_bn_bwd_reduce_workspace(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0) return 0;
  return ordered_fold_floats(dv_bn_bwd_blocks(M, C), cp8(C)) * (int64_t)sizeof(float);
}

extern "C" int dv_bn_bwd_apply(int32_t dtype, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* x,
                               int32_t ldx, const float* mean, const float* invstd, const float* gamma,
                               const float* sums_global, int32_t rep_global, float inv_count, float dparam_scale,
                               float* dgamma, float* dbeta, void* dx, int32_t lddx, void* dres,
                               int32_t lddres, int64_t M, int32_t C, int32_t flags, void* stream) {
  const int CP = cp8(C);
  const bool mask = !(flags & DV_NO_RELU_MASK);
  if (mask && (flags & DV_MASK_FROM_X)) return DV_EINVAL;          // (as dv_bn_bwd_reduce: multi-tensor form only)
  if (!dy || !x || (mask && !y) || !mean || !invstd || !gamma || !sums_global || !dx || M <= 0 || C <= 0) return DV_EINVAL;
  if ((dgamma == nullptr) != (dbeta == nullptr) || rep_global <= 0) return DV_EINVAL;
  if (lddy < CP || ldx < CP || lddx < CP || (mask && ldy < CP) || (dres && lddres < CP)) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(x) || !aligned16(dx) || (mask && !aligned16(y)) || (dres && !aligned16(dres))) return DV_EALIGN;
  if (3 * CP * 4 > 60 * 1024) return DV_EUNSUPPORTED;
  DISPATCH_T(dtype, {
    constexpr int V = DT<T>::VEC;
    if (lddy % V || ldx % V || lddx % V || (mask && ldy % V) || (dres && lddres % V)) return DV_EALIGN;
    const int64_t total = M * (CP / V);
    if (total >= (1ll << 31)) return DV_EINVAL;
    int grid = grid_for(total, 2048);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(grid), dim3(kThreads), 3 * CP * sizeof(float), ST(stream),
                       (const T*)dy, lddy, (const T*)y, ldy, (const T*)x, ldx, mean, invstd, gamma, sums_global,
                       rep_global, inv_count, dparam_scale, dgamma, dbeta, (T*)dx, lddx, (T*)dres, lddres, (uint32_t)total, C, CP,
                       make_fastdiv((uint32_t)(CP / V)), flags);
  });
  return dv_launch_status();
}

static int gate_bwd_args(const float* g, const float* dmean, int32_t S, int32_t ldg, const int32_t* gate_off) {
  if (!g || !dmean || !gate_off || S <= 0 || ldg <= 0 || ldg % 8) return DV_EINVAL;
  if (!aligned16(g) || !aligned16(dmean)) return DV_EALIGN;
  return DV_OK;
}

extern "C" int dv_bn_bwd_reduce_multi_gated(int32_t dtype, const dv_bn_item* items, int32_t n, int32_t total_blocks, const float* g,
                                            const float* dmean, int32_t S, int32_t ldg, const int32_t* gate_off, void* stream) {
  if (!items || n <= 0 || total_blocks <= 0) return DV_EINVAL;
  if (int rc = gate_bwd_args(g, dmean, S, ldg, gate_off)) return rc;
  DISPATCH_T(dtype, hipLaunchKernelGGL((bn_bwd_reduce_multi_gated_kernel<T>), dim3(total_blocks), dim3(kThreads), 0, ST(stream), items,
                                       n, gate_off, g, dmean, make_fastdiv((uint32_t)S), ldg));
  return dv_launch_status();
}

extern "C" int dv_bn_bwd_apply_multi_gated(int32_t dtype, const dv_bn_item* items, int32_t n, int32_t total_blocks, int32_t max_c,
                                           const float* g, const float* dmean, int32_t S, int32_t ldg, const int32_t* gate_off,
                                           void* stream) {
  if (!items || n <= 0 || total_blocks <= 0 || max_c <= 0) return DV_EINVAL;
  if (int rc = gate_bwd_args(g, dmean, S, ldg, gate_off)) return rc;
  const int CP = cp8(max_c);
  if (5 * CP * 4 > 60 * 1024) return DV_EUNSUPPORTED;
  DISPATCH_T(dtype, hipLaunchKernelGGL((bn_bwd_apply_multi_gated_kernel<T>), dim3(total_blocks), dim3(kThreads),
                                       5 * CP * sizeof(float), ST(stream), items, n, gate_off, g, dmean, make_fastdiv((uint32_t)S),
                                       ldg));
  return dv_launch_status();
}
