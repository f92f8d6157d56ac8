// What two or more of the streaming (HBM-bound) files batchnorm.hip, pool.hip, gate.hip and elementwise.hip use: NDHWC, 16-byte
// vector accesses along the channel axis, fp32 math, wavefront(64)-shuffle + LDS reductions.  Everything here has internal
// linkage (each kernel template is instantiated by exactly one of those files).
#pragma once
#include "common.hpp"
#include "ordered_fold.hpp"

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------ block reduce helper
__device__ __forceinline__ float block_sum(float v, float* sh /*>= blockDim/64 floats*/) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
  return r;
}

// V per-channel parameters from c0 on, as 16-byte vector loads (the per-channel arrays are padded to a multiple of 8 floats)
template <int V>
__device__ __forceinline__ void load_params(const float* __restrict__ p, int c0, float (&v)[V]) {
#pragma unroll
  for (int q = 0; q < V / 4; ++q) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p + c0 + 4 * q);
    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
  }
}

// The BatchNorm's affine map, ONE expression for bn_apply, the DV_MASK_FROM_X sites and the gate-on-load kernels: whoever
// rebuilds an activation (or its sign) from x gets the bits the forward stored.  (The library is built with -ffp-contract=off:
// a product and a sum, two roundings, wherever this is inlined.)
__device__ __forceinline__ float bn_affine(float x, float sc, float sh) { return x * sc + sh; }
// a value as it comes back from a tensor of type T it was stored to (bf16: rounded; fp32: itself)
template <typename T>
__device__ __forceinline__ float as_stored(float v) { return DT<T>::to_f(DT<T>::from_f(v)); }
// relu(bn(x)) as bn_apply (DV_RELU, no residual) leaves it in memory
template <typename T>
__device__ __forceinline__ float bn_relu_stored(float x, float sc, float sh) { return as_stored<T>(fmaxf(bn_affine(x, sc, sh), 0.f)); }
// the gradient behind a self-gating scale, dy*g + dmean/S, as rowscale_kernel<T, 1> forms it (and, as_stored, leaves it)
__device__ __forceinline__ float gate_grad(float dy, float g, float dm, float invS) { return dy * g + dm * invS; }

// ------------------------------------------------------------------ column reductions over rows
// Generic: rows [r_begin, r_end) of a [rows][ld] matrix, lanes along channel vectors.  F maps
// (row, c0) -> V values for NS sums.  Result: out[s][c] for this block (written by the caller's lambda).
struct NoPre { __device__ __forceinline__ void operator()(int) const {} };

template <int V, int NS, int UNROLL = 0, typename F, typename W, typename Pre = NoPre>
__device__ __forceinline__ void column_reduce(int64_t r_begin, int64_t r_end, int CP, F f, W write, Pre pre = Pre()) {
  __shared__ float lds[kThreads * V * NS > 4096 ? 4096 : kThreads * V * NS];
  const int CV = CP / V;
  for (int cvb = 0; cvb < CV; cvb += kThreads) {
    const int cvc = min(kThreads, CV - cvb);
    int rg = kThreads / cvc;                       // row groups
    // LDS budget: rg * cvc * V * NS floats <= 4096
    while (rg > 1 && rg * cvc * V * NS > 4096) rg >>= 1;
    const int t = threadIdx.x;
    const int my_cv = t % cvc, my_rg = t / cvc;
    float acc[NS][V];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[s][e] = 0.f;
    if (my_rg < rg) {
      pre((cvb + my_cv) * V);                       // per-thread constants of this channel vector
      // four rows in flight for 4-element (fp32) vectors, two for 8-element (bf16) ones: the same 16 values per sum and thread.
      // (unroll 4 for bf16 needed > 128 VGPRs: with the 1 024-thread default bound the reduce kernels spilled 112 B per lane and
      // their traffic went 1.08x -> 1.55x algorithmic -- round 3's bf16 regression; tests/test_abi_and_host.py now fails on
      // any kernel with scratch.)
#pragma unroll(UNROLL ? UNROLL : V == 4 ? 4 : 2)
      for (int64_t r = r_begin + my_rg; r < r_end; r += rg) f(r, (cvb + my_cv) * V, acc);
    }
    __syncthreads();
    if (rg == 1 && cvc * V * NS > 4096) {
      // too wide for LDS staging (cannot happen for CP <= 4096/NS); write directly
      if (my_rg < rg) write((cvb + my_cv) * V, acc);
    } else {
      if (my_rg < rg) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int e = 0; e < V; ++e) lds[((my_rg * NS + s) * cvc + my_cv) * V + e] = acc[s][e];
      }
      __syncthreads();
      // fold the row groups pairwise with every thread (a serial fold by the first cvc threads costs ~10 us
      // when the tensor has few channels and therefore up to 128 row groups)
      for (int n = rg; n > 1;) {
        const int half = (n + 1) >> 1;
        if (my_rg < rg && my_rg + half < n) {
#pragma unroll
          for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int e = 0; e < V; ++e)
              lds[((my_rg * NS + s) * cvc + my_cv) * V + e] += lds[(((my_rg + half) * NS + s) * cvc + my_cv) * V + e];
        }
        __syncthreads();
        n = half;
      }
      if (t < cvc) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int e = 0; e < V; ++e) acc[s][e] = lds[(s * cvc + t) * V + e];
        write((cvb + t) * V, acc);
      }
    }
    __syncthreads();
  }
}

// Tail of an ordered reduction over the nblk blocks of one item, each of which has stored NO = 2*CP partial sums to
// ws[bid][NO] (coherent_store).  Two levels, so that no single block has to walk hundreds of partial rows: the block that
// takes the last ticket of its group of kFoldGroup blocks adds the group's rows in block order into a group row; the block
// that takes the last group ticket adds the group rows in group order and WRITES out[NO].  The hand-off (rows -> ticket ->
// reader) is the sc1 / s_waitcnt protocol of ordered_fold.hpp, not agent-scope fences.  Layout of ws: [nblk][NO] rows,
// [ngrp][NO] group rows, [ngrp + 1] ticket words (zero on entry, zero again on exit).
static inline int64_t ordered_fold_floats(int nblk, int CP) { return fold_rows_total(nblk) * 2 * CP + fold_ticket_words(nblk); }

__device__ __forceinline__ void fold_rows(const float* __restrict__ rows, int n, int NO, int C, int CP, float* __restrict__ dst,
                                          bool coherent_dst) {
  for (int i = threadIdx.x; i < NO; i += blockDim.x) {
    const int c = i < CP ? i : i - CP;
    const float t = c < C ? fold_in_order<32>(rows + i, n, NO) : 0.f;
    if (coherent_dst) coherent_store(dst + i, t);
    else dst[i] = t;
  }
}
__device__ __forceinline__ void ordered_fold(float* __restrict__ ws, uint32_t bid, uint32_t nblk, int C, int CP, float* __restrict__ out) {
  __shared__ uint32_t last;
  const int NO = 2 * CP;
  constexpr uint32_t gfold = kFoldGroup;
  const uint32_t ngrp = fold_groups((int)nblk), grp = bid / gfold;
  const uint32_t gsize = min(gfold, nblk - grp * gfold);
  float* grows = ws + (size_t)nblk * NO;
  uint32_t* tick = reinterpret_cast<uint32_t*>(grows + (size_t)ngrp * NO);
  if (!took_last_ticket(tick + grp, gsize, &last)) return;
  if (ngrp == 1) {                                   // one group: its last block writes the result (0 + the group row: same bits)
    fold_rows(ws, (int)gsize, NO, C, CP, out, false);
    clear_ticket(tick);
    return;
  }
  fold_rows(ws + (size_t)grp * gfold * NO, (int)gsize, NO, C, CP, grows + (size_t)grp * NO, true);
  clear_ticket(tick + grp);
  if (!took_last_ticket(tick + ngrp, ngrp, &last)) return;
  fold_rows(grows, (int)ngrp, NO, C, CP, out, false);
  clear_ticket(tick + ngrp);
}

// ------------------------------------------------------------------ BN backward: one body per pass over a dL/dy source
// Where a BatchNorm-backward pass takes dL/dy from (PlainDy, GatedDy: batchnorm.hip; PooledDy: pool.hip).  load() issues the source's loads for the V channels at (row r, c0): g
// itself, or what finish() forms it from in registers once the body has issued its own loads of y / x.  kRows: the rows
// column_reduce keeps in flight (0: its default).  kPooled: see PooledDy.
template <typename T, typename Src>
__device__ __forceinline__ void bn_bwd_reduce_body(const Src& src, const T* __restrict__ y, int ldy,
                                                   const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                   const float* __restrict__ invstd, int64_t M, int C, int CP, int flags,
                                                   int64_t rows_per_block, float* __restrict__ sums_all, int n_rep,
                                                   uint32_t bid, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, float* __restrict__ ws, uint32_t nblk) {
  constexpr int V = DT<T>::VEC;
  if (Src::kPooled) { flags = DV_MASK_FROM_X; ws = nullptr; }
  // Ordered mode (ws != nullptr): the block stores its partial sums to ws[bid][2][CP] (sc1 stores); the block that takes the
  // last ticket (ordered_fold: drained stores -> ticket -> sc1 loads) adds the partials in block order into sums_all[0] -- no
  // float atomics, so the sums do not depend on the order blocks finish in.  Legacy mode: atomics, spread over n_rep replicas because atomics on one
  // address serialise at the memory side (~12 ns each).
  float* sums = ws ? ws + (size_t)bid * 2 * CP : sums_all + (size_t)(bid % n_rep) * 2 * CP;
  const int64_t r0 = (int64_t)bid * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  const bool mask = !(flags & DV_NO_RELU_MASK);
  // DV_MASK_FROM_X: the ReLU mask is recomputed from x exactly as the forward computed y = relu(x*scale + shift)
  // (same expression, same rounding), so the output tensor is not read at all: 2 tensor reads instead of 3
  const bool fromx = mask && (flags & DV_MASK_FROM_X);
  float mu[V], is[V], sc[V], sh[V];
  column_reduce<V, 2, Src::kRows>(
      r0, r1, CP,
      [&](int64_t r, int c0, float(&acc)[2][V]) {
        float g[V], yy[V], xx[V];
        typename Src::Pend pend;
        src.load(r, c0, g, pend);
        if (mask && !fromx) Pack16<T>::load(y + r * ldy + c0, yy);
        Pack16<T>::load(x + r * ldx + c0, xx);
        src.finish(r, c0, g, pend);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float act = fromx ? bn_affine(xx[e], sc[e], sh[e]) : yy[e];
          float gg = (mask && !(act > 0.f)) ? 0.f : g[e];
          acc[0][e] += gg;
          acc[1][e] += gg * (xx[e] - mu[e]) * is[e];
        }
      },
      [&](int c0, float(&acc)[2][V]) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (c0 + e < C) {
            if (ws) { coherent_store(sums + c0 + e, acc[0][e]); coherent_store(sums + CP + c0 + e, acc[1][e]); }
            else { atomicAdd(sums + c0 + e, acc[0][e]); atomicAdd(sums + CP + c0 + e, acc[1][e]); }
          }
      },
      [&](int c0) {
        load_params<V>(mean, c0, mu);
        load_params<V>(invstd, c0, is);
        if (fromx) { load_params<V>(scale, c0, sc); load_params<V>(shift, c0, sh); }
      });
  if (ws) ordered_fold(ws, bid, nblk, C, CP, sums_all);
}

// dx = k1[c]*g + k2[c]*x + k3[c] with  k1 = gamma*invstd, k2 = -k1*invstd*sgx/M, k3 = -k1*sg/M - k2*mean
// (sg, sgx = global sums of g and g*xhat).  The table is built once per block in LDS.
template <typename T, typename Src>
__device__ __forceinline__ void bn_bwd_apply_body(const Src& src, const T* __restrict__ y, int ldy,
                                                  const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ sums_g, int rep_g, float inv_count,
                                                  float dscale, float* dgamma, float* dbeta, T* __restrict__ dx,
                                                  int lddx, T* __restrict__ dres, int lddres, uint32_t total, int C,
                                                  int CP, const FastDiv& fcv, int flags, uint32_t bid, uint32_t nblk,
                                                  const float* __restrict__ scale, const float* __restrict__ shift) {
  constexpr int V = DT<T>::VEC;
  if (Src::kPooled) { flags = DV_MASK_FROM_X; dres = nullptr; }
  extern __shared__ __attribute__((aligned(16))) float coef[];      // [3][CP] (+ [2][CP] scale, shift with DV_MASK_FROM_X)
  const bool fromx = !(flags & DV_NO_RELU_MASK) && (flags & DV_MASK_FROM_X);
  if (bid == 0 && dgamma) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float sb = 0.f, sg = 0.f;
      for (int r = 0; r < rep_g; ++r) { sb += sums_g[(size_t)r * 2 * CP + c]; sg += sums_g[(size_t)r * 2 * CP + CP + c]; }
      dbeta[c] += dscale * sb;
      dgamma[c] += dscale * sg;
    }
  }
  for (int c = threadIdx.x; c < CP; c += blockDim.x) {
    float k1 = 0.f, k2 = 0.f, k3 = 0.f;
    if (c < C) {
      float sg = 0.f, sgx = 0.f;
      for (int r = 0; r < rep_g; ++r) { sg += sums_g[(size_t)r * 2 * CP + c]; sgx += sums_g[(size_t)r * 2 * CP + CP + c]; }
      k1 = gamma[c] * invstd[c];
      k2 = -k1 * invstd[c] * sgx * inv_count;
      k3 = -k1 * sg * inv_count - k2 * mean[c];
    }
    coef[c] = k1; coef[CP + c] = k2; coef[2 * CP + c] = k3;
    if (fromx) { coef[3 * CP + c] = c < C ? scale[c] : 0.f; coef[4 * CP + c] = c < C ? shift[c] : 0.f; }
  }
  __syncthreads();
  const uint32_t CV = fcv.d;
  const bool mask = !(flags & DV_NO_RELU_MASK);
  for (uint32_t i = bid * blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
    const uint32_t row = fd_div(i, fcv);
    const int c0 = (int)(i - row * CV) * V;
    float g[V], yy[V], xx[V], o[V], ro[V], k1[V], k2[V], k3[V], sc[V], sh[V];
    typename Src::Pend pend;
    src.load(row, c0, g, pend);
    if (mask && !fromx) Pack16<T>::load(y + (size_t)row * ldy + c0, yy);
    Pack16<T>::load(x + (size_t)row * ldx + c0, xx);
    if (dres && (flags & DV_ACCUM)) Pack16<T>::load(dres + (size_t)row * lddres + c0, ro);
    src.finish(row, c0, g, pend);                         // (as in bn_bwd_reduce_body: the same dL/dy in both passes)
    load_params<V>(coef, c0, k1);
    load_params<V>(coef + CP, c0, k2);
    load_params<V>(coef + 2 * CP, c0, k3);
    if (fromx) { load_params<V>(coef + 3 * CP, c0, sc); load_params<V>(coef + 4 * CP, c0, sh); }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float act = fromx ? bn_affine(xx[e], sc[e], sh[e]) : yy[e];     // the forward's expression: same mask bit for bit
      const float gg = (mask && !(act > 0.f)) ? 0.f : g[e];
      o[e] = k1[e] * gg + k2[e] * xx[e] + k3[e];
      // (pad lanes [C, CP) of dres are written as zeros, whatever dy / y / dres held there, as dx's are through k1..k3 = 0)
      if (dres) ro[e] = c0 + e >= C ? 0.f : (flags & DV_ACCUM) ? ro[e] + gg : gg;
    }
    Pack16<T>::store(dx + (size_t)row * lddx + c0, o);
    if (dres) Pack16<T>::store(dres + (size_t)row * lddres + c0, ro);
  }
}

}  // namespace

#define DISPATCH_T(dtype, ...)                                  \
  do {                                                          \
    if ((dtype) == DV_F32) { typedef float T; __VA_ARGS__; }    \
    else if ((dtype) == DV_BF16) { typedef bf16_t T; __VA_ARGS__; } \
    else return DV_EUNSUPPORTED;                                \
  } while (0)

static inline int cp8(int c) { return (c + 7) & ~7; }
