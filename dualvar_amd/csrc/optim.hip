// Everything that steps a parameter arena on gfx950: SGD with momentum, Adam, LARS, the MoCo key EMA and the arena cast.
// The arithmetic (and, for LARS, the summation tree) is the contract of include/dualvar_hip.h; -ffp-contract=off: every
// operation below rounds once.  SGD, Adam and LARS share ONE walk over the arena (arena_walk) and differ only in their
// per-element update, so "a DECAY-only LARS segment has the bits of dv_sgd_momentum" is the same code, not two copies of it.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLarsThreads = 256;
constexpr int kLarsTrips = 16;
constexpr int kLarsTrip = kLarsThreads * 4;               // elements per trip of a block
constexpr int kLarsChunk = kLarsTrip * kLarsTrips;        // elements per block

__device__ __forceinline__ float lars_d(float p, float g, float gs, float wd, bool decay) {
  const float a1 = g * gs;
  return decay ? a1 + wd * p : a1;
}

// ------------------------------------------------------------------ the per-element updates
// An update has NS fp32 state arrays and maps (p, g, s[NS]) to the new p, writing the new state into s.
struct SgdUpdate {
  static constexpr int NS = 1;
  float lr, mu, wd, gs;
  __device__ __forceinline__ float operator()(float p, float g, float (&s)[1]) const {
    const float d = g * gs + wd * p;
    s[0] = mu * s[0] + d;
    return p - lr * s[0];
  }
};
// q is the trust ratio of the block's segment (1 without ADAPT), decay its DECAY flag
struct LarsUpdate {
  static constexpr int NS = 1;
  float lr, mu, wd, gs, q;
  bool decay;
  __device__ __forceinline__ float operator()(float p, float g, float (&s)[1]) const {
    const float t = q * lars_d(p, g, gs, wd, decay);
    s[0] = mu * s[0] + t;
    return p - lr * s[0];
  }
};
// Adam (torch.optim.Adam's single-tensor form, L2 weight decay coupled into the gradient): s = (exp_avg, exp_avg_sq).  sqrtf and
// `/` are hipcc's default correctly rounded pair.  step = lr / bc1 and sb2 = sqrt(bc2) are wave-uniform.
struct AdamUpdate {
  static constexpr int NS = 2;
  float b2, omb1, omb2, eps, wd, gs, step, sb2;
  __device__ __forceinline__ float operator()(float p, float g, float (&s)[2]) const {
    const float d = g * gs + wd * p;
    s[0] = s[0] + omb1 * (d - s[0]);
    s[1] = b2 * s[1] + (omb2 * d) * d;
    const float den = sqrtf(s[1]) / sb2 + eps;
    return p - step * (s[0] / den);
  }
};

// four consecutive elements of the compute copy; bf16 as one 8-byte store where the destination allows it (it does for every
// arena: offsets are multiples of 4 elements) -- the cast is the same round-to-nearest-even conversion either way
template <typename CT>
__device__ __forceinline__ void store_copy4(CT* dst, const f32x4& v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = (CT)v[e];
}
template <>
__device__ __forceinline__ void store_copy4<bf16_t>(bf16_t* dst, const f32x4& v) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  if ((reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
    const bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    *reinterpret_cast<bf16x4*>(dst) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = (bf16_t)v[e];
  }
}

// The walk: this thread's elements [i, i + 4) for i = i0, i0 + stride, ... below n of p, g (16-byte aligned) and the state
// arrays; whole vectors through 16-byte accesses, the last n % 4 elements one by one.  copy (may be null) takes the cast of
// every new p.  I is the index type of the launch shape: int64_t for a grid-stride over an arena, int inside a LARS chunk.
template <typename Upd, typename CT, typename I>
__device__ __forceinline__ void arena_walk(const Upd& upd, float* __restrict__ p, const float* __restrict__ g,
                                           float* const (&s)[Upd::NS], CT* __restrict__ copy, I i0, I stride, I n) {
  constexpr int NS = Upd::NS;
  for (I i = i0; i < n; i += stride) {
    if (i + 4 <= n) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), sv[NS];
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int k = 0; k < NS; ++k) sv[k] = *reinterpret_cast<f32x4*>(s[k] + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float se[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) se[k] = sv[k][e];
        pv[e] = upd(pv[e], gv[e], se);
#pragma unroll
        for (int k = 0; k < NS; ++k) sv[k][e] = se[k];
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
#pragma unroll
      for (int k = 0; k < NS; ++k) *reinterpret_cast<f32x4*>(s[k] + i) = sv[k];
      if (copy) store_copy4<CT>(copy + i, pv);
    } else {
      for (I j = i; j < n; ++j) {
        float se[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) se[k] = s[k][j];
        const float np = upd(p[j], g[j], se);
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k][j] = se[k];
        p[j] = np;
        if (copy) copy[j] = (CT)np;
      }
    }
  }
}
// the grid-stride launch shape of dv_sgd_momentum / dv_adam: grid_for((n + 3) / 4, 2048) blocks of kThreads
template <typename Upd, typename CT>
__device__ __forceinline__ void arena_walk_grid(const Upd& upd, float* p, const float* g, float* const (&s)[Upd::NS], CT* copy,
                                                int64_t n) {
  arena_walk(upd, p, g, s, copy, (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4, (int64_t)gridDim.x * blockDim.x * 4, n);
}

template <typename CT>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n,
                           float lr, float mu, float wd, float gs, CT* __restrict__ copy) {
  float* const s[1] = {buf};
  arena_walk_grid(SgdUpdate{lr, mu, wd, gs}, p, g, s, copy, n);
}
// p, g, m, v in, p, m, v and the compute copy out, in one pass
template <typename CT>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            int64_t n, float lr, float omb1, float b2, float omb2, float eps, float wd, float bc1, float bc2,
                            float gs, CT* __restrict__ copy) {
  float* const s[2] = {m, v};
  arena_walk_grid(AdamUpdate{b2, omb1, omb2, eps, wd, gs, lr / bc1, sqrtf(bc2)}, p, g, s, copy, n);
}
template <typename CT>
__global__ void ema_kernel(float* __restrict__ k, const float* __restrict__ q, int64_t n, float m, CT* __restrict__ copy) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = k[i] * m + q[i] * (1.f - m);
    k[i] = v;
    if (copy) copy[i] = (CT)v;
  }
}
template <typename CT>
__global__ void cast_kernel(const float* __restrict__ s, CT* __restrict__ d, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (CT)s[i];
}

// ------------------------------------------------------------------ LARS: two launches per store and step, no tickets, no host round trip
// the block's place in the table: its segment, and [c0, c0 + m) of that segment
struct LarsBlock {
  dv_lars_seg s;
  int64_t base;     // s.off + c0
  int m;            // elements of this chunk (0 for a block the table should not have)
};
__device__ __forceinline__ LarsBlock lars_block(const dv_lars_seg* __restrict__ segs, const int32_t* __restrict__ block_seg) {
  LarsBlock b;
  b.s = segs[block_seg[blockIdx.x]];
  const int64_t c0 = (int64_t)((int)blockIdx.x - b.s.first_block) * kLarsChunk;
  const int64_t rem = c0 >= 0 ? b.s.n - c0 : 0;
  b.m = rem <= 0 ? 0 : rem < kLarsChunk ? (int)rem : kLarsChunk;
  b.base = b.s.off + c0;
  return b;
}

__global__ __launch_bounds__(kLarsThreads) void lars_partial_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                    const dv_lars_seg* __restrict__ segs,
                                                                    const int32_t* __restrict__ block_seg, float wd, float gs,
                                                                    float* __restrict__ partials) {
  const LarsBlock b = lars_block(segs, block_seg);
  if (!(b.s.flags & DV_LARS_ADAPT)) return;               // q = 1: the step never reads this block's pair
  const bool decay = (b.s.flags & DV_LARS_DECAY) != 0;
  const float* pp = p + b.base;
  const float* gg = g + b.base;
  float sp = 0.f, sd = 0.f;
  for (int k = 0; k < kLarsTrips && k * kLarsTrip < b.m; ++k) {
    const int i = k * kLarsTrip + (int)threadIdx.x * 4;
    if (i + 4 <= b.m) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pp + i), gv = *reinterpret_cast<const f32x4*>(gg + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = lars_d(pv[e], gv[e], gs, wd, decay);
        sp += pv[e] * pv[e];
        sd += d * d;
      }
    } else {
      for (int j = i; j < b.m; ++j) {
        const float d = lars_d(pp[j], gg[j], gs, wd, decay);
        sp += pp[j] * pp[j];
        sd += d * d;
      }
    }
  }
  __shared__ float sh[2][kLarsThreads / DV_WAVE];
  sp = wave_sum(sp);
  sd = wave_sum(sd);
  if ((threadIdx.x & (DV_WAVE - 1)) == 0) {
    sh[0][threadIdx.x / DV_WAVE] = sp;
    sh[1][threadIdx.x / DV_WAVE] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = sh[0][0], c = sh[1][0];
    for (int w = 1; w < kLarsThreads / DV_WAVE; ++w) { a += sh[0][w]; c += sh[1][w]; }
    partials[2 * (size_t)blockIdx.x] = a;
    partials[2 * (size_t)blockIdx.x + 1] = c;
  }
}

template <typename CT>
__global__ __launch_bounds__(kLarsThreads) void lars_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ buf, const dv_lars_seg* __restrict__ segs,
                                                                 const int32_t* __restrict__ block_seg, float lr, float mu, float wd,
                                                                 float eta, float gs, const float* __restrict__ partials,
                                                                 CT* __restrict__ copy, float* __restrict__ q_out) {
  const LarsBlock b = lars_block(segs, block_seg);
  float q = 1.f;
  if (b.s.flags & DV_LARS_ADAPT) {
    // the segment's partials, folded in double in index order: the same few hundred pairs at most in every block of the
    // segment (block-uniform addresses, hot in L2), so every block forms the same q
    double Sp = 0.0, Sd = 0.0;
    const float* pr = partials + 2 * (size_t)b.s.first_block;
    for (int i = 0; i < b.s.n_blocks; ++i) {
      Sp += (double)pr[2 * i];
      Sd += (double)pr[2 * i + 1];
    }
    if (Sp > 0.0 && Sd > 0.0) q = (float)((double)eta * sqrt(Sp) / sqrt(Sd));
  }
  if (q_out && (int)blockIdx.x == b.s.first_block && threadIdx.x == 0) q_out[block_seg[blockIdx.x]] = q;
  float* const s[1] = {buf + b.base};
  arena_walk(LarsUpdate{lr, mu, wd, gs, q, (b.s.flags & DV_LARS_DECAY) != 0}, p + b.base, g + b.base, s,
             copy ? copy + b.base : (CT*)nullptr, (int)threadIdx.x * 4, kLarsTrip, b.m);
}

}  // namespace

// The compute copy of an entry: a bf16 copy instantiates the kernel with bf16_t, everything else with float, and that
// copy pointer is null unless the dtype is DV_F32.  LAUNCH names the kernel as K<CT> and the copy as (CT*)cp.
#define LAUNCH_COPY(copy_dtype, p_copy, LAUNCH)                                                                       \
  do {                                                                                                                \
    if ((p_copy) && (copy_dtype) == DV_BF16) { typedef bf16_t CT; void* const cp = (p_copy); LAUNCH; }                \
    else { typedef float CT; void* const cp = (copy_dtype) == DV_F32 ? (p_copy) : nullptr; LAUNCH; }                  \
  } while (0)

extern "C" int dv_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float mu, float wd, float gs,
                               int32_t copy_dtype, void* p_copy, void* stream) {
  if (!p || !g || !buf || n <= 0) return DV_EINVAL;
  if (!aligned16(p) || !aligned16(g) || !aligned16(buf)) return DV_EALIGN;
  LAUNCH_COPY(copy_dtype, p_copy, hipLaunchKernelGGL((sgd_kernel<CT>), dim3(grid_for((n + 3) / 4, 2048)), dim3(kThreads), 0,
                                                     ST(stream), p, g, buf, n, lr, mu, wd, gs, (CT*)cp));
  return dv_launch_status();
}
extern "C" int dv_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float omb1, float b2, float omb2, float eps,
                       float wd, float bc1, float bc2, float gs, int32_t copy_dtype, void* p_copy, void* stream) {
  if (!p || !g || !m || !v || n <= 0) return DV_EINVAL;
  // eps > 0: arena padding has g = v = 0 and must stay 0, not become 0 / 0
  if (!(eps > 0.f) || !(bc1 > 0.f) || !(bc2 > 0.f) || !(omb1 > 0.f && omb1 <= 1.f) || !(b2 >= 0.f && b2 < 1.f) ||
      !(omb2 > 0.f && omb2 <= 1.f)) return DV_EINVAL;
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return DV_EALIGN;
  LAUNCH_COPY(copy_dtype, p_copy, hipLaunchKernelGGL((adam_kernel<CT>), dim3(grid_for((n + 3) / 4, 2048)), dim3(kThreads), 0,
                                                     ST(stream), p, g, m, v, n, lr, omb1, b2, omb2, eps, wd, bc1, bc2, gs, (CT*)cp));
  return dv_launch_status();
}
extern "C" int dv_ema(float* k, const float* q, int64_t n, float m, int32_t copy_dtype, void* k_copy, void* stream) {
  if (!k || !q || n <= 0) return DV_EINVAL;
  LAUNCH_COPY(copy_dtype, k_copy, hipLaunchKernelGGL((ema_kernel<CT>), dim3(grid_for(n, 2048)), dim3(kThreads), 0, ST(stream), k, q,
                                                     n, m, (CT*)cp));
  return dv_launch_status();
}
extern "C" int dv_cast_arena(int32_t dtype, const float* src, void* dst, int64_t n, void* stream) {
  if (!src || !dst || n <= 0) return DV_EINVAL;
  if (dtype == DV_BF16) hipLaunchKernelGGL((cast_kernel<bf16_t>), dim3(grid_for(n, 2048)), dim3(kThreads), 0, ST(stream), src, (bf16_t*)dst, n);
  else if (dtype == DV_F32) hipLaunchKernelGGL((cast_kernel<float>), dim3(grid_for(n, 2048)), dim3(kThreads), 0, ST(stream), src, (float*)dst, n);
  else return DV_EUNSUPPORTED;
  return dv_launch_status();
}

extern "C" int dv_lars_chunk(void) { return kLarsChunk; }

extern "C" int dv_lars_norms(const float* p, const float* g, const dv_lars_seg* segs, const int32_t* block_seg, int32_t n_segs,
                             int32_t total_blocks, float wd, float gs, float* partials, void* stream) {
  if (!p || !g || !segs || !block_seg || !partials || n_segs <= 0 || total_blocks <= 0) return DV_EINVAL;
  if (!aligned16(p) || !aligned16(g)) return DV_EALIGN;
  hipLaunchKernelGGL(lars_partial_kernel, dim3(total_blocks), dim3(kLarsThreads), 0, ST(stream), p, g, segs, block_seg, wd, gs,
                     partials);
  return dv_launch_status();
}

extern "C" int dv_lars_step(float* p, const float* g, float* buf, const dv_lars_seg* segs, const int32_t* block_seg, int32_t n_segs,
                            int32_t total_blocks, float lr, float mu, float wd, float eta, float gs, const float* partials,
                            int32_t copy_dtype, void* p_copy, float* q_out, void* stream) {
  if (!p || !g || !buf || !segs || !block_seg || !partials || n_segs <= 0 || total_blocks <= 0) return DV_EINVAL;
  if (!aligned16(p) || !aligned16(g) || !aligned16(buf)) return DV_EALIGN;
  LAUNCH_COPY(copy_dtype, p_copy, hipLaunchKernelGGL((lars_step_kernel<CT>), dim3(total_blocks), dim3(kLarsThreads), 0, ST(stream),
                                                     p, g, buf, segs, block_seg, lr, mu, wd, eta, gs, partials, (CT*)cp, q_out));
  return dv_launch_status();
}
