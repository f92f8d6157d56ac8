// LARS over the tensors of a parameter arena on gfx950: two launches per store and step, no tickets, no host round trip.
// The arithmetic and the summation tree are the contract of include/dualvar_hip.h (dv_lars_norms / dv_lars_step);
// -ffp-contract=off: every operation below rounds once, exactly as sgd_kernel (csrc/elementwise.hip) does.
#include "common.hpp"

namespace {

constexpr int kLarsThreads = 256;
constexpr int kLarsTrips = 16;
constexpr int kLarsTrip = kLarsThreads * 4;               // elements per trip of a block
constexpr int kLarsChunk = kLarsTrip * kLarsTrips;        // elements per block

__device__ __forceinline__ float lars_d(float p, float g, float gs, float wd, bool decay) {
  const float a1 = g * gs;
  return decay ? a1 + wd * p : a1;
}

// four consecutive elements of the compute copy; bf16 as one 8-byte store where the destination allows it (it does for every
// arena: offsets are multiples of 4 elements) -- the cast is the same round-to-nearest-even conversion either way
template <typename CT>
__device__ __forceinline__ void lars_store_copy4(CT* dst, const f32x4& v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = (CT)v[e];
}
template <>
__device__ __forceinline__ void lars_store_copy4<bf16_t>(bf16_t* dst, const f32x4& v) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  if ((reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
    const bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    *reinterpret_cast<bf16x4*>(dst) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = (bf16_t)v[e];
  }
}

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
  const bool decay = (b.s.flags & DV_LARS_DECAY) != 0;
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
  float* pp = p + b.base;
  const float* gg = g + b.base;
  float* bb = buf + b.base;
  CT* cc = copy ? copy + b.base : nullptr;
  for (int k = 0; k < kLarsTrips && k * kLarsTrip < b.m; ++k) {
    const int i = k * kLarsTrip + (int)threadIdx.x * 4;
    if (i + 4 <= b.m) {
      f32x4 pv = *reinterpret_cast<f32x4*>(pp + i), bv = *reinterpret_cast<f32x4*>(bb + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gg + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = q * lars_d(pv[e], gv[e], gs, wd, decay);
        bv[e] = mu * bv[e] + t;
        pv[e] = pv[e] - lr * bv[e];
      }
      *reinterpret_cast<f32x4*>(pp + i) = pv;
      *reinterpret_cast<f32x4*>(bb + i) = bv;
      if (cc) lars_store_copy4<CT>(cc + i, pv);
    } else {
      for (int j = i; j < b.m; ++j) {
        const float t = q * lars_d(pp[j], gg[j], gs, wd, decay);
        const float nb = mu * bb[j] + t;
        const float np = pp[j] - lr * nb;
        bb[j] = nb;
        pp[j] = np;
        if (cc) cc[j] = (CT)np;
      }
    }
  }
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

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
  if (p_copy && copy_dtype == DV_BF16)
    hipLaunchKernelGGL((lars_step_kernel<bf16_t>), dim3(total_blocks), dim3(kLarsThreads), 0, ST(stream), p, g, buf, segs, block_seg,
                       lr, mu, wd, eta, gs, partials, (bf16_t*)p_copy, q_out);
  else
    hipLaunchKernelGGL((lars_step_kernel<float>), dim3(total_blocks), dim3(kLarsThreads), 0, ST(stream), p, g, buf, segs, block_seg,
                       lr, mu, wd, eta, gs, partials, (float*)(copy_dtype == DV_F32 ? p_copy : nullptr), q_out);
  return dv_launch_status();
}
