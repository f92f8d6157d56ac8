// Nearest-neighbour selection and the weighted k-NN vote (include/dualvar_select.h: dv_topk_merge_f32, dv_knn_vote).
//
// Both kernels give one row to one wavefront (a workgroup of 64 threads), so a call with few rows uses little of the GPU:
// accepted for an evaluation path ("Weighted k-NN evaluation").
#include "common.hpp"
#include "../../include/dualvar_select.h"

// The total order "larger value first, then smaller index" as ONE unsigned comparison: the value's bits made monotone
// (negative: all bits flipped, else the sign bit set) in the high word, ~index in the low word.  v + 0.0f folds -0 into +0.
// A real candidate (value > -inf) has a high word above 0x007fffff, so key 0 is free to mean "empty slot" and sorts last.
__device__ __forceinline__ unsigned long long topk_key(float v, int idx) {
  const uint32_t b = __float_as_uint(v + 0.0f);
  const uint32_t o = b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
  return ((unsigned long long)o << 32) | (uint32_t)~(uint32_t)idx;
}
__device__ __forceinline__ bool topk_selectable(float v) { return v > -INFINITY; }      // false for NaN and -inf

// Bitonic sort of keys[0..P) into DESCENDING order by the 64 threads of the workgroup; P a power of two >= 128.
__device__ __forceinline__ void bitonic_desc(unsigned long long* keys, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = lane; t < (P >> 1); t += 64) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));     // t with a 0 inserted at the stride bit
        const int hi = lo | stride;
        const unsigned long long a = keys[lo], b = keys[hi];
        const bool desc = (lo & size) == 0;
        if ((a < b) == desc) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
    }
  }
  __syncthreads();
}

// keys[0..k): the row's current selection, sorted, empty slots 0.  keys[k..P): survivors of the threshold tau = keys[k-1]
// that wait for the next sort.  P = 2 * pow2ceil(max(k, 64)), so the buffer holds at least 64 and at most 512 keys are sorted.
__global__ void __launch_bounds__(64) topk_merge_kernel(const float* __restrict__ sim, int ld, int n_cols, int col0, int k, int P,
                                                        float* __restrict__ top_val, int* __restrict__ top_idx, int ldk, int first) {
  __shared__ unsigned long long keys[2 * DV_TOPK_MAX_K];
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* row = sim + (size_t)r * ld;
  float* tv = top_val + (size_t)r * ldk;
  int* ti = top_idx + (size_t)r * ldk;
  for (int i = lane; i < P; i += 64) {
    unsigned long long key = 0;
    if (!first && i < k) {
      const float v = tv[i];
      const int idx = ti[i];
      if (idx >= 0 && topk_selectable(v)) key = topk_key(v, idx);
    }
    keys[i] = key;
  }
  __syncthreads();
  const int cap = P - k;                 // >= 64
  int fill = 0;                          // uniform over the wavefront
  unsigned long long tau = keys[k - 1];  // 0 while fewer than k are held: every real key is above it
  const unsigned long long below = (1ull << lane) - 1;

  for (int base = 0; base < n_cols; base += 256) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {        // four coalesced loads in flight
      const int j = base + u * 64 + lane;
      v[u] = j < n_cols ? row[j] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + u * 64 + lane;
      const unsigned long long key = topk_selectable(v[u]) ? topk_key(v[u], col0 + j) : 0ull;
      const bool pass = key > tau;
      const unsigned long long mask = __ballot(pass);
      if (mask == 0) continue;
      if (pass) keys[k + fill + __popcll(mask & below)] = key;
      fill += __popcll(mask);
      if (fill > cap - 64) {             // the buffer cannot take another 64: sort, keep k, refresh the threshold
        for (int i = k + fill + lane; i < P; i += 64) keys[i] = 0;
        bitonic_desc(keys, P, lane);
        tau = keys[k - 1];
        fill = 0;                        // the buffer lies above keys[k-1]: refilling it needs no further barrier
      }
    }
  }
  if (fill > 0) {
    for (int i = k + fill + lane; i < P; i += 64) keys[i] = 0;
    bitonic_desc(keys, P, lane);
  }
  for (int i = lane; i < k; i += 64) {
    const unsigned long long key = keys[i];
    const uint32_t o = (uint32_t)(key >> 32);
    const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
    tv[i] = key ? __uint_as_float(b) : -INFINITY;
    ti[i] = key ? (int)~(uint32_t)key : -1;
  }
}

extern "C" int dv_topk_merge_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0, int32_t k,
                                 float* top_val, int32_t* top_idx, int32_t ldk, int32_t first, void* stream) {
  // n_cols <= 2^31 - 513: the kernel's `base += 256` and `base + u * 64 + lane` stay inside int32
  if (!sim || !top_val || !top_idx || R <= 0 || n_cols <= 0 || n_cols > 0x7fffffff - 512 || ld < n_cols || k < 1 ||
      k > DV_TOPK_MAX_K || ldk < k || col0 < 0 || (int64_t)col0 + n_cols > 0x7fffffffLL)
    return DV_EINVAL;
  int P = 128;
  while (P < 2 * k) P <<= 1;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(R), dim3(64), 0, ST(stream), sim, ld, n_cols, col0, k, P, top_val, top_idx, ldk,
                     first);
  return dv_launch_status();
}

// Weighted vote: the row's k labels and weights are staged in LDS; every lane sums the total in ascending i, lane c (strided
// over the classes) sums its class in ascending i, and (score, lowest c) is folded over the wavefront.  No atomics.
__global__ void __launch_bounds__(64) knn_vote_kernel(const float* __restrict__ top_val, const int* __restrict__ top_idx, int ldk,
                                                      int k, const int* __restrict__ bank_labels, int n_bank, int n_class,
                                                      float inv_T, float* __restrict__ score, int lds, int* __restrict__ pred) {
  __shared__ int lab[DV_TOPK_MAX_K];
  __shared__ float wgt[DV_TOPK_MAX_K];
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* tv = top_val + (size_t)r * ldk;
  const int* ti = top_idx + (size_t)r * ldk;
  const float v0 = tv[0];
  for (int i = lane; i < k; i += 64) {
    const int idx = ti[i];
    int y = -1;
    if (idx >= 0 && idx < n_bank) {
      y = bank_labels[idx];
      if (y < 0 || y >= n_class) y = -1;
    }
    lab[i] = y;
    wgt[i] = inv_T == 0.f ? 1.f : expf((tv[i] - v0) * inv_T);
  }
  __syncthreads();
  float total = 0.f;
  int n_valid = 0;
  for (int i = 0; i < k; ++i)
    if (lab[i] >= 0) {
      total += wgt[i];
      ++n_valid;
    }
  float best = -1.f;
  int best_c = -1;
  // a total of 0, inf or NaN (lists not as the merge leaves them, see the header) counts as V empty
  if (n_valid > 0 && total > 0.f && total < INFINITY) {
    for (int c = lane; c < n_class; c += 64) {
      float s = 0.f;
      for (int i = 0; i < k; ++i)
        if (lab[i] == c) s += wgt[i];
      s = s / total;
      score[(size_t)r * lds + c] = s;
      if (s > best) {                    // ascending c: the lowest class of the largest score stays
        best = s;
        best_c = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oc = __shfl_xor(best_c, o);
      if (oc >= 0 && (best_c < 0 || ob > best || (ob == best && oc < best_c))) {
        best = ob;
        best_c = oc;
      }
    }
  } else {
    for (int c = lane; c < n_class; c += 64) score[(size_t)r * lds + c] = 0.f;
  }
  if (lane == 0) pred[r] = best_c;
}

extern "C" int dv_knn_vote(const float* top_val, const int32_t* top_idx, int32_t ldk, int32_t R, int32_t k,
                           const int32_t* bank_labels, int32_t n_bank, int32_t n_class, float inv_T, float* score, int32_t lds,
                           int32_t* pred, void* stream) {
  if (!top_val || !top_idx || !bank_labels || !score || !pred || R <= 0 || k < 1 || k > DV_TOPK_MAX_K || ldk < k || n_bank <= 0 ||
      n_class < 1 || n_class > 4096 || lds < n_class || !(inv_T >= 0.f) || !(inv_T < INFINITY))
    return DV_EINVAL;
  hipLaunchKernelGGL(knn_vote_kernel, dim3(R), dim3(64), 0, ST(stream), top_val, top_idx, ldk, k, bank_labels, n_bank, n_class,
                     inv_T, score, lds, pred);
  return dv_launch_status();
}
