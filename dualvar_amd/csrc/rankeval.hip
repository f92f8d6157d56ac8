// Full-ranking retrieval figures (include/dualvar_rankeval.h: dv_rankeval_gather_f32, dv_rankeval_sort, dv_rankeval_count_f32,
// dv_rankeval_finish).
//
// The rank of every positive of a query in the full ordering of the bank without sorting the bank: the positives of a row are
// gathered into a short list and sorted, then every valid item of the row is counted into the bucket its binary search of that
// list gives; a prefix sum over the buckets is the ranks.  An item (key, bank index) is ONE 64-bit word here,
//   code = (~ord(key)) << 32 | index,   ord = the order-preserving map of fp32 onto uint32,
// so that "a precedes b" of the header is code_a < code_b and "p precedes j or p is j" is code_p <= code_j: the sort and the
// search compare integers.  The lists in memory stay (f32, i32); the map is a bijection on the keys (no NaN, no -0.0).
// Counts are integers and go through integer atomics only.
#include "common.hpp"
#include "../../include/dualvar_rankeval.h"

#define RE_THREADS 256
#define RE_STEP (4 * RE_THREADS)                // columns a workgroup takes per step: four per lane
#define RE_SPAN_STEPS 16                        // count: at least this many steps per workgroup when the columns are split
#define RE_TARGET_GROUPS 2048                   // count / gather: workgroups wanted before the columns stop being split
#define RE_PAD 0xffffffffffffffffull            // behind every item: the last item's code is at most 0xff800000'7ffffffe

typedef unsigned long long u64;

__device__ __forceinline__ float re_key(float s) { return s != s ? -INFINITY : s + 0.0f; }      // NaN -> -inf, -0.0 -> +0.0
__device__ __forceinline__ u64 re_code(float key, int idx) {
  const uint32_t u = __float_as_uint(key);
  const uint32_t ord = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);        // ascending in the key
  return ((u64)(~ord) << 32) | (uint32_t)idx;
}
__device__ __forceinline__ float re_code_key(u64 c) {
  const uint32_t ord = ~(uint32_t)(c >> 32);
  return __uint_as_float(ord ^ ((ord >> 31) ? 0x80000000u : 0xffffffffu));
}

// The four columns lane `tid` owns in the step at `base`: VEC: base + 4 tid + u (one 16-byte load where all four exist);
// otherwise base + tid + 256 u (four coalesced 4-byte loads).  Columns at or beyond n_cols are not read (value 0, skipped by
// the caller's j < end test).
template <bool VEC>
__device__ __forceinline__ void re_load4(const float* __restrict__ p, uint32_t base, uint32_t tid, uint32_t n_cols, float (&v)[4],
                                         uint32_t (&j)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) j[u] = base + (VEC ? 4 * tid + u : tid + RE_THREADS * u);
  if (VEC && j[3] < n_cols) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p + j[0]);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = j[u] < n_cols ? p[j[u]] : 0.f;
  }
}

// the column of row r that `exclude == 1` removes, or a column no item has
__device__ __forceinline__ uint32_t re_self(int exclude, long long diag, uint32_t r, uint32_t n_cols) {
  const long long dj = diag + (long long)r;
  return (exclude == 1 && dj >= 0 && dj < (long long)n_cols) ? (uint32_t)dj : 0xffffffffu;
}

__global__ void __launch_bounds__(RE_THREADS) rankeval_zero_cnt_kernel(int* __restrict__ pos_cnt, int R) {
  const int r = blockIdx.x * RE_THREADS + threadIdx.x;
  if (r < R) pos_cnt[r] = 0;
}

// workgroup (r, s): row r, columns [s * span, min((s + 1) * span, n_cols)); span is a multiple of RE_STEP
template <bool VEC>
__global__ void __launch_bounds__(RE_THREADS)
rankeval_gather_kernel(const float* __restrict__ sim, int ld, uint32_t n_cols, int col0, const int* __restrict__ row_cls,
                       const int* __restrict__ col_cls, const int* __restrict__ row_vid, const int* __restrict__ col_vid, int exclude,
                       long long diag, float* __restrict__ pos_val, int* __restrict__ pos_idx, int ldp, int* __restrict__ pos_cnt,
                       uint32_t span, uint32_t splits) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t r = blockIdx.x / splits, sp = blockIdx.x - r * splits;
  const uint32_t begin = sp * span, end = n_cols - begin < span ? n_cols : begin + span;
  const float* p = sim + (size_t)r * ld;
  const int rc = row_cls[r];
  const int rv = exclude == 2 ? row_vid[r] : 0;
  const uint32_t self = re_self(exclude, diag, r, n_cols);
  float* lv = pos_val + (size_t)r * ldp;
  int* li = pos_idx + (size_t)r * ldp;
  for (uint32_t base = begin; base < end; base += RE_STEP) {
    float v[4];
    uint32_t j[4];
    re_load4<VEC>(p, base, tid, n_cols, v, j);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bool pos = j[u] < end && j[u] != self && col_cls[j[u]] == rc;
      if (pos && exclude == 2) pos = col_vid[j[u]] != rv;
      // one atomic per wavefront: the first positive lane takes slots for all of them
      const u64 m = __ballot(pos);
      if (m == 0) continue;                                   // wave-uniform
      const int leader = __ffsll((long long)m) - 1;
      int slot0 = 0;
      if ((int)lane == leader) slot0 = atomicAdd(&pos_cnt[r], (int)__popcll(m));
      slot0 = __shfl(slot0, leader);
      const int slot = slot0 + (int)__popcll(m & ((1ull << lane) - 1ull));
      if (pos && slot < ldp) {
        lv[slot] = re_key(v[u]);
        li[slot] = (int)((uint32_t)col0 + j[u]);
      }
    }
  }
}

// One workgroup per row: the list as codes in LDS, padded to a power of two m with RE_PAD, a bitonic network, the first n back.
__global__ void __launch_bounds__(RE_THREADS)
rankeval_sort_kernel(float* __restrict__ pos_val, int* __restrict__ pos_idx, int ldp, const int* __restrict__ pos_cnt) {
  extern __shared__ u64 sc[];
  const uint32_t tid = threadIdx.x, r = blockIdx.x;
  const int cnt = pos_cnt[r];
  const uint32_t n = (uint32_t)(cnt < ldp ? (cnt < 0 ? 0 : cnt) : ldp);
  if (n < 2) return;                                          // uniform over the workgroup
  uint32_t m = 2;
  while (m < n) m <<= 1;                                      // <= 4096: ldp <= DV_RANKEVAL_MAX_POS, and the launch sized sc for it
  float* lv = pos_val + (size_t)r * ldp;
  int* li = pos_idx + (size_t)r * ldp;
  for (uint32_t i = tid; i < m; i += RE_THREADS) sc[i] = i < n ? re_code(re_key(lv[i]), li[i]) : RE_PAD;
  __syncthreads();
  for (uint32_t k = 2; k <= m; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (m >> 1); t += RE_THREADS) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;      // the t-th pair at distance j
        const u64 a = sc[lo], b = sc[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) {
          sc[lo] = b;
          sc[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < n; i += RE_THREADS) {
    lv[i] = re_code_key(sc[i]);
    li[i] = (int)(uint32_t)sc[i];
  }
}

__global__ void __launch_bounds__(RE_THREADS)
rankeval_zero_hist_kernel(uint32_t* __restrict__ hist, int ldh, const int* __restrict__ pos_cnt, int ldp) {
  const int cnt = pos_cnt[blockIdx.x];
  const int n = cnt < ldp ? (cnt < 0 ? 0 : cnt) : ldp;
  for (int i = threadIdx.x; i <= n; i += RE_THREADS) hist[(size_t)blockIdx.x * ldh + i] = 0u;
}

// workgroup (r, s) as in the gather kernel.  LDS: list codes u64 [ldp], then the histogram u32 [ldp + 1].
template <bool VEC>
__global__ void __launch_bounds__(RE_THREADS)
rankeval_count_kernel(const float* __restrict__ sim, int ld, uint32_t n_cols, int col0, const int* __restrict__ row_vid,
                      const int* __restrict__ col_vid, int exclude, long long diag, const float* __restrict__ pos_val,
                      const int* __restrict__ pos_idx, int ldp, const int* __restrict__ pos_cnt, uint32_t* __restrict__ hist, int ldh,
                      uint32_t span, uint32_t splits) {
  extern __shared__ u64 sc[];
  uint32_t* lh = reinterpret_cast<uint32_t*>(sc + ldp);
  const uint32_t tid = threadIdx.x;
  const uint32_t r = blockIdx.x / splits, sp = blockIdx.x - r * splits;
  const uint32_t begin = sp * span, end = n_cols - begin < span ? n_cols : begin + span;
  const int cnt = pos_cnt[r];
  const uint32_t n = (uint32_t)(cnt < ldp ? (cnt < 0 ? 0 : cnt) : ldp);
  const float* lv = pos_val + (size_t)r * ldp;
  const int* li = pos_idx + (size_t)r * ldp;
  for (uint32_t i = tid; i < n; i += RE_THREADS) sc[i] = re_code(lv[i], li[i]);
  for (uint32_t i = tid; i <= n; i += RE_THREADS) lh[i] = 0u;
  __syncthreads();
  const float* p = sim + (size_t)r * ld;
  const int rv = exclude == 2 ? row_vid[r] : 0;
  const uint32_t self = re_self(exclude, diag, r, n_cols);
  for (uint32_t base = begin; base < end; base += RE_STEP) {
    float v[4];
    uint32_t j[4];
    re_load4<VEC>(p, base, tid, n_cols, v, j);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bool valid = j[u] < end && j[u] != self;
      if (valid && exclude == 2) valid = col_vid[j[u]] != rv;
      const u64 c = re_code(re_key(v[u]), (int)((uint32_t)col0 + j[u]));      // j beyond n_cols: not counted
      // b = #{i < n : sc[i] <= c}: the list ascends, so the predicate holds on a prefix
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc[mid] <= c) lo = mid + 1; else hi = mid;
      }
      // one LDS add per item, also where most lanes of a wavefront meet in the bucket behind the last positive: merging those
      // adds per wavefront first (a ballot and a population count) measured 12 to 15 % slower
      if (valid) atomicAdd(&lh[lo], 1u);
    }
  }
  __syncthreads();
  uint32_t* h = hist + (size_t)r * ldh;
  for (uint32_t i = tid; i <= n; i += RE_THREADS) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&h[i], c);
  }
}

// One workgroup per row.  LDS: the inclusive prefix sums u32 [ldp + 1] (padded to 8 bytes), then the AP terms f64 [ldp].
__global__ void __launch_bounds__(RE_THREADS)
rankeval_finish_kernel(const uint32_t* __restrict__ hist, int ldh, const int* __restrict__ pos_cnt, int ldp, const int* __restrict__ ks,
                       int n_k, int* __restrict__ rank, double* __restrict__ ap, int* __restrict__ first_rank, int* __restrict__ hits,
                       int* __restrict__ rhits, int* __restrict__ n_valid) {
  extern __shared__ u64 sc[];
  uint32_t* cum = reinterpret_cast<uint32_t*>(sc);
  double* term = reinterpret_cast<double*>(sc + (ldp + 2) / 2);
  __shared__ uint32_t part[RE_THREADS];
  const uint32_t tid = threadIdx.x, r = blockIdx.x;
  const int cnt = pos_cnt[r];
  const uint32_t P = (uint32_t)(cnt < ldp ? (cnt < 0 ? 0 : cnt) : ldp);
  const uint32_t* h = hist + (size_t)r * ldh;
  // inclusive prefix sums of hist[r][0..P]: a lane owns `seg` consecutive buckets
  const uint32_t seg = (P + RE_THREADS) / RE_THREADS;          // ceil((P + 1) / 256)
  const uint32_t b0 = tid * seg, b1 = b0 + seg < P + 1 ? b0 + seg : P + 1;
  uint32_t s = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    s += h[b];
    cum[b] = s;
  }
  part[tid] = s;
  __syncthreads();
  uint32_t off = 0;
  for (uint32_t t = 0; t < tid; ++t) off += part[t];
  for (uint32_t b = b0; b < b1; ++b) cum[b] += off;
  __syncthreads();
  for (uint32_t i = tid; i < P; i += RE_THREADS) {
    const int rho = 1 + (int)cum[i];
    rank[(size_t)r * ldp + i] = rho;
    term[i] = (double)(int)(i + 1) / (double)rho;
  }
  // hits(k) = #{i < P : 1 + cum[i] <= k}: the ranks ascend strictly, so one binary search each; lane n_k takes k = P
  if (tid <= (uint32_t)n_k) {
    const long long k = tid < (uint32_t)n_k ? (long long)ks[tid] : (long long)P;
    uint32_t lo = 0, hi = P;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((long long)cum[mid] + 1 <= k) lo = mid + 1; else hi = mid;
    }
    if (tid < (uint32_t)n_k) hits[(size_t)r * n_k + tid] = (int)lo; else rhits[r] = (int)lo;
  }
  __syncthreads();
  if (tid == 0) {
    double a = -1.0;
    if (P) {
      a = 0.0;
      for (uint32_t i = 0; i < P; ++i) a += term[i];          // ascending i: the order the header states
      a /= (double)(int)P;
    }
    ap[r] = a;
    first_rank[r] = P ? 1 + (int)cum[0] : 0;
    n_valid[r] = (int)cum[P];
  }
}

// (span, splits) of the columns for R rows: one workgroup per row once there are RE_TARGET_GROUPS rows, otherwise spans of at
// least min_steps steps; R * splits fits a 1-D grid
static inline void rankeval_split(int32_t R, int32_t n_cols, int min_steps, uint32_t& span, uint32_t& splits) {
  const int64_t steps = cdiv64(n_cols, RE_STEP);
  int64_t want = cdiv64(RE_TARGET_GROUPS, R);
  const int64_t most = cdiv64(steps, min_steps);
  if (want > most) want = most;
  if (want > 0x7fffffffLL / R) want = 0x7fffffffLL / R;
  if (want < 1) want = 1;
  const int64_t span_steps = cdiv64(steps, want);
  span = (uint32_t)(span_steps * RE_STEP);                      // < 2^31 + RE_STEP
  splits = (uint32_t)cdiv64(steps, span_steps);
}

static inline bool rankeval_block_bad(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0, const int32_t* row_vid,
                                      const int32_t* col_vid, int32_t exclude, int32_t ldp) {
  return !sim || R <= 0 || n_cols <= 0 || ld < n_cols || ldp < 1 || ldp > DV_RANKEVAL_MAX_POS || exclude < 0 || exclude > 2 ||
         (exclude == 2 && (!row_vid || !col_vid)) || col0 < 0 || (int64_t)col0 + n_cols > 0x7fffffffLL;
}

extern "C" int dv_rankeval_gather_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0, const int32_t* row_cls,
                                      const int32_t* col_cls, const int32_t* row_vid, const int32_t* col_vid, int32_t exclude,
                                      int64_t diag, float* pos_val, int32_t* pos_idx, int32_t ldp, int32_t* pos_cnt, int32_t first,
                                      void* stream) {
  if (rankeval_block_bad(sim, ld, R, n_cols, col0, row_vid, col_vid, exclude, ldp) || !row_cls || !col_cls || !pos_val || !pos_idx ||
      !pos_cnt)
    return DV_EINVAL;
  uint32_t span, splits;
  rankeval_split(R, n_cols, 4, span, splits);
  if (first) hipLaunchKernelGGL(rankeval_zero_cnt_kernel, dim3((unsigned)cdiv64(R, RE_THREADS)), dim3(RE_THREADS), 0, ST(stream), pos_cnt, R);
  const dim3 grid((unsigned)((int64_t)R * splits));
  if (aligned16(sim) && ld % 4 == 0)
    hipLaunchKernelGGL(rankeval_gather_kernel<true>, grid, dim3(RE_THREADS), 0, ST(stream), sim, ld, (uint32_t)n_cols, col0, row_cls,
                       col_cls, row_vid, col_vid, exclude, (long long)diag, pos_val, pos_idx, ldp, pos_cnt, span, splits);
  else
    hipLaunchKernelGGL(rankeval_gather_kernel<false>, grid, dim3(RE_THREADS), 0, ST(stream), sim, ld, (uint32_t)n_cols, col0, row_cls,
                       col_cls, row_vid, col_vid, exclude, (long long)diag, pos_val, pos_idx, ldp, pos_cnt, span, splits);
  return dv_launch_status();
}

extern "C" int dv_rankeval_sort(float* pos_val, int32_t* pos_idx, int32_t ldp, const int32_t* pos_cnt, int32_t R, void* stream) {
  if (!pos_val || !pos_idx || !pos_cnt || R <= 0 || ldp < 1 || ldp > DV_RANKEVAL_MAX_POS) return DV_EINVAL;
  size_t m = 2;
  while (m < (size_t)ldp) m <<= 1;
  hipLaunchKernelGGL(rankeval_sort_kernel, dim3((unsigned)R), dim3(RE_THREADS), m * sizeof(u64), ST(stream), pos_val, pos_idx, ldp,
                     pos_cnt);
  return dv_launch_status();
}

extern "C" int dv_rankeval_count_f32(const float* sim, int32_t ld, int32_t R, int32_t n_cols, int32_t col0, const int32_t* row_vid,
                                     const int32_t* col_vid, int32_t exclude, int64_t diag, const float* pos_val,
                                     const int32_t* pos_idx, int32_t ldp, const int32_t* pos_cnt, uint32_t* hist, int32_t ldh,
                                     int32_t first, void* stream) {
  if (rankeval_block_bad(sim, ld, R, n_cols, col0, row_vid, col_vid, exclude, ldp) || !pos_val || !pos_idx || !pos_cnt || !hist ||
      ldh < ldp + 1)
    return DV_EINVAL;
  uint32_t span, splits;
  rankeval_split(R, n_cols, RE_SPAN_STEPS, span, splits);
  if (first) hipLaunchKernelGGL(rankeval_zero_hist_kernel, dim3((unsigned)R), dim3(RE_THREADS), 0, ST(stream), hist, ldh, pos_cnt, ldp);
  const dim3 grid((unsigned)((int64_t)R * splits));
  const size_t lds = (size_t)ldp * sizeof(u64) + ((size_t)ldp + 1) * sizeof(uint32_t);
  if (aligned16(sim) && ld % 4 == 0)
    hipLaunchKernelGGL(rankeval_count_kernel<true>, grid, dim3(RE_THREADS), lds, ST(stream), sim, ld, (uint32_t)n_cols, col0, row_vid,
                       col_vid, exclude, (long long)diag, pos_val, pos_idx, ldp, pos_cnt, hist, ldh, span, splits);
  else
    hipLaunchKernelGGL(rankeval_count_kernel<false>, grid, dim3(RE_THREADS), lds, ST(stream), sim, ld, (uint32_t)n_cols, col0, row_vid,
                       col_vid, exclude, (long long)diag, pos_val, pos_idx, ldp, pos_cnt, hist, ldh, span, splits);
  return dv_launch_status();
}

extern "C" int dv_rankeval_finish(const uint32_t* hist, int32_t ldh, const int32_t* pos_cnt, int32_t ldp, int32_t R, const int32_t* ks,
                                  int32_t n_k, int32_t* rank, double* ap, int32_t* first_rank, int32_t* hits, int32_t* rhits,
                                  int32_t* n_valid, void* stream) {
  if (!hist || !pos_cnt || !rank || !ap || !first_rank || !rhits || !n_valid || R <= 0 || ldp < 1 || ldp > DV_RANKEVAL_MAX_POS ||
      ldh < ldp + 1 || n_k < 0 || n_k > 16 || (n_k > 0 && (!ks || !hits)))
    return DV_EINVAL;
  if ((uintptr_t)ap & 7) return DV_EALIGN;
  const size_t lds = ((size_t)(ldp + 2) / 2 + (size_t)ldp) * sizeof(u64);
  hipLaunchKernelGGL(rankeval_finish_kernel, dim3((unsigned)R), dim3(RE_THREADS), lds, ST(stream), hist, ldh, pos_cnt, ldp, ks, n_k,
                     rank, ap, first_rank, hits, rhits, n_valid);
  return dv_launch_status();
}
