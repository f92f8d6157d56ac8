// MaxPool3d on gfx950: the per-element gather kernels, the 2x2-quad backward, the LDS-staged 3x3x3 tiles, and the stem pools
// fused with the BatchNorm + ReLU in front of them (forward, and the BatchNorm backward over the pooled gradient).
// Everything here is launched through a dv_pool_desc; pool_route is the one place that picks a kernel.
#include "streaming.hpp"

namespace {

// ------------------------------------------------------------------ MaxPool3d
// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  With a grid that is a multiple of 8, this gives
// XCD x the logical blocks [x * grid/8, (x+1) * grid/8): neighbouring windows share an L2 instead of each XCD fetching
// every plane.
__device__ __forceinline__ uint32_t xcd_block() { return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3); }
static inline int grid8_for(int64_t work_items, int max_blocks) { return (grid_for(work_items, max_blocks) + 7) & ~7; }

struct PoolArgs {
  int N, Ti, Hi, Wi, C, CP;
  int To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int ldx, ldy;
  FastDiv fcv, fWo, fHo, fTo, fWi, fHi, fTi;
};

template <typename T>
__global__ void maxpool_fwd_kernel(PoolArgs a, const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = a.fcv.d;
  const uint32_t total = (uint32_t)a.N * a.To * a.Ho * a.Wo * CV;
  for (uint32_t i = xcd_block() * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    uint32_t m, cvi, q, wo_, ho_, to_, n_;
    fd_divmod(i, a.fcv, m, cvi);
    const int c0 = (int)cvi * V;
    fd_divmod(m, a.fWo, q, wo_);
    fd_divmod(q, a.fHo, q, ho_);
    fd_divmod(q, a.fTo, n_, to_);
    const int wo = (int)wo_, ho = (int)ho_, to = (int)to_, n = (int)n_;
    float best[V]; int bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    bool first = true;
    int tap = 0;
    for (int dt = 0; dt < a.kt; ++dt) {
      const int t = to * a.st - a.pt + dt;
      for (int dh = 0; dh < a.kh; ++dh) {
        const int hh = ho * a.sh - a.ph + dh;
        for (int dw = 0; dw < a.kw; ++dw, ++tap) {
          const int w = wo * a.sw - a.pw + dw;
          if ((unsigned)t >= (unsigned)a.Ti || (unsigned)hh >= (unsigned)a.Hi || (unsigned)w >= (unsigned)a.Wi) continue;
          float v[V];
          Pack16<T>::load(x + ((int64_t)((n * a.Ti + t) * a.Hi + hh) * a.Wi + w) * a.ldx + c0, v);
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (first || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = tap; }
          first = false;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) if (c0 + e >= a.C) best[e] = 0.f;
    Pack16<T>::store(y + (size_t)m * a.ldy + c0, best);
    uint8_t* ip = idx + (size_t)m * a.CP + c0;
#pragma unroll
    for (int e = 0; e < V; ++e) ip[e] = (uint8_t)bi[e];
  }
}

template <typename T>
__device__ __forceinline__ void pool_gather(const PoolArgs& a, const T* __restrict__ dyp, const uint8_t* __restrict__ idx,
                                            uint32_t m_in, int c0, float (&g)[DT<T>::VEC]);

template <typename T>
__global__ void maxpool_bwd_kernel(PoolArgs a, const T* __restrict__ dy, const uint8_t* __restrict__ idx,
                                   T* __restrict__ dx, int accumulate) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = a.fcv.d;
  const uint32_t total = (uint32_t)a.N * a.Ti * a.Hi * a.Wi * CV;
  for (uint32_t i = xcd_block() * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    uint32_t m, cvi;
    fd_divmod(i, a.fcv, m, cvi);
    const int c0 = (int)cvi * V;
    float acc[V];
    if (accumulate) Pack16<T>::load(dx + (size_t)m * a.ldx + c0, acc);
    else {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = 0.f;
    }
    pool_gather<T>(a, dy, idx, m, c0, acc);
    Pack16<T>::store(dx + (size_t)m * a.ldx + c0, acc);
  }
}

// Backward of the pools with a 3x3 window, stride 2, padding 1 in (h, w) -- the stem pools (s3dg.py:139,145, 1x3x3 / 1x2x2;
// resnet_2d3d.py:130) and MaxPool_4a (3x3x3 / 2x2x2) -- with any window along t.  A thread owns a 2x2 QUAD of input pixels:
// together they are covered by the four windows (hq, wq) .. (hq+1, wq+1) only, so a thread loads four (dy, idx) vectors per
// t-window and applies them to its pixels in nine compares, the same count for every thread -- the per-pixel gather has 1, 2,
// 2 or 4 windows depending on the parity of the pixel (divergent trip counts) and loads every window vector four times.
// Same sums, same (ascending tap) order as pool_gather.
template <typename T>
__global__ void maxpool_bwd_quad_kernel(PoolArgs a, FastDiv fWq, FastDiv fHq, const T* __restrict__ dy,
                                        const uint8_t* __restrict__ idx, T* __restrict__ dx, int accumulate) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = a.fcv.d;
  const uint32_t total = (uint32_t)a.N * a.Ti * fHq.d * fWq.d * CV;
  const int st1 = a.st - 1;
  for (uint32_t i = xcd_block() * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    uint32_t q, cvi, wq_, hq_, ti_, n_;
    fd_divmod(i, a.fcv, q, cvi);
    fd_divmod(q, fWq, q, wq_);
    fd_divmod(q, fHq, q, hq_);
    fd_divmod(q, a.fTi, n_, ti_);
    const int c0 = (int)cvi * V, wq = (int)wq_, hq = (int)hq_, ti = (int)ti_, n = (int)n_;
    float acc[2][2][V];
    bool pix[2][2];
#pragma unroll
    for (int pa = 0; pa < 2; ++pa)
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        pix[pa][pb] = 2 * hq + pa < a.Hi && 2 * wq + pb < a.Wi;
        const size_t m = ((size_t)(n * a.Ti + ti) * a.Hi + 2 * hq + pa) * a.Wi + 2 * wq + pb;
        if (accumulate && pix[pa][pb]) Pack16<T>::load(dx + m * a.ldx + c0, acc[pa][pb]);
        else {
#pragma unroll
          for (int e = 0; e < V; ++e) acc[pa][pb][e] = 0.f;
        }
      }
    const int tn = ti + a.pt;
    const int t_hi = min(tn >> st1, a.To - 1), t_lo = max((tn - a.kt + 1 + st1) >> st1, 0);
    for (int to = t_hi; to >= t_lo; --to) {
      const int dt = tn - to * a.st;
      float g[2][2][V];
      uint32_t iw[2][2][V / 4];
#pragma unroll
      for (int wy = 0; wy < 2; ++wy)
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
          const bool ok = hq + wy < a.Ho && wq + wx < a.Wo;
          const int64_t mo = (int64_t)((n * a.To + to) * a.Ho + hq + wy) * a.Wo + wq + wx;
          if (ok) {
            Pack16<T>::load(dy + mo * a.ldy + c0, g[wy][wx]);
#pragma unroll
            for (int j = 0; j < V / 4; ++j) iw[wy][wx][j] = reinterpret_cast<const uint32_t*>(idx + mo * a.CP + c0)[j];
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) g[wy][wx][e] = 0.f;
#pragma unroll
            for (int j = 0; j < V / 4; ++j) iw[wy][wx][j] = 0xffffffffu;
          }
        }
      // pixel (pa, pb) lies in window (wy, wx) iff wy <= pa and wx <= pb, at tap (dh, dw) = (pa + 1 - 2 wy, pb + 1 - 2 wx)
#pragma unroll
      for (int pa = 0; pa < 2; ++pa)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int wy = 1; wy >= 0; --wy)
#pragma unroll
            for (int wx = 1; wx >= 0; --wx) {
              if (wy > pa || wx > pb) continue;
              const uint32_t tap = (uint32_t)((dt * 3 + pa + 1 - 2 * wy) * 3 + pb + 1 - 2 * wx);
#pragma unroll
              for (int e = 0; e < V; ++e)
                if (((iw[wy][wx][e >> 2] >> (8 * (e & 3))) & 0xffu) == tap) acc[pa][pb][e] += g[wy][wx][e];
            }
    }
#pragma unroll
    for (int pa = 0; pa < 2; ++pa)
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        if (!pix[pa][pb]) continue;
        const size_t m = ((size_t)(n * a.Ti + ti) * a.Hi + 2 * hq + pa) * a.Wi + 2 * wq + pb;
        Pack16<T>::store(dx + m * a.ldx + c0, acc[pa][pb]);
      }
  }
}

// ------------------------------------------------------------------ BatchNorm + ReLU + MaxPool3d as one pass each way
// A pool that is the ONLY consumer of y = relu(x*scale + shift) (the stems: s3dg.py:138-151, resnet_2d3d.py:128-131) never
// needs y in memory: the backward of that BatchNorm rebuilds the ReLU mask from x (DV_MASK_FROM_X) and the pool's own
// backward only needs the tap indices.  Forward: the window elements are normalised, rectified and rounded to the storage
// type on the fly, exactly the values bn_apply would have stored (same expression, same rounding), so pooled values and
// indices are bit-identical to the two-pass form.  Backward: g = dL/dy of an input element is the gather of the pooled
// gradients through idx (maxpool_bwd's inner loop), evaluated inside the reduce and the apply pass of the BatchNorm
// backward instead of being written and read back twice.  Saved per stem pool: one write + one read of y forward, one
// write + two reads of dL/dy backward, two launches.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_maxpool_kernel(PoolArgs a, const T* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, T* __restrict__ y,
                                                               uint8_t* __restrict__ idx) {
  constexpr int V = DT<T>::VEC;
  const uint32_t CV = a.fcv.d;
  const uint32_t total = (uint32_t)a.N * a.To * a.Ho * a.Wo * CV;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    uint32_t m, cvi, q, wo_, ho_, to_, n_;
    fd_divmod(i, a.fcv, m, cvi);
    const int c0 = (int)cvi * V;
    fd_divmod(m, a.fWo, q, wo_);
    fd_divmod(q, a.fHo, q, ho_);
    fd_divmod(q, a.fTo, n_, to_);
    const int wo = (int)wo_, ho = (int)ho_, to = (int)to_, n = (int)n_;
    float sc[V], sh[V];
    load_params<V>(scale, c0, sc);
    load_params<V>(shift, c0, sh);
    float best[V]; int bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    bool first = true;
    int tap = 0;
    for (int dt = 0; dt < a.kt; ++dt) {
      const int t = to * a.st - a.pt + dt;
      for (int dh = 0; dh < a.kh; ++dh) {
        const int hh = ho * a.sh - a.ph + dh;
        for (int dw = 0; dw < a.kw; ++dw, ++tap) {
          const int w = wo * a.sw - a.pw + dw;
          if ((unsigned)t >= (unsigned)a.Ti || (unsigned)hh >= (unsigned)a.Hi || (unsigned)w >= (unsigned)a.Wi) continue;
          float v[V];
          Pack16<T>::load(x + ((int64_t)((n * a.Ti + t) * a.Hi + hh) * a.Wi + w) * a.ldx + c0, v);
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float yv = bn_relu_stored<T>(v[e], sc[e], sh[e]);     // what bn_apply stores
            if (first || yv > best[e] || yv != yv) { best[e] = yv; bi[e] = tap; }
          }
          first = false;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) if (c0 + e >= a.C) best[e] = 0.f;
    Pack16<T>::store(y + (size_t)m * a.ldy + c0, best);
    uint8_t* ip = idx + (size_t)m * a.CP + c0;
#pragma unroll
    for (int e = 0; e < V; ++e) ip[e] = (uint8_t)bi[e];
  }
}

// g[e] += dL/dy of input element (row m_in, channels c0..c0+V): the pooled gradients of the windows that chose it.  Only
// the windows that contain the element are visited (o*s - p <= i < o*s - p + k per dimension: 3.4 of the 27 taps of a
// 3x3x3 / stride 2 pool on average), in ascending tap order, which fixes the order of the fp32 sums.
template <typename T>
__device__ __forceinline__ void pool_gather(const PoolArgs& a, const T* __restrict__ dyp, const uint8_t* __restrict__ idx,
                                            uint32_t m_in, int c0, float (&g)[DT<T>::VEC]) {
  constexpr int V = DT<T>::VEC;
  uint32_t q, wi_, hi_, ti_, n_;
  fd_divmod(m_in, a.fWi, q, wi_);
  fd_divmod(q, a.fHi, q, hi_);
  fd_divmod(q, a.fTi, n_, ti_);
  const int n = (int)n_;
  // strides are 1 or 2 (checked on the host): division by the stride is a shift, ceil(x / s) = (x + s - 1) >> (s - 1)
  const int st1 = a.st - 1, sh1 = a.sh - 1, sw1 = a.sw - 1;
  const int tn = (int)ti_ + a.pt, hn = (int)hi_ + a.ph, wn = (int)wi_ + a.pw;
  const int t_hi = min(tn >> st1, a.To - 1), t_lo = max((tn - a.kt + 1 + st1) >> st1, 0);
  const int h_hi = min(hn >> sh1, a.Ho - 1), h_lo = max((hn - a.kh + 1 + sh1) >> sh1, 0);
  const int w_hi = min(wn >> sw1, a.Wo - 1), w_lo = max((wn - a.kw + 1 + sw1) >> sw1, 0);
  for (int to = t_hi; to >= t_lo; --to) {
    const int dt = tn - to * a.st;
    for (int ho = h_hi; ho >= h_lo; --ho) {
      const int dh = hn - ho * a.sh;
      for (int wo = w_hi; wo >= w_lo; --wo) {
        const uint32_t tap = (uint32_t)((dt * a.kh + dh) * a.kw + wn - wo * a.sw);
        const int64_t mo = (int64_t)((n * a.To + to) * a.Ho + ho) * a.Wo + wo;
        float d[V];
        Pack16<T>::load(dyp + mo * a.ldy + c0, d);
        const uint8_t* ip = idx + mo * a.CP + c0;
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (ip[e] == tap) g[e] += d[e];
      }
    }
  }
}

// dL/dy gathered from the pooled gradient: the third source of bn_bwd_reduce_body / bn_bwd_apply_body.  kPooled fixes, at
// compile time, what the one consumer of such a BatchNorm never varies -- the mask rebuilt from x (DV_MASK_FROM_X), sums by
// atomics (no ordered-fold workspace, hence no ticket word in LDS), no residual gradient -- so those branches fold away.
template <typename T>
struct PooledDy {
  static constexpr int V = DT<T>::VEC, kRows = 0;
  static constexpr bool kPooled = true;
  struct Pend {};
  const PoolArgs& a; const T* dyp; const uint8_t* idx;
  __device__ __forceinline__ void load(int64_t r, int c0, float (&g)[V], Pend&) const {
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    pool_gather<T>(a, dyp, idx, (uint32_t)r, c0, g);
  }
  __device__ __forceinline__ void finish(int64_t, int, float (&)[V], Pend&) const {}
};

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_maxpool_kernel(PoolArgs a, const T* __restrict__ dyp, const uint8_t* __restrict__ idx,
                                             const T* __restrict__ x, const float* __restrict__ mean,
                                             const float* __restrict__ invstd, const float* __restrict__ scale,
                                             const float* __restrict__ shift, int64_t M, int C, int CP, int64_t rows_per_block,
                                             float* __restrict__ sums_all, int n_rep) {
  bn_bwd_reduce_body<T>(PooledDy<T>{a, dyp, idx}, nullptr, 0, x, a.ldx, mean, invstd, M, C, CP, 0, rows_per_block, sums_all,
                        n_rep, blockIdx.x, scale, shift, nullptr, gridDim.x);
}

template <typename T>
__global__ void bn_bwd_apply_maxpool_kernel(PoolArgs a, const T* __restrict__ dyp, const uint8_t* __restrict__ idx,
                                            const T* __restrict__ x, const float* __restrict__ mean,
                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                            const float* __restrict__ sums_g, int rep_g, float inv_count, float dscale,
                                            float* dgamma, float* dbeta, T* __restrict__ dx, int lddx, uint32_t total, int C,
                                            int CP) {
  bn_bwd_apply_body<T>(PooledDy<T>{a, dyp, idx}, nullptr, 0, x, a.ldx, mean, invstd, gamma, sums_g, rep_g, inv_count, dscale,
                       dgamma, dbeta, dx, lddx, nullptr, 0, total, C, CP, a.fcv, 0, blockIdx.x, gridDim.x, scale, shift);
}

// ------------------------------------------------------------------ MaxPool3d 3x3x3 / stride 1 / padding 1, LDS-staged
// The gather kernels above read every window element through L1 / L2 (27 taps): with workgroups dealt round-robin to
// the 8 XCDs, neighbouring windows land in different L2s and each of them fetches the whole tensor (PMC: 7.2x the
// algorithmic bytes forward, 8.8x backward on the 14x14 fp32 pools).  Here a workgroup owns a TH x TW spatial tile of
// one clip and a chunk of CV 16-byte channel vectors, and walks the T planes once: plane t+1 is in flight to
// registers while plane t-1 is computed from a three-slot ring in LDS that holds planes t-2 .. t with a one-pixel
// halo, so every element leaves L2 once (1.29x with the halo rows) and the 27 taps are LDS reads.  Workgroup order
// is XCD-aware: consecutive tiles of a clip go to the same XCD, so halo rows and the other channel chunks of a
// 128-byte line are L2 hits.
//   forward : values are staged as order-preserving 32-bit keys (key_f32: a plain unsigned compare orders them, padding
//             is key 0 below every real value, a NaN with the sign bit clear wins as in PyTorch; -0.0 orders below
//             +0.0, a tie in PyTorch -- inputs are post-ReLU).  Taps are scanned in PyTorch's order with a strict
//             compare: first maximum wins, same values and uint8 tap index as maxpool_fwd_kernel.
//   backward: (dy, idx) staged with idx = 0xff outside the tensor; an input element adds dy of the windows that chose it
//             in the tap order of maxpool_bwd_kernel, so the fp32 sums are bit-identical to that kernel's.
struct PoolTileArgs {
  int N, T, H, W, C, CP, ldx, ldy;
  int nth, ntw, ncc, cpv;              // tiles along H and W, channel chunks, 16-byte vectors per pixel
  uint32_t groups, per_xcd;            // workgroups with work; ceil(groups / 8)
  FastDiv fcc, ftw, fth;
  int accumulate;
};

__device__ __forceinline__ uint32_t key_f32(uint32_t x) { return x ^ ((uint32_t)((int32_t)x >> 31) | 0x80000000u); }
__device__ __forceinline__ uint32_t unkey_f32(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// CV 16-byte global vectors per pixel and workgroup; Q = 4-channel quads per global vector (1 for fp32, 2 for bf16).  LDS
// holds one uint4 of 32-bit entries per quad (bf16 is widened while staging), and a work item is one quad of one pixel.
template <int TH, int TW, int CV, int Q>
struct PoolTile {
  static constexpr int HW = TW + 2, NPX = (TH + 2) * HW, NST = NPX * CV, SR = (NST + kThreads - 1) / kThreads;
  static constexpr int QV = CV * Q, NLE = NPX * QV, NIT = TH * TW * QV, R = (NIT + kThreads - 1) / kThreads;
  int n, h0, w0, cv0;
  __device__ __forceinline__ bool locate(const PoolTileArgs& a) {
    const uint32_t lb = (blockIdx.x & 7u) * a.per_xcd + (blockIdx.x >> 3);
    if (lb >= a.groups) return false;
    uint32_t q, cc, tw, th, nn;
    fd_divmod(lb, a.fcc, q, cc);
    fd_divmod(q, a.ftw, q, tw);
    fd_divmod(q, a.fth, nn, th);
    n = (int)nn; h0 = (int)th * TH; w0 = (int)tw * TW; cv0 = (int)cc * CV;
    return true;
  }
  // staged vector i of a plane -> halo pixel (h, w) and channel vector cv; false when nothing is to be fetched
  __device__ __forceinline__ bool stage_src(const PoolTileArgs& a, int i, int& h, int& w, int& cv) const {
    const int px = i / CV;
    cv = cv0 + (i - px * CV);
    const int hh = px / HW;
    h = h0 - 1 + hh; w = w0 - 1 + (px - hh * HW);
    return i < NST && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W && cv < a.cpv;
  }
  // item it of the tile -> pixel (ph, pw) inside the tile and quad ql of the chunk; false for lanes without an output
  __device__ __forceinline__ bool item(const PoolTileArgs& a, int it, int& ph, int& pw, int& ql) const {
    const int px = it / QV;
    ql = it - px * QV;
    ph = px / TW; pw = px - ph * TW;
    return it < NIT && h0 + ph < a.H && w0 + pw < a.W && cv0 * Q + ql < a.cpv * Q;
  }
};

// the two quads of a 16-byte vector of bf16, widened to fp32 bit patterns
__device__ __forceinline__ void widen_bf16x8(const uint4& v, uint4& q0, uint4& q1) {
  q0 = make_uint4(v.x << 16, v.x & 0xffff0000u, v.y << 16, v.y & 0xffff0000u);
  q1 = make_uint4(v.z << 16, v.z & 0xffff0000u, v.w << 16, v.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 key_quad(const uint4& v) { return make_uint4(key_f32(v.x), key_f32(v.y), key_f32(v.z), key_f32(v.w)); }

template <typename T, int TH, int TW, int CV>
__global__ __launch_bounds__(kThreads) void pool333_fwd_tile_kernel(PoolTileArgs a, const T* __restrict__ x,
                                                                    T* __restrict__ y, uint8_t* __restrict__ idx) {
  constexpr int V = DT<T>::VEC, Q = V / 4;
  using PT = PoolTile<TH, TW, CV, Q>;
  __shared__ uint4 slots[2][PT::NLE];
  PT tl;
  if (!tl.locate(a)) return;
  const int tid = threadIdx.x;
  const int64_t plane = (int64_t)a.H * a.W * a.ldx;
  int64_t soff[PT::SR];
  bool sval[PT::SR];
#pragma unroll
  for (int s = 0; s < PT::SR; ++s) {
    int h, w, cv;
    sval[s] = tl.stage_src(a, s * kThreads + tid, h, w, cv);
    soff[s] = ((int64_t)(tl.n * a.T) * a.H * a.W + (int64_t)h * a.W + w) * a.ldx + cv * V;
  }
  uint4 pre[PT::SR];
  auto prefetch = [&](int t) {
#pragma unroll
    for (int s = 0; s < PT::SR; ++s)
      pre[s] = sval[s] ? *reinterpret_cast<const uint4*>(x + soff[s] + t * plane) : make_uint4(0u, 0u, 0u, 0u);
  };
  auto commit = [&](int slot) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int s = 0; s < PT::SR; ++s) {
      const int i = s * kThreads + tid;
      if (i >= PT::NST) break;
      if constexpr (Q == 1) {
        slots[slot][i] = sval[s] ? key_quad(pre[s]) : zero;
      } else {
        uint4 q0, q1;
        widen_bf16x8(pre[s], q0, q1);
        slots[slot][2 * i] = sval[s] ? key_quad(q0) : zero;
        slots[slot][2 * i + 1] = sval[s] ? key_quad(q1) : zero;
      }
    }
  };
  // The window maximum is taken plane by plane: the first maximum of the 3x3 spatial window of one plane (key and spatial
  // tap 0..8) is kept in registers for the two previous planes; an output is the first maximum of its three plane maxima in
  // plane order -- the element PyTorch's (dt, dh, dw) scan with a strict compare picks, with 9 + 3 compares, not 27.
  uint32_t k2[PT::R][4], c2[PT::R][4], k1[PT::R][4], c1[PT::R][4], k0[PT::R][4], c0[PT::R][4];
  bool live[PT::R];
  int base[PT::R];
#pragma unroll
  for (int r = 0; r < PT::R; ++r) {
    int ph, pw, ql;
    live[r] = tl.item(a, r * kThreads + tid, ph, pw, ql);
    base[r] = (ph * PT::HW + pw) * PT::QV + ql;
#pragma unroll
    for (int e = 0; e < 4; ++e) { k1[r][e] = 0u; c1[r][e] = 0u; k0[r][e] = 0u; c0[r][e] = 0u; }
  }
  prefetch(0);
  for (int t = 0; t <= a.T; ++t) {
    if (t < a.T) {
      commit(t & 1);
      if (t + 1 < a.T) prefetch(t + 1);
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < PT::R; ++r) {
      if (!live[r]) continue;
      const int it = r * kThreads + tid, px = it / PT::QV, ph = px / TW, pw = px - ph * TW;
      const int h = tl.h0 + ph, w = tl.w0 + pw;
      const uint32_t code0 = (h == 0 ? 3u : 0u) + (w == 0 ? 1u : 0u);
#pragma unroll
      for (int e = 0; e < 4; ++e) { k2[r][e] = k1[r][e]; c2[r][e] = c1[r][e]; k1[r][e] = k0[r][e]; c1[r][e] = c0[r][e]; }
      if (t < a.T) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { k0[r][e] = 0u; c0[r][e] = code0; }
        const uint4* pl = slots[t & 1] + base[r];
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
#pragma unroll
          for (int dw = 0; dw < 3; ++dw) {
            const uint4 k = pl[(dh * PT::HW + dw) * PT::QV];
            const uint32_t kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (kk[e] > k0[r][e]) { k0[r][e] = kk[e]; c0[r][e] = (uint32_t)(dh * 3 + dw); }
          }
      }
      if (t == 0) continue;
      const int to = t - 1;
      uint32_t best[4], bi[4];
      // planes to-1 (k2), to (k1), to+1 (k0); k2 / k0 are absent at the ends of the clip
      if (to >= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { best[e] = k2[r][e]; bi[e] = c2[r][e]; }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k1[r][e] > best[e]) { best[e] = k1[r][e]; bi[e] = 9u + c1[r][e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { best[e] = k1[r][e]; bi[e] = 9u + c1[r][e]; }
      }
      if (t < a.T) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0[r][e] > best[e]) { best[e] = k0[r][e]; bi[e] = 18u + c0[r][e]; }
      }
      const int cc0 = (tl.cv0 * Q + (it - px * PT::QV)) * 4;
      uint32_t ov[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = (cc0 + e < a.C) ? unkey_f32(best[e]) : 0u;
      const int64_t m = ((int64_t)(tl.n * a.T + to) * a.H + h) * a.W + w;
      if constexpr (Q == 1)
        *reinterpret_cast<uint4*>(y + m * a.ldy + cc0) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
      else
        *reinterpret_cast<uint2*>(y + m * a.ldy + cc0) = make_uint2((ov[0] >> 16) | (ov[1] & 0xffff0000u), (ov[2] >> 16) | (ov[3] & 0xffff0000u));
      *reinterpret_cast<uint32_t*>(idx + m * a.CP + cc0) = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    }
  }
}

// acc[e] += g[e] for the elements whose tap byte in iw equals tap.  v_cmpx leaves the compare in EXEC, the add runs on the
// lanes it kept and EXEC comes back from a scalar copy: two vector instructions per element where the compiler's
// and / compare / add / select sequence takes four.
__device__ __forceinline__ void add_if_tap4(float (&acc)[4], const uint4& g, uint32_t iw, uint32_t tap) {
  uint64_t sv;
  asm volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "v_cmpx_eq_u32_sdwa vcc, %[iw], %[tap] src0_sel:BYTE_0 src1_sel:DWORD\n\t"
      "v_add_f32_e32 %[a0], %[a0], %[g0]\n\t"
      "s_mov_b64 exec, %[sv]\n\t"
      "v_cmpx_eq_u32_sdwa vcc, %[iw], %[tap] src0_sel:BYTE_1 src1_sel:DWORD\n\t"
      "v_add_f32_e32 %[a1], %[a1], %[g1]\n\t"
      "s_mov_b64 exec, %[sv]\n\t"
      "v_cmpx_eq_u32_sdwa vcc, %[iw], %[tap] src0_sel:BYTE_2 src1_sel:DWORD\n\t"
      "v_add_f32_e32 %[a2], %[a2], %[g2]\n\t"
      "s_mov_b64 exec, %[sv]\n\t"
      "v_cmpx_eq_u32_sdwa vcc, %[iw], %[tap] src0_sel:BYTE_3 src1_sel:DWORD\n\t"
      "v_add_f32_e32 %[a3], %[a3], %[g3]\n\t"
      "s_mov_b64 exec, %[sv]\n\t"
      : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [sv] "=&s"(sv)
      : [iw] "v"(iw), [tap] "s"(tap), [g0] "v"(g.x), [g1] "v"(g.y), [g2] "v"(g.z), [g3] "v"(g.w)
      : "vcc");
}

template <typename T, int TH, int TW, int CV>
__global__ __launch_bounds__(kThreads) void pool333_bwd_tile_kernel(PoolTileArgs a, const T* __restrict__ dy,
                                                                    const uint8_t* __restrict__ idx, T* __restrict__ dx) {
  constexpr int V = DT<T>::VEC, Q = V / 4;
  using PT = PoolTile<TH, TW, CV, Q>;
  __shared__ uint4 gring[3][PT::NLE];
  __shared__ uint32_t iring[3][PT::NLE];
  PT tl;
  if (!tl.locate(a)) return;
  const int tid = threadIdx.x;
  const int64_t plane = (int64_t)a.H * a.W;
  int64_t srow[PT::SR];
  int scv[PT::SR];
  bool sval[PT::SR];
#pragma unroll
  for (int s = 0; s < PT::SR; ++s) {
    int h, w;
    sval[s] = tl.stage_src(a, s * kThreads + tid, h, w, scv[s]);
    srow[s] = (int64_t)(tl.n * a.T) * a.H * a.W + (int64_t)h * a.W + w;
  }
  uint4 pre[PT::SR];
  uint32_t prei[PT::SR][Q];
  auto prefetch = [&](int t) {
#pragma unroll
    for (int s = 0; s < PT::SR; ++s) {
      const int64_t m = srow[s] + t * plane;
      pre[s] = sval[s] ? *reinterpret_cast<const uint4*>(dy + m * a.ldy + scv[s] * V) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int j = 0; j < Q; ++j)
        prei[s][j] = sval[s] ? reinterpret_cast<const uint32_t*>(idx + m * a.CP + scv[s] * V)[j] : 0xffffffffu;
    }
  };
  auto commit = [&](int slot) {
#pragma unroll
    for (int s = 0; s < PT::SR; ++s) {
      const int i = s * kThreads + tid;
      if (i >= PT::NST) break;
      if constexpr (Q == 1) {
        gring[slot][i] = pre[s];
        iring[slot][i] = prei[s][0];
      } else {
        uint4 q0, q1;
        widen_bf16x8(pre[s], q0, q1);
        gring[slot][2 * i] = q0; gring[slot][2 * i + 1] = q1;
        iring[slot][2 * i] = prei[s][0]; iring[slot][2 * i + 1] = prei[s][1];
      }
    }
  };
  auto compute = [&](int ti) {
#pragma unroll
    for (int r = 0; r < PT::R; ++r) {
      int ph, pw, ql;
      if (!tl.item(a, r * kThreads + tid, ph, pw, ql)) continue;
      const int c0 = (tl.cv0 * Q + ql) * 4;
      const int64_t m = ((int64_t)(tl.n * a.T + ti) * a.H + tl.h0 + ph) * a.W + tl.w0 + pw;
      T* dst = dx + m * a.ldx + c0;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.accumulate) {
        if constexpr (Q == 1) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(dst);
          acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w;
        } else {
          const uint2 v = *reinterpret_cast<const uint2*>(dst);
          acc[0] = __uint_as_float(v.x << 16); acc[1] = __uint_as_float(v.x & 0xffff0000u);
          acc[2] = __uint_as_float(v.y << 16); acc[3] = __uint_as_float(v.y & 0xffff0000u);
        }
      }
      // window (dh, dw) of this input pixel is the output at tile offset (ph + 1 - dh, pw + 1 - dw), i.e. halo pixel
      // (ph + 2 - dh, pw + 2 - dw): offsets from the tile-corner base stay non-negative (immediate LDS offsets)
      const int base = (ph * PT::HW + pw) * PT::QV + ql;
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const int to = ti + 1 - dt;
        if (to < 0 || to >= a.T) continue;
        const uint4* gs = gring[to % 3] + base;
        const uint32_t* is = iring[to % 3] + base;
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
#pragma unroll
          for (int dw = 0; dw < 3; ++dw) {
            const int o = ((2 - dh) * PT::HW + (2 - dw)) * PT::QV;
            add_if_tap4(acc, gs[o], is[o], (uint32_t)(dt * 9 + dh * 3 + dw));
          }
      }
      if constexpr (Q == 1) {
        f32x4 v = {acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(dst) = v;
      } else {
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        bf16x4 v = {(bf16_t)acc[0], (bf16_t)acc[1], (bf16_t)acc[2], (bf16_t)acc[3]};
        *reinterpret_cast<bf16x4*>(dst) = v;
      }
    }
  };
  prefetch(0);
  for (int t = 0; t <= a.T; ++t) {
    if (t < a.T) commit(t % 3);
    if (t + 1 < a.T) prefetch(t + 1);
    __syncthreads();
    if (t >= 1) compute(t - 1);
    __syncthreads();
  }
}

static bool pool333_shape(const dv_pool_desc* d) {
  return d->kt == 3 && d->kh == 3 && d->kw == 3 && d->st == 1 && d->sh == 1 && d->sw == 1 && d->pt == 1 && d->ph == 1 &&
         d->pw == 1;
}
// tile geometry for a staged launch; false when the plane is too small to be worth a tile (the gather kernels run then)
static bool pool_tile_args(const PoolArgs& p, int V, int TH, int TW, int CV, int accumulate, PoolTileArgs& a) {
  if (p.Hi * p.Wi < 25) return false;
  a.N = p.N; a.T = p.Ti; a.H = p.Hi; a.W = p.Wi; a.C = p.C; a.CP = p.CP; a.ldx = p.ldx; a.ldy = p.ldy;
  a.nth = (p.Hi + TH - 1) / TH; a.ntw = (p.Wi + TW - 1) / TW; a.cpv = p.CP / V; a.ncc = (a.cpv + CV - 1) / CV;
  const int64_t groups = (int64_t)p.N * a.nth * a.ntw * a.ncc;
  if (groups >= (1ll << 28)) return false;
  a.groups = (uint32_t)groups; a.per_xcd = (uint32_t)((groups + 7) / 8);
  a.fcc = make_fastdiv((uint32_t)a.ncc); a.ftw = make_fastdiv((uint32_t)a.ntw); a.fth = make_fastdiv((uint32_t)a.nth);
  a.accumulate = accumulate;
  return true;
}
// Tile width / channel vectors per workgroup.  Measured on the 14x14 and 7x7 pools of S3D-G (tools/pool_sweep.sh): the
// backward is occupancy-bound (three-plane ring of dy + idx), so it takes the 7-wide tile and 64 bytes of dy per pixel; the
// forward (two single-plane slots) is flat between the shapes.
static int pool_tile_tw(int W, bool narrow) { return (W <= 7 || narrow) ? 7 : 14; }

}  // namespace

static int pool_args(const dv_pool_desc* d, PoolArgs& a) {
  if (!d) return DV_EINVAL;
  if (d->N <= 0 || d->C <= 0 || d->kt <= 0 || d->kh <= 0 || d->kw <= 0 || d->st <= 0 || d->sh <= 0 || d->sw <= 0) return DV_EINVAL;
  if (d->kt * d->kh * d->kw > 255) return DV_EUNSUPPORTED;
  if ((d->Ti + 2 * d->pt - d->kt) / d->st + 1 != d->To || (d->Hi + 2 * d->ph - d->kh) / d->sh + 1 != d->Ho ||
      (d->Wi + 2 * d->pw - d->kw) / d->sw + 1 != d->Wo) return DV_EINVAL;
  if (2 * d->pt > d->kt || 2 * d->ph > d->kh || 2 * d->pw > d->kw) return DV_EINVAL;
  a.N = d->N; a.Ti = d->Ti; a.Hi = d->Hi; a.Wi = d->Wi; a.C = d->C; a.CP = cp8(d->C);
  a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo;
  a.kt = d->kt; a.kh = d->kh; a.kw = d->kw; a.st = d->st; a.sh = d->sh; a.sw = d->sw;
  a.pt = d->pt; a.ph = d->ph; a.pw = d->pw; a.ldx = d->ldx; a.ldy = d->ldy;
  if (a.ldx < a.CP || a.ldy < a.CP) return DV_EINVAL;
  const int V = d->dtype == DV_F32 ? 4 : 8;
  if (a.ldx % V || a.ldy % V) return DV_EALIGN;
  if (d->st > 2 || d->sh > 2 || d->sw > 2) return DV_EUNSUPPORTED;
  if ((int64_t)a.N * a.Ti * a.Hi * a.Wi * (a.CP / V) >= (1ll << 31)) return DV_EINVAL;
  a.fcv = make_fastdiv((uint32_t)(a.CP / V));
  a.fWo = make_fastdiv((uint32_t)a.Wo); a.fHo = make_fastdiv((uint32_t)a.Ho); a.fTo = make_fastdiv((uint32_t)a.To);
  a.fWi = make_fastdiv((uint32_t)a.Wi); a.fHi = make_fastdiv((uint32_t)a.Hi); a.fTi = make_fastdiv((uint32_t)a.Ti);
  return DV_OK;
}

// The ONE place that picks a pool launch (dv_maxpool3d_route answers from it, dv_maxpool3d_fwd / _bwd launch what it says):
// 0 = per-element gather kernel, 1 = 2x2-quad backward, 2 = LDS-staged 3x3x3 tile (ta, tw, cv filled).  idx_aligned: idx is
// 8-byte aligned (the quad and staged kernels read it in 32-bit words).
enum { kPoolGather = 0, kPoolQuad = 1, kPoolTile = 2 };
static int pool_route(const dv_pool_desc* d, const PoolArgs& a, bool bwd, bool idx_aligned, int accumulate, PoolTileArgs& ta,
                      int& tw, int& cv) {
  tw = cv = 0;
  if (pool333_shape(d) && idx_aligned) {
    const int V = d->dtype == DV_F32 ? 4 : 8;
    const int cv_ = bwd && d->dtype == DV_BF16 ? 2 : 4;
    const int tw_ = pool_tile_tw(a.Wi, bwd || d->dtype == DV_BF16);
    if (pool_tile_args(a, V, 7, tw_, cv_, accumulate, ta)) {
      tw = tw_; cv = cv_;
      return kPoolTile;
    }
  }
  if (bwd && a.kh == 3 && a.kw == 3 && a.sh == 2 && a.sw == 2 && a.ph == 1 && a.pw == 1 && idx_aligned) return kPoolQuad;
  return kPoolGather;
}

extern "C" int dv_maxpool3d_route(const dv_pool_desc* d, int32_t bwd, int32_t* tile_w, int32_t* chunk_vecs) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (d->dtype != DV_F32 && d->dtype != DV_BF16) return DV_EINVAL;
  PoolTileArgs ta;
  int tw, cv;
  const int route = pool_route(d, a, bwd != 0, true, 0, ta, tw, cv);
  if (route == kPoolTile) {
    if (tile_w) *tile_w = tw;
    if (chunk_vecs) *chunk_vecs = cv;
  }
  return route;
}

extern "C" int dv_maxpool3d_fwd(const dv_pool_desc* d, const void* x, void* y, uint8_t* idx, void* stream) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (!x || !y || !idx) return DV_EINVAL;
  if (!aligned16(x) || !aligned16(y) || (reinterpret_cast<uintptr_t>(idx) & 7)) return DV_EALIGN;
  PoolTileArgs ta;
  int tw, cv;
  if (pool_route(d, a, false, true, 0, ta, tw, cv) == kPoolTile) {
#define POOL_FWD_TILE(TW_, CV_)                                                                                             \
  DISPATCH_T(d->dtype, {                                                                                                     \
    if (cv == CV_ && tw == TW_) {                                                                                            \
      hipLaunchKernelGGL((pool333_fwd_tile_kernel<T, 7, TW_, CV_>), dim3(8 * ta.per_xcd), dim3(kThreads), 0, ST(stream), ta, \
                         (const T*)x, (T*)y, idx);                                                                           \
      return dv_launch_status();                                                                                             \
    }                                                                                                                        \
  })
    POOL_FWD_TILE(7, 2); POOL_FWD_TILE(7, 4); POOL_FWD_TILE(7, 8);
    POOL_FWD_TILE(14, 2); POOL_FWD_TILE(14, 4); POOL_FWD_TILE(14, 8);
#undef POOL_FWD_TILE
    return DV_EUNSUPPORTED;                       // (pool_route only names the tiles instantiated above)
  }
  DISPATCH_T(d->dtype, {
    const int64_t total = (int64_t)a.N * a.To * a.Ho * a.Wo * (a.CP / DT<T>::VEC);
    hipLaunchKernelGGL((maxpool_fwd_kernel<T>), dim3(grid8_for(total, 16384)), dim3(kThreads), 0, ST(stream), a, (const T*)x,
                       (T*)y, idx);
  });
  return dv_launch_status();
}

extern "C" int dv_maxpool3d_bwd(const dv_pool_desc* d, const void* dy, const uint8_t* idx, void* dx, int32_t flags,
                                void* stream) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (!dy || !dx || !idx) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(dx)) return DV_EALIGN;
  PoolTileArgs ta;
  int tw, cv;
  const int acc = (flags & DV_ACCUM) ? 1 : 0;
  const int route = pool_route(d, a, true, (reinterpret_cast<uintptr_t>(idx) & 7) == 0, acc, ta, tw, cv);
  if (route == kPoolTile) {
#define POOL_BWD_TILE(TW_, CV_)                                                                                             \
  DISPATCH_T(d->dtype, {                                                                                                     \
    if (cv == CV_ && tw == TW_) {                                                                                            \
      hipLaunchKernelGGL((pool333_bwd_tile_kernel<T, 7, TW_, CV_>), dim3(8 * ta.per_xcd), dim3(kThreads), 0, ST(stream), ta, \
                         (const T*)dy, idx, (T*)dx);                                                                         \
      return dv_launch_status();                                                                                             \
    }                                                                                                                        \
  })
    POOL_BWD_TILE(7, 2); POOL_BWD_TILE(7, 4); POOL_BWD_TILE(7, 8);
    POOL_BWD_TILE(14, 2); POOL_BWD_TILE(14, 4); POOL_BWD_TILE(14, 8);
#undef POOL_BWD_TILE
    return DV_EUNSUPPORTED;
  }
  if (route == kPoolQuad) {
    const int Hq = (a.Hi + 1) / 2, Wq = (a.Wi + 1) / 2;
    DISPATCH_T(d->dtype, {
      const int64_t total = (int64_t)a.N * a.Ti * Hq * Wq * (a.CP / DT<T>::VEC);
      hipLaunchKernelGGL((maxpool_bwd_quad_kernel<T>), dim3(grid8_for(total, 16384)), dim3(kThreads), 0, ST(stream), a,
                         make_fastdiv((uint32_t)Wq), make_fastdiv((uint32_t)Hq), (const T*)dy, idx, (T*)dx, acc);
    });
    return dv_launch_status();
  }
  DISPATCH_T(d->dtype, {
    const int64_t total = (int64_t)a.N * a.Ti * a.Hi * a.Wi * (a.CP / DT<T>::VEC);
    hipLaunchKernelGGL((maxpool_bwd_kernel<T>), dim3(grid8_for(total, 16384)), dim3(kThreads), 0, ST(stream), a, (const T*)dy,
                       idx, (T*)dx, acc);
  });
  return dv_launch_status();
}

extern "C" int dv_bn_apply_maxpool(const dv_pool_desc* d, const void* x, const float* scale, const float* shift, void* y,
                                   uint8_t* idx, void* stream) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (!x || !scale || !shift || !y || !idx) return DV_EINVAL;
  if (!aligned16(x) || !aligned16(y) || !aligned16(scale) || !aligned16(shift) || (reinterpret_cast<uintptr_t>(idx) & 7)) return DV_EALIGN;
  DISPATCH_T(d->dtype, {
    const int64_t total = (int64_t)a.N * a.To * a.Ho * a.Wo * (a.CP / DT<T>::VEC);
    hipLaunchKernelGGL((bn_apply_maxpool_kernel<T>), dim3(grid_for(total, 16384)), dim3(kThreads), 0, ST(stream), a, (const T*)x,
                       scale, shift, (T*)y, idx);
  });
  return dv_launch_status();
}

extern "C" int dv_bn_bwd_reduce_maxpool(const dv_pool_desc* d, const void* dy_pool, const uint8_t* idx, const void* x,
                                        const float* mean, const float* invstd, const float* scale, const float* shift,
                                        float* sums, int32_t n_rep, void* stream) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (!dy_pool || !idx || !x || !mean || !invstd || !scale || !shift || !sums || n_rep <= 0) return DV_EINVAL;
  if (!aligned16(dy_pool) || !aligned16(x) || !aligned16(mean) || !aligned16(invstd) || !aligned16(scale) || !aligned16(shift)) return DV_EALIGN;
  const int64_t M = (int64_t)a.N * a.Ti * a.Hi * a.Wi;
  const int blocks = dv_bn_bwd_blocks(M, a.C);
  const int64_t rpb = (M + blocks - 1) / blocks;
  DISPATCH_T(d->dtype, hipLaunchKernelGGL((bn_bwd_reduce_maxpool_kernel<T>), dim3(blocks), dim3(kThreads), 0, ST(stream), a,
                                          (const T*)dy_pool, idx, (const T*)x, mean, invstd, scale, shift, M, a.C, a.CP, rpb,
                                          sums, n_rep));
  return dv_launch_status();
}

extern "C" int dv_bn_bwd_apply_maxpool(const dv_pool_desc* d, const void* dy_pool, const uint8_t* idx, const void* x,
                                       const float* mean, const float* invstd, const float* gamma, const float* scale,
                                       const float* shift, const float* sums_global, int32_t rep_global, float inv_count,
                                       float dparam_scale, float* dgamma, float* dbeta, void* dx, int32_t lddx, void* stream) {
  PoolArgs a;
  int rc = pool_args(d, a);
  if (rc) return rc;
  if (!dy_pool || !idx || !x || !mean || !invstd || !gamma || !scale || !shift || !sums_global || !dx || rep_global <= 0) return DV_EINVAL;
  if ((dgamma == nullptr) != (dbeta == nullptr) || lddx < a.CP) return DV_EINVAL;
  if (!aligned16(dy_pool) || !aligned16(x) || !aligned16(dx)) return DV_EALIGN;
  if (5 * a.CP * 4 > 60 * 1024) return DV_EUNSUPPORTED;
  DISPATCH_T(d->dtype, {
    constexpr int V = DT<T>::VEC;
    if (lddx % V) return DV_EALIGN;
    const int64_t total = (int64_t)a.N * a.Ti * a.Hi * a.Wi * (a.CP / V);
    hipLaunchKernelGGL((bn_bwd_apply_maxpool_kernel<T>), dim3(grid_for(total, 2048)), dim3(kThreads), 5 * a.CP * sizeof(float),
                       ST(stream), a, (const T*)dy_pool, idx, (const T*)x, mean, invstd, gamma, scale, shift, sums_global,
                       rep_global, inv_count, dparam_scale, dgamma, dbeta, (T*)dx, lddx, (uint32_t)total, a.C, a.CP);
  });
  return dv_launch_status();
}
