// The small streaming kernels that belong to no larger subject: the NCDHW ingest, column fill / sum, addcmul, l2norm, ReLU
// backward, mean, the data gradient's weight repacking -- and the library's ABI version / device check.
// (BatchNorm: batchnorm.hip; pooling: pool.hip; gating: gate.hip; fp8: quantize.hip; whatever steps a parameter arena: optim.hip.)
#include "streaming.hpp"

namespace {

// ------------------------------------------------------------------ ingest
template <typename T>
__global__ void ingest_kernel(const float* __restrict__ x, T* __restrict__ y, int N, int C, int T_, int H, int W,
                              int64_t sxn, int ldy, const float* mean3, const float* istd3,
                              const int* perm, int n_seg, int pad, int Hp, int Wp) {
  const int64_t total = (int64_t)N * T_ * H * W;
  const int64_t plane = (int64_t)H * W;
  const int seg = n_seg > 0 ? T_ / n_seg : T_;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t hw = i % plane;
    int64_t nt = i / plane;
    int t = (int)(nt % T_);
    int n = (int)(nt / T_);
    int ts = t;
    if (perm) ts = perm[n * n_seg + t / seg] * seg + t % seg;
    const float* src = x + (int64_t)n * sxn + (int64_t)ts * plane + hw;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C && c < 4; ++c) {
      float a = src[(int64_t)c * T_ * plane];
      if (mean3) a = (a - mean3[c]) * istd3[c];
      v[c] = a;
    }
    // destination pixel inside the (optionally zero-bordered) [N*T][Hp][Wp] frame
    const int hh = (int)(hw / W), ww = (int)(hw - (int64_t)hh * W);
    T* dst = y + ((nt * Hp + hh + pad) * (int64_t)Wp + ww + pad) * ldy;
    if (sizeof(T) == 4) {
      f32x4 o = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(dst) = o;
    } else {
      typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
      bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
      *reinterpret_cast<bf16x4*>(dst) = o;
    }
  }
}

// partials [n_blocks][W] -> out[W] (+=): 32 columns x 8 row lanes per block
__global__ void reduce_rows_kernel(const float* __restrict__ part, int64_t ld, int n_rows, int Wd, float* __restrict__ out,
                                   int accumulate) {
  __shared__ float sh[8][33];
  const int col = blockIdx.x * 32 + (threadIdx.x & 31);
  const int rl = threadIdx.x >> 5;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < Wd) {
    int r = rl;
    for (; r + 24 < n_rows; r += 32) {
      a0 += part[(size_t)r * ld + col];
      a1 += part[(size_t)(r + 8) * ld + col];
      a2 += part[(size_t)(r + 16) * ld + col];
      a3 += part[(size_t)(r + 24) * ld + col];
    }
    for (; r < n_rows; r += 8) a0 += part[(size_t)r * ld + col];
  }
  sh[rl][threadIdx.x & 31] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (rl == 0 && col < Wd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += sh[i][threadIdx.x & 31];
    out[col] = accumulate ? out[col] + s : s;
  }
}

// ------------------------------------------------------------------ small fp32 helpers
// one wave per row
__global__ void l2norm_fwd_kernel(const float* __restrict__ x, int R, int D, float eps, float* __restrict__ y,
                                  float* __restrict__ norm) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) { float v = x[(size_t)row * D + d]; s += v * v; }
  s = wave_sum(s);
  const float nrm = fmaxf(sqrtf(s), eps);
  for (int d = lane; d < D; d += 64) y[(size_t)row * D + d] = x[(size_t)row * D + d] / nrm;
  if (lane == 0) norm[row] = nrm;
}
__global__ void l2norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                  const float* __restrict__ norm, int R, int D, float* __restrict__ dx) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += dy[(size_t)row * D + d] * y[(size_t)row * D + d];
  s = wave_sum(s);
  const float inv = 1.f / norm[row];
  for (int d = lane; d < D; d += 64)
    dx[(size_t)row * D + d] = (dy[(size_t)row * D + d] - y[(size_t)row * D + d] * s) * inv;
}
__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, int64_t n, float* __restrict__ dx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}
__global__ void mean_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
  __shared__ float sh[8];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = s / (float)n;
}

// ------------------------------------------------------------------ weight layout for the data gradient
// one block per (desc, input channel c): Wd[c][tap][n] = W[n][tap][c]
template <typename CT>
__global__ void pack_dgrad_kernel(const float* __restrict__ master, CT* __restrict__ dst,
                                  const dv_pack_desc* __restrict__ descs, const int* __restrict__ bmap) {
  const dv_pack_desc d = descs[bmap[2 * blockIdx.x]];
  const int c = bmap[2 * blockIdx.x + 1];
  const int rowlen = d.taps * d.cout_pitch;
  const float* src = master + d.src_off;
  CT* out = dst + d.dst_off + (int64_t)c * rowlen;
  for (int i = threadIdx.x; i < rowlen; i += blockDim.x) {
    const int tap = i / d.cout_pitch, n = i % d.cout_pitch;
    float v = 0.f;
    if (n < d.Cout) v = src[((int64_t)n * d.taps + tap) * d.cin_pitch + c];
    out[i] = (CT)v;
  }
}

}  // namespace

extern "C" int dv_abi_version(void) { return DV_ABI_VERSION; }

extern "C" int dv_check_device(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return DV_EUNSUPPORTED;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return DV_EUNSUPPORTED;
  const char* a = prop.gcnArchName;
  return (a[0] == 'g' && a[1] == 'f' && a[2] == 'x' && a[3] == '9' && a[4] == '5' && a[5] == '0') ? DV_OK : DV_EUNSUPPORTED;
}

extern "C" int dv_ingest_ncdhw(int32_t dtype, const float* x, void* y, int32_t N, int32_t C, int32_t T_, int32_t H,
                               int32_t W, int64_t sxn, int32_t ldy, const float* mean3, const float* istd3,
                               const int32_t* perm, int32_t n_seg, void* stream) {
  if (!x || !y || N <= 0 || C <= 0 || C > 4 || ldy < 4 || ldy % 4) return DV_EINVAL;
  if (perm && (n_seg <= 0 || T_ % n_seg)) return DV_EINVAL;
  if ((mean3 == nullptr) != (istd3 == nullptr)) return DV_EINVAL;
  const int64_t total = (int64_t)N * T_ * H * W;
  DISPATCH_T(dtype, hipLaunchKernelGGL((ingest_kernel<T>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream), x,
                                       (T*)y, N, C, T_, H, W, sxn, ldy, mean3, istd3, perm, n_seg, 0, H, W));
  return dv_launch_status();
}

extern "C" int dv_ingest_ncdhw_pad(int32_t dtype, const float* x, void* y, int32_t N, int32_t C, int32_t T_, int32_t H,
                                   int32_t W, int64_t sxn, int32_t ldy, const float* mean3, const float* istd3,
                                   const int32_t* perm, int32_t n_seg, int32_t pad, void* stream) {
  if (!x || !y || N <= 0 || C <= 0 || C > 4 || ldy < 4 || ldy % 4 || pad < 0) return DV_EINVAL;
  if (perm && (n_seg <= 0 || T_ % n_seg)) return DV_EINVAL;
  if ((mean3 == nullptr) != (istd3 == nullptr)) return DV_EINVAL;
  const int64_t total = (int64_t)N * T_ * H * W;
  DISPATCH_T(dtype, hipLaunchKernelGGL((ingest_kernel<T>), dim3(grid_for(total)), dim3(kThreads), 0, ST(stream), x,
                                       (T*)y, N, C, T_, H, W, sxn, ldy, mean3, istd3, perm, n_seg, pad, H + 2 * pad,
                                       W + 2 * pad));
  return dv_launch_status();
}

__global__ void fill_cols_kernel(float* __restrict__ p, int64_t rows, int pitch, int col0, int ncols, float v) {
  const int64_t total = rows * ncols;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ncols;
    p[r * pitch + col0 + (int)(i - r * ncols)] = v;
  }
}

extern "C" int dv_fill_cols_f32(float* p, int64_t rows, int32_t pitch, int32_t col0, int32_t ncols, float value, void* stream) {
  if (!p || rows <= 0 || ncols <= 0 || col0 < 0 || col0 + ncols > pitch) return DV_EINVAL;
  hipLaunchKernelGGL(fill_cols_kernel, dim3(grid_for(rows * ncols)), dim3(kThreads), 0, ST(stream), p, rows, pitch, col0, ncols,
                     value);
  return dv_launch_status();
}

__global__ void addcmul_kernel(float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b, float alpha, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += alpha * a[i] * (b ? b[i] : 1.f);
}

extern "C" int dv_addcmul_f32(float* y, const float* a, const float* b, float alpha, int32_t n, void* stream) {
  if (!y || !a || n <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(addcmul_kernel, dim3((n + 255) / 256), dim3(256), 0, ST(stream), y, a, b, alpha, n);
  return dv_launch_status();
}

extern "C" int dv_colsum_f32(const float* x, int32_t ldx, int32_t R, int32_t C, float* out, void* stream) {
  if (!x || !out || R <= 0 || C <= 0 || ldx < C) return DV_EINVAL;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3((C + 31) / 32), dim3(256), 0, ST(stream), x, (int64_t)ldx, R, C, out, 1);
  return dv_launch_status();
}
extern "C" int dv_l2norm_fwd(const float* x, int32_t R, int32_t D, float eps, float* y, float* norm, void* stream) {
  if (!x || !y || !norm || R <= 0 || D <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, ST(stream), x, R, D, eps, y, norm);
  return dv_launch_status();
}
extern "C" int dv_l2norm_bwd(const float* dy, const float* y, const float* norm, int32_t R, int32_t D, float* dx, void* stream) {
  if (!dy || !y || !norm || !dx || R <= 0 || D <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, ST(stream), dy, y, norm, R, D, dx);
  return dv_launch_status();
}
extern "C" int dv_relu_bwd_f32(const float* dy, const float* y, int64_t n, float* dx, void* stream) {
  if (!dy || !y || !dx || n <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ST(stream), dy, y, n, dx);
  return dv_launch_status();
}
extern "C" int dv_mean_f32(const float* x, int32_t n, float* out, void* stream) {
  if (!x || !out || n <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, ST(stream), x, n, out);
  return dv_launch_status();
}

extern "C" int dv_pack_dgrad_weights(int32_t dtype, const float* master, void* dst, const dv_pack_desc* descs,
                                     const int32_t* block_map, int32_t n_blocks, void* stream) {
  if (!master || !dst || !descs || !block_map || n_blocks <= 0) return DV_EINVAL;
  if (dtype == DV_BF16) hipLaunchKernelGGL((pack_dgrad_kernel<bf16_t>), dim3(n_blocks), dim3(kThreads), 0, ST(stream), master, (bf16_t*)dst, descs, block_map);
  else if (dtype == DV_F32) hipLaunchKernelGGL((pack_dgrad_kernel<float>), dim3(n_blocks), dim3(kThreads), 0, ST(stream), master, (float*)dst, descs, block_map);
  else return DV_EUNSUPPORTED;
  return dv_launch_status();
}
