// PIL-exact resample of decoded uint8 RGB frames (include/dualvar_hip.h: dv_resample_u8): the reference's A.Scale((128, 171)),
// i.e. PIL Image.resize((128, 171), BICUBIC) of every decoded frame (utils/augmentation.py:125-146), on the GPU.  Pillow's
// resample (src/libImaging/Resample.c) is integer arithmetic over coefficient tables it computes in float64; the tables come from
// the host (dualvar_amd/utils/resample.py restates that float64 code), so this file holds no float at all:
//   acc = 2^21 + sum_k w[k] * in[xmin + k]   (int32, 22-bit fixed-point weights)
//   out = clamp(acc >> 22, 0, 255)
// horizontal pass first, its result stored as uint8, then the vertical pass; a pass whose size does not change is skipped.
// One workgroup per (frame, band of kBand output rows).  The source rows the band's vertical taps reach are brought into LDS
// kChunk rows at a time with 16-byte loads, the horizontal pass turns each chunk into rows of the uint8 intermediate (also in
// LDS), and the vertical pass reads the intermediate four bytes at a time and writes the output rows.
#include <unordered_map>

#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kBand = 32;                  // output rows per workgroup
constexpr int kChunk = 8;                  // source rows staged per horizontal step
constexpr int kLdsMax = 64 * 1024;
constexpr int kHead = 4;                   // table header words {in, out, ksize, 0}

struct RsArgs {
  const uint8_t* src;
  const struct dv_resample_desc* desc;
  const int32_t* coef;
  uint8_t* out;
  int Ho, Wo, n_bands;
  int ip;                                  // intermediate row pitch in bytes: Wo * 3 rounded up to 4
  int stage_bytes;                         // LDS bytes in front of the intermediate (the staged source chunk)
  int max_rows;                            // intermediate rows the LDS holds
};

__device__ __forceinline__ uint8_t clip8(int32_t acc) {       // Pillow's clip8: clamp(acc >> 22, 0, 255), arithmetic shift
  const int32_t v = acc >> 22;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(kThreads) resample_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_rs[];
  const int f = blockIdx.x / a.n_bands, band = blockIdx.x - f * a.n_bands;
  const int tid = threadIdx.x;
  const struct dv_resample_desc d = a.desc[f];
  const int Hs = d.Hs, Ws = d.Ws, W3 = Ws * 3, Wo = a.Wo;
  const int r0 = band * kBand, r1 = min(r0 + kBand, a.Ho);
  const int32_t* ht = d.h_coef >= 0 ? a.coef + d.h_coef + kHead : nullptr;
  const int32_t* vt = d.v_coef >= 0 ? a.coef + d.v_coef + kHead : nullptr;
  const int hstride = ht ? 2 + a.coef[d.h_coef + 2] : 0, vstride = vt ? 2 + a.coef[d.v_coef + 2] : 0;

  // source rows [ry0, ry1) the band's vertical taps reach (validated on the host to lie inside the frame and to fit max_rows)
  int ry0 = r0, ry1 = r1;
  if (vt) {
    ry0 = 0x7fffffff; ry1 = 0;
    for (int r = r0; r < r1; ++r) {
      const int32_t* e = vt + (int64_t)r * vstride;
      ry0 = min(ry0, e[0]);
      ry1 = max(ry1, e[0] + e[1]);
    }
  }
  ry1 = min(ry1, min(Hs, ry0 + a.max_rows));             // no-ops for validated tables: a bad table cannot leave LDS or the frame

  uint8_t* stage = lds_rs;
  uint8_t* inter = lds_rs + a.stage_bytes;
  for (int c0 = ry0; c0 < ry1; c0 += kChunk) {
    const int c1 = min(c0 + kChunk, ry1);
    // rows [c0, c1) are contiguous in the frame; copy the 16-byte words that cover them (src_offset % 16 == 0 and the frame's
    // bytes rounded up to 16 lie inside src: checked by the entry)
    const int64_t s = d.src_offset + (int64_t)c0 * W3, e = d.src_offset + (int64_t)c1 * W3;
    const int64_t b0 = s & ~(int64_t)15;
    const int nv = (int)((((e + 15) & ~(int64_t)15) - b0) >> 4);
    const i32x4* gsrc = reinterpret_cast<const i32x4*>(a.src + b0);
    for (int v = tid; v < nv; v += kThreads) reinterpret_cast<i32x4*>(stage)[v] = gsrc[v];
    __syncthreads();
    const uint8_t* rows = stage + (int)(s - b0);
    const int px = (c1 - c0) * Wo;
    for (int i = tid; i < px; i += kThreads) {
      const int rr = i / Wo, x = i - rr * Wo;
      const uint8_t* line = rows + rr * W3;
      uint8_t* dst = inter + (c0 - ry0 + rr) * a.ip + x * 3;
      if (!ht) {                                        // Ws == Wo: no horizontal pass
        dst[0] = line[x * 3]; dst[1] = line[x * 3 + 1]; dst[2] = line[x * 3 + 2];
        continue;
      }
      const int32_t* t = ht + (int64_t)x * hstride;
      const int xmin = t[0], n = t[1];
      const uint8_t* p = line + xmin * 3;
      int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int k = 0; k < n; ++k) {
        const int32_t w = t[2 + k];
        s0 += (int32_t)p[3 * k] * w;
        s1 += (int32_t)p[3 * k + 1] * w;
        s2 += (int32_t)p[3 * k + 2] * w;
      }
      dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
    }
    __syncthreads();
  }

  // vertical pass: four consecutive bytes of an output row per work item (the intermediate's rows are padded to ip, so every
  // dword read is aligned; bytes past Wo * 3 are computed and dropped)
  const int ob = Wo * 3, nd = a.ip >> 2;
  uint8_t* orow0 = a.out + (int64_t)f * a.Ho * ob;
  for (int i = tid; i < (r1 - r0) * nd; i += kThreads) {
    const int rr = i / nd, q = i - rr * nd, r = r0 + rr;
    uint32_t word;
    if (!vt) {                                          // Hs == Ho: no vertical pass
      word = *reinterpret_cast<const uint32_t*>(inter + (r - ry0) * a.ip + 4 * q);
    } else {
      const int32_t* t = vt + (int64_t)r * vstride;
      const int y = t[0] - ry0, n = t[1];
      int32_t acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21, acc3 = 1 << 21;
      for (int k = 0; k < n; ++k) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(inter + (y + k) * a.ip + 4 * q);
        const int32_t w = t[2 + k];
        acc0 += (int32_t)(v & 255u) * w;
        acc1 += (int32_t)((v >> 8) & 255u) * w;
        acc2 += (int32_t)((v >> 16) & 255u) * w;
        acc3 += (int32_t)(v >> 24) * w;
      }
      word = (uint32_t)clip8(acc0) | ((uint32_t)clip8(acc1) << 8) | ((uint32_t)clip8(acc2) << 16) | ((uint32_t)clip8(acc3) << 24);
    }
    uint8_t* o = orow0 + (int64_t)r * ob + 4 * q;
    const int valid = min(4, ob - 4 * q);
    if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) = word;
    } else {
      for (int j = 0; j < valid; ++j) o[j] = (uint8_t)(word >> (8 * j));
    }
  }
}

// host check of one coefficient table at word offset t: {in, out, ksize, 0} + out entries {xmin, n, w[ksize]}; *rows = the most
// input lines one group of kBand consecutive entries reaches (for a vertical table: the rows one band stages)
bool check_table(const int32_t* coef, int64_t words, int64_t t, int in, int out, int* rows) {
  if (t < 0 || t + kHead > words) return false;
  const int32_t* h = coef + t;
  const int ksize = h[2];
  if (h[0] != in || h[1] != out || ksize < 1 || ksize > DV_RESAMPLE_MAX_KSIZE) return false;
  if (t + kHead + (int64_t)out * (2 + ksize) > words) return false;
  int most = 0;
  for (int b0 = 0; b0 < out; b0 += kBand) {
    int lo = in, hi = 0;
    for (int x = b0; x < out && x < b0 + kBand; ++x) {
      const int32_t* e = h + kHead + (int64_t)x * (2 + ksize);
      const int xmin = e[0], n = e[1];
      if (xmin < 0 || n < 1 || n > ksize || (int64_t)xmin + n > in) return false;
      lo = xmin < lo ? xmin : lo;
      hi = xmin + n > hi ? xmin + n : hi;
    }
    most = hi - lo > most ? hi - lo : most;
  }
  *rows = most;
  return true;
}

}  // namespace

extern "C" int dv_resample_u8(const uint8_t* src, int64_t src_bytes, const struct dv_resample_desc* desc,
                              const struct dv_resample_desc* host_desc, int32_t N, const int32_t* coef, const int32_t* host_coef, int64_t coef_words, uint8_t* out, int32_t Ho,
                              int32_t Wo, void* stream) {
  if (!src || !desc || !host_desc || !out || N <= 0 || Ho <= 0 || Wo <= 0 || src_bytes <= 0 || coef_words < 0) return DV_EINVAL;
  if (coef_words > 0 && (!coef || !host_coef)) return DV_EINVAL;
  if ((int64_t)Wo * 3 > kLdsMax || (int64_t)N * cdiv64(Ho, kBand) > 0x7fffffff) return DV_EINVAL;
  if (!aligned16(src)) return DV_EALIGN;
  const int ip = round_up(Wo * 3, 4);
  int max_rows = Ho < kBand ? Ho : kBand, max_w3 = 0;
  std::unordered_map<int64_t, int> seen;              // validated table offset -> rows per band (a batch shares a few tables)
  for (int32_t i = 0; i < N; ++i) {
    const struct dv_resample_desc& d = host_desc[i];
    if (d.Hs <= 0 || d.Ws <= 0 || (int64_t)d.Hs * d.Ws > (1ll << 28)) return DV_EINVAL;
    if (d.src_offset < 0) return DV_EINVAL;
    if (d.src_offset & 15) return DV_EALIGN;
    if (d.src_offset + (((int64_t)d.Hs * d.Ws * 3 + 15) & ~(int64_t)15) > src_bytes) return DV_EINVAL;
    const int w3 = d.Ws * 3;
    max_w3 = w3 > max_w3 ? w3 : max_w3;
    for (int pass = 0; pass < 2; ++pass) {
      const bool vertical = pass == 1;
      const int64_t t = vertical ? d.v_coef : d.h_coef;
      const int in = vertical ? d.Hs : d.Ws, o = vertical ? Ho : Wo;
      if (t == -1) {                                   // Pillow skips a pass whose size does not change, and only then
        if (in != o) return DV_EINVAL;
        continue;
      }
      auto it = seen.find(t);
      int rows = 0;
      if (it == seen.end()) {
        if (!check_table(host_coef, coef_words, t, in, o, &rows)) return DV_EINVAL;
        seen.emplace(t, rows);
      } else {
        const int32_t* h = host_coef + t;              // validated before, but perhaps for the other direction / other sizes
        if (h[0] != in || h[1] != o) return DV_EINVAL;
        rows = it->second;
      }
      if (vertical) max_rows = rows > max_rows ? rows : max_rows;
    }
  }
  RsArgs a;
  a.src = src; a.desc = desc; a.coef = coef; a.out = out;
  a.Ho = Ho; a.Wo = Wo; a.n_bands = (int)cdiv64(Ho, kBand); a.ip = ip; a.max_rows = max_rows;
  a.stage_bytes = round_up(kChunk * max_w3 + 32, 16);
  const int64_t lds = (int64_t)a.stage_bytes + (int64_t)max_rows * ip;
  if (lds > kLdsMax) return DV_EINVAL;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(N * a.n_bands)), dim3(kThreads), (size_t)lds, (hipStream_t)stream, a);
  return dv_launch_status();
}
