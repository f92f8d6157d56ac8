// The forward / data-gradient convolution as implicit GEMM on the gfx950 matrix cores: conv_gemm_kernel, conv_gemm_ks_kernel (K
// split over the waves) and the ladders that name their instantiations.  Nothing is decided here: conv.hip's route says which form
// runs and launches it through the dvg_ functions of conv_gemm_fwd.hip / conv_gemm_dgrad.hip, which instantiate this header for
// one MODE each (two translation units: its 141 kernels are most of the library's compile time).
// One gather routine serves all three convolution kernels: a tile of the (virtual) im2col matrix A[row m][k = tap*CP + c] is built
// from 16-byte (8-byte for the 3->4-channel stem) vectors, each lying inside one tap.  fwd/dgrad read it K-contiguous (ds_read_b128).
// MFMA: v_mfma_f32_32x32x16_bf16 (bf16 storage) / v_mfma_f32_32x32x2_f32 (f32 parity mode);
// both share the 32x32 C/D layout  col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
#pragma once
#include "conv_common.hpp"

namespace {
// ------------------------------------------------------------------------------------------
// fwd / dgrad kernel.  256 threads = 4 waves arranged WAVES_M x WAVES_N over a BM x BN tile.
// LDS rows hold 64 bytes of K, padded to 80 so that ds_read_b128 fragments are conflict free.
// GM (gather mode): 0 = generic (a K-step may straddle taps; per-lane tap decode through the LDS tap table);
// 1 = uniform tap (channel pitch a multiple of the K-step, <= 32 taps, DMA path): the tap, its source offset and the
// K offset are wave-uniform and live in SGPRs, the separable validity masks are folded into ONE inverted bit mask per
// row in the prologue, and a gather address costs three VALU instructions (add, bfe, lshl_or) instead of ~12 -- the K
// loop was issue bound on exactly that address arithmetic (VALU ~ half of all issued cycles in the PMC profile).
// NS: LDS stages of the DMA pipeline (tiles k+1 .. k+NS-1 are in flight while tile k is multiplied; counted vmcnt).
// Waves per SIMD the register allocator is asked to make room for (the LDS footprint allows that many workgroups; the
// K loop is issue bound and resident waves are what hides it): 6 for the 128x64 / 64x128 bf16 tiles (<= 80 VGPRs instead
// of 84-88), 3 for 128x128 (<= 168 instead of 172), no request otherwise.
constexpr int conv_waves_per_simd(int es, int gvb, int bm, int bn) {
  return (es == 4 && gvb == 16 && bm == 256) ? 3 : (es != 2 || gvb != 16) ? 1 : (bm * bn == 128 * 64) ? 6 : (bm == 128 && bn == 128) ? 3 : 1;
}

// WF (fp32 split mode): the weights arrive PRE-SPLIT in fragment order (dv_pack_w3: [K tile][k half h][row][hi|mid|lo][8]
// bf16, 48 bytes per (row, h)), so a B tile is two contiguous chunks that the DMA copies as they are and a lane's three
// operand fragments are three conflict-free ds_read_b128 -- no vector instruction is spent on the weight operand; only
// the activation fragments are split in the kernel (the kernel was bound by exactly those instructions).
// BNL (dv_conv3d_fwd_bn_in): the gathered tensor is the INPUT of the BatchNorm (+ReLU) in front of this conv; the A fragments are
// y = [relu](x * scale + shift) formed between the LDS read and the split (coefficients in a small LDS table, one inverted tap
// mask per fragment row: a tap that leaves the tensor is a ZERO of y, not [relu](shift)).
template <typename T, int MODE, int GVB, int BM, int BN, int WAVES_M, int WAVES_N, int GM, int NS = 2, bool SPLIT = false,
          bool WF = false, bool BNL = false>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64)
__attribute__((amdgpu_waves_per_eu(conv_waves_per_simd(sizeof(T), GVB, BM, BN)))) void conv_gemm_kernel(ConvArgs a) {
  static_assert(!SPLIT || sizeof(T) == 4, "the bf16 split is the fp32 mode's product");
  static_assert(!WF || (SPLIT && GVB == 16), "pre-split weights belong to the fp32 split kernels");
  static_assert(!BNL || (WF && GM == 1 && MODE == MODE_FWD), "BatchNorm on load: forward, uniform-tap gathers, pre-split weights");
  // DMA: 16-byte gathers go global -> LDS directly (buffer_load ... lds), no VGPR staging and no ds_write.  One wave
  // instruction fills 16 rows x 64 B = 1 KiB of a row-linear, UNPADDED tile; bank conflicts of the ds_read_b128 fragment
  // reads are avoided by XOR-swizzling the 16-byte slot with (row>>2)&3, applied on the source side (which k-slot a
  // lane fetches) and on the read side.  The 8-byte-gather instantiation (RGB stem) keeps register staging + padding.
  constexpr bool DMA = (GVB == 16);
  static_assert(GM == 0 || DMA, "uniform-tap gathers are DMA only");
  constexpr int ROWB = 64, PITCH = DMA ? 64 : 80;
  constexpr int BKE = ROWB / (int)sizeof(T);
  constexpr int GV = GVB / (int)sizeof(T);
  constexpr int VPR = ROWB / GVB;           // vectors per row (4 or 8)
  constexpr int NT = WAVES_M * WAVES_N * 64; // threads
  constexpr int RPP = NT / VPR;             // rows per pass
  constexpr int A_PASSES = BM / RPP;
  constexpr int B_PASSES = (BN + RPP - 1) / RPP;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  static_assert(BN <= NT && BM % RPP == 0, "tile / thread layout");
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int A_G = DMA ? (BM / 16) / NW : A_PASSES;          // 16-row groups of the A tile per wave
  constexpr int BROWB = WF ? 96 : PITCH;                       // bytes of one B row in LDS (WF: hi|mid|lo of both k halves)
  constexpr int BPC = (BN * BROWB + 1023) / 1024;              // 1 KiB DMA pieces of the B tile
  constexpr int B_G = DMA ? (BPC + NW - 1) / NW : B_PASSES;
  static_assert(!DMA || (BM / 16) % NW == 0, "A groups per wave");
  static_assert(TM >= 1 && TN >= 1, "tile");
  typedef typename VecB<GVB>::type vec_t;

  static_assert(NS == 2 || GVB == 16, "deeper pipelines are DMA only");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * (BM * PITCH + BPC * 1024)];
  constexpr int BUFB = BM * PITCH + BPC * 1024;   // A tile then B tile, NS times

  const ConvGeom& g = a.g;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int lbid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_n = lbid % a.ntn, tile_m = lbid / a.ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;

  // register-staged path: thread -> (vector slot, row); DMA path: lane -> (row within a 16-row group, swizzled slot)
  const int uwave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int vslot = DMA ? ((lane & 3) ^ ((lane >> 4) & 3)) : tid % VPR;
  const int vrow = DMA ? (lane >> 2) : tid / VPR;
  auto a_row_of = [&](int p) { return DMA ? 16 * (uwave + p * NW) + vrow : vrow + p * RPP; };
  auto b_row_of = [&](int p) { return DMA ? 16 * (uwave + p * NW) + vrow : vrow + p * RPP; };
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  constexpr int ES = (int)sizeof(T);
  constexpr unsigned kOOB = 0x80000000u;      // beyond every buffer (tensors are < 2 GiB): the load returns zeros

  // ---- gather set-up -------------------------------------------------------------------------------------------
  // The K loop used to spend ~50 scalar/vector instructions and 19 branches per MFMA on coordinate arithmetic and
  // zero-fill selects.  Now: (1) loads go through buffer descriptors, so an invalid tap is just an out-of-range
  // offset and the hardware returns zeros (no branch, no select); (2) tap validity is separable, valid(dt,dh,dw) =
  // vt(dt)&vh(dh)&vw(dw), kept as three small bit masks per row; (3) the source offset of a tap is linear in the tap
  // (for dgrad with stride 2 in the halved coordinates), looked up from a per-kernel LDS table.
  __shared__ int2 taptab[256];
  const int ntaps = g.kt * g.kh * g.kw;
  {
    const int st_s = g.st - 1, sh_s = g.sh - 1, sw_s = g.sw - 1;     // strides are 1 or 2 on the dgrad path
    for (int tp = tid; tp < ntaps; tp += NT) {
      const int dw = tp % g.kw, t2 = tp / g.kw, dh = t2 % g.kh, dt = t2 / g.kh;
      const int toff = MODE == MODE_FWD ? (dt * g.sH + dh) * g.sW + dw
                                        : -(((dt >> st_s) * g.sH + (dh >> sh_s)) * g.sW + (dw >> sw_s));
      const int otap = a.cls_on ? ((a.crt + a.cst * dt) * a.oKH + a.crh + a.csh * dh) * a.oKW + a.crw + a.csw * dw : tp;
      taptab[tp] = make_int2(toff, dt | (dh << 8) | (dw << 16) | (otap << 24));
    }
  }
  const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.src), 0, a.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, a.w_bytes, 0x00020000);
  const dma_rsrc_t src_dma = dma_make_rsrc(a.src, (unsigned)a.src_bytes), w_dma = dma_make_rsrc(a.w, (unsigned)a.w_bytes);
  const unsigned smem_base = lds_addr(smem);
  const unsigned ldb = (unsigned)a.lds_ * ES;

  unsigned rowoff[A_G], mt[A_G], mh[A_G], mw[A_G];
#pragma unroll
  for (int p = 0; p < A_G; ++p) {
    const RowPos r = decode_row<MODE>((uint32_t)(m0 + a_row_of(p)), a.M, g);
    unsigned bt = 0, bh = 0, bw = 0;
    int pos;
    if (MODE == MODE_FWD) {
      for (int d = 0; d < g.kt; ++d) bt |= ((unsigned)(r.t0 + d) < (unsigned)g.sT ? 1u : 0u) << d;
      for (int d = 0; d < g.kh; ++d) bh |= ((unsigned)(r.h0 + d) < (unsigned)g.sH ? 1u : 0u) << d;
      for (int d = 0; d < g.kw; ++d) bw |= ((unsigned)(r.w0 + d) < (unsigned)g.sW ? 1u : 0u) << d;
      pos = r.base + (r.t0 * g.sH + r.h0) * g.sW + r.w0;
    } else {
      const int st_s = g.st - 1, sh_s = g.sh - 1, sw_s = g.sw - 1;
      for (int d = 0; d < g.kt; ++d) { int v = r.t0 - d; bt |= ((v >= 0 && !(v & st_s) && (v >> st_s) < g.sT) ? 1u : 0u) << d; }
      for (int d = 0; d < g.kh; ++d) { int v = r.h0 - d; bh |= ((v >= 0 && !(v & sh_s) && (v >> sh_s) < g.sH) ? 1u : 0u) << d; }
      for (int d = 0; d < g.kw; ++d) { int v = r.w0 - d; bw |= ((v >= 0 && !(v & sw_s) && (v >> sw_s) < g.sW) ? 1u : 0u) << d; }
      pos = r.base + ((r.t0 >> st_s) * g.sH + (r.h0 >> sh_s)) * g.sW + (r.w0 >> sw_s);
    }
    if (!r.valid) bt = 0;
    mt[p] = bt; mh[p] = bh; mw[p] = bw;
    rowoff[p] = (unsigned)pos * ldb;           // modulo 2^32; exact for every valid (row, tap)
  }
  unsigned woff[B_G];
#pragma unroll
  for (int p = 0; p < B_G; ++p) {
    if constexpr (WF) {
      // LDS byte o of the B region <- W3 byte (h * NPad + n0) * 48 + (o mod BN*48), h = o / (BN*48); a.ldw carries NPad
      const unsigned o = (unsigned)(uwave + p * NW) * 1024u + (unsigned)lane * 16u;
      const unsigned hh = o / (BN * 48u), rem = o - hh * (BN * 48u);
      woff[p] = o < BN * 96u ? (hh * (unsigned)a.ldw + (unsigned)n0) * 48u + rem : kOOB;
    } else {
      const int r = b_row_of(p), n = n0 + r;
      woff[p] = (r < BN && n < a.N) ? (unsigned)n * (unsigned)a.ldw * ES : kOOB;
    }
  }
  // uniform-tap mode: wave-uniform K cursor (next tile to load) and per-row inverted tap masks
  int u_c0 = 0, u_tap = 0, u_dt = 0, u_dh = 0, u_dw = 0;
  int u_otap = a.cls_on ? (a.crt * a.oKH + a.crh) * a.oKW + a.crw : 0;     // weight tap of class tap 0
  unsigned u_toffb = 0;                        // source byte offset of the current tap relative to tap 0
  unsigned imask[A_G];
  if constexpr (GM == 1) {
#pragma unroll
    for (int p = 0; p < A_G; ++p) {
      unsigned inv = 0;
      int tp = 0;
      for (int dt = 0; dt < g.kt; ++dt)
        for (int dh = 0; dh < g.kh; ++dh)
          for (int dw = 0; dw < g.kw; ++dw, ++tp)
            inv |= ((((mt[p] >> dt) & (mh[p] >> dh) & (mw[p] >> dw)) & 1u) ^ 1u) << tp;
      imask[p] = inv;
      rowoff[p] += (unsigned)vslot * GVB;
    }
#pragma unroll
    for (int p = 0; p < B_G; ++p)
      if (!WF && woff[p] != kOOB) woff[p] += (unsigned)vslot * GVB;
  }
  // BNL: scale | shift of the gathered channels (pad lanes: 0, 0) and the inverted tap masks of this lane's FRAGMENT rows
  constexpr int kBnlC = 256;
  float* bncoef = nullptr;
  unsigned cmask[TM];
  int c_c0 = 0, c_tap = 0;                     // wave-uniform K cursor of the tile being multiplied
  if constexpr (BNL) {
    __shared__ __attribute__((aligned(16))) float bntab[2 * kBnlC];
    bncoef = bntab;
    for (int c = tid; c < g.CP; c += NT) {
      bntab[c] = c < a.in_C ? a.in_scale[c] : 0.f;
      bntab[kBnlC + c] = c < a.in_C ? a.in_shift[c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const RowPos r = decode_row<MODE>((uint32_t)(m0 + wm0 + i * 32 + l31), a.M, g);
      unsigned inv = 0;
      int tp = 0;
      for (int dt = 0; dt < g.kt; ++dt)
        for (int dh = 0; dh < g.kh; ++dh)
          for (int dw = 0; dw < g.kw; ++dw, ++tp) {
            const bool ok = r.valid && (unsigned)(r.t0 + dt) < (unsigned)g.sT && (unsigned)(r.h0 + dh) < (unsigned)g.sH &&
                            (unsigned)(r.w0 + dw) < (unsigned)g.sW;
            inv |= (ok ? 0u : 1u) << tp;
          }
      cmask[i] = inv;
    }
  }
  __syncthreads();                             // taptab (and the coefficient table)

  const int nk = (g.Ktot + BKE - 1) / BKE;
  vec_t ra[A_G], rb[B_G];

  // gload(tile, buf): register-staged -> ra/rb (buf ignored); DMA -> straight into LDS buffer `buf`
  auto gload = [&](int kt_idx, int buf) {
    if constexpr (GM == 1) {
      const unsigned s_a = u_toffb + (unsigned)u_c0 * ES;
#pragma unroll
      for (int p = 0; p < A_G; ++p) {
        const unsigned off = ((__builtin_amdgcn_ubfe(imask[p], (unsigned)u_tap, 1u)) << 31) | (rowoff[p] + s_a);
        dma_load16(src_dma, smem_base + buf * BUFB + (uwave + p * NW) * 1024, off);
      }
      const unsigned s_b = (unsigned)(u_otap * g.CP + u_c0) * ES;
#pragma unroll
      for (int p = 0; p < B_G; ++p)
        if (uwave + p * NW < BPC)
          dma_load16(w_dma, smem_base + buf * BUFB + BM * PITCH + (uwave + p * NW) * 1024,
                     WF ? (woff[p] == kOOB ? kOOB : woff[p] + ((unsigned)(u_otap * g.CP + u_c0) / (unsigned)BKE) * (unsigned)a.ldw * 96u)
                        : woff[p] + s_b);                       // (WF: the K tile of the weights' own tap; == kt_idx unless taps are remapped)
      u_c0 += BKE;
      if (u_c0 >= g.CP) {
        u_c0 = 0;
        ++u_tap;
        if (++u_dw == g.kw) {
          u_dw = 0;
          if (++u_dh == g.kh) { u_dh = 0; ++u_dt; }
        }
        const int toff = MODE == MODE_FWD ? (u_dt * g.sH + u_dh) * g.sW + u_dw
                                          : -(((u_dt >> (g.st - 1)) * g.sH + (u_dh >> (g.sh - 1))) * g.sW + (u_dw >> (g.sw - 1)));
        u_toffb = (unsigned)toff * ldb;
        u_otap = a.cls_on ? ((a.crt + a.cst * u_dt) * a.oKH + a.crh + a.csh * u_dh) * a.oKW + a.crw + a.csw * u_dw : u_tap;
      }
      return;
    }
    const unsigned k = (unsigned)(kt_idx * BKE + vslot * GV);
    const unsigned tap = fd_div(k, a.fCP);
    const unsigned c = k - tap * (unsigned)g.CP;
    const bool tin = (int)tap < ntaps;
    const int2 ti = taptab[tin ? tap : 0];
    const unsigned dt = ti.y & 255, dh = (ti.y >> 8) & 255, dw = (ti.y >> 16) & 255, otap = (unsigned)ti.y >> 24;
    const unsigned tb = (unsigned)ti.x * ldb + c * ES;
#pragma unroll
    for (int p = 0; p < A_G; ++p) {
      const unsigned ok = (mt[p] >> dt) & (mh[p] >> dh) & (mw[p] >> dw) & (tin ? 1u : 0u);
      const unsigned off = ok ? rowoff[p] + tb : kOOB;
      if constexpr (DMA) {
        dma_load16(src_dma, smem_base + buf * BUFB + (uwave + p * NW) * 1024, off);
      } else if constexpr (GVB == 16) {
        u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(src_rsrc, off, 0, 0);
        ra[p] = make_uint4(v.x, v.y, v.z, v.w);
      } else {
        u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(src_rsrc, off, 0, 0);
        ra[p] = make_uint2(v.x, v.y);
      }
    }
    const unsigned kb = tin ? (otap * (unsigned)g.CP + c) * ES : kOOB;      // weights sit at the original tap index
#pragma unroll
    for (int p = 0; p < B_G; ++p) {
      const unsigned off = WF ? (woff[p] == kOOB ? kOOB : woff[p] + (unsigned)kt_idx * (unsigned)a.ldw * 96u)
                              : ((woff[p] | kb) >= kOOB ? kOOB : woff[p] + kb);
      if constexpr (DMA) {
        if (uwave + p * NW < BPC)
          dma_load16(w_dma, smem_base + buf * BUFB + BM * PITCH + (uwave + p * NW) * 1024, off);
      } else if constexpr (GVB == 16) {
        u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, off, 0, 0);
        rb[p] = make_uint4(v.x, v.y, v.z, v.w);
      } else {
        u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(w_rsrc, off, 0, 0);
        rb[p] = make_uint2(v.x, v.y);
      }
    }
  };
  auto lstore = [&](int buf) {
    if constexpr (!DMA) {
#pragma unroll
      for (int p = 0; p < A_G; ++p)
        *reinterpret_cast<vec_t*>(smem + buf * BUFB + (vrow + p * RPP) * PITCH + vslot * GVB) = ra[p];
#pragma unroll
      for (int p = 0; p < B_G; ++p) {
        int r = vrow + p * RPP;
        if (r < BN) *reinterpret_cast<vec_t*>(smem + buf * BUFB + (BM + r) * PITCH + vslot * GVB) = rb[p];
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // 32-row fragment blocks start at multiples of 32, so (row>>2)&3 of a fragment row is (l31>>2)&3 for A and B alike
  const int swz = DMA ? ((l31 >> 2) & 3) : 0;
  auto compute = [&](int buf) {
    if constexpr (SPLIT) {
      // each fragment is split ONCE per K tile and used by TN (TM) blocks
      Split3 af[TM], bf[TN];
      if constexpr (BNL) {
        const f32x4* cs = reinterpret_cast<const f32x4*>(bncoef + c_c0 + 8 * h);
        const f32x4* ch = reinterpret_cast<const f32x4*>(bncoef + kBnlC + c_c0 + 8 * h);
        const f32x4 s0 = cs[0], s1 = cs[1], h0 = ch[0], h1 = ch[1];
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const unsigned char* row = smem + buf * BUFB + (wm0 + i * 32 + l31) * PITCH;
          const f32x4 lo4 = *reinterpret_cast<const f32x4*>(row + ((2 * h) ^ swz) * 16);
          const f32x4 hi4 = *reinterpret_cast<const f32x4*>(row + ((2 * h + 1) ^ swz) * 16);
          float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
          // [relu] and "a tap outside the tensor is a zero of y" as ONE clamp per element: live rows [0 | -inf, +inf], dead rows [0, 0]
          const bool dead = (cmask[i] >> c_tap) & 1u;
          const float lo = (dead || a.in_relu) ? 0.f : -__builtin_inff(), hi = dead ? 0.f : __builtin_inff();
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e] * sc[e] + sh[e], lo, hi);      // dv_bn_apply's expression
          af[i] = split3(v);
        }
        c_c0 += BKE;
        if (c_c0 >= g.CP) { c_c0 = 0; ++c_tap; }
      } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = split3_row(smem + buf * BUFB + (wm0 + i * 32 + l31) * PITCH, h, swz);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (WF) {
          const unsigned char* pb = smem + buf * BUFB + BM * PITCH + ((h * BN + wn0 + j * 32 + l31) * 3) * 16;
          bf[j].hi = *reinterpret_cast<const bf16x8*>(pb);
          bf[j].mid = *reinterpret_cast<const bf16x8*>(pb + 16);
          bf[j].lo = *reinterpret_cast<const bf16x8*>(pb + 32);
        } else {
          bf[j] = split3_row(smem + buf * BUFB + (BM + wn0 + j * 32 + l31) * PITCH, h, swz);
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma_split3(af[i], bf[j], acc[i][j]);
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          Mma<T>::tile(smem + buf * BUFB + (wm0 + i * 32 + l31) * PITCH,
                       smem + buf * BUFB + (BM + wn0 + j * 32 + l31) * PITCH, h, swz, swz, acc[i][j]);
    }
  };
  if constexpr (DMA) {
    // pieces this wave issues per tile (the B groups may not divide evenly over the waves)
    int pieces = A_G;
#pragma unroll
    for (int p = 0; p < B_G; ++p) pieces += (uwave + p * NW < BPC) ? 1 : 0;
    constexpr int D = NS - 1;                  // prefetch distance
    for (int t = 0; t < D && t < nk; ++t) gload(t, t);
    int cur = 0, nxt = D % NS;                 // stage of tile k / of tile k + D
    for (int kt_idx = 0; kt_idx < nk; ++kt_idx) {
      dma_wait_upto(min(D - 1, nk - 1 - kt_idx) * pieces);   // tile k has landed (this wave's pieces)
      __syncthreads();                         // ... everybody's; and stage `nxt` (tile k-1) is no longer read
      if (kt_idx + D < nk) gload(kt_idx + D, nxt);
      compute(cur);
      cur = cur + 1 == NS ? 0 : cur + 1;
      nxt = nxt + 1 == NS ? 0 : nxt + 1;
    }
  } else {
    gload(0, 0);
    lstore(0);
    __syncthreads();
    for (int kt_idx = 0; kt_idx < nk; ++kt_idx) {
      const int cur = kt_idx & 1;
      if (kt_idx + 1 < nk) gload(kt_idx + 1, cur ^ 1);
      compute(cur);
      if (kt_idx + 1 < nk) lstore(cur ^ 1);
      __syncthreads();
    }
  }

  // ---------------- epilogue
  typedef typename OutOf<T>::type OT;           // what is stored (T, or bf16 for the fp8 GEMMs)
  OT* out = reinterpret_cast<OT*>(a.out);
  const int flags = a.flags;
  if constexpr (sizeof(T) == 1) {               // fp8 operands were scaled per tensor: undo it on the fp32 accumulators
    const float sc = a.sc_a[0] * a.sc_b[0];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= sc;
  }
  // row of the output tensor for row `m` of this launch (identity, or class sub-lattice -> full input: see ConvArgs)
  auto out_row = [&](int m) -> size_t {
    if (a.cls_on != 1) return (size_t)m;           // (2: taps remapped only -- trimmed window, rows are the tensor's)
    uint32_t q_, w_, h_, t_, n_;
    fd_divmod((uint32_t)m, g.dW, q_, w_);
    fd_divmod(q_, g.dH, q_, h_);
    fd_divmod(q_, g.dT, n_, t_);
    return ((size_t)(n_ * a.oT + t_ * a.cst + a.cot) * a.oH + h_ * a.csh + a.coh) * a.oW + w_ * a.csw + a.cow;
  };
  // BatchNorm partials of this tile (fwd + DV_STATS): per column the sum and M2 (about the tile mean) of the values AS
  // STORED, over valid rows.  One pass, fused into the conversion loop: each wave accumulates sum(v - c) and
  // sum((v - c)^2) about a provisional centre c = its first row's value (a sample of the column, so no cancellation
  // problem), which needs no second sweep over the accumulators -- keeping them alive for a two-pass M2 used to cost
  // the forward kernel 16..50 more VGPRs (one resident workgroup per CU less) than the otherwise identical dgrad.
  constexpr bool STATS_MODE = (MODE == MODE_FWD);
  const bool do_stats = STATS_MODE && (flags & DV_STATS);
  const int n_mt = (a.M + BM - 1) / BM;        // partials are stored [2][N][n_mt]: a channel's tiles are contiguous
  const bool full_tile = m0 + BM <= a.M;
  float st_c[TN], st_s1[TN], st_s2[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) st_c[j] = st_s1[j] = st_s2[j] = 0.f;
  auto stat_acc = [&](int i, int j, int r, float vs, int rl /* row inside the wave strip i */) {
    if constexpr (STATS_MODE) {
      if (i == 0 && r == 0) st_c[j] = __shfl(vs, l31);          // row 0 of the wave's rows (held by the h == 0 half)
      float d = vs - st_c[j];
      if (!full_tile && m0 + wm0 + i * 32 + rl >= a.M) d = 0.f;
      st_s1[j] += d;
      st_s2[j] = fmaf(d, d, st_s2[j]);
    }
  };
  {
    // Each wave stages a strip of its tile in LDS ([row][col], element writes at immediate offsets) and writes it out as
    // 16-byte vectors, a row segment per group of lanes -- instead of one element store and a 64-bit address computation per
    // element (the per-element form was ~1/3 of all instructions of the bf16 kernel, and for f32 -- 64 dword stores, 64
    // address chains and the row-mapping divisions per lane -- more than the K loop of the 1x1x1 layers).
    constexpr int EO = (int)sizeof(OT);
    constexpr int SP = WN * EO + 16;                 // staging row pitch (bytes)
    constexpr int CPR = WN * EO / 16;                // 16-byte chunks per strip row
    constexpr int EPC = 16 / EO;                     // elements per chunk
    constexpr int SROWS = (NW * 32 * SP <= (int)sizeof(smem)) ? 32 : 16;   // strip height that fits the tile buffers
    static_assert(NW * SROWS * SP <= (int)sizeof(smem), "staging fits the tile buffers");
    constexpr int RPS = SROWS / 2;                   // accumulator registers per strip (16 cover 32 rows)
    // fp32 outputs whose rows are the tensor's rows (no parity-class row map): straight from the accumulators.  One register
    // of a 32x32 block is 32 consecutive floats of a row per half wave (two 128-byte segments per store instruction: full
    // rate); the row of register r is a wave-uniform offset (soffset: scalar arithmetic only), the lane's part of the address
    // is fixed per column block.  FULL tiles only: the row term sits in soffset, which the buffer range check does NOT cover
    // (only voffset + the immediate offset are checked), so on a partial last tile rows >= M would be written behind the
    // tensor -- such tiles take the staged path below, which tests every row (the sentinel test is
    // tests/test_ops_gpu.py::test_fp32_partial_tiles_do_not_write_behind_the_output).  No LDS staging, no barrier, no
    // per-element address arithmetic (what made the per-element form of round 1 slow).
    bool direct = false;
    if constexpr (EO == 4) direct = full_tile && a.out_bytes > 0 && a.cls_on != 1;
    if (direct) {
      const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, a.out_bytes, 0x00020000);
      const unsigned ldo4 = (unsigned)a.ldo * 4u;
      const bool plain32 = !(flags & (DV_BIAS | DV_RELU | DV_SIGMOID));
      const unsigned rbase = (unsigned)(m0 + wm0 + 4 * h) * ldo4;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn0 + j * 32 + l31;
        const float bv = ((flags & DV_BIAS) && col < a.N) ? a.bias[col] : 0.f;
        const unsigned vo = col < a.NP ? rbase + (unsigned)col * 4u : 0x80000000u;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          unsigned old[16];
          if (flags & DV_ACCUM) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              old[r] = __builtin_amdgcn_raw_buffer_load_b32(orsrc, (int)vo, (int)((unsigned)(i * 32 + (r & 3) + 8 * (r >> 2)) * ldo4), 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rl = (r & 3) + 8 * (r >> 2);
            float v = acc[i][j][r];
            if (!plain32) {
              v = act_apply(v + bv, flags);
              if (col >= a.N) v = 0.f;
            }
            acc[i][j][r] = v;                        // as stored: feeds the two-pass statistics
            if (flags & DV_ACCUM) v += __builtin_bit_cast(float, old[r]);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), orsrc, (int)vo, (int)((unsigned)(i * 32 + rl) * ldo4), 0);
          }
        }
      }
    }
    if (!direct) {
    __syncthreads();                                 // every wave is done reading the last K tile
    unsigned char* stg = smem + wave * (SROWS * SP);
    const bool plain = EO == 2 && !(flags & (DV_BIAS | DV_RELU | DV_SIGMOID));
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int sub = 0; sub < 32 / SROWS; ++sub) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = n0 + wn0 + j * 32 + l31;
          const float bv = ((flags & DV_BIAS) && col < a.N) ? a.bias[col] : 0.f;
#pragma unroll
          for (int rr = 0; rr < RPS; ++rr) {
            const int r = sub * RPS + rr;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;          // row inside the 32-row block
            float v = acc[i][j][r];
            if (!plain) {                            // (plain: rows >= M and columns >= N are exact zeros already)
              v = act_apply(v + bv, flags);
              if (col >= a.N || m0 + wm0 + i * 32 + rl >= a.M) v = 0.f;
            }
            const OT tv = DT<OT>::from_f(v);
            *reinterpret_cast<OT*>(stg + (rl - sub * SROWS) * SP + (j * 32 + l31) * EO) = tv;
            if constexpr (EO == 2) {
              if (do_stats) stat_acc(i, j, r, DT<OT>::to_f(tv), rl);
            } else {
              acc[i][j][r] = v;                      // as stored (0 outside the valid region): feeds the two-pass statistics
            }
          }
        }
#pragma unroll
        for (int it = 0; it < (SROWS * CPR) / 64; ++it) {
          const int idx = it * 64 + lane;
          const int rl = idx / CPR, ch = idx % CPR;
          const int row = m0 + wm0 + i * 32 + sub * SROWS + rl, col0 = n0 + wn0 + ch * EPC;
          if (row < a.M && col0 < a.NP) {
            OT* p = out + out_row(row) * a.ldo + col0;
            if constexpr (EO == 2) {
              bf16x8 v = *reinterpret_cast<const bf16x8*>(stg + rl * SP + ch * 16);
              if (flags & DV_ACCUM) {
                const bf16x8 o = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (bf16_t)((float)v[e] + (float)o[e]);
              }
              *reinterpret_cast<bf16x8*>(p) = v;
            } else {
              f32x4 v = *reinterpret_cast<const f32x4*>(stg + rl * SP + ch * 16);
              if (flags & DV_ACCUM) v += *reinterpret_cast<const f32x4*>(p);
              *reinterpret_cast<f32x4*>(p) = v;
            }
          }
        }
      }
    }
    }   // !direct
  }

  if constexpr (STATS_MODE && sizeof(T) == 4) {
    // f32 parity mode: exact two-pass M2 about the tile mean (register pressure is no concern here)
    if (do_stats) {
      float* red = reinterpret_cast<float*>(smem);            // [WAVES_M][BN]
      float* meanb = red + WAVES_M * BN;                      // [BN]
      const int rows_here = min(BM, a.M - m0);
      const int wmi = wave / WAVES_N;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) s += acc[i][j][r];
        s += __shfl_xor(s, 32);
        if (h == 0) red[wmi * BN + wn0 + j * 32 + l31] = s;
      }
      __syncthreads();
      if (tid < BN) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_M; ++w) s += red[w * BN + tid];
        meanb[tid] = s / (float)rows_here;
        if (n0 + tid < a.N) a.stats[(size_t)(n0 + tid) * n_mt + tile_m] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float mu = meanb[wn0 + j * 32 + l31];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float dlt = acc[i][j][r] - mu;
            s += (row < a.M) ? dlt * dlt : 0.f;
          }
        s += __shfl_xor(s, 32);
        if (h == 0) red[wmi * BN + wn0 + j * 32 + l31] = s;
      }
      __syncthreads();
      if (tid < BN && n0 + tid < a.N) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_M; ++w) s += red[w * BN + tid];
        a.stats[(size_t)(a.N + n0 + tid) * n_mt + tile_m] = s;
      }
    }
  }
  if constexpr (STATS_MODE && sizeof(OT) == 2) {
    if (do_stats) {
      // merge: halves of a wave share the centre; the WAVES_M row strips of a column are combined pairwise (Chan)
      float* red = reinterpret_cast<float*>(smem);            // [WAVES_M][2][BN]
      static_assert(WAVES_M * 2 * BN * 4 <= (int)sizeof(smem), "stats scratch");
      const int wmi = wave / WAVES_N;
      const float nw = (float)max(0, min(WM, a.M - (m0 + wm0)));
      __syncthreads();                                         // staging reads are done
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float s1 = st_s1[j], s2 = st_s2[j];
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (h == 0) {
          red[(wmi * 2 + 0) * BN + wn0 + j * 32 + l31] = s1 + nw * st_c[j];                    // sum
          red[(wmi * 2 + 1) * BN + wn0 + j * 32 + l31] = nw > 0.f ? s2 - s1 * s1 / nw : 0.f;   // M2 about the strip mean
        }
      }
      __syncthreads();
      if (tid < BN && n0 + tid < a.N) {
        float n = 0.f, S = 0.f, M2 = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_M; ++w) {
          const float nq = (float)max(0, min(WM, a.M - (m0 + w * WM)));
          const float sw = red[(w * 2 + 0) * BN + tid], qw = red[(w * 2 + 1) * BN + tid];
          if (nq > 0.f) {
            if (n > 0.f) {
              const float d = sw / nq - S / n;
              M2 += qw + d * d * (n * nq / (n + nq));
            } else {
              M2 = qw;
            }
            S += sw;
            n += nq;
          }
        }
        a.stats[(size_t)(n0 + tid) * n_mt + tile_m] = S;
        a.stats[(size_t)(a.N + n0 + tid) * n_mt + tile_m] = fmaxf(M2, 0.f);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// fwd / dgrad for FEW ROWS and a LONG K (fp32 split mode; the 1 152- and 12 544-row levels of S3D-G, Mixed_4b .. 5c, and the
// projection heads): "K split over the waves".  With 18 .. 196 row tiles the grid of conv_gemm_kernel cannot fill the chip and
// every workgroup walks 30 .. 216 K tiles one after the other, each step costing a global -> LDS round trip and a barrier
// (measured 0.5 us per 64-byte K step: 12.9 TFLOP/s on the 1x3x3 data gradient of Mixed_5c).  Here the FOUR WAVES of a
// workgroup own the same 64 x BN output tile and a quarter of the K range each: every wave runs a private NS-stage DMA
// pipeline (its own LDS stages: no barrier in the K loop, only counted vmcnt waits), so four K steps are in flight per
// workgroup and the sequential depth is a quarter.  The four partial tiles are added through LDS in wave order (fixed order:
// bit-reproducible), then bias / activation / store / BatchNorm partials as in conv_gemm_kernel.
// Restricted to what the engine's fp32 mode issues for those layers: pre-split weights (DV_W3), uniform-tap gathers
// (channel pitch a multiple of 16, <= 32 taps), no parity classes, no fused BatchNorm-backward reduce.
// The body of one workgroup: block `bid` of the `nblk` blocks of the problem `a` (a grid of its own, or one member's share of
// conv_gemm_ks_pair_kernel's).  `a` by value: its fields stay the scalar kernel-argument loads of a kernel that takes the block.
template <int MODE, int BN, int NS>
__device__ __forceinline__ void conv_gemm_ks_body(const ConvArgs a, const int bid, const int nblk) {
  constexpr int BM = 64, NW = 4, TM = 2, TN = BN / 32;
  constexpr int A_BYTES = BM * 64, B_BYTES = BN * 96;          // one K tile: 16 f32 per row of A; hi|mid|lo of both k halves of B
  constexpr int BPC = B_BYTES / 1024;
  static_assert(B_BYTES % 1024 == 0, "B tile in 1 KiB pieces");
  constexpr int STG = A_BYTES + B_BYTES;
  constexpr int PIECES = A_BYTES / 1024 + BPC;
  constexpr int D = NS - 1;
  static_assert(D >= 1 && (D - 1) * PIECES <= 24, "counted wait");
  constexpr unsigned kOOB = 0x80000000u;
  static_assert(NW * NS * STG >= NW * BM * BN * 4 + BM * BN * 4, "the reduction scratch fits the stage buffers");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NW * NS * STG];

  const ConvGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int lbid = xcd_remap(bid, nblk);
  const int tile_n = lbid % a.ntn, tile_m = lbid / a.ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const dma_rsrc_t src_dma = dma_make_rsrc(a.src, (unsigned)a.src_bytes), w_dma = dma_make_rsrc(a.w, (unsigned)a.w_bytes);
  unsigned char* wsm = smem + wave * (NS * STG);               // this wave's stages
  const unsigned wbase = lds_addr(wsm);
  const unsigned ldb = (unsigned)a.lds_ * 4u;
  const int vslot = (lane & 3) ^ ((lane >> 4) & 3), vrow = lane >> 2;

  unsigned rowoff[4], imask[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const RowPos r = decode_row<MODE>((uint32_t)(m0 + 16 * p + vrow), a.M, g);
    unsigned bt = 0, bh = 0, bw = 0;
    int pos;
    if (MODE == MODE_FWD) {
      for (int d = 0; d < g.kt; ++d) bt |= ((unsigned)(r.t0 + d) < (unsigned)g.sT ? 1u : 0u) << d;
      for (int d = 0; d < g.kh; ++d) bh |= ((unsigned)(r.h0 + d) < (unsigned)g.sH ? 1u : 0u) << d;
      for (int d = 0; d < g.kw; ++d) bw |= ((unsigned)(r.w0 + d) < (unsigned)g.sW ? 1u : 0u) << d;
      pos = r.base + (r.t0 * g.sH + r.h0) * g.sW + r.w0;
    } else {                                                   // stride 1 (checked on the host)
      for (int d = 0; d < g.kt; ++d) { int v = r.t0 - d; bt |= ((v >= 0 && v < g.sT) ? 1u : 0u) << d; }
      for (int d = 0; d < g.kh; ++d) { int v = r.h0 - d; bh |= ((v >= 0 && v < g.sH) ? 1u : 0u) << d; }
      for (int d = 0; d < g.kw; ++d) { int v = r.w0 - d; bw |= ((v >= 0 && v < g.sW) ? 1u : 0u) << d; }
      pos = r.base + (r.t0 * g.sH + r.h0) * g.sW + r.w0;
    }
    if (!r.valid) bt = 0;
    unsigned inv = 0;
    int tp = 0;
    for (int dt = 0; dt < g.kt; ++dt)
      for (int dh = 0; dh < g.kh; ++dh)
        for (int dw = 0; dw < g.kw; ++dw, ++tp) inv |= ((((bt >> dt) & (bh >> dh) & (bw >> dw)) & 1u) ^ 1u) << tp;
    imask[p] = inv;
    rowoff[p] = (unsigned)pos * ldb + (unsigned)vslot * 16u;
  }
  unsigned woff[BPC];
#pragma unroll
  for (int p = 0; p < BPC; ++p) {
    const unsigned o = (unsigned)p * 1024u + (unsigned)lane * 16u;
    const unsigned hh = o / (BN * 48u), rem = o - hh * (BN * 48u);
    woff[p] = (hh * (unsigned)a.ldw + (unsigned)n0) * 48u + rem;          // + K tile * ldw * 96 (a.ldw = padded rows)
  }
  // this wave's K range and its wave-uniform cursor
  const int nk = g.Ktot / 16;
  const int k_lo = (int)(((long long)nk * wave) / NW), k_hi = (int)(((long long)nk * (wave + 1)) / NW);
  int u_tap = (k_lo * 16) / g.CP, u_c0 = k_lo * 16 - u_tap * g.CP;
  int u_dw = u_tap % g.kw, u_dh = (u_tap / g.kw) % g.kh, u_dt = u_tap / (g.kw * g.kh);
  auto tap_off = [&]() -> unsigned {
    const int toff = MODE == MODE_FWD ? (u_dt * g.sH + u_dh) * g.sW + u_dw : -((u_dt * g.sH + u_dh) * g.sW + u_dw);
    return (unsigned)toff * ldb;
  };
  unsigned u_toffb = tap_off();
  auto w_tap = [&]() -> int { return a.cls_on ? ((a.crt + u_dt) * a.oKH + a.crh + u_dh) * a.oKW + a.crw + u_dw : u_tap; };
  int u_otap = w_tap();
  auto gload = [&](int, int st) {
    const unsigned kt = (unsigned)(u_otap * g.CP + u_c0) >> 4;   // K tile of the weights (their own tap when the window is trimmed)
    const unsigned s_a = u_toffb + (unsigned)u_c0 * 4u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned off = ((__builtin_amdgcn_ubfe(imask[p], (unsigned)u_tap, 1u)) << 31) | (rowoff[p] + s_a);
      dma_load16(src_dma, wbase + st * STG + p * 1024, off);
    }
#pragma unroll
    for (int p = 0; p < BPC; ++p)
      dma_load16(w_dma, wbase + st * STG + A_BYTES + p * 1024, woff[p] + (unsigned)kt * (unsigned)a.ldw * 96u);
    u_c0 += 16;
    if (u_c0 >= g.CP) {
      u_c0 = 0;
      ++u_tap;
      if (++u_dw == g.kw) { u_dw = 0; if (++u_dh == g.kh) { u_dh = 0; ++u_dt; } }
      u_toffb = tap_off();
      u_otap = w_tap();
    }
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int swz = (l31 >> 2) & 3;
  const int nmine = k_hi - k_lo;
  for (int t = 0; t < D && t < nmine; ++t) gload(k_lo + t, t);
  int cur = 0, nxt = D % NS;
  for (int t = 0; t < nmine; ++t) {
    dma_wait_upto(min(D - 1, nmine - 1 - t) * PIECES);         // tile t of this wave has landed
    if (t + D < nmine) gload(k_lo + t + D, nxt);               // its stage was read by step t - 1 of THIS wave (program order)
    const unsigned char* sa = wsm + cur * STG;
    const unsigned char* sb = sa + A_BYTES;
    Split3 af[TM], bf[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = split3_row(sa + (i * 32 + l31) * 64, h, swz);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned char* pb = sb + ((h * BN + j * 32 + l31) * 3) * 16;
      bf[j].hi = *reinterpret_cast<const bf16x8*>(pb);
      bf[j].mid = *reinterpret_cast<const bf16x8*>(pb + 16);
      bf[j].lo = *reinterpret_cast<const bf16x8*>(pb + 32);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) mma_split3(af[i], bf[j], acc[i][j]);
    cur = cur + 1 == NS ? 0 : cur + 1;
    nxt = nxt + 1 == NS ? 0 : nxt + 1;
  }
  // ---- the four partial tiles -> LDS [wave][row][col], added in wave order
  __syncthreads();                                             // every wave is done with its stages
  float* red = reinterpret_cast<float*>(smem);                 // [NW][BM][BN]
  float* fin = red + NW * BM * BN;                             // [BM][BN]: the tile as stored (statistics)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        red[(wave * BM + row) * BN + j * 32 + l31] = acc[i][j][r];
      }
  __syncthreads();
  constexpr int CPT = BN / 4;                                  // columns per thread: thread = (row, quarter of the columns)
  const int row = tid >> 2, c0 = (tid & 3) * CPT;
  const int flags = a.flags;
  const bool row_ok = m0 + row < a.M;
  float* out = reinterpret_cast<float*>(a.out);
#pragma unroll
  for (int c4 = 0; c4 < CPT / 4; ++c4) {
    const int col = c0 + c4 * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(red + (0 * BM + row) * BN + col);
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *reinterpret_cast<const f32x4*>(red + (w * BM + row) * BN + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int cg = n0 + col + e;
      float x = v[e];
      if (flags & DV_BIAS) x += cg < a.N ? a.bias[cg] : 0.f;
      x = act_apply(x, flags);
      if (cg >= a.N || !row_ok) x = 0.f;
      v[e] = x;
    }
    *reinterpret_cast<f32x4*>(fin + row * BN + col) = v;
    if (row_ok && n0 + col < a.NP) {
      float* p = out + (size_t)(m0 + row) * a.ldo + n0 + col;
      if (flags & DV_ACCUM) v += *reinterpret_cast<const f32x4*>(p);
      *reinterpret_cast<f32x4*>(p) = v;
    }
  }
  if constexpr (MODE == MODE_FWD) {
    if (flags & DV_STATS) {                                    // per column: sum and M2 about the tile mean of the values as stored
      __syncthreads();
      if (tid < BN && n0 + tid < a.N) {
        const int rows_here = min(BM, a.M - m0);
        const int n_mt = (a.M + BM - 1) / BM;
        float s = 0.f;
        for (int r = 0; r < rows_here; ++r) s += fin[r * BN + tid];
        const float mu = s / (float)rows_here;
        float m2 = 0.f;
        for (int r = 0; r < rows_here; ++r) { const float dlt = fin[r * BN + tid] - mu; m2 += dlt * dlt; }
        a.stats[(size_t)(n0 + tid) * n_mt + tile_m] = s;
        a.stats[(size_t)(a.N + n0 + tid) * n_mt + tile_m] = m2;
      }
    }
  }
}

template <int MODE, int BN, int NS>
__global__ __launch_bounds__(256) void conv_gemm_ks_kernel(ConvArgs a) {
  conv_gemm_ks_body<MODE, BN, NS>(a, (int)blockIdx.x, (int)gridDim.x);
}

// Two independent problems of the same instantiation in one grid (the spatial branch convs of the 1 152-row Inception levels:
// 72 - 216 workgroups each, one per CU): blocks [0, nblk0) are member 0's grid, the others member 1's, as conv_tap_pair_kernel
// (conv_tap.hip).  The exchange of the partial tiles stays inside a workgroup: nothing crosses members.
struct KsPair {
  ConvArgs m[2];
  int nblk0;
};

template <int MODE, int BN, int NS>
__global__ __launch_bounds__(256) void conv_gemm_ks_pair_kernel(KsPair p) {
  const int b = (int)blockIdx.x, second = b >= p.nblk0 ? 1 : 0;
  conv_gemm_ks_body<MODE, BN, NS>(p.m[second], second ? b - p.nblk0 : b, second ? (int)gridDim.x - p.nblk0 : p.nblk0);
}

// The tiles of conv_gemm_kernel, each named here and nowhere else: (bm, bn) -> BM x BN on WAVES_M x WAVES_N waves.  A bm that is
// not 64 means 128 and a bn that is not 32 / 64 means 128; the 256 x 64 tile exists for the fp32 split forms alone (SPLIT).
template <int BM_, int BN_, int WM_, int WN_> struct GemmTile { static constexpr int BM = BM_, BN = BN_, WAVES_M = WM_, WAVES_N = WN_; };
template <bool SPLIT, class F>
static void with_gemm_tile(int bm, int bn, F&& f) {
  if constexpr (SPLIT) if (bm == 256) return f(GemmTile<256, 64, 4, 1>());
  if (bm == 64) {
    if (bn == 32) f(GemmTile<64, 32, 2, 1>());
    else if (bn == 64) f(GemmTile<64, 64, 2, 2>());
    else f(GemmTile<64, 128, 2, 2>());
  } else if (bn == 32) f(GemmTile<128, 32, 4, 1>());
  else if (bn == 64) f(GemmTile<128, 64, 4, 1>());
  else f(GemmTile<128, 128, 2, 2>());
}

// SPLIT / WF: the bf16 split of the fp32 mode without / with pre-split weights; they select the trailing template arguments only
template <typename T, int MODE, int GVB, int GM, int NS, bool SPLIT = false, bool WF = false>
static void launch_gemm_ns(const GemmForm& f, const ConvArgs& a, int grid, hipStream_t s) {
  if constexpr (WF && MODE == MODE_FWD && GM == 1 && NS == 2 && sizeof(T) == 4) {
    if (f.bnl) {             // BatchNorm on load (route_conv has checked: 256 x 64 tile, channel pitch <= 256)
      hipLaunchKernelGGL((conv_gemm_kernel<T, MODE, GVB, 256, 64, 4, 1, GM, NS, true, true, true>), dim3(grid), dim3(256), 0, s, a);
      return;
    }
  }
  with_gemm_tile<SPLIT>(f.bm, f.bn, [&](auto tile) {
    using Tl = decltype(tile);
    hipLaunchKernelGGL((conv_gemm_kernel<T, MODE, GVB, Tl::BM, Tl::BN, Tl::WAVES_M, Tl::WAVES_N, GM, NS, SPLIT, WF>), dim3(grid),
                       dim3(Tl::WAVES_M * Tl::WAVES_N * 64), 0, s, a);
  });
}

// the form -> the template (sizeof(T) == 1: the fp8 pointwise GEMMs)
template <typename T, int MODE, int GVB>
static void launch_gemm(const GemmForm& f, ConvArgs& a, hipStream_t s) {
  a.ntn = (a.NP + f.bn - 1) / f.bn;
  const int grid = a.ntn * ((a.M + f.bm - 1) / f.bm);
  if constexpr (sizeof(T) == 4) {
    if (f.wf && f.gm) launch_gemm_ns<T, MODE, GVB, 1, 2, true, true>(f, a, grid, s);
    else if (f.wf) launch_gemm_ns<T, MODE, GVB, 0, 2, true, true>(f, a, grid, s);
    else if (f.split) launch_gemm_ns<T, MODE, GVB, 0, 2, true>(f, a, grid, s);
    else launch_gemm_ns<T, MODE, GVB, 0, 2>(f, a, grid, s);
  } else if constexpr (GVB == 8) {
    launch_gemm_ns<T, MODE, GVB, 0, 2>(f, a, grid, s);
  } else if constexpr (sizeof(T) == 1) {
    if (f.gm) launch_gemm_ns<T, MODE, GVB, 1, 2>(f, a, grid, s);
    else launch_gemm_ns<T, MODE, GVB, 0, 2>(f, a, grid, s);
  } else {
    if (f.gm && f.ns == 4) launch_gemm_ns<T, MODE, GVB, 1, 4>(f, a, grid, s);
    else if (f.gm) launch_gemm_ns<T, MODE, GVB, 1, 2>(f, a, grid, s);
    else if (f.ns == 4) launch_gemm_ns<T, MODE, GVB, 0, 4>(f, a, grid, s);
    else launch_gemm_ns<T, MODE, GVB, 0, 2>(f, a, grid, s);
  }
}

template <int MODE>
static void launch_gemm_dt(int dtype, const GemmForm& f, ConvArgs& a, hipStream_t s) {
  if (dtype == DV_F32) launch_gemm<float, MODE, 16>(f, a, s);
  else if (f.gvb == 16) launch_gemm<bf16_t, MODE, 16>(f, a, s);
  else if constexpr (MODE == MODE_FWD) launch_gemm<bf16_t, MODE, 8>(f, a, s);       // (8-byte gathers: the padded RGB input)
}

template <int MODE>
static void launch_ks(int bn, ConvArgs& a, hipStream_t s) {
  a.ntn = (a.NP + bn - 1) / bn;
  const int grid = a.ntn * ((a.M + 63) / 64);
  if (bn == 32) hipLaunchKernelGGL((conv_gemm_ks_kernel<MODE, 32, 4>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_gemm_ks_kernel<MODE, 64, 3>), dim3(grid), dim3(256), 0, s, a);
}
// two problems with the same column tile (the instantiation follows from it) in one grid
template <int MODE>
static void launch_ks_pair(int bn, ConvArgs& a0, ConvArgs& a1, hipStream_t s) {
  KsPair p;
  a0.ntn = (a0.NP + bn - 1) / bn;
  a1.ntn = (a1.NP + bn - 1) / bn;
  p.m[0] = a0; p.m[1] = a1;
  p.nblk0 = a0.ntn * ((a0.M + 63) / 64);
  const int grid = p.nblk0 + a1.ntn * ((a1.M + 63) / 64);
  if (bn == 32) hipLaunchKernelGGL((conv_gemm_ks_pair_kernel<MODE, 32, 4>), dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((conv_gemm_ks_pair_kernel<MODE, 64, 3>), dim3(grid), dim3(256), 0, s, p);
}

}  // namespace
