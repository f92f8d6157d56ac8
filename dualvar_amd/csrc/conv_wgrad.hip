// The convolution's weight gradient as implicit GEMM on the gfx950 matrix cores: its kernels, its plan (plan_wgrad: one per
// call, read by the launch and every query) and its entry points.
//   wgrad: dW[n][j] = sum_m dY[m][n]  * A_x[m][j]            j = (tap,c)
// A_x is the same kind of im2col tile the forward gathers (conv_gemm.hpp), read transposed (ds_read_b64_tr_b16 for bf16, plain
// b32 for f32); the MFMAs and their 32x32 C/D layout are the forward's.
#include "conv_common.hpp"

namespace {
// ------------------------------------------------------------------------------------------
// wgrad kernels.  Each workgroup owns a BI (output channels) x BJ (im2col columns) tile of dW and a contiguous slice of
// rows (a "row split"); 32 rows per step.  DETERMINISTIC two-phase accumulation: a workgroup stores its fp32 partial
// tile with plain stores into slab[split] (caller-owned scratch, [splits][Cout][J]) and wgrad_reduce_kernel adds the
// slabs to dW in a fixed order -- no float atomics (their order changed results from run to run, and at ~1.3 TB/s
// chip-wide they were ~40 % of a mid-size launch).  With one split the tile is added to dW directly.
// dW[e] += sum_s slab[s][e], s ascending inside each of the 16 interleaved groups, groups combined in ascending order:
// a fixed summation tree, so the result does not depend on scheduling.  Thread (cx, sg) of a block sums slabs
// sg, sg+16, ... of float4 column blockIdx*16 + cx (16 lanes = 256 contiguous bytes per slab).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, long long stride, int splits,
                                                           float* __restrict__ dw, long long n4) {
  __shared__ f32x4 part[16][17];
  const int cx = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const long long c = (long long)blockIdx.x * 16 + cx;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f};
  if (c < n4) {
    const f32x4* p = reinterpret_cast<const f32x4*>(slab) + c;
    const long long st4 = stride / 4;
    int s = sg;
    for (; s + 48 < splits; s += 64) {                 // four independent loads in flight
      const f32x4 v0 = p[(long long)s * st4], v1 = p[(long long)(s + 16) * st4], v2 = p[(long long)(s + 32) * st4],
                  v3 = p[(long long)(s + 48) * st4];
      s0 += v0; s0 += v1; s0 += v2; s0 += v3;
    }
    for (; s < splits; s += 16) s0 += p[(long long)s * st4];
  }
  part[sg][cx] = s0;
  __syncthreads();
  if (sg == 0 && c < n4) {
    f32x4* d = reinterpret_cast<f32x4*>(dw) + c;
    f32x4 t = part[0][cx];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += part[g][cx];
    *d = *d + t;
  }
}

// smallest 16-byte-multiple pitch >= bytes with pitch mod 256 in {64, 192}: four consecutive rows of a
// ds_read_b64_tr_b16 block then fall on four different 64-byte bank groups
constexpr int tr_pitch(int bytes) {
  int p = (bytes + 15) / 16 * 16;
  while (p % 256 != 64 && p % 256 != 192) p += 16;
  return p;
}

template <typename T> struct WgMma;
template <> struct WgMma<bf16_t> {
  // P: [32 rows m][pitchP bytes] holding i-columns; Q likewise for j-columns
  static __device__ __forceinline__ bf16x8 frag(const unsigned char* tile, int pitch, int col0, int lane, int ks) {
    const int g16 = lane >> 4, li = lane & 15;
    const int q = li >> 2, p = li & 3;
    const int row = ks * 16 + 8 * (g16 >> 1) + q;
    const unsigned char* ad = tile + row * pitch + (col0 + 16 * (g16 & 1) + 4 * p) * 2;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(ad));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(ad + 4 * pitch));
    s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(bf16x8, v);
  }
};

template <typename T, int GVB, int BI, int BJ>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int ES = (int)sizeof(T);
  constexpr int GV = GVB / ES;
  constexpr int ROWS = 32;
  // pitches: bf16 transposed reads want (pitch mod 256) == 64 or 192 bytes; f32 reads are row-linear
  constexpr int PITCH_P = ES == 2 ? tr_pitch(BI * 2) : BI * 4 + 16;
  constexpr int PITCH_Q = ES == 2 ? tr_pitch(BJ * 2) : BJ * 4 + 16;
  constexpr int PV = BI * ES / 16;               // 16-byte vectors per P row
  constexpr int P_PER_THREAD = ROWS * PV / 256;
  constexpr int QV = BJ * ES / GVB;              // gather vectors per Q row
  constexpr int Q_PER_THREAD = (ROWS * QV + 255) / 256;
  constexpr int WI = BI / 2, WJ = BJ / 2;        // waves 2x2
  constexpr int TI = WI / 32, TJ = WJ / 32;
  static_assert(TI >= 1 && TJ >= 1, "tile");
  static_assert(P_PER_THREAD >= 1, "P tile");
  typedef typename VecB<GVB>::type qvec_t;

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ROWS * (PITCH_P + PITCH_Q)];
  constexpr int BUFB = ROWS * (PITCH_P + PITCH_Q);   // P tile then Q tile, twice
  constexpr int QOFF = ROWS * PITCH_P;

  const ConvGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  int bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_j = bid % a.ntj; bid /= a.ntj;
  const int tile_i = bid % a.nti;
  const int split = bid / a.nti;
  const int i0 = tile_i * BI, j0 = tile_j * BJ;
  const int wi0 = (wave >> 1) * WI, wj0 = (wave & 1) * WJ;
  const int m_begin = split * a.rows_per_split;
  const int m_end = min(a.M, m_begin + a.rows_per_split);
  if (m_begin >= m_end) return;

  const T* x = reinterpret_cast<const T*>(a.x);
  const T* dy = reinterpret_cast<const T*>(a.dy);

  // fixed column cursors of this thread's Q vectors
  KCursor qc[Q_PER_THREAD];
  int qrow[Q_PER_THREAD], qcol[Q_PER_THREAD];
  bool qok[Q_PER_THREAD];
#pragma unroll
  for (int u = 0; u < Q_PER_THREAD; ++u) {
    int id = tid + u * 256;
    qrow[u] = id / QV;
    qcol[u] = (id % QV) * GV;
    int j = j0 + qcol[u];
    qok[u] = (qrow[u] < ROWS) && (j < a.J);
    qc[u].init(qok[u] ? j : 0, g);
  }

  uint4 rp[P_PER_THREAD];
  qvec_t rq[Q_PER_THREAD];
  auto gload = [&](int mb) {
#pragma unroll
    for (int u = 0; u < P_PER_THREAD; ++u) {
      int id = tid + u * 256;
      int r = id / PV, cv = (id % PV) * (16 / ES);
      int m = mb + r, n = i0 + cv;
      bool ok = (m < m_end) && (n < a.CoutP);
      rp[u] = ok ? *reinterpret_cast<const uint4*>(dy + (size_t)m * a.ldy + n) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < Q_PER_THREAD; ++u) {
      int m = mb + qrow[u];
      int pos = -1;
      if (qok[u] && m < m_end) {
        RowPos rpos = decode_row<MODE_FWD>((uint32_t)m, a.M, g);
        pos = src_pos(rpos, qc[u], g);
      }
      rq[u] = pos >= 0 ? *reinterpret_cast<const qvec_t*>(x + (size_t)pos * a.ldx + qc[u].c) : VecB<GVB>::zero();
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int u = 0; u < P_PER_THREAD; ++u) {
      int id = tid + u * 256;
      int r = id / PV, cb = (id % PV) * 16;
      *reinterpret_cast<uint4*>(smem + buf * BUFB + r * PITCH_P + cb) = rp[u];
    }
#pragma unroll
    for (int u = 0; u < Q_PER_THREAD; ++u)
      if (qrow[u] < ROWS) *reinterpret_cast<qvec_t*>(smem + buf * BUFB + QOFF + qrow[u] * PITCH_Q + qcol[u] * ES) = rq[u];
  };

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nsteps = (m_end - m_begin + ROWS - 1) / ROWS;
  gload(m_begin);
  lstore(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    if (s + 1 < nsteps) gload(m_begin + (s + 1) * ROWS);
    if constexpr (ES == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 af[TI], bf[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = WgMma<bf16_t>::frag(smem + cur * BUFB, PITCH_P, wi0 + i * 32, lane, ks);
#pragma unroll
        for (int j = 0; j < TJ; ++j) bf[j] = WgMma<bf16_t>::frag(smem + cur * BUFB + QOFF, PITCH_Q, wj0 + j * 32, lane, ks);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < ROWS / 2; ++ks) {
        float af[TI], bf[TJ];
        const int kr = ks * 2 + h;
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = *reinterpret_cast<const float*>(smem + cur * BUFB + kr * PITCH_P + (wi0 + i * 32 + l31) * 4);
#pragma unroll
        for (int j = 0; j < TJ; ++j) bf[j] = *reinterpret_cast<const float*>(smem + cur * BUFB + QOFF + kr * PITCH_Q + (wj0 + j * 32 + l31) * 4);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) lstore(cur ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
      wgrad_store_block(a, split, i0 + wi0 + i * 32, j0 + wj0 + j * 32 + l31, h, acc[i][j]);
}

// ------------------------------------------------------------------------------------------
// wgrad with global -> LDS DMA gathers (16-byte vectors; bf16 and f32).  The 8-byte-gather case keeps the
// register-staged kernel above.  Differences from it:
//  * both tiles are UNPADDED row-linear LDS images filled by buffer_load ... lds (one wave instruction = 1 KiB), so no
//    VGPR staging and no ds_write.  bf16 reads them transposed (ds_read_b64_tr_b16); the bank conflicts of those reads
//    (4 rows x 64 B per half wave) are removed by XOR-swizzling the 64-byte chunk index with the row (row&3 for 256- and
//    512-byte rows, (row>>1)&1 for 128-byte rows), applied on the source side (which column slot a lane fetches) and on
//    the read side.  f32 reads one dword per lane along a row (conflict free as it is);
//  * a row's im2col coordinates are decoded ONCE per workgroup (not once per 16-byte vector): each thread decodes one of
//    the next 256 rows into an LDS table {byte offset of the row's first tap, separable tap-validity masks}; a lane's
//    column slot -- hence its tap and channel -- is fixed for the whole kernel, so the per-step address is
//    table.offset + constant, or an out-of-range offset (hardware zero fill) when the tap falls into the padding;
//  * wave tiles are 64 x 64 (2 x 2 MFMA blocks: 8 MFMAs per 32-row step and wave instead of 4, for the same barrier),
//    workgroup tiles 128 x 128 or 64 x 256 (f32: 64 x 128 with 32 x 64 wave tiles): half the dY / im2col re-reads of
//    the 128 x 64 tiles this replaces.

// NS: LDS stages -- tiles s+1 .. s+NS-1 are in flight while tile s is multiplied (counted vmcnt; every wave issues the
// same NPW + NQW pieces per tile).  WVI x WVJ waves, each a 64 x 64 tile of dW.
// workgroups per CU the LDS footprint admits (<= 3), and the waves per SIMD that makes (the register allocator is
// asked to make room for them)
constexpr int wgrad_wgs_per_cu(int es, int bi, int bj, int nw, int ns) {
  const int lds = ns * 32 * (bi + bj) * es + 24 * nw * 64;
  const int by_lds = 163840 / lds, by_waves = 32 / nw;
  const int k = by_lds < by_waves ? by_lds : by_waves;
  return k >= 3 ? 3 : (k >= 2 ? 2 : 1);
}
constexpr int wgrad_waves_per_simd(int es, int bi, int bj, int nw, int ns) {
  return (wgrad_wgs_per_cu(es, bi, bj, nw, ns) * nw + 3) / 4;
}

// SHARE (fp32 split mode, 1 x 4 waves): the dY fragments of a step -- which every one of the four waves needs -- are split
// ONCE per workgroup (one fragment per thread, the bf16 triples written to LDS in fragment order, a barrier, operands
// fetched as ds_read_b128); each wave splits only its own 32 columns of x.  Three fragments per wave and step instead of the
// six of the 2 x 2 layout (where the two waves of a row / column each split the fragments they share): the kernel is bound
// by the count of exactly those vector instructions.  12 KB of LDS more: still two workgroups per CU.
// BNA (SHARE only; dv_conv3d_wgrad_bn): the dY tile is dv_bn_bwd_apply's output formed on the fly -- a third DMA tile carries
// the BatchNorm's input beside dL/dy, and the thread that splits a dY fragment (its column = its channel: k1, k2, k3, scale and
// shift are per-thread constants) first forms k1*g' + k2*x + k3 with dv_bn_bwd_apply's expression.  8 KB of LDS more per
// stage; the row tables shrink to 128 rows per round so that two workgroups still fit a CU (80 896 bytes each).
template <typename T, int BI, int BJ, int WVI, int WVJ, int NS, bool SPLIT = false, bool SHARE = false, bool BNA = false>
__global__ __launch_bounds__(WVI * WVJ * 64)
__attribute__((amdgpu_waves_per_eu(wgrad_waves_per_simd(sizeof(T), BI, BJ, WVI * WVJ, NS)))) void conv_wgrad_dma_kernel(WgradDmaArgs aa) {
  static_assert(!SPLIT || sizeof(T) == 4, "the bf16 split is the fp32 mode's product");
  static_assert(!SHARE || SPLIT, "the shared split belongs to the fp32 split mode");
  static_assert(!BNA || (SHARE && BI == 64), "the fused BatchNorm backward rides on the shared dY split (one channel per lane)");
  const WgradArgs& a = aa.w;
  constexpr int ES = (int)sizeof(T);
  constexpr int EPV = 16 / ES;                       // elements per 16-byte DMA slot
  constexpr int ROWS = 32;
  constexpr int NW = WVI * WVJ, NT = NW * 64;
  constexpr int RBP = BI * ES, RBQ = BJ * ES;        // row bytes of the dY (P) and im2col (Q) tiles
  static_assert(RBP % 128 == 0 && RBQ % 128 == 0, "row bytes (swizzle, 1 KiB DMA pieces)");
  constexpr int DP = RBP / 16, DQ = RBQ / 16;        // 16-byte slots per row
  constexpr int QOFF = ROWS * RBP, YOFF = ROWS * (RBP + RBQ), BUFB = YOFF + (BNA ? ROWS * RBP : 0);
  constexpr int PPC = QOFF / 1024, QPC = (YOFF - QOFF) / 1024;                   // 1 KiB DMA pieces per tile
  constexpr int NPW = (PPC + NW - 1) / NW, NQW = (QPC + NW - 1) / NW;             // ... per wave (the last round may be partial)
  constexpr int RT = BNA ? NT / 2 : NT;              // rows per decode round: one row per thread (BNA: per thread of the first half)
  constexpr int SPR = RT / ROWS;                     // steps per round
  constexpr int WI = BI / WVI, WJ = BJ / WVJ, TI = WI / 32, TJ = WJ / 32;
  static_assert(TI >= 1 && TJ >= 1, "wave tile");
  constexpr unsigned kOOB = 0x80000000u;

  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * BUFB];
  __shared__ uint2 rowtab[2][RT];
  __shared__ unsigned rowdy[2][RT];                  // byte offset of the row in dY (kOOB beyond the slice)
  // SHARE: [k half * 2 + h][hi | mid | lo][column] bf16x8 fragments of the current step's dY tile
  constexpr int NFRAG = SHARE ? BI * 4 : 1;
  __shared__ uint4 planes[NFRAG * 3];
  static_assert(!SHARE || (NFRAG == NT && WVI == 1), "one dY fragment per thread, every wave spans all of BI");

  const ConvGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile_j = bid % a.ntj; bid /= a.ntj;
  const int tile_i = bid % a.nti;
  const int split = bid / a.nti;
  const int i0 = tile_i * BI, j0 = tile_j * BJ;
  const int wi0 = (wave / WVJ) * WI, wj0 = (wave % WVJ) * WJ;
  const int m_begin = split * a.rows_per_split;
  const int m_end = min(a.M, m_begin + a.rows_per_split);      // (the host sizes the splits so that none is empty)

  const dma_rsrc_t x_rsrc = dma_make_rsrc(a.x, (unsigned)aa.x_bytes), dy_rsrc = dma_make_rsrc(a.dy, (unsigned)aa.dy_bytes);
  const dma_rsrc_t bnx_rsrc = dma_make_rsrc(BNA ? aa.bn.x : a.dy, (unsigned)aa.dy_bytes);
  const unsigned smem_base = lds_addr(smem);
  const unsigned ldxb = (unsigned)a.ldx * ES, ldyb = (unsigned)a.ldy * ES;

  // fixed per-lane roles: LDS slot -> (row, swizzled source column)
  int prow[NPW]; unsigned pcolb[NPW];
#pragma unroll
  for (int u = 0; u < NPW; ++u) {
    const int sl = (wave + NW * u) * 64 + lane;
    prow[u] = sl / DP;
    const int jj = ES == 2 ? ((sl % DP) ^ (wg_swz<RBP>(prow[u]) << 2)) : (sl % DP);
    const int n = i0 + jj * EPV;
    pcolb[u] = n < a.CoutP ? (unsigned)n * ES : kOOB;
  }
  int qrow[NQW]; unsigned qtb[NQW], qbit[NQW];
#pragma unroll
  for (int u = 0; u < NQW; ++u) {
    const int sl = (wave + NW * u) * 64 + lane;
    qrow[u] = sl / DQ;
    const int jj = ES == 2 ? ((sl % DQ) ^ (wg_swz<RBQ>(qrow[u]) << 2)) : (sl % DQ);
    const int col = j0 + jj * EPV;
    if (col < a.J) {
      const int tap = col / g.CP, c = col - tap * g.CP;
      const int dw = tap % g.kw, t2 = tap / g.kw, dh = t2 % g.kh, dt = t2 / g.kh;
      qbit[u] = (1u << dt) | (1u << (8 + dh)) | (1u << (16 + dw));
      qtb[u] = (unsigned)((dt * g.sH + dh) * g.sW + dw) * ldxb + (unsigned)c * ES;
    } else {
      qbit[u] = 0xffffffffu;                         // never matches a 24-bit mask: zero fill
      qtb[u] = 0;
    }
  }

  // decode RT rows of round `rnd` (one per thread) into rowtab[rnd & 1]
  auto decode = [&](int rnd) {
    if (RT < NT && tid >= RT) return;
    const int q = m_begin + rnd * RT + tid;          // position in the row sequence
    uint2 e = make_uint2(0u, 0u);
    unsigned dyo = kOOB;
    if (q < m_end) {
      const uint32_t m = a.perm.on ? perm_row(a.perm, (uint32_t)q) : (uint32_t)q;
      dyo = m * ldyb;
      const RowPos r = decode_row<MODE_FWD>(m, a.M, g);
      auto range = [](int x0, int k, int lim) -> unsigned {      // bits d in [0,k) with 0 <= x0 + d < lim
        const int lo = max(0, -x0), hi = min(k, lim - x0);
        return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
      };
      const unsigned bt = range(r.t0, g.kt, g.sT), bh = range(r.h0, g.kh, g.sH), bw = range(r.w0, g.kw, g.sW);
      e.x = (unsigned)(r.base + (r.t0 * g.sH + r.h0) * g.sW + r.w0) * ldxb;   // modulo 2^32; exact for valid taps
      e.y = (bt && bh && bw) ? (bt | (bh << 8) | (bw << 16)) : 0u;
    }
    rowtab[rnd & 1][tid] = e;
    rowdy[rnd & 1][tid] = dyo;
  };

  auto issue = [&](int s, int buf) {
    const unsigned* dtab = rowdy[(s / SPR) & 1] + (s % SPR) * ROWS;
    unsigned dyo[NPW];
#pragma unroll
    for (int u = 0; u < NPW; ++u) dyo[u] = dtab[prow[u]];
#pragma unroll
    for (int u = 0; u < NPW; ++u) {
      if (PPC % NW != 0 && wave + NW * u >= PPC) break;           // (wave-uniform)
      const unsigned off = (dyo[u] != kOOB && pcolb[u] != kOOB) ? dyo[u] + pcolb[u] : kOOB;
      dma_load16(dy_rsrc, smem_base + buf * BUFB + (wave + NW * u) * 1024, off);
    }
    if constexpr (BNA) {                             // the BatchNorm's input: same rows, same pitch, its own tile
#pragma unroll
      for (int u = 0; u < NPW; ++u) {
        const unsigned off = (dyo[u] != kOOB && pcolb[u] != kOOB) ? dyo[u] + pcolb[u] : kOOB;
        dma_load16(bnx_rsrc, smem_base + buf * BUFB + YOFF + (wave + NW * u) * 1024, off);
      }
    }
    const unsigned long long* tab = reinterpret_cast<const unsigned long long*>(rowtab[(s / SPR) & 1] + (s % SPR) * ROWS);
    unsigned long long e[NQW];
#pragma unroll
    for (int u = 0; u < NQW; ++u) e[u] = tab[qrow[u] & (ROWS - 1)];   // one ds_read_b64 each, issued back to back
#pragma unroll
    for (int u = 0; u < NQW; ++u) {
      if (QPC % NW != 0 && wave + NW * u >= QPC) break;
      const unsigned ex = (unsigned)e[u], ey = (unsigned)(e[u] >> 32);
      const unsigned off = ((ey & qbit[u]) == qbit[u]) ? ex + qtb[u] : kOOB;
      dma_load16(x_rsrc, smem_base + buf * BUFB + QOFF + (wave + NW * u) * 1024, off);
    }
  };
  // pieces this wave issues per step (wave-uniform)
  int my_pieces = 0;
#pragma unroll
  for (int u = 0; u < NPW; ++u) my_pieces += (wave + NW * u < PPC) ? (BNA ? 2 : 1) : 0;
#pragma unroll
  for (int u = 0; u < NQW; ++u) my_pieces += (wave + NW * u < QPC) ? 1 : 0;

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5, l31 = lane & 31;
  // BNA: this thread's channel (= its column of the dY tile) and dv_bn_bwd_apply's coefficients for it, same expressions
  float bk1 = 0.f, bk2 = 0.f, bk3 = 0.f, bsc = 0.f, bsh = 0.f;
  if constexpr (BNA) {
    const int c = i0 + lane, cpb = (a.Cout + 7) & ~7;
    if (c < a.Cout) {
      float sg = 0.f, sgx = 0.f;
      for (int r = 0; r < aa.bn.rep; ++r) { sg += aa.bn.sums[(size_t)r * 2 * cpb + c]; sgx += aa.bn.sums[(size_t)r * 2 * cpb + cpb + c]; }
      bk1 = aa.bn.gamma[c] * aa.bn.invstd[c];
      bk2 = -bk1 * aa.bn.invstd[c] * sgx * aa.bn.inv_count;
      bk3 = -bk1 * sg * aa.bn.inv_count - bk2 * aa.bn.mean[c];
      if (aa.bn.mask) { bsc = aa.bn.scale[c]; bsh = aa.bn.shift[c]; }
      if (split == 0 && tile_j == 0 && wave == 0 && aa.bn.dgamma) {       // one workgroup per channel tile: dgamma, dbeta
        aa.bn.dbeta[c] += aa.bn.dscale * sg;
        aa.bn.dgamma[c] += aa.bn.dscale * sgx;
      }
    }
  }
  const int nsteps = (m_end - m_begin + ROWS - 1) / ROWS;
  constexpr int D = NS - 1;                          // prefetch distance (the row table runs one round = SPR steps ahead)
  static_assert(D >= 1 && D < SPR, "stages");
  decode(0);
  __syncthreads();
  for (int t = 0; t < D && t < nsteps; ++t) issue(t, t);
  int cur = 0, nxt = D % NS;
  for (int s = 0; s < nsteps; ++s) {
    dma_wait_upto(min(D - 1, nsteps - 1 - s) * my_pieces);         // tile s has landed (this wave's pieces)
    __syncthreads();                                 // ... everybody's; stage `nxt` (tile s-1) and the old row table are free
    // table of round R+1 is written during the first step of round R; its previous contents (round R-1) were last read
    // at least one barrier ago, and its first reader (the issue for step SPR(R+1), at step SPR(R+1)-D) is later
    if ((s % SPR) == 0 && (s + SPR) < nsteps) decode(s / SPR + 1);
    if (s + D < nsteps) issue(s + D, nxt);
    const unsigned char* tp = smem + cur * BUFB;
    const unsigned char* tq = tp + QOFF;
    if constexpr (ES == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 af[TI], bf[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = wg_frag<RBP>(tp, wi0 + i * 32, lane, ks);
#pragma unroll
        for (int j = 0; j < TJ; ++j) bf[j] = wg_frag<RBQ>(tq, wj0 + j * 32, lane, ks);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    } else if constexpr (SHARE) {
      // split phase: thread -> dY fragment (kh = k half * 2 + h = its wave, column = its lane): conflict-free dword reads of 8
      // rows of a column, 16-byte writes of the three planes
      {
        const int kh = wave, col = lane;
        const int rr0 = (kh >> 1) * 16 + 8 * (kh & 1);
        const unsigned char* src = tp + rr0 * RBP + col * 4;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const float*>(src + e * RBP);
        if constexpr (BNA) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            // (rows past the end of the split need no special case: their im2col rows are zero-filled too, so whatever this forms
            // for them -- k3 -- is multiplied by zeros)
            const float xv = *reinterpret_cast<const float*>(src + YOFF + e * RBP);
            const float act = xv * bsc + bsh;              // the forward's expression (dv_bn_apply), same rounding
            const float gg = (aa.bn.mask && !(act > 0.f)) ? 0.f : v[e];
            v[e] = bk1 * gg + bk2 * xv + bk3;              // dv_bn_bwd_apply's expression
          }
        }
        const Split3 s3 = split3w(v);
        uint4* dst = planes + kh * 3 * BI + col;
        dst[0] = __builtin_bit_cast(uint4, s3.hi);
        dst[BI] = __builtin_bit_cast(uint4, s3.mid);
        dst[2 * BI] = __builtin_bit_cast(uint4, s3.lo);
      }
      // this wave's own x fragments (both K halves) are split while the other waves finish their dY fragment (splitting K half 1
      // under the MFMAs of K half 0 instead was measured equal)
      Split3 bfr[2][TJ];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const float*>(tq + (ks * 16 + 8 * h + e) * RBQ + (wj0 + j * 32 + l31) * 4);
          bfr[ks][j] = split3w(v);
        }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Split3 af[TI];
        const int kh = ks * 2 + h;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const uint4* pa = planes + kh * 3 * BI + wi0 + i * 32 + l31;
          af[i].hi = __builtin_bit_cast(bf16x8, pa[0]);
          af[i].mid = __builtin_bit_cast(bf16x8, pa[BI]);
          af[i].lo = __builtin_bit_cast(bf16x8, pa[2 * BI]);
        }
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) mma_split3(af[i], bfr[ks][j], acc[i][j]);
      }
    } else if constexpr (SPLIT) {
      // f32 tiles, products on the bf16 matrix cores (split3 above): the K index of this GEMM is the ROW, so a lane's
      // fragment is 8 rows of one column (conflict-free dword reads, immediate offsets)
      // Software pipeline inside the step: the fragments of K half 1 are split while the MFMAs of K half 0 run.  In program order
      // a wave would split everything (vector ALU only), then multiply (matrix pipe only); sched_group_barrier makes the
      // scheduler emit one MFMA, then its share of the split instructions, so both pipes work at once.
      auto frag_a = [&](int ks, int i, float (&v)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const float*>(tp + (ks * 16 + 8 * h + e) * RBP + (wi0 + i * 32 + l31) * 4);
      };
      auto frag_b = [&](int ks, int j, float (&v)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const float*>(tq + (ks * 16 + 8 * h + e) * RBQ + (wj0 + j * 32 + l31) * 4);
      };
      Split3 a0[TI], b0[TJ], a1[TI], b1[TJ];
      float ra[TI][8], rb[TJ][8];
#pragma unroll
      for (int i = 0; i < TI; ++i) { float v[8]; frag_a(0, i, v); a0[i] = split3w(v); }
#pragma unroll
      for (int j = 0; j < TJ; ++j) { float v[8]; frag_b(0, j, v); b0[j] = split3w(v); }
#pragma unroll
      for (int i = 0; i < TI; ++i) frag_a(1, i, ra[i]);
#pragma unroll
      for (int j = 0; j < TJ; ++j) frag_b(1, j, rb[j]);
#pragma unroll
      for (int i = 0; i < TI; ++i) a1[i] = split3w(ra[i]);
#pragma unroll
      for (int j = 0; j < TJ; ++j) b1[j] = split3w(rb[j]);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) mma_split3(a0[i], b0[j], acc[i][j]);
      {
        constexpr int NM = TI * TJ * 6, VPM = (44 * (TI + TJ) + NM - 1) / NM;
#pragma unroll
        for (int qq = 0; qq < NM; ++qq) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x2, VPM, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) mma_split3(a1[i], b1[j], acc[i][j]);
    } else {
#pragma unroll 4
      for (int ks = 0; ks < ROWS / 2; ++ks) {
        float af[TI], bf[TJ];
        const int kr = ks * 2 + h;
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = *reinterpret_cast<const float*>(tp + kr * RBP + (wi0 + i * 32 + l31) * 4);
#pragma unroll
        for (int j = 0; j < TJ; ++j) bf[j] = *reinterpret_cast<const float*>(tq + kr * RBQ + (wj0 + j * 32 + l31) * 4);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    }
    cur = cur + 1 == NS ? 0 : cur + 1;
    nxt = nxt + 1 == NS ? 0 : nxt + 1;
  }

#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
      wgrad_store_block(a, split, i0 + wi0 + i * 32, j0 + wj0 + j * 32 + l31, h, acc[i][j]);
}

}  // namespace

// ---- weight gradient -------------------------------------------------------------------------------------------------------
// conv_wgrad_dma_kernel's configurations.  The kernel is bound by what a CU can pull from L2 into LDS (~70 GB/s per CU): the
// bytes filled per unit of work go with 1/BI + 1/BJ, so the largest tile that wastes little padding wins -- see plan_wgrad.
// A list's row is both what the cost model walks and the launch of its instantiation: no other place names a tile.
struct WgradCfg {
  int BI, BJ, WVI, WVJ, NS;   // as the cost model and wgrad_wgs_per_cu see the configuration
  bool bna;                   // the fp32 split mode runs it on the SHARE form, which has a BNA variant (dv_conv3d_wgrad_bn)
  void (*launch)(const WgradDmaArgs& aa, int grid, hipStream_t s);
};
template <typename T, int BI, int BJ, int WVI, int WVJ, int NS, bool... FORM>
static void launch_wgrad_dma(const WgradDmaArgs& aa, int grid, hipStream_t s) {
  hipLaunchKernelGGL((conv_wgrad_dma_kernel<T, BI, BJ, WVI, WVJ, NS, FORM...>), dim3(grid), dim3(WVI * WVJ * 64), 0, s, aa);
}
// fp32: exact-f32 mode <BI, BJ, WVI, WVJ, NS>; split mode SWI x SWJ waves, <.., true> or (SHARE) <.., true, true> / its BNA form
template <int BI, int BJ, int WVI, int WVJ, int NS, int SWI, int SWJ, bool SHARE>
static void launch_wgrad_dma_f32(const WgradDmaArgs& aa, int grid, hipStream_t s) {
  if (f32_exact()) launch_wgrad_dma<float, BI, BJ, WVI, WVJ, NS>(aa, grid, s);
  else if constexpr (!SHARE) launch_wgrad_dma<float, BI, BJ, SWI, SWJ, NS, true>(aa, grid, s);
  else if (aa.bn.x) launch_wgrad_dma<float, BI, BJ, SWI, SWJ, NS, true, true, true>(aa, grid, s);
  else launch_wgrad_dma<float, BI, BJ, SWI, SWJ, NS, true, true>(aa, grid, s);
}
#define WG_BF16(BI, BJ, WVI, WVJ, NS) {BI, BJ, WVI, WVJ, NS, false, launch_wgrad_dma<bf16_t, BI, BJ, WVI, WVJ, NS>}
#define WG_F32(BI, BJ, WVI, WVJ, NS, SWI, SWJ, SHARE) \
  {BI, BJ, WVI, WVJ, NS, SHARE, launch_wgrad_dma_f32<BI, BJ, WVI, WVJ, NS, SWI, SWJ, SHARE>}
static const WgradCfg kWgBf16[] = {WG_BF16(128, 128, 2, 2, 3), WG_BF16(64, 256, 1, 4, 3), WG_BF16(128, 256, 2, 2, 3),
                                   WG_BF16(192, 256, 3, 4, 4)};
// (f32 split mode: a two-wave 64 x 128 workgroup with 64 x 64 wave tiles -- one fragment split per 32x32 block instead of
// 1.5 -- was measured slower than the four-wave one with 32 x 64 wave tiles: 950 vs 827 us on the 7x1x1 stem layer.)  Both
// modes are costed with the 2 x 2 rows; the split mode's 1 x 4 layout has the same four waves and LDS bytes.
static const WgradCfg kWgF32[] = {WG_F32(128, 128, 2, 2, 2, 2, 2, false), WG_F32(64, 128, 2, 2, 2, 1, 4, true)};
#undef WG_BF16
#undef WG_F32
template <int N> static constexpr int count_of(const WgradCfg (&)[N]) { return N; }

// Which kernel runs a weight gradient, on which tiles, row splits and grid: decided once per call by plan_wgrad and read by
// the launch (launch_wgrad), the argument filling and every query (dv_conv3d_wgrad_tile ... dv_conv3d_bn_in_ok).
enum {
  WGRAD_GENERIC,        // conv_wgrad_kernel: register-staged gathers (8-byte vectors, windows > 8, operands >= 2 GiB)
  WGRAD_DMA,            // conv_wgrad_dma_kernel, configuration `cfg`
  WGRAD_F32S,           // conv_wgrad_f32s_kernel (conv_experiments.hip), configuration `f32s`: DUALVAR_WGRAD_F32S only
  WGRAD_TM,             // the LDS-staged forms (conv_tap_wgrad.hip), `kind` 1 - 4
};
struct WgradPlan {
  int route;                  // WGRAD_*
  int kind;                   // WGRAD_TM: wgrad_tm_kind's form, else 0
  const WgradCfg* cfg;        // WGRAD_DMA
  int f32s;                   // WGRAD_F32S
  int M, J;                   // rows of dY; columns of dW = taps x cin_pitch (its row pitch)
  int BI, BJ, nti, ntj;       // tile of dW (rows = output channels) and tiles per axis
  int splits, rows_per_split; // row splits: each writes its own slab of the workspace when there are several
  int nchunks, chunks_per_split;      // WGRAD_TM: steps in all / per row split
  int grid;                   // workgroups of the launch
  int gvb;                    // gather vector bytes of x
  int64_t x_bytes, dy_bytes;  // extents of the operands (< 2 GiB on every route but WGRAD_GENERIC)
  long long slab_stride;      // elements
  int64_t workspace_bytes;    // 0: one split, dW += tile
  bool bn_apply_ok;           // the kernel has a form that carries dv_conv3d_wgrad_bn
  bool bn_in_ok;              // ... dv_conv3d_wgrad_bn_in (BatchNorm on load)
};

// The LDS-staged form that takes the problem, or 0.  1: stride 1, 3x1x1, T = 2 / 4; 2: the 7x1x1 / stride-2 stem conv (8 -> 4
// frames); 3: stride 1, 1x3x3, padding 1; 4: the pixel-pair RGB stem conv.  fits: both operands' extents are < 2 GiB.
static int wgrad_tm_kind(const dv_conv_desc* d, bool fits) {
  static const int on = env_int("DUALVAR_WGRAD_TM", 1);           // (A/B switch; 2: temporal forms only)
  if (!on || d->dtype != DV_F32 || f32_exact() || !fits) return 0;
  if (d->cin_pitch % 8 || d->cout_pitch % 8) return 0;
  // (DUALVAR_CONV_TAP_GRID <= 1, the test knob of the LDS-staged kernels, also lets tiny problems through: tools/tap_check.py)
  if ((int64_t)d->N * d->To * d->Ho * d->Wo < (conv_tap_any_size() ? 1 : 8192)) return 0;
  // 4: the pixel-pair RGB stem conv: window 1 x 7 x 4 over 8-channel pixel pairs, stride (1, 2, 1), no padding
  if (on != 2 && d->kt == 1 && d->kh == 7 && d->kw == 4 && d->st == 1 && d->sh == 2 && d->sw == 1 && !d->pt && !d->ph && !d->pw &&
      d->cin_pitch == 8 && d->ldx == 8 && d->Wo <= 64 && d->Wi <= 68)
    return 4;
  if (d->sh != 1 || d->sw != 1) return 0;
  int kind = 0;
  if (d->kh == 1 && d->kw == 1 && !d->ph && !d->pw) {
    if (d->kt == 3 && d->st == 1 && d->pt == 1 && d->To == d->Ti && (d->Ti == 2 || d->Ti == 4)) kind = 1;
    else if (d->kt == 7 && d->st == 2 && d->pt == 3 && d->Ti == 8 && d->To == 4) kind = 2;
  } else if (on != 2 && d->kt == 1 && d->st == 1 && !d->pt && d->kh == 3 && d->kw == 3 && d->ph == 1 && d->pw == 1 &&
             d->Hi >= 2 && d->Wi >= 2) {
    // the spatial form pays on the large maps whose channel count fills its 64-channel x tiles: Conv_2c 710 -> 542 us, Mixed_3c
    // (128 channels) 310 -> 240; Mixed_3b (96 channels: a half-empty second tile) 148 -> 156 and the 12 544-row levels 89 -> 87
    // stay on conv_wgrad_dma_kernel (isolated, one box)
    const int64_t rows = (int64_t)d->N * d->Ti * d->Hi * d->Wi;
    if ((conv_tap_any_size() && d->cin_pitch >= 16) || (rows >= 50000 && (d->cin_pitch + 63) / 64 * 64 * 10 <= d->cin_pitch * 11)) kind = 3;
  }
  return kind;
}

static WgradPlan plan_wgrad(const dv_conv_desc* d) {
  WgradPlan p{};
  const int M = p.M = d->N * d->To * d->Ho * d->Wo;
  const int J = p.J = d->kt * d->kh * d->kw * d->cin_pitch;
  const int es = d->dtype == DV_F32 ? 4 : 2;
  p.gvb = gather_bytes(d->dtype, d->cin_pitch);
  p.x_bytes = extent_bytes((int64_t)d->N * d->Ti * d->Hi * d->Wi, d->ldx, d->cin_pitch, es);
  p.dy_bytes = extent_bytes(M, d->ldy, d->cout_pitch, es);
  p.slab_stride = ((long long)d->Cout * J + 63) / 64 * 64;
  const bool fits = fits_descriptor(p.x_bytes) && fits_descriptor(p.dy_bytes);
  const bool dma = p.gvb == 16 && d->kt <= 8 && d->kh <= 8 && d->kw <= 8 && fits;
  constexpr int minrows = 256;           // fewest rows of a row split, see below
  int per_cu = 3;
  if ((p.kind = wgrad_tm_kind(d, fits))) {
    // 64 x 64 (n, c) tiles carrying all three taps; the row splits are ranges of 64 / T-pixel steps: one round of three
    // co-resident workgroups per CU, at least 8 steps each, and not more than the slab traffic pays for (as below)
    p.route = WGRAD_TM;
    p.bn_apply_ok = p.kind == 4;                                   // conv_wgrad_pp_kernel<BNA>
    p.bn_in_ok = p.kind == 1 || p.kind == 2;                       // conv_wgrad_tm_kernel<.., BNL>
    const int bc = p.kind == 2 ? 32 : 64;                          // channel tile of x (conv_tap_wgrad.hip)
    p.BI = 64; p.BJ = (p.kind == 3 ? 3 : d->kt) * bc;
    p.nti = (d->Cout + 63) / 64; p.ntj = (d->cin_pitch + bc - 1) / bc;
    const int krows = p.kind == 3 ? 3 : 1;                         // spatial: one workgroup per kernel row dh
    if (p.kind == 4) { p.BJ = 224; p.ntj = 1; }
    const int pxs = 64 / d->To;                                   // kinds 1, 2: steps of 64 / T pixels
    p.nchunks = p.kind == 4 ? d->N * d->To * d->Ho                // output lines
              : p.kind == 3 ? (M + 63) / 64                       // 64-row steps
              : (int)(((int64_t)d->N * d->Hi * d->Wi + pxs - 1) / pxs);
    int splits = std::max(1, ((p.kind == 2 || p.kind == 4) ? 512 : 768) / (p.nti * p.ntj * krows));  // (the stem forms: two workgroups per CU)
    splits = std::min(splits, std::max(1, p.nchunks / 8));
    const double slab_us = 8.0 * d->Cout * (double)J / 4e6;
    const int s_opt = (int)(std::sqrt(p.nchunks * 1.2 / slab_us) + 0.5);          // ~1.2 us per step of one workgroup
    splits = std::max(1, std::min(splits, s_opt));
    p.chunks_per_split = (p.nchunks + splits - 1) / splits;
    p.splits = (p.nchunks + p.chunks_per_split - 1) / p.chunks_per_split;
    p.rows_per_split = p.chunks_per_split * 64;
    p.grid = p.nti * p.ntj * p.splits * krows;
    p.workspace_bytes = p.splits > 1 ? (int64_t)p.splits * p.slab_stride * 4 : 0;
    return p;
  }
  // DUALVAR_WGRAD_F32S = 0 | 2: conv_wgrad_f32s_kernel (conv_experiments.hip) in its 64 x 256 / 128 x 128 form for every fp32
  // weight gradient (sweeps: tools/wgrad_sweep.sh).  Not selected by default: isolated it gains 8 - 10 % on the layers whose
  // shape its tiles fit (128-channel layers on 128 x 128, the 7x1x1 stem conv on 64 x 256) and nothing elsewhere, and a
  // per-layer rule built on that measured 19.39 vs 19.39 ms on the whole step ("Round 3").
  static const int f32s_force = env_int("DUALVAR_WGRAD_F32S", -1);
  const bool split_mode = d->dtype == DV_F32 && !f32_exact();
  if (dma && split_mode && (f32s_force == 0 || f32s_force == 2)) {
    p.route = WGRAD_F32S;
    p.f32s = f32s_force;
    per_cu = std::max(1, std::min(2, 163840 / dvx_wgrad_f32s_shape(p.f32s, &p.BI, &p.BJ)));
  } else if (dma) {
    // candidate with the least estimated time: LDS-fill bytes at ~18 TB/s chip-wide against padded MFMA work at ~2/3 of
    // peak; a configuration whose tiles cannot even fill the chip once (few rows) pays for the idle CUs
    p.route = WGRAD_DMA;
    const WgradCfg* tab = d->dtype == DV_F32 ? kWgF32 : kWgBf16;
    const int ncfg = d->dtype == DV_F32 ? count_of(kWgF32) : count_of(kWgBf16);
    double best = 0;
    for (int c = 0; c < ncfg; ++c) {
      const WgradCfg& k = tab[c];
      const int nti = (d->Cout + k.BI - 1) / k.BI, ntj = (J + k.BJ - 1) / k.BJ;
      const double fill = (double)M * nti * ntj * (k.BI + k.BJ) * es / 18e12;
      const double mfma = 2.0 * M * (double)(nti * k.BI) * (ntj * k.BJ) / (d->dtype == DV_F32 ? 120e12 : 1600e12);
      const int wgs_per_cu = wgrad_wgs_per_cu(es, k.BI, k.BJ, k.WVI * k.WVJ, k.NS);
      const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(256 * wgs_per_cu / (nti * ntj), (M + minrows - 1) / minrows));
      const double wgs = (double)nti * ntj * sp;
      const double t = std::max(fill, mfma) * std::max(1.0, 256.0 / wgs);
      if (!p.cfg || t < best) { best = t; p.cfg = &k; per_cu = wgs_per_cu; }
    }
    p.BI = p.cfg->BI; p.BJ = p.cfg->BJ;
    p.bn_apply_ok = split_mode && p.cfg->bna;
  } else {
    // tile heights 64 or 128: whichever pads Cout less (144 -> 3 x 64 rather than 2 x 128)
    p.route = WGRAD_GENERIC;
    const bool narrow = (d->Cout + 63) / 64 * 64 < (d->Cout + 127) / 128 * 128;
    p.BI = narrow ? 64 : 128;
    p.BJ = narrow ? 128 : 64;
  }
  p.nti = (d->Cout + p.BI - 1) / p.BI;
  p.ntj = (J + p.BJ - 1) / p.BJ;
  const int tiles = p.nti * p.ntj;
  // Row splits: ONE round of co-resident workgroups (256 CUs x the workgroups per CU the kernel's LDS / registers admit)
  // -- a grid of 1.5 rounds leaves half the chip idle for the second one -- but at least `minrows` rows each: a split's
  // partial tile costs as much traffic as ~128 rows of its inputs.
  const int tgt = 256 * per_cu;
  int splits = std::min(tgt / tiles, (M + minrows - 1) / minrows);       // round down: never more workgroups than fit at once
  // ... and not more than pays: every split writes (and the reduce re-reads) a whole partial dW.  With S splits a workgroup
  // runs M/(32 S) steps of ~t_step and the slabs cost 2 S |W| 4 bytes at ~4 TB/s: the sum is least at
  // S = sqrt(M/32 * t_step / (8 |W| / 4e6 us)).  (Layers with few rows and a large dW -- Mixed_4/5 -- had slab traffic of
  // 3x their operands.)
  const double t_step = d->dtype == DV_F32 ? 1.5 : 0.7;                          // us per 32-row step of one workgroup
  const double slab_us = 8.0 * d->Cout * (double)J / 4e6;
  const int s_opt = (int)(std::sqrt(M / 32.0 * t_step / slab_us) + 0.5);
  splits = std::max(1, std::min(splits, s_opt));
  p.rows_per_split = ((M + splits - 1) / splits + 31) / 32 * 32;
  p.splits = (M + p.rows_per_split - 1) / p.rows_per_split;
  p.grid = tiles * p.splits;
  p.workspace_bytes = p.splits > 1 ? (int64_t)p.splits * p.slab_stride * 4 : 0;
  return p;
}

extern "C" int dv_conv3d_wgrad_tile(const dv_conv_desc* d, int32_t* rows, int32_t* cols, int32_t* splits) {
  if (!d || !rows || !cols || !splits) return DV_EINVAL;
  if (const int rc = check_desc(d)) return rc;
  const WgradPlan p = plan_wgrad(d);
  *rows = p.BI; *cols = p.BJ; *splits = p.splits;
  return DV_OK;
}

extern "C" int64_t dv_conv3d_wgrad_workspace(const dv_conv_desc* d) {
  return check_desc(d) ? 0 : plan_wgrad(d).workspace_bytes;
}

extern "C" int dv_conv3d_wgrad_bn_ok(const dv_conv_desc* d) {
  return d && !check_desc(d) && plan_wgrad(d).bn_apply_ok ? 1 : 0;
}

bool dvwg_bn_in_ok(const dv_conv_desc* d) { return plan_wgrad(d).bn_in_ok; }      // (dv_conv3d_bn_in_ok, conv.hip; d is checked)

static BnBwdFuse bn_bwd_fuse(const dv_bn_bwd* bn) {
  BnBwdFuse f{};
  if (!bn) return f;
  f.x = bn->x; f.mean = bn->mean; f.invstd = bn->invstd; f.gamma = bn->gamma; f.scale = bn->scale; f.shift = bn->shift;
  f.sums = bn->sums; f.dgamma = bn->dgamma; f.dbeta = bn->dbeta; f.inv_count = bn->inv_count; f.dscale = bn->dparam_scale;
  f.rep = bn->n_rep; f.mask = (bn->flags & DV_NO_RELU_MASK) ? 0 : 1;
  return f;
}

// The argument block of one weight gradient: `t` on WGRAD_TM, else `aa` (aa.w alone for conv_wgrad_kernel).
static void fill_wgrad_args(const dv_conv_desc* d, const WgradPlan& p, const void* x, const void* dy, float* dw, float* slab,
                            const dv_bn_bwd* bn, const dv_bn_in* bn_in, WgradDmaArgs& aa, TmWgradArgs& t) {
  if (p.route != WGRAD_TM) {
    WgradArgs& a = aa.w;
    fill_geom(d, MODE_FWD, a.g);
    a.x = x; a.dy = dy; a.dw = dw; a.slab = slab; a.slab_stride = p.slab_stride;
    a.M = p.M; a.Cout = d->Cout; a.CoutP = d->cout_pitch; a.J = p.J;
    a.ldx = d->ldx; a.ldy = d->ldy; a.ldw = p.J;
    a.nti = p.nti; a.ntj = p.ntj; a.rows_per_split = p.rows_per_split;
    a.perm = make_row_perm(d->kt > 1 && d->To > 1, d->To, d->Ho * d->Wo);
    aa.x_bytes = (int)p.x_bytes; aa.dy_bytes = (int)p.dy_bytes;           // (read by the DMA kernels only)
    aa.bn = bn_bwd_fuse(bn);
    return;
  }
  t.x = x; t.dy = dy; t.dw = dw; t.slab = slab; t.slab_stride = p.slab_stride;
  t.S = d->Hi * d->Wi; t.NQ = d->N * t.S; t.T = d->To; t.kind = p.kind;
  t.Cout = d->Cout; t.CoutP = d->cout_pitch; t.CP = d->cin_pitch;
  t.ldx = d->ldx; t.ldy = d->ldy; t.ldw = p.J;
  t.nti = p.nti; t.ntc = p.ntj; t.nchunks = p.nchunks; t.chunks_per_split = p.chunks_per_split;
  t.x_bytes = (int)p.x_bytes; t.dy_bytes = (int)p.dy_bytes;
  t.fS = make_fastdiv((uint32_t)t.S);
  t.M = p.M; t.H = d->Hi; t.W = d->Wi;
  t.fW = make_fastdiv((uint32_t)d->Wi);
  t.fH = make_fastdiv((uint32_t)(p.kind == 4 ? d->Ho : d->Hi));  // kind 4: line -> (image, output line)
  t.Wo = d->Wo; t.Ho = d->Ho; t.Wp = d->Wi; t.Hp = d->Hi;
  t.bn = bn_bwd_fuse(bn);
  if (bn_in) { t.in_scale = bn_in->scale; t.in_shift = bn_in->shift; t.in_C = d->Cin; t.in_relu = (bn_in->flags & DV_RELU) ? 1 : 0; }
}

template <typename T, int GVB>
static void launch_wgrad_generic(const WgradPlan& p, const WgradArgs& a, hipStream_t s) {
  if (p.BI == 64) hipLaunchKernelGGL((conv_wgrad_kernel<T, GVB, 64, 128>), dim3(p.grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<T, GVB, 128, 64>), dim3(p.grid), dim3(256), 0, s, a);
}
// the launch of one weight gradient along its plan
static void launch_wgrad(const WgradPlan& p, int dtype, const WgradDmaArgs& aa, const TmWgradArgs& t, hipStream_t s) {
  switch (p.route) {
    case WGRAD_TM: dvw_wgrad_tm_launch(t, p.grid, s); break;
    case WGRAD_F32S: dvx_launch_wgrad_f32s(p.f32s, aa, p.grid, s); break;
    case WGRAD_DMA: p.cfg->launch(aa, p.grid, s); break;
    default:
      if (dtype == DV_F32) launch_wgrad_generic<float, 16>(p, aa.w, s);
      else if (p.gvb == 16) launch_wgrad_generic<bf16_t, 16>(p, aa.w, s);
      else launch_wgrad_generic<bf16_t, 8>(p, aa.w, s);
  }
}

// validate -> plan -> fill the arguments -> launch -> reduce the row splits' slabs
static int wgrad_impl(const dv_conv_desc* d, const void* x, const void* dy, float* dw, void* workspace,
                      int64_t workspace_bytes, const dv_bn_bwd* bn, void* stream, const dv_bn_in* bn_in = nullptr) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!x || !dy || !dw) return DV_EINVAL;
  if (!aligned16(dy) || !aligned16(dw) || (reinterpret_cast<uintptr_t>(x) & 7)) return DV_EALIGN;
  const WgradPlan p = plan_wgrad(d);
  if (bn_in) {
    if (bn || !bn_in->scale || !bn_in->shift) return DV_EINVAL;
    if (!p.bn_in_ok) return DV_EUNSUPPORTED;
  }
  if (bn) {
    if (!bn->x || !bn->mean || !bn->invstd || !bn->gamma || !bn->sums || bn->n_rep <= 0) return DV_EINVAL;
    if ((bn->dgamma == nullptr) != (bn->dbeta == nullptr)) return DV_EINVAL;
    if (!(bn->flags & DV_NO_RELU_MASK) && (!bn->scale || !bn->shift)) return DV_EINVAL;
    if (bn->ldx != d->ldy) return DV_EINVAL;
    if (!aligned16(bn->x)) return DV_EALIGN;
    if (!p.bn_apply_ok) return DV_EUNSUPPORTED;
  }
  const int64_t need = p.workspace_bytes;
  if (need && (!workspace || workspace_bytes < need)) return DV_EINVAL;
  if (need && !aligned16(workspace)) return DV_EALIGN;
  if (p.gvb == 16 && !aligned16(x)) return DV_EALIGN;
  float* slab = need ? reinterpret_cast<float*>(workspace) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  WgradDmaArgs aa;
  TmWgradArgs t;
  fill_wgrad_args(d, p, x, dy, dw, slab, bn, bn_in, aa, t);
  launch_wgrad(p, d->dtype, aa, t, s);
  // (folding this reduce into the weight-gradient kernel -- VERDICT round 3 item 6 -- was priced first: with EVERY reduce launch
  // skipped the step went 17.69 -> 17.66 ms, two A/B pairs on one box; the launches overlap on the side stream.  Not built.)
  if (need) {
    const long long n4 = (long long)d->Cout * p.J / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n4 + 15) / 16)), dim3(256), 0, s, slab, p.slab_stride,
                       p.splits, dw, n4);
  }
  return dv_launch_status();
}

extern "C" int dv_conv3d_wgrad(const dv_conv_desc* d, const void* x, const void* dy, float* dw, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  return wgrad_impl(d, x, dy, dw, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int dv_conv3d_wgrad_bn(const dv_conv_desc* d, const void* x, const void* g, float* dw, void* workspace,
                                  int64_t workspace_bytes, const dv_bn_bwd* bn, void* stream) {
  if (!bn) return DV_EINVAL;
  return wgrad_impl(d, x, g, dw, workspace, workspace_bytes, bn, stream);
}

extern "C" int dv_conv3d_wgrad_bn_in(const dv_conv_desc* d, const void* x_bn, const dv_bn_in* bn, const void* dy, float* dw,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (!bn) return DV_EINVAL;
  return wgrad_impl(d, x_bn, dy, dw, workspace, workspace_bytes, nullptr, stream, bn);
}
