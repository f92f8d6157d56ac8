// 3-D convolution, forward and data gradient: the host layer.  NDHWC activations, K-contiguous packed weights; see
// include/dualvar_hip.h.  Both are implicit GEMMs over a (virtual) im2col matrix A[row m][k = tap*CP + c]:
//   fwd  : Y[m][n]  = sum_k A_x [m][k] * Wf[n][k]            m = output position
//   dgrad: dX[m][c] = sum_k A_dy[m][k] * Wd[c][k]            m = input position, k=(tap,n)
// route_conv decides once per call which kernel runs it -- conv_gemm.hpp's or conv_tap.hip's, through conv_common.hpp's interface
// section -- and the entry points and kernel-choice queries all read that route.  The weight gradient is conv_wgrad.hip.
#include "conv_common.hpp"
#include "../../include/dualvar_conv_pair.h"

// ---- pre-split weights of the fp32 split mode (DV_W3) ---------------------------------------------------------------------
static int w3_rows(int n) { return (n + 127) / 128 * 128; }                         // rows incl. padding (any tile fits)
static int64_t w3_bytes(int n, int ktot) { return (int64_t)((ktot + 15) / 16) * 2 * w3_rows(n) * 48; }

namespace {
// one thread per (K tile, k half, row): 8 floats of W[row][kt*16 + 8h ..] -> hi | mid | lo, 48 bytes
__global__ __launch_bounds__(256) void pack_w3_kernel(const float* __restrict__ base, unsigned char* __restrict__ out_base,
                                                      const dv_w3_desc* __restrict__ descs, const int2* __restrict__ block_map) {
  const int2 bm = block_map[blockIdx.x];                     // (descriptor, first unit of this block)
  const dv_w3_desc d = descs[bm.x];
  const int npad = (d.N + 127) / 128 * 128;
  const long long unit = (long long)bm.y + threadIdx.x;      // unit = (kt * 2 + h) * npad + n
  const long long units = (long long)((d.Ktot + 15) / 16) * 2 * npad;
  if (unit >= units) return;
  const int n = (int)(unit % npad);
  const int kh = (int)(unit / npad), k0 = (kh >> 1) * 16 + (kh & 1) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (n < d.N && k0 + e < d.Ktot) ? base[d.src_off + (long long)n * d.Ktot + k0 + e] : 0.f;
  const Split3 s3 = split3(v);
  bf16x8* o = reinterpret_cast<bf16x8*>(out_base + d.dst_off + unit * 48);
  o[0] = s3.hi; o[1] = s3.mid; o[2] = s3.lo;
}
}  // namespace

extern "C" int64_t dv_w3_bytes(int32_t rows, int32_t ktot) { return rows > 0 && ktot > 0 ? w3_bytes(rows, ktot) : 0; }

extern "C" int dv_pack_w3(const float* base, void* out_base, const dv_w3_desc* descs, const int32_t* block_map, int32_t n_blocks,
                          void* stream) {
  if (!base || !out_base || !descs || !block_map || n_blocks <= 0) return DV_EINVAL;
  hipLaunchKernelGGL(pack_w3_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, base, (unsigned char*)out_base, descs,
                     reinterpret_cast<const int2*>(block_map));
  return dv_launch_status();
}

static int pick_bn(int np) {
  if (np <= 32) return 32;
  if (np <= 64) return 64;
  int w128 = (np + 127) / 128 * 128, w64 = (np + 63) / 64 * 64;
  return (w128 <= w64) ? 128 : 64;
}

// Tile rows: 128, or 64 when a 128-row grid would leave most CUs with fewer than ~4 workgroups (the K loop is
// latency bound at low occupancy; twice as many, half as tall workgroups hide it)
static int pick_bm(int M, int ntn) {
  return ((int64_t)((M + 127) / 128) * ntn >= 1024) ? 128 : 64;
}

// Tile (rows x columns) of the fwd / dgrad GEMM over M rows and NP (padded) columns: columns 32 / 64 / 128 by least
// padding, rows 128 when that still gives >= 1024 workgroups, else 64.  (96- and 192-column tiles -- wave tiles 32x96
// and 64x96 -- were measured too: 15-20 % faster on random data in isolation, but equal within noise inside the real
// training step, where post-ReLU activations are half zeros and the clocks are higher; not kept.)
// fp32 through the bf16 split (split3): every fragment costs ~44 vector instructions to split, so the kernel is bound
// by the vector ALU unless a fragment feeds enough MFMAs -- 256 x 64 tiles (wave tiles 64x64: 1 fragment per 32x32 block
// instead of the 1.5 of 128 x 64) wherever the grid still fills the chip twice over (c2c 1x3x3 forward 664 -> 609 us;
// a 256 x 128 tile with 128 x 64 wave tiles spills registers and is far slower).
static void pick_tile(int dtype, int M, int NP, int& bm, int& bn) {
  bn = pick_bn(NP);
  const int ntn = (NP + bn - 1) / bn;
  bm = pick_bm(M, ntn);
  if (dtype == DV_F32 && !f32_exact() && bm == 128 && bn == 64 && (int64_t)((M + 255) / 256) * ntn >= 512) bm = 256;
  // Few rows (the 1 152-row layers of Mixed_5b/5c: 18 row tiles): 128-column tiles leave three quarters of the CUs without a
  // workgroup while each busy CU runs one latency-bound K loop -- narrower tiles until the grid covers the chip
  constexpr int fill = 256;
  if (bm == 64) {
    const int64_t mt = (M + 63) / 64;
    while (bn > 32 && mt * ((NP + bn - 1) / bn) < fill) bn >>= 1;
  }
}

// the conv_gemm form for a launch over `a` with tile bm x bn
static GemmForm gemm_form(int dtype, const ConvArgs& a, int bm, int bn) {
  GemmForm f{};
  f.bm = bm; f.bn = bn; f.ns = 2;
  f.gvb = gather_bytes(dtype, a.g.CP);
  // uniform-tap gathers: every K-step (64 bytes: 32 bf16 / 16 f32) inside one tap, tap bit mask in one register.
  // f32: for the pre-split-weight kernels (the fp32 split mode's hot path; its K loop is bound by vector instructions)
  const int bke = dtype == DV_F32 ? 16 : 32;
  f.gm = f.gvb == 16 && a.g.CP % bke == 0 && a.g.kt * a.g.kh * a.g.kw <= 32;
  if (dtype == DV_F32) {
    f.split = !f32_exact();
    f.wf = f.split && (a.flags & DV_W3);
    f.gm = f.gm && f.wf;          // (only the pre-split-weight kernels are built with uniform-tap gathers)
    f.bnl = f.wf && f.gm && a.in_scale != nullptr;
    // (four or six stages for the small grids, as for bf16 below, were measured SLOWER here: Mixed_5c 1x3x3 forward 57 -> 68 -> 71
    // us; with one workgroup per CU the K step is bound by its own ds_read -> split -> MFMA chain, not by the DMA round trip)
    return f;
  }
  // Two LDS stages where the grid fills the chip several times over: there three to six stages measured equal or slower
  // (they cost resident workgroups, and the K loop is issue bound).  Launches of at most ~2 workgroups per CU (64-row tiles
  // of the 12 544- and 1 152-row layers) are latency bound instead -- one workgroup per CU waits out every DMA round trip --
  // and get four stages: those layers 252 -> 200 us (1 152 rows) and 581 -> 541 us (12 544 rows) per pass, step 10.53 ->
  // 10.35 ms.  Three stages, and six on the smallest grids, were measured equal or slower.
  const int64_t grid = (int64_t)((a.NP + bn - 1) / bn) * ((a.M + bm - 1) / bm);
  if (f.gvb == 16 && bm == 64 && grid <= 512) f.ns = 4;
  return f;
}

// Taps that fall into the padding for EVERY row of the launch contribute nothing: run the window of the live taps instead
// (per axis a contiguous range [lo, hi]).  Mixed_5b / 5c of S3D-G at 8-frame clips have ONE frame left: their 3x1x1 convs
// (padding 1) keep one tap of three -- a third of the K loop.  Weights stay where they are: the kernel addresses a live tap
// at its original index (ConvArgs::cls_on == 2).  Stride-1 data gradients and forward convs; not for the generic-gather
// pre-split-weight path (its K tiles straddle taps).
static void trim_dead_taps(ConvArgs& a, int mode) {
  ConvGeom& g = a.g;
  if (a.cls_on || g.kt * g.kh * g.kw <= 1) return;
  if (mode == MODE_DGRAD && (g.st > 1 || g.sh > 1 || g.sw > 1)) return;
  if ((a.flags & DV_W3) && (g.CP % 16 != 0 || g.kt * g.kh * g.kw > 32)) return;
  auto live = [&](int k, int rdim, int sdim, int stride, int pad, int& lo, int& hi) {
    lo = k; hi = -1;
    for (int d = 0; d < k; ++d) {
      bool any = false;
      for (int o = 0; o < rdim && !any; ++o) {
        const int v = mode == MODE_FWD ? o * stride - pad + d : o + pad - d;
        any = v >= 0 && v < sdim;
      }
      if (any) { lo = std::min(lo, d); hi = std::max(hi, d); }
    }
  };
  int lt, ht, lh, hh, lw, hw;
  live(g.kt, g.rT, g.sT, g.st, g.pt, lt, ht);
  live(g.kh, g.rH, g.sH, g.sh, g.ph, lh, hh);
  live(g.kw, g.rW, g.sW, g.sw, g.pw, lw, hw);
  if (ht < lt || hh < lh || hw < lw) return;                   // (no live tap at all: leave it to the zero fill)
  if (ht - lt + 1 == g.kt && hh - lh + 1 == g.kh && hw - lw + 1 == g.kw) return;
  a.cls_on = 2;
  a.cst = a.csh = a.csw = 1; a.cot = a.coh = a.cow = 0;
  a.crt = lt; a.crh = lh; a.crw = lw; a.oKH = g.kh; a.oKW = g.kw; a.oT = g.rT; a.oH = g.rH; a.oW = g.rW;
  // tap d' = d - lo: forward t = o*s - p + d = o*s - (p - lo) + d'; data gradient t = o + p - d = o + (p - lo) - d'
  g.kt = ht - lt + 1; g.kh = hh - lh + 1; g.kw = hw - lw + 1;
  g.pt -= lt; g.ph -= lh; g.pw -= lw;
  g.Ktot = g.kt * g.kh * g.kw * g.CP;
}

// conv_gemm_ks_kernel (K split over the waves) takes a fwd / dgrad launch when the ordinary tiling leaves a small grid with a
// long K loop.  Returns the column tile (32 / 64) or 0.  DUALVAR_CONV_KS=0 switches it off (A/B runs).
static int ks_tile(int dtype, const ConvArgs& a, int bm) {
  constexpr int max_grid = 400, min_nk = 16;       // (a larger grid limit was measured slower: 19.54 -> 20.44 ms at 1024)
  if (!conv_ks() || dtype != DV_F32 || !(a.flags & DV_W3) || f32_exact() || a.cls_on == 1 || a.bn_x != nullptr || bm != 64) return 0;
  if (a.g.CP % 16 != 0 || a.g.kt * a.g.kh * a.g.kw > 32 || a.g.Ktot / 16 < min_nk) return 0;
  if (a.g.st > 1 || a.g.sh > 1 || a.g.sw > 1) return 0;       // (few-row layers are stride 1; keeps one gather form)
  const int64_t mt = (a.M + 63) / 64;
  const int64_t g32 = mt * ((a.NP + 31) / 32), g64 = mt * ((a.NP + 63) / 64);
  // one workgroup per CU (its four private pipelines fill the LDS): a grid of at most one round, and as many workgroups as that
  // allows; 64-column tiles when 32-column ones would need a second round
  if (g32 <= 256) return 32;
  if (g64 <= max_grid) return g64 <= 256 || g32 > max_grid ? 64 : 32;
  return 0;
}

// the parity classes of a strided data gradient (ConvArgs::cls_on == 1): `a` holds the launch-wide fields; -> number of classes
static int dgrad_classes(const dv_conv_desc* d, const ConvArgs& a, ConvArgs (&out)[8]) {
  int n = 0;
  for (int rt = 0; rt < d->st; ++rt)
    for (int rh = 0; rh < d->sh; ++rh)
      for (int rw = 0; rw < d->sw; ++rw) {
        auto first = [](int r, int p, int st_) { return ((r - p) % st_ + st_) % st_; };   // smallest pos with (pos+p)%s == r
        const int ot = first(rt, d->pt, d->st), oh = first(rh, d->ph, d->sh), ow = first(rw, d->pw, d->sw);
        if (ot >= d->Ti || oh >= d->Hi || ow >= d->Wi) continue;
        ConvArgs& c = out[n++];
        c = a;                                                  // (ldw stays that of the whole window)
        ConvGeom& g = c.g;
        g.rT = (d->Ti - ot + d->st - 1) / d->st; g.rH = (d->Hi - oh + d->sh - 1) / d->sh; g.rW = (d->Wi - ow + d->sw - 1) / d->sw;
        g.kt = (d->kt - rt + d->st - 1) / d->st; g.kh = (d->kh - rh + d->sh - 1) / d->sh; g.kw = (d->kw - rw + d->sw - 1) / d->sw;
        g.st = g.sh = g.sw = 1;
        g.pt = (ot + d->pt - rt) / d->st; g.ph = (oh + d->ph - rh) / d->sh; g.pw = (ow + d->pw - rw) / d->sw;
        g.Ktot = g.kt * g.kh * g.kw * g.CP;
        g.dW = make_fastdiv((uint32_t)g.rW); g.dH = make_fastdiv((uint32_t)g.rH); g.dT = make_fastdiv((uint32_t)g.rT);
        c.M = d->N * g.rT * g.rH * g.rW;
        c.cls_on = 1; c.cst = d->st; c.csh = d->sh; c.csw = d->sw; c.cot = ot; c.coh = oh; c.cow = ow;
        c.crt = rt; c.crh = rh; c.crw = rw; c.oKH = d->kh; c.oKW = d->kw; c.oT = d->Ti; c.oH = d->Hi; c.oW = d->Wi;
      }
  return n;
}

// The ConvArgs of a forward (MODE_FWD) / data gradient (MODE_DGRAD) of `d`, all but the pointers and the fused extras (bias,
// stats, bn_*, in_*, the fp8 scales), which the entry points set.  fp8: the pointwise fp8 GEMMs (one-byte operands; DV_STATS /
// DV_ACCUM are their only flags).  DV_EUNSUPPORTED when no kernel takes the problem's extents or its DV_W3; `a` is complete
// either way (the kernel-choice queries read it too).
static int conv_args(const dv_conv_desc* d, int mode, ConvArgs& a, bool fp8 = false) {
  const bool fwd = mode == MODE_FWD;
  a = ConvArgs();
  fill_geom(d, mode, a.g);
  a.M = fwd ? d->N * d->To * d->Ho * d->Wo : d->N * d->Ti * d->Hi * d->Wi;
  a.N = fwd ? d->Cout : d->Cin;
  a.NP = fwd ? d->cout_pitch : d->cin_pitch;
  a.lds_ = fwd ? d->ldx : d->ldy;
  a.ldo = fwd ? d->ldy : d->ldx;
  a.flags = d->flags & (fp8 ? (fwd ? DV_STATS : DV_ACCUM) : fwd ? (DV_W3 | DV_BIAS | DV_RELU | DV_SIGMOID | DV_STATS) : (DV_W3 | DV_ACCUM));
  const bool w3 = (a.flags & DV_W3) != 0;
  a.ldw = w3 ? w3_rows(a.N) : a.g.Ktot;
  a.fCP = make_fastdiv((uint32_t)a.g.CP);
  const int es = fp8 ? 1 : d->dtype == DV_F32 ? 4 : 2;
  const int64_t src_rows = fwd ? (int64_t)d->N * d->Ti * d->Hi * d->Wi : (int64_t)d->N * d->To * d->Ho * d->Wo;
  const int64_t sb = extent_bytes(src_rows, a.lds_, a.g.CP, es);
  const int64_t wb = w3 ? w3_bytes(a.N, a.g.Ktot) : (int64_t)a.N * a.g.Ktot * es;
  const int64_t ob = extent_bytes(a.M, a.ldo, a.NP, 4);                // fp32 outputs: direct-store epilogue
  a.out_bytes = (d->dtype == DV_F32 && fits_descriptor(ob)) ? (int)ob : 0;
  const bool fits = fits_descriptor(sb) && fits_descriptor(wb) && d->kt <= 32 && d->kh <= 32 && d->kw <= 32 && d->kt * d->kh * d->kw <= 256;
  a.src_bytes = fits ? (int)sb : 0;
  a.w_bytes = fits ? (int)wb : 0;
  return fits && !(w3 && (d->dtype != DV_F32 || f32_exact())) ? DV_OK : DV_EUNSUPPORTED;
}

// Which kernel runs a forward / data gradient, with which tile: decided once per call by route_conv and read by the launch
// (launch_route) and by every kernel-choice query (dv_conv3d_tap_kind ... dv_conv3d_dgrad_bn_workspace).  WgradPlan / plan_wgrad /
// launch_wgrad (conv_wgrad.hip) are the same three for the weight gradient.  In particular `rows` fixes the layout of the BatchNorm
// partials dv_bn_reduce_stats reads.
enum {
  ROUTE_NONE,           // no kernel takes this call: DV_EUNSUPPORTED
  ROUTE_PP,             // the pixel-pair stem form (conv_tap.hip: conv_pp_fwd_kernel), forward only
  ROUTE_TAP,            // the LDS-staged input-tile kernel (conv_tap.hip), kind 1 spatial / 2 temporal
  ROUTE_TAP_CLASSES,    // strided data gradient, pre-split weights: every parity class on the temporal form
  ROUTE_KS,             // conv_gemm_ks_kernel: K split over the waves
  ROUTE_GEMM_CLASSES,   // strided data gradient without pre-split weights: conv_gemm per parity class
  ROUTE_GEMM,           // conv_gemm_kernel
};
struct ConvRoute {
  int path;             // ROUTE_*
  int kind;             // what dv_conv3d_tap_kind reports: 1 / 2 the LDS-staged kernel's form, 3 the pixel-pair form, else 0
  int rows;             // rows per tile = rows per BatchNorm partial (ROUTE_PP: lines per tile * Wo)
  int bm, bn;           // pick_tile over the whole problem (dv_conv3d_tile_shape)
  int ks_cols;          // ROUTE_KS: the column tile
  int ncls;             // ROUTE_*_CLASSES: parity classes (dgrad_classes)
  GemmForm gemm[8];     // ROUTE_GEMM: [0]; ROUTE_GEMM_CLASSES: one per class
};

// `a`: conv_args plus the call's extras (bn_x / bn_ws of the ordered fused BatchNorm reduce, in_scale of BatchNorm on load).
// Trims dead taps in `a` where the launch runs the trimmed window.
static ConvRoute route_conv(const dv_conv_desc* d, int mode, ConvArgs& a) {
  ConvRoute r{};
  pick_tile(d->dtype, a.M, a.NP, r.bm, r.bn);
  r.rows = r.bm;
  const bool w3 = (a.flags & DV_W3) != 0;
  if (w3 && (d->dtype != DV_F32 || f32_exact())) return r;
  const bool strided = d->st > 1 || d->sh > 1 || d->sw > 1;
  if (mode == MODE_DGRAD && strided && d->st <= 2 && d->sh <= 2 && d->sw <= 2 && d->kt >= d->st && d->kh >= d->sh && d->kw >= d->sw) {
    // one dense stride-1 launch per parity class of the input positions (see ConvArgs): every class has >= 1 tap
    ConvArgs cls[8];
    r.ncls = dgrad_classes(d, a, cls);
    if (w3) {
      // pre-split weights: every class on the LDS-staged input-tile kernel (conv_tap.hip, temporal form), or not at all
      for (int i = 0; i < r.ncls; ++i)
        if (!dvt_conv_tap_kind(cls[i], MODE_DGRAD)) return r;
      r.path = ROUTE_TAP_CLASSES; r.kind = 2; r.rows = dvt_conv_tap_bm(cls[0], 2);
      return r;
    }
    if (a.bn_ws) return r;
    for (int i = 0; i < r.ncls; ++i) {
      int bm, bn;
      pick_tile(d->dtype, cls[i].M, cls[i].NP, bm, bn);
      r.gemm[i] = gemm_form(d->dtype, cls[i], bm, bn);
    }
    r.path = ROUTE_GEMM_CLASSES;
    return r;
  }
  if (!a.in_scale) {
    trim_dead_taps(a, mode);
  } else if (!strided) {                                // BatchNorm on load: never on a trimmed window
    ConvArgs t = a;
    trim_dead_taps(t, mode);
    if (t.cls_on) return r;
  }
  if (d->dtype == DV_F32 && w3) {
    if (const int G = dvt_conv_pp_lines(a, mode)) {
      r.path = ROUTE_PP; r.kind = 3; r.rows = G * a.g.rW;
      return r;
    }
    if (const int k = dvt_conv_tap_kind(a, mode)) {
      r.path = ROUTE_TAP; r.kind = k; r.rows = dvt_conv_tap_bm(a, k);
      return r;
    }
    if (a.in_scale) {                                   // (the plain call would take the spatial LDS-staged form: keep it)
      ConvArgs p = a;
      p.in_scale = nullptr;
      if (dvt_conv_tap_kind(p, mode)) return r;
    }
  }
  if (a.bn_ws) return r;                                // (the ordered fused reduce exists on the LDS-staged kernel only)
  if ((r.ks_cols = ks_tile(d->dtype, a, r.bm))) {
    r.path = a.in_scale ? ROUTE_NONE : ROUTE_KS;        // (the K-split kernel applies no BatchNorm on load)
    return r;
  }
  r.gemm[0] = gemm_form(d->dtype, a, r.bm, r.bn);
  // BatchNorm on load on conv_gemm: its 256 x 64 uniform-tap pre-split-weight form only, no bias / activation
  if (a.in_scale && !(r.gemm[0].bnl && r.bm == 256 && r.bn == 64 && a.g.CP <= 256 && !(a.flags & (DV_BIAS | DV_RELU | DV_SIGMOID))))
    return r;
  r.path = ROUTE_GEMM;
  return r;
}

// the launches of one forward / data gradient along its route
static int launch_route(const dv_conv_desc* d, int mode, const ConvRoute& r, ConvArgs& a, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool fwd = mode == MODE_FWD;
  switch (r.path) {
    case ROUTE_PP: dvt_conv_pp_launch(a, r.rows / a.g.rW, s); break;
    case ROUTE_TAP: dvt_conv_tap_launch(a, mode, r.kind, r.rows, s); break;
    case ROUTE_KS: (fwd ? dvg_fwd_ks : dvg_dgrad_ks)(r.ks_cols, a, s); break;
    case ROUTE_GEMM: (fwd ? dvg_fwd_gemm : dvg_dgrad_gemm)(d->dtype, r.gemm[0], a, s); break;
    case ROUTE_TAP_CLASSES:
    case ROUTE_GEMM_CLASSES: {
      ConvArgs cls[8];
      dgrad_classes(d, a, cls);
      for (int i = 0; i < r.ncls; ++i) {
        if (r.path == ROUTE_TAP_CLASSES) dvt_conv_tap_launch(cls[i], MODE_DGRAD, r.kind, r.rows, s);
        else dvg_dgrad_gemm(d->dtype, r.gemm[i], cls[i], s);
      }
      break;
    }
    default: return DV_EUNSUPPORTED;
  }
  return dv_launch_status();
}

// the route of dv_conv3d_fwd (dgrad = 0) / dv_conv3d_dgrad (1) on this problem, as the kernel-choice queries report it
static ConvRoute query_route(const dv_conv_desc* d, int dgrad) {
  const int mode = dgrad ? MODE_DGRAD : MODE_FWD;
  if (check_desc(d)) {                  // (no route; the GEMM tile, as dv_conv3d_tile_shape / tile_rows have always reported it)
    ConvRoute r{};
    const int64_t m = dgrad ? (int64_t)d->N * d->Ti * d->Hi * d->Wi : (int64_t)d->N * d->To * d->Ho * d->Wo;
    pick_tile(d->dtype, (int)m, dgrad ? d->cin_pitch : d->cout_pitch, r.bm, r.bn);
    r.rows = r.bm;
    return r;
  }
  ConvArgs a;
  conv_args(d, mode, a);
  return route_conv(d, mode, a);
}

extern "C" int dv_conv3d_tap_kind(const dv_conv_desc* d, int32_t dgrad) {
  return d ? query_route(d, dgrad).kind : 0;
}

extern "C" int dv_conv3d_tap_rows(const dv_conv_desc* d, int32_t dgrad) {
  if (!d) return 0;
  const ConvRoute r = query_route(d, dgrad);
  return r.kind ? r.rows : 0;
}

extern "C" int dv_conv3d_tile_rows(const dv_conv_desc* d) {
  return d ? query_route(d, 0).rows : DV_EINVAL;
}

extern "C" int dv_conv3d_stat_tiles(const dv_conv_desc* d) {
  if (!d) return DV_EINVAL;
  const int64_t m = (int64_t)d->N * d->To * d->Ho * d->Wo;
  const int bm = query_route(d, 0).rows;
  return (int)((m + bm - 1) / bm);
}

extern "C" int dv_conv3d_tile_shape(const dv_conv_desc* d, int32_t dgrad, int32_t* rows, int32_t* cols) {
  if (!d || !rows || !cols) return DV_EINVAL;
  const ConvRoute r = query_route(d, dgrad);
  *rows = r.bm; *cols = r.bn;
  return DV_OK;
}

extern "C" int dv_conv3d_ksplit_cols(const dv_conv_desc* d, int32_t dgrad) {
  if (!d) return 0;
  const ConvRoute r = query_route(d, dgrad);
  return r.path == ROUTE_KS ? r.ks_cols : 0;
}

// a forward call checked, its arguments in `a`, its route in `r`: all of dv_conv3d_fwd / dv_conv3d_fwd_bn_in but the launch
static int fwd_prepare(const dv_conv_desc* d, const void* x, const void* w, const float* bias, void* y, float* stats,
                       const dv_bn_in* bn_in, ConvArgs& a, ConvRoute& r) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!x || !w || !y) return DV_EINVAL;
  if ((d->flags & DV_BIAS) && !bias) return DV_EINVAL;
  if ((d->flags & DV_STATS) && !stats) return DV_EINVAL;
  if (!aligned16(w) || !aligned16(y) || (reinterpret_cast<uintptr_t>(x) & 7)) return DV_EALIGN;
  if (bn_in && (!bn_in->scale || !bn_in->shift)) return DV_EINVAL;
  if ((rc = conv_args(d, MODE_FWD, a))) return rc;
  a.src = x; a.w = w; a.out = y; a.bias = bias; a.stats = stats;
  if (bn_in) { a.in_scale = bn_in->scale; a.in_shift = bn_in->shift; a.in_C = d->Cin; a.in_relu = (bn_in->flags & DV_RELU) ? 1 : 0; }
  r = route_conv(d, MODE_FWD, a);
  if (r.path == ROUTE_NONE) return DV_EUNSUPPORTED;
  const int gvb = gather_bytes(d->dtype, d->cin_pitch);
  if (gvb == 16 && !aligned16(x)) return DV_EALIGN;
  const int esz = d->dtype == DV_F32 ? 4 : 2;
  if ((d->ldx * esz) % gvb || (a.ldw * esz) % gvb) return DV_EALIGN;
  return DV_OK;
}

static int fwd_impl(const dv_conv_desc* d, const void* x, const void* w, const float* bias, void* y, float* stats,
                    const dv_bn_in* bn_in, void* stream) {
  ConvArgs a;
  ConvRoute r;
  const int rc = fwd_prepare(d, x, w, bias, y, stats, bn_in, a, r);
  return rc ? rc : launch_route(d, MODE_FWD, r, a, stream);
}

// ---- two independent convs in one grid ---------------------------------------------------------------------------------------
// What the two routed calls share a grid on, or 0: the kind (1 spatial / 2 temporal) of the LDS-staged kernel when both select
// the identical instantiation of it and may share a grid (conv_tap.hip: conv_tap_pair_kernel); DV_PAIR_KS when both run
// conv_gemm_ks_kernel with the same column tile (which fixes its instantiation; that route never carries a fused reduce, a
// BatchNorm on load or a parity class).  The query and the three pair entries all ask here.
static int pair_kind(const ConvRoute& r0, const ConvArgs& a0, const ConvRoute& r1, const ConvArgs& a1, int mode) {
  if (r0.path == ROUTE_KS && r1.path == ROUTE_KS) return r0.ks_cols == r1.ks_cols ? DV_PAIR_KS : 0;
  if (r0.path != ROUTE_TAP || r1.path != ROUTE_TAP) return 0;
  return dvt_conv_tap_pair_inst(a0, r0.kind, r0.rows, a1, r1.kind, r1.rows, mode) ? r0.kind : 0;
}

// both members are checked before anything is launched; a pair that does not qualify runs its two launches in order
static int launch_pair(const dv_conv_desc* d0, ConvRoute& r0, ConvArgs& a0, const dv_conv_desc* d1, ConvRoute& r1, ConvArgs& a1,
                       int mode, void* stream) {
  if (const int kind = pair_kind(r0, a0, r1, a1, mode)) {
    if (kind != DV_PAIR_KS) dvt_conv_tap_launch_pair(a0, a1, mode, kind, r0.rows, (hipStream_t)stream);
    else (mode == MODE_FWD ? dvg_fwd_ks_pair : dvg_dgrad_ks_pair)(r0.ks_cols, a0, a1, (hipStream_t)stream);
    return dv_launch_status();
  }
  if (r0.path == ROUTE_NONE || r1.path == ROUTE_NONE) return DV_EUNSUPPORTED;
  const int rc = launch_route(d0, mode, r0, a0, stream);
  return rc ? rc : launch_route(d1, mode, r1, a1, stream);
}

extern "C" int dv_conv3d_fwd_bn_in_pair(const dv_conv_desc* d0, const void* x0, const dv_bn_in* bn0, const void* w0, void* y0,
                                        float* stats0, const dv_conv_desc* d1, const void* x1, const dv_bn_in* bn1, const void* w1,
                                        void* y1, float* stats1, void* stream) {
  ConvArgs a0, a1;
  ConvRoute r0, r1;
  int rc = fwd_prepare(d0, x0, w0, nullptr, y0, stats0, bn0, a0, r0);
  if (!rc) rc = fwd_prepare(d1, x1, w1, nullptr, y1, stats1, bn1, a1, r1);
  return rc ? rc : launch_pair(d0, r0, a0, d1, r1, a1, MODE_FWD, stream);
}

extern "C" int dv_conv3d_fwd_pair(const dv_conv_desc* d0, const void* x0, const void* w0, void* y0, float* stats0,
                                  const dv_conv_desc* d1, const void* x1, const void* w1, void* y1, float* stats1, void* stream) {
  return dv_conv3d_fwd_bn_in_pair(d0, x0, nullptr, w0, y0, stats0, d1, x1, nullptr, w1, y1, stats1, stream);
}

extern "C" int dv_conv3d_fwd(const dv_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                             float* stats, void* stream) {
  return fwd_impl(d, x, w, bias, y, stats, nullptr, stream);
}

extern "C" int dv_conv3d_fwd_bn_in(const dv_conv_desc* d, const void* x_bn, const dv_bn_in* bn, const void* w, void* y,
                                   float* stats, void* stream) {
  if (!bn) return DV_EINVAL;
  return fwd_impl(d, x_bn, w, nullptr, y, stats, bn, stream);
}

// ---- fp8 pointwise GEMMs (BASELINE configs[4]: the 1x1x1 convs of resnet_2d3d.py's bottleneck blocks) --------------------
static int check_fp8_desc(const dv_conv_desc* d) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (d->dtype != DV_BF16) return DV_EUNSUPPORTED;                       // the bf16 side of the GEMM (output, other tensors)
  if (d->kt != 1 || d->kh != 1 || d->kw != 1 || d->st != 1 || d->sh != 1 || d->sw != 1 || d->pt || d->ph || d->pw)
    return DV_EUNSUPPORTED;                                              // pointwise only
  if (d->cin_pitch % 16 || d->cout_pitch % 16) return DV_EALIGN;          // 16-byte gathers of fp8 channels
  return DV_OK;
}

// forward: src = x (e4m3), scales (x, w); data gradient: src = dy (e5m2), scales (dy, w)
static int fp8_impl(const dv_conv_desc* d, int mode, const void* src, const void* w, const float* sc_a, const float* sc_b, void* out,
                    float* stats, void* stream) {
  int rc = check_fp8_desc(d);
  if (rc) return rc;
  const bool fwd = mode == MODE_FWD;
  if (!src || !w || !out || !sc_a || !sc_b) return DV_EINVAL;
  if ((d->flags & DV_STATS) && fwd && !stats) return DV_EINVAL;
  if (!aligned16(src) || !aligned16(w) || !aligned16(out) || (fwd ? d->ldx : d->ldy) % 16 || ((fwd ? d->ldy : d->ldx) * 2) % 16)
    return DV_EALIGN;
  ConvArgs a;
  if ((rc = conv_args(d, mode, a, true))) return rc;
  a.src = src; a.w = w; a.out = out; a.stats = stats; a.sc_a = sc_a; a.sc_b = sc_b;
  GemmForm f{};
  pick_tile(DV_BF16, a.M, a.NP, f.bm, f.bn);
  f.gvb = 16; f.ns = 2;
  f.gm = a.g.CP % 64 == 0;      // one tap, channel pitch a multiple of the 64-element K tile: the uniform-tap gather (tap state in SGPRs)
  (fwd ? dvg_fwd_gemm_fp8 : dvg_dgrad_gemm_fp8)(f, a, (hipStream_t)stream);
  return dv_launch_status();
}

extern "C" int dv_conv3d_fwd_fp8(const dv_conv_desc* d, const void* x8, const void* w8, const float* scale_x,
                                 const float* scale_w, void* y, float* stats, void* stream) {
  return fp8_impl(d, MODE_FWD, x8, w8, scale_x, scale_w, y, stats, stream);
}

extern "C" int dv_conv3d_dgrad_fp8(const dv_conv_desc* d, const void* dy8, const void* wd8, const float* scale_dy,
                                   const float* scale_w, void* dx, void* stream) {
  return fp8_impl(d, MODE_DGRAD, dy8, wd8, scale_dy, scale_w, dx, nullptr, stream);
}

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// dv_conv3d_dgrad_bn, the ATOMIC form of the BatchNorm-backward reduce behind a data gradient (engine.FUSE_BN_REDUCE, off by
// default; rounds 1 - 3 carried it as a tail inside conv_gemm_kernel): a pass over the tile rows the data gradient has just
// written (L2-resident for the layers it was meant for) and the BatchNorm's input, sum g and sum g * xhat per column, one atomic
// per column and 128-row tile into replica tile % n_rep.  Measured a loss on every step it was tried on; kept as a
// tested entry point: it runs on every dv_conv3d_dgrad_bn call.  The ORDERED form that the default plan uses lives in conv_tap.hip
// (dv_conv3d_dgrad_bn_ws).
struct BnTailArgs {
  const void* g;          // dL/dy as written by the data gradient, [M][ldg]
  const void* x;          // the BatchNorm's input, [M][ldx]
  const float *mean, *invstd, *scale, *shift;
  float* sums;            // [n_rep][2][cp8(N)]
  int M, N, NP, ldg, ldx, n_rep, mask;
};

template <typename T>
__global__ __launch_bounds__(256) void dgrad_bn_tail_kernel(BnTailArgs a) {
  constexpr int BM = 128, BN = 64, NT = 256, EO = (int)sizeof(T), EPC = 16 / EO, CPT = BN * EO / 16, RG = NT / CPT;
  __shared__ float red[RG * 2 * BN];
  const int tid = threadIdx.x;
  const int ntn = (a.NP + BN - 1) / BN;
  const int tile_n = blockIdx.x % ntn, tile_m = blockIdx.x / ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int ch = tid % CPT, rg = tid / CPT, col0 = n0 + ch * EPC;
  float mu[EPC], is[EPC], sc[EPC], sh[EPC], s1[EPC], s2[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    const bool ok = col0 + e < a.N;
    mu[e] = ok ? a.mean[col0 + e] : 0.f;
    is[e] = ok ? a.invstd[col0 + e] : 0.f;
    sc[e] = (ok && a.mask) ? a.scale[col0 + e] : 0.f;
    sh[e] = (ok && a.mask) ? a.shift[col0 + e] : 0.f;
    s1[e] = s2[e] = 0.f;
  }
  if (col0 < a.NP) {
    const int rows_here = min(BM, a.M - m0);
    const T* g = reinterpret_cast<const T*>(a.g);
    const T* x = reinterpret_cast<const T*>(a.x);
    for (int r = rg; r < rows_here; r += RG) {
      const size_t row = (size_t)(m0 + r);
      float gq[EPC], xq[EPC];
      Pack16<T>::load(g + row * a.ldg + col0, gq);
      Pack16<T>::load(x + row * a.ldx + col0, xq);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float act = xq[e] * sc[e] + sh[e];          // the forward's expression (dv_bn_apply), same rounding
        const float gg = (a.mask && !(act > 0.f)) ? 0.f : gq[e];
        s1[e] += gg;
        s2[e] += gg * (xq[e] - mu[e]) * is[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    red[(rg * 2 + 0) * BN + ch * EPC + e] = s1[e];
    red[(rg * 2 + 1) * BN + ch * EPC + e] = s2[e];
  }
  __syncthreads();
  if (tid < BN && n0 + tid < a.N) {
    float t1 = 0.f, t2 = 0.f;
    for (int w = 0; w < RG; ++w) { t1 += red[(w * 2 + 0) * BN + tid]; t2 += red[(w * 2 + 1) * BN + tid]; }
    const int cpb = (a.N + 7) & ~7;
    float* dst = a.sums + (size_t)(tile_m % a.n_rep) * 2 * cpb + n0 + tid;
    atomicAdd(dst, t1);
    atomicAdd(dst + cpb, t2);
  }
}

}  // namespace

// the reduce over what the data gradient `c` has just written
static void launch_dgrad_bn_tail(const ConvArgs& c, int dtype, hipStream_t s) {
  BnTailArgs t;
  t.g = c.out; t.x = c.bn_x; t.mean = c.bn_mean; t.invstd = c.bn_invstd; t.scale = c.bn_scale; t.shift = c.bn_shift;
  t.sums = c.bn_sums; t.M = c.M; t.N = c.N; t.NP = c.NP; t.ldg = c.ldo; t.ldx = c.bn_ldx; t.n_rep = c.bn_rep; t.mask = c.bn_mask;
  const int grid = ((c.NP + 63) / 64) * ((c.M + 127) / 128);
  if (dtype == DV_F32) hipLaunchKernelGGL((dgrad_bn_tail_kernel<float>), dim3(grid), dim3(256), 0, s, t);
  else hipLaunchKernelGGL((dgrad_bn_tail_kernel<bf16_t>), dim3(grid), dim3(256), 0, s, t);
}

// a data-gradient call checked and its arguments in `a` (the route is the caller's: the atomic form routes the plain call)
static int dgrad_prepare(const dv_conv_desc* d, const void* dy, const void* wd, void* dx, const dv_bn_reduce* bnr, void* bn_ws,
                         int64_t bn_ws_bytes, ConvArgs& a) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!dy || !wd || !dx) return DV_EINVAL;
  if (bnr) {
    if (!bnr->x || !bnr->mean || !bnr->invstd || !bnr->sums || bnr->n_rep <= 0 || (d->flags & DV_ACCUM)) return DV_EINVAL;
    if (!(bnr->flags & DV_NO_RELU_MASK) && (!bnr->scale || !bnr->shift)) return DV_EINVAL;
    if (!aligned16(bnr->x) || bnr->ldx < d->cin_pitch || (bnr->ldx * (d->dtype == DV_F32 ? 4 : 2)) % 16) return DV_EALIGN;
  }
  if (d->st > 2 || d->sh > 2 || d->sw > 2) return DV_EUNSUPPORTED;
  if (d->cin_pitch % 8) return DV_EUNSUPPORTED;      // the RGB input never needs a data gradient
  if (!aligned16(dy) || !aligned16(wd) || !aligned16(dx)) return DV_EALIGN;
  const int esz = d->dtype == DV_F32 ? 4 : 2;
  if ((d->ldx * esz) % 16) return DV_EALIGN;
  if ((rc = conv_args(d, MODE_DGRAD, a))) return rc;
  a.src = dy; a.w = wd; a.out = dx;
  if (bnr) {
    a.bn_x = bnr->x; a.bn_ldx = bnr->ldx; a.bn_mean = bnr->mean; a.bn_invstd = bnr->invstd; a.bn_scale = bnr->scale;
    a.bn_shift = bnr->shift; a.bn_sums = bnr->sums; a.bn_rep = bnr->n_rep; a.bn_mask = (bnr->flags & DV_NO_RELU_MASK) ? 0 : 1;
    if (bn_ws) {                                       // dv_conv3d_dgrad_bn_ws: the ordered form, on the LDS-staged kernel only
      const int64_t need = dvt_bn_ws_floats(a.M, a.NP) * 4;
      const int64_t xb = extent_bytes(a.M, bnr->ldx, a.NP, 4);
      if (need <= 0) return DV_EUNSUPPORTED;             // (more tiles than the ticket region of the workspace holds)
      if (bn_ws_bytes < need || !aligned16(bn_ws) || !fits_descriptor(xb) || d->dtype != DV_F32) return DV_EINVAL;
      a.bn_ws = reinterpret_cast<float*>(bn_ws);
      a.bn_bytes = (int)xb;
    }
  }
  return DV_OK;
}

static int dgrad_impl(const dv_conv_desc* d, const void* dy, const void* wd, void* dx, const dv_bn_reduce* bnr, void* stream,
                      void* bn_ws = nullptr, int64_t bn_ws_bytes = 0) {
  ConvArgs a;
  int rc = dgrad_prepare(d, dy, wd, dx, bnr, bn_ws, bn_ws_bytes, a);
  if (rc) return rc;
  if (bnr && !bn_ws) {
    // dv_conv3d_dgrad_bn, the atomic form: the plain data gradient on whatever kernel takes it, then the reduce over what it wrote
    const ConvArgs tail = a;
    a.bn_x = nullptr;
    if ((rc = launch_route(d, MODE_DGRAD, route_conv(d, MODE_DGRAD, a), a, stream))) return rc;
    launch_dgrad_bn_tail(tail, d->dtype, (hipStream_t)stream);
    return dv_launch_status();
  }
  return launch_route(d, MODE_DGRAD, route_conv(d, MODE_DGRAD, a), a, stream);
}

extern "C" int dv_conv3d_dgrad(const dv_conv_desc* d, const void* dy, const void* wd, void* dx, void* stream) {
  return dgrad_impl(d, dy, wd, dx, nullptr, stream);
}

extern "C" int dv_conv3d_dgrad_bn(const dv_conv_desc* d, const void* dy, const void* wd, void* dx, const dv_bn_reduce* bn,
                                  void* stream) {
  if (!bn) return DV_EINVAL;
  return dgrad_impl(d, dy, wd, dx, bn, stream);
}

// bn0 / bn1: a member that carries the ordered fused BatchNorm-backward reduce (dv_conv3d_dgrad_bn_ws with `workspace`), or NULL.
// Such a member shares no grid: the two calls then run one after the other.
extern "C" int dv_conv3d_dgrad_pair(const dv_conv_desc* d0, const void* dy0, const void* wd0, void* dx0, const dv_bn_reduce* bn0,
                                    const dv_conv_desc* d1, const void* dy1, const void* wd1, void* dx1, const dv_bn_reduce* bn1,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  if ((bn0 || bn1) && !workspace) return DV_EINVAL;
  ConvArgs a0, a1;
  int rc = dgrad_prepare(d0, dy0, wd0, dx0, bn0, bn0 ? workspace : nullptr, bn0 ? workspace_bytes : 0, a0);
  if (!rc) rc = dgrad_prepare(d1, dy1, wd1, dx1, bn1, bn1 ? workspace : nullptr, bn1 ? workspace_bytes : 0, a1);
  if (rc) return rc;
  ConvRoute r0 = route_conv(d0, MODE_DGRAD, a0), r1 = route_conv(d1, MODE_DGRAD, a1);
  return launch_pair(d0, r0, a0, d1, r1, a1, MODE_DGRAD, stream);
}

extern "C" int dv_conv3d_pair_ok(const dv_conv_desc* d0, const dv_conv_desc* d1, int32_t mode) {
  if (!d0 || !d1 || check_desc(d0) || check_desc(d1)) return 0;
  if (mode & (DV_PAIR_BN_REDUCE0 | DV_PAIR_BN_REDUCE1)) return 0;
  const int m = (mode & DV_PAIR_DGRAD) ? MODE_DGRAD : MODE_FWD;
  if (m == MODE_DGRAD && (mode & (DV_PAIR_BN_IN0 | DV_PAIR_BN_IN1))) return 0;
  for (const dv_conv_desc* d : {d0, d1})
    if (m == MODE_DGRAD && (d->st > 2 || d->sh > 2 || d->sw > 2 || d->cin_pitch % 8)) return 0;      // (dv_conv3d_dgrad refuses these)
  static const float dummy = 0.f;
  ConvArgs a0, a1;
  if (conv_args(d0, m, a0) || conv_args(d1, m, a1)) return 0;
  if (mode & DV_PAIR_BN_IN0) a0.in_scale = &dummy;
  if (mode & DV_PAIR_BN_IN1) a1.in_scale = &dummy;
  const ConvRoute r0 = route_conv(d0, m, a0), r1 = route_conv(d1, m, a1);
  return pair_kind(r0, a0, r1, a1, m);
}

extern "C" int64_t dv_conv3d_dgrad_bn_workspace(const dv_conv_desc* d) {
  if (!d || check_desc(d) || (d->flags & DV_ACCUM)) return 0;
  const int path = query_route(d, 1).path;
  if (path != ROUTE_TAP && path != ROUTE_TAP_CLASSES) return 0;
  const int64_t rows = (int64_t)d->N * d->Ti * d->Hi * d->Wi;
  return dvt_bn_ws_floats(rows, d->cin_pitch) * 4;
}

extern "C" int dv_conv3d_dgrad_bn_ws(const dv_conv_desc* d, const void* dy, const void* wd, void* dx, const dv_bn_reduce* bn,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (!bn || !workspace) return DV_EINVAL;
  return dgrad_impl(d, dy, wd, dx, bn, stream, workspace, workspace_bytes);
}

// BatchNorm on load for both of a conv's consumers of x: the weight gradient has the form (the plan) and the forward's route
// takes it; 1: the forward runs on the LDS-staged kernel, 2: on conv_gemm_kernel
extern "C" int dv_conv3d_bn_in_ok(const dv_conv_desc* d) {
  if (!d || check_desc(d) || !dvwg_bn_in_ok(d)) return 0;
  static const float dummy = 0.f;
  ConvArgs a;
  conv_args(d, MODE_FWD, a);
  a.in_scale = &dummy;
  const int path = route_conv(d, MODE_FWD, a).path;
  return path == ROUTE_TAP ? 1 : path == ROUTE_GEMM ? 2 : 0;
}
