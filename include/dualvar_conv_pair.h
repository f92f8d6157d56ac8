/* Two independent convs in one grid, beside dualvar_hip.h: the pair entries of dv_conv3d_fwd / dv_conv3d_fwd_bn_in /
 * dv_conv3d_dgrad (csrc/conv.hip; kernels csrc/conv_gemm.hpp, csrc/conv_tap.hip).  Same conventions: plain C, device pointers, the stream last, 0 on success,
 * DV_E* (< 0) for refused arguments before anything is launched, a hipError_t (> 0) for a failed launch.
 * ctypes mirror: dualvar_amd/_lib.py PAIR_SIGNATURES (tests/test_conv_pair_host.py compares the two). */
#ifndef DUALVAR_CONV_PAIR_H
#define DUALVAR_CONV_PAIR_H
#include "dualvar_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The two separable branches of an Inception level (backbone/s3dg.py SepInception: 1x3x3
 * -> BatchNorm -> 3x1x1, twice) have the same geometry and mostly run the same instantiation of the LDS-staged input-tile kernel
 * (dv_conv3d_tap_kind); the small branch alone occupies a third of the chip and is almost all latency.  A pair entry runs both
 * problems in one launch: the first member's workgroups, then the second's, every workgroup exactly the code and the operands it
 * has in the single entry -- the outputs and BatchNorm partials are bit for bit those of the two single calls in order.  The
 * caller guarantees that the members are independent (neither reads or adds to what the other writes).
 * dv_conv3d_pair_ok: 0, or the route of the shared launch: the kind (1 spatial / 2 temporal, as dv_conv3d_tap_kind) when both members
 * route to that kernel with the same form, tile height, staging depth, tap count and BatchNorm-on-load choice; DV_PAIR_KS when
 * both run the "K split over the waves" kernel with the same column tile (dv_conv3d_ksplit_cols: the spatial branch convs of the
 * 1 152-row levels).  `mode`: DV_PAIR_* bits --
 * the data gradients (else the forwards) of d0 / d1; a member of dv_conv3d_fwd_bn_in_pair that has a dv_bn_in; a member of
 * dv_conv3d_dgrad_pair that has a dv_bn_reduce (never shares a grid: the fused reduces share one ticket workspace).  Parity-class
 * launches of strided data gradients never share a grid either.  A pair entry called where the query says 0 runs the two single
 * launches in order (dv_conv3d_fwd / _fwd_bn_in / _dgrad / _dgrad_bn_ws by the member's bn pointer) and returns their status;
 * both members' arguments are checked before anything is launched. */
enum { DV_PAIR_DGRAD = 1, DV_PAIR_BN_IN0 = 2, DV_PAIR_BN_IN1 = 4, DV_PAIR_BN_REDUCE0 = 8, DV_PAIR_BN_REDUCE1 = 16 };
enum { DV_PAIR_KS = 4 };               /* dv_conv3d_pair_ok's answer for a shared conv_gemm_ks launch */
int dv_conv3d_pair_ok(const dv_conv_desc* d0, const dv_conv_desc* d1, int32_t mode);
int dv_conv3d_fwd_pair(const dv_conv_desc* d0, const void* x0, const void* w_fwd0, void* y0, float* stats0,
                       const dv_conv_desc* d1, const void* x1, const void* w_fwd1, void* y1, float* stats1, void* stream);
int dv_conv3d_fwd_bn_in_pair(const dv_conv_desc* d0, const void* x_bn0, const dv_bn_in* bn0, const void* w_fwd0, void* y0,
                             float* stats0, const dv_conv_desc* d1, const void* x_bn1, const dv_bn_in* bn1, const void* w_fwd1,
                             void* y1, float* stats1, void* stream);
int dv_conv3d_dgrad_pair(const dv_conv_desc* d0, const void* dy0, const void* w_dgrad0, void* dx0, const dv_bn_reduce* bn0,
                         const dv_conv_desc* d1, const void* dy1, const void* w_dgrad1, void* dx1, const dv_bn_reduce* bn1,
                         void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
