// conv_gemm.hpp's kernels for the forward: the launches of what conv.hip's route decided (declared in conv_common.hpp)
#include "conv_gemm.hpp"
void dvg_fwd_gemm(int dtype, const GemmForm& f, ConvArgs& a, hipStream_t s) { launch_gemm_dt<MODE_FWD>(dtype, f, a, s); }
void dvg_fwd_gemm_fp8(const GemmForm& f, ConvArgs& a, hipStream_t s) { launch_gemm<fp8e4_t, MODE_FWD, 16>(f, a, s); }
void dvg_fwd_ks(int bn, ConvArgs& a, hipStream_t s) { launch_ks<MODE_FWD>(bn, a, s); }
void dvg_fwd_ks_pair(int bn, ConvArgs& a0, ConvArgs& a1, hipStream_t s) { launch_ks_pair<MODE_FWD>(bn, a0, a1, s); }
