// conv_gemm.hpp's kernels for the data gradient: the launches of what conv.hip's route decided (declared in conv_common.hpp)
#include "conv_gemm.hpp"
void dvg_dgrad_gemm(int dtype, const GemmForm& f, ConvArgs& a, hipStream_t s) { launch_gemm_dt<MODE_DGRAD>(dtype, f, a, s); }
void dvg_dgrad_gemm_fp8(const GemmForm& f, ConvArgs& a, hipStream_t s) { launch_gemm<fp8e5_t, MODE_DGRAD, 16>(f, a, s); }
void dvg_dgrad_ks(int bn, ConvArgs& a, hipStream_t s) { launch_ks<MODE_DGRAD>(bn, a, s); }
void dvg_dgrad_ks_pair(int bn, ConvArgs& a0, ConvArgs& a1, hipStream_t s) { launch_ks_pair<MODE_DGRAD>(bn, a0, a1, s); }
