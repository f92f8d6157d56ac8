"""The coverage ledger of the C ABI: every entry of dualvar_amd._lib.SIGNATURES -> (the test file that holds its strongest
reference test, the kind of that reference).  tests/test_abi_and_host.py::test_every_abi_entry_names_its_strongest_test keeps
the keys equal to SIGNATURES and checks that each file mentions its entry, so a new entry has to say here how it is tested and
whatever is still 'torch fp32 only' stays visible as the next gap.

The ledger is per entry.  Above it: tests/test_plan_audit_gpu.py checks every op of a backbone plan against float64, and
tests/test_plan_streams_host.py / tests/test_plan_streams_gpu.py (support: tests/plan_hazards.py) check WHEN the launches of a
plan run relative to each other -- what each launch reads and writes, and that the backward's side stream orders every pair
that conflicts."""

FLOAT64 = 'float64'
BIT_EXACT = 'bit-exact against PIL / torch cast'
BIT_EQUAL_TESTED = 'bit-exact against float64-tested entries'      # a fused entry that promises the bits of the sequence it replaces
CPU_ORACLE = 'fp32 CPU oracle'                                     # the augmentation oracle of oracle/augment_ref.py
TORCH_FP32 = 'torch fp32 only'
HOST_QUERY = 'host query'
KINDS = (FLOAT64, BIT_EXACT, BIT_EQUAL_TESTED, CPU_ORACLE, TORCH_FP32, HOST_QUERY)

_CONV, _BNM, _BNS = 'test_conv_float64_gpu.py', 'test_batchnorm_multi_gpu.py', 'test_batchnorm_single_gpu.py'
_LOSS, _POOL, _HOST, _OPS = 'test_loss_gemm_optim_gpu.py', 'test_pool_gate_float64_gpu.py', 'test_abi_and_host.py', 'test_ops_gpu.py'
_GATE, _LARS, _AUG, _FP8 = 'test_gate_fold_gpu.py', 'test_lars_gpu.py', 'test_augment_blocks_gpu.py', 'test_fp8_float64_gpu.py'

ENTRY_COVERAGE = {
    'dv_abi_version': (_HOST, HOST_QUERY),
    'dv_check_device': (_HOST, HOST_QUERY),
    'dv_conv3d_stat_tiles': (_HOST, HOST_QUERY),
    'dv_conv3d_tile_rows': (_HOST, HOST_QUERY),
    'dv_conv3d_tile_shape': (_HOST, HOST_QUERY),
    'dv_conv3d_ksplit_cols': (_HOST, HOST_QUERY),
    'dv_conv3d_tap_kind': (_HOST, HOST_QUERY),
    'dv_conv3d_tap_rows': (_HOST, HOST_QUERY),
    'dv_conv3d_fwd': (_CONV, FLOAT64),
    'dv_conv3d_dgrad': (_CONV, FLOAT64),
    'dv_conv3d_dgrad_bn': (_CONV, FLOAT64),
    'dv_conv3d_dgrad_bn_workspace': (_CONV, HOST_QUERY),
    'dv_conv3d_dgrad_bn_ws': (_CONV, FLOAT64),
    'dv_conv3d_wgrad_workspace': (_HOST, HOST_QUERY),
    'dv_conv3d_wgrad_tile': (_HOST, HOST_QUERY),
    'dv_conv3d_wgrad': (_CONV, FLOAT64),
    'dv_conv3d_wgrad_bn_ok': (_HOST, HOST_QUERY),
    'dv_conv3d_bn_in_ok': (_HOST, HOST_QUERY),
    'dv_conv3d_fwd_bn_in': (_CONV, FLOAT64),
    'dv_conv3d_wgrad_bn_in': (_CONV, FLOAT64),
    'dv_conv3d_wgrad_bn': (_CONV, FLOAT64),
    'dv_quantize_fp8_workspace': (_HOST, HOST_QUERY),
    'dv_quantize_fp8': (_FP8, FLOAT64),
    'dv_conv3d_fwd_fp8': (_FP8, FLOAT64),
    'dv_conv3d_dgrad_fp8': (_FP8, FLOAT64),
    'dv_w3_bytes': (_CONV, HOST_QUERY),
    'dv_pack_w3': (_CONV, BIT_EXACT),
    'dv_pack_dgrad_weights': (_CONV, BIT_EXACT),
    'dv_cast_arena': (_LOSS, BIT_EXACT),
    'dv_ingest_ncdhw': (_POOL, FLOAT64),
    'dv_ingest_ncdhw_pad': (_POOL, FLOAT64),
    'dv_fill_cols_f32': (_BNS, BIT_EXACT),
    'dv_addcmul_f32': (_BNS, FLOAT64),
    'dv_bn_eval_coeffs': (_BNS, FLOAT64),
    'dv_bn_rows_partials_f32': (_BNS, FLOAT64),
    'dv_softmax_ce_fwd': (_LOSS, FLOAT64),
    'dv_knn_rank': (_LOSS, FLOAT64),
    'dv_softmax_rows_f32': (_LOSS, FLOAT64),
    'dv_augment_ingest': (_AUG, CPU_ORACLE),
    'dv_augment_ingest_blocks': (_AUG, CPU_ORACLE),
    'dv_resample_u8': ('test_frame_dataset_gpu.py', BIT_EXACT),
    'dv_bn_reduce_stats': (_BNS, FLOAT64),
    'dv_bn_finalize': (_BNS, FLOAT64),
    'dv_bn_stats_finalize': (_BNS, FLOAT64),
    'dv_bn_apply': (_BNS, FLOAT64),
    'dv_bn_stats_multi': (_BNM, FLOAT64),
    'dv_bn_apply_multi': (_BNM, FLOAT64),
    'dv_bn_finalize_multi': (_BNM, FLOAT64),
    'dv_bn_bwd_reduce_multi': (_BNM, FLOAT64),
    'dv_bn_bwd_apply_multi': (_BNM, FLOAT64),
    'dv_bn_bwd_blocks': (_HOST, HOST_QUERY),
    'dv_bn_bwd_reduce': (_BNS, FLOAT64),
    'dv_bn_bwd_reduce_workspace': (_HOST, HOST_QUERY),
    'dv_bn_bwd_apply': (_BNS, FLOAT64),
    'dv_maxpool3d_fwd': (_POOL, FLOAT64),
    'dv_maxpool3d_bwd': (_POOL, FLOAT64),
    'dv_maxpool3d_route': (_HOST, HOST_QUERY),
    'dv_bn_apply_maxpool': (_POOL, FLOAT64),
    'dv_bn_bwd_reduce_maxpool': (_POOL, FLOAT64),
    'dv_bn_bwd_apply_maxpool': (_POOL, FLOAT64),
    'dv_spatial_mean': (_POOL, FLOAT64),
    'dv_spatial_chunks': (_HOST, HOST_QUERY),
    'dv_spatial_mean_bwd': (_POOL, FLOAT64),
    'dv_gate_scale': (_POOL, FLOAT64),
    'dv_gate_bwd_reduce': (_POOL, FLOAT64),
    'dv_gate_bwd_apply': (_POOL, FLOAT64),
    'dv_gate_mean_bn': (_POOL, FLOAT64),
    'dv_gate_scale_bn': (_POOL, FLOAT64),
    'dv_bn_bwd_reduce_multi_gated': (_GATE, BIT_EQUAL_TESTED),
    'dv_bn_bwd_apply_multi_gated': (_GATE, BIT_EQUAL_TESTED),
    'dv_colsum_f32': (_LOSS, FLOAT64),
    'dv_l2norm_fwd': (_POOL, FLOAT64),
    'dv_l2norm_bwd': (_POOL, FLOAT64),
    'dv_relu_bwd_f32': (_POOL, FLOAT64),
    'dv_mean_f32': (_LOSS, FLOAT64),
    'dv_ntxent_fwd': (_LOSS, FLOAT64),
    'dv_infonce_fwd': (_LOSS, FLOAT64),
    'dv_infonce_workspace': (_LOSS, HOST_QUERY),
    'dv_rank_margin': (_LOSS, FLOAT64),
    'dv_gemm_f32': (_LOSS, FLOAT64),
    'dv_gemm_f32_grouped': (_LOSS, FLOAT64),
    'dv_gemm_f32_ex': (_LOSS, FLOAT64),
    'dv_group_mean_f32': (_LOSS, FLOAT64),
    'dv_group_mean_bwd_f32': (_LOSS, FLOAT64),
    'dv_sgd_momentum': (_LOSS, FLOAT64),
    'dv_ema': (_LOSS, FLOAT64),
    'dv_adam': ('test_adam_gpu.py', FLOAT64),
    'dv_lars_chunk': ('test_lars_host.py', HOST_QUERY),
    'dv_lars_norms': (_LARS, FLOAT64),
    'dv_lars_step': (_LARS, FLOAT64),
}
