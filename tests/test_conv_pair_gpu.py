"""GPU: two independent convs of one instantiation of the LDS-staged kernel in one grid (csrc/conv_tap.hip conv_tap_pair_kernel;
dv_conv3d_fwd_pair, dv_conv3d_fwd_bn_in_pair, dv_conv3d_dgrad_pair, dv_conv3d_pair_ok) and the plan pass that uses them
(engine.PAIR_CONVS).  A pair runs the code and the operands of its two single launches, so every comparison is torch.equal: these
are conditions, not tolerances.

The checks live in tools/pair_check.py and run in child processes: DUALVAR_CONV_TAP_GRID=1, which lets the small shapes onto
the kernel, is read once per process (as in test_lds_staged_input_tile_kernel_on_small_and_ragged_shapes)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXACT = os.environ.get('DUALVAR_F32_EXACT', '0') not in ('', '0')


def _child(mode, tap_grid='1', **env):
    if _EXACT:
        pytest.skip('the LDS-staged and K-split kernels belong to the split mode (DUALVAR_F32_EXACT=1 runs none of them)')
    env = dict(os.environ, DUALVAR_CONV_TAP_GRID=tap_grid, **env)
    for k in ('DUALVAR_PAIR_CONVS', 'DUALVAR_CONV_TAP', 'DUALVAR_FUSE_BN_IN', 'DUALVAR_CONV_KS') + (() if tap_grid else ('DUALVAR_CONV_TAP_GRID',)):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pair_check.py'), mode], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_pair_entries_give_the_bits_of_the_single_launches(gpu):
    """Op level, 128-row tiles.  Spatial 1x3x3 on 2 clips of 2 x 7 x 7 (M = 196: two row tiles, the last with 68 rows), members
    Cin16 -> Cout48 (one partial column tile) and Cin96 -> Cout208 (four, the last 16 wide) in both orders (member 0 has 2 and 8
    blocks: neither the boundary nor the sub-grids are multiples of the 8 XCDs): forward with DV_STATS, data gradient, `+=` on one
    member.  Temporal 3x1x1 at T = 2 and T = 4, C = 48 and 208: with BatchNorm on load (coefficient tables of different sizes),
    plain, data gradient, `+=` on one member.  Outputs, BatchNorm partials and the sentinel rows behind the outputs are those of
    dv_conv3d_fwd / dv_conv3d_fwd_bn_in / dv_conv3d_dgrad.  Refused pairs -- spatial with temporal, BatchNorm on load with plain,
    128- with 256-row tiles, a member that carries the fused BatchNorm-backward reduce (dv_conv3d_dgrad_bn_ws: dx and sums) --:
    dv_conv3d_pair_ok is 0 and the entry still gives the single launches' bits."""
    out = _child('ops')
    assert out.strip().endswith('ok')
    assert out.count('pair_ok 1') == 5 and out.count('pair_ok 2') == 8 and out.count('refused') == 7 and 'rows 128' in out, out[-3000:]
    for line in out.splitlines():
        assert ('pair_ok 0' in line) == line.startswith('refused'), line


@pytest.mark.gpu
def test_pair_entries_on_the_256_row_tiles(gpu):
    """The same spatial pair on the 256-row instantiation (DUALVAR_CONV_TAP_BM128=0), 3 clips: M = 294, tiles of 256 and 38 rows."""
    out = _child('ops', DUALVAR_CONV_TAP_BM128='0')
    assert out.strip().endswith('ok') and out.count('pair_ok 1') == 5 and 'rows 256' in out and 'pair_ok 0' not in out, out[-3000:]


@pytest.mark.gpu
def test_pair_entries_on_the_k_split_kernel(gpu):
    """conv_gemm_ks_kernel's two-member entry, default thresholds (the members are too small for the LDS-staged kernel): the
    spatial branch convs of Mixed_5b, Cin32 -> Cout128 and Cin160 -> Cout320, at the smallest number of 1 x 7 x 7 clips at which
    dv_conv3d_ksplit_cols puts both there (2 clips: M = 98, row tiles of 64 and 34 rows), in both orders: forward with DV_STATS,
    data gradient, `+=` on one member; dv_conv3d_pair_ok says DV_PAIR_KS (4)."""
    out = _child('ks', tap_grid='')
    assert out.strip().endswith('ok') and out.count('pair_ok 4') == 5, out[-3000:]
    for line in out.splitlines():
        assert ('pair_ok 0' in line) == line.startswith('refused'), line


@pytest.mark.gpu
def test_paired_plan_gives_the_same_bits(gpu):
    """Plan level: one S3D-G SimCLR training step (4 samples x 2 views of 8 x 112 x 112, fp32) with engine.PAIR_CONVS off and on:
    the loss and every gradient agree bit for bit, and so do two passes through the paired plan.  The paired plan holds the
    pairs of every form -- counted, so the test cannot pass without running them: spatial forwards of Mixed_3b - 5c but 4c / 4d
    (their small branch has 24 input channels: conv_gemm), temporal forwards with BatchNorm on load and temporal data gradients of
    3b - 4f (the 72-row levels run the temporal convs on conv_gemm_ks), spatial data gradients of all nine levels; and the pointwise
    branch convs of 4b - 5c, which both run conv_gemm_ks<64,32>, forward only (their data gradients write one gradient with `=` and
    `+=`)."""
    out = _child('plan')
    r = json.loads([ln for ln in out.splitlines() if ln.startswith('RESULT ')][-1][7:])
    assert r['pairs_off'] == dict(fwd_sp=0, fwd_tm_bn_in=0, dgrad_sp=0, dgrad_tm=0, fwd_ks=0, dgrad_ks=0, other=0), r
    assert r['pairs_on'] == dict(fwd_sp=7, fwd_tm_bn_in=7, dgrad_sp=9, dgrad_tm=7, fwd_ks=7, dgrad_ks=0, other=0), r
    assert r['launches_off'] - r['launches_on'] == 37, r
    assert r['finite'] and r['loss_equal'] and r['grads_equal'], r
    assert r['second_pass_equal'], r
