"""CPU: every conv of a plan runs each of its directions exactly once, on the entry its fusion markers name, with a descriptor
the library itself accepts for that entry (engine.ConvOp: d_in / d_w / dgrad_desc(), fwd_launches / wgrad_launches / dgrad_launches).

The sibling of test_bn_launches_host.py.  The plans are built on the CPU (a plan only allocates and binds; nothing is launched)
at the smallest shapes at which BatchNorm on load and fp8 are taken, and each conv is asked for its launches once more.  Which
flags and pointers a launch carries is pinned by `tools/plan_dump.py --args`, not here."""
import ctypes as C

import pytest
import torch

from dualvar_amd import _lib as L, engine
from dualvar_amd.backbone.select_backbone import select_backbone

CASES = {'s3dg': ('s3dg', 'fp32', 8, 'train_grad', {}),
         'r21d': ('r21d', 'fp32', 8, 'train_grad', {}),
         'r50_fp8pw': ('r50', 'fp8pw', 4, 'train_grad', {}),
         's3dg_reduce': ('s3dg', 'fp32', 8, 'train_grad', dict(FUSE_BN_REDUCE=True)),
         's3dg_reduce_tap': ('s3dg', 'fp32', 8, 'train_grad', dict(FUSE_BN_REDUCE_TAP=True)),
         's3dg_eval': ('s3dg', 'fp32', 8, 'eval_map', {})}
# the kinds a case has to show (so that no case passes by leaving every conv out)
EXPECT = {'s3dg': ('plain', 'bn_in', 'bn_apply'), 'r21d': ('plain', 'bn_in', 'bn_apply'), 'r50_fp8pw': ('plain', 'fp8'),
          's3dg_reduce': ('plain', 'bn_in', 'reduce'), 's3dg_reduce_tap': ('plain', 'bn_in', 'reduce_tap'), 's3dg_eval': ('plain',)}


def _plan(case, monkeypatch):
    net, dtype, clips, mode, switches = CASES[case]
    for k, v in switches.items():
        monkeypatch.setattr(engine, k, v)
    torch.manual_seed(0)
    m = select_backbone(net)[0]
    m.set_compute_dtype(dtype)
    m.train(mode == 'train_grad')
    m.store.materialize(torch.device('cpu'), m.dtype)
    plan = m._acquire_plan(torch.empty(clips, 3, 8, 112, 112), False, mode == 'eval_map', mode == 'train_grad')
    m._plans.clear()
    return plan


def _conv_launches(op, monkeypatch):
    """op.launches() once more, with every Launch constructed on the way counted: all of them must be returned"""
    made = []

    class Counted(engine.Launch):
        __slots__ = ()

        def __init__(self, *a, **k):
            made.append(self)
            super().__init__(*a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(engine, 'Launch', Counted)
        f, b = op.launches()
    assert len(made) == len(f + b) and {id(l) for l in made} == {id(l) for l in f + b}, (len(made), len(f + b))
    return f, b


def _desc(l):
    return l.args[0]._obj            # (C.byref(descriptor) -> the descriptor)


@pytest.mark.parametrize('case', list(CASES))
def test_every_direction_of_every_conv_runs_once_on_its_entry(case, monkeypatch):
    plan = _plan(case, monkeypatch)
    lib, grad = plan.lib, plan.with_grad
    seen = dict.fromkeys(('plain', 'bn_in', 'bn_apply', 'reduce', 'reduce_tap', 'fp8'), 0)
    for op in plan.ops:
        if not isinstance(op, engine.ConvOp):
            continue
        f, b = _conv_launches(op, monkeypatch)
        fwd = [l for l in f if l.name == 'conv_fwd']
        wg = [l for l in b if l.name == 'conv_wgrad']
        dg = [l for l in b if l.name == 'conv_dgrad']
        quant = [l for l in f + b if l.name == 'quantize_fp8']
        pad = [l for l in b if l.name == 'stem_pad_taps']
        assert len(fwd) == 1 and len(wg) == int(grad) and len(dg) == int(bool(op.need_dx)), (case, len(fwd), len(wg), len(dg))
        assert len(f + b) == len(fwd + wg + dg + quant + pad)
        assert len(pad) == int(grad and op.zero_pad_taps is not None) and (not pad or b.index(pad[0]) == b.index(wg[0]) + 1)
        # forward
        on_load = op.bn_in is not None
        assert not (op.fp8 and on_load)
        assert fwd[0].fn is (lib.dv_conv3d_fwd_fp8 if op.fp8 else lib.dv_conv3d_fwd_bn_in if on_load else lib.dv_conv3d_fwd)
        assert _desc(fwd[0]) is op.d_in
        assert len([l for l in f if l.name == 'quantize_fp8']) == int(op.fp8)
        assert len(quant) == (int(op.fp8) + int(bool(op.fp8 and op.need_dx)))
        if op.fp8:
            assert f.index(fwd[0]) == 1 and (not dg or b.index(dg[0]) == len(b) - 1 and b[-2].name == 'quantize_fp8')
        if on_load:
            assert op.bn_in.fused_conv is op and op.bn_in.y.buf is op.x.buf and op.bn_in.y.off == op.x.off
            assert fwd[0].args[1] == op.bn_in.x.ptr
            assert int(lib.dv_conv3d_bn_in_ok(C.byref(_desc(fwd[0])))) > 0
        # weight gradient
        if grad:
            apply = op.bn_apply is not None
            assert not (apply and on_load)
            assert wg[0].fn is (lib.dv_conv3d_wgrad_bn if apply else lib.dv_conv3d_wgrad_bn_in if on_load else lib.dv_conv3d_wgrad)
            assert _desc(wg[0]) is op.d_w
            if on_load:
                assert wg[0].args[1] == op.bn_in.x.ptr
                # dv_conv3d_bn_in_ok is ONE query for both consumers of x: the weight gradient's form AND the forward's route,
                # which goes by the forward's flags (DV_W3).  The weight gradient carries no flags, so its descriptor is asked
                # with the forward's put on -- and must then be the forward's descriptor, field for field.
                dw = L.ConvDesc.from_buffer_copy(_desc(wg[0]))
                assert dw.flags == 0
                dw.flags = _desc(fwd[0]).flags
                assert bytes(dw) == bytes(_desc(fwd[0])) and int(lib.dv_conv3d_bn_in_ok(C.byref(dw))) > 0
            if apply:
                assert op.bn_apply.apply_fused and op.bn_apply.conv is op and not op.need_dx
                assert int(lib.dv_conv3d_wgrad_bn_ok(C.byref(_desc(wg[0])))) > 0
        else:
            assert op.bn_apply is None
        # data gradient
        if dg:
            reduce = op.bn_fuse is not None
            assert not (op.fp8 and reduce) and (reduce or not op.bn_fuse_tap)
            assert dg[0].fn is (lib.dv_conv3d_dgrad_fp8 if op.fp8 else lib.dv_conv3d_dgrad_bn_ws if op.bn_fuse_tap
                                else lib.dv_conv3d_dgrad_bn if reduce else lib.dv_conv3d_dgrad)
            assert _desc(dg[0]) is op.dgrad_desc()
            assert bool(_desc(dg[0]).flags & L.DV_ACCUM) == bool(op.acc['x'])
            if reduce:
                assert op.bn_fuse.reduce_fused and op.bn_fuse.y.buf is op.x.buf and op.bn_fuse.y.off == op.x.off
            if op.bn_fuse_tap:
                nb = int(lib.dv_conv3d_dgrad_bn_workspace(C.byref(_desc(dg[0]))))
                assert 0 < nb <= plan.bn_fuse_ws.numel() * 4 == dg[0].args[-1]
        else:
            assert op.bn_fuse is None and not op.bn_fuse_tap
        for k, on in (('bn_in', on_load), ('bn_apply', op.bn_apply is not None), ('fp8', op.fp8), ('reduce_tap', op.bn_fuse_tap),
                      ('reduce', op.bn_fuse is not None and not op.bn_fuse_tap)):
            seen[k] += bool(on)
        seen['plain'] += not (on_load or op.bn_apply is not None or op.fp8 or op.bn_fuse is not None)
    assert all(seen[k] for k in EXPECT[case]), (case, seen)
    # the markers point back from every member, too: a member marked as fused names a conv that carries it
    for g in plan.ops:
        for m in g.members if isinstance(g, engine.BNGroupOp) else ():
            assert m.fused_conv is None or m.fused_conv.bn_in is m
            assert not m.apply_fused or m.conv.bn_apply is m
            assert not m.reduce_fused or sum(1 for o in plan.ops if isinstance(o, engine.ConvOp) and o.bn_fuse is m) == 1
