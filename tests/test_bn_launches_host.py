"""CPU: every BatchNorm phase of a plan is run exactly once -- by the launches its BNGroupOp returns or by the one fusion that took
it over (engine.BNGroupOp.launches, engine.BNMember).

The plans are built on the CPU (a plan only allocates and binds; nothing is launched) and each group is asked for its launches
once more.  A single-tensor launch is matched to its member by the row count, channel count and input pointer it passes, a
multi-tensor launch by the member's own share of the block prefix in the dv_bn_item table the launch receives.  Which flags and
pointers a launch carries is pinned by `tools/plan_dump.py --args`, not here."""
import pytest
import torch

from dualvar_amd import _lib as L, engine
from dualvar_amd.backbone.select_backbone import select_backbone

# phase -> (single-tensor launch names, positions of (M, C, x) in their arguments (the statistics read the conv's partial sums,
#           not x), multi-tensor launch name, position of the table in its arguments (the item count follows), blk_* field)
TRAIN = {'stats': (('bn_stats_finalize', 'bn_reduce_stats'), (4, 5, None), 'bn_stats_multi', 0, 'blk_stats'),
         'apply': (('bn_apply',), (9, 10, 1), 'bn_apply_multi', 1, 'blk_apply'),
         'red': (('bn_bwd_reduce',), (9, 10, 5), 'bn_bwd_reduce_multi', 1, 'blk_red'),
         'bapply': (('bn_bwd_apply',), (20, 21, 5), 'bn_bwd_apply_multi', 1, 'blk_bapply')}
_plans = {}


def _plan(net, mode):
    if (net, mode) not in _plans:
        torch.manual_seed(0)
        m = select_backbone(net)[0]
        m.set_compute_dtype('fp32')
        m.train(mode == 'train_grad')
        m.store.materialize(torch.device('cpu'), m.dtype)
        _plans[net, mode] = m._acquire_plan(torch.empty(2, 3, 8, 112, 112), False, mode == 'eval_map', mode == 'train_grad')
        m._plans.clear()
    return _plans[net, mode]


def _owners(m, phase):
    """the fusions recorded as running `phase` of member m"""
    return {'stats': [], 'apply': [o for o in (m.fused_conv, m.gate, m.fused_pool) if o is not None],
            'red': [True] if m.reduce_fused else [], 'bapply': [True] if m.apply_fused else []}[phase]


def _group_launches(op, monkeypatch):
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
    out = [l for l in f + b if isinstance(l, engine.Launch)]
    assert len(made) == len(out) and {id(l) for l in made} == {id(l) for l in out}, (len(made), len(out))
    return out


@pytest.mark.parametrize('net', ['s3dg', 'r21d', 'c3d'])
def test_every_phase_of_every_member_has_one_owner(net, monkeypatch):
    plan = _plan(net, 'train_grad')
    seen = dict(single=0, multi=0, fused=0)
    for op in plan.ops:
        if not isinstance(op, engine.BNGroupOp):
            continue
        ls = _group_launches(op, monkeypatch)
        for phase, (singles, (iM, iC, iP), multi, itab, blk) in TRAIN.items():
            one = [l for l in ls if l.name in singles]
            many = [l for l in ls if l.name == multi]
            assert len(many) <= 1 and not (one and many), (net, phase)
            items = (L.BnItem * many[0].args[itab + 1]).from_address(many[0].args[itab]) if many else None
            assert items is None or len(items) == len(op.members)
            for i, m in enumerate(op.members):
                mine = [l for l in one if l.args[iM] == m.M and l.args[iC] == m.C and (iP is None or l.args[iP] == m.x.ptr)]
                share = 0 if items is None else getattr(items[i], blk) - (getattr(items[i - 1], blk) if i else 0)
                assert share >= 0
                owners = _owners(m, phase)
                assert len(mine) + (share > 0) + len(owners) == 1, (net, phase, i, len(mine), share, len(owners))
                seen['single'] += len(mine)
                seen['multi'] += share > 0
                seen['fused'] += len(owners)
    assert seen['single'] and seen['fused'] and (seen['multi'] or net == 'c3d'), seen


def test_eval_plan(monkeypatch):
    plan = _plan('s3dg', 'eval_map')
    applied = pooled = 0
    for op in plan.ops:
        if not isinstance(op, engine.BNGroupOp):
            continue
        ls = _group_launches(op, monkeypatch)
        assert all(l.name in ('bn_eval_coeffs', 'bn_bias_shift', 'bn_apply') for l in ls)
        for m in op.members:
            coeffs = [l for l in ls if l.name == 'bn_eval_coeffs' and l.args[5] == m.C and l.args[6] == m.scale.data_ptr()]
            mine = [l for l in ls if l.name == 'bn_apply' and l.args[9] == m.M and l.args[10] == m.C and l.args[1] == m.x.ptr]
            assert len(coeffs) == 1 and len(mine) + len(_owners(m, 'apply')) == 1
            assert m.fused_conv is None and m.gate is None         # (training-mode fusions)
            applied += len(mine)
            pooled += m.fused_pool is not None
    assert applied and pooled
