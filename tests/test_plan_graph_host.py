"""CPU: the reader / gradient-writer index behind the fusions of Plan.finalize (engine.PlanGraph, Op.inputs()).

First on stub ops over small CPU activations, then on the real plans of all seven backbones, built on the CPU (a plan only
allocates and binds; nothing is launched): wherever a BatchNorm's forward apply is skipped, nobody but the op that took it over
reads its output, and every gradient has exactly one non-accumulating writer, the last one in forward order."""
from types import SimpleNamespace

import pytest
import torch

import dualvar_amd.backbone.base as base
from dualvar_amd import engine, ops
from dualvar_amd.backbone.select_backbone import select_backbone
from dualvar_amd.ops import DV_F32


def _act(C_=16, grad=True):
    a = ops.new_act(1, 1, 2, 2, C_, DV_F32, 'cpu')
    if grad:
        a.grad = ops.new_act(1, 1, 2, 2, C_, DV_F32, 'cpu', zero=True)
    return a


def _slice(a, off, C_):
    s = a.slice(off, C_)
    s.grad = a.grad.slice(off, C_)
    return s


class Reads(engine.Op):
    """stub: reads `acts`, writes the gradient of each of them (named x0, x1, ...)"""

    def __init__(self, *acts):
        super().__init__(None)
        self.acts = acts

    def inputs(self):
        return list(self.acts)

    def grad_targets(self):
        return [('x%d' % i, a) for i, a in enumerate(self.acts)]


class StubMember:
    def __init__(self, x, res):
        self.x, self.res = x, res


def test_sole_reader():
    a, b = _act(), _act()
    one, two, three = Reads(a), Reads(b), Reads(b)
    g = engine.PlanGraph([one, two, three])
    assert g.sole_reader(a) is one and g.readers(a) == [one]
    assert g.sole_reader(b) is None and g.readers(b) == [two, three]          # forward order
    assert g.sole_reader(_act()) is None and g.readers(_act()) == []


def test_a_read_of_another_slice_of_the_buffer_counts():
    a = _act(32)
    lo, hi = _slice(a, 0, 16), _slice(a, 16, 16)
    r_lo, r_hi = Reads(lo), Reads(hi)
    g = engine.PlanGraph([r_lo, r_hi])
    assert g.sole_reader(lo) is None and g.sole_reader(hi) is None and g.readers(a) == [r_lo, r_hi]
    assert engine.PlanGraph([r_lo]).sole_reader(hi) is r_lo


def test_a_batchnorm_residual_counts():
    x, res = _act(), _act()
    bn = engine.BNGroupOp.__new__(engine.BNGroupOp)          # (inputs() and grad_targets() read these three attributes only)
    bn.plan, bn.acc, bn.members = SimpleNamespace(with_grad=True), {}, [StubMember(x, res), StubMember(_act(), None)]
    conv = Reads(res)
    assert [t is u for t, u in zip(bn.inputs(), (x, res, bn.members[1].x))] == [True] * 3
    g = engine.PlanGraph([conv, bn])
    g.set_accumulate_flags()
    assert conv.acc == {'x0': True} and bn.acc == {'res0': False}
    assert g.sole_reader(res) is None and g.readers(res) == [conv, bn]
    assert g.sole_reader(x) is bn


def test_a_host_read_buffer_has_no_sole_reader():
    a = _act(32)
    r = Reads(a)
    assert engine.PlanGraph([r]).sole_reader(a) is r
    assert engine.PlanGraph([r], [a]).sole_reader(a) is None
    assert engine.PlanGraph([r], [_slice(a, 16, 16)]).sole_reader(a) is None      # any slice of it
    assert engine.PlanGraph([r], [a]).readers(a) == [r]


def test_an_op_without_inputs_raises_and_names_its_class():
    class Forgetful(engine.Op):
        pass
    with pytest.raises(NotImplementedError, match='Forgetful'):
        engine.PlanGraph([Forgetful(None)])


def test_accumulate_flags():
    a = _act(32)
    lo, hi = _slice(a, 0, 16), _slice(a, 16, 16)
    first, second, third = Reads(a), Reads(a, hi), Reads(lo)
    g = engine.PlanGraph([first, second, third])
    g.set_accumulate_flags()
    # a and lo start at offset 0 of the same gradient buffer: one key, three writers; hi is a key of its own
    assert first.acc == {'x0': True} and second.acc == {'x0': True, 'x1': False} and third.acc == {'x0': False}
    assert [(op, n) for op, n, _ in g.grad_writers(lo)] == [(first, 'x0'), (second, 'x0'), (third, 'x0')]
    assert [(op, n) for op, n, _ in g.grad_writers(hi)] == [(second, 'x1')]
    early, late = Reads(a), Reads(a)
    engine.PlanGraph([early, late]).set_accumulate_flags()
    assert early.acc == {'x0': True} and late.acc == {'x0': False}


def test_every_op_class_says_what_it_reads():
    def walk(cls):
        for sub in cls.__subclasses__():
            yield sub
            yield from walk(sub)
    subs = [c for c in walk(engine.Op) if c.__module__.startswith('dualvar_amd')]
    assert base.IngestOp in subs and len(subs) >= 6
    for c in subs:
        assert c.inputs is not engine.Op.inputs, c.__name__


NETS = ('s3dg', 's3d', 'r21d', 'r3d', 'r50', 'r2d3d18', 'c3d')
_models = {}


def _plan(net, dtype, training, want_map, with_grad):
    if net not in _models:
        torch.manual_seed(0)
        _models[net] = select_backbone(net)[0]
    m = _models[net]
    m.set_compute_dtype(dtype)
    m.train(training)
    if not m.store.ready(torch.device('cpu'), m.dtype):
        m.store.materialize(torch.device('cpu'), m.dtype)
    plan = m._acquire_plan(torch.empty(4 if net == 'r50' else 8, 3, 8, 112, 112), False, want_map, with_grad)
    m._plans.clear()
    return plan


@pytest.mark.parametrize('mode', ['train', 'eval_map'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('net', NETS)
def test_real_plans(net, dtype, mode):
    plan = _plan(net, dtype, mode == 'train', mode == 'eval_map', mode == 'train')
    assert plan.host_reads and plan.host_reads[0] is plan.out_act
    pos = {id(op): i for i, op in enumerate(plan.ops)}

    def readers(buf):
        return [op for op in plan.ops if any(a.buf is buf for a in op.inputs())]
    skipped = 0
    for op in plan.ops:
        for m in getattr(op, 'members', ()):
            if m.fused_pool is not None or m.fused_conv is not None:
                # the output is never written: only the op that applies the BatchNorm itself may list it
                taker = m.fused_pool if m.fused_pool is not None else m.fused_conv
                assert readers(m.y.buf) == [taker], (net, type(taker).__name__)
                assert all(h.buf is not m.y.buf for h in plan.host_reads)
                skipped += 1
            elif m.gate is not None:
                # the gate writes the gated values where the un-gated ones would have been, in place, so the levels after
                # it (and the host, for the last level) do read this buffer -- what must hold is that nobody reads it BEFORE
                # the gate has written it: the gate is its first reader in forward order
                rd = readers(m.y.buf)
                assert rd and rd[0] is m.gate[0] and all(pos[id(o)] > pos[id(m.gate[0])] for o in rd[1:]), net
                assert pos[id(op)] < pos[id(m.gate[0])]
                skipped += 1
    if net in ('s3dg', 's3d', 'r50', 'r2d3d18'):      # their stems end in conv + BatchNorm + ReLU + max-pool
        assert skipped, 'no fusion engaged: the assertions above checked nothing'
    writers = {}
    for op in plan.ops:
        for name, a in op.grad_targets():
            g = a.grad if a.grad is not None else a
            writers.setdefault((g.buf.data_ptr(), g.off), []).append((op, name))
    assert bool(writers) == (mode == 'train')
    for key, w in writers.items():
        first = [(op, name) for op, name in w if not op.acc[name]]
        assert first == [w[-1]], (net, key, [type(op).__name__ for op, _ in w])
