"""CPU: the backward's two-stream schedule against what each launch touches (tests/plan_hazards.py).

Plans of all seven backbones, fp32 and bf16, train mode with gradients, built on the CPU as tests/test_plan_graph_host.py builds
them (a plan only allocates and binds).  For each: the declared reads / writes of every launch cover every pointer the launch
carries; one call of the real Plan.run_backward, recorded with fake streams and events, orders every pair of launches that
conflict, the way the list orders them -- for WGRAD_BATCH 1 / 4 / 10**6, early release forced off and on, grad_ready unarmed, armed
at the default 8 MB buckets and at buckets small enough to give five; the pass is closed; Launch.gend is what is written; the
grad_ready promise holds; the one-stream switch gives the list.  The launch lists themselves are those of
tests/golden/plan_launch_digests.json (regenerate: python -m tests.test_plan_streams_host, when a change to the lists is meant).

Then the checker against planted faults, on stub launch lists over small CPU tensors and one doctored trace of a real plan: a
checker that passes because it finds nothing would pass everything above.

The SyncBN exchange of a world-2 plan is a third stream: test_world2_backward_orders_every_conflict."""
import json
import os
import sys

import pytest
import torch

from dualvar_amd import engine
from dualvar_amd.parallel import bucket_ranges
from tests import plan_hazards as H
from tests.test_plan_graph_host import NETS, _plan

DTYPES = ('fp32', 'bf16')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plan_launch_digests.json')
_cache = {}


def built(net, dtype):
    """(plan, registry, normalised access sets) of a net's training plan, built once per module"""
    key = (net, dtype)
    if key not in _cache:
        _cache.clear()                 # (one plan's CPU buffers at a time)
        plan = _plan(net, dtype, True, False, True)
        reg = H.Registry(plan)
        _cache[key] = (plan, reg, H.Sets(reg))
    return _cache[key]


def small_buckets(plan):
    """bucket starts for the largest bucket that still gives at least five"""
    return tuple(a for a, _ in bucket_ranges(plan.store.total, max(8, plan.store.total // 5)))


nets = pytest.mark.parametrize('net', NETS)
dtypes = pytest.mark.parametrize('dtype', DTYPES)


@dtypes
@nets
def test_declared_accesses_cover_every_pointer(net, dtype):
    plan, reg, sets = built(net, dtype)
    n = sum(len(v) for l in H.launches(plan) for v in H.scan(reg, l).values())
    assert n > 10 * len(H.launches(plan)) / 3, 'the pointer scan found next to nothing: %d' % n
    for l in H.launches(plan):
        assert l.name in ('zero_bwd_sums', 'ingest') or l.reads, H.label(l)       # (no clips are bound to a plan built here)
        assert l.writes, H.label(l)
    bad = H.check_complete(plan, reg)
    assert not bad, '\n'.join(bad[:20])


@dtypes
@nets
def test_eval_plans_declare_every_pointer(net, dtype):
    """the forward-only lists of .eval() (running statistics, conv bias folded into the shift, the gate unfused and in place)"""
    plan = _plan(net, dtype, False, True, False)
    assert plan.f_list and not plan.b_list and all(l.writes for l in plan.f_list)
    bad = H.check_complete(plan, H.Registry(plan))
    assert not bad, '\n'.join(bad[:20])


def test_fp8_pointwise_plan():
    """mode 'fp8pw' of the bottleneck net: the quantise launches in front of the fp8 convs share one workspace, on the main stream"""
    plan = _plan('r50', 'fp8pw', True, False, True)
    n_q = sum(1 for l in H.launches(plan) if l.name == 'quantize_fp8')
    assert n_q > 20
    reg = H.Registry(plan)
    sets = H.Sets(reg)
    bad = H.check_complete(plan, reg) + H.check_gend(plan, reg, sets)
    rec = H.record(plan)
    order = H.Order(rec.trace)
    assert any(n.launch.name == 'quantize_fp8' for n in order.nodes)
    bad += [t for _, _, t in H.check_conflicts(order, sets, plan.b_list)] + H.check_closed(rec, order)
    assert not bad, '\n'.join(bad[:20])


@dtypes
@nets
def test_gend_is_what_is_written(net, dtype):
    plan, reg, sets = built(net, dtype)
    assert sum(1 for l in plan.b_list if getattr(l, 'gend', 0)) >= sum(1 for l in plan.b_list if l.name == 'conv_wgrad') > 0
    bad = H.check_gend(plan, reg, sets)
    assert not bad, '\n'.join(bad[:20])


@dtypes
@nets
def test_backward_orders_every_conflict(net, dtype, monkeypatch):
    plan, reg, sets = built(net, dtype)
    n_side = sum(1 for i, l in enumerate(plan.b_list) if l.name in engine.SIDE_LAUNCHES
                 or (l.name == 'stem_pad_taps' and plan.b_list[i - 1].name in engine.SIDE_LAUNCHES))
    default = tuple(a for a, _ in bucket_ranges(plan.store.total, int(8 * (1 << 20) // 4)))
    small = small_buckets(plan)
    assert len(small) >= 5
    early0 = plan.wgrad_early
    try:
        for batch in (1, 4, 10 ** 6):
            monkeypatch.setattr(engine, 'WGRAD_BATCH', batch)
            for early in (False, True):
                plan.wgrad_early = early
                for armed, starts in ((False, ()), (True, default), (True, small)):
                    what = '%s %s WGRAD_BATCH=%d early=%s buckets=%d' % (net, dtype, batch, early, len(starts))
                    rec = H.record(plan, armed, starts)
                    order = H.Order(rec.trace)
                    on_side = [n for n in order.nodes if n.stream.name == 'side']
                    assert len(order.nodes) == len(plan.b_list) and len(on_side) == n_side > 0, what
                    assert {s.name for s in rec.streams.values()} == {'main', 'side'}, what
                    bad = [t for _, _, t in H.check_conflicts(order, sets, plan.b_list)]
                    assert not bad, what + '\n' + '\n'.join(bad[:20])
                    bad = H.check_closed(rec, order)
                    assert not bad, what + '\n' + '\n'.join(bad[:20])
                    if armed:
                        # (every bucket start is announced once the arena is final from there; the last call is ready(0))
                        assert order.ready and order.ready[-1].lo == 0 and len(order.ready) <= len(starts), what
                        assert [r.lo for r in order.ready] == sorted((r.lo for r in order.ready), reverse=True), what
                    else:
                        assert not order.ready
                    bad = H.check_ready(plan, reg, order, sets)
                    assert not bad, what + '\n' + '\n'.join(bad[:20])
    finally:
        plan.wgrad_early = early0


@dtypes
@nets
def test_one_stream_switch_gives_the_list(net, dtype):
    plan, reg, sets = built(net, dtype)
    rec = H.one_stream_trace(plan)
    assert [k for k, *_ in rec.trace] == ['launch'] * len(plan.b_list)
    assert all(s is rec.main and l is want for (_, s, l), want in zip(rec.trace, plan.b_list))
    assert list(rec.streams.values()) == [rec.main]


def _digests():
    return {'%s/%s' % (net, dtype): H.launch_digest(*built(net, dtype)[:2]) for net in NETS for dtype in DTYPES}


def test_launch_lists_are_the_recorded_ones():
    """name, kernel, every argument (pointers as buffer + offset) and gend of every launch of every plan, position by position,
    against the digests recorded from the lists as they were before launches carried reads / writes: the metadata changed no
    launch, argument or order -- pairing included, which reads the sets"""
    want = json.load(open(GOLDEN))
    got = _digests()
    assert set(got) == set(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff


def test_paired_launches_carry_their_members_sets():
    plan, reg, sets = built('s3dg', 'fp32')
    pairs = [l for l in H.launches(plan) if getattr(l, 'members', ())]
    assert len(pairs) >= 20
    for p in pairs:
        a, b = p.members
        assert p.reads == a.reads + b.reads and p.writes == a.writes + b.writes
        assert a.pair.reads is a.reads and a.pair.writes is a.writes              # one copy: the launch's


# ------------------------------------------------------------------------------------------------------------ planted faults
def _stub_plan(lst, total=64):
    """a Plan that holds nothing but a backward list, over small CPU tensors; run_backward is the real one"""
    p = engine.Plan.__new__(engine.Plan)
    p.store = engine.ParamStore()
    p.store.grad, p.store.total = torch.zeros(total), total
    p.device, p.b_list, p.f_list, p.timer, p.grad_ready = torch.device('cpu'), lst, [], None, None
    p._side = p._events = p._triggers = None
    p.wgrad_early, p.bucket_starts = False, ()
    p.bufs = {}
    return p


def _l(name, tag, reads=(), writes=(), gend=0, args=()):
    l = engine.Launch(name, tag, None, args, reads=reads, writes=writes)
    l.gend = gend
    return l


def _check(plan, monkeypatch, batch, armed=False, starts=()):
    monkeypatch.setattr(engine, 'WGRAD_BATCH', batch)
    reg = H.Registry(plan)
    sets = H.Sets(reg)
    rec = H.record(plan, armed, starts)
    order = H.Order(rec.trace)
    return reg, sets, rec, order


def test_planted_main_launch_overtakes_a_pending_side_launch(monkeypatch):
    """[reduce, wgrad (reads dy), apply (writes dy in place)]: with the weight gradient still pending when `apply` is issued, the
    main stream overwrites its input first.  Both ARE ordered -- the wrong way round."""
    dy, x = torch.zeros(32), torch.zeros(32)
    plan = _stub_plan([])
    lst = [_l('bn_bwd_reduce', 'produces', reads=[H_all(x)], writes=[H_all(dy)]),
           _l('conv_wgrad', 'pending', reads=[H_all(dy), H_all(x)], writes=[(plan.store.grad, 0, 16)], gend=16),
           _l('gate_bwd_apply', 'in place', reads=[H_all(dy)], writes=[H_all(dy)])]
    plan.b_list, plan.bufs = lst, dict(dy=dy, x=x)
    reg, sets, rec, order = _check(plan, monkeypatch, 4)
    assert [(k, str(s)) for k, s, *_ in rec.trace if k == 'launch'] == [('launch', 'main'), ('launch', 'main'), ('launch', 'side')]
    bad = H.check_conflicts(order, sets, lst)
    assert len(bad) == 1 and bad[0][0].launch is lst[1] and bad[0][1].launch is lst[2], bad
    assert 'conv_wgrad[pending' in bad[0][2] and 'gate_bwd_apply[in place' in bad[0][2] and 'runs BEFORE it' in bad[0][2]
    assert not H.check_closed(rec, order) and not H.check_gend(plan, reg, sets)
    # the same list without the in-place write is clean
    lst[2].writes = ()
    assert not H.check_conflicts(H.Order(rec.trace), H.Sets(reg), lst)


def H_all(t):
    return (t, 0, t.numel())


def test_planted_input_written_after_the_event(monkeypatch):
    """the weight gradient leaves at once (WGRAD_BATCH 1): the event is recorded at its list position, and the main-stream launch
    behind it, which writes the weight gradient's input, runs beside it"""
    dy, x = torch.zeros(32), torch.zeros(32)
    plan = _stub_plan([])
    lst = [_l('bn_bwd_reduce', 'produces', reads=[H_all(x)], writes=[H_all(dy)]),
           _l('conv_wgrad', 'released', reads=[H_all(dy), H_all(x)], writes=[(plan.store.grad, 0, 16)], gend=16),
           _l('gate_bwd_apply', 'in place', reads=[H_all(dy)], writes=[H_all(dy)]),
           _l('maxpool_bwd', 'innocent', reads=[H_all(dy)], writes=[H_all(x)])]
    plan.b_list, plan.bufs = lst, dict(dy=dy, x=x)
    reg, sets, rec, order = _check(plan, monkeypatch, 1)
    assert [k for k, *_ in rec.trace][:4] == ['launch', 'record', 'wait_event', 'launch']
    bad = H.check_conflicts(order, sets, lst)
    # the in-place write of dy, and the later write of x: both race with the released weight gradient's reads
    assert [(a.launch, b.launch) for a, b, _ in bad] == [(lst[1], lst[2]), (lst[1], lst[3])], bad
    assert all('is not ordered with it' in t and 'conv_wgrad[released' in t for _, _, t in bad)
    assert 'gate_bwd_apply[in place' in bad[0][2] and 'maxpool_bwd[innocent' in bad[1][2]
    # what the weight gradient waits for is ordered: the reduce that produced dy
    assert order.before(order.nodes[0], [n for n in order.nodes if n.launch is lst[1]][0].vc)


def test_planted_gend_below_the_write(monkeypatch):
    """a launch that writes the arena up to 48 and says 16: check_gend names it, and the promise made from it breaks -- ready(32)
    is announced while the launch is still to come"""
    dy = torch.zeros(32)
    plan = _stub_plan([])
    g = plan.store.grad
    lst = [_l('conv_wgrad', 'top', reads=[H_all(dy)], writes=[(g, 48, 64)], gend=64),
           _l('bn_bwd_apply', 'main', reads=[H_all(dy)], writes=[H_all(dy)]),
           _l('conv_wgrad', 'understated', reads=[H_all(dy)], writes=[(g, 16, 48)], gend=16),
           _l('conv_wgrad', 'bottom', reads=[H_all(dy)], writes=[(g, 0, 16)], gend=16)]
    lst[1].reads = ()
    plan.b_list, plan.bufs = lst, dict(dy=dy)
    reg, sets, rec, order = _check(plan, monkeypatch, 1, True, (32, 0))
    bad = H.check_gend(plan, reg, sets)
    assert len(bad) == 1 and 'conv_wgrad[understated' in bad[0] and 'gend 16' in bad[0] and 'up to 48' in bad[0]
    assert [r.lo for r in order.ready] == [32, 0]
    bad = H.check_ready(plan, reg, order, sets)
    assert len(bad) == 1 and 'conv_wgrad[understated' in bad[0] and 'after ready(32)' in bad[0], bad
    lst[2].gend = 48
    reg, sets, rec, order = _check(plan, monkeypatch, 1, True, (32, 0))
    assert not H.check_gend(plan, reg, sets) and not H.check_ready(plan, reg, order, sets)


def test_planted_ready_before_a_side_launch_is_ordered(monkeypatch):
    """a ready(lo) node that does not join the side stream: the promise check names the side launches it cannot see"""
    dy = torch.zeros(32)
    plan = _stub_plan([])
    g = plan.store.grad
    lst = [_l('conv_wgrad', 'w', reads=[H_all(dy)], writes=[(g, 0, 64)], gend=64)]
    plan.b_list, plan.bufs = lst, dict(dy=dy)
    reg, sets, rec, order = _check(plan, monkeypatch, 4, True, (0,))
    assert not H.check_ready(plan, reg, order, sets)
    order.ready[0].vc = dict(order.end[rec.main])
    order.ready[0].vc.pop([s for s in rec.streams.values() if s.name == 'side'][0], None)
    bad = H.check_ready(plan, reg, order, sets)
    assert len(bad) == 1 and 'conv_wgrad[w' in bad[0] and 'not ordered before ready(0)' in bad[0]


def test_planted_undeclared_pointer():
    a, b, tab = torch.zeros(16), torch.zeros(16), torch.zeros(16)
    plan = _stub_plan([])
    l = _l('bn_apply', 'forgets b', reads=[H_all(a)], writes=[(a, 0, 8)], args=(a.data_ptr(), 16, b.data_ptr() + 8, 3.0))
    outside = _l('bn_apply', 'past its range', reads=[(a, 0, 8)], args=(a.data_ptr() + 4 * 12,))
    stranger = _l('bn_apply', 'not of the plan', reads=[H_all(torch.zeros(4))])
    plan.f_list, plan.bufs = [l, outside, stranger], dict(a=a, b=b, tab=tab)
    assert a.data_ptr() >= H.POINTER_MIN
    bad = H.check_complete(plan, H.Registry(plan))
    assert len(bad) == 3, bad
    assert 'bn_apply[forgets b' in bad[0] and 'bufs.b' in bad[0] and 'neither a read nor a write' in bad[0]
    assert 'bn_apply[past its range' in bad[1] and 'outside every range' in bad[1]
    assert 'bn_apply[not of the plan' in bad[2] and 'outside the plan' in bad[2]
    l.reads += (H_all(b),)
    assert H.check_complete(plan, H.Registry(plan), [l]) == []


def test_planted_pointer_behind_a_device_table():
    """a pointer the launch carries only inside a table on the device is found through the table"""
    import ctypes as C
    from dualvar_amd import _lib as L
    x, hidden = torch.zeros(16), torch.zeros(16)
    arr = (L.BnItem * 2)()
    arr[0].x, arr[1].dx = x.data_ptr(), hidden.data_ptr()
    plan = _stub_plan([])
    plan._items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    l = _l('bn_apply_multi', 'table', reads=[H_all(plan._items), H_all(x)], args=(0, plan._items.data_ptr(), 2))
    plan.f_list, plan.bufs = [l], dict(x=x, hidden=hidden)
    bad = H.check_complete(plan, H.Registry(plan))
    assert len(bad) == 1 and 'bufs.hidden' in bad[0] and 'bn_apply_multi[table' in bad[0], bad
    assert C.sizeof(L.BnItem) * 2 == plan._items.numel()


def test_without_the_event_waits_every_side_launch_is_flagged(monkeypatch):
    """S3D-G fp32, WGRAD_BATCH 1: the trace with its wait_event steps deleted leaves nothing between the main stream's writers
    and the side stream -- every side launch must come out flagged, by name: each conv_wgrad and gate_db through the gradient or
    table it reads, the stem's pad-tap fill through the weight gradient it follows on its own stream"""
    plan, reg, sets = built('s3dg', 'fp32')
    monkeypatch.setattr(engine, 'WGRAD_BATCH', 1)
    rec = H.record(plan)
    n_side = sum(1 for k, s, *_ in rec.trace if k == 'launch' and s.name == 'side')
    assert sum(1 for k, *_ in rec.trace if k == 'wait_event') == n_side > 0          # (each has an event of its own)
    order = H.Order(rec.trace, drop=('wait_event',))
    side = [n.launch for n in order.nodes if n.stream.name == 'side']
    bad = H.check_conflicts(order, sets, plan.b_list)
    hit = H.flagged(order, sets, bad)
    direct = {id(n.launch) for a, b, _ in bad for n in (a, b)}
    assert sum(1 for l in side if id(l) in hit) == len(side) == n_side
    assert [l.name for l in side if id(l) not in direct] == ['stem_pad_taps']
    text = '\n'.join(t for _, _, t in bad)
    assert all(H.label(l) in text for l in side if id(l) in direct)
    assert not H.check_conflicts(H.Order(rec.trace), sets, plan.b_list)          # (with the waits, the same trace is clean)


def _world2_comm():
    """engine.Comm as a process of a two-rank job holds it over a backend without flat gathers, made by hand: no process group
    exists here, torch.distributed is not touched, and the exchange steps of the plan are recorded, never called"""
    c = engine.Comm.__new__(engine.Comm)
    c.group, c.world, c.rank, c.exchange, c.flat_gather, c.rccl, c._xstream = None, 2, 0, True, False, None, None
    return c


@dtypes
@nets
def test_world2_backward_orders_every_conflict(net, dtype, monkeypatch):
    """The SyncBN exchange as a third stream: a world-2 plan has syncbn_allreduce_start / _wait steps around every group's
    in-place all-reduce of its zero-arena range, and overlap_bn_exchange has moved the weight gradients issued since the previous
    exchange between them.  The all-reduce counts as a read and write of that range on the exchange stream (Recorder.timer).  The
    event hops around a direct RCCL call (DUALVAR_BN_BWD_ASYNC=1) need the RCCL communicator and are not traced here."""
    from tests.test_plan_graph_host import _models
    _cache.clear()
    _plan(net, dtype, True, False, True)                     # (makes the model)
    m = _models[net]
    m.comm = _world2_comm()
    try:
        plan = _plan(net, dtype, True, False, True)
    finally:
        m.comm = None
    assert plan.comm.world == 2
    reg = H.Registry(plan)
    sets = H.Sets(reg)
    assert not H.check_complete(plan, reg) and not H.check_gend(plan, reg, sets)
    starts = [i for i, l in enumerate(plan.b_list) if l.name == 'syncbn_allreduce_start']
    assert len(starts) == sum(1 for op in plan.ops if isinstance(op, engine.BNGroupOp)) > 0
    moved = sum(1 for i in starts if plan.b_list[i + 1].name == 'conv_wgrad')
    assert moved > 0, 'no weight gradient stands between a start and its wait: the reorder did nothing'
    for batch in (1, 4, 10 ** 6):
        monkeypatch.setattr(engine, 'WGRAD_BATCH', batch)
        for armed, bs in ((False, ()), (True, small_buckets(plan))):
            rec = H.record(plan, armed, bs)
            order = H.Order(rec.trace)
            assert {s.name for s in rec.streams.values()} == {'main', 'side', 'exchange'}
            assert sum(1 for n in order.nodes if n.stream.name == 'exchange') == len(starts)
            bad = [t for _, _, t in H.check_conflicts(order, sets, plan.b_list)] + H.check_closed(rec, order) + \
                H.check_ready(plan, reg, order, sets)
            assert not bad, 'WGRAD_BATCH=%d armed=%s\n' % (batch, armed) + '\n'.join(bad[:20])
    # the checker sees the third stream: without the hop back (the wait step's event), every apply that reads the reduced sums
    # races with its all-reduce
    monkeypatch.setattr(engine, 'WGRAD_BATCH', 4)
    rec = H.record(plan)
    trace = [st for st in rec.trace if not (st[0] == 'wait_event' and st[1] is rec.main)]
    assert len(rec.trace) - len(trace) == len(starts)
    bad = H.check_conflicts(H.Order(trace), sets, plan.b_list)
    assert len({id(a.launch) for a, _, _ in bad if a.stream.name == 'exchange'}) == len(starts)


if __name__ == '__main__':
    json.dump(_digests(), open(GOLDEN, 'w'), indent=1, sort_keys=True)
    print('wrote', GOLDEN, file=sys.stderr)
