"""CPU side of the plan audit (tests/plan_audit.py): a reference for its references, the coverage of its ledger, the cap on
undecidable ReLU masks from the float64 chain alone, and the fusion counts of the 8 x 112 x 112 cases of
tests/test_plan_audit_gpu.py -- plans build without a GPU, as in tests/test_plan_graph_host.py."""
import pytest
import torch

from dualvar_amd import engine
from dualvar_amd.backbone import select_backbone
from oracle import procedural as P
from oracle import torch_ref as O
from tests import plan_audit as A
from tests.plan_audit import LARGE, NETS, SMALL, fusion_counts

CPU = torch.device('cpu')
_free = {}


def cpu_plan(net, dtype, N, T, HW, training=True, want_map=False, init=False):
    torch.manual_seed(0)
    m = select_backbone(net)[0]
    if init:
        P.procedural_init(m)
    m.set_compute_dtype(dtype)
    m.train(training)
    m.store.materialize(CPU, m.dtype)
    plan = m._acquire_plan(torch.empty(N, 3, T, HW, HW), False, want_map, training)
    m._plans.clear()
    return m, plan


def free_run(net, N, T, HW):
    """the float64 references free running over the fp32 plan's op list, once per case"""
    key = (net, N, T, HW)
    if key not in _free:
        m, plan = cpu_plan(net, 'fp32', N, T, HW, init=True)
        x = P.procedural_clips(N, 1, T, HW, HW)[:, 0].double()
        G = torch.randn(N, m.feature_size, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        _free[key] = (m, plan, x, G, A.Audit(plan, m, mode='free', x=x, dout=G).run())
    return _free[key]


@pytest.mark.parametrize('net', ['s3dg', 'r21d', 'c3d', 'r50'])
def test_free_running_references_reproduce_the_float64_model(net):
    """pooled output, every parameter gradient and the gradient of the first conv's output against oracle/torch_ref.py's
    module in float64 with autograd, to 1e-10 relative (of the largest element of the tensor; a conv bias in front of a
    BatchNorm has a gradient of exactly zero here and of cancellation noise there: below 1e-10 of the largest gradient)"""
    T, HW = SMALL[net]
    m, plan, x, G, a = free_run(net, 2, T, HW)
    o = O.select_backbone(net)[0]
    P.procedural_init(o)
    o.double().train()
    first = next(mod for mod in o.modules() if isinstance(mod, torch.nn.Conv3d))
    kept = {}

    def keep(_m, _i, out):
        out.retain_grad()
        kept['y'] = out
    hook = first.register_forward_hook(keep)
    pooled = o(x).mean((2, 3, 4))
    pooled.backward(G)
    hook.remove()
    rel = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())      # noqa: E731
    assert rel(a.load(plan.mean_op.out), pooled.detach()) <= 1e-10
    ref = o.state_dict(keep_vars=True)
    gmax = max(float(p.grad.abs().max()) for p in ref.values() if getattr(p, 'grad', None) is not None)
    names = {id(v): k for k, v in m.state_dict(keep_vars=True).items()}
    biases = {id(mem.conv_bias) for op in plan.ops if isinstance(op, engine.BNGroupOp) for mem in op.members if mem.conv_bias is not None}
    ga, worst = a.garena(), 0.0
    for s in m.store.slots:
        g, r = m.store._view(ga, s), ref[names[id(s.tensor)]].grad
        if id(s.tensor) in biases:
            assert float(g.abs().max()) == 0.0 and float(r.abs().max()) <= 1e-10 * gmax, names[id(s.tensor)]
            continue
        worst = max(worst, rel(g, r))
        assert rel(g, r) <= 1e-10, (names[id(s.tensor)], rel(g, r))
    conv1 = next(op for op in plan.ops if isinstance(op, engine.ConvOp))
    gy = a.act(conv1.y.grad).permute(0, 4, 1, 2, 3)
    assert rel(gy, kept['y'].grad) <= 1e-10
    print('\n  %s: pooled %.2e, worst gradient %.2e relative' % (net, rel(a.load(plan.mean_op.out), pooled.detach()), worst))


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('net', NETS)
def test_ledger_coverage(net, dtype, mode):
    T, HW = SMALL[net]
    m, plan = cpu_plan(net, dtype, 2, T, HW, training=mode == 'train')
    rows = A.Audit(plan, m, mode='dry').run().rows               # (an op type the walk does not know raises)
    assert {r.op for r in rows} == set(range(len(plan.ops)))
    for r in rows:
        assert r.how in ('direct', 'not applicable') or r.how.startswith('composite via '), r
        if r.how.startswith('composite via '):
            i, kind = r.how[len('composite via '):].split(':')
            assert type(plan.ops[int(i)]).__name__ == kind
    if mode == 'eval':
        assert not any(r.info and 'pids' in r.info for r in rows)
        return
    # every conv weight, BatchNorm parameter and gate parameter (and c3d's conv biases) in exactly one gradient row
    covered = [pid for r in rows if r.info and 'pids' in r.info for pid in r.info['pids']]
    params = {id(p) for p in m.parameters()}
    assert sorted(covered) == sorted(params)
    # every gradient buffer of the plan is tiled by the dx rows: each column of it in exactly one row
    width = {}
    for op in plan.ops:
        for a in list(op.inputs()) + [getattr(op, 'y', None)] + [mem.y for mem in getattr(op, 'members', ())]:
            if a is not None and a.grad is not None:
                k = engine._bufkey(a.grad)
                width[k] = max(width.get(k, 0), a.grad.off + a.C)
    if plan.mean_op is None:
        del width[engine._bufkey(plan.out_act.grad)]             # (the host writes it)
    spans = {}
    for r in rows:
        if r.qty.split('.')[-1] == 'dx':
            (k, off), C_ = r.info['act'], r.info['C']
            spans.setdefault(k, []).append((off, off + C_))
    assert set(spans) == set(width)
    for k, sp in spans.items():
        sp.sort()
        assert sp[0][0] == 0 and sp[-1][1] == width[k] and all(a[1] == b[0] for a, b in zip(sp, sp[1:])), sp


CAP_CASES = [(net, 2) + SMALL[net] for net in NETS] + [(net, LARGE[net][0], 8, 112) for net in sorted(LARGE)]


@pytest.mark.parametrize('case', CAP_CASES, ids=lambda c: '%s-%dx%dx%d' % c)
def test_undecidable_masks_stay_under_the_cap(case):
    """from the float64 chain alone, on the inputs the GPU cases use: at most 1e-4 of any tensor has a pre-activation inside
    its own forward bound"""
    a = free_run(*case)[4]
    masks = [r for r in a.rows if r.qty.endswith('.mask') and r.info]
    assert masks
    worst = max(r.info['undecidable'] for r in masks)
    print('\n  %s: %d masked tensors, largest undecidable fraction %.2e' % (case[0], len(masks), worst))
    assert all(r.ok for r in masks) and worst <= A.MASK_CAP


@pytest.mark.parametrize('net', sorted(LARGE))
def test_fusion_counts_of_the_large_cases(net):
    """the N of each 8 x 112 x 112 case is the smallest at which the shipped fp32 plan holds every fusion and pairing the net
    can hold; a change in routing shows up here before it reaches a GPU"""
    N, want = LARGE[net]
    assert fusion_counts(cpu_plan(net, 'fp32', N, 8, 112)[1]) == want
    kinds = [k for k, v in want.items() if v]
    for n in range(1, N):
        c = fusion_counts(cpu_plan(net, 'fp32', n, 8, 112)[1])
        assert any(c[k] == 0 for k in kinds), (n, c)
