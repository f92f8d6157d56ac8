"""Every op of a backbone's launch plan against float64, in fp32 and bf16: tests/plan_audit.py walks the plan after one real
forward and backward pass and checks each op alone, on the inputs the plan stored for it.

Drive: procedural weights and clips (oracle/procedural.py), `.train()`, forward_pooled(x), pooled.backward(G) with a fixed
Gaussian G, the plan from the backbone's cache, switches as shipped.  Every case prints its ledger size and its largest
err / bound; the module prints the largest ratio per (op kind, quantity, dtype) at the end (DESIGN.md section 2 has the table).

SMALL: the smallest T x H x W (by volume, T in 1..16, H = W in 16..112) at which the net's plan builds on the CPU with a final map
of at least 2 x 2 -- found with plans built on the CPU, as tests/test_plan_graph_host.py builds them.  N = 2.  The last
level of each has M = 8 rows: partial tiles and the small-M routes.
LARGE: 8 x 112 x 112 at the smallest N at which the shipped fp32 plan holds at least one of every fusion and pairing the net can
hold (tests/test_plan_audit_host.py pins the counts without a GPU): S3D-G needs N = 8 for the paired spatial / temporal forwards and
the paired data gradients, R(2+1)D N = 3 for BatchNorm on load.

Mutants (S3D-G, SMALL, fp32), each applied to the Python plan objects and memory-safe by construction (a flag, or two pointers to
buffers of the same size exchanged): the audit must fail at the mutated op's rows and nowhere else.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L  # noqa: E402
from dualvar_amd import engine  # noqa: E402
from dualvar_amd._lib import DV_ACCUM  # noqa: E402
from tests import plan_audit as A  # noqa: E402
from tests.plan_audit import LARGE, NETS, SMALL, fusion_counts  # noqa: E402

DTYPES = ['fp32', 'bf16']


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    A.report()


def make(net, dtype, dev, training=True):
    from dualvar_amd.backbone import select_backbone
    from oracle import procedural as P
    m, _ = select_backbone(net)
    P.procedural_init(m)
    m.set_compute_dtype(dtype).train(training).to(dev)
    return m


def clips(N, T, HW, dev, seed=1234):
    from oracle import procedural as P
    return P.procedural_clips(N, 1, T, HW, HW, seed=seed)[:, 0].to(dev)


def gauss(shape, dev, seed=5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def one_pass(m, x, want_map=False, mutate=None, between=None):
    """forward (+ backward when the module trains) on the plan the backbone caches for x -> (plan, pre, snaps)"""
    m.prepare(x.device)
    plan = m._acquire_plan(x, False, want_map, with_grad=m.training)
    if mutate is not None:
        mutate(plan)
    snaps, pre = A.arm(plan), A.capture(m)
    try:
        if m.training:
            out = m(x) if want_map else m.forward_pooled(x)
            if between is not None:
                torch.cuda.synchronize()
                between(plan, pre, snaps)
            out.backward(gauss(out.shape, x.device))
        else:
            with torch.no_grad():
                m(x) if want_map else m.forward_pooled(x)
        torch.cuda.synchronize()
    finally:
        A.disarm(plan)
    assert sum(len(v) for v in m._plans.values()) == 1, 'the pass did not run on the plan that was prepared'
    return plan, pre, snaps


def green(a, what):
    kinds = {r.how.split(' ')[0] for r in a.rows}
    assert kinds <= {'direct', 'composite', 'not'}, kinds
    print('\n  %s: %d ledger rows, largest err / bound %.3f' % (what, len(a.rows), a.worst()))
    bad = a.failed()
    assert not bad, '%s: %d rows outside their bound, first: %s' % (what, len(bad), [(r.op, r.kind, r.qty, r.ratio) for r in bad[:8]])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', NETS)
def test_small(gpu, net, dtype):
    T, HW = SMALL[net]
    m = make(net, dtype, gpu)
    plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu))
    green(A.Audit(plan, m, pre, snaps).run(), '%s %s 2x%dx%dx%d' % (net, dtype, T, HW, HW))


@pytest.mark.parametrize('net', sorted(LARGE))
def test_large_holds_every_fusion(gpu, net):
    N, want = LARGE[net]
    m = make(net, 'fp32', gpu)
    plan, pre, snaps = one_pass(m, clips(N, 8, 112, gpu))
    assert fusion_counts(plan) == want
    green(A.Audit(plan, m, pre, snaps).run(), '%s fp32 %dx8x112x112' % (net, N))


def test_map_output(gpu):
    """m(x): no pooled mean, the backward starts from out_act.grad"""
    T, HW = SMALL['s3dg']
    m = make('s3dg', 'fp32', gpu)
    plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu), want_map=True)
    assert plan.mean_op is None
    green(A.Audit(plan, m, pre, snaps).run(), 's3dg fp32 map output')


def test_two_passes_accumulate(gpu):
    """two passes on different inputs without zero_grad: each pass's gradient rows are the arena BEFORE the pass plus that pass's
    float64 dw, inside that pass's bound plus the one fp32 addition -- so the final gradient is the float64 sum of the two
    passes' dw inside the two bounds"""
    T, HW = SMALL['r21d']
    m = make('r21d', 'fp32', gpu)
    for i, seed in enumerate((1234, 77)):
        plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu, seed=seed))
        assert bool((pre['grad'] != 0).any()) == (i == 1)
        green(A.Audit(plan, m, pre, snaps).run(), 'r21d fp32 pass %d' % (i + 1))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', ['s3dg', 'c3d'])
def test_eval_plans(gpu, net, dtype):
    """.eval(): running statistics, forward only; c3d folds its conv bias into the shift; S3D-G's gate runs unfused, in place"""
    T, HW = SMALL[net]
    m = make(net, dtype, gpu)
    with torch.no_grad():
        m.forward_pooled(clips(2, T, HW, gpu, seed=77))            # (running statistics that are not 0 / 1)
    m.eval()
    m._plans.clear()
    plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu))
    if net == 's3dg':
        assert len(snaps) == 9
    green(A.Audit(plan, m, pre, snaps).run(), '%s %s eval' % (net, dtype))


# ------------------------------------------------------------------------------------------------------------ mutants
def _s3dg_pass(gpu, mutate=None, between=None):
    T, HW = SMALL['s3dg']
    m = make('s3dg', 'fp32', gpu)
    plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu), mutate=mutate, between=between)
    return m, plan, pre, snaps


def test_mutant_dropped_accumulate_flag(gpu):
    """DV_ACCUM dropped for the max-pool reader of an Inception level's input gradient"""
    hit = {}

    def mutate(plan):
        for op in plan.ops:
            if isinstance(op, engine.PoolOp) and op.acc.get('x'):
                for l in plan.b_list:
                    if l.name == 'maxpool_bwd' and l.args[3] == op.x.grad.ptr and l.args[4] == DV_ACCUM:
                        l.args = l.args[:4] + (0,)
                        hit['key'] = engine.PlanGraph._gkey(op.x)
                        return
        raise AssertionError('no accumulating pool in the plan')
    m, plan, pre, snaps = _s3dg_pass(gpu, mutate)
    bad = A.Audit(plan, m, pre, snaps, record=False).run().failed()
    print('\n  mutant 1 fails:', [(r.op, r.kind, r.qty, r.ratio) for r in bad])
    assert [(r.qty, r.info['act']) for r in bad] == [('dx', hit['key'])]


def test_mutant_stale_dgrad_weights(gpu):
    """a conv's master weight moved by 1 % between the forward and the backward, without a refresh: its data gradient still
    multiplies with the old dgrad-layout copy"""
    hit = {}

    def between(plan, pre, snaps):
        hit['fwd'] = A.Audit(plan, hit['m'], pre, snaps).run(backward=False)
        op = [o for o in plan.ops if isinstance(o, engine.ConvOp) and o.need_dx and o.slot.kind == 'conv' and o.k == (3, 1, 1)][3]
        op.slot.tensor.data.mul_(1.01)
        hit['op'] = plan.ops.index(op)
    T, HW = SMALL['s3dg']
    m = hit['m'] = make('s3dg', 'fp32', gpu)
    plan, pre, snaps = one_pass(m, clips(2, T, HW, gpu), between=between)
    assert not hit['fwd'].failed()
    bad = A.Audit(plan, m, pre, snaps, record=False).run(forward=False).failed()
    print('\n  mutant 2 fails:', [(r.op, r.kind, r.qty, r.ratio) for r in bad])
    assert [(r.op, r.qty) for r in bad] == [(hit['op'], 'dx')]


def test_mutant_exchanged_batchnorm_coefficients(gpu):
    """two members of one BatchNorm group with equal C exchange their scale and shift pointers in the group's item table"""
    hit = {}

    def mutate(plan):
        for op in plan.ops:
            if isinstance(op, engine.BNGroupOp) and len(op.members) > 1:
                ms = op.members
                pairs = [(i, j) for i in range(len(ms)) for j in range(i + 1, len(ms)) if ms[i].C == ms[j].C]
                if pairs:
                    i, j = pairs[0]
                    arr = (L.BnItem * len(ms)).from_buffer_copy(bytes(op._items.cpu().numpy()))
                    for f in ('scale', 'shift'):
                        a, b = getattr(arr[i], f), getattr(arr[j], f)
                        setattr(arr[i], f, b)
                        setattr(arr[j], f, a)
                    op._items.copy_(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
                    hit.update(op=plan.ops.index(op), i=i, j=j)
                    return
        raise AssertionError('no BatchNorm group with two members of equal C')
    m, plan, pre, snaps = _s3dg_pass(gpu, mutate)
    bad = A.Audit(plan, m, pre, snaps, record=False).run().failed()
    print('\n  mutant 3 fails:', [(r.op, r.kind, r.qty, r.ratio) for r in bad])
    assert bad and {r.op for r in bad} == {hit['op']}
    assert {'m%d.%s' % (k, q) for k in (hit['i'], hit['j']) for q in ('scale', 'shift')} <= {r.qty for r in bad}
