"""MI355X: what tests/test_plan_streams_host.py takes on trust.

  * Declared writes are the real writes.  After one real forward and backward, every launch of f_list / b_list runs again, alone,
    on the state the pass left: the allocations it points at (tests/plan_hazards.scan) and declares are cloned before, compared
    after -- every byte outside the declared write ranges must be unchanged -- and restored.  The ticket words of an ordered
    reduction's workspace read zero after any launch that touches it.  The host checks order launches by their declared sets; the
    direction of each access (a write declared as a read would hide a race) is only visible here.
  * Two streams give the bits of one.  The backward with engine.WGRAD_SIDE_STREAM off is the list order; the gradient arena and
    every activation gradient after it must equal, bit for bit, those of the pass as shipped, with WGRAD_BATCH 1 and 10**6, and
    with early release forced off and on -- each setting run twice in a row on the same plan, without a host synchronisation in
    between, so that a launch still in flight when the next pass starts would show.  Same kernels, same operands, ordered
    reductions: equality is what the code promises.

Shapes: tests/plan_audit.SMALL (s3dg 8 x 64 x 64, r21d / r3d 1 x 32 x 32, r50 1 x 48 x 48), N = 2, fp32 and bf16.  No launch here runs
with arguments other than the plan's own."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import engine, ops  # noqa: E402
from tests import plan_hazards as H  # noqa: E402
from tests.plan_audit import SMALL  # noqa: E402
from tests.test_plan_audit_gpu import clips, gauss, make  # noqa: E402

NETS = ('s3dg', 'r21d', 'r3d', 'r50')
DTYPES = ('fp32', 'bf16')
POISON = 0xA5


def one_pass(m, x):
    m.store.zero_grad()
    out = m.forward_pooled(x)
    out.backward(gauss(out.shape, x.device))


def the_plan(m):
    plans = [p for v in m._plans.values() for p in v]
    assert len(plans) == 1
    return plans[0]


def ticket_words(plan):
    """[(name, the ticket words of an ordered reduction's workspace)]: they read zero between launches (dualvar_amd/_lib.py:
    register_ticket_workspace).  A BatchNorm member's red_ws is [rows][2][CP] partial sums, then the tickets: one per group of 32
    blocks and one for the groups, rounded up to 8 words (include/dualvar_hip.h: dv_bn_bwd_reduce_workspace)."""
    out = []
    for i, op in enumerate(plan.ops):
        for j, m in enumerate(getattr(op, 'members', ())):
            if getattr(m, 'red_ws', None) is not None:
                nblk = int(plan.lib.dv_bn_bwd_blocks(m.M, m.C))
                groups = (nblk + 31) // 32
                tw = (groups + 1 + 7) & ~7
                assert m.red_ws.numel() == (nblk + groups) * 2 * m.CP + tw, 'the workspace layout this test reads has changed'
                out.append(('ops[%d].members[%d].red_ws' % (i, j), m.red_ws, m.red_ws[-tw:]))
    if getattr(plan, 'bn_fuse_ws', None) is not None:
        out.append(('bn_fuse_ws', plan.bn_fuse_ws, plan.bn_fuse_ws[:16384]))      # (its tickets: the first 64 KiB)
    return out


@pytest.mark.parametrize('which', ['f_list', 'b_list'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', NETS)
def test_declared_writes_are_the_real_writes(gpu, net, dtype, which):
    T, HW = SMALL[net]
    m = make(net, dtype, gpu)
    x = clips(2, T, HW, gpu)
    one_pass(m, x)
    torch.cuda.synchronize()
    plan = the_plan(m)
    reg = H.Registry(plan)
    assert not H.check_complete(plan, reg)              # (on the device too; the clips are bound now)
    tickets = ticket_words(plan)
    assert tickets and all(not bool(t.any()) for _, _, t in tickets)
    ticket_of = {}
    for name, ws, t in tickets:
        ticket_of.setdefault(reg.find(ws.data_ptr()), []).append((name, t))
    bad, n_checked, n_poisoned = [], 0, 0
    s = ops.stream_ptr()
    for l in getattr(plan, which):
        spans = [H.norm(reg, a) for a in l.writes]
        read = {H.norm(reg, a).alloc for a in l.reads}
        touched = set(H.scan(reg, l)) | {sp.alloc for sp in spans} | read
        before = {a: a.bytes().clone() for a in touched}
        # An allocation the launch only writes is filled with a pattern first: a stray write there shows even if it stores the
        # value the real pass left.  Where the launch also reads, a write shows if it changes a byte.
        for a in touched - read:
            a.bytes().fill_(POISON)
            n_poisoned += 1
        l(s)
        torch.cuda.synchronize()
        for a, was in before.items():
            now = a.bytes()
            allowed = torch.zeros(a.nbytes, dtype=torch.bool, device=gpu)
            for sp in spans:
                if sp.alloc is a:
                    sp.mask(allowed)
            stray = ((now != POISON) if a not in read else (now != was)) & ~allowed
            if bool(stray.any()):
                bad.append('%s changed %d bytes of %s outside its declared writes, the first at byte %d' % (
                    H.label(l), int(stray.sum()), a.name, int(stray.nonzero()[0])))
            for name, t in ticket_of.get(a, ()):
                if bool(t.any()):
                    bad.append('%s left ticket words of %s set' % (H.label(l), name))
            now.copy_(was)
            n_checked += 1
    torch.cuda.synchronize()
    print('\n  %s %s %s: %d launches, %d allocations compared, %d of them write-only and filled with a pattern first' % (
        net, dtype, which, len(getattr(plan, which)), n_checked, n_poisoned))
    assert n_checked >= 2 * len(getattr(plan, which)) and n_poisoned > 0
    assert not bad, '\n'.join(bad[:20])


def backward_outputs(plan):
    """the gradient arena and every activation the backward list writes (the activation gradients), as stream-ordered copies"""
    bufs, seen = [('store.grad', plan.store.grad)], {plan.store.grad.untyped_storage().data_ptr()}
    for l in plan.b_list:
        for w in l.writes:
            if isinstance(w, ops.Act) and w.buf.untyped_storage().data_ptr() not in seen:
                seen.add(w.buf.untyped_storage().data_ptr())
                bufs.append(('%s -> %s' % (H.label(l), tuple(w.buf.shape)), w.buf))
    return [(name, t.clone()) for name, t in bufs]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', NETS)
def test_two_streams_give_the_bits_of_one(gpu, net, dtype, monkeypatch):
    T, HW = SMALL[net]
    m = make(net, dtype, gpu)
    x = clips(2, T, HW, gpu)
    one_pass(m, x)                                      # (builds the plan; every later pass starts from a zeroed arena)
    torch.cuda.synchronize()
    plan = the_plan(m)
    early0, batch0 = plan.wgrad_early, engine.WGRAD_BATCH
    n_side = sum(1 for l in plan.b_list if l.name in engine.SIDE_LAUNCHES)
    assert n_side > 0

    def twice(side, batch, early):
        monkeypatch.setattr(engine, 'WGRAD_SIDE_STREAM', side)
        monkeypatch.setattr(engine, 'WGRAD_BATCH', batch)
        plan.wgrad_early = early
        got = []
        for _ in range(2):                              # back to back: no host synchronisation between the passes
            one_pass(m, x)
            got.append(backward_outputs(plan))
        assert the_plan(m) is plan
        return got
    try:
        ref = twice(False, batch0, early0)
        torch.cuda.synchronize()
        assert len(ref[0]) > 10 and bool((ref[0][0][1] != 0).any())
        settings = [('as shipped', batch0, early0), ('WGRAD_BATCH 1', 1, early0), ('WGRAD_BATCH 10**6', 10 ** 6, early0),
                    ('early release off', batch0, False), ('early release on', batch0, True)]
        runs = [('one stream, second pass', ref[1])]
        for what, batch, early in settings:
            for i, got in enumerate(twice(True, batch, early)):
                runs.append(('%s, pass %d' % (what, i + 1), got))
        torch.cuda.synchronize()
    finally:
        plan.wgrad_early = early0
    bad = []
    for what, got in runs:
        assert [n for n, _ in got] == [n for n, _ in ref[0]]
        for (name, want), (_, have) in zip(ref[0], got):
            if not torch.equal(want.view(torch.uint8), have.view(torch.uint8)):
                d = (want.view(torch.uint8) != have.view(torch.uint8)).sum()
                bad.append('%s: %s differs from the one-stream pass in %d bytes' % (what, name, int(d)))
    print('\n  %s %s: %d buffers x %d passes compared with the one-stream pass, %d side launches' % (
        net, dtype, len(ref[0]), len(runs), n_side))
    assert not bad, '\n'.join(bad[:20])
