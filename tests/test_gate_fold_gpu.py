"""S3D-G self gating folded into the BatchNorm passes around it (engine.FUSE_GATE; dv_gate_mean_bn, dv_gate_scale_bn,
dv_bn_bwd_reduce_multi_gated, dv_bn_bwd_apply_multi_gated).

The fused entry points promise the BITS of the sequences they replace, so each is compared with that sequence on the same
inputs with torch.equal:

    dv_bn_apply_multi -> dv_spatial_mean                                  ==  dv_gate_mean_bn
    dv_bn_apply_multi -> dv_gate_scale (in place)                         ==  dv_gate_scale_bn
    dv_gate_bwd_apply (in place) -> dv_bn_bwd_reduce_multi -> dv_bn_bwd_apply_multi
                                                                           ==  the two *_gated launches

Layout of a case: four gated members of widths 8, 24, 16, 8 (Ct = 56) writing slices of a concat buffer of pitch 72, two of
them reading x from a channel slice (non-zero 8-aligned offset) of a wider buffer, plus a fifth, un-gated member (offset -1,
C = 20: pad lanes) in the same backward launches, whose results must be those of the plain kernels.  Rows per block of the
backward reduce are not a multiple of S, so the row -> sample lookup crosses sample boundaries inside a block.

So that the fused backward is not only compared with other code of the library, it is also checked once against the float64
reference of tests/test_batchnorm_multi_gpu.py with that file's bounds: the gated gradient dy*g + dmean/S is evaluated by
torch in fp32, operation by operation as the header documents it, and handed to the float64 helpers as dL/dy.

The plan-level tests run one S3D-G training step with engine.FUSE_GATE off and on: same loss, same gradients, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import DV_BF16, DV_F32  # noqa: E402
from tests import bn_support as B  # noqa: E402
from tests.checks import View, bits, is_sent, launch, sent  # noqa: E402

WIDTHS = (8, 24, 16, 8)
OFFS = (0, 8, 32, 48)
CT = 56
CAT_LD = 72                        # concat pitch > Ct
SLICED_X = (1, 3)                  # members whose x (and dx) are channel slices of wider buffers
UNGATED_C = 20
SHAPES = [(3, 98), (37, 9)]        # (N, S)


def _shared_view(dtype, M, C_, off, buf, values=None):
    """a tests.checks.View on columns [off, off + C) of an existing [M][ld] buffer"""
    v = View(dtype, M, C_, off, buf.shape[1], buf.device)
    v.buf = buf
    if values is not None:
        v.set(values, pad=None)
    return v


class Level:
    """the members of one gated level (+ one un-gated member), their concat buffers and the gate tables"""

    def __init__(self, dev, dtype, N, S):
        self.dev, self.dtype, self.N, self.S, self.M = dev, dtype, N, S, N * S
        M = self.M
        self.cat = sent((M, CAT_LD), dev, dtype)
        self.dcat = sent((M, CAT_LD), dev, dtype)
        self.members = []
        for k, (w, off) in enumerate(zip(WIDTHS, OFFS)):
            m = B.Member(dev, dtype, M, w, seed=100 + 17 * k, exact=False, from_x=True, views=k in SLICED_X)
            if k in SLICED_X:
                assert m.x.off > 0 and m.x.off % 8 == 0 and m.x.ld > m.x.off + w
            m.y = _shared_view(dtype, M, w, off, self.cat)
            m.dy = _shared_view(dtype, M, w, off, self.dcat, m.dy.val())
            self.members.append(m)
        self.members.append(B.Member(dev, dtype, M, UNGATED_C, seed=999, exact=False, from_x=True, views=True))
        self.gate_off = torch.tensor(list(OFFS) + [-1], dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(7 + N)
        self.g = torch.sigmoid(torch.randn(N, CT, generator=gen, device=dev))
        self.dmean = torch.randn(N, CT, generator=gen, device=dev) * 4
        self.mean = sent((N * CT,), dev).view(N, CT)

    @property
    def gated(self):
        return self.members[:4]

    def table(self, sums_idx=0):
        return B.make_table(self.members, L.load(), self.dev, self.dtype, sums_idx=sums_idx)

    def apply_multi(self):
        tab, ends = self.table()
        launch('dv_bn_apply_multi', self.dtype, tab.data_ptr(), len(self.members), ends['apply'])

    def backward_outputs(self):
        out = []
        for m in self.members:
            out += [m.sums[0], bits(m.dx.buf), m.dgamma, m.dbeta]
        return [bits(t) if t.dtype == torch.float32 else t for t in out]


DTYPES = [pytest.param(DV_F32, id='fp32'), pytest.param(DV_BF16, id='bf16')]


def test_reduce_blocks_cross_sample_boundaries():
    """the shapes above give the backward reduce more than one block per member, with a row count per block that is no
    multiple of S: the gate's row / S lookup changes sample inside a block"""
    lib = L.load()
    hit = 0
    for N, S in SHAPES:
        for w in WIDTHS:
            nb = int(lib.dv_bn_bwd_blocks(N * S, w))
            rpb = -(-(N * S) // nb)
            hit += nb > 1 and rpb % S != 0
    assert hit >= 1
    assert all(int(lib.dv_bn_bwd_blocks(N * S, w)) > 1 and (-(-(N * S) // int(lib.dv_bn_bwd_blocks(N * S, w)))) % S != 0
               for N, S in SHAPES for w in WIDTHS)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,S', SHAPES)
def test_gate_mean_and_scale_equal_the_unfused_sequence(gpu, dtype, N, S):
    a, b = Level(gpu, dtype, N, S), Level(gpu, dtype, N, S)
    n = len(a.members)
    # today's sequence
    a.apply_multi()
    launch('dv_spatial_mean', dtype, a.cat.data_ptr(), CAT_LD, N, S, CT, a.mean.data_ptr())
    launch('dv_gate_scale', dtype, a.cat.data_ptr(), CAT_LD, a.g.data_ptr(), N, S, CT, a.cat.data_ptr(), CAT_LD)
    # fused
    tab, _ = b.table()
    launch('dv_gate_mean_bn', dtype, tab.data_ptr(), n, b.gate_off.data_ptr(), N, S, CT, b.mean.data_ptr())
    torch.cuda.synchronize()
    assert b.members[0].y.untouched(), 'dv_gate_mean_bn wrote the concat'
    launch('dv_gate_scale_bn', dtype, tab.data_ptr(), n, b.gate_off.data_ptr(), a.g.data_ptr(), N, S, CT)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a.mean).all()) and float(a.mean.abs().max()) > 0
    assert torch.equal(bits(a.mean), bits(b.mean)), float((a.mean - b.mean).abs().max())
    assert torch.equal(bits(a.cat), bits(b.cat)), 'gated concat differs (or a column past Ct was written)'
    assert is_sent(b.cat[:, CT:])
    assert b.members[4].y.untouched(), 'the un-gated member is not the gate kernels\' to write'
    for m in b.members:
        assert not m.x.untouched() and m.dx.untouched()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,S', SHAPES)
def test_gated_batchnorm_backward_equals_the_unfused_sequence(gpu, dtype, N, S):
    a, b = Level(gpu, dtype, N, S), Level(gpu, dtype, N, S)
    n = len(a.members)
    lib = L.load()
    dcat0 = b.dcat.clone()
    # the un-gated activation, as the backward's float64 reference takes its ReLU mask
    a.apply_multi()
    torch.cuda.synchronize()
    y_in = [m.y.val() for m in a.members]
    # today's sequence: the gate rewrites dy in place, then the plain BatchNorm backward
    launch('dv_gate_bwd_apply', dtype, a.dcat.data_ptr(), CAT_LD, a.g.data_ptr(), a.dmean.data_ptr(), N, S, CT,
             a.dcat.data_ptr(), CAT_LD, 0)
    tab, ends = a.table()
    launch('dv_bn_bwd_reduce_multi', dtype, tab.data_ptr(), n, ends['red'])
    launch('dv_bn_bwd_apply_multi', dtype, tab.data_ptr(), n, ends['bapply'], max(m.C for m in a.members))
    # fused: gate on load
    tab, ends = b.table()
    gargs = (a.g.data_ptr(), a.dmean.data_ptr(), S, CT, b.gate_off.data_ptr())
    launch('dv_bn_bwd_reduce_multi_gated', dtype, tab.data_ptr(), n, ends['red'], *gargs)
    launch('dv_bn_bwd_apply_multi_gated', dtype, tab.data_ptr(), n, ends['bapply'], max(m.C for m in b.members), *gargs)
    torch.cuda.synchronize()
    assert torch.equal(bits(b.dcat), bits(dcat0)), 'the gated launches must leave dy as it was'
    assert not torch.equal(bits(a.dcat), bits(dcat0))
    names = [f'member {i} {what}' for i in range(n) for what in ('sums', 'dx', 'dgamma', 'dbeta')]
    for name, x, y in zip(names, a.backward_outputs(), b.backward_outputs()):
        assert torch.equal(x, y), name
    for i, m in enumerate(b.members):
        B.check_ticket_area(m, f'member {i}')
        assert bool(torch.isfinite(m.sums[0][:m.C]).all()) and float(m.sums[0].abs().max()) > 0
    if (N, S) != SHAPES[0]:
        return
    # once against float64 (tests/test_batchnorm_multi_gpu.py's reference and bounds): dL/dy of a gated member is the
    # documented fp32 expression, evaluated by torch one operation at a time and rounded to the storage type
    tdt = ops.TORCH_DTYPE[dtype]
    inv_s = torch.tensor(1.0, dtype=torch.float32, device=gpu) / S
    rows = torch.arange(N * S, device=gpu) // S
    for i, m in enumerate(b.members):
        if i < 4:
            cols = slice(OFFS[i], OFFS[i] + m.C)
            dy = dcat0[:, cols].float()
            gated = (dy * a.g[rows][:, cols] + a.dmean[rows][:, cols] * inv_s).to(tdt)
            m.dy = View(dtype, m.M, m.C, 0, m.C, gpu, gated.double(), pad=None)
        g, xhat = B.backward_terms(m, y_in[i])
        B.check_reduce(m, m.sums[0], g, xhat, 1, f'gated member {i}')
        B.check_bwd_apply(m, g, m.sums[0], 1.0 / m.M, f'gated member {i}')
    assert int(lib.dv_bn_bwd_blocks(N * S, 8)) > 1


# ----------------------------------------------------------------------------------------------------------- plans
def _step(gpu, monkeypatch, kind, dtype, on):
    from dualvar_amd import engine, model as M
    monkeypatch.setattr(engine, 'FUSE_GATE', on)
    block = torch.randn(4, 2, 3, 8, 112, 112, generator=torch.Generator().manual_seed(3)).to(gpu)
    torch.manual_seed(0)
    m = M.SimCLR_Naked('s3dg', 128, 0.07, False) if kind == 'simclr_naked' else M.MoCo_Naked('s3dg', 128, 256, 0.999, 0.07, False)
    m.set_compute_dtype(dtype).train().to(gpu)
    ret = m(block)
    for st in m.stores():
        st.zero_grad()
    ret['clip_contrast_loss'].backward()
    torch.cuda.synchronize()
    loss = ret['clip_contrast_loss'].detach().clone()
    grads = torch.cat([st.grad.detach().float().flatten().clone() for st in m.stores()])
    plans = [pl for mod in m.modules() if hasattr(mod, '_plans') for lst in mod._plans.values() for pl in lst]
    names = [l.name for pl in plans for l in pl.f_list + pl.b_list]
    fused = [sum(1 for op in pl.ops if getattr(op, 'fused', None)) for pl in plans]
    return loss, grads, names, fused, [pl.with_grad for pl in plans]


@pytest.mark.parametrize('kind,dtype', [('simclr_naked', 'fp32'), ('simclr_naked', 'bf16'), ('moco_naked', 'fp32')])
def test_gate_fold_plan_gives_the_same_bits(gpu, monkeypatch, kind, dtype):
    """engine.FUSE_GATE (default on): one S3D-G step (4 samples x 2 views of 8 x 112 x 112) with the self gating folded into
    the BatchNorm passes and without: the loss and every gradient agree BIT FOR BIT.  MoCo's key encoder takes the
    no-gradient forward plan."""
    off = _step(gpu, monkeypatch, kind, dtype, False)
    on = _step(gpu, monkeypatch, kind, dtype, True)
    print(kind, dtype, 'gate ops fused per plan:', off[3], on[3], 'loss', float(off[0]), float(on[0]))
    assert all(f == 0 for f in off[3]) and 'gate_scale' in off[2] and 'gate_bwd_apply' in off[2]
    assert on[3] and all(f == 9 for f in on[3]), on[3]
    assert 'gate_scale' not in on[2] and 'gate_bwd_apply' not in on[2]
    assert 'gate_mean_bn' in on[2] and 'gate_scale_bn' in on[2]
    if kind == 'moco_naked':
        assert sorted(on[4]) == [False, True], on[4]
    assert bool(torch.isfinite(on[1]).all()) and float(on[1].abs().max()) > 0
    assert torch.equal(off[0], on[0]), (float(off[0]), float(on[0]))
    assert torch.equal(off[1], on[1]), float((off[1] - on[1]).abs().max())
