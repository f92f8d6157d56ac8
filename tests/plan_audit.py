"""Op-by-op audit of an engine.Plan against float64 (not a test file: tests/test_plan_audit_gpu.py and _host.py drive it).

After run_forward (and run_backward) every activation and gradient of a plan is still resident, so each op is checked ALONE:
its inputs are taken as the plan stored them (teacher forcing), that one op is computed in float64 by torch, and the result is
compared with what the plan stored as the op's output.  The error of one op is that op's own arithmetic: the bounds are the
per-entry tests' expressions, imported where those files have them as functions and restated next to a citation otherwise.

Three modes, one walk over plan.ops (an op type the walk does not know raises):
  audit   GPU, after a real pass: compares, returns the ledger
  dry     no data (plans built on the CPU): only the ledger's rows, for the coverage test
  free    CPU float64, free running: each op's float64 output feeds the next through float64 shadows of the plan's buffers; the
          host test compares the end of that chain with oracle/torch_ref.py's model, so a slip in this file's reading of the plan
          (padding, residual, gate slice, accumulate flag) cannot hide a slip in the plan

A ledger row is (op index, op kind, quantity, how, err / bound, ok): how is 'direct' (the quantity is stored and compared),
'composite via <i>:<Op>' (never stored: it is checked inside the first stored quantity downstream, whose reference is the composite
float64 expression and whose bound carries the intermediate's) or 'not applicable'.  Which quantities are not stored is read from
the plan's own markers: fused_conv / bn_in (BatchNorm on load), fused_pool, gate (FUSE_GATE), apply_fused / bn_apply
(BatchNorm-backward apply inside the stem's weight gradient).  reduce_fused / bn_fuse (FUSE_BN_REDUCE, FUSE_BN_REDUCE_TAP: off
as shipped), fp8 convs, world > 1 exchanges and an unfused gate's in-place backward raise NotImplementedError.

Bounds (u = 2^-24; bf16 store: half a bf16 ulp of |ref| + b, i.e. 2^-8 (|ref| + b)):
  conv y / dx / dw      gauss_bound of tests/conv_reference.py on the float64 S = sum|terms| and cnt, with the route the
                        library reports for the op's own descriptor (K-split fold, slab additions, split3 / split3w drop terms)
  DV_STATS partials     the expressions of _stats_check (tests/test_conv_float64_gpu.py, restated in stats_partials below)
  BatchNorm             check_finalized / check_apply / check_reduce / check_bwd_apply of tests/bn_support.py
                        (restated: they take that file's Member objects), eval coefficients as test_eval_chain_against_float64
  pool                  values exact, the stored tap points at an element equal to the maximum; dx: (windows - 1) u sum|gy|
  gate, mean            run_means_and_gates of tests/test_pool_gate_float64_gpu.py; the FC: any order of the K + 1 additions,
                        gamma(K + 1) sum|terms|, then the sigmoid's bound of check_desc_result (tests/test_loss_gemm_optim_gpu.py)
                        and |sigma(a) - sigma(b)| <= |a - b| / 4
  several writers       each writer's bound, plus one storage rounding per `+=` (u, or 2^-8 in bf16, of the running total)
Composite bounds no per-entry test has, derived from the stated roundings.  An intermediate v that is formed in registers with
|v_kernel - v_float64| <= e (elementwise, e from the intermediate's own per-entry bound) enters a bilinear op (conv, weight
gradient, mean, product with the gate) linearly, so the op's output moves by at most op(e, |other operand|): that term is added
to the op's bound, and the op's own bound is evaluated on |v| + e.  BatchNorm on load in front of the operand split: v = relu(x
scale + shift) is formed in fp32 (3 u (|x scale| + |shift|), check_apply's count) BEFORE split3, so the split sees an fp32 number
and gauss_bound applies unchanged; |relu(a) - relu(b)| <= |a - b| covers an activation whose sign the rounding decides.  A max
over a window moves by at most the largest e in the window.

ReLU masks: an element is undecidable when |x scale + shift| in float64 is at most its own forward bound; such elements are left
out of dx, widen the two sums by sum|dy| / sum|dy xhat| over them, and may be at most 1e-4 of any tensor ('mask' rows).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from dualvar_amd import _lib as L
from dualvar_amd._lib import DV_F32
from dualvar_amd.backbone.base import IngestOp
from dualvar_amd.engine import BNGroupOp, ConvOp, GateGroupOp, MeanOp, PlanGraph, PoolOp, _bufkey
from tests import bn_cases
from tests import conv_cases as CT
from tests.chains import bwd_reduce_chain, column_chain, e_exp, gamma, m2_bound, stats_chain
from tests.checks import BF16_U, F64, U, ceil_div, cp8, vec
from tests.conv_reference import gauss_bound, ref_dgrad, ref_fwd, ref_wgrad
from tests.pool_reference import ref_pool_bwd, ref_pool_fwd

MASK_CAP = 1e-4
Row = namedtuple('Row', 'op kind qty how ratio ok info')
Shim = namedtuple('Shim', 'dtype fwd dgrad wgrad')           # what gauss_bound reads of a conv_cases.Case
PoolShim = namedtuple('PoolShim', 'N T H W C k s p')         # what ref_pool_fwd / ref_pool_bwd read of a pool_cases.PoolCase
RATIOS = {}                                                  # (op kind, quantity, dtype) -> largest err / bound of the process
# the cases of tests/test_plan_audit_gpu.py and _host.py: net -> (T, H = W) of the SMALL cases
SMALL = {'s3dg': (8, 64), 'r21d': (1, 32), 'r3d': (1, 32), 'r50': (1, 48), 's3d': (8, 64), 'r2d3d18': (1, 48), 'c3d': (8, 32)}
NETS = tuple(SMALL)
# net -> N of the LARGE (8 x 112 x 112, fp32) cases and the counts the plan must hold there
LARGE = {'s3dg': (8, dict(bn_in=1, bn_wgrad=1, pool=2, gate=9, pair_fwd_sp=1, pair_fwd_tm=1, pair_dgrad=1, pair_ks=20)),
         'r21d': (3, dict(bn_in=1, bn_wgrad=1, pool=0, gate=0, pair_fwd_sp=0, pair_fwd_tm=0, pair_dgrad=0, pair_ks=0))}


def fusion_counts(plan):
    """how many of each fusion and pairing a plan holds"""
    c = dict(bn_in=0, bn_wgrad=0, pool=0, gate=0, pair_fwd_sp=0, pair_fwd_tm=0, pair_dgrad=0, pair_ks=0)
    for op in plan.ops:
        if isinstance(op, ConvOp):
            c['bn_in'] += op.bn_in is not None
            c['bn_wgrad'] += op.bn_apply is not None
        elif isinstance(op, PoolOp):
            c['pool'] += op.bn_member is not None
        elif isinstance(op, GateGroupOp):
            c['gate'] += bool(op.fused)
    for l in plan.f_list + plan.b_list:
        if getattr(l, 'members', ()):
            key = ('pair_ks' if 'conv_gemm_ks' in l.kname else 'pair_dgrad' if l.name == 'conv_dgrad'
                   else 'pair_fwd_sp' if ',sp,' in l.kname else 'pair_fwd_tm' if ',tm,' in l.kname else None)
            assert key is not None, l.kname
            c[key] += 1
    return c


def capture(model):
    """what an audit needs from BEFORE the pass: the running statistics and the gradient arena"""
    st = model.store
    return dict(grad=st.grad.clone() if st.grad is not None else None,
                running={id(bn): (bn.running_mean.clone(), bn.running_var.clone()) for bn in st.nbt if bn.running_mean is not None})


def arm(plan):
    """snapshot, through Plan.timer, the buffers a later launch overwrites in place: the concat in front of an unfused gate_scale.
    -> the dict the snapshots land in (Audit(snaps=...)); disarm() takes the hook off again"""
    snaps = {}
    gates = {op.cat.ptr: op for op in plan.ops if isinstance(op, GateGroupOp) and not op.fused}

    def hook(launch, stream, side=None):
        if launch.name == 'gate_scale' and launch.args[1] in gates:
            gop = gates[launch.args[1]]
            snaps[id(gop)] = gop.cat.buf.clone()
        launch(stream)
    plan.timer = hook
    return snaps


def disarm(plan):
    plan.timer = None


def _copy(d):
    return type(d).from_buffer_copy(d)


class Audit:
    def __init__(self, plan, model=None, pre=None, snaps=None, mode='audit', x=None, dout=None, record=True):
        assert mode in ('audit', 'dry', 'free')
        self.plan, self.mode, self.pre, self.snaps = plan, mode, pre, snaps or {}
        self.dt = 'fp32' if plan.dtype == DV_F32 else 'bf16'
        self.su = 0.0 if plan.dtype == DV_F32 else BF16_U
        self.rows = []
        self.virt = {}            # id(Act) -> BNMember whose output that activation would have been
        self.gate_dy = {}         # id(BNMember) -> GateGroupOp: dL/dy is dy g + dmean / S, formed on load
        self.dxvirt = {}          # id(ConvOp) -> (dL/d(conv output), bound) formed inside its weight gradient
        self.pending = {}         # gradient key -> [total, bound, writers seen]
        self.shadow = {}          # free mode: storage pointer -> float64 copy
        self.fidx = {}            # free mode: id(PoolOp) -> taps
        self.x, self.dout = x, dout
        self.record = record      # False: a mutant's ratios stay out of the module's table
        self.graph = PlanGraph(plan.ops, plan.host_reads)
        self.pos = {id(op): i for i, op in enumerate(plan.ops)}
        self.pname = {}
        if model is not None:
            for k, v in model.state_dict(keep_vars=True).items():
                self.pname.setdefault(id(v), k)
        if plan.comm.exchange:
            raise NotImplementedError('world > 1 exchanges are not audited')
        if plan.dtype == DV_F32 and L.f32_exact():
            raise NotImplementedError('DUALVAR_F32_EXACT: tests/test_conv_float64_gpu.py has no bound for it (NOT COVERED YET)')

    # ------------------------------------------------------------------------------------------------------ storage
    def load(self, t):
        """a flat tensor of the plan in float64: as stored (audit) / the float64 shadow (free)"""
        if self.mode == 'audit':
            return t.double()
        key = (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape))
        if key not in self.shadow:
            self.shadow[key] = t.double().clone()
        return self.shadow[key]

    def buf(self, a):
        if self.mode == 'audit':
            return a.buf
        key = _bufkey(a)
        if key not in self.shadow:
            self.shadow[key] = torch.zeros(a.buf.shape, dtype=F64)
        return self.shadow[key]

    def act(self, a, buf=None):
        b = self.buf(a) if buf is None else buf
        if b.shape[1] != a.ld:                   # (the pixel-pair view of the ingest buffer)
            b = b.reshape(-1, a.ld)
        return b[:, a.off:a.off + a.C].double().reshape(a.N, a.T, a.H, a.W, a.C)

    def rd(self, a):
        """-> (values [N,T,H,W,C] float64, bound or None): stored, or the composite expression of a BatchNorm applied on load"""
        m = self.virt.get(id(a))
        if m is None:
            return self.act(a), None
        x = self.act(m.x)
        sc, sh = self.load(m.scale)[:m.C], self.load(m.shift)[:m.C]
        y = x * sc + sh
        b = 3 * U * ((x * sc).abs() + sh.abs())              # check_apply, tests/bn_support.py
        if m.relu:
            y = y.clamp_min(0)
        if self.su:
            b = b * (1 + BF16_U) + BF16_U * y.abs()
        return y, b

    def master(self, slot, k, arena=None):
        """[Cout, kt, kh, kw, Cin] float64 of a conv slot in an fp32 arena (master weights or their gradients)"""
        st = self.plan.store
        arena = st.master if arena is None else arena
        taps = k[0] * k[1] * k[2]
        n = slot.Cout * taps * slot.cin_pitch
        return arena[slot.off:slot.off + n].view(slot.Cout, k[0], k[1], k[2], slot.cin_pitch)[..., :slot.Cin].double()

    def weights(self, slot, k):
        """the values the kernels multiply with: the master, in bf16 its stored compute copy (the cast itself is the 'cast' row)"""
        if self.mode == 'audit' and self.su:
            return self.master(slot, k, self.plan.store.cc)
        return self.master(slot, k)

    def vecp(self, t, arena=None):
        st = self.plan.store
        s = st.slot(t)
        arena = st.master if arena is None else arena
        return arena[s.off:s.off + t.numel()].double()

    def garena(self):
        st = self.plan.store
        if self.mode == 'audit':
            return st.grad
        if 'grad' not in self.shadow:
            self.shadow['grad'] = torch.zeros(st.total, dtype=F64)
        return self.shadow['grad']

    def gold(self):
        """the gradient arena before the pass"""
        if self.mode == 'free':
            return self.garena()
        if self.pre is not None and self.pre['grad'] is not None:
            return self.pre['grad']
        return torch.zeros_like(self.plan.store.grad)

    # ------------------------------------------------------------------------------------------------------ ledger
    def label(self, op):
        return '%d:%s' % (self.pos[id(op)], type(op).__name__)

    def note(self, op, qty, how, info=None):
        self.rows.append(Row(self.pos[id(op)], type(op).__name__, qty, how, None, True, info))

    def check(self, op, qty, thunk, info=None, how='direct'):
        """thunk() -> (got, ref, bound[, skip mask]); audit: compare; free: thunk stores; dry: the row only"""
        if self.mode != 'audit':
            if self.mode == 'free':
                thunk()
            self.rows.append(Row(self.pos[id(op)], type(op).__name__, qty, how, None, True, info))
            return
        out = thunk()
        got, ref, bound = out[0].double(), out[1], out[2]
        bound = torch.as_tensor(bound, dtype=F64, device=ref.device).expand_as(ref) if not torch.is_tensor(bound) or bound.shape != ref.shape \
            else bound
        err = (got - ref).abs()
        if len(out) > 3 and out[3] is not None:
            err = torch.where(out[3], torch.zeros_like(err), err)
        finite = bool(torch.isfinite(got).all())
        zero = bound == 0
        ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
        if bool((err[zero] != 0).any()):
            ratio = float('inf')
        if not finite or ratio != ratio:
            ratio = float('inf')
        key = (type(op).__name__, qty, self.dt)
        if self.record:
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        self.rows.append(Row(self.pos[id(op)], type(op).__name__, qty, how, ratio, ratio <= 1.0, info))

    def failed(self):
        return [r for r in self.rows if not r.ok]

    def worst(self):
        rs = [r.ratio for r in self.rows if r.ratio is not None]
        return max(rs) if rs else 0.0

    # ------------------------------------------------------------------------------------------------------ gradients
    def emitg(self, op, name, a, ref, bound):
        """one writer's contribution to a.grad; compared once every writer of that gradient has been seen"""
        writers = self.graph.grad_writers(a)
        key = self.graph._gkey(a)
        if self.mode == 'free':
            g = self.buf(a.grad)
            view = g[:, a.grad.off:a.grad.off + a.C]
            r2 = ref.reshape(-1, a.C)
            if op.acc.get(name):
                view += r2
            else:
                view.copy_(r2)
        if self.mode == 'dry':
            ref = bound = None
        p = self.pending.get(key)
        if p is None:
            p = self.pending[key] = [None, None, 0]
        p[2] += 1
        if self.mode == 'audit':
            own = bound + self.su * (ref.abs() + bound)      # the writer's own result, rounded to storage (bf16: the `+=` forms
            if p[0] is None:                                 # round(round(new) + old): test_conv_dgrad's accumulate case)
                p[0], p[1] = ref, own
            else:
                tot, b = p[0] + ref, p[1] + own
                p[0], p[1] = tot, b + (self.su or U) * (tot.abs() + b)
        if p[2] == len(writers):
            names = ['%s.%s' % (self.label(w), n) for w, n, _ in writers]
            tot, b = p[0], p[1]
            self.check(op, 'dx', lambda: (self.act(a.grad), tot, b), info=dict(act=key, C=a.C, writers=names))
            del self.pending[key]

    # ------------------------------------------------------------------------------------------------------ the walk
    def run(self, forward=True, backward=None):
        plan = self.plan
        backward = (plan.with_grad and plan.training) if backward is None else backward
        known = {IngestOp: (self.f_ingest, None), ConvOp: (self.f_conv, self.b_conv), BNGroupOp: (self.f_bn, self.b_bn),
                 PoolOp: (self.f_pool, self.b_pool), GateGroupOp: (self.f_gate, self.b_gate), MeanOp: (self.f_mean, self.b_mean)}
        for op in plan.ops:
            if type(op) not in known:
                raise TypeError('plan_audit does not know the op type %s' % type(op).__name__)
        self.markers()
        with torch.no_grad():
            if forward:
                if self.su and self.mode != 'free':
                    st = plan.store
                    self.check(plan.ops[0], 'cast', lambda: (st.cc, st.master.double(), BF16_U * st.master.double().abs()))
                for op in plan.ops:
                    known[type(op)][0](op)
            if backward:
                for op in reversed(plan.ops):
                    if known[type(op)][1] is not None:
                        known[type(op)][1](op)
                assert not self.pending, 'a gradient with a writer the walk never reached'
        return self

    def markers(self):
        """which quantities the plan never stores, from its own markers"""
        for op in self.plan.ops:
            if isinstance(op, ConvOp):
                if op.fp8:
                    raise NotImplementedError('fp8pw plans are not audited')
                if op.bn_fuse is not None:
                    raise NotImplementedError('FUSE_BN_REDUCE / FUSE_BN_REDUCE_TAP plans are not audited')
            for m in getattr(op, 'members', ()) if isinstance(op, BNGroupOp) else ():
                if m.reduce_fused:
                    raise NotImplementedError('FUSE_BN_REDUCE / FUSE_BN_REDUCE_TAP plans are not audited')
                if m.fused_conv is not None or m.fused_pool is not None or m.gate is not None:
                    self.virt[id(m.y)] = m
                if m.gate is not None:
                    self.gate_dy[id(m)] = m.gate[0]

    # ------------------------------------------------------------------------------------------------------ ingest
    def f_ingest(self, op):
        y, p = op.y, op.pad

        def ref():
            x = self.x if self.mode == 'free' else self.plan._keep
            r = torch.zeros(y.N, y.T, y.H, y.W, y.ld, dtype=F64, device=x.device)
            r[:, :, p:y.H - p, p:y.W - p, :3] = x.double().permute(0, 2, 3, 4, 1)
            return r.reshape(-1, y.ld)

        def thunk():
            r = ref()
            if self.mode == 'free':
                self.buf(y).copy_(r)
                return None
            return y.buf, r, self.su * r.abs()
        self.check(op, 'y', thunk)                # the whole buffer: zero border and pad lane included

    # ------------------------------------------------------------------------------------------------------ conv
    def shim(self, op):
        fwd = CT.query_fwd(_copy(op.d_in))
        dg = CT.query_dgrad(_copy(op.dgrad_desc())) if op.need_dx else None
        wg = CT.query_wgrad(_copy(op.d_w)) if self.plan.with_grad else None
        return Shim(self.plan.dtype, fwd, dg, wg)

    def conv_bound(self, sh, mode, S, cnt, ref, prop=None):
        """gauss_bound without the bf16 store's term (emitg / the caller adds the storage rounding), plus the propagated bound
        of a composite operand"""
        b = gauss_bound(sh, mode, S, cnt, ref)
        if self.su and mode != 'wgrad':
            b = (b - BF16_U * ref.abs()) / (1 + BF16_U)
        return b if prop is None else b + prop

    def f_conv(self, op):
        how = 'direct'
        info = dict(route=None)
        if self.mode == 'dry':
            self.note(op, 'y', how)
            self.note(op, 'stats', how if op.stats is not None else 'not applicable')
            return
        x, bx = self.rd(op.x)
        w = self.weights(op.slot, op.k)
        ref = ref_fwd(x, w, op.s, op.p)
        y = op.y
        if self.mode == 'free':
            self.buf(y)[:, y.off:y.off + y.C] = ref.reshape(-1, y.C)
            self.rows.append(Row(self.pos[id(op)], 'ConvOp', 'y', how, None, True, None))
            return
        sh = self.shim(op)
        info['route'] = sh.fwd.path
        xa = x.abs() if bx is None else x.abs() + bx
        S = ref_fwd(xa, w.abs(), op.s, op.p)
        cnt = ref_fwd((xa != 0).double(), (w != 0).double(), op.s, op.p)
        prop = None if bx is None else ref_fwd(bx, w.abs(), op.s, op.p)
        b = self.conv_bound(sh, 'fwd', S, cnt, ref, prop)
        b = b + self.su * (ref.abs() + b)
        self.check(op, 'y', lambda: (self.act(y), ref, b), info=info)
        if op.stats is None:
            self.note(op, 'stats', 'not applicable')
        else:
            self.stats_partials(op, sh.fwd)

    def stats_partials(self, op, route):
        """the DV_STATS partials against float64 of the values AS STORED: _stats_check, tests/test_conv_float64_gpu.py"""
        y = self.act(op.y)
        dev = y.device
        M, Co = op.y.rows, op.y.C
        rows, tiles = route.rows, route.tiles
        assert tiles * rows >= M > (tiles - 1) * rows
        yp = torch.zeros(tiles * rows, Co, dtype=F64, device=dev)
        if route.kind == 2:
            yp[:M] = y.reshape(op.y.N, op.y.T, -1, Co).permute(0, 2, 1, 3).reshape(M, Co)
        else:
            yp[:M] = y.reshape(M, Co)
        yt = yp.reshape(tiles, rows, Co)
        valid = (torch.arange(tiles * rows, device=dev) < M).reshape(tiles, rows, 1)
        nrow = valid.sum(1).double()
        s = yt.sum(1)
        mu = s / nrow
        dlt = torch.where(valid, yt - mu[:, None, :], torch.zeros_like(yt))
        m2 = (dlt ** 2).sum(1)
        amax = yt.abs().amax(1)
        if not self.su:
            bs = gamma(rows + 8) * yt.abs().sum(1)
            e = U * (mu.abs()[:, None, :] + dlt.abs()) + U * mu.abs()[:, None, :]
            bq = torch.where(valid, 2 * dlt.abs() * e + e * e + U * dlt ** 2, torch.zeros_like(yt)).sum(1) + gamma(rows + 2) * m2
        else:
            bs = gamma(rows + 8) * (yt.abs().sum(1) + rows * amax)
            bq = gamma(rows + 8) * 2 * ((yt ** 2).sum(1) + rows * amax ** 2)
        self.check(op, 'stats', lambda: (torch.cat([op.stats[0].t(), op.stats[1].t()]), torch.cat([s, m2]), torch.cat([bs, bq])))

    def b_conv(self, op):
        plan, st, sl = self.plan, self.plan.store, op.slot
        params = [self.pname.get(id(p.tensor), id(p.tensor)) for p in (sl.parts if sl.kind == 'merged' else [sl])]
        pids = [id(p.tensor) for p in (sl.parts if sl.kind == 'merged' else [sl])]
        info = dict(params=params, pids=pids)
        if self.mode == 'dry':
            self.note(op, 'dw', 'direct', info)
            if op.need_dx:
                self.emitg(op, 'x', op.x, None, None)
            return
        if op.bn_apply is not None:
            dy, bdy = self.dxvirt.pop(id(op))
        else:
            dy, bdy = self.act(op.y.grad), None
        x, bx = self.rd(op.x)
        old = self.master(sl, op.k, self.gold())
        ref = ref_wgrad(x, dy, op.k, op.s, op.p)
        if op.zero_pad_taps is not None:         # the pixel-pair stem: the 8th tap of a kernel row is structural (stem_pad_taps clears it)
            ref.view(sl.Cout, op.k[0], 7, 4, 8)[:, :, :, 3, 4:] = 0
        if self.mode == 'free':
            g = self.garena()
            n = sl.Cout * op.k[0] * op.k[1] * op.k[2] * sl.cin_pitch
            g[sl.off:sl.off + n].view(sl.Cout, op.k[0], op.k[1], op.k[2], sl.cin_pitch)[..., :sl.Cin] += ref
            self.rows.append(Row(self.pos[id(op)], 'ConvOp', 'dw', 'direct', None, True, info))
        else:
            sh = self.shim(op)
            xa = x.abs() if bx is None else x.abs() + bx
            da = dy.abs() if bdy is None else dy.abs() + bdy
            S = ref_wgrad(xa, da, op.k, op.s, op.p)
            cnt = ref_wgrad((xa != 0).double(), (da != 0).double(), op.k, op.s, op.p)
            b = self.conv_bound(sh, 'wgrad', S, cnt, ref) + U * (ref + old).abs()     # test_conv_wgrad, tests/test_conv_float64_gpu.py
            if bx is not None:
                b = b + ref_wgrad(bx, dy.abs(), op.k, op.s, op.p)
            if bdy is not None:
                b = b + ref_wgrad(xa, bdy, op.k, op.s, op.p)
            if op.zero_pad_taps is not None:
                b.view(sl.Cout, op.k[0], 7, 4, 8)[:, :, :, 3, 4:] = 0
                old = old.clone()
                old.view(sl.Cout, op.k[0], 7, 4, 8)[:, :, :, 3, 4:] = 0
            tot = ref + old
            self.check(op, 'dw', lambda: (self.master(sl, op.k, st.grad), tot, b), info=info)
        if op.need_dx:
            w = self.weights(sl, op.k)
            xd = (op.x.T, op.x.H, op.x.W)
            r = ref_dgrad(dy, w, xd, op.s, op.p)
            b = None
            if self.mode == 'audit':
                S = ref_dgrad(dy.abs(), w.abs(), xd, op.s, op.p)
                cnt = ref_dgrad((dy != 0).double(), (w != 0).double(), xd, op.s, op.p)
                b = self.conv_bound(self.shim(op), 'dgrad', S, cnt, r)
            self.emitg(op, 'x', op.x, r, b)

    # ------------------------------------------------------------------------------------------------------ BatchNorm
    def f_bn(self, op):
        plan = self.plan
        for m in op.members:
            taker = m.fused_conv or m.fused_pool or (m.gate[0] if m.gate is not None else None)
            how_y = 'direct' if taker is None else 'composite via ' + self.label(taker)
            tag = 'm%d.' % m.index
            info = dict(member=m.index)
            if self.mode == 'dry':
                for q in ('scale', 'shift'):
                    self.note(op, tag + q, 'direct', info)
                for q in ('mean', 'invstd', 'running_mean', 'running_var'):
                    self.note(op, tag + q, 'direct' if plan.training else 'not applicable', info)
                self.note(op, tag + 'y', how_y, info)
                continue
            if plan.training:
                self.bn_stats(op, m, tag, info)
            else:
                self.bn_eval(op, m, tag, info)
            if taker is not None:
                self.note(op, tag + 'y', how_y, info)
                continue
            x = self.act(m.x)
            sc, sh = self.load(m.scale)[:m.C], self.load(m.shift)[:m.C]
            res = self.act(m.res) if m.res is not None else None
            ref = x * sc + sh + (res if res is not None else 0)
            if m.relu:
                ref = ref.clamp_min(0)
            terms = (x * sc).abs() + sh.abs() + (res.abs() if res is not None else 0)
            b = 3 * U * terms                                  # check_apply, tests/bn_support.py
            if self.su:
                b = b * (1 + BF16_U) + BF16_U * ref.abs()
            snap = self.snaps.get(id(self.gate_of(m.y)))

            def thunk(m=m, ref=ref, b=b, snap=snap):
                if self.mode == 'free':
                    self.buf(m.y)[:, m.y.off:m.y.off + m.C] = ref.reshape(-1, m.C)
                    return None
                return self.act(m.y, snap), ref, b
            self.check(op, tag + 'y', thunk, info)

    def gate_of(self, a):
        """the unfused GateGroupOp that overwrites the buffer a lives in, if any"""
        for op in self.plan.ops:
            if isinstance(op, GateGroupOp) and not op.fused and _bufkey(op.cat) == _bufkey(a):
                return op
        return None

    def bn_stats(self, op, m, tag, info):
        """mean / invstd / scale / shift / running statistics from the stored partials: stats_reference and check_finalized,
        check_finalized and stats_reference, tests/bn_support.py"""
        bn, Cn, M = m.bn, m.C, m.M
        gam, bet = self.vecp(bn.weight), self.vecp(bn.bias)
        eps = float(torch.tensor(float(bn.eps), dtype=torch.float32))     # (the C ABI takes eps and momentum as fp32 numbers)
        mom = float(torch.tensor(float(bn.momentum if bn.momentum is not None else 0.1), dtype=torch.float32))
        if self.mode == 'free':
            eps = float(bn.eps)                  # (the float64 chain is compared with torch's float64 module)
            x = self.act(m.x).reshape(M, Cn)
            mean = x.mean(0)
            M2 = ((x - mean) ** 2).sum(0)
            dmean = dM2 = torch.zeros_like(mean)
        else:
            conv = m.conv
            coff = m.x.off - conv.y.off
            ps = conv.stats[0, coff:coff + Cn, :].double().t()
            pq = conv.stats[1, coff:coff + Cn, :].double().t()
            tiles, rows = conv.tiles, conv.tile_rows
            n = (M - torch.arange(tiles, device=ps.device) * rows).clamp(max=rows).double()[:, None]
            threads = 256 if len(op.members) > 1 else bn_cases.stats_threads(tiles)
            chain = stats_chain(tiles, threads)
            S = ps.sum(0)
            mean = S / M
            dS = chain * U * ps.abs().sum(0)
            a = ps / n
            d = a - mean
            M2 = (pq + n * d * d).sum(0)
            dM2 = m2_bound(n, U * a.abs(), d, pq, torch.zeros_like(pq), dS / M + U * mean.abs(), chain)
            dmean = dS / M + U * mean.abs()
        var = M2 / M
        dvar = dM2 / M + U * var
        inv = (var + eps).rsqrt()
        rel_inv = 0.5 * (dvar + U * (var + eps) + U * eps) / (var + eps) + 4 * U
        sc = gam * inv
        dsc = sc.abs() * (rel_inv + U)
        sh = bet - mean * sc
        dsh = dmean * sc.abs() + mean.abs() * dsc + U * (mean * sc).abs() + U * sh.abs()
        for q, t, r, b in (('mean', m.mean, mean, dmean * (1 + 2 * U)), ('invstd', m.invstd, inv, inv * rel_inv * (1 + 2 * U)),
                           ('scale', m.scale, sc, dsc * (1 + 2 * U)), ('shift', m.shift, sh, dsh * (1 + 2 * U))):
            def thunk(t=t, r=r, b=b):
                if self.mode == 'free':
                    self.load(t)[:Cn] = r
                    return None
                return t[:Cn], r, b
            self.check(op, tag + q, thunk, info)
        if bn.running_mean is None or self.mode == 'free':
            for q in ('running_mean', 'running_var'):
                self.note(op, tag + q, 'not applicable' if bn.running_mean is None else 'direct', info)
            return
        rm0, rv0 = (t.double() for t in self.pre['running'][id(bn)])
        unb = M2 / (M - 1) if M > 1 else var
        dunb = dM2 / max(M - 1, 1) + U * unb
        rm_ref = (1 - mom) * rm0 + mom * mean
        brm = 4 * U * ((1 - mom) * rm0.abs() + mom * mean.abs()) + mom * dmean
        if m.conv_bias is not None:              # running_mean += momentum * b, one addcmul behind the finalize: its three roundings
            cb = self.vecp(m.conv_bias)          # (dadd of test_eval_chain_against_float64, tests/test_batchnorm_single_gpu.py)
            brm = brm + 3 * U * (rm_ref.abs() + brm + (mom * cb).abs())
            rm_ref = rm_ref + mom * cb
        rv_ref = (1 - mom) * rv0 + mom * unb
        brv = 4 * U * ((1 - mom) * rv0.abs() + mom * unb.abs()) + mom * dunb
        self.check(op, tag + 'running_mean', lambda: (bn.running_mean, rm_ref, brm), info)
        self.check(op, tag + 'running_var', lambda: (bn.running_var, rv_ref, brv), info)

    def bn_eval(self, op, m, tag, info):
        """eval coefficients and the conv-bias fold: test_eval_chain_against_float64, tests/test_batchnorm_single_gpu.py"""
        bn, Cn = m.bn, m.C
        g64, b64 = self.vecp(bn.weight), self.vecp(bn.bias)
        rm, rv = bn.running_mean.double(), bn.running_var.double()
        eps = float(torch.tensor(float(bn.eps), dtype=torch.float32))
        inv = (rv + eps).rsqrt()
        rel_inv = 0.5 * (U * (rv + eps) + U * eps) / (rv + eps) + 4 * U
        sc = g64 * inv
        dsc = sc.abs() * (rel_inv + U) * (1 + 2 * U)
        sh = b64 - rm * sc
        dsh = (rm.abs() * dsc + U * (rm * sc).abs() + U * sh.abs()) * (1 + 2 * U)
        if m.conv_bias is not None:              # shift += scale * b with the STORED scale: 3 u (|shift| + |scale b|) more
            cb = self.vecp(m.conv_bias)
            sck = self.load(m.scale)[:Cn] if self.mode == 'audit' else sc
            dsh = dsh + cb.abs() * dsc + 3 * U * (sh.abs() + dsh + (sck * cb).abs())
            sh = sh + sc * cb
        for q in ('mean', 'invstd', 'running_mean', 'running_var'):
            self.note(op, tag + q, 'not applicable', info)
        for q, t, r, b in (('scale', m.scale, sc, dsc), ('shift', m.shift, sh, dsh)):
            def thunk(t=t, r=r, b=b):
                if self.mode == 'free':
                    self.load(t)[:Cn] = r
                    return None
                return t[:Cn], r, b
            self.check(op, tag + q, thunk, info)

    def b_bn(self, op):
        plan, st = self.plan, self.plan.store
        for m in reversed(op.members):
            tag = 'm%d.' % m.index
            bn, Cn, M = m.bn, m.C, m.M
            gop = self.gate_dy.get(id(m))
            ginfo = dict(member=m.index, params=[self.pname.get(id(t), id(t)) for t in (bn.weight, bn.bias)],
                         pids=[id(bn.weight), id(bn.bias)])
            how_dx = 'direct' if not m.apply_fused else 'composite via ' + self.label(m.conv)
            if m.conv_bias is not None:
                cbs = st.slot(m.conv_bias)
                self.check(op, tag + 'dconv_bias', lambda: (self.garena()[cbs.off:cbs.off + Cn], self.gold()[cbs.off:cbs.off + Cn].double(), 0.0),
                           dict(params=[self.pname.get(id(m.conv_bias))], pids=[id(m.conv_bias)]))
            if self.mode == 'dry':
                for q in ('sum_g', 'sum_gx'):
                    self.note(op, tag + q, 'direct')
                self.note(op, tag + 'mask', 'direct' if m.relu else 'not applicable')
                self.note(op, tag + 'dparams', 'direct', ginfo)
                self.rows.append(Row(self.pos[id(op)], 'BNGroupOp', tag + 'dx', how_dx, None, True, dict(act=self.graph._gkey(m.x), C=m.C)))
                if m.res is not None and m.res.grad is not None:
                    self.emitg(op, 'res%d' % m.index, m.res, None, None)
                elif m.res is None:
                    self.note(op, tag + 'dres', 'not applicable')
                continue
            x = self.act(m.x).reshape(M, Cn)
            dy = self.act(m.y.grad).reshape(M, Cn)
            bdy = torch.zeros_like(dy)
            if gop is not None:                  # dy g + dmean / S on load: gate_bwd_apply, tests/test_pool_gate_float64_gpu.py
                off, S_ = m.gate[1], gop.cat.S
                rows = torch.arange(M, device=dy.device) // S_
                t1 = dy * self.load(gop.g)[:, off:off + Cn][rows]
                t2 = self.load(gop.dmean)[:, off:off + Cn][rows] / S_
                dy = t1 + t2
                bdy = U * (2 * t1.abs() + 3 * t2.abs())
                if self.su:
                    bdy = bdy + BF16_U * (dy.abs() + bdy)
            mean, inv = self.load(m.mean)[:Cn], self.load(m.invstd)[:Cn]
            sc, sh = self.load(m.scale)[:Cn], self.load(m.shift)[:Cn]
            gam = self.vecp(bn.weight)
            und = torch.zeros_like(dy, dtype=torch.bool)
            if m.relu:
                if m.mask_from_x:
                    pre = x * sc + sh
                    und = pre.abs() <= 3 * U * ((x * sc).abs() + sh.abs())
                    mask = pre > 0
                else:
                    mask = self.act(m.y).reshape(M, Cn) > 0
                frac = float(und.double().mean())
                self.rows.append(Row(self.pos[id(op)], 'BNGroupOp', tag + 'mask', 'direct', frac / MASK_CAP, frac <= MASK_CAP, dict(undecidable=frac)))
                g = dy * mask
                bdy = bdy * mask
            else:
                self.note(op, tag + 'mask', 'not applicable')
                g = dy
            xhat = (x - mean) * inv
            sg, sgx = g.sum(0), (g * xhat).sum(0)
            ud, udx = (dy.abs() * und).sum(0), ((dy * xhat).abs() * und).sum(0)
            if self.mode == 'free':
                sgk, sgxk = sg, sgx
                self.note(op, tag + 'sum_g', 'direct')
                self.note(op, tag + 'sum_gx', 'direct')
            else:
                nblk = int(plan.lib.dv_bn_bwd_blocks(M, Cn))
                chain = bwd_reduce_chain(M, Cn, plan.dtype, nblk)
                sums = plan.zero_arena[m.sums_off:m.sums_off + 2 * m.CP].view(2, m.CP)
                # check_reduce, tests/bn_support.py
                self.check(op, tag + 'sum_g', lambda: (sums[0, :Cn], sg, chain * U * g.abs().sum(0) + bdy.sum(0) + ud))
                self.check(op, tag + 'sum_gx', lambda: (sums[1, :Cn], sgx, (chain + 3) * U * (g * xhat).abs().sum(0) + (bdy * xhat.abs()).sum(0) + udx))
                sgk, sgxk = sums[0, :Cn].double(), sums[1, :Cn].double()
            # check_bwd_apply, tests/bn_support.py, with the sums as stored
            ic = 1.0 / M
            k1 = gam * inv
            k2 = -k1 * inv * sgxk * ic
            k3 = -k1 * sgk * ic - k2 * mean
            dxr = k1 * g + k2 * x + k3
            bdx = 12 * U * ((k1 * g).abs() + (k2 * x).abs() + k3.abs() + (k2 * mean).abs()) + k1.abs() * bdy
            dxr5, bdx5, und5 = (t.reshape(m.x.N, m.x.T, m.x.H, m.x.W, Cn) for t in (dxr, bdx, und))
            if m.apply_fused:
                self.dxvirt[id(m.conv)] = (dxr5, bdx5 + (k1.abs() * dy.abs() * und).reshape(dxr5.shape))
                if self.mode == 'free':          # (the float64 chain keeps it, for the comparison with autograd)
                    self.buf(m.x.grad)[:, m.x.grad.off:m.x.grad.off + m.C] = dxr5.reshape(-1, m.C)
                self.rows.append(Row(self.pos[id(op)], 'BNGroupOp', tag + 'dx', how_dx, None, True, dict(act=self.graph._gkey(m.x), C=m.C)))
            else:
                bst = bdx5 * (1 + BF16_U) + BF16_U * dxr5.abs() if self.su else bdx5

                def thunk(m=m, dxr5=dxr5, bst=bst, und5=und5):
                    if self.mode == 'free':
                        self.buf(m.x.grad)[:, m.x.grad.off:m.x.grad.off + m.C] = dxr5.reshape(-1, m.C)
                        return None
                    return self.act(m.x.grad), dxr5, bst, und5
                self.check(op, tag + 'dx', thunk, dict(act=self.graph._gkey(m.x), C=m.C))
            gs, bs = st.slot(bn.weight), st.slot(bn.bias)
            old = self.gold()
            dg0, db0 = old[gs.off:gs.off + Cn].double(), old[bs.off:bs.off + Cn].double()

            def thunk(gs=gs, bs=bs, dg0=dg0, db0=db0, sgk=sgk, sgxk=sgxk):
                ga = self.garena()
                if self.mode == 'free':
                    ga[gs.off:gs.off + Cn] += sgxk
                    ga[bs.off:bs.off + Cn] += sgk
                    return None
                return (torch.cat([ga[gs.off:gs.off + Cn], ga[bs.off:bs.off + Cn]]), torch.cat([dg0 + sgxk, db0 + sgk]),
                        torch.cat([2 * U * (dg0.abs() + sgxk.abs()), 2 * U * (db0.abs() + sgk.abs())]))
            self.check(op, tag + 'dparams', thunk, ginfo)
            if m.res is not None and m.res.grad is not None:
                self.emitg(op, 'res%d' % m.index, m.res, g.reshape(m.x.N, m.x.T, m.x.H, m.x.W, Cn), torch.zeros_like(dxr5))
            elif m.res is None:
                self.note(op, tag + 'dres', 'not applicable')

    # ------------------------------------------------------------------------------------------------------ pool
    def pool_shim(self, op):
        x = op.x
        return PoolShim(x.N, x.T, x.H, x.W, x.C, op.k, op.s, op.p)

    def tapped(self, x, idx, op):
        """the element of x [N,T,H,W,C] each stored tap [N,To,Ho,Wo,C] points at (-inf outside the tensor)"""
        k, s, p = op.k, op.s, op.p
        xp = F.pad(x, (0, 0, p[2], p[2], p[1], p[1], p[0], p[0]), value=-float('inf'))
        do = idx.shape[1:4]
        out = torch.full(idx.shape, float('nan'), dtype=F64, device=x.device)
        for tp in range(k[0] * k[1] * k[2]):
            tap = (tp // (k[1] * k[2]), (tp // k[2]) % k[1], tp % k[2])
            sl = tuple(slice(d, d + (o - 1) * ss + 1, ss) for d, o, ss in zip(tap, do, s))
            out = torch.where(idx == tp, xp[:, sl[0], sl[1], sl[2], :], out)
        return out

    def f_pool(self, op):
        how = 'direct'
        if self.mode == 'dry':
            self.note(op, 'y', how)
            self.note(op, 'tap', how)
            return
        x, bx = self.rd(op.x)
        c = self.pool_shim(op)
        dev = x.device
        yr, tr = ref_pool_fwd(x.cpu(), c)
        yr, y = yr.to(dev), op.y
        if self.mode == 'free':
            self.buf(y)[:, y.off:y.off + y.C] = yr.reshape(-1, y.C)
            self.fidx[id(op)] = tr
            self.note(op, 'y', how)
            self.note(op, 'tap', how)
            return
        if bx is None:
            b = torch.zeros_like(yr)
        else:                                   # a max over a window moves by at most the largest bound in the window
            b = F.max_pool3d(bx.permute(0, 4, 1, 2, 3), op.k, op.s, op.p).permute(0, 2, 3, 4, 1)
        self.check(op, 'y', lambda: (self.act(y), yr, b))
        idx = op.idx[:, :y.C].reshape(yr.shape).long()
        ok = (idx >= 0) & (idx < op.k[0] * op.k[1] * op.k[2])
        at = self.tapped(x, idx.clamp(0, op.k[0] * op.k[1] * op.k[2] - 1), op)
        at = torch.where(ok, at, torch.full_like(at, -float('inf')))
        self.check(op, 'tap', lambda: (torch.where(at == yr, yr, at).nan_to_num(posinf=1e300, neginf=-1e300),
                                       yr.nan_to_num(posinf=1e300, neginf=-1e300), 2 * b))

    def b_pool(self, op):
        if not op.need_dx:
            return
        if self.mode == 'dry':
            self.emitg(op, 'x', op.x, None, None)
            return
        y, x = op.y, op.x
        gy = self.act(y.grad)
        dev = gy.device
        tap = self.fidx[id(op)] if self.mode == 'free' else op.idx[:, :y.C].reshape(gy.shape).cpu()
        c = self.pool_shim(op)
        acc, cnt, mag = ref_pool_bwd(gy.cpu(), tap, c, torch.zeros(x.N, x.T, x.H, x.W, x.C, dtype=F64))
        b = ((cnt - 1).clamp_min(0).double() * U * mag).to(dev)       # the windows' contributions are added in fp32, one rounding each
        self.emitg(op, 'x', x, acc.to(dev), b)

    # ------------------------------------------------------------------------------------------------------ gate, mean
    def mean_chain(self, N, S, Cn):
        """column_chain of dv_spatial_mean / dv_gate_bwd_reduce: run_means_and_gates, tests/test_pool_gate_float64_gpu.py"""
        dt = self.plan.dtype
        CV, chunks = cp8(Cn) // vec(dt), int(self.plan.lib.dv_spatial_chunks(dt, N, S, Cn))
        ccv = ceil_div(CV, chunks)
        return max(column_chain(S, w * vec(dt), dt, 1) for w in {ccv, CV - (chunks - 1) * ccv} if w > 0)

    def f_gate(self, op):
        cat = op.cat
        N, S, Ct = cat.N, cat.S, cat.C
        if self.mode == 'dry':
            for q in ('mean', 'g', 'y'):
                self.note(op, q, 'direct')
            return
        if op.fused:
            parts = [self.rd(m.y) for m in op.fused]
            u = torch.cat([v.reshape(N, S, -1) for v, _ in parts], 2)
            bu = torch.cat([b.reshape(N, S, -1) for _, b in parts], 2)
        else:
            u = self.act(cat, self.snaps[id(op)] if self.mode == 'audit' else None).reshape(N, S, Ct)
            bu = torch.zeros_like(u)
        Lc = self.mean_chain(N, S, Ct) if self.mode == 'audit' else 0
        mref = u.mean(1)

        def t_mean():
            if self.mode == 'free':
                self.load(op.mean).copy_(mref)
                return None
            return op.mean, mref, (Lc + 2) * U * u.abs().mean(1) + bu.mean(1)       # spatial_mean, same file :672
        self.check(op, 'mean', t_mean)
        mk = self.load(op.mean)
        gref, gb = torch.zeros_like(mref), torch.zeros_like(mref)
        for fc, off, w in op.fcs:
            W = self.master(self.plan.store.slot(fc.weight), (1, 1, 1)).reshape(w, w)
            bias = self.vecp(fc.bias)
            a = mk[:, off:off + w]
            pre = a @ W.t() + bias
            dpre = gamma(w + 1) * (a.abs() @ W.abs().t() + bias.abs())
            sg = torch.sigmoid(pre)
            gref[:, off:off + w] = sg
            gb[:, off:off + w] = sg * (e_exp(pre) * (1 - sg) + 2 * U) + dpre / 4     # check_desc_result, test_loss_gemm_optim_gpu.py
        def t_g():
            if self.mode == 'free':
                self.load(op.g).copy_(gref)
                return None
            return op.g, gref, gb
        self.check(op, 'g', t_g)
        gk = self.load(op.g)
        yref = u * gk[:, None, :]
        b = U * yref.abs() + bu * gk[:, None, :]                                    # gate_scale, same file :686
        b = b + self.su * (yref.abs() + b)

        def t_y():
            if self.mode == 'free':
                self.buf(cat)[:, cat.off:cat.off + Ct] = yref.reshape(-1, Ct)
                return None
            return self.act(cat).reshape(N, S, Ct), yref, b
        self.check(op, 'y', t_y)

    def b_gate(self, op):
        plan, st, cat = self.plan, self.plan.store, op.cat
        N, S, Ct = cat.N, cat.S, cat.C
        if not op.fused:
            raise NotImplementedError('the in-place backward of an unfused gate is not audited')
        winfo = [dict(params=[self.pname.get(id(fc.weight), id(fc.weight))], pids=[id(fc.weight)]) for fc, _, _ in op.fcs]
        binfo = dict(params=[self.pname.get(id(fc.bias), id(fc.bias)) for fc, _, _ in op.fcs], pids=[id(fc.bias) for fc, _, _ in op.fcs])
        bn_op = op.fused[0].group
        if self.mode == 'dry':
            for q in ('dpre', 'dmean'):
                self.note(op, q, 'direct')
            for k in range(len(op.fcs)):
                self.note(op, 'dW%d' % k, 'direct', winfo[k])
            self.note(op, 'db', 'direct', binfo)
            self.note(op, 'gated_grad', 'composite via ' + self.label(bn_op))
            return
        dy = self.act(cat.grad).reshape(N, S, Ct)
        out = self.act(cat).reshape(N, S, Ct)
        g, mean = self.load(op.g), self.load(op.mean)
        prod = dy * out
        Lc = self.mean_chain(N, S, Ct) if self.mode == 'audit' else 0
        dpre = prod.sum(1) * (1 - g)

        def t_dpre():
            if self.mode == 'free':
                self.load(op.dpre).copy_(dpre)
                return None
            return op.dpre, dpre, (Lc + 1 + 3) * U * prod.abs().sum(1) * (1 - g).abs()   # gate_bwd_reduce, test_pool_gate_float64_gpu.py
        self.check(op, 'dpre', t_dpre)
        dk = self.load(op.dpre)
        dm, dmb = torch.zeros_like(dk), torch.zeros_like(dk)
        old = self.gold()
        for k, (fc, off, w) in enumerate(op.fcs):
            ws = st.slot(fc.weight)
            W = self.master(ws, (1, 1, 1)).reshape(w, w)
            a = dk[:, off:off + w]
            dm[:, off:off + w] = a @ W
            dmb[:, off:off + w] = gamma(w) * (a.abs() @ W.abs())
            dW = a.t() @ mean[:, off:off + w]
            o = old[ws.off:ws.off + w * w].double().view(w, w)

            def t_dw(ws=ws, w=w, dW=dW, o=o, a=a, off=off):
                ga = self.garena()
                if self.mode == 'free':
                    ga[ws.off:ws.off + w * w].view(w, w).add_(dW)
                    return None
                return ga[ws.off:ws.off + w * w].view(w, w), o + dW, gamma(N + 1) * (o.abs() + a.abs().t() @ mean[:, off:off + w].abs())
            self.check(op, 'dW%d' % k, t_dw, winfo[k])

        def t_dmean():
            if self.mode == 'free':
                self.load(op.dmean).copy_(dm)
                return None
            return op.dmean, dm, dmb
        self.check(op, 'dmean', t_dmean)
        b0 = st.slot(op.fcs[0][0].bias)
        ob = old[b0.off:b0.off + Ct].double()

        def t_db():
            ga = self.garena()
            if self.mode == 'free':
                ga[b0.off:b0.off + Ct] += dk.sum(0)
                return None
            # test_colsum_f32, tests/test_loss_gemm_optim_gpu.py
            return ga[b0.off:b0.off + Ct], ob + dk.sum(0), (ceil_div(N, 32) + 2 + 8 + 1) * U * (ob.abs() + dk.abs().sum(0))
        self.check(op, 'db', t_db, binfo)
        self.note(op, 'gated_grad', 'composite via ' + self.label(bn_op))

    def f_mean(self, op):
        x = op.x
        if self.mode == 'dry':
            self.note(op, 'out', 'direct')
            return
        v = self.act(x).reshape(x.N, x.S, x.C)
        Lc = self.mean_chain(x.N, x.S, x.C) if self.mode == 'audit' else 0

        def thunk():
            if self.mode == 'free':
                self.load(op.out).copy_(v.mean(1))
                return None
            return op.out, v.mean(1), (Lc + 2) * U * v.abs().mean(1)
        self.check(op, 'out', thunk)

    def b_mean(self, op):
        x = op.x
        if x.grad is None:
            return
        if self.mode == 'dry':
            self.emitg(op, 'x', x, None, None)
            return
        dout = self.dout.double() if self.mode == 'free' else op.dout.double()
        t2 = (dout / x.S)[:, None, :].expand(x.N, x.S, x.C).reshape(x.N, x.T, x.H, x.W, x.C)
        self.emitg(op, 'x', x, t2, 2 * U * t2.abs())          # spatial_mean_bwd, tests/test_pool_gate_float64_gpu.py


def report():
    print('\nlargest err / bound per (op kind, quantity, dtype):')
    agg = {}
    for (kind, qty, dt), r in RATIOS.items():
        q = qty.split('.', 1)[-1] if qty[:1] == 'm' and '.' in qty else qty
        q = 'dW' if q.startswith('dW') else q
        agg[(kind, q, dt)] = max(agg.get((kind, q, dt), 0.0), r)
    for k in sorted(agg):
        print('  %-12s %-14s %-5s %.3f' % (k + (agg[k],)))
