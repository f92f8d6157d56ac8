"""Fused optimizers over the parameter arenas: SGD (pretrain.py:262-272,451: momentum 0.9, weight decay applied to
every tensor incl. BN and biases, one lr for all groups), LARS on top of it for large-batch pretraining, and Adam for finetuning.

One launch per encoder updates master weights, optimizer state and the bf16 compute copy; the classes derive from
torch.optim.Optimizer only so that torch LR schedulers (MultiStepLR, pretrain.py:328) drive `param_groups`.  What they share
-- the state arenas, their views in torch's parameter order, the state_dict format, the all-or-nothing load and the loop of
step() over the stores -- is written once, in ArenaOptimizer."""
import warnings

import torch

from . import ops


class ArenaOptimizer(torch.optim.Optimizer):
    """An optimizer whose state is one fp32 arena per name in STATE and ParamStore, laid out like the store's master arena.  A
    subclass names its state as torch.optim does (STATE), what a partial load reports (RESTORED), and launches in _step_store."""

    STATE = ()
    RESTORED = 'states'

    def __init__(self, params, defaults, stores, grad_sync):
        if stores is None:
            raise ValueError('dualvar_amd.optim.%s updates ParamStore arenas: pass stores=model.stores()' % type(self).__name__)
        super().__init__(params, defaults)
        self.stores = list(stores)
        self.grad_sync = grad_sync
        self._buf = {}

    def _arenas(self, st):
        """the state arenas of one store, [total] fp32 each (one allocation per name: ParamStore._view addresses a slot from the
        start of the tensor's storage); allocated as zeros, and anew when the store's size or device changed"""
        b = self._buf.get(id(st))
        if b is None or b[0].numel() != st.total or b[0].device != st.master.device:
            b = tuple(torch.zeros(st.total, dtype=torch.float32, device=st.master.device) for _ in self.STATE)
            self._buf[id(st)] = b
        return b

    def _views(self):
        """[(index in torch's flat parameter order, one view per name in STATE shaped like the parameter)] for every parameter
        that lives in one of the materialised arenas"""
        where = {}
        for st in self.stores:
            if st.master is None:
                continue
            arenas = self._arenas(st)
            for s in st.slots:
                where[id(s.tensor)] = tuple(st._view(a, s) for a in arenas)
        out, i = [], 0
        for g in self.param_groups:
            for p in g['params']:
                if id(p) in where:
                    out.append((i,) + where[id(p)])
                i += 1
        return out

    def zero_grad(self, set_to_none=False):
        for st in self.stores:
            st.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        hyper = self._begin_step()
        for st in self.stores:
            if st.master is None:
                continue
            scale = 1.0
            if self.grad_sync is not None:
                scale = self.grad_sync(st)
            self._step_store(st, scale, st.compute_copy(), *hyper)
            st.mark_dirty(cast_done=True)
            st.pending_backward = 0           # a forward whose result was never back-propagated must not stall the overlap

    def _launch_ranges(self, entry, st, copy, *scalars):
        """entry(p, g, state arenas..., n, scalars..., dtype, copy): one launch over the whole arena, or one per contiguous run of
        trainable tensors when part of the model is frozen (classifier.py:240-246 '--train_what last': requires_grad = False on
        the backbone -- torch's optimizers would not touch those tensors, not even with weight decay)"""
        arenas = (st.master, st.grad) + self._arenas(st)
        es = ops.ESIZE[st.dtype]
        for a, n in st.trainable_ranges():
            ops.call(entry, *[t.data_ptr() + 4 * a for t in arenas], n, *scalars, st.dtype,
                     (copy.data_ptr() + es * a) if copy is not None else None)

    def _entry_extra(self):
        """what every state_dict()['state'][i] holds besides the tensors of STATE; None: there is no state yet"""
        return {}

    def state_dict(self):
        """torch.optim's format (pretrain.py:343-349 stores it in the checkpoint; `--resume` feeds it back): param_groups with
        flat parameter indices, state[i][name] shaped like parameter i for every name in STATE."""
        groups, i = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != 'params'}
            d['params'] = list(range(i, i + len(g['params'])))
            i += len(g['params'])
            groups.append(d)
        state = {}
        if self._entry_extra() is not None:
            state = {i: dict(self._entry_extra(), **{k: v.detach().cpu().clone() for k, v in zip(self.STATE, vs)})
                     for i, *vs in self._views()}
        return {'state': state, 'param_groups': groups}

    def _check_entry(self, i, e):
        """state[i] of a state_dict being loaded -> e, or None to start parameter i at zero; a subclass may refuse it"""
        return e if all(k in e for k in self.STATE) else None

    def _check_groups(self, sd):
        if len(sd['param_groups']) != len(self.param_groups):
            raise ValueError('optimizer state has %d param_groups, this optimizer %d' % (len(sd['param_groups']), len(self.param_groups)))

    def _stage(self, sd):
        """The first half of load_state_dict: validate EVERYTHING and change nothing -- a mismatch must leave this optimizer exactly
        as it was (pretrain.py logs 'optimizer state not restored' and trains on; with a half-restored state that would be a
        different, silent run).  -> [(views of parameter i, state[i] or None)]"""
        self._check_groups(sd)
        state = sd.get('state', {})
        staged = []
        for i, *vs in self._views():
            e = state.get(i, state.get(str(i)))
            if e is not None:
                e = self._check_entry(i, e)
            if e is not None:
                for k in self.STATE:
                    if tuple(e[k].shape) != tuple(vs[0].shape):
                        raise ValueError('%s %d has shape %s, parameter has %s' % (k, i, tuple(e[k].shape), tuple(vs[0].shape)))
            staged.append((vs, e))
        return staged

    def _update_groups(self, sd):
        for g, s in zip(self.param_groups, sd['param_groups']):
            g.update({k: v for k, v in s.items() if k != 'params'})

    def _commit(self, sd, staged):
        """The second half: take the groups' values, copy what was staged, zero the rest; returns the number of parameters whose
        state was restored and warns when some are missing (a silent cold restart of the state is a different training run)."""
        self._update_groups(sd)
        restored = 0
        with torch.no_grad():
            for vs, e in staged:
                for k, v in zip(self.STATE, vs):
                    if e is None:
                        v.zero_()
                    else:
                        v.copy_(e[k].to(device=v.device, dtype=v.dtype))
                restored += e is not None
        if restored != len(staged):
            warnings.warn('optimizer state: %d of %d %s restored, the rest start at zero' % (restored, len(staged), self.RESTORED))
        return restored


class SGD(ArenaOptimizer):
    STATE = ('momentum_buffer',)
    RESTORED = 'momentum buffers'

    def __init__(self, params, lr=0.03, momentum=0.9, weight_decay=0.0, stores=None, grad_sync=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay), stores, grad_sync)

    def _momentum_buf(self, st):
        return self._arenas(st)[0]

    _momentum_views = ArenaOptimizer._views

    def _begin_step(self):
        g = self.param_groups[0]
        return float(g['lr']), float(g['momentum']), float(g['weight_decay'])

    def _step_store(self, st, scale, copy, lr, mu, wd):
        self._launch_ranges('dv_sgd_momentum', st, copy, lr, mu, wd, scale)

    def load_state_dict(self, sd):
        """Accepts torch.optim.SGD state (the reference's checkpoints), this class's own and the round-1 format (one flat
        'momentum_arenas' entry per store); returns the number of momentum buffers restored.  Stores that are not materialised
        yet are passed over."""
        if 'momentum_arenas' not in sd:
            return self._commit(sd, self._stage(sd))
        live = [st for st in self.stores if st.master is not None]
        self._check_groups(sd)
        if len(sd['momentum_arenas']) != len(live) or any(b.numel() != st.total for st, b in zip(live, sd['momentum_arenas'])):
            raise ValueError('momentum arenas do not match the parameter stores')
        self._update_groups(sd)
        for st, b in zip(live, sd['momentum_arenas']):
            self._momentum_buf(st).copy_(b)
        return len(self._views())


class _LarsTable:
    """device copies of one store's dv_lars_seg table and block map, with the partials and trust-ratio buffers"""
    __slots__ = ('key', 'segs', 'block_seg', 'n_segs', 'total_blocks', 'partials', 'q_out', 'slots', 'host')


class LARS(SGD):
    """Momentum SGD with layer-wise adaptive rate scaling over the parameter arenas, in the form of the PyTorch SimCLR / SSL
    code bases (include/dualvar_hip.h, dv_lars_step): per tensor, with d = g * scale + wd * p,
        q = eta |p| / |d|  (1 where either norm is 0);   buf = mu buf + q d;   p = p - lr buf
    -- the update norm is taken after weight decay, the ratio sits inside the momentum, lr outside (MultiStepLR acts at once), and
    the momentum buffer has SGD's meaning, so state_dict() / load_state_dict() are SGD's (torch.optim.SGD's format with
    'momentum_buffer'; the groups also carry 'eta' and 'exclude_vec').  Convolution and linear weights ('conv' slots) take the
    ratio and weight decay; BatchNorm weights / biases and linear biases ('vec' slots) take neither when exclude_vec (they are
    stepped as plain momentum SGD without weight decay), both otherwise.  Tensors that do not require gradients have no segment
    and are never touched (the MoCo key encoder, the backbone under --train_what last).
    Two launches per store and step (dv_lars_norms, dv_lars_step), no host synchronisation: the norms never leave the device.
    With grad_sync, the norms are those of the all-reduced gradient times the scale grad_sync returns -- the very values of the
    update -- so every rank forms the same q from the same bits and no further collective is needed.
    One lr, momentum, weight decay and eta for all groups, as SGD here: step() reads group 0."""

    ADAPT, DECAY = 1, 2

    def __init__(self, params, lr=0.03, momentum=0.9, weight_decay=0.0, eta=1e-3, exclude_vec=True, stores=None, grad_sync=None):
        if not eta > 0.0:
            raise ValueError('LARS eta must be > 0: %r' % (eta,))
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay, stores=stores, grad_sync=grad_sync)
        for g in self.param_groups:
            g['eta'], g['exclude_vec'] = eta, bool(exclude_vec)
        self.defaults.update(eta=eta, exclude_vec=bool(exclude_vec))
        self._tab = {}

    def segments(self, st):
        """[(slot, off, n, flags, first_block, n_blocks)] of one materialised store: one segment per slot whose tensor requires
        gradients, in arena order, n = the slot's extent rounded up to 8 elements (structural padding holds zeros in both arenas
        and adds nothing to a norm)"""
        from . import _lib as L
        from .engine import _align8
        chunk = int(L.load().dv_lars_chunk())
        exclude = bool(self.param_groups[0]['exclude_vec'])
        out, first = [], 0
        for s in st.slots:
            if not s.tensor.requires_grad:
                continue
            n = _align8(s.size)
            flags = 0 if (s.kind == 'vec' and exclude) else (self.ADAPT | self.DECAY)
            nb = (n + chunk - 1) // chunk
            out.append((s, s.off, n, flags, first, nb))
            first += nb
        return out

    def _table(self, st):
        from . import _lib as L
        key = (st.generation, tuple(bool(s.tensor.requires_grad) for s in st.slots), bool(self.param_groups[0]['exclude_vec']),
               st.master.device)
        t = self._tab.get(id(st))
        if t is not None and t.key == key:
            return t
        segs = self.segments(st)
        dev = st.master.device
        t = _LarsTable()
        t.key, t.slots, t.n_segs = key, [e[0] for e in segs], len(segs)
        t.total_blocks = sum(e[5] for e in segs)
        arr = (L.LarsSeg * max(len(segs), 1))()
        bmap = []
        for i, (_, off, n, flags, first, nb) in enumerate(segs):
            a = arr[i]
            a.off, a.n, a.flags, a.first_block, a.n_blocks = off, n, flags, first, nb
            bmap += [i] * nb
        t.host = (arr, bmap)
        t.segs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        t.block_seg = torch.tensor(bmap or [0], dtype=torch.int32).to(dev)
        t.partials = torch.zeros(2 * max(t.total_blocks, 1), dtype=torch.float32, device=dev)
        t.q_out = torch.ones(max(t.n_segs, 1), dtype=torch.float32, device=dev)
        self._tab[id(st)] = t
        return t

    def _begin_step(self):
        return super()._begin_step() + (float(self.param_groups[0]['eta']),)

    def _step_store(self, st, scale, copy, lr, mu, wd, eta):
        t = self._table(st)
        if t.n_segs:
            ops.call('dv_lars_norms', st.master, st.grad, t.segs, t.block_seg, t.n_segs, t.total_blocks, wd, scale, t.partials)
            ops.call('dv_lars_step', st.master, st.grad, self._momentum_buf(st), t.segs, t.block_seg, t.n_segs, t.total_blocks, lr, mu,
                     wd, eta, scale, t.partials, st.dtype, copy, t.q_out)

    def trust_ratios(self):
        """[(parameter name or index in torch's flat parameter order, q of the last step)] for every stepped tensor, 1.0 for the
        tensors that take no ratio.  Copies to the host (a synchronisation): for logging, never called from step()."""
        where, i = {}, 0
        for g in self.param_groups:
            names = g.get('param_names')
            for j, p in enumerate(g['params']):
                where[id(p)] = names[j] if names else i
                i += 1
        out = []
        for st in self.stores:
            if st.master is None:
                continue
            t = self._table(st)
            q = t.q_out.cpu().tolist()
            out += [(where[id(s.tensor)], q[k]) for k, s in enumerate(t.slots) if id(s.tensor) in where]
        return out


def _step_value(s):
    """state[i]['step'] of torch.optim.Adam: an int (torch 1.8, the reference's) or a 0-dim tensor (torch >= 1.12)"""
    v = float(s.item()) if torch.is_tensor(s) else float(s)
    if v < 0 or v != int(v):
        raise ValueError('Adam step %r is not a non-negative whole number' % (s,))
    return int(v)


class Adam(ArenaOptimizer):
    """Fused Adam over the parameter arenas (classifier.py:261-262 `--optim adam`: optim.Adam(params, lr, weight_decay) --
    L2 weight decay coupled into the gradient, no amsgrad).  One dv_adam launch per run of trainable tensors updates the
    master weights, both moments and the compute copy.  ONE step counter serves every tensor: all of them are stepped
    together, and tensors that do not require gradients are never touched (torch's Adam skips them, weight decay included).
    state_dict() / load_state_dict() speak torch.optim.Adam's format: state[i] = {'step', 'exp_avg', 'exp_avg_sq'} (empty before
    the first step, as torch's is).
    One lr, betas, eps and weight decay for all groups, as SGD here (the reference builds one group per tensor with the same
    values, classifier.py:242-262): step() reads group 0, and load_state_dict refuses a state whose groups disagree.
    The two moment arenas span the whole store, also when only the head trains: a slot is addressed by its arena offset."""

    STATE = ('exp_avg', 'exp_avg_sq')
    RESTORED = 'Adam moments'
    UNIFORM = ('lr', 'betas', 'eps', 'weight_decay')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, stores=None, grad_sync=None):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('Adam betas must lie in [0, 1): %r' % (betas,))
        if not eps > 0.0:
            raise ValueError('Adam eps must be > 0 (the zero padding between arena slots divides by it): %r' % (eps,))
        # the remaining keys of torch.optim.Adam's groups at their defaults, so that torch's Adam can step on our state_dict
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=False), stores, grad_sync)
        self._step = 0

    _moments = ArenaOptimizer._arenas
    _moment_views = ArenaOptimizer._views

    def _begin_step(self):
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = float(g['lr']), g['betas'], float(g['eps']), float(g['weight_decay'])
        self._step += 1
        bc1, bc2 = 1.0 - float(b1) ** self._step, 1.0 - float(b2) ** self._step       # in double, as torch forms them
        return lr, 1.0 - float(b1), float(b2), 1.0 - float(b2), eps, wd, bc1, bc2

    def _step_store(self, st, scale, copy, *hyper):
        self._launch_ranges('dv_adam', st, copy, *hyper, scale)

    def moment_summary(self):
        """(step count, L2 norm of all exp_avg, L2 norm of all exp_avg_sq) over the optimizer's parameters: what a driver logs
        after a resume"""
        views = self._moment_views()
        norms = [float(torch.sqrt(sum((x.double().pow(2).sum() for x in col), torch.zeros((), dtype=torch.float64,
                                                                                          device=col[0].device))))
                 for col in zip(*[(m, v) for _, m, v in views])] if views else [0.0, 0.0]
        return self._step, norms[0], norms[1]

    def _entry_extra(self):
        return {'step': torch.tensor(float(self._step))} if self._step > 0 else None

    def _check_entry(self, i, e):
        missing = [k for k in ('step',) + self.STATE if k not in e]
        if missing:
            raise ValueError('optimizer state %d lacks %s: not an Adam state' % (i, ', '.join(missing)))
        return e

    def load_state_dict(self, sd):
        """Accepts torch.optim.Adam state ('step' an int or a tensor) and this class's own; returns the number of parameters
        whose moments were restored and warns when some are missing.  Everything is validated before anything changes."""
        if any(st.master is None for st in self.stores):
            raise ValueError('the parameter arenas are not materialised yet (backbone.prepare(device), or one forward pass): '
                             'there is nowhere to load the moments into')
        for s in sd['param_groups']:
            for k in ('amsgrad', 'maximize', 'decoupled_weight_decay'):
                if s.get(k):
                    raise ValueError('optimizer state was saved with %s=True, which this Adam does not implement' % k)
        for k in self.UNIFORM:
            vals = {(tuple(s[k]) if k == 'betas' else s[k]) for s in sd['param_groups'] if k in s}
            if len(vals) > 1:
                raise ValueError('optimizer state has groups with different %s %s: this Adam steps every tensor with one value'
                                 % (k, sorted(vals)))
        staged = self._stage(sd)
        steps = {_step_value(e['step']) for _, e in staged if e is not None}
        if len(steps) > 1:
            raise ValueError('optimizer state holds different step counts %s: this Adam keeps one counter' % sorted(steps))
        self._step = steps.pop() if steps else 0
        restored = self._commit(sd, staged)
        for g in self.param_groups:
            g['betas'] = tuple(g['betas'])
        return restored
