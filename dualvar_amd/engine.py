"""Execution engine: flat parameter arenas + static launch plans over the HIP kernels.

A backbone is described once as a graph of ops on NDHWC activations (`Plan`); the plan owns
every buffer (activations, their gradients, BatchNorm scratch) and replays a fixed list of kernel
launches for forward and for backward.  Nothing is traced or compiled: the lists are built by
ordinary Python that mirrors the reference's module structure, and they are replayed on the
current HIP stream (so a whole step can be captured into a hipGraph).

`ParamStore` keeps the fp32 master weights of one encoder in a single arena laid out
[Cout][taps][Cin_pad] (K-contiguous, what the implicit-GEMM kernels read), with the nn.Parameters
re-pointed to strided views of it so that state_dict()/optimizers see the reference's shapes.
Gradients accumulate in a twin arena (one flat all-reduce for data parallel), bf16 compute
copies and the dgrad-layout weights are refreshed by two launches after every update.
"""
import ctypes as C
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import rccl
from . import ops
from ._lib import DV_MASK_FROM_X
from .ops import DV_ACCUM, DV_BF16, DV_BIAS, DV_F32, DV_NO_RELU_MASK, DV_RELU, DV_SIGMOID, DV_STATS, Act, cp8


BN_REPLICAS = 1       # the BN-backward sums are reduced in block order (dv_bn_bwd_reduce's ordered form): one final copy


def _align8(n):
    return (n + 7) & ~7


# weight gradients on a side stream (see Plan.run_backward); DUALVAR_WGRAD_STREAM=0 keeps everything on one stream
WGRAD_SIDE_STREAM = os.environ.get('DUALVAR_WGRAD_STREAM', '1') != '0'
# backward launches whose results only the optimizer reads: weight gradients, the gate FCs' bias gradients
SIDE_LAUNCHES = ('conv_wgrad', 'gate_db')
# side launches issued per main-stream event (the event marker costs the main stream a few microseconds each)
WGRAD_BATCH = int(os.environ.get('DUALVAR_WGRAD_BATCH', '4'))
# ... but a LARGE weight gradient (>= WGRAD_FLUSH_FLOPS) is released at once and runs beside its own layer's data gradient --
# where that pays.  Batched, the last ones of an S3D-G pass (the stem's and Conv_2c's, 0.4 - 0.6 ms each) waited for the end of the
# main chain although their operands had been ready for up to a millisecond (tools/step_timeline.py: 1.6 ms of the step ran
# nothing but those; 0.65 ms now), step 16.41 -> 16.15 ms.  It pays where the main chain has bandwidth-bound work for the weight
# gradients to run beside (BatchNorm backward, pools, gating); where the chain is as matrix-bound as they are, two such kernels
# on one GPU are slower than one after the other: R3D 26.5 -> 27.6 ms, even for its last four only.  The plan decides from its own
# composition: estimated time of the chain's non-conv launches / of its data gradients (S3D-G 1.03, r50 0.93, R(2+1)D 0.65 --
# measured gain, gain, neutral --, R3D 0.27 -- measured loss): early release at >= WGRAD_EARLY_RATIO.
WGRAD_FLUSH_FLOPS = float(os.environ.get('DUALVAR_WGRAD_FLUSH_GFLOP', '3')) * 1e9
WGRAD_EARLY_RATIO = 0.5
WGRAD_EARLY = os.environ.get('DUALVAR_WGRAD_EARLY', 'auto')        # 'auto' | '0' | '1' (A/B)
# The fusions of a BatchNorm with its neighbours, decided by Plan.finalize from the plan's PlanGraph.  (A lone BatchNorm + ReLU
# whose only reader is a max-pool -- the stems -- always runs fused with it: that one has no switch.)
# conv -> BatchNorm -> conv with a single reader: the BatchNorm-backward reduce can run in the second conv's data-gradient
# epilogue (dv_conv3d_dgrad_bn).  OFF by default -- measured on the S3D-G step (MI355X, fp32 / bf16): the reduce launches shrink
# 1.36 -> 0.66 / 1.07 -> 0.55 ms per step, but the data gradients that carry them grow by 0.62 / 0.52 ms (a serial tail per
# workgroup that re-reads its tile and the BatchNorm input), and they sit on the critical path: 20.47 -> 20.77 / 9.79 -> 9.98 ms.
FUSE_BN_REDUCE = False        # (module switch, no environment variable: tests/test_models_gpu.py monkeypatches it)
# The same fusion in its ORDERED form on the LDS-staged input-tile kernel (dv_conv3d_dgrad_bn_ws: the sums come from the
# accumulators and one read of the BatchNorm's input, tile rows are folded in tile order -- no float atomics): taken wherever the
# consuming conv's data gradient runs on that kernel (fp32 mode: the separable pairs and the strided stem conv of S3D-G / R(2+1)D).
# OFF by default since the end of round 4: while the step's tail was weight gradients waiting for the end of the main chain it was
# a wash (data gradients +0.35 ms, reduce launches -0.25 ms, step equal); with the large weight gradients released early
# (WGRAD_EARLY_RATIO) the main chain is the critical path again and the fusion costs 0.15 ms (16.23 vs 16.38 ms, three A/B pairs;
# every K threshold between 512 and 2 900 lies in between).
FUSE_BN_REDUCE_TAP = os.environ.get('DUALVAR_FUSE_BN_REDUCE_TAP', '0') != '0'      # (A/B switch; tests monkeypatch the module attribute)
# ... only behind a long K loop (>= 512 = taps x channel pitch of dY) and never for the strided stem conv: the epilogue's read of
# the BatchNorm input is exposed at the end of a workgroup's life, and for a short loop it costs more than the standalone reduce
# saves -- all eight candidates of the S3D-G step fused: data gradients +740 us, reduce launches -565 us (the stem conv alone 422 ->
# 854 us for a 312 us reduce); with this rule the step is 0.03 - 0.05 ms faster, i.e. the fusion VERDICT round 3 priced at -0.26 ms
# is worth a tenth of that.
FUSE_BN_REDUCE_TAP_MIN_K = int(os.environ.get('DUALVAR_FUSE_BN_REDUCE_TAP_MIN_K', '512'))
# BatchNorm-backward APPLY inside the weight gradient of a conv whose input needs no gradient (the first conv of a network:
# dL/d(conv output) has that weight gradient as its only reader): dv_conv3d_wgrad_bn forms it on the fly from dL/dy and the
# conv output -- one read of each instead of read + read + write (apply) + read (wgrad).  fp32 split mode only.
FUSE_BN_WGRAD = os.environ.get('DUALVAR_FUSE_BN_WGRAD', '1') != '0'      # (A/B switch; tests monkeypatch the module attribute)
# BatchNorm ON LOAD (include/dualvar_hip.h: dv_conv3d_fwd_bn_in / dv_conv3d_wgrad_bn_in): conv -> BN -> ReLU -> conv chains whose
# second conv is the only reader of the BatchNorm's output (the 1xkxk -> kx1x1 pairs of backbone/s3dg.py:30-65 and the stem): the
# output is never written; the second conv's forward and weight gradient read the BatchNorm's INPUT and apply the affine map +
# ReLU while they stage it.  Priced before it was built (apply launches skipped, stale data in the buffers): 17.09 -> 16.59 ms.
FUSE_BN_IN = os.environ.get('DUALVAR_FUSE_BN_IN', '1') != '0'         # (A/B switch; tests monkeypatch the module attribute)


# S3D-G self gating folded into the BatchNorm passes around it: the gate's mean and scale apply relu(bn(x)) of the gated members on
# load (dv_gate_mean_bn / dv_gate_scale_bn: the un-gated concat is never written), and the members' BatchNorm backward forms
# dy*g + dmean/S where it loads dy (dv_bn_bwd_*_multi_gated: the gated gradient is never written).  4 of the 14 passes over a
# level's concat buffer and 2 launches per level less, same bits (tests/test_gate_fold_gpu.py).
FUSE_GATE = os.environ.get('DUALVAR_FUSE_GATE', '1') != '0'        # (A/B switch; tests monkeypatch the module attribute)
# Two independent convs that run the same instantiation of the LDS-staged kernel or of conv_gemm_ks -- the two separable branches
# of an Inception level -- share one grid (dv_conv3d_fwd_pair / _fwd_bn_in_pair / _dgrad_pair): the small branch's launch is almost
# all latency on a third of the chip.  An emit-time pass over the finished launch lists (pair_convs); '0' gives the unpaired lists.
PAIR_CONVS = os.environ.get('DUALVAR_PAIR_CONVS', '1') != '0'      # (A/B switch; tests monkeypatch the module attribute)


class Slot:
    __slots__ = ('tensor', 'kind', 'off', 'size', 'Cout', 'Cin', 'taps', 'cin_pitch', 'cout_pitch', 'wd_off',
                 'shape', 'strides', 'parts', 'kw_store', 'w3_off', 'wd3_off')


class ParamStore:
    """Arenas for the trainable tensors of one encoder (registered in forward order)."""

    def __init__(self):
        self.slots = []
        self.merged = []           # virtual slots: several convs that share their input, stored back to back
        self._by_id = {}
        self.buffers = []          # (module, name) float buffers (BN running stats) -- left where they are
        self.nbt = []              # BN modules whose num_batches_tracked is bumped per forward
        self.master = self.grad = self.cc = self.wd = None
        self.dtype = None
        self.generation = 0
        self._dirty = True            # master changed: compute copy + dgrad layout stale
        self._cast_done = False       # ... but the bf16 copy was already refreshed by the update kernel
        self._versions = None
        self.total = 0
        self.no_dgrad = False         # key encoders (never back-propagated) skip the dgrad-layout weights
        self.pending_backward = 0     # forward passes with autograd history whose backward has not run yet (reset by the optimizer)
        self._fp8, self._fp8_ws, self._fp8_stale = {}, None, False    # fp8 copies of pointwise-conv weights (fp8_weights)

    # ---- registration (idempotent per tensor: S3D registers its stem twice)
    def _add(self, t, kind, **kw):
        if id(t) in self._by_id:
            return self._by_id[id(t)]
        s = Slot()
        s.tensor, s.kind = t, kind
        s.Cout = s.Cin = s.taps = s.cin_pitch = s.cout_pitch = 0
        s.wd_off = -1
        s.kw_store = 0
        for k, v in kw.items():
            setattr(s, k, v)
        self.slots.append(s)
        self._by_id[id(t)] = s
        return s

    def add_conv(self, weight, cin_pitch=None, need_dgrad=True, kw_store=0):
        """weight: [O, I, kt, kh, kw] or [O, I] parameter.  kw_store > kw stores each kernel row kw_store taps wide
        (the extra taps are structural zeros that the parameter view skips): the RGB stem, see Plan.conv."""
        O, I = weight.shape[:2]
        taps = 1
        for d in weight.shape[2:]:
            taps *= d
        if kw_store:
            assert weight.dim() == 5 and kw_store >= weight.shape[4] and not need_dgrad
            taps = taps // weight.shape[4] * kw_store
        return self._add(weight, 'conv', Cout=O, Cin=I, taps=taps, cin_pitch=cin_pitch or cp8(I), cout_pitch=cp8(O),
                         wd_off=0 if (need_dgrad and not self.no_dgrad) else -1, kw_store=kw_store)

    def add_merged(self, weights):
        """Several 1x1x1 convs reading the same input become ONE GEMM: their [Cout_i][Cin] blocks are registered
        back to back, so together they are a [sum Cout_i][Cin] matrix (forward / wgrad use it in place; the dgrad
        layout gets its own packed copy).  Returns the virtual slot."""
        parts = [self.add_conv(w, need_dgrad=False) for w in weights]
        key = tuple(id(w) for w in weights)
        for m in self.merged:
            if tuple(id(p.tensor) for p in m.parts) == key:
                return m
        assert all(p.taps == 1 and p.Cin == parts[0].Cin and p.Cout % 8 == 0 for p in parts)
        m = Slot()
        m.tensor, m.kind, m.parts = None, 'merged', parts
        m.Cin, m.taps, m.cin_pitch = parts[0].Cin, 1, parts[0].cin_pitch
        m.Cout = sum(p.Cout for p in parts)
        m.cout_pitch = cp8(m.Cout)
        m.wd_off = -1 if self.no_dgrad else 0
        m.off = m.size = 0
        self.merged.append(m)
        return m

    def add_vec(self, t):
        return self._add(t, 'vec')

    def add_bn(self, bn):
        self.add_vec(bn.weight)
        self.add_vec(bn.bias)
        if bn not in self.nbt:
            self.nbt.append(bn)

    def slot(self, t):
        return self._by_id[id(t)]

    # ---- materialisation
    def ready(self, device, dtype):
        if self.master is None or self.master.device != device or self.dtype != dtype:
            return False
        s0, s1 = self.slots[0], self.slots[-1]
        es = 4
        return (s0.tensor.data_ptr() == self.master.data_ptr() + s0.off * es and
                s1.tensor.data_ptr() == self.master.data_ptr() + s1.off * es)

    def _view(self, arena, s):
        if s.kind == 'vec':
            return arena.narrow(0, s.off, s.tensor.numel()).view(s.tensor.shape)
        return torch.as_strided(arena, s.shape, s.strides, s.off)

    def materialize(self, device, dtype):
        off = 0
        wd_off = 0
        for s in self.slots:
            s.off = off
            if s.kind == 'vec':
                s.size = _align8(s.tensor.numel())
            else:
                s.size = s.Cout * s.taps * s.cin_pitch
                shp = tuple(s.tensor.shape)
                rowp = s.taps * s.cin_pitch
                if len(shp) == 5:
                    kt, kh, kw = shp[2:]
                    kw = s.kw_store or kw
                    s.strides = (rowp, 1, kh * kw * s.cin_pitch, kw * s.cin_pitch, s.cin_pitch)
                else:
                    s.strides = (rowp, 1)
                s.shape = shp
                if s.wd_off >= 0:
                    s.wd_off = wd_off
                    wd_off += _align8(s.Cin * s.taps * s.cout_pitch)
            off += _align8(s.size)
        for m in self.merged:
            m.off, m.size = m.parts[0].off, sum(p.size for p in m.parts)
            for a, b in zip(m.parts, m.parts[1:]):
                assert b.off == a.off + a.size, 'merged convs must be registered back to back'
            if m.wd_off >= 0:
                m.wd_off = wd_off
                wd_off += _align8(m.Cin * m.taps * m.cout_pitch)
        self.total = off
        master = torch.zeros(off, dtype=torch.float32, device=device)
        grad = torch.zeros(off, dtype=torch.float32, device=device)
        with torch.no_grad():
            for s in self.slots:
                v = self._view(master, s)
                v.copy_(s.tensor.data.to(device=device, dtype=torch.float32))
                rg = s.tensor.requires_grad
                s.tensor.data = v
                s.tensor.grad = self._view(grad, s) if rg else None
        self.master, self.grad, self.dtype = master, grad, dtype
        self.cc = master if dtype == DV_F32 else torch.zeros(off, dtype=torch.bfloat16, device=device)
        self.wd = torch.zeros(max(wd_off, 8), dtype=ops.TORCH_DTYPE[dtype], device=device)
        self._w3_setup(device, dtype)
        # pack descriptors (device copies)
        packs = [s for s in self.slots + self.merged if s.kind in ('conv', 'merged') and s.wd_off >= 0]
        self._n_pack_blocks = 0
        if packs:
            arr = (L.PackDesc * len(packs))()
            bmap = []
            for i, s in enumerate(packs):
                a = arr[i]
                a.src_off, a.dst_off, a.Cout, a.Cin, a.taps, a.cin_pitch, a.cout_pitch = \
                    s.off, s.wd_off, s.Cout, s.Cin, s.taps, s.cin_pitch, s.cout_pitch
                bmap += [(i, c) for c in range(s.Cin)]
            self._pack_descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
            self._pack_map = torch.tensor(bmap, dtype=torch.int32).to(device)
            self._n_pack_blocks = len(bmap)
        # BN counters in one int64 arena
        if self.nbt:
            self._nbt_arena = torch.zeros(len(self.nbt), dtype=torch.long, device=device)
            for i, bn in enumerate(self.nbt):
                if bn.num_batches_tracked is not None:
                    self._nbt_arena[i] = int(bn.num_batches_tracked)
                    bn.num_batches_tracked.data = self._nbt_arena[i]
                for nm in ('running_mean', 'running_var'):
                    b = getattr(bn, nm)
                    if b.device != device:
                        b.data = b.data.to(device)
        self.generation += 1
        self._dirty = True
        self._versions = None
        self._fp8, self._fp8_stale = {}, False

    def trainable_ranges(self):
        """[(first element, count)] of the maximal runs of arena slots whose tensors require gradients (alignment
        padding between trainable neighbours is included: it is zero and stays zero)"""
        sig = tuple(bool(s.tensor.requires_grad) for s in self.slots)
        if getattr(self, '_tr_sig', None) != (sig, self.generation):
            out, start, end = [], None, 0
            for s, rg in zip(self.slots, sig):
                if rg:
                    if start is None:
                        start = s.off
                    end = s.off + _align8(s.size)
                elif start is not None:
                    out.append((start, end - start))
                    start = None
            if start is not None:
                out.append((start, end - start))
            self._tr_sig, self._tr = (sig, self.generation), out
        return self._tr

    def attach_grads(self):
        """Re-attach .grad views (e.g. after zero_grad(set_to_none=True)); zeroes the arena if any was dropped.
        Called at the start of every backward: the full walk over the (hundreds of) slots only happens when the first
        and last trainable tensors show that views were dropped (torch drops all of them together) -- walking them
        every time left the GPU idle for ~70 us per call, twice per step."""
        trainable = [s for s in (self.slots[0], self.slots[-1]) if s.tensor.requires_grad] or \
            [s for s in self.slots if s.tensor.requires_grad][:1]
        if all(s.tensor.grad is not None for s in trainable):
            return
        dropped = False
        for s in self.slots:
            if s.tensor.requires_grad and s.tensor.grad is None:
                dropped = True
                s.tensor.grad = self._view(self.grad, s)
        if dropped:
            self.grad.zero_()

    def zero_grad(self):
        # bucket all-reduces started from inside a backward whose optimizer step never ran (parallel.GradSync._on_ready): wait
        # for them and re-arm, or every later backward would be refused as "gradient accumulation" 
        if getattr(self, '_sync_started', False):
            owner = getattr(self, '_sync_owner', None)
            if owner is not None:
                owner.abandon(self)
            self._sync_started = False
        # (pending_backward is NOT reset here: the reference's loop -- and ours -- calls zero_grad() between the forward and the
        # backward of a step, pretrain.py:447-448; the optimizer step resets it)
        if self.grad is not None:
            self.grad.zero_()

    def compute_copy(self):
        """the arena a kernel that rewrites the master must also write the cast of the new values to: the compute copy, or None
        for an fp32 store (its compute copy IS the master)"""
        return self.cc if self.dtype != DV_F32 else None

    def mark_dirty(self, cast_done=False):
        self._dirty = True
        self._cast_done = cast_done

    def _version_sum(self):
        return sum(s.tensor._version for s in self.slots)

    def refresh(self, check_versions=True):
        """Bring the compute-dtype copy and the dgrad-layout weights up to date with the master."""
        if not self._dirty and check_versions:
            v = self._version_sum()
            if v != self._versions:
                self._dirty = True
        if not self._dirty:
            if self._fp8_stale:
                self._refresh_fp8()
            return
        if self.dtype == DV_BF16 and not self._cast_done:
            ops.call('dv_cast_arena', DV_BF16, self.master, self.cc, self.total)
        if self._n_pack_blocks:
            ops.call('dv_pack_dgrad_weights', self.dtype, self.master, self.wd, self._pack_descs, self._pack_map,
                     self._n_pack_blocks)
        self._refresh_w3()
        self._refresh_fp8()
        self._dirty = False
        self._cast_done = False
        self._versions = self._version_sum()

    # ---- fp32 mode: weights pre-split into three bf16 in fragment order (include/dualvar_hip.h: dv_pack_w3, DV_W3)
    def _w3_setup(self, device, dtype):
        self.w3 = self.wd3 = None
        self._w3_jobs = []
        for s_ in self.slots + self.merged:
            s_.w3_off = s_.wd3_off = -1
        if dtype != DV_F32 or L.f32_exact():
            return
        lib = L.load()
        convs = [s_ for s_ in self.slots + self.merged if s_.kind in ('conv', 'merged')]

        def table(rows_k, src_of, attr):
            arr, bmap, off = (L.W3Desc * len(rows_k))(), [], 0
            for i, (s_, rows, ktot) in enumerate(rows_k):
                setattr(s_, attr, off)
                arr[i].src_off, arr[i].dst_off, arr[i].N, arr[i].Ktot = src_of(s_), off, rows, ktot
                nbytes = int(lib.dv_w3_bytes(rows, ktot))
                bmap += [(i, u) for u in range(0, nbytes // 48, 256)]
                off += nbytes
            return (torch.zeros(max(off, 16), dtype=torch.uint8, device=device),
                    torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device),
                    torch.tensor(bmap, dtype=torch.int32).to(device), len(bmap))
        fwd = [(s_, s_.Cout, s_.taps * s_.cin_pitch) for s_ in convs]
        self.w3, d1, m1, n1 = table(fwd, lambda s_: s_.off, 'w3_off')
        self._w3_jobs.append(('master', self.w3, d1, m1, n1))
        bwd = [(s_, s_.Cin, s_.taps * s_.cout_pitch) for s_ in convs if s_.wd_off >= 0]
        if bwd:
            self.wd3, d2, m2, n2 = table(bwd, lambda s_: s_.wd_off, 'wd3_off')
            self._w3_jobs.append(('wd', self.wd3, d2, m2, n2))

    def _refresh_w3(self):
        for src, out, descs, bmap, n in getattr(self, '_w3_jobs', ()):
            base = self.master if src == 'master' else self.wd
            ops.call('dv_pack_w3', base, out, descs, bmap, n)

    def fp8_weights(self, s):
        """(w8 [Cout][CinP] e4m3, scale, wd8 [Cin][CoutP] e4m3, scale) of a 1x1x1 conv slot for the fp8 pointwise path; the
        copies are re-quantised (per-tensor amax scaling) whenever the master weights change -- see refresh()"""
        e = self._fp8.get(id(s))
        if e is None:
            dev = self.master.device
            e = (s, torch.zeros(s.Cout, s.cin_pitch, dtype=torch.uint8, device=dev), torch.ones(1, device=dev),
                 torch.zeros(s.Cin, s.cout_pitch, dtype=torch.uint8, device=dev), torch.ones(1, device=dev))
            self._fp8[id(s)] = e
            self._fp8_stale = True
        return e[1:]

    def _refresh_fp8(self):
        if not self._fp8:
            return
        lib = L.load()
        if self._fp8_ws is None:
            self._fp8_ws = torch.empty(lib.dv_quantize_fp8_workspace() // 4, dtype=torch.float32, device=self.master.device)
        es = ops.ESIZE[self.dtype]
        for s, w8, sw, wd8, swd in self._fp8.values():
            ops.call('dv_quantize_fp8', self.dtype, self.cc.data_ptr() + s.off * es, s.Cout, s.cin_pitch, s.cin_pitch, 0, w8, s.cin_pitch,
                     sw, self._fp8_ws)
            if s.wd_off >= 0:
                ops.call('dv_quantize_fp8', self.dtype, self.wd.data_ptr() + s.wd_off * es, s.Cin, s.cout_pitch, s.cout_pitch, 0, wd8,
                         s.cout_pitch, swd, self._fp8_ws)
        self._fp8_stale = False

    # pointers
    def w_fwd(self, s):
        """-> (pointer, extra conv flags): the forward-layout weights of a slot for dv_conv3d_fwd"""
        if getattr(s, 'w3_off', -1) is not None and getattr(s, 'w3_off', -1) >= 0 and self.w3 is not None:
            return self.w3.data_ptr() + s.w3_off, L.DV_W3
        return self.cc.data_ptr() + s.off * ops.ESIZE[self.dtype], 0

    def w_master(self, s):
        return self.master.data_ptr() + s.off * 4

    def w_grad(self, s):
        return self.grad.data_ptr() + s.off * 4

    def w_dgrad(self, s, strided=False):
        """-> (pointer, extra conv flags) for dv_conv3d_dgrad (the pre-split form serves stride-1 problems only)"""
        if not strided and getattr(s, 'wd3_off', -1) is not None and getattr(s, 'wd3_off', -1) >= 0 and self.wd3 is not None:
            return self.wd3.data_ptr() + s.wd3_off, L.DV_W3
        return self.wd.data_ptr() + s.wd_off * ops.ESIZE[self.dtype], 0

    # what those pointers cover, as accesses (tensor, first element, end element): Launch.reads / Launch.writes
    @staticmethod
    def _span(s):
        return s.size if s.kind != 'vec' else s.tensor.numel()

    def fwd_range(self, s):
        if getattr(s, 'w3_off', -1) is not None and getattr(s, 'w3_off', -1) >= 0 and self.w3 is not None:
            return self.w3, s.w3_off, s.w3_off + int(L.load().dv_w3_bytes(s.Cout, s.size // s.Cout))
        return self.cc, s.off, s.off + s.size

    def master_range(self, s):
        return self.master, s.off, s.off + self._span(s)

    def grad_range(self, s):
        return self.grad, s.off, s.off + self._span(s)

    def dgrad_range(self, s, w3):
        """w3: the pre-split form (the DV_W3 flag w_dgrad answered with)"""
        if w3:
            return self.wd3, s.wd3_off, s.wd3_off + int(L.load().dv_w3_bytes(s.Cin, s.taps * s.cout_pitch))
        return self.wd, s.wd_off, s.wd_off + s.Cin * s.taps * s.cout_pitch

    def bump_bn_counters(self):
        if self.nbt:
            self._nbt_arena += 1


class Comm:
    """Data-parallel context for SyncBatchNorm statistics (one process per GPU, RCCL)."""

    def __init__(self, group=None):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        # `exchange`: take the multi-rank code path.  DUALVAR_FORCE_EXCHANGE=1 takes it with ONE rank too: the only way
        # to run the RCCL calls (stream semantics, flat gather, async handles) on a single-GPU box, where two ranks
        # cannot share the device (tests/test_distributed_gpu.py::test_rccl_single_rank_rehearsal)
        self.exchange = self.world > 1 or (os.environ.get('DUALVAR_FORCE_EXCHANGE') == '1' and dist.is_available()
                                           and dist.is_initialized())
        # RCCL gathers straight into one flat tensor; gloo (the CPU / single-GPU tests) only has the list form
        self.flat_gather = self.exchange and dist.get_backend(group) == 'nccl'
        # RCCL enqueued directly on the step's own streams (dualvar_amd/rccl.py); None: torch.distributed calls
        self.rccl = rccl.get('bn', group) if self.flat_gather else None
        self._xstream = None

    def xstream(self, device):
        """the stream the backward sum exchanges run on, next to the main chain"""
        if self._xstream is None:
            self._xstream = torch.cuda.Stream(device=device)
        return self._xstream


def _all(t):
    """a whole flat buffer as an access"""
    return None if t is None else (t, 0, t.numel())


def _accesses(seq):
    return tuple(a for a in seq if a is not None)


class Launch:
    """One kernel launch of a plan: a bound C-ABI call plus its algorithmic cost (for the roofline report), and what it
    touches: `reads` / `writes` are accesses -- an ops.Act (its allocation, the channel columns [off, off + cpitch) of every
    row) or a flat range (tensor, first element, end element).  A target that is added to stands in both."""
    __slots__ = ('name', 'kname', 'fn', 'args', 'bytes', 'flops', 'shape', 'gend', 'pair', 'members', 'reads', 'writes')

    def __init__(self, name, kname, fn, args, nbytes=0, flops=0, shape='', reads=(), writes=()):
        self.name, self.kname, self.fn, self.args, self.bytes, self.flops, self.shape = name, kname, fn, args, nbytes, flops, shape
        self.reads, self.writes = _accesses(reads), _accesses(writes)
        self.gend = 0                # end (element offset) of the highest gradient-arena range this launch writes
        self.pair = None             # PairMember: this conv launch as one member of a shared grid (pair_convs), if it can be one
        self.members = ()            # the two launches a paired launch replaces

    def __call__(self, stream):
        rc = self.fn(*self.args, stream)
        if rc:
            L.check(rc, self.name)


class StreamStep:
    """A host-side step that needs the stream it is issued on (event hops around a direct RCCL call)."""
    __slots__ = ('name', 'kname', 'call', 'bytes', 'flops', 'reads', 'writes')

    def __init__(self, name, call, reads=(), writes=()):
        self.name, self.kname, self.call, self.bytes, self.flops = name, 'host:' + name, call, 0, 0
        self.reads, self.writes = _accesses(reads), _accesses(writes)

    def __call__(self, stream):
        self.call(stream)


class HostStep:
    """A host-side step inside a plan (a torch.distributed collective on the current stream)."""
    __slots__ = ('name', 'kname', 'call', 'bytes', 'flops', 'reads', 'writes')

    def __init__(self, name, call, reads=(), writes=()):
        self.name, self.kname, self.call, self.bytes, self.flops = name, 'host:' + name, call, 0, 0
        self.reads, self.writes = _accesses(reads), _accesses(writes)

    def __call__(self, stream):
        self.call()


def _conv_kname(lib, d, dgrad, dt, gv=16):
    """label of the kernel dv_conv3d_fwd / dv_conv3d_dgrad will launch for this descriptor (bench.py / profiles group by it)"""
    mode = 'DGRAD' if dgrad else 'FWD'
    tap = int(lib.dv_conv3d_tap_kind(C.byref(d), int(dgrad)))
    if tap == 3:
        return 'conv_pp<%s,%s>' % (dt, mode)         # (the pixel-pair stem form: tiles of whole output lines)
    if tap:
        return 'conv_tap<%s,%s,%s,%d,64>' % (dt, mode, 'sp' if tap == 1 else 'tm', int(lib.dv_conv3d_tap_rows(C.byref(d), int(dgrad))))
    ks = int(lib.dv_conv3d_ksplit_cols(C.byref(d), int(dgrad)))
    if ks:
        return 'conv_gemm_ks<%s,%s,64,%d>' % (dt, mode, ks)
    return 'conv_gemm<%s,%s,%d,%d,%d>' % ((dt, mode, gv) + _tile_shape(lib, d, dgrad))


def _tile_shape(lib, d, dgrad):
    """(rows, cols) of the GEMM tile the library will pick: only for the per-launch profiling labels."""
    r, c = C.c_int32(0), C.c_int32(0)
    L.check(lib.dv_conv3d_tile_shape(C.byref(d), int(dgrad), C.byref(r), C.byref(c)), 'dv_conv3d_tile_shape')
    return r.value, c.value


def _dt(dtype):
    return 'f32' if dtype == DV_F32 else 'bf16'


def _bufkey(a):
    """the allocation an activation lives in (views and channel slices of one buffer share it)"""
    return a.buf.untyped_storage().data_ptr()


class PlanGraph:
    """Who reads each activation and who writes each gradient, over a plan's ops in forward order (anything with inputs(),
    grad_targets() and an `acc` dict) and the activations the host reads: what every fusion of Plan.finalize asks.  A read of
    any channel slice counts as a read of the whole buffer (conservative); gradient writers are per (buffer, channel offset)."""

    def __init__(self, ops, host_reads=()):
        self._readers, self._writers, self._host = {}, {}, {_bufkey(a) for a in host_reads}
        for op in ops:
            for a in op.inputs():
                r = self._readers.setdefault(_bufkey(a), [])
                if op not in r:
                    r.append(op)
            for name, a in op.grad_targets():
                w = self._writers.setdefault(self._gkey(a), [])
                assert not w or w[-1][0] is not op, '%s writes one gradient twice' % type(op).__name__
                w.append((op, name, a))

    @staticmethod
    def _gkey(a):
        g = a.grad if a.grad is not None else a      # (an activation fused away has no buffer of its own: key on the gradient)
        return _bufkey(g), g.off

    def readers(self, a):
        return self._readers.get(_bufkey(a), [])

    def sole_reader(self, a):
        """the one op that reads a's buffer; None if there are several, or the host reads it too"""
        r = self.readers(a)
        return r[0] if len(r) == 1 and _bufkey(a) not in self._host else None

    def grad_writers(self, a):
        """[(op, name, activation)]: the grad_targets() that write a's gradient"""
        return self._writers.get(self._gkey(a), [])

    def set_accumulate_flags(self):
        """the last consumer (forward order) of an activation is the first writer of its gradient: the earlier ones add to it"""
        for w in self._writers.values():
            for op, name, _ in w:
                op.acc[name] = op is not w[-1][0]


class PairMember:
    """A conv forward / data-gradient launch as one member of a two-member grid: its arguments as the pair entry takes them, and
    what it reads and writes (its launch's own sets: activations, flat buffers or ranges of them) for the independence check."""
    __slots__ = ('role', 'desc', 'args', 'reads', 'writes')

    def __init__(self, role, desc, args, reads, writes):
        self.role, self.desc, self.args, self.reads = role, desc, args, reads
        self.writes = [w for w in writes if w is not None] if any(w is None for w in writes) else writes


PAIR_ENTRIES = {'fwd': ('dv_conv3d_fwd_pair', 0), 'fwd_bn_in': ('dv_conv3d_fwd_bn_in_pair', L.DV_PAIR_BN_IN0 | L.DV_PAIR_BN_IN1),
                'dgrad': ('dv_conv3d_dgrad_pair', L.DV_PAIR_DGRAD)}       # role -> (entry, dv_conv3d_pair_ok's mode)


def _storage(t):
    if isinstance(t, tuple):
        t = t[0]
    return _bufkey(t) if isinstance(t, ops.Act) else t.untyped_storage().data_ptr()


def _written(t):
    """(allocation, first, end): the channel columns of an activation's rows a conv writes / the elements of a flat buffer"""
    if isinstance(t, ops.Act):
        return _bufkey(t), t.off, t.off + t.cpitch
    if isinstance(t, tuple):
        return t[0].untyped_storage().data_ptr(), t[0].storage_offset() + t[1], t[0].storage_offset() + t[2]
    return t.untyped_storage().data_ptr(), t.storage_offset(), t.storage_offset() + t.numel()


def pair_independent(m0, m1):
    """Neither member reads an allocation the other writes into (any slice of it: conservative, as PlanGraph counts reads) and
    they write disjoint ranges -- so `=` and `+=` into one gradient, or a conv that consumes the other's output, never pair."""
    for a, b in ((m0, m1), (m1, m0)):
        if any(_storage(w) == _storage(r) for w in a.writes for r in b.reads):
            return False
    for w0 in map(_written, m0.writes):
        for w1 in map(_written, m1.writes):
            if w0[0] == w1[0] and w0[1] < w1[2] and w1[1] < w0[2]:
                return False
    return True


def pair_convs(lst, lib, side=()):
    """The emit-time pass behind PAIR_CONVS: two launches of the same kind (conv_fwd / conv_dgrad) that are next to each other
    but for launches named in `side` (the side stream's: they keep their order behind the pair), can both be members
    (Launch.pair), are independent and route to one instantiation (dv_conv3d_pair_ok) become one launch at the earlier one's
    position.  name stays; kname gets '+pair'; bytes and flops are the members' sums."""
    out, i = [], 0
    while i < len(lst):
        l0 = lst[i]
        m0 = getattr(l0, 'pair', None)
        j = i + 1
        if m0 is not None:
            while j < len(lst) and lst[j].name in side:
                j += 1
        l1 = lst[j] if j < len(lst) else None
        m1 = getattr(l1, 'pair', None)
        if (m0 is not None and m1 is not None and l1.name == l0.name and m0.role == m1.role and pair_independent(m0, m1)
                and int(lib.dv_conv3d_pair_ok(C.byref(m0.desc), C.byref(m1.desc), PAIR_ENTRIES[m0.role][1]))):
            extra = (0, 0) if m0.role == 'dgrad' else ()          # (no member carries the fused reduce: no workspace)
            p = Launch(l0.name, l0.kname + '+pair', getattr(lib, PAIR_ENTRIES[m0.role][0]), m0.args + m1.args + extra,
                       l0.bytes + l1.bytes, l0.flops + l1.flops, l0.shape + ' | ' + l1.shape)
            p.gend, p.members = max(l0.gend, l1.gend), (l0, l1)
            p.reads, p.writes = l0.reads + l1.reads, l0.writes + l1.writes
            out.append(p)
            out += lst[i + 1:j]
            i = j + 1
        else:
            out.append(l0)
            i += 1
    return out


class Plan:
    """Static forward/backward launch lists for one backbone at one input shape."""

    def __init__(self, store, dtype, device, with_grad=True, comm=None, training=True):
        self.store, self.dtype, self.device, self.with_grad = store, dtype, device, with_grad
        self.training = training     # False: eval-mode BatchNorm (running statistics), forward only
        assert training or not with_grad, 'eval-mode plans are forward only' 
        self.comm = comm if comm is not None else Comm()
        self.ops = []
        self.host_reads = []         # activations the host reads after run_forward (the caller registers them before finalize)
        self.bn_out = {}             # (buffer, channel offset) -> (BNGroupOp, BNMember) that writes there (bn_group)
        self.f_list, self.b_list = [], []
        self.bytes = 0
        self.lib = L.load()
        self.timer = None            # set by bench.py: callable(launch, stream) recording HIP events
        self._zero_words = 0         # fp32 words that must be zero at the start of every backward (atomic targets)
        self.zero_arena = None
        self._side = None            # side stream + events of run_backward
        self.wgrad_early = False     # large weight gradients leave for the side stream at once (finalize decides)
        self._events = None
        self.grad_ready = None       # callable(plan, lo): gradient-arena elements [lo, total) are final (GradSync.attach)
        self.fp8_pointwise = False   # compute mode 'fp8pw' (backbone/base.py: set_compute_dtype)
        self._fp8_ws = None
        self.bucket_starts = ()      # ... called when lo drops to / below each of these element offsets
        self._triggers = None

    # ------------------------------------------------------------------ buffers
    def act(self, N, T, H, W, C_, dtype=None, cpitch=None, grad=None, zero=False):
        dtype = self.dtype if dtype is None else dtype
        a = ops.new_act(N, T, H, W, C_, dtype, self.device, cpitch=cpitch, zero=zero)
        self.bytes += a.buf.numel() * a.buf.element_size()
        want_grad = self.with_grad if grad is None else grad
        if want_grad:
            a.grad = ops.new_act(N, T, H, W, C_, dtype, self.device, cpitch=cpitch, zero=True)
            self.bytes += a.buf.numel() * a.buf.element_size()
        return a

    def slice(self, a, off, C_):
        s = a.slice(off, C_)
        if a.grad is not None:
            s.grad = a.grad.slice(off, C_)
        return s

    def f32(self, *shape, zero=True):
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device=self.device)
        self.bytes += t.numel() * 4
        return t

    def reserve_zero(self, n):
        off = self._zero_words
        self._zero_words += (n + 7) & ~7
        return off

    def zero_ptr(self, off):
        return self.zero_arena.data_ptr() + off * 4

    # ------------------------------------------------------------------ graph ops
    def _push(self, op):
        self.ops.append(op)
        return op

    def conv(self, slot, x, k, s, p, out=None, stats=True, fp8=False):
        fp8 = bool(fp8 and getattr(self, 'fp8_pointwise', False) and self.dtype == DV_BF16 and tuple(k) == (1, 1, 1)
                   and tuple(s) == (1, 1, 1) and tuple(p) == (0, 0, 0) and slot.cin_pitch % 16 == 0 and slot.cout_pitch % 16 == 0
                   and slot.kind == 'conv' and x.cpitch == slot.cin_pitch)
        if getattr(x, 'hw_pad', 0):
            # RGB stem on the zero-bordered ingest frames (include/dualvar_hip.h, dv_ingest_ncdhw_pad): the 7x7
            # stride-2 padding-3 conv becomes a (kt,7,4)-tap stride-(st,2,1) conv over 8-channel pixel pairs
            assert k[1:] == (7, 7) and s[1:] == (2, 2) and p[1:] == (3, 3) and x.hw_pad == 3 and slot.kw_store == 8, \
                'the bordered ingest layout is for 7x7 / stride 2 / padding 3 RGB stems'
            pairs = Act(x.buf.view(-1, 8), x.N, x.T, x.H, x.W // 2, 8, 8, 0, x.dtype, 8)
            view = Slot()
            for f in Slot.__slots__:
                setattr(view, f, getattr(slot, f, None))
            view.cin_pitch, view.Cin = 8, 8
            op = self._push(ConvOp(self, view, pairs, (k[0], 7, 4), (s[0], 2, 1), (p[0], 0, 0), out, stats))
            op.alg_k = k[0] * 49 * 3                     # algorithmic K for the flop count (not the padded 224)
            op.zero_pad_taps = (slot.Cout * k[0] * 7, 32, 28, 4)    # rows, pitch, first pad column, count
            op.y.producer = op
            return op.y
        op = self._push(ConvOp(self, slot, x, k, s, p, out, stats, fp8=fp8))
        op.y.producer = op
        return op.y

    def bn_group(self, specs):
        """specs: [(bn_module, raw_conv_output, relu, residual_or_None, out_or_None), ...] of mutually independent
        layers -> their outputs.  One statistics exchange for the whole group."""
        op = self._push(BNGroupOp(self, specs))
        for m in op.members:
            self.bn_out[(_bufkey(m.y), m.y.off)] = (op, m)
        return [m.y for m in op.members]

    def bn(self, bn_mod, x, relu=True, residual=None, out=None, conv_bias=None):
        """conv_bias: the bias vector of the conv that produced x (c3d.py: Conv3d(bias=True) + BatchNorm3d).  The conv
        kernel runs bias-free: in train mode the bias cancels in the normalised output and only shifts the running mean,
        in eval mode it folds into the shift; its gradient is identically zero (weight decay still applies)."""
        ys = self.bn_group([(bn_mod, x, relu, residual, out)])
        self.ops[-1].members[0].conv_bias = conv_bias
        return ys[0]

    def maxpool(self, x, k, s, p):
        """If x turns out to be the output of a lone BatchNorm + ReLU that nothing else reads, the pair runs fused
        (finalize: _fuse_pools)."""
        return self._push(PoolOp(self, x, k, s, p)).y

    def gate_group(self, fcs, cat):
        """in-place self gating of a concat buffer: fcs = [(nn.Linear, channel offset, width), ...]"""
        self._push(GateGroupOp(self, fcs, cat))
        return cat

    def spatial_mean(self, x):
        return self._push(MeanOp(self, x)).out

    def finalize(self):
        """Decide the fusions -- each pass asks the graph who reads an activation and who writes a gradient -- then emit the
        launch lists.  The order matters: a pass sees what the ones before it took."""
        g = PlanGraph(self.ops, self.host_reads)
        self._fuse_pools(g)
        g.set_accumulate_flags()
        grad, f32 = self.with_grad and self.training, self.dtype == DV_F32
        if grad and FUSE_BN_REDUCE:
            for m, cop in self._bn_reduce_candidates(g):     # the atomic form (dv_conv3d_dgrad_bn)
                cop.take_bn_reduce(m)
        if self.training and FUSE_BN_IN and f32:
            self._fuse_bn_in(g)
        self.bn_fuse_ws = None
        if grad and FUSE_BN_REDUCE_TAP and f32 and not FUSE_BN_REDUCE:
            self._fuse_bn_reduce_tap(g)
        if grad and FUSE_BN_WGRAD and f32:
            self._fuse_bn_wgrad()
        if self.training and FUSE_GATE:
            for op in self.ops:
                if isinstance(op, GateGroupOp):
                    op.try_fuse(g)
        self._emit()

    def _bn_members(self, lone=False):
        return [m for op in self.ops if isinstance(op, BNGroupOp) and not (lone and len(op.members) > 1) for m in op.members]

    def _fuse_pools(self, g):
        """A lone BatchNorm + ReLU whose output only a max-pool reads (the stems): the pool applies it while it reads its
        windows (dv_bn_apply_maxpool / dv_bn_bwd_*_maxpool) and the output is never written -- nor kept."""
        for m in self._bn_members(lone=True):
            pool = g.sole_reader(m.y)
            if isinstance(pool, PoolOp) and pool.x is m.y and m.y.off == 0 and m.plain() and m.relu and m.conv_bias is None:
                pool.fuse_bn(m)
                self.bytes -= m.y.buf.numel() * m.y.buf.element_size()
                m.y.buf = m.y.buf.new_empty(0)

    def _bn_reduce_candidates(self, g):
        """conv -> BatchNorm(+ReLU) -> conv chains: when the second conv is the only writer of the gradient of the BatchNorm's
        output, its data gradient IS dL/dy of that BatchNorm, complete after one launch -- the BatchNorm backward's reduce
        (sum g, sum g*xhat) can run in that launch's epilogue instead of re-reading dL/dy in a pass of its own.
        -> (member, consuming ConvOp); whether that conv's data gradient can carry the reduce is the conv's to say."""
        for m in self._bn_members():
            y = m.y
            if y.grad is None or not m.plain() or m.fused_pool is not None:
                continue
            w = g.grad_writers(y)
            if len(w) != 1 or not isinstance(w[0][0], ConvOp):
                continue
            cop, _, a = w[0]
            if a.buf is not y.buf or a.off != y.off or a.C != y.C or a.rows != y.rows:
                continue
            yield m, cop

    def _fuse_bn_reduce_tap(self, g):
        """the ordered form on the LDS-staged input-tile kernel (dv_conv3d_dgrad_bn_ws)"""
        need_ws = 0
        for m, cop in self._bn_reduce_candidates(g):
            if m.x.ld * 4 * (m.x.rows - 1) < (1 << 31):
                need_ws = max(need_ws, cop.take_bn_reduce(m, ordered=True))
        if need_ws:
            # one workspace for all of them (they run one after the other on the main stream; the ticket words are zero
            # between launches, and after a failed launch: _lib.register_ticket_workspace)
            self.bn_fuse_ws = L.register_ticket_workspace(self.f32(need_ws // 4))

    def _fuse_bn_in(self, g):
        """BatchNorm on load: the conv that alone reads a BatchNorm's output applies it while it stages the BatchNorm's input"""
        for m in self._bn_members():
            y, cop = m.y, g.sole_reader(m.y)
            if not m.plain() or m.fused_pool is not None or m.conv_bias is not None or not isinstance(cop, ConvOp):
                continue
            if cop.x.buf is y.buf and cop.x.off == y.off and cop.x.C == y.C and m.x.rows == y.rows and m.x.C == y.C:
                cop.take_bn_in(m)

    def _fuse_bn_wgrad(self):
        """BatchNorm-backward apply inside the weight gradient of the producing conv, when that conv's input needs no gradient:
        the weight gradient is the only reader of dL/d(conv output) then"""
        for m in self._bn_members(lone=True):
            cop = m.conv
            if (not isinstance(cop, ConvOp) or cop.need_dx or not m.plain() or m.x.buf is not cop.y.buf or m.x.off != cop.y.off
                    or m.x.C != cop.y.C or m.x.grad is None or m.y.grad is None or m.x.ld != m.y.grad.ld):
                continue
            cop.take_bn_apply(m)

    def _emit(self):
        # scratch of the deterministic weight gradients (row-split partial tiles): ONE buffer per plan, sized for the
        # largest layer -- the plan's weight gradients all run on one stream (the side stream), each followed by its
        # reduce, so they can share it
        self.wgrad_ws = None
        if self.with_grad:
            need = max([ops.wgrad_workspace_bytes(o.d_w) for o in self.ops if isinstance(o, ConvOp)] + [0])
            if need:
                self.wgrad_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                self.bytes += need
        if self.with_grad and self._zero_words:
            self.zero_arena = self.f32(self._zero_words)
            arena = self.zero_arena
            self.b_list.append(HostStep('zero_bwd_sums', arena.zero_, writes=[_all(arena)]))
        for op in self.ops:
            f, b = op.launches()
            self.f_list += f
            op._b = b
        for op in reversed(self.ops):
            self.b_list += op._b
        self.b_list = overlap_bn_exchange(self.b_list)
        # early release of the large weight gradients: see WGRAD_EARLY_RATIO
        t_conv = sum(max(l.flops / 1.5e14, l.bytes / 4e12) for l in self.b_list if l.name == 'conv_dgrad')
        t_other = sum(l.bytes / 4e12 for l in self.b_list if l.name != 'conv_dgrad' and l.name not in SIDE_LAUNCHES)
        self.wgrad_early = (t_other >= WGRAD_EARLY_RATIO * t_conv) if WGRAD_EARLY == 'auto' else WGRAD_EARLY == '1'
        # (after the estimate above, which so sees one launch per conv as it always has)
        if PAIR_CONVS and self.dtype == DV_F32:
            self.f_list = pair_convs(self.f_list, self.lib)
            self.b_list = pair_convs(self.b_list, self.lib, SIDE_LAUNCHES)

    # ------------------------------------------------------------------ execution
    def _run(self, lst):
        s = ops.stream_ptr()
        t = self.timer
        if t is None:
            for l in lst:
                l(s)
        else:
            for l in lst:
                t(l, s)

    def run_forward(self):
        # (Independent convs of an Inception level on a second stream, forked / joined with one event each way -- 27 pairs per pass --
        # were measured again in round 4, with the LDS-staged kernels that can share a CU: 16.97 -> 17.10 ms, three A/B pairs.  The
        # event hops cost more than the overlap of two 20 - 70 us kernels gains.  Not kept.)
        self._run(self.f_list)

    def run_backward(self):
        """Weight gradients leave the critical path: a conv's wgrad needs only the finished gradient of its own
        output and a forward activation, and nothing reads its result before the optimizer -- so every conv_wgrad
        (and the stem's pad-tap clear that follows it) is issued on a SIDE stream behind an event recorded on the main
        stream at its list position, and the main stream joins the side stream at the end.  The dgrad / BatchNorm /
        pool chain of the small late layers leaves most CUs idle; the wgrads fill them."""
        if not WGRAD_SIDE_STREAM or not self.b_list:
            return self._run(self.b_list)
        trig = self._grad_triggers() if self.grad_ready is not None else {}
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
            self._events = [torch.cuda.Event() for l in self.b_list if l.name in SIDE_LAUNCHES]
        side = self._side
        sm, ss = main.cuda_stream, side.cuda_stream
        t = self.timer
        k = 0
        pending = []                 # side-stream launches waiting for the next event (one event serves WGRAD_BATCH of them)
        last_side = False

        def flush():
            nonlocal k
            if not pending:
                return
            ev = self._events[k % len(self._events)]
            k += 1
            ev.record(main)
            side.wait_event(ev)
            for q in pending:
                if t is None:
                    q(ss)
                else:
                    t(q, ss, side)
            pending.clear()
        early = self.wgrad_early
        for l in self.b_list:
            nm = l.name
            if nm in SIDE_LAUNCHES or (nm == 'stem_pad_taps' and last_side):
                pending.append(l)
                last_side = True
                if len(pending) >= WGRAD_BATCH or (early and l.flops >= WGRAD_FLUSH_FLOPS):
                    flush()
            else:
                last_side = False
                if t is None:
                    l(sm)
                else:
                    t(l, sm)
            if trig:
                lo = trig.get(id(l))
                if lo is not None:
                    flush()
                    self.grad_ready(self, lo)
        flush()
        main.wait_stream(side)

    def _grad_triggers(self):
        """{id(launch): lo}: once that launch has been issued, no later launch of the backward list writes the
        gradient arena at or above element lo -- for the bucket starts GradSync asked about (highest first)."""
        key = tuple(self.bucket_starts)
        if self._triggers is None or self._triggers[0] != key:
            trig, remaining = {}, sorted(key, reverse=True)
            frontier = 0                                   # max gend over launches AFTER position i, built backwards
            after = [0] * len(self.b_list)
            for i in range(len(self.b_list) - 1, -1, -1):
                after[i] = frontier
                frontier = max(frontier, getattr(self.b_list[i], 'gend', 0))
            for i, l in enumerate(self.b_list):
                while remaining and after[i] <= remaining[0]:
                    trig[id(l)] = remaining.pop(0)          # several buckets may become final at once: keep the lowest
            self._triggers = (key, trig)
        return self._triggers[1]

    def cost(self):
        """(algorithmic bytes, flops) of one forward+backward replay."""
        ls = self.f_list + self.b_list
        return sum(l.bytes for l in ls), sum(l.flops for l in ls)


def _gend(*slots):
    """highest gradient-arena element a launch writing these slots touches (+1)"""
    return max(s.off + (s.size if s.kind != 'vec' else s.tensor.numel()) for s in slots)


def overlap_bn_exchange(b_list):
    """Reorder a backward launch list so that every SyncBN sum exchange overlaps the weight-gradient kernels issued
    since the previous exchange: [.. wgrad_a .. wgrad_b .. reduce, START, WAIT, apply ..] becomes
    [.. reduce, START, wgrad_a, wgrad_b, WAIT, apply ..].  Safe because a weight gradient only reads a forward
    activation and the (already final) gradient of its own conv output, and nothing in a backward list writes either
    again; its own output (the fp32 gradient arena) is not read before the optimizer."""
    out, since = [], 0                       # `since`: index in `out` just after the previous WAIT
    for l in b_list:
        if l.name == 'syncbn_allreduce_start':
            moved = [x for x in out[since:] if x.name == 'conv_wgrad']
            if moved:
                out[since:] = [x for x in out[since:] if x.name != 'conv_wgrad']
            out.append(l)
            out += moved
        else:
            out.append(l)
            if l.name == 'syncbn_allreduce_wait':
                since = len(out)
    return out


class Op:
    def __init__(self, plan):
        self.plan = plan
        self.acc = {}            # per grad_targets() name: this op ADDS to that gradient (PlanGraph.set_accumulate_flags)

    def inputs(self):
        """-> the activations this op's forward reads.  No default: an op that PlanGraph cannot see would let a fusion take
        away an activation it still reads."""
        raise NotImplementedError('%s.inputs()' % type(self).__name__)

    def grad_targets(self):
        return []

    def launches(self):
        """-> (forward launches, backward launches) in execution order"""
        raise NotImplementedError


def _abytes(a, c=None):
    return a.rows * (a.C if c is None else c) * ops.ESIZE[a.dtype]


class ConvOp(Op):
    """conv (bias-free, BN partial statistics in the epilogue) with wgrad + dgrad.

    Each direction has ONE descriptor, the one its launch carries: d_in / d_w / dgrad_desc(), all built by _desc.
    A fusion of Plan.finalize asks take_bn_in / take_bn_apply / take_bn_reduce; each queries the library with the
    descriptor the launch will then carry, so what was asked and what is launched cannot part."""

    def __init__(self, plan, slot, x, k, s, p, out, stats, fp8=False):
        super().__init__(plan)
        self.slot, self.x, self.k, self.s, self.p = slot, x, k, s, p
        self.fp8 = fp8
        self.dtype = plan.dtype
        To, Ho, Wo = ops.conv_out_dims(x, k, s, p)
        self.y = out if out is not None else plan.act(x.N, To, Ho, Wo, slot.Cout)
        assert x.cpitch == slot.cin_pitch, (x.cpitch, slot.cin_pitch)
        stats = stats and plan.training              # eval-mode BatchNorm needs no batch statistics
        self._wf, wflag = plan.store.w_fwd(slot)
        self.d = self._desc(x, (DV_STATS if stats else 0) | wflag)
        self.tiles = ops.stat_tiles(self.d)
        self.tile_rows = ops.tile_rows(self.d)
        self.stats = plan.f32(2, slot.Cout, self.tiles) if stats else None
        self.need_dx = plan.with_grad and x.grad is not None and slot.wd_off >= 0
        self.alg_k = None
        self.zero_pad_taps = None
        self.bn_fuse = None          # BNMember whose backward reduce this conv's data gradient carries (Plan.finalize)
        self.bn_fuse_tap = False     # ... in the ordered form of the LDS-staged kernel (dv_conv3d_dgrad_bn_ws)
        self.bn_apply = None         # BNMember (of this conv's output) whose backward apply this conv's weight gradient carries
        self.bn_in = None            # BNMember (of this conv's INPUT) applied on load: x is never materialised (FUSE_BN_IN)
        # the descriptors the three directions launch with.  d_in, the forward's, and d_w, the weight gradient's (no flags: its
        # operands are activations), are on the input actually read: x, or the input of the BatchNorm applied on load
        # (take_bn_in); d_g, the data gradient's, is fixed by dgrad_desc()
        self.d_in, self.d_w, self.d_g, self._wd = self.d, self._desc(x, 0), None, None
        if fp8:                      # the quantised copy of x is dense: pitch = channel pitch (dv_conv3d_fwd_fp8)
            self.d_in = self._desc(x, self.d.flags)
            self.d_in.ldx = x.cpitch

    def inputs(self):
        return [self.x]

    def grad_targets(self):
        return [('x', self.x)] if self.need_dx else []

    def _desc(self, x, flags):
        """this conv on input x (self.x, or the input of a BatchNorm applied on load): the one builder of its descriptors"""
        return ops.conv_desc(self.dtype, x, self.y, self.k, self.s, self.p, flags=flags)

    def dgrad_desc(self):
        """of the data gradient, with its accumulate flag and the weight form it takes (self._wd).  Fixed at the first call:
        not before PlanGraph.set_accumulate_flags, nor before an atomic reduce is taken (take_bn_reduce)."""
        if self.d_g is None:
            st, sl, acc = self.plan.store, self.slot, DV_ACCUM if self.acc['x'] else 0
            self._wd, wdflag = st.w_dgrad(sl, strided=max(self.s) > 1)
            if max(self.s) > 1 and (self.bn_fuse is None or self.bn_fuse_tap):
                # a strided data gradient takes the pre-split weights only where every parity class of it runs on the
                # LDS-staged input-tile kernel (the 7x1x1 / stride-2 stem conv: dv_conv3d_tap_kind says so)
                wdp3, wdflag3 = st.w_dgrad(sl, strided=False)
                if wdflag3 and int(self.plan.lib.dv_conv3d_tap_kind(C.byref(self._desc(self.x, acc | wdflag3)), 1)):
                    self._wd, wdflag = wdp3, wdflag3
            self.d_g = self._desc(self.x, acc | wdflag)
            if self.fp8:             # the quantised copy of dL/dy is dense (dv_conv3d_dgrad_fp8; bf16 has no pre-split weights)
                self.d_g.ldy = self.y.cpitch
        return self.d_g

    def take_bn_in(self, m):
        """Plan.finalize: apply BatchNorm member m, whose output x is, on load in the forward and the weight gradient"""
        d = self._desc(m.x, self.d.flags)
        if not (self.fp8 or self.bn_in is not None or m.x.cpitch != self.slot.cin_pitch
                or not int(self.plan.lib.dv_conv3d_bn_in_ok(C.byref(d))) or ops.tile_rows(d) != self.tile_rows):
            self.bn_in, m.fused_conv, self.d_in, self.d_w = m, self, d, self._desc(m.x, 0)

    def take_bn_apply(self, m):
        """Plan.finalize: form the backward apply of member m, the BatchNorm of this conv's output, inside the weight gradient
        (never beside a BatchNorm on load: that weight gradient has an entry of its own)"""
        d = self.d_w
        if not (self.fp8 or self.bn_apply is not None or self.bn_in is not None or d.ldy != m.y.grad.ld
                or not self.plan.lib.dv_conv3d_wgrad_bn_ok(C.byref(d))):
            self.bn_apply, m.apply_fused = m, True

    def take_bn_reduce(self, m, ordered=False):
        """Plan.finalize: carry the backward reduce of member m, whose output x is, in the data gradient's epilogue.  ordered: in
        the form of the LDS-staged input-tile kernel only -> the bytes of workspace that takes (0: not taken).
        dv_conv3d_dgrad_bn_workspace answers 0 for DV_ACCUM (the form does not add to dx): m's sole gradient writer never
        accumulates (PlanGraph.set_accumulate_flags), and the query sees the launch's own flag."""
        if self.fp8 or self.bn_fuse is not None or (ordered and max(self.s) > 1):
            return 0
        nb = 0
        if ordered:
            d = self.dgrad_desc()
            # (not behind a short K loop: the epilogue's read of the BatchNorm input is not hidden there)
            if d.flags & L.DV_W3 and self.slot.cout_pitch * self.k[0] * self.k[1] * self.k[2] >= FUSE_BN_REDUCE_TAP_MIN_K:
                nb = int(self.plan.lib.dv_conv3d_dgrad_bn_workspace(C.byref(d)))
            if nb <= 0:
                return 0
        assert ordered or self.d_g is None      # (dgrad_desc's weight choice looks at bn_fuse)
        self.bn_fuse, self.bn_fuse_tap, m.reduce_fused = m, ordered, True
        return nb

    def launches(self):
        return self.fwd_launches(), (self.wgrad_launches() + self.dgrad_launches() if self.plan.with_grad else [])

    def _cost(self):
        """-> (algorithmic K, flops, weight bytes, gather width, shape label): the same for the three directions"""
        sl = self.slot
        kdim = self.alg_k if self.alg_k is not None else self.k[0] * self.k[1] * self.k[2] * sl.Cin
        gv = 8 if (self.dtype == DV_BF16 and sl.cin_pitch % 8) else 16
        shp = 'M%d Cin%d Cout%d k%s s%s' % (self.y.rows, sl.Cin, sl.Cout, 'x'.join(map(str, self.k)), 'x'.join(map(str, self.s)))
        return kdim, 2 * self.y.rows * sl.Cout * kdim, sl.Cout * kdim * ops.ESIZE[self.dtype], gv, shp

    def _quantize(self, a, fmt, shp):
        """-> (dense fp8 copy of activation a, its scale, the launch that fills them): in front of an fp8 conv (mode 'fp8pw')"""
        p = self.plan
        if p._fp8_ws is None:
            p._fp8_ws = p.f32(p.lib.dv_quantize_fp8_workspace() // 4)
        q, sc = torch.empty(a.rows, a.cpitch, dtype=torch.uint8, device=p.device), p.f32(1)
        p.bytes += q.numel()
        return q, sc, Launch('quantize_fp8', 'quantize_fp8<%s>' % ('e5m2' if fmt else 'e4m3'), p.lib.dv_quantize_fp8,
                             (DV_BF16, a.ptr, a.rows, a.cpitch, a.ld, fmt, q.data_ptr(), a.cpitch, sc.data_ptr(), p._fp8_ws.data_ptr()),
                             2 * _abytes(a) + q.numel(), 0, shp, reads=[a, _all(p._fp8_ws)], writes=[_all(q), _all(sc), _all(p._fp8_ws)])

    def fwd_launches(self):
        """plain / with the BatchNorm of the input applied on load / fp8 behind the quantisation of x"""
        lib, x, y, d = self.plan.lib, self.x, self.y, self.d_in
        _, flops, wbytes, gv, shp = self._cost()
        stats = self.stats.data_ptr() if self.stats is not None else 0
        wr = [y, _all(self.stats)]
        if self.fp8:
            w8, sw, _, _ = self.plan.store.fp8_weights(self.slot)
            self.x8, self.sx, ql = self._quantize(x, 0, shp)
            return [ql, Launch('conv_fwd', 'conv_gemm<fp8,FWD,16,%d,%d>' % _tile_shape(lib, d, 0), lib.dv_conv3d_fwd_fp8,
                               (C.byref(d), self.x8.data_ptr(), w8.data_ptr(), self.sx.data_ptr(), sw.data_ptr(), y.ptr, stats),
                               self.x8.numel() + wbytes // 2 + _abytes(y), flops, shp,
                               reads=[_all(self.x8), _all(w8), _all(self.sx), _all(sw)], writes=wr)]
        kf, nbytes = _conv_kname(lib, d, 0, _dt(self.dtype), gv), _abytes(x) + wbytes + _abytes(y)
        w = self.plan.store.fwd_range(self.slot)
        if self.bn_in is not None:
            m = self.bn_in
            args = (C.byref(d), m.x.ptr, C.byref(ops.bn_in_desc(m.scale, m.shift, m.relu)), self._wf, y.ptr, stats)
            l = Launch('conv_fwd', kf + '+bn_in', lib.dv_conv3d_fwd_bn_in, args, nbytes, flops, shp + ' +bn_in',
                       reads=[m.x, _all(m.scale), _all(m.shift), w], writes=wr)
            l.pair = PairMember('fwd_bn_in', d, args, l.reads, l.writes)
        else:
            l = Launch('conv_fwd', kf, lib.dv_conv3d_fwd, (C.byref(d), x.ptr, self._wf, 0, y.ptr, stats), nbytes, flops, shp,
                       reads=[x, w], writes=wr)
            l.pair = PairMember('fwd', d, (C.byref(d), x.ptr, self._wf, y.ptr, stats), l.reads, l.writes)
        return [l]

    def wgrad_launches(self):
        """plain / forming the backward apply of the output's BatchNorm / on load; then the stem's pad-tap clear"""
        p, st, lib, sl, x, y, d = self.plan, self.plan.store, self.plan.lib, self.slot, self.x, self.y, self.d_w
        kdim, flops, _, gv, shp = self._cost()
        tr, tc, tsp = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(lib.dv_conv3d_wgrad_tile(C.byref(d), C.byref(tr), C.byref(tc), C.byref(tsp)), 'dv_conv3d_wgrad_tile')
        kw = 'conv_wgrad<%s,%d,%d,%d>' % (_dt(self.dtype), gv, tr.value, tc.value)
        ws = (p.wgrad_ws.data_ptr(), p.wgrad_ws.numel()) if p.wgrad_ws is not None else (0, 0)
        dw, nbytes, gend = st.w_grad(sl), _abytes(x) + _abytes(y) + sl.Cout * kdim * 4, sl.off + sl.size
        # dw += x^T dy through the shared partial-tile scratch: the target is read and written
        tgt, wsa = (st.grad, sl.off, sl.off + sl.size), _all(p.wgrad_ws)
        if self.bn_apply is not None:
            m = self.bn_apply
            gs, bs = st.slot(m.bn.weight), st.slot(m.bn.bias)
            r = L.BnBwd()
            r.x, r.ldx = y.ptr, y.ld
            r.mean, r.invstd, r.scale, r.shift = (t.data_ptr() for t in (m.mean, m.invstd, m.scale, m.shift))
            r.gamma, r.dgamma, r.dbeta = st.w_master(gs), st.w_grad(gs), st.w_grad(bs)
            r.sums, r.n_rep, r.flags = p.zero_ptr(m.sums_off), BN_REPLICAS, (0 if m.relu else DV_NO_RELU_MASK)
            r.inv_count, r.dparam_scale = 1.0 / (m.M * p.comm.world), 1.0 / p.comm.world
            dpar = [st.grad_range(gs), st.grad_range(bs)]
            b = [Launch('conv_wgrad', kw + '+bn_bwd_apply', lib.dv_conv3d_wgrad_bn, (C.byref(d), x.ptr, m.y.grad.ptr, dw) + ws + (C.byref(r),),
                        nbytes + _abytes(y), flops, shp + ' +bn_bwd_apply',
                        reads=[x, m.y.grad, y, _all(m.mean), _all(m.invstd), _all(m.scale), _all(m.shift), st.master_range(gs),
                               (p.zero_arena, m.sums_off, m.sums_off + m.sums_len), tgt, wsa] + dpar, writes=[tgt, wsa] + dpar)]
            b[0].gend = _gend(gs, bs)    # (it writes the BatchNorm's parameter gradients too)
        elif self.bn_in is not None:
            m = self.bn_in
            b = [Launch('conv_wgrad', kw + '+bn_in', lib.dv_conv3d_wgrad_bn_in,
                        (C.byref(d), m.x.ptr, C.byref(ops.bn_in_desc(m.scale, m.shift, m.relu)), y.grad.ptr, dw) + ws,
                        nbytes, flops, shp + ' +bn_in', reads=[m.x, _all(m.scale), _all(m.shift), y.grad, tgt, wsa], writes=[tgt, wsa])]
        else:
            b = [Launch('conv_wgrad', kw, lib.dv_conv3d_wgrad, (C.byref(d), x.ptr, y.grad.ptr, dw) + ws, nbytes, flops, shp,
                        reads=[x, y.grad, tgt, wsa], writes=[tgt, wsa])]
        if self.zero_pad_taps is not None:
            rows, pitch, c0, nc = self.zero_pad_taps
            b.append(Launch('stem_pad_taps', 'fill_cols', lib.dv_fill_cols_f32, (dw, rows, pitch, c0, nc, 0.0), reads=[tgt], writes=[tgt]))
        for l in b:
            l.gend = max(l.gend, gend)
        return b

    def dgrad_launches(self):
        """plain / with a BatchNorm-backward reduce in the epilogue, atomic or ordered / fp8 behind the quantisation of dL/dy"""
        if not self.need_dx:
            return []
        p, lib, x, y, d = self.plan, self.plan.lib, self.x, self.y, self.dgrad_desc()
        _, flops, wbytes, _, shp = self._cost()
        dxbytes = _abytes(x) * (2 if d.flags & DV_ACCUM or self.bn_fuse is not None else 1)      # (the reduce re-reads its tile)
        acc = [x.grad] if d.flags & DV_ACCUM else []
        if self.fp8:
            _, _, wd8, swd = p.store.fp8_weights(self.slot)
            self.dy8, self.sdy, ql = self._quantize(y.grad, 1, shp)
            return [ql, Launch('conv_dgrad', 'conv_gemm<fp8,DGRAD,16,%d,%d>' % _tile_shape(lib, d, 1), lib.dv_conv3d_dgrad_fp8,
                               (C.byref(d), self.dy8.data_ptr(), wd8.data_ptr(), self.sdy.data_ptr(), swd.data_ptr(), x.grad.ptr),
                               self.dy8.numel() + wbytes // 2 + dxbytes, flops, shp,
                               reads=[_all(self.dy8), _all(wd8), _all(self.sdy), _all(swd)] + acc, writes=[x.grad])]
        kd, args = _conv_kname(lib, d, 1, _dt(self.dtype)), (C.byref(d), y.grad.ptr, self._wd, x.grad.ptr)
        nbytes = _abytes(y) + wbytes + dxbytes
        rd = [y.grad, p.store.dgrad_range(self.slot, d.flags & L.DV_W3)] + acc
        if self.bn_fuse is None:
            l = Launch('conv_dgrad', kd, lib.dv_conv3d_dgrad, args, nbytes, flops, shp, reads=rd, writes=[x.grad])
            l.pair = PairMember('dgrad', d, args + (0,), l.reads, l.writes)
            return [l]
        m = self.bn_fuse
        r = ops.bn_reduce_desc(m.x, m.mean, m.invstd, m.scale, m.shift, p.zero_ptr(m.sums_off), BN_REPLICAS,
                               0 if m.relu else DV_NO_RELU_MASK)
        sums = (p.zero_arena, m.sums_off, m.sums_off + m.sums_len)       # (added to: read and written)
        rd += [m.x, _all(m.mean), _all(m.invstd), _all(m.scale), _all(m.shift), sums]
        if self.bn_fuse_tap:
            ws = p.bn_fuse_ws
            return [Launch('conv_dgrad', kd + '+bn_reduce', lib.dv_conv3d_dgrad_bn_ws, args + (C.byref(r), ws.data_ptr(), ws.numel() * 4),
                           nbytes, flops, shp + ' +bn_reduce', reads=rd + [_all(ws)], writes=[x.grad, sums, _all(ws)])]
        return [Launch('conv_dgrad', kd, lib.dv_conv3d_dgrad_bn, args + (C.byref(r),), nbytes, flops, shp + ' +bn_reduce',
                       reads=rd, writes=[x.grad, sums])]


BN_PHASES = ('stats', 'apply', 'red', 'bapply')     # forward statistics and apply, backward reduce and apply: dv_bn_item's blk_*


class BNMember:
    """One BatchNorm of a BNGroupOp: its state, and the ONE description of it every launch is derived from -- item() holds each
    pointer, flag and constant, fused() / blocks() / nbytes() say per phase who runs it, on how many blocks, over how many bytes."""

    def __init__(self, plan, bn, x, relu, residual, out):
        self.plan, self.bn, self.x, self.relu, self.res, self.conv = plan, bn, x, relu, residual, x.producer
        self.C, self.M = x.C, x.rows
        self.CP = cp8(self.C)
        self.y = out if out is not None else plan.act(x.N, x.T, x.H, x.W, x.C)
        # per-channel arrays are read with 16-byte loads: padded to CP
        self.mean, self.invstd, self.scale, self.shift = (plan.f32(self.CP) for _ in range(4))
        self.width = 2 * self.C + 1
        # y = relu(x*scale + shift) with nothing added: the backward recomputes the ReLU mask from x (which it reads for
        # xhat anyway) with the forward's expression and never touches y -- 5 tensor passes per BatchNorm instead of 7
        self.conv_bias = None        # Plan.bn(conv_bias=...)
        self.fused_pool = None       # the PoolOp that consumes y on the fly (Plan.finalize: y's only reader)
        self.fused_conv = None       # the ConvOp that applies this BatchNorm while it stages x (Plan.finalize, FUSE_BN_IN)
        self.reduce_fused = False    # the backward reduce runs in the epilogue of the consuming conv's data gradient
        self.apply_fused = False     # the backward apply runs inside the producing conv's weight gradient (dv_conv3d_wgrad_bn)
        self.gate = None             # (GateGroupOp, column offset): the gate applies this BatchNorm on load (FUSE_GATE)
        self.mask_from_x = bool(relu) and residual is None
        self.sums_off = plan.reserve_zero(BN_REPLICAS * 2 * self.CP) if plan.with_grad else 0
        self.sums_len = BN_REPLICAS * 2 * self.CP
        # per-block partial sums + ticket of the ordered backward reduce (zero once: the kernel leaves the ticket zero)
        self.red_ws = (L.register_ticket_workspace(plan.f32(int(plan.lib.dv_bn_bwd_reduce_workspace(self.M, self.C)) // 4))
                       if plan.with_grad else None)
        self.group, self.index, self.loff = None, 0, 0      # BNGroupOp: the group, the place in it, the offset in its statistics
        self._item = None

    def plain(self):
        """y = act(x*scale + shift) with nothing added: whoever holds x can form y itself, and the backward takes the ReLU mask
        from x.  What every fusion of Plan.finalize asks first; each adds its own conditions."""
        return self.res is None and (self.mask_from_x or not self.relu)

    def item(self):
        """This member as a dv_bn_item, filled once when the plan emits its launches (the accumulate flags are set by then).  The
        blk_* prefixes stay zero: they belong to the table an item is copied into (BNGroupOp._table)."""
        if self._item is not None:
            return self._item
        p, st, bn, x, y, res, conv = self.plan, self.plan.store, self.bn, self.x, self.y, self.res, self.conv
        it = self._item = L.BnItem()
        gs, bs = st.slot(bn.weight), st.slot(bn.bias)
        it.gamma, it.beta = st.w_master(gs), st.w_master(bs)
        it.running_mean, it.running_var = (t.data_ptr() if t is not None else 0 for t in (bn.running_mean, bn.running_var))
        it.mean, it.invstd, it.scale, it.shift = (t.data_ptr() for t in (self.mean, self.invstd, self.scale, self.shift))
        it.x, it.ldx, it.y, it.ldy = x.ptr, x.ld, y.ptr, y.ld
        it.residual, it.ldr = (res.ptr, res.ld) if res is not None else (0, 0)
        it.M, it.C, it.fwd_flags = self.M, self.C, DV_RELU if self.relu else 0
        it.eps, it.momentum = float(bn.eps), float(bn.momentum if bn.momentum is not None else 0.1)
        if p.training:   # x may be a channel slice of a merged conv's output: columns [coff, coff+C) of a wider [2][Cout][tiles] table
            it.partials = conv.stats.data_ptr() + 4 * (x.off - conv.y.off) * conv.tiles
            it.n_tiles, it.tile_rows, it.pitch = conv.tiles, conv.tile_rows, conv.slot.Cout
            it.local_stats = self.group.local.data_ptr() + 4 * self.loff
        if p.training and p.with_grad:
            R = p.comm.world
            dres = res.grad if (res is not None and res.grad is not None) else None
            it.dy, it.lddy, it.dx, it.lddx = y.grad.ptr, y.grad.ld, x.grad.ptr, x.grad.ld
            it.dres, it.lddres = (dres.ptr, dres.ld) if dres is not None else (0, 0)
            it.sums, it.n_rep, it.red_ws = p.zero_ptr(self.sums_off), BN_REPLICAS, self.red_ws.data_ptr()
            it.dgamma, it.dbeta = st.w_grad(gs), st.w_grad(bs)
            it.inv_count, it.dparam_scale = 1.0 / (self.M * R), 1.0 / R
            it.bwd_flags = ((0 if self.relu else DV_NO_RELU_MASK) | (DV_MASK_FROM_X if self.mask_from_x else 0)
                            | (DV_ACCUM if (dres is not None and self.group.acc.get('res%d' % self.index)) else 0))
        return it

    def touched(self):
        """{field of dv_bn_item: the access behind that pointer}, for the pointers item() sets.  A launch that takes a table of
        items declares every one of them a read (the table points there) and, of these, the ones its phase writes (written())."""
        p, st, x, y, res = self.plan, self.plan.store, self.x, self.y, self.res
        gs, bs = st.slot(self.bn.weight), st.slot(self.bn.bias)
        t = dict(gamma=st.master_range(gs), beta=st.master_range(bs), running_mean=_all(self.bn.running_mean),
                 running_var=_all(self.bn.running_var), mean=_all(self.mean), invstd=_all(self.invstd), scale=_all(self.scale),
                 shift=_all(self.shift), x=x, residual=res, y=y if y.buf.numel() else None)
        if p.training:
            t.update(partials=_all(self.conv.stats), local_stats=(self.group.local, self.loff, self.loff + self.width))
        if p.training and p.with_grad:
            t.update(dy=y.grad, dx=x.grad, dres=res.grad if res is not None else None, red_ws=_all(self.red_ws),
                     sums=(p.zero_arena, self.sums_off, self.sums_off + self.sums_len),
                     dgamma=st.grad_range(gs), dbeta=st.grad_range(bs))
        return {k: v for k, v in t.items() if v is not None}

    PHASE_WRITES = {'stats': ('local_stats',), 'finalize': ('running_mean', 'running_var', 'mean', 'invstd', 'scale', 'shift'),
                    'apply': ('y',), 'red': ('sums', 'red_ws'), 'bapply': ('dgamma', 'dbeta', 'dx', 'dres')}

    def written(self, *phases):
        """the accesses of touched() that the launches of `phases` write for this member (none where a fusion runs the phase)"""
        t = self.touched()
        return [t[f] for ph in phases if not (ph in BN_PHASES and self.fused(ph)) for f in self.PHASE_WRITES[ph] if f in t]

    def fused(self, phase):
        """a fusion of Plan.finalize runs `phase` of this member in place of the group's own launch (the apply: on load in the
        consuming conv, in the gate or in the max-pool)"""
        return {'stats': False, 'apply': not (self.fused_conv is None and self.gate is None and self.fused_pool is None),
                'red': self.reduce_fused, 'bapply': self.apply_fused}[phase]

    def blocks(self, phase):
        """blocks of this member in the group's launch of `phase` (the contract of dv_bn_item's blk_*, include/dualvar_hip.h);
        none where a fusion runs the phase"""
        if self.fused(phase):
            return 0
        if phase == 'stats':
            return self.C
        if phase == 'red':
            return int(self.plan.lib.dv_bn_bwd_blocks(self.M, self.C))
        total = self.M * (self.CP // (4 if self.plan.dtype == DV_F32 else 8))
        return max(1, min(4096 if phase == 'apply' else 2048, (total + 255) // 256))

    def nbytes(self, phase):
        """algorithmic bytes of `phase` where the group runs it"""
        if self.fused(phase):
            return 0
        if phase == 'stats':
            return self.conv.tiles * 2 * self.C * 4
        if phase == 'apply':
            return _abytes(self.x) * (3 if self.res is not None else 2)
        it = self.item()
        nact = 3 if (self.relu and not self.mask_from_x) else 2      # dy, x (and y for a mask that x does not give)
        nres = 0 if not it.dres else (2 if it.bwd_flags & DV_ACCUM else 1)
        return _abytes(self.x) * (nact if phase == 'red' else nact + 1 + nres)


def _bn_apply_launch(m):
    """y = act(x*scale + shift (+res)) of one member, in training and in eval mode"""
    p, it = m.plan, m.item()
    return Launch('bn_apply', 'bn_apply<%s>' % _dt(p.dtype), p.lib.dv_bn_apply,
                  (p.dtype, it.x, it.ldx, it.scale, it.shift, it.residual, it.ldr, it.y, it.ldy, it.M, it.C, it.fwd_flags),
                  m.nbytes('apply'), 0, 'M%d C%d' % (m.M, m.C), reads=[m.x, _all(m.scale), _all(m.shift), m.res], writes=[m.y])


class BNGroupOp(Op):
    """Training-mode BatchNorm (+residual) (+ReLU) for one or several independent layers.

    With world > 1 the members' statistics travel in ONE all-gather forward and ONE all-reduce backward
    (SyncBatchNorm, torch/nn/modules/_functions.py:39-200): the four branch-entry BNs of an Inception block cost
    one small collective instead of four."""

    def __init__(self, plan, specs):
        super().__init__(plan)
        self.members = [BNMember(plan, *sp) for sp in specs]
        self.width = sum(m.width for m in self.members)
        self.local = plan.f32(self.width)
        self.gathered = plan.f32(plan.comm.world, self.width) if plan.comm.exchange else self.local
        off = 0
        for i, m in enumerate(self.members):
            m.group, m.index, m.loff = self, i, off
            off += m.width

    def inputs(self):
        return [t for m in self.members for t in (m.x, m.res) if t is not None]

    def grad_targets(self):
        if not self.plan.with_grad:
            return []
        return [('res%d' % i, m.res) for i, m in enumerate(self.members) if m.res is not None and m.res.grad is not None]

    def _table(self):
        """the members' items on the device, each with the running block count of every phase up to and including itself
        -> (pointer, {phase: blocks of the whole group})"""
        p = self.plan
        arr = (L.BnItem * len(self.members))(*[m.item() for m in self.members])
        ends = dict.fromkeys(BN_PHASES, 0)
        for it, m in zip(arr, self.members):
            for ph in BN_PHASES if p.with_grad else BN_PHASES[:2]:
                ends[ph] += m.blocks(ph)
                setattr(it, 'blk_' + ph, ends[ph])
        self._items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(p.device)
        p.bytes += self._items.numel()
        return self._items.data_ptr(), ends

    def _eval_launches(self):
        """module.eval(): y = act(x * scale + shift (+res)) with the affine map of the RUNNING statistics; no
        exchange, no update, no backward"""
        st, lib = self.plan.store, self.plan.lib
        f = []
        for m in self.members:
            it = m.item()
            if m.bn.running_mean is None:
                raise NotImplementedError('eval-mode BatchNorm without running statistics')
            t = m.touched()
            f.append(Launch('bn_eval_coeffs', 'bn_eval_coeffs', lib.dv_bn_eval_coeffs,
                            (it.gamma, it.beta, it.running_mean, it.running_var, it.eps, it.C, it.scale, it.shift),
                            reads=[t[k] for k in ('gamma', 'beta', 'running_mean', 'running_var')], writes=[t['scale'], t['shift']]))
            if m.conv_bias is not None:          # y = scale*(conv + b) + shift
                f.append(Launch('bn_bias_shift', 'addcmul', lib.dv_addcmul_f32,
                                (it.shift, it.scale, st.w_master(st.slot(m.conv_bias)), 1.0, it.C),
                                reads=[t['shift'], t['scale'], st.master_range(st.slot(m.conv_bias))], writes=[t['shift']]))
            if not m.fused('apply'):             # (else: the pool op applies it while it reads its windows)
                f.append(_bn_apply_launch(m))
        return f, []

    def _exchange(self):
        """-> (forward, backward) steps that exchange the group's statistics between the ranks: the all-gather of `local` into
        `gathered` between the statistics and their finalize, the all-reduce of the replica sums between the backward reduce
        and apply"""
        p, R = self.plan, self.plan.comm.world
        f, b = [], []
        local, gathered, group = self.local, self.gathered, p.comm.group
        rc = p.comm.rccl
        if rc is not None:       # in-stream: ordered with the reduce kernels before and the finalize after, no hop
            f.append(Launch('syncbn_allgather', 'rccl:all_gather', rc.all_gather,
                            (local.data_ptr(), gathered.data_ptr(), self.width), 4 * self.width * (R + 1),
                            reads=[_all(local)], writes=[_all(gathered)]))
        elif p.comm.flat_gather:
            f.append(HostStep('syncbn_allgather', lambda: dist.all_gather_into_tensor(gathered, local, group=group),
                              reads=[_all(local)], writes=[_all(gathered)]))
        else:
            f.append(HostStep('syncbn_allgather', lambda: dist.all_gather(list(gathered.unbind(0)), local, group=group),
                              reads=[_all(local)], writes=[_all(gathered)]))
        if p.with_grad:
            first, last = self.members[0], self.members[-1]
            lo, n = first.sums_off, last.sums_off + last.sums_len - first.sums_off
            pending = []
            inplace = dict(reads=[(p.zero_arena, lo, lo + n)], writes=[(p.zero_arena, lo, lo + n)])      # the all-reduce's, on its start step

            # In place on the (contiguous) replica accumulators of the group, asynchronously: Plan.finalize moves
            # the weight-gradient kernels of the layers above between `start` and `wait`, so the exchange latency
            # (the dominant multi-GPU cost of this path) hides behind work that does not need it.
            def _start():
                pending.append(dist.all_reduce(p.zero_arena.narrow(0, lo, n), group=group, async_op=True))

            def _wait():
                pending.pop().wait()
            if rc is not None and os.environ.get('DUALVAR_BN_BWD_ASYNC') != '1':
                # in-stream between the group's reduce and apply kernels.  Measured (one rank, every collective issued):
                # the two event hops of the overlapped form cost ~24 us per exchange, more than a small RCCL
                # all-reduce inside a node takes -- step 11.71 ms overlapped vs 10.95 ms in-stream (10.74 without exchange)
                b.append(Launch('syncbn_allreduce', 'rccl:all_reduce', lambda stream: rc.all_reduce(p.zero_ptr(lo), n, stream), (),
                                8 * n, **inplace))
            elif rc is not None:
                # same overlap with RCCL called directly: main --event--> exchange stream: all-reduce --event--> main
                ev_a, ev_b = torch.cuda.Event(), torch.cuda.Event()
                dev = p.device

                def _start_direct(stream):
                    xs = p.comm.xstream(dev)
                    ev_a.record(torch.cuda.current_stream(dev))
                    xs.wait_event(ev_a)
                    L.check(rc.all_reduce(p.zero_ptr(lo), n, xs.cuda_stream), 'ncclAllReduce')
                    ev_b.record(xs)

                def _wait_direct(stream):
                    torch.cuda.current_stream(dev).wait_event(ev_b)
                b.append(StreamStep('syncbn_allreduce_start', _start_direct, **inplace))
                b.append(StreamStep('syncbn_allreduce_wait', _wait_direct))
            else:
                b.append(HostStep('syncbn_allreduce_start', _start, **inplace))
                b.append(HostStep('syncbn_allreduce_wait', _wait))
        return f, b

    def launches(self):
        p, st, lib, ms = self.plan, self.plan.store, self.plan.lib, self.members
        if not p.training:
            return self._eval_launches()
        R, dt, n, exchange = p.comm.world, _dt(p.dtype), len(ms), p.comm.exchange
        # The form of each direction, decided here: the forward of two or more members is one multi-tensor launch per phase (the
        # layers are small and latency bound), a lone (large) layer keeps the single-tensor kernels (1024-thread stats); the
        # backward is multi-tensor for a lone member too when it takes the ReLU mask from x (the form that carries scale / shift).
        fwd_multi = n > 1
        bwd_multi = p.with_grad and (n > 1 or ms[0].mask_from_x)
        tab, ends = self._table() if (fwd_multi or bwd_multi) else (0, None)
        m, it = ms[0], ms[0].item()          # (the single-tensor forms: the lone member)
        shape = 'M%d C%d' % (m.M, m.C)
        stats_in = (it.partials, it.n_tiles, it.tile_rows, it.pitch, it.M, it.C, it.local_stats)
        finalize = (it.gamma, it.beta, it.eps, it.momentum, it.running_mean, it.running_var, it.mean, it.invstd, it.scale, it.shift)
        bwd_in = (p.dtype, it.dy, it.lddy, it.y, it.ldy, it.x, it.ldx, it.mean, it.invstd)
        xf, xb = self._exchange() if exchange else ([], [])
        nb = {ph: sum(m.nbytes(ph) for m in ms) for ph in (BN_PHASES if p.with_grad else BN_PHASES[:2])}      # bytes per phase
        # every launch of the group reads what the members' items point at (and the table of them); it writes its phases' part
        rd = [a for m_ in ms for a in m_.touched().values()] + ([_all(self._items)] if tab else [])

        def wr(*phases):
            return [a for m_ in ms for a in m_.written(*phases)]

        # forward: statistics -> exchange -> finalize -> conv bias -> apply
        if fwd_multi:
            f = [Launch('bn_stats_multi', 'bn_stats_multi', lib.dv_bn_stats_multi, (tab, n, 0 if exchange else 1, ends['stats']),
                        nb['stats'], reads=rd, writes=wr('stats') if exchange else wr('stats', 'finalize'))]
        elif exchange:
            f = [Launch('bn_reduce_stats', 'bn_reduce_stats', lib.dv_bn_reduce_stats, stats_in, nb['stats'], reads=rd, writes=wr('stats'))]
        else:
            f = [Launch('bn_stats_finalize', 'bn_reduce_stats', lib.dv_bn_stats_finalize, stats_in + finalize, nb['stats'],
                        reads=rd, writes=wr('stats', 'finalize'))]
        f += xf
        if exchange and fwd_multi:       # ONE finalize launch for the group after the all-gather (instead of one per member)
            f.append(Launch('bn_finalize_multi', 'bn_finalize_multi', lib.dv_bn_finalize_multi,
                            (tab, n, sum((m.C + 127) // 128 for m in ms), self.local.data_ptr(), self.gathered.data_ptr(), R,
                             self.width), reads=rd + [_all(self.local), _all(self.gathered)], writes=wr('finalize')))
        elif exchange:
            f.append(Launch('bn_finalize', 'bn_finalize', lib.dv_bn_finalize,
                            (self.gathered.data_ptr() + 4 * m.loff, R, self.width, it.C) + finalize,
                            reads=rd + [_all(self.gathered)], writes=wr('finalize')))
        if any(m.conv_bias is not None and m.bn.running_mean is not None for m in ms):
            assert n == 1                # conv bias in front of the BN: only the running mean sees it
            f.append(Launch('bn_bias_running_mean', 'addcmul', lib.dv_addcmul_f32,
                            (it.running_mean, st.w_master(st.slot(m.conv_bias)), 0, it.momentum, it.C),
                            reads=[_all(m.bn.running_mean), st.master_range(st.slot(m.conv_bias))], writes=[_all(m.bn.running_mean)]))
        if fwd_multi and ends['apply']:
            f.append(Launch('bn_apply_multi', 'bn_apply_multi<%s>' % dt, lib.dv_bn_apply_multi, (p.dtype, tab, n, ends['apply']),
                            nb['apply'], reads=rd, writes=wr('apply')))
        elif not fwd_multi and not m.fused('apply'):
            f.append(_bn_apply_launch(m))
        if not p.with_grad:
            return f, []

        # backward: reduce -> exchange -> apply; a phase that a fusion runs for every member is not launched
        b_red, b_app = [], []
        gated = [m for m in ms if m.gate is not None]
        if bwd_multi:
            red_fn, app_fn, suffix, gargs, gbytes = lib.dv_bn_bwd_reduce_multi, lib.dv_bn_bwd_apply_multi, '', (), 0
            if gated:
                # the `+gate` instantiations take dL/dy of the gated members as dy*g + dmean/S on load (the other members of
                # the launch run as before); they also read the members' columns of the two [N][Ct] tables
                gop = gated[0].gate[0]
                assert all(m.gate[0] is gop and not m.reduce_fused and not m.apply_fused for m in gated)
                self._gate_off = torch.tensor([m.gate[1] if m.gate is not None else -1 for m in ms], dtype=torch.int32).to(p.device)
                p.bytes += self._gate_off.numel() * 4
                red_fn, app_fn, suffix = lib.dv_bn_bwd_reduce_multi_gated, lib.dv_bn_bwd_apply_multi_gated, '+gate'
                gargs = (gop.g.data_ptr(), gop.dmean.data_ptr(), gop.cat.S, gop.cat.C, self._gate_off.data_ptr())
                gbytes = sum(8 * gop.cat.N * m.C for m in gated)
                rd = rd + [_all(gop.g), _all(gop.dmean), _all(self._gate_off)]
            if ends['red'] or gated:
                b_red.append(Launch('bn_bwd_reduce_multi', 'bn_bwd_reduce_multi<%s>%s' % (dt, suffix), red_fn,
                                    (p.dtype, tab, n, ends['red']) + gargs, nb['red'] + gbytes,
                                    reads=rd, writes=wr('red')))
            if ends['bapply'] or gated:
                b_app.append(Launch('bn_bwd_apply_multi', 'bn_bwd_apply_multi<%s>%s' % (dt, suffix), app_fn,
                                    (p.dtype, tab, n, ends['bapply'], max(m.C for m in ms)) + gargs, nb['bapply'] + gbytes,
                                    reads=rd, writes=wr('bapply')))
        else:
            if not m.fused('red'):       # (the reduce writes no dres: without DV_ACCUM)
                b_red.append(Launch('bn_bwd_reduce', 'bn_bwd_reduce<%s>' % dt, lib.dv_bn_bwd_reduce,
                                    bwd_in + (it.M, it.C, it.bwd_flags & ~DV_ACCUM, it.sums, it.n_rep, it.red_ws),
                                    nb['red'], 0, shape, reads=rd, writes=wr('red')))
            if not m.fused('bapply'):
                b_app.append(Launch('bn_bwd_apply', 'bn_bwd_apply<%s>' % dt, lib.dv_bn_bwd_apply,
                                    bwd_in + (it.gamma, it.sums, it.n_rep, it.inv_count, it.dparam_scale, it.dgamma, it.dbeta, it.dx,
                                              it.lddx, it.dres, it.lddres, it.M, it.C, it.bwd_flags), nb['bapply'], 0, shape,
                                    reads=rd, writes=wr('bapply')))
        for l in b_app:
            l.gend = _gend(*[st.slot(t) for m in ms for t in (m.bn.weight, m.bn.bias)])
        return f, b_red + xb + b_app


class PoolOp(Op):
    def __init__(self, plan, x, k, s, p):
        super().__init__(plan)
        self.bn_member = None        # the lone BatchNorm + ReLU applied while the windows are read (fuse_bn)
        self.x, self.k, self.s, self.p = x, k, s, p
        To, Ho, Wo = ops.conv_out_dims(x, k, s, p)
        self.y = plan.act(x.N, To, Ho, Wo, x.C)
        self.idx = torch.empty(self.y.rows, cp8(x.C), dtype=torch.uint8, device=plan.device)
        plan.bytes += self.idx.numel()
        self.d = ops.pool_desc(plan.dtype, x, self.y, k, s, p)
        self.need_dx = plan.with_grad and x.grad is not None

    def fuse_bn(self, m):
        """forward fused with the BatchNorm + ReLU that produces x: the windows are read from the conv output and normalised
        on the fly, x itself is never written (its gradient still is: the BatchNorm backward reads it)"""
        self.bn_member, m.fused_pool = m, self
        self.d_fused = ops.pool_desc(self.plan.dtype, m.x, self.y, self.k, self.s, self.p)

    def inputs(self):
        return [self.x]

    def grad_targets(self):
        return [('x', self.x)] if self.need_dx else []

    def launches(self):
        p, lib, x, y = self.plan, self.plan.lib, self.x, self.y
        dt = _dt(p.dtype)
        if self.bn_member is not None:
            m = self.bn_member
            f = [Launch('bn_apply_maxpool', 'bn_apply_maxpool<%s>' % dt, lib.dv_bn_apply_maxpool,
                        (C.byref(self.d_fused), m.x.ptr, m.scale.data_ptr(), m.shift.data_ptr(), y.ptr, self.idx.data_ptr()),
                        _abytes(x) + _abytes(y) + y.rows * x.C, reads=[m.x, _all(m.scale), _all(m.shift)], writes=[y, _all(self.idx)])]
        else:
            f = [Launch('maxpool_fwd', 'maxpool_fwd<%s>' % dt, lib.dv_maxpool3d_fwd,
                        (C.byref(self.d), x.ptr, y.ptr, self.idx.data_ptr()), _abytes(x) + _abytes(y) + y.rows * x.C,
                        reads=[x], writes=[y, _all(self.idx)])]
        b = []
        if self.need_dx:
            acc = bool(self.acc.get('x'))
            b.append(Launch('maxpool_bwd', 'maxpool_bwd<%s>' % dt, lib.dv_maxpool3d_bwd,
                            (C.byref(self.d), y.grad.ptr, self.idx.data_ptr(), x.grad.ptr, DV_ACCUM if acc else 0),
                            _abytes(y) + y.rows * x.C + _abytes(x) * (2 if acc else 1),
                            reads=[y.grad, _all(self.idx)] + ([x.grad] if acc else []), writes=[x.grad]))
        return f, b


class GateGroupOp(Op):
    """S3D-G self gating of a whole Inception output, in place on the concat buffer (s3dg.py:68-78,112-128):
        cat[n,s,c] *= sigmoid(fc_i(mean_s cat[n,:,slice_i]))[c]
    Three launches forward (mean, the four FCs as ONE grouped fp32 MFMA GEMM with bias+sigmoid epilogue, scale) and
    four backward.  The un-gated activations are not kept: the gate is positive, so the ReLU mask of the producing
    BatchNorm is unchanged, and sum_s dy*y = (sum_s dy*out)/g.

    FUSE_GATE (try_fuse): when the four slices are the outputs of BatchNorm + ReLU members, the mean and the scale read the
    members' conv outputs and apply the BatchNorm on load, and the members' BatchNorm backward forms the gated gradient on
    load: the un-gated concat and the gated gradient are never written (mean_bn, fc, scale_bn forward; three backward)."""

    def __init__(self, plan, fcs, cat):
        super().__init__(plan)
        self.fcs, self.cat = fcs, cat
        N, Ct = cat.N, cat.C
        assert sum(w for _, _, w in fcs) == Ct and all(o % 8 == 0 and w % 8 == 0 for _, o, w in fcs)
        self.mean, self.g = plan.f32(N, Ct), plan.f32(N, Ct)
        if plan.with_grad:
            self.dpre, self.dmean = plan.f32(N, Ct), plan.f32(N, Ct)
        self.fused = None            # the BNMembers behind the four slices, in fcs order (try_fuse)

    def inputs(self):
        return [self.cat]

    def try_fuse(self, g):
        """Plan.finalize, after the other fusions are decided: take over the forward apply of the BatchNorms that write the
        gated slices, if every slice has one, none of them is applied or differentiated somewhere else, and nothing reads
        the concat before the gate has written it."""
        p, cat = self.plan, self.cat
        if g.readers(cat)[0] is not self or len(self.fcs) > 8 or cat.rows * (cat.C // 4) >= (1 << 31):
            return
        ms = []
        for _, off, w in self.fcs:
            op, m = p.bn_out.get((_bufkey(cat), cat.off + off), (None, None))
            if (m is None or len(op.members) < 2 or m.C != w or m.M != cat.rows or not m.plain() or not m.relu
                    or m.conv_bias is not None or m.fused_pool is not None or m.fused_conv is not None or m.reduce_fused
                    or m.apply_fused or m.gate is not None or m.C % 8):
                return
            ms.append(m)
        self.fused = ms
        for m, (_, off, _) in zip(ms, self.fcs):
            m.gate = (self, off)

    def _table(self, descs):
        arr = (L.GemmDesc * len(descs))()
        tiles = 0
        for i, d in enumerate(descs):
            for k, v in d.items():
                setattr(arr[i], k, v)
            tiles += ((d['M'] + 31) // 32) * ((d['N'] + 31) // 32)
            arr[i].tile_end = tiles
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.plan.device)
        self.plan.bytes += dev.numel()
        return dev, tiles

    def launches(self):
        p, st, lib, cat = self.plan, self.plan.store, self.plan.lib, self.cat
        N, Ct, S, dt = cat.N, cat.C, cat.S, _dt(p.dtype)
        mean, g = self.mean.data_ptr(), self.g.data_ptr()
        fwd_d, bwd_d = [], []
        wm = [st.master_range(st.slot(fc.weight)) for fc, _, _ in self.fcs]
        wg = [st.grad_range(st.slot(fc.weight)) for fc, _, _ in self.fcs]
        bias0 = None
        for fc, off, w in self.fcs:
            ws, bs = st.slot(fc.weight), st.slot(fc.bias)
            assert ws.cin_pitch == w
            if bias0 is None:
                bias0 = bs
            assert bs.off == bias0.off + off, 'gate biases must be registered back to back (see SepInception.register)'
            W = st.w_master(ws)
            fwd_d.append(dict(A=mean + 4 * off, sam=Ct, sak=1, B=W, sbk=1, sbn=w, C=g + 4 * off, ldc=Ct,
                              bias=st.w_master(bs), M=N, N=w, K=w, flags=DV_SIGMOID, alpha=1.0))
            if p.with_grad:
                dpre, dmean = self.dpre.data_ptr() + 4 * off, self.dmean.data_ptr() + 4 * off
                bwd_d.append(dict(A=dpre, sam=Ct, sak=1, B=W, sbk=w, sbn=1, C=dmean, ldc=Ct, bias=0,
                                  M=N, N=w, K=w, flags=0, alpha=1.0))                      # dmean = dpre @ W
                bwd_d.append(dict(A=dpre, sam=1, sak=Ct, B=mean + 4 * off, sbk=Ct, sbn=1, C=st.w_grad(ws), ldc=w, bias=0,
                                  M=w, N=w, K=N, flags=DV_ACCUM, alpha=1.0))               # dW += dpre^T @ mean
        self._ft, ftiles = self._table(fwd_d)
        f = [Launch('gate_mean', 'spatial_mean<%s>' % dt, lib.dv_spatial_mean,
                    (p.dtype, cat.ptr, cat.ld, N, S, Ct, mean), _abytes(cat), reads=[cat], writes=[_all(self.mean)]),
             Launch('gate_fc', 'gemm_f32_grouped', lib.dv_gemm_f32_grouped, (self._ft.data_ptr(), len(fwd_d), ftiles),
                    sum(w * w * 4 for _, _, w in self.fcs), sum(2 * N * w * w for _, _, w in self.fcs),
                    reads=[_all(self._ft), _all(self.mean), (st.master, bias0.off, bias0.off + Ct)] + wm, writes=[_all(self.g)]),
             Launch('gate_scale', 'rowscale<%s,0>' % dt, lib.dv_gate_scale,
                    (p.dtype, cat.ptr, cat.ld, g, N, S, Ct, cat.ptr, cat.ld), 2 * _abytes(cat), reads=[cat, _all(self.g)], writes=[cat])]
        if self.fused:
            # the members' own table (the two kernels read x, y, scale, shift and C of it) and their first columns in mean / g
            arr = (L.BnItem * len(self.fused))(*[m.item() for m in self.fused])
            self._items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(p.device)
            self._gate_off = torch.tensor([off for _, off, _ in self.fcs], dtype=torch.int32).to(p.device)
            p.bytes += self._items.numel() + 4 * self._gate_off.numel()
            tab, goff, nm = self._items.data_ptr(), self._gate_off.data_ptr(), len(self.fused)
            xbytes = sum(_abytes(m.x) for m in self.fused)
            rd = [a for m in self.fused for a in m.touched().values()] + [_all(self._items), _all(self._gate_off)]
            f[0] = Launch('gate_mean_bn', 'gate_mean_bn<%s>' % dt, lib.dv_gate_mean_bn,
                          (p.dtype, tab, nm, goff, N, S, Ct, mean), xbytes, reads=rd, writes=[_all(self.mean)])
            f[2] = Launch('gate_scale_bn', 'gate_scale_bn<%s>' % dt, lib.dv_gate_scale_bn,
                          (p.dtype, tab, nm, goff, g, N, S, Ct), xbytes + _abytes(cat) + 4 * N * Ct,
                          reads=rd + [_all(self.g)], writes=[m.y for m in self.fused])
        b = []
        if p.with_grad:
            dy = cat.grad
            self._bt, btiles = self._table(bwd_d)
            b = [Launch('gate_bwd_reduce', 'gate_bwd_reduce<%s>' % dt, lib.dv_gate_bwd_reduce,
                        (p.dtype, dy.ptr, dy.ld, cat.ptr, cat.ld, g, N, S, Ct, self.dpre.data_ptr(), 1), 2 * _abytes(cat),
                        reads=[dy, cat, _all(self.g)], writes=[_all(self.dpre)]),
                 Launch('gate_fc_bwd', 'gemm_f32_grouped', lib.dv_gemm_f32_grouped, (self._bt.data_ptr(), len(bwd_d), btiles),
                        sum(w * w * 12 for _, _, w in self.fcs), sum(4 * N * w * w for _, _, w in self.fcs),
                        reads=[_all(self._bt), _all(self.dpre), _all(self.mean)] + wm + wg, writes=[_all(self.dmean)] + wg),
                 Launch('gate_db', 'reduce_rows', lib.dv_colsum_f32, (self.dpre.data_ptr(), Ct, N, Ct, st.w_grad(bias0)),
                        reads=[_all(self.dpre), (st.grad, bias0.off, bias0.off + Ct)], writes=[(st.grad, bias0.off, bias0.off + Ct)]),
                 Launch('gate_bwd_apply', 'rowscale<%s,1>' % dt, lib.dv_gate_bwd_apply,
                        (p.dtype, dy.ptr, dy.ld, g, self.dmean.data_ptr(), N, S, Ct, dy.ptr, dy.ld, 0), 2 * _abytes(cat),
                        reads=[dy, _all(self.g), _all(self.dmean)], writes=[dy])]
            b[1].gend = _gend(*[st.slot(fc.weight) for fc, _, _ in self.fcs])
            b[2].gend = _gend(*[st.slot(fc.bias) for fc, _, _ in self.fcs])
            if self.fused:
                del b[3]             # (the members' BatchNorm backward forms dy*g + dmean/S on load: BNGroupOp.launches)
        return f, b


class MeanOp(Op):
    """global average pool -> fp32 [N, C] (AdaptiveAvgPool3d((1,1,1)))."""

    def __init__(self, plan, x):
        super().__init__(plan)
        self.x = x
        self.out = plan.f32(x.N, x.C)
        self.dout = plan.f32(x.N, x.C) if plan.with_grad else None

    def inputs(self):
        return [self.x]

    def grad_targets(self):
        return [('x', self.x)] if (self.plan.with_grad and self.x.grad is not None) else []

    def launches(self):
        p, x, dt = self.plan, self.x, _dt(self.plan.dtype)
        f = [Launch('avgpool', 'spatial_mean<%s>' % dt, p.lib.dv_spatial_mean,
                    (p.dtype, x.ptr, x.ld, x.N, x.S, x.C, self.out.data_ptr()), _abytes(x), reads=[x], writes=[_all(self.out)])]
        b = []
        if p.with_grad and x.grad is not None:
            acc = bool(self.acc.get('x'))
            b = [Launch('avgpool_bwd', 'rowscale<%s,2>' % dt, p.lib.dv_spatial_mean_bwd,
                        (p.dtype, self.dout.data_ptr(), x.N, x.S, x.C, x.grad.ptr, x.grad.ld, DV_ACCUM if acc else 0),
                        _abytes(x) * (2 if acc else 1), reads=[_all(self.dout)] + ([x.grad] if acc else []), writes=[x.grad])]
        return f, b
