"""Print what Plan.finalize decided, for a matrix of plans built on the CPU (no GPU needed, only the built library).

Two commits whose dumps are identical byte for byte launch the same kernels on the same shapes with the same fusions: the
check for a change of the planning code that is meant to change no plan.

    python tools/plan_dump.py > dump.txt              # the whole matrix (several minutes)
    python tools/plan_dump.py --nets s3dg --anchors   # one net, with the per-plan fusion counts on stderr
    python tools/plan_dump.py --nets s3dg --args      # with the arguments of the BatchNorm / gate / SyncBatchNorm / conv launches
    python tools/plan_dump.py --nets s3dg --args --exchange     # the same plans on the multi-rank path (one gloo rank)

Per plan: every entry of the forward and the backward list (name, kernel, shape, bytes, flops, gradient-arena end), per op its
accumulate flags and the fusions it takes, and the plan's bytes.  Two convs that share a grid (engine.PAIR_CONVS) are one entry:
kernel '...+pair', both shapes, the members' bytes and flops summed; the setting no_pair dumps the unpaired lists.  Pointers differ from run to run: they are left out, or, with
--args, printed as (ordinal of the storage they point into, in order of first appearance in the plan's dump; byte offset)."""
import argparse
import bisect
import ctypes as C
import gc
import os
import socket
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dualvar_amd import _lib as L, engine                           # noqa: E402
from dualvar_amd.backbone.select_backbone import select_backbone    # noqa: E402

NETS = ('s3dg', 's3d', 'r21d', 'r3d', 'r50', 'r2d3d18', 'c3d')
SWITCHES = ('FUSE_BN_REDUCE', 'FUSE_BN_REDUCE_TAP', 'FUSE_BN_IN', 'FUSE_BN_WGRAD', 'FUSE_GATE', 'PAIR_CONVS')
DEFAULT = dict(FUSE_BN_REDUCE=False, FUSE_BN_REDUCE_TAP=False, FUSE_BN_IN=True, FUSE_BN_WGRAD=True, FUSE_GATE=True, PAIR_CONVS=True)
SETTINGS = (('default', {}),
            ('reduce', dict(FUSE_BN_REDUCE=True, FUSE_BN_REDUCE_TAP=False)),
            ('reduce_tap', dict(FUSE_BN_REDUCE_TAP=True)),
            ('no_bn_in', dict(FUSE_BN_IN=False)),
            ('no_bn_wgrad', dict(FUSE_BN_WGRAD=False)),
            ('no_gate', dict(FUSE_GATE=False)),
            ('no_pair', dict(PAIR_CONVS=False)))
MODES = (('train_grad', True, False, True), ('train_nograd', True, False, False), ('eval_map', False, True, False))
OP_FLAGS = ('bn_fuse', 'bn_fuse_tap', 'bn_apply', 'bn_in', 'fused', 'bn_member')
ARG_PREFIXES = ('bn_', 'gate_', 'syncbn_', 'conv_', 'stem_', 'quantize_')
# the entries that take a device table of dv_bn_item: position of the pointer (the number of items follows it)
ITEM_TABLES = dict(dv_bn_stats_multi=0, dv_bn_finalize_multi=0, dv_bn_apply_multi=1, dv_bn_bwd_reduce_multi=1,
                   dv_bn_bwd_apply_multi=1, dv_bn_bwd_reduce_multi_gated=1, dv_bn_bwd_apply_multi_gated=1, dv_gate_mean_bn=1,
                   dv_gate_scale_bn=1)


def build_plan(model, clips, training, want_map, with_grad):
    model.train(training)
    model._plans.clear()
    x = torch.empty(clips, 3, 8, 112, 112)
    return model._acquire_plan(x, False, want_map, with_grad)


class Pointers:
    """addresses of a plan built on the CPU -> (storage ordinal, byte offset); the storages are those of the live tensors"""

    def __init__(self):
        spans = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')          # (isinstance() wakes the deprecated lazy attributes of torch's modules)
            tensors = [o for o in gc.get_objects() if isinstance(o, torch.Tensor)]
        for st in (t.untyped_storage() for t in tensors if t.device.type == 'cpu'):
            if st.nbytes():
                spans[st.data_ptr()] = max(spans.get(st.data_ptr(), 0), st.nbytes())
        self.starts = sorted(spans)
        self.sizes = [spans[a] for a in self.starts]
        self.ordinal = {}

    def __call__(self, addr):
        if not addr:
            return '0'
        i = bisect.bisect_right(self.starts, addr) - 1
        if i < 0 or addr - self.starts[i] >= self.sizes[i]:
            return '(?)'                 # (points into no live tensor)
        return '(%d,%d)' % (self.ordinal.setdefault(self.starts[i], len(self.ordinal)), addr - self.starts[i])


def _value(ctype, v, ptr):
    if isinstance(v, C.Structure):
        return '{%s}' % ' '.join('%s=%s' % (n, _value(t, getattr(v, n), ptr)) for n, t in v._fields_)
    if ctype is C.c_void_p:
        return ptr(v)
    if ctype is C.c_float:
        return repr(C.c_float(v).value)      # (as the callee receives it)
    return repr(v)


def dump_args(l, out, ptr):
    """the arguments of one launch as its entry receives them; a host step or a closure (the collectives) goes by its name only"""
    types = getattr(getattr(l, 'fn', None), 'argtypes', None)
    if types is None or not isinstance(getattr(l, 'args', None), tuple):
        return
    vals = [a._obj if hasattr(a, '_obj') else a for a in l.args]             # (C.byref(descriptor) -> the descriptor)
    out.write('  args %s\n' % ', '.join(_value(t, v, ptr) for t, v in zip(types, vals)))
    at = ITEM_TABLES.get(l.fn.__name__)
    if at is not None:
        for k, it in enumerate((L.BnItem * vals[at + 1]).from_address(vals[at])):
            out.write('  item %d %s\n' % (k, _value(None, it, ptr)))


def dump_plan(plan, out, args=False):
    ptr = Pointers() if args else None
    for tag, lst in (('f', plan.f_list), ('b', plan.b_list)):
        for l in lst:
            out.write('%s %s, %s, %s, %d, %d, %d\n' % (tag, l.name, l.kname, getattr(l, 'shape', ''), l.bytes, l.flops,
                                                       getattr(l, 'gend', 0)))
            if args and l.name.startswith(ARG_PREFIXES):
                dump_args(l, out, ptr)
    for i, op in enumerate(plan.ops):
        on = [f for f in OP_FLAGS if getattr(op, f, None) not in (None, False)]
        out.write('op %d %s acc=%s %s\n' % (i, type(op).__name__, sorted(op.acc.items()), ' '.join(on)))
    out.write('bytes %d\n' % plan.bytes)


def counts(plan):
    n = lambda f: sum(1 for op in plan.ops if getattr(op, f, None) not in (None, False))      # noqa: E731
    pairs = sum(1 for l in plan.f_list + plan.b_list if getattr(l, 'members', ()))
    return 'bn_in %d  bn_apply %d  gates %d  pools %d  bn_fuse %d  bn_fuse_tap %d  conv pairs %d' % (
        n('bn_in'), n('bn_apply'), n('fused'), n('bn_member'), n('bn_fuse'), n('bn_fuse_tap'), pairs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--nets', nargs='+', default=list(NETS), choices=NETS)
    ap.add_argument('--anchors', action='store_true', help='per plan, print the number of ops that take each fusion on stderr')
    ap.add_argument('--args', action='store_true', help='print the arguments, and the dv_bn_item tables, of the launches named '
                    + ' / '.join(p + '*' for p in ARG_PREFIXES))
    ap.add_argument('--exchange', action='store_true', help='build the plans on the multi-rank path: DUALVAR_FORCE_EXCHANGE=1 in '
                    'a gloo group of one rank on the loopback address')
    a = ap.parse_args()
    if os.environ.get('DUALVAR_F32_EXACT'):
        sys.exit('unset DUALVAR_F32_EXACT: the matrix is defined for the default fp32 kernels')
    out = sys.stdout
    if a.exchange:
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), DUALVAR_FORCE_EXCHANGE='1')
        torch.distributed.init_process_group('gloo', rank=0, world_size=1)
    for net in a.nets:
        for dtype in ('fp32', 'bf16') + (('fp8pw',) if net == 'r50' else ()):
            torch.manual_seed(0)
            model, _ = select_backbone(net)
            model.set_compute_dtype(dtype)
            model.store.materialize(torch.device('cpu'), model.dtype)
            for clips in ((4,) if net == 'r50' else (8,)) + ((64,) if net in ('s3dg', 'r21d') else ()):
                for mode, training, want_map, with_grad in MODES:
                    for sname, over in SETTINGS:
                        for k in SWITCHES:
                            setattr(engine, k, over.get(k, DEFAULT[k]))
                        head = '%s %s clips=%d %s %s' % (net, dtype, clips, mode, sname)
                        out.write('== %s\n' % head)
                        plan = build_plan(model, clips, training, want_map, with_grad)
                        dump_plan(plan, out, a.args)
                        if a.anchors:
                            sys.stderr.write('%s: %s\n' % (head, counts(plan)))
                        del plan
                        model._plans.clear()
                        gc.collect()                 # (a plan and its ops refer to each other; the 64-clip plans hold gigabytes)


if __name__ == '__main__':
    main()
