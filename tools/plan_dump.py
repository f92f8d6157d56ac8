"""Print what Plan.finalize decided, for a matrix of plans built on the CPU (no GPU needed, only the built library).

Two commits whose dumps are identical byte for byte launch the same kernels on the same shapes with the same fusions: the
check for a change of the planning code that is meant to change no plan.

    python tools/plan_dump.py > dump.txt              # the whole matrix (several minutes)
    python tools/plan_dump.py --nets s3dg --anchors   # one net, with the per-plan fusion counts on stderr

Per plan: every entry of the forward and the backward list (name, kernel, shape, bytes, flops, gradient-arena end), per op its
accumulate flags and the fusions it takes, and the plan's bytes.  Pointers are left out: they differ from run to run."""
import argparse
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dualvar_amd import engine                                      # noqa: E402
from dualvar_amd.backbone.select_backbone import select_backbone    # noqa: E402

NETS = ('s3dg', 's3d', 'r21d', 'r3d', 'r50', 'r2d3d18', 'c3d')
SWITCHES = ('FUSE_BN_REDUCE', 'FUSE_BN_REDUCE_TAP', 'FUSE_BN_IN', 'FUSE_BN_WGRAD', 'FUSE_GATE')
DEFAULT = dict(FUSE_BN_REDUCE=False, FUSE_BN_REDUCE_TAP=False, FUSE_BN_IN=True, FUSE_BN_WGRAD=True, FUSE_GATE=True)
SETTINGS = (('default', {}),
            ('reduce', dict(FUSE_BN_REDUCE=True, FUSE_BN_REDUCE_TAP=False)),
            ('reduce_tap', dict(FUSE_BN_REDUCE_TAP=True)),
            ('no_bn_in', dict(FUSE_BN_IN=False)),
            ('no_bn_wgrad', dict(FUSE_BN_WGRAD=False)),
            ('no_gate', dict(FUSE_GATE=False)))
MODES = (('train_grad', True, False, True), ('train_nograd', True, False, False), ('eval_map', False, True, False))
OP_FLAGS = ('bn_fuse', 'bn_fuse_tap', 'bn_apply', 'bn_in', 'fused', 'bn_member')


def build_plan(model, clips, training, want_map, with_grad):
    model.train(training)
    model._plans.clear()
    x = torch.empty(clips, 3, 8, 112, 112)
    return model._acquire_plan(x, False, want_map, with_grad)


def dump_plan(plan, out):
    for tag, lst in (('f', plan.f_list), ('b', plan.b_list)):
        for l in lst:
            out.write('%s %s, %s, %s, %d, %d, %d\n' % (tag, l.name, l.kname, getattr(l, 'shape', ''), l.bytes, l.flops,
                                                       getattr(l, 'gend', 0)))
    for i, op in enumerate(plan.ops):
        on = [f for f in OP_FLAGS if getattr(op, f, None) not in (None, False)]
        out.write('op %d %s acc=%s %s\n' % (i, type(op).__name__, sorted(op.acc.items()), ' '.join(on)))
    out.write('bytes %d\n' % plan.bytes)


def counts(plan):
    n = lambda f: sum(1 for op in plan.ops if getattr(op, f, None) not in (None, False))      # noqa: E731
    return 'bn_in %d  bn_apply %d  gates %d  pools %d  bn_fuse %d  bn_fuse_tap %d' % (
        n('bn_in'), n('bn_apply'), n('fused'), n('bn_member'), n('bn_fuse'), n('bn_fuse_tap'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--nets', nargs='+', default=list(NETS), choices=NETS)
    ap.add_argument('--anchors', action='store_true', help='per plan, print the number of ops that take each fusion on stderr')
    a = ap.parse_args()
    if os.environ.get('DUALVAR_F32_EXACT'):
        sys.exit('unset DUALVAR_F32_EXACT: the matrix is defined for the default fp32 kernels')
    out = sys.stdout
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
                        dump_plan(plan, out)
                        if a.anchors:
                            sys.stderr.write('%s: %s\n' % (head, counts(plan)))
                        del plan
                        model._plans.clear()
                        gc.collect()                 # (a plan and its ops refer to each other; the 64-clip plans hold gigabytes)


if __name__ == '__main__':
    main()
