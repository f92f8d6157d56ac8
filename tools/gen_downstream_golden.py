#!/usr/bin/env python
"""Records the downstream fixtures from the reference (only where the reference tree is present):

  tests/golden/classifier_adam.npz     three Adam steps of the reference's LinearClassifier on r3d, num_class = 10, B = 4, the
      procedural clips and labels of classifier_train.npz, weight_decay 1e-4: 'ft' (use_dropout=False) at lr 1e-4 and 'last'
      (dropout, L2 norm, final BN; frozen eval-mode backbone) at lr 1e-3.  Per mode: loss0..2, eval_logit, sens/* (the
      reference re-run on the 1e-6-perturbed input, as oracle.gen_golden.case_classifier_train does) and f64/* (the reference
      in float64).  Refuses to write when a sens/loss* exceeds 2e-4: such a setting cannot pin an implementation.
      ('ft' at lr 1e-3 is such a setting: its eval logits differ by 0.12 between fp32 and fp64.)
  tests/golden/finetune_sampling.npz   the frame indices dataset/local_dataset.py's UCF101LMDB (train and test mode) and
      UCF101_10CLIP open, for several (vlen, num_frames, ds) incl. vlen <= num_frames * ds, under fixed seeds, and the next
      draw of `random` and `numpy.random` after each call (what the sampler consumed).

Run from the repository root:  python tools/gen_downstream_golden.py"""
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import harness, procedural as P  # noqa: E402
from oracle.gen_golden import CLIP, GOLD  # noqa: E402

SENS_LIMIT = 2e-4
ADAM_MODES = (('ft', dict(use_dropout=False), 1e-4), ('last', dict(use_dropout=True, use_l2_norm=True, use_final_bn=True), 1e-3))
SAMPLING_CASES = [(70, 16, 1), (70, 16, 2), (40, 16, 4), (32, 16, 2), (9, 16, 1), (300, 32, 2), (165, 16, 4), (33, 16, 2), (64, 8, 4)]
SAMPLING_SEEDS = (0, 1, 2)


def adam_train(c, mode, xa, xb, labels, lr, steps=3, dtype=torch.float32):
    """classifier.py:240-262,422-470 with --optim adam: 'ft' = model.train(), every parameter; 'last' = model.eval(),
    final_bn.train(), backbone frozen.  Adam(lr, weight_decay 1e-4); CrossEntropyLoss."""
    c = c.to(dtype)
    xa, xb = xa.to(dtype), xb.to(dtype)
    with torch.no_grad():
        c.train()
        c.backbone(xa)                                   # non-trivial running statistics
    if mode == 'last':
        for n_, p_ in c.named_parameters():
            if 'backbone' in n_:
                p_.requires_grad = False
    opt = torch.optim.Adam([{'params': [p_]} for p_ in c.parameters() if p_.requires_grad], lr=lr, weight_decay=1e-4)
    crit = torch.nn.CrossEntropyLoss()
    rec = {}
    for it in range(steps):
        if mode == 'last':
            c.eval()
            if getattr(c, 'use_final_bn', False):
                c.final_bn.train()
        else:
            c.train()
        logit, _ = c(xb)
        loss = crit(logit, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        rec['loss%d' % it] = np.array(float(loss.detach()))
    with torch.no_grad():
        rec['eval_logit'] = c.eval()(xb)[0].double().numpy().copy()
    return rec


def case_classifier_adam(ref):
    xa = P.procedural_clips(4, 1, **CLIP)[:, 0]
    xb = P.procedural_clips(4, 1, seed=77, **CLIP)[:, 0]
    labels = torch.tensor([3, 0, 2, 1])
    noise = torch.from_numpy(np.random.RandomState(99).standard_normal(xb.numel())).float().reshape(xb.shape)
    out = {}
    for mode, kw, lr in ADAM_MODES:
        def run(x, dtype=torch.float32):
            torch.manual_seed(0)
            c = ref.linear_classifier('r3d', num_class=10, **kw)
            P.procedural_init(c)
            return adam_train(c, mode, xa, x, labels, lr, dtype=dtype)
        base, pert, f64 = run(xb), run(xb * (1 + 1e-6 * noise)), run(xb, torch.float64)
        for k, v in base.items():
            out['%s/%s' % (mode, k)] = v.astype(np.float32) if v.ndim else v
            out['%s/sens/%s' % (mode, k)] = np.array(float(np.max(np.abs(np.asarray(v, np.float64) - np.asarray(pert[k], np.float64)))))
            out['%s/f64/%s' % (mode, k)] = f64[k]
        out['%s/lr' % mode] = np.array(lr)
        print('classifier adam', mode, 'losses', [float(base['loss%d' % i]) for i in range(3)],
              'sens', max(float(out['%s/sens/loss%d' % (mode, i)]) for i in range(3)),
              'fp32 vs fp64', max(abs(float(base['loss%d' % i]) - float(f64['loss%d' % i])) for i in range(3)),
              'eval_logit fp32 vs fp64', float(np.max(np.abs(base['eval_logit'] - f64['eval_logit']))))
    worst = max(float(v) for k, v in out.items() if '/sens/loss' in k)
    if worst > SENS_LIMIT:
        raise SystemExit('refusing to write classifier_adam.npz: sens/loss reaches %.3g > %g' % (worst, SENS_LIMIT))
    np.savez_compressed(os.path.join(GOLD, 'classifier_adam.npz'), **out)


def reference_dataset(LD, cls, vlen, num_frames, ds, mode):
    """an instance of the reference's dataset class on a one-row table; Image.open is replaced so that no file is needed: the
    'frames' handed to the transform are the paths the class opens"""
    import pandas as pd
    d = object.__new__(cls)
    opened = []

    def record(seq):
        opened.append(list(seq))
        return [torch.zeros(1) for _ in seq]
    d.__dict__.update(num_frames=num_frames, ds=ds, mode=mode, transform=record, return_label=False, return_path=False, db_path='',
                      video_subset=pd.DataFrame([['/d/frame/Walk/v/', vlen, 'Walk', 'Walk/v']]))
    LD.Image = types.SimpleNamespace(open=lambda path: path)
    return d, opened


def opened_indices(paths):
    return np.asarray([int(os.path.basename(p)[len('image_'):-len('.jpg')]) - 1 for p in paths], dtype=np.int32)


def case_finetune_sampling(ref):
    import dataset.local_dataset as LD
    real_image = LD.Image
    out = {'cases': np.asarray([(v, n, d, s) for v, n, d in SAMPLING_CASES for s in SAMPLING_SEEDS], dtype=np.int32)}
    try:
        for k, (vlen, nf, ds, seed) in enumerate(out['cases'].tolist()):
            for mode, cls, dmode in (('train', LD.UCF101LMDB, 'train'), ('test', LD.UCF101LMDB, 'test'), ('10clip', LD.UCF101_10CLIP, 'test')):
                d, opened = reference_dataset(LD, cls, vlen, nf, ds, dmode)
                random.seed(seed)
                np.random.seed(seed)
                d[0]
                out['%s/%d' % (mode, k)] = opened_indices(opened[-1])
                out['%s/rng/%d' % (mode, k)] = np.asarray([random.random(), np.random.random()])
    finally:
        LD.Image = real_image
    np.savez_compressed(os.path.join(GOLD, 'finetune_sampling.npz'), **out)
    print('finetune sampling: %d cases x 3 modes' % len(out['cases']))


def main():
    if not harness.available():
        raise SystemExit('the reference tree is not present: nothing to record from')
    ref = harness.load_reference()
    which = sys.argv[1:] or ['adam', 'sampling']
    if 'sampling' in which:
        case_finetune_sampling(ref)
    if 'adam' in which:
        case_classifier_adam(ref)


if __name__ == '__main__':
    main()
