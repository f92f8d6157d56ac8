"""What the frame-dataset, finetune, driver and evaluation suites share: a tiny frame dataset on disk, test images, the three
RNGs' seeding and state, and the fixture that loads the reference's own dataset classes where its tree is present."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

SIZES = [(240, 320), (240, 426), (240, 456), (360, 240), (240, 240), (171, 128), (100, 60), (17, 5), (1, 9), (9, 1)]
TARGETS = [(171, 128), (128, 171), (300, 400), (1, 3)]


def _img(r, H, W):
    a = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
    a[:H // 3, :W // 3] = 255                        # saturated regions: the bicubic overshoot must clamp
    a[H // 2:, W // 2:] = 0
    return a


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _rng_state():
    return random.getstate(), np.random.get_state()[1].tolist(), torch.get_rng_state().tolist()


def write_dataset(root, videos=((0, 40), (0, 9), (1, 70)), classes=('Walk', 'Jump'), rows=810, sizes=None, seed=0):
    """<root>/split/{ClassInd.txt, train_split01.csv, test_split01.csv}, <root>/frame/<class>/<video>/image_%05d.jpg; the train
    CSV repeats the videos to `rows` rows (the train / val split sets 800 aside)"""
    r = np.random.RandomState(seed)
    split, frame = os.path.join(root, 'split'), os.path.join(root, 'frame')
    os.makedirs(split, exist_ok=True)
    with open(os.path.join(split, 'ClassInd.txt'), 'w') as f:
        f.write(''.join('%d,%s\n' % (i + 1, c) for i, c in enumerate(classes)))
    lines = []
    for v, (ci, vlen) in enumerate(videos):
        vname = '%s/v_%s_g%02d' % (classes[ci], classes[ci], v)
        d = os.path.join(frame, vname)
        os.makedirs(d, exist_ok=True)
        H, W = sizes[v] if sizes else (240, 320)
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(vlen):
            base = (np.sin(yy / (7.0 + v) + i * 0.3)[..., None] * np.cos(xx / 9.0)[..., None] * 0.4 + 0.5) * r.uniform(0.5, 1, 3)
            img = ((base + r.uniform(-0.1, 0.1, (H, W, 3))).clip(0, 1) * 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, 'image_%05d.jpg' % (i + 1)), quality=80)
        lines.append('/data/frame/%s/,%d\n' % (vname, vlen))
    with open(os.path.join(split, 'train_split01.csv'), 'w') as f:
        f.write(''.join(lines[i % len(lines)] for i in range(rows)))
    with open(os.path.join(split, 'test_split01.csv'), 'w') as f:
        f.write(''.join(lines))
    return split, frame


@pytest.fixture
def ref():
    """the reference's dataset and augmentation modules; the test is skipped where its tree is not present"""
    from oracle import harness
    if not harness.available():
        pytest.skip('reference tree not present')
    harness.load_reference()
    import dataset.local_dataset as LD
    import utils.augmentation as RA
    return LD, RA
