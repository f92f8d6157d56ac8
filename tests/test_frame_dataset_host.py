"""CPU: the real-frame pretraining path on the host -- PIL-exact Scale tables and their integer mirror against PIL itself
(dualvar_amd/utils/resample.py), the reference's frame datasets (dualvar_amd/utils/frame_dataset.py: sampler, RNG order,
aug_series reuse, the D9 split repair, collate packing) and pretrain.py's refusals.  Where the reference tree is present, its own
dataset class and MultiRandomizedTransform are run through oracle.harness."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import pretrain                                     # before oracle.harness puts the reference tree in front on sys.path
from dualvar_amd.utils import frame_dataset as FD
from dualvar_amd.utils import resample as R
from dualvar_amd.utils import transforms as T
from tests.dataset_support import SIZES, TARGETS, _img, _rng_state, _seed, ref, write_dataset  # noqa: F401  (ref: a fixture)


@pytest.mark.parametrize('filt', ['bicubic', 'bilinear'])
def test_mirror_equals_pil(filt):
    r = np.random.RandomState(1)
    pf = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}[filt]
    for H, W in SIZES:
        img = _img(r, H, W)
        for Ho, Wo in TARGETS:
            want = np.asarray(Image.fromarray(img).resize((Wo, Ho), pf))
            got = R.resize_u8(img, (Ho, Wo), filt)
            assert got.dtype == np.uint8 and np.array_equal(got, want), ((H, W), (Ho, Wo), filt)


def test_tables_and_skip_rule():
    ksize, xmin, n, w = R.coeffs(320, 128)
    assert ksize == 11 and len(xmin) == 128 and int(xmin.min()) >= 0 and int((xmin + n).max()) <= 320
    assert np.all(np.abs(w.sum(1) - (1 << 22)) <= ksize)                   # normalised weights, rounded per tap
    t = R.table_words(240, 171)
    assert t.dtype == np.int32 and list(t[:4]) == [240, 171, R.coeffs(240, 171)[0], 0]
    assert len(t) == 4 + 171 * (2 + t[2])
    with pytest.raises(ValueError):
        R.table_words(2000, 128)                                            # 33 taps: over the kernel's cap
    img = _img(np.random.RandomState(2), 171, 90)
    assert np.array_equal(R.resize_u8(img, (171, 128))[:, :, :], np.asarray(Image.fromarray(img).resize((128, 171), Image.BICUBIC)))
    _, desc, _ = R.pack([img, _img(np.random.RandomState(3), 240, 128)], (171, 128))
    assert desc['v_coef'][0] == -1 and desc['h_coef'][0] >= 0                # rows unchanged: no vertical pass
    assert desc['h_coef'][1] == -1 and desc['v_coef'][1] >= 0


def test_pack_mixed_sizes():
    r = np.random.RandomState(4)
    frames = [_img(r, *s) for s in [(240, 320), (240, 426), (240, 320), (17, 5), (171, 128)]]
    src, desc, coef = R.pack(frames, (171, 128))
    assert R.DESC.itemsize == 24 and desc.dtype == R.DESC and len(desc) == 5
    assert np.all(desc['src_offset'] % 16 == 0)
    for f, d in zip(frames, desc):
        assert (d['Hs'], d['Ws']) == f.shape[:2]
        o = int(d['src_offset'])
        assert np.array_equal(src[o:o + f.nbytes].reshape(f.shape), f)
        assert o + (f.nbytes + 15) // 16 * 16 <= len(src)
        for key, i, o_ in (('h_coef', 1, 128), ('v_coef', 0, 171)):
            t = int(d[key])
            if f.shape[i] == o_:
                assert t == -1
            else:
                assert list(coef[t:t + 2]) == [f.shape[i], o_]
    assert desc['h_coef'][0] == desc['h_coef'][2] and desc['v_coef'][0] == desc['v_coef'][1]     # shared tables, stored once


def test_desc_mirror_matches_header(tmp_path):
    """dv_resample_desc (a plain struct of include/dualvar_hip.h) against its numpy mirror: a C probe prints sizeof / offsetof"""
    import shutil
    import subprocess
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'no host C compiler'
    names = list(R.DESC.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dualvar_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(struct dv_resample_desc));']
    lines += ['  printf("%s %%zu\\n", offsetof(struct dv_resample_desc, %s));' % (f, f) for f in names]
    lines += ['  printf("ksize %d\\n", DV_RESAMPLE_MAX_KSIZE);', '  return 0;', '}']
    (tmp_path / 'probe.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'probe')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([cc, '-std=c11', '-I', os.path.join(root, 'include'), str(tmp_path / 'probe.c'), '-o', exe], check=True)
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got['size'] == R.DESC.itemsize == 24 and got['ksize'] == R.MAX_KSIZE
    assert all(got[f] == R.DESC.fields[f][1] for f in names)


def test_split_repairs_d9(tmp_path):
    split, frame = write_dataset(str(tmp_path), rows=830)
    import pandas as pd
    info = pd.read_csv(os.path.join(split, 'train_split01.csv'), header=None)
    val_idx = info.sample(n=800, random_state=666).index
    tr, va, te = (FD.read_split(split, m) for m in ('train', 'val', 'test'))
    assert len(tr) == 30 and len(va) == 800 and len(te) == 3
    assert set(tr.index).isdisjoint(va.index) and list(va.index) == list(val_idx)
    assert sorted(set(tr.index) | set(va.index)) == list(range(830))
    assert list(tr.columns) == [0, 1, 2, 3]
    row = te.iloc[2]
    assert row[2] == 'Jump' and row[3] == 'Jump/v_Jump_g02' and int(row[1]) == 70
    small, _ = write_dataset(str(tmp_path / 'small'), videos=((0, 3), (1, 3)), rows=20)
    with pytest.raises(ValueError, match='800'):
        FD.read_split(small, 'train')


def test_sampler_draws_and_aug_series(tmp_path):
    split, frame = write_dataset(str(tmp_path))
    ds = FD.StagePrototypeFrames(split, frame, num_frames=16, ds=4, rand_flip=True, aug_series=True)
    for vlen in (9, 40, 200):
        _seed(vlen)
        i1, i2 = ds.sample_indices(vlen)
        assert len(i1) == len(i2) == 16 and i1.min() >= 0 and i1.max() <= vlen - 1
    _seed(0)
    out = ds[0]
    vlen = int(ds.video_subset.iloc[0][1])
    _seed(0)
    i1, i2 = ds.sample_indices(vlen)
    distinct = list(dict.fromkeys(np.concatenate([i1, i2]).tolist()))
    assert len(out['decoded']) == len(distinct) and all(f.shape == (240, 320, 3) for f in out['decoded'])
    # with a transform: three clips, the third = clip 1's frames, read once
    tr = FD.stage_prototype_transform(112, 16)
    ds_t = FD.StagePrototypeFrames(split, frame, num_frames=16, ds=4, rand_flip=True, aug_series=True, transform=tr)
    _seed(5)
    s = ds_t[1]
    assert s['aug'].shape == (48,) and s['blur'].shape == (48,) and s['patch'].shape == (48,)
    assert np.array_equal(s['aug']['src'][32:], s['aug']['src'][:16])
    assert int(s['aug']['src'].max()) == len(s['decoded']) - 1
    assert np.all(s['aug']['crop_h'] == 112) and np.all(s['aug']['crop_i'] <= 171 - 112) and np.all(s['aug']['crop_j'] <= 128 - 112)
    with pytest.raises(ValueError, match='3 clips'):
        FD.StagePrototypeFrames(split, frame, aug_series=False, transform=tr)


def test_refusals():
    base = ['--dataset', 'ucf101-2clip-stage-prototype', '--num_seq', '3', '--aug_series']
    a = pretrain.parse_args(base)
    assert a.split_root.endswith(os.path.join('process_data', 'data', 'ucf101')) and a.frame_root.endswith(os.path.join('data', 'UCF101', 'frame'))
    a = pretrain.parse_args(['--dataset', 'k400-2clip-stage-prototype', '--num_seq', '3', '--aug_series', '--split_root', '/s'])
    assert a.split_root == '/s' and a.frame_root.endswith(os.path.join('data', 'K400', 'frame'))
    for bad in (base[:4], ['--dataset', 'ucf101-2clip-stage-prototype', '--num_seq', '2', '--aug_series'],
                base + ['--n_proto', '2']):
        with pytest.raises(SystemExit):
            pretrain.parse_args(bad)
    assert pretrain.parse_args(['--dataset', 'ucf101', '--num_seq', '2']).split_root is None     # other names: unchanged


def test_pil_crop_and_patched_jitter_draws():
    _seed(7)
    st = T.PILRandomCrop(112)(T.ClipState(range(4), 171, 128))
    _seed(7)
    left, top = random.randint(0, 128 - 112), random.randint(0, 171 - 112)
    assert (st.i, st.j, st.h, st.w) == (top, left, 112, 112)
    _seed(8)
    st = T.ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.8, patched=True)(T.ClipState(range(6), 171, 128))
    rows = st.patch_rows(171, 128, block=1)
    _seed(8)
    for n in range(6):                               # utils/augmentation.py:587-600 at block 1: gate, four draws, shuffle
        ops = []
        if np.random.uniform(0., 1.) < 0.8:
            ops = [(c, random.uniform(*rg)) for c, rg in zip((1, 2, 3, 5), ([0.2, 1.8],) * 3 + ([-0.2, 0.2],))]
            random.shuffle(ops)
        got = [(int(c), float(f)) for c, f in zip(rows[n]['op'], rows[n]['factor']) if c]
        assert [c for c, _ in got] == [c for c, _ in ops]
        assert np.allclose([f for _, f in got], [f for _, f in ops], rtol=1e-6)


def test_collate_packs_ragged_frames(tmp_path):
    split, frame = write_dataset(str(tmp_path), sizes=[(240, 320), (240, 426), (120, 96)])
    tr = FD.stage_prototype_transform(64, 8)
    ds = FD.StagePrototypeFrames(split, frame, mode='test', num_frames=8, ds=2, aug_series=True, transform=tr, img_dim=64)
    _seed(3)
    samples = [ds[i] for i in range(3)]
    b = FD.collate_frame_clips(samples)
    desc, coef = b['rs_host']
    n = sum(len(s['decoded']) for s in samples)
    assert b['n_frames'] == n == len(desc) and b['rs_desc'].numel() == n * 24 and b['rs_coef'].dtype == torch.int32
    assert sorted(set(zip(desc['Hs'].tolist(), desc['Ws'].tolist()))) == [(120, 96), (240, 320), (240, 426)]
    aug = b['aug'].numpy().view(T.AUG_ROW).reshape(3, -1)
    base = 0
    for k, s in enumerate(samples):
        assert np.array_equal(aug[k]['src'], s['aug']['src'] + base)
        for j, f in enumerate(s['decoded']):
            d = desc[base + j]
            o = int(d['src_offset'])
            assert np.array_equal(b['src'].numpy()[o:o + f.nbytes].reshape(f.shape), f)
        base += len(s['decoded'])
    assert b['patch'].shape == (3, 24 * T.AUG_PATCH.itemsize) and b['blur'].shape == (3, 24 * T.AUG_BLUR.itemsize)


# ------------------------------------------------------------------ against the reference's own classes

@pytest.mark.parametrize('rand_flip', [False, True])
@pytest.mark.parametrize('ds_', [1, 4])
def test_getitem_order_against_reference(ref, tmp_path, rand_flip, ds_):
    """the reference's __getitem__ (frame files it opens, incl. the aug_series repeat) and the RNG state it leaves, against
    ours, for a short video (vlen < num_frames * ds) and a long one"""
    LD, _ = ref
    split, frame = write_dataset(str(tmp_path), videos=((0, 9), (1, 70)), rows=810)
    mine = FD.StagePrototypeFrames(split, frame, mode='test', num_frames=16, ds=ds_, rand_flip=rand_flip, aug_series=True)
    theirs = object.__new__(LD.UCF101LMDB_2CLIP_Stage_Prototype)
    opened = []

    def record(seq):
        opened.append([os.path.relpath(im.filename, frame) for im in seq])
        return [torch.zeros(1) for _ in seq]
    theirs.__dict__.update(num_frames=16, ds=ds_, rand_flip=rand_flip, aug_series=True, transform=record, return_label=False,
                           db_path=frame, video_subset=mine.video_subset, mode='test')
    for idx in (0, 1):
        for seed in range(4):
            _seed(seed)
            theirs[idx]
            after = _rng_state()
            _seed(seed)
            vlen, vname = int(mine.video_subset.iloc[idx][1]), mine.video_subset.iloc[idx][3]
            i1, i2 = mine.sample_indices(vlen)
            assert _rng_state() == after
            want = [os.path.relpath(mine.frame_path(vname, i), frame) for i in list(i1) + list(i2) + list(i1)]
            assert opened[-1] == want


def test_multi_randomized_choice_against_reference(ref):
    _, RA = ref
    weights = [[0.2, 0.8, 0], [0, 1.0, 0], [0, 0., 1.0]]
    picked = []

    def tag(k):
        def t(x):
            picked.append(k)
            return x
        return t
    theirs = RA.MultiRandomizedTransform([tag(0), tag(1), tag(2)], 4, weights=weights)
    mine = T.MultiRandomizedTransform([tag(0), tag(1), tag(2)], weights=weights)
    seen = set()
    for seed in range(40):
        np.random.seed(seed)
        picked.clear()
        theirs(list(range(12)))
        want, st = list(picked), np.random.get_state()[1].tolist()
        np.random.seed(seed)
        picked.clear()
        mine([T.ClipState(range(4), 171, 128) for _ in range(3)])
        assert picked == want and np.random.get_state()[1].tolist() == st
        seen.add(tuple(want))
    assert seen == {(0, 1, 2), (1, 1, 2)}
    with pytest.raises(ValueError):
        mine([T.ClipState(range(4), 171, 128)] * 2)


def test_pil_random_crop_against_reference(ref):
    _, RA = ref
    for seed in range(10):
        random.seed(seed)
        h_start, w_start = random.randint(0, 128 - 112), random.randint(0, 171 - 112)
        random.seed(seed)
        st = T.PILRandomCrop(112)(T.ClipState(range(1), 171, 128))
        assert (st.j, st.i) == (h_start, w_start)
        random.seed(seed)
        full = np.random.RandomState(seed).randint(0, 256, (171, 128, 3)).astype(np.uint8)
        crop = np.asarray(RA.RandomCrop(112)([Image.fromarray(full)])[0])
        assert np.array_equal(crop, full[st.i:st.i + 112, st.j:st.j + 112])
