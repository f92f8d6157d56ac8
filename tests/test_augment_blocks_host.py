"""CPU: the block-wise and time-graded colour jitter of the augmenting ingest on the host side -- the reference's
utils/augmentation.py:ColorJitter(block=b, grad_consistent=...) (:429-661) restated as per-patch op lists
(dualvar_amd.utils.transforms: ColorJitter, ClipState.patch_rows, FrameBatch; pretrain.py: gpu_transform, SyntheticFrames,
collate_frames).  Where the reference tree is present, its own draws are compared through oracle.harness."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import pretrain                                     # before oracle.harness puts the reference tree in front on sys.path
from dualvar_amd.utils import transforms as T
from dualvar_amd.utils.transforms import (AUG_BRIGHTNESS, AUG_CONTRAST, AUG_GRAY, AUG_HUE, AUG_NONE, AUG_PATCH, AUG_SATURATION,
                                          ClipState, ColorJitter, FrameBatch)
from tests.dataset_support import _seed

FOUR = (AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE)


def _clip(N=8, crop=112, Hs=128, Ws=171):
    st = ClipState(range(N), Hs, Ws)
    return T.RandomCrop((crop, crop))(st)


def _lists(t, N, nb):
    """AUG_PATCH rows -> [frame][patch] = [(code, factor)]"""
    out = []
    for n in range(N):
        fr = []
        for p in range(nb * nb):
            e = t[n * nb * nb + p]
            fr.append([(int(c), float(f)) for c, f in zip(e['op'], e['factor']) if c != AUG_NONE])
        out.append(fr)
    return out


def test_block_and_graded_constructors():
    cj = ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.8, block=2)
    assert cj.block == 2 and cj.n_seqblock == 16 and not cj.grad_consistent
    cj = ColorJitter(0.8, 0.8, 0.8, hue=0.2, grad_consistent=True, seq_len=8)
    assert cj.grad_consistent and cj.seq_len == 8 and cj.block == 1


def test_patch_table_shapes_and_gate_frequency():
    _seed(3)
    N, nb, H = 8, 3, 112
    st = ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.5, block=nb)(_clip(N, H))
    rows = st.rows(H, H)
    assert rows.shape == (N,) and not rows['op'].any() and not rows['factor'].any()     # geometry only
    t = st.patch_rows(H, H)
    assert t.dtype == AUG_PATCH and AUG_PATCH.itemsize == 40 and t.shape == (N * nb * nb,)
    on = total = 0
    for _ in range(60):
        lists = _lists(ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.5, block=nb)(_clip(N, H)).patch_rows(H, H), N, nb)
        for fr in lists:
            for ops in fr:
                total += 1
                if ops:
                    assert sorted(c for c, _ in ops) == sorted(FOUR)
                    on += 1
    assert total == 60 * N * nb * nb
    assert abs(on / total - 0.5) < 0.04, on / total                   # 4320 Bernoulli(0.5) draws: sd 0.0076


def test_redraw_frequency_consistent_and_n_seqblock():
    _seed(5)
    N, nb = 8, 2
    free = _lists(ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=nb)(_clip(N)).patch_rows(112, 112), N, nb)
    assert all(free[n] != free[n + 1] for n in range(N - 1))                # a fresh draw for every frame
    one = _lists(ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=nb, consistent=True, seq_len=N)(_clip(N)).patch_rows(112, 112),
                 N, nb)
    assert all(one[n] == one[0] for n in range(N))                          # consistent: one draw per clip
    assert one[0][0] != one[0][1]                                           # ... but one per patch
    four = _lists(ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=nb, consistent=True, seq_len=N, n_seqblock=4)(_clip(N))
                  .patch_rows(112, 112), N, nb)
    assert all(four[n] == four[0] for n in range(4)) and all(four[n] == four[4] for n in range(4, 8)) and four[0] != four[4]


def _ref_block_draws(cj, N):
    """utils/augmentation.py:ColorJitter.__call__ (:587-600, non-graded): per frame (unless consistent and idx % n_seqblock),
    the list comprehension over patches -- np.random.uniform(0., 1.) < p, then get_params (:482-510): random.uniform for
    brightness, contrast, saturation, hue, then random.shuffle"""
    out = []
    for idx in range(N):
        if not cj.consistent or idx % cj.n_seqblock == 0:
            cur = []
            for _ in range(cj.block * cj.block):
                if np.random.uniform(0., 1.) < cj.p:
                    ops = [(c, random.uniform(*r)) for c, r in zip(FOUR, (cj.brightness, cj.contrast, cj.saturation, cj.hue))]
                    random.shuffle(ops)
                    cur.append(ops)
                else:
                    cur.append([])
        out.append(cur)
    return out


def _ref_graded_draws(cj, N):
    """:602-611 -- per seq_len frames, per patch: get_grad_consistent_factors (:512-525, start then end for each of the four ops)
    and random.shuffle([0, 1, 2, 3]); frame t runs get_params_fixed (:528-551) on np.linspace(start, end, seq_len)[t]"""
    out = []
    for idx in range(N):
        if idx % cj.seq_len == 0:
            blocks = []
            for _ in range(cj.block * cj.block):
                fac = np.stack([np.linspace(random.uniform(*r), random.uniform(*r), cj.seq_len)
                                for r in (cj.brightness, cj.contrast, cj.saturation, cj.hue)], axis=1)
                order = [0, 1, 2, 3]
                random.shuffle(order)
                blocks.append((fac, order))
        out.append([[(FOUR[i], fac[idx % cj.seq_len, i]) for i in order] for fac, order in blocks])
    return out


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for gp, wp in zip(g, w):
            assert [c for c, _ in gp] == [c for c, _ in wp]
            assert [f for _, f in gp] == [float(np.float32(f)) for _, f in wp]


@pytest.mark.parametrize('kw', [dict(block=2), dict(block=3, p=0.5), dict(block=2, consistent=True, seq_len=8, n_seqblock=2),
                                dict(block=2, grad_consistent=True, seq_len=8), dict(block=1, grad_consistent=True, seq_len=8),
                                dict(block=3, grad_consistent=True, seq_len=4)])
def test_draws_follow_the_reference_sequence(kw):
    N = 8
    cj = ColorJitter(0.8, 0.8, 0.8, hue=0.2, **{'p': 0.8, **kw})
    for s in (0, 1, 17):
        st = _clip(N)
        _seed(s)
        got = _lists(cj(st).patch_rows(112, 112), N, cj.block)
        after = (random.random(), float(np.random.uniform()))              # both streams left where the reference leaves them
        _seed(s)
        want = (_ref_graded_draws if cj.grad_consistent else _ref_block_draws)(cj, N)
        _same(got, want)
        assert after == (random.random(), float(np.random.uniform()))


def test_graded_mode_all_four_ops_one_order_linspace():
    _seed(11)
    N, nb, L = 8, 2, 8
    cj = ColorJitter(0.8, 0.8, 0.8, hue=0.2, block=nb, grad_consistent=True, seq_len=L)
    st = _clip(N)
    _seed(11)
    st = cj(st)
    lists = _lists(st.patch_rows(112, 112), N, nb)
    _seed(11)
    for p in range(nb * nb):
        start_end = [(random.uniform(*r), random.uniform(*r)) for r in (cj.brightness, cj.contrast, cj.saturation, cj.hue)]
        order = [0, 1, 2, 3]
        random.shuffle(order)
        for n in range(N):
            assert [c for c, _ in lists[n][p]] == [FOUR[i] for i in order]          # all four, one order per clip and patch
            for c, f in lists[n][p]:
                s, e = start_end[FOUR.index(c)]
                assert f == np.linspace(s, e, L).astype(np.float32)[n]
    # the gate p is not used: no draw from numpy's stream
    _seed(11)
    np_state = np.random.get_state()[1].copy()
    cj(_clip(N))
    assert np.array_equal(np.random.get_state()[1], np_state)


def test_reference_class_draws_through_the_harness(monkeypatch):
    """the reference's own ColorJitter (imported through oracle.harness; its torchvision calls replaced by recorders) draws what
    the host class draws: get_grad_consistent_factors directly, and __call__'s per-patch op lists and factors"""
    from oracle import harness
    if not harness.available():
        pytest.skip('reference tree not present')
    import sys
    RA = harness.load_reference().augmentation
    N, H = 8, 112
    # get_grad_consistent_factors itself
    kw = dict(brightness=0.8, contrast=0.8, saturation=0.8, hue=0.2)
    ref = RA.ColorJitter(**kw, seq_len=N, grad_consistent=True, block=2)
    _seed(4)
    want = ref.get_grad_consistent_factors()
    _seed(4)
    got = ColorJitter(0.8, 0.8, 0.8, hue=0.2, seq_len=N, grad_consistent=True, block=2)._grad_factors()
    assert np.array_equal(got, want)
    # __call__ on [3, H, W] frames: record every adjust_* call (name, factor, patch slice shape) in order
    calls = []
    tvt = sys.modules['torchvision.transforms']
    monkeypatch.setattr(tvt, 'Lambda', lambda f: f, raising=False)
    monkeypatch.setattr(tvt, 'Compose', lambda fs: (lambda img: [img := f(img) for f in fs] and img), raising=False)
    for name, code in (('adjust_brightness', AUG_BRIGHTNESS), ('adjust_contrast', AUG_CONTRAST),
                       ('adjust_saturation', AUG_SATURATION), ('adjust_hue', AUG_HUE)):
        monkeypatch.setattr(RA.F, name, (lambda c: lambda img, f: calls.append((c, f, tuple(img.shape))) or img)(code), raising=False)
    for kw2 in (dict(block=3, p=0.8), dict(block=2, p=0.8, consistent=True, n_seqblock=4), dict(block=3, grad_consistent=True)):
        for s in (0, 9):
            calls.clear()
            _seed(s)
            RA.ColorJitter(**kw, seq_len=N, **kw2)([torch.zeros(3, H, H) for _ in range(N)])
            cj, st = ColorJitter(0.8, 0.8, 0.8, hue=0.2, seq_len=N, **kw2), _clip(N, H)
            _seed(s)
            lists = _lists(cj(st).patch_rows(H, H), N, cj.block)
            flat = [(c, f) for fr in lists for ops in fr for c, f in ops]
            assert [c for c, _, _ in calls] == [c for c, _ in flat]
            assert [float(np.float32(f)) for _, f, _ in calls] == [f for _, f in flat]
            nb, u = cj.block, H // cj.block                                # patch shapes: H // b, remainder to the last
            shapes = [(3, u if p // nb < nb - 1 else H - (nb - 1) * u, u if p % nb < nb - 1 else H - (nb - 1) * u)
                      for fr in lists for p, ops in enumerate(fr) for _ in ops]
            assert [sh for _, _, sh in calls] == shapes


def test_refusals():
    with pytest.raises(ValueError, match='mutually exclusive'):
        ColorJitter(0.8, 0.8, 0.8, hue=0.2, consistent=True, grad_consistent=True)
    with pytest.raises(ValueError, match='need a range'):
        ColorJitter(0.8, 0.8, 0.8, grad_consistent=True)                    # hue None: the reference would crash
    with pytest.raises(ValueError, match='need a range'):
        ColorJitter(0, 0.8, 0.8, hue=0.2, grad_consistent=True, block=2)
    for b in (0, 9, 2.0):
        with pytest.raises(ValueError, match='block'):
            ColorJitter(0.8, 0.8, 0.8, block=b)
    with pytest.raises(ValueError, match='n_seqblock'):
        ColorJitter(0.8, 0.8, 0.8, block=2, seq_len=8, n_seqblock=3)
    # geometry after a patched jitter stays refused, as after any colour op
    cj = ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=2)
    for after in (T.RandomCrop((64, 64)), T.Resize((64, 64)), T.RandomHorizontalFlip(p=1.0), cj):
        _seed(0)
        with pytest.raises(ValueError):
            after(cj(_clip()))
    # per patch: at most five ops and one contrast
    _seed(0)
    st = T.RandomGray(p=1.0)(T.RandomGray(p=1.0)(cj(_clip())))
    with pytest.raises(ValueError, match='per patch'):
        st.patch_rows(112, 112)
    _seed(0)
    st = cj(ColorJitter(0, 0.5, 0, p=1.0)(_clip()))
    with pytest.raises(ValueError, match='one contrast'):
        st.patch_rows(112, 112)
    # a grid that does not fit, a clip jittered on another grid
    _seed(0)
    with pytest.raises(ValueError):
        ColorJitter(0.8, p=1.0, block=8)(_clip(crop=6)).patch_rows(6, 6)
    _seed(0)
    with pytest.raises(ValueError, match='grid'):
        cj(_clip()).patch_rows(112, 112, block=3)


def test_gray_after_the_patched_jitter_joins_every_patch():
    _seed(2)
    N, nb = 8, 2
    st = T.RandomGray(p=0.5)(ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=nb)(_clip(N)))
    gray = st.ops[0][1]
    assert gray.any() and not gray.all()
    lists = _lists(st.patch_rows(112, 112), N, nb)
    for n in range(N):
        for ops in lists[n]:
            assert len(ops) == 4 + int(gray[n]) and (ops[-1][0] == AUG_GRAY) == bool(gray[n])


def test_entry_refuses_bad_grids_without_gpu():
    """dv_augment_ingest_blocks rejects its grid arguments before anything is launched (no device pointer is read)"""
    from dualvar_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)

    def call(patches, nb, H=112, W=112, N=1):
        return lib.dv_augment_ingest_blocks(0, fake, 1, 128, 171, fake, N, 8, H, W, fake, 4, 0, None, None, None, 0, fake, None,
                                            None, patches, nb, None)
    assert call(fake, 0) == -1
    assert call(fake, 9) == -1
    assert call(fake, 5, H=4) == -1 and call(fake, 5, W=4) == -1
    assert call(None, 2) == -1
    assert call(fake, 2, H=0) == -1                                          # the ordinary checks still apply
    assert call(fake, 8, N=1 << 23) == -1                                    # N*T fits, N*T*64 contrast workgroups do not


def _default_args(*extra):
    return pretrain.parse_args(['--net', 's3dg', '--model', 'simclr_naked', '--batch_size', '4', '--seq_len', '8', '--img_dim', '112',
                                '--dataset', 'synthetic-frames'] + list(extra))


@pytest.mark.parametrize('extra', [[], ['--rand_flip'], ['--aug_temp_consist']])
def test_gpu_transform_default_flags_are_todays_composition(extra):
    a = _default_args(*extra)
    todays = [T.RandomCrop((112, 112))] + ([T.RandomHorizontalFlip()] if '--rand_flip' in extra else []) + [
        T.ColorJitter(0.8, 0.8, 0.8, consistent='--aug_temp_consist' in extra, p=0.8 * 0.8, hue=0.2),
        T.RandomApply([T.GaussianBlur([.1, 2.], seq_len=8)], p=0.5)]
    fr = torch.zeros(16, 128, 171, 3, dtype=torch.uint8)
    clips = [list(range(8)), list(range(8, 16))]
    _seed(21)
    got = FrameBatch.build(fr, clips, pretrain.gpu_transform(a), (112, 112), views=2, device='cpu')
    _seed(21)
    want = FrameBatch.build(fr, clips, T.Compose(todays), (112, 112), views=2, device='cpu')
    assert got.patches is None and torch.equal(got.table, want.table)
    assert (got.blur is None) == (want.blur is None) and (got.blur is None or torch.equal(got.blur, want.blur))


def test_cli_flags_build_the_reference_structure():
    tr = pretrain.gpu_transform(_default_args('--n_block', '4', '--aug_temp_grad_consist'))
    ra = tr.transforms[1]
    assert isinstance(ra, T.RandomApply) and ra.p == 0.8
    cj = ra.transforms[0]
    assert (cj.block, cj.seq_len, cj.grad_consistent, cj.consistent, cj.p) == (4, 8, True, False, 0.8)
    assert cj.brightness == [0.19999999999999996, 1.8] and cj.hue == [-0.2, 0.2]
    with pytest.raises(SystemExit):
        _default_args('--aug_temp_consist', '--aug_temp_grad_consist')


def test_framebatch_carries_patches():
    N, nb = 8, 2
    cj = T.Compose([T.RandomCrop((64, 64)), ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=1.0, block=nb)])
    fr = torch.zeros(24, 128, 171, 3, dtype=torch.uint8)
    clips = [list(range(0, 8)), list(range(8, 16)), list(range(16, 24))]
    _seed(1)
    fb = FrameBatch.build(fr, clips, cj, (64, 64), views=2, device='cpu')
    per_view = N * nb * nb * AUG_PATCH.itemsize
    assert fb.n_block == nb and fb.patches.numel() == 3 * 2 * per_view
    v1 = fb[:, 1]
    assert v1.n_block == nb and torch.equal(v1.patches.view(3, -1), fb.patches.view(3, 2, -1)[:, 1])
    flat = fb.reshape(-1, 3, 8, 64, 64)
    assert flat.shape[0] == 6 and flat.patches is fb.patches and flat.n_block == nb
    both = FrameBatch.cat([v1, v1])
    assert both.shape[0] == 6 and torch.equal(both.patches, torch.cat([v1.patches, v1.patches]))
    plain = FrameBatch.build(fr, clips, T.RandomCrop((64, 64)), (64, 64), device='cpu')
    assert plain.patches is None and plain.n_block == 1
    with pytest.raises(ValueError):
        FrameBatch.cat([plain, v1])
    with pytest.raises(ValueError):
        FrameBatch(fr, v1.table, v1.shape, patches=v1.patches, n_block=3)
    # a clip that RandomApply left alone repeats its frame ops in every patch of the batch's grid
    _seed(0)
    st = T.RandomCrop((64, 64))(ClipState(range(8), 128, 171))
    st = T.RandomGray(p=1.0)(st)
    t = st.patch_rows(64, 64, block=nb)
    assert (t['op'][:, 0] == AUG_GRAY).all() and (t['op'][:, 1:] == 0).all()


def test_worker_rows_carry_patches_through_collate():
    a = _default_args('--n_block', '2', '--aug_temp_grad_consist', '--rand_flip')
    tr = pretrain.gpu_transform(a)
    ds = pretrain.SyntheticFrames(a, 16, transform=tr, views=2)
    _seed(7)
    batch = pretrain.collate_frames([ds[i] for i in range(4)])
    assert batch['patch'].shape == (4, 2 * 8 * 4 * AUG_PATCH.itemsize) and batch['patch'].dtype == torch.uint8
    fr = batch['frames']
    _seed(7)
    ref = FrameBatch.build(fr.view(-1, 128, 171, 3), [list(range(b * 8, b * 8 + 8)) for b in range(4)], tr, (112, 112), views=2,
                           device='cpu')
    assert ref.patches is not None and ref.n_block == 2
    assert torch.equal(batch['aug'].view(-1), ref.table.view(-1)) and torch.equal(batch['patch'].view(-1), ref.patches.view(-1))
    got = FrameBatch(fr.view(-1, 128, 171, 3), batch['aug'].view(-1), (4, 2, 3, 8, 112, 112), patches=batch['patch'].view(-1),
                     n_block=a.n_block)
    assert got.n_block == 2 and torch.equal(got.patches, ref.patches)
    # default flags: no patch rows at all
    plain = pretrain.SyntheticFrames(_default_args(), 16, transform=pretrain.gpu_transform(_default_args()), views=2)
    assert 'patch' not in plain[0]
