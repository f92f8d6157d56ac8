"""CPU: the host side of the downstream driver -- the finetune / test samplers and datasets (dualvar_amd/utils/finetune_dataset.py)
against tests/golden/finetune_sampling.npz and, where the reference tree is present, against the reference's own classes; the
(flip, crop) view rows against the PIL pipeline bit for bit; classifier.py's command line and refusals; the interchange of
dualvar_amd.optim.Adam's state with torch.optim.Adam."""
import copy
import glob
import os
import random
import shlex
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import pretrain  # noqa: F401            before oracle.harness puts the reference tree in front on sys.path
import classifier as CLI
from dualvar_amd.utils import finetune_dataset as FD
from dualvar_amd.utils import resample as R
from dualvar_amd.utils import transforms as T
from tests.dataset_support import _rng_state, _seed, ref, write_dataset  # noqa: F401  (ref: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _sampler(cls, num_frames, ds, mode):
    d = object.__new__(cls)
    d.__dict__.update(num_frames=num_frames, ds=ds, mode=mode)
    return d


MODES = (('train', FD.FinetuneFrames, 'train'), ('test', FD.FinetuneFrames, 'test'), ('10clip', FD.TenClipFrames, 'test'))


def test_samplers_against_fixture():
    g = np.load(os.path.join(GOLD, 'finetune_sampling.npz'), allow_pickle=False)
    cases = g['cases'].tolist()
    assert len(cases) >= 20 and any(v <= n * d for v, n, d, _ in cases) and any(v > n * d for v, n, d, _ in cases)
    for k, (vlen, nf, ds, seed) in enumerate(cases):
        for mode, cls, dmode in MODES:
            random.seed(seed)
            np.random.seed(seed)
            idx = np.asarray(_sampler(cls, nf, ds, dmode).sample_indices(vlen)).reshape(-1)
            want = g['%s/%d' % (mode, k)]
            assert idx.tolist() == want.tolist(), (mode, vlen, nf, ds, seed)
            assert [random.random(), np.random.random()] == g['%s/rng/%d' % (mode, k)].tolist(), ('rng', mode, vlen, nf, ds, seed)
            assert 0 <= idx.min() and idx.max() < vlen
            if mode == 'train':
                assert len(idx) == nf
            elif mode == '10clip':
                assert len(idx) == 10 * nf
            elif vlen > nf * ds:                 # half-overlapping windows, step num_frames * ds // 2 - 1
                n_win = len(range(0, vlen - nf * ds + 1, nf * ds // 2 - 1))
                assert len(idx) == n_win * nf and (n_win == 1 or idx[nf] - idx[0] == nf * ds // 2 - 1)
            else:
                assert len(idx) == nf


def test_getitem_order_against_reference(ref, tmp_path, monkeypatch):
    """the frame files the reference's UCF101LMDB (train, test) and UCF101_10CLIP open, and the RNG state they leave, against
    ours, for a short video (vlen <= num_frames * ds) and a long one"""
    LD, _ = ref
    split, frame = write_dataset(str(tmp_path), videos=((0, 9), (1, 70)), rows=810)
    for ds_ in (1, 4):
        for mode, cls, dmode in MODES:
            mine = cls(split, frame, mode=dmode, num_frames=16, ds=ds_)
            mine.mode = 'train' if mode == 'train' else dmode
            theirs = object.__new__(LD.UCF101_10CLIP if mode == '10clip' else LD.UCF101LMDB)
            opened = []

            def record(seq):
                opened.append([os.path.relpath(im.filename, frame) for im in seq])
                return [torch.zeros(1) for _ in seq]
            theirs.__dict__.update(num_frames=16, ds=ds_, transform=record, return_label=False, db_path=frame,
                                   video_subset=mine.video_subset, mode=mine.mode)
            for idx in (0, 1):
                for seed in range(3):
                    _seed(seed)
                    theirs[idx]
                    after = _rng_state()
                    _seed(seed)
                    s = mine[idx]
                    assert _rng_state() == after, (mode, ds_, idx, seed)
                    vname = mine.video_subset.iloc[idx][3]
                    assert opened[-1] == [os.path.relpath(mine.frame_path(vname, i), frame) for i in s['frame_index'].tolist()]
                    assert len(s['decoded']) == len(set(s['frame_index'].tolist()))       # each distinct frame decoded once


def test_transform_draws_against_reference(ref):
    """RandomCrop -> RandomHorizontalFlip(consistent=False, seq_len) of classifier.py:1008-1016 on PIL images whose pixels hold
    (x, y, frame) against the table rows: the same window and orientation per frame, the same RNG state"""
    _, RA = ref
    W, H, L = 170, 128, 32
    yy, xx = np.mgrid[0:H, 0:W]
    src = [np.stack([xx, yy, np.full_like(xx, i)], -1).astype(np.uint8) for i in range(L)]
    imgs = [Image.fromarray(a) for a in src]
    flips = set()
    for seed in range(8):
        _seed(seed)
        out = RA.RandomHorizontalFlip(consistent=False, seq_len=16)(RA.RandomCrop(112)(imgs))
        after = _rng_state()
        _seed(seed)
        st = FD.finetune_transform('train', 112, 16, rand_flip=True)(T.ClipState(range(L), H, W))
        assert _rng_state() == after
        rows = st.rows(112, 112)
        for r, o in zip(rows, out):
            win = src[r['src']][r['crop_i']:r['crop_i'] + r['crop_h'], r['crop_j']:r['crop_j'] + r['crop_w']]
            assert np.array_equal(win[:, ::-1] if r['flip'] else win, np.asarray(o)), (seed, int(r['src']))
        flips.add((int(rows['flip'][0]), int(rows['flip'][16])))
    assert len(flips) >= 3                      # the two blocks of a clip are flipped independently, both ways seen


def test_splits_and_getitem_on_a_tree(tmp_path):
    split, frame = write_dataset(str(tmp_path), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(240, 320), (120, 90), (101, 163)])
    tf = FD.finetune_transform('train', 64, 8, rand_flip=True, with_color_jitter=True)
    tr = FD.build_dataset('ucf101', split, frame, mode='train', num_frames=8, ds=2, transform=tf, img_dim=64, scale=72)
    va = FD.build_dataset('ucf101', split, frame, mode='val', num_frames=8, ds=2, transform=FD.finetune_transform('val', 64, 8), img_dim=64, scale=72)
    te = FD.build_dataset('hmdb51', split, frame, mode='test', num_frames=8, ds=2, img_dim=64, scale=72, views=FD.CROP_VIEWS['ten'])
    tc = FD.build_dataset('ucf101-10clip', split, frame, mode='test', num_frames=8, ds=2, transform=FD.finetune_transform('test', 64, 8),
                          img_dim=64, scale=72)
    assert (len(tr), len(va), len(te), len(tc)) == (30, 800, 3, 3) and isinstance(tc, FD.TenClipFrames)
    with pytest.raises(ValueError, match='unknown dataset'):
        FD.build_dataset('k400', split, frame)
    _seed(0)
    s = tr[0]
    assert s['aug'].shape == (8,) and s['patch'].shape == (8,) and s['vid'] in (0, 1) and s['vname'].count('/') == 1
    assert set(s['aug']['crop_h'].tolist()) == {64} and len(set(s['aug']['flip'].tolist())) == 1
    s = va[0]
    assert 'patch' not in s and s['aug']['flip'].sum() == 0
    # the three test videos: 40 frames of 240x320 -> 72x96, 9 frames of 120x90 -> 96x72, 70 frames of 101x163 -> 72x116
    sizes, n_win = [(72, 96), (96, 72), (72, 116)], [len(range(0, 40 - 16 + 1, 7)), 1, len(range(0, 70 - 16 + 1, 7))]
    samples = [te[i] for i in range(3)]
    for s, sz, nw in zip(samples, sizes, n_win):
        assert s['size'] == sz and s['aug'].shape == (10 * nw * 8,)
        assert s['aug']['flip'].reshape(10, -1).tolist() == [[0] * (nw * 8)] * 5 + [[1] * (nw * 8)] * 5
    assert tc[1]['aug'].shape == (80,) and tc[2]['frame_index'].max() <= 69
    batch = FD.collate_finetune(samples)
    assert [g[0] for g in batch['groups']] == sizes and batch['n_rows'] == [len(s['aug']) for s in samples]
    assert batch['vid'].tolist() == [0, 0, 1] and batch['vpath'][2].endswith('v_Jump_g02/')
    rows = batch['aug'].numpy().view(T.AUG_ROW)
    n0, n1 = len(samples[0]['decoded']), len(samples[1]['decoded'])
    assert rows['src'][:len(samples[0]['aug'])].max() == n0 - 1 and rows['src'][len(samples[0]['aug'])] >= n0
    assert batch['n_frames'] == n0 + n1 + len(samples[2]['decoded'])
    for g, (sz, pos, desc, coef) in enumerate(batch['groups']):
        assert len(desc) == len(pos) and batch['src%d' % g].dtype == torch.uint8


def _pil_view(frame, scale, size, flip, where):
    """RandomHorizontalFlip(command) -> Scale -> FiveCrop(where) as the reference's classes compute them (where = 4 repaired)"""
    im = Image.fromarray(frame)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    w, h = im.size
    if isinstance(scale, int):
        if not ((w <= h and w == scale) or (h <= w and h == scale)):
            im = im.resize((scale, int(scale * h / w)) if w < h else (int(scale * w / h), scale), Image.BICUBIC)
    else:
        im = im.resize(scale, Image.BICUBIC)
    w, h = im.size
    th = tw = size
    box = {1: (0, 0, tw, th), 2: (w - tw, 0, w, th), 3: (0, h - th, tw, h), 4: (w - tw, h - th, w, h),
           5: (int(round((w - tw) / 2.)), int(round((h - th) / 2.)), int(round((w - tw) / 2.)) + tw, int(round((h - th) / 2.)) + th)}[where]
    return np.asarray(im.crop(box))


@pytest.mark.parametrize('scale', [128, (128, 171)])
def test_crop_view_rows_equal_the_pil_pipeline(scale):
    r = np.random.RandomState(3)
    for H, W in [(240, 320), (360, 240), (101, 163), (128, 200), (131, 129), (240, 426), (113, 112)]:
        frame = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
        h, w = FD.scaled_size(H, W, scale)
        if isinstance(scale, int):
            assert min(h, w) == scale or (h, w) == (H, W)
            assert (h, w) == ((int(scale * H / W), scale) if W < H else (scale, int(scale * W / H))) or min(H, W) == scale
        else:
            assert (h, w) == (171, 128)
        scaled = R.resize_u8(frame, (h, w))
        rows = FD.view_rows([0], h, w, 112, FD.CROP_VIEWS['ten'])
        assert [(int(x['flip']), k) for x, k in zip(rows, [5, 1, 2, 3, 4] * 2)] == FD.CROP_VIEWS['ten']
        for row, (flip, where) in zip(rows, FD.CROP_VIEWS['ten']):
            win = scaled[row['crop_i']:row['crop_i'] + row['crop_h'], row['crop_j']:row['crop_j'] + row['crop_w']]
            assert win.shape == (112, 112, 3)
            got = win[:, ::-1] if row['flip'] else win
            assert np.array_equal(got, _pil_view(frame, scale, 112, flip, where)), (H, W, flip, where)
    assert FD.CROP_VIEWS['center'] == [(0, 5)] and FD.CROP_VIEWS['five'] == FD.CROP_VIEWS['ten'][:5]
    with pytest.raises(ValueError, match='bigger than input'):
        FD.view_rows([0], 100, 200, 112, FD.CROP_VIEWS['center'])
    assert FD.scale_arg(128, 112, True) == (128, 171) and FD.scale_arg(128, 224, True) == 128 and FD.scale_arg(256, 112, False) == 256


FINETUNE = ('--prefix p --name_prefix e --net r21d --model linclr --dataset ucf101 --which_split 1 --train_what ft --seq_len 16 '
            '--num_seq 1 --epochs 150 --schedule 50 100 --optim adam --img_dim 112 --img_resize_dim 128 --aug_crop --rand_flip '
            '--with_color_jitter -j 4 --lr 0.05 --wd 0.001 --batch_size 4 --print_freq 100 --eval_freq 1 --save_freq 1 --ds 2 '
            '--pretrain log/x/model/epoch189.pth.tar --steps 3 --seed 1 --dtype bf16 --split_root s --frame_root f')
TENCLIP = ('--model linclr --net r21d --dataset ucf101-10clip --seq_len 16 --batch_size 8 --temporal_ten_clip --num_seq 10 -j 8 '
           '--gpu 0 --ds 2 --aug_crop --rand_flip --test log/x/ft/e/ucf/model/epoch149.pth.tar')
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --aug_crop '
             '--rand_flip --retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')


def test_parse_args_and_checks():
    a = CLI.parse_args([])
    assert (a.net, a.model, a.train_what, a.dropout, a.dataset, a.seq_len, a.num_seq, a.ds, a.batch_size, a.img_resize_dim, a.img_dim,
            a.optim, a.lr, a.schedule, a.wd, a.epochs, a.print_freq, a.eval_freq, a.save_freq, a.prefix, a.workers, a.world_size,
            a.local_rank, a.steps, a.seed, a.dtype) == \
        ('myrealr21d', 'linclr', 'ft', 1.0, 'ucf101', 16, 1, 4, 32, 128, 112, 'sgd', 5e-2, [10, 20, 30, 40], 1e-4, 50, 5, 1, 10,
         'linclr', 8, -1, -1, 0, 0, 'fp32')
    a = CLI.parse_args(shlex.split(FINETUNE))
    assert a.optim == 'adam' and a.schedule == [50, 100] and a.with_color_jitter and a.steps == 3 and a.dtype == 'bf16'
    CLI.check_args(a, environ={})
    a = CLI.parse_args(shlex.split(TENCLIP))
    assert a.temporal_ten_clip and a.num_seq == 10 and a.gpu == 0
    CLI.check_args(a, environ={})
    a = CLI.parse_args(shlex.split(RETRIEVAL))
    assert a.retrieval and a.test.endswith('epoch189.pth.tar')
    CLI.check_args(a, environ={})


def test_crop_views_ignore_aug_crop_as_the_reference_does(tmp_path):
    """test_10crop builds its own transform with A.Scale(img_resize_dim) (classifier.py:589-600): --aug_crop changes the 10-clip
    and retrieval passes and the train / val transforms, not the crop views; retrieval reads split 1 whatever --which_split"""
    split, frame = write_dataset(str(tmp_path), videos=((0, 20), (1, 20)), rows=810, sizes=[(240, 320), (240, 320)])
    a = CLI.parse_args(['--aug_crop', '--img_dim', '112', '--img_resize_dim', '128', '--split_root', split, '--frame_root', frame,
                        '--seq_len', '8', '--ds', '1'])
    crop = CLI.get_data('test', a, views=FD.CROP_VIEWS['ten'])
    assert crop.scale == 128 and crop[0]['size'] == (128, 170)
    a.img_resize_dim = 136
    assert CLI.get_data('test', a, views=FD.CROP_VIEWS['center']).scale == 136
    for mode in ('train', 'val', 'test'):
        assert CLI.get_data(mode, a).scale == (128, 171) and CLI.get_data(mode, a)[0]['size'] == (171, 128)
    assert CLI.get_data('test', a, dataset='ucf101-10clip').scale == (128, 171)
    a.which_split = 3
    assert CLI.get_data('train', a, dataset='ucf101-10clip', transform_mode='test', which_split=1).scale == (128, 171)
    with pytest.raises(FileNotFoundError):
        CLI.get_data('test', a)                 # split 3 does not exist on this tree: which_split is honoured elsewhere


def test_parse_args_accepts_every_paper_script():
    from oracle import harness
    if not harness.available():
        pytest.skip('reference tree not present')
    scripts = [f for f in glob.glob(os.path.join(harness.REFERENCE_ROOT, 'paper_scripts', '*', '*', '*.sh'))
               if 'classifier.py' in open(f).read()]
    assert len(scripts) >= 20
    kinds = set()
    for f in scripts:
        text = open(f).read().replace('\\\n', ' ')
        for line in text.splitlines():
            if 'classifier.py' not in line:
                continue
            words = shlex.split(line.split('classifier.py', 1)[1].replace('${exp_name}', 'e').replace('$1', '0'))
            a = CLI.parse_args(words)
            kinds.add('retrieval' if a.retrieval else 'tenclip' if a.temporal_ten_clip else 'test' if a.test else 'finetune')
            CLI.check_args(a, environ={})          # single process: the launcher's WORLD_SIZE is what is refused, not the flags
    assert {'retrieval', 'tenclip', 'finetune'} <= kinds


@pytest.mark.parametrize('argv,env,word', [
    (FINETUNE, {'WORLD_SIZE': '4'}, 'distributed'),
    (FINETUNE + ' --multiprocessing-distributed', {}, 'distributed'),
    (FINETUNE.replace('--num_seq 1', '--num_seq 2'), {}, 'num_seq'),
    (FINETUNE.replace('--dataset ucf101', '--dataset k400'), {}, 'dataset'),
    (TENCLIP.replace('--num_seq 10', '--num_seq 1'), {}, 'num_seq 10'),
    (TENCLIP.replace('--dataset ucf101-10clip', '--dataset ucf101'), {}, 'ucf101-10clip'),
])
def test_refusals_exit_with_one_line(argv, env, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created


def test_adam_state_interchanges_with_torch_adam():
    """torch.optim.Adam's state loads into the moment arenas through the parameter views and back, 'step' as a tensor or as the
    int of torch 1.8; a mismatch leaves the optimizer as it was; missing moments are reported"""
    from dualvar_amd.model import LinearClassifier
    from dualvar_amd.ops import DV_F32
    from dualvar_amd.optim import Adam
    torch.manual_seed(0)
    c = LinearClassifier(num_class=10, network='r3d', use_dropout=False)
    with pytest.raises(ValueError, match='not materialised'):       # nowhere to load into yet: said, not skipped
        Adam(list(c.parameters()), stores=c.stores()).load_state_dict({'state': {}, 'param_groups': [{}]})
    with pytest.raises(ValueError, match='stores='):
        Adam(list(c.parameters()))
    for st in c.stores():
        st.materialize(torch.device('cpu'), DV_F32)
    params = list(c.parameters())
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.Adam([{'params': [q]} for q in twins], lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        for q in twins:
            q.grad = torch.randn(q.shape, generator=g)
        topt.step()
    for g_ in topt.param_groups:                                    # e.g. after adjust_learning_rate
        g_['lr'] = 1e-4
    opt = Adam([{'params': [p]} for p in params], lr=0.5, betas=(0.5, 0.5), stores=c.stores())
    assert opt.state_dict()['state'] == {}                          # as torch's before the first step
    assert opt.load_state_dict(topt.state_dict()) == len(params) and opt._step == 2
    assert all(g_['lr'] == 1e-4 and g_['betas'] == (0.9, 0.999) for g_ in opt.param_groups)
    st = c.stores()[0]
    m_arena, v_arena = opt._moments(st)
    for i, m, v in opt._moment_views():
        assert torch.equal(m, topt.state[twins[i]]['exp_avg']) and torch.equal(v, topt.state[twins[i]]['exp_avg_sq'])
        s = st.slot(params[i])                                      # ... and they sit where dv_adam addresses them
        assert m.data_ptr() == m_arena.data_ptr() + 4 * s.off and v.data_ptr() == v_arena.data_ptr() + 4 * s.off
    assert float(v_arena.min()) >= 0.0 and float(m_arena.min()) < 0.0
    step, nm, nv = opt.moment_summary()
    assert step == 2 and nm == pytest.approx(float(sum(topt.state[q]['exp_avg'].double().pow(2).sum() for q in twins)) ** 0.5, rel=1e-12)
    assert nv == pytest.approx(float(sum(topt.state[q]['exp_avg_sq'].double().pow(2).sum() for q in twins)) ** 0.5, rel=1e-12)
    # and back: torch's Adam takes our state_dict and steps on it
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and sd['param_groups'][3]['params'] == [3] and len(sd['state']) == len(params)
    topt2 = torch.optim.Adam([{'params': [q]} for q in twins], lr=0.3)
    topt2.load_state_dict(sd)
    for q in twins:
        assert torch.equal(topt2.state[q]['exp_avg_sq'], topt.state[q]['exp_avg_sq']) and float(topt2.state[q]['step']) == 2
        q.grad = torch.randn(q.shape, generator=g)
    topt2.step()
    assert topt2.param_groups[0]['lr'] == 1e-4 and float(topt2.state[twins[0]]['step']) == 3
    # torch 1.8 stores 'step' as an int
    sd8 = copy.deepcopy(topt.state_dict())
    for e in sd8['state'].values():
        e['step'] = 2
    assert opt.load_state_dict(sd8) == len(params) and opt._step == 2
    # validate everything, then mutate: a bad entry leaves moments, counter and groups as they were
    before = [x.clone() for x in opt._moments(st)]
    bad = copy.deepcopy(topt.state_dict())
    [g_.update(lr=7.0) for g_ in bad['param_groups']]
    bad['state'][5]['exp_avg'] = torch.zeros(3)
    with pytest.raises(ValueError, match='shape'):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(topt.state_dict())
    [g_.update(lr=7.0) for g_ in bad['param_groups']]
    bad['state'][5]['step'] = torch.tensor(9.)
    with pytest.raises(ValueError, match='one counter'):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(topt.state_dict())
    bad['param_groups'][1]['lr'] = 1e-3                              # step() uses one lr for every tensor: said, not ignored
    with pytest.raises(ValueError, match='different lr'):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(topt.state_dict())
    bad['state'][0] = {'momentum_buffer': torch.zeros_like(twins[0])}
    with pytest.raises(ValueError, match='not an Adam state'):
        opt.load_state_dict(bad)
    assert opt.param_groups[0]['lr'] == 1e-4 and opt._step == 2
    assert all(torch.equal(a, b) for a, b in zip(before, opt._moments(st)))
    # a state without moments (fresh torch optimizer) is loaded with a warning, not silently
    fresh = torch.optim.Adam([{'params': [q]} for q in twins], lr=0.1).state_dict()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        assert opt.load_state_dict(fresh) == 0 and opt._step == 0
    assert any('Adam moments restored' in str(x.message) for x in w)
    assert all(float(x.abs().sum()) == 0.0 for x in opt._moments(st))


def test_pretrain_optim_flag_parses():
    """what the flag selects is checked where it runs: tests/test_classifier_driver_gpu.py pretrains with --optim adam"""
    assert pretrain.parse_args(['--optim', 'adam']).optim == 'adam' and pretrain.parse_args([]).optim == 'sgd'
