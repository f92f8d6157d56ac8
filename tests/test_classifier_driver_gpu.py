"""GPU: the downstream driver (classifier.py) end to end.

  * three Adam steps of LinearClassifier on r3d against tests/golden/classifier_adam.npz (recorded from the reference by
    tools/gen_downstream_golden.py): losses and eval logits within max(1e-3, 5 * sens), the bounds of
    test_models_gpu.py::test_classifier_finetune_steps_against_reference_fixture.  Measured on an MI355X (|ours - reference|):
        ft    loss 4.8e-07 / 7.3e-06 / 1.3e-05    eval_logit 8.9e-04   (the reference's own fp32 vs fp64: 2.2e-05, 6.4e-04;
                                                                     its sens: 2.2e-05, 1.1e-03 -> bounds 1e-3, 5.5e-3)
        last  loss 7.2e-07 / 7.2e-07 / 7.2e-07    eval_logit 1.5e-07   (fp32 vs fp64: 4.1e-07, 1.2e-07; bounds 1e-3, 1e-3)
  * the ten (flip, crop) views of the crop test, on a generated JPEG tree with mixed frame sizes: the stem input of every view
    against Normalize(ToTensor(PIL pipeline)) computed on the CPU, within the F32_TOL of tests/test_frame_dataset_gpu.py
    (measured: max abs err 2.4e-07 over 130 clips).
  * validate and the crop / 10-clip summaries against a direct torch computation on the same logits (accuracies exactly).
  * classifier.py as a child process: finetune from a pretrain.py checkpoint (ft + SGD; last + Adam with --resume), then the
    ten-crop, temporal 10-clip and retrieval tests.  Every child has its own timeout; after a child failed, no further one starts.
"""
import json
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch
from PIL import Image

import pretrain  # noqa: F401
import classifier as CLI
from dualvar_amd import ops
from dualvar_amd.ops import DV_F32
from dualvar_amd.utils import finetune_dataset as FD
from tests.checks import child as _child
from tests.dataset_support import _seed, write_dataset
from tests.util import CLIP, gold

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
F32_TOL = 3e-5          # tests/test_frame_dataset_gpu.py: the bound of the same comparison (unblurred frames)


@pytest.mark.parametrize('mode,kw', [('ft', dict(use_dropout=False)),
                                     ('last', dict(use_dropout=True, use_l2_norm=True, use_final_bn=True))])
def test_classifier_adam_steps_against_reference_fixture(gpu, mode, kw):
    from dualvar_amd import functional as DF
    from dualvar_amd.model import LinearClassifier
    from dualvar_amd.optim import Adam
    from oracle import procedural as P
    g = gold('classifier_adam')
    c = LinearClassifier(num_class=10, network='r3d', **kw)
    P.procedural_init(c)
    c.set_compute_dtype('fp32').train().to(gpu)
    xa = P.procedural_clips(4, 1, **CLIP)[:, 0].to(gpu)
    xb = P.procedural_clips(4, 1, seed=77, **CLIP)[:, 0].to(gpu)
    labels = torch.tensor([3, 0, 2, 1], device=gpu)
    with torch.no_grad():
        c.backbone.forward_pooled(xa)
    if mode == 'last':
        for n_, p_ in c.named_parameters():
            if 'backbone' in n_:
                p_.requires_grad = False
    opt = Adam([{'params': [p_]} for p_ in c.parameters() if p_.requires_grad], lr=float(g[f'{mode}/lr']), weight_decay=1e-4,
               stores=c.stores())
    frozen0 = {k: v.clone() for k, v in c.state_dict().items() if 'backbone' in k and v.dtype.is_floating_point} if mode == 'last' else {}

    def bound(key):
        return max(1e-3, 5 * float(g[f'{mode}/sens/{key}']))
    dist = []
    for it in range(3):
        if mode == 'last':
            c.eval()
            c.final_bn.train()
        else:
            c.train()
        logit, _ = c(xb)
        loss, _ = DF.cross_entropy(logit, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        dist.append(abs(float(loss.detach()) - float(g[f'{mode}/loss{it}'])))
    with torch.no_grad():
        ev = c.eval()(xb)[0].cpu().numpy()
    d_ev = float(np.max(np.abs(ev - g[f'{mode}/eval_logit'])))
    print(f'    classifier adam {mode}: |loss - reference| ' + ' / '.join('%.1e' % d for d in dist) + f'   eval_logit {d_ev:.1e}'
          f'   (reference fp32 vs fp64: loss ' +
          '%.1e' % max(abs(float(g[f'{mode}/loss{i}']) - float(g[f'{mode}/f64/loss{i}'])) for i in range(3)) +
          ', eval_logit %.1e; sens loss %.1e, eval_logit %.1e)' % (
              float(np.max(np.abs(g[f'{mode}/eval_logit'] - g[f'{mode}/f64/eval_logit']))),
              max(float(g[f'{mode}/sens/loss{i}']) for i in range(3)), float(g[f'{mode}/sens/eval_logit'])))
    for it in range(3):
        assert dist[it] < bound(f'loss{it}'), (it, dist[it])
    assert d_ev < bound('eval_logit'), d_ev
    for k, v in frozen0.items():
        assert torch.equal(c.state_dict()[k], v), k
    assert opt._step == 3


# ------------------------------------------------------------------------------------------------------ crop views
def _pil_stem(path, scale, size, flip, where):
    """Normalize(ToTensor(RandomHorizontalFlip(command) -> Scale -> FiveCrop(where))) of one frame file -> [3, size, size]"""
    im = Image.open(path).convert('RGB')
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    w, h = im.size
    if not ((w <= h and w == scale) or (h <= w and h == scale)):
        im = im.resize((scale, int(scale * h / w)) if w < h else (int(scale * w / h), scale), Image.BICUBIC)
    w, h = im.size
    x1, y1 = int(round((w - size) / 2.)), int(round((h - size) / 2.))
    box = {1: (0, 0, size, size), 2: (w - size, 0, w, size), 3: (0, h - size, size, h), 4: (w - size, h - size, w, h),
           5: (x1, y1, x1 + size, y1 + size)}[where]
    x = torch.from_numpy(np.asarray(im.crop(box))).permute(2, 0, 1).float().div(255)
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def test_crop_views_stem_input_against_pil(gpu, tmp_path):
    T_, img, scale = 8, 64, 72
    split, frame = write_dataset(str(tmp_path), videos=((0, 40), (0, 9), (1, 70)), sizes=[(240, 320), (120, 90), (101, 163)])
    views = FD.CROP_VIEWS['ten']
    ds = FD.build_dataset('ucf101', split, frame, mode='test', num_frames=T_, ds=2, img_dim=img, scale=scale, views=views)
    _seed(0)
    samples = [ds[i] for i in range(3)]
    batch = FD.collate_finetune(samples)
    assert len(batch['groups']) == 3                                  # three scaled sizes: 72x96, 96x72, 72x116
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in batch.items()}
    fr = FD.scale_batch(dev)
    assert tuple(fr.shape[1:]) == (96, 116, 3)
    n_rows = sum(batch['n_rows'])
    N = n_rows // T_
    a = ops.new_act(N, T_, img, img, 3, DV_F32, gpu, cpitch=4, zero=True)
    ops.call('dv_augment_ingest', DV_F32, fr, fr.shape[0], fr.shape[1], fr.shape[2], dev['aug'].view(-1), N, T_, img, img, a, 4, 0,
             torch.tensor(MEAN).to(gpu), (1 / torch.tensor(STD)).to(gpu), None, 0, torch.empty(N * T_, device=gpu), None, None)
    torch.cuda.synchronize()
    got = ops.act_to_ncdhw(a).cpu()                                   # [N, 3, T, img, img]
    worst, clip = 0.0, 0
    for s in samples:
        idx = s['frame_index'].tolist()
        n_win = len(idx) // T_
        for flip, where in views:
            for w_ in range(n_win):
                for t in (0, T_ - 1):                                 # first and last frame of every window of every view
                    want = _pil_stem(ds.frame_path(s['vname'], idx[w_ * T_ + t]), scale, img, flip, where)
                    err = float((got[clip, :, t] - want).abs().max())
                    worst = max(worst, err)
                    assert err <= F32_TOL, (s['vname'], flip, where, w_, t, err)
                clip += 1
    assert clip == N
    print(f'    ten crop views, {N} clips of 3 videos with 3 scaled sizes: max abs err of the stem input {worst:.2e}')
    # the same batch as the driver feeds it: a FrameBatch of [N, 3, T, img, img]
    args = types.SimpleNamespace(seq_len=T_, img_dim=img)
    fb, n_clips = CLI.model_input(dev, args)
    assert n_clips == N and tuple(fb.shape) == (N, 3, T_, img, img) and fb.patches is None


# -------------------------------------------------------------------------------- validate and the summaries
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(str(s))


def _topk(prob, target, ks=(1, 5)):
    pred = prob.topk(max(ks), 1, True, True)[1]
    hit = pred.eq(target.view(-1, 1))
    return [float(hit[:, :k].any(1).float().mean()) for k in ks]


def test_validate_and_summaries_equal_torch(gpu, tmp_path, monkeypatch):
    gen = torch.Generator().manual_seed(0)
    K, B = 10, 6
    logits = [(torch.randn(B, K, generator=gen) * 3).to(gpu) for _ in range(5)]
    labels = [torch.randint(0, K, (B,), generator=gen).to(gpu) for _ in range(5)]
    loader = [{'vid': y, 'k': i} for i, y in enumerate(labels)]
    monkeypatch.setattr(CLI, 'model_input', lambda batch, args: (batch['k'], B))

    class Model:
        def eval(self):
            return self

        def __call__(self, k):
            return logits[k], None
    args = types.SimpleNamespace(gpu=0, steps=0, logger=_Log())
    loss, top1 = CLI.validate(loader, Model(), 0, args)
    want_loss = float(np.mean([float(torch.nn.functional.cross_entropy(lg, y)) for lg, y in zip(logits, labels)]))
    want_top1 = float(np.mean([_topk(lg, y)[0] for lg, y in zip(logits, labels)]))
    assert abs(loss - want_loss) < 1e-5 and top1 == pytest.approx(want_top1, abs=1e-7), (loss, want_loss, top1, want_top1)
    assert 'val Epoch: [0]' in args.logger.lines[-1] and 'Acc@5' in args.logger.lines[-1]
    args.steps = 2
    loss2, _ = CLI.validate(loader, Model(), 0, args)
    assert abs(loss2 - float(np.mean([float(torch.nn.functional.cross_entropy(lg, y)) for lg, y in zip(logits[:2], labels[:2])]))) < 1e-5
    # crop summary: three videos, ten views, 4 / 1 / 7 windows
    classes = ['Walk', 'Jump', 'Run']
    args = types.SimpleNamespace(test=str(tmp_path / 'epoch0.pth.tar'), logger=_Log())
    prob_dict, want = {}, {1: [], 5: [], 10: []}
    for v, n_win in enumerate((4, 1, 7)):
        lg = (torch.randn(10 * n_win, 3, generator=gen) * 2).to(gpu)
        vpath = '/data/frame/%s/v_%d/' % (classes[v], v)
        mp = CLI.group_probabilities(lg, 10)
        ref = torch.softmax(lg, -1).view(10, n_win, 3).mean(1)
        assert mp.shape == (10, 3) and float((mp - ref).abs().max()) < 1e-6
        prob_dict[vpath] = {'mean_prob': mp}
        for rows in want:
            want[rows].append(_topk(ref[:rows], torch.full((rows,), v, device=gpu), (1, 2)))
    for title, rows in (('center', 1), ('five', 5), ('ten', None)):
        acc = CLI.summarize_probability(prob_dict, classes.index, title, args, rows=rows)
        w = np.mean([x[0] for x in want[rows or 10]])
        assert acc[0].avg == pytest.approx(w, abs=1e-7) and acc[0].count == 3, (title, acc[0].avg, w)
        stat = json.load(open(str(tmp_path / ('epoch0.pth.tar-prob-%s.json' % title))))
        assert sorted(len(s['mean_prob']) for s in stat.values()) == [rows or 10] * 3
    # 10-clip test: two batches (4 and 3 videos) of [B * 10, K] logits, video-major, five classes of which one is met three times
    classes = ['Walk', 'Jump', 'Run', 'Sit', 'Dive']
    vids = [[0, 3, 1, 3], [2, 3, 4]]
    prob_dict, cls_dict, ref_mean, ref_vid = {}, {}, [], []
    for b, ids in enumerate(vids):
        lg = (torch.randn(len(ids) * 10, 5, generator=gen) * 2).to(gpu)
        batch = {'vpath': ['/data/frame/%s/v_%d_%d/' % (classes[c], b, i) for i, c in enumerate(ids)], 'vid': torch.tensor(ids)}
        mean = CLI.collect_ten_clip(lg, batch, lambda c: classes[c], prob_dict, cls_dict)
        ref = torch.softmax(lg, -1).view(len(ids), 10, 5).mean(1)
        assert mean.shape == (len(ids), 5) and float((mean - ref).abs().max()) < 1e-6
        # the grouping is by VIDEO: clip-major rows would give other means
        assert float((mean - torch.softmax(lg, -1).view(10, len(ids), 5).mean(0)).abs().max()) > 1e-3
        ref_mean.append(ref)
        ref_vid += ids
    ref_mean, ref_vid = torch.cat(ref_mean), torch.tensor(ref_vid, device=gpu)
    assert list(cls_dict) == ['Walk', 'Sit', 'Jump', 'Run', 'Dive'] and len(cls_dict['Sit']['mean_prob']) == 3
    acc = CLI.summarize_probability(prob_dict, classes.index, 'temporal_10_clip', args)
    w1, w2 = _topk(ref_mean, ref_vid, (1, 5))                      # one row per video: the mean over videos of its hit
    assert acc[0].count == 7 and acc[0].avg == pytest.approx(w1, abs=1e-7) and acc[1].avg == pytest.approx(w2, abs=1e-7)
    stat = json.load(open(str(tmp_path / 'epoch0.pth.tar-prob-temporal_10_clip.json')))
    assert len(stat) == 7 and np.allclose([s['mean_prob'][0] for s in stat.values()], ref_mean.cpu().numpy(), atol=1e-6)
    acc = CLI.summarize_classwise_probability(cls_dict, classes.index, 'temporal_10_clip', args)
    per_class = [_topk(ref_mean[ref_vid == c], ref_vid[ref_vid == c], (1, 3)) for c in (0, 3, 1, 2, 4)]     # class-wise, then over classes
    assert acc[0].count == 5 and acc[0].avg == pytest.approx(np.mean([p[0] for p in per_class]), abs=1e-7)
    stat = json.load(open(str(tmp_path / 'epoch0.pth.tar-classwise_prob-temporal_10_clip.json')))
    assert {k: len(v['mean_prob']) for k, v in stat.items()} == {'Walk': 1, 'Sit': 3, 'Jump': 1, 'Run': 1, 'Dive': 1}
    assert np.allclose(stat['Sit']['mean_prob'], ref_mean[ref_vid == 3].cpu().numpy(), atol=1e-6)


# ----------------------------------------------------------------------------------------------- the command line
STATE = {}
COMMON = ['--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
          '--print_freq', '1']


def _data(tmp):
    if 'data' not in STATE:
        d = tmp.getbasetemp() / 'clf_data'
        STATE['data'] = write_dataset(str(d), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
        STATE['cwd'] = str(d)
    return STATE['data'], STATE['cwd']


def _train_lines(out):
    losses = [float(v) for v in re.findall(r'train Epoch: \[\d+\]\[\d+/\d+\]\tLoss: ([0-9.naif+-]+)', out)]
    assert losses and all(np.isfinite(v) and v > 0 for v in losses), out[-2000:]
    val = re.findall(r'val Epoch: \[(\d+)\]\tLoss: ([0-9.naif+-]+) Acc@1: ([0-9.]+) Acc@5: ([0-9.]+)', out)
    assert val and all(0.0 <= float(v[2]) <= 1.0 and np.isfinite(float(v[1])) for v in val), out[-2000:]
    return losses


def test_cli_finetune_from_pretrain_checkpoint(gpu, tmp_path_factory):
    (split, frame), cwd = _data(tmp_path_factory)
    _child([os.path.join(ROOT, 'pretrain.py'), '--net', 'r3d', '--model', 'simclr_naked', '--batch_size', '4', '--seq_len', '8',
            '--img_dim', '64', '--num_seq', '2', '--epochs', '1', '--steps', '2', '--epoch_size', '8', '--prefix', 'pre', '--save_freq', '1',
            '-j', '0', '--optim', 'adam', '--lr', '0.001'], cwd, 300)
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(cwd, 'log-pre')) for f in fs if f == 'epoch0.pth.tar']
    assert len(ck) == 1
    STATE['pretrain'] = ck[0]
    # pretrain.py --optim adam ran the fused Adam: torch.optim.Adam's state, two steps, in the checkpoint ...
    ost = torch.load(ck[0], map_location='cpu', weights_only=True)['optimizer']['state']
    assert len(ost) >= 20 and all(set(e) == {'step', 'exp_avg', 'exp_avg_sq'} and int(e['step']) == 2 for e in ost.values())
    assert any(float(e['exp_avg_sq'].abs().sum()) > 0 for e in ost.values())
    # ... and --resume restores it (the arenas exist before the state is loaded)
    out = _child([os.path.join(ROOT, 'pretrain.py'), '--net', 'r3d', '--model', 'simclr_naked', '--batch_size', '4', '--seq_len', '8',
                  '--img_dim', '64', '--num_seq', '2', '--epochs', '2', '--steps', '1', '--epoch_size', '8', '--prefix', 'pre',
                  '--save_freq', '1', '-j', '0', '--optim', 'adam', '--lr', '0.001', '--resume', ck[0]], cwd, 300)
    assert 'optimizer state restored (%d Adam moment pairs)' % len(ost) in out, out[-2000:]
    ost1 = torch.load(os.path.join(os.path.dirname(ck[0]), 'epoch1.pth.tar'), map_location='cpu', weights_only=True)['optimizer']['state']
    assert all(int(e['step']) == 3 for e in ost1.values())
    out = _child([os.path.join(ROOT, 'classifier.py'), '--pretrain', ck[0], '--train_what', 'ft', '--optim', 'sgd', '--steps', '2',
                  '--epochs', '1', '--save_freq', '1', '--prefix', 'ft', '--split_root', split, '--frame_root', frame, '--rand_flip',
                  '--with_color_jitter', '--lr', '0.01'] + COMMON, cwd, 300)
    _train_lines(out)
    assert 'clips/s' in out and "loaded pretrained checkpoint" in out
    saved = os.path.join(cwd, 'log-ft', 'ft', 'ucf', 'model', 'epoch0.pth.tar')
    assert os.path.isfile(saved)
    sd = torch.load(saved, map_location='cpu', weights_only=True)
    assert sd['epoch'] == 0 and 'momentum_buffer' in sd['optimizer']['state'][0] and 0.0 <= sd['best_acc'] <= 1.0
    from dualvar_amd.model import LinearClassifier
    m = LinearClassifier(num_class=2, network='r3d')
    keys = [k for k in sd['state_dict'] if k.startswith('backbone.')]
    assert len(keys) > 50 and sd['state_dict']['final_fc.0.weight'].shape == (2, 512)
    m.backbone.load_state_dict({k[len('backbone.'):]: v for k, v in sd['state_dict'].items() if k.startswith('backbone.')})
    STATE['ft'] = saved


def test_cli_last_layer_adam_and_resume(gpu, tmp_path_factory):
    (split, frame), cwd = _data(tmp_path_factory)
    assert 'pretrain' in STATE, 'the earlier child failed: no further GPU child is started'
    base = [os.path.join(ROOT, 'classifier.py'), '--train_what', 'last', '--optim', 'adam', '--use_bn', '--use_norm', '--steps', '2',
            '--save_freq', '1', '--prefix', 'last', '--split_root', split, '--frame_root', frame, '--lr', '0.001'] + COMMON
    out = _child(base + ['--pretrain', STATE['pretrain'], '--epochs', '1'], cwd, 300)
    _train_lines(out)
    saved = os.path.join(cwd, 'log-last', 'ft', 'ucf', 'model', 'epoch0.pth.tar')
    sd = torch.load(saved, map_location='cpu', weights_only=True)
    pre = torch.load(STATE['pretrain'], map_location='cpu', weights_only=True)['state_dict']
    n = 0
    for k, v in pre.items():
        if k.startswith('encoder_q.0.'):
            mine = sd['state_dict'][k.replace('encoder_q.0.', 'backbone.')]
            assert mine.dtype == v.dtype and torch.equal(mine, v), k + ': a frozen backbone tensor changed'
            n += 1
    assert n > 50
    st = sd['optimizer']['state']
    assert len(st) == 4 and all(int(e['step']) == 2 for e in st.values()) and sd['iteration'] == 3
    want_m = float(sum(float(e['exp_avg'].double().pow(2).sum()) for e in st.values()) ** 0.5)
    want_v = float(sum(float(e['exp_avg_sq'].double().pow(2).sum()) for e in st.values()) ** 0.5)
    assert want_m > 0 and want_v > 0
    out = _child(base + ['--resume', saved, '--epochs', '2'], cwd, 300)
    got = re.search(r'Adam state restored: 4 tensors, step (\d+), \|exp_avg\| ([0-9.e+-]+), \|exp_avg_sq\| ([0-9.e+-]+)', out)
    assert got, out[-2000:]
    assert int(got.group(1)) == 2
    assert float(got.group(2)) == pytest.approx(want_m, rel=1e-5) and float(got.group(3)) == pytest.approx(want_v, rel=1e-5)
    assert 'Epoch:[1/2]' in out and 'Epoch:[0/2]' not in out
    sd1 = torch.load(os.path.join(os.path.dirname(saved), 'epoch1.pth.tar'), map_location='cpu', weights_only=True)
    assert sd1['epoch'] == 1 and all(int(e['step']) == 4 for e in sd1['optimizer']['state'].values())
    STATE['last'] = os.path.join(os.path.dirname(saved), 'epoch1.pth.tar')


def test_cli_test_passes(gpu, tmp_path_factory):
    (split, frame), cwd = _data(tmp_path_factory)
    assert 'ft' in STATE, 'the earlier child failed: no further GPU child is started'
    ck = STATE['ft']
    base = [os.path.join(ROOT, 'classifier.py'), '--test', ck, '--split_root', split, '--frame_root', frame] + COMMON

    def accs(out):
        a = [float(v) for pair in re.findall(r'Acc@1: ([0-9.]+) Acc@5: ([0-9.]+)', out) for v in pair]
        assert a and all(0.0 <= v <= 1.0 for v in a), out[-2000:]
        return a
    out = _child(base + ['--ten_crop'], cwd, 300)
    assert len(accs(out)) >= 6
    for title, rows in (('center', 1), ('five', 5), ('ten', 10)):
        stat = json.load(open('%s-prob-%s.json' % (ck, title)))
        assert len(stat) == 3 and all(len(s['mean_prob']) == rows and len(s['mean_prob'][0]) == 2 for s in stat.values()), title
        p = np.asarray([s['mean_prob'] for s in stat.values()])
        assert np.all(p >= 0) and np.allclose(p.sum(-1), 1, atol=1e-5)
    out = _child(base + ['--temporal_ten_clip', '--num_seq', '10', '--dataset', 'ucf101-10clip'], cwd, 300)
    accs(out)
    stat = json.load(open('%s-prob-temporal_10_clip.json' % ck))
    assert len(stat) == 3 and all(len(s['mean_prob']) == 1 for s in stat.values())
    assert set(json.load(open('%s-classwise_prob-temporal_10_clip.json' % ck))) == {'Walk', 'Jump'}
    out = _child(base + ['--retrieval', '--num_seq', '10'], cwd, 600)
    nn = [float(v) for v in re.findall(r'\t\d+NN acc = ([0-9.]+)', out)]
    assert len(nn) == 5 and all(0.0 <= v <= 1.0 for v in nn) and nn == sorted(nn), out[-2000:]
    fdir = os.path.join(os.path.dirname(ck), 'feature')
    for split_, n in (('test', 3), ('train', 30)):
        f = torch.load(os.path.join(fdir, 'ucf101_%s_feature.pth.tar' % split_), map_location='cpu', weights_only=True)
        per = torch.load(os.path.join(fdir, 'ucf101_%s_per_feature.pth.tar' % split_), map_location='cpu', weights_only=True)
        lab = torch.load(os.path.join(fdir, 'ucf101_%s_label.pth.tar' % split_), map_location='cpu', weights_only=True)
        assert tuple(f.shape) == (n, 512) and tuple(per.shape) == (n, 10, 512) and tuple(lab.shape) == (n,)
        assert float((per.mean(1) - f).abs().max()) < 1e-5
        assert len(pickle.load(open(os.path.join(fdir, 'ucf101_%s_vname.pkl' % split_), 'rb'))) == n
    sim = torch.load(os.path.join(fdir, 'ucf101_sim.pth.tar'), map_location='cpu', weights_only=True)
    assert tuple(sim.shape) == (3, 30) and float(sim.abs().max()) <= 1 + 1e-5
