"""GPU: dv_resample_u8 (PIL-exact Scale) against PIL itself, and the real-frame pretraining path end to end: loader -> resample ->
augmenting ingest against PIL open -> resize((128, 171), BICUBIC) -> the CPU augmentation oracle on the same rows, and
pretrain.py's command line on a tiny generated JPEG dataset."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from dualvar_amd import _lib as L
from dualvar_amd import ops
from dualvar_amd.ops import DV_F32
from dualvar_amd.utils import frame_dataset as FD
from dualvar_amd.utils import resample as R
from tests.dataset_support import SIZES, TARGETS, _img, _seed, write_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
F32_TOL = 3e-5          # the bound of test_ops_gpu.py::test_augment_ingest_full_size_rows_against_oracle, same arithmetic and oracle


def _launch(gpu, frames, size, extra=0, filt='bicubic', tamper=None):
    """pack + dv_resample_u8 into a buffer `extra` bytes longer than needed, filled with a sentinel -> (out [n, Ho, Wo, 3], tail)"""
    src, desc, coef = R.pack(frames, size, filt)
    if tamper is not None:
        tamper(desc, coef)
    n, (Ho, Wo) = len(frames), size
    buf = torch.full((n * Ho * Wo * 3 + extra,), 0xA5, dtype=torch.uint8, device=gpu)
    R.resample_u8(torch.from_numpy(src).to(gpu), torch.from_numpy(desc.view(np.uint8).copy()).to(gpu),
                  torch.from_numpy(coef).to(gpu), desc, coef, size, out=buf)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return b[:n * Ho * Wo * 3].reshape(n, Ho, Wo, 3), b[n * Ho * Wo * 3:]


@pytest.mark.parametrize('filt', ['bicubic', 'bilinear'])
def test_resample_equals_pil(gpu, filt):
    r = np.random.RandomState(11)
    pf = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}[filt]
    for H, W in SIZES:
        img = _img(r, H, W)
        for size in TARGETS:
            if max(R.coeffs(W, size[1], filt)[0], R.coeffs(H, size[0], filt)[0]) > R.MAX_KSIZE:
                with pytest.raises(ValueError, match='at most'):           # over the kernel's tap cap: refused on the host
                    _launch(gpu, [img], size, filt=filt)
                continue
            got, tail = _launch(gpu, [img, img[::-1].copy()], size, extra=64, filt=filt)
            for k, im in enumerate((img, img[::-1].copy())):
                want = np.asarray(Image.fromarray(im).resize((size[1], size[0]), pf))
                assert np.array_equal(got[k], want), ((H, W), size, filt, k)
            assert np.all(tail == 0xA5)


def test_resample_ragged_launch(gpu):
    """one launch over frames of mixed sizes (UCF101, K400 widths, portrait, unchanged rows / columns, tiny) == PIL per frame"""
    r = np.random.RandomState(12)
    shapes = [(240, 320), (240, 426), (240, 456), (360, 240), (171, 90), (240, 128), (171, 128), (17, 5), (240, 320)] * 3
    frames = [_img(r, *s) for s in shapes]
    got, tail = _launch(gpu, frames, FD.FRAME_SIZE, extra=4096)
    for k, im in enumerate(frames):
        assert np.array_equal(got[k], np.asarray(Image.fromarray(im).resize((128, 171), Image.BICUBIC))), (k, im.shape)
        assert np.array_equal(got[k], R.resize_u8(im, FD.FRAME_SIZE))
    assert np.all(tail == 0xA5)


def test_resample_refuses_bad_tables(gpu):
    r = np.random.RandomState(13)
    frames = [_img(r, 240, 320), _img(r, 240, 426)]

    def bad(fn):
        with pytest.raises(L.DualVarHipError, match='DV_EINVAL|DV_EALIGN'):
            _launch(gpu, frames, FD.FRAME_SIZE, tamper=fn)

    def wrong_table(d, c):                           # frame 1's columns through frame 0's 320 -> 128 table
        d['h_coef'][1] = d['h_coef'][0]

    def outside(d, c):                               # an entry reaching past the source row
        t = int(d['h_coef'][0])
        k = int(c[t + 2])
        c[t + 4 + 127 * (2 + k)] = 320 - 1
    bad(wrong_table)
    bad(outside)
    bad(lambda d, c: c.__setitem__(int(d['v_coef'][0]) + 2, R.MAX_KSIZE + 1))      # ksize over the cap
    bad(lambda d, c: d.__setitem__('Hs', 0))
    bad(lambda d, c: d['src_offset'].__setitem__(1, d['src_offset'][1] + 8))        # misaligned
    bad(lambda d, c: d['src_offset'].__setitem__(1, 10 ** 9))                       # outside src
    bad(lambda d, c: d['v_coef'].__setitem__(0, -1))                                # skipping a pass whose size changes


def _oracle_batch(batch, frame_root, samples_paths, T_, img):
    """CPU: every distinct frame PIL-decoded and resized((128, 171), BICUBIC), then oracle/augment_ref on the batch's rows (the
    one-patch op lists are the frame's op list)"""
    from oracle import augment_ref as A
    from dualvar_amd.utils.transforms import AUG_BLUR, AUG_PATCH, AUG_ROW
    frames = np.stack([np.asarray(Image.open(p).convert('RGB').resize((128, 171), Image.BICUBIC)) for p in samples_paths])
    aug = batch['aug'].cpu().numpy().reshape(-1).view(AUG_ROW).copy()
    patch = batch['patch'].cpu().numpy().reshape(-1).view(AUG_PATCH)
    aug['op'], aug['factor'] = patch['op'], patch['factor']
    blur = batch['blur'].cpu().numpy().reshape(-1).view(AUG_BLUR)
    N = len(aug) // T_
    return frames, A.augment_ingest(frames, aug, N, T_, img, img, mean=MEAN, std=STD, blur=blur)


def _stem_input(gpu, batch, T_, img):
    """what IngestOp feeds the stem: dv_resample_u8 then dv_augment_ingest_blocks on the batch's rows (pretrain.py's path)"""
    fr = FD.scale_batch(batch)
    N = batch['aug'].numel() // 64 // T_
    a = ops.new_act(N, T_, img, img, 3, DV_F32, gpu, cpitch=4, zero=True)
    ops.call('dv_augment_ingest_blocks', DV_F32, fr, fr.shape[0], fr.shape[1], fr.shape[2], batch['aug'].view(-1), N, T_, img, img, a,
             4, 0, torch.tensor(MEAN).to(gpu), (1 / torch.tensor(STD)).to(gpu), None, 0, torch.empty(N * T_, device=gpu),
             batch['blur'].view(-1), torch.empty(N * T_ * img * img * 3, dtype=torch.uint8, device=gpu), batch['patch'].view(-1), 1)
    torch.cuda.synchronize()
    return fr.cpu().numpy(), ops.act_to_ncdhw(a).cpu()


def _loader(split, frame, workers, T_, img, seed=0):
    _seed(seed)
    ds = FD.StagePrototypeFrames(split, frame, mode='train', num_frames=T_, ds=4, rand_flip=True, aug_series=True, img_dim=img,
                                 transform=FD.stage_prototype_transform(img, T_))
    import pretrain
    dl = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=True, num_workers=workers, collate_fn=FD.collate_frame_clips,
                                     pin_memory=True, drop_last=True, worker_init_fn=pretrain.seed_worker)
    return ds, dl


@pytest.mark.parametrize('workers', [0, 2])
def test_end_to_end_against_pil_and_oracle(gpu, tmp_path, workers):
    T_, img = 8, 64
    split, frame = write_dataset(str(tmp_path), sizes=[(240, 320), (240, 426), (180, 240)])
    ds, dl = _loader(split, frame, workers, T_, img)
    batch = next(iter(dl))
    paths = _decoded_paths(ds, batch, frame)
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in batch.items()}
    fr, got = _stem_input(gpu, dev, T_, img)
    frames, want = _oracle_batch(batch, frame, paths, T_, img)
    assert np.array_equal(fr, frames)                                # the GPU's Scale == PIL's, byte for byte
    err = (got - want).abs()
    blurred = torch.from_numpy(batch['blur'].numpy().reshape(-1).view(np.uint32).reshape(-1, 4)[:, 1] != 0)
    on = blurred.view(-1, 1, T_, 1, 1).expand_as(err)
    step = float((1 / 255.0 / torch.tensor(STD)).max())
    print(f'end to end ({workers} workers): max abs err {float(err.max()):.2e}, {int(blurred.sum())} blurred frames')
    # as test_augment_blocks_gpu.py::test_blocks_with_gaussian_blur: unblurred frames to the fp32 bound; a blurred frame may
    # re-quantise one pixel a uint8 step the other way
    if bool((~on).any()):
        assert float(err[~on].max()) <= F32_TOL
    assert float(err.max()) <= step + F32_TOL and int((err > F32_TOL).sum()) <= 0.01 * max(int(on.sum()), 1)
    # same seed, same bytes
    _, dl2 = _loader(split, frame, workers, T_, img)
    b2 = next(iter(dl2))
    for k in ('src', 'rs_desc', 'rs_coef', 'aug', 'blur', 'patch'):
        assert torch.equal(batch[k], b2[k]), k
    _, got2 = _stem_input(gpu, {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in b2.items()}, T_, img)
    assert torch.equal(got, got2)


def _decoded_paths(ds, batch, frame):
    """the file of every packed frame, found by matching bytes against the dataset's decode of its videos"""
    desc = batch['rs_host'][0]
    src = batch['src'].numpy()
    table = {}
    for _, row in ds.video_subset.drop_duplicates(3).iterrows():
        for i in range(int(row[1])):
            p = ds.frame_path(row[3], i)
            table[np.asarray(Image.open(p).convert('RGB')).tobytes()] = p
    out = []
    for d in desc:
        o, n = int(d['src_offset']), int(d['Hs']) * int(d['Ws']) * 3
        out.append(table[src[o:o + n].tobytes()])
    return out


def test_pretrain_cli_on_frames(gpu, tmp_path):
    split, frame = write_dataset(str(tmp_path / 'data'), sizes=[(240, 320), (240, 426), (180, 240)])
    base = [sys.executable, os.path.join(ROOT, 'pretrain.py'), '--net', 'r3d', '--model', 'simclr_timeseriesv4', '--batch_size', '4',
            '--seq_len', '8', '--img_dim', '64', '--epochs', '1', '--print_freq', '1', '--prefix', 't',
            '--dataset', 'ucf101-2clip-stage-prototype', '--ds', '4', '--rand_flip', '--aug_temp_consist', '--steps', '2', '-j', '2',
            '--split_root', split, '--frame_root', frame]
    r = subprocess.run(base + ['--aug_series', '--num_seq', '3'], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    losses = [float(v) for v in re.findall(r'Loss:([0-9.naif+-]+)', out)]
    assert losses and all(np.isfinite(v) and v > 0 for v in losses), out[-2000:]
    bad = subprocess.run(base + ['--num_seq', '3'], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert bad.returncode != 0 and 'three clips' in bad.stderr and 'Traceback' not in bad.stderr
