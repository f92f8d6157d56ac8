"""GPU: dv_augment_ingest_blocks, the block-wise colour jitter of the augmenting ingest (the reference's
utils/augmentation.py:ColorJitter(block=b), __call__ :587-652) -- against a CPU oracle assembled here from oracle/augment_ref.py
(geometry of the frame row, then each patch's ops on its own slice with the contrast mean taken over that slice), against
dv_augment_ingest for a 1 x 1 grid, through a backbone, and through pretrain.py's command line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from dualvar_amd import ops
from dualvar_amd.ops import DV_BF16, DV_F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
F32_TOL = 3e-5          # the bound of test_ops_gpu.py::test_augment_ingest_full_size_rows_against_oracle, same arithmetic and oracle


def _frames(r, n_src=10, Hs=128, Ws=171):
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    return (((np.sin(yy / 9.0)[..., None] * np.cos(xx / 7.0)[..., None] * 0.4 + 0.5)[None] * r.uniform(0.4, 1, (n_src, 1, 1, 3))
             + r.uniform(-0.2, 0.2, (n_src, Hs, Ws, 3))).clip(0, 1) * 255).round().astype(np.uint8)


def _case(r, frames, F, H, W, nb, gray=True):
    """random frame rows (plain crops, resized crops, flips) and per-patch op lists (every op, contrast at every position)"""
    from oracle import augment_ref as A
    from dualvar_amd.utils.transforms import AUG_PATCH
    n_src, Hs, Ws = frames.shape[:3]
    table = np.zeros(F, dtype=A.ROW)
    for f in range(F):
        row = table[f]
        row['src'] = r.randint(n_src)
        if f % 3 == 0:
            row['crop_h'], row['crop_w'] = H, W
        else:
            row['crop_h'], row['crop_w'] = r.randint(H // 2, Hs + 1), r.randint(W // 2, Ws + 1)
        row['crop_i'], row['crop_j'] = r.randint(0, Hs - row['crop_h'] + 1), r.randint(0, Ws - row['crop_w'] + 1)
        row['flip'] = r.randint(2)
        row['op'][0], row['factor'][0] = A.BRIGHTNESS, 0.1                        # never read by the patched entry
    codes = [A.BRIGHTNESS, A.CONTRAST, A.SATURATION, A.HUE] + ([A.GRAY] if gray else [])
    patches = np.zeros(F * nb * nb, dtype=AUG_PATCH)
    for e in patches:
        for k, c in enumerate(list(r.permutation(codes))[:r.randint(0, len(codes) + 1)]):
            e['op'][k], e['factor'][k] = c, 1.0 if c == A.GRAY else r.uniform(-0.3, 0.3) if c == A.HUE else r.uniform(0.2, 1.8)
    return table, patches


def _oracle(frames, table, patches, nb, N, T, H, W, perm=None, blur=None):
    """fp32 [N, 3, T, H, W] after Normalize: augment_frame on a geometry-only row, then every patch's ops on its slice"""
    from oracle import augment_ref as A
    out = torch.empty(N, 3, T, H, W)
    hu, wu = H // nb, W // nb
    for n in range(N):
        for t in range(T):
            ts = t
            if perm is not None:
                seg = T // perm.shape[1]
                ts = int(perm[n, t // seg]) * seg + t % seg
            row = table[n * T + ts].copy()
            row['op'][:] = 0
            x = A.augment_frame(frames, row, H, W).clone()
            for p in range(nb * nb):
                bi, bj = divmod(p, nb)
                h0, w0 = bi * hu, bj * wu
                h1, w1 = (h0 + hu if bi < nb - 1 else H), (w0 + wu if bj < nb - 1 else W)
                s = x[:, h0:h1, w0:w1]
                e = patches[(n * T + ts) * nb * nb + p]
                for op, f in zip(e['op'], e['factor']):
                    op, f = int(op), float(f)
                    if op == A.BRIGHTNESS:
                        s = A._blend(s, 0, f)
                    elif op == A.CONTRAST:
                        s = A._blend(s, A._luma(s).mean(-1).mean(-1), f)
                    elif op == A.SATURATION:
                        s = A._blend(s, A._luma(s)[None], f)
                    elif op == A.GRAY:
                        s = A._luma(s)[None].expand(3, -1, -1)
                    elif op == A.HUE:
                        s = A._hue(s, f)
                x[:, h0:h1, w0:w1] = s
            if blur is not None and int(blur[n * T + ts]['ww']) != 0:
                x = A.blur_frame(x, blur[n * T + ts])
            out[n, :, t] = x
    return (out - torch.tensor(MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1, 1)


def _run(gpu, entry, dtype, frames, table, patches, nb, N, T, H, W, perm=None, pad=0, blur=None):
    a = ops.new_act(N, T, H + 2 * pad, W + 2 * pad, 3, dtype, gpu, cpitch=4, zero=True)
    fr = torch.from_numpy(np.ascontiguousarray(frames)).to(gpu)
    tb = torch.from_numpy(table.view(np.uint8).copy()).to(gpu)
    pm = None if perm is None else perm.to(gpu)
    bl = None if blur is None else torch.from_numpy(blur.view(np.uint8).copy()).to(gpu)
    btmp = None if blur is None else torch.empty(N * T * H * W * 3, dtype=torch.uint8, device=gpu)
    args = [dtype, fr, fr.shape[0], fr.shape[1], fr.shape[2], tb, N, T, H, W, a, 4, pad, torch.tensor(MEAN).to(gpu),
            (1 / torch.tensor(STD)).to(gpu), pm, 0 if perm is None else perm.shape[1]]
    if entry == 'dv_augment_ingest':
        ops.call(entry, *args, torch.full((N * T,), float('nan'), device=gpu), bl, btmp)
    else:
        pt = None if patches is None else torch.from_numpy(patches.view(np.uint8).copy()).to(gpu)
        ops.call(entry, *args, torch.full((N * T * nb * nb,), float('nan'), device=gpu), bl, btmp, pt, nb)
    torch.cuda.synchronize()
    y = ops.act_to_ncdhw(a)
    if pad:
        inner = y[:, :, :, pad:-pad, pad:-pad].clone()
        y[:, :, :, pad:-pad, pad:-pad] = 0
        assert float(y.abs().max()) == 0.0                                         # the border stays zero
        y = inner
    assert float(a.buf[:, 3].abs().max()) == 0.0
    return y.cpu()


def _bf16_ulp(x):
    _, e = torch.frexp(x)                                                          # x = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.ones_like(x), e - 8)                                  # bf16: 8 significant bits


@pytest.mark.parametrize('nb,H,W,dtype,pad', [(2, 112, 112, DV_F32, 0), (3, 112, 112, DV_F32, 3), (5, 112, 112, DV_F32, 0),
                                              (3, 64, 80, DV_F32, 3), (5, 64, 80, DV_BF16, 3), (2, 112, 112, DV_BF16, 0)])
def test_blocks_against_oracle(gpu, nb, H, W, dtype, pad):
    r = np.random.RandomState(100 + nb * 7 + H + W + dtype)
    N, T = 3, 4
    frames = _frames(r)
    table, patches = _case(r, frames, N * T, H, W, nb)
    perm = torch.tensor([[1, 0], [0, 1], [1, 0]], dtype=torch.int32)
    got = _run(gpu, 'dv_augment_ingest_blocks', dtype, frames, table, patches, nb, N, T, H, W, perm=perm, pad=pad)
    want = _oracle(frames, table, patches, nb, N, T, H, W, perm=perm.numpy())
    err = (got - want).abs()
    print(f'blocks nb={nb} {H}x{W} {"bf16" if dtype == DV_BF16 else "fp32"}: max abs err {float(err.max()):.2e}')
    if dtype == DV_F32:
        assert float(err.max()) <= F32_TOL
    else:
        assert bool((err <= _bf16_ulp(want) + F32_TOL).all())


def test_blocks_with_gaussian_blur(gpu):
    """blurred frames: the patched colour ops, then PIL's blur of the re-quantised frame, then Normalize"""
    from dualvar_amd.utils.transforms import AUG_BLUR, box_blur_params
    r = np.random.RandomState(9)
    N, T, H, W, nb = 2, 4, 112, 112, 3
    frames = _frames(r)
    table, patches = _case(r, frames, N * T, H, W, nb)
    blur = np.zeros(N * T, dtype=AUG_BLUR)
    for f in range(0, N * T, 2):
        blur['radius'][f], blur['ww'][f], blur['fw'][f] = box_blur_params(0.3 + 0.2 * f)
    got = _run(gpu, 'dv_augment_ingest_blocks', DV_F32, frames, table, patches, nb, N, T, H, W, blur=blur)
    want = _oracle(frames, table, patches, nb, N, T, H, W, blur=blur)
    e = (got - want).abs()
    on = torch.from_numpy(blur['ww'] != 0).view(N, 1, T, 1, 1).expand_as(e)
    step = float((1 / 255.0 / torch.tensor(STD)).max())
    print(f'blocks + blur: max abs err {float(e.max()):.2e}, elements beyond {F32_TOL}: {int((e > F32_TOL).sum())} of {e.numel()}')
    # unblurred frames: the fp32 bound; blurred ones: a float frame within one ulp of a byte boundary may truncate the other way
    # on the GPU (see test_ops_gpu.py: test_augment_gaussian_blur_against_pil_fixture) -- one uint8 step, on few pixels
    assert float(e[~on].max()) <= F32_TOL
    off = e > F32_TOL
    assert float(e.max()) <= step + F32_TOL and int(off.sum()) <= 0.01 * int(on.sum())


@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
def test_one_block_is_the_plain_entry(gpu, dtype):
    """a 1 x 1 grid whose patch lists are the frame rows' own op lists == dv_augment_ingest, bit for bit (perm, blur, pad)"""
    from oracle import augment_ref as A
    from dualvar_amd.utils.transforms import AUG_BLUR, AUG_PATCH, box_blur_params
    r = np.random.RandomState(4)
    N, T, H, W = 3, 8, 112, 112
    frames = _frames(r)
    table, _ = _case(r, frames, N * T, H, W, 1)
    codes = [A.BRIGHTNESS, A.CONTRAST, A.SATURATION, A.GRAY, A.HUE]
    for row in table:
        row['op'][:] = 0
        for k, c in enumerate(list(r.permutation(codes))[:r.randint(0, 6)]):
            row['op'][k], row['factor'][k] = c, 1.0 if c == A.GRAY else r.uniform(-0.3, 0.3) if c == A.HUE else r.uniform(0.2, 1.8)
    patches = np.zeros(N * T, dtype=AUG_PATCH)
    patches['op'], patches['factor'] = table['op'], table['factor']
    blur = np.zeros(N * T, dtype=AUG_BLUR)
    for f in range(1, N * T, 3):
        blur['radius'][f], blur['ww'][f], blur['fw'][f] = box_blur_params(1.1)
    perm = torch.tensor([[1, 0], [0, 1], [1, 0]], dtype=torch.int32)
    want = _run(gpu, 'dv_augment_ingest', dtype, frames, table, None, 1, N, T, H, W, perm=perm, pad=3, blur=blur)
    got = _run(gpu, 'dv_augment_ingest_blocks', dtype, frames, table, patches, 1, N, T, H, W, perm=perm, pad=3, blur=blur)
    assert torch.equal(got, want)
    nul = _run(gpu, 'dv_augment_ingest_blocks', dtype, frames, table, None, 1, N, T, H, W, perm=perm, pad=3, blur=blur)
    assert torch.equal(nul, want)


def test_bad_patch_entries_cannot_fault(gpu):
    r = np.random.RandomState(2)
    N, T, H, W, nb = 1, 4, 64, 64, 4
    frames = _frames(r)
    table, patches = _case(r, frames, N * T, H, W, nb)
    patches['op'][0, 0], patches['op'][1, :] = 99, -7
    y = _run(gpu, 'dv_augment_ingest_blocks', DV_F32, frames, table, patches, nb, N, T, H, W)
    assert torch.isfinite(y).all()


def test_backbone_on_patched_frame_batch(gpu):
    """IngestOp: a FrameBatch with patches goes through dv_augment_ingest_blocks (the backbone's output equals the same backbone
    fed the kernel's own NDHWC output as float clips, bit for bit)"""
    import random
    from oracle import procedural as P
    from dualvar_amd.backbone import select_backbone
    from dualvar_amd.utils import transforms as T
    r = np.random.RandomState(5)
    frames = r.randint(0, 256, size=(16, 72, 96, 3)).astype(np.uint8)
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    tr = T.Compose([T.RandomSizedCrop((64, 64)), T.RandomHorizontalFlip(),
                    T.ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.8, block=3), T.RandomGray(0.2)])
    clips = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [4, 5, 6, 7, 8, 9, 10, 11], [1, 3, 5, 7, 9, 11, 13, 15]]
    fb = T.FrameBatch.build(torch.from_numpy(frames), clips, tr, (64, 64), views=2, device=gpu)
    assert fb.patches is not None and fb.n_block == 3
    act = ops.new_act(8, 8, 64, 64, 3, DV_F32, gpu, cpitch=4, zero=True)
    ops.call('dv_augment_ingest_blocks', DV_F32, fb.frames, 16, 72, 96, fb.table, 8, 8, 64, 64, act, 4, 0,
             torch.tensor(MEAN).to(gpu), (1 / torch.tensor(STD)).to(gpu), None, 0, torch.empty(8 * 8 * 9, device=gpu), None, None,
             fb.patches, 3)
    block = ops.act_to_ncdhw(act).contiguous()
    m, _ = select_backbone('r3d')
    P.procedural_init(m)
    m.set_compute_dtype('fp32').eval().to(gpu)                    # running statistics: no cross-sample reduction
    m.set_input_normalization(MEAN, STD)
    with torch.no_grad():
        a = m.forward_pooled(fb.reshape(-1, 3, 8, 64, 64)).clone()
        v1 = m.forward_pooled(fb[:, 1]).clone()
    m.set_input_normalization(None, None)
    with torch.no_grad():
        b = m.forward_pooled(block).clone()
        b1 = m.forward_pooled(block.view(4, 2, 3, 8, 64, 64)[:, 1].contiguous()).clone()
    assert torch.equal(a, b) and torch.equal(v1, b1)


def _cli(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'pretrain.py'), '--net', 'r3d', '--batch_size', '8', '--seq_len', '8', '--img_dim', '64',
           '--steps', '4', '--epochs', '1', '--epoch_size', '64', '--print_freq', '1', '--prefix', 't',
           '--model', 'simclr_naked', '--num_seq', '2'] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))


def test_pretrain_cli_block_jitter(gpu, tmp_path):
    r = _cli(tmp_path, '--dataset', 'synthetic-frames', '--n_block', '2', '--aug_temp_grad_consist', '-j', '2')
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    losses = [float(v) for v in re.findall(r'VLoss ([0-9.]+)', out)]
    assert losses and all(0.0 < v < 50.0 for v in losses), losses
    bad = _cli(tmp_path, '--dataset', 'synthetic-frames', '--aug_temp_consist', '--aug_temp_grad_consist', '-j', '0')
    assert bad.returncode != 0 and 'mutually exclusive' in bad.stderr
