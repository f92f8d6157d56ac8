"""The reference's downstream datasets on extracted video frames: `--dataset ucf101 / hmdb51` (dataset/local_dataset.py:
UCF101LMDB `:176-201` with the sampler `:107-138`, HMDB51LMDB) and `ucf101-10clip / hmdb51-10clip` (UCF101_10CLIP `:311-350`,
HMDB51_10CLIP), read with the transforms of classifier.py:1006-1033 and the crop views of its test_10crop `:545-654`.

Same contract as the pretraining dataset (utils/frame_dataset.py): a DataLoader worker draws the sample's frame indices and
augmentations from `random` / `numpy.random` call for call in the reference's order, decodes every distinct frame once at its
stored size, and returns the decoded frames plus dv_aug_frame (and, under the colour jitter, dv_aug_patch) rows.  The GPU then
scales (dv_resample_u8: PIL's `A.Scale`, bit-exact) and crops / flips / jitters / normalises (dv_augment_ingest).

`A.Scale(int)` (utils/augmentation.py:131-144) depends on the frame's own size, so a batch may hold several scaled sizes: the
collate groups the frames by scaled size, each group is resampled by one launch, and the groups land in ONE buffer of the largest
size (top-left aligned, the rest zero) that a single ingest launch reads -- every row's window lies inside its own frame.

Differences from the reference, on purpose:
  * test mode, a video with vlen <= num_frames * ds: the pad side (random.randint(0, 1), `:111`) is drawn once per VIDEO, and all
    crop views share it; the reference re-reads the dataset once per (flip, crop) view and draws it once per pass.
  * `FiveCrop(where=4)` takes its top edge from `h - tw` (utils/augmentation.py:216); here `h - th` (the same for square crops).
  * UCF101_10CLIP opens every frame of the video and keeps 10 * num_frames of them; here only those are decoded."""
import os
import random

import numpy as np
import torch

from . import resample as R
from . import transforms as T
from .frame_dataset import read_classes, read_split

DATASETS = {                                   # --dataset -> (split_root, frame_root, ten_clip): the reference's defaults
    'ucf101': ('process_data/data/ucf101', 'data/UCF101/frame', False),
    'ucf101-10clip': ('process_data/data/ucf101', 'data/UCF101/frame', True),
    'hmdb51': ('process_data/data/hmdb51', 'data/HMDB51/frame', False),
    'hmdb51-10clip': ('process_data/data/hmdb51', 'data/HMDB51/frame', True),
}
NUM_CLASS = {'ucf101': 101, 'ucf101-10clip': 101, 'hmdb51': 51, 'hmdb51-10clip': 51}        # classifier.py:192
AUG_LIST, FLIP_LIST = (5, 1, 2, 3, 4), (0, 1)      # classifier.py:549-565: 1..5 = top-left, top-right, bottom-left, bottom-right, centre
CROP_VIEWS = {'center': [(0, 5)], 'five': [(0, a) for a in AUG_LIST], 'ten': [(f, a) for f in FLIP_LIST for a in AUG_LIST]}


def scaled_size(h, w, size):
    """(rows, columns) of A.Scale(size) on an h x w frame: an int scales the shorter side to `size` and the other to
    int(size * long / short) (nothing when the shorter side already matches); a pair is PIL's (width, height)"""
    if not isinstance(size, int):
        return int(size[1]), int(size[0])
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def scale_arg(img_resize_dim, img_dim, aug_crop):
    """classifier.py:1017-1018,1028-1029: --aug_crop with img_dim == 112 switches to Scale((128, 171))"""
    return (128, 171) if (aug_crop and img_dim == 112) else int(img_resize_dim)


def _pad(sequence, total, left):
    seq_idx = np.zeros_like(sequence) if left else np.ones_like(sequence) * (total - 1)
    sequence = sequence[sequence < total]
    if left:
        seq_idx[-len(sequence)::] = sequence
    else:
        seq_idx[:len(sequence)] = sequence
    return seq_idx


def window_sampler(total, num_frames, ds, mode):
    """UCF101LMDB_2CLIP.frame_sampler (dataset/local_dataset.py:107-138).  test: every half-overlapping window (step
    num_frames * ds // 2 - 1), flattened to [n_windows * num_frames]; a video that does not hold one window is padded on a
    drawn side.  train / val: one window from a start drawn with np.random.choice (short videos: a phase, then the pad side)."""
    span = num_frames * ds
    if mode == 'test':
        if total - span <= 0:
            return _pad(np.arange(num_frames) * ds, total, random.randint(0, 1))
        start = np.expand_dims(np.arange(0, total - span + 1, span // 2 - 1), 1)
        return (np.expand_dims(np.arange(num_frames) * ds, 0) + start).flatten()
    if total - span <= 0:
        sequence = np.arange(num_frames) * ds + np.random.choice(range(ds), 1)
        return _pad(sequence, total, random.randint(0, 1))
    return np.arange(num_frames) * ds + np.random.choice(range(total - span), 1)


def ten_clip_indices(vlen, num_frames, ds):
    """UCF101_10CLIP.__getitem__ (`:324-333`): ten clip centres np.linspace'd over the video, each clip clamped to it"""
    half = num_frames * ds // 2
    min_index = min(half, vlen)
    max_index = max(min_index, vlen - half)
    out = []
    for clip_center in np.linspace(min_index, max_index, 10):
        clip_start = max(0, int(clip_center - half))
        out.extend(min(t, vlen - 1) for t in range(clip_start, clip_start + num_frames * ds, ds))
    return np.asarray(out, dtype=np.int64)


def crop_window(h, w, size, where):
    """A.FiveCrop(size, where) / A.CenterCrop (utils/augmentation.py:178-220) on an h x w frame -> (top, left)"""
    th, tw = (size, size) if isinstance(size, int) else size
    if th > h or tw > w:
        raise ValueError('Requested crop size %s is bigger than input size %s' % ((th, tw), (h, w)))
    if where == 5:
        return int(round((h - th) / 2.)), int(round((w - tw) / 2.))
    return (0 if where in (1, 2) else h - th), (0 if where in (1, 3) else w - tw)


def view_rows(src, h, w, size, views):
    """dv_aug_frame rows of the (flip, where) views of one video, view-major: RandomHorizontalFlip(command) -> Scale ->
    FiveCrop(where) of classifier.py:589-600.  The crop of the MIRRORED frame at (top, left) is the window at
    (top, w - left - tw) of the frame itself, read right to left (flip = 1)."""
    th, tw = (size, size) if isinstance(size, int) else size
    t = np.zeros(len(views) * len(src), dtype=T.AUG_ROW)
    n = len(src)
    for v, (flip, where) in enumerate(views):
        top, left = crop_window(h, w, (th, tw), where)
        r = t[v * n:(v + 1) * n]
        r['src'], r['crop_i'], r['crop_j'], r['crop_h'], r['crop_w'] = src, top, (w - left - tw) if flip else left, th, tw
        r['flip'] = flip
    return t


class BlockHorizontalFlip(object):
    """A.RandomHorizontalFlip(consistent=False, seq_len=...) (utils/augmentation.py:332-341): one random.random() per block of
    seq_len frames; the block is mirrored when the draw is below 0.5.  Sits after the crop (classifier.py:1016)."""

    def __init__(self, seq_len, p=0.5):
        self.seq_len, self.p = seq_len, p

    def __call__(self, st):
        st._no_colour_yet('flip')
        flip = np.zeros(st.N, dtype=bool)
        for idx in range(st.N):
            if idx % self.seq_len == 0:
                th = random.random()
            flip[idx] = th < self.p
        st.flip = np.logical_xor(flip, st.flip)
        return st


def finetune_transform(mode, img_dim, seq_len, rand_flip=False, with_color_jitter=False):
    """get_transform of classifier.py:1006-1033 without its Scale / ToTensor.  train: RandomCrop (the PIL class: left edge first),
    the per-block flip under --rand_flip, ColorJitter(0.8, 0.8, 0.8, 0.2, p=0.8, consistent=True, block=1) under
    --with_color_jitter (the reference appends it behind ToTensor, where its PIL class cannot run: placed in front, as meant).
    val / test: CenterCrop."""
    if mode != 'train':
        return T.Compose([T.CenterCrop((img_dim, img_dim))])
    steps = [T.PILRandomCrop(img_dim)]
    if rand_flip:
        steps.append(BlockHorizontalFlip(seq_len))
    if with_color_jitter:
        steps.append(T.ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.8, consistent=True, seq_len=seq_len, block=1, patched=True))
    return T.Compose(steps)


class FinetuneFrames(torch.utils.data.Dataset):
    """UCF101LMDB / HMDB51LMDB for the GPU pipeline.  mode train / val: one window of num_frames frames; test: every
    half-overlapping window.  `views` (a CROP_VIEWS list) replaces the transform by the crop views of the centre / five /
    ten-crop test: rows view-major, [n_views * n_windows * num_frames].
    Returns {'decoded': [uint8 [H, W, 3]] (each distinct frame once), 'size': the scaled (rows, columns), 'aug': AUG_ROW rows
    (source = position in 'decoded'), 'patch': AUG_PATCH rows under a colour jitter, 'vid', 'vpath', 'vname'}."""

    def __init__(self, split_root, frame_root, mode='val', num_frames=16, ds=1, transform=None, which_split=1, img_dim=112,
                 scale=128, views=None):
        self.frame_root, self.mode, self.num_frames, self.ds = frame_root, mode, num_frames, ds
        self.transform, self.img_dim, self.scale, self.views = transform, img_dim, scale, views
        self.classes = read_classes(split_root)
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.video_subset = read_split(split_root, mode, which_split)

    def __len__(self):
        return len(self.video_subset)

    def encode_action(self, action_name):
        return self.class_to_idx[action_name]

    def decode_action(self, action_code):
        return self.classes[action_code]

    def sample_indices(self, vlen):
        return window_sampler(vlen, self.num_frames, self.ds, self.mode)

    def frame_path(self, vname, i):
        return os.path.join(self.frame_root, vname, 'image_%05d.jpg' % (i + 1))

    def __getitem__(self, index):
        from PIL import Image
        vpath, vlen, vlabel, vname = self.video_subset.iloc[index]
        idx = np.asarray(self.sample_indices(int(vlen))).reshape(-1).tolist()
        pos = {}
        for i in idx:
            pos.setdefault(i, len(pos))
        decoded = [None] * len(pos)
        for i, p in pos.items():
            with Image.open(self.frame_path(vname, i)) as im:
                decoded[p] = np.asarray(im.convert('RGB'))
        src = [pos[i] for i in idx]
        h, w = scaled_size(decoded[0].shape[0], decoded[0].shape[1], self.scale)
        if min(h, w) < self.img_dim:                   # every window the rows name must lie inside the scaled frame
            raise ValueError('%s scales to %dx%d, smaller than the %d-pixel crop' % (vname, h, w, self.img_dim))
        if any(f.shape != decoded[0].shape for f in decoded):
            raise ValueError('%s holds frames of different sizes' % vname)
        out = {'decoded': decoded, 'size': (h, w), 'frame_index': np.asarray(idx), 'vid': self.encode_action(vlabel),
               'vpath': vpath, 'vname': vname}
        if self.views is not None:
            out['aug'] = view_rows(src, h, w, self.img_dim, self.views)
        elif self.transform is not None:
            st = self.transform(T.ClipState(src, h, w))
            out['aug'] = st.rows(self.img_dim, self.img_dim)
            if st.block is not None:
                out['patch'] = st.patch_rows(self.img_dim, self.img_dim, block=1)
        return out


class TenClipFrames(FinetuneFrames):
    """UCF101_10CLIP / HMDB51_10CLIP: ten uniformly spaced clips of num_frames frames -> [10 * num_frames]"""

    def sample_indices(self, vlen):
        return ten_clip_indices(vlen, self.num_frames, self.ds)


def build_dataset(name, split_root, frame_root, **kw):
    if name not in DATASETS:
        raise ValueError('unknown dataset %r (one of %s)' % (name, ', '.join(sorted(DATASETS))))
    return (TenClipFrames if DATASETS[name][2] else FinetuneFrames)(split_root, frame_root, **kw)


def collate_finetune(samples):
    """samples -> one batch: the decoded frames grouped by scaled size, group g packed as 'src<g>' / 'rs_desc<g>' / 'rs_coef<g>'
    (dualvar_amd.utils.resample.pack) with 'groups'[g] = (size, positions in the batch's frame list, host tables); the rows'
    source index moved to the frame's position in the batch; 'aug' / 'patch' as flat uint8; 'n_rows' per sample"""
    frames, base, sizes = [], [], []
    for s in samples:
        base.append(len(frames))
        frames.extend(s['decoded'])
        sizes.extend([tuple(s['size'])] * len(s['decoded']))
    groups = {}
    for p, sz in enumerate(sizes):
        groups.setdefault(sz, []).append(p)
    batch = {'n_frames': len(frames), 'groups': [], 'vid': torch.tensor([s['vid'] for s in samples], dtype=torch.long),
             'vpath': [s['vpath'] for s in samples], 'vname': [s['vname'] for s in samples]}
    for g, (sz, pos) in enumerate(groups.items()):
        src, desc, coef = R.pack([frames[p] for p in pos], sz)
        batch['src%d' % g] = torch.from_numpy(src)
        batch['rs_desc%d' % g] = torch.from_numpy(desc.view(np.uint8))
        batch['rs_coef%d' % g] = torch.from_numpy(coef)
        batch['groups'].append((sz, pos, desc, coef))
    if 'aug' in samples[0]:
        rows = []
        for s, b in zip(samples, base):
            a = s['aug'].copy()
            a['src'] += b
            rows.append(a)
        batch['n_rows'] = [len(a) for a in rows]
        batch['aug'] = torch.from_numpy(np.concatenate(rows).view(np.uint8).copy())
        if any('patch' in s for s in samples):
            pt = [s['patch'] if 'patch' in s else np.zeros(len(s['aug']), dtype=T.AUG_PATCH) for s in samples]
            batch['patch'] = torch.from_numpy(np.concatenate(pt).view(np.uint8).copy())
    return batch


def scale_batch(batch):
    """the GPU half of A.Scale: batch (tensors on the device) -> uint8 [n_frames, Hmax, Wmax, 3]; a frame of a smaller scaled
    size sits in the top-left corner of its slot, the rest is zero"""
    outs = [R.resample_u8(batch['src%d' % g], batch['rs_desc%d' % g], batch['rs_coef%d' % g], desc, coef, sz)
            for g, (sz, pos, desc, coef) in enumerate(batch['groups'])]
    if len(outs) == 1:
        return outs[0]
    Hm, Wm = max(sz[0] for sz, _, _, _ in batch['groups']), max(sz[1] for sz, _, _, _ in batch['groups'])
    buf = torch.zeros((batch['n_frames'], Hm, Wm, 3), dtype=torch.uint8, device=outs[0].device)
    for o, (sz, pos, _, _) in zip(outs, batch['groups']):
        buf[torch.as_tensor(pos, device=buf.device), :sz[0], :sz[1]] = o
    return buf


def frame_batch(batch, frames, n_clips, seq_len, img_dim):
    """the model's input: [n_clips, 3, seq_len, img_dim, img_dim] as a FrameBatch over the scaled frames"""
    dev = frames.device
    return T.FrameBatch(frames, batch['aug'].to(dev).view(-1), (n_clips, 3, seq_len, img_dim, img_dim),
                        patches=batch['patch'].to(dev).view(-1) if 'patch' in batch else None, n_block=1)
