"""The reference's pretraining datasets on extracted video frames: `--dataset ucf101-2clip-stage-prototype` and
`k400-2clip-stage-prototype` (dataset/local_dataset.py: UCF101LMDB_2CLIP_Stage_Prototype and its K400 subclass, read with the
transform of pretrain.py:491-533).

On disk, as the reference lays it out (process_data/src/write_csv.py, extract_frame.py):
  <split_root>/ClassInd.txt                        one class per line (`index,name` or a bare name)
  <split_root>/{train,test}_split%02d.csv          rows (vpath, vlen); vpath ends in <class>/<video>/
  <frame_root>/<class>/<video>/image_%05d.jpg      the frames, 1-based

A sample is decoded on the host (the DataLoader workers) and everything else runs on the GPU: the workers draw the sample's
frame indices and augmentations from `random`, `numpy.random` and torch's RNG call for call as the reference does, decode
every distinct frame once, and hand over the decoded frames at their own size plus the augmentation table rows.  The batch
then goes through dv_resample_u8 (PIL's Scale((128, 171)), bit-exact: dualvar_amd/utils/resample.py) and dv_augment_ingest.

Scale((128, 171)) is PIL (width, height): the scaled frames have 171 rows and 128 columns (FRAME_SIZE)."""
import os
import random

import numpy as np
import torch

from . import resample as R
from . import transforms as T

FRAME_SIZE = (171, 128)                              # (rows, columns) after the reference's A.Scale((128, 171))
VAL_ROWS, VAL_SEED = 800, 666                        # dataset/local_dataset.py: sample(n=800, random_state=666)
DATASETS = {                                         # --dataset -> (split_root, frame_root): the reference's hard-coded defaults
    'ucf101-2clip-stage-prototype': ('process_data/data/ucf101', 'data/UCF101/frame'),
    'k400-2clip-stage-prototype': ('process_data/data/k400', 'data/K400/frame'),
}


def read_classes(split_root):
    with open(os.path.join(split_root, 'ClassInd.txt')) as f:
        classes = [ln.strip() for ln in f.readlines()]
    if ',' in classes[0]:
        classes = [c.split(',')[-1].strip() for c in classes]
    return classes


def read_split(split_root, mode='train', which_split=1):
    """rows (vpath, vlen, class, vname) of a split, as UCF101LMDB_2CLIP.__init__ selects them.  The reference never assigns
    `video_subset` and drops the wrong thing (`video_info.drop(val_split)`): defect D9, repaired here as its code intends --
    `val` is the 800 rows of sample(n=800, random_state=666) of the train split, `train` is the train split without them."""
    import pandas as pd
    if mode not in ('train', 'val', 'test'):
        raise ValueError('mode must be train, val or test, got %r' % (mode,))
    num_class = len(read_classes(split_root))
    csv = os.path.join(split_root, '%s_split%02d.csv' % ('test' if mode == 'test' else 'train', which_split))
    info = pd.read_csv(csv, header=None)
    info[2] = info[0].str.split('/').str.get(-3)                 # class, e.g. ApplyEyeMakeup
    info[3] = info[2] + '/' + info[0].str.split('/').str.get(-2)  # frame directory, class/video
    if mode != 'test':
        if len(info) <= VAL_ROWS:
            raise ValueError('%s has %d rows: the train / val split sets %d of them aside and needs more' % (csv, len(info), VAL_ROWS))
        val = info.sample(n=VAL_ROWS, random_state=VAL_SEED)
        info = info.drop(val.index) if mode == 'train' else val
    if len(pd.unique(info[2])) != num_class:
        raise ValueError('the %s split of %s holds %d classes, ClassInd.txt lists %d' % (mode, split_root, len(pd.unique(info[2])),
                                                                                         num_class))
    return info[[0, 1, 2, 3]]


def frame_sampler(total, num_frames, ds, center_lower=0, center_upper=0, repeat_prob=0.25, length=0):
    """UCF101LMDB_2CLIP_Stage_Prototype.frame_sampler: a centre from np.random.randint, then two random.uniform draws that may
    widen the clamp window (for sample_prototype's (0, total) they change nothing, but they are drawn)"""
    length = num_frames if length == 0 else length
    if center_upper == 0:
        center_upper = total
    center_ind = np.random.randint(center_lower, center_upper)
    diff_seq = (np.arange(length) - length // 2) * ds
    if random.uniform(0., 1.) >= repeat_prob:
        center_lower = 0
    if random.uniform(0., 1.) >= repeat_prob:
        center_upper = total
    return np.clip(diff_seq + center_ind, center_lower, center_upper - 1).astype(np.int32)


def stage_prototype_transform(img_dim, seq_len, consistent=False, n_block=1, grad_consistent=False):
    """get_transform of pretrain.py:491-533 without its Scale / ToTensor (the GPU scales; the ingest makes floats):
    MultiRandomizedTransform([null, base, same_series], weights=[[.2, .8, 0], [0, 1, 0], [0, 0, 1]]), where null = RandomCrop and
    base = same_series = RandomCrop, RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2, p=0.8, ...)], p=0.8),
    RandomApply([GaussianBlur([.1, 2.])], p=0.5).  The crop is the PIL class's (left edge drawn first) and the jitter draws as the
    PIL-pipeline class does, per frame and patch, at every n_block."""
    def base():
        return T.Compose([
            T.PILRandomCrop(img_dim),
            T.RandomApply([T.ColorJitter(0.8, 0.8, 0.8, hue=0.2, p=0.8, consistent=consistent, seq_len=seq_len, block=n_block,
                                         grad_consistent=grad_consistent, patched=True)], p=0.8),
            T.RandomApply([T.GaussianBlur([.1, 2.], seq_len=seq_len)], p=0.5)])
    return T.MultiRandomizedTransform([T.PILRandomCrop(img_dim), base(), base()], weights=[[0.2, 0.8, 0], [0, 1.0, 0], [0, 0., 1.0]])


class StagePrototypeFrames(torch.utils.data.Dataset):
    """UCF101LMDB_2CLIP_Stage_Prototype / K400LMDB_2CLIP_Stage_Prototype (dataset/local_dataset.py), for the GPU pipeline.

    __getitem__ consumes the RNGs in the reference's order: the rand_flip draw (random.randint(0, 1): it REVERSES THE FRAME ORDER
    of both clips, it is not a horizontal flip), the two frame_sampler calls, then -- per clip -- the MultiRandomizedTransform
    choice and the chosen transform's draws.  With aug_series the third clip is clip 1 again (same frames, its own draws).
    Returns {'decoded': [uint8 [H, W, 3]] (each distinct frame index once, at its stored size), 'aug': AUG_ROW rows (source =
    position in 'decoded'), 'blur': AUG_BLUR rows, 'patch': AUG_PATCH rows (n_block^2 per frame)}, rows clip-major."""

    def __init__(self, split_root, frame_root, mode='train', num_frames=16, ds=1, rand_flip=False, aug_series=True, transform=None,
                 which_split=1, img_dim=112, n_block=1):
        self.num_clips = 3 if aug_series else 2
        if transform is not None and len(transform.weights) != self.num_clips:
            raise ValueError('the stage-prototype transform takes %d clips per sample (num_seq * n_proto = %d, with --aug_series); '
                             'this dataset yields %d' % (len(transform.weights), len(transform.weights), self.num_clips))
        self.frame_root, self.mode, self.num_frames, self.ds = frame_root, mode, num_frames, ds
        self.rand_flip, self.aug_series, self.transform = rand_flip, aug_series, transform
        self.img_dim, self.n_block = img_dim, n_block
        self.classes = read_classes(split_root)
        self.video_subset = read_split(split_root, mode, which_split)

    def __len__(self):
        return len(self.video_subset)

    def sample_indices(self, vlen):
        """the RNG draws in front of decoding -> (frame indices of clip 1, of clip 2), 0-based"""
        flip = random.randint(0, 1) if self.rand_flip else 0
        i1 = frame_sampler(vlen, self.num_frames, self.ds)
        if flip:
            i1 = i1[::-1]
        i2 = frame_sampler(vlen, self.num_frames, self.ds)
        if flip:
            i2 = i2[::-1]
        return i1, i2

    def frame_path(self, vname, i):
        return os.path.join(self.frame_root, vname, 'image_%05d.jpg' % (i + 1))

    def __getitem__(self, index):
        from PIL import Image
        vpath, vlen, vlabel, vname = self.video_subset.iloc[index]
        i1, i2 = self.sample_indices(int(vlen))
        pos = {}
        for i in np.concatenate([i1, i2]).tolist():
            pos.setdefault(i, len(pos))
        decoded = [None] * len(pos)
        for i, p in pos.items():
            with Image.open(self.frame_path(vname, i)) as im:
                decoded[p] = np.asarray(im.convert('RGB'))
        clips = [[pos[i] for i in i1.tolist()], [pos[i] for i in i2.tolist()]]
        if self.aug_series:
            clips.append(clips[0])
        out = {'decoded': decoded}
        if self.transform is not None:
            states = self.transform([T.ClipState(c, *FRAME_SIZE) for c in clips])
            size = (self.img_dim, self.img_dim)
            out['aug'] = np.concatenate([st.rows(*size) for st in states])
            out['blur'] = np.concatenate([st.blur_rows() for st in states])
            out['patch'] = np.concatenate([st.patch_rows(*size, block=self.n_block) for st in states])
        return out


def collate_frame_clips(samples, size=FRAME_SIZE):
    """samples of StagePrototypeFrames -> one batch: every decoded frame of the batch packed into one uint8 buffer ('src') with one
    dv_resample_desc row per frame ('rs_desc') and the coefficient tables they name ('rs_coef'), plus the same two tables as numpy
    arrays ('rs_host', for the entry's validation: not tensors, so they stay on the host); the augmentation rows' source index
    moved to the frame's position in the packed batch; 'aug' / 'blur' / 'patch' as uint8 [B, bytes] like collate_frames"""
    frames, base = [], []
    for s in samples:
        base.append(len(frames))
        frames.extend(s['decoded'])
    src, desc, coef = R.pack(frames, size)
    batch = {'src': torch.from_numpy(src), 'rs_desc': torch.from_numpy(desc.view(np.uint8)), 'rs_coef': torch.from_numpy(coef),
             'rs_host': (desc, coef), 'n_frames': len(frames)}
    if 'aug' in samples[0]:
        aug = np.stack([s['aug'] for s in samples])
        aug['src'] += np.asarray(base, dtype=np.int32)[:, None]
        blur = np.stack([s['blur'] for s in samples])
        batch['aug'] = torch.from_numpy(aug.view(np.uint8).reshape(len(samples), -1).copy())
        batch['blur'] = torch.from_numpy(blur.view(np.uint8).reshape(len(samples), -1).copy())
        batch['has_blur'] = bool(blur['ww'].any())
        batch['patch'] = torch.from_numpy(np.stack([s['patch'] for s in samples]).view(np.uint8).reshape(len(samples), -1).copy())
    return batch


def scale_batch(batch, size=FRAME_SIZE):
    """the GPU half of the pipeline's Scale: batch (on the device, 'rs_host' on the host) -> uint8 [n_frames, Ho, Wo, 3]"""
    desc, coef = batch['rs_host']
    return R.resample_u8(batch['src'], batch['rs_desc'], batch['rs_coef'], desc, coef, size)
