#!/usr/bin/env python
"""classifier.py -- DualVar downstream evaluation on MI355X (drop-in for the reference's second entry script): finetune
(`--train_what ft / last`), validation, the centre / five / ten-crop test, the temporal 10-clip test and nearest-neighbour
retrieval, on the reference's extracted JPEG frames.

Same command line as the reference (classifier.py:38-107, every flag with its default) plus `--split_root`, `--frame_root`,
`--dtype`, `--steps` (caps the iterations of a train epoch and of a validation pass; 0 = the whole pass) and `--seed`, as
pretrain.py has them.  `num_class` is 101 / 51 by dataset name (`:192`), or the length of ClassInd.txt under `--split_root`.
Model build `:200-211`, `--train_what last` freezing and SGD / Adam `:240-264`, `--pretrain` (with the `encoder_q.0.` ->
`backbone.` rename) / `--resume` / the neq_load_customized fallback `:335-379`, adjust_learning_rate `:998-1003`, the train
loop `:422-498`, validate `:501-542`, checkpoints with best_acc `:400-415`, the test passes `:545-995`.

What differs, deliberately:
  * data: frames are decoded in the DataLoader workers and scaled (PIL-exact), cropped, flipped, jittered and normalised on
    the GPU (dualvar_amd/utils/finetune_dataset.py); Normalize is fused into the ingest kernel;
  * the crop test reads every video ONCE: all (flip, crop) views of a video are rows of one ingest table, where the reference
    re-reads the whole dataset once per view (ten passes).  A video shorter than num_frames * ds therefore draws its pad side
    once per video, not once per pass;
  * loss and accuracy come from the fused cross-entropy kernel (DF.cross_entropy and its rank0) and reach the host through an
    asynchronous copy, one step late: no per-step sync;
  * single process only: a distributed launch (WORLD_SIZE > 1, --multiprocessing-distributed) is refused -- the reference
    itself asserts a single process for every test pass; TensorBoard plots are not written.

Kept as the reference's code has it, though it may surprise: the crop test scales with A.Scale(img_resize_dim) and ignores
`--aug_crop` (`:589-600`; the 10-clip and retrieval passes honour it), and retrieval always reads split 1 (`:830,839`).
The parameter arenas are materialised before `--resume` loads the optimizer state: this project's arena optimizers need
somewhere to load into.

Defects of the reference, repaired as its code intends:
  * `ft_mode=` is passed to dataset constructors that have no such argument (`:1041`, `:1050`): dropped;
  * `video_subset` is never assigned and `drop(val_split)` drops the wrong thing (dataset/local_dataset.py:102-104): train / val
    are the train split without / the 800 sampled rows (dualvar_amd.utils.frame_dataset.read_split);
  * `FiveCrop(where=4)` takes its top edge from `h - tw` (utils/augmentation.py:216): `h - th`;
  * `--with_color_jitter` appends the PIL ColorJitter behind ToTensor (`:1014`), where it cannot run: placed in front;
  * labels are moved with `.cuda()` inside the summaries (`:748`, `:773`): they stay on the logits' device;
  * `args.logger.info(name, param.requires_grad)` (`:258`) passes two arguments to a one-argument method: formatted;
  * the summary's comment says it averages the views' probabilities; its CODE scores every view's row on its own and averages
    the hits per video, then over videos (`:762-784`): the code is followed;
  * set_path takes dirname(dirname(ckpt)) as the experiment directory and appends the dataset folder again (`:1088-1101`), so
    resuming <exp>/ucf/model/epochN writes to <exp>/ucf/ucf/model: a checkpoint of this driver resumes into its own directory;
  * `--temporal_ten_clip` on a dataset that is not a -10clip one reshapes whatever windows it gets into ten "clips" (`:670-677`):
    refused;
  * the crop test's `tr` only works for num_seq == 1 (it squeezes that axis): any other value is refused, as in training.
"""
import os as _os
_os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
import argparse
import json
import math
import os
import pickle
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from dualvar_amd.utils import finetune_dataset as FD  # noqa: E402
from dualvar_amd.utils.utils import AverageMeter, ProgressMeter, neq_load_customized, save_checkpoint  # noqa: E402
from pretrain import MEAN, STD, DevicePrefetcher, DistLogger, seed_worker  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    # model
    p.add_argument('--net', default='myrealr21d', type=str)
    p.add_argument('--model', default='linclr', type=str)
    p.add_argument('--num_fc', default=1, type=int)
    p.add_argument('--train_what', default='ft', type=str)
    p.add_argument('--use_dropout', action='store_true')
    p.add_argument('--use_norm', action='store_true')
    p.add_argument('--use_bn', action='store_true')
    p.add_argument('--dropout', default=1., type=float)
    p.add_argument('--ft-mode', action='store_true')
    p.add_argument('--with_color_jitter', action='store_true')
    # dataset
    p.add_argument('--dataset', default='ucf101', type=str)
    p.add_argument('--which_split', default=1, type=int)
    p.add_argument('--seq_len', default=16, type=int)
    p.add_argument('--num_seq', default=1, type=int)
    p.add_argument('--ds', default=4, type=int)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--img_resize_dim', default=128, type=int)
    p.add_argument('--img_dim', default=112, type=int)
    # optimizer
    p.add_argument('--optim', default='sgd', type=str)
    p.add_argument('--lr', default=5e-2, type=float)
    p.add_argument('--schedule', default=[10, 20, 30, 40], nargs='*', type=int)
    p.add_argument('--wd', default=1e-4, type=float)
    p.add_argument('--epochs', default=50, type=int)
    p.add_argument('--start_epoch', default=0, type=int)
    p.add_argument('--gpu', default=None, type=int)
    # log
    p.add_argument('--print_freq', default=5, type=int)
    p.add_argument('--eval_freq', default=1, type=int)
    p.add_argument('--save_freq', default=10, type=int)
    # exp settings
    p.add_argument('--prefix', default='linclr', type=str)
    p.add_argument('--name_prefix', default='', type=str)
    p.add_argument('-j', '--workers', default=8, type=int)
    p.add_argument('--dirname', default=None, type=str)
    # mode
    p.add_argument('--resume', default='', type=str)
    p.add_argument('--pretrain', default='', type=str)
    p.add_argument('--test', default='', type=str)
    p.add_argument('--retrieval', action='store_true')
    p.add_argument('--knn', action='store_true', help='with --test ... --retrieval: also the weighted k-NN classifier on the same features')
    p.add_argument('--knn_k', default=200, type=int)
    p.add_argument('--knn_t', default=0.07, type=float)
    p.add_argument('--variance', action='store_true', help='with --test ... --retrieval: also the inter- / intra-video variance report of the clip features')
    p.add_argument('--var_bins', default=64, type=int)
    p.add_argument('--var_t', default=2.0, type=float)
    p.add_argument('--tsne', action='store_true', help='with --test ... --retrieval: also the t-SNE map of the clip features')
    p.add_argument('--tsne_perplexity', default=30, type=int)
    p.add_argument('--tsne_iter', default=1000, type=int)
    p.add_argument('--tsne_seed', default=0, type=int)
    p.add_argument('--tsne_split', default='test', choices=['test', 'train', 'both'])
    p.add_argument('--cluster', action='store_true', help='with --test ... --retrieval: also spherical k-means of the clip features, scored against the classes')
    p.add_argument('--cluster_k', default=0, type=int, help='clusters (0: as many as the dataset has classes)')
    p.add_argument('--cluster_iter', default=100, type=int)
    p.add_argument('--cluster_init', default=10, type=int)
    p.add_argument('--cluster_seed', default=0, type=int)
    p.add_argument('--cluster_split', default='test', choices=['test', 'train', 'both'])
    p.add_argument('--ridge', action='store_true', help='with --test ... --retrieval: also the closed-form ridge probe, fitted on the train clip features and scored on the test clips')
    p.add_argument('--ridge_lambda', default=[1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1], type=float, nargs='*', help='the grid of lambda (relative to the number of training clips)')
    p.add_argument('--ridge_holdout', default=5, type=int, help='one training video in this many, per class, is held out to choose lambda')
    p.add_argument('--spectrum', action='store_true', help='with --test ... --retrieval: also the eigenvalue spectrum of the clip-feature covariance (effective rank, RankMe, alpha, PCA retrieval)')
    p.add_argument('--spectrum_k', default=[32, 64, 128], type=int, nargs='*', help='the numbers of leading principal components to project on (values above the feature width are clamped)')
    p.add_argument('--map', action='store_true', help='with --test ... --retrieval: also mean average precision, precision@k, recall@k, R-precision and MRR over the full ranking')
    p.add_argument('--map_k', default=[1, 5, 10, 20, 50], type=int, nargs='+', help='the cut-offs k of precision@k / recall@k / success@k (at most 16)')
    p.add_argument('--map_level', default='video', choices=['video', 'clip', 'both'], help='rank test videos against train videos (mean features), test clips against train clips, or both')
    p.add_argument('--map_within', action='store_true', help='with --map: also the test clips among themselves, the clips of their own video left out')
    p.add_argument('--center_crop', action='store_true')
    p.add_argument('--five_crop', action='store_true')
    p.add_argument('--ten_crop', action='store_true')
    p.add_argument('--temporal_ten_clip', action='store_true')
    # parallel
    p.add_argument('--world-size', default=-1, type=int)
    p.add_argument('--rank', default=-1, type=int)
    p.add_argument('--dist-url', default='env://', type=str)
    p.add_argument('--dist-backend', default='nccl', type=str)
    p.add_argument('--multiprocessing-distributed', action='store_true')
    p.add_argument('--local_rank', '--local-rank', dest='local_rank', default=-1, type=int)
    p.add_argument('--aug_crop', action='store_true')
    p.add_argument('--rand_flip', action='store_true')
    # this build (as pretrain.py)
    p.add_argument('--split_root', default=None, type=str, help='ClassInd.txt and {train,test}_split%%02d.csv (default: the reference\'s path)')
    p.add_argument('--frame_root', default=None, type=str, help='<class>/<video>/image_%%05d.jpg (default: the reference\'s path)')
    p.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    p.add_argument('--steps', default=0, type=int, help='cap the iterations of a train epoch and of a validation pass (0 = whole pass)')
    p.add_argument('--seed', default=0, type=int)
    return p.parse_args(argv)


def refuse(msg):
    sys.stderr.write('classifier.py: %s\n' % msg)
    sys.exit(2)


def check_args(args, environ=None):
    """everything this driver refuses, one line each, before anything touches the GPU"""
    environ = os.environ if environ is None else environ
    world = args.world_size
    if world == -1:
        try:
            world = int(environ.get('WORLD_SIZE', 1))
        except ValueError:
            world = 1
    if world > 1 or args.multiprocessing_distributed:
        refuse('distributed launches are not built (WORLD_SIZE / --world-size > 1, --multiprocessing-distributed): run one process on one GPU')
    if args.dataset not in FD.DATASETS:
        refuse('unknown --dataset %r: one of %s' % (args.dataset, ', '.join(sorted(FD.DATASETS))))
    if args.model != 'linclr':
        refuse('unknown --model %r: only linclr' % args.model)
    if args.optim not in ('sgd', 'adam'):
        refuse('unknown --optim %r: sgd or adam' % args.optim)
    if args.save_freq % args.eval_freq != 0:
        refuse('--save_freq must be a multiple of --eval_freq')
    if args.knn and not (args.test and args.retrieval):
        refuse('--knn votes on the retrieval features: pass --test <checkpoint> --retrieval with it')
    if not 1 <= args.knn_k <= 256:
        refuse('--knn_k must be between 1 and 256 (the selection kernel keeps at most 256 neighbours)')
    if not args.knn_t > 0:
        refuse('--knn_t must be positive')
    if args.variance and not (args.test and args.retrieval):
        refuse('--variance reports on the retrieval clip features: pass --test <checkpoint> --retrieval with it')
    if not 1 <= args.var_bins <= 256:
        refuse('--var_bins must be between 1 and 256 (the pair-statistics kernel keeps at most 256 bins)')
    if not (args.var_t >= 0 and math.isfinite(args.var_t)):
        refuse('--var_t must be finite and not negative')
    if args.tsne and not (args.test and args.retrieval):
        refuse('--tsne maps the retrieval clip features: pass --test <checkpoint> --retrieval with it')
    if args.tsne_perplexity < 2:
        refuse('--tsne_perplexity must be at least 2')
    if 3 * args.tsne_perplexity + 1 > 256:
        refuse('--tsne_perplexity must be at most 85 (the selection kernel keeps at most 256 neighbours, 3 * perplexity + 1 of them are needed)')
    if args.tsne_iter < 1:
        refuse('--tsne_iter must be at least 1')
    if args.cluster and not (args.test and args.retrieval):
        refuse('--cluster clusters the retrieval clip features: pass --test <checkpoint> --retrieval with it')
    if not 0 <= args.cluster_k <= 4096:
        refuse('--cluster_k must be between 0 (the class count) and 4096 (the k-means kernels keep at most 4096 clusters)')
    if args.cluster_iter < 1:
        refuse('--cluster_iter must be at least 1')
    if args.cluster_init < 1:
        refuse('--cluster_init must be at least 1')
    if args.ridge and not (args.test and args.retrieval):
        refuse('--ridge fits on the retrieval clip features: pass --test <checkpoint> --retrieval with it')
    if not args.ridge_lambda or any(not (v > 0 and math.isfinite(v)) for v in args.ridge_lambda):
        refuse('--ridge_lambda takes one or more positive finite values')
    if args.ridge_holdout < 2:
        refuse('--ridge_holdout must be at least 2')
    if args.spectrum and not (args.test and args.retrieval):
        refuse('--spectrum decomposes the covariance of the retrieval clip features: pass --test <checkpoint> --retrieval with it')
    if not args.spectrum_k or any(k < 1 for k in args.spectrum_k):
        refuse('--spectrum_k takes one or more component counts of at least 1')
    if args.map and not (args.test and args.retrieval):
        refuse('--map ranks the retrieval features: pass --test <checkpoint> --retrieval with it')
    if not 1 <= len(args.map_k) <= 16 or any(k < 1 for k in args.map_k):
        refuse('--map_k takes one to 16 cut-offs of at least 1')
    if args.map_within and not args.map:
        refuse('--map_within adds to the --map report: pass --map with it')
    if args.map_level != 'video' and not args.map:
        refuse('--map_level chooses the features of the --map report: pass --map with it')
    if args.test:
        if args.retrieval:
            if args.num_seq != 10:
                refuse('--retrieval samples ten clips per video: pass --num_seq 10')
            if args.dataset not in ('ucf101', 'hmdb51'):
                refuse('--retrieval takes --dataset ucf101 or hmdb51')
        elif args.center_crop or args.five_crop or args.ten_crop:
            if args.num_seq != 1:
                refuse('the crop tests squeeze the num_seq axis: pass --num_seq 1')
        elif args.temporal_ten_clip:
            if args.num_seq != 10:
                refuse('--temporal_ten_clip needs --num_seq 10')
            if not FD.DATASETS[args.dataset][2]:
                refuse('--temporal_ten_clip reads ten clips per video: pass --dataset %s-10clip' % args.dataset)
        else:
            refuse('--test needs one of --retrieval, --center_crop, --five_crop, --ten_crop, --temporal_ten_clip')
    elif args.num_seq != 1:
        refuse('training squeezes the num_seq axis (num_seq is always 1 there): pass --num_seq 1')


def set_path(args):
    """classifier.py:1087-1116 (directory naming kept, under log-<prefix>/ like pretrain.py's)"""
    fold = 'ucf' if 'ucf' in args.dataset else 'hmdb'
    if args.resume or args.test:
        exp_path = os.path.dirname(os.path.dirname(os.path.abspath(args.resume or args.test)))
        if os.path.basename(exp_path) == fold:        # a checkpoint of this driver, <exp>/<fold>/model/: back to <exp>
            exp_path = os.path.dirname(exp_path)
    else:
        exp_path = os.path.join('log-' + args.prefix, 'ft', args.name_prefix)
    img_path, model_path = os.path.join(exp_path, fold, 'img'), os.path.join(exp_path, fold, 'model')
    if not args.test:
        log_name = 'log'
    elif args.retrieval:
        log_name = 'test_retrieval_log'
    elif not args.temporal_ten_clip:
        log_name = 'test_log'
    else:
        log_name = 'temporal_10_test_log'
    os.makedirs(img_path, exist_ok=True)
    os.makedirs(model_path, exist_ok=True)
    return img_path, model_path, exp_path, os.path.join(exp_path, fold, log_name)


def adjust_learning_rate(optimizer, epoch, args):
    """classifier.py:998-1003"""
    ratio = 0.1 if epoch in args.schedule else 1.
    for g in optimizer.param_groups:
        g['lr'] = g['lr'] * ratio


def get_data(mode, args, views=None, dataset=None, transform_mode=None, which_split=None):
    """get_transform + get_data of classifier.py:1006-1058 (transform_mode, which_split: retrieval reads its train split with the
    test transform and always split 1, `:809-841`).  The crop views are cut from A.Scale(img_resize_dim) frames whatever
    --aug_crop says: test_10crop builds its own transform (`:589-600`); every other pass honours --aug_crop."""
    name = dataset or args.dataset
    ten = FD.DATASETS[name][2]
    tf = FD.finetune_transform(transform_mode or mode, args.img_dim, args.seq_len, rand_flip=args.rand_flip,
                               with_color_jitter=args.with_color_jitter)
    scale = int(args.img_resize_dim) if views is not None else FD.scale_arg(args.img_resize_dim, args.img_dim, args.aug_crop)
    return FD.build_dataset(name, args.split_root, args.frame_root, mode=mode,
                            num_frames=args.seq_len if ten else args.seq_len * args.num_seq, ds=args.ds,
                            transform=None if views is not None else tf,
                            which_split=args.which_split if which_split is None else which_split, img_dim=args.img_dim,
                            scale=scale, views=views)


def get_dataloader(dataset, mode, args, batch_size=None):
    """classifier.py:1061-1084: train and val shuffle and drop the last batch; the test passes read in order"""
    nw = min(args.workers, 16)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size or args.batch_size, shuffle=mode in ('train', 'val'),
                                         num_workers=nw, pin_memory=True, drop_last=mode in ('train', 'val'),
                                         worker_init_fn=seed_worker, collate_fn=FD.collate_finetune,
                                         persistent_workers=nw > 0 and mode == 'train', prefetch_factor=4 if nw > 0 else None)
    args.logger.info('"%s" dataset size: %d' % (mode, len(dataset)))
    return DevicePrefetcher(loader, args.gpu)


def model_input(batch, args):
    """a batch of collate_finetune, on the device -> (FrameBatch [n_clips, 3, seq_len, H, W], n_clips)"""
    frames = FD.scale_batch(batch)
    n_rows = batch['aug'].numel() // FD.T.AUG_ROW.itemsize
    n_clips = n_rows // args.seq_len
    return FD.frame_batch(batch, frames, n_clips, args.seq_len, args.img_dim), n_clips


class AsyncScalars:
    """device scalars -> host on a copy stream, read one step late (pretrain.py's train loop does the same): no per-step sync"""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device)
        self.bufs, self.pending, self.k = [None, None], None, 0

    def push(self, dev_vec, tag):
        prev, slot = self.pending, self.k & 1
        self.k += 1
        if self.bufs[slot] is None or self.bufs[slot].numel() != dev_vec.numel():
            self.bufs[slot] = torch.empty(dev_vec.numel(), dtype=torch.float32).pin_memory()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        dev_vec.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            self.bufs[slot].copy_(dev_vec, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        self.pending = (done, self.bufs[slot], tag)
        return self._read(prev)

    def flush(self):
        prev, self.pending = self.pending, None
        return self._read(prev)

    @staticmethod
    def _read(p):
        if p is None:
            return None
        p[0].synchronize()
        return p[1].tolist(), p[2]


def step_scalars(loss, rank0):
    """[loss, top1, top5] on the device (calc_topk_accuracy(logit, target, (1, 5)) from the criterion's rank0)"""
    r = rank0.float()
    return torch.stack([loss.detach().float().reshape(()), (r < 1).float().mean(), (r < 5).float().mean()])


def train_one_epoch(loader, model, optimizer, epoch, args):
    """classifier.py:422-498"""
    from dualvar_amd import functional as DF
    batch_time, data_time = AverageMeter('Time', ':.2f'), AverageMeter('Data', ':.2f')
    losses, top1_meter, top5_meter = AverageMeter('Loss', ':.4f'), AverageMeter('acc@1', ':.4f'), AverageMeter('acc@5', ':.4f')
    args.lr = optimizer.param_groups[0]['lr']
    progress = ProgressMeter(len(loader), [batch_time, data_time, losses, top1_meter, top5_meter],
                             prefix='Epoch:[{}/{}] lr:{} '.format(epoch, args.epochs, args.lr), logger=args.logger)
    if args.train_what == 'last':
        model.eval()                   # totally freeze BN in backbone
    else:
        model.train()
    if args.use_bn:
        model.final_bn.train()
    scal = AsyncScalars(args.gpu)

    def account(got):
        if got is not None:
            (l_, t1, t5), B_ = got
            losses.update(l_, B_)
            top1_meter.update(t1, B_)
            top5_meter.update(t5, B_)

    tic = end = time.time()
    clips, idx = 0, -1
    for idx, batch in enumerate(loader):
        data_time.update(time.time() - end)
        input_seq, B = model_input(batch, args)
        logit, _ = model(input_seq)
        loss, rank0 = DF.cross_entropy(logit, batch['vid'])
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        account(scal.push(step_scalars(loss, rank0), B))
        clips += B
        batch_time.update(time.time() - end)
        end = time.time()
        if (idx + 1) % args.print_freq == 0:
            progress.display(idx)
        args.iteration += 1
        if args.steps and idx + 1 >= args.steps:
            break
    account(scal.flush())
    dt = time.time() - tic
    args.logger.info('train Epoch: [{0}][{1}/{2}]\tLoss: {loss.avg:.4f} Acc@1: {top1.avg:.4f} Acc@5: {top5.avg:.4f}\t'
                     'T-epoch:{t:.2f}\t{cps:.1f} clips/s'.format(epoch, idx + 1, len(loader), loss=losses, top1=top1_meter,
                                                                 top5=top5_meter, t=dt, cps=clips / max(dt, 1e-9)))
    return losses.avg, top1_meter.avg


def validate(loader, model, epoch, args):
    """classifier.py:501-542"""
    from dualvar_amd import functional as DF
    losses, top1_meter, top5_meter = AverageMeter(), AverageMeter('acc@1', ':.4f'), AverageMeter('acc@5', ':.4f')
    model.eval()
    scal = AsyncScalars(args.gpu)

    def account(got):
        if got is not None:
            (l_, t1, t5), B_ = got
            losses.update(l_, B_)
            top1_meter.update(t1, B_)
            top5_meter.update(t5, B_)

    with torch.no_grad():
        for idx, batch in enumerate(loader):
            input_seq, B = model_input(batch, args)
            logit, _ = model(input_seq)
            loss, rank0 = DF.cross_entropy(logit, batch['vid'])
            account(scal.push(step_scalars(loss, rank0), B))
            if args.steps and idx + 1 >= args.steps:
                break
    account(scal.flush())
    args.logger.info('val Epoch: [{0}]\tLoss: {loss.avg:.4f} Acc@1: {top1.avg:.4f} Acc@5: {top5.avg:.4f}\t'
                     .format(epoch, loss=losses, top1=top1_meter, top5=top5_meter))
    return losses.avg, top1_meter.avg


# ------------------------------------------------------------------------------------------------------- test passes
def group_probabilities(logit, n_groups):
    """[n_groups * n, K] logits, group-major -> [n_groups, K]: softmax, then the mean over each group's n rows.  The groups are
    the (flip, crop) views of one video over its windows (classifier.py:620) or the videos of a batch over their ten clips
    (`:716-718`)"""
    from dualvar_amd.utils.evaluation import softmax_rows
    from dualvar_amd import _lib as L, ops
    prob = softmax_rows(logit)
    n, K = prob.shape[0] // n_groups, prob.shape[1]
    if n * n_groups != prob.shape[0]:
        raise ValueError('%d rows do not split into %d groups' % (prob.shape[0], n_groups))
    mean = torch.empty(n_groups, K, dtype=torch.float32, device=prob.device)
    L.check(L.load().dv_group_mean_f32(prob.data_ptr(), n_groups, n, K, mean.data_ptr(), ops.stream_ptr()), 'dv_group_mean_f32')
    return mean


def collect_ten_clip(logit, batch, decode_action, prob_dict, cls_prob_dict):
    """one batch of the 10-clip test (classifier.py:716-730): [B * 10, K] logits, video-major -> the per-video mean probability,
    filed under the video's path and under its class"""
    mean = group_probabilities(logit, len(batch['vpath']))
    for i, vname in enumerate(batch['vpath']):
        prob_dict[vname] = {'mean_prob': mean[i:i + 1].clone()}
        cls_prob_dict.setdefault(decode_action(int(batch['vid'][i])), {'mean_prob': []})['mean_prob'].append(mean[i].clone())
    return mean


def summarize_probability(prob_dict, action_to_idx, title, args, rows=None):
    """classifier.py:762-784: every row of a video's 'mean_prob' is scored on its own against the video's class; the hits are
    averaged per video, then over the videos.  `rows` keeps the first rows only (centre: 1, five-crop: 5 of the ten).
    Writes <ckpt>-prob-<title>.json.  -> [top-1 meter, top-5 meter]"""
    from dualvar_amd.utils.evaluation import topk_of_mean
    acc = [AverageMeter(), AverageMeter()]
    stat = {}
    for vname, item in prob_dict.items():
        parts = vname.split('/')
        action_name = parts[-3] if len(parts) >= 3 else parts[-2]
        mean_prob = item['mean_prob'] if rows is None else item['mean_prob'][:rows]
        target = torch.full((mean_prob.shape[0],), action_to_idx(action_name), dtype=torch.long, device=mean_prob.device)
        top1, top5 = topk_of_mean(mean_prob, target, (1, 5))
        stat[vname] = {'mean_prob': mean_prob.tolist()}
        acc[0].update(top1, 1)
        acc[1].update(top5, 1)
    args.logger.info('Mean: Acc@1: {acc[0].avg:.4f} Acc@5: {acc[1].avg:.4f}'.format(acc=acc))
    with open(os.path.join(os.path.dirname(args.test), '%s-prob-%s.json' % (os.path.basename(args.test), title)), 'w') as fp:
        json.dump(stat, fp)
    return acc


def summarize_classwise_probability(cls_prob_dict, action_to_idx, title, args):
    """classifier.py:741-759"""
    from dualvar_amd.utils.evaluation import topk_of_mean
    acc = [AverageMeter(), AverageMeter()]
    stat = {}
    for action_name, item in cls_prob_dict.items():
        mean_prob = torch.stack(item['mean_prob'], 0)
        target = torch.full((mean_prob.shape[0],), action_to_idx(action_name), dtype=torch.long, device=mean_prob.device)
        top1, top5 = topk_of_mean(mean_prob, target, (1, 5))
        stat[action_name] = {'mean_prob': mean_prob.tolist()}
        acc[0].update(top1, 1)
        acc[1].update(top5, 1)
        args.logger.info('{action_name}Mean: Acc@1: {acc[0].avg:.4f} Acc@5: {acc[1].avg:.4f}'.format(action_name=action_name, acc=acc))
    with open(os.path.join(os.path.dirname(args.test), '%s-classwise_prob-%s.json' % (os.path.basename(args.test), title)), 'w') as fp:
        json.dump(stat, fp)
    return acc


def test_10crop(model, epoch, args):
    """classifier.py:545-654 in one pass over the videos"""
    title = 'ten' if args.ten_crop else ('five' if args.five_crop else 'center')
    args.logger.info('Test using %s crop' % {'center': 'center', 'five': '5', 'ten': '10'}[title])
    views = FD.CROP_VIEWS[title]
    dataset = get_data('test', args, views=views)
    loader = get_dataloader(dataset, 'test', args, batch_size=1)
    model.eval()
    prob_dict = {}
    with torch.no_grad():
        for batch in loader:
            input_seq, _ = model_input(batch, args)
            logit, _ = model(input_seq)
            prob_dict[batch['vpath'][0]] = {'mean_prob': group_probabilities(logit, len(views))}
    fmt = 'test Epoch: [{0}]\tMean: Acc@1: {acc[0].avg:.4f} Acc@5: {acc[1].avg:.4f}'
    if title == 'ten':
        for name, rows in (('center', 1), ('five', 5)):
            args.logger.info('%s-crop result:' % name)
            acc = summarize_probability(prob_dict, dataset.encode_action, name, args, rows=rows)
            args.logger.info('%s-crop:' % name)
            args.logger.info(fmt.format(epoch, acc=acc))
    args.logger.info('%s-crop result:' % title)
    # the reference writes its final summary under the title 'ten' whatever the mode (`:648-649`)
    acc = summarize_probability(prob_dict, dataset.encode_action, 'ten', args)
    args.logger.info('%s-crop:' % title)
    args.logger.info(fmt.format(epoch, acc=acc))
    return acc


def temporal_test_10clip(model, epoch, args):
    """classifier.py:657-738"""
    args.logger.info('Test using temporal 10 center clip crop')
    title = 'temporal_10_clip'
    dataset = get_data('test', args)
    loader = get_dataloader(dataset, 'test', args)
    model.eval()
    prob_dict, cls_prob_dict = {}, {}
    with torch.no_grad():
        for batch in loader:
            input_seq, n_clips = model_input(batch, args)
            if n_clips != 10 * len(batch['vpath']):
                raise ValueError('%d clips for %d videos: the 10-clip test needs ten per video' % (n_clips, len(batch['vpath'])))
            logit, _ = model(input_seq)
            collect_ten_clip(logit, batch, dataset.decode_action, prob_dict, cls_prob_dict)
    args.logger.info('<<<<<< temporal uniform 10 crop result: >>>>>>>>> ')
    acc = summarize_probability(prob_dict, dataset.encode_action, title, args)
    args.logger.info('######## temporal uniform 10 crop classwise result: #########')
    summarize_classwise_probability(cls_prob_dict, dataset.encode_action, title, args)
    return acc


def test_retrieval(model, epoch, args):
    """classifier.py:787-995: ten clips per video, per-video mean feature, centred and normalised k-NN on the train set"""
    from dualvar_amd.utils.retrieval import nn_retrieval, video_features
    model.eval()
    name = args.dataset + '-10clip'
    out_dir = os.path.join(os.path.dirname(args.test), args.dirname if args.dirname is not None else 'feature')
    os.makedirs(out_dir, exist_ok=True)
    feats, clips = {}, {}
    with torch.no_grad():
        for split in ('test', 'train'):
            dataset = get_data(split, args, dataset=name, transform_mode='test', which_split=1)
            args.logger.info('%s dataset size: %d' % (split, len(dataset)))
            args.logger.info('Computing %s set feature ... ' % split)
            feature, per_feature, label, vnames = [], [], [], []
            for batch in get_dataloader(dataset, 'test', args):
                input_seq, n_clips = model_input(batch, args)
                _, feat = model(input_seq)
                feature.append(video_features(feat, args.num_seq))
                per_feature.append(feat.view(n_clips // args.num_seq, args.num_seq, feat.size(-1)).clone())
                label.append(batch['vid'])
                vnames.extend(batch['vname'])
            feature, label = torch.cat(feature, dim=0), torch.cat(label).long()
            args.logger.info(feature.size())
            torch.save(feature, os.path.join(out_dir, '%s_%s_feature.pth.tar' % (args.dataset, split)))
            torch.save(label, os.path.join(out_dir, '%s_%s_label.pth.tar' % (args.dataset, split)))
            with open(os.path.join(out_dir, '%s_%s_vname.pkl' % (args.dataset, split)), 'wb') as fp:
                pickle.dump(vnames, fp)
            per_feature = torch.cat(per_feature, dim=0)
            torch.save(per_feature, os.path.join(out_dir, '%s_%s_per_feature.pth.tar' % (args.dataset, split)))
            feats[split] = (feature, label)
            if args.variance or args.tsne or args.cluster or args.ridge or args.spectrum or args.map:
                clips[split] = per_feature
    acc, sim = nn_retrieval(feats['test'][0], feats['test'][1], feats['train'][0], feats['train'][1], ks=(1, 5, 10, 20, 50))
    torch.save(sim, os.path.join(out_dir, '%s_sim.pth.tar' % args.dataset))
    args.logger.info('NN-Retrieval on %s:' % args.dataset)
    for k, a in acc.items():
        args.logger.info('\t%dNN acc = %.4f' % (k, a))
    if args.knn:
        from dualvar_amd.utils.knn import knn_eval
        res = knn_eval(feats['test'][0], feats['test'][1], feats['train'][0], feats['train'][1], args.num_class, k=args.knn_k,
                       T=args.knn_t, ks=())              # the retrieval accuracies are reported above: lists of the voters only
        if res['k'] < args.knn_k:
            args.logger.info('kNN classifier: k reduced from %d to the train-set size %d' % (args.knn_k, res['k']))
        args.logger.info('kNN classifier (k=%d, T=%g) on %s: Acc@1 = %.4f Acc@5 = %.4f'
                         % (res['k'], args.knn_t, args.dataset, res['knn_top1'], res['knn_top5']))
        torch.save(res['idx'].cpu(), os.path.join(out_dir, '%s_knn_idx.pth.tar' % args.dataset))
        torch.save(res['val'].cpu(), os.path.join(out_dir, '%s_knn_val.pth.tar' % args.dataset))
    if args.variance:
        from dualvar_amd.utils.variance import CATEGORIES, variance_eval

        def show(v):                     # a figure whose pairs are missing is None
            return 'n/a' if v is None else '%.4f' % v
        for split in ('test', 'train'):
            rep = variance_eval(clips[split], feats[split][1], bins=args.var_bins, t=args.var_t)
            args.logger.info('Variance report on %s %s (%d clips, t=%g):' % (args.dataset, split, clips[split].shape[0] * clips[split].shape[1], args.var_t))
            args.logger.info('\tintra-video = %s inter-video = %s ratio = %s' % tuple(show(rep[k]) for k in ('var_intra_video', 'var_inter_video', 'ratio_video')))
            args.logger.info('\tintra-class = %s inter-class = %s ratio = %s' % tuple(show(rep[k]) for k in ('var_intra_class', 'var_inter_class', 'ratio_class')))
            args.logger.info('\talignment = %s uniformity = %s' % (show(rep['alignment']), show(rep['uniformity'])))
            for name in CATEGORIES:
                args.logger.info('\tmean similarity, %s: %s over %d pairs' % (name, show(rep['categories'][name]['mean']), rep['categories'][name]['count']))
            with open(os.path.join(out_dir, '%s_%s_variance.json' % (args.dataset, split)), 'w') as fp:
                json.dump(rep, fp, indent=1)
    if args.tsne:
        for split in (('test', 'train') if args.tsne_split == 'both' else (args.tsne_split,)):
            write_tsne(clips[split], feats[split][1], split, out_dir, args)
    if args.cluster:
        for split in (('test', 'train') if args.cluster_split == 'both' else (args.cluster_split,)):
            write_cluster(clips[split], feats[split][1], split, out_dir, args)
    if args.ridge:
        write_ridge(clips['train'], feats['train'][1], clips['test'], feats['test'][1], out_dir, args)
    if args.spectrum:
        write_spectrum(clips, feats, out_dir, args)
    if args.map:
        write_map(clips, feats, out_dir, args)
    return acc


def write_map(clips, feats, out_dir, args):
    """--map: mean average precision and the other full-ranking figures per level -> <dataset>_map.json (the reports) and
    <dataset>_map.pth.tar (per level: ap, pos_cnt, first_rank of every query); the only writer of these two files"""
    from dualvar_amd.utils.features import clip_rows
    from dualvar_amd.utils.rankeval import ranking_eval, ranking_eval_within

    def show(v):                         # a figure without queries is None
        return 'n/a' if v is None else '%.4f' % v
    ks = sorted(set(args.map_k))
    runs = []
    if args.map_level in ('video', 'both'):
        runs.append(('video', lambda: ranking_eval(feats['test'][0], feats['test'][1], feats['train'][0], feats['train'][1],
                                                   args.num_class, ks=ks)))
    if args.map_level in ('clip', 'both'):
        def clip_level():
            te, _, te_cls, _, _ = clip_rows(clips['test'], feats['test'][1])
            tr, _, tr_cls, _, _ = clip_rows(clips['train'], feats['train'][1])
            return ranking_eval(te, te_cls, tr, tr_cls, args.num_class, ks=ks)
        runs.append(('clip', clip_level))
    if args.map_within:
        runs.append(('within', lambda: ranking_eval_within(clips['test'], feats['test'][1], args.num_class, ks=ks)))
    reports, tensors = {}, {}
    for level, run in runs:
        rep, state = run()
        reports[level] = rep
        tensors[level] = {name: state[name].cpu() for name in ('ap', 'pos_cnt', 'first_rank')}
        args.logger.info('Ranking report on %s, %s level (%d queries, %d without a positive, bank of %d):'
                         % (args.dataset, level, rep['n_query'], rep['n_skipped'], rep['n_bank']))
        args.logger.info('\tmAP = %s macro mAP = %s MRR = %s R-precision = %s'
                         % tuple(show(rep[name]) for name in ('mAP', 'mAP_macro', 'MRR', 'R_precision')))
        for k in ks:
            args.logger.info('\tP@%d = %s recall@%d = %s success@%d = %s'
                             % (k, show(rep['precision_at'][k]), k, show(rep['recall_at'][k]), k, show(rep['success_at'][k])))
    with open(os.path.join(out_dir, '%s_map.json' % args.dataset), 'w') as fp:
        json.dump(reports, fp, indent=1)
    torch.save(tensors, os.path.join(out_dir, '%s_map.pth.tar' % args.dataset))


def write_spectrum(clips, feats, out_dir, args):
    """--spectrum: the eigenvalue spectrum of each split's clip-feature covariance -> <dataset>_{test,train}_spectrum.json, and
    the train fit (mean, leading components, eigenvalues) -> <dataset>_spectrum.pth.tar, with the retrieval repeated on its PCA
    projections in the train JSON; the only writer of these three files"""
    from dualvar_amd.utils.spectrum import pca_retrieval, spectrum_eval

    def show(v):                         # a share whose eigenvalue is numerically zero is None
        return 'n/a' if v is None else '%.4f' % v
    D = clips['train'].shape[-1]
    ks = sorted({min(k, D) for k in args.spectrum_k})
    if any(k > D for k in args.spectrum_k):
        args.logger.info('spectrum: --spectrum_k %s clamped to the feature width %d: %s'
                         % (' '.join(str(k) for k in args.spectrum_k), D, ' '.join(str(k) for k in ks)))
    for split in ('test', 'train'):
        rep = spectrum_eval(clips[split], feats[split][1], ks=tuple(ks))
        met, info = rep['metrics'], rep['info']
        args.logger.info('Spectrum of %s %s (%d clips, D = %d; %d sweeps, %d rotations%s):'
                         % (args.dataset, split, met['n'], met['D'], info['sweeps'], info['rotations'],
                            '' if info['converged'] else ', NOT converged'))
        args.logger.info('\teffective rank = %.2f RankMe = %.2f participation ratio = %.2f numerical rank = %d'
                         % (met['effective_rank'], met['rankme'], met['participation_ratio'], met['numerical_rank']))
        args.logger.info('\ttop-1 share = %s alpha = %s (R2 = %s) dims for 90 / 95 / 99 %% = %s'
                         % (show(met['top1_share']), show(met['alpha']), show(met['alpha_r2']),
                            ' / '.join(str(v) for v in met['dims_for'].values())))
        args.logger.info('\tbetween-video share of the first components: %s' % ' '.join(show(v) for v in rep['video_share'][:8]))
        out = {'metrics': met, 'info': info, 'video_share': rep['video_share'], 'ks': rep['ks'],
               'eigenvalues': rep['eigenvalues'].cpu().tolist()}
        if split == 'train':
            ret_ks = [k for k in rep['ks'] if k % 8 == 0]
            if len(ret_ks) < len(rep['ks']):
                args.logger.info('spectrum: PCA retrieval takes component counts that are multiples of 8: %s left out'
                                 % ' '.join(str(k) for k in rep['ks'] if k % 8))
            res = pca_retrieval(feats['train'][0], feats['train'][1], feats['test'][0], feats['test'][1], rep['mean'],
                                rep['components'], rep['eigenvalues'], ret_ks)
            for k, row in res.items():
                args.logger.info('\tPCA retrieval, %d components: 1NN acc = %.4f whitened = %.4f' % (k, row['pca'], row['whitened']))
            out['pca_retrieval'] = {str(k): row for k, row in res.items()}
            torch.save({'mean': rep['mean'].cpu(), 'components': rep['components'][:rep['ks'][-1]].cpu(),
                        'eigenvalues': rep['eigenvalues'].cpu()}, os.path.join(out_dir, '%s_spectrum.pth.tar' % args.dataset))
        with open(os.path.join(out_dir, '%s_%s_spectrum.json' % (args.dataset, split)), 'w') as fp:
            json.dump(out, fp, indent=1)


def write_ridge(train_clips, train_label, test_clips, test_label, out_dir, args):
    """--ridge: the closed-form ridge probe, fitted on the train clips and scored on the test clips -> <dataset>_ridge.{json,
    pth.tar}; the only writer of these two files"""
    from dualvar_amd.utils.probe import ridge_probe
    rep = ridge_probe(train_clips, train_label, test_clips, test_label, args.num_class, lambdas=tuple(args.ridge_lambda),
                      holdout=args.ridge_holdout)
    for row in rep['sweep']:
        args.logger.info('ridge probe, lambda = %g: held-out clip Acc@1 = %.4f Acc@5 = %.4f video Acc@1 = %.4f Acc@5 = %.4f'
                         % (row['lambda'], row['clip_top1'], row['clip_top5'], row['video_top1'], row['video_top5']))
    args.logger.info('ridge probe on %s (%d train clips, %d videos held out, lambda = %g): clip Acc@1 = %.4f Acc@5 = %.4f '
                     'video Acc@1 = %.4f Acc@5 = %.4f' % (args.dataset, rep['n_train'], rep['n_held_videos'], rep['lambda'],
                                                          rep['clip_top1'], rep['clip_top5'], rep['video_top1'], rep['video_top5']))
    stem = os.path.join(out_dir, '%s_ridge' % args.dataset)
    torch.save({'W': rep['W'].cpu(), 'lambda': rep['lambda']}, stem + '.pth.tar')
    with open(stem + '.json', 'w') as fp:
        json.dump({k: v for k, v in rep.items() if k != 'W'}, fp, indent=1)


def write_cluster(per_feature, label, split, out_dir, args):
    """--cluster: spherical k-means of one split's clip features -> <dataset>_<split>_cluster.{json, pth.tar}; the only writer
    of these two files"""
    from dualvar_amd.utils.cluster import cluster_eval
    n = per_feature.shape[0] * per_feature.shape[1]
    k = min(args.cluster_k or args.num_class, n)
    if k < (args.cluster_k or args.num_class):
        args.logger.info('k-means: clusters reduced from %d to %d, the %s split holds %d clips' % (args.cluster_k or args.num_class, k, split, n))
    fit, rep = cluster_eval(per_feature, label, k=k, n_class=args.num_class, n_iter=args.cluster_iter, n_init=args.cluster_init,
                            seed=args.cluster_seed)
    args.logger.info('k-means of %s %s (%d clips, k=%d, %d restarts, %d iterations, %d empty): NMI = %.4f ARI = %.4f purity = %.4f '
                     'accuracy = %.4f video consistency = %.4f'
                     % (args.dataset, split, n, k, args.cluster_init, fit['iterations'], fit['empty'], rep['nmi'], rep['ari'],
                        rep['purity'], rep['accuracy'], rep['video_consistency']))
    stem = os.path.join(out_dir, '%s_%s_cluster' % (args.dataset, split))
    torch.save({'assign': fit['assign'].cpu(), 'centroids': fit['centroids'].cpu()}, stem + '.pth.tar')
    with open(stem + '.json', 'w') as fp:
        json.dump({'k': k, 'n_iter': args.cluster_iter, 'n_init': args.cluster_init, 'seed': args.cluster_seed, 'n': n,
                   'objective': fit['objective'], 'iterations': fit['iterations'], 'restart': fit['restart'], 'empty': fit['empty'],
                   'init_index': fit['init_index'], 'trace': fit['trace'], 'sizes': fit['sizes'], 'metrics': rep}, fp, indent=1)


def write_tsne(per_feature, label, split, out_dir, args):
    """--tsne: the t-SNE map of one split's clip features -> <dataset>_<split>_tsne.{pth.tar, json, png}; the only writer of
    these three files"""
    from dualvar_amd.utils.embed import tsne_eval
    n = per_feature.shape[0] * per_feature.shape[1]
    y, trace, rep, k = tsne_eval(per_feature, label, perplexity=args.tsne_perplexity, n_iter=args.tsne_iter, seed=args.tsne_seed)
    if k < 3 * args.tsne_perplexity:
        args.logger.info('t-SNE: neighbours per clip reduced from %d to %d, the %s split holds %d clips'
                         % (3 * args.tsne_perplexity, k, split, n))
    args.logger.info('t-SNE map of %s %s (%d clips, perplexity=%d, %d iterations): CE = %.4f Z = %.4g'
                     % (args.dataset, split, n, args.tsne_perplexity, args.tsne_iter, trace['ce'][-1], trace['z'][-1]))
    args.logger.info('\tpurity video = %.4f purity class = %.4f kNN preservation = %.4f (k=%d)'
                     % (rep['purity_video'], rep['purity_class'], rep['knn_preservation'], rep['k']))
    stem = os.path.join(out_dir, '%s_%s_tsne' % (args.dataset, split))
    torch.save(y, stem + '.pth.tar')
    with open(stem + '.json', 'w') as fp:
        json.dump({'perplexity': args.tsne_perplexity, 'n_iter': args.tsne_iter, 'seed': args.tsne_seed, 'neighbours': k, 'n': n,
                   'trace': trace, 'z': trace['z'][-1], 'report': rep}, fp, indent=1)
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return
    lo, hi = y.min(0).values, y.max(0).values
    xy = ((y - lo) / (hi - lo).clamp(min=1e-12)).numpy()                    # min-max scaled to [0, 1]^2, as the paper's figure
    cls = torch.as_tensor(label).cpu().long().repeat_interleave(per_feature.shape[1]).numpy()
    fig = plt.figure(figsize=(6, 6))
    plt.scatter(xy[:, 0], xy[:, 1], c=cls, s=3, cmap='nipy_spectral')
    plt.xlim(-0.02, 1.02)
    plt.ylim(-0.02, 1.02)
    plt.axis('off')
    fig.savefig(stem + '.png', dpi=150, bbox_inches='tight')
    plt.close(fig)


# --------------------------------------------------------------------------------------------------------------- main
def main(args):
    check_args(args)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    args.distributed, args.rank = False, 0
    args.gpu = args.gpu if args.gpu is not None else 0
    torch.cuda.set_device(args.gpu)
    if args.split_root:
        from dualvar_amd.utils.frame_dataset import read_classes
        args.num_class = len(read_classes(args.split_root))
    else:
        args.num_class = FD.NUM_CLASS[args.dataset]
    split_root, frame_root, _ = FD.DATASETS[args.dataset]
    args.split_root = args.split_root or os.path.join(ROOT, split_root)
    args.frame_root = args.frame_root or os.path.join(ROOT, frame_root)
    args.img_path, args.model_path, args.exp_path, args.log_file = set_path(args)
    args.logger = DistLogger(args.log_file, True)
    args.logger.info('=> Effective BatchSize = %d' % args.batch_size)

    from dualvar_amd.model import LinearClassifier
    from dualvar_amd.optim import SGD, Adam
    model = LinearClassifier(network=args.net, num_class=args.num_class, dropout=args.dropout, use_dropout=args.use_dropout,
                             use_final_bn=args.use_bn, use_l2_norm=args.use_norm)
    message = 'Classifier to %d classes with %s backbone;' % (args.num_class, args.net)
    message += ' + L2Norm' * args.use_norm + ' + final BN' * args.use_bn + (' + dropout %f' % args.dropout) * args.use_dropout
    args.logger.info(message)
    model.set_compute_dtype(args.dtype)
    model.set_input_normalization(MEAN, STD)
    model.cuda(args.gpu)

    if args.train_what == 'last':
        args.logger.info('=> [optimizer] only train last layer')
        params = []
        for name, param in model.named_parameters():
            if 'backbone' in name:
                param.requires_grad = False
            else:
                params.append({'params': [param]})
                args.logger.info('%s %s' % (name, param.requires_grad))
    else:
        args.logger.info('=> [optimizer] finetune all layer')
        params = [{'params': [param]} for _, param in model.named_parameters()]
    if args.optim == 'adam':
        optimizer = Adam(params, lr=args.lr, weight_decay=args.wd, stores=model.stores())
    else:
        optimizer = SGD(params, lr=args.lr, weight_decay=args.wd, momentum=0.9, stores=model.stores())
    args.logger.info(' => use %s optimizer' % args.optim)
    # the parameter arenas exist from here on (not only after the first forward): --resume loads the optimizer state into them
    model.backbone.prepare(torch.device('cuda', args.gpu))
    args.iteration = 1
    best_acc = 0

    if args.test:
        epoch = 0
        if os.path.isfile(args.test):
            args.logger.info("=> loading testing checkpoint '{}'".format(args.test))
            checkpoint = torch.load(args.test, map_location='cpu', weights_only=True)
            epoch, state_dict = checkpoint['epoch'], checkpoint['state_dict']
            if args.retrieval:                                    # directly on a pretrained network
                state_dict = {k.replace('encoder_q.0.', 'backbone.').replace('linear_fc', 'pretrain_fc'): v for k, v in state_dict.items()}
            try:
                model.load_state_dict(state_dict)
            except Exception:
                neq_load_customized(model, state_dict, verbose=True, args=args)
        else:
            args.logger.info("[Warning] no checkpoint found at '{}'".format(args.test))
        if args.retrieval:
            test_retrieval(model, epoch, args)
        elif args.center_crop or args.five_crop or args.ten_crop:
            test_10crop(model, epoch, args)
        else:
            temporal_test_10clip(model, epoch, args)
        return 0

    train_loader = get_dataloader(get_data('train', args), 'train', args)
    val_loader = get_dataloader(get_data('val', args), 'val', args)
    args.logger.info('===================================')
    if args.resume:
        if os.path.isfile(args.resume):
            checkpoint = torch.load(args.resume, map_location='cpu', weights_only=True)
            args.start_epoch, args.iteration, best_acc = checkpoint['epoch'] + 1, checkpoint['iteration'], checkpoint['best_acc']
            try:
                model.load_state_dict(checkpoint['state_dict'])
            except Exception:
                args.logger.info('[WARNING] resuming training with different weights')
                neq_load_customized(model, checkpoint['state_dict'], verbose=True, args=args)
            args.logger.info("=> load resumed checkpoint '{}' (epoch {})".format(args.resume, checkpoint['epoch']))
            try:
                n = optimizer.load_state_dict(checkpoint['optimizer'])
                if args.optim == 'adam':
                    args.logger.info('Adam state restored: %d tensors, step %d, |exp_avg| %.6e, |exp_avg_sq| %.6e'
                                     % ((n,) + optimizer.moment_summary()))
                else:
                    args.logger.info('optimizer state restored (%d momentum buffers)' % n)
            except Exception as e:
                args.logger.info('[WARNING] failed to load optimizer state, initialize optimizer: %s' % e)
        else:
            args.logger.info("[Warning] no checkpoint found at '{}', use random init".format(args.resume))
    elif args.pretrain:
        if not os.path.isfile(args.pretrain):
            refuse("no checkpoint found at '%s'" % args.pretrain)
        checkpoint = torch.load(args.pretrain, map_location='cpu', weights_only=True)
        state_dict = {k.replace('encoder_q.0.', 'backbone.').replace('final_fc', 'pretrain_fc'): v
                      for k, v in checkpoint['state_dict'].items()}
        try:
            model.load_state_dict(state_dict)
        except Exception:
            neq_load_customized(model, state_dict, verbose=True, args=args)
        args.logger.info("=> loaded pretrained checkpoint '{}' (epoch {})".format(args.pretrain, checkpoint['epoch']))
    else:
        args.logger.info('=> train from scratch')

    for epoch in range(args.start_epoch, args.epochs):
        np.random.seed(epoch)
        random.seed(epoch)
        adjust_learning_rate(optimizer, epoch, args)
        train_one_epoch(train_loader, model, optimizer, epoch, args)
        if (epoch + 1) % args.eval_freq == 0:
            _, val_acc = validate(val_loader, model, epoch, args)
            is_best = val_acc > best_acc
            best_acc = max(val_acc, best_acc)
            save_checkpoint({'epoch': epoch, 'state_dict': model.state_dict(), 'best_acc': best_acc,
                             'optimizer': optimizer.state_dict(), 'iteration': args.iteration}, is_best, 0,
                            filename=os.path.join(args.model_path, 'epoch%d.pth.tar' % epoch), keep_all=False,
                            is_save=((epoch + 1) % args.save_freq == 0))
    args.logger.info('Training from ep %d to ep %d finished' % (args.start_epoch, args.epochs))
    return 0


if __name__ == '__main__':
    sys.exit(main(parse_args()))
