"""Supervised linear read-out of an encoder's clip features without an optimiser: multi-class ridge regression onto one-hot
targets, W = (Z~^T Z~ + lambda n diag(1, ..., 1, 0))^-1 Z~^T Y with Z~ = (Z, 1) (the intercept is not penalised), one closed
form per lambda.  The normal equations are formed once in double by `dv_ridge_gram_f64` and solved per lambda by
`dv_ridge_solve_f64` (include/dualvar_ridge.h: blocked Cholesky, substitution), every sum in a fixed order, so the same features
give the same bits.  lambda is chosen on a stratified hold-out of the training videos: the held rows are left out of the first
system and added by a second, accumulating call, so each feature row is read once per system and the refit on all rows costs no
further pass.  The scores are fp32 (`dv_gemm_f32_ex` with the intercept as bias), averaged over a video's clips
(`dv_group_mean_f32`) and ranked by `dv_softmax_ce_fwd`'s rank0.  The host does the control flow and counts hits."""
import ctypes as C
import math

import torch

from .. import _lib as L
from .. import ops
from . import features as F

LAMBDAS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)


def holdout_mask(video_class, every=5):
    """video_class [V] -> bool [V]: the j-th video of a class in dataset order (j from 0 within its class) is held out iff
    j % every == every - 1.  Stratified on purpose: index % every aliases with a dataset laid out class by class or round-robin.
    A class with fewer than `every` videos holds none out."""
    every = int(every)
    if every < 2:
        raise ValueError('every = %d: hold out one video in at least 2' % every)
    cls = torch.as_tensor(video_class).reshape(-1).cpu().long().tolist()
    seen, mask = {}, []
    for c in cls:
        j = seen.get(c, 0)
        seen[c] = j + 1
        mask.append(j % every == every - 1)
    return torch.tensor(mask, dtype=torch.bool)


def _check_lambdas(lambdas):
    lam = [float(v) for v in lambdas]
    if not lam or any(not (v > 0 and math.isfinite(v)) for v in lam):
        raise ValueError('every lambda must be positive and finite, got %r' % (lam,))
    return lam


def _check_z(z):
    if z.dim() != 2 or z.shape[0] < 1 or not 1 <= z.shape[1] <= L.DV_RIDGE_MAX_D:
        raise ValueError('z must be [n, D] clip features with 1 <= D <= %d (DV_RIDGE_MAX_D), got %s' % (L.DV_RIDGE_MAX_D, tuple(z.shape)))


def ridge_gram(z, label, n_class, G, B, accumulate, ws):
    """one dv_ridge_gram_f64 launch: z [n, D] fp32, label [n] int32 (-1: the row is left out), G [D + 1, D + 1], B [D + 1, n_class]
    float64, all contiguous on the device; ws from dv_ridge_gram_workspace(n, D, n_class)"""
    n, D = z.shape
    L.check(L.load().dv_ridge_gram_f64(z.data_ptr(), D, n, D, label.data_ptr(), n_class, G.data_ptr(), D + 1, B.data_ptr(), n_class,
                                       int(accumulate), ws.data_ptr(), ops.stream_ptr()), 'dv_ridge_gram_f64')


def ridge_systems(z, clip_label, held_rows, n_class=None):
    """z [n, D] fp32 on the device, clip_label [n] (0 <= label < n_class; n_class defaults to the largest label + 1), held_rows
    [n] bool -> (G_fit [Da, Da], B_fit [Da, n_class], G_full, B_full) in float64 on the device, Da = D + 1: the normal equations
    of the rows not held and of all rows.  Two calls of dv_ridge_gram_f64: the first with label -1 on the held rows, the second
    on the held rows alone, accumulating into a copy of the first."""
    _check_z(z)
    n, D = z.shape
    label = torch.as_tensor(clip_label).reshape(-1)
    held = torch.as_tensor(held_rows).reshape(-1).bool()
    if label.numel() != n or held.numel() != n:
        raise ValueError('clip_label and held_rows must hold one entry per row (%d), got %d and %d' % (n, label.numel(), held.numel()))
    n_class = int(n_class) if n_class else int(label.max()) + 1
    if not 1 <= n_class <= L.DV_RIDGE_MAX_C:
        raise ValueError('n_class = %d: the ridge kernels keep 1 <= n_class <= %d (DV_RIDGE_MAX_C)' % (n_class, L.DV_RIDGE_MAX_C))
    L.require_device()
    dev = z.device if z.is_cuda else torch.device('cuda')
    z = z.to(dev).float().contiguous()
    label = label.to(device=dev, dtype=torch.int32)
    held = held.to(dev)
    ws = F.workspace(L.load().dv_ridge_gram_workspace(n, D, n_class), dev, 'dv_ridge_gram_workspace')
    G = torch.empty(D + 1, D + 1, dtype=torch.float64, device=dev)
    B = torch.empty(D + 1, n_class, dtype=torch.float64, device=dev)
    minus = torch.full_like(label, -1)
    ridge_gram(z, torch.where(held, minus, label).contiguous(), n_class, G, B, 0, ws)
    G_full, B_full = G.clone(), B.clone()
    if bool(held.any()):
        ridge_gram(z, torch.where(held, label, minus).contiguous(), n_class, G_full, B_full, 1, ws)
    return G, B, G_full, B_full


def ridge_solve(G, B, lam, n_pen):
    """G [Da, Da], B [Da, C] float64 on the device -> W [Da, C] float64 = (G + lam diag(1 x n_pen, 0 ...))^-1 B by
    dv_ridge_solve_f64; raises DualVarHipError naming the pivot if the matrix is not positive definite to working precision"""
    if G.dim() != 2 or G.shape[0] != G.shape[1] or B.dim() != 2 or B.shape[0] != G.shape[0]:
        raise ValueError('G must be [Da, Da] and B [Da, C], got %s and %s' % (tuple(G.shape), tuple(B.shape)))
    if G.dtype != torch.float64 or B.dtype != torch.float64:
        raise ValueError('G and B must be float64')
    lam = float(lam)
    if not (lam >= 0 and math.isfinite(lam)):
        raise ValueError('lam must be finite and not negative')
    L.require_device()
    G, B = G.contiguous(), B.contiguous()
    Da, Cn = B.shape
    W, chol = torch.empty_like(B), torch.empty_like(G)
    info = torch.empty(1, dtype=torch.int32, device=G.device)
    L.check(L.load().dv_ridge_solve_f64(G.data_ptr(), Da, Da, int(n_pen), lam, B.data_ptr(), Cn, Cn, W.data_ptr(), Cn, chol.data_ptr(),
                                        Da, info.data_ptr(), ops.stream_ptr()), 'dv_ridge_solve_f64')
    piv = int(info.item())
    if piv:
        raise L.DualVarHipError('dv_ridge_solve_f64: pivot %d of %d is not a finite positive number (lambda = %g): the system is not '
                                'positive definite, raise lambda' % (piv, Da, lam))
    return W


def ridge_scores(z, W, video_label=None, num_seq=1):
    """z [n, D] fp32 on the device (n = videos * num_seq, a video's clips adjacent), W [D + 1, C] float64 -> {'logits' [n, C] fp32 =
    z W[:D] + W[D] (W cast to fp32 once), 'video_score' [videos, C]: the mean over a video's clips}; with video_label [videos]
    also 'clip_rank0' [n] and 'video_rank0' [videos] (classes scoring above the target, int32) and 'clip_top1', 'clip_top5',
    'video_top1', 'video_top5' (hits / rows, counted as utils.topk_from_rank does)"""
    _check_z(z)
    n, D = z.shape
    if W.dim() != 2 or W.shape[0] != D + 1:
        raise ValueError('W must be [D + 1, C] = [%d, C], got %s' % (D + 1, tuple(W.shape)))
    num_seq = int(num_seq)
    if num_seq < 1 or n % num_seq:
        raise ValueError('%d rows are no whole number of videos of %d clips' % (n, num_seq))
    L.require_device()
    lib, s = L.load(), ops.stream_ptr()
    dev = z.device if z.is_cuda else torch.device('cuda')
    z = z.to(dev).float().contiguous()
    w32 = W.to(device=dev, dtype=torch.float32).contiguous()
    Cn, V = w32.shape[1], n // num_seq
    logits = torch.empty(n, Cn, dtype=torch.float32, device=dev)
    d = F.gemm_desc(z.data_ptr(), w32.data_ptr(), logits.data_ptr(), n, Cn, D, Cn, 1, bias=w32.data_ptr() + 4 * D * Cn)
    L.check(lib.dv_gemm_f32_ex(C.byref(d), s), 'dv_gemm_f32_ex')
    video = torch.empty(V, Cn, dtype=torch.float32, device=dev)
    L.check(lib.dv_group_mean_f32(logits.data_ptr(), V, num_seq, Cn, video.data_ptr(), s), 'dv_group_mean_f32')
    out = {'logits': logits, 'video_score': video}
    if video_label is not None:
        vl = torch.as_tensor(video_label).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if vl.numel() != V:
            raise ValueError('video_label must hold one label per video (%d), got %d' % (V, vl.numel()))
        for name, x, lab in (('clip', logits, vl.repeat_interleave(num_seq).contiguous()), ('video', video, vl)):
            rows = torch.empty(x.shape[0], dtype=torch.float32, device=dev)
            rank0 = torch.empty(x.shape[0], dtype=torch.int32, device=dev)
            L.check(lib.dv_softmax_ce_fwd(x.data_ptr(), Cn, x.shape[0], Cn, lab.data_ptr(), rows.data_ptr(), None, Cn, rank0.data_ptr(), s),
                    'dv_softmax_ce_fwd')
            out[name + '_rank0'] = rank0
            for k in (1, 5):
                out['%s_top%d' % (name, k)] = int((rank0 < k).sum()) / x.shape[0]
    return out


def ridge_probe(train_clips, train_label, test_clips, test_label, n_class, lambdas=LAMBDAS, holdout=5):
    """train_clips [V, S, D] with train_label [V], test_clips [Vt, St, D] with test_label [Vt] -> the report of the closed-form
    ridge probe: {'lambda' (the one kept), 'sweep' (per lambda: held-out clip / video top-1 / top-5), 'clip_top1', 'clip_top5',
    'video_top1', 'video_top5' on the test split, 'n_train', 'n_fit', 'n_held_videos', 'n_class', 'D', 'W' [D + 1, n_class]
    float64 on the device}.
    Every lambda of the grid is solved on the system of the videos not held out (holdout_mask, one in `holdout` per class) with
    lambda * n_fit on the D feature rows of the diagonal and scored on the held-out videos; the lambda of largest held-out video
    top-1 is kept, the larger among equals; the refit on all training clips uses lambda * n_train.  If no video can be held
    out the sweep is skipped and the single lambda given, or the middle one of the grid, is used."""
    train, _, cls, V, S = F.clip_rows(train_clips, train_label)
    test, _, _, _, St = F.clip_rows(test_clips, test_label)
    D = train.shape[1]
    if test.shape[1] != D:
        raise ValueError('train_clips and test_clips must be [V, S, D] with one D, got %s and %s' % (tuple(train_clips.shape), tuple(test_clips.shape)))
    lam = _check_lambdas(lambdas)
    n_class = int(n_class)
    tl = cls[::S]                        # the videos' labels, int64 on the host
    if int(tl.min()) < 0 or int(tl.max()) >= n_class:
        raise ValueError('train labels must lie in [0, n_class)')
    held_video = holdout_mask(tl, holdout)
    L.require_device()
    z = F.normalise(train)
    n = V * S
    held_rows = held_video.repeat_interleave(S)
    n_held = int(held_rows.sum())
    G_fit, B_fit, G_full, B_full = ridge_systems(z, cls, held_rows, n_class=n_class)
    sweep = []
    if n_held:
        z_held = z[held_rows.to(z.device)].contiguous()
        held_label = tl[held_video]
        best = None
        for v in lam:
            W = ridge_solve(G_fit, B_fit, v * (n - n_held), D)
            sc = ridge_scores(z_held, W, held_label, S)
            sweep.append({'lambda': v, 'clip_top1': sc['clip_top1'], 'clip_top5': sc['clip_top5'], 'video_top1': sc['video_top1'],
                          'video_top5': sc['video_top5']})
            if best is None or (sc['video_top1'], v) > best:
                best = (sc['video_top1'], v)
        chosen = best[1]
    else:
        chosen = lam[0] if len(lam) == 1 else lam[len(lam) // 2]
    W = ridge_solve(G_full, B_full, chosen * n, D)
    sc = ridge_scores(F.normalise(test), W, test_label, St)
    return {'lambda': chosen, 'sweep': sweep, 'clip_top1': sc['clip_top1'], 'clip_top5': sc['clip_top5'],
            'video_top1': sc['video_top1'], 'video_top5': sc['video_top5'], 'n_train': n, 'n_fit': n - n_held,
            'n_held_videos': int(held_video.sum()), 'n_class': n_class, 'D': D, 'W': W}
