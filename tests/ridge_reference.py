"""Float64 reference of the closed-form ridge probe (include/dualvar_ridge.h, dualvar_amd/utils/probe.py), in numpy and written
independently of both: the slab cut and the workspace formula of the header, the Gram matrix and the class sums in the header's
slab order, the penalised system, np.linalg.solve, the stratified hold-out and the whole probe (sweep, choice, refit, scores).
tests/test_ridge_host.py checks it against np.linalg.lstsq on the stacked system [Z~; sqrt(lambda) I_pen]."""
import numpy as np
import torch

from tests.checks import ceil_div

MAX_D, MAX_C, SLAB, MAX_SLABS, TILE = 4096, 4096, 512, 8, 64
LAMBDAS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
U32 = 2.0 ** -24


def slab_cut(n):
    """-> (rows per slab, slabs)"""
    rows = ceil_div(ceil_div(n, SLAB), MAX_SLABS) * SLAB
    return rows, ceil_div(n, rows)


def gram_workspace_bytes(n, D, C):
    Da, T = D + 1, ceil_div(D + 1, TILE)
    return 8 * slab_cut(n)[1] * (T * (T + 1) // 2 * TILE * TILE + C * Da)


def augment(z):
    z = np.asarray(z, dtype=np.float64)
    return np.concatenate([z, np.ones((z.shape[0], 1))], axis=1)


def gram_ref(z, label, C):
    """z [n][D] (any float type, taken to float64 exactly), label [n] -> (G [Da][Da], B [Da][C]) over the live rows: one partial
    per slab, the slabs added in ascending order from 0.0"""
    zt, label = augment(z), np.asarray(label)
    n, Da = zt.shape
    rows, P = slab_cut(n)
    G, B = np.zeros((Da, Da)), np.zeros((Da, C))
    for p in range(P):
        sl = slice(p * rows, min(n, (p + 1) * rows))
        zs, ls = zt[sl], label[sl]
        live = (ls >= 0) & (ls < C)
        zs, ls = zs[live], ls[live]
        G = G + zs.T @ zs
        Y = np.zeros((zs.shape[0], C))
        Y[np.arange(zs.shape[0]), ls] = 1.0
        B = B + zs.T @ Y
    return G, B


def abs_gram(z, label, C):
    """(|Z~|^T |Z~|, |Z~|^T Y) over the live rows: the right-hand sides of the summation bounds"""
    return gram_ref(np.abs(np.asarray(z, dtype=np.float64)), label, C)


def penalised(G, lam, n_pen):
    A = np.array(G, dtype=np.float64)
    idx = np.arange(n_pen)
    A[idx, idx] = A[idx, idx] + lam
    return A


def solve_ref(G, B, lam, n_pen):
    return np.linalg.solve(penalised(G, lam, n_pen), B)


def holdout_mask_ref(video_class, every=5):
    cls = np.asarray(video_class).reshape(-1)
    mask = np.zeros(cls.size, dtype=bool)
    for c in np.unique(cls):
        where = np.flatnonzero(cls == c)
        mask[where[every - 1::every]] = True
    return mask


def normalise_ref(clips):
    """[V][S][D] fp32 -> [V * S][D] float64: x / max(|x|, 1e-12)"""
    x = np.asarray(clips, dtype=np.float64).reshape(-1, np.asarray(clips).shape[-1])
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def rank0(score, label):
    """classes scoring strictly above the target, per row"""
    score, label = np.asarray(score), np.asarray(label)
    return (score > score[np.arange(score.shape[0]), label][:, None]).sum(1)


def scores_ref(z, W, video_label, S):
    """-> dict as dualvar_amd.utils.probe.ridge_scores fills it, in float64, plus 'clip_margin' [n] and 'video_margin' [videos]:
    the distance of the target's score to the nearest other score of the row (the top-2 margin where the target leads): as long
    as the fp32 scores move by less than half of it, rank0 and with it every top-k count is the float64 one"""
    logits = augment(z) @ W
    V = logits.shape[0] // S
    video = logits.reshape(V, S, -1).mean(1)
    vl = np.asarray(video_label).reshape(-1)
    out = {'logits': logits, 'video_score': video}
    for name, x, lab in (('clip', logits, np.repeat(vl, S)), ('video', video, vl)):
        r = rank0(x, lab)
        out[name + '_rank0'] = r
        gap = np.abs(x - x[np.arange(x.shape[0]), lab][:, None])
        gap[np.arange(x.shape[0]), lab] = np.inf
        out[name + '_margin'] = gap.min(1)
        for k in (1, 5):
            out['%s_top%d' % (name, k)] = int((r < k).sum()) / x.shape[0]
    return out


def gemm_chain_tile4(K):
    """the longest chain of fp32 additions of dv_gemm_f32_ex's four-wave kernel (gemm_chain of tests/chains.py)"""
    return 16 * ceil_div(ceil_div(K, 16), 4) + 3


def score_bound(z, W, S):
    """the fp32 GEMM element bound of test_loss_gemm_optim_gpu.py, (L + 2) u sum_k |a_k b_k| with the bias as one more term, per
    row, the largest over the classes -> (per clip [n], per video [n / S]: the mean over its clips)"""
    D = z.shape[1]
    b = (gemm_chain_tile4(D) + 2) * U32 * (np.abs(augment(z)) @ np.abs(W))
    return b.max(1), b.reshape(b.shape[0] // S, S, -1).mean(1).max(1)


def _margins(sc, bounds):
    return np.concatenate([sc['clip_margin'], sc['video_margin']]), np.concatenate(bounds)


def probe_ref(train_clips, train_label, test_clips, test_label, n_class, lambdas=LAMBDAS, holdout=5, normalise=None):
    """the report of ridge_probe in float64 (without 'W'), plus 'margins': per scored set (one per lambda, then the test split)
    the pairs (margin, fp32 bound) of its clip rows and of its video rows, concatenated.  `normalise` maps [V][S][D] clips to
    [V * S][D] float64 rows (the GPU test hands in the rows the library normalised, so that both sides solve the same system)"""
    train_clips, test_clips = np.asarray(train_clips), np.asarray(test_clips)
    V, S, D = train_clips.shape
    tl = np.asarray(train_label).reshape(-1)
    normalise = normalise or normalise_ref
    z = normalise(train_clips)
    held_video = holdout_mask_ref(tl, holdout)
    held_rows = np.repeat(held_video, S)
    cl = np.repeat(tl, S)
    n, n_held = V * S, int(held_rows.sum())
    G_fit, B_fit = gram_ref(z, np.where(held_rows, -1, cl), n_class)
    G_held, B_held = gram_ref(z, np.where(held_rows, cl, -1), n_class)
    sweep, margins = [], []
    if n_held:
        best = None
        for lam in lambdas:
            W = solve_ref(G_fit, B_fit, lam * (n - n_held), D)
            sc = scores_ref(z[held_rows], W, tl[held_video], S)
            margins.append(_margins(sc, score_bound(z[held_rows], W, S)))
            sweep.append({'lambda': lam, 'clip_top1': sc['clip_top1'], 'clip_top5': sc['clip_top5'], 'video_top1': sc['video_top1'],
                          'video_top5': sc['video_top5']})
            if best is None or (sc['video_top1'], lam) > best:
                best = (sc['video_top1'], lam)
        chosen = best[1]
    else:
        chosen = lambdas[0] if len(lambdas) == 1 else lambdas[len(lambdas) // 2]
    W = solve_ref(G_fit + G_held, B_fit + B_held, chosen * n, D)
    zt = normalise(test_clips)
    sc = scores_ref(zt, W, test_label, test_clips.shape[1])
    margins.append(_margins(sc, score_bound(zt, W, test_clips.shape[1])))
    return {'lambda': chosen, 'sweep': sweep, 'clip_top1': sc['clip_top1'], 'clip_top5': sc['clip_top5'],
            'video_top1': sc['video_top1'], 'video_top5': sc['video_top5'], 'n_train': n, 'n_fit': n - n_held,
            'n_held_videos': int(held_video.sum()), 'n_class': n_class, 'D': D, 'margins': margins}


def probe_fixture():
    """60 videos of 2 clips in 6 classes at D = 129, all draws from one generator in a fixed order -> (clips [60][2][129] fp32,
    label [60])"""
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(6, 129, generator=g)
    label = torch.arange(60) % 6
    offset = 0.5 * torch.randn(60, 129, generator=g)
    clips = centres[label][:, None, :] + offset[:, None, :] + 4.0 * torch.randn(60, 2, 129, generator=g)
    return clips.float(), label
