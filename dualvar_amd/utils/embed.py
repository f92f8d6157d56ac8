"""t-SNE feature map of an encoder's clip features (the picture of the feature distribution: SimCLR collapses a video's clips
into a dot, the dual representation spreads them), on the entries of include/dualvar_tsne.h.  Attraction runs over the
k = 3 * perplexity nearest neighbours in feature space (knn.topk_neighbours: the [n, n] similarity is never formed), repulsion is
the exact sum over all ordered pairs of 2-D points (dv_tsne_repulse_f32: no tree, no grid), and every sum has a fixed order, so
the same features, seed and parameters give the same bits.  All floating-point arithmetic on the features and the map runs in
the HIP library; the host does index bookkeeping (the reverse neighbour lists) and enqueues the loop."""
import math

import torch

from .. import _lib as L
from .. import ops
from . import features as F
from . import knn

MIN_GAIN = 0.01
MOMENTUM = (0.5, 0.8)                # during / after the early exaggeration


def _check_perplexity(perplexity):
    if not (perplexity >= 2 and math.isfinite(perplexity)):
        raise ValueError('perplexity must be finite and at least 2')
    if 3 * int(perplexity) + 1 > L.DV_TOPK_MAX_K:
        raise ValueError('perplexity = %g: the lists hold 3 * perplexity + 1 <= %d (DV_TOPK_MAX_K) neighbours' % (perplexity, L.DV_TOPK_MAX_K))


def _check_feat(feat):
    if feat.dim() != 2 or feat.shape[0] < 2:
        raise ValueError('feat must be [n, D] clip features with n >= 2, got %s' % (tuple(feat.shape),))
    L.require_device()                   # no GPU: DualVarHipError, there is no other path
    if not feat.is_cuda:
        raise ValueError('feat must be a device tensor (the kernels read the pointers as they are)')


def reverse_csr(top_idx, included):
    """top_idx [n, ldk] int, included [n, ldk] bool -> (rev_ptr [n + 1] i32, rev_edge [E] i32): for every row i the flat
    positions j * ldk + slot of the included entries that point at i, in ascending flat position.  One stable sort of the
    included targets, a bincount and a cumsum: integer bookkeeping only."""
    n = top_idx.shape[0]
    flat = included.reshape(-1).nonzero().reshape(-1)                       # ascending flat positions
    target = top_idx.reshape(-1)[flat].long()
    order = torch.sort(target, stable=True).indices
    rev_edge = flat[order].to(torch.int32)
    rev_ptr = torch.zeros(n + 1, dtype=torch.int64, device=top_idx.device)
    rev_ptr[1:] = torch.cumsum(torch.bincount(target, minlength=n), 0)
    return rev_ptr.to(torch.int32), rev_edge


def affinities_from_lists(val, idx, perplexity, row0=0):
    """neighbour lists [n, k1] (as knn.topk_neighbours returns them, the point itself among them) -> the dict tsne_embed walks:
    'idx', 'p' [n, k1], 'beta' [n], 'rev_ptr' [n + 1], 'rev_edge' [E], 'k1'"""
    L.require_device()
    n, k1 = val.shape
    val, idx = val.float().contiguous(), idx.to(torch.int32).contiguous()
    p = torch.empty(n, k1, dtype=torch.float32, device=val.device)
    beta = torch.empty(n, dtype=torch.float32, device=val.device)
    L.check(L.load().dv_tsne_perplexity_f32(val.data_ptr(), idx.data_ptr(), k1, n, k1, row0, float(perplexity), p.data_ptr(),
                                            beta.data_ptr(), ops.stream_ptr()), 'dv_tsne_perplexity_f32')
    rows = torch.arange(row0, row0 + n, device=idx.device, dtype=torch.int32)[:, None]
    rev_ptr, rev_edge = reverse_csr(idx, (idx >= 0) & (idx != rows))
    return {'idx': idx, 'p': p, 'beta': beta, 'rev_ptr': rev_ptr, 'rev_edge': rev_edge, 'k1': k1, 'val': val}


def tsne_affinities(feat, perplexity):
    """feat [n, D] on the device -> the sparse conditional affinities p_{j|i} over the k = min(3 * perplexity, n - 1) nearest
    neighbours of the centred, L2-normalised features (features.centre_normalise) with their reverse lists; the
    symmetrised P_ij = (p_{j|i} + p_{i|j}) / 2n is never materialised (dv_tsne_attract_f32 sums both lists)."""
    _check_perplexity(perplexity)
    _check_feat(feat)
    n = feat.shape[0]
    k = min(3 * int(perplexity), n - 1)
    z = F.centre_normalise(feat)
    val, idx = knn.topk_neighbours(z, z, k + 1)
    aff = affinities_from_lists(val, idx, perplexity)
    aff['k'] = k
    return aff


class _Workspace:
    """the device arrays of one embedding: forces, velocity, gains, the repulsion workspace and the trace"""

    def __init__(self, n, dev, n_trace):
        self.ws = F.workspace(L.load().dv_tsne_repulse_workspace(n, None), dev, 'dv_tsne_repulse_workspace')
        self.fa = torch.empty(n, 2, dtype=torch.float32, device=dev)
        self.fr = torch.empty(n, 2, dtype=torch.float32, device=dev)
        self.ce_row = torch.empty(n, dtype=torch.float32, device=dev)
        self.vel = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        self.gain = torch.ones(n, 2, dtype=torch.float32, device=dev)
        self.trace = torch.zeros(n_trace + 1, 2, dtype=torch.float64, device=dev)        # (Z, sum ce_row); the last row is scratch


def forces(y, aff, w, slot):
    """fa, ce_row, fr of the map y into the workspace; (Z, sum ce_row) into trace[slot] (the cross-entropy sum only for a
    slot that is kept: the scratch slot gets Z alone)"""
    lib, s, n = L.load(), ops.stream_ptr(), y.shape[0]
    keep = slot < w.trace.shape[0] - 1
    zp = w.trace.data_ptr() + 16 * slot
    L.check(lib.dv_tsne_attract_f32(y.data_ptr(), aff['idx'].data_ptr(), aff['p'].data_ptr(), aff['k1'], n, aff['k1'],
                                    aff['rev_ptr'].data_ptr(), aff['rev_edge'].data_ptr(), aff['rev_edge'].numel(),
                                    w.fa.data_ptr(), w.ce_row.data_ptr(), zp + 8 if keep else None, s), 'dv_tsne_attract_f32')
    L.check(lib.dv_tsne_repulse_f32(y.data_ptr(), n, w.fr.data_ptr(), zp, w.ws.data_ptr(), s), 'dv_tsne_repulse_f32')
    return zp


def tsne_embed(feat, perplexity=30, n_iter=1000, seed=0, exaggeration=12, exaggeration_iter=250, lr=None, trace_every=50,
               affinities=None):
    """feat [n, D] clip features on the device -> (y [n, 2] f32 on the device, trace): gradient descent with gains and momentum
    on KL(P || Q), Q the Student-t kernel of the map.  lr None: max(n / exaggeration / 4, 50); momentum 0.5 while P is multiplied
    by `exaggeration` (the first `exaggeration_iter` iterations), 0.8 after; gains clamped below at 0.01; the initial map is
    1e-4 * N(0, 1) from a CPU torch.Generator seeded with `seed`.  The whole loop is enqueued without a host synchronisation (the
    update reads Z from the device); the trace is read once at the end.

    trace = {'iter': [...], 'ce': [...], 'z': [...]}: for the map ENTERING every `trace_every`-th iteration, and for the final
    map (iter = n_iter), Z = sum_{i != j} q_ij and the cross-entropy CE = sum_ij P_ij log(1 + |y_i - y_j|^2) + log Z
    = -sum P_ij log Q_ij (P unexaggerated).  CE = KL(P || Q) + H(P), and the entropy H(P) is a constant of the affinities, so CE
    falls exactly as KL does."""
    _check_feat(feat)
    n_iter, trace_every, exaggeration_iter = int(n_iter), int(trace_every), int(exaggeration_iter)
    if n_iter < 1 or trace_every < 1:
        raise ValueError('n_iter and trace_every must be at least 1')
    aff = tsne_affinities(feat, perplexity) if affinities is None else affinities
    n, dev = feat.shape[0], feat.device
    lr = max(n / float(exaggeration) / 4.0, 50.0) if lr is None else float(lr)
    gen = torch.Generator().manual_seed(int(seed))
    y = (1e-4 * torch.randn((n, 2), generator=gen, dtype=torch.float32)).to(dev)
    traced = list(range(0, n_iter, trace_every))
    w = _Workspace(n, dev, len(traced) + 1)
    lib, s = L.load(), ops.stream_ptr()
    for it in range(n_iter):
        early = it < exaggeration_iter
        slot = it // trace_every if it % trace_every == 0 else len(traced) + 1
        zp = forces(y, aff, w, slot)
        L.check(lib.dv_tsne_update_f32(y.data_ptr(), w.vel.data_ptr(), w.gain.data_ptr(), w.fa.data_ptr(), w.fr.data_ptr(), zp,
                                       2 * n, float(exaggeration) if early else 1.0, MOMENTUM[0] if early else MOMENTUM[1], lr,
                                       MIN_GAIN, s), 'dv_tsne_update_f32')
    forces(y, aff, w, len(traced))
    t = w.trace.cpu()[:len(traced) + 1]                                      # the one synchronisation
    trace = {'iter': traced + [n_iter], 'z': [float(v) for v in t[:, 0]],
             'ce': [float(c) + math.log(float(z)) if float(z) > 0 else float('nan') for z, c in t.tolist()]}
    return y, trace


def embedding_report(y, vid, cls, hi_idx, k=10):
    """y [n, 2] map on the device, vid / cls [n] ids, hi_idx [n, >= k + 1] the neighbour lists in feature space (the point itself
    among them) -> {'purity_video', 'purity_class': share of the k nearest neighbours in the map with the same id,
    'knn_preservation': share of the k nearest neighbours in feature space found among the k nearest in the map, 'k'}.
    The neighbours in the map come from knn.topk_neighbours on augmented rows: (y_x, y_y, 1) . (2 y_x, 2 y_y, -|y|^2)
    = |y_i|^2 - |y_i - y_j|^2, largest first = nearest first (the map is centred first; the count bookkeeping is the host's)."""
    n = y.shape[0]
    k = min(int(k), n - 1)
    if k < 1:
        raise ValueError('embedding_report needs at least two points')
    L.require_device()
    yc = (y.float() - y.float().mean(0)).contiguous()
    zero = torch.zeros(n, 1, dtype=torch.float32, device=y.device)
    q = torch.cat([yc, torch.ones_like(zero), zero], 1).contiguous()
    b = torch.cat([2 * yc, -(yc * yc).sum(1, keepdim=True), zero], 1).contiguous()
    _, lo = knn.topk_neighbours(q, b, k + 1)
    lo, hi = lo.cpu().long(), torch.as_tensor(hi_idx).cpu().long()
    rows = torch.arange(n)[:, None]

    def first_k(lists):                  # the first k entries that are valid and not the row itself, padded with -1
        ok = (lists >= 0) & (lists != rows)
        rank = torch.cumsum(ok.long(), 1)
        keep = ok & (rank <= k)
        out = torch.full((n, k), -1, dtype=torch.long)
        r, c = keep.nonzero(as_tuple=True)
        out[r, rank[r, c] - 1] = lists[r, c]
        return out
    lo_k, hi_k = first_k(lo), first_k(hi)
    valid = lo_k >= 0
    rep = {'k': k}
    for name, ids in (('purity_video', vid), ('purity_class', cls)):
        ids = torch.as_tensor(ids).cpu().long().reshape(-1)
        same = (ids[lo_k.clamp(min=0)] == ids[:, None]) & valid
        rep[name] = float(same.sum()) / max(int(valid.sum()), 1)
    found = ((hi_k[:, :, None] == lo_k[:, None, :]) & (hi_k >= 0)[:, :, None]).any(2)
    rep['knn_preservation'] = float(found.sum()) / max(int((hi_k >= 0).sum()), 1)
    return rep


def tsne_eval(per_feature, video_label, perplexity=30, n_iter=1000, seed=0, k=10):
    """per_feature [n_video, num_seq, D] (the per-clip features `classifier.py --retrieval` saves), video_label [n_video] ->
    (y [n_video * num_seq, 2] on the host, row = video * num_seq + clip; trace; report; the neighbours per row that attract,
    min(3 * perplexity, n - 1))"""
    feat, vid, cls, _, _ = F.clip_rows(per_feature, video_label)
    aff = tsne_affinities(feat, perplexity)
    y, trace = tsne_embed(feat, perplexity=perplexity, n_iter=n_iter, seed=seed, affinities=aff)
    rep = embedding_report(y, vid, cls, aff['idx'], k=k)
    return y.cpu(), trace, rep, aff['k']
