"""Weighted k-NN evaluation of an encoder on extracted features (the InstDisc / MoCo protocol: the k = 200 nearest train
samples vote for their label with weight exp(sim / T), T = 0.07), on a streaming top-k selection: the similarity is formed
in [row_block, chunk] pieces by `dv_gemm_f32`, `dv_topk_merge_f32` folds each piece into the [R, k] neighbour lists and
`dv_knn_vote` takes the vote.  The full [n_test, n_train] matrix is never allocated.  All arithmetic runs in the HIP library."""
import math

import torch

from .. import _lib as L
from .. import ops
from . import features as F


def _check_k(k):
    if not 1 <= k <= L.DV_TOPK_MAX_K:
        raise ValueError('k = %d: the selection kernel keeps 1 <= k <= %d (DV_TOPK_MAX_K) neighbours per row' % (k, L.DV_TOPK_MAX_K))


def topk_neighbours(query, bank, k, chunk=None, row_block=None):
    """query [R, D], bank [N, D] fp32 on the device -> (val [R, k] f32, idx [R, k] i32): per query row the k largest raw dot
    products query . bank^T, larger first and lower index first among equals; slots beyond N hold (-inf, -1)."""
    k = int(k)
    _check_k(k)
    if query.dim() != 2 or bank.dim() != 2 or query.shape[1] != bank.shape[1] or query.shape[0] < 1 or bank.shape[0] < 1:
        raise ValueError('topk_neighbours takes query [R, D] and bank [N, D], got %s and %s' % (tuple(query.shape), tuple(bank.shape)))
    if not (query.is_cuda and bank.is_cuda):
        raise ValueError('topk_neighbours takes device tensors (the kernels read the pointers as they are)')
    L.require_device()
    q, b = query.float().contiguous(), bank.float().contiguous()
    R = q.shape[0]
    row_block, chunk = F.blocks(R, b.shape[0], row_block, chunk)
    lib, s = L.load(), ops.stream_ptr()
    walk = F.SimilarityWalk(row_block, chunk, q.device)
    val = torch.empty(R, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(R, k, dtype=torch.int32, device=q.device)
    for r0, nr, c0, nc, _, _ in walk(q, b):
        L.check(lib.dv_topk_merge_f32(walk.sim.data_ptr(), chunk, nr, nc, c0, k, val.data_ptr() + 4 * r0 * k, idx.data_ptr() + 4 * r0 * k,
                                      k, int(c0 == 0), s), 'dv_topk_merge_f32')
    return val, idx


def knn_classify(val, idx, bank_labels, n_class, T=0.07):
    """neighbour lists [R, k] (as topk_neighbours returns them) -> (score [R, n_class] f32, pred [R] i32); T None or inf: plain
    majority vote"""
    if T is None or math.isinf(T):
        inv_T = 0.0
    elif not T > 0:
        raise ValueError('T must be positive (or None / inf for the plain majority vote)')
    else:
        inv_T = 1.0 / T
    if val.dim() != 2 or val.shape != idx.shape:
        raise ValueError('val and idx must be [R, k] of one shape')
    _check_k(val.shape[1])
    if not val.is_cuda:
        raise ValueError('knn_classify takes the lists as device tensors (the kernel reads the pointers as they are)')
    L.require_device()
    v, i = val, idx.to(device=val.device)
    if not (v.dtype == torch.float32 and i.dtype == torch.int32 and v.stride(1) == i.stride(1) == 1 and v.stride(0) == i.stride(0) >= v.shape[1]):
        v, i = v.float().contiguous(), i.to(torch.int32).contiguous()         # otherwise the lists are read in place, pitch = stride
    lab = bank_labels.to(device=v.device, dtype=torch.int32).contiguous()
    (R, k), ldk = v.shape, v.stride(0)
    score = torch.empty(R, n_class, dtype=torch.float32, device=v.device)
    pred = torch.empty(R, dtype=torch.int32, device=v.device)
    L.check(L.load().dv_knn_vote(v.data_ptr(), i.data_ptr(), ldk, R, k, lab.data_ptr(), lab.numel(), n_class, inv_T, score.data_ptr(),
                                 n_class, pred.data_ptr(), ops.stream_ptr()), 'dv_knn_vote')
    return score, pred


def knn_eval(test_feature, test_label, train_feature, train_label, n_class, k=200, T=0.07, ks=(1, 5, 10, 20, 50)):
    """-> {'knn_top1', 'knn_top5', 'retrieval': {k: accuracy}, 'k', 'T', 'val', 'idx', 'pred'}: the weighted k-NN classifier on
    centred, L2-normalised features (as nn_retrieval prepares them) and, from the same neighbour lists, the retrieval accuracy
    of the reference's torch.topk definition (a same-label sample among the first k neighbours).  'k' is the number of
    neighbours that voted, min(k, n_train); 'val' / 'idx' are the [n_test, k'] lists, k' = min(max(k, max(ks)), n_train)."""
    L.require_device()
    te, tr = F.centre_normalise(test_feature), F.centre_normalise(train_feature)
    n_train = tr.shape[0]
    kk = min(max([k] + list(ks)), n_train)
    k_vote = min(k, n_train)
    val, idx = topk_neighbours(te, tr, kk)
    tl = train_label.to(device=te.device, dtype=torch.int32).contiguous()
    ql = test_label.to(device=te.device, dtype=torch.int32).contiguous()
    score, pred = knn_classify(val[:, :k_vote], idx[:, :k_vote], tl, n_class, T)
    R = te.shape[0]
    # Acc@5 without a sort, as evaluation.topk_of_mean: the number of classes scoring strictly above the target's
    cls = torch.arange(n_class, dtype=torch.int32, device=te.device)
    rank = torch.empty(R, dtype=torch.int32, device=te.device)
    L.check(L.load().dv_knn_rank(score.data_ptr(), n_class, R, n_class, cls.data_ptr(), ql.data_ptr(), rank.data_ptr(),
                                 ops.stream_ptr()), 'dv_knn_rank')
    # the accuracies are host bookkeeping on the lists, as nn_retrieval's: position of the first same-label neighbour per row
    idx_h, tl_h, ql_h, pred_h = idx.cpu().long(), tl.cpu(), ql.cpu(), pred.cpu()
    hit = (tl_h[idx_h.clamp(min=0)] == ql_h[:, None]) & (idx_h >= 0)
    first_hit = torch.where(hit.any(1), hit.int().argmax(1), torch.full((R,), kk))
    top5 = (rank.cpu() < 5) & (pred_h >= 0)                      # a row without a valid neighbour predicts nothing
    return {'knn_top1': float((pred_h == ql_h).float().mean()), 'knn_top5': float(top5.float().mean()),
            'retrieval': {kq: float((first_hit < kq).float().mean()) for kq in ks},
            'k': k_vote, 'T': T, 'val': val, 'idx': idx, 'pred': pred}
