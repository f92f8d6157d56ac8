"""Full-ranking retrieval figures of an encoder on extracted features: mean average precision, precision@k, recall@k,
R-precision and the mean reciprocal rank, from the exact rank of every positive of every query in the full ordering of the bank.
Nothing is sorted but each query's own positives, and the [n_query, n_bank] matrix never exists: per row block of a
`features.SimilarityWalk`, `dv_rankeval_gather_f32` collects the positives chunk by chunk, `dv_rankeval_sort` orders them,
`dv_rankeval_count_f32` counts the bank against them over the same chunks and `dv_rankeval_finish` turns the counts into ranks
and per-query figures (include/dualvar_rankeval.h).  The counts are integers: the figures do not depend on the blocking.  All
device arithmetic runs in the HIP library; `ranking_report` is host bookkeeping in float64."""
import math

import torch

from .. import _lib as L
from .. import ops
from . import features as F

EXCLUDE = {'none': 0, 'self': 1, 'video': 2}


def _ids(x, n, name):
    """labels / video ids -> int64 [n] on the host"""
    t = torch.as_tensor(x).reshape(-1).cpu()
    if t.numel() != n or t.dtype.is_floating_point:
        raise ValueError('%s must hold one integer id per row (%d), got %s of %s' % (name, n, tuple(t.shape), t.dtype))
    t = t.long()
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise ValueError('%s must fit int32' % name)
    return t


def _count_in(keys, of):
    """for every entry of `of`: how many entries of `keys` equal it (host, int64)"""
    uniq, cnt = torch.unique(keys, return_counts=True)
    if uniq.numel() == 0:
        return torch.zeros_like(of)
    at = torch.searchsorted(uniq, of).clamp(max=uniq.numel() - 1)
    return torch.where(uniq[at] == of, cnt[at], torch.zeros_like(of))


def positives_per_query(q_cls, b_cls, q_vid, b_vid, exclude):
    """host: the number of positives of every query (int64 [R]): the bank items of its class, less what `exclude` removes"""
    P = _count_in(b_cls, q_cls)
    if exclude == 'self':
        P = P - 1                        # query r is bank item r, of its own class
    elif exclude == 'video':             # less the bank items of the query's class AND its video: one id per (class, video) pair
        pairs = torch.cat([torch.stack([b_cls, b_vid], 1), torch.stack([q_cls, q_vid], 1)])
        pair_id = torch.unique(pairs, dim=0, return_inverse=True)[1]
        P = P - _count_in(pair_id[:b_cls.numel()], pair_id[b_cls.numel():])
    return P


def positive_ranks(query, bank, q_cls, b_cls, q_vid=None, b_vid=None, exclude='none', ks=(), chunk=None, row_block=None):
    """query [R, D], bank [N, D] fp32 on the device, q_cls [R], b_cls [N] integer labels (q_vid, b_vid: video ids) -> a dict of
    device tensors over the raw dot products query . bank^T in the order of include/dualvar_rankeval.h (larger first, lower bank
    index first among equals; NaN as -inf):
      rank [R, P_max] i32      the 1-based ranks of row r's positives, ascending; 0 beyond pos_cnt[r]
      pos_idx [R, P_max] i32   their bank indices (-1 beyond pos_cnt[r]);   pos_cnt [R] i32
      ap [R] f64 (-1.0 for a query without positives), first_rank [R] i32 (0 for such a query), hits [R, len(ks)] i32,
      rhits [R] i32 (positives among the first pos_cnt[r]), n_valid [R] i32 (bank items not excluded)
    and 'ks', 'n_bank'.  exclude: 'none'; 'self' (query and bank are the same set: item r is left out for query r); 'video' (every
    bank item of the query's video is left out; needs q_vid and b_vid).  A positive is a bank item of the query's label that is
    not excluded; P_max is the largest number of them (at least 1)."""
    if query.dim() != 2 or bank.dim() != 2 or query.shape[1] != bank.shape[1] or query.shape[0] < 1 or bank.shape[0] < 1:
        raise ValueError('positive_ranks takes query [R, D] and bank [N, D], got %s and %s' % (tuple(query.shape), tuple(bank.shape)))
    if exclude not in EXCLUDE:
        raise ValueError("exclude must be 'none', 'self' or 'video', got %r" % (exclude,))
    R, N = query.shape[0], bank.shape[0]
    ks = [int(k) for k in ks]
    if len(ks) > 16 or any(k < 1 for k in ks):
        raise ValueError('ks takes at most 16 cut-offs of at least 1, got %s' % (ks,))
    qc, bc = _ids(q_cls, R, 'q_cls'), _ids(b_cls, N, 'b_cls')
    qv = bv = None
    if exclude == 'video':
        if q_vid is None or b_vid is None:
            raise ValueError("exclude='video' needs q_vid and b_vid")
        qv, bv = _ids(q_vid, R, 'q_vid'), _ids(b_vid, N, 'b_vid')
    if exclude == 'self' and (R != N or not torch.equal(qc, bc)):
        raise ValueError("exclude='self' needs query and bank to be the same set (%d rows against %d, or the labels differ)" % (R, N))
    P = positives_per_query(qc, bc, qv, bv, exclude)
    worst = int(P.argmax())
    P_max = max(int(P[worst]), 1)
    if P_max > L.DV_RANKEVAL_MAX_POS:
        raise ValueError('class %d has %d positives for one query: the ranking kernels keep at most %d (DV_RANKEVAL_MAX_POS) per query'
                         % (int(qc[worst]), P_max, L.DV_RANKEVAL_MAX_POS))
    if not (query.is_cuda and bank.is_cuda):
        raise ValueError('positive_ranks takes device tensors (the kernels read the pointers as they are)')
    if query.dtype != torch.float32 or bank.dtype != torch.float32:
        raise ValueError('positive_ranks takes fp32 features, got %s and %s' % (query.dtype, bank.dtype))
    L.require_device()
    q, b = query.contiguous(), bank.contiguous()
    dev = q.device
    row_block, chunk = F.blocks(R, N, row_block, chunk)
    lib, s = L.load(), ops.stream_ptr()
    walk = F.SimilarityWalk(row_block, chunk, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    qc_d, bc_d = qc.to(**i32), bc.to(**i32)
    qv_d, bv_d = (qv.to(**i32), bv.to(**i32)) if qv is not None else (None, None)
    ex, ldp, ldh, n_k = EXCLUDE[exclude], P_max, P_max + 1, len(ks)
    ks_d = torch.tensor(ks or [1], **i32)
    pos_val = torch.empty(row_block, ldp, dtype=torch.float32, device=dev)     # the row block's lists and counts: reused
    hist = torch.empty(row_block, ldh, **i32)
    out = {'rank': torch.zeros(R, ldp, **i32), 'pos_idx': torch.full((R, ldp), -1, **i32), 'pos_cnt': torch.empty(R, **i32),
           'ap': torch.empty(R, dtype=torch.float64, device=dev), 'first_rank': torch.empty(R, **i32),
           'hits': torch.empty(R, n_k, **i32), 'rhits': torch.empty(R, **i32), 'n_valid': torch.empty(R, **i32)}

    def at(t, r0, width=1, size=4):
        return t.data_ptr() + size * r0 * width

    def vid(t, i0):
        return None if t is None else at(t, i0)

    for r0 in range(0, R, row_block):
        nr = min(row_block, R - r0)
        qb = q[r0:r0 + nr]
        idx_p, cnt_p = at(out['pos_idx'], r0, ldp), at(out['pos_cnt'], r0)

        def gather(c0, nc):
            L.check(lib.dv_rankeval_gather_f32(walk.sim.data_ptr(), chunk, nr, nc, c0, at(qc_d, r0), at(bc_d, c0), vid(qv_d, r0),
                                               vid(bv_d, c0), ex, r0 - c0, pos_val.data_ptr(), idx_p, ldp, cnt_p, int(c0 == 0), s),
                    'dv_rankeval_gather_f32')

        def sort():
            L.check(lib.dv_rankeval_sort(pos_val.data_ptr(), idx_p, ldp, cnt_p, nr, s), 'dv_rankeval_sort')

        def count(c0, nc):
            L.check(lib.dv_rankeval_count_f32(walk.sim.data_ptr(), chunk, nr, nc, c0, vid(qv_d, r0), vid(bv_d, c0), ex, r0 - c0,
                                              pos_val.data_ptr(), idx_p, ldp, cnt_p, hist.data_ptr(), ldh, int(c0 == 0), s),
                    'dv_rankeval_count_f32')

        if chunk >= N:                   # the whole bank is one chunk: its product serves both passes
            for _ in walk(qb, b):
                gather(0, N)
                sort()
                count(0, N)
        else:
            for _, _, c0, nc, _, _ in walk(qb, b):
                gather(c0, nc)
            sort()
            for _, _, c0, nc, _, _ in walk(qb, b):
                count(c0, nc)
        L.check(lib.dv_rankeval_finish(hist.data_ptr(), ldh, cnt_p, ldp, nr, ks_d.data_ptr() if n_k else None, n_k,
                                       at(out['rank'], r0, ldp), at(out['ap'], r0, 1, 8), at(out['first_rank'], r0),
                                       at(out['hits'], r0, n_k) if n_k else None, at(out['rhits'], r0), at(out['n_valid'], r0), s),
                'dv_rankeval_finish')
    if not torch.equal(out['pos_cnt'].cpu().long(), P):      # the lists never overflow when this holds: P <= P_max = ldp
        raise L.DualVarHipError('positive_ranks: the device found other positives than the labels give (%d rows differ)'
                                % int((out['pos_cnt'].cpu().long() != P).sum()))
    out['ks'], out['n_bank'] = ks, N
    return out


def ranking_report(state, q_cls, n_class, ks):
    """the per-query figures of positive_ranks (`state`: ap, pos_cnt, first_rank, hits [R, len(ks)], rhits, and n_bank; device or
    host) -> a JSON-ready dict.  Pure host code in float64.  A query without positives (pos_cnt = 0) is SKIPPED: it enters none of
    mAP, mAP_macro, per_class_AP, MRR, R_precision, precision_at and recall_at, whose means run over the other n_query -
    n_skipped queries.  success_at[k], the share of queries with a positive among the first k, runs over ALL n_query queries (a
    skipped one cannot succeed), which makes it the retrieval accuracy of nn_retrieval.
      mAP: math.fsum of the per-query AP / their number (independent of the order of the queries)
      per_class_AP: [n_class], the mean AP of the class's queries, None for a class without one; mAP_macro: their mean
      MRR: mean of 1 / first_rank;  R_precision: mean of rhits / pos_cnt
      precision_at[k]: mean of hits(k) / k;  recall_at[k]: mean of hits(k) / pos_cnt;  a figure without queries is None"""
    ks = [int(k) for k in ks]
    ap = torch.as_tensor(state['ap']).cpu().double().tolist()
    P = torch.as_tensor(state['pos_cnt']).cpu().long().tolist()
    first = torch.as_tensor(state['first_rank']).cpu().long().tolist()
    rhits = torch.as_tensor(state['rhits']).cpu().long().tolist()
    hits = torch.as_tensor(state['hits']).cpu().long().reshape(len(P), -1).tolist()
    cls = torch.as_tensor(q_cls).reshape(-1).cpu().long().tolist()
    if not (len(ap) == len(first) == len(rhits) == len(cls) == len(P)) or any(len(h) != len(ks) for h in hits):
        raise ValueError('ranking_report: the state holds %d queries, q_cls %d labels, hits %d columns for %d cut-offs'
                         % (len(P), len(cls), len(hits[0]) if hits else 0, len(ks)))
    used = [r for r in range(len(P)) if P[r] > 0]
    n = len(used)

    def mean(values):
        values = list(values)
        return math.fsum(values) / len(values) if values else None

    per_class = []
    for c in range(n_class):
        per_class.append(mean(ap[r] for r in used if cls[r] == c))
    rep = {'mAP': mean(ap[r] for r in used), 'mAP_macro': mean(v for v in per_class if v is not None), 'per_class_AP': per_class,
           'MRR': mean(1.0 / first[r] for r in used), 'R_precision': mean(rhits[r] / P[r] for r in used),
           'precision_at': {k: mean(hits[r][q] / k for r in used) for q, k in enumerate(ks)},
           'recall_at': {k: mean(hits[r][q] / P[r] for r in used) for q, k in enumerate(ks)},
           'success_at': {k: (sum(1 for r in used if first[r] <= k) / len(P) if P else None) for k in ks},
           'n_query': len(P), 'n_skipped': len(P) - n, 'n_bank': int(state['n_bank']) if state.get('n_bank') is not None else None}
    return rep


def ranking_eval(test_feature, test_label, train_feature, train_label, n_class, ks=(1, 5, 10, 20, 50), chunk=None, row_block=None):
    """-> (report, state): the full-ranking figures of the test set querying the train set on centred, L2-normalised features (as
    nn_retrieval prepares them); state is positive_ranks' dict, report is ranking_report's"""
    L.require_device()
    te, tr = F.centre_normalise(test_feature), F.centre_normalise(train_feature)
    state = positive_ranks(te, tr, test_label, train_label, ks=ks, chunk=chunk, row_block=row_block)
    return ranking_report(state, test_label, n_class, ks), state


def ranking_eval_within(per_feature, video_label, n_class, ks=(1, 5, 10, 20, 50), chunk=None, row_block=None):
    """per_feature [n_video, num_seq, D] (the clips of one split), video_label [n_video] -> (report, state): every clip queries
    the clips of its own split with those of its own video left out (exclude='video'), on centred, L2-normalised clip features"""
    feat, vid, cls, _, _ = F.clip_rows(per_feature, video_label)
    if cls is None:
        raise ValueError('ranking_eval_within needs video_label')
    L.require_device()
    f = F.normalise(feat, centre=True)
    state = positive_ranks(f, f, cls, cls, vid, vid, exclude='video', ks=ks, chunk=chunk, row_block=row_block)
    return ranking_report(state, cls, n_class, ks), state
