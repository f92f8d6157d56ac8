"""Inter- / intra-video variance report of an encoder's clip features: statistics over all ordered clip pairs (i, j), i != j, of
the cosine similarity s_ij, split into same video / same class, other video / different class.  The [n, n] similarity is never
formed (71 GB for UCF101 at ten clips per video): it arrives in [row_block, chunk] pieces from `dv_gemm_f32` in one reused
workspace and `dv_pairstat_accum_f32` (include/dualvar_pairstat.h) folds each piece into a state of a few kilobytes.  All
arithmetic over the pairs runs in the HIP library; `report_from_state` is float64 bookkeeping on that state, on the host.

The one definition behind the derived figures: on unit vectors  1/2 E |z_i - z_j|^2 = 1 - E s_ij."""
import math

import torch

from .. import _lib as L
from .. import ops
from . import features as F

CATEGORIES = ('same_video', 'same_class', 'diff_class')


def _check_bins_t(bins, t):
    if not 1 <= bins <= L.DV_PAIRSTAT_MAX_BINS:
        raise ValueError('bins = %d: the histogram keeps 1 <= bins <= %d (DV_PAIRSTAT_MAX_BINS)' % (bins, L.DV_PAIRSTAT_MAX_BINS))
    if not (t >= 0 and math.isfinite(t)):
        raise ValueError('t must be finite and not negative')


def _ids(v, n, dev, what):
    v = torch.as_tensor(v)
    if v.dim() != 1 or v.numel() != n:
        raise ValueError('%s must hold one id per feature row (%d), got %s' % (what, n, tuple(v.shape)))
    return v.to(device=dev, dtype=torch.int32).contiguous()


class _State:
    """the state of dv_pairstat_accum_f32 on the device"""

    def __init__(self, dev, bins, t, row_block, chunk):
        self.bins, self.t = bins, float(t)
        self.sums = torch.empty(3, 4, dtype=torch.float64, device=dev)
        self.ext = torch.empty(3, 2, dtype=torch.float32, device=dev)
        self.hist = torch.empty(3, bins + 1, dtype=torch.int64, device=dev)      # the kernel's uint64; counts stay below 2^63
        # the grid grows with the block: the largest one
        self.ws = F.workspace(L.load().dv_pairstat_workspace(row_block, chunk), dev, 'dv_pairstat_workspace')
        self.first = 1

    def accumulate(self, sim, ld, q_ids, b_ids, r0, nr, c0, nc, diag, mult):
        """the pairs of the [nr, nc] similarity block `sim` (pitch ld; rows from r0, columns from c0) into the state"""
        L.check(L.load().dv_pairstat_accum_f32(sim.data_ptr(), ld, nr, nc, q_ids[0].data_ptr() + 4 * r0, q_ids[1].data_ptr() + 4 * r0,
                                               b_ids[0].data_ptr() + 4 * c0, b_ids[1].data_ptr() + 4 * c0, diag, mult, self.t,
                                               self.bins, self.sums.data_ptr(), self.ext.data_ptr(), self.hist.data_ptr(),
                                               self.bins + 1, self.ws.data_ptr(), self.first, ops.stream_ptr()),
                'dv_pairstat_accum_f32')
        self.first = 0

    def result(self):
        return self.sums.cpu(), self.ext.cpu(), self.hist.cpu()


def _prepare(feat, what):
    if feat.dim() != 2 or feat.shape[0] < 1:
        raise ValueError('%s must be [n, D] clip features, got %s' % (what, tuple(feat.shape)))
    if not feat.is_cuda:
        raise ValueError('%s must be a device tensor (the kernels read the pointers as they are)' % what)


def pair_statistics(feat, vid, cls, bins=64, t=2.0, centre=True, symmetric=True, chunk=None, row_block=None):
    """feat [n, D] clip features on the device, vid / cls [n] video and class ids -> (sums [3, 4] f64, ext [3, 2] f32,
    hist [3, bins + 1] i64) on the host: the state of dv_pairstat_accum_f32 over the n (n - 1) ordered pairs i != j of the
    normalised features (centred first as retrieval does when `centre`), categories 0 / 1 / 2 as in CATEGORIES.

    The walk is features.SimilarityWalk, as knn.topk_neighbours: row blocks of `row_block`, column chunks of `chunk`, one reused
    workspace within features.WORKSPACE_BYTES.  symmetric=True takes the spans of features.block_spans aligned to the diagonal:
    a square on it counts once (mult = 1, the self pairs on its diagonal skipped), a block to its right twice (mult = 2)."""
    bins = int(bins)
    _check_bins_t(bins, t)
    _prepare(feat, 'feat')
    L.require_device()
    n = feat.shape[0]
    ids = (_ids(vid, n, feat.device, 'vid'), _ids(cls, n, feat.device, 'cls'))
    z = F.normalise(feat, centre)
    row_block, chunk = F.blocks(n, n, row_block, chunk)
    st, walk = _State(z.device, bins, t, row_block, chunk), F.SimilarityWalk(row_block, chunk, z.device)
    for span in walk(z, z, symmetric):
        st.accumulate(walk.sim, chunk, ids, ids, *span)
    return st.result()


def pair_statistics_cross(q, q_vid, q_cls, bank, bank_vid, bank_cls, bins=64, t=2.0, centre=True, chunk=None, row_block=None):
    """the same state over the n_q * n_bank pairs (query clip, bank clip), test x train: no self pairs, every pair counted once.
    Each set is centred on its own mean, as retrieval centres test and train."""
    bins = int(bins)
    _check_bins_t(bins, t)
    _prepare(q, 'q')
    _prepare(bank, 'bank')
    if q.shape[1] != bank.shape[1]:
        raise ValueError('q and bank differ in the feature size: %s and %s' % (tuple(q.shape), tuple(bank.shape)))
    L.require_device()
    R, N = q.shape[0], bank.shape[0]
    q_ids = (_ids(q_vid, R, q.device, 'q_vid'), _ids(q_cls, R, q.device, 'q_cls'))
    b_ids = (_ids(bank_vid, N, q.device, 'bank_vid'), _ids(bank_cls, N, q.device, 'bank_cls'))
    zq, zb = F.normalise(q, centre), F.normalise(bank, centre)
    row_block, chunk = F.blocks(R, N, row_block, chunk)
    st, walk = _State(zq.device, bins, t, row_block, chunk), F.SimilarityWalk(row_block, chunk, zq.device)
    no_self = -(1 << 40)                 # no (r, j) has j == r + diag
    for r0, nr, c0, nc, _, mult in walk(zq, zb):
        st.accumulate(walk.sim, chunk, q_ids, b_ids, r0, nr, c0, nc, no_self, mult)
    return st.result()


def report_from_state(sums, ext, hist, bins, t):
    """the state of dv_pairstat_accum_f32 -> the report, in float64 on the host (no GPU).  Per category of CATEGORIES: count
    (finite pairs), skipped (non-finite similarities), mean, std (population), min, max, hist (bins counts over [-1, 1]).
    Derived: var_* = 1 - mean (half the mean squared distance), the two ratios, alignment = 2 var_intra_video,
    uniformity = log(sum w / count) over all pairs with w = exp(-t |z_i - z_j|^2).  A figure whose pairs are missing is None."""
    sums = torch.as_tensor(sums).double().reshape(3, 4)
    ext = torch.as_tensor(ext).double().reshape(3, 2)
    hist = torch.as_tensor(hist).reshape(3, -1)[:, :bins + 1].long()
    count = [int(hist[c, :bins].sum()) for c in range(3)]
    rep = {'bins': int(bins), 't': float(t), 'categories': {}}

    def mean_of(cs):
        n = sum(count[c] for c in cs)
        return None if n == 0 else float(sum(float(sums[c, 0]) for c in cs) / n)

    def one_minus(m):
        return None if m is None else 1.0 - m

    def ratio(a, b):
        return None if a is None or b is None or b == 0 else a / b

    for c, name in enumerate(CATEGORIES):
        n, m = count[c], mean_of([c])
        var = None if n == 0 else max(float(sums[c, 1]) / n - m * m, 0.0)
        rep['categories'][name] = {'count': n, 'skipped': int(hist[c, bins]), 'mean': m, 'std': None if var is None else math.sqrt(var),
                                   'min': float(ext[c, 0]) if n else None, 'max': float(ext[c, 1]) if n else None,
                                   'hist': [int(v) for v in hist[c, :bins]]}
    rep['var_intra_video'] = one_minus(mean_of([0]))
    rep['var_inter_video'] = one_minus(mean_of([1, 2]))
    rep['var_intra_class'] = one_minus(mean_of([1]))
    rep['var_inter_class'] = one_minus(mean_of([2]))
    rep['ratio_video'] = ratio(rep['var_intra_video'], rep['var_inter_video'])
    rep['ratio_class'] = ratio(rep['var_intra_class'], rep['var_inter_class'])
    rep['alignment'] = None if rep['var_intra_video'] is None else 2.0 * rep['var_intra_video']
    total, w = sum(count), float(sums[:, 2].sum())
    rep['uniformity'] = math.log(w / total) if total > 0 and w > 0 else None
    return rep


def variance_eval(per_feature, video_label, bins=64, t=2.0):
    """per_feature [n_video, num_seq, D] (the per-clip features `classifier.py --retrieval` saves), video_label [n_video] ->
    the report of report_from_state over all ordered pairs of the n_video * num_seq clips: vid = the video's row, cls = its label"""
    feat, vid, cls, _, _ = F.clip_rows(per_feature, video_label)
    state = pair_statistics(feat, vid, cls, bins=bins, t=t)
    return report_from_state(*state, bins, t)
