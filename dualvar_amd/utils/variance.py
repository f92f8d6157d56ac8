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
from . import knn
from .retrieval import _centre_normalise

CATEGORIES = ('same_video', 'same_class', 'diff_class')


def _check_bins_t(bins, t):
    if not 1 <= bins <= L.DV_PAIRSTAT_MAX_BINS:
        raise ValueError('bins = %d: the histogram keeps 1 <= bins <= %d (DV_PAIRSTAT_MAX_BINS)' % (bins, L.DV_PAIRSTAT_MAX_BINS))
    if not (t >= 0 and math.isfinite(t)):
        raise ValueError('t must be finite and not negative')


def _normalise(x, centre):
    if centre:
        return _centre_normalise(x)
    x = x.float().contiguous()
    y, nrm = torch.empty_like(x), torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.load().dv_l2norm_fwd(x.data_ptr(), x.shape[0], x.shape[1], 1e-12, y.data_ptr(), nrm.data_ptr(), ops.stream_ptr()),
            'dv_l2norm_fwd')
    return y


def _ids(v, n, dev, what):
    v = torch.as_tensor(v)
    if v.dim() != 1 or v.numel() != n:
        raise ValueError('%s must hold one id per feature row (%d), got %s' % (what, n, tuple(v.shape)))
    return v.to(device=dev, dtype=torch.int32).contiguous()


class _State:
    """the state of dv_pairstat_accum_f32 on the device and the similarity workspace the walk reuses"""

    def __init__(self, dev, bins, t, row_block, chunk):
        self.bins, self.t, self.row_block, self.chunk = bins, float(t), row_block, chunk
        self.sums = torch.empty(3, 4, dtype=torch.float64, device=dev)
        self.ext = torch.empty(3, 2, dtype=torch.float32, device=dev)
        self.hist = torch.empty(3, bins + 1, dtype=torch.int64, device=dev)      # the kernel's uint64; counts stay below 2^63
        self.sim = torch.empty(row_block, chunk, dtype=torch.float32, device=dev)
        nbytes = L.load().dv_pairstat_workspace(row_block, chunk)                # the grid grows with the block: the largest one
        if nbytes < 0:
            L.check(int(nbytes), 'dv_pairstat_workspace')
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.first = 1

    def block(self, q, b, q_ids, b_ids, r0, nr, c0, nc, diag, mult):
        """similarity of q[r0:r0+nr] . b[c0:c0+nc]^T into the workspace, then its pairs into the state"""
        lib, s, D = L.load(), ops.stream_ptr(), q.shape[1]
        L.check(lib.dv_gemm_f32(nr, nc, D, q.data_ptr() + 4 * r0 * D, D, 1, b.data_ptr() + 4 * c0 * D, 1, D, self.sim.data_ptr(),
                                self.chunk, 1.0, 0, s), 'dv_gemm_f32')
        L.check(lib.dv_pairstat_accum_f32(self.sim.data_ptr(), self.chunk, nr, nc, q_ids[0].data_ptr() + 4 * r0,
                                          q_ids[1].data_ptr() + 4 * r0, b_ids[0].data_ptr() + 4 * c0, b_ids[1].data_ptr() + 4 * c0,
                                          diag, mult, self.t, self.bins, self.sums.data_ptr(), self.ext.data_ptr(),
                                          self.hist.data_ptr(), self.bins + 1, self.ws.data_ptr(), self.first, s),
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

    The walk is that of knn.topk_neighbours: row blocks of `row_block`, column chunks of `chunk`, one reused workspace within
    knn.WORKSPACE_BYTES.  symmetric=True visits, per row block [r0, r0 + nr), only the columns from r0 on and cuts the chunks at
    r0 + nr, so the block grid is aligned to the diagonal: the square [r0, r0 + nr)^2 holds both orders of its pairs and is
    counted once (mult = 1, self pairs on its diagonal skipped), every block to its right lies strictly above the diagonal and is
    counted twice (mult = 2).  No block straddles the diagonal raggedly, so no mirror block is ever needed."""
    bins = int(bins)
    _check_bins_t(bins, t)
    _prepare(feat, 'feat')
    L.require_device()
    n = feat.shape[0]
    ids = (_ids(vid, n, feat.device, 'vid'), _ids(cls, n, feat.device, 'cls'))
    z = _normalise(feat, centre)
    row_block, chunk = knn.blocks(n, n, row_block, chunk)
    st = _State(z.device, bins, t, row_block, chunk)
    for r0 in range(0, n, row_block):
        nr = min(row_block, n - r0)
        # (first column, end, mult) of the column ranges this row block visits
        spans = [(r0, r0 + nr, 1), (r0 + nr, n, 2)] if symmetric else [(0, n, 1)]
        for lo, hi, mult in spans:
            for c0 in range(lo, hi, chunk):
                st.block(z, z, ids, ids, r0, nr, c0, min(chunk, hi - c0), r0 - c0, mult)
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
    zq, zb = _normalise(q, centre), _normalise(bank, centre)
    row_block, chunk = knn.blocks(R, N, row_block, chunk)
    st = _State(zq.device, bins, t, row_block, chunk)
    no_self = -(1 << 40)                 # no (r, j) has j == r + diag
    for r0 in range(0, R, row_block):
        nr = min(row_block, R - r0)
        for c0 in range(0, N, chunk):
            st.block(zq, zb, q_ids, b_ids, r0, nr, c0, min(chunk, N - c0), no_self, 1)
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
    if per_feature.dim() != 3:
        raise ValueError('per_feature must be [n_video, num_seq, D], got %s' % (tuple(per_feature.shape),))
    n_video, num_seq, D = per_feature.shape
    label = torch.as_tensor(video_label).reshape(-1)
    if label.numel() != n_video:
        raise ValueError('video_label must hold one label per video (%d), got %d' % (n_video, label.numel()))
    vid = torch.arange(n_video, dtype=torch.int32).repeat_interleave(num_seq)
    cls = label.to(torch.int32).cpu().repeat_interleave(num_seq)
    state = pair_statistics(per_feature.reshape(n_video * num_seq, D), vid, cls, bins=bins, t=t)
    return report_from_state(*state, bins, t)
