"""The host layer the evaluations of the cached clip features share (knn, variance, embed, cluster, probe, spectrum): how the
features are prepared, how the [n_video, num_seq, D] array `classifier.py --retrieval` saves becomes rows with ids, how a
workspace query becomes a tensor, and the streaming walk that forms a similarity in [row_block, chunk] pieces by `dv_gemm_f32`
in one reused workspace.  All arithmetic runs in the HIP library."""
import torch

from .. import _lib as L
from .. import ops
from ..ops import DV_F32

WORKSPACE_BYTES = 256 << 20          # the largest similarity workspace a walk allocates by default
_DEFAULT_ROW_BLOCK = 4096


def blocks(R, N, row_block=None, chunk=None):
    """(row_block, chunk) of the similarity workspace for R query rows and N bank rows: what the caller forces, clipped to the
    problem; the defaults keep row_block * chunk * 4 bytes at or below WORKSPACE_BYTES"""
    row_block = min(R, _DEFAULT_ROW_BLOCK) if row_block is None else int(row_block)
    if row_block < 1:
        raise ValueError('row_block must be positive')
    row_block = min(row_block, R)
    chunk = max(1, WORKSPACE_BYTES // 4 // row_block) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be positive')
    return row_block, min(chunk, N)


def block_spans(R, N, row_block, chunk, symmetric=False):
    """the blocks of an [R, N] similarity in the order a walk visits them, as (r0, nr, c0, nc, diag, mult): rows [r0, r0 + nr),
    columns [c0, c0 + nc), diag = r0 - c0 (row r of the block meets itself in column r + diag), mult = how often the block's
    pairs count.  Row blocks of `row_block`, column chunks of `chunk`, all columns with mult 1.  symmetric (R == N, one set
    against itself) visits, per row block, only the columns from r0 on and cuts the chunks at r0 + nr, so the block grid is
    aligned to the diagonal: the square [r0, r0 + nr)^2 holds both orders of its pairs and counts once (mult 1), every block to
    its right lies strictly above the diagonal and counts twice (mult 2).  No block straddles the diagonal raggedly, so no
    mirror block is ever needed.  Pure Python: no GPU."""
    for r0 in range(0, R, row_block):
        nr = min(row_block, R - r0)
        # (first column, end, mult) of the column ranges this row block visits
        ranges = [(r0, r0 + nr, 1), (r0 + nr, N, 2)] if symmetric else [(0, N, 1)]
        for lo, hi, mult in ranges:
            for c0 in range(lo, hi, chunk):
                yield r0, nr, c0, min(chunk, hi - c0), r0 - c0, mult


class SimilarityWalk:
    """one reused [row_block, chunk] fp32 workspace `sim` (pitch `chunk`); walk(q, b) forms q[r0:r0+nr] . b[c0:c0+nc]^T in it
    by dv_gemm_f32, span by span of block_spans, and hands each span to the caller while the block is there"""

    def __init__(self, row_block, chunk, device):
        self.row_block, self.chunk = row_block, chunk
        self.sim = torch.empty(row_block, chunk, dtype=torch.float32, device=device)

    def __call__(self, q, b, symmetric=False):
        """q [R, D], b [N, D] fp32, contiguous, on the device"""
        lib, s, D = L.load(), ops.stream_ptr(), q.shape[1]
        for span in block_spans(q.shape[0], b.shape[0], self.row_block, self.chunk, symmetric):
            r0, nr, c0, nc = span[:4]
            L.check(lib.dv_gemm_f32(nr, nc, D, q.data_ptr() + 4 * r0 * D, D, 1, b.data_ptr() + 4 * c0 * D, 1, D, self.sim.data_ptr(),
                                    self.chunk, 1.0, 0, s), 'dv_gemm_f32')
            yield span


def centre_normalise(x):
    """x [n, D] fp32 on the device -> the rows minus the column mean, then L2-normalised (eps 1e-12): retrieval's preparation"""
    lib, s = L.load(), ops.stream_ptr()
    x = x.float().contiguous()
    M, D = x.shape
    assert D % 8 == 0
    col = torch.zeros(D, dtype=torch.float32, device=x.device)
    L.check(lib.dv_colsum_f32(x.data_ptr(), D, M, D, col.data_ptr(), s), 'dv_colsum_f32')
    one, shift = torch.ones(D, dtype=torch.float32, device=x.device), torch.zeros(D, dtype=torch.float32, device=x.device)
    L.check(lib.dv_addcmul_f32(shift.data_ptr(), col.data_ptr(), 0, -1.0 / M, D, s), 'dv_addcmul_f32')       # -mean
    c = torch.empty_like(x)
    L.check(lib.dv_bn_apply(DV_F32, x.data_ptr(), D, one.data_ptr(), shift.data_ptr(), 0, 0, c.data_ptr(), D, M, D, 0, s), 'centre')
    y, nrm = torch.empty_like(x), torch.empty(M, dtype=torch.float32, device=x.device)
    L.check(lib.dv_l2norm_fwd(c.data_ptr(), M, D, 1e-12, y.data_ptr(), nrm.data_ptr(), s), 'dv_l2norm_fwd')
    return y


def normalise(x, centre=False):
    """x [n, D] -> [n, D] fp32 on the device, every row L2-normalised (eps 1e-12), centred first as retrieval does when `centre`;
    a host tensor is moved to the device"""
    if not x.is_cuda:
        x = x.to('cuda')
    if centre:
        return centre_normalise(x)
    x = x.float().contiguous()
    y, nrm = torch.empty_like(x), torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.load().dv_l2norm_fwd(x.data_ptr(), x.shape[0], x.shape[1], 1e-12, y.data_ptr(), nrm.data_ptr(), ops.stream_ptr()),
            'dv_l2norm_fwd')
    return y


def clip_rows(per_feature, video_label=None):
    """per_feature [n_video, num_seq, D] (the per-clip features `classifier.py --retrieval` saves; a video's clips adjacent),
    video_label [n_video] or None -> (feat [n, D] with row = video * num_seq + clip, vid [n] = the video's row, cls [n] = its
    label or None, n_video, num_seq); the ids are int64 on the host"""
    if per_feature.dim() != 3:
        raise ValueError('per_feature must be [n_video, num_seq, D] (= [V, S, D]), got %s' % (tuple(per_feature.shape),))
    n_video, num_seq, D = per_feature.shape
    cls = None
    if video_label is not None:
        label = torch.as_tensor(video_label).reshape(-1)
        if label.numel() != n_video:
            raise ValueError('video_label must hold one label per video (%d), got %d' % (n_video, label.numel()))
        cls = label.cpu().long().repeat_interleave(num_seq)
    vid = torch.arange(n_video).repeat_interleave(num_seq)
    return per_feature.reshape(n_video * num_seq, D), vid, cls, n_video, num_seq


def workspace(nbytes, device, name):
    """the answer of the workspace query `name` -> a float64 tensor of at least nbytes (and at least one element, so that it has
    a pointer); a negative answer is the query's error code and raises through L.check"""
    nbytes = int(nbytes)
    if nbytes < 0:
        L.check(nbytes, name)
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)


def gemm_desc(A, B, C, M, N, K, sbk, sbn, bias=None, alpha=1.0):
    """the GemmDesc of dv_gemm_f32_ex for C [M, N] = alpha A B (+ bias [N], DV_BIAS): A [M, K] and C row-major and dense, B read
    as B[k * sbk + n * sbn]; A, B, C, bias are device pointers"""
    d = L.GemmDesc()
    d.A, d.B, d.C, d.bias = A, B, C, bias
    d.sam, d.sak, d.sbk, d.sbn, d.ldc = K, 1, sbk, sbn, N
    d.M, d.N, d.K, d.flags, d.alpha = M, N, K, 0 if bias is None else L.DV_BIAS, alpha
    return d
