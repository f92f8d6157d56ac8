"""CPU: the host layer the clip-feature evaluations share (dualvar_amd/utils/features.py), as far as it needs no GPU: the default
blocks keep the similarity workspace bounded, block_spans covers an [R, N] similarity as the symmetric and the full walk of
variance.pair_statistics did, clip_rows and workspace on hand cases."""
import itertools

import pytest
import torch

from dualvar_amd import _lib
from dualvar_amd.utils import features as F


def test_default_blocks_keep_the_workspace_bounded():
    assert F.WORKSPACE_BYTES == 256 << 20
    for R, N in ((3, 30), (3783, 9537), (19900, 240000), (1, 10 ** 8), (10 ** 6, 7)):       # UCF101, Kinetics-400, extremes
        rb, ch = F.blocks(R, N)
        assert 1 <= rb <= R and 1 <= ch <= N and rb * ch * 4 <= F.WORKSPACE_BYTES, (R, N, rb, ch)
        assert rb * ch * 4 < R * N * 4 or R * N * 4 <= F.WORKSPACE_BYTES                   # never the full matrix beyond the bound
    assert F.blocks(3783, 9537) == (3783, 9537)                                            # UCF101: one product, 144 MB
    assert F.blocks(130, 1000, row_block=64, chunk=257) == (64, 257) and F.blocks(5, 300, 1000, 1000) == (5, 300)
    for bad in ((0, None), (None, 0), (-1, 5)):
        with pytest.raises(ValueError):
            F.blocks(10, 10, *bad)


def _count(R, N, row_block, chunk, symmetric):
    """how often the spans count each cell of [R, N]; every span is checked on the way"""
    count = torch.zeros(R, N, dtype=torch.int64)
    for r0, nr, c0, nc, diag, mult in F.block_spans(R, N, row_block, chunk, symmetric):
        assert 1 <= nr <= row_block and 1 <= nc <= chunk and diag == r0 - c0, (r0, nr, c0, nc, diag)
        assert 0 <= r0 and r0 + nr <= R and 0 <= c0 and c0 + nc <= N
        count[r0:r0 + nr, c0:c0 + nc] += mult
    return count


@pytest.mark.parametrize('n', (1, 2, 5, 17, 64, 65, 130))
def test_block_spans_cover_the_square(n):
    """non-symmetric: every cell once.  Symmetric: a cell counts once if its column lies in its row's block, twice if in a later
    block, never if in an earlier one: with the mirror pairs, every unordered pair twice."""
    for rb, ch in itertools.product((1, 3, 16, 64, 200), (1, 7, 64, 257)):
        row_block, chunk = F.blocks(n, n, rb, ch)
        assert torch.equal(_count(n, n, row_block, chunk, False), torch.ones(n, n, dtype=torch.int64)), (n, rb, ch)
        block = torch.arange(n) // row_block
        want = torch.where(block[None, :] == block[:, None], 1, torch.where(block[None, :] > block[:, None], 2, 0))
        assert torch.equal(_count(n, n, row_block, chunk, True), want), (n, rb, ch)


def test_block_spans_cover_a_rectangle():
    assert torch.equal(_count(13, 29, 5, 7, False), torch.ones(13, 29, dtype=torch.int64))
    assert list(F.block_spans(3, 5, 2, 4)) == [(0, 2, 0, 4, 0, 1), (0, 2, 4, 1, -4, 1), (2, 1, 0, 4, 2, 1), (2, 1, 4, 1, -2, 1)]


def test_clip_rows():
    x = torch.arange(3 * 2 * 4, dtype=torch.float32).reshape(3, 2, 4)
    feat, vid, cls, n_video, num_seq = F.clip_rows(x, [7, 5, 7])
    assert (n_video, num_seq) == (3, 2) and torch.equal(feat, x.reshape(6, 4))
    assert vid.tolist() == [0, 0, 1, 1, 2, 2] and cls.tolist() == [7, 7, 5, 5, 7, 7]
    assert vid.dtype == cls.dtype == torch.int64 and not vid.is_cuda and not cls.is_cuda
    assert F.clip_rows(x)[2] is None and F.clip_rows(x, torch.tensor([[1], [2], [3]]))[2].tolist() == [1, 1, 2, 2, 3, 3]
    for bad in (torch.zeros(6, 4), torch.zeros(3, 2, 4, 1), torch.zeros(4)):
        with pytest.raises(ValueError, match='n_video, num_seq, D'):
            F.clip_rows(bad, [0, 1, 2])
    for bad in ([0, 1], [0, 1, 2, 3], torch.zeros(3, 2)):
        with pytest.raises(ValueError, match='one label per video'):
            F.clip_rows(x, bad)


def test_workspace():
    with pytest.raises(_lib.DualVarHipError, match='dv_some_workspace'):
        F.workspace(-1, 'cpu', 'dv_some_workspace')
    for nbytes, want in ((0, 1), (8, 1), (12, 2)):
        ws = F.workspace(nbytes, 'cpu', 'dv_some_workspace')
        assert ws.dtype == torch.float64 and ws.numel() == want and ws.numel() * 8 >= nbytes and ws.data_ptr() % 8 == 0
