"""GPU: the streaming similarity walk of dualvar_amd/utils/features.py.  Every block SimilarityWalk hands to its caller holds
exactly what a direct dv_gemm_f32 call at the same offsets and pitch writes (the same launch, so the comparison is bitwise), the
spans cover what block_spans says and nothing else is written."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from dualvar_amd.utils import features as F  # noqa: E402


@pytest.mark.parametrize('R,N,row_block,chunk,symmetric', [(13, 29, 5, 7, False), (17, 17, 5, 4, True)])
def test_walk_blocks_are_the_direct_products(gpu, R, N, row_block, chunk, symmetric):
    D = 8
    gen = torch.Generator().manual_seed(R * N)
    q = torch.randn((R, D), generator=gen).to(gpu)
    b = q if symmetric else torch.randn((N, D), generator=gen).to(gpu)
    lib, s = _lib.load(), ops.stream_ptr()
    walk = F.SimilarityWalk(row_block, chunk, gpu)
    assert tuple(walk.sim.shape) == (row_block, chunk) and walk.sim.dtype == torch.float32
    got = torch.full((R, N), math.nan, device=gpu)
    want = torch.full((R, N), math.nan, device=gpu)
    direct = torch.empty(row_block, chunk, device=gpu)
    spans = walk(q, b, symmetric)
    while True:
        walk.sim.fill_(math.nan)
        span = next(spans, None)
        if span is None:
            break
        r0, nr, c0, nc = span[:4]
        got[r0:r0 + nr, c0:c0 + nc] = walk.sim[:nr, :nc]
        assert bool(torch.isnan(walk.sim[nr:]).all()) and bool(torch.isnan(walk.sim[:, nc:]).all()), span      # nothing beyond the block
        direct.fill_(math.nan)
        _lib.check(lib.dv_gemm_f32(nr, nc, D, q.data_ptr() + 4 * r0 * D, D, 1, b.data_ptr() + 4 * c0 * D, 1, D, direct.data_ptr(),
                                   chunk, 1.0, 0, s), 'dv_gemm_f32')
        want[r0:r0 + nr, c0:c0 + nc] = direct[:nr, :nc]
    covered = torch.zeros(R, N, dtype=torch.bool)
    for r0, nr, c0, nc, _, _ in F.block_spans(R, N, row_block, chunk, symmetric):
        covered[r0:r0 + nr, c0:c0 + nc] = True
    covered = covered.to(gpu)
    assert bool(covered.all()) != symmetric
    assert not bool(torch.isnan(want[covered]).any())
    assert torch.equal(got[covered], want[covered])
    assert bool(torch.isnan(got[~covered]).all())                    # symmetric: the blocks below the diagonal squares stay untouched
