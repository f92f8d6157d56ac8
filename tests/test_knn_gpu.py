"""The streaming top-k selection (dv_topk_merge_f32), the weighted k-NN vote (dv_knn_vote), their host module
(dualvar_amd/utils/knn.py) and `classifier.py --retrieval --knn` against float64 references written here from
include/dualvar_select.h.

Conventions (those of tests/test_loss_gemm_optim_gpu.py; the helpers are tests/checks.py's): outputs sit in buffers filled with a NaN
bit pattern no kernel produces and larger than needed (two more rows, ldk = k + 2, lds = n_class + 3): after every call the rows
>= R and the columns >= k / >= n_class must still hold it.  Input rows carry NaN in sim[:, n_cols:ld).

Selection reference: the row in float64, NaN -> -inf, -0 -> +0, torch.sort(descending, stable) (the stable sort keeps ascending
index among equals), -inf entries dropped, k taken, padded with (-inf, -1).  Values must match as bits (after + 0.0), indices
with torch.equal.  The grid data (multiples of 1/4 in [-2, 2], 17 distinct values) puts the k-th boundary inside a tie group
(asserted from the reference for every case with n_cols >= 4k).

Vote bounds, u = 2^-24:
  inv_T = 0: the counts are exact integers, score = cnt / n_valid is one correctly rounded division: |err| <= u * score, and
      exact where n_valid is a power of two.  pred = the lowest-index arg-max of the integer counts in every row.
  inv_T > 0: x_i = (v_i - v_0) * inv_T has two roundings (<= 2u |x_i|), scaled 1:1 into w_i = expf(x_i) (measured 1.39 u on
      [-87, 0], taken as E_EXPF = 2.8 u); the class sum and the total are chains of at most k additions of positive terms
      (k u each), the division one more:   b(score_c) = score_c * [(2k + 2) u + 2 max_i (E_EXPF + 2u |x_i|)].
      The kernel calls expf, not __expf.  pred must equal the float64 arg-max wherever the float64 top-two gap exceeds the sum
      of the two classes' bounds; at least 95 % of the rows must be decidable so (condition on the data, asserted).
  knn_eval: the lists come from dv_gemm_f32 products, |v_i - s64_i| <= g_i (gemm_bound), so x_i carries (g_i + g_0) inv_T more:
      the bracket gains 2 * 2 max_i g_i * inv_T; where the k-th and (k+1)-th float64 products are closer than 2 max g, either
      may vote in fp32 and the row is decidable if both choices are and agree (see eval_ref64).  Acc@5 is decided by the number
      of classes above the target's score beyond the two bounds (>= 5: a miss) or possibly above it (< 5: a hit).
Each case prints (-s) err / bound.  Largest err / bound measured on an MI355X: vote.count 0.99 (one correctly rounded division
reaches its half ulp), vote.score 0.035, topk_neighbours |val - s64| 0.011; every row of the Gaussian vote cases decidable,
128 / 127 of 130 rows of knn_eval at k = 200 for Acc@1 / Acc@5.  The whole file takes about 15 s, 11.5 s of it the two
classifier.py children (5 s each, so the optional second child runs).
"""
import functools
import math
import os
import re
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import ops  # noqa: E402
from tests import checks  # noqa: E402
from tests.chains import E_EXPF, gemm_bound, gemm_chain  # noqa: E402
from tests.checks import U, Ratios, child as _child, f32, is_sent, report_fixture, sent  # noqa: E402
from tests.dataset_support import write_dataset  # noqa: E402
from tests.eval_support import chunks_of, grid_rows, knn_eval_case, unit_gauss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
RATIO = Ratios()
within = RATIO.within
_report = report_fixture(RATIO, 20)
# bit for bit against float64: the reference must be an fp32 number; + 0.0 on both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)


# --------------------------------------------------------------------------------------------------------------- helpers
def select_ref(rows, k, col0=0):
    """rows [R, n] (any float dtype, NaN / inf allowed) -> (val [R, k] float64, idx [R, k] int32) of the header's total order"""
    x = rows.double().clone()
    x[torch.isnan(x)] = -INF
    x = x + 0.0
    v, i = torch.sort(x, dim=1, descending=True, stable=True)
    i = i + col0
    i[v == -INF] = -1
    R, n = x.shape
    if n < k:
        v = torch.cat([v, torch.full((R, k - n), -INF, dtype=v.dtype, device=v.device)], 1)
        i = torch.cat([i, torch.full((R, k - n), -1, dtype=i.dtype, device=i.device)], 1)
    return v[:, :k].contiguous(), i[:, :k].int().contiguous()


class Lists:
    """the [R][ldk] state inside sentinel buffers of R + 2 rows and ldk = k + 2 columns"""

    def __init__(self, R, k, dev):
        self.R, self.k, self.ldk = R, k, k + 2
        self.val, self.idx = sent((R + 2, self.ldk), dev), sent((R + 2, self.ldk), dev, torch.int32)

    def frame_ok(self):
        return (is_sent(self.val[self.R:]) and is_sent(self.idx[self.R:]) and is_sent(self.val[:self.R, self.k:])
                and is_sent(self.idx[:self.R, self.k:]))

    def check(self, ref_v, ref_i, what):
        assert self.frame_ok(), what + ': wrote outside [R][k]'
        same_bits(self.val[:self.R, :self.k], ref_v.to(self.val.device), what + ' values')
        got = self.idx[:self.R, :self.k]
        want = ref_i.to(got.device)
        bad = got != want
        assert torch.equal(got, want), '%s indices: %d differ, first at %s: got %d want %d' % (
            what, int(bad.sum()), bad.nonzero()[0].tolist(), int(got[bad][0]), int(want[bad][0]))


def sim_buffer(rows, dev):
    """rows [R, n] -> device buffer [R, n + 3] with NaN in the pitch padding"""
    R, n = rows.shape
    buf = torch.full((R, n + 3), float('nan'), dtype=torch.float32, device=dev)
    buf[:, :n] = rows.to(dev)
    return buf


def merge(buf, n, k, col0, lists, chunks=None):
    """feed columns [0, n) of buf to dv_topk_merge_f32, whole or as the (start, length) chunks given; `first` on the first call"""
    R, ld = buf.shape
    for t, (c, m) in enumerate(chunks or [(0, n)]):
        ops.call('dv_topk_merge_f32', buf.data_ptr() + 4 * c, ld, R, m, col0 + c, k, lists.val, lists.idx, lists.ldk, int(t == 0))
        assert lists.frame_ok(), 'chunk %d wrote outside [R][k]' % t


# -------------------------------------------------------------------------------------------- 1. selection, exact with ties
#         (R, k, n_cols, col0): the wave (63 / 64 / 65), buffer and power-of-two edges of k and n_cols; n_cols < k for every k > 1
SELECT_CASES = [
    (1, 1, 1, 0), (5, 1, 64, 7), (130, 1, 257, 0), (5, 1, 5000, 7),
    (5, 5, 1, 0), (1, 5, 63, 7), (130, 5, 65, 0), (5, 5, 256, 7), (5, 5, 1000, 0), (1, 5, 5000, 7),
    (5, 63, 1, 7), (130, 63, 63, 0), (5, 63, 64, 7), (1, 63, 255, 0), (5, 63, 1000, 7), (5, 63, 5000, 0),
    (5, 64, 63, 0), (1, 64, 64, 7), (130, 64, 65, 0), (5, 64, 256, 7), (5, 64, 257, 0), (130, 64, 5000, 7),
    (5, 65, 64, 7), (1, 65, 65, 0), (5, 65, 255, 7), (130, 65, 1000, 0), (5, 65, 5000, 7),
    (5, 200, 1, 0), (5, 200, 65, 7), (1, 200, 255, 0), (130, 200, 256, 7), (5, 200, 257, 0), (5, 200, 1000, 7), (130, 200, 5000, 0),
    (5, 256, 63, 7), (1, 256, 255, 0), (5, 256, 256, 7), (130, 256, 257, 0), (5, 256, 1000, 7), (5, 256, 5000, 0), (1, 256, 5000, 7),
]


def select_seed(R, k, n):
    return 100000 * R + 1000 * k + n


@pytest.mark.parametrize('case', SELECT_CASES, ids=['R%d-k%d-n%d-c%d' % c for c in SELECT_CASES])
def test_selection_exact_with_ties(gpu, case):
    R, k, n, col0 = case
    rows = grid_rows(select_seed(R, k, n), R, n)
    ref_v, ref_i = select_ref(rows, k, col0)
    if n >= 4 * k:                  # the k-th and the (k+1)-th of some row are equal: the boundary falls inside a tie group
        full = torch.sort(rows.double(), dim=1, descending=True).values
        assert bool((full[:, k - 1] == full[:, k]).any()), 'no tie at the k-th boundary in the test data'
    if n < k:
        assert bool((ref_i[:, n:] == -1).all()) and bool((ref_v[:, n:] == -INF).all())
    lists = Lists(R, k, gpu)
    merge(sim_buffer(rows, gpu), n, k, col0, lists)
    lists.check(ref_v, ref_i, 'topk R=%d k=%d n=%d col0=%d' % case)


# -------------------------------------------------------------------------------------------------- 2. adversarial rows
def adversarial_rows(n):
    asc = torch.arange(n, dtype=torch.float32) / 8 - 300                    # strictly ascending: every element beats the threshold
    mixed = grid_rows(77, 1, n)[0]
    mixed[[3, 64, 1000, n - 1]] = float('nan')
    mixed[[0, 65, 2000]] = -INF
    mixed[[5, 4097]] = INF
    mixed[[7, 63, 128, 129, 3000]] = -0.0
    mixed[[8, 200]] = 0.0
    empty = torch.full((n,), float('nan'))
    empty[1::2] = -INF
    return {'ascending': asc, 'descending': asc.flip(0), 'constant': torch.full((n,), 0.25), 'empty': empty, 'mixed': mixed}


@pytest.mark.parametrize('kind', ['ascending', 'descending', 'constant', 'empty', 'mixed'])
@pytest.mark.parametrize('k', [64, 200])
def test_selection_adversarial_rows(gpu, k, kind):
    n = 5000
    rows = adversarial_rows(n)[kind][None, :]
    ref_v, ref_i = select_ref(rows, k, 7)
    if kind == 'empty':
        assert bool((ref_i == -1).all()) and bool((ref_v == -INF).all())
    if kind == 'mixed':
        assert ref_i[0, :2].tolist() == [7 + 5, 7 + 4097] and bool(torch.isinf(ref_v[0, :2]).all())
        assert not bool(torch.isin(ref_i[0], torch.tensor([3, 64, 1000, n - 1, 0, 65, 2000], dtype=torch.int32) + 7).any())
    if kind == 'constant':
        assert ref_i[0].tolist() == list(range(7, 7 + k))
    lists = Lists(1, k, gpu)
    merge(sim_buffer(rows, gpu), n, k, 7, lists)
    lists.check(ref_v, ref_i, 'topk %s k=%d' % (kind, k))


# ----------------------------------------------------------------------------------------------- 3. chunking is invisible
@pytest.mark.parametrize('k', [5, 200])
def test_chunking_is_invisible(gpu, k):
    R, N = 5, 5000
    rows = grid_rows(4242, R, N)
    buf = sim_buffer(rows, gpu)
    ref_v, ref_i = select_ref(rows, k)
    single = Lists(R, k, gpu)
    merge(buf, N, k, 0, single)
    single.check(ref_v, ref_i, 'single call k=%d' % k)
    again = Lists(R, k, gpu)                                                # a second launch: the same bits
    merge(buf, N, k, 0, again)
    assert torch.equal(again.val.view(torch.int32), single.val.view(torch.int32)) and torch.equal(again.idx, single.idx)
    for m, desc in ((1000, False), (257, False), (64, False), (257, True)):
        lists = Lists(R, k, gpu)
        merge(buf, N, k, 0, lists, chunks_of(N, m, desc))
        what = 'chunks of %d %s k=%d' % (m, 'descending' if desc else 'ascending', k)
        lists.check(ref_v, ref_i, what)
        assert torch.equal(lists.val.view(torch.int32), single.val.view(torch.int32)) and torch.equal(lists.idx, single.idx), what
    n1 = 300                                                                # one column per call: 300 launches
    ref_v1, ref_i1 = select_ref(rows[:, :n1], k)
    one, whole = Lists(R, k, gpu), Lists(R, k, gpu)
    merge(buf, n1, k, 0, one, chunks_of(n1, 1))
    merge(buf, n1, k, 0, whole)
    one.check(ref_v1, ref_i1, 'chunks of 1 k=%d' % k)
    whole.check(ref_v1, ref_i1, 'single call N=300 k=%d' % k)
    assert torch.equal(one.val.view(torch.int32), whole.val.view(torch.int32)) and torch.equal(one.idx, whole.idx)


# ------------------------------------------------------------------------------------------------ 4. vote, exact (inv_T = 0)
def run_vote(gpu, val, idx, labels, n_class, inv_T):
    """val / idx [R, k] on the host -> (score [R, n_class], pred [R]) from dv_knn_vote, frames checked"""
    R, k = val.shape
    ldk, lds = k + 2, n_class + 3
    tv, ti = sent((R + 2, ldk), gpu), sent((R + 2, ldk), gpu, torch.int32)
    tv[:R, :k], ti[:R, :k] = val.to(gpu), idx.to(gpu)
    score, pred = sent((R + 2, lds), gpu), sent((R + 8,), gpu, torch.int32)
    ops.call('dv_knn_vote', tv, ti, ldk, R, k, labels.to(gpu), labels.numel(), n_class, inv_T, score, lds, pred)
    assert is_sent(score[R:]) and is_sent(score[:R, n_class:]) and is_sent(pred[R:]), 'dv_knn_vote wrote outside its outputs'
    return score[:R, :n_class], pred[:R]


def valid_labels(idx, labels, n_class):
    """[R, k] label of every valid neighbour, -1 for the invalid ones (the header's set V)"""
    n_bank = labels.numel()
    ok = (idx >= 0) & (idx < n_bank)
    lab = labels.long()[idx.long().clamp(0, n_bank - 1)]
    return torch.where(ok & (lab >= 0) & (lab < n_class), lab, torch.full_like(lab, -1))


@pytest.mark.parametrize('C', [1, 3, 101, 400])
@pytest.mark.parametrize('k', [1, 64, 200, 256])
def test_vote_exact_counts(gpu, k, C):
    """neighbour lists of the grid data of case 1 (R = 130, 300 columns, col0 = 7), labels from 0..C-1; one bank label out of
    range above, one below, one index >= n_bank, rows with -1 slots (one of them down to a power of two), one empty row"""
    R, n, col0 = 130, 300, 7
    val, idx = select_ref(grid_rows(select_seed(R, k, n), R, n), k, col0)
    n_bank = col0 + n
    gen = torch.Generator().manual_seed(31 * k + C)
    labels = torch.randint(0, C, (n_bank,), generator=gen, dtype=torch.int32)
    labels[int(idx[0, 0])] = C                                              # out of range: that neighbour does not vote
    labels[int(idx[1, 0])] = -3
    idx[2, 0] = n_bank + 5                                                  # not read
    p2 = 1 << (k.bit_length() - 1)
    if k > 7:
        idx[10:20, -7:], val[10:20, -7:] = -1, -INF
        idx[20:30, p2 // 2:], val[20:30, p2 // 2:] = -1, -INF               # p2 / 2 valid neighbours
    idx[3, :], val[3, :] = -1, -INF                                         # empty row
    lab = valid_labels(idx, labels, C)
    assert int(lab[0, 0]) == -1 and int(lab[1, 0]) == -1 and int(lab[2, 0]) == -1 and bool((lab[3] == -1).all())
    cnt = torch.stack([(lab == c).sum(1) for c in range(C)], 1)             # [R, C] exact integers
    n_valid = (lab >= 0).sum(1)
    empty = n_valid == 0
    assert bool(empty[3]) and (k > 1 or bool(empty[:4].all()))              # k = 1: rows 0, 1, 2 lose their only neighbour
    ref = torch.where(empty[:, None], torch.zeros(R, C, dtype=torch.float64), cnt.double() / n_valid.clamp(min=1)[:, None].double())
    want_pred = torch.where(empty, torch.full((R,), -1), cnt.argmax(1))
    assert torch.equal(want_pred[~empty], (cnt == cnt.max(1, keepdim=True).values).int().argmax(1)[~empty])   # the LOWEST arg-max
    if C >= 3 and k >= 64:          # count ties between the two leading classes pin the lowest-class rule
        top2 = cnt.topk(2, dim=1).values
        assert bool(((top2[:, 0] == top2[:, 1]) & ~empty).any()), 'no count tie between the two leading classes in the test data'
    score, pred = run_vote(gpu, val.float(), idx, labels, C, 0.0)
    what = 'vote.count k=%d C=%d' % (k, C)
    within(score, ref.to(gpu), (U * ref).to(gpu), what)
    pow2 = (n_valid & (n_valid - 1)) == 0
    assert bool((pow2 & ~empty).any())
    if k > 7 and k != p2:
        assert bool((~pow2).any())
    same_bits(score[pow2.to(gpu)], ref[pow2].to(gpu), what + ' (n_valid a power of two)')
    assert torch.equal(pred.cpu().long(), want_pred), what + ': pred is not the lowest-index arg-max of the counts'
    assert bool((score[3] == 0).all()) and int(pred[3]) == -1


def test_vote_degenerate_totals_count_as_empty(gpu):
    """lists that are not as dv_topk_merge_f32 leaves them: top_val[r][0] = -inf in front of valid slots (every weight +inf) and
    an invalid leading slot so far above the rest that every valid weight underflows (total 0): both rows come out as an empty
    vote -- zero scores, pred -1, nothing NaN -- while a regular row beside them is scored as usual"""
    k, C = 4, 3
    inv_T = f32(1.0 / 0.07)
    labels = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)
    val = torch.tensor([[-INF, 0.5, 0.25, 0.0], [100.0, -100.0, -100.0, -100.0], [1.0, 0.5, 0.25, 0.0]])
    idx = torch.tensor([[-1, 1, 2, 3], [77, 1, 2, 3], [0, 1, 2, 3]], dtype=torch.int32)       # 77 >= n_bank: not a voter
    score, pred = run_vote(gpu, val, idx, labels, C, inv_T)
    assert bool(torch.isfinite(score).all())
    assert bool((score[:2] == 0).all()) and pred[:2].tolist() == [-1, -1]
    score64, bound = vote_ref64(val[2:].double(), valid_labels(idx[2:], labels, C), C, inv_T)
    within(score[2:], score64.to(gpu), bound.to(gpu), 'vote.score beside degenerate rows')
    assert int(pred[2]) == int(score64.argmax(1)[0]) == 0


# ------------------------------------------------------------------------------------------- 5. vote, Gaussian, derived bound
def vote_ref64(val, lab, n_class, inv_T, extra=0.0):
    """val [R, k] fp32 values as float64, lab [R, k] valid labels -> (score64 [R, C], bound [R, C]); extra: added to the bracket's
    per-weight term (the error the values themselves carry, times inv_T)"""
    k = val.shape[1]
    x = (val - val[:, :1]) * inv_T
    w = torch.exp(x) * (lab >= 0)
    num = torch.stack([(w * (lab == c)).sum(1) for c in range(n_class)], 1)
    score = num / w.sum(1, keepdim=True)
    per_w = (E_EXPF + 2 * U * x.abs() + extra).max(1).values
    return score, score * ((2 * k + 2) * U + 2 * per_w)[:, None]


def decidable_top1(score, bound):
    top = score.topk(min(2, score.shape[1]), dim=1)
    if score.shape[1] == 1:
        return torch.ones(score.shape[0], dtype=torch.bool, device=score.device), top.indices[:, 0]
    gap = top.values[:, 0] - top.values[:, 1]
    room = bound.gather(1, top.indices[:, :1])[:, 0] + bound.gather(1, top.indices[:, 1:2])[:, 0]
    return gap > room, top.indices[:, 0]


VOTE_GAUSS = [(130, 1000, 128, 200, 10, 0.07), (130, 5000, 128, 200, 101, 0.07), (5, 257, 64, 64, 3, 1.0), (130, 1000, 128, 256, 10, 0.07)]


def test_vote_gaussian_bounds(gpu):
    rows_total = rows_decidable = 0
    for t, (R, N, D, k, C, T) in enumerate(VOTE_GAUSS):
        gen = torch.Generator().manual_seed(900 + t)
        q, b = unit_gauss(gen, R, D), unit_gauss(gen, N, D)
        labels = torch.randint(0, C, (N,), generator=gen, dtype=torch.int32)
        s = (q.double() @ b.double().t()).float()
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        val, idx = v[:, :k].contiguous(), i[:, :k].int().contiguous()
        inv_T = f32(1.0 / T)
        score64, bound = vote_ref64(val.double(), valid_labels(idx, labels, C), C, inv_T)
        ok, arg64 = decidable_top1(score64, bound)
        score, pred = run_vote(gpu, val, idx, labels, C, inv_T)
        within(score, score64.to(gpu), bound.to(gpu), 'vote.score R=%d N=%d k=%d C=%d T=%g' % (R, N, k, C, T))
        assert torch.equal(pred.cpu().long()[ok], arg64[ok]), 'pred differs from the float64 arg-max in a decidable row'
        rows_total, rows_decidable = rows_total + R, rows_decidable + int(ok.sum())
        top = score64.topk(2, dim=1).values
        print('    decidable rows %d of %d; smallest top-two gap %.2e, largest relative bound %.2e'
              % (int(ok.sum()), R, float((top[:, 0] - top[:, 1]).min()), float((bound / score64.clamp(min=1e-300)).max())))
    assert rows_decidable >= 0.95 * rows_total, (rows_decidable, rows_total)


# ----------------------------------------------------------------------------------- 6. topk_neighbours end to end, exact
@pytest.mark.parametrize('R,N,k', [(5, 300, 5), (130, 1000, 200), (3, 5000, 256)])
def test_topk_neighbours_grid_exact(gpu, R, N, k):
    """features are multiples of 1/4 in [-2, 2], D = 128: every dot product is a multiple of 1/16 below 512, exact in fp32 in any
    order, so every chunking equals float64 bit for bit, ties included"""
    from dualvar_amd.utils import features, knn
    D = 128
    q64, b64 = grid_rows(R + N, R, D).double(), grid_rows(R * N + 1, N, D).double()
    assert float((q64.abs() @ b64.abs().t()).max()) < 512
    ref_v, ref_i = select_ref(q64 @ b64.t(), k)
    if N >= 1000:                   # (the five largest of 300 products are distinct; equal products inside the list need k >> 5)
        tie = torch.sort(q64 @ b64.t(), dim=1, descending=True).values
        assert bool((tie[:, k - 1] == tie[:, k]).any()), 'no tie at the k-th boundary in the test data'
    q, b = q64.float().to(gpu), b64.float().to(gpu)
    for chunk in (64, 257, N):
        for row_block in (1, 64, R):
            val, idx = knn.topk_neighbours(q, b, k, chunk=chunk, row_block=row_block)
            what = 'topk_neighbours R=%d N=%d k=%d chunk=%d row_block=%d' % (R, N, k, chunk, row_block)
            assert val.shape == (R, k) and idx.shape == (R, k) and val.dtype == torch.float32 and idx.dtype == torch.int32
            same_bits(val, ref_v.to(gpu), what)
            assert torch.equal(idx, ref_i.to(gpu)), what
    if (R, N) == (3, 5000):         # the [R, N] matrix is never allocated: the peak stays below R * N floats
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        val, idx = knn.topk_neighbours(q, b, k, chunk=64)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        outputs = 2 * R * k * 4
        assert grown < R * N * 4 and grown <= features.WORKSPACE_BYTES + outputs, grown     # here: a [3, 64] workspace and the lists
        assert torch.equal(idx, ref_i.to(gpu))


# ------------------------------------------------------------------- 7. topk_neighbours end to end, Gaussian, interval check
def test_topk_neighbours_gaussian_interval(gpu):
    from dualvar_amd.utils import features, knn
    R, N, D, k = 130, 5000, 512, 200
    gen = torch.Generator().manual_seed(7)
    q, b = unit_gauss(gen, R, D).to(gpu), unit_gauss(gen, N, D).to(gpu)
    s64 = q.double() @ b.double().t()
    bound = gemm_bound(q.double(), b.double(), 1.0, gemm_chain(R, N, D))     # the defaults form one [R, N] product here
    assert features.blocks(R, N) == (R, N)
    val, idx = knn.topk_neighbours(q, b, k)
    li = idx.long()
    assert bool((idx >= 0).all()) and bool((idx < N).all())
    assert all(len(set(row)) == k for row in idx.cpu().tolist()), 'an index is returned twice'
    err = (val.double() - s64.gather(1, li)).abs()
    ratio = float((err / bound.gather(1, li)).max())
    print('    topk_neighbours gaussian: max |val - s64| / bound = %.3f' % ratio)
    assert ratio <= 1.0
    dv, di = val[:, 1:] - val[:, :-1], idx[:, 1:] - idx[:, :-1]
    assert bool((dv <= 0).all()) and bool((di[dv == 0] > 0).all()), 'not in the order of the header'
    out = torch.ones(R, N, dtype=torch.bool, device=gpu)
    out.scatter_(1, li, False)
    assert int(out.sum()) == R * (N - k)
    assert bool((s64 <= val[:, -1:].double() + bound)[out].all()), 'a column that was not returned beats the k-th value by more than its bound'


# ------------------------------------------------------------------------- 8. knn_eval against the tested retrieval path
def eval_ref64(ten, trn, tel, trl, C, k, T, ks, gpu):
    """float64 protocol on the normalised fp32 features the library formed: retrieval hits, decidable rows, pred, top-5 hits"""
    n_train = trn.shape[0]
    s64 = ten @ trn.t()
    g = gemm_bound(ten, trn, 1.0, gemm_chain(ten.shape[0], n_train, ten.shape[1]))     # one product of this shape in both paths
    gmax = g.max(1).values
    v, i = torch.sort(s64, dim=1, descending=True, stable=True)
    same = trl.to(gpu)[None, :] == tel.to(gpu)[:, None]
    masked = torch.where(same, s64, torch.full_like(s64, -INF))
    best, best_j = masked.max(1)
    rank64 = (s64 > best[:, None]).sum(1)
    # data property: the neighbours on either side of the ranks 1, 5, 10, 20, 50 lie more than twice the bound away from the best
    # same-label sample (unless they are that sample), so "a same-label sample among the first k" is the same decision in fp32
    for kq in ks:
        for pos in (kq - 1, kq):
            clear = (i[:, pos] == best_j) | ((v[:, pos] - best).abs() > 2 * gmax)
            assert bool(clear.all()), 'rank %d: a neighbour lies within twice the GEMM bound of the best same-label sample: take another seed' % kq
    retr = {kq: float((rank64.cpu() < kq).float().mean()) for kq in ks}
    kv = min(k, n_train)
    inv_T = 1.0 / T
    y = tel.to(gpu).long()
    others = torch.ones(ten.shape[0], C, dtype=torch.bool, device=s64.device).scatter_(1, y[:, None], False)

    def vote(cols):
        """the protocol with the voters i[:, cols]: (Acc@1 decidable, arg-max, Acc@5 decidable, Acc@5 hit)"""
        score64, bound = vote_ref64(v[:, cols], trl.to(gpu).long()[i[:, cols]], C, inv_T, extra=2 * gmax[:, None] * inv_T)
        ok, arg64 = decidable_top1(score64, bound)
        sy, by = score64.gather(1, y[:, None]), bound.gather(1, y[:, None])
        sure = (((score64 - sy) > bound + by) & others).sum(1)              # classes above the target's whatever the rounding
        maybe = (((score64 - sy) >= -(bound + by)) & others).sum(1)
        return ok, arg64, (sure >= 5) | (maybe < 5), maybe < 5

    ok, arg64, ok5, hit5 = vote(list(range(kv)))
    if kv < n_train:
        # where the kv-th and the (kv+1)-th product are closer than twice the bound, fp32 may let either one vote: such a row is
        # decidable if both choices are and agree (three products that close: undecidable)
        amb = (v[:, kv - 1] - v[:, kv]) <= 2 * gmax
        ok_b, arg_b, ok5_b, hit5_b = vote(list(range(kv - 1)) + [kv])
        crowded = ((v[:, kv - 2] - v[:, kv]) <= 2 * gmax) | ((v[:, kv - 1] - v[:, kv + 1]) <= 2 * gmax)
        ok = torch.where(amb, ok & ok_b & (arg64 == arg_b) & ~crowded, ok)
        ok5 = torch.where(amb, ok5 & ok5_b & (hit5 == hit5_b) & ~crowded, ok5)
    return retr, ok, arg64, ok5, hit5


def check_eval(res, ref, tel, trl, C, gpu, what):
    retr, ok, arg64, ok5, hit5 = ref
    R = tel.numel()
    assert int(ok.sum()) >= 0.95 * R and int(ok5.sum()) >= 0.95 * R, (what, int(ok.sum()), int(ok5.sum()))
    print('    %s: %d / %d of %d rows decidable for Acc@1 / Acc@5' % (what, int(ok.sum()), int(ok5.sum()), R))
    pred = res['pred'].long()
    assert torch.equal(pred[ok], arg64[ok]), what + ': pred differs from float64 in a decidable row'
    y = tel.to(gpu).long()
    lo1, lo5 = int(((arg64 == y) & ok).sum()), int((hit5 & ok5).sum())
    hi1, hi5 = lo1 + int((~ok).sum()), lo5 + int((~ok5).sum())
    assert lo1 - 0.5 <= res['knn_top1'] * R <= hi1 + 0.5 and lo5 - 0.5 <= res['knn_top5'] * R <= hi5 + 0.5, what
    assert abs(res['knn_top1'] - float((pred == y).float().mean())) < 1e-7
    # Acc@5 row by row: the vote again on the returned lists gives the scores knn_eval ranked (same entry, same bits)
    from dualvar_amd.utils import knn
    score, pred2 = knn.knn_classify(res['val'][:, :res['k']], res['idx'][:, :res['k']], trl, C, res['T'])
    assert torch.equal(pred2, res['pred'])
    row_hit = ((score > score.gather(1, y[:, None])).sum(1) < 5) & (pred2 >= 0)
    assert torch.equal(row_hit[ok5], hit5[ok5]), what + ': the Acc@5 decision differs from float64 in a decidable row'
    assert abs(res['knn_top5'] - float(row_hit.float().mean())) < 1e-7


def test_knn_eval_against_retrieval_and_float64(gpu):
    from dualvar_amd.utils import knn
    from dualvar_amd.utils.retrieval import nn_retrieval
    te, tel, tr, trl, C, ten, trn = knn_eval_case(gpu)
    ks = (1, 5, 10, 20, 50)
    ref = eval_ref64(ten, trn, tel, trl, C, 200, 0.07, ks, gpu)
    res = knn.knn_eval(te, tel, tr, trl, C, k=200, T=0.07, ks=ks)
    acc, _ = nn_retrieval(te, tel, tr, trl, ks=ks)
    assert res['retrieval'] == acc == ref[0], (res['retrieval'], acc, ref[0])
    assert res['k'] == 200 and res['T'] == 0.07 and res['val'].shape == (130, 200) and res['idx'].dtype == torch.int32
    check_eval(res, ref, tel, trl, C, gpu, 'knn_eval k=200')
    # k above the train-set size is clipped to it.  1500 > n_train = 1000 asks for lists of 1000 > DV_TOPK_MAX_K neighbours, which
    # topk_neighbours refuses; the clip itself is checked on the first 150 train samples
    with pytest.raises(ValueError, match='DV_TOPK_MAX_K'):
        knn.knn_eval(te, tel, tr, trl, C, k=1500)
    n_small = 150
    from dualvar_amd.utils.features import centre_normalise
    trn_s = centre_normalise(tr[:n_small]).double()
    ref_s = eval_ref64(ten, trn_s, tel, trl[:n_small], C, 1500, 0.07, ks, gpu)
    res_s = knn.knn_eval(te, tel, tr[:n_small], trl[:n_small], C, k=1500, T=0.07, ks=ks)
    acc_s, _ = nn_retrieval(te, tel, tr[:n_small], trl[:n_small], ks=ks)
    assert res_s['k'] == n_small and res_s['val'].shape == (130, n_small)
    assert torch.equal(res_s['idx'].long().sort(1).values, torch.arange(n_small, device=gpu).expand(130, n_small))
    assert res_s['retrieval'] == acc_s == ref_s[0]
    check_eval(res_s, ref_s, tel, trl[:n_small], C, gpu, 'knn_eval k=1500 clipped to 150')


# --------------------------------------------------------------------------------------------------- 9. the driver, one child
def test_cli_retrieval_with_knn(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp('knn_cli')
    split, frame = write_dataset(str(d / 'data'), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
    os.makedirs(str(d / 'run' / 'model'))
    base = [os.path.join(ROOT, 'classifier.py'), '--test', str(d / 'run' / 'model' / 'none.pth.tar'), '--retrieval', '--num_seq', '10',
            '--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
            '--split_root', split, '--frame_root', frame]
    t0 = time.time()
    out = _child(base + ['--knn', '--knn_k', '5'], str(d), 600)
    took = time.time() - t0
    assert 'no checkpoint found' in out                                     # random weights: the driver only warns
    nn = [float(v) for v in re.findall(r'\t\d+NN acc = ([0-9.]+)', out)]
    assert len(nn) == 5 and all(0.0 <= v <= 1.0 for v in nn) and nn == sorted(nn), out[-2000:]
    line = re.findall(r'kNN classifier \(k=5, T=0\.07\) on ucf101: Acc@1 = ([0-9.]+) Acc@5 = ([0-9.]+)', out)
    assert len(line) == 1 and all(0.0 <= float(v) <= 1.0 for v in line[0]), out[-2000:]
    fdir = str(d / 'run' / 'model' / 'feature')
    idx = torch.load(os.path.join(fdir, 'ucf101_knn_idx.pth.tar'), map_location='cpu', weights_only=True)
    val = torch.load(os.path.join(fdir, 'ucf101_knn_val.pth.tar'), map_location='cpu', weights_only=True)
    sim = torch.load(os.path.join(fdir, 'ucf101_sim.pth.tar'), map_location='cpu', weights_only=True)
    assert tuple(idx.shape) == (3, 5) and idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < 30
    assert all(len(set(r)) == 5 for r in idx.tolist())
    assert tuple(val.shape) == (3, 5) and val.dtype == torch.float32
    assert bool((val[:, 1:] <= val[:, :-1]).all()) and float(val.max()) <= 1 + 1e-5
    assert tuple(sim.shape) == (3, 30)
    sv, si = torch.sort(sim.double(), dim=1, descending=True, stable=True)
    clear = torch.ones(3, 5, dtype=torch.bool)
    gap = (sv[:, :5] - sv[:, 1:6]) > 1e-5                                   # position i differs from i + 1 ...
    clear &= gap
    clear[:, 1:] &= gap[:, :-1]                                             # ... and from i - 1
    assert torch.equal(idx.long()[clear], si[:, :5][clear])         # (the 30 train rows repeat 3 videos: many sims are equal)
    assert float((val.double() - sv[:, :5]).abs().max()) <= 1e-5
    if took <= 60:                  # the optional second child: without --knn nothing of it appears
        out2 = _child(base + ['--dirname', 'feature_plain'], str(d), 600)
        assert 'kNN classifier' not in out2 and len(re.findall(r'\t\d+NN acc = ', out2)) == 5
        plain = os.listdir(str(d / 'run' / 'model' / 'feature_plain'))
        assert plain and not [f for f in plain if 'knn' in f], plain
        print('    second child (without --knn) run: the first took %.0f s' % took)
    else:
        print('    second child (without --knn) not run: the first took %.0f s' % took)
