"""The full-ranking entries (dv_rankeval_gather_f32, dv_rankeval_sort, dv_rankeval_count_f32, dv_rankeval_finish), their host
module (dualvar_amd/utils/rankeval.py) and `classifier.py --retrieval --map` against the float64 / integer model of
tests/rankeval_reference.py, written from include/dualvar_rankeval.h.

Everything the kernels produce is an integer or a fixed sequence of IEEE operations, so the tests ask for equality: ranks,
indices, counts and hits as integers, the list values and the average precision bit for bit (AP = ascending sum of
double(i + 1) / double(rank_i), one division by double(P): the model does the same operations in Python floats).

Conventions (those of tests/test_loss_gemm_optim_gpu.py; the helpers are tests/checks.py's): the similarity block sits in a buffer of
pitch ld > n_cols whose padding holds NaN (a kernel that read it would count it); lists, counts and outputs sit in buffers
filled with a NaN bit pattern no kernel produces, two rows longer than needed and with pitches larger than needed (ldp = P_max +
3 unless P_max is the cap, ldh = ldp + 4); after every call the rows >= R, the list and rank slots >= P, the buckets > P must
still hold it.  Only the Gaussian test has a bound: the ranks there come from fp32 products, each within its gemm_bound b of
float64, so a positive j certainly follows every k with s_k - b_k > s_j + b_j and may follow every k with s_k + b_k >= s_j - b_j.
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import ops  # noqa: E402
from tests import rankeval_reference as M  # noqa: E402
from tests.chains import gemm_bound, gemm_chain  # noqa: E402
from tests.checks import child as _child, is_sent, sent  # noqa: E402
from tests.dataset_support import write_dataset  # noqa: E402
from tests.eval_support import chunks_of, grid_rows, knn_eval_case, unit_gauss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
MAX_POS = 4096
KS = (1, 2, 5, 50, 5000)
I32, F32, F64 = torch.int32, torch.float32, torch.float64


# --------------------------------------------------------------------------------------------------------------- helpers
def sim_buffer(rows, dev, ld4=True, misalign=False):
    """rows [R, n] -> a [R, ld] device view with NaN in the pitch padding; ld a multiple of 4 or not; the view starts on a
    16-byte boundary or one float behind one"""
    R, n = rows.shape
    ld = (n + 7) // 4 * 4 if ld4 else (n + 3) // 4 * 4 + 3
    flat = torch.full((R * ld + 8,), NAN, dtype=F32, device=dev)
    assert flat.data_ptr() % 16 == 0
    off = 1 if misalign else 0
    buf = flat[off:off + R * ld].view(R, ld)
    buf[:, :n] = rows.to(dev)
    assert (buf.data_ptr() % 16 == 0) != misalign and (ld % 4 == 0) == ld4 and ld > n
    return buf


class State:
    """lists, counts and outputs of a chain over R rows inside sentinel buffers; P [R]: the model's number of positives per row"""

    def __init__(self, R, P, dev, ks=KS, ldp=None):
        self.R, self.ks, self.dev = R, list(ks), dev
        self.P = torch.as_tensor(np.asarray(P), dtype=torch.int64, device=dev)
        pm = max(int(self.P.max()), 1)
        self.ldp = ldp if ldp is not None else (pm if pm + 3 > MAX_POS else pm + 3)
        self.ldh = self.ldp + 4
        self.val, self.idx, self.rank = sent((R + 2, self.ldp), dev), sent((R + 2, self.ldp), dev, I32), sent((R + 2, self.ldp), dev, I32)
        self.hist = sent((R + 2, self.ldh), dev, I32)
        self.cnt, self.first_rank, self.rhits, self.n_valid = (sent((R + 2,), dev, I32) for _ in range(4))
        self.hits = sent((R + 2, len(self.ks)), dev, I32)
        self.ap = torch.full((R + 2,), 0x7ff8123412341234, dtype=torch.int64, device=dev).view(F64)
        self.ks_d = torch.tensor(self.ks or [1], dtype=I32, device=dev)

    def frame_ok(self):
        R, n = self.R, self.P.clamp(max=self.ldp)[:, None]
        beyond = torch.arange(self.ldp, device=self.dev)[None, :] >= n
        above = torch.arange(self.ldh, device=self.dev)[None, :] > n
        return (all(is_sent(t[R:]) for t in (self.val, self.idx, self.rank, self.hist, self.cnt, self.first_rank, self.rhits, self.n_valid, self.hits))
                and bool((self.ap[R:].view(torch.int64) == 0x7ff8123412341234).all())
                and all(is_sent(t[:R][beyond]) for t in (self.val, self.idx, self.rank)) and is_sent(self.hist[:R][above]))

    def bits(self):
        """everything the chain wrote, as integers"""
        return [t.clone() for t in (self.val.view(I32), self.idx, self.rank, self.hist, self.cnt, self.first_rank, self.rhits,
                                    self.n_valid, self.hits, self.ap.view(torch.int64))]


def run_chain(buf, n, st, row_cls, col_cls, chunks=None, col0=0, exclude=0, diag=0, row_vid=None, col_vid=None):
    """gather over the chunks -> sort -> count over the same chunks -> finish; a chunk (c, m) is the columns [c, c + m) of buf,
    fed with the column ids and the diag of that block.  The frame is checked after every call."""
    R, ld = buf.shape
    chunks = chunks or [(0, n)]

    def ids(t, c):
        return None if t is None else t[c:]
    for t, (c, m) in enumerate(chunks):
        ops.call('dv_rankeval_gather_f32', buf.data_ptr() + 4 * c, ld, R, m, col0 + c, row_cls, col_cls[c:], row_vid, ids(col_vid, c),
                 exclude, diag - c, st.val, st.idx, st.ldp, st.cnt, int(t == 0))
        assert st.frame_ok(), 'gather, chunk %d, wrote outside its ranges' % t
    ops.call('dv_rankeval_sort', st.val, st.idx, st.ldp, st.cnt, R)
    assert st.frame_ok(), 'sort wrote outside its ranges'
    for t, (c, m) in enumerate(chunks):
        ops.call('dv_rankeval_count_f32', buf.data_ptr() + 4 * c, ld, R, m, col0 + c, row_vid, ids(col_vid, c), exclude, diag - c,
                 st.val, st.idx, st.ldp, st.cnt, st.hist, st.ldh, int(t == 0))
        assert st.frame_ok(), 'count, chunk %d, wrote outside its ranges' % t
    ops.call('dv_rankeval_finish', st.hist, st.ldh, st.cnt, st.ldp, R, st.ks_d if st.ks else None, len(st.ks), st.rank, st.ap,
             st.first_rank, st.hits if st.ks else None, st.rhits, st.n_valid)
    assert st.frame_ok(), 'finish wrote outside its ranges'


def check_state(st, m, what):
    """the chain's state equals the model `m` (tests/rankeval_reference.model): integers equal, pos_val and ap bit for bit"""
    R, dev = st.R, st.dev
    pm = m['rank'].shape[1]
    inside = torch.arange(pm, device=dev)[None, :] < st.P[:, None]

    def t(a, dtype=torch.int64):
        return torch.as_tensor(np.asarray(a), dtype=dtype, device=dev)
    assert torch.equal(st.cnt[:R].long(), t(m['pos_cnt'])), what + ': pos_cnt'
    assert torch.equal(st.P, t(m['pos_cnt']))
    for name, got in (('rank', st.rank), ('pos_idx', st.idx)):
        g, w = got[:R, :pm].long()[inside], t(m[name])[inside]
        bad = g != w
        assert not bool(bad.any()), '%s: %s differs in %d places, first got %d want %d' % (what, name, int(bad.sum()), int(g[bad][0]), int(w[bad][0]))
    want_val = t(m['pos_val'], F64)[inside]
    assert bool((want_val.float().double() == want_val).all())
    assert torch.equal(st.val[:R, :pm][inside].view(I32), want_val.float().view(I32)), what + ': pos_val bits'
    for name, got in (('first_rank', st.first_rank), ('rhits', st.rhits), ('n_valid', st.n_valid)):
        assert torch.equal(got[:R].long(), t(m[name])), '%s: %s' % (what, name)
    assert torch.equal(st.hits[:R].long(), t(m['hits']).reshape(R, len(st.ks))), what + ': hits'
    got_ap, want_ap = st.ap[:R].view(torch.int64), t(m['ap'], F64).view(torch.int64)
    bad = got_ap != want_ap
    assert not bool(bad.any()), '%s: ap differs from the model in %d rows, first row %d: got %r want %r' % (
        what, int(bad.sum()), int(bad.nonzero()[0]), float(st.ap[:R][bad][0]), float(t(m['ap'], F64)[bad][0]))


def classes_for(seed, R, n, targets):
    """row r queries class r % len(targets); class c labels exactly targets[c] columns, the other columns are class -7; shuffled"""
    assert sum(targets) <= n
    col = torch.full((n,), -7, dtype=I32)
    at = 0
    for c, p in enumerate(targets):
        col[at:at + p] = c
        at += p
    col = col[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]
    return torch.arange(R, dtype=I32) % len(targets), col


def chain_case(gpu, rows, row_cls, col_cls, what, ld4=True, misalign=False, chunks=None, col0=0, exclude=0, diag=0, row_vid=None,
               col_vid=None, ks=KS):
    """one block through the chain and against the model; -> (the state, the model)"""
    R, n = rows.shape
    m = M.model(rows.numpy(), row_cls.numpy(), col_cls.numpy(), exclude=exclude, diag=diag, row_vid=None if row_vid is None else row_vid.numpy(),
                col_vid=None if col_vid is None else col_vid.numpy(), col0=col0, ks=ks)
    st = State(R, m['pos_cnt'], gpu, ks)

    def dev(t):
        return None if t is None else t.to(gpu)
    run_chain(sim_buffer(rows, gpu, ld4, misalign), n, st, dev(row_cls), dev(col_cls), chunks, col0, exclude, diag, dev(row_vid), dev(col_vid))
    check_state(st, m, what)
    return st, m


# ------------------------------------------------------------------------------------------ 1. the chain, exact with ties
#        (R, n, the classes' sizes P): P in {0, 1, 2, 63, 64, 65, 257, 4096}; (2, 40000): the columns of a row split over workgroups
CHAIN_CASES = [(1, 1, (1,)), (1, 1, (0,)), (3, 7, (0, 1, 2)), (3, 7, (7,)), (5, 300, (0, 1, 2, 63, 64, 65)),
               (67, 1000, (0, 1, 2, 63, 64, 65, 257)), (3, 5000, (4096, 257, 65, 0)), (2, 40000, (257, 65))]
LAYOUTS = [('ld4', True, False), ('ldodd', False, False), ('misaligned', True, True)]


@pytest.mark.parametrize('layout', LAYOUTS, ids=[v[0] for v in LAYOUTS])
@pytest.mark.parametrize('case', CHAIN_CASES, ids=['R%d-n%d-P%s' % (c[0], c[1], '.'.join(str(p) for p in c[2])) for c in CHAIN_CASES])
def test_chain_exact_with_ties(gpu, case, layout):
    (R, n, targets), (name, ld4, misalign) = case, layout
    rows = grid_rows(7000 * R + n + len(targets), R, n)                     # multiples of 1/4 in [-2, 2]: ties abound
    row_cls, col_cls = classes_for(n + R, R, n, targets)
    st, m = chain_case(gpu, rows, row_cls, col_cls, 'chain R=%d n=%d %s' % (R, n, name), ld4, misalign, col0=11)
    assert m['pos_cnt'].tolist() == [targets[r % len(targets)] for r in range(R)]
    if n >= 300:                    # the data has what the case is about: a positive tied with a negative on either side of its index
        key = M.keys(rows.numpy())
        pos = col_cls.numpy()[None, :] == row_cls.numpy()[:, None]
        assert any(((key[r][pos[r]][:, None] == key[r][~pos[r]][None, :]).any()) for r in range(R))


def test_list_overflow_is_counted_not_written(gpu):
    """ldp below the number of positives: pos_cnt still counts them all, nothing is written beyond the pitch (the next row's
    slots and the rows behind keep what they held), and the slots hold some of the row's positives, sorted"""
    R, n, ldp = 4, 300, 8
    rows = grid_rows(31, R, n)
    row_cls, col_cls = classes_for(32, R, n, (40, 3, 70, 8))
    m = M.model(rows.numpy(), row_cls.numpy(), col_cls.numpy())
    st = State(R, np.minimum(m['pos_cnt'], ldp), gpu, ks=(), ldp=ldp)
    buf = sim_buffer(rows, gpu)
    ops.call('dv_rankeval_gather_f32', buf, buf.shape[1], R, n, 0, row_cls.to(gpu), col_cls.to(gpu), None, None, 0, 0, st.val, st.idx, ldp,
             st.cnt, 1)
    assert st.frame_ok() and st.cnt[:R].tolist() == [40, 3, 70, 8]
    ops.call('dv_rankeval_sort', st.val, st.idx, ldp, st.cnt, R)
    assert st.frame_ok()
    for r in range(R):
        k = min(int(m['pos_cnt'][r]), ldp)
        got = st.idx[r, :k].tolist()
        assert len(set(got)) == k and set(got) <= set(m['pos_idx'][r].tolist()) - {-1}
        order = [m['pos_idx'][r].tolist().index(j) for j in got]
        assert order == sorted(order), 'row %d is not in the order of the header' % r
    # the rows that fit are the model's lists
    assert st.idx[1, :3].tolist() == m['pos_idx'][1, :3].tolist() and st.idx[3, :8].tolist() == m['pos_idx'][3, :8].tolist()


# -------------------------------------------------------------------------------------------------- 2. adversarial rows
def adversarial(n):
    gen = torch.Generator().manual_seed(5)
    asc = torch.arange(n, dtype=F32) / 8 - 150                              # strictly ascending: the last column ranks first
    rnd = (torch.rand(n, generator=gen) < 0.1).int()                        # about one column in ten is a positive
    head, tail = torch.zeros(n, dtype=I32), torch.zeros(n, dtype=I32)
    head[:300], tail[-300:] = 1, 1
    mixed = grid_rows(77, 1, n)[0]
    mixed[[3, 64, 1000, n - 1]] = NAN
    mixed[[0, 65, 2000]] = -INF
    mixed[[5, 2049]] = INF
    mixed[[7, 63, 128, 129, 2500]] = -0.0
    mixed[[8, 200]] = 0.0
    special = rnd.clone()
    special[[3, 1000, 0, 2000, 5, 7, 128, 8]] = 1                           # a positive of every special kind ...
    special[[64, n - 1, 65, 2049, 63, 129, 2500, 200]] = 0                  # ... and a negative
    return {'constant': (torch.full((n,), 0.25), rnd), 'ascending': (asc, rnd), 'descending': (asc.flip(0), rnd),
            'positives_first': (asc.flip(0), head), 'positives_last': (asc.flip(0), tail), 'positives_first_ascending': (asc, head),
            'specials': (mixed, special)}


@pytest.mark.parametrize('kind', ['constant', 'ascending', 'descending', 'positives_first', 'positives_last',
                                  'positives_first_ascending', 'specials'])
def test_chain_adversarial_rows(gpu, kind):
    n = 3000
    row, cls = adversarial(n)[kind]
    st, m = chain_case(gpu, row[None, :], torch.ones(1, dtype=I32), cls, 'adversarial ' + kind, col0=7)
    P = int(m['pos_cnt'][0])
    if kind == 'constant':          # all equal: the index alone decides, a positive's rank is its column + 1
        assert m['rank'][0, :P].tolist() == [j - 7 + 1 for j in m['pos_idx'][0, :P].tolist()]
    if kind == 'positives_first':
        assert m['ap'][0] == 1.0 and m['rank'][0, :P].tolist() == list(range(1, 301))
    if kind in ('positives_last', 'positives_first_ascending'):
        assert m['rank'][0, :P].tolist() == list(range(n - 299, n + 1)) and m['first_rank'][0] == n - 299
    if kind == 'specials':          # +inf first, the NaN / -inf positives last and by index, -0.0 among the zeros
        assert m['pos_idx'][0, 0] == 7 + 5 and m['pos_val'][0, 0] == INF and m['rank'][0, 0] == 1 and m['rank'][0, 1] > 2
        last = m['pos_idx'][0, P - 4:P].tolist()
        assert last == [7 + 0, 7 + 3, 7 + 1000, 7 + 2000] and m['n_valid'][0] == n and m['rank'][0, P - 1] <= n


# ----------------------------------------------------------------------------------------------- 3. chunking is invisible
def test_chunking_is_invisible(gpu):
    R, N = 5, 5000
    rows = grid_rows(4242, R, N)
    row_cls, col_cls = torch.arange(R, dtype=I32), torch.randint(0, 10, (N,), generator=torch.Generator().manual_seed(1), dtype=I32)
    single, m = chain_case(gpu, rows, row_cls, col_cls, 'single call')
    want = single.bits()
    again, _ = chain_case(gpu, rows, row_cls, col_cls, 'second identical run')
    assert all(torch.equal(a, b) for a, b in zip(again.bits(), want)), 'a second run gives other bits'
    for size, desc in ((1000, False), (257, False), (64, False), (257, True)):
        what = 'chunks of %d %s' % (size, 'descending' if desc else 'ascending')
        st, _ = chain_case(gpu, rows, row_cls, col_cls, what, chunks=chunks_of(N, size, desc))
        assert all(torch.equal(a, b) for a, b in zip(st.bits(), want)), what
    n1 = 300                                                                # one column per call: 600 launches
    whole, _ = chain_case(gpu, rows[:, :n1], row_cls, col_cls[:n1], 'single call n=300')
    one, _ = chain_case(gpu, rows[:, :n1], row_cls, col_cls[:n1], 'chunks of 1', chunks=chunks_of(n1, 1))
    assert all(torch.equal(a, b) for a, b in zip(one.bits(), whole.bits()))


# --------------------------------------------------------------------------------------------------------- 4. exclusion
def test_exclusion_modes(gpu):
    """130 clips in videos of 4 (the last one has 2), the classes 0..7 by video and class 9 for the last video alone: in mode 2
    its clips have no positive left"""
    n = 130
    g = grid_rows(99, n, n)
    sim = ((g + g.t()) / 2).contiguous()                                    # symmetric, multiples of 1/8
    vid = (torch.arange(n) // 4).int()
    cls = (vid % 8).int()
    cls[128:] = 9
    for exclude in (0, 1, 2):
        st, m = chain_case(gpu, sim, cls, cls, 'symmetric block, exclude=%d' % exclude, exclude=exclude, row_vid=vid, col_vid=vid)
        assert m['n_valid'].tolist() == [n - (0, 1, 4)[exclude]] * 128 + [n - (0, 1, 2)[exclude]] * 2
        assert m['pos_cnt'][128:].tolist() == [(2, 1, 0)[exclude]] * 2
        if exclude == 2:
            assert m['ap'][128:].tolist() == [-1.0, -1.0] and m['first_rank'][128:].tolist() == [0, 0]
            assert not bool((torch.as_tensor(m['pos_idx'][:128]) // 4 == torch.arange(128)[:, None] // 4).any())
    # an off-diagonal block of the same problem: rows 20..49 against the columns 10..129 in two chunks, so row r meets itself in
    # column r + 10 of the block
    rows, cols = slice(20, 50), slice(10, 130)
    for diag, chunks in ((10, None), (10, [(0, 37), (37, 83)]), (10, [(64, 56), (0, 64)])):
        st, m = chain_case(gpu, sim[rows, cols].contiguous(), cls[rows], cls[cols], 'off-diagonal block diag=%d' % diag, exclude=1, diag=diag,
                           col0=10, chunks=chunks, ld4=False)
        assert m['n_valid'].tolist() == [119] * 30
        assert not bool((torch.as_tensor(m['pos_idx']) == torch.arange(20, 50)[:, None]).any())
    for diag in (1000, -1000, 120, -30):                                    # nobody's column: the same as exclude = 0
        st, m = chain_case(gpu, sim[rows, cols].contiguous(), cls[rows], cls[cols], 'diag=%d' % diag, exclude=1, diag=diag, col0=10)
        assert m['n_valid'].tolist() == [120] * 30
    # exclude = 0 and 1 never read the video ids: null pointers are accepted
    chain_case(gpu, sim, cls, cls, 'exclude=1 without video ids', exclude=1)


# -------------------------------------------------------------------------------- 5. positive_ranks end to end, exact
def state_model(q64, b64, q_cls, b_cls, ks, exclude=0, q_vid=None, b_vid=None):
    return M.model((q64 @ b64.t()).numpy(), q_cls.numpy(), b_cls.numpy(), exclude=exclude, diag=0, row_vid=None if q_vid is None else q_vid.numpy(),
                   col_vid=None if b_vid is None else b_vid.numpy(), ks=ks)


def check_result(res, m, what):
    """positive_ranks' dict equals the model: rank is 0 and pos_idx -1 beyond pos_cnt there as here"""
    dev = res['rank'].device
    pm = m['rank'].shape[1]
    assert res['rank'].shape == res['pos_idx'].shape == (m['rank'].shape[0], pm), what
    for name in ('rank', 'pos_idx', 'pos_cnt', 'first_rank', 'hits', 'rhits', 'n_valid'):
        assert res[name].dtype == I32 and torch.equal(res[name].long(), torch.as_tensor(m[name], device=dev).reshape(res[name].shape)), '%s: %s' % (what, name)
    assert res['ap'].dtype == F64 and torch.equal(res['ap'].view(torch.int64), torch.as_tensor(m['ap'], device=dev).view(torch.int64)), what + ': ap bits'


@pytest.mark.parametrize('R,N,C', [(5, 300, 4), (130, 1000, 10)])
def test_positive_ranks_grid_exact(gpu, R, N, C):
    """features are multiples of 1/4 in [-2, 2], D = 128: every dot product is a multiple of 1/16 below 512, exact in fp32 in any
    order, so every blocking equals float64 exactly, ties included"""
    from dualvar_amd.utils import knn, rankeval
    D, ks = 128, (1, 5, 10, 20, 50)
    q64, b64 = grid_rows(R + N, R, D).double(), grid_rows(R * N + 1, N, D).double()
    assert float((q64.abs() @ b64.abs().t()).max()) < 512
    gen = torch.Generator().manual_seed(R)
    q_cls, b_cls = torch.randint(0, C, (R,), generator=gen), torch.randint(0, C, (N,), generator=gen)
    m = state_model(q64, b64, q_cls, b_cls, ks)
    q, b = q64.float().to(gpu), b64.float().to(gpu)
    for chunk in (64, 257, N):
        for row_block in (1, 64, R):
            res = rankeval.positive_ranks(q, b, q_cls, b_cls, ks=ks, chunk=chunk, row_block=row_block)
            check_result(res, m, 'positive_ranks R=%d N=%d chunk=%d row_block=%d' % (R, N, chunk, row_block))
    # hits(k) = the same-label entries among the first k neighbours of the tested selection
    val, idx = knn.topk_neighbours(q, b, 50)
    same = b_cls.to(gpu)[idx.long()] == q_cls.to(gpu)[:, None]
    for col, k in enumerate(ks):
        assert torch.equal(res['hits'][:, col].long(), same[:, :k].sum(1)), 'hits(%d) against topk_neighbours' % k
    # the other exclusions through the host module: the bank against itself
    vid = torch.arange(N) // 7
    for exclude, kw in (('self', {}), ('video', dict(q_vid=vid, b_vid=vid))):
        ms = state_model(b64[:R * 2], b64[:R * 2], b_cls[:R * 2], b_cls[:R * 2], ks, EX[exclude], vid[:R * 2], vid[:R * 2])
        rs = rankeval.positive_ranks(b[:R * 2], b[:R * 2], b_cls[:R * 2], b_cls[:R * 2], ks=ks, exclude=exclude, chunk=64, row_block=3,
                                     **{k: v[:R * 2] for k, v in kw.items()})
        check_result(rs, ms, 'positive_ranks exclude=%s' % exclude)


EX = {'none': 0, 'self': 1, 'video': 2}


def test_positive_ranks_never_allocates_the_matrix(gpu):
    """(3, 5000) with chunk = 64: the peak stays below R * N floats; the result is still the model's"""
    from dualvar_amd.utils import features, rankeval
    R, N, D, C, ks = 3, 5000, 128, 50, (1, 5, 10, 20, 50)
    q64, b64 = grid_rows(R + N, R, D).double(), grid_rows(R * N + 1, N, D).double()
    gen = torch.Generator().manual_seed(R)
    q_cls, b_cls = torch.randint(0, C, (R,), generator=gen), torch.randint(0, C, (N,), generator=gen)
    q, b = q64.float().to(gpu), b64.float().to(gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = rankeval.positive_ranks(q, b, q_cls, b_cls, ks=ks, chunk=64)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < R * N * 4 and grown <= features.WORKSPACE_BYTES, grown   # a [3, 64] workspace, the lists and the labels
    check_result(res, state_model(q64, b64, q_cls, b_cls, ks), 'positive_ranks R=3 N=5000 chunk=64')


# -------------------------------------------------------------------- 6. positive_ranks, Gaussian features, interval check
def test_positive_ranks_gaussian_interval(gpu):
    from dualvar_amd.utils import features, rankeval
    R, N, D, C = 130, 5000, 512, 10
    gen = torch.Generator().manual_seed(11)
    q, b = unit_gauss(gen, R, D).to(gpu), unit_gauss(gen, N, D).to(gpu)
    q_cls, b_cls = torch.randint(0, C, (R,), generator=gen), torch.randint(0, C, (N,), generator=gen)
    s64 = q.double() @ b.double().t()
    bound = gemm_bound(q.double(), b.double(), 1.0, gemm_chain(R, N, D))     # the defaults form one [R, N] product here
    assert features.blocks(R, N) == (R, N)
    res = rankeval.positive_ranks(q, b, q_cls, b_cls, ks=(1, 5))
    P = res['pos_cnt'].long()
    assert torch.equal(P, (b_cls.to(gpu)[None, :] == q_cls.to(gpu)[:, None]).sum(1)) and int(P.min()) > 0
    assert bool((res['n_valid'] == N).all())
    inside = torch.arange(res['rank'].shape[1], device=gpu)[None, :] < P[:, None]
    pi = res['pos_idx'].long().clamp(min=0)
    assert bool((b_cls.to(gpu)[pi] == q_cls.to(gpu)[:, None])[inside].all()), 'a listed item is not a positive'
    assert all(len(set(row[:p])) == p for row, p in zip(res['pos_idx'].tolist(), P.tolist())), 'a positive is listed twice'
    lo_sorted, hi_sorted = (s64 - bound).sort(1).values, (s64 + bound).sort(1).values
    v_lo, v_hi = (s64 - bound).gather(1, pi), (s64 + bound).gather(1, pi)
    least = 1 + N - torch.searchsorted(lo_sorted, v_hi.contiguous(), right=True)          # 1 + #{k : s_k - b_k > s_j + b_j}
    most = N - torch.searchsorted(hi_sorted, v_lo.contiguous(), right=False)              # #{k : s_k + b_k >= s_j - b_j}, j among them
    rank = res['rank'].long()
    ok = (rank >= least) & (rank <= most)
    assert bool(ok[inside].all()), '%d of %d ranks lie outside their interval' % (int((~ok)[inside].sum()), int(inside.sum()))
    width = (most - least)[inside]
    print('    gaussian ranks: %d positives, interval width mean %.2f max %d' % (int(inside.sum()), float(width.float().mean()), int(width.max())))
    d = rank[:, 1:] - rank[:, :-1]
    assert bool((d > 0)[inside[:, 1:]].all()), 'the ranks of a row do not ascend strictly'


# ------------------------------------------------------------------------- 7. ranking_eval against the tested retrieval path
def test_ranking_eval_against_retrieval(gpu):
    from dualvar_amd.utils import features, rankeval
    from dualvar_amd.utils.retrieval import nn_retrieval
    te, tel, tr, trl, C, _, _ = knn_eval_case(gpu)
    ks = (1, 5, 10, 20, 50)
    assert features.blocks(te.shape[0], tr.shape[0]) == (te.shape[0], tr.shape[0])      # one product, the one nn_retrieval forms
    acc, sim = nn_retrieval(te, tel, tr, trl, ks=ks)
    m = M.model(sim.cpu().numpy(), tel.numpy(), trl.numpy(), ks=ks)
    rep, state = rankeval.ranking_eval(te, tel, tr, trl, C, ks=ks)
    check_result(state, m, 'ranking_eval')
    # data: no row has a negative exactly tied with its best positive, so "a positive among the first k" does not depend on the
    # tie rule and success_at is nn_retrieval's accuracy
    s = sim.cpu().double()
    same = trl[None, :] == tel[:, None]
    best = torch.where(same, s, torch.full_like(s, -INF)).max(1).values
    assert not bool(((s == best[:, None]) & ~same).any()), 'a negative ties with the best positive of a row: take another seed'
    for k in ks:                    # nn_retrieval's accuracy is an fp32 mean: the same count of rows
        assert round(rep['success_at'][k] * 130) == round(acc[k] * 130) and abs(rep['success_at'][k] - acc[k]) < 1e-6, (k, rep['success_at'], acc)
    assert rep['n_query'] == 130 and rep['n_skipped'] == 0 and rep['n_bank'] == 1000
    ap = [float(v) for v in m['ap']]
    assert rep['mAP'] == math.fsum(ap) / 130 and 0.0 < rep['mAP'] < 1.0
    assert rep['MRR'] == math.fsum(1.0 / int(f) for f in m['first_rank']) / 130
    assert rep['R_precision'] == math.fsum(int(h) / int(p) for h, p in zip(m['rhits'], m['pos_cnt'])) / 130
    assert len(rep['per_class_AP']) == C and all(v is not None for v in rep['per_class_AP']) and 0.0 < rep['mAP_macro'] < 1.0
    json.dumps(rep)


# ----------------------------------------------------------------------------- 8. ranking_eval_within, known by construction
def mirrored(videos, labels, S, gpu):
    """videos [V, S, D] -> every video followed by its negation under a label of its own (so that the column mean is zero and
    centring leaves the directions as they are; a mirror's clips rank last for everyone else)"""
    both = torch.cat([videos, -videos])
    lab = torch.cat([labels, labels + int(labels.max()) + 1])
    return both.to(gpu), lab


def test_ranking_eval_within_by_construction(gpu):
    from dualvar_amd.utils import rankeval
    S, D = 4, 16
    e = torch.eye(D)
    # (a) three classes of three videos, every clip of a class the same vector: a clip's valid neighbours are the clips of the
    # other two videos of its class (similarity 1), then everything else
    vids = torch.stack([e[c].expand(S, D) for c in (0, 0, 0, 1, 1, 1, 2, 2, 2)])
    per, lab = mirrored(vids, torch.tensor([0, 0, 0, 1, 1, 1, 2, 2, 2]), S, gpu)
    rep, state = rankeval.ranking_eval_within(per, lab, 6, ks=(1, 8, 9))
    assert state['pos_cnt'].tolist() == [2 * S] * (18 * S) and state['n_valid'].tolist() == [17 * S] * (18 * S)
    assert state['ap'].tolist() == [1.0] * (18 * S) and state['rank'][:, :2 * S].tolist() == [list(range(1, 2 * S + 1))] * (18 * S)
    assert rep['mAP'] == 1.0 and rep['mAP_macro'] == 1.0 and rep['R_precision'] == 1.0 and rep['MRR'] == 1.0
    assert rep['success_at'] == {1: 1.0, 8: 1.0, 9: 1.0} and rep['recall_at'][8] == 1.0 and rep['precision_at'][8] == 1.0
    assert rep['precision_at'][9] == pytest.approx(8 / 9, abs=1e-15) and rep['n_query'] == 18 * S and rep['n_skipped'] == 0
    # (b) class 0: three videos around e0 (cosine 0.8 to each other); video X of class 1 holds ONE clip at their centroid (cosine
    # 0.93 to each of them), its other clips and the videos of class 2 lie elsewhere: for every clip of class 0 the intruder is
    # first, then its 2 S positives at the ranks 2 .. 2 S + 1
    a = [e[0] + 0.5 * e[i] for i in (1, 2, 3)]
    x = torch.stack([e[0] + (e[1] + e[2] + e[3]) / 6] + [e[5]] * (S - 1))
    vids = torch.stack([v.expand(S, D) for v in a] + [x] + [e[6].expand(S, D), e[7].expand(S, D)])
    per, lab = mirrored(vids, torch.tensor([0, 0, 0, 1, 2, 2]), S, gpu)
    rep, state = rankeval.ranking_eval_within(per, lab, 6, ks=(1, 2))
    P = 2 * S
    closed = 0.0
    for i in range(P):
        closed += float(i + 1) / float(i + 2)
    closed /= float(P)
    rows = slice(0, 3 * S)                                                  # the clips of class 0
    assert state['pos_cnt'][rows].tolist() == [P] * (3 * S) and state['first_rank'][rows].tolist() == [2] * (3 * S)
    assert state['rank'][rows, :P].tolist() == [list(range(2, P + 2))] * (3 * S)
    assert state['ap'][rows].tolist() == [closed] * (3 * S)
    assert rep['per_class_AP'][0] == pytest.approx(closed, abs=1e-15) and state['hits'][rows].tolist() == [[0, 1]] * (3 * S)
    assert state['rhits'][rows].tolist() == [P - 1] * (3 * S)


# --------------------------------------------------------------------------------------------------- 9. the driver, one child
def test_cli_retrieval_with_map(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp('map_cli')
    split, frame = write_dataset(str(d / 'data'), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
    os.makedirs(str(d / 'run' / 'model'))
    argv = [os.path.join(ROOT, 'classifier.py'), '--test', str(d / 'run' / 'model' / 'none.pth.tar'), '--retrieval', '--num_seq', '10',
            '--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
            '--split_root', split, '--frame_root', frame, '--map', '--map_level', 'both', '--map_within']
    out = _child(argv, str(d), 600)
    nn = [float(v) for v in re.findall(r'\t\d+NN acc = ([0-9.]+)', out)]
    assert len(nn) == 5, out[-2000:]
    fdir = str(d / 'run' / 'model' / 'feature')
    with open(os.path.join(fdir, 'ucf101_map.json')) as fp:
        rep = json.load(fp)
    t = torch.load(os.path.join(fdir, 'ucf101_map.pth.tar'), map_location='cpu', weights_only=True)
    assert set(rep) == set(t) == {'video', 'clip', 'within'}
    assert ['%.4f' % rep['video']['success_at'][k] for k in ('1', '5', '10', '20', '50')] == ['%.4f' % v for v in nn], (rep['video'], nn)
    n_test = rep['video']['n_query']
    assert rep['video']['n_bank'] * 10 == rep['clip']['n_bank'] and rep['clip']['n_query'] == rep['within']['n_query'] == 10 * n_test
    for level, n in (('video', n_test), ('clip', 10 * n_test), ('within', 10 * n_test)):
        assert set(t[level]) == {'ap', 'pos_cnt', 'first_rank'}
        assert t[level]['ap'].shape == (n,) and t[level]['ap'].dtype == F64 and not t[level]['ap'].is_cuda
        used = t[level]['pos_cnt'] > 0
        assert bool(((t[level]['ap'][used] > 0) & (t[level]['ap'][used] <= 1)).all()) and bool((t[level]['ap'][~used] == -1).all())
        assert rep[level]['n_skipped'] == int((~used).sum())
        if rep[level]['mAP'] is not None:
            assert rep[level]['mAP'] == pytest.approx(float(t[level]['ap'][used].mean()), abs=1e-12)
    assert len(re.findall(r'Ranking report on ucf101, (video|clip|within) level', out)) == 3
    assert len(re.findall(r'\tmAP = \S+ macro mAP = \S+ MRR = \S+ R-precision = \S+', out)) == 3
    assert len(re.findall(r'\tP@\d+ = \S+ recall@\d+ = \S+', out)) == 15
