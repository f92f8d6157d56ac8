"""CPU: the four ranking entries (dv_rankeval_gather_f32, dv_rankeval_sort, dv_rankeval_count_f32, dv_rankeval_finish) refuse every
bad argument of their header comments before any launch (include/dualvar_rankeval.h); the header, its ctypes table and the
library agree; the float64 model of tests/rankeval_reference.py gives the ranks worked out by hand here, and its streaming route
(sorted positives, binary search, histogram, prefix sum) equals its brute-force sort for any chunking; ranking_report
(dualvar_amd/utils/rankeval.py, pure host float64) gives the figures worked out by hand; classifier.py parses and checks --map /
--map_k / --map_level / --map_within in a child process that never opens a GPU; positive_ranks refuses a class beyond
DV_RANKEVAL_MAX_POS before it asks for the device."""
import math
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import abi_coverage as A
from tests import rankeval_reference as M
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it
INT32_MAX = 2 ** 31 - 1
INF, NAN = math.inf, math.nan

# dv_rankeval_gather_f32(sim, ld, R, n_cols, col0, row_cls, col_cls, row_vid, col_vid, exclude, diag, pos_val, pos_idx, ldp,
#                        pos_cnt, first, stream)
GATHER_OK = dict(sim=X, ld=70, R=3, n_cols=64, col0=0, row_cls=X, col_cls=X, row_vid=X, col_vid=X, exclude=0, diag=0, pos_val=X,
                 pos_idx=X, ldp=8, pos_cnt=X, first=1)
BLOCK_BAD = [dict(sim=None), dict(R=0), dict(R=-1), dict(n_cols=0), dict(n_cols=-3), dict(ld=63), dict(ldp=0), dict(ldp=-1),
             dict(ldp=4097), dict(exclude=-1), dict(exclude=3), dict(exclude=2, row_vid=None), dict(exclude=2, col_vid=None),
             dict(col0=-1), dict(col0=INT32_MAX - 62), dict(col0=INT32_MAX, n_cols=1, ld=1)]
GATHER_BAD = BLOCK_BAD + [dict(row_cls=None), dict(col_cls=None), dict(pos_val=None), dict(pos_idx=None), dict(pos_cnt=None)]
# dv_rankeval_sort(pos_val, pos_idx, ldp, pos_cnt, R, stream)
SORT_OK = dict(pos_val=X, pos_idx=X, ldp=8, pos_cnt=X, R=3)
SORT_BAD = [dict(pos_val=None), dict(pos_idx=None), dict(pos_cnt=None), dict(R=0), dict(R=-1), dict(ldp=0), dict(ldp=4097)]
# dv_rankeval_count_f32(sim, ld, R, n_cols, col0, row_vid, col_vid, exclude, diag, pos_val, pos_idx, ldp, pos_cnt, hist, ldh,
#                       first, stream)
COUNT_OK = dict(sim=X, ld=70, R=3, n_cols=64, col0=0, row_vid=X, col_vid=X, exclude=0, diag=0, pos_val=X, pos_idx=X, ldp=8, pos_cnt=X,
                hist=X, ldh=9, first=1)
COUNT_BAD = [dict(b, ldh=4200) if b.get('ldp') == 4097 else b for b in BLOCK_BAD] + [
    dict(pos_val=None), dict(pos_idx=None), dict(pos_cnt=None), dict(hist=None), dict(ldh=8), dict(ldh=0), dict(ldp=4096, ldh=4096)]
# dv_rankeval_finish(hist, ldh, pos_cnt, ldp, R, ks, n_k, rank, ap, first_rank, hits, rhits, n_valid, stream)
FINISH_OK = dict(hist=X, ldh=9, pos_cnt=X, ldp=8, R=3, ks=X, n_k=2, rank=X, ap=X, first_rank=X, hits=X, rhits=X, n_valid=X)
FINISH_BAD = [dict(hist=None), dict(pos_cnt=None), dict(rank=None), dict(ap=None), dict(first_rank=None), dict(rhits=None),
              dict(n_valid=None), dict(ks=None), dict(hits=None), dict(R=0), dict(R=-1), dict(ldp=0), dict(ldp=4097, ldh=4200),
              dict(ldh=8), dict(n_k=-1), dict(n_k=17)]
FINISH_MISALIGNED = [dict(ap=X + 4), dict(ap=X + 1)]
# accepted shapes of the arguments that may be null: no launch follows a refusal, so only "not refused for THIS reason" can be
# shown without a device -- these are exercised on the GPU (tests/test_rankeval_gpu.py)

# The coverage ledger of include/dualvar_rankeval.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.RANKEVAL_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
RANKEVAL_COVERAGE = {
    'dv_rankeval_gather_f32': ('test_rankeval_gpu.py', A.FLOAT64),
    'dv_rankeval_sort': ('test_rankeval_gpu.py', A.FLOAT64),
    'dv_rankeval_count_f32': ('test_rankeval_gpu.py', A.FLOAT64),
    'dv_rankeval_finish': ('test_rankeval_gpu.py', A.FLOAT64),
}


def _ids(d):
    return ','.join('%s=%s' % kv for kv in d.items())


def test_rankeval_header_table_and_library_agree():
    """include/dualvar_rankeval.h, _lib.RANKEVAL_SIGNATURES, the library's exports and RANKEVAL_COVERAGE name the same entries
    with the same argument counts, types and return widths (tests/util.py check_header_binding); the ledger's file calls each"""
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_rankeval.h')
    assert set(decl) == set(_lib.RANKEVAL_SIGNATURES) == set(RANKEVAL_COVERAGE) and len(decl) == 4
    assert int(re.search(r'#define\s+DV_RANKEVAL_MAX_POS\s+(\d+)', hdr).group(1)) == _lib.DV_RANKEVAL_MAX_POS == 4096
    assert 'rankeval.hip' in build.SOURCES
    for name, (fname, kind) in RANKEVAL_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"ops\.call\('%s'" % name, open(os.path.join(ROOT, 'tests', fname)).read()), \
            '%s is not called by tests/%s' % (name, fname)


def _refused(entry, ok, bad):
    from dualvar_amd import _lib
    a = dict(ok, **bad)
    return getattr(_lib.load(), entry)(*[a[n] for n in ok], None)


@pytest.mark.parametrize('bad', GATHER_BAD, ids=_ids)
def test_gather_refuses_without_gpu(bad):
    """each refused argument of the header comment returns DV_EINVAL before anything is launched: safe on a CPU-only host"""
    assert _refused('dv_rankeval_gather_f32', GATHER_OK, bad) == EINVAL


@pytest.mark.parametrize('bad', SORT_BAD, ids=_ids)
def test_sort_refuses_without_gpu(bad):
    assert _refused('dv_rankeval_sort', SORT_OK, bad) == EINVAL


@pytest.mark.parametrize('bad', COUNT_BAD, ids=_ids)
def test_count_refuses_without_gpu(bad):
    assert _refused('dv_rankeval_count_f32', COUNT_OK, bad) == EINVAL


@pytest.mark.parametrize('bad', FINISH_BAD, ids=_ids)
def test_finish_refuses_without_gpu(bad):
    assert _refused('dv_rankeval_finish', FINISH_OK, bad) == EINVAL


@pytest.mark.parametrize('bad', FINISH_MISALIGNED, ids=_ids)
def test_finish_refuses_a_misaligned_ap(bad):
    assert _refused('dv_rankeval_finish', FINISH_OK, bad) == EALIGN


# ------------------------------------------------------------------------------------------------- the model, by hand
def one_row(sims, col_cls, row_cls=1, ks=(), **kw):
    return M.model(np.array([sims], dtype=np.float32), [row_cls], col_cls, ks=ks, **kw)


def test_model_tie_between_a_positive_and_negatives_on_both_sides():
    """0.5 three times, the positive in the middle: the negative of the lower index precedes it, the other one follows"""
    m = one_row([1.0, 0.5, 0.5, 0.5, 0.0], [0, 0, 1, 0, 0], ks=(2, 3))
    assert m['rank'].tolist() == [[3]] and m['pos_idx'].tolist() == [[2]] and m['pos_cnt'].tolist() == [1]
    assert m['ap'][0] == 1.0 / 3.0 and m['first_rank'].tolist() == [3] and m['hits'].tolist() == [[0, 1]]
    assert m['rhits'].tolist() == [0] and m['n_valid'].tolist() == [5]


def test_model_two_equal_positives():
    m = one_row([0.5, 0.5, 1.0, 0.0], [1, 1, 0, 0], ks=(1, 2, 3))
    assert m['rank'].tolist() == [[2, 3]] and m['pos_idx'].tolist() == [[0, 1]]
    assert m['ap'][0] == (1.0 / 2.0 + 2.0 / 3.0) / 2.0 and m['hits'].tolist() == [[0, 1, 2]] and m['rhits'].tolist() == [1]


def test_model_nan_and_minus_inf_positives_rank_last_by_index():
    """NaN counts as -inf; both are valid items behind every finite one, the lower index first"""
    m = one_row([NAN, 0.0, -INF, 1.0, -INF], [1, 0, 1, 0, 0])
    assert m['rank'].tolist() == [[3, 4]] and m['pos_idx'].tolist() == [[0, 2]] and m['n_valid'].tolist() == [5]
    assert m['pos_val'].tolist() == [[-INF, -INF]] and m['ap'][0] == (1.0 / 3.0 + 2.0 / 4.0) / 2.0
    p = one_row([INF, INF, 2.0], [0, 1, 1])                                  # +inf is an ordinary value
    assert p['rank'].tolist() == [[2, 3]] and p['pos_val'].tolist() == [[INF, 2.0]]


def test_model_minus_zero_equals_plus_zero():
    m = one_row([0.0, -0.0, 0.0], [0, 1, 0])
    assert m['rank'].tolist() == [[2]] and not np.signbit(m['pos_val'][0, 0])   # equal keys: the index decides; returned as +0.0
    m = one_row([-0.0, 0.0], [1, 0])
    assert m['rank'].tolist() == [[1]]


def test_model_no_positive_and_only_positives():
    m = one_row([0.5, 0.25, 1.0], [0, 0, 0], ks=(1, 5))
    assert m['pos_cnt'].tolist() == [0] and m['ap'][0] == -1.0 and m['first_rank'].tolist() == [0]
    assert m['hits'].tolist() == [[0, 0]] and m['rhits'].tolist() == [0] and m['n_valid'].tolist() == [3]
    assert m['rank'].shape == (1, 1) and m['rank'].tolist() == [[0]] and m['pos_idx'].tolist() == [[-1]]
    a = one_row([0.5, 0.25, 1.0, 0.25], [1, 1, 1, 1], ks=(1, 2, 9))
    assert a['rank'].tolist() == [[1, 2, 3, 4]] and a['pos_idx'].tolist() == [[2, 0, 1, 3]] and a['ap'][0] == 1.0
    assert a['hits'].tolist() == [[1, 2, 4]] and a['rhits'].tolist() == [4] and a['n_valid'].tolist() == [4]


def test_model_exclusion_modes():
    """two rows of a block whose row r meets itself in column r + 1 (diag = 1); videos of two items"""
    sim = np.array([[0.1, 0.9, 0.8, 0.7, 0.6], [0.5, 0.4, 0.9, 0.3, 0.2]], dtype=np.float32)
    row_cls, col_cls = [1, 1], [1, 1, 1, 0, 1]
    row_vid, col_vid = [10, 11], [12, 10, 11, 11, 10]
    none = M.model(sim, row_cls, col_cls, col0=100)
    assert none['rank'].tolist() == [[1, 2, 4, 5], [1, 2, 3, 5]] and none['n_valid'].tolist() == [5, 5]
    assert none['pos_idx'].tolist() == [[101, 102, 104, 100], [102, 100, 101, 104]]
    own = M.model(sim, row_cls, col_cls, exclude=1, diag=1)                 # row 0 loses column 1, row 1 loses column 2
    assert own['rank'].tolist() == [[1, 3, 4], [1, 2, 4]] and own['n_valid'].tolist() == [4, 4]
    assert own['pos_idx'].tolist() == [[2, 4, 0], [0, 1, 4]]
    assert M.model(sim, row_cls, col_cls, exclude=1, diag=7)['rank'].tolist() == none['rank'].tolist()     # nobody's column
    assert M.model(sim, row_cls, col_cls, exclude=1, diag=-3)['rank'].tolist() == none['rank'].tolist()
    vid = M.model(sim, row_cls, col_cls, exclude=2, row_vid=row_vid, col_vid=col_vid)
    # row 0 (video 10) loses columns 1 and 4; row 1 (video 11) loses columns 2 and 3
    assert vid['pos_idx'].tolist() == [[2, 0, -1], [0, 1, 4]] and vid['rank'].tolist() == [[1, 3, 0], [1, 2, 3]]
    assert vid['n_valid'].tolist() == [3, 3] and vid['ap'][0] == (1.0 / 1.0 + 2.0 / 3.0) / 2.0 and vid['ap'][1] == 1.0
    gone = M.model(sim[:1], [1], col_cls, exclude=2, row_vid=[5], col_vid=[5, 5, 5, 6, 5])      # every positive excluded
    assert gone['pos_cnt'].tolist() == [0] and gone['ap'][0] == -1.0 and gone['n_valid'].tolist() == [1]


def test_model_streaming_identity_equals_the_sort():
    """rank = 1 + prefix sum of the bucket counts, on 300 random rows with ties, NaN, +-inf, -0.0 and random validity; the
    counts do not depend on the chunk size nor on the order of the chunks"""
    rng = np.random.RandomState(20260)
    special = np.array([NAN, INF, -INF, -0.0, 0.0])
    for t in range(300):
        n = int(rng.randint(1, 41))
        sims = rng.randint(-4, 5, n).astype(np.float64) / 4
        odd = rng.rand(n) < 0.2
        sims[odd] = special[rng.randint(0, 5, int(odd.sum()))]
        key, idx = M.keys(sims), np.arange(n) + int(rng.randint(0, 1000))
        valid, positive = rng.rand(n) < 0.85, rng.rand(n) < (0.0, 0.3, 1.0)[t % 3]
        want = M.row_model(key, idx, valid, positive & valid)
        first = None
        for trial in range(3):
            size = (n, int(rng.randint(1, n + 1)), 1)[trial]
            chunks = [(c, min(size, n - c)) for c in range(0, n, size)]
            rng.shuffle(chunks)
            hist, order = M.streaming_hist(key, idx, valid, positive & valid, chunks)
            ranks, n_valid = M.ranks_from_hist(hist)
            assert ranks == want['rank'] and n_valid == want['n_valid'] and idx[order].tolist() == want['pos_idx'], (t, trial)
            first = hist if first is None else first
            assert hist == first, (t, trial)


# ------------------------------------------------------------------------------------------------------- ranking_report
def test_ranking_report_by_hand():
    """four queries of the classes 0, 0, 1, 2; the last one has no positive.  Class 3 has no query at all."""
    from dualvar_amd.utils.rankeval import ranking_report
    state = {'ap': torch.tensor([1.0, 0.5, 0.25, -1.0], dtype=torch.float64), 'pos_cnt': torch.tensor([2, 2, 4, 0], dtype=torch.int32),
             'first_rank': torch.tensor([1, 2, 3, 0], dtype=torch.int32), 'rhits': torch.tensor([2, 1, 1, 0], dtype=torch.int32),
             'hits': torch.tensor([[1, 2], [0, 1], [0, 1], [0, 0]], dtype=torch.int32), 'n_bank': 9}
    rep = ranking_report(state, torch.tensor([0, 0, 1, 2]), 4, (1, 3))
    assert rep['n_query'] == 4 and rep['n_skipped'] == 1 and rep['n_bank'] == 9
    assert rep['mAP'] == pytest.approx(1.75 / 3, abs=1e-15)
    assert rep['per_class_AP'] == [0.75, 0.25, None, None]
    assert rep['mAP_macro'] == pytest.approx(0.5, abs=1e-15) and rep['mAP_macro'] != rep['mAP']
    assert rep['MRR'] == pytest.approx((1 + 1 / 2 + 1 / 3) / 3, abs=1e-15)
    assert rep['R_precision'] == pytest.approx((1 + 0.5 + 0.25) / 3, abs=1e-15)
    assert rep['precision_at'][1] == pytest.approx(1 / 3, abs=1e-15) and rep['precision_at'][3] == pytest.approx((2 / 3 + 1 / 3 + 1 / 3) / 3, abs=1e-15)
    assert rep['recall_at'][1] == pytest.approx(0.5 / 3, abs=1e-15) and rep['recall_at'][3] == pytest.approx((1 + 0.5 + 0.25) / 3, abs=1e-15)
    assert rep['success_at'] == {1: 0.25, 3: 0.75}              # from first_rank, over all four queries: the skipped one fails
    import json
    assert 'NaN' not in json.dumps(rep) and 'Infinity' not in json.dumps(rep)
    # the order of the queries does not move mAP by a bit (math.fsum)
    perm = [2, 3, 0, 1]
    again = ranking_report({k: (v[perm] if torch.is_tensor(v) else v) for k, v in state.items()}, torch.tensor([0, 0, 1, 2])[perm], 4, (1, 3))
    assert again == rep
    empty = ranking_report({k: (v[3:] if torch.is_tensor(v) else v) for k, v in state.items()}, torch.tensor([2]), 4, (1, 3))
    assert empty['mAP'] is None and empty['mAP_macro'] is None and empty['MRR'] is None and empty['n_skipped'] == 1
    assert empty['success_at'] == {1: 0.0, 3: 0.0} and empty['precision_at'] == {1: None, 3: None}
    with pytest.raises(ValueError, match='ranking_report'):
        ranking_report(state, torch.tensor([0, 0, 1]), 4, (1, 3))


def test_positive_ranks_refuses_before_the_device(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import rankeval as RE

    def no_device():
        raise AssertionError('the device was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_device', no_device)
    monkeypatch.setattr(_lib, 'load', no_device)
    q, b = torch.zeros(2, 8), torch.zeros(5000, 8)
    lab = torch.zeros(5000, dtype=torch.int64)
    lab[4500:] = 3                                                          # class 0: 4500 bank items, class 3: 500
    with pytest.raises(ValueError, match=r'class 0 has 4500 positives.*DV_RANKEVAL_MAX_POS'):
        RE.positive_ranks(q, b, torch.tensor([3, 0]), lab)
    with pytest.raises(ValueError, match='device tensors'):                 # 500 positives are fine; host tensors are not
        RE.positive_ranks(q, b, torch.tensor([3, 3]), lab)
    # 'video' removes the query's own video from its class: 4500 - 450 = 4050 fit
    vid = torch.arange(5000) // 450
    with pytest.raises(ValueError, match='device tensors'):
        RE.positive_ranks(q, b, torch.tensor([3, 0]), lab, torch.tensor([11, 0]), vid, exclude='video')
    with pytest.raises(ValueError, match='q_vid and b_vid'):
        RE.positive_ranks(q, b, torch.tensor([3, 0]), lab, exclude='video')
    with pytest.raises(ValueError, match='same set'):
        RE.positive_ranks(q, b, torch.tensor([3, 0]), lab, exclude='self')
    with pytest.raises(ValueError, match='exclude must be'):
        RE.positive_ranks(q, b, torch.tensor([3, 0]), lab, exclude='clip')
    with pytest.raises(ValueError, match=r'query \[R, D\] and bank \[N, D\]'):
        RE.positive_ranks(q, torch.zeros(5000, 9), torch.tensor([3, 0]), lab)
    with pytest.raises(ValueError, match='one integer id per row'):
        RE.positive_ranks(q, b, torch.tensor([3]), lab)
    for ks in ((0,), tuple(range(1, 18))):
        with pytest.raises(ValueError, match='ks takes'):
            RE.positive_ranks(q, b, torch.tensor([3, 3]), lab, ks=ks)
    with pytest.raises(ValueError, match='n_video, num_seq, D'):
        RE.ranking_eval_within(q, torch.tensor([0, 1]), 2)


def test_positives_per_query_on_the_host():
    from dualvar_amd.utils.rankeval import positives_per_query
    q_cls, b_cls = torch.tensor([0, 1, 2, 7]), torch.tensor([0, 0, 1, 1, 1, 2])
    assert positives_per_query(q_cls, b_cls, None, None, 'none').tolist() == [2, 3, 1, 0]
    q_vid, b_vid = torch.tensor([5, 6, 9, 9]), torch.tensor([5, 4, 6, 6, 8, 9])
    assert positives_per_query(q_cls, b_cls, q_vid, b_vid, 'video').tolist() == [1, 1, 0, 0]
    assert positives_per_query(b_cls, b_cls, None, None, 'self').tolist() == [1, 1, 2, 2, 2, 0]


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_map_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --map --map_k 1 3 100 --map_level both --map_within'))
    assert a.map is True and a.map_k == [1, 3, 100] and a.map_level == 'both' and a.map_within is True
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.map is False and d.map_k == [1, 5, 10, 20, 50] and d.map_level == 'video' and d.map_within is False
    CLI.check_args(d, environ={})
    for ok in (' --map', ' --map --map_level clip', ' --map --map_k ' + ' '.join(str(k) for k in range(1, 17)), ' --map --knn --variance'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --map', '--map'),                                            # --map alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --map', '--map'),
    (RETRIEVAL + ' --map --map_k 0', '--map_k'),
    (RETRIEVAL + ' --map --map_k ' + ' '.join(str(k) for k in range(1, 18)), '--map_k'),
    (RETRIEVAL + ' --map_within', '--map_within'),
    (RETRIEVAL + ' --map_level clip', '--map_level'),
])
def test_map_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))
