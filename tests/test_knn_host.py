"""CPU: the two k-NN entries (dv_topk_merge_f32, dv_knn_vote) refuse every bad argument of their header comments before any
launch (include/dualvar_select.h), the header, its ctypes table and the library agree, classifier.py parses and checks --knn / --knn_k / --knn_t, and utils/knn.py refuses k > DV_TOPK_MAX_K before it asks
for the device."""
import math
import os
import re
import shlex
import subprocess
import sys

import pytest

from tests import abi_coverage as A
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
X = 4096                 # stands for a non-null pointer: a refused call never dereferences it
INT32_MAX = 2 ** 31 - 1

# dv_topk_merge_f32(sim, ld, R, n_cols, col0, k, top_val, top_idx, ldk, first, stream)
TOPK_OK = dict(sim=X, ld=70, R=3, n_cols=64, col0=0, k=5, top_val=X, top_idx=X, ldk=5, first=1)
TOPK_BAD = [dict(sim=None), dict(top_val=None), dict(top_idx=None), dict(R=0), dict(R=-1), dict(n_cols=0), dict(n_cols=-3),
            dict(n_cols=INT32_MAX - 511, ld=INT32_MAX), dict(ld=63), dict(k=0), dict(k=-1), dict(k=257, ldk=300), dict(ldk=4), dict(col0=-1),
            dict(col0=INT32_MAX - 63), dict(col0=INT32_MAX, n_cols=1, ld=1)]
# dv_knn_vote(top_val, top_idx, ldk, R, k, bank_labels, n_bank, n_class, inv_T, score, lds, pred, stream)
VOTE_OK = dict(top_val=X, top_idx=X, ldk=5, R=3, k=5, bank_labels=X, n_bank=10, n_class=4, inv_T=1.0, score=X, lds=4, pred=X)
VOTE_BAD = [dict(top_val=None), dict(top_idx=None), dict(bank_labels=None), dict(score=None), dict(pred=None), dict(R=0), dict(R=-2),
            dict(k=0), dict(k=257, ldk=300), dict(ldk=4), dict(n_bank=0), dict(n_bank=-1), dict(n_class=0), dict(n_class=4097, lds=5000),
            dict(lds=3), dict(inv_T=-1.0), dict(inv_T=-1e-30), dict(inv_T=math.inf), dict(inv_T=-math.inf), dict(inv_T=math.nan)]


# The coverage ledger of include/dualvar_select.h, in the form and with the kinds of tests/abi_coverage.py (which lists
# _lib.SIGNATURES): every entry of _lib.SELECT_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
# test_select_header_table_and_library_agree keeps the keys equal to the table, so a new entry has to say here how it is tested.
SELECT_COVERAGE = {
    'dv_topk_merge_f32': ('test_knn_gpu.py', A.FLOAT64),
    'dv_knn_vote': ('test_knn_gpu.py', A.FLOAT64),
}


def test_select_header_table_and_library_agree():
    """include/dualvar_select.h, its ctypes table _lib.SELECT_SIGNATURES and the library's exports name the same entries with the
    same argument counts and types (tests/util.py check_header_binding, as for every header; tests/test_abi_and_host.py keeps
    the tables disjoint), and every entry here is called by the float64 tests of tests/test_knn_gpu.py"""
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_select.h')
    assert set(decl) == set(_lib.SELECT_SIGNATURES) == set(SELECT_COVERAGE)
    assert int(re.search(r'#define\s+DV_TOPK_MAX_K\s+(\d+)', hdr).group(1)) == _lib.DV_TOPK_MAX_K == 256
    assert 'select.hip' in build.SOURCES
    for name, (fname, kind) in SELECT_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"ops\.call\('%s'" % name, open(os.path.join(ROOT, 'tests', fname)).read()), '%s is not called by tests/%s' % (name, fname)


@pytest.mark.parametrize('bad', TOPK_BAD, ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_topk_merge_refuses_without_gpu(bad):
    """each refused argument of the header comment returns DV_EINVAL before anything is launched: safe on a CPU-only host"""
    from dualvar_amd import _lib
    a = dict(TOPK_OK, **bad)
    assert _lib.load().dv_topk_merge_f32(*[a[n] for n in TOPK_OK], None) == EINVAL


@pytest.mark.parametrize('bad', VOTE_BAD, ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_knn_vote_refuses_without_gpu(bad):
    from dualvar_amd import _lib
    a = dict(VOTE_OK, **bad)
    assert _lib.load().dv_knn_vote(*[a[n] for n in VOTE_OK], None) == EINVAL


RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_knn_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --knn --knn_k 50 --knn_t 0.1'))
    assert a.knn is True and a.knn_k == 50 and a.knn_t == 0.1
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.knn is False and d.knn_k == 200 and d.knn_t == 0.07
    CLI.check_args(d, environ={})
    CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ' --knn --knn_k 256')), environ={})
    CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ' --knn --knn_k 1')), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --knn', '--knn'),                                            # --knn without --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --knn', '--knn'),
    (RETRIEVAL + ' --knn --knn_k 0', '--knn_k'),
    (RETRIEVAL + ' --knn --knn_k 257', '--knn_k'),
    (RETRIEVAL + ' --knn --knn_t 0', '--knn_t'),
    (RETRIEVAL + ' --knn --knn_t -0.07', '--knn_t'),
])
def test_knn_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))


def test_topk_neighbours_refuses_a_large_k_before_the_device(monkeypatch):
    import torch
    from dualvar_amd import _lib
    from dualvar_amd.utils import knn

    def no_device():
        raise AssertionError('the device was asked for before k was checked')
    monkeypatch.setattr(_lib, 'require_device', no_device)
    monkeypatch.setattr(_lib, 'load', no_device)
    q, b = torch.zeros(2, 8), torch.zeros(300, 8)
    for k in (257, 1000, 0, -1):
        with pytest.raises(ValueError, match='DV_TOPK_MAX_K'):
            knn.topk_neighbours(q, b, k)
    with pytest.raises(ValueError, match='DV_TOPK_MAX_K'):
        knn.knn_classify(torch.zeros(2, 300), torch.zeros(2, 300, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 3)
    # host tensors are refused too (their pointers would reach the kernels as they are), before the device is asked for
    with pytest.raises(ValueError, match='device tensors'):
        knn.topk_neighbours(q, b, 5)
    with pytest.raises(ValueError, match='device tensors'):
        knn.knn_classify(torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 3)
