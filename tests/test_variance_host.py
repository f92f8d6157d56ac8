"""CPU: the pair-statistics entries (dv_pairstat_workspace, dv_pairstat_accum_f32) refuse every bad argument of their header
comment before any launch (include/dualvar_pairstat.h); the header, its ctypes table and the library agree; report_from_state
(dualvar_amd/utils/variance.py, pure host float64) gives the figures worked out by hand here; classifier.py parses and checks
--variance / --var_bins / --var_t in a child process that never opens a GPU."""
import math
import os
import re
import shlex
import subprocess
import sys

import pytest
import torch

from tests import abi_coverage as A
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it
INF = math.inf

# dv_pairstat_accum_f32(sim, ld, R, n_cols, row_vid, row_cls, col_vid, col_cls, diag, mult, t, bins, sums, ext, hist, ldh,
#                       workspace, first, stream)
ACCUM_OK = dict(sim=X, ld=70, R=3, n_cols=64, row_vid=X, row_cls=X, col_vid=X, col_cls=X, diag=0, mult=1, t=2.0, bins=64, sums=X,
                ext=X, hist=X, ldh=65, workspace=X, first=1)
ACCUM_BAD = [dict(sim=None), dict(row_vid=None), dict(row_cls=None), dict(col_vid=None), dict(col_cls=None), dict(sums=None),
             dict(ext=None), dict(hist=None), dict(workspace=None), dict(R=0), dict(R=-1), dict(n_cols=0), dict(n_cols=-3), dict(ld=63),
             dict(bins=0), dict(bins=-1), dict(bins=257, ldh=300), dict(ldh=64), dict(bins=256, ldh=256), dict(mult=0), dict(mult=3),
             dict(mult=-1), dict(t=-1.0), dict(t=-1e-30), dict(t=INF), dict(t=-INF), dict(t=math.nan),
             dict(R=65536, n_cols=65536, ld=65536),                        # 2^32 pairs: one more than a call carries
             dict(R=2 ** 31 - 1, n_cols=3, ld=3)]
ACCUM_MISALIGNED = [dict(sums=X + 4), dict(hist=X + 4), dict(workspace=X + 2)]

# The coverage ledger of include/dualvar_pairstat.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.PAIRSTAT_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
PAIRSTAT_COVERAGE = {
    'dv_pairstat_workspace': ('test_variance_gpu.py', A.HOST_QUERY),
    'dv_pairstat_accum_f32': ('test_variance_gpu.py', A.FLOAT64),
}


def test_pairstat_header_table_and_library_agree():
    """include/dualvar_pairstat.h, _lib.PAIRSTAT_SIGNATURES, the library's exports and PAIRSTAT_COVERAGE name the same entries with
    the same argument counts, types and return widths (tests/util.py check_header_binding); the ledger's files call each entry"""
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_pairstat.h')
    assert set(decl) == set(_lib.PAIRSTAT_SIGNATURES) == set(PAIRSTAT_COVERAGE) == {'dv_pairstat_workspace', 'dv_pairstat_accum_f32'}
    assert int(re.search(r'#define\s+DV_PAIRSTAT_MAX_BINS\s+(\d+)', hdr).group(1)) == _lib.DV_PAIRSTAT_MAX_BINS == 256
    assert 'pairstat.hip' in build.SOURCES
    for name, (fname, kind) in PAIRSTAT_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"ops\.call\('%s'|lib\.%s\(" % (name, name), open(os.path.join(ROOT, 'tests', fname)).read()), \
            '%s is not called by tests/%s' % (name, fname)


@pytest.mark.parametrize('bad', ACCUM_BAD, ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_pairstat_accum_refuses_without_gpu(bad):
    """each refused argument of the header comment returns DV_EINVAL before anything is launched: safe on a CPU-only host"""
    from dualvar_amd import _lib
    a = dict(ACCUM_OK, **bad)
    assert _lib.load().dv_pairstat_accum_f32(*[a[n] for n in ACCUM_OK], None) == EINVAL


@pytest.mark.parametrize('bad', ACCUM_MISALIGNED, ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_pairstat_accum_refuses_misaligned_state(bad):
    from dualvar_amd import _lib
    a = dict(ACCUM_OK, **bad)
    assert _lib.load().dv_pairstat_accum_f32(*[a[n] for n in ACCUM_OK], None) == EALIGN


def test_pairstat_workspace_query():
    """negative for bad sizes; otherwise 96 bytes per workgroup, one workgroup per 64 x 1024 tile up to 1024 of them"""
    from dualvar_amd import _lib
    ws = _lib.load().dv_pairstat_workspace
    for R, n in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert ws(R, n) < 0, (R, n)
    assert ws(1, 1) == 96 and ws(64, 1024) == 96 and ws(65, 1024) == 2 * 96 and ws(64, 1025) == 2 * 96 and ws(130, 2049) == 9 * 96
    assert ws(4096, 16384) == 1024 * 96 == ws(2 ** 31 - 1, 2 ** 31 - 1)          # capped: the 64-bit tile count does not wrap


# ------------------------------------------------------------------------------------------------------- report_from_state
def hand_state():
    """bins = 4, t = 0.5.  Category 0: the pairs s = 0.5, 0.5, 1.0, -0.5 (and one non-finite); category 1: empty; category 2:
    s = 0.0 (x2), -1.0 (x2).  w = exp((s - 1) * 2t) = exp(s - 1)."""
    s0, s2 = [0.5, 0.5, 1.0, -0.5], [0.0, 0.0, -1.0, -1.0]
    sums = torch.zeros(3, 4, dtype=torch.float64)
    for c, ss in ((0, s0), (2, s2)):
        sums[c, 0], sums[c, 1], sums[c, 2] = sum(ss), sum(v * v for v in ss), sum(math.exp(v - 1.0) for v in ss)
    ext = torch.tensor([[-0.5, 1.0], [INF, -INF], [-1.0, 0.0]])
    # bins of width 0.5 over [-1, 1]: -1.0 -> 0, -0.5 -> 1, 0.0 -> 2, 0.5 -> 3, 1.0 -> 3 (clamped); the last column: non-finite
    hist = torch.tensor([[0, 1, 0, 3, 1], [0, 0, 0, 0, 0], [2, 0, 2, 0, 0]])
    return sums, ext, hist


def test_report_from_state_by_hand():
    from dualvar_amd.utils.variance import CATEGORIES, report_from_state
    assert CATEGORIES == ('same_video', 'same_class', 'diff_class')
    sums, ext, hist = hand_state()
    rep = report_from_state(sums, ext, hist, 4, 0.5)
    c0, c1, c2 = (rep['categories'][n] for n in CATEGORIES)
    assert (c0['count'], c0['skipped'], c1['count'], c1['skipped'], c2['count'], c2['skipped']) == (4, 1, 0, 0, 4, 0)
    assert c0['hist'] == [0, 1, 0, 3] and c2['hist'] == [2, 0, 2, 0] and c1['hist'] == [0, 0, 0, 0]
    for c in (c0, c1, c2):
        assert sum(c['hist']) == c['count']
    # category 0: mean 1.5 / 4 = 0.375, E s^2 = 1.75 / 4 = 0.4375, var = 0.4375 - 0.140625 = 0.296875
    assert c0['mean'] == pytest.approx(0.375, abs=1e-15) and c0['std'] == pytest.approx(math.sqrt(0.296875), abs=1e-15)
    assert (c0['min'], c0['max']) == (-0.5, 1.0)
    # category 2: mean -0.5, E s^2 = 0.5, var 0.25
    assert c2['mean'] == pytest.approx(-0.5, abs=1e-15) and c2['std'] == pytest.approx(0.5, abs=1e-15) and (c2['min'], c2['max']) == (-1.0, 0.0)
    # the empty category: None, never NaN or the infinities of its extrema
    assert c1['mean'] is None and c1['std'] is None and c1['min'] is None and c1['max'] is None
    assert rep['var_intra_video'] == pytest.approx(0.625, abs=1e-15)                  # 1 - 0.375
    assert rep['var_inter_video'] == pytest.approx(1.5, abs=1e-15)                    # categories 1 u 2 = category 2: 1 + 0.5
    assert rep['var_intra_class'] is None and rep['ratio_class'] is None
    assert rep['var_inter_class'] == pytest.approx(1.5, abs=1e-15)
    assert rep['ratio_video'] == pytest.approx(0.625 / 1.5, abs=1e-15)
    assert rep['alignment'] == pytest.approx(1.25, abs=1e-15)
    w = 2 * math.exp(-0.5) + 1.0 + math.exp(-1.5) + 2 * math.exp(-1.0) + 2 * math.exp(-2.0)
    assert rep['uniformity'] == pytest.approx(math.log(w / 8), abs=1e-15)
    assert rep['bins'] == 4 and rep['t'] == 0.5
    import json
    assert 'NaN' not in json.dumps(rep) and 'Infinity' not in json.dumps(rep)


def test_report_from_state_pools_categories_one_and_two_by_count():
    """var_inter_video is one minus the mean over the union of categories 1 and 2 (weighted by their counts, not the mean of the
    two means); a pitch beyond bins + 1 is ignored; everything empty gives None throughout"""
    from dualvar_amd.utils.variance import report_from_state
    sums = torch.tensor([[0.9, 0.81, 1.0, 0.0], [0.5, 0.25, 1.0, 0.0], [-0.75, 0.1875, 3.0, 0.0]], dtype=torch.float64)
    ext = torch.tensor([[0.9, 0.9], [0.5, 0.5], [-0.25, -0.25]])
    hist = torch.tensor([[0, 1, 7, 99, 99], [0, 1, 0, 99, 99], [3, 0, 0, 99, 99]])      # bins = 2, ldh = 5
    rep = report_from_state(sums, ext, hist, 2, 2.0)
    assert [rep['categories'][n]['count'] for n in ('same_video', 'same_class', 'diff_class')] == [1, 1, 3]
    assert rep['categories']['same_video']['skipped'] == 7
    assert rep['var_inter_video'] == pytest.approx(1.0 - (0.5 - 0.75) / 4, abs=1e-15)
    assert rep['var_intra_class'] == pytest.approx(0.5, abs=1e-15) and rep['var_inter_class'] == pytest.approx(1.25, abs=1e-15)
    assert rep['ratio_class'] == pytest.approx(0.4, abs=1e-15)
    assert rep['uniformity'] == pytest.approx(0.0, abs=1e-15)                          # log(5 / 5)
    assert rep['categories']['diff_class']['std'] == pytest.approx(0.0, abs=1e-9)      # three equal values
    empty = report_from_state(torch.zeros(3, 4, dtype=torch.float64), torch.tensor([[INF, -INF]] * 3), torch.zeros(3, 3, dtype=torch.int64), 2, 2.0)
    for key in ('var_intra_video', 'var_inter_video', 'var_intra_class', 'var_inter_class', 'ratio_video', 'ratio_class', 'alignment', 'uniformity'):
        assert empty[key] is None, key


def test_host_module_refuses_before_the_device(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import variance as V

    def no_device():
        raise AssertionError('the device was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_device', no_device)
    monkeypatch.setattr(_lib, 'load', no_device)
    f, ids = torch.zeros(6, 8), torch.zeros(6, dtype=torch.int32)
    for bins in (0, 257, -1):
        with pytest.raises(ValueError, match='DV_PAIRSTAT_MAX_BINS'):
            V.pair_statistics(f, ids, ids, bins=bins)
    for t in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match='t must be'):
            V.pair_statistics(f, ids, ids, t=t)
        with pytest.raises(ValueError, match='t must be'):
            V.pair_statistics_cross(f, ids, ids, f, ids, ids, t=t)
    with pytest.raises(ValueError, match='device tensor'):
        V.pair_statistics(f, ids, ids)
    with pytest.raises(ValueError, match='device tensor'):
        V.pair_statistics_cross(f, ids, ids, f, ids, ids)
    with pytest.raises(ValueError, match='n_video, num_seq, D'):
        V.variance_eval(f, ids)


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_variance_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --variance --var_bins 32 --var_t 3.5'))
    assert a.variance is True and a.var_bins == 32 and a.var_t == 3.5
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.variance is False and d.var_bins == 64 and d.var_t == 2.0
    CLI.check_args(d, environ={})
    for ok in (' --variance --var_bins 1', ' --variance --var_bins 256', ' --variance --var_t 0', ' --variance --knn'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --variance', '--variance'),                                  # --variance alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --variance', '--variance'),
    (RETRIEVAL + ' --variance --var_bins 0', '--var_bins'),
    (RETRIEVAL + ' --variance --var_bins 257', '--var_bins'),
    (RETRIEVAL + ' --variance --var_t -1', '--var_t'),
    (RETRIEVAL + ' --variance --var_t nan', '--var_t'),
    (RETRIEVAL + ' --variance --var_t inf', '--var_t'),
])
def test_variance_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))
