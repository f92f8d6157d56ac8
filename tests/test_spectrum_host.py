"""CPU: the spectrum entries (include/dualvar_spectrum.h) agree with their ctypes table and the library's exports and refuse every
bad argument of their header comments before any launch; the round-robin schedule of dv_spectrum_pair is a schedule (disjoint
slots, every pair once per sweep) and equals the model's; the float64 model of tests/spectrum_reference.py against
numpy.linalg.eigh on the case table (its largest ratios are MODEL_RATIOS, the yardstick of tests/test_spectrum_gpu.py);
spectrum_metrics on hand cases; classifier.py parses and checks the --spectrum flags and only that branch writes the _spectrum
files; without a GPU every host entry raises DualVarHipError."""
import ast
import ctypes
import json
import logging
import os
import re
import shlex
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import spectrum_reference as R
from tests.checks import lib
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it


def __getattr__(name):
    """MODEL_RATIOS: the largest ratios of the model over the case table, each in its unit (eps n |A|_2 for the eigenvalues, the
    residual and the trace, eps n for the orthogonality); MODEL_INFO: the info of every case.  The GPU test allows four times
    the ratios.  Computed on first use (the model runs for some seconds), once per process."""
    if name in ('MODEL_RATIOS', 'MODEL_INFO'):
        return R.model_ratios()[name == 'MODEL_INFO']
    raise AttributeError(name)


def test_spectrum_header_table_and_library_agree():
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_spectrum.h')
    assert set(decl) == set(_lib.SPECTRUM_SIGNATURES) and len(decl) == 6
    assert all(ret == 'int' for ret, _ in decl.values())
    assert 'spectrum.hip' in build.SOURCES
    for macro, want in (('DV_SPECTRUM_MAX_D', R.MAX_D), ('DV_SPECTRUM_MAX_SWEEPS', R.MAX_SWEEPS), ('DV_SPECTRUM_BLOCK', R.BLOCK)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == want, macro
    assert _lib.DV_SPECTRUM_MAX_D == R.MAX_D and _lib.DV_SPECTRUM_MAX_SWEEPS == R.MAX_SWEEPS
    gpu_test = open(os.path.join(ROOT, 'tests', 'test_spectrum_gpu.py')).read()
    for name in decl:
        where = open(__file__).read() if name in ('dv_spectrum_rounds', 'dv_spectrum_pair') else gpu_test
        assert re.search(r"lib\(\)\.%s\(" % name, where), '%s is not called by its test file' % name


def test_spectrum_source_keeps_the_launch_boundary():
    """no read-modify-write instruction, no ticket and no fence in csrc/spectrum.hip: a round ends with its launch"""
    src = open(os.path.join(ROOT, 'dualvar_amd', 'csrc', 'spectrum.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert not re.search(r'atomic|__HIP_MEMORY_SCOPE|ordered_fold|__threadfence', code)
    assert len(re.findall(r'\bsp_pair\(', code)) == 3              # the definition, the query and the kernel: one schedule


# ------------------------------------------------------------------------------------------------------------ schedule
def _pair(n, r, k):
    p, q = ctypes.c_int32(-7), ctypes.c_int32(-7)
    assert lib().dv_spectrum_pair(n, r, k, ctypes.byref(p), ctypes.byref(q)) == 0, (n, r, k)
    return p.value, q.value


def test_rounds_query():
    for n, want in ((1, 0), (2, 1), (3, 3), (4, 3), (7, 7), (8, 7), (65, 65), (4095, 4095), (4096, 4095)):
        assert lib().dv_spectrum_rounds(n) == want == R.rounds(n), n
    for bad in (0, -1, 4097):
        assert lib().dv_spectrum_rounds(bad) == EINVAL


@pytest.mark.parametrize('n', [1, 2, 3, 7, 8, 65, 4096])
def test_pair_is_a_round_robin_schedule(n):
    m = n + (n & 1)
    rounds = lib().dv_spectrum_rounds(n)
    p, q = ctypes.c_int32(), ctypes.c_int32()
    for bad in ((rounds, 0), (-1, 0), (0, m // 2), (0, -1)):
        assert lib().dv_spectrum_pair(n, bad[0], bad[1], ctypes.byref(p), ctypes.byref(q)) == EINVAL, bad
    if n == 1:
        assert rounds == 0
        return
    assert lib().dv_spectrum_pair(n, 0, 0, None, ctypes.byref(q)) == EINVAL
    assert lib().dv_spectrum_pair(n, 0, 0, ctypes.byref(p), None) == EINVAL
    seen = np.zeros((m, m), dtype=np.int32)
    check_rounds = range(rounds) if n <= 65 else (0, 1, 2, rounds // 2, rounds - 2, rounds - 1)
    for r in check_rounds:
        pairs = [_pair(n, r, k) for k in range(m // 2)]
        assert pairs == [R.pair(n, r, k) for k in range(m // 2)], r
        assert pairs[0] == (r, m - 1)
        assert all(a < b for a, b in pairs)
        assert sorted(i for ab in pairs for i in ab) == list(range(m)), r       # disjoint, and every index sits in one slot
        live = [(a, b) for a, b in pairs if b < n]
        mp, mq = R.round_pairs(n, r)
        assert live == list(zip(mp.tolist(), mq.tolist()))
        assert len(live) == (m // 2 if n == m else m // 2 - 1)                   # odd n: exactly one slot is the bye
        for a, b in pairs:
            seen[a, b] += 1
    if n <= 65:
        assert (seen[np.triu_indices(m, 1)] == 1).all() and seen.sum() == m * (m - 1) // 2
    else:                                                                        # every pair once per sweep, from the model's table
        count = np.zeros((m, m), dtype=np.int32)
        for r in range(rounds):
            mp, mq = R.round_pairs(n, r)
            count[mp, mq] += 1
        assert (count[np.triu_indices(m, 1)] == 1).all()


# ------------------------------------------------------------------------------------------------------------ refusals
COV_OK = dict(G=X, ldg=9, D=8, Cov=X, ldc=8, mean=X)
COV_BAD = [dict(G=None), dict(Cov=None), dict(mean=None), dict(D=0), dict(D=-1), dict(D=4097, ldg=5000, ldc=5000), dict(ldg=8), dict(ldc=7)]
COV_MIS = [dict(G=X + 4), dict(Cov=X + 4), dict(mean=X + 4)]
INIT_OK = dict(A=X, lda=8, n=8, W=X, ldw=8, V=X, ldv=8, scale=X)
INIT_BAD = [dict(A=None), dict(W=None), dict(V=None), dict(scale=None), dict(n=0), dict(n=-2), dict(n=4097, lda=5000, ldw=5000, ldv=5000),
            dict(lda=7), dict(ldw=7), dict(ldv=7)]
INIT_MIS = [dict(A=X + 4), dict(W=X + 4), dict(V=X + 4), dict(scale=X + 4)]
ROUNDS_OK = dict(W=X, ldw=8, V=X, ldv=8, n=8, round_lo=0, round_hi=7, scale=X, stat=X)
ROUNDS_BAD = [dict(W=None), dict(V=None), dict(scale=None), dict(stat=None), dict(n=0), dict(n=4097, ldw=5000, ldv=5000), dict(ldw=7),
              dict(ldv=7), dict(round_lo=-1), dict(round_lo=5, round_hi=4), dict(round_hi=8), dict(n=1, round_hi=1)]
ROUNDS_MIS = [dict(W=X + 4), dict(V=X + 4), dict(scale=X + 4), dict(stat=X + 4)]
VALUES_OK = dict(W=X, ldw=8, V=X, ldv=8, n=8, lam=X)
VALUES_BAD = [dict(W=None), dict(V=None), dict(lam=None), dict(n=0), dict(n=4097, ldw=5000, ldv=5000), dict(ldw=7), dict(ldv=7)]
VALUES_MIS = [dict(W=X + 4), dict(V=X + 4), dict(lam=X + 4)]
_ids = lambda d: ','.join('%s=%s' % kv for kv in d.items())       # noqa: E731


@pytest.mark.parametrize('bad', COV_BAD + COV_MIS, ids=_ids)
def test_cov_refuses_without_gpu(bad):
    a = dict(COV_OK, **bad)
    assert lib().dv_spectrum_cov_f64(*[a[n] for n in COV_OK], None) == (EALIGN if bad in COV_MIS else EINVAL)


@pytest.mark.parametrize('bad', INIT_BAD + INIT_MIS, ids=_ids)
def test_init_refuses_without_gpu(bad):
    a = dict(INIT_OK, **bad)
    assert lib().dv_spectrum_init_f64(*[a[n] for n in INIT_OK], None) == (EALIGN if bad in INIT_MIS else EINVAL)


@pytest.mark.parametrize('bad', ROUNDS_BAD + ROUNDS_MIS, ids=_ids)
def test_rounds_refuse_without_gpu(bad):
    a = dict(ROUNDS_OK, **bad)
    assert lib().dv_spectrum_rounds_f64(*[a[n] for n in ROUNDS_OK], None) == (EALIGN if bad in ROUNDS_MIS else EINVAL)


@pytest.mark.parametrize('bad', VALUES_BAD + VALUES_MIS, ids=_ids)
def test_values_refuse_without_gpu(bad):
    a = dict(VALUES_OK, **bad)
    assert lib().dv_spectrum_values_f64(*[a[n] for n in VALUES_OK], None) == (EALIGN if bad in VALUES_MIS else EINVAL)


def test_the_limits_themselves_pass_the_argument_check():
    """n = D = DV_SPECTRUM_MAX_D, the pitches equal to n, round_lo == round_hi and round_hi == rounds are not refused: only the
    misalignment stops these calls before a launch"""
    a = dict(COV_OK, D=4096, ldg=4097, ldc=4096, mean=X + 4)
    assert lib().dv_spectrum_cov_f64(*[a[n] for n in COV_OK], None) == EALIGN
    a = dict(INIT_OK, n=4096, lda=4096, ldw=4096, ldv=4096, scale=X + 4)
    assert lib().dv_spectrum_init_f64(*[a[n] for n in INIT_OK], None) == EALIGN
    for edge in (dict(round_lo=7, round_hi=7), dict(round_lo=0, round_hi=0), dict(round_hi=7), dict(n=1, ldw=1, ldv=1, round_hi=0),
                 dict(n=4096, ldw=4096, ldv=4096, round_lo=4094, round_hi=4095)):
        a = dict(ROUNDS_OK, stat=X + 4, **edge)
        assert lib().dv_spectrum_rounds_f64(*[a[n] for n in ROUNDS_OK], None) == EALIGN, edge
    a = dict(VALUES_OK, n=4096, ldw=4096, ldv=4096, lam=X + 4)
    assert lib().dv_spectrum_values_f64(*[a[n] for n in VALUES_OK], None) == EALIGN


# --------------------------------------------------------------------------------------------------------------- model
def test_model_against_numpy_eigh():
    """every case converges within the cap; the ratios stay at what the design promises: a few units of eps n.  (2.3, 2.3 and 0.5
    were seen with lambda = v . w; the Rayleigh quotient proper, divided by v . v, brings the eigenvalues to 0.41 and the trace,
    otherwise off by up to 70 units, to 0.55.)"""
    MODEL_RATIOS, MODEL_INFO = R.model_ratios()
    print('MODEL_RATIOS', MODEL_RATIOS)
    for name, info in MODEL_INFO.items():
        print(name, info)
        assert info['converged'] and info['sweeps'] <= 30, name
    assert MODEL_RATIOS['values'] <= 2.3 and MODEL_RATIOS['orth'] <= 2.3 and MODEL_RATIOS['resid'] <= 0.5 and MODEL_RATIOS['trace'] <= 2.3
    assert MODEL_INFO['diag'] == {'sweeps': 1, 'converged': True, 'max_ratio': 0.0, 'rotations': 0}
    assert MODEL_INFO['n1']['sweeps'] == 1 and MODEL_INFO['n2']['rotations'] == 1
    lam, comps, _ = R.eigh_model(R.cases()['diag'])
    assert lam.tolist() == sorted(np.diag(R.cases()['diag']).tolist(), reverse=True)
    lam, comps, _ = R.eigh_model(R.cases()['powerlaw'])
    want = np.arange(1, 131, dtype=np.float64) ** -2.0
    assert np.abs(lam - want).max() <= 4 * R.EPS * 130
    assert (comps[np.arange(130), np.abs(comps).argmax(1)] > 0).all()


def test_the_floor_is_what_ends_the_sweeps():
    """ten duplicated feature columns: with the floor the model converges in 10 sweeps, without it the null rows keep rotating
    against each other and 30 sweeps do not end it"""
    MODEL_INFO = R.model_ratios()[1]
    A = R.cases()['duplicated']
    assert np.linalg.matrix_rank(A) == 30
    assert MODEL_INFO['duplicated']['converged'] and MODEL_INFO['duplicated']['sweeps'] <= 12
    _, _, info = R.eigh_model(A, max_sweeps=30, floor=False)
    assert not info['converged'] and info['sweeps'] == 30 and info['rotations'] > 0


def test_the_kernel_order_of_the_sums_stays_within_the_gpu_bounds():
    """the model with every dot product summed as the kernels sum it (strided partials, then the tree) meets the bounds the GPU
    test sets, on the cases small enough to be quick here"""
    MODEL_RATIOS = R.model_ratios()[0]
    for name in ('n3', 'n7', 'n65', 'duplicated', 'rank_deficient'):
        A = R.cases()[name]
        lam, comps, info = R.eigh_model(A, kernel_order=True)
        q = R.quality(A, lam, comps)
        assert info['converged']
        assert q['values'] <= 4 * MODEL_RATIOS['values'] and q['orth'] <= 4 * MODEL_RATIOS['orth'], (name, q)
        assert q['resid'] <= 4 * MODEL_RATIOS['resid'] and q['trace'] <= 4 * MODEL_RATIOS['values'], (name, q)


def test_the_fixture_of_the_gpu_test():
    """the facts tests/test_spectrum_gpu.py relies on, from the model alone: of the three leading components of the fixture the
    first two lie between videos (shares 0.9994 and 0.9983) and the third within them (0.0008)"""
    clips, _ = R.spectrum_fixture()
    z = R.normalise_ref(clips).astype(np.float32).astype(np.float64)
    mean, cov = R.cov_from_gram(R.gram_of(z))
    assert np.abs(cov - R.cov_of(z)).max() < 1e-15 and np.abs(mean - z.mean(0)).max() < 1e-15
    lam, comps, info = R.eigh_model(cov)
    share = R.video_share_ref(z, 24, 4, mean, comps, lam, 8)
    print('video share', share, 'lam', lam[:5], info)
    assert info['converged'] and share[0] >= 0.99 and share[1] >= 0.99 and share[2] <= 0.01
    assert lam[2] > 5 * lam[3]                                  # the three planted directions stand clear of the rest
    y = R.project_ref(z, mean, comps, lam, 8)
    assert np.abs(R.cov_of(y) - np.diag(lam[:8])).max() < 1e-15
    yw = R.project_ref(z, mean, comps, lam, 8, whiten=True)
    assert np.abs(R.cov_of(yw) - np.eye(8)).max() < 3e-8         # eps = 1e-12 under the root against lam_8 of 5e-5: 2e-8


# ------------------------------------------------------------------------------------------------------------- metrics
def test_spectrum_metrics_hand_cases():
    from dualvar_amd.utils.spectrum import spectrum_metrics
    m = spectrum_metrics([1.0, 1.0, 1.0, 1.0], 100)
    assert abs(m['effective_rank'] - 4) < 1e-12 and abs(m['participation_ratio'] - 4) < 1e-12 and m['numerical_rank'] == 4
    assert m['explained'] == {'1': 0.25, '2': 0.5, '4': 1.0} and m['dims_for'] == {'0.90': 4, '0.95': 4, '0.99': 4}
    assert m['trace'] == 4.0 and m['lambda_max'] == 1.0 and m['top1_share'] == 0.25
    assert abs(m['alpha']) < 1e-12                             # a flat spectrum: slope 0
    m = spectrum_metrics([1.0, 0.0, 0.0], 100)
    assert m['effective_rank'] == 1.0 and m['dims_for'] == {'0.90': 1, '0.95': 1, '0.99': 1} and m['numerical_rank'] == 1
    assert m['participation_ratio'] == 1.0 and m['alpha'] is None and abs(m['rankme'] - 1) < 1e-5
    lam = np.arange(1, 201, dtype=np.float64) ** -1.5
    m = spectrum_metrics(torch.from_numpy(lam[::-1].copy()), 1000)            # any order
    assert abs(m['alpha'] - 1.5) < 1e-12 and abs(m['alpha_r2'] - 1) < 1e-12
    m = spectrum_metrics(lam, 51)                              # the ranks are capped at n - 1 = 50
    assert abs(m['alpha'] - 1.5) < 1e-12
    m = spectrum_metrics([2.0, 1.0, -1e-17, -3e-18], 10)       # round-off below zero is clipped
    assert m['trace'] == 3.0 and m['numerical_rank'] == 2 and abs(m['effective_rank'] - np.exp(-(2 / 3 * np.log(2 / 3) + 1 / 3 * np.log(1 / 3)))) < 1e-12
    z = spectrum_metrics([0.0, 0.0], 5)
    assert z['effective_rank'] == 0.0 and z['alpha'] is None and z['numerical_rank'] == 0
    rng = np.random.RandomState(5)
    for D, n in ((7, 4), (40, 96), (130, 2000)):
        lam = np.sort(rng.rand(D) ** 3)[::-1]
        got, want = spectrum_metrics(lam, n), R.metrics_ref(lam, n)
        for key in ('trace', 'lambda_max', 'top1_share', 'effective_rank', 'rankme', 'participation_ratio', 'alpha', 'alpha_r2'):
            assert abs(got[key] - want[key]) <= 1e-10 * max(1.0, abs(want[key])), (D, key)
        assert got['numerical_rank'] == want['numerical_rank'] and got['dims_for'] == want['dims_for']
        assert got['explained'].keys() == want['explained'].keys()
        assert all(abs(got['explained'][k] - want['explained'][k]) < 1e-12 for k in want['explained'])
    json.dumps(got)                                            # the report is plain data


# ------------------------------------------------------------------------------------------------------- no GPU, no result
def test_host_entries_raise_without_a_gpu(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import spectrum as SP
    asked = []
    monkeypatch.setattr(_lib, 'require_device', lambda: asked.append(1))
    with pytest.raises(ValueError, match='DV_SPECTRUM_MAX_D'):
        SP.covariance(torch.zeros(4, 4097))
    with pytest.raises(ValueError, match='DV_SPECTRUM_MAX_D'):
        SP.eigh_jacobi(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match='float64'):
        SP.eigh_jacobi(torch.zeros(3, 3))
    with pytest.raises(ValueError, match='at least one sweep'):
        SP.eigh_jacobi(torch.zeros(3, 3, dtype=torch.float64), max_sweeps=0)
    with pytest.raises(ValueError, match='components'):
        SP.pca_project(torch.zeros(5, 8), torch.zeros(8), torch.zeros(8, 8), torch.zeros(8), 9)
    with pytest.raises(ValueError, match='mean'):
        SP.pca_project(torch.zeros(5, 8), torch.zeros(7), torch.zeros(8, 8), torch.zeros(8), 2)
    with pytest.raises(ValueError, match='V, S, D'):
        SP.spectrum_eval(torch.zeros(5, 8))
    with pytest.raises(ValueError, match='one label per video'):
        SP.spectrum_eval(torch.zeros(5, 2, 8), torch.zeros(4))
    with pytest.raises(ValueError, match='at least 1'):
        SP.spectrum_eval(torch.zeros(5, 2, 8), ks=(0, 4))
    assert not asked
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, '_device_ok', False)
    with pytest.raises(_lib.DualVarHipError):
        SP.covariance(torch.zeros(20, 8))
    with pytest.raises(_lib.DualVarHipError):
        SP.eigh_jacobi(torch.eye(3, dtype=torch.float64))
    with pytest.raises(_lib.DualVarHipError):
        SP.pca_project(torch.zeros(5, 8), torch.zeros(8), torch.zeros(8, 8), torch.zeros(8), 2)
    with pytest.raises(_lib.DualVarHipError):
        SP.spectrum_eval(torch.zeros(5, 2, 8))


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_spectrum_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --spectrum --spectrum_k 8 5000'))
    assert a.spectrum is True and a.spectrum_k == [8, 5000]
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.spectrum is False and d.spectrum_k == [32, 64, 128]
    CLI.check_args(d, environ={})
    for ok in (' --spectrum', ' --spectrum --spectrum_k 1', ' --spectrum --knn --variance --tsne --cluster --ridge'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --spectrum', '--spectrum'),                                  # --spectrum alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --spectrum', '--spectrum'),
    (RETRIEVAL + ' --spectrum --spectrum_k 0', '--spectrum_k'),
    (RETRIEVAL + ' --spectrum --spectrum_k 32 -4', '--spectrum_k'),
    (RETRIEVAL + ' --spectrum --spectrum_k', '--spectrum_k'),                   # an empty list
])
def test_spectrum_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))


def test_only_the_spectrum_branch_writes_spectrum_files(tmp_path, monkeypatch):
    """every '_spectrum' file name is formed inside write_spectrum, write_spectrum is called from one place, under
    `if args.spectrum:`, and nothing else in the driver reads a spectrum flag but check_args; with spectrum_eval and
    pca_retrieval stubbed write_spectrum writes exactly its three files"""
    import classifier as CLI
    from dualvar_amd.utils import spectrum as SP
    src = open(os.path.join(ROOT, 'classifier.py')).read()
    tree = ast.parse(src)
    funcs = {f.name: f for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}
    lo, hi = funcs['write_spectrum'].lineno, funcs['write_spectrum'].end_lineno
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and '_spectrum' in node.value and not node.value.startswith('--'):
            assert lo <= node.lineno <= hi, (node.lineno, node.value)
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'id', None) == 'write_spectrum']
    assert len(calls) == 1
    guards = [n for n in ast.walk(funcs['test_retrieval']) if isinstance(n, ast.If) and ast.unparse(n.test) == 'args.spectrum']
    assert len(guards) == 1 and guards[0].lineno < calls[0].lineno <= guards[0].end_lineno
    users = {n for n, f in funcs.items() for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr.startswith('spectrum')}
    assert users == {'check_args', 'test_retrieval', 'write_spectrum'}, users
    # in test_retrieval the flag is read twice: to keep the clip features and to enter the branch
    reads = [a for a in ast.walk(funcs['test_retrieval']) if isinstance(a, ast.Attribute) and a.attr.startswith('spectrum')]
    assert sorted(a.attr for a in reads) == ['spectrum', 'spectrum'], [a.attr for a in reads]

    seen = {'eval': [], 'retrieval': []}

    def eval_stub(clips, video_label=None, ks=()):
        seen['eval'].append((tuple(clips.shape), tuple(ks)))
        D = clips.shape[-1]
        return {'metrics': SP.spectrum_metrics(np.arange(D, 0, -1.0), clips.shape[0] * clips.shape[1]),
                'info': {'sweeps': 3, 'converged': True, 'max_ratio': 0.0, 'rotations': 17},
                'video_share': [0.5, None] + [0.25] * (max(ks) - 2), 'ks': sorted(ks), 'mean': torch.zeros(D, dtype=torch.float64),
                'components': torch.eye(D, dtype=torch.float64), 'eigenvalues': torch.arange(D, 0, -1, dtype=torch.float64)}

    def retrieval_stub(train_feat, train_label, test_feat, test_label, mean, comps, lam, ks):
        seen['retrieval'].append((tuple(train_feat.shape), tuple(test_feat.shape), tuple(ks)))
        return {k: {'pca': 0.5, 'whitened': 0.75} for k in ks}
    monkeypatch.setattr(SP, 'spectrum_eval', eval_stub)
    monkeypatch.setattr(SP, 'pca_retrieval', retrieval_stub)
    messages = []
    logger = types.SimpleNamespace(info=lambda m: messages.append(str(m)))
    args = types.SimpleNamespace(spectrum_k=[4, 8, 64], dataset='ucf101', logger=logger)
    clips = {'train': torch.zeros(6, 10, 12), 'test': torch.zeros(3, 10, 12)}
    feats = {'train': (torch.zeros(6, 12), torch.tensor([0, 1, 2, 0, 1, 2])), 'test': (torch.zeros(3, 12), torch.tensor([0, 1, 2]))}
    CLI.write_spectrum(clips, feats, str(tmp_path), args)
    assert sorted(os.listdir(str(tmp_path))) == ['ucf101_spectrum.pth.tar', 'ucf101_test_spectrum.json', 'ucf101_train_spectrum.json']
    assert seen['eval'] == [((3, 10, 12), (4, 8, 12)), ((6, 10, 12), (4, 8, 12))]            # 64 clamped to D = 12
    assert seen['retrieval'] == [((6, 12), (3, 12), (8,))]                                   # multiples of 8 only
    assert any('clamped' in m and '12' in m for m in messages) and any('left out' in m for m in messages)
    train = json.load(open(str(tmp_path / 'ucf101_train_spectrum.json')))
    test = json.load(open(str(tmp_path / 'ucf101_test_spectrum.json')))
    assert train['pca_retrieval'] == {'8': {'pca': 0.5, 'whitened': 0.75}} and 'pca_retrieval' not in test
    assert train['ks'] == [4, 8, 12] and train['info']['rotations'] == 17 and train['video_share'][1] is None
    assert len(train['eigenvalues']) == 12 and train['metrics']['D'] == 12 and test['metrics']['n'] == 30
    saved = torch.load(str(tmp_path / 'ucf101_spectrum.pth.tar'), weights_only=True)
    assert saved['mean'].shape == (12,) and saved['components'].shape == (12, 12) and saved['eigenvalues'].shape == (12,)
    assert saved['components'].dtype == torch.float64
