"""CPU: the ridge-probe entries (include/dualvar_ridge.h) agree with their ctypes table, the library's exports and the ledger below
and refuse every bad argument of their header comments before any launch; the workspace query returns what the header says; the
float64 reference of tests/ridge_reference.py against np.linalg.lstsq on the stacked system; holdout_mask on hand cases;
classifier.py parses and checks the --ridge flags and only that branch writes the _ridge files; without a GPU every host entry
raises DualVarHipError."""
import ast
import json
import logging
import math
import os
import re
import shlex
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import abi_coverage as A
from tests import ridge_reference as R
from tests.checks import lib
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it

# The coverage ledger of include/dualvar_ridge.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.RIDGE_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
RIDGE_COVERAGE = {
    'dv_ridge_gram_workspace': ('test_ridge_host.py', A.HOST_QUERY),
    'dv_ridge_gram_f64': ('test_ridge_gpu.py', A.FLOAT64),
    'dv_ridge_solve_f64': ('test_ridge_gpu.py', A.FLOAT64),
}


def test_ridge_header_table_and_library_agree():
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_ridge.h')
    assert set(decl) == set(_lib.RIDGE_SIGNATURES) == set(RIDGE_COVERAGE) and len(decl) == 3
    assert 'ridge.hip' in build.SOURCES
    for macro, want in (('DV_RIDGE_MAX_D', R.MAX_D), ('DV_RIDGE_MAX_C', R.MAX_C), ('DV_RIDGE_SLAB', R.SLAB),
                        ('DV_RIDGE_MAX_SLABS', R.MAX_SLABS), ('DV_RIDGE_TILE', R.TILE)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == want, macro
    assert _lib.DV_RIDGE_MAX_D == R.MAX_D and _lib.DV_RIDGE_MAX_C == R.MAX_C
    for name, (fname, kind) in RIDGE_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"lib\.%s\(|lib\(\)\.%s\(" % (name, name), open(os.path.join(ROOT, 'tests', fname)).read()), \
            '%s is not called by tests/%s' % (name, fname)


def test_ridge_source_keeps_the_launch_boundary():
    """no atomics of any kind and no ticket in csrc/ridge.hip: the slabs are folded by a second launch"""
    src = open(os.path.join(ROOT, 'dualvar_amd', 'csrc', 'ridge.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert not re.search(r'atomic|__HIP_MEMORY_SCOPE|ordered_fold|__threadfence', code)
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64' in code


GRAM_OK = dict(z=X, ldz=8, n=5, D=8, label=X, C=3, G=X, ldg=9, B=X, ldb=3, accumulate=0, workspace=X)
GRAM_BAD = [dict(z=None), dict(label=None), dict(G=None), dict(B=None), dict(workspace=None), dict(n=0), dict(n=-3), dict(D=0),
            dict(D=4097, ldz=5000, ldg=5000), dict(C=0), dict(C=4097, ldb=5000), dict(ldz=7), dict(ldg=8), dict(ldb=2)]
GRAM_MIS = [dict(G=X + 4), dict(B=X + 4), dict(workspace=X + 4)]
SOLVE_OK = dict(G=X, ldg=9, Da=9, n_pen=8, lam=0.5, B=X, ldb=3, C=3, W=X, ldw=3, chol=X, ldc=9, info=X)
SOLVE_BAD = [dict(G=None), dict(B=None), dict(W=None), dict(chol=None), dict(info=None), dict(Da=0), dict(Da=-1),
             dict(Da=4098, ldg=5000, ldc=5000, n_pen=0), dict(n_pen=-1), dict(n_pen=10), dict(lam=-1e-300), dict(lam=math.inf),
             dict(lam=math.nan), dict(C=0), dict(C=4097, ldb=5000, ldw=5000), dict(ldg=8), dict(ldc=8), dict(ldb=2), dict(ldw=2)]
SOLVE_MIS = [dict(G=X + 4), dict(B=X + 4), dict(W=X + 4), dict(chol=X + 4), dict(info=X + 2)]
_ids = lambda d: ','.join('%s=%s' % kv for kv in d.items())       # noqa: E731


@pytest.mark.parametrize('bad', GRAM_BAD + GRAM_MIS, ids=_ids)
def test_gram_refuses_without_gpu(bad):
    a = dict(GRAM_OK, **bad)
    assert lib().dv_ridge_gram_f64(*[a[n] for n in GRAM_OK], None) == (EALIGN if bad in GRAM_MIS else EINVAL)


@pytest.mark.parametrize('bad', SOLVE_BAD + SOLVE_MIS, ids=_ids)
def test_solve_refuses_without_gpu(bad):
    a = dict(SOLVE_OK, **bad)
    assert lib().dv_ridge_solve_f64(*[a[n] for n in SOLVE_OK], None) == (EALIGN if bad in SOLVE_MIS else EINVAL)


def test_the_limits_themselves_pass_the_argument_check():
    """D = DV_RIDGE_MAX_D, C = DV_RIDGE_MAX_C, n_pen = 0 and n_pen = Da, lambda = 0 are not refused: the refusals above are
    the edge, not a band around it.  (Only misalignment stops these calls before a launch.)"""
    a = dict(GRAM_OK, D=4096, ldz=4096, ldg=4097, C=4096, ldb=4096, G=X + 4)
    assert lib().dv_ridge_gram_f64(*[a[n] for n in GRAM_OK], None) == EALIGN
    for edge in (dict(n_pen=0), dict(n_pen=9), dict(lam=0.0), dict(Da=4097, ldg=4097, ldc=4097), dict(C=4096, ldb=4096, ldw=4096)):
        a = dict(SOLVE_OK, W=X + 4, **edge)
        assert lib().dv_ridge_solve_f64(*[a[n] for n in SOLVE_OK], None) == EALIGN, edge


def test_workspace_query():
    """8 P (T (T + 1) / 2 * 64^2 + C Da): P slabs of q * 512 rows, q = ceil(ceil(n / 512) / 8), T = ceil(Da / 64)"""
    def ws(n, D, C):
        return lib().dv_ridge_gram_workspace(n, D, C)
    for bad in ((0, 8, 3), (-1, 8, 3), (5, 0, 3), (5, 4097, 3), (5, 8, 0), (5, 8, 4097)):
        assert ws(*bad) == EINVAL, bad
    assert ws(1, 1, 1) == 8 * (4096 + 2) and ws(512, 63, 2) == 8 * (4096 + 128) and ws(513, 64, 2) == 8 * 2 * (3 * 4096 + 130)
    assert R.slab_cut(4096) == (512, 8) and R.slab_cut(4097) == (1024, 5) and R.slab_cut(95370) == (12288, 8)
    for n, D, C in ((1, 1, 1), (5, 3, 2), (518, 37, 7), (1076, 129, 17), (4096, 512, 101), (4097, 512, 101), (95370, 512, 101),
                    (95370, 2048, 101), (2 ** 31 - 1, 4096, 4096)):
        assert ws(n, D, C) == R.gram_workspace_bytes(n, D, C) and ws(n, D, C) % 8 == 0, (n, D, C)
    assert ws(95370, 2048, 101) < 160 * 2 ** 20              # modest: the slab count is capped


# ------------------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize('n,D,C,lam', [(40, 7, 3, 0.5), (30, 12, 4, 1e-3), (600, 5, 2, 2.0)])
def test_reference_against_least_squares(n, D, C, lam):
    """the normal equations of the reference solve  min |Z~ W - Y|^2 + lam |W[:D]|^2: the stacked system [Z~; sqrt(lam) I_pen]"""
    rng = np.random.RandomState(n)
    z = rng.randn(n, D).astype(np.float32)
    label = rng.randint(-1, C + 1, size=n)                    # -1 and C: rows that are skipped
    G, B = R.gram_ref(z, label, C)
    live = (label >= 0) & (label < C)
    zt = R.augment(z[live])
    Y = np.eye(C)[label[live]]
    assert np.abs(G - zt.T @ zt).max() < 1e-12 * n and np.abs(B - zt.T @ Y).max() < 1e-12 * n
    assert G[D, D] == live.sum() and (B[D] == np.bincount(label[live], minlength=C)).all()
    pen = np.concatenate([np.sqrt(lam) * np.eye(D), np.zeros((D, 1))], axis=1)
    want = np.linalg.lstsq(np.concatenate([zt, pen]), np.concatenate([Y, np.zeros((D, C))]), rcond=None)[0]
    got = R.solve_ref(G, B, lam, D)
    assert np.abs(got - want).max() < 1e-10
    # a skipped row may hold anything
    z2 = z.copy()
    z2[~live] = np.nan
    G2, B2 = R.gram_ref(z2, label, C)
    assert (G2 == G).all() and (B2 == B).all()


def test_holdout_mask_hand_cases():
    from dualvar_amd.utils.probe import holdout_mask
    # round-robin classes: index % 5 would remove class 4 whole and nothing else; the stratified mask takes one in five of each
    cls = np.arange(50) % 5
    m = holdout_mask(cls, 5).numpy()
    assert (np.flatnonzero(m) == np.arange(20, 25).tolist() + np.arange(45, 50).tolist()).all()
    assert all(m[cls == c].sum() == 2 for c in range(5))
    assert set(cls[np.arange(50) % 5 == 4]) == {4}            # the aliasing the plain rule would have
    # class by class: 7, 4 and 10 videos -> one, none, two
    cls = np.repeat([2, 0, 1], [7, 4, 10])
    m = holdout_mask(torch.from_numpy(cls), 5).numpy()
    assert np.flatnonzero(m).tolist() == [4, 15, 20]
    assert m[cls == 0].sum() == 0
    assert holdout_mask([3, 3, 3, 3], 2).tolist() == [False, True, False, True]
    assert holdout_mask([], 5).tolist() == []
    rng = np.random.RandomState(0)
    for every in (2, 3, 5):
        cls = rng.randint(0, 6, size=97)
        assert (holdout_mask(cls, every).numpy() == R.holdout_mask_ref(cls, every)).all()
    with pytest.raises(ValueError):
        holdout_mask([0, 1], 1)


def test_the_fixture_of_the_gpu_test():
    """the facts tests/test_ridge_gpu.py relies on, from the float64 reference alone: with all 60 videos as the training set the
    stratified hold-out takes 12, the video-level sweep reads 0.417 0.417 0.5 0.667 1.0 0.917 and lambda = 1e-2 wins alone; in
    both settings every score row keeps more than 20 times the fp32 GEMM element bound between the target and its nearest rival"""
    clips, label = R.probe_fixture()
    clips, label = clips.numpy(), label.numpy()
    rep = R.probe_ref(clips, label, clips[40:], label[40:], 6)
    assert rep['n_held_videos'] == 12 and rep['lambda'] == 1e-2
    assert [round(s['video_top1'], 3) for s in rep['sweep']] == [0.417, 0.417, 0.5, 0.667, 1.0, 0.917]
    rep40 = R.probe_ref(clips[:40], label[:40], clips[40:], label[40:], 6)
    assert rep40['n_held_videos'] == 6
    for r in (rep, rep40):
        assert min(float((m / b).min()) for m, b in r['margins']) > 20


# ------------------------------------------------------------------------------------------------------- no GPU, no result
def test_host_entries_raise_without_a_gpu(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import probe as PR
    asked = []
    monkeypatch.setattr(_lib, 'require_device', lambda: asked.append(1))
    z = torch.zeros(20, 8)
    with pytest.raises(ValueError, match='DV_RIDGE_MAX_D'):
        PR.ridge_systems(torch.zeros(4, 4097), torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match='one entry per row'):
        PR.ridge_systems(z, torch.zeros(19), torch.zeros(20))
    with pytest.raises(ValueError, match='DV_RIDGE_MAX_C'):
        PR.ridge_systems(z, torch.zeros(20), torch.zeros(20), n_class=4097)
    with pytest.raises(ValueError, match='float64'):
        PR.ridge_solve(torch.zeros(9, 9), torch.zeros(9, 3), 1.0, 8)
    with pytest.raises(ValueError, match='finite'):
        PR.ridge_solve(torch.zeros(9, 9, dtype=torch.float64), torch.zeros(9, 3, dtype=torch.float64), -1.0, 8)
    with pytest.raises(ValueError, match=r'D \+ 1'):
        PR.ridge_scores(z, torch.zeros(8, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='positive and finite'):
        PR.ridge_probe(torch.zeros(4, 2, 8), torch.zeros(4), torch.zeros(2, 2, 8), torch.zeros(2), 3, lambdas=(0.0,))
    with pytest.raises(ValueError, match='V, S, D'):
        PR.ridge_probe(torch.zeros(4, 8), torch.zeros(4), torch.zeros(2, 2, 8), torch.zeros(2), 3)
    assert not asked
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, '_device_ok', False)
    g, b = torch.zeros(9, 9, dtype=torch.float64), torch.zeros(9, 3, dtype=torch.float64)
    with pytest.raises(_lib.DualVarHipError):
        PR.ridge_systems(z, torch.zeros(20), torch.zeros(20), n_class=3)
    with pytest.raises(_lib.DualVarHipError):
        PR.ridge_solve(g, b, 1.0, 8)
    with pytest.raises(_lib.DualVarHipError):
        PR.ridge_scores(z, b)
    with pytest.raises(_lib.DualVarHipError):
        PR.ridge_probe(torch.zeros(4, 2, 8), torch.zeros(4), torch.zeros(2, 2, 8), torch.zeros(2), 3)


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_ridge_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --ridge --ridge_lambda 0.5 1e-3 --ridge_holdout 4'))
    assert a.ridge is True and a.ridge_lambda == [0.5, 1e-3] and a.ridge_holdout == 4
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.ridge is False and tuple(d.ridge_lambda) == R.LAMBDAS and d.ridge_holdout == 5
    CLI.check_args(d, environ={})
    for ok in (' --ridge', ' --ridge --ridge_holdout 2', ' --ridge --ridge_lambda 1', ' --ridge --knn --variance --tsne --cluster'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --ridge', '--ridge'),                                        # --ridge alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --ridge', '--ridge'),
    (RETRIEVAL + ' --ridge --ridge_lambda 0', '--ridge_lambda'),
    (RETRIEVAL + ' --ridge --ridge_lambda 1e-3 -1', '--ridge_lambda'),
    (RETRIEVAL + ' --ridge --ridge_lambda inf', '--ridge_lambda'),
    (RETRIEVAL + ' --ridge --ridge_lambda nan', '--ridge_lambda'),
    (RETRIEVAL + ' --ridge --ridge_lambda', '--ridge_lambda'),                  # an empty grid
    (RETRIEVAL + ' --ridge --ridge_holdout 1', '--ridge_holdout'),
])
def test_ridge_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))


def test_only_the_ridge_branch_writes_ridge_files(tmp_path, monkeypatch):
    """every '_ridge' file name is formed inside write_ridge, write_ridge is called from one place, under `if args.ridge:`, and
    nothing else in the driver reads a ridge flag but check_args; with the probe stubbed write_ridge writes its two files"""
    import classifier as CLI
    from dualvar_amd.utils import probe as PR
    src = open(os.path.join(ROOT, 'classifier.py')).read()
    tree = ast.parse(src)
    funcs = {f.name: f for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}
    lo, hi = funcs['write_ridge'].lineno, funcs['write_ridge'].end_lineno
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and '_ridge' in node.value and not node.value.startswith('--'):
            assert lo <= node.lineno <= hi, (node.lineno, node.value)
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'id', None) == 'write_ridge']
    assert len(calls) == 1
    guards = [n for n in ast.walk(funcs['test_retrieval']) if isinstance(n, ast.If) and ast.unparse(n.test) == 'args.ridge']
    assert len(guards) == 1 and guards[0].lineno < calls[0].lineno <= guards[0].end_lineno
    users = {n for n, f in funcs.items() for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr.startswith('ridge')}
    assert users == {'check_args', 'test_retrieval', 'write_ridge'}, users
    # in test_retrieval the flag is read twice: to keep the clip features and to enter the branch
    reads = [a for a in ast.walk(funcs['test_retrieval']) if isinstance(a, ast.Attribute) and a.attr.startswith('ridge')]
    assert sorted(a.attr for a in reads) == ['ridge', 'ridge'], [a.attr for a in reads]

    seen = {}

    def stub(train_clips, train_label, test_clips, test_label, n_class, **kw):
        seen.update(kw, n_class=n_class, shapes=(tuple(train_clips.shape), tuple(test_clips.shape)))
        sweep = [{'lambda': v, 'clip_top1': 0.5, 'clip_top5': 1.0, 'video_top1': 0.5, 'video_top5': 1.0} for v in kw['lambdas']]
        return {'lambda': kw['lambdas'][-1], 'sweep': sweep, 'clip_top1': 0.25, 'clip_top5': 0.75, 'video_top1': 0.5,
                'video_top5': 1.0, 'n_train': 60, 'n_fit': 50, 'n_held_videos': 1, 'n_class': n_class, 'D': 8,
                'W': torch.ones(9, n_class, dtype=torch.float64)}
    monkeypatch.setattr(PR, 'ridge_probe', stub)
    args = types.SimpleNamespace(num_class=3, ridge_lambda=[1e-3, 1e-2], ridge_holdout=4, dataset='ucf101',
                                 logger=logging.getLogger('test_ridge_host'))
    CLI.write_ridge(torch.zeros(6, 10, 8), torch.tensor([0, 1, 2, 0, 1, 2]), torch.zeros(3, 10, 8), torch.tensor([0, 1, 2]),
                    str(tmp_path), args)
    assert sorted(os.listdir(str(tmp_path))) == ['ucf101_ridge.json', 'ucf101_ridge.pth.tar']
    assert seen == dict(lambdas=(1e-3, 1e-2), holdout=4, n_class=3, shapes=((6, 10, 8), (3, 10, 8)))
    rep = json.load(open(str(tmp_path / 'ucf101_ridge.json')))
    assert (rep['lambda'], rep['video_top1'], rep['n_train'], len(rep['sweep'])) == (1e-2, 0.5, 60, 2) and 'W' not in rep
    saved = torch.load(str(tmp_path / 'ucf101_ridge.pth.tar'), weights_only=True)
    assert saved['W'].shape == (9, 3) and saved['W'].dtype == torch.float64 and saved['lambda'] == 1e-2
