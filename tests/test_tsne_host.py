"""CPU: the t-SNE entries (include/dualvar_tsne.h) agree with their ctypes table, the library's exports and the ledger below and
refuse every bad argument of their header comments before any launch; the float64 reference of tests/tsne_reference.py is itself
checked (its gradient against central finite differences of its own KL); the reverse-list builder of dualvar_amd/utils/embed.py
against brute force; classifier.py parses and checks the --tsne flags; without a GPU every host entry raises DualVarHipError."""
import ast
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
from tests import tsne_reference as R
from tests.checks import lib
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it
INF = math.inf

# The coverage ledger of include/dualvar_tsne.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.TSNE_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
TSNE_COVERAGE = {
    'dv_tsne_perplexity_f32': ('test_tsne_gpu.py', A.FLOAT64),
    'dv_tsne_attract_f32': ('test_tsne_gpu.py', A.FLOAT64),
    'dv_tsne_repulse_workspace': ('test_tsne_host.py', A.HOST_QUERY),
    'dv_tsne_repulse_f32': ('test_tsne_gpu.py', A.FLOAT64),
    'dv_tsne_update_f32': ('test_tsne_gpu.py', A.FLOAT64),
}


def test_tsne_header_table_and_library_agree():
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_tsne.h')
    assert set(decl) == set(_lib.TSNE_SIGNATURES) == set(TSNE_COVERAGE) and len(decl) == 5
    assert 'tsne.hip' in build.SOURCES
    for macro, want in (('DV_TSNE_BETA_START', R.BETA_START), ('DV_TSNE_MAX_STEPS', R.MAX_STEPS), ('DV_TSNE_ENTROPY_TOL', R.ENTROPY_TOL)):
        assert float(re.search(r'#define\s+%s\s+([0-9.e+-]+)' % macro, hdr).group(1)) == want, macro
    for name, (fname, kind) in TSNE_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"ops\.call\('%s'|lib\.%s\(|lib\(\)\.%s\(" % (name, name, name), open(os.path.join(ROOT, 'tests', fname)).read()), \
            '%s is not called by tests/%s' % (name, fname)


PERP_OK = dict(top_val=X, top_idx=X, ldk=8, n=5, k1=8, row0=0, perplexity=2.0, p=X, beta=X)
PERP_BAD = [dict(top_val=None), dict(top_idx=None), dict(p=None), dict(beta=None), dict(n=0), dict(n=-1), dict(k1=0), dict(k1=257, ldk=300),
            dict(ldk=7), dict(n=2 ** 24, ldk=128, k1=128), dict(row0=-1), dict(row0=2 ** 31 - 3), dict(perplexity=0.5),
            dict(perplexity=INF), dict(perplexity=math.nan)]
ATTR_OK = dict(y=X, top_idx=X, p=X, ldk=8, n=5, k1=8, rev_ptr=X, rev_edge=X, E=3, fa=X, ce_row=X, ce_sum=X)
ATTR_BAD = [dict(y=None), dict(top_idx=None), dict(p=None), dict(rev_ptr=None), dict(rev_edge=None), dict(fa=None), dict(ce_row=None),
            dict(n=0), dict(n=2 ** 24 + 1, ldk=1, k1=1), dict(k1=0), dict(k1=257, ldk=257), dict(ldk=7), dict(n=2 ** 24, ldk=128, k1=8),
            dict(E=-1)]
ATTR_MIS = [dict(y=X + 4), dict(fa=X + 4), dict(ce_sum=X + 4)]
UPD_OK = dict(y=X, vel=X, gain=X, fa=X, fr=X, Z=X, m=10, exaggeration=12.0, momentum=0.5, lr=50.0, min_gain=0.01)
UPD_BAD = [dict(y=None), dict(vel=None), dict(gain=None), dict(fa=None), dict(fr=None), dict(Z=None), dict(m=0), dict(m=-2),
           dict(exaggeration=INF), dict(exaggeration=math.nan), dict(momentum=-0.1), dict(momentum=INF), dict(lr=-1.0), dict(lr=math.nan),
           dict(min_gain=-0.01), dict(min_gain=INF)]
_ids = lambda d: ','.join('%s=%s' % kv for kv in d.items())       # noqa: E731


@pytest.mark.parametrize('bad', PERP_BAD, ids=_ids)
def test_perplexity_refuses_without_gpu(bad):
    a = dict(PERP_OK, **bad)
    assert lib().dv_tsne_perplexity_f32(*[a[n] for n in PERP_OK], None) == EINVAL


@pytest.mark.parametrize('bad', ATTR_BAD + ATTR_MIS, ids=_ids)
def test_attract_refuses_without_gpu(bad):
    a = dict(ATTR_OK, **bad)
    assert lib().dv_tsne_attract_f32(*[a[n] for n in ATTR_OK], None) == (EALIGN if bad in ATTR_MIS else EINVAL)


@pytest.mark.parametrize('bad', UPD_BAD + [dict(Z=X + 4)], ids=_ids)
def test_update_refuses_without_gpu(bad):
    a = dict(UPD_OK, **bad)
    assert lib().dv_tsne_update_f32(*[a[n] for n in UPD_OK], None) == (EALIGN if 'Z' in bad and bad['Z'] else EINVAL)


def test_repulse_refusals_and_workspace_query():
    """S = min(T, ceil(1024 / B)) with T = B = ceil(n / 256); bytes = 24 n S + 8 B; a function of n only"""
    import ctypes
    f = lib().dv_tsne_repulse_f32

    def ws(n, parts):
        return lib().dv_tsne_repulse_workspace(n, parts)
    for bad in ((None, 5, X, X, X), (X, 5, None, X, X), (X, 5, X, None, X), (X, 5, X, X, None), (X, 0, X, X, X), (X, -1, X, X, X)):
        assert f(*bad, None) == EINVAL, bad
    for bad in ((X + 4, 5, X, X, X), (X, 5, X + 4, X, X), (X, 5, X, X + 4, X), (X, 5, X, X, X + 4)):
        assert f(*bad, None) == EALIGN, bad
    assert ws(0, None) < 0 and ws(-3, None) < 0
    for n, S in ((1, 1), (256, 1), (257, 2), (300, 2), (513, 3), (3000, 12), (8192, 32), (8193, 32), (37830, 7), (95370, 3), (2 ** 24, 1)):
        parts = ctypes.c_int32(-1)
        B = -(-n // 256)
        assert S == min(B, -(-1024 // B))
        assert ws(n, ctypes.byref(parts)) == 24 * n * S + 8 * B == ws(n, None) and parts.value == S, n


# ------------------------------------------------------------------------------------------------- the reference itself
def small_problem(n=12, k=5, seed=0):
    rng = np.random.RandomState(seed)
    z = rng.randn(n, 6)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    s = (z @ z.T).astype(np.float32)
    idx = np.argsort(-s, axis=1, kind='stable')[:, :k + 1]
    val = np.take_along_axis(s, idx, 1)
    p, beta = R.perplexity_ref(val, idx, 3.0)
    return idx, p, R.sparse_P(idx, p, n), rng.randn(n, 2)


def test_reference_gradient_equals_finite_differences_of_its_kl():
    idx, p, P, y = small_problem()
    n = P.shape[0]
    assert abs(P.sum() - 1.0) < 1e-12 and np.allclose(P, P.T) and (np.diag(P) == 0).all()
    assert np.allclose(p.sum(1), 1.0, atol=1e-12)
    g, Z, ce = R.gradient(P, y)
    (fa, ce_row, _), (fr, Z2, _) = R.attraction(P, y), R.repulsion(y)      # the term-by-term form the GPU tests take their bounds from
    assert np.abs(g - 4.0 * (fa - fr / Z2)).max() < 1e-13 and abs(Z - Z2) < 1e-12 and abs(ce - ce_row.sum() - math.log(Z2)) < 1e-12
    h = 1e-5
    fd = np.zeros_like(y)
    for i in range(n):
        for c in range(2):
            yp, ym = y.copy(), y.copy()
            yp[i, c] += h
            ym[i, c] -= h
            fd[i, c] = (R.kl(P, yp) - R.kl(P, ym)) / (2 * h)
    assert np.abs(g - fd).max() <= 1e-6 * np.abs(g).max(), (np.abs(g - fd).max(), np.abs(g).max())
    # CE = KL + H(P): the entropy of P does not depend on the map
    m = P > 0
    assert abs(ce - (R.kl(P, y) - (P[m] * np.log(P[m])).sum())) < 1e-12


def test_reference_bisection_meets_the_perplexity():
    idx, p, P, y = small_problem(n=40, k=12, seed=3)
    H = -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(1)
    assert np.abs(H - math.log(3.0)).max() <= R.ENTROPY_TOL + 1e-6
    # nothing included, all equal, perplexity above the list: the header's special rows
    val = np.array([[1.0, -np.inf, -np.inf], [1.0, 0.5, 0.5], [1.0, 0.9, 0.1]], dtype=np.float32)
    ix = np.array([[0, -1, -1], [1, 0, 2], [2, 0, 1]])
    p, beta = R.perplexity_ref(val, ix, 5.0)
    assert (p[0] == 0).all() and beta[0] == 0.0
    assert p[1].tolist() == [0.0, 0.5, 0.5] and beta[1] == R.BETA_START
    assert p[2, 0] == 0 and abs(p[2, 1] - 0.5) < 1e-6 and beta[2] == 2.0 ** -(R.MAX_STEPS - 1)


def test_reverse_csr_against_brute_force():
    """row 0 is a hub (everybody lists it), row 5 is listed by nobody, row 3 lists itself in slot 2 and a -1; a pitch beyond k"""
    from dualvar_amd.utils.embed import reverse_csr
    idx = torch.tensor([[0, 1, 2, 9], [1, 0, 2, 9], [0, 2, 1, 9], [0, 1, 3, -1], [4, 0, -1, -1], [0, 5, 4, 3], [0, 6, 6, 1]])
    n = idx.shape[0]
    inc = (idx >= 0) & (idx != torch.arange(n)[:, None])
    inc[:, 3] &= idx[:, 3] < n                                              # the 9s of the padding column are not included
    ptr, edge = reverse_csr(idx, inc)
    bptr, bedge = R.reverse_csr_brute(idx.numpy(), inc.numpy())
    assert ptr.dtype == torch.int32 and edge.dtype == torch.int32
    assert ptr.tolist() == bptr.tolist() and edge.tolist() == bedge.tolist()
    assert ptr[1] - ptr[0] == 6 and ptr[6] - ptr[5] == 0 and int(ptr[-1]) == int(inc.sum())
    for i in range(n):                   # ascending flat position within a row; every edge points at its row
        e = edge[ptr[i]:ptr[i + 1]]
        assert bool((e[1:] > e[:-1]).all()) and bool((idx.reshape(-1)[e.long()] == i).all())


# ------------------------------------------------------------------------------------------------------- no GPU, no result
def test_host_entries_raise_without_a_gpu(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import embed as E
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, '_device_ok', False)
    f = torch.zeros(20, 8)
    with pytest.raises(_lib.DualVarHipError):
        E.tsne_affinities(f, 3)
    with pytest.raises(_lib.DualVarHipError):
        E.tsne_embed(f, perplexity=3, n_iter=2)
    with pytest.raises(_lib.DualVarHipError):
        E.affinities_from_lists(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32), 2)
    with pytest.raises(_lib.DualVarHipError):
        E.embedding_report(torch.zeros(20, 2), torch.zeros(20), torch.zeros(20), torch.zeros(20, 11, dtype=torch.int32))
    with pytest.raises(_lib.DualVarHipError):
        E.tsne_eval(torch.zeros(2, 10, 8), torch.zeros(2), perplexity=3, n_iter=2)
    # what is refused before the device is asked for
    for bad in (1, 1.5, 86, math.nan):
        with pytest.raises(ValueError, match='perplexity'):
            E.tsne_affinities(f, bad)
    with pytest.raises(ValueError, match='n, D'):
        E.tsne_embed(torch.zeros(1, 8))
    with pytest.raises(ValueError, match='n_video, num_seq, D'):
        E.tsne_eval(f, torch.zeros(20))


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_tsne_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --tsne --tsne_perplexity 5 --tsne_iter 60 --tsne_seed 3 --tsne_split both'))
    assert a.tsne is True and (a.tsne_perplexity, a.tsne_iter, a.tsne_seed, a.tsne_split) == (5, 60, 3, 'both')
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.tsne is False and (d.tsne_perplexity, d.tsne_iter, d.tsne_seed, d.tsne_split) == (30, 1000, 0, 'test')
    CLI.check_args(d, environ={})
    for ok in (' --tsne --tsne_perplexity 2', ' --tsne --tsne_perplexity 85', ' --tsne --tsne_iter 1', ' --tsne --knn --variance',
               ' --tsne --tsne_split train'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --tsne', '--tsne'),                                          # --tsne alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --tsne', '--tsne'),
    (RETRIEVAL + ' --tsne --tsne_perplexity 1', '--tsne_perplexity'),
    (RETRIEVAL + ' --tsne --tsne_perplexity 86', '--tsne_perplexity'),
    (RETRIEVAL + ' --tsne --tsne_iter 0', '--tsne_iter'),
])
def test_tsne_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))


def test_only_the_tsne_branch_writes_tsne_files():
    """without --tsne the files written and the log are what they were: every '_tsne' file name is formed inside write_tsne,
    write_tsne is called from one place, under `if args.tsne:`, and nothing else in the driver reads a tsne flag but check_args"""
    src = open(os.path.join(ROOT, 'classifier.py')).read()
    tree = ast.parse(src)
    funcs = {f.name: f for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}
    span = lambda f: (f.lineno, f.end_lineno)                                # noqa: E731
    lo, hi = span(funcs['write_tsne'])
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and '_tsne' in node.value and not node.value.startswith('--'):
            assert lo <= node.lineno <= hi, (node.lineno, node.value)
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'id', None) == 'write_tsne']
    assert len(calls) == 1
    guards = [n for n in ast.walk(funcs['test_retrieval']) if isinstance(n, ast.If) and ast.unparse(n.test) == 'args.tsne']
    assert len(guards) == 1 and guards[0].lineno < calls[0].lineno <= guards[0].end_lineno
    users = {n for n, f in funcs.items() for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr.startswith('tsne')}
    assert users == {'check_args', 'test_retrieval', 'write_tsne'}, users
    # in test_retrieval the flag is read twice: to keep the clip features and to enter the branch
    reads = [a for a in ast.walk(funcs['test_retrieval']) if isinstance(a, ast.Attribute) and a.attr.startswith('tsne')]
    assert sorted(a.attr for a in reads) == ['tsne', 'tsne', 'tsne_split', 'tsne_split'], [a.attr for a in reads]
