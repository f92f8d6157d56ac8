"""CPU: the k-means entries (include/dualvar_cluster.h) agree with their ctypes table, the library's exports and the ledger below
and refuse every bad argument of their header comments before any launch; the two workspace queries return what the header
says; cluster_metrics of dualvar_amd/utils/cluster.py against the float64 reference of tests/cluster_reference.py (itself
checked against brute force over all permutations) and, where it imports, against scikit-learn; classifier.py parses and checks
the --cluster flags and only that branch writes the _cluster files; without a GPU every host entry raises DualVarHipError."""
import ast
import itertools
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
from tests import cluster_reference as R
from tests.checks import lib
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
X = 4096                 # stands for a non-null (8-byte aligned) pointer: a refused call never dereferences it

# The coverage ledger of include/dualvar_cluster.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.CLUSTER_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).
CLUSTER_COVERAGE = {
    'dv_kmeans_assign_f32': ('test_cluster_gpu.py', A.FLOAT64),
    'dv_kmeans_update_workspace': ('test_cluster_host.py', A.HOST_QUERY),
    'dv_kmeans_update_f32': ('test_cluster_gpu.py', A.FLOAT64),
    'dv_kmeans_dot_f32': ('test_cluster_gpu.py', A.FLOAT64),
    'dv_kmeans_seed_workspace': ('test_cluster_host.py', A.HOST_QUERY),
    'dv_kmeans_seed_f32': ('test_cluster_gpu.py', A.FLOAT64),
}


def test_cluster_header_table_and_library_agree():
    from dualvar_amd import _lib, build
    hdr, decl = check_header_binding('dualvar_cluster.h')
    assert set(decl) == set(_lib.CLUSTER_SIGNATURES) == set(CLUSTER_COVERAGE) and len(decl) == 6
    assert 'cluster.hip' in build.SOURCES
    for macro, want in (('DV_KMEANS_MAX_K', R.MAX_K), ('DV_KMEANS_PART', R.PART), ('DV_KMEANS_SORT_ROWS', R.SORT_ROWS),
                        ('DV_KMEANS_SEED_BLOCK', R.SEED_BLOCK)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == want, macro
    assert _lib.DV_KMEANS_MAX_K == R.MAX_K
    for name, (fname, kind) in CLUSTER_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r"lib\.%s\(|lib\(\)\.%s\(" % (name, name), open(os.path.join(ROOT, 'tests', fname)).read()), \
            '%s is not called by tests/%s' % (name, fname)


ASSIGN_OK = dict(sim=X, ld=8, R=5, K=8, assign=X, best=X, changed=X)
ASSIGN_BAD = [dict(sim=None), dict(assign=None), dict(best=None), dict(changed=None), dict(R=0), dict(R=-1), dict(K=0),
              dict(K=4097, ld=5000), dict(ld=7)]
UPDATE_OK = dict(z=X, ldz=8, n=5, D=8, assign=X, best=X, K=3, cent_in=X, cent_out=X, ldc=8, counts=X, within=X, workspace=X)
UPDATE_BAD = [dict(z=None), dict(assign=None), dict(best=None), dict(cent_in=None), dict(cent_out=None), dict(counts=None),
              dict(within=None), dict(workspace=None), dict(n=0), dict(n=-4), dict(D=0), dict(K=0), dict(K=4097), dict(ldz=7), dict(ldc=7)]
UPDATE_MIS = [dict(within=X + 4), dict(workspace=X + 4)]
SEED_OK = dict(s=X, n=5, mind=X, first=1, u=0.5, pick=X, total=X, workspace=X)
SEED_BAD = [dict(s=None), dict(mind=None), dict(pick=None), dict(total=None), dict(workspace=None), dict(n=0), dict(n=-1),
            dict(u=-1e-9), dict(u=1.0), dict(u=math.nan), dict(u=math.inf)]
SEED_MIS = [dict(total=X + 4), dict(workspace=X + 4)]
_ids = lambda d: ','.join('%s=%s' % kv for kv in d.items())       # noqa: E731


@pytest.mark.parametrize('bad', ASSIGN_BAD + [dict(changed=X + 4)], ids=_ids)
def test_assign_refuses_without_gpu(bad):
    a = dict(ASSIGN_OK, **bad)
    assert lib().dv_kmeans_assign_f32(*[a[n] for n in ASSIGN_OK], None) == (EALIGN if bad.get('changed') else EINVAL)


@pytest.mark.parametrize('bad', UPDATE_BAD + UPDATE_MIS, ids=_ids)
def test_update_refuses_without_gpu(bad):
    a = dict(UPDATE_OK, **bad)
    assert lib().dv_kmeans_update_f32(*[a[n] for n in UPDATE_OK], None) == (EALIGN if bad in UPDATE_MIS else EINVAL)


@pytest.mark.parametrize('bad', [dict(z=None), dict(c=None), dict(s=None), dict(n=0), dict(n=-1), dict(D=0), dict(ldz=7)], ids=_ids)
def test_dot_refuses_without_gpu(bad):
    a = dict(dict(z=X, ldz=8, n=5, D=8, c=X, s=X), **bad)
    assert lib().dv_kmeans_dot_f32(*[a[n] for n in ('z', 'ldz', 'n', 'D', 'c', 's')], None) == EINVAL


@pytest.mark.parametrize('bad', SEED_BAD + SEED_MIS, ids=_ids)
def test_seed_refuses_without_gpu(bad):
    a = dict(SEED_OK, **bad)
    assert lib().dv_kmeans_seed_f32(*[a[n] for n in SEED_OK], None) == (EALIGN if bad in SEED_MIS else EINVAL)


def test_workspace_queries():
    """update: 8 (P D + P + K D) + 4 (B K + 2 (K + 1) + n) rounded up to 8, P = n / 64 + K, B = ceil(n / 512); seed: 8 ceil(n / 256)"""
    def up(n, D, K):
        return lib().dv_kmeans_update_workspace(n, D, K)

    def sd(n):
        return lib().dv_kmeans_seed_workspace(n)
    for bad in ((0, 8, 3), (-1, 8, 3), (5, 0, 3), (5, 8, 0), (5, 8, 4097)):
        assert up(*bad) == EINVAL, bad
    assert sd(0) == EINVAL and sd(-7) == EINVAL
    assert up(1, 1, 1) == 8 * (1 + 1 + 1) + 4 * (1 + 4 + 1) and sd(1) == 8 and sd(256) == 8 and sd(257) == 16
    for n, D, K in ((1, 1, 1), (5, 3, 3), (1000, 130, 101), (5000, 512, 1), (37830, 512, 101), (37830, 512, 4096), (2 ** 31 - 1, 512, 4096)):
        assert up(n, D, K) == R.update_workspace_bytes(n, D, K) and up(n, D, K) % 8 == 0, (n, D, K)
        assert sd(n) == R.seed_workspace_bytes(n), n


# ------------------------------------------------------------------------------------------------------------ the scores
def test_hungarian_against_all_permutations():
    from dualvar_amd.utils.cluster import best_matching
    rng = np.random.RandomState(0)
    for K, C in itertools.product(range(1, 7), range(1, 7)):
        for trial in range(3):
            t = rng.randint(0, 9, size=(K, C)).astype(np.float64)
            if trial == 2:
                t[rng.rand(K, C) < 0.5] = 0                                  # many ties
            if t.sum() == 0:
                t[0, 0] = 1
            got, pairs = best_matching(t)
            assert got / t.sum() == R.accuracy_brute(t), (K, C, t)
            assert len(pairs) == min(K, C) and len({k for k, _ in pairs}) == len({c for _, c in pairs}) == len(pairs)
            assert got == sum(t[k, c] for k, c in pairs)


def test_hungarian_on_a_wide_table():
    """101 classes against 300 clusters with a planted one-to-one map: the match finds it"""
    from dualvar_amd.utils.cluster import best_matching
    rng = np.random.RandomState(1)
    t = rng.randint(0, 5, size=(300, 101)).astype(np.float64)
    rows = rng.permutation(300)[:101]
    t[rows, np.arange(101)] += 50
    got, pairs = best_matching(t)
    assert sorted(pairs) == sorted((int(r), c) for c, r in enumerate(rows)) and got == t[rows, np.arange(101)].sum()


def test_metrics_perfect_partition_up_to_relabelling():
    from dualvar_amd.utils.cluster import cluster_metrics
    cls = np.repeat(np.arange(5), [3, 1, 7, 2, 4])
    assign = np.array([3, 0, 4, 1, 2])[cls]
    rep = cluster_metrics(assign, cls, vid=np.arange(cls.size) // 2)
    assert rep['nmi'] == pytest.approx(1.0, abs=1e-15) and rep['ari'] == 1.0 and rep['purity'] == 1.0 and rep['accuracy'] == 1.0
    assert sorted(rep['sizes']) == [1, 2, 3, 4, 7] and rep['n'] == 17 and rep['unassigned'] == 0


def test_metrics_one_cluster():
    from dualvar_amd.utils.cluster import cluster_metrics
    cls = np.repeat(np.arange(4), 5)
    rep = cluster_metrics(np.zeros(20, dtype=np.int64), cls, vid=np.arange(20) // 10)
    assert rep['nmi'] == 0.0 and rep['ari'] == 0.0 and rep['purity'] == 0.25 and rep['accuracy'] == 0.25
    assert rep['video_consistency'] == 1.0 and rep['sizes'] == [20]
    both = cluster_metrics(np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64))       # one cluster, one class
    assert both['nmi'] == 1.0 and both['ari'] == 1.0


def random_labels(seed, n, K, C):
    rng = np.random.RandomState(seed)
    cls = rng.randint(0, C, size=n)
    assign = np.where(rng.rand(n) < 0.6, cls % K, rng.randint(0, K, size=n))
    return assign, cls


@pytest.mark.parametrize('seed,n,K,C', [(0, 30, 3, 3), (1, 60, 6, 4), (2, 60, 4, 6), (3, 200, 5, 5), (4, 17, 2, 6)])
def test_metrics_against_the_reference(seed, n, K, C):
    from dualvar_amd.utils.cluster import cluster_metrics
    assign, cls = random_labels(seed, n, K, C)
    vid = np.arange(n) // 5
    rep = cluster_metrics(torch.from_numpy(assign).int(), torch.from_numpy(cls), vid=vid)
    assert abs(rep['nmi'] - R.nmi_ref(assign, cls)) < 1e-12
    assert abs(rep['ari'] - R.ari_ref(assign, cls)) < 1e-12
    assert abs(rep['purity'] - R.purity_ref(assign, cls)) < 1e-15
    assert abs(rep['accuracy'] - R.accuracy_brute(R.contingency(assign, cls))) < 1e-15
    assert abs(rep['video_consistency'] - R.video_consistency_ref(assign, vid)) < 1e-15
    assert rep['sizes'][:int(assign.max()) + 1] == [int((assign == k).sum()) for k in range(int(assign.max()) + 1)]


def test_metrics_hand_made_table_and_unassigned_rows():
    """[[2, 0], [1, 3]]: purity 5/6, accuracy 5/6, ARI from the pair counts by hand: together 1 + 0 + 0 + 3 = 4, rows 1 + 6, columns
    3 + 3, all 15 -> (4 - 7 * 6 / 15) / (6.5 - 2.8)"""
    from dualvar_amd.utils.cluster import cluster_metrics
    assign, cls = np.array([0, 0, 1, 1, 1, 1]), np.array([0, 0, 0, 1, 1, 1])
    rep = cluster_metrics(assign, cls)
    assert rep['purity'] == 5 / 6 and rep['accuracy'] == 5 / 6 and abs(rep['ari'] - (4 - 2.8) / (6.5 - 2.8)) < 1e-15
    h = lambda ps: -sum(p * math.log(p) for p in ps if p > 0)      # noqa: E731
    mi = h([1 / 3, 2 / 3]) + h([0.5, 0.5]) - h([2 / 6, 1 / 6, 3 / 6])
    assert abs(rep['nmi'] - mi / (0.5 * (h([1 / 3, 2 / 3]) + h([0.5, 0.5])))) < 1e-14
    # rows without a cluster are left out of the table and count against their video
    rep = cluster_metrics(np.array([0, 0, 1, 1, 1, 1, -1, -1]), np.array([0, 0, 0, 1, 1, 1, 0, 1]), vid=np.array([0, 0, 1, 1, 1, 1, 0, 0]), n_class=4)
    assert rep['n'] == 6 and rep['unassigned'] == 2 and rep['purity'] == 5 / 6 and rep['n_class'] == 4
    assert rep['video_consistency'] == (2 / 4 + 4 / 4) / 2
    with pytest.raises(ValueError):
        cluster_metrics(np.zeros(3), np.zeros(4))


def test_metrics_against_sklearn():
    M = pytest.importorskip('sklearn.metrics')
    from dualvar_amd.utils.cluster import cluster_metrics
    for seed, n, K, C in ((0, 300, 7, 5), (1, 1000, 20, 30), (2, 50, 3, 3)):
        assign, cls = random_labels(seed, n, K, C)
        rep = cluster_metrics(assign, cls)
        assert abs(rep['nmi'] - M.normalized_mutual_info_score(cls, assign)) < 1e-12
        assert abs(rep['ari'] - M.adjusted_rand_score(cls, assign)) < 1e-12


def test_reference_lloyd_recovers_separated_groups():
    """the fixture of test_cluster_gpu.py's fit tests: the reference's own run from one point of each group recovers the groups"""
    x, cls = R.fit_fixture()
    z = R.centre_normalise(x)
    assert x.shape == (300, 32) and np.abs(np.linalg.norm(z, axis=1) - 1).max() < 1e-15
    assign, cent, trace = R.lloyd_ref(z, z[::50])
    wrong = R.lloyd_ref(z, z[[0, 1, 50, 100, 150, 200, 250]])[0]           # seven centres on six groups: the first group is split
    assert set(wrong[:50]) == {0, 1} and (wrong[50:] == cls[50:] + 1).all()
    assert (assign == cls).all() and trace[-1]['changed'] == 0 and len(trace) <= 5
    obj = [t['objective'] for t in trace]
    assert all(b >= a - 1e-12 for a, b in zip(obj, obj[1:]))
    assert np.abs(np.linalg.norm(cent, axis=1) - 1).max() < 1e-14
    # the seeded fit test (seed 0, three restarts): of the runs from k-means++ on these rows with those draws, the one of largest
    # objective recovers the groups (the others need not)
    gen = torch.Generator().manual_seed(0)
    runs = []
    for _ in range(3):
        index = R.kmeanspp_ref(z, 6, gen)
        a, _, t = R.lloyd_ref(z, z[index])
        runs.append((t[-1]['objective'], bool((a[::50][cls] == a).all() and len(set(a[::50])) == 6)))
    assert max(runs)[1] and max(runs)[0] == pytest.approx(obj[-1], abs=1e-9), runs


# ------------------------------------------------------------------------------------------------------- no GPU, no result
def test_host_entries_raise_without_a_gpu(monkeypatch):
    from dualvar_amd import _lib
    from dualvar_amd.utils import cluster as CL
    # what is refused before the device is asked for
    asked = []
    monkeypatch.setattr(_lib, 'require_device', lambda: asked.append(1))
    f = torch.zeros(20, 8)
    with pytest.raises(ValueError, match='DV_KMEANS_MAX_K'):
        CL.kmeans_fit(torch.zeros(5000, 8), 4097)
    with pytest.raises(ValueError, match='DV_KMEANS_MAX_K'):
        CL.kmeans_fit(f, 0)
    with pytest.raises(ValueError, match='clusters for n'):
        CL.kmeans_fit(f, 21)
    with pytest.raises(ValueError, match='device tensors'):
        CL.kmeans_fit(f, 3)
    with pytest.raises(ValueError, match='n, D'):
        CL.kmeans_fit(torch.zeros(20), 3)
    with pytest.raises(ValueError, match='init must be'):
        CL.kmeans_fit(f, 3, init=torch.zeros(4, 8))
    with pytest.raises(ValueError, match='n_iter'):
        CL.kmeans_fit(f, 3, n_iter=0)
    with pytest.raises(ValueError, match='n_video, num_seq, D'):
        CL.cluster_eval(f, torch.zeros(20))
    assert not asked
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, '_device_ok', False)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))       # past the host-tensor check, as a device tensor would be
    with pytest.raises(_lib.DualVarHipError):
        CL.kmeans_fit(f, 3)
    with pytest.raises(_lib.DualVarHipError):
        CL.cluster_eval(torch.zeros(2, 10, 8), torch.zeros(2))


# ------------------------------------------------------------------------------------------------------- classifier.py
RETRIEVAL = ('--model linclr --net r21d --dataset ucf101 --seq_len 16 --batch_size 8 --num_seq 10 -j 8 --gpu 0 --prefix p '
             '--retrieval --ds 4 --test log/x/pretrain/e/model/epoch189.pth.tar')
FINETUNE = '--prefix p --name_prefix e --net r21d --dataset ucf101 --num_seq 1 --split_root s --frame_root f'


def test_parse_args_accepts_the_cluster_flags():
    import classifier as CLI
    a = CLI.parse_args(shlex.split(RETRIEVAL + ' --cluster --cluster_k 20 --cluster_iter 7 --cluster_init 2 --cluster_seed 3 --cluster_split both'))
    assert a.cluster is True and (a.cluster_k, a.cluster_iter, a.cluster_init, a.cluster_seed, a.cluster_split) == (20, 7, 2, 3, 'both')
    CLI.check_args(a, environ={})
    d = CLI.parse_args(shlex.split(RETRIEVAL))
    assert d.cluster is False and (d.cluster_k, d.cluster_iter, d.cluster_init, d.cluster_seed, d.cluster_split) == (0, 100, 10, 0, 'test')
    CLI.check_args(d, environ={})
    for ok in (' --cluster --cluster_k 4096', ' --cluster --cluster_k 1', ' --cluster --cluster_iter 1', ' --cluster --knn --variance --tsne',
               ' --cluster --cluster_split train'):
        CLI.check_args(CLI.parse_args(shlex.split(RETRIEVAL + ok)), environ={})


@pytest.mark.parametrize('argv,word', [
    (FINETUNE + ' --cluster', '--cluster'),                                    # --cluster alone: no --test ... --retrieval
    (RETRIEVAL.replace('--retrieval', '--center_crop').replace('--num_seq 10', '--num_seq 1') + ' --cluster', '--cluster'),
    (RETRIEVAL + ' --cluster --cluster_k 4097', '--cluster_k'),
    (RETRIEVAL + ' --cluster --cluster_k -1', '--cluster_k'),
    (RETRIEVAL + ' --cluster --cluster_iter 0', '--cluster_iter'),
    (RETRIEVAL + ' --cluster --cluster_init 0', '--cluster_init'),
])
def test_cluster_refusals_exit_with_one_line(argv, word):
    e = {k: v for k, v in os.environ.items() if k != 'WORLD_SIZE'}
    e['HIP_VISIBLE_DEVICES'] = e['CUDA_VISIBLE_DEVICES'] = ''               # the child could not open a GPU if it tried
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'classifier.py')] + shlex.split(argv), env=e, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2
    lines = [ln for ln in r.stderr.strip().splitlines() if ln.strip()]
    assert 'Traceback' not in r.stderr and len(lines) == 1 and word in lines[0], r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'log-p'))          # refused before anything was created
    assert not os.path.exists(os.path.join(ROOT, 'log'))


def test_only_the_cluster_branch_writes_cluster_files(tmp_path, monkeypatch):
    """every '_cluster' file name is formed inside write_cluster, write_cluster is called from one place, under `if args.cluster:`,
    and nothing else in the driver reads a cluster flag but check_args; with the fit stubbed write_cluster writes its two files"""
    import classifier as CLI
    from dualvar_amd.utils import cluster as CL
    src = open(os.path.join(ROOT, 'classifier.py')).read()
    tree = ast.parse(src)
    funcs = {f.name: f for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}
    lo, hi = funcs['write_cluster'].lineno, funcs['write_cluster'].end_lineno
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and '_cluster' in node.value and not node.value.startswith('--'):
            assert lo <= node.lineno <= hi, (node.lineno, node.value)
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'id', None) == 'write_cluster']
    assert len(calls) == 1
    guards = [n for n in ast.walk(funcs['test_retrieval']) if isinstance(n, ast.If) and ast.unparse(n.test) == 'args.cluster']
    assert len(guards) == 1 and guards[0].lineno < calls[0].lineno <= guards[0].end_lineno
    users = {n for n, f in funcs.items() for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr.startswith('cluster')}
    assert users == {'check_args', 'test_retrieval', 'write_cluster'}, users
    # in test_retrieval the flag is read twice: to keep the clip features and to enter the branch
    reads = [a for a in ast.walk(funcs['test_retrieval']) if isinstance(a, ast.Attribute) and a.attr.startswith('cluster')]
    assert sorted(a.attr for a in reads) == ['cluster', 'cluster', 'cluster_split', 'cluster_split'], [a.attr for a in reads]

    seen = {}

    def stub(per_feature, label, **kw):
        seen.update(kw)
        n = per_feature.shape[0] * per_feature.shape[1]
        fit = {'assign': torch.arange(n, dtype=torch.int32) % kw['k'], 'centroids': torch.zeros(kw['k'], per_feature.shape[2]),
               'objective': 1.5, 'iterations': 2, 'restart': 1, 'empty': 0, 'init_index': [0, 1, 2], 'sizes': [n // kw['k']] * kw['k'],
               'trace': [{'objective': 1.0, 'changed': n}, {'objective': 1.5, 'changed': 0}]}
        cls = torch.as_tensor(label).repeat_interleave(per_feature.shape[1])
        return fit, CL.cluster_metrics(fit['assign'], cls, vid=torch.arange(per_feature.shape[0]).repeat_interleave(per_feature.shape[1]))
    monkeypatch.setattr(CL, 'cluster_eval', stub)
    args = types.SimpleNamespace(cluster_k=0, num_class=3, cluster_iter=7, cluster_init=2, cluster_seed=5, dataset='ucf101',
                                 logger=logging.getLogger('test_cluster_host'))
    CLI.write_cluster(torch.zeros(6, 10, 8), torch.tensor([0, 1, 2, 0, 1, 2]), 'test', str(tmp_path), args)
    assert sorted(os.listdir(str(tmp_path))) == ['ucf101_test_cluster.json', 'ucf101_test_cluster.pth.tar']
    assert seen == dict(k=3, n_class=3, n_iter=7, n_init=2, seed=5)
    rep = json.load(open(str(tmp_path / 'ucf101_test_cluster.json')))
    assert (rep['k'], rep['n'], rep['n_iter'], rep['n_init'], rep['seed'], rep['iterations']) == (3, 60, 7, 2, 5, 2)
    assert set(rep['metrics']) >= {'nmi', 'ari', 'purity', 'accuracy', 'video_consistency', 'sizes'} and len(rep['trace']) == 2
    saved = torch.load(str(tmp_path / 'ucf101_test_cluster.pth.tar'), weights_only=True)
    assert saved['assign'].shape == (60,) and saved['centroids'].shape == (3, 8)
