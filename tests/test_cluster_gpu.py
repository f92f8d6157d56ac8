"""GPU: the k-means entries of include/dualvar_cluster.h against the float64 reference of tests/cluster_reference.py, which is
written from the header.

assign and the seeding's mind are exact (comparisons and single fp32 operations); counts are exact.  The bounds of the rest follow
from the contract: sums are accumulated in double in a stated order and rounded once.
  centroid component:  2^-24 |c_d|  (the one rounding to fp32)
                       + a_d / |s_k|,  a_d = |M_k| 2^-52 sum_{r in M_k} |z_rd|  (the accumulated sum, the reference's own included)
                       + |c_d| (sum_d |s_d| a_d / |s_k|^2 + (D + 4) 2^-52)      (the same relative term for the norm)
  within[k]:           |M_k| 2^-52 sum |best_r|
  seeding total:       n 2^-52 total; the pick is checked against the kernel's own mind: the float64 cumulative sums in the header's
                       order bracket u * total at the picked row within that slack, and the row is off every centre (mind > 0).
  fit:                 the objective is a sum of n similarities from dv_gemm_f32, each within the element bound
                       (chain + 2) 2^-24 |z_r| |c_k| of test_loss_gemm_optim_gpu.py at this D, so an iteration may lose at most
                       2 n times that.
  dot:                 (4 ceil(D / 256) + 7) 2^-24 sum_d |z_rd c_d|: a lane's chain, the six sums of the fold, one rounding a product.
Each case prints (-s) err / bound; the module prints the largest per quantity at its end.  Largest measured on an MI355X:
centroid 0.997 (the one rounding to fp32 is the bound and the worst component nearly meets it), dot 0.12, within and the seeding
total 0.000 (the reference adds in the header's order)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from tests import cluster_reference as R  # noqa: E402
from tests.chains import gemm_chain  # noqa: E402
from tests.checks import U, Ratios, bits, is_sent, lib, report_fixture, sent  # noqa: E402
from tests.dataset_support import write_dataset  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E52 = 2.0 ** -52
WORST = Ratios()
ratio = WORST.ratio
_report_worst = report_fixture(WORST, 28)
NAN, INF = float('nan'), float('inf')


# --------------------------------------------------------------------------------------------------------------- assign
def assign_block(R_, K, seed):
    """[R_, K] float32 with the rows that can go wrong first: ties, NaN only, +-0, one number among NaN, a doubled maximum far
    apart, -inf only, +inf"""
    rng = np.random.RandomState(seed)
    sim = rng.randn(R_, K).astype(np.float32)
    kinds = ['ties', 'nan', 'zeros', 'one_number', 'double_max', 'neg_inf', 'pos_inf']
    for r in range(R_):
        kind = kinds[(r + seed) % len(kinds)] if r < 14 or r >= R_ - 7 else None
        if kind == 'ties':
            sim[r] = np.float32(0.25)
        elif kind == 'nan':
            sim[r] = np.nan
        elif kind == 'zeros':
            sim[r] = np.where(np.arange(K) % 2 == 0, np.float32(-0.0), np.float32(0.0))
        elif kind == 'one_number':
            sim[r] = np.nan
            sim[r, K - 1] = -3.0
        elif kind == 'double_max':
            sim[r, K // 3] = sim[r, K - 1] = 9.0
        elif kind == 'neg_inf':
            sim[r] = -np.inf
        elif kind == 'pos_inf':
            sim[r, K // 2] = np.inf
            sim[r, 0] = np.nan
    return sim


@pytest.mark.parametrize('K', [1, 2, 63, 64, 65, 257, 4096])
@pytest.mark.parametrize('R_', [1, 7, 300])
def test_assign(gpu, R_, K):
    ld = K + 3
    pad = torch.tensor([INF, NAN, INF])
    old = np.random.RandomState(K + R_).randint(-1, K, size=R_).astype(np.int32)
    assign = torch.cat([torch.from_numpy(old), torch.full((2,), 77, dtype=torch.int32)]).to(gpu)
    best = sent((R_ + 2,), gpu)
    changed = torch.zeros(1, dtype=torch.int64, device=gpu)
    want_changed, prev = 0, old
    for call in range(2):                        # two successive calls, one zeroing: the counts add up
        sim = assign_block(R_, K, seed=call)
        full = torch.cat([torch.from_numpy(sim), pad.expand(R_, 3)], 1).contiguous().to(gpu)
        _lib.check(lib().dv_kmeans_assign_f32(full.data_ptr(), ld, R_, K, assign.data_ptr(), best.data_ptr(), changed.data_ptr(),
                                              ops.stream_ptr()), 'dv_kmeans_assign_f32')
        ra, rb, rc = R.assign_ref(sim, K, prev)
        want_changed += rc
        got_a, got_b = assign.cpu().numpy(), best.cpu()
        assert (got_a[:R_] == ra).all(), (call, np.nonzero(got_a[:R_] != ra)[0][:5])
        assert (bits(got_b[:R_]).numpy() == rb.view(np.int32)).all(), call
        assert (got_a[R_:] == 77).all() and is_sent(got_b[R_:])
        prev = ra
    assert int(changed.item()) == want_changed
    print('    R=%d K=%d: assign and best exact, changed %d' % (R_, K, want_changed))


# --------------------------------------------------------------------------------------------------------------- update
UPDATE_CASES = [
    # n, D, K, how the rows are assigned
    (1, 1, 1, 'all'),
    (5, 3, 3, 'cancel'),            # cluster 0: two opposite rows (norm 0), cluster 1: one row, cluster 2: empty, rows with -1 and K
    (5, 512, 3, 'all'),
    (1000, 130, 101, 'random'),     # some rows with -1 and K; with n / K = 10 some clusters stay empty
    (1000, 64, 1, 'random'),
    (5000, 512, 3, 'one'),          # cluster 1 owns every row: 79 parts; clusters 0 and 2 empty
    (5000, 64, 101, 'random'),
    (5000, 3, 101, 'skewed'),       # one cluster with most rows, parts of every length
]


def update_case(n, D, K, how, seed=0):
    rng = np.random.RandomState(seed)
    z = rng.randn(n, D).astype(np.float32)
    best = rng.rand(n).astype(np.float32)
    if how == 'all':
        a = np.zeros(n, dtype=np.int32)
    elif how == 'one':
        a = np.ones(n, dtype=np.int32)
    elif how == 'cancel':
        a = np.array([0, 0, 1, K, -1], dtype=np.int32)
        z[1] = -z[0]
    elif how == 'skewed':
        a = np.where(rng.rand(n) < 0.7, 5, rng.randint(0, K, size=n)).astype(np.int32)
    else:
        a = rng.randint(0, K, size=n).astype(np.int32)
        if K > 1:
            a[a == K // 2] = 0                                                # an empty cluster whatever the draw
        a[rng.rand(n) < 0.02] = -1
        a[rng.rand(n) < 0.02] = K
    out = (a < 0) | (a >= K)
    z[out] = np.nan                               # a row of no cluster is read nowhere: it would poison its sum
    best[out] = np.nan
    return z, a, best


@pytest.mark.parametrize('n,D,K,how', UPDATE_CASES)
def test_update(gpu, n, D, K, how):
    z, a, best = update_case(n, D, K, how)
    ldz, ldc = D + 3, D + 5
    zf = sent((n, ldz), gpu)
    zf[:, :D] = torch.from_numpy(z).to(gpu)
    cent_in = torch.randn(K, ldc, generator=torch.Generator().manual_seed(1)).to(gpu)
    ws = torch.empty(lib().dv_kmeans_update_workspace(n, D, K) // 8, dtype=torch.float64, device=gpu)
    a_d, b_d = torch.from_numpy(a).to(gpu), torch.from_numpy(best).to(gpu)
    outs = []
    for rep in range(2):
        cent_out = sent((K + 1, ldc), gpu)
        counts = sent((K + 1,), gpu, torch.int32)
        within = sent((K + 1, 2), gpu, torch.int32).view(torch.float64).reshape(K + 1)
        ws.fill_(float(rep))                      # the workspace carries nothing from call to call
        _lib.check(lib().dv_kmeans_update_f32(zf.data_ptr(), ldz, n, D, a_d.data_ptr(), b_d.data_ptr(), K, cent_in.data_ptr(),
                                              cent_out.data_ptr(), ldc, counts.data_ptr(), within.data_ptr(), ws.data_ptr(),
                                              ops.stream_ptr()), 'dv_kmeans_update_f32')
        outs.append((cent_out.cpu(), counts.cpu(), within.cpu()))
    (c0, n0, w0), (c1, n1, w1) = outs
    assert bool((bits(c0) == bits(c1)).all()) and bool((n0 == n1).all()) and bool((bits(w0) == bits(w1)).all()), 'two calls differ in bits'
    assert is_sent(c0[:K, D:]) and is_sent(c0[K:]) and is_sent(n0[K:]) and is_sent(w0[K:].view(torch.int32))
    ref, counts_ref, within_ref, s, mass = R.update_ref(z, a, best, K, None)
    assert (n0[:K].numpy() == counts_ref).all()
    best64 = np.where(np.isnan(best), 0.0, best).astype(np.float64)
    wb = np.array([counts_ref[k] * E52 * np.abs(best64[a == k]).sum() for k in range(K)])
    rw = ratio(np.abs(w0[:K].numpy() - within_ref), wb, 'update.within')
    got = c0[:K, :D].double().numpy()
    kept, rc = 0, 0.0
    for k in range(K):
        if ref[k] is None:                        # empty, or norm 0: cent_in bit for bit
            assert bool((bits(c0[k, :D]) == bits(cent_in[k, :D].cpu())).all()), k
            kept += 1
            continue
        nrm = math.sqrt(float((s[k] * s[k]).sum()))
        acc = counts_ref[k] * E52 * mass[k]
        bound = U * np.abs(ref[k]) + acc / nrm + np.abs(ref[k]) * ((np.abs(s[k]) * acc).sum() / nrm ** 2 + (D + 4) * E52)
        rc = max(rc, ratio(np.abs(got[k] - ref[k]), bound, 'update.centroid'))
    if how in ('cancel', 'one') or (how == 'random' and K > 1):
        assert kept >= 1
    print('    n=%d D=%d K=%d %s: %d clusters keep their centroid; err / bound centroid %.3f within %.3f' % (n, D, K, how, kept, rc, rw))


# ------------------------------------------------------------------------------------------------------------------ dot
@pytest.mark.parametrize('n,D,ldz', [(1, 1, 1), (7, 3, 5), (300, 130, 131), (5, 64, 68), (300, 512, 512), (1000, 516, 520), (5, 1028, 1028)])
def test_dot(gpu, n, D, ldz):
    """one and several groups a lane, D no multiple of 4 / of 256, both load widths: D % 4 == 0 cases run from a 16-byte aligned
    and from a misaligned copy and must agree in every bit"""
    rng = np.random.RandomState(D)
    z, c = rng.randn(n, D).astype(np.float32), rng.randn(D).astype(np.float32)
    ref, bound = R.dot_ref(z, c)
    outs = []
    for shift in ((0, 1) if D % 4 == 0 else (0,)):
        buf = sent((n * ldz + 4,), gpu)
        zf = buf[shift:shift + n * ldz].view(n, ldz)
        zf[:, :D] = torch.from_numpy(z).to(gpu)
        cbuf = sent((D + 4,), gpu)
        cf = cbuf[shift:shift + D]
        cf.copy_(torch.from_numpy(c))
        s = sent((n + 1,), gpu)
        _lib.check(lib().dv_kmeans_dot_f32(zf.data_ptr(), ldz, n, D, cf.data_ptr(), s.data_ptr(), ops.stream_ptr()), 'dv_kmeans_dot_f32')
        assert is_sent(s[n:])
        outs.append(s[:n].cpu())
    r = ratio(np.abs(outs[0].double().numpy() - ref), bound, 'dot.s')
    if len(outs) == 2:
        assert bool((bits(outs[0]) == bits(outs[1])).all()), 'the two load widths differ in bits'
    print('    n=%d D=%d ldz=%d: err / bound %.3f' % (n, D, ldz, r))


# ----------------------------------------------------------------------------------------------------------------- seed
US =[0.0, 2.0 ** -60, 0.5, 1.0 - 2.0 ** -53]


def run_seed(s, mind, first, u, ws, gpu):
    pick = torch.full((2,), 77, dtype=torch.int32, device=gpu)
    total = sent((2, 2), gpu, torch.int32).view(torch.float64).reshape(2)
    _lib.check(lib().dv_kmeans_seed_f32(s.data_ptr(), s.numel() - 1, mind.data_ptr(), first, u, pick.data_ptr(), total.data_ptr(),
                                        ws.data_ptr(), ops.stream_ptr()), 'dv_kmeans_seed_f32')
    pick, total = pick.cpu(), total.cpu()
    assert int(pick[1]) == 77 and is_sent(total[1:].view(torch.int32)) and is_sent(mind[-1:])
    return int(pick[0]), float(total[0])


def check_pick(pick, total, mind, u, n, what):
    cum, t_ref = R.seed_cum_ref(mind)
    ratio([abs(total - t_ref)], [n * E52 * t_ref], 'seed.total ' + what)
    if t_ref == 0:
        assert pick == -1 and total == 0.0, what
        return
    slack, target = n * E52 * t_ref, u * t_ref
    assert 0 <= pick < n and mind[pick] > 0, (what, pick)
    assert cum[pick] > target - slack, (what, pick)
    assert pick == 0 or cum[pick - 1] <= target + slack, (what, pick)
    assert pick == R.seed_pick_ref(mind, u)[0], what        # the header's order is the reference's: the row itself


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 70000])
def test_seed(gpu, n):
    rng = np.random.RandomState(n)
    ws = torch.empty(lib().dv_kmeans_seed_workspace(n) // 8, dtype=torch.float64, device=gpu)

    def sims(seed):
        s = (np.random.RandomState(seed).rand(n) * 2 - 1).astype(np.float32)
        s[rng.rand(n) < 0.2] = 1.0                                             # rows on the centre
        s[rng.rand(n) < 0.05] = np.float32(1.0000001)                          # past it: clamped to 0
        if n > 2:
            s[n // 2] = np.nan                                                 # counts as +0
            s[0] = 1.0                                                         # the first row is never the pick
        return s
    s1, s2 = sims(1), sims(2)
    picks = []
    for u in US:
        mind = sent((n + 1,), gpu)
        d1 = torch.from_numpy(np.append(s1, np.float32(0))).to(gpu)            # one element more than n: never read past n
        pick, total = run_seed(d1, mind, 1, u, ws, gpu)
        m1 = mind[:n].cpu().numpy()
        want1 = R.seed_mind_ref(s1, None, True)
        assert (m1.view(np.int32) == want1.view(np.int32)).all(), 'mind of a first call'
        check_pick(pick, total, m1, u, n, 'first n=%d u=%g' % (n, u))
        d2 = torch.from_numpy(np.append(s2, np.float32(0))).to(gpu)
        pick2, total2 = run_seed(d2, mind, 0, u, ws, gpu)
        m2 = mind[:n].cpu().numpy()
        assert (m2.view(np.int32) == R.seed_mind_ref(s2, want1, False).view(np.int32)).all(), 'mind of a later call'
        check_pick(pick2, total2, m2, u, n, 'later n=%d u=%g' % (n, u))
        picks.append((pick, pick2))
        # every row at distance 0
        ones = torch.ones(n + 1, device=gpu)
        pick0, total0 = run_seed(ones, mind, 0, u, ws, gpu)
        assert pick0 == -1 and total0 == 0.0 and bool((mind[:n] == 0).all())
    print('    n=%d: picks (first, later) for u = 0, 2^-60, 0.5, 1 - 2^-53: %s; largest err / bound total %.3f' % (n, picks, WORST.get('seed.total', 0.0)))


# ------------------------------------------------------------------------------------------------------------------ fit
CACHE = {}


def fit_data(gpu):
    """the six groups of cluster_reference.fit_fixture, prepared on the device as kmeans_fit prepares them, and the float64
    reference's run from one point of each group on exactly those rows (computed once, left unchanged)"""
    if not CACHE:
        from dualvar_amd.utils.features import centre_normalise
        x, cls = R.fit_fixture()
        feat = torch.from_numpy(x).to(gpu)
        z = centre_normalise(feat)
        z64 = z.double().cpu().numpy()
        assign, cent, trace = R.lloyd_ref(z64, z64[::50])
        assert (assign == cls).all()
        CACHE.update(feat=feat, cls=cls, z=z, z64=z64, ref=(assign, cent, trace))
    return CACHE


def centroid_bound(z64, assign, K):
    ref, counts, _, s, mass = R.update_ref(z64, assign, np.zeros(len(assign)), K, None)
    D = z64.shape[1]
    bounds = []
    for k in range(K):
        nrm = math.sqrt(float((s[k] * s[k]).sum()))
        acc = counts[k] * E52 * mass[k]
        bounds.append(U * np.abs(ref[k]) + acc / nrm + np.abs(ref[k]) * ((np.abs(s[k]) * acc).sum() / nrm ** 2 + (D + 4) * E52))
    return np.stack(ref), np.stack(bounds)


def test_fit_from_explicit_init(gpu):
    from dualvar_amd.utils.cluster import kmeans_fit
    d = fit_data(gpu)
    n, D = d['z'].shape
    res = kmeans_fit(d['feat'], 6, init=d['z'][::50].clone(), row_block=128)       # three row blocks, the last one short
    assign, cent, trace = d['ref']
    assert res['assign'].dtype == torch.int32 and (res['assign'].cpu().numpy() == assign).all()
    assert res['iterations'] == len(res['trace']) == len(trace) and res['trace'][-1]['changed'] == 0 and res['trace'][0]['changed'] == n
    assert [t['changed'] for t in res['trace']] == [t['changed'] for t in trace]
    assert res['empty'] == 0 and res['sizes'] == [50] * 6 and res['init_index'] is None
    ref_c, bound = centroid_bound(d['z64'], assign, 6)
    assert np.abs(ref_c - cent).max() < 1e-14
    rc = ratio(np.abs(res['centroids'].double().cpu().numpy() - ref_c), bound, 'fit.centroid')
    elem = (max(gemm_chain(128, 6, D), gemm_chain(300 - 256, 6, D)) + 2) * U       # |z_r| = |c_k| = 1; row blocks of 128 and 44
    obj = [t['objective'] for t in res['trace']]
    assert res['objective'] == obj[-1]
    assert all(b >= a - 2 * n * elem for a, b in zip(obj, obj[1:])), obj
    ro = ratio([abs(a - b['objective']) for a, b in zip(obj, trace)], [n * elem * 1.0 + n * E52 * n] * len(obj), 'fit.objective')
    print('    fit from an explicit init: %d iterations, err / bound centroid %.3f objective %.3f' % (res['iterations'], rc, ro))


def test_fit_with_seeding_is_reproducible(gpu):
    from dualvar_amd.utils.cluster import cluster_metrics, kmeans_fit
    d = fit_data(gpu)
    a = kmeans_fit(d['feat'], 6, n_init=3, seed=0)
    b = kmeans_fit(d['feat'], 6, n_init=3, seed=0)
    rep = cluster_metrics(a['assign'], d['cls'], vid=np.arange(300) // 10)
    assert rep['nmi'] == pytest.approx(1.0, abs=1e-12) and rep['accuracy'] == 1.0 and rep['ari'] == 1.0 and rep['video_consistency'] == 1.0
    assert bool((a['assign'] == b['assign']).all()) and bool((bits(a['centroids']) == bits(b['centroids'])).all())
    assert a['objective'] == b['objective'] and a['trace'] == b['trace'] and a['init_index'] == b['init_index'] and a['restart'] == b['restart']
    assert len(a['init_index']) == len(set(a['init_index'])) == 6 and all(0 <= i < 300 for i in a['init_index'])
    c = kmeans_fit(d['feat'], 6, n_init=1, seed=1)                                 # another seed: other draws
    assert c['init_index'] != a['init_index']
    print('    seeded fit: restart %d of 3 kept, rows %s, objective %.6f' % (a['restart'], a['init_index'], a['objective']))


def test_fit_with_seven_clusters_on_six_groups(gpu):
    from dualvar_amd.utils.cluster import cluster_metrics, kmeans_fit
    d = fit_data(gpu)
    z = d['z']
    split = kmeans_fit(d['feat'], 7, init=z[[0, 1, 50, 100, 150, 200, 250]].clone())
    want = R.lloyd_ref(d['z64'], d['z64'][[0, 1, 50, 100, 150, 200, 250]])[0]
    assert (split['assign'].cpu().numpy() == want).all() and split['empty'] == 0 and sum(split['sizes']) == 300
    far = -z[::50].sum(0, keepdim=True)                                          # away from every group
    far = far / far.norm()
    init = torch.cat([z[::50], far.float()], 0).contiguous()                    # the seventh centre attracts nobody
    empty = kmeans_fit(d['feat'], 7, init=init.clone())
    assert empty['empty'] == 1 and empty['sizes'][6] == 0 and (empty['assign'].cpu().numpy() == d['cls']).all()
    assert bool((bits(empty['centroids'][6]) == bits(init[6])).all())                # it keeps its centroid bit for bit
    rep = cluster_metrics(split['assign'], d['cls'])
    assert rep['purity'] == 1.0 and rep['accuracy'] < 1.0 and rep['n_cluster'] == 7
    seeded = kmeans_fit(d['feat'], 7, n_init=2, seed=0)
    assert sum(seeded['sizes']) == 300 and seeded['iterations'] >= 1
    print('    K = 7 on six groups: sizes split %s, empty %s, seeded %s' % (split['sizes'], empty['sizes'], seeded['sizes']))


# ------------------------------------------------------------------------------------------------------- the driver, one child
def test_cli_retrieval_with_cluster(gpu, tmp_path_factory):
    from dualvar_amd.utils.cluster import cluster_eval
    d = tmp_path_factory.mktemp('cluster_cli')
    split, frame = write_dataset(str(d / 'data'), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
    os.makedirs(str(d / 'run' / 'model'))
    argv = [os.path.join(ROOT, 'classifier.py'), '--test', str(d / 'run' / 'model' / 'none.pth.tar'), '--retrieval', '--num_seq', '10',
            '--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
            '--split_root', split, '--frame_root', frame, '--cluster', '--cluster_k', '3', '--cluster_iter', '20', '--cluster_init', '2',
            '--cluster_seed', '4', '--cluster_split', 'both']
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=600, cwd=str(d))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    fdir = str(d / 'run' / 'model' / 'feature')
    assert out.count('k-means of ucf101') == 2 and 'video consistency = ' in out, out[-2000:]
    assert not [f for f in os.listdir(fdir) if '_tsne' in f or '_variance' in f or '_knn' in f]
    for split_name, n_video in (('test', 3), ('train', 30)):
        stem = os.path.join(fdir, 'ucf101_%s_cluster' % split_name)
        saved = torch.load(stem + '.pth.tar', map_location='cpu', weights_only=True)
        assert saved['assign'].shape == (10 * n_video,) and saved['assign'].dtype == torch.int32 and saved['centroids'].shape[0] == 3
        with open(stem + '.json') as fp:
            rep = json.load(fp)
        assert (rep['k'], rep['n_iter'], rep['n_init'], rep['seed'], rep['n']) == (3, 20, 2, 4, 10 * n_video)
        per = torch.load(os.path.join(fdir, 'ucf101_%s_per_feature.pth.tar' % split_name), map_location='cpu', weights_only=True)
        label = torch.load(os.path.join(fdir, 'ucf101_%s_label.pth.tar' % split_name), map_location='cpu', weights_only=True)
        fit, direct = cluster_eval(per.to(gpu), label, k=3, n_class=rep['metrics']['n_class'], n_iter=20, n_init=2, seed=4)
        assert bool((fit['assign'].cpu() == saved['assign']).all()) and bool((bits(fit['centroids'].cpu()) == bits(saved['centroids'])).all())
        assert rep['metrics'] == json.loads(json.dumps(direct)) and rep['trace'] == fit['trace'] and rep['objective'] == fit['objective']
        assert rep['sizes'] == fit['sizes'] and sum(rep['sizes']) == 10 * n_video and rep['init_index'] == fit['init_index']
        for key in ('nmi', 'purity', 'accuracy', 'video_consistency'):
            assert 0.0 <= rep['metrics'][key] <= 1.0, (key, rep['metrics'])
