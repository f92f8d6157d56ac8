"""GPU: the spectrum entries (include/dualvar_spectrum.h) and dualvar_amd/utils/spectrum.py against float64 numpy.

  covariance   integer features with n = 64 rows must reproduce numpy bit for bit (every intermediate is exact), both triangles
               equal; random data, given numpy's G, within four roundings per element.
  eigensolver  every matrix of tests/spectrum_reference.py cases() -- no pair, one pair, the bye, 7, 64, 65, 256 / 257 (the
               second element per thread), a diagonal matrix, a prescribed power-law spectrum, duplicated columns (the floor), a
               rank-deficient covariance -- must converge and meet, against numpy.linalg.eigh,
                 |lam^_i - lam_i| <= K eps n |A|_2,  |V V^T - I|_max <= K eps n,  |A V - V L|_max <= K eps n |A|_2,
                 |sum lam^ - tr A| <= K eps n |A|_2 (the K of the eigenvalues),
               with K four times the matching ratio of the CPU model (R.model_ratios(): 0.41, 1.86, 0.28 -> K = 1.6, 7.4, 1.1);
               the factor four covers the different summation tree.  The model is never the code under test.
  wide         n = 513, 1025, 2049, three rounds, one call each: V orthogonal, W = V A, the pairs of each round orthogonal, the
               row that sits out untouched bit for bit, nothing written outside [n][n] and stat [m].
  end to end   spectrum_eval on the planted fixture, pca_project's covariance, classifier.py's branch.

Largest err / bound seen on an MI355X (printed with -s): DESIGN.md section 6h."""
import json
import logging
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from tests import spectrum_reference as R  # noqa: E402
from tests.checks import F64, equal_bits, is_sent, lib, sent  # noqa: E402

EPS = R.EPS
U = 2.0 ** -24


def framed(x, dev, rows=2, cols=3):
    """x [r][c] float64 numpy -> a device buffer [r + rows][c + cols] of sentinels with x in its corner"""
    buf = sent((x.shape[0] + rows, x.shape[1] + cols), dev, F64)
    buf[:x.shape[0], :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return buf


def frame_ok(buf, r, c):
    return is_sent(buf[:r, c:]) and is_sent(buf[r:])


@pytest.fixture(scope='module')
def K():
    worst, _ = R.model_ratios()
    k = {name: 4 * v for name, v in worst.items()}
    print('model ratios %s -> K %s' % (worst, k))
    return k


# ---------------------------------------------------------------------------------------------------------- covariance
@pytest.mark.parametrize('D', [1, 5, 64, 65])
def test_covariance_exact_integers(gpu, D):
    """n = 64 rows of integers in [-8, 8]: G, s_i s_j (< 2^18), the quotient by 64, the difference and the second quotient are
    all exact, so the result equals numpy's bit for bit, through covariance() (the Gram kernel, then dv_spectrum_cov_f64)"""
    from dualvar_amd.utils import spectrum as SP
    z = np.random.RandomState(D).randint(-8, 9, size=(64, D)).astype(np.float32)
    mean, cov = SP.covariance(torch.from_numpy(z).to(gpu))
    want_mean, want = R.cov_from_gram(R.gram_of(z))
    assert cov.dtype == torch.float64 and tuple(cov.shape) == (D, D) and tuple(mean.shape) == (D,)
    assert equal_bits(cov.cpu(), torch.from_numpy(want)) and equal_bits(mean.cpu(), torch.from_numpy(want_mean))
    assert equal_bits(cov, cov.t())
    assert np.array_equal(want, R.cov_of(z))                   # and that is the covariance


def test_covariance_random_within_four_roundings(gpu):
    """n = 333, D = 130, numpy's G handed to dv_spectrum_cov_f64 at padded pitches: |err| <= 4 eps (|G_ij| + |s_i| |s_j| / n) / n
    against the same formula in extended precision; both triangles equal; nothing written outside [D][D] and [D]"""
    n, D = 333, 130
    z = np.random.RandomState(1).randn(n, D).astype(np.float32)
    G = R.gram_of(z)
    Gd, Cd = framed(G, gpu), sent((D + 2, D + 5), gpu, F64)
    md = sent((D + 3,), gpu, F64)
    _lib.check(lib().dv_spectrum_cov_f64(Gd.data_ptr(), Gd.shape[1], D, Cd.data_ptr(), Cd.shape[1], md.data_ptr(), ops.stream_ptr()),
               'dv_spectrum_cov_f64')
    torch.cuda.synchronize()
    assert frame_ok(Cd, D, D) and is_sent(md[D:])
    cov, mean = Cd[:D, :D].cpu().numpy(), md[:D].cpu().numpy()
    Gl = G.astype(np.longdouble)
    s, nn = Gl[D, :D], Gl[D, D]
    want = (Gl[:D, :D] - s[:, None] * s[None, :] / nn) / nn
    bound = 4 * EPS * (np.abs(G[:D, :D]) + np.abs(G[D, :D])[:, None] * np.abs(G[D, :D])[None, :] / n) / n
    err = np.abs(cov.astype(np.longdouble) - want).astype(np.float64)
    print('cov random: err / bound = %.4f' % float((err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(cov, cov.T)
    assert np.array_equal(mean, G[D, :D] / n)                  # one correctly rounded quotient


# ---------------------------------------------------------------------------------------------------------- eigensolver
@pytest.mark.parametrize('name', list(R.cases()))
def test_eigh_jacobi_against_numpy(gpu, K, name):
    from dualvar_amd.utils import spectrum as SP
    A = R.cases()[name]
    n = A.shape[0]
    lam, comps, info = SP.eigh_jacobi(torch.from_numpy(A).to(gpu))
    lam, comps = lam.cpu().numpy(), comps.cpu().numpy()
    q = R.quality(A, lam, comps)
    print('%s (n = %d): %s, values %.3f / %.2f orth %.3f / %.2f resid %.3f / %.2f trace %.3f / %.2f'
          % (name, n, info, q['values'], K['values'], q['orth'], K['orth'], q['resid'], K['resid'], q['trace'], K['values']))
    assert info['converged'] and info['sweeps'] <= R.MAX_SWEEPS
    assert (np.diff(lam) <= 0).all()                           # descending
    assert (comps[np.arange(n), np.abs(comps).argmax(1)] > 0).all()
    assert q['values'] <= K['values'] and q['orth'] <= K['orth'] and q['resid'] <= K['resid'] and q['trace'] <= K['values']
    if name == 'n1':
        assert lam.tolist() == [3.5] and comps.tolist() == [[1.0]] and info == {'sweeps': 1, 'converged': True, 'max_ratio': 0.0, 'rotations': 0}
    if name == 'n2':
        assert info['rotations'] >= 1 and info['sweeps'] >= 2
    if name == 'diag':
        assert info == {'sweeps': 1, 'converged': True, 'max_ratio': 0.0, 'rotations': 0}
        assert lam.tolist() == sorted(np.diag(A).tolist(), reverse=True)           # bit for bit
        assert np.array_equal(comps, np.eye(n)[np.argsort(-np.diag(A), kind='stable')])
    if name == 'duplicated':
        assert info['sweeps'] <= 20 and int((lam > 1e-10 * lam[0]).sum()) == 30       # the floor: ten null rows left alone
    if name == 'rank_deficient':
        assert int((lam > 1e-10 * lam[0]).sum()) == 2


def test_eigh_jacobi_is_deterministic_and_reports_a_nan(gpu):
    from dualvar_amd.utils import spectrum as SP
    for name in ('n65', 'duplicated'):
        A = torch.from_numpy(R.cases()[name]).to(gpu)
        l1, c1, i1 = SP.eigh_jacobi(A)
        l2, c2, i2 = SP.eigh_jacobi(A.clone())
        assert equal_bits(l1, l2) and equal_bits(c1, c2) and i1 == i2
    _, _, capped = SP.eigh_jacobi(torch.from_numpy(R.cases()['n65']).to(gpu), max_sweeps=2)
    assert capped == dict(capped, sweeps=2, converged=False) and capped['rotations'] > 0
    bad = R.cases()['n7'].copy()
    bad[2, 3] = bad[3, 2] = np.nan
    with pytest.raises(_lib.DualVarHipError, match='NaN'):
        SP.eigh_jacobi(torch.from_numpy(bad).to(gpu))


# ---------------------------------------------------------------------------------------------------------------- wide
def norm2_from_below(A, steps=30):
    """|A x| / |x| after a few power steps: never above |A|_2, so a bound built on it is never wider than the stated one"""
    x = np.ones(A.shape[0]) / np.sqrt(A.shape[0])
    for _ in range(steps):
        y = A @ x
        x = y / np.linalg.norm(y)
    return float(np.linalg.norm(A @ x))


@pytest.mark.parametrize('n', [513, 1025, 2049])
def test_three_rounds_of_a_wide_matrix(gpu, K, n):
    m = n + (n & 1)
    A = R.wide_matrix(n, n)
    norm2 = norm2_from_below(A)
    s = ops.stream_ptr()
    Ad = torch.from_numpy(A).to(gpu)
    W, V = sent((n + 2, n + 3), gpu, F64), sent((n + 2, n + 5), gpu, F64)
    scale, stat = sent((3,), gpu, F64), sent((m + 4,), gpu, F64)
    _lib.check(lib().dv_spectrum_init_f64(Ad.data_ptr(), n, n, W.data_ptr(), W.shape[1], V.data_ptr(), V.shape[1], scale.data_ptr(), s),
               'dv_spectrum_init_f64')
    assert equal_bits(W[:n, :n], Ad) and equal_bits(V[:n, :n], torch.eye(n, dtype=torch.float64, device=gpu))
    fro = float(scale[0])
    assert abs(fro - np.linalg.norm(A)) <= (n * n // 256 + 10) * EPS * fro and is_sent(scale[1:])
    assert lib().dv_spectrum_rounds(n) == m - 1
    rotated = 0
    for r in range(3):
        before_w, before_v = W[r, :n].clone(), V[r, :n].clone()
        _lib.check(lib().dv_spectrum_rounds_f64(W.data_ptr(), W.shape[1], V.data_ptr(), V.shape[1], n, r, r + 1, scale.data_ptr(),
                                                stat.data_ptr(), s), 'dv_spectrum_rounds_f64')
        torch.cuda.synchronize()
        # the row that sits out: row r is paired with index m - 1 = n, which does not exist
        assert equal_bits(W[r, :n], before_w) and equal_bits(V[r, :n], before_v)
        p, q = R.round_pairs(n, r)
        assert p.size == m // 2 - 1
        Wn = W[:n, :n].cpu().numpy()
        dot = np.abs((Wn[p] * Wn[q]).sum(1))
        lim = K['orth'] * EPS * n * np.linalg.norm(Wn[p], axis=1) * np.linalg.norm(Wn[q], axis=1)
        print('n = %d round %d: pair orthogonality err / bound = %.4f' % (n, r, float((dot / lim).max())))
        assert (dot <= lim).all()
        rotated += p.size
    assert frame_ok(W, n, n) and frame_ok(V, n, n) and is_sent(stat[m:]) and is_sent(scale[1:])
    st = stat[:m].cpu().numpy().reshape(-1, 2)
    assert st[0].tolist() == [0.0, 0.0]                        # slot 0 held the bye in every round
    assert st[:, 1].sum() == rotated and (st[1:, 1] == 3).all()                  # round_lo > 0 does not clear
    assert (st[1:, 0] > 0).all() and (st[:, 0] <= 1.0 + 4 * EPS).all()
    Vn, Wn = V[:n, :n].cpu().numpy(), W[:n, :n].cpu().numpy()
    orth = float(np.abs(Vn @ Vn.T - np.eye(n)).max()) / (K['orth'] * EPS * n)
    prod = float(np.abs(Wn - Vn @ A).max()) / (K['resid'] * EPS * n * norm2)
    print('n = %d: |V V^T - I| err / bound = %.4f, |W - V A| err / bound = %.4f' % (n, orth, prod))
    assert orth <= 1 and prod <= 1
    lam = sent((n + 3,), gpu, F64)
    _lib.check(lib().dv_spectrum_values_f64(W.data_ptr(), W.shape[1], V.data_ptr(), V.shape[1], n, lam.data_ptr(), s), 'dv_spectrum_values_f64')
    torch.cuda.synchronize()
    assert is_sent(lam[n:])
    want = (Vn * Wn).sum(1) / (Vn * Vn).sum(1)
    assert (np.abs(lam[:n].cpu().numpy() - want) <= (n // 256 + 24) * EPS * (np.abs(Vn) * np.abs(Wn)).sum(1)).all()


def test_rounds_clear_stat_only_from_round_zero(gpu):
    """n = 8: rounds [0, 7) in one call equal the seven calls of one round bit for bit, and the second sweep starts from a
    cleared stat"""
    A = R.psd(8, 8)
    s = ops.stream_ptr()
    out = []
    for split in (False, True):
        Ad = torch.from_numpy(A).to(gpu)
        W, V = torch.empty_like(Ad), torch.empty_like(Ad)
        scale, stat = torch.empty(1, dtype=torch.float64, device=gpu), sent((8,), gpu, F64)
        _lib.check(lib().dv_spectrum_init_f64(Ad.data_ptr(), 8, 8, W.data_ptr(), 8, V.data_ptr(), 8, scale.data_ptr(), s), 'dv_spectrum_init_f64')
        for lo, hi in ([(r, r + 1) for r in range(7)] if split else [(0, 7)]):
            _lib.check(lib().dv_spectrum_rounds_f64(W.data_ptr(), 8, V.data_ptr(), 8, 8, lo, hi, scale.data_ptr(), stat.data_ptr(), s),
                       'dv_spectrum_rounds_f64')
        out.append((W.clone(), V.clone(), stat.clone()))
    assert all(equal_bits(a, b) for a, b in zip(*out))
    assert float(out[0][2][1::2].sum()) == 28                  # every pair of a full 8 x 8 matrix rotates in the first sweep


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def planted(gpu):
    """the fixture, its rows as the library normalises them (both sides then decompose the same numbers), and spectrum_eval"""
    from dualvar_amd.utils import features as F
    from dualvar_amd.utils import spectrum as SP
    clips, label = R.spectrum_fixture()
    clips = torch.from_numpy(clips)
    z = F.normalise(clips.reshape(-1, clips.shape[-1])).double().cpu().numpy()
    rep = SP.spectrum_eval(clips.to(gpu), torch.from_numpy(label), ks=(4, 8))
    return clips, label, z, rep


def cov_error_bound(z):
    """element-wise bound on the covariance of n rows formed from a Gram matrix summed in any order: each of G_ij, s_i is off by
    at most (n + 2) eps of its sum of magnitudes; the four operations of the formula add 4 eps of (|G_ij| + |s_i| |s_j| / n) / n"""
    n = z.shape[0]
    za = np.abs(z)
    Ga, sa = za.T @ za, za.sum(0)
    return (n + 6) * EPS * (Ga + 2 * sa[:, None] * sa[None, :] / n) / n


def test_spectrum_eval_on_the_planted_fixture(gpu, K, planted):
    """the model on the same rows: shares 0.9994, 0.9983 (the two video directions) and 0.0008 (the within-video one); the
    eigenvalues agree within the eigen bound plus the two covariances' rounding"""
    clips, label, z, rep = planted
    n, D = z.shape
    mean, cov = R.cov_from_gram(R.gram_of(z))
    lam, comps, info = R.eigh_model(cov)
    share = R.video_share_ref(z, 24, 4, mean, comps, lam, 8)
    assert share[0] >= 0.99 and share[1] >= 0.99 and share[2] <= 0.01
    got = rep['eigenvalues'].cpu().numpy()
    tol = K['values'] * EPS * D * lam[0] + 2 * np.linalg.norm(cov_error_bound(z))
    print('spectrum_eval: eigenvalue err / bound = %.4f; video share %s (model %s); %s'
          % (float(np.abs(got - lam).max()) / tol, rep['video_share'][:4], share[:4], rep['info']))
    assert rep['info']['converged'] and np.abs(got - lam).max() <= tol
    assert np.abs(rep['mean'].cpu().numpy() - mean).max() <= (n + 3) * EPS * np.abs(z).mean(0).max()
    vs = rep['video_share']
    assert len(vs) == 8 and rep['ks'] == [4, 8]
    assert vs[0] >= 0.9 and vs[1] >= 0.9 and vs[2] <= 0.2
    want = R.metrics_ref(got, n)
    met = rep['metrics']
    for key in ('trace', 'effective_rank', 'rankme', 'participation_ratio', 'alpha', 'alpha_r2', 'top1_share'):
        assert abs(met[key] - want[key]) <= 1e-10 * max(1.0, abs(want[key])), key
    assert met['dims_for'] == want['dims_for'] and met['dims_for']['0.90'] == 3 and met['numerical_rank'] == 40 and met['D'] == 40 and met['n'] == 96


@pytest.mark.parametrize('whiten', [False, True])
def test_pca_project_covariance(gpu, K, planted, whiten):
    """the projected training rows have covariance diag(lam_1 .. lam_k); whitened, diag(lam / (lam + eps)), the identity to 2e-8.
    Expected values from numpy.linalg.eigvalsh of numpy's covariance.  Tolerance, element (j, k), for y = y_exact + e:
      |Cov(y) - Cov(y_exact)|_jk <= (|e_j| |y_k| + |y_j| |e_k| + |e_j| |e_k|) / n      (column 2-norms; centring shrinks them)
      |e|_ij <= u ((chain + 4) |z_i| . |c_j| + (chain + 6) |mean| . |c_j|)
    (dv_gemm_f32's bound (chain + 2) u |A| |B| of test_loss_gemm_optim_gpu.py with chain = 16 ceil(ceil(K / 16) / 4) + 3, one
    rounding for the bias addition and one for the cast of the components; the bias is a second such product and carries the
    cast of the mean as well), plus the eigen bound: Cov(y_exact) = C A C^T misses diag(lam) by at most
    (sqrt(D) K_resid + K_orth + K_values) eps D |A|_2 and the rounding of the two covariances."""
    from dualvar_amd.utils import spectrum as SP
    clips, label, z, rep = planted
    n, D = z.shape
    k = 8
    mean, comps, lam = rep['mean'], rep['components'], rep['eigenvalues']
    y = SP.pca_project(torch.from_numpy(z).float().to(gpu), mean, comps, lam, k, whiten=whiten)
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, k)
    y = y.double().cpu().numpy()
    mean, comps, lam = mean.cpu().numpy(), comps.cpu().numpy(), lam.cpu().numpy()
    A = R.cov_of(z)
    ref = np.sort(np.linalg.eigvalsh(A))[::-1]
    scale = 1.0 / np.sqrt(np.clip(lam[:k], 0, None) + 1e-12) if whiten else np.ones(k)
    c = np.abs(comps[:k] * scale[:, None])
    chain = 16 * -(-(-(-D // 16)) // 4) + 3
    assert chain == 19
    E = 1.01 * U * ((chain + 4) * np.abs(z) @ c.T + (chain + 6) * (np.abs(mean) @ c.T)[None, :])
    exact = R.project_ref(z, mean, comps, lam, k, whiten=whiten)
    assert (np.abs(y - exact) <= E).all()
    ej = np.linalg.norm(E, axis=0)
    yj = np.linalg.norm(exact - exact.mean(0), axis=0)
    tol = (ej[:, None] * yj[None, :] + yj[:, None] * ej[None, :] + ej[:, None] * ej[None, :]) / n
    eig = 1.01 * (np.sqrt(D) * K['resid'] + K['orth'] + K['values']) * EPS * D * ref[0] + 2 * np.linalg.norm(cov_error_bound(z))
    tol = tol + eig * scale[:, None] * scale[None, :]
    want = np.diag(ref[:k] * scale * scale)
    err = np.abs(R.cov_of(y) - want)
    print('pca_project whiten=%s: err / bound = %.4f (projection err / bound = %.4f)'
          % (whiten, float((err / tol).max()), float((np.abs(y - exact) / E).max())))
    assert (err <= tol).all()
    if whiten:
        assert np.abs(want - np.eye(k)).max() < 3e-8 and np.abs(R.cov_of(y) - np.eye(k)).max() < 1e-4


def test_classifier_spectrum_branch_writes_its_three_files(gpu, planted, tmp_path):
    """write_spectrum of classifier.py on stubbed features (the fixture in place of an encoder's): 16 videos train, 8 test; the
    three files appear and hold the report and the train fit"""
    import classifier as CLI
    from dualvar_amd.utils import spectrum as SP
    clips, label, z, rep = planted
    label = torch.from_numpy(label)
    parts = {'train': clips[:16].to(gpu), 'test': clips[16:].to(gpu)}
    feats = {'train': (parts['train'].mean(1), label[:16]), 'test': (parts['test'].mean(1), label[16:])}
    args = types.SimpleNamespace(spectrum_k=[8, 16, 64], dataset='ucf101', logger=logging.getLogger('test_spectrum_gpu'))
    CLI.write_spectrum(parts, feats, str(tmp_path), args)
    assert sorted(os.listdir(str(tmp_path))) == ['ucf101_spectrum.pth.tar', 'ucf101_test_spectrum.json', 'ucf101_train_spectrum.json']
    train = json.load(open(str(tmp_path / 'ucf101_train_spectrum.json')))
    test = json.load(open(str(tmp_path / 'ucf101_test_spectrum.json')))
    want = SP.spectrum_eval(parts['train'], label[:16], ks=(8, 16, 40))
    assert train['ks'] == [8, 16, 40] and train['eigenvalues'] == want['eigenvalues'].cpu().tolist()          # the same bits
    assert train['info'] == want['info'] and train['info']['converged'] and train['metrics']['n'] == 64 and test['metrics']['n'] == 32
    assert sorted(train['pca_retrieval']) == ['16', '40', '8'] and 'pca_retrieval' not in test
    assert all(0.0 <= v <= 1.0 for row in train['pca_retrieval'].values() for v in row.values())
    assert train['video_share'][0] >= 0.9 and len(train['video_share']) == 40
    saved = torch.load(str(tmp_path / 'ucf101_spectrum.pth.tar'), weights_only=True)
    assert saved['components'].shape == (40, 40) and saved['components'].dtype == torch.float64
    assert equal_bits(saved['eigenvalues'], want['eigenvalues'].cpu()) and equal_bits(saved['mean'], want['mean'].cpu())
