"""GPU: the ridge-probe entries of include/dualvar_ridge.h against float64, and dualvar_amd/utils/probe.py end to end against the
reference of tests/ridge_reference.py.

Two kinds of data.
  (A) exact integers: every partial sum is an integer far below 2^53, so any order gives the same double and the result must
      EQUAL the integer one.  For the Gram this pins the MFMA lane maps, every tile edge, the mirror and the slab fold; for the
      solve (A = L0 L0^T with a small integer L0, B = A W0) every pivot, quotient and update is an integer, so chol must equal
      L0 and W must equal W0 bit for bit.
  (B) random data with bounds that are derived, not measured:
      Gram     |G - G_ref| <= (n + 2) 2^-52 |Z~|^T |Z~|  element-wise, the same form for B: the products are exact (fp32 x fp32
               in double), so this is the bound of a sum of n terms in any order (the reference's own sum included).
      factor   |A - L L^T| <= (Da + 2) 2^-52 |L| |L^T|                        (Higham, Accuracy and Stability, Theorem 10.3)
      residual |A W - B|   <= (3 Da + 8) 2^-52 |L| (|L^T| |W|)                (Theorem 10.4), A W formed in numpy float64;
               2^-52 stands for the unit roundoff 2^-53 to cover the test's own products.
Each case prints (-s) err / bound.  Largest measured on an MI355X: Gram 0.007 (B 0.000: the reference adds the same few terms),
factor 0.074, residual 0.015.  The end-to-end test compares counts: every accuracy of ridge_probe must equal the float64
reference's, and the reference shows that no score row is within 4 fp32 GEMM element bounds of a change of rank."""
import json
import logging
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from tests import ridge_reference as R  # noqa: E402
from tests.checks import F64, is_sent, lib, sent  # noqa: E402

E52 = 2.0 ** -52
SLAB = R.SLAB


def ratio(err, bound, what):
    """largest err / bound over the elements; where the bound is 0 the error must be 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), what + ': non-finite output'
    zero = bound == 0
    assert (err[zero] == 0).all(), what + ': error where the bound is exactly 0'
    r = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print('%s: err / bound = %.4f' % (what, r))
    assert r <= 1.0, '%s: err / bound = %.3f' % (what, r)
    return r


# ---------------------------------------------------------------------------------------------------------------- Gram
def run_gram(dev, z, label, C, G, B, accumulate, pad=3):
    """z [n][D] fp32 numpy at pitch D + pad (the padding holds NaN), G / B device buffers with sentinel margins"""
    n, D = z.shape
    full = np.full((n, D + pad), np.nan, dtype=np.float32)
    full[:, :D] = z
    zd = torch.from_numpy(full).to(dev)
    ld = torch.from_numpy(np.asarray(label, dtype=np.int32)).to(dev)
    nbytes = lib().dv_ridge_gram_workspace(n, D, C)
    assert nbytes == R.gram_workspace_bytes(n, D, C)
    ws = sent((nbytes // 8 + 4,), dev, F64)
    _lib.check(lib().dv_ridge_gram_f64(zd.data_ptr(), D + pad, n, D, ld.data_ptr(), C, G.data_ptr(), G.shape[1], B.data_ptr(), B.shape[1],
                                       accumulate, ws.data_ptr(), ops.stream_ptr()), 'dv_ridge_gram_f64')
    torch.cuda.synchronize()
    assert is_sent(ws[nbytes // 8:])


def gram_buffers(dev, D, C):
    """[Da + 1][Da + 2] and [Da + 1][C + 2] of sentinels: one row and two columns more than the entry may write"""
    return sent((D + 2, D + 3), dev, F64), sent((D + 2, C + 2), dev, F64)


def labels_with_skips(rng, n, C):
    label = rng.randint(0, C, size=n)
    skip = rng.rand(n) < 0.2
    label[skip] = np.where(rng.rand(int(skip.sum())) < 0.5, -1, C)
    if n > 2:
        label[n // 2] = -7
    return label


GRAM_SHAPES = [(1, 1, 1), (5, 3, 2), (63, 16, 5), (65, 17, 5), (SLAB + 6, 37, 7), (2 * SLAB + 52, 129, 17),
               (8 * SLAB + 70, 3, 2),            # more than DV_RIDGE_MAX_SLABS slabs of DV_RIDGE_SLAB rows: the slabs double
               (40, 64, 70)]                     # Da = 65: one column in the second tile; two class blocks


@pytest.mark.parametrize('n,D,C', GRAM_SHAPES)
def test_gram_exact_integers(gpu, n, D, C):
    rng = np.random.RandomState(n + D)
    Da = D + 1
    z1, z2 = (rng.randint(-4, 5, size=(m, D)).astype(np.float32) for m in (n, n // 2 + 1))
    l1, l2 = labels_with_skips(rng, n, C), labels_with_skips(rng, n // 2 + 1, C)
    if n == 1:
        l1[:] = 0
    for z, l in ((z1, l1), (z2, l2)):            # a skipped row may hold anything
        z[(l < 0) | (l >= C)] = np.nan
    G, B = gram_buffers(gpu, D, C)
    run_gram(gpu, z1, l1, C, G, B, 0)
    G1, B1 = R.gram_ref(np.nan_to_num(z1), l1, C)
    assert np.abs(G1).max() < 2 ** 40
    assert (G[:Da, :Da].cpu().numpy() == G1).all() and (B[:Da, :C].cpu().numpy() == B1).all()
    assert is_sent(G[Da:]) and is_sent(G[:, Da:]) and is_sent(B[Da:]) and is_sent(B[:, C:])
    assert G1[D, D] == ((l1 >= 0) & (l1 < C)).sum()
    run_gram(gpu, z2, l2, C, G, B, 1)            # a second row set on top
    G2, B2 = R.gram_ref(np.nan_to_num(z2), l2, C)
    assert (G[:Da, :Da].cpu().numpy() == G1 + G2).all() and (B[:Da, :C].cpu().numpy() == B1 + B2).all()
    assert is_sent(G[Da:]) and is_sent(G[:, Da:]) and is_sent(B[Da:]) and is_sent(B[:, C:])


@pytest.mark.parametrize('n,D,C', [(300, 38, 5), (2 * SLAB + 9, 130, 101), (5 * SLAB, 513, 7)])
def test_gram_random_within_the_summation_bound(gpu, n, D, C):
    rng = np.random.RandomState(D)
    Da = D + 1
    z = rng.randn(n, D).astype(np.float32)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    label = labels_with_skips(rng, n, C)
    z[(label < 0) | (label >= C)] = np.nan
    G, B = gram_buffers(gpu, D, C)
    run_gram(gpu, z, label, C, G, B, 0)
    Gr, Br = R.gram_ref(np.nan_to_num(z), label, C)
    Ga, Ba = R.abs_gram(np.nan_to_num(z), label, C)
    got_G, got_B = G[:Da, :Da].cpu().numpy(), B[:Da, :C].cpu().numpy()
    ratio(np.abs(got_G - Gr), (n + 2) * E52 * Ga, 'gram.G n=%d D=%d' % (n, D))
    ratio(np.abs(got_B - Br), (n + 2) * E52 * Ba, 'gram.B n=%d D=%d C=%d' % (n, D, C))
    assert (got_G == got_G.T).all()              # both triangles, bit for bit
    G2, B2 = gram_buffers(gpu, D, C)             # the same inputs, the same bits
    run_gram(gpu, z, label, C, G2, B2, 0)
    assert torch.equal(G.view(torch.int64), G2.view(torch.int64)) and torch.equal(B.view(torch.int64), B2.view(torch.int64))


# --------------------------------------------------------------------------------------------------------------- solve
def run_solve(dev, G, B, lam, n_pen, pad=2):
    """G [Da][Da], B [Da][C] numpy -> (chol [Da + 1][Da + pad], W [Da + 1][C + pad] device buffers on sentinels, info)"""
    Da, C = B.shape
    Gd = torch.from_numpy(np.triu(np.full((Da, Da), np.nan), 1) + np.tril(G)).to(dev)      # the upper triangle is never read
    Bd = torch.from_numpy(np.ascontiguousarray(B)).to(dev)
    chol, W = sent((Da + 1, Da + pad), dev, F64), sent((Da + 1, C + pad), dev, F64)
    info = torch.full((2,), 77, dtype=torch.int32, device=dev)
    _lib.check(lib().dv_ridge_solve_f64(Gd.data_ptr(), Da, Da, n_pen, lam, Bd.data_ptr(), C, C, W.data_ptr(), C + pad, chol.data_ptr(),
                                        Da + pad, info.data_ptr(), ops.stream_ptr()), 'dv_ridge_solve_f64')
    torch.cuda.synchronize()
    assert int(info[1]) == 77
    return chol, W, int(info[0])


def untouched(chol, W, Da, C):
    upper = torch.triu(torch.ones(Da, Da, dtype=torch.bool, device=chol.device), 1)
    return (is_sent(chol[:Da, :Da][upper]) and is_sent(chol[Da:]) and is_sent(chol[:, Da:]) and is_sent(W[Da:]) and
            is_sent(W[:, C:]))


@pytest.mark.parametrize('Da,C', [(1, 1), (17, 3), (64, 2), (65, 33), (66, 65), (130, 7), (257, 5)])
def test_solve_exact_integers(gpu, Da, C):
    rng = np.random.RandomState(Da)
    L0 = np.tril(rng.randint(-2, 3, size=(Da, Da)).astype(np.float64), -1) + np.diag(rng.choice([1.0, 2.0, 4.0], size=Da))
    W0 = rng.randint(-3, 4, size=(Da, C)).astype(np.float64)
    A = L0 @ L0.T
    B = A @ W0
    assert np.abs(B).max() < 2 ** 40
    chol, W, info = run_solve(gpu, A, B, 0.0, Da)
    assert info == 0
    got_L = np.tril(chol[:Da, :Da].cpu().numpy())
    assert (got_L == L0).all(), 'first difference at %s' % (np.argwhere(got_L != L0)[:1],)
    assert (W[:Da, :C].cpu().numpy() == W0).all()
    assert untouched(chol, W, Da, C)


def unit_gram(Da, n, seed):
    rng = np.random.RandomState(seed)
    z = rng.randn(n, Da - 1).astype(np.float32)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    label = rng.randint(0, 1 << 30, size=n)
    return z, label


@pytest.mark.parametrize('rel', [1e-6, 1e-2])
@pytest.mark.parametrize('Da,C', [(38, 5), (130, 101), (513, 5), (513, 101)])
def test_solve_random_within_the_higham_bounds(gpu, Da, C, rel):
    n = 2 * Da + 11
    z, label = unit_gram(Da, n, Da + C)
    G, B = R.gram_ref(z, label % C, C)
    lam = rel * n
    chol, W, info = run_solve(gpu, G, B, lam, Da - 1)
    assert info == 0 and untouched(chol, W, Da, C)
    A = R.penalised(G, lam, Da - 1)
    Lh = np.tril(chol[:Da, :Da].cpu().numpy())
    Wh = W[:Da, :C].cpu().numpy()
    what = 'Da=%d C=%d lambda=%g n' % (Da, C, rel)
    ratio(np.tril(np.abs(A - Lh @ Lh.T)), np.tril((Da + 2) * E52 * (np.abs(Lh) @ np.abs(Lh.T))), 'solve.factor ' + what)
    ratio(np.abs(A @ Wh - B), (3 * Da + 8) * E52 * (np.abs(Lh) @ (np.abs(Lh.T) @ np.abs(Wh))), 'solve.residual ' + what)
    chol2, W2, _ = run_solve(gpu, G, B, lam, Da - 1)          # the same inputs, the same bits
    assert torch.equal(chol.view(torch.int64), chol2.view(torch.int64)) and torch.equal(W.view(torch.int64), W2.view(torch.int64))


def test_solve_reports_the_first_bad_pivot(gpu):
    A, B = np.diag([1.0, -1.0, 1.0]), np.ones((3, 2))
    assert run_solve(gpu, A, B, 0.0, 3)[2] == 2
    assert run_solve(gpu, A, B, 0.5, 3)[2] == 2              # 0.5 - 1 is still negative
    chol, W, info = run_solve(gpu, A, B, 3.0, 3)             # diag(4, 2, 4)
    assert info == 0 and np.abs(W[:3, :2].cpu().numpy() - np.array([[0.25], [0.5], [0.25]])).max() <= 2.0 ** -51
    assert run_solve(gpu, A, B, 3.0, 1)[2] == 2              # the penalty reaches the first entry only
    # beyond the first block: the pivot index is the global one
    d = np.ones(70)
    d[66] = 0.0
    assert run_solve(gpu, np.diag(d), np.ones((70, 1)), 0.0, 70)[2] == 67
    d[66] = np.nan
    assert run_solve(gpu, np.diag(d), np.ones((70, 1)), 0.0, 70)[2] == 67


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def fixture():
    clips, label = R.probe_fixture()
    return clips, label


def gpu_rows(clips):
    """the rows as the library normalises them, in float64: both sides then solve the same system"""
    from dualvar_amd.utils import features as F
    clips = torch.as_tensor(clips)
    return F.normalise(clips.reshape(-1, clips.shape[-1])).double().cpu().numpy()


@pytest.mark.parametrize('n_train', [40, 60])
def test_ridge_probe_equals_the_reference(gpu, fixture, n_train):
    """the first 40 videos train and the last 20 test; and all 60 as the training set, the setting whose figures the reference
    is asserted on: 12 held out, the video sweep 0.417 0.417 0.5 0.667 1.0 0.917, lambda = 1e-2 alone on top"""
    from dualvar_amd.utils import probe as PR
    clips, label = fixture
    tr, te = slice(0, n_train), slice(40, 60)
    got = PR.ridge_probe(clips[tr].to(gpu), label[tr], clips[te].to(gpu), label[te], 6)
    # the normalisation is an existing entry, relative to the float64 rows within 8 u: a product, at most 3 additions of a lane
    # and 6 of the fold on the sum of squares (10 u, halved by the root), the root, the division
    z32, z64 = gpu_rows(clips[tr]), R.normalise_ref(clips[tr].numpy())
    assert (np.abs(z32 - z64) <= 8 * 2.0 ** -24 * np.abs(z64)).all()
    want = R.probe_ref(clips[tr].numpy(), label[tr].numpy(), clips[te].numpy(), label[te].numpy(), 6, normalise=gpu_rows)
    # a score row may be left out only if its margin is below 4 fp32 GEMM element bounds; none is
    left_out = sum(int((m < 4 * b).sum()) for m, b in want['margins'])
    worst = min(float((m / b).min()) for m, b in want['margins'])
    print('n_train=%d: smallest margin / bound = %.1f, sweep %s' % (n_train, worst, [round(s['video_top1'], 3) for s in want['sweep']]))
    assert left_out == 0 and worst > 20
    if n_train == 60:
        assert want['n_held_videos'] == 12 and want['lambda'] == 1e-2
        assert [round(s['video_top1'], 3) for s in want['sweep']] == [0.417, 0.417, 0.5, 0.667, 1.0, 0.917]
    assert got['sweep'] == want['sweep']
    for key in ('lambda', 'clip_top1', 'clip_top5', 'video_top1', 'video_top5', 'n_train', 'n_fit', 'n_held_videos', 'n_class', 'D'):
        assert got[key] == want[key], key
    assert got['W'].shape == (130, 6) and got['W'].dtype == torch.float64
    again = PR.ridge_probe(clips[tr].to(gpu), label[tr], clips[te].to(gpu), label[te], 6)
    assert torch.equal(got['W'].view(torch.int64), again['W'].view(torch.int64))


def test_ridge_systems_read_each_row_once_per_system(gpu, fixture):
    """fit + held = full, and the held rows do not reach the fit system (NaN in them stays out)"""
    from dualvar_amd.utils import probe as PR
    clips, label = fixture
    z = torch.from_numpy(gpu_rows(clips)).float().to(gpu)
    cl = label.repeat_interleave(2)
    held = PR.holdout_mask(label, 5).repeat_interleave(2)
    G_fit, B_fit, G_full, B_full = PR.ridge_systems(z, cl, held, n_class=6)
    zn = z.cpu().numpy()
    Gr, Br = R.gram_ref(zn, np.where(held.numpy(), -1, cl.numpy()), 6)
    Ga, Ba = R.abs_gram(zn, np.where(held.numpy(), -1, cl.numpy()), 6)
    ratio(np.abs(G_fit.cpu().numpy() - Gr), 122 * E52 * Ga, 'systems.G_fit')
    ratio(np.abs(B_fit.cpu().numpy() - Br), 122 * E52 * Ba, 'systems.B_fit')
    Gr, Br = R.gram_ref(zn, cl.numpy(), 6)
    Ga, Ba = R.abs_gram(zn, cl.numpy(), 6)
    ratio(np.abs(G_full.cpu().numpy() - Gr), 123 * E52 * Ga, 'systems.G_full')          # one more addition: the two systems
    ratio(np.abs(B_full.cpu().numpy() - Br), 123 * E52 * Ba, 'systems.B_full')
    assert float(G_fit[129, 129]) == 96 and float(G_full[129, 129]) == 120
    poisoned = z.clone()
    poisoned[held.to(gpu)] = float('nan')
    G2, B2, _, _ = PR.ridge_systems(poisoned, cl, held, n_class=6)
    assert torch.equal(G2.view(torch.int64), G_fit.view(torch.int64)) and torch.equal(B2.view(torch.int64), B_fit.view(torch.int64))
    with pytest.raises(_lib.DualVarHipError, match='pivot'):
        PR.ridge_solve(torch.diag(torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64, device=gpu)),
                       torch.ones(3, 2, dtype=torch.float64, device=gpu), 0.0, 3)


def test_ridge_probe_without_a_holdout(gpu, fixture):
    """five videos per class at holdout = 7: nothing can be held out, the sweep is skipped and the single lambda is used"""
    from dualvar_amd.utils import probe as PR
    clips, label = fixture
    got = PR.ridge_probe(clips[:30].to(gpu), label[:30], clips[40:].to(gpu), label[40:], 6, lambdas=(1e-2,), holdout=7)
    want = R.probe_ref(clips[:30].numpy(), label[:30].numpy(), clips[40:].numpy(), label[40:].numpy(), 6, lambdas=(1e-2,), holdout=7,
                       normalise=gpu_rows)
    assert got['sweep'] == [] and got['n_held_videos'] == 0 and got['lambda'] == 1e-2 and got['n_fit'] == 60
    assert sum(int((m < 4 * b).sum()) for m, b in want['margins']) == 0
    for key in ('clip_top1', 'clip_top5', 'video_top1', 'video_top5'):
        assert got[key] == want[key], key
    assert PR.ridge_probe(clips[:30].to(gpu), label[:30], clips[40:].to(gpu), label[40:], 6, holdout=7)['lambda'] == 1e-3


def test_classifier_ridge_branch_writes_its_two_files(gpu, fixture, tmp_path):
    """write_ridge of classifier.py on stubbed features (the fixture in place of an encoder's): the two files appear and hold the
    report and the weights"""
    import classifier as CLI
    clips, label = fixture
    args = types.SimpleNamespace(num_class=6, ridge_lambda=list(R.LAMBDAS), ridge_holdout=5, dataset='ucf101',
                                 logger=logging.getLogger('test_ridge_gpu'))
    CLI.write_ridge(clips[:40].to(gpu), label[:40], clips[40:].to(gpu), label[40:], str(tmp_path), args)
    assert sorted(os.listdir(str(tmp_path))) == ['ucf101_ridge.json', 'ucf101_ridge.pth.tar']
    rep = json.load(open(str(tmp_path / 'ucf101_ridge.json')))
    want = R.probe_ref(clips[:40].numpy(), label[:40].numpy(), clips[40:].numpy(), label[40:].numpy(), 6, normalise=gpu_rows)
    assert rep['lambda'] == want['lambda'] and rep['video_top1'] == want['video_top1'] and rep['sweep'] == want['sweep']
    saved = torch.load(str(tmp_path / 'ucf101_ridge.pth.tar'), weights_only=True)
    assert saved['W'].shape == (130, 6) and saved['W'].dtype == torch.float64 and saved['lambda'] == want['lambda']
