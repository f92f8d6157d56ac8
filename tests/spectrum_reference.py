"""Float64 numpy model of the feature spectrum (include/dualvar_spectrum.h, dualvar_amd/utils/spectrum.py): the round-robin
schedule, the one-sided Jacobi sweeps with the floor on null rows and the rotation formula of the header, the covariance from the
augmented Gram matrix, the spectrum figures, the PCA projection and the between-video share; and the seeded matrices and the
fixture the tests use.  The model sums with numpy (pairwise), the kernels with a strided loop and a fixed tree: the two agree to
rounding, not bit for bit, which is what the factor four of the GPU test's bounds covers."""
import functools
import math

import numpy as np

MAX_D, MAX_SWEEPS, BLOCK = 4096, 64, 256
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------ schedule
def rounds(n):
    return 0 if n == 1 else n + (n & 1) - 1


def pair(n, r, k):
    m = n + (n & 1)
    a, b = (m - 1, r) if k == 0 else ((r + k) % (m - 1), (r - k) % (m - 1))
    return (a, b) if a < b else (b, a)


def round_pairs(n, r):
    """(p [slots], q [slots]) of round r without the bye"""
    m = n + (n & 1)
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (r + k) % (m - 1)])
    b = np.concatenate([[r], (r - k) % (m - 1)])
    p, q = np.minimum(a, b), np.maximum(a, b)
    live = q < n
    return p[live], q[live]


# ---------------------------------------------------------------------------------------------------------- eigensolver
def dots(X, Y, kernel_order=False):
    """row-wise dot products of X, Y [k, n]: numpy's pairwise sum, or with kernel_order the order of the header (thread t adds
    i = t, t + 256, ... ascending from 0.0, then the tree s = 128 .. 1)"""
    P = X * Y
    if not kernel_order:
        return P.sum(1)
    k, n = P.shape
    pad = np.zeros((k, -(-n // BLOCK) * BLOCK))
    pad[:, :n] = P
    pad = pad.reshape(k, -1, BLOCK)
    part = np.zeros((k, BLOCK))
    for chunk in range(pad.shape[1]):                # 0.0 + x = x and x + 0.0 = x exactly, so the padding changes no bit
        part = part + pad[:, chunk]
    s = BLOCK // 2
    while s:
        part = part[:, :s] + part[:, s:2 * s]
        s //= 2
    return part[:, 0]


def jacobi_round(W, V, n, r, scale, floor=True, kernel_order=False):
    """one round in place -> (rotations, largest cosine among the pairs above the floor)"""
    p, q = round_pairs(n, r)
    if p.size == 0:
        return 0, 0.0
    wp, wq = W[p], W[q]
    a, b, c = dots(wp, wp, kernel_order), dots(wq, wq, kernel_order), dots(wp, wq, kernel_order)
    ra, rb = np.sqrt(a), np.sqrt(b)
    above = np.minimum(ra, rb) > (EPS * scale if floor else 0.0)
    rot = above & (np.abs(c) > EPS * ra * rb)
    with np.errstate(all='ignore'):
        cosine = np.where(above, np.abs(c) / (ra * rb), 0.0)
        zeta = (b - a) / (2.0 * c)
        t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    cs = 1.0 / np.sqrt(1.0 + t * t)
    sn = cs * t
    cs, sn = np.where(rot, cs, 1.0)[:, None], np.where(rot, sn, 0.0)[:, None]
    i, j = p[rot], q[rot]
    cs, sn = cs[rot], sn[rot]
    W[i], W[j] = cs * W[i] - sn * W[j], sn * W[i] + cs * W[j]
    V[i], V[j] = cs * V[i] - sn * V[j], sn * V[i] + cs * V[j]
    return int(rot.sum()), float(cosine.max())


def eigh_model(A, max_sweeps=MAX_SWEEPS, floor=True, kernel_order=False):
    """-> (lam descending, comps with the eigenvectors as ROWS, first largest component positive, info); with kernel_order every
    dot product is summed in the kernels' order (the norm of A excepted), otherwise pairwise by numpy"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    W, V = A.copy(), np.eye(n)
    scale = math.sqrt(float((A * A).sum()))
    sweeps = total = 0
    ratio, converged = 0.0, False
    while sweeps < max_sweeps and not converged:
        rot, ratio = 0, 0.0
        for r in range(rounds(n)):
            k, c = jacobi_round(W, V, n, r, scale, floor, kernel_order)
            rot, ratio = rot + k, max(ratio, c)
        sweeps, total, converged = sweeps + 1, total + rot, rot == 0
    lam = dots(V, W, kernel_order) / dots(V, V, kernel_order)
    order = np.argsort(-lam, kind='stable')
    comps = V[order]
    first = np.abs(comps).argmax(axis=1)
    comps = comps * np.where(comps[np.arange(n), first] < 0, -1.0, 1.0)[:, None]
    return lam[order], comps, {'sweeps': sweeps, 'converged': converged, 'max_ratio': ratio, 'rotations': total}


def quality(A, lam, comps):
    """the three ratios of a decomposition against numpy.linalg.eigh: eigenvalue error / (eps n |A|_2),
    |comps comps^T - I|_max / (eps n), |A comps^T - comps^T diag(lam)|_max / (eps n |A|_2); and the trace error in the first unit"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    ref = np.sort(np.linalg.eigvalsh(A))[::-1]
    norm2 = float(np.abs(ref).max())
    unit = EPS * n * norm2
    if unit == 0:
        unit = EPS
    return {'values': float(np.abs(np.sort(lam)[::-1] - ref).max()) / unit,
            'orth': float(np.abs(comps @ comps.T - np.eye(n)).max()) / (EPS * n),
            'resid': float(np.abs(A @ comps.T - comps.T * lam[None, :]).max()) / unit,
            'trace': abs(float(lam.sum()) - float(np.trace(A))) / unit}


# -------------------------------------------------------------------------------------------------------------- cases
def psd(n, seed, extra=5):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, n + extra)
    return x @ x.T / (n + extra)


def prescribed(n, seed, power=2.0):
    """Q diag(i^-power) Q^T"""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(n, n))
    lam = np.arange(1, n + 1, dtype=np.float64) ** -power
    return (q * lam[None, :]) @ q.T


def cov_of(z):
    z = np.asarray(z, dtype=np.float64)
    zc = z - z.mean(0)
    return zc.T @ zc / z.shape[0]


def duplicated(seed=3, n=200, D=40, dup=10):
    """a covariance with `dup` duplicated feature columns: rank D - dup, the null rows must stop rotating (the floor)"""
    rng = np.random.RandomState(seed)
    z = rng.randn(n, D)
    z[:, D - dup:] = z[:, :dup]
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return cov_of(z)


def rank_deficient(seed=4):
    """3 samples in D = 7: rank 2"""
    return cov_of(np.random.RandomState(seed).randn(3, 7))


def sym(A):
    return (A + A.T) / 2


@functools.lru_cache(maxsize=None)
def cases():
    """name -> symmetric positive semi-definite matrix; every size of the issue: no pair (1), one pair (2), the bye (3), 7, 64,
    65, the second element per thread (256 / 257), a diagonal matrix, a prescribed power-law spectrum, duplicated columns and a
    rank-deficient covariance"""
    out = {'n1': np.array([[3.5]])}
    for n in (2, 3, 7, 64, 65, 256, 257):
        out['n%d' % n] = sym(psd(n, n))
    out['diag'] = np.diag([4.0, 0.25, 9.0, 1.0, 0.5, 7.0, 2.0, 3.0, 6.0])
    out['powerlaw'] = sym(prescribed(130, 11))
    out['duplicated'] = sym(duplicated())
    out['rank_deficient'] = sym(rank_deficient())
    return out


@functools.lru_cache(maxsize=None)
def model_ratios():
    """the largest ratios of the MODEL over the case table, and every case's info: the yardstick of the GPU test (K = 4 x)"""
    worst = {'values': 0.0, 'orth': 0.0, 'resid': 0.0, 'trace': 0.0}
    infos = {}
    for name, A in cases().items():
        lam, comps, info = eigh_model(A)
        infos[name] = info
        for k, v in quality(A, lam, comps).items():
            worst[k] = max(worst[k], v)
    return worst, infos


def wide_matrix(n, seed):
    """a seeded symmetric matrix for the wide classes (three rounds only, no full solve)"""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, n)
    return (x + x.T) / 2


# --------------------------------------------------------------------------------------------------- covariance, PCA
def cov_from_gram(G):
    """(mean, Cov) from the augmented Gram matrix, operation by operation as dv_spectrum_cov_f64"""
    D = G.shape[0] - 1
    s, n = G[D, :D], G[D, D]
    return s / n, (G[:D, :D] - (s[:, None] * s[None, :]) / n) / n


def gram_of(z):
    z = np.asarray(z, dtype=np.float64)
    zt = np.concatenate([z, np.ones((z.shape[0], 1))], axis=1)
    return zt.T @ zt


def metrics_ref(lam, n):
    lam = np.sort(np.clip(np.asarray(lam, dtype=np.float64), 0, None))[::-1]
    D, tr = lam.size, lam.sum()
    p = lam / tr
    cum = np.cumsum(p)
    out = {'trace': tr, 'lambda_max': lam[0], 'top1_share': p[0]}
    out['explained'] = {str(k): min(cum[k - 1], 1.0) for k in (2 ** i for i in range(13)) if k <= D}
    out['dims_for'] = {'%.2f' % f: int(np.argmax(cum >= f - 1e-15)) + 1 for f in (0.90, 0.95, 0.99)}
    nz = p[p > 0]
    out['effective_rank'] = float(np.exp(-(nz * np.log(nz)).sum()))
    sig = np.sqrt(lam)
    ps = sig / sig.sum() + 1e-7
    out['rankme'] = float(np.exp(-(ps * np.log(ps)).sum()))
    out['participation_ratio'] = float(tr * tr / (lam * lam).sum())
    out['numerical_rank'] = int((lam > D * EPS * lam[0]).sum())
    r = min(int((lam > 1e-12 * lam[0]).sum()), D, n - 1)
    if r >= 2:
        x, y = np.log(np.arange(1, r + 1)), np.log(lam[:r])
        slope, icpt = np.polyfit(x, y, 1)
        res = y - (slope * x + icpt)
        out['alpha'] = -slope
        out['alpha_r2'] = 1.0 - (res * res).sum() / ((y - y.mean()) ** 2).sum()
    else:
        out['alpha'] = out['alpha_r2'] = None
    return out


def project_ref(z, mean, comps, lam, k, whiten=False, eps=1e-12):
    y = (np.asarray(z, dtype=np.float64) - mean) @ comps[:k].T
    return y / np.sqrt(np.clip(lam[:k], 0, None) + eps) if whiten else y


def video_share_ref(z, V, S, mean, comps, lam, k):
    y = project_ref(z, mean, comps, lam, k)
    M = y.reshape(V, S, k).mean(1)
    return S * (M * M).sum(0) / (V * S * lam[:k])


def normalise_ref(clips):
    x = np.asarray(clips, dtype=np.float64).reshape(-1, clips.shape[-1])
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def spectrum_fixture(seed=7, V=24, S=4, D=40):
    """clips [V, S, D] fp32 with three planted strong directions on a common offset: u1 and u2 carry a value per VIDEO (constant
    over its clips: variance 1 and 0.49), u3 a value per CLIP that sums to zero over a video's clips (variance about 0.2), the
    rest isotropic noise of 0.03.  The three leading principal components are then the two video directions and the within-video
    one, in that order."""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(D, D))
    u0, u1, u2, u3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    a, b = rng.randn(V), 0.7 * rng.randn(V)
    pattern = np.array([-1.5, -0.5, 0.5, 1.5]) * 0.4
    c = (0.6 + 0.8 * rng.rand(V))[:, None] * pattern[None, :]
    x = (6.0 * u0[None, None, :] + a[:, None, None] * u1 + b[:, None, None] * u2 + c[:, :, None] * u3 +
         0.03 * rng.randn(V, S, D))
    return x.astype(np.float32), np.arange(V) % 6
