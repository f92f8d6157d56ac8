"""How many dimensions an encoder uses: the eigenvalue spectrum of the covariance of its clip features, label-free.  The Gram
matrix of the features is formed once in double by `dv_ridge_gram_f64` (one class, every label 0: the augmented row and column
hold the column sums and the row count), `dv_spectrum_cov_f64` turns it into mean and covariance, and `eigh_jacobi` diagonalises
the covariance by a parallel-ordered one-sided Jacobi method in double (include/dualvar_spectrum.h): the rounds of a sweep are
launches, the pairs of a round are workgroups, every sum has a fixed order, so the same features give the same bits.  From the
eigenvalues `spectrum_metrics` reads, on the host, the explained variance, the effective rank, RankMe, the participation ratio,
the numerical rank and the power-law decay alpha; `pca_project` projects on the leading components, plain or whitened, with
`dv_gemm_f32_ex`; `spectrum_eval` adds the share of each component's variance that lies between video means, and
`pca_retrieval` repeats the nearest-neighbour retrieval on the projected video features."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib as L
from .. import ops
from . import features as F
from .probe import ridge_gram

MAX_SWEEPS = L.DV_SPECTRUM_MAX_SWEEPS
EPS = 2.0 ** -52


def covariance(z):
    """z [n, D] fp32 on the device -> (mean [D], Cov [D, D]) in float64 on the device, divisor n: dv_ridge_gram_f64 with one
    class and every label 0, then dv_spectrum_cov_f64.  The feature rows are read once, by the Gram kernel."""
    if z.dim() != 2 or z.shape[0] < 1 or not 1 <= z.shape[1] <= L.DV_SPECTRUM_MAX_D:
        raise ValueError('z must be [n, D] clip features with 1 <= D <= %d (DV_SPECTRUM_MAX_D), got %s'
                         % (L.DV_SPECTRUM_MAX_D, tuple(z.shape)))
    L.require_device()
    lib, s = L.load(), ops.stream_ptr()
    dev = z.device if z.is_cuda else torch.device('cuda')
    z = z.to(dev).float().contiguous()
    n, D = z.shape
    ws = F.workspace(lib.dv_ridge_gram_workspace(n, D, 1), dev, 'dv_ridge_gram_workspace')
    label = torch.zeros(n, dtype=torch.int32, device=dev)
    G = torch.empty(D + 1, D + 1, dtype=torch.float64, device=dev)
    B = torch.empty(D + 1, 1, dtype=torch.float64, device=dev)
    ridge_gram(z, label, 1, G, B, 0, ws)
    cov = torch.empty(D, D, dtype=torch.float64, device=dev)
    mean = torch.empty(D, dtype=torch.float64, device=dev)
    L.check(lib.dv_spectrum_cov_f64(G.data_ptr(), D + 1, D, cov.data_ptr(), D, mean.data_ptr(), s), 'dv_spectrum_cov_f64')
    return mean, cov


def eigh_jacobi(A, max_sweeps=MAX_SWEEPS):
    """A [D, D] float64, symmetric positive semi-definite (a covariance) -> (lam [D] descending, comps [D, D] whose ROWS are the
    eigenvectors, info) on the device.  The host loops over sweeps: one dv_spectrum_rounds_f64 call over all rounds and one read
    of its statistics per sweep; it stops after the first sweep without a rotation, or at max_sweeps.
    info = {'sweeps', 'converged', 'max_ratio' (the largest cosine between two rows met in the last sweep), 'rotations' (of all
    sweeps)}.  The final order is a stable descending sort of the D values on the host and a row gather; each eigenvector's sign
    makes its first component of largest magnitude positive.  A NaN met by the kernel raises DualVarHipError."""
    if A.dim() != 2 or A.shape[0] != A.shape[1] or not 1 <= A.shape[0] <= L.DV_SPECTRUM_MAX_D:
        raise ValueError('A must be [D, D] with 1 <= D <= %d (DV_SPECTRUM_MAX_D), got %s' % (L.DV_SPECTRUM_MAX_D, tuple(A.shape)))
    if A.dtype != torch.float64:
        raise ValueError('A must be float64')
    max_sweeps = int(max_sweeps)
    if max_sweeps < 1:
        raise ValueError('max_sweeps = %d: at least one sweep' % max_sweeps)
    L.require_device()
    lib, s = L.load(), ops.stream_ptr()
    dev = A.device if A.is_cuda else torch.device('cuda')
    A = A.to(dev).contiguous()
    n = A.shape[0]
    m = n + (n & 1)
    W, V = torch.empty_like(A), torch.empty_like(A)
    scale = torch.empty(1, dtype=torch.float64, device=dev)
    stat = torch.empty(m, dtype=torch.float64, device=dev)
    lam = torch.empty(n, dtype=torch.float64, device=dev)
    L.check(lib.dv_spectrum_init_f64(A.data_ptr(), n, n, W.data_ptr(), n, V.data_ptr(), n, scale.data_ptr(), s), 'dv_spectrum_init_f64')
    rounds = lib.dv_spectrum_rounds(n)
    if rounds < 0:
        L.check(rounds, 'dv_spectrum_rounds')
    sweeps, total, ratio, converged = 0, 0, 0.0, False
    while sweeps < max_sweeps and not converged:
        L.check(lib.dv_spectrum_rounds_f64(W.data_ptr(), n, V.data_ptr(), n, n, 0, rounds, scale.data_ptr(), stat.data_ptr(), s),
                'dv_spectrum_rounds_f64')
        st = stat.cpu().view(m // 2, 2)
        sweeps += 1
        if bool(torch.isnan(st).any()):
            raise L.DualVarHipError('dv_spectrum_rounds_f64: a row product is NaN in sweep %d: the matrix holds a NaN or overflowed' % sweeps)
        rot = int(st[:, 1].sum())
        total += rot
        ratio = float(st[:, 0].max())
        converged = rot == 0
    L.check(lib.dv_spectrum_values_f64(W.data_ptr(), n, V.data_ptr(), n, n, lam.data_ptr(), s), 'dv_spectrum_values_f64')
    order = torch.sort(lam.cpu(), descending=True, stable=True).indices
    comps = V.cpu()[order]
    first = comps.abs().numpy().argmax(axis=1)               # numpy's argmax: the first of equal magnitudes
    sign = torch.where(comps[torch.arange(n), torch.from_numpy(first)] < 0, -1.0, 1.0).to(torch.float64)
    comps = (comps * sign[:, None]).to(dev)
    info = {'sweeps': sweeps, 'converged': converged, 'max_ratio': ratio, 'rotations': total}
    return lam[order.to(dev)], comps, info


def _entropy_exp(p):
    p = [v for v in p if v > 0]
    return math.exp(-sum(v * math.log(v) for v in p))


def spectrum_metrics(lam, n):
    """lam: the eigenvalues (any order; clipped at 0 and sorted descending here), n: the samples behind the covariance -> the
    label-free figures, pure host float64:
      trace, lambda_max, top1_share; explained {k: cumulative share} at k = 1, 2, 4, ... <= D; dims_for {'0.90', '0.95', '0.99':
      the smallest k reaching that share}; effective_rank = exp H(lam / sum lam) (0 log 0 = 0); rankme = exp H(p) with
      p = sigma / sum sigma + 1e-7, sigma = sqrt(lam); participation_ratio = (sum lam)^2 / sum lam^2;
      numerical_rank = #{lam_i > D eps lam_1}; alpha, alpha_r2: the negated slope and R^2 of the least-squares line of
      log lam_i on log i over the ranks 1 .. r, r = #{lam_i > 1e-12 lam_1} capped at min(D, n - 1) (None below two ranks)."""
    if isinstance(lam, np.ndarray):
        lam = np.ascontiguousarray(lam)                      # a reversed view has negative strides
    lam = torch.as_tensor(lam).detach().reshape(-1).cpu().to(torch.float64)
    lam = torch.sort(torch.clamp(lam, min=0.0), descending=True, stable=True).values
    D = lam.numel()
    v = lam.tolist()
    trace = math.fsum(v)
    out = {'D': D, 'n': int(n), 'trace': trace, 'lambda_max': v[0]}
    if not trace > 0:
        out.update(top1_share=None, explained={}, dims_for={}, effective_rank=0.0, rankme=0.0, participation_ratio=0.0,
                   numerical_rank=0, alpha=None, alpha_r2=None)
        return out
    cum, acc = [], 0.0
    for x in v:
        acc += x
        cum.append(min(acc / trace, 1.0))
    cum[-1] = 1.0
    out['top1_share'] = v[0] / trace
    ks, k = [], 1
    while k <= D:
        ks.append(k)
        k *= 2
    out['explained'] = {str(k): cum[k - 1] for k in ks}
    out['dims_for'] = {'%.2f' % f: next(i + 1 for i, c in enumerate(cum) if c >= f) for f in (0.90, 0.95, 0.99)}
    out['effective_rank'] = _entropy_exp([x / trace for x in v])
    sig = [math.sqrt(x) for x in v]
    ssum = math.fsum(sig)
    out['rankme'] = _entropy_exp([x / ssum + 1e-7 for x in sig])
    out['participation_ratio'] = trace * trace / math.fsum(x * x for x in v)
    out['numerical_rank'] = sum(1 for x in v if x > D * EPS * v[0])
    r = min(sum(1 for x in v if x > 1e-12 * v[0]), D, max(int(n) - 1, 0))
    out['alpha'] = out['alpha_r2'] = None
    if r >= 2:
        xs = [math.log(i + 1.0) for i in range(r)]
        ys = [math.log(v[i]) for i in range(r)]
        mx, my = math.fsum(xs) / r, math.fsum(ys) / r
        sxx = math.fsum((x - mx) ** 2 for x in xs)
        sxy = math.fsum((x - mx) * (y - my) for x, y in zip(xs, ys))
        syy = math.fsum((y - my) ** 2 for y in ys)
        slope = sxy / sxx
        out['alpha'] = -slope
        out['alpha_r2'] = 1.0 if syy == 0 else 1.0 - math.fsum((y - my - slope * (x - mx)) ** 2 for x, y in zip(xs, ys)) / syy
    return out


def pca_project(z, mean, comps, lam, k, whiten=False, eps=1e-12):
    """z [n, D] fp32 on the device -> y [n, k] fp32 = (z - mean) comps[:k]^T by dv_gemm_f32_ex: the components go in through the
    B strides and -mean comps[:k]^T (the same kernel, one row, alpha = -1) as the bias.  With whiten row j of comps[:k] is scaled
    by 1 / sqrt(lam_j + eps) in double before the single cast to fp32, so the projected training rows have unit variance."""
    if z.dim() != 2 or comps.dim() != 2 or comps.shape[1] != z.shape[1] or mean.numel() != z.shape[1]:
        raise ValueError('z must be [n, D], mean [D] and comps [*, D], got %s, %s and %s' % (tuple(z.shape), tuple(mean.shape), tuple(comps.shape)))
    k = int(k)
    if not 1 <= k <= comps.shape[0]:
        raise ValueError('k = %d: between 1 and the %d components' % (k, comps.shape[0]))
    L.require_device()
    lib, s = L.load(), ops.stream_ptr()
    dev = z.device if z.is_cuda else torch.device('cuda')
    z = z.to(dev).float().contiguous()
    n, D = z.shape
    c = comps[:k].to(device=dev, dtype=torch.float64)
    if whiten:
        c = c * (1.0 / torch.sqrt(torch.clamp(lam[:k].to(device=dev, dtype=torch.float64), min=0.0) + float(eps)))[:, None]
    c32 = c.to(torch.float32).contiguous()
    m32 = mean.to(device=dev, dtype=torch.float32).reshape(1, D).contiguous()
    bias = torch.empty(1, k, dtype=torch.float32, device=dev)
    y = torch.empty(n, k, dtype=torch.float32, device=dev)
    for d in (F.gemm_desc(m32.data_ptr(), c32.data_ptr(), bias.data_ptr(), 1, k, D, 1, D, alpha=-1.0),
              F.gemm_desc(z.data_ptr(), c32.data_ptr(), y.data_ptr(), n, k, D, 1, D, bias=bias.data_ptr())):
        L.check(lib.dv_gemm_f32_ex(C.byref(d), s), 'dv_gemm_f32_ex')
    return y


def spectrum_eval(clips, video_label=None, ks=(32, 64, 128)):
    """clips [V, S, D] (a video's clips adjacent), normalised as the ridge probe does (features.normalise, not centred) -> {'metrics'
    (spectrum_metrics), 'info' (eigh_jacobi), 'video_share' [k_max], 'ks' (clamped to D), 'mean' [D], 'components' [D, D],
    'eigenvalues' [D]} (the last three float64 on the device).
    video_share[j] is the share of component j's variance that lies between the video means: the clips are projected on the top
    k_max = max(ks) components, dv_group_mean_f32 averages a video's S clips to M [V, k_max], and the share is
    S sum_v M[v, j]^2 / (n lam_j) with n = V S; None where lam_j is not above the numerical-rank threshold D eps lam_1.
    video_label is not needed (a video is S adjacent rows); it is accepted so that callers can pass what they hold."""
    feat, _, _, V, S = F.clip_rows(clips, video_label)
    D = feat.shape[1]
    if not 1 <= D <= L.DV_SPECTRUM_MAX_D:
        raise ValueError('D = %d: the spectrum kernels keep 1 <= D <= %d (DV_SPECTRUM_MAX_D)' % (D, L.DV_SPECTRUM_MAX_D))
    ks = sorted({min(int(k), D) for k in ks})
    if not ks or ks[0] < 1:
        raise ValueError('every k must be at least 1')
    L.require_device()
    z = F.normalise(feat)
    n = V * S
    mean, cov = covariance(z)
    lam, comps, info = eigh_jacobi(cov)
    kmax = ks[-1]
    y = pca_project(z, mean, comps, lam, kmax)
    M = torch.empty(V, kmax, dtype=torch.float32, device=y.device)
    L.check(L.load().dv_group_mean_f32(y.data_ptr(), V, S, kmax, M.data_ptr(), ops.stream_ptr()), 'dv_group_mean_f32')
    between = (M.double() ** 2).sum(dim=0).cpu().tolist()
    lam_h = lam.cpu().tolist()
    floor = D * EPS * max(lam_h[0], 0.0)
    share = [S * between[j] / (n * lam_h[j]) if lam_h[j] > floor else None for j in range(kmax)]
    return {'metrics': spectrum_metrics(lam, n), 'info': info, 'video_share': share, 'ks': ks, 'mean': mean, 'components': comps,
            'eigenvalues': lam}


def pca_retrieval(train_video_feat, train_label, test_video_feat, test_label, mean, comps, lam, ks):
    """{k: {'pca': acc@1, 'whitened': acc@1}}: both splits' video features [*, D], normalised like the clips of the fit, are
    projected on the top k components of the TRAIN fit (mean, comps, lam of spectrum_eval), plain and whitened, and scored by the
    existing nn_retrieval (which centres and normalises again and keeps k a multiple of 8)."""
    from .retrieval import nn_retrieval
    out = {}
    tr, te = F.normalise(train_video_feat), F.normalise(test_video_feat)
    for k in ks:
        k = int(k)
        if k % 8:
            raise ValueError('k = %d: the retrieval kernels take a multiple of 8 columns' % k)
        row = {}
        for name, whiten in (('pca', False), ('whitened', True)):
            acc, _ = nn_retrieval(pca_project(te, mean, comps, lam, k, whiten=whiten), test_label,
                                  pca_project(tr, mean, comps, lam, k, whiten=whiten), train_label, ks=(1,))
            row[name] = acc[1]
        out[k] = row
    return out
