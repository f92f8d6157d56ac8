"""Float64 numpy reference of the t-SNE entries, written from include/dualvar_tsne.h (not from the kernels): the distances and
exclusions of a neighbour list, the entropy and its bisection, the sparse symmetrised P from forward lists, the gradient with Z
and the cross-entropy, the update step, and a whole embedding loop on tsne_embed's schedule.  Dense [n, n] arrays throughout:
for the few hundred points of the tests only."""
import math

import numpy as np

BETA_START, MAX_STEPS, ENTROPY_TOL = 1.0, 100, 1e-5        # DV_TSNE_BETA_START, DV_TSNE_MAX_STEPS, DV_TSNE_ENTROPY_TOL
F32 = np.float32


def list_distances(val, idx, row0=0):
    """val [n, k1] f32, idx [n, k1] int -> (e [n, k1] f32, included [n, k1] bool): the header's fp32 expressions, each step one
    IEEE operation, so e carries the very bits the kernel works on; e = 0 in excluded slots"""
    val, idx = np.asarray(val, dtype=F32), np.asarray(idx)
    n = val.shape[0]
    inc = (idx >= 0) & (idx != (row0 + np.arange(n))[:, None])
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.fmax(F32(2.0) - F32(2.0) * val, F32(0.0)).astype(F32)
        m = np.where(inc, d, np.inf).min(1, keepdims=True).astype(F32)
        e = np.where(inc & (d != m), d - m, F32(0.0)).astype(F32)
    return e, inc


def entropy(e, inc, beta):
    """one row in float64: (H, w, S) at beta, H = log S + beta sum(w e) / S, w = exp(-beta e) over the included slots"""
    e64 = np.asarray(e, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        w = np.where(inc, np.exp(-float(beta) * e64), 0.0)
        we = np.where(w > 0, w * np.where(np.isfinite(e64), e64, 0.0), 0.0)
    S = w.sum()
    return math.log(S) + float(beta) * we.sum() / S, w, S


def bisect_row(e, inc, perplexity):
    """the header's bisection for one row, evaluated in float64 -> (p, beta)"""
    k = int(inc.sum())
    if k == 0:
        return np.zeros(e.shape), 0.0
    if not (np.where(inc, e, 0) > 0).any():
        return np.where(inc, 1.0 / k, 0.0), BETA_START
    target = float(F32(math.log(float(F32(perplexity)))))
    beta, lo, hi = BETA_START, 0.0, math.inf
    for step in range(MAX_STEPS):
        H, w, S = entropy(e, inc, beta)
        if abs(H - target) <= ENTROPY_TOL or step == MAX_STEPS - 1:
            break
        if H > target:
            lo, beta = beta, (beta * 2.0 if hi == math.inf else (beta + hi) * 0.5)
        else:
            hi, beta = beta, (lo + beta) * 0.5
    return w / S, beta


def perplexity_ref(val, idx, perplexity, row0=0):
    """-> (p [n, k1] f64, beta [n] f64)"""
    e, inc = list_distances(val, idx, row0)
    rows = [bisect_row(e[r], inc[r], perplexity) for r in range(e.shape[0])]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])


def forward_edges(idx, p, n):
    """the forward edges the header lets contribute: (i, j, p) with p > 0 and 0 <= j < n"""
    idx, p = np.asarray(idx), np.asarray(p, dtype=np.float64)
    ok = (p > 0) & (idx >= 0) & (idx < n)
    i, s = np.nonzero(ok)
    return i, idx[i, s], p[i, s]


def sparse_P(idx, p, n):
    """dense P [n, n] f64 = (p_{j|i} + p_{i|j}) / 2n from the forward lists alone (a target listed twice adds twice)"""
    i, j, pe = forward_edges(idx, p, n)
    P = np.zeros((n, n))
    np.add.at(P, (i, j), pe)
    return (P + P.T) / (2.0 * n)


def pair_terms(y):
    """y [n, 2] f64 -> (diff [n, n, 2], d2 [n, n], q [n, n] with a zero diagonal)"""
    y = np.asarray(y, dtype=np.float64)
    diff = y[:, None, :] - y[None, :, :]
    d2 = (diff ** 2).sum(2)
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    return diff, d2, q


def repulsion(y):
    """-> (fr [n, 2], Z, abs_fr [n, 2], the sums of |term|)"""
    diff, _, q = pair_terms(y)
    t = (q ** 2)[:, :, None] * diff
    return t.sum(1), q.sum(), np.abs(t).sum(1)


def attraction(P, y):
    """-> (fa [n, 2], ce_row [n], abs_fa [n, 2])"""
    diff, d2, q = pair_terms(y)
    t = (P * q)[:, :, None] * diff
    return t.sum(1), (P * np.log1p(d2)).sum(1), np.abs(t).sum(1)


def gradient(P, y, exaggeration=1.0):
    """dKL/dy [n, 2] = 4 (exaggeration fa - fr / Z), with Z and the cross-entropy CE = sum P log(1 + d2) + log Z.  The sums
    sum_j W_ij (y_i - y_j) are taken as (sum_j W_ij) y_i - W y: the same numbers as attraction / repulsion give, without the
    [n, n, 2] arrays (tests/test_tsne_host.py compares the two forms)"""
    y = np.asarray(y, dtype=np.float64)
    d2 = ((y[:, None, :] - y[None, :, :]) ** 2).sum(2)
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    Wa, Wr = P * q, q * q
    fa = Wa.sum(1)[:, None] * y - Wa @ y
    fr = Wr.sum(1)[:, None] * y - Wr @ y
    return 4.0 * (exaggeration * fa - fr / Z), Z, (P * np.log1p(d2)).sum() + math.log(Z)


def kl(P, y):
    """KL(P || Q), Q_ij = q_ij / Z"""
    _, _, q = pair_terms(y)
    Q = q / q.sum()
    m = P > 0
    return float((P[m] * np.log(P[m] / Q[m])).sum())


def update(y, vel, gain, g, momentum, lr, min_gain=0.01):
    """one step of the header's update in float64 (0.2 and 0.8 as the fp32 constants the kernel holds) -> (y, vel, gain)"""
    gain = np.where((g > 0) != (vel > 0), gain + float(F32(0.2)), gain * float(F32(0.8)))
    gain = np.maximum(gain, min_gain)
    vel = momentum * vel - (lr * gain) * g
    return y + vel, vel, gain


def embed(P, y0, n_iter, exaggeration=12.0, exaggeration_iter=250, lr=None, trace_every=50):
    """tsne_embed's schedule in float64 -> (y, trace) with trace as tsne_embed's"""
    n = P.shape[0]
    lr = max(n / float(exaggeration) / 4.0, 50.0) if lr is None else lr
    y = np.array(y0, dtype=np.float64)
    vel, gain = np.zeros_like(y), np.ones_like(y)
    trace = {'iter': [], 'ce': [], 'z': []}
    for it in range(n_iter + 1):
        early = it < exaggeration_iter
        g, Z, ce = gradient(P, y, exaggeration if early else 1.0)
        if it == n_iter or it % trace_every == 0:
            trace['iter'].append(it)
            trace['ce'].append(ce)
            trace['z'].append(Z)
        if it == n_iter:
            break
        y, vel, gain = update(y, vel, gain, g, 0.5 if early else 0.8, lr)
    return y, trace


def knn_purity(y, cls, k=10):
    """share of the k nearest neighbours of a point (itself left out) with its class id"""
    y, cls = np.asarray(y, dtype=np.float64), np.asarray(cls)
    d2 = ((y[:, None, :] - y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    nn = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return float((cls[nn] == cls[:, None]).mean())


def reverse_csr_brute(idx, included):
    """(rev_ptr, rev_edge) by two loops"""
    idx, included = np.asarray(idx), np.asarray(included)
    n, ldk = idx.shape
    ptr, edge = [0], []
    for i in range(n):
        for f in range(n * ldk):
            if included.reshape(-1)[f] and idx.reshape(-1)[f] == i:
                edge.append(f)
        ptr.append(len(edge))
    return np.array(ptr), np.array(edge, dtype=np.int64)
