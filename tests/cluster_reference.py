"""float64 numpy reference of include/dualvar_cluster.h, written from the header (not from the kernels): the three entries,
Lloyd's loop of dualvar_amd/utils/cluster.py and the scores of cluster_metrics.  Used by test_cluster_host.py and
test_cluster_gpu.py."""
import itertools
import math

import numpy as np

MAX_K = 4096
PART = 64
SORT_ROWS = 512
SEED_BLOCK = 256


# -------------------------------------------------------------------------------------------------------------- entries
def assign_ref(sim, K, old):
    """sim [R, >= K] float32, old [R] -> (assign [R] i32, best [R] f32, changed): the lowest column among the row's largest
    values that are not NaN (-0.0 == +0.0); a row of NaN only gets (-1, -inf)"""
    R = sim.shape[0]
    assign, best = np.full(R, -1, dtype=np.int32), np.full(R, -np.inf, dtype=np.float32)
    for r in range(R):
        row = sim[r, :K]
        ok = ~np.isnan(row)
        if ok.any():
            m = row[ok].max()
            j = int(np.nonzero(ok & (row == m))[0][0])
            assign[r], best[r] = j, row[j]
    return assign, best, int((assign != np.asarray(old)).sum())


def update_ref(z, assign, best, K, cent_in):
    """-> (cent [K, D] float64 before the rounding to fp32, None for a cluster that keeps cent_in; counts; within; s [K, D];
    mass [K, D] = sum |z| over the members, for the bound)"""
    z64 = np.asarray(z, dtype=np.float64)
    n, D = z64.shape
    counts, within = np.zeros(K, dtype=np.int64), np.zeros(K)
    s, mass = np.zeros((K, D)), np.zeros((K, D))
    cent = []
    for k in range(K):
        m = np.nonzero(np.asarray(assign) == k)[0]
        counts[k] = m.size
        within[k] = np.asarray(best, dtype=np.float64)[m].sum()
        s[k] = z64[m].sum(0)
        mass[k] = np.abs(z64[m]).sum(0)
        nrm = math.sqrt(float((s[k] * s[k]).sum()))
        cent.append(s[k] / nrm if m.size and nrm > 0 and math.isfinite(nrm) else None)
    return cent, counts, within, s, mass


def dot_ref(z, c):
    """-> (s [n] float64, bound [n]): a lane's chain holds 4 ceil(D / 256) sums, the wave fold six more, every product is
    rounded once: (4 ceil(D / 256) + 7) 2^-24 sum_d |z_rd c_d|"""
    z, c = np.asarray(z, dtype=np.float64), np.asarray(c, dtype=np.float64)
    D = z.shape[1]
    return z @ c, (4 * -(-D // 256) + 7) * 2.0 ** -24 * (np.abs(z) @ np.abs(c))


def seed_mind_ref(s, mind, first):
    """the fp32 formula of the header, operation by operation"""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        d = np.float32(2.0) - np.float32(2.0) * s
    d = np.where(np.isnan(d), np.float32(0), np.maximum(d, np.float32(0))).astype(np.float32)
    return d if first else np.minimum(np.asarray(mind, dtype=np.float32), d)


def seed_cum_ref(mind):
    """-> (cum [n] float64 in the header's order: T_b + p_r, total)"""
    m = np.asarray(mind, dtype=np.float64)
    n = m.size
    cum, T = np.zeros(n), 0.0
    for b0 in range(0, n, SEED_BLOCK):
        p = np.cumsum(m[b0:b0 + SEED_BLOCK])                 # one addition after the other, in ascending order
        cum[b0:b0 + SEED_BLOCK] = T + p
        T = T + float(p[-1])
    return cum, T


def kmeanspp_ref(z, k, gen):
    """the seeding of dualvar_amd/utils/cluster.py in float64 with the draws taken from `gen` in its order -> the rows chosen"""
    import torch
    z = np.asarray(z, dtype=np.float64)
    n = z.shape[0]

    def draw():
        return float(torch.rand((), generator=gen, dtype=torch.float64))
    index, mind = [min(int(draw() * n), n - 1)], None
    for j in range(1, k):
        u = draw()
        mind = seed_mind_ref((z @ z[index[-1]]).astype(np.float32), mind, j == 1)
        pick = seed_pick_ref(mind, u)[0]
        index.append(pick if pick >= 0 else min(int(draw() * n), n - 1))
    return index


def seed_pick_ref(mind, u):
    cum, total = seed_cum_ref(mind)
    if total == 0:
        return -1, total
    hit = np.nonzero(cum > u * total)[0]
    if hit.size:
        return int(hit[0]), total
    return int(np.nonzero(np.asarray(mind) > 0)[0][-1]), total


def update_workspace_bytes(n, D, K):
    P, B = n // PART + K, -(-n // SORT_ROWS)
    return (8 * (P * D + P + K * D) + 4 * (B * K + 2 * (K + 1) + n) + 7) // 8 * 8


def seed_workspace_bytes(n):
    return 8 * -(-n // SEED_BLOCK)


# ----------------------------------------------------------------------------------------------------------------- Lloyd
def fit_fixture(groups=6, per=50, D=32, noise=0.05, seed=0):
    """-> (x [groups * per, D] float32, cls): `per` points around each of `groups` random directions, row = group * per + i;
    the noise (0.05 a coordinate, 0.28 in norm) is small against the distance of two directions (about 1.4)"""
    rng = np.random.RandomState(seed)
    c = rng.randn(groups, D)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = np.repeat(c, per, axis=0) + noise * rng.randn(groups * per, D)
    return x.astype(np.float32), np.repeat(np.arange(groups), per)


def centre_normalise(x):
    """the features as retrieval prepares them: minus the mean row, then unit rows (float64)"""
    x = np.asarray(x, dtype=np.float64)
    x = x - x.mean(0)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def lloyd_ref(z, init, n_iter=100):
    """spherical k-means from the centroids `init` on the rows z as they are, in float64 -> (assign, centroids, trace)"""
    z = np.asarray(z, dtype=np.float64)
    cent = np.asarray(init, dtype=np.float64).copy()
    K = cent.shape[0]
    assign = np.full(z.shape[0], -1)
    trace = []
    for _ in range(n_iter):
        sim = z @ cent.T
        new = sim.argmax(1)                                  # the lowest index among equals
        best = sim[np.arange(z.shape[0]), new]
        changed = int((new != assign).sum())
        assign = new
        got, _, within, _, _ = update_ref(z, assign, best, K, cent)
        cent = np.stack([cent[k] if got[k] is None else got[k] for k in range(K)])
        trace.append({'objective': float(within.sum()), 'changed': changed})
        if changed == 0:
            break
    return assign, cent, trace


# ---------------------------------------------------------------------------------------------------------------- scores
def contingency(assign, cls):
    a, c = np.asarray(assign), np.asarray(cls)
    t = np.zeros((int(a.max()) + 1, int(c.max()) + 1))
    for i, j in zip(a, c):
        t[i, j] += 1
    return t


def nmi_ref(assign, cls):
    """I(U; V) / ((H(U) + H(V)) / 2) from the definitions"""
    t = contingency(assign, cls)
    n = t.sum()
    pu, pv = t.sum(1) / n, t.sum(0) / n
    hu = -sum(p * math.log(p) for p in pu if p > 0)
    hv = -sum(p * math.log(p) for p in pv if p > 0)
    mi = sum(t[i, j] / n * math.log(t[i, j] / n / (pu[i] * pv[j])) for i in range(t.shape[0]) for j in range(t.shape[1]) if t[i, j] > 0)
    return 1.0 if hu == 0 and hv == 0 else mi / (0.5 * (hu + hv))


def ari_ref(assign, cls):
    """from the pair counts over all unordered pairs of rows: 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn))"""
    a, c = np.asarray(assign), np.asarray(cls)
    same_a, same_c = a[:, None] == a[None, :], c[:, None] == c[None, :]
    iu = np.triu_indices(a.size, 1)
    sa, sc = same_a[iu], same_c[iu]
    tp, tn = float((sa & sc).sum()), float((~sa & ~sc).sum())
    fp, fn = float((sa & ~sc).sum()), float((~sa & sc).sum())
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def purity_ref(assign, cls):
    t = contingency(assign, cls)
    return float(t.max(1).sum() / t.sum())


def accuracy_brute(table):
    """the best one-to-one map of clusters to classes over ALL of them: permutations of the larger side (for tables up to 6)"""
    t = np.asarray(table, dtype=np.float64)
    if t.shape[0] > t.shape[1]:
        t = t.T
    r, c = t.shape
    assert c <= 6
    return max(sum(t[i, p[i]] for i in range(r)) for p in itertools.permutations(range(c), r)) / t.sum()


def video_consistency_ref(assign, vid):
    a, v = np.asarray(assign), np.asarray(vid)
    shares = []
    for x in sorted(set(v.tolist())):
        mine = a[v == x]
        shares.append(max(int((mine == k).sum()) for k in set(mine.tolist())) / mine.size)
    return float(np.mean(shares))
