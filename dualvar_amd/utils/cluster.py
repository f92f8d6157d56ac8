"""Label-free evaluation of an encoder's clip features: spherical k-means (Lloyd's algorithm on cosine similarity, k-means++
seeding, the best of several restarts) on the entries of include/dualvar_cluster.h, scored against the classes afterwards (NMI,
ARI, purity, matched accuracy) and against the videos (how often the clips of one video share a cluster: the discrete
counterpart of the intra-video variance).  The features are prepared exactly as retrieval prepares them.  The [n, K] similarity
arrives in row blocks from `dv_gemm_f32` in one reused workspace; all arithmetic over the n x D features and the n x K
similarities runs in the HIP library, every sum in a fixed order, so one seed gives one result bit for bit.  The host does the
control flow, draws the random numbers (one CPU generator, float64) and does float64 bookkeeping on K- and K x C-sized tables."""
import numpy as np
import torch

from .. import _lib as L
from .. import ops
from . import features as F


def _check_fit_args(feat, k, n_iter, n_init, init):
    if feat.dim() != 2 or feat.shape[0] < 1:
        raise ValueError('feat must be [n, D] clip features, got %s' % (tuple(feat.shape),))
    if not 1 <= k <= L.DV_KMEANS_MAX_K:
        raise ValueError('k = %d: the k-means kernels keep 1 <= k <= %d (DV_KMEANS_MAX_K) clusters' % (k, L.DV_KMEANS_MAX_K))
    if k > feat.shape[0]:
        raise ValueError('k = %d clusters for n = %d rows' % (k, feat.shape[0]))
    if n_iter < 1 or n_init < 1:
        raise ValueError('n_iter and n_init must be at least 1')
    if init is not None and (init.dim() != 2 or tuple(init.shape) != (k, feat.shape[1])):
        raise ValueError('init must be [k, D] = [%d, %d], got %s' % (k, feat.shape[1], tuple(init.shape)))
    if not feat.is_cuda or (init is not None and not init.is_cuda):
        raise ValueError('feat (and init) must be device tensors (the kernels read the pointers as they are)')


class _Fit:
    """the device arrays one fit reuses over its restarts and iterations"""

    def __init__(self, z, k, row_block):
        self.z, self.k = z, k
        self.n, self.D = z.shape
        dev, lib = z.device, L.load()
        row_block, _ = F.blocks(self.n, k, row_block, None)              # 4096 rows by default, as the sibling walks
        self.walk = F.SimilarityWalk(row_block, k, dev)                  # the bank is the centroids: one chunk of k columns
        self.assign = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.best = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.changed = torch.zeros(1, dtype=torch.int64, device=dev)             # the kernel's uint64
        self.counts = torch.empty(k, dtype=torch.int32, device=dev)
        self.within = torch.empty(k, dtype=torch.float64, device=dev)
        self.update_ws = F.workspace(lib.dv_kmeans_update_workspace(self.n, self.D, k), dev, 'dv_kmeans_update_workspace')
        self.seed_ws = F.workspace(lib.dv_kmeans_seed_workspace(self.n), dev, 'dv_kmeans_seed_workspace')
        self.col = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.mind = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.pick = torch.empty(1, dtype=torch.int32, device=dev)
        self.total = torch.empty(1, dtype=torch.float64, device=dev)

    def assign_step(self, cent):
        """the arg-max of every row against cent [k, D], one row block of similarities at a time; the rows whose cluster changed
        add up in self.changed"""
        lib, s, sim = L.load(), ops.stream_ptr(), self.walk.sim
        self.changed.zero_()
        for r0, nr, _, _, _, _ in self.walk(self.z, cent):
            L.check(lib.dv_kmeans_assign_f32(sim.data_ptr(), self.k, nr, self.k, self.assign.data_ptr() + 4 * r0,
                                             self.best.data_ptr() + 4 * r0, self.changed.data_ptr(), s), 'dv_kmeans_assign_f32')

    def update_step(self, cent_in, cent_out):
        L.check(L.load().dv_kmeans_update_f32(self.z.data_ptr(), self.D, self.n, self.D, self.assign.data_ptr(), self.best.data_ptr(),
                                              self.k, cent_in.data_ptr(), cent_out.data_ptr(), self.D, self.counts.data_ptr(),
                                              self.within.data_ptr(), self.update_ws.data_ptr(), ops.stream_ptr()),
                'dv_kmeans_update_f32')

    def seed(self, gen):
        """k-means++: the first centre uniformly, each further one with probability proportional to its squared distance to the
        nearest centre so far -> (cent [k, D], the rows chosen)"""
        lib, s, n = L.load(), ops.stream_ptr(), self.n

        def uniform():
            return min(int(float(torch.rand((), generator=gen, dtype=torch.float64)) * n), n - 1)
        index = [uniform()]
        cent = torch.empty(self.k, self.D, dtype=torch.float32, device=self.z.device)
        cent[0] = self.z[index[0]]
        for j in range(1, self.k):
            u = float(torch.rand((), generator=gen, dtype=torch.float64))
            L.check(lib.dv_kmeans_dot_f32(self.z.data_ptr(), self.D, n, self.D, cent.data_ptr() + 4 * (j - 1) * self.D,
                                          self.col.data_ptr(), s), 'dv_kmeans_dot_f32')
            L.check(lib.dv_kmeans_seed_f32(self.col.data_ptr(), n, self.mind.data_ptr(), int(j == 1), u, self.pick.data_ptr(),
                                           self.total.data_ptr(), self.seed_ws.data_ptr(), s), 'dv_kmeans_seed_f32')
            pick = int(self.pick.item())
            if pick < 0:                 # every row sits on a centre already
                pick = uniform()
            index.append(pick)
            cent[j] = self.z[pick]
        return cent, index

    def lloyd(self, cent, n_iter):
        """-> dict of one run from the centroids `cent` (left unchanged)"""
        self.assign.fill_(-1)
        cur, nxt = cent.clone(), torch.empty_like(cent)
        trace = []
        for it in range(n_iter):
            self.assign_step(cur)
            self.update_step(cur, nxt)
            cur, nxt = nxt, cur
            within, changed = self.within.cpu(), int(self.changed.item())
            objective = 0.0
            for w in within.tolist():                                            # ascending k, float64
                objective += w
            trace.append({'objective': objective, 'changed': changed})
            if changed == 0:
                break
        counts = self.counts.cpu()
        return {'assign': self.assign.clone(), 'centroids': cur, 'objective': trace[-1]['objective'], 'trace': trace,
                'iterations': len(trace), 'empty': int((counts == 0).sum()), 'sizes': [int(c) for c in counts]}


def kmeans_fit(feat, k, n_iter=100, n_init=10, seed=0, centre=True, init=None, row_block=None):
    """feat [n, D] clip features on the device -> {'assign' [n] i32 and 'centroids' [k, D] f32 on the device, 'objective'
    (float64: the sum over the rows of the similarity to their centroid, as the last assignment saw it), 'trace' (objective and
    changed rows per iteration), 'iterations', 'empty' (clusters without a member), 'sizes', 'init_index' (the rows k-means++
    chose, None with `init`), 'restart'}.

    Spherical k-means on the features centred and L2-normalised as retrieval does (centre=False: normalised only).  An iteration
    assigns every row to the centroid of largest cosine similarity (lowest index among equals) and replaces each centroid by the
    normalised sum of its members; an empty cluster keeps its centroid.  It stops when no row changes cluster or after n_iter
    iterations.  Of the n_init restarts the one of largest objective is kept, the lowest restart among equals.  All draws come
    from one CPU torch.Generator seeded with `seed`, in float64.  An explicit `init` [k, D] on the device (rows used as they are)
    skips seeding and restarts."""
    k, n_iter, n_init = int(k), int(n_iter), int(n_init)
    _check_fit_args(feat, k, n_iter, n_init, init)
    L.require_device()
    f = _Fit(F.normalise(feat, centre), k, row_block)
    if init is not None:
        res = f.lloyd(init.float().contiguous(), n_iter)
        res.update(init_index=None, restart=0)
        return res
    gen = torch.Generator().manual_seed(int(seed))
    keep = None
    for restart in range(n_init):
        cent, index = f.seed(gen)
        res = f.lloyd(cent, n_iter)
        res.update(init_index=index, restart=restart)
        if keep is None or res['objective'] > keep['objective']:
            keep = res
    return keep


# ------------------------------------------------------------------------------------------------ the scores (host, float64)
def _assign_min_cost(cost):
    """cost [r, c] float64, r <= c -> the column of every row in a one-to-one assignment of least total cost (the Hungarian
    method with potentials, O(r^2 c); the scan over the columns is vectorised)"""
    r, c = cost.shape
    u, v = np.zeros(r + 1), np.zeros(c + 1)
    owner = np.zeros(c + 1, dtype=np.int64)                  # the row (1-based) that holds column j; 0: free
    way = np.zeros(c + 1, dtype=np.int64)
    for i in range(1, r + 1):
        owner[0] = i
        j0 = 0
        minv = np.full(c + 1, np.inf)
        used = np.zeros(c + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = owner[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(used[1:], np.inf, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[owner[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if owner[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            owner[j0] = owner[j1]
            j0 = j1
    col = np.zeros(r, dtype=np.int64)
    for j in range(1, c + 1):
        if owner[j]:
            col[owner[j] - 1] = j - 1
    return col


def best_matching(table):
    """table [K, C] of counts -> (the largest sum of table[k][m(k)] over the one-to-one maps m of clusters to classes - the
    smaller side is matched completely - , the pairs (k, c) of such a map)"""
    t = np.asarray(table, dtype=np.float64)
    if t.shape[0] <= t.shape[1]:
        col = _assign_min_cost(-t)
        pairs = [(k, int(c)) for k, c in enumerate(col)]
    else:
        col = _assign_min_cost(-t.T)
        pairs = [(int(k), c) for c, k in enumerate(col)]
    return float(sum(t[k, c] for k, c in pairs)), pairs


def _entropy(counts, n):
    p = counts[counts > 0] / n
    return float(-(p * np.log(p)).sum())


def cluster_metrics(assign, cls, vid=None, n_class=None):
    """assign [n] cluster per row (a negative entry is a row without a cluster: left out and counted in 'unassigned'), cls [n]
    class per row -> {'nmi' (arithmetic-mean normalisation), 'ari', 'purity', 'accuracy' (under the best one-to-one map of
    clusters to classes), 'sizes', 'n', 'unassigned', 'n_cluster', 'n_class'} from the K x C contingency table, in float64 on the
    host; with vid [n], 'video_consistency': the mean over the videos of the largest share of a video's clips in one cluster."""
    a = np.asarray(torch.as_tensor(assign).cpu()).astype(np.int64).reshape(-1)
    c = np.asarray(torch.as_tensor(cls).cpu()).astype(np.int64).reshape(-1)
    if a.shape != c.shape:
        raise ValueError('assign and cls must hold one entry per row, got %d and %d' % (a.size, c.size))
    if c.size and c.min() < 0:
        raise ValueError('cls must not be negative')
    ok = a >= 0
    K = int(a.max()) + 1 if ok.any() else 1
    C = max(int(c.max()) + 1 if c.size else 1, int(n_class or 0))
    table = np.bincount(a[ok] * C + c[ok], minlength=K * C).reshape(K, C).astype(np.float64)
    n = float(table.sum())
    rep = {'n': int(n), 'unassigned': int((~ok).sum()), 'n_cluster': K, 'n_class': C, 'sizes': [int(v) for v in table.sum(1)]}
    if n == 0:
        rep.update(nmi=None, ari=None, purity=None, accuracy=None)
    else:
        rows, cols = table.sum(1), table.sum(0)
        hu, hv = _entropy(rows, n), _entropy(cols, n)
        nz = table > 0
        outer = rows[:, None] * cols[None, :]
        mi = float((table[nz] / n * (np.log(table[nz]) + np.log(n) - np.log(outer[nz]))).sum())
        rep['nmi'] = 1.0 if hu == 0 and hv == 0 else max(mi, 0.0) / (0.5 * (hu + hv))

        def pairs(x):
            return float((x * (x - 1.0) / 2.0).sum())
        together, pa, pb, total = pairs(table), pairs(rows), pairs(cols), n * (n - 1.0) / 2.0
        expected = pa * pb / total if total > 0 else 0.0
        most = 0.5 * (pa + pb)
        rep['ari'] = 1.0 if most == expected else (together - expected) / (most - expected)
        rep['purity'] = float(table.max(1).sum()) / n
        rep['accuracy'] = best_matching(table)[0] / n
    if vid is not None:
        v = np.asarray(torch.as_tensor(vid).cpu()).astype(np.int64).reshape(-1)
        if v.shape != a.shape:
            raise ValueError('vid must hold one entry per row')
        _, vi = np.unique(v, return_inverse=True)
        nv = int(vi.max()) + 1 if vi.size else 0
        per = np.bincount(vi[ok] * K + a[ok], minlength=nv * K).reshape(nv, K)
        clips = np.bincount(vi, minlength=nv).astype(np.float64)                 # unassigned clips count against the video
        rep['video_consistency'] = float((per.max(1) / clips).mean()) if nv else None
    return rep


def cluster_eval(per_feature, video_label, k=0, n_class=None, n_iter=100, n_init=10, seed=0):
    """per_feature [n_video, num_seq, D] (the per-clip features `classifier.py --retrieval` saves), video_label [n_video] ->
    (fit, metrics): kmeans_fit over the n_video * num_seq clips (row = video * num_seq + clip; k = 0: as many clusters as
    classes, n_class or the largest label + 1) and cluster_metrics of its assignment against the classes and the videos"""
    feat, vid, cls, _, _ = F.clip_rows(per_feature, video_label)
    n_class = int(n_class) if n_class else int(cls.max()) + 1
    k = int(k) if k else n_class
    fit = kmeans_fit(feat, k, n_iter=n_iter, n_init=n_init, seed=seed)
    return fit, cluster_metrics(fit['assign'], cls, vid=vid, n_class=n_class)
