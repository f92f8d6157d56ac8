"""Float64 / integer model of include/dualvar_rankeval.h (not the product; no GPU, no dependency on the library).

Per query row: the valid items are put in the header's total order by a brute-force sort (key descending, bank index ascending;
key = the similarity with NaN -> -inf and -0.0 -> +0.0), the 1-based positions of the positives are the ranks, and from the ranks
    AP = (sum over ascending i of float(i + 1) / float(rank_i)) / float(P)      in IEEE double, in that order
    hits(k) = #{i : rank_i <= k},  rhits = hits(P),  first = rank_0,  n_valid = the number of valid items;
P = 0 gives AP = -1.0, first = 0, hits = 0.  `streaming_hist` is the other route to the same ranks, the one the kernels take:
the sorted positives, a binary search of every valid item and a histogram of the results, chunk by chunk."""
import bisect

import numpy as np


def keys(sim):
    """similarities (any float array) -> float64 keys: NaN -> -inf, -0.0 -> +0.0; +-inf stay"""
    k = np.asarray(sim, dtype=np.float64).copy()
    k[np.isnan(k)] = -np.inf
    return k + 0.0


def valid_mask(R, n, exclude, diag=0, row_vid=None, col_vid=None):
    """[R, n] bool: exclude 0 nothing, 1 the self pair j == r + diag, 2 every pair of equal video ids"""
    ok = np.ones((R, n), dtype=bool)
    if exclude == 1:
        r = np.arange(R)
        j = r + diag
        hit = (j >= 0) & (j < n)
        ok[r[hit], j[hit]] = False
    elif exclude == 2:
        ok &= np.asarray(row_vid)[:, None] != np.asarray(col_vid)[None, :]
    else:
        assert exclude == 0
    return ok


def figures(ranks, ks):
    """ascending ranks of one query's positives -> (ap, first, [hits(k)], rhits)"""
    P = len(ranks)
    if P == 0:
        return -1.0, 0, [0] * len(ks), 0
    a = 0.0
    for i, rho in enumerate(ranks):
        a += float(i + 1) / float(rho)
    a /= float(P)
    return a, int(ranks[0]), [sum(1 for rho in ranks if rho <= k) for k in ks], sum(1 for rho in ranks if rho <= P)


def row_model(key, idx, valid, positive, ks=()):
    """one query: key float64 [n] (already `keys`), idx int [n] bank indices, valid / positive bool [n] -> dict"""
    sel = np.nonzero(valid)[0]
    order = sel[np.lexsort((idx[sel], -key[sel]))]              # primary: key descending; among equals: index ascending
    is_pos = positive[order]
    ranks = (np.nonzero(is_pos)[0] + 1).tolist()
    ap, first, hits, rhits = figures(ranks, ks)
    return {'rank': ranks, 'pos_idx': idx[order[is_pos]].tolist(), 'pos_val': key[order[is_pos]].tolist(), 'ap': ap, 'first_rank': first,
            'hits': hits, 'rhits': rhits, 'n_valid': int(len(sel)), 'pos_cnt': len(ranks)}


def model(sim, row_cls, col_cls, exclude=0, diag=0, row_vid=None, col_vid=None, col0=0, ks=()):
    """sim [R, n] -> dict of arrays padded to P_max = the longest list (at least 1): rank [R, P_max] int64 (0 beyond P), pos_idx
    (-1 beyond P), pos_val float64 (NaN beyond P), pos_cnt, ap float64, first_rank, hits [R, len(ks)], rhits, n_valid"""
    sim = np.asarray(sim)
    R, n = sim.shape
    key = keys(sim)
    ok = valid_mask(R, n, exclude, diag, row_vid, col_vid)
    pos = ok & (np.asarray(row_cls)[:, None] == np.asarray(col_cls)[None, :])
    idx = np.arange(n, dtype=np.int64) + col0
    rows = [row_model(key[r], idx, ok[r], pos[r], ks) for r in range(R)]
    pm = max([1] + [row['pos_cnt'] for row in rows])
    out = {'rank': np.zeros((R, pm), dtype=np.int64), 'pos_idx': np.full((R, pm), -1, dtype=np.int64),
           'pos_val': np.full((R, pm), np.nan), 'hits': np.zeros((R, len(ks)), dtype=np.int64)}
    for r, row in enumerate(rows):
        P = row['pos_cnt']
        out['rank'][r, :P], out['pos_idx'][r, :P], out['pos_val'][r, :P] = row['rank'], row['pos_idx'], row['pos_val']
        out['hits'][r] = row['hits']
    for name in ('pos_cnt', 'first_rank', 'rhits', 'n_valid'):
        out[name] = np.array([row[name] for row in rows], dtype=np.int64)
    out['ap'] = np.array([row['ap'] for row in rows], dtype=np.float64)
    return out


def streaming_hist(key, idx, valid, positive, chunks):
    """the kernels' route for one query: the sorted (key, index) list of the positives; per chunk (start, length) of the columns,
    every valid item j is searched in it with the predicate "p precedes j or p is j" and counted -> (hist [P + 1], the list)"""
    sel = np.nonzero(valid & positive)[0]
    order = sel[np.lexsort((idx[sel], -key[sel]))]
    code = [(-key[j], int(idx[j])) for j in order]             # ascending tuples = the header's order (-(-inf) = +inf sorts last)
    hist = [0] * (len(code) + 1)
    for c0, m in chunks:
        for j in range(c0, c0 + m):
            if valid[j]:
                hist[bisect.bisect_right(code, (-key[j], int(idx[j])))] += 1
    return hist, order


def ranks_from_hist(hist):
    """rank(p_i) = 1 + sum_{b <= i} hist[b]; the last prefix sum is the number of valid items"""
    cum = np.cumsum(np.asarray(hist, dtype=np.int64))
    return (1 + cum[:-1]).tolist(), int(cum[-1])
