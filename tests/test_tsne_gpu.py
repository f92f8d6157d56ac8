"""The t-SNE entries (include/dualvar_tsne.h), their host module (dualvar_amd/utils/embed.py) and `classifier.py --retrieval --tsne`
against the float64 reference of tests/tsne_reference.py, which is written from the header.

Conventions (those of tests/test_variance_gpu.py): outputs sit in buffers filled with a NaN bit pattern no kernel produces and
larger than needed; after every call everything beyond what the header says is written must still hold it.  Lists come with
ldk = k1 and ldk = k1 + 3.  u = 2^-24; E_EXPF, E_LOG, E_LOG1P are the device-function figures of tests/chains.py.

Bounds, each from the header's expressions (first order, times 1.01 for the higher orders):
  perplexity  e_j is formed by the reference in fp32 with the header's own operations: the same bits.  At the returned beta, in
              float64: x_j = beta e_j, w_j = exp(-x_j), S = sum w, p_j = w_j / S, B = beta sum(w e) / S, H = log S + B.
              rel(w_j) = E_EXPF + u x_j (the rounding of x_j);  rel(S) = rS = sum w_j rel(w_j) / S + 9u (a lane's chain of 3
              additions and the 6 levels of the wave fold);  |p - p64| <= p64 (rel(w_j) + rS + u) + 2^-126.
              |H_fp32 - H64| <= bH = E_LOG |log S| + rS + [beta sum w_j e_j (rel(w_j) + 10u) / S + B (rS + 2u)] + u |H|, and the
              kernel stopped at |H_fp32 - target| <= DV_TSNE_ENTROPY_TOL, so |H64 - target| <= DV_TSNE_ENTROPY_TOL + bH wherever
              the target can be met (ties at the minimum < perplexity < included slots).
  repulse     per pair: d2 carries 4u, t = 1 + d2 5u, q = v_rcp_f32(t) 5u + 1 ulp (2u) = 7u, q^2 15u, q^2 dx 17u; at most 128
              fp32 additions above a term (DV_TSNE_TILE / 2); the double sums add nothing visible; fr is rounded once.
              |Z - Z64| <= 136u sum q;   |fr - fr64| <= 147u sum |q^2 (y_i - y_j)|  (one u of slack each for the double sums).
  attract     c = p (0.5f / n) 2u, q (IEEE division) 6u, (c q) dx 11u, sums in double, one rounding to fp32:
              |fa - fa64| <= 13u sum |P q (y_i - y_j)|;  the ce term c log1pf(d2): 2u + 4u (d2 through log1p, whose relative
              condition is <= 1) + E_LOG1P + u, one rounding: |ce_row - ce64| <= (8u + E_LOG1P) ce64.
              *ce_sum against the float64 sum of the ce_row the kernel wrote: n 2^-53 of it.
  update      the kernel's steps are IEEE operations the reference repeats in fp32: the same bits in y, vel and gain.  Against the
              float64 formula: b(g) = 4u (|ex fa| + |fr / Z| + |ex fa - fr / Z|); b(vel) = u |m vel| + |lr gain g| (3u + b(g) / |g|)
              + u |vel'|; b(y) = b(vel) + u |y'| (the fr / Z rounding is the one step with no fp32 counterpart in the formula).
  iteration   b(g) = 4 (ex b(fa) + b(fr) / Z + |fr| b(Z) / Z^2) + the update's b(g); then as the update.  Elements whose |g| is
              below b(g) could take either gain and are left out (at most 1 %).
Each case prints (-s) err / bound.  Largest err / bound measured on an MI355X: perplexity p 0.789, entropy 0.855 (the stopping
tolerance is most of that bound; 162 to 554 rows per k1 meet their perplexity, none at k1 = 2 where no case's perplexity lies
below the number of slots); repulse fr 0.108, Z 0.029; attract fa 0.186,
ce_row 0.243, ce_sum 0.000; update gain 0.309, vel 0.319, y 0.526 (and the bits of the fp32 steps); one iteration fa 0.136,
fr 0.028, Z 0.000, ce 0.034, vel 0.117, y 0.115 with all 600 coordinates decided.  End to end: purity 1.0000 against the
reference's 1.0000, CE 10.167 -> 8.959 (reference 10.196 -> 8.980).  The whole file takes 14 s, 6.7 s of it the classifier.py
child, 1.6 s the n = 8 500 repulsion (its float64 reference on the host) and 1.0 s the end-to-end case; every other test is
below 0.7 s.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import ops  # noqa: E402
from tests import tsne_reference as R  # noqa: E402
from tests.chains import E_EXPF, E_LOG, E_LOG1P, TINY  # noqa: E402
from tests.checks import U, Ratios, is_sent, lib, report_fixture, sent  # noqa: E402
from tests.dataset_support import write_dataset  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
SLACK = 1.01
TILE = 256                           # DV_TSNE_ROWS = DV_TSNE_TILE
WORST = Ratios()
ratio = WORST.ratio
_report_worst = report_fixture(WORST, 28)


def sent64(count, dev):
    """float64 words that hold the int32 sentinel twice: their frames are checked through int32 views"""
    return sent((count, 2), dev, torch.int32).view(torch.float64).reshape(count)


# ------------------------------------------------------------------------------------------------------------ perplexity
ROW_KINDS = ('self0', 'self3_ties', 'absent', 'padded', 'nothing', 'all_equal', 'one_close', 'nearly_equal', 'only_self')


def make_row(kind, r, k1, rng):
    """one list row (val f32 [k1] descending as the merge leaves it, idx i32 [k1]); the row's own index is r"""
    val = np.sort(rng.uniform(-0.2, 0.95, k1).astype(np.float32))[::-1].copy()
    idx = (1000 + rng.permutation(50000)[:k1]).astype(np.int32)             # never r (r < 1000)
    if kind == 'self0':
        val[0], idx[0] = 1.0, r
    elif kind == 'self3_ties':           # exact ties at the top, the row itself behind them (duplicate clips)
        m = min(4, k1)
        val[:m], idx[m - 1] = 1.0, r
    elif kind == 'padded':               # fewer candidates than slots: (-inf, -1) at the end
        val[0], idx[0] = 1.0, r
        fill = max(1, k1 // 3)
        val[k1 - fill:], idx[k1 - fill:] = -np.inf, -1
    elif kind == 'nothing':
        val[:], idx[:] = -np.inf, -1
    elif kind == 'only_self':
        val[:], idx[:] = -np.inf, -1
        val[0], idx[0] = 1.0, r
    elif kind == 'all_equal':
        val[:] = 0.625
    elif kind == 'one_close':            # one neighbour far closer than the rest
        val[0] = 0.9999
        val[1:] = np.minimum(val[1:], 0.3)
    elif kind == 'nearly_equal':         # differences of 2^-20: a large beta
        val[:] = (0.75 - np.arange(k1) * 2.0 ** -20).astype(np.float32)
    return val, idx


@pytest.mark.parametrize('k1', [2, 7, 64, 91, 256])
def test_perplexity(gpu, k1):
    rng = np.random.RandomState(k1)
    met = 0
    for n in (1, 5, 130):
        for pad in (0, 3):
            for perp in (2.0, 30.0, 85.0):
                for off in (range(len(ROW_KINDS)) if n == 1 else (0,)):
                    ldk = k1 + pad
                    kinds = [ROW_KINDS[(r + off) % len(ROW_KINDS)] for r in range(n)]
                    rows = [make_row(kinds[r], r, k1, rng) for r in range(n)]
                    val = np.full((n, ldk), np.nan, dtype=np.float32)
                    idx = np.full((n, ldk), 7, dtype=np.int32)
                    val[:, :k1], idx[:, :k1] = np.stack([v for v, _ in rows]), np.stack([i for _, i in rows])
                    p, beta = sent((n + 2, ldk), gpu), sent((n + 3,), gpu)
                    ops.call('dv_tsne_perplexity_f32', torch.from_numpy(val).to(gpu), torch.from_numpy(idx).to(gpu), ldk, n, k1, 0, perp, p, beta)
                    assert is_sent(p[n:]) and is_sent(p[:n, k1:]) and is_sent(beta[n:]), 'wrote outside p / beta'
                    ph, bh = p[:n, :k1].cpu().numpy(), beta[:n].cpu().numpy()
                    assert np.isfinite(ph).all() and np.isfinite(bh).all(), 'NaN or inf in the output'
                    e, inc = R.list_distances(val[:, :k1], idx[:, :k1])
                    assert (ph[~inc] == 0).all(), 'an excluded slot is not exactly 0'
                    target = float(np.float32(math.log(float(np.float32(perp)))))
                    for r in range(n):
                        what = 'k1=%d n=%d ldk=%d perp=%g row %d %s' % (k1, n, ldk, perp, r, kinds[r])
                        m = int(inc[r].sum())
                        if m == 0:
                            assert (ph[r] == 0).all() and bh[r] == 0, what
                            continue
                        if not (e[r][inc[r]] > 0).any():
                            assert bh[r] == R.BETA_START and (ph[r][inc[r]] == np.float32(1.0) / np.float32(m)).all(), what
                            continue
                        b = float(bh[r])
                        assert b > 0, what
                        H, w, S = R.entropy(e[r], inc[r], b)
                        e64 = np.where(np.isfinite(e[r]), e[r].astype(np.float64), 0.0)
                        x = np.where(w > 0, b * e64, 0.0)
                        rel_w = E_EXPF + U * x
                        rS = float((w * rel_w).sum() / S) + 9 * U
                        p64 = w / S
                        ratio(np.abs(ph[r] - p64), SLACK * p64 * (rel_w + rS + U) + np.where(inc[r], TINY, 0.0), 'perplexity.p ' + what)
                        ties = int((e[r][inc[r]] == 0).sum())
                        if math.log(ties) + 1e-3 < target < math.log(m) - 1e-3:
                            B = b * float((w * e64).sum()) / S
                            bH = E_LOG * abs(math.log(S)) + rS + b * float((w * e64 * (rel_w + 10 * U)).sum()) / S + B * (rS + 2 * U) + U * abs(H)
                            ratio(abs(H - target), R.ENTROPY_TOL + SLACK * bH, 'perplexity.entropy ' + what)
                            met += 1
                        elif target > math.log(m) + 1e-3:
                            assert b == 2.0 ** -(R.MAX_STEPS - 1), what       # halved to the end: the uniform row
    assert met > 0 or k1 == 2
    print('    k1=%d: %d rows met their perplexity; largest err / bound %s' % (k1, met, ', '.join('%s %.3f' % kv for kv in sorted(WORST.items()) if kv[0].startswith('perp'))))


# ------------------------------------------------------------------------------------------------------------- repulsion
def repulse_ref(y):
    """y [n, 2] fp32 on the host -> (fr [n, 2], Z, sum|terms| [n, 2]) in float64, by row blocks of 512"""
    y = y.double()
    n = y.shape[0]
    fr, ab, Z = torch.zeros(n, 2, dtype=torch.float64), torch.zeros(n, 2, dtype=torch.float64), 0.0
    for r0 in range(0, n, 512):
        d = y[r0:r0 + 512, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(2))
        q[torch.arange(d.shape[0]), torch.arange(r0, r0 + d.shape[0])] = 0.0
        t = (q * q)[:, :, None] * d
        fr[r0:r0 + 512], ab[r0:r0 + 512] = t.sum(1), t.abs().sum(1)
        Z += float(q.sum())
    return fr, Z, ab


def run_repulse(y, gpu):
    n = y.shape[0]
    nbytes = lib().dv_tsne_repulse_workspace(n, None)
    assert nbytes > 0 and nbytes % 8 == 0
    ws, fr, Z = sent64(nbytes // 8 + 8, gpu), sent((n + 3, 2), gpu), sent64(3, gpu)
    ops.call('dv_tsne_repulse_f32', y, n, fr, Z.data_ptr() + 8, ws)
    assert is_sent(ws[nbytes // 8:].view(torch.int32)) and is_sent(fr[n:]) and is_sent(Z[0:1].view(torch.int32)) and is_sent(Z[2:].view(torch.int32))
    return fr[:n].clone(), Z[1:2].clone()


REPULSE_N = [1, 2, 255, 256, 257, 511, 512, 513, 2900]


@pytest.mark.parametrize('n', REPULSE_N)
def test_repulse(gpu, n):
    """one below / at / one above the 256 rows of a workgroup and the 256 columns of a tile (an odd and an even tail), two and
    three row blocks, S = 1 (n <= 256) and S > 1; scales 1e-4 (every q ~ 1), 1 and 50 (q tiny); exact duplicates"""
    import ctypes
    parts = ctypes.c_int32(0)
    lib().dv_tsne_repulse_workspace(n, ctypes.byref(parts))
    assert (parts.value > 1) == (n > 256)
    gen = torch.Generator().manual_seed(n)
    for scale in (1e-4, 1.0, 50.0):
        y = (scale * torch.randn((n, 2), generator=gen)).float()
        if n >= 8:
            y[1::7] = y[0]                                                   # duplicates of point 0, its own block and beyond
        fr64, Z64, ab = repulse_ref(y)
        yd = y.to(gpu)
        fr, Z = run_repulse(yd, gpu)
        what = 'n=%d scale=%g' % (n, scale)
        if n == 1:
            assert float(Z) == 0.0 and bool((fr == 0).all())
        ratio((fr.cpu().double() - fr64).abs().numpy(), (SLACK * 147 * U * ab).numpy(), 'repulse.fr ' + what)
        ratio(abs(float(Z) - Z64), SLACK * 136 * U * Z64, 'repulse.Z ' + what)
        fr2, Z2 = run_repulse(yd, gpu)
        assert torch.equal(fr.view(torch.int32), fr2.view(torch.int32)) and torch.equal(Z.view(torch.int64), Z2.view(torch.int64)), what
    print('    n=%d S=%d: largest err / bound fr %.3f Z %.3f' % (n, parts.value, WORST['repulse.fr'], WORST['repulse.Z']))


def test_repulse_several_tiles_per_part(gpu):
    """n = 8500: 34 row blocks and tiles in S = 31 parts, so three parts walk two tiles and add them in double"""
    import ctypes
    n = 8500
    parts = ctypes.c_int32(0)
    lib().dv_tsne_repulse_workspace(n, ctypes.byref(parts))
    assert parts.value == 31 < -(-n // TILE)
    y = (3.0 * torch.randn((n, 2), generator=torch.Generator().manual_seed(8500))).float()
    fr64, Z64, ab = repulse_ref(y)
    fr, Z = run_repulse(y.to(gpu), gpu)
    ratio((fr.cpu().double() - fr64).abs().numpy(), (SLACK * 147 * U * ab).numpy(), 'repulse.fr n=8500')
    ratio(abs(float(Z) - Z64), SLACK * 136 * U * Z64, 'repulse.Z n=8500')


# ------------------------------------------------------------------------------------------------------------ attraction
def attract_case(n, k1, pad, scale, seed, gpu):
    """random forward lists with -1 entries; for n >= 7 row 0 is a hub (every other row lists it in slot 0) and row 5 is listed
    by nobody -> everything dv_tsne_attract_f32 takes, on the device, and the host copies"""
    from dualvar_amd.utils.embed import reverse_csr
    rng = np.random.RandomState(seed)
    ldk = k1 + pad
    idx = rng.randint(0, n, (n, ldk)).astype(np.int32)
    if n >= 7:
        idx[idx == 5] = 6
        idx[1:, 0] = 0
    idx[rng.uniform(size=idx.shape) < 0.2] = -1
    if n >= 7:
        idx[1:, 0] = 0
    inc = (idx >= 0) & (idx != np.arange(n)[:, None])
    inc[:, k1:] = False
    p = np.where(inc, rng.uniform(0.01, 1.0, idx.shape), 0.0)
    p = (p / np.maximum(p.sum(1, keepdims=True), 1e-30)).astype(np.float32)
    p[:, k1:] = np.nan                                                       # the pitch padding is never read
    y = (scale * rng.randn(n, 2)).astype(np.float32)
    ptr, edge = reverse_csr(torch.from_numpy(idx), torch.from_numpy(inc))
    if n >= 7:
        assert int(ptr[1] - ptr[0]) >= n - 1 and int(ptr[6] - ptr[5]) == 0     # every other row lists the hub, some twice
    dev = [torch.from_numpy(a).to(gpu) for a in (y, idx, p)] + [ptr.to(gpu), edge.to(gpu)]
    return y, idx[:, :k1], np.where(inc, p, 0.0)[:, :k1], dev, ldk


def run_attract(dev, ldk, n, k1, gpu, with_sum=True):
    yd, idxd, pd, ptr, edge = dev
    fa, ce, cs = sent((n + 2, 2), gpu), sent((n + 5,), gpu), sent64(3, gpu)
    edge_arg = edge if edge.numel() else torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.call('dv_tsne_attract_f32', yd, idxd, pd, ldk, n, k1, ptr, edge_arg, edge.numel(), fa, ce, cs.data_ptr() + 8 if with_sum else None)
    assert is_sent(fa[n:]) and is_sent(ce[n:]) and is_sent(cs[0:1].view(torch.int32)) and is_sent(cs[2:].view(torch.int32))
    assert with_sum or is_sent(cs.view(torch.int32))
    return fa[:n].clone(), ce[:n].clone(), cs[1:2].clone()


@pytest.mark.parametrize('n,k1', [(1, 3), (7, 4), (7, 70), (300, 16), (300, 130)])
def test_attract(gpu, n, k1):
    for pad in (0, 3):
        for scale in (1e-4, 1.0, 50.0):
            y, idx, p, dev, ldk = attract_case(n, k1, pad, scale, 100 * n + k1 + pad, gpu)
            P = R.sparse_P(idx, p, n)
            fa64, ce64, ab = R.attraction(P, y)
            fa, ce, cs = run_attract(dev, ldk, n, k1, gpu)
            what = 'n=%d k1=%d ldk=%d scale=%g' % (n, k1, ldk, scale)
            ratio(np.abs(fa.cpu().double().numpy() - fa64), SLACK * 13 * U * ab, 'attract.fa ' + what)
            ratio(np.abs(ce.cpu().double().numpy() - ce64), SLACK * (8 * U + E_LOG1P) * ce64 + TINY, 'attract.ce_row ' + what)
            total = float(ce.cpu().double().sum())
            ratio(abs(float(cs) - total), n * U64 * total, 'attract.ce_sum ' + what)
            if n == 1:
                assert bool((fa == 0).all()) and float(ce) == 0 and float(cs) == 0
            fa2, ce2, cs2 = run_attract(dev, ldk, n, k1, gpu)
            assert torch.equal(fa.view(torch.int32), fa2.view(torch.int32)) and torch.equal(ce.view(torch.int32), ce2.view(torch.int32))
            assert torch.equal(cs.view(torch.int64), cs2.view(torch.int64))
            fa3, ce3, _ = run_attract(dev, ldk, n, k1, gpu, with_sum=False)   # a null ce_sum: the rows all the same, no total
            assert torch.equal(fa.view(torch.int32), fa3.view(torch.int32)) and torch.equal(ce.view(torch.int32), ce3.view(torch.int32))
    print('    n=%d k1=%d: largest err / bound %s' % (n, k1, ', '.join('%s %.3f' % kv for kv in sorted(WORST.items()) if kv[0].startswith('attract'))))


# ---------------------------------------------------------------------------------------------------------------- update
def update_ref32(y, vel, gain, fa, fr, Z, ex, mom, lr, min_gain):
    """the header's steps in fp32, one IEEE operation each"""
    F = np.float32
    r = (fr.astype(np.float64) / Z).astype(F)
    g = F(4.0) * (F(ex) * fa - r)
    gain = np.where((g > 0) != (vel > 0), gain + F(0.2), gain * F(0.8)).astype(F)
    gain = np.maximum(gain, F(min_gain))
    vel = F(mom) * vel - (F(lr) * gain) * g
    return (y + vel).astype(F), vel.astype(F), gain, g


def test_update(gpu):
    """g and vel each positive, negative and zero (g = 0 from fa = fr = 0), gains that grow, shrink and meet the clamp"""
    sg = np.array([1, -1, 0], dtype=np.float32)
    combos = np.array([(a, b, c) for a in sg for b in sg for c in (1.0, 0.012, 0.01, 3.7)], dtype=np.float32)     # 36 elements
    rng = np.random.RandomState(1)
    m = combos.shape[0]
    fa = (combos[:, 0] * rng.uniform(0.5, 2.0, m) * 1e-3).astype(np.float32)
    fr = (-combos[:, 0] * rng.uniform(0.5, 2.0, m) * 40.0).astype(np.float32)
    vel = (combos[:, 1] * rng.uniform(0.5, 2.0, m)).astype(np.float32)
    gain, y = combos[:, 2].copy(), rng.randn(m).astype(np.float32)
    Z, ex, mom, lr, mg = 12345.678, 12.0, 0.5, 50.0, 0.01
    yr, vr, gr, g32 = update_ref32(y, vel, gain, fa, fr, Z, ex, mom, lr, mg)
    assert sorted(set(np.sign(g32).tolist())) == [-1.0, 0.0, 1.0] and (gr == np.float32(mg)).sum() >= 4 and (gr > 3.7).any()
    bufs = [sent((m + 5,), gpu) for _ in range(3)]
    for b, v in zip(bufs, (y, vel, gain)):
        b[:m] = torch.from_numpy(v).to(gpu)
    Zd = sent64(3, gpu)
    Zd[1] = Z
    ops.call('dv_tsne_update_f32', bufs[0], bufs[1], bufs[2], torch.from_numpy(fa).to(gpu), torch.from_numpy(fr).to(gpu), Zd.data_ptr() + 8, m,
             ex, mom, lr, mg)
    assert all(is_sent(b[m:]) for b in bufs) and float(Zd[1]) == Z
    got = [b[:m].cpu().numpy() for b in bufs]
    for name, a, b in zip(('y', 'vel', 'gain'), got, (yr, vr, gr)):
        assert (a.view(np.int32) == b.view(np.int32)).all(), '%s differs in bits from the fp32 steps of the header' % name
    # against the float64 formula (decisions as in float64: |g| is far from 0 or exactly 0 on this data)
    fa64, fr64, v64, gn64, y64 = (a.astype(np.float64) for a in (fa, fr, vel, gain, y))
    a, r = ex * fa64, fr64 / Z
    g = 4.0 * (a - r)
    bg = SLACK * 4 * U * (np.abs(a) + np.abs(r) + np.abs(a - r))
    assert ((np.abs(g) > 100 * bg) | (g == 0)).all()
    y2, v2, gn2 = R.update(y64, v64, gn64, g, mom, lr, mg)
    ratio(np.abs(got[2] - gn2), SLACK * 2 * U * gn2, 'update.gain')         # the constant's rounding and the operation's
    step = np.abs(lr * gn2 * g)
    bv = SLACK * (U * np.abs(mom * v64) + step * (3 * U + 2 * U) + lr * gn2 * bg + U * np.abs(v2))
    ratio(np.abs(got[1] - v2), bv, 'update.vel')
    ratio(np.abs(got[0] - y2), bv + SLACK * U * np.abs(y2), 'update.y')


# ----------------------------------------------------------------------------------------------------- one whole iteration
CACHE = {}


def cluster_data():
    """six unit-norm cluster centres in D = 32, 50 points each, Gaussian noise 0.05, renormalised: n = 300"""
    if 'x' not in CACHE:
        gen = torch.Generator().manual_seed(16)
        c = torch.randn((6, 32), generator=gen, dtype=torch.float64)
        c = c / c.norm(dim=1, keepdim=True)
        x = c.repeat_interleave(50, 0) + 0.05 * torch.randn((300, 32), generator=gen, dtype=torch.float64)
        x = x / x.norm(dim=1, keepdim=True)
        CACHE['x'], CACHE['cls'] = x.float(), torch.arange(6).repeat_interleave(50)
        s = (x @ x.t()).numpy()
        same = (CACHE['cls'][:, None] == CACHE['cls'][None, :]).numpy()
        CACHE['cos'] = (float(s[same].min()), float(s[~same].max()))
    return CACHE['x'], CACHE['cls']


def test_one_iteration_through_all_four_entries(gpu):
    from dualvar_amd.utils import embed as E
    x, cls = cluster_data()
    n = x.shape[0]
    aff = E.tsne_affinities(x.to(gpu), 10)
    assert aff['k'] == 30 and aff['k1'] == 31 and aff['idx'].shape == (n, 31)
    idx, p = aff['idx'].cpu().numpy(), aff['p'].cpu().numpy()
    assert np.abs(p.sum(1) - 1).max() < 1e-5 and (p[idx == np.arange(n)[:, None]] == 0).all()
    P = R.sparse_P(idx, p, n)
    y0 = torch.randn((n, 2), generator=torch.Generator().manual_seed(9)).float()
    w = E._Workspace(n, gpu, 1)
    y = y0.to(gpu).clone()
    ex, mom, lr = 12.0, 0.5, 50.0
    zp = E.forces(y, aff, w, 0)
    ops.call('dv_tsne_update_f32', y, w.vel, w.gain, w.fa, w.fr, zp, 2 * n, ex, mom, lr, E.MIN_GAIN)
    Z, ce = w.trace[0].tolist()
    y64 = y0.double().numpy()
    fa64, ce64, ab_a = R.attraction(P, y64)
    fr64, Z64, ab_r = R.repulsion(y64)
    b_fa, b_fr, b_Z = SLACK * 13 * U * ab_a, SLACK * 147 * U * ab_r, SLACK * 136 * U * Z64
    ratio(np.abs(w.fa.cpu().double().numpy() - fa64), b_fa, 'iteration.fa')
    ratio(np.abs(w.fr.cpu().double().numpy() - fr64), b_fr, 'iteration.fr')
    ratio(abs(Z - Z64), b_Z, 'iteration.Z')
    ratio(abs(ce - ce64.sum()), SLACK * (9 * U + E_LOG1P) * ce64.sum(), 'iteration.ce')
    a, r = ex * fa64, fr64 / Z64
    g = 4.0 * (a - r)
    bg = 4 * (ex * b_fa + b_fr / Z64 + np.abs(fr64) * b_Z / Z64 ** 2) + SLACK * 4 * U * (np.abs(a) + np.abs(r) + np.abs(a - r))
    sure = np.abs(g) > bg
    assert sure.mean() >= 0.99
    y2, v2, gn2 = R.update(y64, np.zeros_like(y64), np.ones_like(y64), g, mom, lr, E.MIN_GAIN)
    assert set(np.round(gn2[sure], 6).tolist()) <= {1.2, 0.8}
    bv = SLACK * (np.abs(lr * gn2 * g) * 5 * U + lr * gn2 * bg + U * np.abs(v2))
    ratio(np.abs(w.vel.cpu().double().numpy() - v2)[sure], bv[sure], 'iteration.vel')
    ratio(np.abs(y.cpu().double().numpy() - y2)[sure], (bv + SLACK * U * np.abs(y2))[sure], 'iteration.y')
    print('    one iteration: %d of %d coordinates decided; largest err / bound %s'
          % (int(sure.sum()), sure.size, ', '.join('%s %.3f' % kv for kv in sorted(WORST.items()) if kv[0].startswith('iteration'))))


# ------------------------------------------------------------------------------------------------------------ end to end
def reference_embedding(x, cls, perplexity, n_iter, seed):
    """tsne_reference's own pipeline on the same data, all float64: centre, normalise, the k + 1 nearest by dot product,
    bisection, sparse P, the loop from tsne_embed's initial map"""
    z = x.double().numpy()
    z = z - z.mean(0)
    z = z / np.linalg.norm(z, axis=1, keepdims=True)
    s = z @ z.T
    k = min(3 * perplexity, z.shape[0] - 1)
    idx = np.argsort(-s, axis=1, kind='stable')[:, :k + 1]
    val = np.take_along_axis(s, idx, 1).astype(np.float32)
    p, _ = R.perplexity_ref(val, idx, perplexity)
    y0 = (1e-4 * torch.randn((z.shape[0], 2), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)).double().numpy()
    return R.embed(R.sparse_P(idx, p, z.shape[0]), y0, n_iter)


def test_end_to_end_clusters(gpu):
    """six clusters, perplexity 10, 500 iterations.  The reference's own loop (tests/tsne_reference.py, float64, same data, seed
    and schedule) gives a 10-NN class purity of 1.0000 on this input; tsne_embed measured 1.0000 on an MI355X.  The smallest
    same-cluster cosine of the data is 0.856, the largest cross-cluster cosine 0.405."""
    from dualvar_amd.utils import embed as E
    x, cls = cluster_data()
    lo_same, hi_cross = CACHE['cos']
    assert lo_same >= 0.85 and hi_cross <= 0.55, (lo_same, hi_cross)            # the input is what the test says it is
    yr, tr = reference_embedding(x, cls, 10, 500, 0)
    ref_purity = R.knn_purity(yr, cls.numpy(), 10)
    assert ref_purity >= 0.99, 'the reference does not separate this input: %.4f' % ref_purity
    xd = x.to(gpu)
    y, trace = E.tsne_embed(xd, perplexity=10, n_iter=500, seed=0)
    yh = y.cpu()
    assert yh.shape == (300, 2) and bool(torch.isfinite(yh).all())
    purity = R.knn_purity(yh.numpy(), cls.numpy(), 10)
    print('    end to end: purity %.4f (reference %.4f), CE %.4f -> %.4f (reference %.4f -> %.4f), same-cluster cos >= %.3f, cross <= %.3f'
          % (purity, ref_purity, trace['ce'][5], trace['ce'][-1], tr['ce'][5], tr['ce'][-1], lo_same, hi_cross))
    assert purity >= ref_purity - 0.02
    assert trace['iter'] == list(range(0, 500, 50)) + [500] == tr['iter'] and len(trace['ce']) == len(trace['z']) == 11
    after = trace['iter'].index(250)                                         # the first traced iteration after exaggeration ends
    assert trace['ce'][-1] < trace['ce'][after] and all(math.isfinite(c) for c in trace['ce'])
    # iteration 0 is the same map in both: the cross-entropies agree before the dynamics part them
    assert abs(trace['ce'][0] - tr['ce'][0]) < 1e-3 * abs(tr['ce'][0])
    y2, trace2 = E.tsne_embed(xd, perplexity=10, n_iter=500, seed=0)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and trace == trace2, 'two calls with one seed differ'
    y3, _ = E.tsne_embed(xd, perplexity=10, n_iter=500, seed=1)
    assert not torch.equal(y, y3)
    rep = E.embedding_report(y, torch.arange(300) // 10, cls, E.tsne_affinities(xd, 10)['idx'], k=10)
    assert abs(rep['purity_class'] - purity) < 0.01 and 0 <= rep['purity_video'] <= rep['purity_class'] and 0 < rep['knn_preservation'] <= 1
    print('    report: %s' % rep)


# ------------------------------------------------------------------------------------------------------- the driver, one child
def test_cli_retrieval_with_tsne(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp('tsne_cli')
    split, frame = write_dataset(str(d / 'data'), videos=((0, 40), (0, 9), (1, 70)), rows=830, sizes=[(90, 120), (120, 90), (80, 100)])
    os.makedirs(str(d / 'run' / 'model'))
    argv = [os.path.join(ROOT, 'classifier.py'), '--test', str(d / 'run' / 'model' / 'none.pth.tar'), '--retrieval', '--num_seq', '10',
            '--net', 'r3d', '--seq_len', '8', '--img_dim', '64', '--img_resize_dim', '72', '--ds', '2', '--batch_size', '4', '-j', '2',
            '--split_root', split, '--frame_root', frame, '--tsne', '--tsne_perplexity', '5', '--tsne_iter', '60', '--tsne_split', 'both']
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=600, cwd=str(d))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    fdir = str(d / 'run' / 'model' / 'feature')
    assert out.count('t-SNE map of ucf101') == 2 and 'kNN preservation = ' in out, out[-2000:]
    try:
        import matplotlib  # noqa: F401
        have_plot = True
    except ImportError:
        have_plot = False
    for split_name, n_video in (('test', 3), ('train', 30)):
        stem = os.path.join(fdir, 'ucf101_%s_tsne' % split_name)
        y = torch.load(stem + '.pth.tar', map_location='cpu', weights_only=True)
        assert y.shape == (10 * n_video, 2) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
        with open(stem + '.json') as fp:
            rep = json.load(fp)
        assert (rep['perplexity'], rep['n_iter'], rep['seed'], rep['n']) == (5, 60, 0, 10 * n_video) and rep['neighbours'] == 15
        assert rep['trace']['iter'] == [0, 50, 60] and len(rep['trace']['ce']) == len(rep['trace']['z']) == 3
        assert rep['z'] == rep['trace']['z'][-1] > 0 and all(math.isfinite(c) for c in rep['trace']['ce'])
        for key in ('purity_video', 'purity_class', 'knn_preservation'):
            assert 0.0 <= rep['report'][key] <= 1.0, (key, rep['report'])
        assert os.path.exists(stem + '.png') == have_plot
