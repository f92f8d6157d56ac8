"""One BatchNorm layer as the BatchNorm suites see it (tests/test_batchnorm_multi_gpu.py, test_batchnorm_single_gpu.py,
test_gate_fold_gpu.py): its data in sentinel-framed views, its parameters, the dv_bn_item table of a group, and the checks of
every stage against float64.  The data kinds (A) exact and (B) Gaussian and the derivation of the bounds are described in
tests/test_batchnorm_multi_gpu.py."""
import math

import pytest
import torch

from dualvar_amd import _lib as L, ops
from dualvar_amd._lib import DV_ACCUM, DV_BF16, DV_F32, DV_MASK_FROM_X, DV_NO_RELU_MASK, DV_RELU
from tests.chains import bwd_reduce_chain, m2_bound, stats_chain
from tests.checks import BF16_U, U, View, ceil_div, chan, cp8, sent, vec, within

DTYPES = [pytest.param(DV_F32, id='fp32'), pytest.param(DV_BF16, id='bf16')]
PHASES = ('stats', 'apply', 'red', 'bapply')
JUNK = 3.0                                                                       # pad lanes [C, CP) of every input
EPS, MOM = 1e-5, 0.1


def check_bound(got, ref, bound, what):
    within(got, ref, bound, what, quiet=True)


def report(what, err, scale):
    """err / (u * sum|terms|), the largest over the channels"""
    r = float((err / (U * scale.clamp_min(1e-300))).max())
    print(f'    {what:<34s} max err / (u sum|terms|) = {r:8.3f}')
    return r


def n_blocks(lib, phase, M, C_, dtype):
    """engine.BNMember.blocks' block counts"""
    if phase == 'stats':
        return C_
    if phase == 'red':
        return int(lib.dv_bn_bwd_blocks(M, C_))
    total = M * (cp8(C_) // vec(dtype))
    return max(1, min(4096 if phase == 'apply' else 2048, ceil_div(total, 256)))


# ----------------------------------------------------------------------------------------------------------- members
class Member:
    """one BatchNorm layer of a group: its data, parameters, outputs and float64 reference"""

    def __init__(self, dev, dtype, M, C_, seed, *, exact, relu=True, res=False, accum=False, from_x=False, views=False,
                 zero=(), dscale=1.0, R=1, tile_rows=256, part_pitch_extra=0):
        assert not (from_x and (res or not relu))
        self.dtype, self.M, self.C, self.CP, self.exact = dtype, M, C_, cp8(C_), exact
        self.relu, self.res_on, self.accum, self.from_x, self.zero, self.R = relu, res, accum, from_x, set(zero), R
        self.dscale = float(torch.tensor(dscale, dtype=torch.float32))             # as the item carries it
        self.exact_dparams = exact and math.frexp(self.dscale)[0] == 0.5         # 1, 1/2: dgamma / dbeta exact
        self.loff, self.local_ptr = 0, 0
        tdt = ops.TORCH_DTYPE[dtype]
        g = torch.Generator(device=dev).manual_seed(seed)
        CP = self.CP
        vw = iter([(8 * (1 + k % 3), 8 * (1 + (k * 5) % 4)) for k in range(8)]) if views else iter([(0, 0)] * 8)

        def layout():
            off, extra = next(vw)
            return off, off + CP + extra
        if exact:
            x = torch.randint(-2, 3, (M, C_), generator=g, device=dev).double()
            r = torch.randint(-2, 3, (M, C_), generator=g, device=dev).double()
            p = min(0.5, 2.0 ** 18 / M)                                          # density of the nonzero g
            dyv = torch.randint(0, 2, (M, C_), generator=g, device=dev).double() * 2 - 1
            dyv = dyv * (torch.rand((M, C_), generator=g, device=dev) < p).double()
            pick = lambda vals: torch.tensor(vals, device=dev, dtype=torch.float64)[   # noqa: E731
                torch.randint(0, len(vals), (C_,), generator=g, device=dev)]
            mean = torch.randint(-4, 5, (C_,), generator=g, device=dev).double() / 4
            invstd = pick([0.5, 1.0, 1.5, 2.0])
            gamma = pick([-0.5, 0.5, 1.0, 1.5])
            beta = torch.randint(-4, 5, (C_,), generator=g, device=dev).double() / 4
            dg0 = torch.randint(-64, 65, (C_,), generator=g, device=dev).double() / 16
            db0 = torch.randint(-64, 65, (C_,), generator=g, device=dev).double() / 16
            dres0 = torch.randint(-2, 3, (M, C_), generator=g, device=dev).double()
        else:
            mu = 0.5 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64)
            sd = 0.5 + torch.rand(C_, generator=g, device=dev, dtype=torch.float64) * 1.5
            x = torch.randn((M, C_), generator=g, device=dev, dtype=torch.float64) * sd + mu
            r = torch.randn((M, C_), generator=g, device=dev, dtype=torch.float64)
            dyv = torch.randn((M, C_), generator=g, device=dev, dtype=torch.float64)
            x, r, dyv = (t.to(tdt).double() for t in (x, r, dyv))                # the values the kernels see
            mean = x.mean(0).float().double()
            invstd = (x.var(0, unbiased=False) + EPS).rsqrt().float().double()
            gamma = (1 + 0.2 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64)).float().double()
            beta = (0.1 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64)).float().double()
            dg0 = torch.randn(C_, generator=g, device=dev, dtype=torch.float64).float().double()
            db0 = torch.randn(C_, generator=g, device=dev, dtype=torch.float64).float().double()
            dres0 = torch.randn((M, C_), generator=g, device=dev, dtype=torch.float64).to(tdt).double()
        scale = (gamma * invstd).float().double()
        shift = (beta - mean * scale).float().double()
        if exact:
            assert torch.equal(scale, gamma * invstd) and torch.equal(shift, beta - mean * scale)
        self.mean, self.invstd, self.gamma, self.beta, self.scale, self.shift = mean, invstd, gamma, beta, scale, shift
        self.dg0, self.db0 = dg0, db0
        # inputs
        self.x = View(dtype, M, C_, *layout(), dev, x, pad=JUNK)
        self.res = View(dtype, M, C_, *layout(), dev, r, pad=JUNK) if res else None
        self.dy = View(dtype, M, C_, *layout(), dev, dyv, pad=JUNK)
        # outputs
        self.y = View(dtype, M, C_, *layout(), dev)
        self.dx = View(dtype, M, C_, *layout(), dev)
        self.dres = View(dtype, M, C_, *layout(), dev, dres0 if accum else None, pad=JUNK) if res else None
        self.dres0 = dres0 if (res and accum) else None
        # per-channel parameters (read) and outputs (written)
        self.p = {k: chan(v.float(), CP, dev) for k, v in
                  (('mean', mean), ('invstd', invstd), ('gamma', gamma), ('beta', beta), ('scale', scale), ('shift', shift))}
        self.o = {k: sent((CP,), dev) for k in ('mean', 'invstd', 'scale', 'shift')}
        self.rm0 = (torch.randint(-8, 9, (C_,), generator=g, device=dev).float() / 8)
        self.rv0 = 0.5 + torch.randint(0, 9, (C_,), generator=g, device=dev).float() / 8
        self.rm, self.rv = chan(self.rm0, CP, dev), chan(self.rv0, CP, dev)
        self.dgamma, self.dbeta = chan(dg0.float(), CP, dev), chan(db0.float(), CP, dev)
        self.sums = [sent((2 * CP,), dev) for _ in range(2)]
        wsn = int(L.load().dv_bn_bwd_reduce_workspace(M, C_))
        assert wsn % 4 == 0
        self.red_ws = L.register_ticket_workspace(torch.zeros(wsn // 4, dtype=torch.float32, device=dev))
        # conv-epilogue-format partials [2][pitch][tiles] of x, this member's channels at column `coff` of a wider table
        self.tile_rows = tile_rows
        self.n_tiles = ceil_div(M, tile_rows)
        self.coff = 8 if part_pitch_extra else 0
        self.pitch = C_ + self.coff + part_pitch_extra
        self.part = torch.full((2, self.pitch, self.n_tiles), float('nan'), dtype=torch.float32, device=dev)
        ps, pq, n = tile_partials(x, tile_rows)
        self.part[0, self.coff:self.coff + C_] = ps.float().t()
        self.part[1, self.coff:self.coff + C_] = pq.float().t()
        self.tile_n = n

    def partials_ptr(self):
        return self.part.data_ptr() + 4 * self.coff * self.n_tiles

    # reference values of the stored partials: [tiles][C]
    def ps(self):
        return self.part[0, self.coff:self.coff + self.C].double().t()

    def pq(self):
        return self.part[1, self.coff:self.coff + self.C].double().t()

    @property
    def fwd_flags(self):
        return DV_RELU if self.relu else 0

    @property
    def bwd_flags(self):
        f = 0 if self.relu else DV_NO_RELU_MASK
        if self.from_x:
            f |= DV_MASK_FROM_X
        if self.res_on and self.accum:
            f |= DV_ACCUM
        return f


def tile_partials(x, tile_rows):
    """(sum, M2 about the tile mean) per tile of tile_rows rows, float64: [tiles][C] x 2, and the rows of each tile"""
    M, C_ = x.shape
    nt = ceil_div(M, tile_rows)
    xp = torch.zeros(nt * tile_rows, C_, dtype=torch.float64, device=x.device)
    xp[:M] = x
    xp = xp.view(nt, tile_rows, C_)
    n = torch.full((nt,), float(tile_rows), dtype=torch.float64, device=x.device)
    n[-1] = M - (nt - 1) * tile_rows
    valid = (torch.arange(tile_rows, device=x.device)[None, :] < n[:, None]).double()[:, :, None]
    s = xp.sum(1)
    m2 = (((xp - (s / n[:, None])[:, None, :]) * valid) ** 2).sum(1)
    return s, m2, n


def make_table(members, lib, dev, dtype, stats_outputs=False, sums_idx=0, rank_local=None):
    """the device dv_bn_item array with the block prefixes of engine.BNGroupOp._table (a member may have 0 blocks in a phase)"""
    arr = (L.BnItem * len(members))()
    ends = dict.fromkeys(PHASES, 0)
    for i, m in enumerate(members):
        it = arr[i]
        it.partials, it.n_tiles, it.tile_rows, it.pitch = m.partials_ptr(), m.n_tiles, m.tile_rows, m.pitch
        it.local_stats = rank_local[i] if rank_local is not None else m.local_ptr
        it.gamma, it.beta = m.p['gamma'].data_ptr(), m.p['beta'].data_ptr()
        it.running_mean, it.running_var = m.rm.data_ptr(), m.rv.data_ptr()
        src = m.o if stats_outputs else m.p
        it.mean, it.invstd, it.scale, it.shift = (src[k].data_ptr() for k in ('mean', 'invstd', 'scale', 'shift'))
        it.x, it.ldx, it.y, it.ldy = m.x.ptr, m.x.ld, m.y.ptr, m.y.ld
        it.residual, it.ldr = (m.res.ptr, m.res.ld) if m.res else (0, 0)
        it.dy, it.lddy, it.dx, it.lddx = m.dy.ptr, m.dy.ld, m.dx.ptr, m.dx.ld
        it.dres, it.lddres = (m.dres.ptr, m.dres.ld) if m.dres else (0, 0)
        it.sums, it.n_rep, it.red_ws = m.sums[sums_idx].data_ptr(), 1, m.red_ws.data_ptr()
        it.dgamma, it.dbeta = m.dgamma.data_ptr(), m.dbeta.data_ptr()
        it.M, it.C = m.M, m.C
        it.eps, it.momentum = EPS, MOM
        it.inv_count, it.dparam_scale = 1.0 / (m.M * m.R), m.dscale
        it.fwd_flags, it.bwd_flags = m.fwd_flags, m.bwd_flags
        for ph in PHASES:
            ends[ph] += 0 if ph in m.zero else n_blocks(lib, ph, m.M, m.C, dtype)
        it.blk_stats, it.blk_apply, it.blk_red, it.blk_bapply = (ends[ph] for ph in PHASES)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return tab, ends


def group_local(members, dev):
    """the group's local statistics row: member i at offset loff_i, 2*C_i+1 floats each (sentinel before the launch)"""
    width = sum(2 * m.C + 1 for m in members)
    local = sent((width,), dev)
    off = 0
    for m in members:
        m.loff = off
        m.local_ptr = local.data_ptr() + 4 * off
        off += 2 * m.C + 1
    return local, width


# ----------------------------------------------------------------------------------------------------------- checks
def check_finalized(m, out, S, M2, cnt, dS, dM2, rm, rv, what):
    """mean / invstd / scale / shift / running statistics against float64 of (S, M2, cnt) whose fp32 evaluation carries
    errors up to dS, dM2: every operation of the finalize adds one rounding (u relative), rsqrtf up to 2 ulp (4 u)"""
    C_ = m.C
    gamma, beta = m.p['gamma'][:C_].double(), m.p['beta'][:C_].double()
    mean = S / cnt
    dmean = dS / cnt + U * mean.abs()
    var = M2 / cnt
    dvar = dM2 / cnt + U * var
    inv = (var + EPS).rsqrt()
    rel_inv = 0.5 * (dvar + U * (var + EPS) + U * EPS) / (var + EPS) + 4 * U     # (+ eps, eps in fp32; rsqrtf: 2 ulp allowed)
    sc = gamma * inv
    dsc = sc.abs() * (rel_inv + U)
    sh = beta - mean * sc
    dsh = dmean * sc.abs() + mean.abs() * dsc + U * (mean * sc).abs() + U * sh.abs()
    g = lambda k: out[k][:C_].double()           # noqa: E731
    check_bound(g('mean'), mean, dmean * (1 + 2 * U), f'{what} mean')
    check_bound(g('invstd'), inv, inv * rel_inv * (1 + 2 * U), f'{what} invstd')
    check_bound(g('scale'), sc, dsc * (1 + 2 * U), f'{what} scale')
    check_bound(g('shift'), sh, dsh * (1 + 2 * U), f'{what} shift')
    if rm is None:                               # running_mean = running_var = NULL: nothing more was written
        return
    mom = float(torch.tensor(MOM, dtype=torch.float32))
    rm0, rv0 = m.rm0.double(), m.rv0.double()
    unb = M2 / (cnt - 1) if cnt > 1 else var
    dunb = dM2 / max(cnt - 1, 1) + U * unb
    rm_ref = (1 - mom) * rm0 + mom * mean
    rv_ref = (1 - mom) * rv0 + mom * unb
    check_bound(rm[:C_].double(), rm_ref, 4 * U * ((1 - mom) * rm0.abs() + mom * mean.abs()) + mom * dmean, f'{what} running_mean')
    check_bound(rv[:C_].double(), rv_ref, 4 * U * ((1 - mom) * rv0.abs() + mom * unb.abs()) + mom * dunb, f'{what} running_var')


def stats_reference(m, threads=256):
    """float64 of the stored partials: S, M2, and the bounds of the kernel's fold of them (stats_chain)"""
    ps, pq = m.ps(), m.pq()
    n = m.tile_n[:, None]
    S = ps.sum(0)
    mean = S / m.M
    chain = stats_chain(m.n_tiles, threads)
    dS = chain * U * ps.abs().sum(0)
    a = ps / n
    d = a - mean
    M2 = (pq + n * d * d).sum(0)
    dM2 = m2_bound(n, U * a.abs(), d, pq, torch.zeros_like(pq), dS / m.M + U * mean.abs(), chain)
    return S, M2, dS, dM2, ps.abs().sum(0)


def check_local(m, local, S, M2, dS, dM2, sabs, what):
    """the local statistics row (S[C], M2[C], count) of one member"""
    row = local[m.loff:m.loff + 2 * m.C + 1].double()
    assert float(row[2 * m.C]) == m.M, f'{what}: count'
    if m.exact:
        assert torch.equal(row[:m.C], S), f'{what}: S not exact'
    check_bound(row[:m.C], S, dS, f'{what} S')
    check_bound(row[m.C:2 * m.C], M2, dM2, f'{what} M2')
    if not m.exact:
        report(f'{what} S', (row[:m.C] - S).abs(), sabs)


def reference_y(m):
    o = m.x.val() * m.scale + m.shift
    if m.res:
        o = o + m.res.val()
    return o.clamp_min(0) if m.relu else o


def check_apply(m, what):
    """y = act(x*scale + shift [+ res]): at most three roundings (product, sum, residual sum) of the fp32 evaluation"""
    m.y.check_frame(f'{what} y')
    ref = reference_y(m)
    got = m.y.val()
    if m.exact:
        assert torch.equal(got, ref), f'{what}: y not exact'
        return
    terms = (m.x.val() * m.scale).abs() + m.shift.abs() + (m.res.val().abs() if m.res else 0)
    bound = 3 * U * terms
    if m.dtype == DV_BF16:
        bound = bound * (1 + BF16_U) + BF16_U * ref.abs()
    check_bound(got, ref, bound, f'{what} y')


def backward_terms(m, y_in):
    """g (masked), xhat, float64.  The mask is the y the backward was given (> 0), or DV_MASK_FROM_X's relu(x*scale+shift)
    -- which the forward's y equals bit for bit; with exact data both equal float64's"""
    g = m.dy.val()
    if m.relu:
        act = y_in
        if m.exact:
            pre = m.x.val() * m.scale + m.shift + (m.res.val() if m.res else 0)
            assert torch.equal(act > 0, pre > 0)
        g = g * (act > 0).double()
    xhat = (m.x.val() - m.mean) * m.invstd
    return g, xhat


def check_reduce(m, s, g, xhat, idx, what):
    """ordered sums [2][CP] = (sum g, sum g*xhat); a term g*(x - mean)*invstd is two roundings away from float64"""
    C_, CP = m.C, m.CP
    sg, sgx = g.sum(0), (g * xhat).sum(0)
    got = s.double()
    assert bool((got[C_:CP] == 0).all()) and bool((got[CP + C_:] == 0).all()), f'{what}: pad lanes of the sums'
    nblk = n_blocks(L.load(), 'red', m.M, C_, m.dtype)
    chain = bwd_reduce_chain(m.M, C_, m.dtype, nblk)
    if m.exact:
        assert torch.equal(got[:C_], sg) and torch.equal(got[CP:CP + C_], sgx), f'{what}: ordered sums not exact'
    check_bound(got[:C_], sg, chain * U * g.abs().sum(0), f'{what} sum g')
    check_bound(got[CP:CP + C_], sgx, (chain + 3) * U * (g * xhat).abs().sum(0), f'{what} sum g*xhat')
    if not m.exact and idx == 0:
        report(f'{what} sum g (L={chain})', (got[:C_] - sg).abs(), g.abs().sum(0))
        report(f'{what} sum g*xhat', (got[CP:CP + C_] - sgx).abs(), (g * xhat).abs().sum(0))


def check_ticket_area(m, what):
    nblk = n_blocks(L.load(), 'red', m.M, m.C, m.dtype)
    ngrp = ceil_div(nblk, 32)
    tick = m.red_ws[(nblk + ngrp) * 2 * m.CP:]
    assert tick.numel() >= ngrp + 1 and tick.numel() % 8 == 0
    assert bool((tick == 0).all()), f'{what}: ticket words left behind'


def check_bwd_apply(m, g, sums_in, inv_count, what, dg0=None, db0=None, dsums=None, dparams=True):
    """dx = k1 g + k2 x + k3 (k1 = gamma invstd, k2 = -k1 invstd sgx inv_count, k3 = -k1 sg inv_count - k2 mean): k1 one
    rounding, k2 four, k3 <= 5 u |k3| + 10 u |k2 mean| (|k1 sg inv_count| <= |k3| + |k2 mean|), the fp32 expression
    three more -> 12 u (|k1 g| + |k2 x| + |k3| + |k2 mean|).  dres (+)= g: exact, one rounding with DV_ACCUM.
    dgamma += dparam_scale sgx, dbeta += dparam_scale sg: two roundings.
    dsums = (dsg, dsgx): what the kernel's own fp32 fold of n_rep replicas may differ by from the sums_in given here (their
    float64 total); it enters k2, k3 and dgamma / dbeta.  dparams = False: dgamma = dbeta = NULL was passed, both stay."""
    C_, CP = m.C, m.CP
    x = m.x.val()
    sin = sums_in.double()
    sg, sgx = sin[:C_], sin[CP:CP + C_]
    k1 = m.gamma * m.invstd
    k2 = -k1 * m.invstd * sgx * inv_count
    k3 = -k1 * sg * inv_count - k2 * m.mean
    ref = k1 * g + k2 * x + k3
    bound = 12 * U * ((k1 * g).abs() + (k2 * x).abs() + k3.abs() + (k2 * m.mean).abs())
    if dsums is not None:
        dk2 = (k1 * m.invstd * inv_count).abs() * dsums[1]
        bound = bound + (dk2 * x.abs() + (k1 * inv_count).abs() * dsums[0] + dk2 * m.mean.abs()) * (1 + 16 * U)
    if m.dtype == DV_BF16:
        bound = bound * (1 + BF16_U) + BF16_U * ref.abs()
    m.dx.check_frame(f'{what} dx')
    check_bound(m.dx.val(), ref, bound, f'{what} dx')
    if not m.exact and m.dtype == DV_F32:
        report(f'{what} dx (12 u allowed)', (m.dx.val() - ref).abs(),
               (k1 * g).abs() + (k2 * x).abs() + k3.abs() + (k2 * m.mean).abs())
    if m.dres:
        m.dres.check_frame(f'{what} dres')
        dref = g + (m.dres0 if m.dres0 is not None else 0)
        if m.exact:
            assert torch.equal(m.dres.val(), dref), f'{what}: dres not exact'
        else:
            b = U * dref.abs() * (1 + BF16_U) + (BF16_U * dref.abs() if m.dtype == DV_BF16 else 0)
            check_bound(m.dres.val(), dref, b, f'{what} dres')
    dg0 = m.dg0 if dg0 is None else dg0
    db0 = m.db0 if db0 is None else db0
    if not dparams:
        assert torch.equal(m.dgamma[:C_].double(), dg0) and torch.equal(m.dbeta[:C_].double(), db0), f'{what}: NULL dgamma / dbeta'
        return
    dgr, dbr = dg0 + m.dscale * sgx, db0 + m.dscale * sg
    dgk, dbk = m.dgamma[:C_].double(), m.dbeta[:C_].double()
    assert bool((m.dgamma[C_:] == 0.625).all()) and bool((m.dbeta[C_:] == 0.625).all()), f'{what}: dgamma / dbeta pad lanes'
    if m.exact_dparams:
        assert torch.equal(dgk, dgr) and torch.equal(dbk, dbr), f'{what}: dgamma / dbeta not exact'
    extra = (0, 0) if dsums is None else (m.dscale * dsums[0], m.dscale * dsums[1])
    check_bound(dgk, dgr, 2 * U * (dg0.abs() + (m.dscale * sgx).abs()) + extra[1], f'{what} dgamma')
    check_bound(dbk, dbr, 2 * U * (db0.abs() + (m.dscale * sg).abs()) + extra[0], f'{what} dbeta')


def assert_exact_data_fits(m, g, xhat):
    """(A): every partial sum of every kernel is a multiple of the terms' dyadic unit below 2^24 units"""
    if not m.exact:
        return
    assert float(m.x.val().abs().sum(0).max()) < 2 ** 24                      # S: integers
    assert float((g * xhat).abs().sum(0).max()) < 2 ** 24 / 8                 # g (x - mean) invstd: multiples of 1/8
    assert float(g.abs().sum(0).max()) < 2 ** 24
    sgx = (g * xhat).sum(0)
    assert float((m.dg0.abs() + (m.dscale * sgx).abs()).max()) < 2 ** 24 / 16  # dgamma: multiples of 1/16
