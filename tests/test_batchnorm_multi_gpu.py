"""The multi-tensor BatchNorm entries (dv_bn_stats_multi, dv_bn_finalize_multi, dv_bn_apply_multi, the ORDERED
dv_bn_bwd_reduce_multi and dv_bn_bwd_apply_multi) against a plain float64 reference of the same operation.

A training-mode BatchNorm group of two or more members runs its forward through these entries, and so does the backward of
every group and of a lone member that takes its ReLU mask from x (dualvar_amd/engine.py BNGroupOp.launches); the other lone
members take the single-tensor entries (tests/test_batchnorm_single_gpu.py).  The item tables here are built from explicit
tensors, never by the engine, with the engine's block-count rules; a member may be given 0 blocks in any phase.  Two kinds of
data:

  (A) exactly representable: integer x in [-2, 2], g in {-1, 0, 1} (sparse), dyadic mean / invstd / scale / shift / gamma
      and dparam_scale in {1, 1/2}.  Every sum the kernels form is then exact in fp32 whatever the order (asserted on the
      host: sum |terms| < 2^24 units of the terms' common dyadic unit), so S, count, sum g, sum g*xhat, dbeta, dgamma, y,
      dres and the ReLU mask must equal float64 BIT FOR BIT: a dropped or doubled row, block, fold group or channel shows
      at any M.  (Also exact in bf16.)
  (B) Gaussian data at the step's shapes, against float64 with DERIVED bounds (u = 2^-24):
        sums:         |err| <= L u sum|terms|, L the longest chain of sequential fp32 additions (bwd_reduce_chain,
                      stats_chain below) plus the roundings inside one term
        elementwise:  a stated count of roundings x u x the magnitudes of the terms of the kernel's own expression, and
                      2^-8 |ref| more for a bf16 store (its unit roundoff: 8 significant bits).
      err / (u sum|terms|) is printed per case (-s): what the fp32 folds cost against float64.

Every case also checks the sentinels: input columns outside [off, off+CP) hold NaN and pad lanes [C, CP) finite junk;
output columns outside [off, off+CP) keep their sentinel bits; output lanes [C, CP) of y / dx / dres are 0; every output of a
zero-block member is untouched; the whole ticket area of every red_ws is zero after each launch; and two launches of the
ordered reduce give the same bits."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import (DV_ACCUM, DV_BF16, DV_F32, DV_MASK_FROM_X, DV_NO_RELU_MASK, DV_RELU, DV_STATS,  # noqa: E402
                              DV_W3)

U = 2.0 ** -24
BF16_U = 2.0 ** -8                 # unit roundoff of a bf16 store (8 significant bits)
DTYPES = [pytest.param(DV_F32, id='fp32'), pytest.param(DV_BF16, id='bf16')]
PHASES = ('stats', 'apply', 'red', 'bapply')
SENT = {DV_F32: (torch.int32, 0x7fb12345), DV_BF16: (torch.int16, 0x7fb1)}      # NaN bit patterns no kernel produces
JUNK = 3.0                                                                       # pad lanes [C, CP) of every input
EPS, MOM = 1e-5, 0.1


def cp8(c):
    return (c + 7) & ~7


def vec(dtype):
    return 4 if dtype == DV_F32 else 8


def ceil_div(a, b):
    return -(-a // b)


def n_blocks(lib, phase, M, C_, dtype):
    """engine.BNMember.blocks' block counts"""
    if phase == 'stats':
        return C_
    if phase == 'red':
        return int(lib.dv_bn_bwd_blocks(M, C_))
    total = M * (cp8(C_) // vec(dtype))
    return max(1, min(4096 if phase == 'apply' else 2048, ceil_div(total, 256)))


def column_chain(rows, CP, dtype, NS, extra=0):
    """longest chain of sequential fp32 additions column_reduce (elementwise.hip) forms over `rows` rows of CP columns with NS
    sums per column: rows per thread, then ceil(log2 rg) for the pairwise fold of the rg row groups; `extra` is what the caller
    adds behind it (block folds, or the blocks that add to one replica with float atomics; 0: every output has one owner)"""
    V, CV = vec(dtype), CP // vec(dtype)
    chain = 0
    for cvb in range(0, CV, 256):
        cvc = min(256, CV - cvb)
        rg = 256 // cvc
        while rg > 1 and rg * cvc * V * NS > 4096:
            rg >>= 1
        chain = max(chain, ceil_div(rows, rg) + math.ceil(math.log2(rg)))
    return chain + extra


def bwd_reduce_chain(M, C_, dtype, nblk):
    """longest chain of sequential fp32 additions of bn_bwd_reduce_body + ordered_fold (elementwise.hip): column_chain over
    the rows of one block, the fold of a group of <= 32 block rows, the fold of the groups"""
    return column_chain(ceil_div(M, nblk), cp8(C_), dtype, 2, min(32, nblk) + ceil_div(nblk, 32))


def stats_chain(n_tiles, threads=256):
    """bn_reduce_stats_body with `threads` threads: tiles per thread, the 64-lane shuffle tree, the threads / 64 wave sums in a
    row (256 threads: 4; the single-tensor launch runs 1024 from 2048 tiles: 16)"""
    return ceil_div(n_tiles, threads) + 6 + threads // 64


# ----------------------------------------------------------------------------------------------------------- buffers
def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def sentinel_like(shape, dtype, dev):
    it, v = SENT[dtype]
    return torch.full(shape, v, dtype=it, device=dev).view(ops.TORCH_DTYPE[dtype])


def f32_sentinel(n, dev):
    return sentinel_like((n,), DV_F32, dev)


def is_sentinel(t, dtype):
    it, v = SENT[dtype]
    return bool((bits(t) == v).all())


class View:
    """[M][C] values as a channel slice at `off` of a [M][ld] buffer (row pitch ld): columns outside [off, off+CP) NaN (inputs)
    or sentinel bits (outputs), pad lanes [C, CP) JUNK (inputs)"""

    def __init__(self, dtype, M, C_, off, ld, dev, values=None, junk=True):
        self.dtype, self.M, self.C, self.CP, self.off, self.ld = dtype, M, C_, cp8(C_), off, ld
        assert off % 8 == 0 and ld % 8 == 0 and off + self.CP <= ld
        self.buf = sentinel_like((M, ld), dtype, dev)
        if values is not None:
            self.set(values, junk)

    def set(self, values, junk=True):
        self.buf[:, self.off:self.off + self.C] = values.to(self.buf.dtype)
        if junk:
            self.buf[:, self.off + self.C:self.off + self.CP] = JUNK

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def val(self):
        return self.buf[:, self.off:self.off + self.C].double()

    def check_frame(self, what):
        """outside [off, off+CP): sentinel bits; pad lanes: exactly 0"""
        assert is_sentinel(self.buf[:, :self.off], self.dtype) and is_sentinel(self.buf[:, self.off + self.CP:], self.dtype), \
            f'{what}: a column outside the view was written'
        assert bool((self.buf[:, self.off + self.C:self.off + self.CP] == 0).all()), f'{what}: pad lanes [C, CP) not zero'

    def untouched(self):
        return is_sentinel(self.buf, self.dtype)


def chan(vals, CP, dev, junk=0.625):
    """per-channel fp32 array readable up to CP (16-byte loads), junk in the pad lanes"""
    t = torch.full((CP,), junk, dtype=torch.float32, device=dev)
    t[:vals.numel()] = vals
    return t


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
        self.x = View(dtype, M, C_, *layout(), dev, x)
        self.res = View(dtype, M, C_, *layout(), dev, r) if res else None
        self.dy = View(dtype, M, C_, *layout(), dev, dyv)
        # outputs
        self.y = View(dtype, M, C_, *layout(), dev)
        self.dx = View(dtype, M, C_, *layout(), dev)
        self.dres = View(dtype, M, C_, *layout(), dev, dres0 if accum else None) if res else None
        self.dres0 = dres0 if (res and accum) else None
        # per-channel parameters (read) and outputs (written)
        self.p = {k: chan(v.float(), CP, dev) for k, v in
                  (('mean', mean), ('invstd', invstd), ('gamma', gamma), ('beta', beta), ('scale', scale), ('shift', shift))}
        self.o = {k: f32_sentinel(CP, dev) for k in ('mean', 'invstd', 'scale', 'shift')}
        self.rm0 = (torch.randint(-8, 9, (C_,), generator=g, device=dev).float() / 8)
        self.rv0 = 0.5 + torch.randint(0, 9, (C_,), generator=g, device=dev).float() / 8
        self.rm, self.rv = chan(self.rm0, CP, dev), chan(self.rv0, CP, dev)
        self.dgamma, self.dbeta = chan(dg0.float(), CP, dev), chan(db0.float(), CP, dev)
        self.sums = [f32_sentinel(2 * CP, dev) for _ in range(2)]
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
    local = f32_sentinel(width, dev)
    off = 0
    for m in members:
        m.loff = off
        m.local_ptr = local.data_ptr() + 4 * off
        off += 2 * m.C + 1
    return local, width


def launch(name, *args):
    L.check(getattr(L.load(), name)(*args, ops.stream_ptr()), name)


def report(what, err, scale):
    """err / (u * sum|terms|), the largest over the channels"""
    r = float((err / (U * scale.clamp_min(1e-300))).max())
    print(f'    {what:<34s} max err / (u sum|terms|) = {r:8.3f}')
    return r


def check_bound(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} values outside the bound, worst err {float(err.max()):.3e} ' \
                                f'(bound there {float(bound.flatten()[int(torch.argmax((err - bound).flatten()))]):.3e})'


# ----------------------------------------------------------------------------------------------------------- checks
def m2_bound(n, da, d, Q, dQ, dmean, chain):
    """error bound of the fp32 M2 = sum_i (Q_i + n_i d_i^2), d_i = a_i - mean, evaluated term by term ([terms][C]):
    a_i carries da_i, mean dmean, Q_i dQ_i; then d (1 rounding), n*d*d (2), Q + n d^2 (1), and a fold of `chain` additions"""
    dd = da + dmean + U * (d.abs() + da + dmean)
    ad = d.abs() + dd
    term = Q + dQ + n * ad * ad
    e = dQ + n * (2 * d.abs() * dd + dd * dd) + 2 * U * n * ad * ad + U * term
    return e.sum(0) + chain * U * term.sum(0)


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


# ----------------------------------------------------------------------------------------------------------- driver
def run_group(dev, dtype, members, what, max_c=None):
    """one group through stats_multi(finalize=1) -> apply_multi -> 2x ordered bwd_reduce_multi -> bwd_apply_multi"""
    lib = L.load()
    n = len(members)
    print(f'\n  {what}: ' + ', '.join(f'M={m.M} C={m.C}' + (f' zero={sorted(m.zero)}' if m.zero else '') for m in members))
    local, _ = group_local(members, dev)
    stab, ends = make_table(members, lib, dev, dtype, stats_outputs=True)
    launch('dv_bn_stats_multi', stab.data_ptr(), n, 1, ends['stats'])
    torch.cuda.synchronize()
    for i, m in enumerate(members):
        w = f'{what}[{i}]'
        if 'stats' in m.zero:
            assert is_sentinel(local[m.loff:m.loff + 2 * m.C + 1], DV_F32) and all(is_sentinel(t, DV_F32) for t in m.o.values())
            assert torch.equal(m.rm[:m.C], m.rm0) and torch.equal(m.rv[:m.C], m.rv0), f'{w}: zero-block member written'
            continue
        S, M2, dS, dM2, sabs = stats_reference(m)
        check_local(m, local, S, M2, dS, dM2, sabs, w)
        assert all(is_sentinel(t[m.C:], DV_F32) for t in m.o.values()), f'{w}: stats outputs past C'
        check_finalized(m, m.o, S, M2, m.M, dS, dM2, m.rm, m.rv, w)

    tab, ends = make_table(members, lib, dev, dtype)
    if ends['apply']:
        launch('dv_bn_apply_multi', dtype, tab.data_ptr(), n, ends['apply'])
    torch.cuda.synchronize()
    y_in = []
    for i, m in enumerate(members):
        if 'apply' in m.zero:
            assert m.y.untouched(), f'{what}[{i}]: y of a zero-block member written'
            m.y.set(reference_y(m), junk=False)                  # the backward's input
            m.y.buf[:, m.y.off + m.C:m.y.off + m.CP] = 0
        else:
            check_apply(m, f'{what}[{i}]')
        y_in.append(m.y.val())
        m.y.buf[:, m.y.off + m.C:m.y.off + m.CP] = JUNK          # pad lanes of the backward's input: junk

    gx = []
    for i, m in enumerate(members):
        g, xhat = backward_terms(m, y_in[i])
        assert_exact_data_fits(m, g, xhat)
        gx.append((g, xhat))
    for k in range(2):                                         # exactly two launches: the same bits, tickets zero after each
        tk, ends = make_table(members, lib, dev, dtype, sums_idx=k)
        if ends['red']:
            launch('dv_bn_bwd_reduce_multi', dtype, tk.data_ptr(), n, ends['red'])
        torch.cuda.synchronize()
        for i, m in enumerate(members):
            check_ticket_area(m, f'{what}[{i}] launch {k}')
    for i, m in enumerate(members):
        w = f'{what}[{i}]'
        if 'red' in m.zero:
            assert all(is_sentinel(s, DV_F32) for s in m.sums) and bool((m.red_ws == 0).all()), f'{w}: zero-block reduce wrote'
            ref = torch.zeros(2 * m.CP, dtype=torch.float64, device=dev)
            g, xhat = gx[i]
            ref[:m.C], ref[m.CP:m.CP + m.C] = g.sum(0), (g * xhat).sum(0)
            m.sums[0].copy_(ref.float())
            continue
        assert torch.equal(bits(m.sums[0]), bits(m.sums[1])), f'{w}: two ordered reduces differ'
        check_reduce(m, m.sums[0], *gx[i], 0, w)

    if ends['bapply']:
        launch('dv_bn_bwd_apply_multi', dtype, tab.data_ptr(), n, ends['bapply'], max_c or max(m.C for m in members))
    torch.cuda.synchronize()
    for i, m in enumerate(members):
        w = f'{what}[{i}]'
        if 'bapply' in m.zero:
            assert m.dx.untouched(), f'{w}: dx of a zero-block member written'
            if m.dres:
                assert (m.dres.untouched() if m.dres0 is None else torch.equal(m.dres.val(), m.dres0)), f'{w}: dres written'
            assert torch.equal(m.dgamma[:m.C].double(), m.dg0) and torch.equal(m.dbeta[:m.C].double(), m.db0)
            continue
        check_bwd_apply(m, gx[i][0], m.sums[0], 1.0 / m.M, w)


# ----------------------------------------------------------------------------------------------------------- cases
def members_of(dev, dtype, specs, exact, seed=0):
    return [Member(dev, dtype, *sp[:2], seed=seed + 17 * k, exact=exact, **sp[2]) for k, sp in enumerate(specs)]


# (M, C, options).  Rows per reduce block: 32 up to M = 2048, then 64; at most 320 blocks, 1024 from M = 300 000; fold groups
# of 32 blocks.
CASES = {
    # one fold group: M = 2 and M < 32 (one block), M = 1000 (32 blocks, the last one 8 rows), M = 1024 (exactly 32 blocks)
    'one_group': (True, [(2, 16, {}), (31, 3, dict(res=True, views=True)), (1000, 83, dict(res=True, accum=True, views=True)),
                         (1024, 8, dict(from_x=True, dscale=0.5))]),
    # ragged groups: Mixed_5 (36 blocks: 32 + 4), Mixed_4 (196 blocks, last group 4), 197 blocks whose last holds one row
    'ragged_groups': (True, [(1152, 230, dict(res=True, views=True, part_pitch_extra=24)), (12544, 64, dict(from_x=True)),
                             (12545, 24, dict(relu=False, res=True, accum=True, dscale=0.5))]),
    # the 320-block cap, and the 1 024-block cap at the stem's shape (M = 128*8*56*56, C = 64)
    'caps': (True, [(100000, 24, dict(res=True, views=True)), (128 * 8 * 56 * 56, 64, dict(dscale=0.5))]),
    # channels and the n > 8 branch of find_item, with zero-block members first, in the middle and last
    'channels_n12': (True, [(300, 1, dict(zero=('apply', 'red', 'bapply'))), (300, 3, {}), (64, 83, dict(views=True)),
                            (520, 230, dict(res=True, accum=True)), (96, 1024, dict(from_x=True)),
                            (40, 16, dict(zero=('stats',))), (200, 8, dict(relu=False)), (77, 24, dict(res=True)),
                            (2050, 40, dict(zero=('red',), views=True)), (33, 128, dict(from_x=True, dscale=0.5)),
                            (700, 56, {}), (500, 12, dict(zero=('apply', 'bapply')))]),
    'n9': (True, [(64 * (k + 1), 8 * (k + 1), dict(res=k % 2 == 1, views=k % 3 == 0)) for k in range(9)]),
    'n8': (True, [(100 + 37 * k, 3 + 13 * k, dict(zero=('red',)) if k == 7 else {}) for k in range(8)]),
    # the widest channel counts: column_reduce's 4096-float LDS budget (2048 bf16 = 256 vectors x 8), and max_c = 3072, the
    # largest bwd_apply_multi accepts (5 x 3072 floats of LDS)
    'wide': (True, [(300, 2048, dict(views=True)), (40, 3072, dict(res=True))]),
}
GAUSS = {
    # the stem (M = 128*8*56*56, C = 64: 1 024 reduce blocks in 32 groups), Mixed_4 (12 544 rows, 196 blocks) and the
    # R(2+1)D widths (83 / 230 mid channels, C % 8 != 0) at 32 samples x 3 views
    'stem': [(128 * 8 * 56 * 56, 64, {})],
    'mixed4_12544': [(12544, 64, dict(from_x=True)), (12544, 96, dict(res=True, views=True)), (12544, 208, {}),
                     (1152, 832, dict(res=True, accum=True))],
    'r21d_widths': [(96 * 4 * 28 * 28, 230, dict(res=True, accum=True)), (96 * 2 * 14 * 14, 83, dict(views=True))],
}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', list(CASES))
def test_multi_exact_data(gpu, dtype, case):
    exact, specs = CASES[case]
    members = members_of(gpu, dtype, specs, exact, seed=11 * list(CASES).index(case))
    run_group(gpu, dtype, members, f'{case} (A)')
    if case == 'wide':
        tab, ends = make_table(members, L.load(), gpu, dtype)
        rc = L.load().dv_bn_bwd_apply_multi(dtype, tab.data_ptr(), len(members), ends['bapply'], 3073, ops.stream_ptr())
        assert rc == -3                                        # DV_EUNSUPPORTED, nothing launched


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', list(GAUSS))
def test_multi_gaussian_against_float64(gpu, dtype, case):
    members = members_of(gpu, dtype, GAUSS[case], False, seed=100 + 11 * list(GAUSS).index(case))
    run_group(gpu, dtype, members, f'{case} (B)')


@pytest.mark.parametrize('dtype', DTYPES)
def test_stats_multi_then_finalize_multi_is_syncbn(gpu, dtype):
    """three ranks (different row counts) run stats_multi(finalize=0) into their own row of the gathered table;
    finalize_multi over it matches float64 over all rows.  With R = 1, finalize_multi equals stats_multi(finalize=1) bit for
    bit."""
    lib = L.load()
    specs = [(1000, 83, {}), (12544, 24, dict(part_pitch_extra=16)), (333, 230, {})]
    ranks = [members_of(gpu, dtype, [(M + 97 * r, C_, o) for M, C_, o in specs], False, seed=7 + 31 * r) for r in range(3)]
    width = sum(2 * m.C + 1 for m in ranks[0])
    gathered = f32_sentinel(3 * width, gpu).view(3, width)
    for r, mem in enumerate(ranks):
        group_local(mem, gpu)
        rows = [gathered[r].data_ptr() + 4 * m.loff for m in mem]
        tab, ends = make_table(mem, lib, gpu, dtype, stats_outputs=True, rank_local=rows)
        launch('dv_bn_stats_multi', tab.data_ptr(), len(mem), 0, ends['stats'])
    torch.cuda.synchronize()
    for r, mem in enumerate(ranks):
        for m in mem:
            assert all(is_sentinel(t, DV_F32) for t in m.o.values()), 'finalize = 0 wrote the affine map'
            assert torch.equal(m.rm[:m.C], m.rm0), 'finalize = 0 moved the running statistics'
    me = ranks[0]                                              # this rank's items: local row, parameters, outputs
    local, _ = group_local(me, gpu)
    tab, _ = make_table(me, lib, gpu, dtype, stats_outputs=True)
    nb = sum(ceil_div(m.C, 128) for m in me)
    launch('dv_bn_finalize_multi', tab.data_ptr(), len(me), nb, local.data_ptr(), gathered.data_ptr(), 3, width)
    torch.cuda.synchronize()
    for i, m in enumerate(me):
        w = f'syncbn fwd[{i}]'
        per = [stats_reference(mem[i]) for mem in ranks]
        for r, (S, M2, dS, dM2, sabs) in enumerate(per):
            check_local(ranks[r][i], gathered[r], S, M2, dS, dM2, sabs, f'{w} rank {r}')
        # float64 over all rows (of the partials every rank stored), and the bounds through the rank fold (R = 3 additions)
        ps = torch.cat([mem[i].ps() for mem in ranks])
        pq = torch.cat([mem[i].pq() for mem in ranks])
        nn = torch.cat([mem[i].tile_n for mem in ranks])[:, None]
        cnt = sum(mem[i].M for mem in ranks)
        S = ps.sum(0)
        mean = S / cnt
        M2 = (pq + nn * (ps / nn - mean) ** 2).sum(0)
        # the finalize works on the ranks' rows: S_r with error dS_r, M2_r with dM2_r
        Sr = torch.stack([p[0] for p in per])
        dSr = torch.stack([p[2] for p in per])
        dM2r = torch.stack([p[3] for p in per])
        nr = torch.tensor([float(mem[i].M) for mem in ranks], dtype=torch.float64, device=gpu)[:, None]
        dS = dSr.sum(0) + 3 * U * (Sr.abs() + dSr).sum(0)
        Q = torch.stack([p[1] for p in per])
        a = Sr / nr
        dM2 = m2_bound(nr, dSr / nr + U * a.abs(), a - mean, Q, dM2r, dS / cnt + U * mean.abs(), 3)
        check_finalized(m, m.o, S, M2, cnt, dS, dM2, m.rm, m.rv, w)
    # R = 1: finalize_multi over one gathered row == stats_multi(finalize = 1), bit for bit
    outs = []
    for how in ('finalize_multi', 'stats_multi'):
        mem = members_of(gpu, dtype, specs, False, seed=7)
        loc, width = group_local(mem, gpu)
        tab, ends = make_table(mem, lib, gpu, dtype, stats_outputs=True)
        if how == 'finalize_multi':
            launch('dv_bn_stats_multi', tab.data_ptr(), len(mem), 0, ends['stats'])
            launch('dv_bn_finalize_multi', tab.data_ptr(), len(mem), nb, loc.data_ptr(), loc.data_ptr(), 1, width)
        else:
            launch('dv_bn_stats_multi', tab.data_ptr(), len(mem), 1, ends['stats'])
        torch.cuda.synchronize()
        outs.append([bits(t).clone() for m in mem for t in (*m.o.values(), m.rm, m.rv)] + [bits(loc).clone()])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(*outs))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('exact', [pytest.param(True, id='exact'), pytest.param(False, id='gauss')])
def test_ordered_reduce_then_apply_is_syncbn_backward(gpu, dtype, exact):
    """per-rank ordered reduces, summed in place of the all-reduce, then per-rank bwd_apply_multi with inv_count = 1/(M R) and
    dparam_scale = 1/R: dx and the summed sums match float64 over all rows, every rank's dgamma / dbeta = start + total / R"""
    lib = L.load()
    R = 3
    specs = [(1152, 83, dict(res=True, accum=True, R=R, dscale=1 / R)), (12544, 24, dict(from_x=True, R=R, dscale=1 / R))]
    ranks = [members_of(gpu, dtype, specs, exact, seed=50 + 13 * r) for r in range(R)]
    for mem in ranks[1:]:                                     # the ranks share the (global) statistics and parameters
        for m, m0 in zip(mem, ranks[0]):
            for k in m.p:
                m.p[k].copy_(m0.p[k])
            m.mean, m.invstd, m.gamma, m.scale, m.shift = m0.mean, m0.invstd, m0.gamma, m0.scale, m0.shift
            m.dgamma.copy_(m0.dgamma)
            m.dbeta.copy_(m0.dbeta)
            m.dg0, m.db0 = m0.dg0, m0.db0
    gx = []
    for mem in ranks:
        tab, ends = make_table(mem, lib, gpu, dtype)
        launch('dv_bn_apply_multi', dtype, tab.data_ptr(), len(mem), ends['apply'])
        launch('dv_bn_bwd_reduce_multi', dtype, tab.data_ptr(), len(mem), ends['red'])
        torch.cuda.synchronize()
        gx.append([backward_terms(m, m.y.val()) for m in mem])
        for i, m in enumerate(mem):
            check_ticket_area(m, f'syncbn bwd [{i}]')
    total = [ranks[0][i].sums[0] + ranks[1][i].sums[0] + ranks[2][i].sums[0] for i in range(len(specs))]   # the all-reduce, fp32
    for i in range(len(specs)):
        g = torch.cat([gx[r][i][0] for r in range(R)])
        xh = torch.cat([gx[r][i][1] for r in range(R)])
        CP, C_ = ranks[0][i].CP, ranks[0][i].C
        nblk = n_blocks(lib, 'red', ranks[0][i].M, C_, dtype)
        chain = bwd_reduce_chain(ranks[0][i].M, C_, dtype, nblk) + R
        t = total[i].double()
        if exact:
            assert torch.equal(t[:C_], g.sum(0)) and torch.equal(t[CP:CP + C_], (g * xh).sum(0))
        check_bound(t[:C_], g.sum(0), chain * U * g.abs().sum(0), 'syncbn sum g')
        check_bound(t[CP:CP + C_], (g * xh).sum(0), (chain + 3) * U * (g * xh).abs().sum(0), 'syncbn sum g*xhat')
        for r in range(R):
            ranks[r][i].sums[0].copy_(total[i])
    for r, mem in enumerate(ranks):
        tab, ends = make_table(mem, lib, gpu, dtype)
        launch('dv_bn_bwd_apply_multi', dtype, tab.data_ptr(), len(mem), ends['bapply'], max(m.C for m in mem))
    torch.cuda.synchronize()
    for r, mem in enumerate(ranks):
        for i, m in enumerate(mem):
            check_bwd_apply(m, gx[r][i][0], total[i], 1.0 / (m.M * R), f'syncbn bwd rank {r} [{i}]')


@pytest.mark.parametrize('dtype', DTYPES)
def test_stats_from_conv_epilogue_partials(gpu, dtype):
    """a pointwise conv with DV_STATS whose Cout is split into three members, as the engine slices a merged conv (partials
    pointer at the member's first channel, pitch = Cout): the statistics against float64 of the STORED conv output.
    The epilogue's tile sum and M2 add at most tile_rows terms in a row.  fp32 takes M2 about the tile mean (two passes);
    bf16 about a provisional centre c, one of the tile's values (conv.hip), merged with Chan's formula: its terms are
    bounded by (x - c)^2 <= 4 max_tile (x - m)^2 and its sum by |x| + |c| <= |x| + max_tile |x|."""
    f32 = dtype == DV_F32
    if f32 and L.f32_exact():
        pytest.skip('pre-split weights (DV_W3) do not exist under DUALVAR_F32_EXACT=1')
    lib = L.load()
    tdt = ops.TORCH_DTYPE[dtype]
    g = torch.Generator().manual_seed(21)
    N, T, H, W, Cin, widths = 8, 4, 14, 14, 64, (32, 24, 40)
    Cout = sum(widths)
    xin = ops.new_act(N, T, H, W, Cin, dtype, gpu)
    xin.buf.copy_((torch.randn(xin.buf.shape, generator=g) + 0.3).to(tdt))
    y = ops.new_act(N, T, H, W, Cout, dtype, gpu)
    d = ops.conv_desc(dtype, xin, y, (1, 1, 1), (1, 1, 1), (0, 0, 0), flags=DV_STATS | (DV_W3 if f32 else 0))
    w = (torch.randn(Cout, Cin, generator=g) / 8).to(gpu).to(tdt)
    tiles, tr = ops.stat_tiles(d), ops.tile_rows(d)
    part = torch.zeros(2, Cout, tiles, device=gpu)
    ops.conv_fwd(d, xin, ops.pack_w3(w) if f32 else w, None, y, part)
    torch.cuda.synchronize()
    M = y.rows
    assert tiles == ceil_div(M, tr)
    members, off = [], 0
    for k, C_ in enumerate(widths):
        xs = y.buf[:, off:off + C_].double()
        m = Member(gpu, dtype, M, C_, seed=90 + k, exact=False)
        m.x = View(dtype, M, C_, 0, C_, gpu, xs)               # (the stats phase reads partials only)
        m.part, m.coff, m.pitch, m.n_tiles, m.tile_rows = part, off, Cout, tiles, tr
        m.xs = xs
        members.append(m)
        off += C_
    local, _ = group_local(members, gpu)
    tab, ends = make_table(members, lib, gpu, dtype, stats_outputs=True)
    launch('dv_bn_stats_multi', tab.data_ptr(), len(members), 1, ends['stats'])
    torch.cuda.synchronize()
    for i, m in enumerate(members):
        xs = m.xs
        S = xs.sum(0)
        mean = S / M
        M2 = ((xs - mean) ** 2).sum(0)
        ps, pq, n = tile_partials(xs, tr)
        nn = n[:, None]
        xa = tile_partials(xs.abs(), tr)[0]                    # sum |x| per tile
        pad = torch.zeros(tiles * tr - M, m.C, dtype=torch.float64, device=gpu)
        xt = torch.cat([xs, pad]).view(tiles, tr, m.C)
        xmax = xt.abs().amax(1)                                # max |x| per tile (padding rows: 0)
        dev_max = torch.cat([xs - (ps / nn).repeat_interleave(tr, 0)[:M], pad]).view(tiles, tr, m.C).abs().amax(1)
        chain = stats_chain(tiles)
        dps = (tr + 3) * U * (xa + nn * xmax)                  # error of one tile sum
        dS = dps.sum(0) + chain * U * (ps.abs() + dps).sum(0)
        a = ps / nn
        dpq = (tr + 4) * U * (pq + 4 * nn * dev_max ** 2) + 8 * U * nn * (xa / nn + xmax) * dev_max
        dM2 = m2_bound(nn, dps / nn + U * a.abs(), a - mean, pq, dpq, dS / M + U * mean.abs(), chain)
        row = local[m.loff:m.loff + 2 * m.C + 1].double()
        assert float(row[2 * m.C]) == M
        check_bound(row[:m.C], S, dS, f'conv stats[{i}] S')
        check_bound(row[m.C:2 * m.C], M2, dM2, f'conv stats[{i}] M2')
        report(f'conv stats[{i}] S (L={tr}+{chain})', (row[:m.C] - S).abs(), xs.abs().sum(0))
        check_finalized(m, m.o, S, M2, M, dS, dM2, m.rm, m.rv, f'conv stats[{i}]')


def test_float64_reference_matches_autograd(gpu):
    """the reference formulas of this file (y, g, sum g, sum g*xhat, dx, dres, dgamma, dbeta) against
    torch.nn.functional.batch_norm + residual + ReLU under float64 autograd"""
    g = torch.Generator().manual_seed(3)
    M, C_ = 500, 13
    x = torch.randn(M, C_, generator=g, dtype=torch.float64) * 1.5 + 0.4
    res = torch.randn(M, C_, generator=g, dtype=torch.float64)
    dy = torch.randn(M, C_, generator=g, dtype=torch.float64)
    gamma = 1 + 0.3 * torch.randn(C_, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(C_, generator=g, dtype=torch.float64)
    rm0, rv0 = torch.randn(C_, generator=g, dtype=torch.float64), 1 + torch.rand(C_, generator=g, dtype=torch.float64)
    xr, rr = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    out = torch.relu(torch.nn.functional.batch_norm(xr, rm, rv, gr, br, training=True, momentum=MOM, eps=EPS) + rr)
    out.backward(dy)
    # this file's formulas
    mean = x.mean(0)
    M2 = ((x - mean) ** 2).sum(0)
    invstd = (M2 / M + EPS).rsqrt()
    scale = gamma * invstd
    shift = beta - mean * scale
    y = (x * scale + shift + res).clamp_min(0)
    assert torch.allclose(y, out.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(rm, (1 - MOM) * rm0 + MOM * mean, rtol=1e-12) and torch.allclose(rv, (1 - MOM) * rv0 + MOM * M2 / (M - 1))
    gg = dy * (y > 0).double()
    xhat = (x - mean) * invstd
    sg, sgx = gg.sum(0), (gg * xhat).sum(0)
    k1 = gamma * invstd
    k2 = -k1 * invstd * sgx / M
    k3 = -k1 * sg / M - k2 * mean
    dx = k1 * gg + k2 * x + k3
    assert torch.allclose(dx, xr.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(gg, rr.grad, rtol=0, atol=0)
    assert torch.allclose(sgx, gr.grad, rtol=1e-12, atol=1e-12) and torch.allclose(sg, br.grad, rtol=1e-12, atol=1e-12)
