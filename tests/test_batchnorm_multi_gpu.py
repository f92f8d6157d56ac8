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
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib as L, ops  # noqa: E402
from dualvar_amd._lib import DV_F32, DV_STATS, DV_W3  # noqa: E402
from tests.bn_support import (DTYPES, EPS, JUNK, MOM, Member, assert_exact_data_fits, backward_terms, check_apply,  # noqa: E402
                              check_bound, check_bwd_apply, check_finalized, check_local, check_reduce, check_ticket_area,
                              group_local, make_table, n_blocks, reference_y, report, stats_reference, tile_partials)
from tests.chains import bwd_reduce_chain, m2_bound, stats_chain  # noqa: E402
from tests.checks import U, View, bits, ceil_div, is_sent, launch, sent  # noqa: E402


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
            assert is_sent(local[m.loff:m.loff + 2 * m.C + 1]) and all(is_sent(t) for t in m.o.values())
            assert torch.equal(m.rm[:m.C], m.rm0) and torch.equal(m.rv[:m.C], m.rv0), f'{w}: zero-block member written'
            continue
        S, M2, dS, dM2, sabs = stats_reference(m)
        check_local(m, local, S, M2, dS, dM2, sabs, w)
        assert all(is_sent(t[m.C:]) for t in m.o.values()), f'{w}: stats outputs past C'
        check_finalized(m, m.o, S, M2, m.M, dS, dM2, m.rm, m.rv, w)

    tab, ends = make_table(members, lib, dev, dtype)
    if ends['apply']:
        launch('dv_bn_apply_multi', dtype, tab.data_ptr(), n, ends['apply'])
    torch.cuda.synchronize()
    y_in = []
    for i, m in enumerate(members):
        if 'apply' in m.zero:
            assert m.y.untouched(), f'{what}[{i}]: y of a zero-block member written'
            m.y.set(reference_y(m), pad=None)                  # the backward's input
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
            assert all(is_sent(s) for s in m.sums) and bool((m.red_ws == 0).all()), f'{w}: zero-block reduce wrote'
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
    gathered = sent((3 * width,), gpu).view(3, width)
    for r, mem in enumerate(ranks):
        group_local(mem, gpu)
        rows = [gathered[r].data_ptr() + 4 * m.loff for m in mem]
        tab, ends = make_table(mem, lib, gpu, dtype, stats_outputs=True, rank_local=rows)
        launch('dv_bn_stats_multi', tab.data_ptr(), len(mem), 0, ends['stats'])
    torch.cuda.synchronize()
    for r, mem in enumerate(ranks):
        for m in mem:
            assert all(is_sent(t) for t in m.o.values()), 'finalize = 0 wrote the affine map'
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
    bf16 about a provisional centre c, one of the tile's values (conv_gemm.hpp), merged with Chan's formula: its terms are
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
        m.x = View(dtype, M, C_, 0, C_, gpu, xs, pad=JUNK)               # (the stats phase reads partials only)
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
