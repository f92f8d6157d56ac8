#!/usr/bin/env python
"""Checks of the two-member launches of the LDS-staged conv kernel (csrc/conv_tap.hip: conv_tap_pair_kernel; the entries
dv_conv3d_fwd_pair / dv_conv3d_fwd_bn_in_pair / dv_conv3d_dgrad_pair and the query dv_conv3d_pair_ok) and of the plan pass that
uses them (engine.pair_convs, engine.PAIR_CONVS).  Run with DUALVAR_CONV_TAP_GRID=1, which forces small problems onto that kernel
(the variable is read once per process: tests/test_conv_pair_*.py start this script as a child).

    DUALVAR_CONV_TAP_GRID=1 python tools/pair_check.py ops       # op level: the pair entry against the two single entries
    DUALVAR_CONV_TAP_GRID=1 DUALVAR_CONV_TAP_BM128=0 python tools/pair_check.py ops      # ... on the 256-row tiles
    python tools/pair_check.py ks                                # op level, default thresholds: a conv_gemm_ks pair
    DUALVAR_CONV_TAP_GRID=1 python tools/pair_check.py plan      # one S3D-G SimCLR step with PAIR_CONVS off and on
    DUALVAR_CONV_TAP_GRID=1 python tools/pair_check.py host      # no GPU: the S3D-G plan's lists, paired against unpaired

Every comparison is torch.equal -- the pair runs the code and the operands of the single launches --, on whole buffers: outputs
are views into larger buffers with sentinel rows behind them."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualvar_amd import _lib as L          # noqa: E402
from dualvar_amd import ops                # noqa: E402

DT = L.DV_F32
SENTINEL = 12345.0
SP, TM = ((1, 3, 3), (0, 1, 1)), ((3, 1, 1), (1, 0, 0))


def cp16(c):
    return (c + 15) // 16 * 16


def view(rows, pitch, dev, N, T, H, W, C_, fill=None):
    """an activation that is a view into a larger buffer: 300 sentinel rows behind it; fill: a tensor for the rows, or zeros"""
    buf = torch.full((rows + 300, pitch), SENTINEL, dtype=torch.float32, device=dev)
    buf[:rows] = 0 if fill is None else fill
    return ops.Act(buf[:rows], N, T, H, W, C_, pitch, 0, DT, pitch), buf


class Member:
    """one conv problem with its operands: x, the packed weights of both directions, dY, and fresh outputs on request"""

    def __init__(self, dev, N, Ci, T, H, W, Co, form, seed):
        self.dev, self.dims, self.Ci, self.Co, (self.k, self.p) = dev, (N, T, H, W), Ci, Co, form
        g = torch.Generator().manual_seed(seed)
        taps = self.k[0] * self.k[1] * self.k[2]
        x = torch.randn(N, Ci, T, H, W, generator=g)
        w = torch.randn(Co, Ci, *self.k, generator=g) * (Ci * taps) ** -0.5
        gy = torch.randn(N, Co, T, H, W, generator=g)
        self.M = N * T * H * W
        self.x = ops.act_from_ncdhw(x.to(dev), DT, cpitch=cp16(Ci))
        self.x.buf[:, Ci:] = 777.0 if form is TM else 0.0       # (BatchNorm on load: pad lanes of its input must not reach the products)
        self.w3 = ops.pack_w3(ops.pack_weight(w.to(dev), self.x.cpitch).view(Co, -1))
        self.dy = ops.act_from_ncdhw(gy.to(dev), DT, cpitch=cp16(Co))
        wd = torch.zeros(Ci, taps, cp16(Co), device=dev)
        wd[:, :, :Co] = w.to(dev).reshape(Co, Ci, taps).permute(1, 2, 0)
        self.wd3 = ops.pack_w3(wd.view(Ci, -1))
        self.dx0 = torch.randn(self.M, self.x.cpitch, generator=g).to(dev)        # what a `+=` adds to
        CPi = ops.cp8(Ci)
        self.scale, self.shift = torch.zeros(CPi, device=dev), torch.zeros(CPi, device=dev)
        self.scale[:Ci] = (1 + 0.3 * torch.randn(Ci, generator=g)).to(dev)
        self.shift[:Ci] = (0.2 * torch.randn(Ci, generator=g)).to(dev)
        self.bn_in = ops.bn_in_desc(self.scale, self.shift, True)
        self.mean, self.invstd = (0.1 * torch.randn(CPi, generator=g)).to(dev), (1 + 0.1 * torch.rand(CPi, generator=g)).to(dev)
        self.bn_x = ops.act_from_ncdhw(torch.randn(N, Ci, T, H, W, generator=g).to(dev), DT, cpitch=self.x.cpitch)

    def fwd(self):
        """-> (descriptor, y, its whole buffer, BatchNorm partials)"""
        N, T, H, W = self.dims
        y, ybuf = view(self.M, ops.cp8(self.Co), self.dev, N, T, H, W, self.Co)
        d = ops.conv_desc(DT, self.x, y, self.k, (1, 1, 1), self.p, flags=L.DV_STATS | L.DV_W3)
        return d, y, ybuf, torch.full((2, self.Co, ops.stat_tiles(d)), SENTINEL, device=self.dev)

    def dgrad(self, accum):
        N, T, H, W = self.dims
        dx, dxbuf = view(self.M, self.x.cpitch, self.dev, N, T, H, W, self.Ci, self.dx0 if accum else None)
        return ops.conv_desc(DT, dx, self.dy, self.k, (1, 1, 1), self.p, flags=L.DV_W3 | (L.DV_ACCUM if accum else 0)), dx, dxbuf


def same(a, b, what):
    assert torch.equal(a, b), '%s: the pair differs from the single launches (max %g)' % (what, float((a - b).abs().max()))


def intact(buf, rows, what):
    assert bool((buf[rows:] == SENTINEL).all()), what + ': wrote behind the output'
    assert bool(torch.isfinite(buf[:rows]).all()) and float(buf[:rows].abs().max()) > 0, what + ': empty or non-finite output'


def check_fwd(lib, m0, m1, bn=(False, False), want=None, tag=''):
    """the forward pair entry against the single entries; want: what dv_conv3d_pair_ok must say (None: only 'not 0')"""
    s = ops.stream_ptr()
    single, pair = [mm.fwd() for mm in (m0, m1)], [mm.fwd() for mm in (m0, m1)]
    for mm, (d, y, _, st), b in zip((m0, m1), single, bn):
        (ops.conv_fwd_bn_in(d, mm.x, mm.bn_in, mm.w3, y, st) if b else ops.conv_fwd(d, mm.x, mm.w3, None, y, st))
    mode = (L.DV_PAIR_BN_IN0 if bn[0] else 0) | (L.DV_PAIR_BN_IN1 if bn[1] else 0)
    ok = int(lib.dv_conv3d_pair_ok(C.byref(pair[0][0]), C.byref(pair[1][0]), mode))
    (d0, y0, _, st0), (d1, y1, _, st1) = pair
    if any(bn):
        L.check(lib.dv_conv3d_fwd_bn_in_pair(C.byref(d0), m0.x.ptr, C.byref(m0.bn_in) if bn[0] else None, m0.w3.data_ptr(), y0.ptr,
                                             st0.data_ptr(), C.byref(d1), m1.x.ptr, C.byref(m1.bn_in) if bn[1] else None,
                                             m1.w3.data_ptr(), y1.ptr, st1.data_ptr(), s), 'dv_conv3d_fwd_bn_in_pair')
    else:
        L.check(lib.dv_conv3d_fwd_pair(C.byref(d0), m0.x.ptr, m0.w3.data_ptr(), y0.ptr, st0.data_ptr(),
                                       C.byref(d1), m1.x.ptr, m1.w3.data_ptr(), y1.ptr, st1.data_ptr(), s), 'dv_conv3d_fwd_pair')
    torch.cuda.synchronize()
    for i, (mm, a, b) in enumerate(zip((m0, m1), single, pair)):
        same(a[2], b[2], '%s forward, member %d' % (tag, i))
        same(a[3], b[3], '%s BatchNorm partials, member %d' % (tag, i))
        intact(b[2], mm.M, '%s forward, member %d' % (tag, i))
        assert not bool((b[3] == SENTINEL).any()), '%s: BatchNorm partials not all written' % tag
    assert (ok != 0) if want is None else (ok == want), (tag, 'dv_conv3d_pair_ok', ok, want)
    print('%-58s fwd%s pair_ok %d rows %d grids %d + %d' % (tag, ' +bn_in' if any(bn) else '', ok, ops.tile_rows(d0), grid(lib, d0, 0), grid(lib, d1, 0)), flush=True)
    return ok


def grid(lib, d, dgrad):
    rows = int(lib.dv_conv3d_tap_rows(C.byref(d), dgrad))
    if not rows:
        return 0
    m = d.N * (d.Ti * d.Hi * d.Wi if dgrad else d.To * d.Ho * d.Wo)
    return (m + rows - 1) // rows * (((d.cin_pitch if dgrad else d.cout_pitch) + 63) // 64)


def check_dgrad(lib, m0, m1, accum=(False, False), want=None, tag=''):
    s = ops.stream_ptr()
    single, pair = [mm.dgrad(a) for mm, a in zip((m0, m1), accum)], [mm.dgrad(a) for mm, a in zip((m0, m1), accum)]
    for mm, (d, dx, _) in zip((m0, m1), single):
        ops.conv_dgrad(d, mm.dy, mm.wd3, dx)
    (d0, dx0, _), (d1, dx1, _) = pair
    ok = int(lib.dv_conv3d_pair_ok(C.byref(d0), C.byref(d1), L.DV_PAIR_DGRAD))
    L.check(lib.dv_conv3d_dgrad_pair(C.byref(d0), m0.dy.ptr, m0.wd3.data_ptr(), dx0.ptr, None,
                                     C.byref(d1), m1.dy.ptr, m1.wd3.data_ptr(), dx1.ptr, None, None, 0, s), 'dv_conv3d_dgrad_pair')
    torch.cuda.synchronize()
    for i, (mm, a, b) in enumerate(zip((m0, m1), single, pair)):
        same(a[2], b[2], '%s data gradient, member %d' % (tag, i))
        intact(b[2], mm.M, '%s data gradient, member %d' % (tag, i))
    assert (ok != 0) if want is None else (ok == want), (tag, 'dv_conv3d_pair_ok', ok, want)
    print('%-58s dgrad accum %s pair_ok %d grids %d + %d' % (tag, accum, ok, grid(lib, d0, 1), grid(lib, d1, 1)), flush=True)
    return ok


def check_dgrad_with_fused_reduce(lib, m0, m1, tag):
    """member 0 carries the ordered fused BatchNorm-backward reduce: never in a shared grid, and the pair entry gives what
    dv_conv3d_dgrad_bn_ws + dv_conv3d_dgrad give -- dx and the sums"""
    s = ops.stream_ptr()
    (d0, a0, b0), (d1, a1, b1) = m0.dgrad(False), m1.dgrad(False)
    (_, p0, q0), (_, p1, q1) = m0.dgrad(False), m1.dgrad(False)
    need = int(lib.dv_conv3d_dgrad_bn_workspace(C.byref(d0)))
    assert need > 0, tag
    ws = torch.zeros(need // 4, device=m0.dev)
    sums = [torch.zeros(1, 2, ops.cp8(m0.Ci), device=m0.dev) for _ in range(2)]
    r = [ops.bn_reduce_desc(m0.bn_x, m0.mean, m0.invstd, m0.scale, m0.shift, t, 1, 0) for t in sums]
    L.check(lib.dv_conv3d_dgrad_bn_ws(C.byref(d0), m0.dy.ptr, m0.wd3.data_ptr(), a0.ptr, C.byref(r[0]), ws.data_ptr(), need, s), 'dv_conv3d_dgrad_bn_ws')
    ops.conv_dgrad(d1, m1.dy, m1.wd3, a1)
    ok = int(lib.dv_conv3d_pair_ok(C.byref(d0), C.byref(d1), L.DV_PAIR_DGRAD | L.DV_PAIR_BN_REDUCE0))
    L.check(lib.dv_conv3d_dgrad_pair(C.byref(d0), m0.dy.ptr, m0.wd3.data_ptr(), p0.ptr, C.byref(r[1]),
                                     C.byref(d1), m1.dy.ptr, m1.wd3.data_ptr(), p1.ptr, None, ws.data_ptr(), need, s), 'dv_conv3d_dgrad_pair')
    torch.cuda.synchronize()
    same(b0, q0, tag + ' data gradient, member 0')
    same(b1, q1, tag + ' data gradient, member 1')
    same(sums[0], sums[1], tag + ' fused BatchNorm-backward sums')
    intact(q0, m0.M, tag)
    assert float(sums[1].abs().max()) > 0 and ok == 0, (tag, ok)
    print('%-58s dgrad +bn_reduce on member 0: pair_ok %d' % (tag, ok), flush=True)


def ops_main():
    L.require_device()
    dev = torch.device('cuda:0')
    lib = L.load()
    bm128 = os.environ.get('DUALVAR_CONV_TAP_BM128', '1') != '0'
    # spatial 1x3x3: 2 clips of 2 x 7 x 7 (M = 196: two 128-row tiles, the last with 68 rows); the 256-row form on 3 clips (256 + 38)
    n = 2 if bm128 else 3
    small, big = Member(dev, n, 16, 2, 7, 7, 48, SP, 1), Member(dev, n, 96, 2, 7, 7, 208, SP, 2)
    d_small = small.fwd()[0]
    assert int(lib.dv_conv3d_tap_kind(C.byref(d_small), 0)) == 1 and ops.tile_rows(d_small) == (128 if bm128 else 256)
    for m0, m1 in ((small, big), (big, small)):                     # blocks of member 0: 2 and 8 (128-row tiles)
        tag = 'spatial Cin%d->%d | Cin%d->%d' % (m0.Ci, m0.Co, m1.Ci, m1.Co)
        assert check_fwd(lib, m0, m1, tag=tag) == 1
        assert check_dgrad(lib, m0, m1, tag=tag) == 1
    assert check_dgrad(lib, small, big, accum=(False, True), tag='spatial, += on the second member') == 1
    if bm128:
        assert grid(lib, d_small, 0) == 2 and grid(lib, big.fwd()[0], 0) == 8
    if not bm128:
        print('ok')
        return
    # temporal 3x1x1 with BatchNorm on load: C = 48 and 208 (coefficient tables of different sizes: the LDS of the launch is the
    # larger member's), T = 2 and T = 4; plain forward and both data-gradient forms as well
    t = {}
    for T in (2, 4):
        a, b = Member(dev, 2, 48, T, 7, 7, 48, TM, 3 + T), Member(dev, 2, 208, T, 7, 7, 208, TM, 4 + T)
        t[T] = (a, b)
        m0, m1 = (a, b) if T == 2 else (b, a)
        tag = 'temporal T%d C%d | C%d' % (T, m0.Ci, m1.Ci)
        assert check_fwd(lib, m0, m1, bn=(True, True), tag=tag) == 2
        assert check_fwd(lib, m0, m1, tag=tag) == 2
        assert check_dgrad(lib, m0, m1, tag=tag) == 2
        assert check_dgrad(lib, m0, m1, accum=(True, False), tag=tag + ', += on the first member') == 2
    # pairs that must be refused: the query says 0 and the entry still gives the single launches' bits
    tm48, tm208 = t[2]
    check_fwd(lib, small, tm48, want=0, tag='refused: spatial with temporal')
    check_dgrad(lib, small, tm48, want=0, tag='refused: spatial with temporal')
    check_fwd(lib, tm48, tm208, bn=(True, False), want=0, tag='refused: BatchNorm on load with plain')
    check_fwd(lib, tm208, tm48, bn=(False, True), want=0, tag='refused: plain with BatchNorm on load')
    t8 = Member(dev, 2, 48, 8, 7, 7, 48, TM, 11)                  # eight-frame temporal tiles stay 256 rows high
    assert ops.tile_rows(t8.fwd()[0]) == 256 and ops.tile_rows(tm48.fwd()[0]) == 128
    check_fwd(lib, tm48, t8, want=0, tag='refused: 128- with 256-row tiles')
    check_dgrad(lib, t8, tm48, want=0, tag='refused: 256- with 128-row tiles')
    check_dgrad_with_fused_reduce(lib, big, small, 'refused: a member with the fused BatchNorm reduce')
    print('ok')


def ks_main():
    """the spatial branch convs of Mixed_5b (Cin32 -> Cout128, Cin160 -> Cout320) on conv_gemm_ks_kernel (default thresholds: they
    are too small for the LDS-staged kernel), at the smallest number of 1 x 7 x 7 clips at which dv_conv3d_ksplit_cols says that
    both members run there, forward and data gradient, with the same column tile"""
    L.require_device()
    dev = torch.device('cuda:0')
    lib = L.load()
    for n in range(2, 40):
        small, big = Member(dev, n, 32, 1, 7, 7, 128, SP, 21), Member(dev, n, 160, 1, 7, 7, 320, SP, 22)
        cols = [int(lib.dv_conv3d_ksplit_cols(C.byref(d), dg)) for m in (small, big) for dg, d in ((0, m.fwd()[0]), (1, m.dgrad(False)[0]))]
        if all(cols) and cols[0] == cols[2] and cols[1] == cols[3]:
            break
    else:
        raise AssertionError('no size at which both members run on conv_gemm_ks')
    assert all(int(lib.dv_conv3d_tap_kind(C.byref(m.fwd()[0]), 0)) == 0 for m in (small, big))
    print('conv_gemm_ks: %d clips, M = %d, column tiles (fwd, dgrad) x (small, big): %s' % (n, small.M, cols), flush=True)
    for m0, m1 in ((small, big), (big, small)):
        tag = 'ks spatial Cin%d->%d | Cin%d->%d' % (m0.Ci, m0.Co, m1.Ci, m1.Co)
        assert check_fwd(lib, m0, m1, want=L.DV_PAIR_KS, tag=tag) == L.DV_PAIR_KS
        assert check_dgrad(lib, m0, m1, want=L.DV_PAIR_KS, tag=tag) == L.DV_PAIR_KS
    assert check_dgrad(lib, small, big, accum=(True, False), want=L.DV_PAIR_KS, tag='ks spatial, += on the first member') == L.DV_PAIR_KS
    # a member on another kernel: refused, and still the single launches' bits
    tm = Member(dev, n, 32, 1, 7, 7, 128, TM, 23)
    if int(lib.dv_conv3d_ksplit_cols(C.byref(tm.fwd()[0]), 0)) != cols[0]:
        check_fwd(lib, small, tm, want=0, tag='refused: conv_gemm_ks with another kernel or column tile')
    print('ok')


# --------------------------------------------------------------------------------------------------------------- plan level
def _key(l):
    return (l.name, l.kname, getattr(l, 'shape', ''), l.bytes, l.flops, getattr(l, 'gend', 0))


def expand(lst, side):
    """a paired list with every pair taken apart again: the first member at the pair's position, the second behind the side-stream
    launches that follow -- where it stood before the pass"""
    out, held = [], None
    for l in lst:
        if held is not None and l.name not in side:
            out.append(held)
            held = None
        if getattr(l, 'members', ()):
            out.append(l.members[0])
            held = l.members[1]
        else:
            out.append(l)
    return out + ([held] if held is not None else [])


def pair_counts(plans):
    n = dict(fwd_sp=0, fwd_tm_bn_in=0, dgrad_sp=0, dgrad_tm=0, fwd_ks=0, dgrad_ks=0, other=0)
    for pl in plans:
        for l in pl.f_list + pl.b_list:
            if not getattr(l, 'members', ()):
                continue
            assert l.kname.endswith('+pair') and l.kname.startswith(('conv_tap<f32,', 'conv_gemm_ks<f32,')), l.kname
            form = 'ks' if l.kname.startswith('conv_gemm_ks') else 'sp' if ',sp,' in l.kname else 'tm'
            key = {('conv_fwd', 'sp', False): 'fwd_sp', ('conv_fwd', 'tm', True): 'fwd_tm_bn_in', ('conv_dgrad', 'sp', False): 'dgrad_sp',
                   ('conv_dgrad', 'tm', False): 'dgrad_tm', ('conv_fwd', 'ks', False): 'fwd_ks',
                   ('conv_dgrad', 'ks', False): 'dgrad_ks'}.get((l.name, form, '+bn_in' in l.kname), 'other')
            n[key] += 1
    return n


def plan_main():
    """one S3D-G SimCLR training step (4 samples x 2 views of 8 x 112 x 112, fp32) with PAIR_CONVS off, then on (two passes
    through the same plan): loss and every gradient bit for bit"""
    from dualvar_amd import engine, model as M
    L.require_device()
    dev = torch.device('cuda:0')
    block = torch.randn(4, 2, 3, 8, 112, 112, generator=torch.Generator().manual_seed(3)).to(dev)
    res = {}
    for on in (False, True):
        engine.PAIR_CONVS = on
        torch.manual_seed(0)
        m = M.SimCLR_Naked('s3dg', 128, 0.07, False)
        m.set_compute_dtype('fp32').train().to(dev)
        passes = []
        for _ in range(2 if on else 1):
            ret = m(block)
            for st in m.stores():
                st.zero_grad()
            ret['clip_contrast_loss'].backward()
            torch.cuda.synchronize()
            passes.append((ret['clip_contrast_loss'].detach().clone(),
                           torch.cat([st.grad.detach().float().flatten().clone() for st in m.stores()])))
        plans = [pl for mod in m.modules() if hasattr(mod, '_plans') for lst in mod._plans.values() for pl in lst]
        res[on] = (passes, pair_counts(plans), sum(len(pl.f_list) + len(pl.b_list) for pl in plans))
    (off,), (on1, on2) = res[False][0], res[True][0]
    out = dict(loss=float(on1[0]), loss_equal=bool(torch.equal(off[0], on1[0])), grads_equal=bool(torch.equal(off[1], on1[1])),
               second_pass_equal=bool(torch.equal(on1[0], on2[0]) and torch.equal(on1[1], on2[1])),
               finite=bool(torch.isfinite(on1[1]).all()) and float(on1[1].abs().max()) > 0,
               max_grad_diff=float((off[1] - on1[1]).abs().max()),
               pairs_off=res[False][1], pairs_on=res[True][1], launches_off=res[False][2], launches_on=res[True][2])
    print('RESULT ' + json.dumps(out))


def _region(ptr, rows, ld, width):
    """the byte intervals [start, end) of `rows` rows of `width` floats at pitch `ld` floats"""
    start = ptr + np.arange(rows, dtype=np.int64) * (ld * 4)
    return start, start + width * 4


def _overlap(a, b):
    i = np.searchsorted(b[0], a[1], side='left')         # first interval of b that starts at or after a's end
    prev = np.clip(i - 1, 0, len(b[0]) - 1)
    return bool(np.any((i > 0) & (b[1][prev] > a[0])))


def member_regions(l):
    """(read regions, write regions) of a member launch, from the raw pointers and the descriptor it will be called with"""
    m = l.pair
    d = m.desc
    rows_x, rows_y = d.N * d.Ti * d.Hi * d.Wi, d.N * d.To * d.Ho * d.Wo
    if m.role == 'dgrad':
        _, dy, _, dx, _ = m.args
        rd = [_region(dy, rows_y, d.ldy, d.cout_pitch)]
        wr = [_region(dx, rows_x, d.ldx, d.cin_pitch)]
        if d.flags & L.DV_ACCUM:
            rd.append(wr[0])
        return rd, wr
    x, y, stats = (m.args[1], m.args[4], m.args[5]) if m.role == 'fwd_bn_in' else (m.args[1], m.args[3], m.args[4])
    wr = [_region(y, rows_y, d.ldy, d.cout_pitch)]
    if stats:
        wr.append(_region(stats, 1, 0, 2 * d.Cout * int(L.load().dv_conv3d_stat_tiles(C.byref(d)))))
    return [_region(x, rows_x, d.ldx, d.cin_pitch)], wr


def host_main():
    """No GPU: the fp32 training plan of S3D-G at 8 clips, built on the CPU with the pass on and off.  The paired lists taken apart
    again are the unpaired lists; cost and the early-release decision do not move; no member of a pair reads or writes a byte
    the other writes (from the raw pointers the launches carry, not from the pass's own bookkeeping)."""
    from dualvar_amd import engine
    from dualvar_amd.backbone.select_backbone import select_backbone
    torch.manual_seed(0)
    m = select_backbone('s3dg')[0]
    m.set_compute_dtype('fp32')
    m.train(True)
    m.store.materialize(torch.device('cpu'), m.dtype)
    plans = {}
    for on in (False, True):
        engine.PAIR_CONVS = on
        m._plans.clear()
        plans[on] = m._acquire_plan(torch.empty(8, 3, 8, 112, 112), False, False, True)
    off, on = plans[False], plans[True]
    side = engine.SIDE_LAUNCHES
    checked = 0
    for l in on.f_list + on.b_list:
        if getattr(l, 'members', ()):
            (r0, w0), (r1, w1) = member_regions(l.members[0]), member_regions(l.members[1])
            clash = any(_overlap(a, b) or _overlap(b, a) for a in w0 for b in r1 + w1) or any(_overlap(a, b) or _overlap(b, a) for a in w1 for b in r0)
            assert not clash, l.shape
            assert l.bytes == sum(x.bytes for x in l.members) and l.flops == sum(x.flops for x in l.members)
            checked += 1
    out = dict(f_equal=[_key(l) for l in expand(on.f_list, ())] == [_key(l) for l in off.f_list],
               b_equal=[_key(l) for l in expand(on.b_list, side)] == [_key(l) for l in off.b_list],
               off_has_pairs=any(getattr(l, 'members', ()) for l in off.f_list + off.b_list),
               cost_equal=off.cost() == on.cost(), wgrad_early=[off.wgrad_early, on.wgrad_early],
               pairs=pair_counts([on]), members_checked=checked,
               side_order_equal=[_key(l) for l in on.b_list if l.name in side] == [_key(l) for l in off.b_list if l.name in side])
    print('RESULT ' + json.dumps(out))


if __name__ == '__main__':
    {'ops': ops_main, 'ks': ks_main, 'plan': plan_main, 'host': host_main}[sys.argv[1] if len(sys.argv) > 1 else 'ops']()
