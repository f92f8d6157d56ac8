"""CPU: the pass that puts two conv launches into one grid (engine.pair_convs behind engine.PAIR_CONVS) and its query
dv_conv3d_pair_ok.  On stub launches over small CPU activations: dependent or aliasing members never pair, side-stream launches
between the members keep their order, only neighbours pair.  Then on the real S3D-G plan built on the CPU (tools/pair_check.py
host, a child process because DUALVAR_CONV_TAP_GRID is read once per process): the paired lists taken apart are the unpaired ones."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import torch

from dualvar_amd import _lib as L, engine, ops
from dualvar_amd.ops import DV_F32
from tests import abi_coverage as A
from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The coverage ledger of include/dualvar_conv_pair.h, in the form and with the kinds of tests/abi_coverage.py: every entry of
# _lib.PAIR_SIGNATURES -> (the test file of its strongest reference test, the kind of reference).  The entries are exercised
# through tools/pair_check.py, which those test files start.
PAIR_COVERAGE = {
    'dv_conv3d_pair_ok': ('test_conv_pair_host.py', A.HOST_QUERY),
    'dv_conv3d_fwd_pair': ('test_conv_pair_gpu.py', A.BIT_EQUAL_TESTED),
    'dv_conv3d_fwd_bn_in_pair': ('test_conv_pair_gpu.py', A.BIT_EQUAL_TESTED),
    'dv_conv3d_dgrad_pair': ('test_conv_pair_gpu.py', A.BIT_EQUAL_TESTED),
}


def test_pair_header_table_and_library_agree():
    """include/dualvar_conv_pair.h, its ctypes table _lib.PAIR_SIGNATURES, the library's exports and PAIR_COVERAGE name the same
    entries with the same argument counts and return widths; the table shares no name with the other headers' tables; the
    DV_PAIR_* constants are the header's; every entry is named by the test file that holds its reference test and called by the
    checking tool behind it."""
    hdr, decl = check_header_binding('dualvar_conv_pair.h')
    assert set(decl) == set(L.PAIR_SIGNATURES) == set(PAIR_COVERAGE) and len(decl) == 4
    assert all(ret == 'int' for ret, _ in decl.values())
    src = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    enums = dict(re.findall(r'(DV_PAIR_\w+)\s*=\s*(\d+)', src))
    assert {k: int(v) for k, v in enums.items()} == {k: getattr(L, k) for k in (
        'DV_PAIR_DGRAD', 'DV_PAIR_BN_IN0', 'DV_PAIR_BN_IN1', 'DV_PAIR_BN_REDUCE0', 'DV_PAIR_BN_REDUCE1', 'DV_PAIR_KS')}
    tool = open(os.path.join(ROOT, 'tools', 'pair_check.py')).read()
    for name, (fname, kind) in PAIR_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        assert re.search(r'\b%s\b' % name, open(os.path.join(ROOT, 'tests', fname)).read()), '%s is not mentioned in tests/%s' % (name, fname)
        assert re.search(r'lib\.%s\(' % name, tool), '%s is not called by tools/pair_check.py' % name


def _act(C_=16, grad=True):
    a = ops.new_act(1, 1, 2, 2, C_, DV_F32, 'cpu')
    if grad:
        a.grad = ops.new_act(1, 1, 2, 2, C_, DV_F32, 'cpu', zero=True)
    return a


class StubLib:
    """says yes to every pair and names the three entries"""
    dv_conv3d_fwd_pair, dv_conv3d_fwd_bn_in_pair, dv_conv3d_dgrad_pair = 'fwd_pair', 'fwd_bn_in_pair', 'dgrad_pair'

    def __init__(self, ok=1):
        self.ok, self.asked = ok, 0

    def dv_conv3d_pair_ok(self, d0, d1, mode):
        self.asked += 1
        return self.ok


def _launch(name, role, reads, writes, tag, nbytes=10, flops=100, gend=0):
    l = engine.Launch(name, 'conv_tap<f32,X,sp,128,64>', None, (), nbytes, flops, tag)
    l.gend = gend
    if role is not None:
        l.pair = engine.PairMember(role, L.ConvDesc(), (tag,), reads, writes)
    return l


def _fwd(x, y, tag, stats=None):
    return _launch('conv_fwd', 'fwd', [x], [y, stats], tag)


def _dgrad(dy, dx, tag, acc=False):
    return _launch('conv_dgrad', 'dgrad', [dy] + ([dx] if acc else []), [dx], tag)


def _shapes(lst):
    return [l.shape for l in lst]


def test_independent_neighbours_pair_and_carry_the_sums():
    cat = _act(32)
    a = _fwd(_act(), cat.slice(0, 16), 'a', torch.zeros(8))
    b = _fwd(_act(), cat.slice(16, 16), 'b', torch.zeros(8))          # the other channel slice of the same concat buffer
    a.gend, b.gend = 3, 7
    lib = StubLib()
    out = engine.pair_convs([a, b], lib)
    assert len(out) == 1 and out[0].members == (a, b) and out[0].pair is None
    p = out[0]
    assert (p.name, p.kname, p.fn, p.args) == ('conv_fwd', 'conv_tap<f32,X,sp,128,64>+pair', 'fwd_pair', ('a', 'b'))
    assert (p.bytes, p.flops, p.shape, p.gend) == (20, 200, 'a | b', 7)
    # the data gradient's entry takes the (unused) workspace of the fused reduce behind the members
    da, db = _dgrad(_act(), _act(), 'da'), _dgrad(_act(), _act(), 'db')
    p = engine.pair_convs([da, db], lib)[0]
    assert (p.fn, p.args) == ('dgrad_pair', ('da', 'db', 0, 0))


def test_dependent_members_never_pair():
    lib = StubLib()
    x, mid, y = _act(), _act(), _act()
    chain = [_fwd(x, mid, 'first'), _fwd(mid, y, 'second')]                 # the second reads what the first writes
    assert engine.pair_convs(chain, lib) == chain
    cat = _act(32)
    sliced = [_fwd(x, cat.slice(0, 16), 'writes a slice'), _fwd(cat.slice(16, 16), y, 'reads another slice of that buffer')]
    assert engine.pair_convs(sliced, lib) == sliced                          # (conservative: any slice, as PlanGraph counts reads)
    same_out = [_fwd(_act(), y, 'one'), _fwd(_act(), y, 'other')]
    assert engine.pair_convs(same_out, lib) == same_out
    overlapping = [_fwd(_act(), cat.slice(0, 24), 'cols 0-24'), _fwd(_act(), cat.slice(16, 16), 'cols 16-32')]
    assert engine.pair_convs(overlapping, lib) == overlapping
    st = torch.zeros(16)
    shared_stats = [_fwd(_act(), _act(), 's0', st[:8]), _fwd(_act(), _act(), 's1', st[8:])]
    assert len(engine.pair_convs(shared_stats, lib)) == 1                   # disjoint halves of one statistics buffer
    shared_stats = [_fwd(_act(), _act(), 's0', st[:8]), _fwd(_act(), _act(), 's1', st[4:12])]
    assert engine.pair_convs(shared_stats, lib) == shared_stats
    # the pointwise convs of a block write the block input's gradient with `=` and `+=`: one target, never one grid
    gx = _act()
    accum = [_dgrad(_act(), gx, 'writes ='), _dgrad(_act(), gx, 'adds +=', acc=True)]
    assert engine.pair_convs(accum, lib) == accum
    gcat = _act(32)
    accum = [_dgrad(_act(), gcat.slice(0, 16), '= into one slice'), _dgrad(_act(), gcat.slice(16, 16), '+= into the other', acc=True)]
    assert engine.pair_convs(accum, lib) == accum                            # (an accumulating member reads its target's buffer)
    assert lib.asked == 1                                                    # the library is asked about independent members only
    plain = [_dgrad(_act(), gcat.slice(0, 16), '='), _dgrad(_act(), gcat.slice(16, 16), '= too')]
    assert len(engine.pair_convs(plain, lib)) == 1


def test_only_like_neighbours_pair_and_the_library_decides():
    a, b, c = (_fwd(_act(), _act(), t) for t in 'abc')
    assert engine.pair_convs([a, b], StubLib(0)) == [a, b]                   # dv_conv3d_pair_ok said 0
    out = engine.pair_convs([a, b, c], StubLib())
    assert [l.members for l in out] == [(a, b), ()] and out[1] is c          # two members, no more
    other = _launch('bn_apply', None, [], [], 'bn')
    assert engine.pair_convs([a, other, b], StubLib()) == [a, other, b]      # not neighbours
    d = _dgrad(_act(), _act(), 'd')
    assert engine.pair_convs([a, d], StubLib()) == [a, d]                    # a forward and a data gradient
    bn = _launch('conv_fwd', 'fwd_bn_in', [_act()], [_act()], 'bn_in')
    assert engine.pair_convs([a, bn], StubLib()) == [a, bn]                  # plain with BatchNorm on load
    fused = _launch('conv_fwd', None, [_act()], [_act()], 'no member')       # (fp8, fused reduce: the launch offers no member)
    assert engine.pair_convs([a, fused, b], StubLib()) == [a, fused, b]


def test_side_stream_launches_between_the_members_keep_their_order():
    side = engine.SIDE_LAUNCHES
    w = [_launch('conv_wgrad', None, [], [], 'w%d' % i, gend=10 * i) for i in range(3)]
    gdb = _launch('gate_db', None, [], [], 'gate_db', gend=5)
    d0, d1, d2 = (_dgrad(_act(), _act(), 'd%d' % i) for i in range(3))
    head = _launch('bn_bwd_apply_multi', None, [], [], 'apply')
    out = engine.pair_convs([head, w[0], d0, w[1], gdb, d1, w[2], d2], StubLib(), side)
    assert _shapes(out) == ['apply', 'w0', 'd0 | d1', 'w1', 'gate_db', 'w2', 'd2']       # the pair stands where the earlier member stood
    assert [l.gend for l in out] == [0, 0, 0, 10, 5, 20, 0] and out[2].members == (d0, d1)
    # without the side-stream names the members are not neighbours; a main-stream launch between them always separates them
    assert len(engine.pair_convs([d0, w[1], d1], StubLib())) == 3
    assert len(engine.pair_convs([d0, w[1], head, d1], StubLib(), side)) == 4
    pad = _launch('stem_pad_taps', None, [], [], 'pad')
    assert len(engine.pair_convs([d0, w[1], pad, d1], StubLib(), side)) == 4


def test_query_refuses_what_cannot_share_a_grid():
    """dv_conv3d_pair_ok without a GPU, default thresholds: the 12 544-row branch convs of Mixed_4b pair (spatial 1, temporal 2 --
    with BatchNorm on load on both or on neither), everything else is 0"""
    lib = L.load()

    def desc(Ci, Co, k, p, N=16, T=4, H=14, flags=L.DV_W3, s=(1, 1, 1), cip=None):
        cip = (Ci + 15) // 16 * 16 if cip is None else cip
        x = SimpleNamespace(N=N, T=T, H=H, W=H, C=Ci, ld=cip, cpitch=cip)
        To, Ho, Wo = ops.conv_out_dims(x, k, s, p)
        y = SimpleNamespace(N=N, T=To, H=Ho, W=Wo, C=Co, ld=(Co + 15) // 16 * 16, cpitch=(Co + 15) // 16 * 16)
        return ops.conv_desc(DV_F32, x, y, k, s, p, flags=flags)

    def ok(d0, d1, mode=0):
        return int(lib.dv_conv3d_pair_ok(C.byref(d0), C.byref(d1), mode))
    sp, tm = ((1, 3, 3), (0, 1, 1)), ((3, 1, 1), (1, 0, 0))
    if os.environ.get('DUALVAR_F32_EXACT', '0') not in ('', '0') or any(
            os.environ.get(k) for k in ('DUALVAR_CONV_TAP', 'DUALVAR_CONV_TAP_GRID', 'DUALVAR_CONV_TAP_BM128', 'DUALVAR_CONV_TAP_BM128_GRID')):
        return          # (the routes below are those of the default thresholds)
    big, small = desc(96, 208, *sp), desc(16, 48, *sp)
    tbig, tsmall = desc(208, 208, *tm), desc(48, 48, *tm)
    both_bn = L.DV_PAIR_BN_IN0 | L.DV_PAIR_BN_IN1
    for dg in (0, L.DV_PAIR_DGRAD):
        assert ok(big, small, dg) == ok(small, big, dg) == 1 and ok(tbig, tsmall, dg) == 2
        assert ok(big, tsmall, dg) == 0 and ok(tsmall, big, dg) == 0                                 # spatial with temporal
        assert ok(big, desc(208, 208, *sp, N=64), dg) == 0                                          # 128- with 256-row tiles
        assert ok(big, desc(24, 64, *sp, cip=24), dg) == (0 if dg == 0 else 1)       # Mixed_4c's 24-channel branch: its forward runs on conv_gemm
        assert ok(big, desc(16, 48, *sp, flags=0), dg) == 0                                          # no pre-split weights: conv_gemm
        assert ok(big, desc(16, 48, *sp, N=1), dg) == 0                                              # too small for the kernel
    assert ok(tbig, tsmall, both_bn) == 2
    assert ok(tbig, tsmall, L.DV_PAIR_BN_IN0) == 0 and ok(tbig, tsmall, L.DV_PAIR_BN_IN1) == 0      # BatchNorm on load with plain
    assert ok(big, small, both_bn) == 0                                                             # (the spatial form has none)
    assert ok(tbig, tsmall, L.DV_PAIR_DGRAD | L.DV_PAIR_BN_IN0) == 0
    assert ok(big, small, L.DV_PAIR_DGRAD | L.DV_PAIR_BN_REDUCE0) == 0 and ok(big, small, L.DV_PAIR_DGRAD | L.DV_PAIR_BN_REDUCE1) == 0
    stem = desc(64, 64, (7, 1, 1), (3, 0, 0), N=16, T=8, H=56, s=(2, 1, 1))
    assert int(lib.dv_conv3d_tap_kind(C.byref(stem), 1)) == 2 and ok(stem, stem, L.DV_PAIR_DGRAD) == 0      # parity-class launches
    # the 1 152-row levels: both spatial members on conv_gemm_ks<64,32>
    kbig, ksmall = desc(160, 320, *sp, T=2, H=6), desc(32, 128, *sp, T=2, H=6)
    for dg in (0, L.DV_PAIR_DGRAD):
        assert int(lib.dv_conv3d_ksplit_cols(C.byref(kbig), dg)) == int(lib.dv_conv3d_ksplit_cols(C.byref(ksmall), dg)) == 32
        assert ok(kbig, ksmall, dg) == ok(ksmall, kbig, dg) == L.DV_PAIR_KS == 4
        assert ok(kbig, small, dg) == 0 and ok(big, ksmall, dg) == 0                                 # conv_gemm_ks with conv_tap
    assert ok(kbig, ksmall, both_bn) == 0                                                           # (no BatchNorm on load there)
    assert lib.dv_conv3d_pair_ok(None, C.byref(big), 0) == 0 and lib.dv_conv3d_pair_ok(C.byref(big), None, 0) == 0
    bad = desc(96, 208, *sp)
    bad.N = 0
    assert ok(big, bad) == 0


def test_pair_entries_validate_both_members_without_gpu():
    """both members are checked before anything is launched: a bad second member fails the call (no launch has happened: this
    process has no GPU context)"""
    lib = L.load()
    x = SimpleNamespace(N=16, T=4, H=14, W=14, C=16, ld=16, cpitch=16)
    y = SimpleNamespace(N=16, T=4, H=14, W=14, C=48, ld=48, cpitch=48)
    d = ops.conv_desc(DV_F32, x, y, (1, 3, 3), (1, 1, 1), (0, 1, 1), flags=L.DV_W3)
    assert lib.dv_conv3d_fwd_pair(C.byref(d), 64, 64, 64, None, C.byref(d), None, 64, 64, None, None) == -1          # DV_EINVAL
    assert lib.dv_conv3d_fwd_pair(C.byref(d), 64, 64, 64, None, C.byref(d), 64, 64, 68, None, None) == -2            # DV_EALIGN
    assert lib.dv_conv3d_fwd_pair(C.byref(d), 64, 64, 64, None, None, 64, 64, 64, None, None) != 0
    assert lib.dv_conv3d_dgrad_pair(C.byref(d), 64, 64, 64, None, C.byref(d), 64, None, 64, None, None, 0, None) == -1
    r = L.BnReduce()
    assert lib.dv_conv3d_dgrad_pair(C.byref(d), 64, 64, 64, C.byref(r), C.byref(d), 64, 64, 64, None, None, 0, None) == -1      # no workspace


def test_paired_s3dg_plan_taken_apart_is_the_unpaired_plan():
    """The fp32 training plan of S3D-G (8 clips of 8 x 112 x 112, built on the CPU) with engine.PAIR_CONVS on and off: with the
    switch off no launch is paired; the paired lists with every pair taken apart -- the second member back behind the side-stream
    launches that follow the pair -- equal the unpaired lists entry for entry (name, kernel, shape, bytes, flops, gradient-arena
    end), so the algorithmic totals and the early-release decision do not move; and for every pair, from the raw pointers its
    members carry, neither member reads or writes a byte the other writes."""
    env = dict(os.environ, DUALVAR_CONV_TAP_GRID='1')
    for k in ('DUALVAR_PAIR_CONVS', 'DUALVAR_F32_EXACT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pair_check.py'), 'host'], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    assert got['f_equal'] and got['b_equal'] and got['side_order_equal'] and got['cost_equal'] and not got['off_has_pairs'], got
    assert got['wgrad_early'][0] == got['wgrad_early'][1], got
    assert got['pairs'] == dict(fwd_sp=7, fwd_tm_bn_in=7, dgrad_sp=9, dgrad_tm=7, fwd_ks=7, dgrad_ks=0, other=0), got
    assert got['members_checked'] == 37, got
