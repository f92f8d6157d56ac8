"""dv_lars_norms / dv_lars_step (csrc/optim.hip) and dualvar_amd.optim.LARS against float64.

The two entries compute (include/dualvar_hip.h), per element with ONE fp32 rounding per operation and no FMA contraction:

    a1 = g gs;   d = DECAY ? a1 + wd p : a1                                  [a2 = wd p]
    per segment:  Sp = sum p^2,  Sd = sum d^2,  q = ADAPT && Sp > 0 && Sd > 0 ? eta sqrt(Sp) / sqrt(Sd) : 1
    t = q d;   x = mu buf;   buf' = x + t;   y = lr buf';   p' = p - y

Summation tree of a segment (the header's): chunks of c = dv_lars_chunk() = 256 threads x 4 x 16 elements; every square is rounded
to fp32 and added to its thread's one accumulator (<= 64 terms, in order), a six-deep butterfly folds the wavefront, the four
wavefront sums are added in order (fp32), and the chunk partials are folded in double in index order; q is formed in double and
rounded once.  Every term is >= 0, so a path from a term to the total crosses 1 squaring and at most 64 + 6 + 4 additions:

    |S^ - sum x^^2| <= G sum x^^2,     G = (1 + u)^75 - 1 + n_blocks 2^-53,      u = 2^-24          (x^: the kernel's own operand)

  (A) a grid on which every operation is exact (|p| = 2^-3, |d| = 2^-4, n = 4^k, eta = 2^-10, mu = 1/2, lr = 2^-8; wd = 0 or 1/4):
      p', buf' and q equal float64 BIT FOR BIT.
  (B) Gaussian data, three steps, against float64 with a DERIVED bound.  b(x) bounds |x_fp32 - x_float64|;
      rnd(x, prop) = prop + u (|x| + prop) is one rounding of a value within prop of x (tests/optim_support.py).  The reference uses
      the very floats the entries receive (lr, mu, wd, eta, gs), the gradient is the same fp32 data, so per step, from b(p), b(buf):
          b(a1) = rnd(a1, 0)        b(a2) = rnd(a2, wd b(p))        b(d) = DECAY ? rnd(d, b(a1) + b(a2)) : b(a1)
          E(x)  = sum (2 |x| b(x) + b(x)^2) + n 2^-149              [sum x^^2 - sum x^2, and a square may underflow]
          b(S)  = E + G (S + E)                                     for S = Sp (x = p) and S = Sd (x = d)
          b(s)  = b(S) / (sqrt(S) + sqrt(S - b(S))) + 2^-52 s       s = sqrt(S) in double
          b(r)  = (b(sp) + r b(sd)) / (sd - b(sd))                  r = sp / sd
          b(q)  = rnd(q, eta b(r) + 2^-51 q)                        [two double operations, then ONE rounding to float]
          b(t)  = rnd(t, |q| b(d) + |d| b(q) + b(q) b(d))           (b(t) = b(d) where q = 1 by the rule: 1 d is exact)
          b(x)  = rnd(x, mu b(buf))      b(buf') = rnd(buf', b(x) + b(t))      b(y) = rnd(y, lr b(buf'))      b(p') = rnd(p', b(p) + b(y))
      Nothing here is fitted to what the kernels return.  Data properties are asserted: Sp > 2 b(Sp) and Sd > 2 b(Sd) for every
      ADAPT segment (otherwise q falls to 1 and the case tests nothing).
  (C) DECAY-only segments over contiguous data give the bits of ONE dv_sgd_momentum call; (D) a segment's result does not depend
      on its place in the table or on its neighbours, and a repeated launch repeats the bits; (E) all-zero segments give q = 1;
      (F) the compute copy is the round-to-nearest-even cast of the new master; (G) optim.LARS on real arenas, with filled
      gradients against a per-tensor float64 replay and after a real forward / backward of R(2+1)D (padded weight rows: the norms
      are those of the tensors' real elements); (H) a state_dict taken after two steps continues with the same bits.

  Each case prints (-s) err / bound; the largest per quantity measured on an MI355X (all 20 tests pass, in about 6 s):
      lars.p 0.996  lars.buf 0.595  lars.q 0.019   (dv_lars_norms + dv_lars_step against float64, 3 steps)
      clf.p  0.998  clf.buf  0.545  clf.q  0.015   (optim.LARS on LinearClassifier arenas)
      model.q 0.017 (after a real backward of R(2+1)D, fp32 0.013 / bf16 0.017 over 26 weights)   zero.p 0.187
  A numpy float32 replay of the operation list and of the summation tree, run under this file's own code on the CPU, gives the
  same lars.* and clf.* figures: every operation rounds as IEEE does.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import _lib, ops  # noqa: E402
from dualvar_amd._lib import DV_BF16, DV_F32  # noqa: E402
from tests import checks  # noqa: E402
from tests.checks import F64, U, Ratios, bits, f32, is_sent, report_fixture, sent  # noqa: E402
from tests.optim_support import _classifier, _fill_grads, rnd  # noqa: E402

ADAPT, DECAY = 1, 2
RATIO = Ratios()
within = RATIO.within
_report = report_fixture(RATIO, 20)
# bit for bit against float64: the reference must be an fp32 number; + 0.0 on both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)


def chunk():
    return int(_lib.load().dv_lars_chunk())


# ------------------------------------------------------------------------------------------------- tables
class Table:
    """segments [(n, flags)] laid out in one arena with `gap` untouched elements in front of, between and behind them (gap = 0:
    contiguous; every offset stays a multiple of 8), and the device copies dv_lars_* read"""

    def __init__(self, specs, dev, gap=8):
        c = chunk()
        self.dev, self.specs = dev, list(specs)
        self.off, self.nb, self.first = [], [], []
        off, first = gap, 0
        for n, _ in self.specs:
            self.off.append(off)
            self.nb.append((n + c - 1) // c)
            self.first.append(first)
            first += self.nb[-1]
            off = ((off + n + 7) & ~7) + gap
        self.total = off + (8 if gap else 0)
        self.total_blocks = first
        arr = (_lib.LarsSeg * len(self.specs))()
        bmap = []
        for i, (n, flags) in enumerate(self.specs):
            arr[i].off, arr[i].n, arr[i].flags, arr[i].first_block, arr[i].n_blocks = self.off[i], n, flags, self.first[i], self.nb[i]
            bmap += [i] * self.nb[i]
        self.segs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.block_seg = torch.tensor(bmap, dtype=torch.int32, device=dev)
        self.partials = sent((2 * first,), dev)
        self.q_out = sent((len(self.specs),), dev)

    def sl(self, i):
        return slice(self.off[i], self.off[i] + self.specs[i][0])

    def arena(self, parts64, dtype=torch.float32):
        """a sentinel-filled arena holding the segments' data"""
        t = sent((self.total,), self.dev, dtype)
        for i, x in enumerate(parts64):
            t[self.sl(i)] = x.to(dtype)
        return t

    def outside(self):
        keep = torch.ones(self.total, dtype=torch.bool, device=self.dev)
        for i in range(len(self.specs)):
            keep[self.sl(i)] = False
        return keep

    def step(self, p, g, buf, c, code=DV_F32, cp=None, q_out=True):
        """exactly the two calls optim.LARS.step makes"""
        n = len(self.specs)
        ops.call('dv_lars_norms', p, g, self.segs, self.block_seg, n, self.total_blocks, c.wd, c.gs, self.partials)
        ops.call('dv_lars_step', p, g, buf, self.segs, self.block_seg, n, self.total_blocks, c.lr, c.mu, c.wd, c.eta, c.gs,
                 self.partials, code, cp, self.q_out if q_out else None)


# ------------------------------------------------------------------------------------------------- the float64 reference
class Hyper:
    """the floats the entries receive: the reference computes with these very values"""

    def __init__(self, lr, mu, wd, eta, gs):
        self.lr, self.mu, self.wd, self.eta, self.gs = f32(lr), f32(mu), f32(wd), f32(eta), f32(gs)


def tree_gamma(n_blocks):
    """G of the module docstring: the relative error of the kernels' summation tree (not chains.gamma: 75 roundings compounded,
    plus the double fold of the chunk partials)"""
    return (1.0 + U) ** 75 - 1.0 + n_blocks * 2.0 ** -53


def sum_bound(x, bx, n_blocks):
    """S = sum x^2 in float64 and b(S) for the kernel's tree over operands within bx of x"""
    S = float((x * x).sum())
    E = float((2 * x.abs() * bx + bx * bx).sum()) + x.numel() * 2.0 ** -149
    return S, E + tree_gamma(n_blocks) * (S + E)


def ratio_ref(p, bp, d, bd, flags, c, n_blocks, what=''):
    """q and b(q) of one segment"""
    if not flags & ADAPT:
        return 1.0, 0.0, False
    Sp, bSp = sum_bound(p, bp, n_blocks)
    Sd, bSd = sum_bound(d, bd, n_blocks)
    if not (Sp > 0 and Sd > 0):
        return 1.0, 0.0, False
    assert Sp > 2 * bSp and Sd > 2 * bSd, f'{what}: a norm is not well above its own error (test data): {Sp} {bSp} {Sd} {bSd}'
    sp, sd = math.sqrt(Sp), math.sqrt(Sd)
    bsp = bSp / (sp + math.sqrt(Sp - bSp)) + 2.0 ** -52 * sp
    bsd = bSd / (sd + math.sqrt(Sd - bSd)) + 2.0 ** -52 * sd
    r = sp / sd
    br = (bsp + r * bsd) / (sd - bsd)
    q = c.eta * r
    prop = c.eta * br + 2.0 ** -51 * q
    return q, prop + U * (q + prop), True


def lars_ref(p, g, buf, bp, bb, flags, c, n_blocks, exact=False, what=''):
    """one step of one segment in float64 and the bounds of the module docstring -> p', buf', q, b(p'), b(buf'), b(q)"""
    a1 = g * c.gs
    b_a1 = U * a1.abs()
    if flags & DECAY:
        a2 = c.wd * p
        d = a1 + a2
        bd = None if exact else rnd(d, b_a1 + rnd(a2, c.wd * bp))
    else:
        a2, d, bd = None, a1, b_a1
    if exact:
        zero = torch.zeros_like(p)
        bp, bb, bd = zero, zero, zero
    q, bq, adapt = ratio_ref(p, bp, d, bd, flags, c, 0 if exact else n_blocks, what)
    t = q * d
    x = c.mu * buf
    buf2 = x + t
    y = c.lr * buf2
    p2 = p - y
    if exact:
        for name, v in (('a1', a1), ('a2', a2), ('d', d), ('t', t), ('x', x), ("buf'", buf2), ('y', y), ("p'", p2)):
            assert v is None or bool((v.float().double() == v).all()), f'{name} is not exact in fp32 (test data)'
        assert f32(q) == q, 'q is not exact in fp32 (test data)'
        return p2, buf2, q, None, None, None
    bt = rnd(t, abs(q) * bd + d.abs() * bq + bq * bd) if adapt else bd
    bx = rnd(x, c.mu * bb)
    bb2 = rnd(buf2, bx + bt)
    by = rnd(y, c.lr * bb2)
    bp2 = rnd(p2, bp + by)
    return p2, buf2, q, bp2, bb2, bq


def check_q(got, q, bq, what, quiet=True):
    within(torch.tensor([got], dtype=F64), torch.tensor([q], dtype=F64), torch.tensor([bq], dtype=F64), what, quiet=quiet)


# ------------------------------------------------------------------------------------------------------ (A) exact grid
@pytest.mark.parametrize('wd', [0.0, 0.25])
def test_lars_exact_grid(gpu, wd):
    """n = 4^k, |p| = 2^-3, |d| = 2^-4 (wd = 0: g = +-1/4 times grad_scale 1/4; wd = 1/4: g = p = +-1/8, so a1 = a2 = +-2^-5):
    Sp = 4^(k-3), Sd = 4^(k-4), both roots and q = 2^-10 * 2 are exact, and so is every later operation -- bit for bit"""
    c = Hyper(2.0 ** -8, 0.5, wd, 2.0 ** -10, 0.25)
    ks = [0, 1, 2, 3, 5, 7, 8, 9]                     # 4^7 = one chunk exactly, 4^9 = 16 chunks
    assert 4 ** 7 == chunk()
    tab = Table([(4 ** k, ADAPT | DECAY) for k in ks], gpu)
    gen = torch.Generator().manual_seed(11)
    p64, g64, b64 = [], [], []
    for k in ks:
        n = 4 ** k
        sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double().to(gpu)
        p64.append(sign / 8)
        g64.append(sign / 8 if wd else (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double().to(gpu) / 4)
        b64.append(torch.randint(-8, 9, (n,), generator=gen).double().to(gpu) / 8)
    p, g, buf = tab.arena(p64), tab.arena(g64), tab.arena(b64)
    tab.step(p, g, buf, c)
    for i, k in enumerate(ks):
        p2, buf2, q, _, _, _ = lars_ref(p64[i], g64[i], b64[i], None, None, ADAPT | DECAY, c, tab.nb[i], exact=True)
        assert q == 2.0 ** -9
        what = f'k={k} wd={wd}'
        same_bits(p[tab.sl(i)], p2, 'lars p ' + what)
        same_bits(buf[tab.sl(i)], buf2, 'lars buf ' + what)
        same_bits(tab.q_out[i:i + 1], torch.tensor([q], dtype=F64, device=gpu), 'lars q ' + what)
        assert torch.equal(g[tab.sl(i)].double(), g64[i]), what + ': the gradient was written'
    keep = tab.outside()
    assert is_sent(p, keep) and is_sent(buf, keep) and is_sent(g, keep)


# ---------------------------------------------------------------------------------------------------- (B) Gaussian data
def mixed_specs():
    c = chunk()
    return [(1, ADAPT | DECAY), (8, 0), (c - 8, DECAY), (c, ADAPT | DECAY), (c + 8, 0), (2 * c + 24, ADAPT | DECAY),
            (40 * c + 5, ADAPT | DECAY)]


def gaussian(n, gen, dev, scale):
    return (torch.randn((n,), generator=gen) * scale).to(dev)


@pytest.mark.parametrize('gs', [1.0, 0.25])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_lars_gaussian_three_steps(gpu, wd, gs):
    c = Hyper(0.3, 0.9, wd, 1e-3, gs)
    tab = Table(mixed_specs(), gpu)
    gen = torch.Generator().manual_seed(int(wd * 1e4) * 2 + int(gs * 4))
    ns = [n for n, _ in tab.specs]
    p32 = [gaussian(n, gen, gpu, 0.05) for n in ns]
    p64 = [x.double() for x in p32]
    b64 = [torch.zeros(n, dtype=F64, device=gpu) for n in ns]
    bp = [torch.zeros(n, dtype=F64, device=gpu) for n in ns]
    bb = [torch.zeros(n, dtype=F64, device=gpu) for n in ns]
    p, buf = tab.arena(p64), tab.arena(b64)
    keep = tab.outside()
    for step in range(3):
        g32 = [gaussian(n, gen, gpu, 0.01 / gs) for n in ns]
        g = tab.arena([x.double() for x in g32])
        tab.q_out.copy_(sent((len(ns),), gpu))
        tab.step(p, g, buf, c)
        q_got = tab.q_out.double().tolist()
        for i, (n, flags) in enumerate(tab.specs):
            tag = f'step {step} seg {i} n={n} flags={flags} wd={wd:g} gs={gs:g}'
            p64[i], b64[i], q, bp[i], bb[i], bq = lars_ref(p64[i], g32[i].double(), b64[i], bp[i], bb[i], flags, c, tab.nb[i], what=tag)
            assert (q != 1.0) == bool(flags & ADAPT), tag + ': an ADAPT segment whose ratio fell to 1 tests nothing (test data)'
            quiet = step < 2 or n < chunk()
            within(p[tab.sl(i)], p64[i], bp[i], 'lars.p ' + tag, quiet=quiet)
            within(buf[tab.sl(i)], b64[i], bb[i], 'lars.buf ' + tag, quiet=quiet)
            check_q(q_got[i], q, bq, 'lars.q ' + tag, quiet=quiet)
            assert torch.equal(g[tab.sl(i)], g32[i]), tag + ': the gradient was written'
        assert is_sent(p, keep) and is_sent(buf, keep) and is_sent(g, keep), \
            'an element outside the segments was written'


# ---------------------------------------------------------------------------------------------------- (C) SGD equivalence
@pytest.mark.parametrize('copy', ['bf16', 'none'])
def test_lars_decay_only_segments_are_sgd_momentum(gpu, copy):
    """segments with DECAY and without ADAPT over contiguous data: the bits of one dv_sgd_momentum call over the same range, in p,
    buf and the bf16 copy, for three steps"""
    c = chunk()
    ns = [8, c - 8, c, c + 8, 2 * c + 24, 5 * c + 5]
    tab = Table([(n, DECAY) for n in ns], gpu, gap=0)
    N = sum(ns)
    assert tab.off[0] == 0 and tab.off[-1] + ns[-1] == N and all(a + n == b for a, n, b in zip(tab.off, ns, tab.off[1:]))
    h = Hyper(0.03, 0.9, 5e-4, 1e-3, 0.125)
    gen = torch.Generator().manual_seed(5)
    p0, buf0 = gaussian(N, gen, gpu, 0.05), gaussian(N, gen, gpu, 0.01)
    dt = torch.bfloat16 if copy == 'bf16' else None
    state = []
    for impl in ('lars', 'sgd'):
        p, buf = torch.cat([p0, sent((8,), gpu)]), torch.cat([buf0, sent((8,), gpu)])
        cp = sent((N + 8,), gpu, torch.bfloat16)
        g2 = torch.Generator().manual_seed(6)
        for step in range(3):
            g = torch.cat([gaussian(N, g2, gpu, 0.02), sent((8,), gpu)])
            if impl == 'lars':
                tab.step(p, g, buf, h, DV_BF16, cp if dt is not None else None)
            else:
                ops.call('dv_sgd_momentum', p, g, buf, N, h.lr, h.mu, h.wd, h.gs, DV_BF16, cp if dt is not None else None)
        state.append((p, buf, cp))
    for a, b, name in zip(state[0], state[1], ('p', 'buf', 'bf16 copy')):
        assert torch.equal(bits(a), bits(b)), f'{name}: LARS without ADAPT is not dv_sgd_momentum'
    assert not torch.equal(state[0][0][:N], p0)
    assert is_sent(state[0][0][N:]) and is_sent(state[0][2][N:])
    assert is_sent(state[0][2]) == (dt is None)
    assert tab.q_out.tolist() == [1.0] * len(ns)


# ------------------------------------------------------------------------------------------- (D) independence, determinism
def test_lars_segment_is_independent_of_its_place_and_launches_repeat(gpu):
    c = chunk()
    h = Hyper(0.3, 0.9, 1e-4, 1e-3, 0.5)
    n = 2 * c + 24
    gen = torch.Generator().manual_seed(9)
    X = [gaussian(n, gen, gpu, s).double() for s in (0.05, 0.01, 0.02)]               # p, g, buf of the segment under test
    results = []
    for specs, at in (([(n, ADAPT | DECAY), (c + 8, ADAPT | DECAY)], 0),
                      ([(8, 0), (3 * c, ADAPT | DECAY), (n, ADAPT | DECAY), (1, DECAY)], 2)):
        tab = Table(specs, gpu, gap=8 if at == 0 else 16)
        parts = [[gaussian(m, gen, gpu, s).double() for m, _ in specs] for s in (0.07, 0.3, 0.02)]
        for k in range(3):
            parts[k][at] = X[k]
        p, g, buf = (tab.arena(x) for x in parts)
        state0 = (p.clone(), buf.clone())
        tab.step(p, g, buf, h)
        results.append((p[tab.sl(at)].clone(), buf[tab.sl(at)].clone(), tab.q_out[at:at + 1].clone()))
        # the same launch pair from the same state: the same bits everywhere
        p2, buf2 = state0[0].clone(), state0[1].clone()
        q1, part1 = tab.q_out.clone(), tab.partials.clone()
        tab.q_out.copy_(sent((len(specs),), gpu))
        tab.step(p2, g, buf2, h)
        assert torch.equal(bits(p2), bits(p)) and torch.equal(bits(buf2), bits(buf)) and torch.equal(bits(tab.q_out), bits(q1))
        assert torch.equal(bits(tab.partials), bits(part1))
    for a, b, name in zip(results[0], results[1], ('p', 'buf', 'q')):
        assert torch.equal(bits(a), bits(b)), f'{name} of a segment depends on its place in the table'
    assert float(results[0][2]) != 1.0 and not torch.equal(results[0][0].double(), X[0])


# ---------------------------------------------------------------------------------------------------- (E) degenerate
def test_lars_zero_segments_take_ratio_one(gpu):
    """all-zero p (Sp = 0), all-zero g with wd = 0 (Sd = 0), both: q = 1, finite outputs, zeros stay zero where d = 0"""
    c = chunk()
    n = c + 8
    gen = torch.Generator().manual_seed(3)
    z = torch.zeros(n, dtype=F64, device=gpu)
    gd = gaussian(n, gen, gpu, 0.01).double()
    pd = gaussian(n, gen, gpu, 0.05).double()
    tab = Table([(n, ADAPT | DECAY)] * 4, gpu)
    h = Hyper(0.3, 0.9, 0.0, 1e-3, 1.0)
    p, g, buf = tab.arena([z, pd, z, pd]), tab.arena([gd, z, z, gd]), tab.arena([z, z, z, z])
    tab.step(p, g, buf, h)
    q = tab.q_out.tolist()
    assert q[:3] == [1.0, 1.0, 1.0] and q[3] != 1.0 and math.isfinite(q[3])
    keep = tab.outside()
    assert bool(torch.isfinite(p[~keep]).all()) and bool(torch.isfinite(buf[~keep]).all())
    # segment 0: p = 0, q = 1: plain momentum SGD from zero state
    same = lars_ref(z, gd, z, z, z, DECAY, h, 2)
    within(p[tab.sl(0)], same[0], same[3], 'zero.p seg 0', quiet=True)
    # segments 1 and 2: d = 0: the momentum stays 0 and p keeps its bits
    for i, want in ((1, pd), (2, z)):
        assert bool((bits(buf[tab.sl(i)]) == 0).all()), i
        assert torch.equal(p[tab.sl(i)].double(), want), i
    # the same with weight decay on and p = g = 0: everything stays +0
    h2 = Hyper(0.3, 0.9, 1e-4, 1e-3, 1.0)
    tab2 = Table([(n, ADAPT | DECAY), (8, 0)], gpu)
    z8 = torch.zeros(8, dtype=F64, device=gpu)
    p, g, buf = tab2.arena([z, z8]), tab2.arena([z, z8]), tab2.arena([z, z8])
    for _ in range(3):
        tab2.step(p, g, buf, h2)
    assert tab2.q_out.tolist() == [1.0, 1.0]
    for t in (p, buf):
        assert bool((bits(t)[~tab2.outside()] == 0).all())


# ---------------------------------------------------------------------------------------------------- (F) compute copy
@pytest.mark.parametrize('copy', ['bf16', 'f32', 'none'])
def test_lars_compute_copy_is_the_cast_of_the_new_master(gpu, copy):
    dt = {'bf16': torch.bfloat16, 'f32': torch.float32, 'none': None}[copy]
    code = DV_BF16 if copy == 'bf16' else DV_F32
    tab = Table(mixed_specs()[:6], gpu)
    ns = [n for n, _ in tab.specs]
    h = Hyper(0.3, 0.9, 1e-4, 1e-3, 1.0)
    gen = torch.Generator().manual_seed(21)
    p = tab.arena([gaussian(n, gen, gpu, 0.05).double() for n in ns])
    buf = tab.arena([torch.zeros(n, dtype=F64, device=gpu) for n in ns])
    cp = sent((tab.total,), gpu, dt or torch.float32)
    keep = tab.outside()
    for step in range(3):
        before = p.clone()
        g = tab.arena([gaussian(n, gen, gpu, 0.01).double() for n in ns])
        tab.step(p, g, buf, h, code, cp if dt is not None else None, q_out=step != 1)
        assert not torch.equal(before[~keep], p[~keep])
        if dt is None:
            assert is_sent(cp), 'copy = NULL but the copy buffer changed'
        else:
            assert torch.equal(bits(cp[~keep]), bits(p[~keep].to(dt))), 'the copy is not the round-to-nearest-even cast of the new master'
            assert is_sent(cp, keep), 'copy written outside the segments'


# ------------------------------------------------------------------------------- (G) optim.LARS on a real model's arenas
def _blocks(st, p):
    s = st.slot(p)
    return (((s.size + 7) & ~7) + chunk() - 1) // chunk()


def _flags(st, p, exclude_vec=True):
    return 0 if (st.slot(p).kind == 'vec' and exclude_vec) else (ADAPT | DECAY)


@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
@pytest.mark.parametrize('mode', ['ft', 'last'])
def test_optim_lars_on_classifier_arenas_against_float64(gpu, mode, dtype):
    """three steps of optim.LARS on a LinearClassifier's arenas against the float64 formula replayed per tensor on the tensor
    views (gradients filled through p.grad): p, momentum and trust ratio within the op bound; frozen tensors and every arena
    element outside the trainable runs bit-identical; the bf16 compute copy is the cast of the master"""
    from dualvar_amd.optim import LARS
    lr, mu, wd, eta = 0.3, 0.9, 1e-4, 1e-3
    c = _classifier(gpu, mode, dtype)
    st = c.stores()[0]
    params = [p for p in c.parameters() if p.requires_grad]
    assert len(params) == (4 if mode == 'last' else len(list(c.parameters())))
    frozen = {k: v.clone() for k, v in c.state_dict().items() if 'backbone' in k} if mode == 'last' else {}
    master0 = st.master.clone()
    opt = LARS([{'params': [p]} for p in params], lr=lr, momentum=mu, weight_decay=wd, eta=eta, stores=c.stores())
    h = Hyper(lr, mu, wd, eta, 1.0)
    gen = torch.Generator().manual_seed(3)
    ref = [dict(p=p.detach().double().clone(), b=torch.zeros_like(p, dtype=F64), bp=torch.zeros_like(p, dtype=F64),
                bb=torch.zeros_like(p, dtype=F64)) for p in params]
    flags = [_flags(st, p) for p in params]
    assert set(flags) == {0, ADAPT | DECAY}
    for t in (1, 2, 3):
        _fill_grads(params, gen)
        grads = [p.grad.detach().double().clone() for p in params]
        opt.step()
        views = dict(opt._momentum_views())
        tr = dict(opt.trust_ratios())
        assert sorted(tr) == list(range(len(params)))
        for i, (p, r) in enumerate(zip(params, ref)):
            tag = f'{mode} step {t} tensor {i}'
            r['p'], r['b'], q, r['bp'], r['bb'], bq = lars_ref(r['p'], grads[i], r['b'], r['bp'], r['bb'], flags[i], h, _blocks(st, p), what=tag)
            assert (q != 1.0) == bool(flags[i]), tag
            within(p.detach(), r['p'], r['bp'], 'clf.p ' + tag, quiet=True)
            within(views[i], r['b'], r['bb'], 'clf.buf ' + tag, quiet=True)
            check_q(tr[i], q, bq, 'clf.q ' + tag)
        if t == 3:
            print(f'    {mode} step {t}: ' + '  '.join(f'{k} {RATIO[k]:.3f}' for k in ('clf.p', 'clf.buf', 'clf.q')))
    assert st._dirty and st._cast_done and st.pending_backward == 0
    for k, v in frozen.items():
        assert torch.equal(c.state_dict()[k], v), k + ': a frozen tensor changed'
    ranges = st.trainable_ranges()
    keep = torch.ones(st.total, dtype=torch.bool, device=gpu)
    for a, n in ranges:
        keep[a:a + n] = False
    assert torch.equal(bits(st.master[keep]), bits(master0[keep])), 'elements outside the trainable runs changed'
    assert bool((opt._momentum_buf(st)[keep] == 0).all()), 'momentum outside the trainable runs changed'
    assert len(ranges) == 1 and (mode == 'last') == bool(keep.any())
    if dtype == DV_BF16:
        for a, n in ranges:
            assert torch.equal(bits(st.cc[a:a + n]), bits(st.master[a:a + n].to(torch.bfloat16)))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_optim_lars_trust_ratios_after_a_real_backward(gpu, dtype):
    """one real forward + backward + LARS.step() of SimCLR_Naked('r21d') on 4 clips of 3x8x32x32 (3-channel stem, 45-channel
    mid-planes: weight rows padded to cin_pitch > Cin): every tensor's q, recomputed in float64 from p and p.grad read before the
    step, matches trust_ratios() within the norm bound -- the norms are those of the tensors' REAL elements (the gradient arena
    holds zeros in the structural padding, or the descriptor would have to skip those lanes)"""
    from dualvar_amd import model as M
    from dualvar_amd.optim import LARS
    from oracle import procedural as P
    torch.manual_seed(0)
    m = M.SimCLR_Naked('r21d', 128, 0.07, False)
    P.procedural_init(m)
    m.train()
    m.set_compute_dtype(dtype).to(gpu)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = LARS([{'params': [p]} for p in params], lr=0.03, momentum=0.9, weight_decay=5e-4, eta=1e-3, stores=m.stores())
    x = P.procedural_clips(2, 2, 8, 32, 32).to(gpu)
    loss = m(x)['clip_contrast_loss']
    opt.zero_grad()
    loss.backward()
    st = m.stores()[0]
    assert any(s.cin_pitch > s.Cin for s in st.slots if s.kind == 'conv')
    h = Hyper(0.03, 0.9, 5e-4, 1e-3, 1.0)
    before = [(p.detach().double().clone(), p.grad.detach().double().clone()) for p in params]
    opt.step()
    tr = dict(opt.trust_ratios())
    assert sorted(tr) == list(range(len(params))) and math.isfinite(float(loss))
    n_adapt = 0
    for i, ((p64, g64), p) in enumerate(zip(before, params)):
        fl = _flags(st, p)
        zero = torch.zeros_like(p64)
        a1 = g64 * h.gs
        d = a1 + h.wd * p64 if fl & DECAY else a1
        bd = rnd(d, U * a1.abs() + rnd(h.wd * p64, zero)) if fl & DECAY else U * a1.abs()
        q, bq, adapt = ratio_ref(p64, zero, d, bd, fl, h, _blocks(st, p), what=f'tensor {i}')
        assert adapt == bool(fl), f'tensor {i} {tuple(p.shape)}: a weight without gradient or without norm'
        n_adapt += adapt
        check_q(tr[i], q, bq, f'model.q {dtype} tensor {i} {tuple(p.shape)}')
        assert not (adapt and torch.equal(p.detach().double(), p64)), f'tensor {i} was not stepped'
    assert n_adapt >= 20
    print(f'    r21d {dtype}: model.q {RATIO["model.q"]:.3f} over {n_adapt} weights')


# ---------------------------------------------------------------------------------------------------- (H) resume
def test_optim_lars_resumes_with_the_same_bits(gpu):
    """state_dict() after two steps, loaded into a fresh LARS on a second identical model: step 3 gives the same bits on both"""
    from dualvar_amd.optim import LARS
    a, b = _classifier(gpu, 'ft', DV_F32), _classifier(gpu, 'ft', DV_F32)
    pa, pb = list(a.parameters()), list(b.parameters())
    kw = dict(momentum=0.9, weight_decay=1e-4, eta=2e-3)
    oa = LARS([{'params': [p]} for p in pa], lr=0.3, stores=a.stores(), **kw)
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        _fill_grads(pa, gen)
        oa.step()
    sd = oa.state_dict()
    assert len(sd['state']) == len(pa) and sd['param_groups'][0]['eta'] == 2e-3 and sd['param_groups'][0]['exclude_vec'] is True
    with torch.no_grad():
        for x, y in zip(pa, pb):
            y.copy_(x)
    ob = LARS([{'params': [p]} for p in pb], lr=0.01, eta=0.5, exclude_vec=False, stores=b.stores())
    assert ob.load_state_dict(sd) == len(pb)
    assert ob.param_groups[0]['lr'] == 0.3 and ob.param_groups[0]['eta'] == 2e-3 and ob.param_groups[0]['exclude_vec'] is True
    _fill_grads(pa, gen)
    with torch.no_grad():
        for x, y in zip(pa, pb):
            y.grad.copy_(x.grad)
    oa.step()
    ob.step()
    sa, sb = a.stores()[0], b.stores()[0]
    assert torch.equal(bits(sa.master), bits(sb.master)), 'the parameters differ after the resumed step'
    assert torch.equal(bits(oa._momentum_buf(sa)), bits(ob._momentum_buf(sb))), 'the momentum differs after the resumed step'
    assert oa.trust_ratios() == ob.trust_ratios()
    assert any(q != 1.0 for _, q in oa.trust_ratios())
