"""dv_adam (csrc/optim.hip) and dualvar_amd.optim.Adam against float64.

The entry computes, per element and with ONE fp32 rounding per operation (include/dualvar_hip.h: no FMA contraction, correctly
rounded sqrtf and division):

    a1 = g gs;  a2 = wd p;  G = a1 + a2
    dm = G - m;  t = omb1 dm;  m' = m + t
    a = b2 v;  c1 = omb2 G;  c2 = c1 G;  v' = a + c2
    s = sqrt(v');  d1 = s / sb2;  den = d1 + eps;  q = m' / den;  r = step q;  p' = p - r
    step = lr / bc1 and sb2 = sqrt(bc2) once per thread.

Two kinds of data, as in tests/test_loss_gemm_optim_gpu.py:

  (A) a grid on which every operation above is exact (omb1 = 1/2, b2 = 3/4, omb2 = 1/4, bc1 = 1/2, bc2 = 1/4, lr = 2^-8,
      |G| = 2^-3, v = 0 or G^2, eps chosen so that den is a power of two): p', m', v' equal float64 BIT FOR BIT.  sqrt is only
      exact on even powers of two, so this is one step from each of two prepared states, with and without weight decay.
  (B) Gaussian data against float64 with a DERIVED bound.  u = 2^-24; b(x) bounds |x_fp32 - x_float64|; a computed operation
      whose exact result on the computed inputs is off by at most `prop` from the float64 value x has
          b = rnd(x, prop) = prop + u (|x| + prop)                                   [one rounding of a value within prop of x]
      A hyper-parameter c that the kernel holds with relative error h_c (0 when the reference uses the very float the entry
      receives) adds h_c |c| |operand|.  Per step, from b(p), b(m), b(v) of the step before (0 at the start):
          b(a1) = rnd(a1, h_gs |a1|)            b(a2) = rnd(a2, wd b(p) + h_wd wd (|p| + b(p)))        b(G) = rnd(G, b(a1) + b(a2))
          m' = (1 - omb1) m + omb1 G exactly, and the two roundings of dm and t (and h_omb1) scale omb1 (G - m):
          b(m') = rnd(m', (1 - omb1) b(m) + omb1 b(G) + omb1 (|dm| + b(G) + b(m)) ((1 + h_omb1)(1 + u)^2 - 1))
          b(a)  = rnd(a, b2 b(v) + h_b2 b2 (|v| + b(v)))       b(c1) = rnd(c1, omb2 b(G) + h_omb2 omb2 (|G| + b(G)))
          b(c2) = rnd(c2, |c1| b(G) + |G| b(c1) + b(c1) b(G))  b(v') = rnd(v', b(a) + b(c2))
          b(s)  = rnd(s, b(v') / (sqrt(v') + sqrt(max(v' - b(v'), 0))))       [sqrt x - sqrt y = (x - y) / (sqrt x + sqrt y)]
          b(d1) = rnd(d1, (b(s) + d1 b(sb2)) / (sb2 - b(sb2)))                [x^/y^ - x/y = ((x^ - x) y - x (y^ - y)) / (y y^)]
          b(den) = rnd(den, b(d1) + h_eps eps)       b(q) = rnd(q, (b(m') + |q| b(den)) / (den - b(den)))
          b(r)  = rnd(r, step b(q) + |q| b(step) + b(step) b(q))              b(p') = rnd(p', b(p) + b(r))
      with b(step) = h_step step, b(sb2) = h_sb2 sb2.  Against the same formula in float64 on the entry's own float arguments:
      h_step = u (one division), h_sb2 = u (one square root), every other h = 0.  Against torch.optim.Adam on float64 tensors
      (double hyper-parameters): lr, bc1 rounded to float and divided: h_step = 3.01 u; bc2 rounded, then sqrt: h_sb2 = 1.51 u;
      omb1, b2, omb2, eps, wd rounded to float: u each.  Nothing here is fitted to what the kernel returns.
      Gradients are Gaussian times 10^U(-12, 3) (|g| from far below eps = 1e-8 to far above 1), the Gaussian factor kept
      >= 2^-10 in magnitude so that g^2 stays a normal number (a data property, asserted).

  Each case prints (-s) err / bound; the largest per quantity measured on an MI355X:
      adam.p 0.996  adam.m 0.656  adam.v 0.760   (dv_adam against float64, 3 steps; single operations reach their half ulp --
                                                  a numpy float32 replay of the same operation list gives the same three figures)
      clf.p  0.994  clf.m  0.910  clf.v  0.792   (optim.Adam on LinearClassifier arenas against torch.optim.Adam in float64)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dualvar_amd import ops  # noqa: E402
from dualvar_amd._lib import DV_BF16, DV_F32  # noqa: E402
from tests import checks  # noqa: E402
from tests.checks import F64, U, Ratios, f32, is_sent, report_fixture, sent  # noqa: E402
from tests.optim_support import _classifier, _fill_grads, arena, check_copy, copy_buffer, rnd  # noqa: E402

RATIO = Ratios()
within = RATIO.within
_report = report_fixture(RATIO, 20)
# bit for bit against float64: the reference must be an fp32 number; + 0.0 on both sides only folds -0 into +0
same_bits = functools.partial(checks.same_bits, ref_exact_in=torch.float32, signed_zeros=False)
NS = [1, 3, 4, 5, 1003, 2 ** 20 + 3, 2 ** 21 + 4099]       # the last: 2048 blocks x 256 threads x 4 elements, then a second trip


# ------------------------------------------------------------------------------------------------- the float64 reference
class Hyper:
    """the reference's hyper-parameters (doubles) and the relative error h_* with which the kernel holds each"""

    def __init__(self, step, sb2, omb1, b2, omb2, eps, wd, gs, h_step, h_sb2, h_other):
        self.step, self.sb2, self.omb1, self.b2, self.omb2, self.eps, self.wd, self.gs = step, sb2, omb1, b2, omb2, eps, wd, gs
        self.h_step, self.h_sb2 = h_step, h_sb2
        self.h_omb1 = self.h_b2 = self.h_omb2 = self.h_eps = self.h_wd = h_other
        self.h_gs = 0.0 if f32(gs) == gs else h_other

    @classmethod
    def of_entry(cls, lr, b1, b2, eps, wd, gs, t):
        """what dv_adam computes with, from the floats optim.Adam hands it: the reference uses these very values"""
        bc1, bc2 = f32(1.0 - b1 ** t), f32(1.0 - b2 ** t)
        return cls(f32(lr) / bc1, float(np.sqrt(bc2)), f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps), f32(wd), f32(gs), U, U, 0.0)

    @classmethod
    def of_torch(cls, lr, b1, b2, eps, wd, t):
        """torch.optim.Adam on float64 tensors: every hyper-parameter a double"""
        return cls(lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5, 1.0 - b1, b2, 1.0 - b2, eps, wd, 1.0, 3.01 * U, 1.51 * U, U)


def adam_ref(p, g, m, v, bp, bm, bv, c, exact=False):
    """one step in float64 and the bounds of the module docstring -> p', m', v', b(p'), b(m'), b(v')"""
    a1 = g * c.gs
    a2 = c.wd * p
    G = a1 + a2
    dm = G - m
    t = c.omb1 * dm
    m2 = m + t
    a = c.b2 * v
    c1 = c.omb2 * G
    c2 = c1 * G
    v2 = a + c2
    s = torch.sqrt(v2)
    d1 = s / c.sb2
    den = d1 + c.eps
    q = m2 / den
    r = c.step * q
    p2 = p - r
    if exact:
        for name, x in (('a1', a1), ('a2', a2), ('G', G), ('dm', dm), ('t', t), ("m'", m2), ('a', a), ('c1', c1), ('c2', c2),
                        ("v'", v2), ('s', s), ('d1', d1), ('den', den), ('q', q), ('r', r), ("p'", p2)):
            assert bool((x.float().double() == x).all()), f'{name} is not exact in fp32 (test data)'
        return p2, m2, v2, None, None, None
    b_a1 = rnd(a1, c.h_gs * a1.abs())
    b_a2 = rnd(a2, c.wd * bp + c.h_wd * c.wd * (p.abs() + bp))
    bG = rnd(G, b_a1 + b_a2)
    bm2 = rnd(m2, (1 - c.omb1) * bm + c.omb1 * bG + c.omb1 * (dm.abs() + bG + bm) * ((1 + c.h_omb1) * (1 + U) ** 2 - 1))
    b_a = rnd(a, c.b2 * bv + c.h_b2 * c.b2 * (v.abs() + bv))
    b_c1 = rnd(c1, c.omb2 * bG + c.h_omb2 * c.omb2 * (G.abs() + bG))
    b_c2 = rnd(c2, c1.abs() * bG + G.abs() * b_c1 + b_c1 * bG)
    bv2 = rnd(v2, b_a + b_c2)
    ssum = s + torch.sqrt((v2 - bv2).clamp_min(0))
    b_s = rnd(s, torch.where(ssum > 0, bv2 / ssum.clamp_min(1e-300), torch.sqrt(bv2)))
    bsb = c.h_sb2 * c.sb2
    b_d1 = rnd(d1, (b_s + d1 * bsb) / (c.sb2 - bsb))
    b_den = rnd(den, b_d1 + c.h_eps * c.eps)
    assert bool((den > 2 * b_den).all())
    b_q = rnd(q, (bm2 + q.abs() * b_den) / (den - b_den))
    bst = c.h_step * c.step
    b_r = rnd(r, c.step * b_q + q.abs() * bst + bst * b_q)
    bp2 = rnd(p2, bp + b_r)
    return p2, m2, v2, bp2, bm2, bv2


def call_adam(p, g, m, v, n, lr, b1, b2, eps, wd, t, gs, code, cp):
    """exactly the call optim.Adam.step makes"""
    ops.call('dv_adam', p, g, m, v, n, lr, 1.0 - b1, b2, 1.0 - b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t, gs, code, cp)


# ------------------------------------------------------------------------------------------------------ (A) exact grid
COPY_CASES = [(n, c) for n in NS for c in ('bf16', 'f32', 'none')] + [(n, 'bf16-odd') for n in (5, 1003)]


@pytest.mark.parametrize('n,copy', COPY_CASES)
def test_adam_exact(gpu, n, copy):
    """b1 = 1/2, b2 = 3/4 at t = 1 (bc1 = 1/2, bc2 = 1/4), lr 2^-8, |G| = 2^-3: one step from v = 0 and one from v = G^2, with
    weight decay 1/4 (p = +-1/4, g = +-1/4, grad_scale 1/4) and without (g = +-1/2, p multiples of 1/4), bit for bit"""
    gen = torch.Generator().manual_seed(n)
    for wd in (0.25, 0.0):
        for v_on in (0, 1):
            sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double().to(gpu)
            if wd:
                p64, g64 = sign / 4, sign / 4                       # G = g/4 + p/4 = +-2^-3
            else:
                p64, g64 = torch.randint(-32, 33, (n,), generator=gen).double().to(gpu) / 4, sign / 2
            m64 = torch.randint(-8, 9, (n,), generator=gen).double().to(gpu) / 8
            v64 = torch.full((n,), 2.0 ** -6 * v_on, dtype=F64, device=gpu)
            eps = 2.0 ** -2 if v_on else 2.0 ** -3                   # den = 2^-1 / 2^-2
            p, g, m, v = arena(p64), arena(g64), arena(m64), arena(v64)
            dt, code, whole, cp = copy_buffer(n, copy, gpu)
            call_adam(p, g, m, v, n, 2.0 ** -8, 0.5, 0.75, eps, wd, 1, 0.25, code, cp if dt is not None else None)
            c = Hyper.of_entry(2.0 ** -8, 0.5, 0.75, eps, wd, 0.25, 1)
            assert (c.step, c.sb2) == (2.0 ** -7, 0.5)
            p64, m64, v64, _, _, _ = adam_ref(p64, g64, m64, v64, None, None, None, c, exact=True)
            what = f'n={n} wd={wd} v0={v_on}'
            same_bits(p[:n], p64, 'adam p ' + what)
            same_bits(m[:n], m64, 'adam m ' + what)
            same_bits(v[:n], v64, 'adam v ' + what)
            assert is_sent(p[n:]) and is_sent(m[n:]) and is_sent(v[n:]) and is_sent(g[n:]), what
            assert torch.equal(g[:n].double(), g64), what + ': the gradient was written'
            check_copy(cp, p, n, dt, 'adam ' + what + ' ' + copy)
            assert is_sent(whole[:whole.numel() - cp.numel()]), what + ' ' + copy + ': copy written in front of its start'


def test_adam_keeps_zero_padding_and_refuses_bad_arguments(gpu):
    """p = g = m = v = 0 (the padding between arena slots) stays 0 with weight decay on; eps = 0, b2 = 1 and misaligned
    pointers are refused before any launch"""
    from dualvar_amd._lib import DualVarHipError
    n = 1003
    z = [torch.zeros(n + 8, device=gpu) for _ in range(4)]
    for t in (1, 2, 3):
        call_adam(*z, n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, t, 1.0, DV_F32, None)
    assert all(bool((x.view(torch.int32) == 0).all()) for x in z)
    for bad in (dict(eps=0.0), dict(b2=1.0), dict(b1=1.0)):
        kw = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, t=1, gs=1.0, code=DV_F32, cp=None)
        kw.update(bad)
        with pytest.raises(DualVarHipError, match='DV_EINVAL'):
            call_adam(*z, n, **kw)
    with pytest.raises(DualVarHipError, match='DV_EALIGN'):
        ops.call('dv_adam', z[0].data_ptr() + 4, z[1], z[2], z[3], 8, 1e-3, 0.1, 0.999, 0.001, 1e-8, 0.0, 0.1, 0.001, 1.0, DV_F32, None)


# ---------------------------------------------------------------------------------------------------- (B) Gaussian data
def wide_gradients(n, gen, dev, gs):
    z = torch.randn((n,), generator=gen)
    z = torch.where(z.abs() < 2.0 ** -10, torch.full_like(z, 2.0 ** -10), z)
    g = (z.double() * 10.0 ** (torch.rand((n,), generator=gen, dtype=F64) * 15 - 12) / gs).float()
    assert float(g.abs().min()) * gs > 1e-16 and float(g.abs().max()) * gs > 10
    return g.to(dev)


@pytest.mark.parametrize('gs', [1.0, 0.25])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('n', [5, 1003, 2 ** 20 + 3])
def test_adam_gaussian_three_steps(gpu, n, wd, gs):
    gen = torch.Generator().manual_seed(n)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p32 = (torch.randn((n,), generator=gen) * 0.05).to(gpu)
    zero = torch.zeros(n, dtype=F64, device=gpu)
    p, m, v = arena(p32.double()), arena(zero), arena(zero)
    p64, m64, v64 = p32.double(), zero.clone(), zero.clone()
    bp, bm, bv = zero.clone(), zero.clone(), zero.clone()
    for step in range(3):
        g32 = wide_gradients(n, gen, gpu, gs) if n > 5 else (torch.randn((n,), generator=gen) * 0.01 / gs).to(gpu)
        call_adam(p, arena(g32.double()), m, v, n, lr, b1, b2, eps, wd, step + 1, gs, DV_F32, None)
        p64, m64, v64, bp, bm, bv = adam_ref(p64, g32.double(), m64, v64, bp, bm, bv, Hyper.of_entry(lr, b1, b2, eps, wd, gs, step + 1))
        tag = f'step {step} n={n} wd={wd:g} gs={gs:g}'
        within(p[:n], p64, bp, 'adam.p ' + tag, quiet=step < 2)
        within(m[:n], m64, bm, 'adam.m ' + tag, quiet=step < 2)
        within(v[:n], v64, bv, 'adam.v ' + tag, quiet=step < 2)
        assert is_sent(p[n:]) and is_sent(m[n:]) and is_sent(v[n:])
    rel = (p[:n].double() - p64).abs() / p64.abs().clamp_min(1e-30)
    print(f'    adam n={n}: after 3 steps |p_fp32 - p_float64| / |p|: median {float(rel.median()):.2e}, bound / |p| median '
          f'{float((bp / p64.abs().clamp_min(1e-30)).median()):.2e}')


@pytest.mark.parametrize('n', [5, 1003, 2 ** 20 + 3])
def test_adam_bf16_copy_is_the_cast_of_the_new_value(gpu, n):
    gen = torch.Generator().manual_seed(n + 7)
    for code, dt in ((DV_BF16, torch.bfloat16), (DV_F32, torch.float32)):
        p = arena((torch.randn((n,), generator=gen) * 0.05).double().to(gpu))
        m, v = arena(torch.zeros(n, dtype=F64, device=gpu)), arena(torch.zeros(n, dtype=F64, device=gpu))
        cp = sent((n + 8,), gpu, dt)
        for step in range(3):
            before = p[:n].clone()
            call_adam(p, arena(torch.randn((n,), generator=gen).double().to(gpu)), m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, step + 1, 1.0, code, cp)
            assert not torch.equal(before, p[:n])
            check_copy(cp, p, n, dt, f'adam gaussian n={n} step {step}')


# ------------------------------------------------------------------------------- optim.Adam on a real model's arenas
@pytest.mark.parametrize('dtype', [DV_F32, DV_BF16])
@pytest.mark.parametrize('mode', ['ft', 'last'])
def test_optim_adam_on_classifier_arenas_against_torch(gpu, mode, dtype):
    """three steps of optim.Adam on a LinearClassifier's arenas against torch.optim.Adam in float64 fed the same gradients,
    tensor by tensor within the op bound; frozen tensors bit-identical; the bf16 compute copy is the cast of the master;
    then the state of each optimizer, loaded by the other, continues within one step's bound"""
    from dualvar_amd.optim import Adam
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-4
    c = _classifier(gpu, mode, dtype)
    st = c.stores()[0]
    params = [p for p in c.parameters() if p.requires_grad]
    assert len(params) == (4 if mode == 'last' else len(list(c.parameters())))
    frozen = {k: v.clone() for k, v in c.state_dict().items() if 'backbone' in k} if mode == 'last' else {}
    master0 = st.master.clone()
    opt = Adam([{'params': [p]} for p in params], lr=lr, betas=betas, eps=eps, weight_decay=wd, stores=c.stores())
    twins = [torch.nn.Parameter(p.detach().double().clone()) for p in params]
    topt = torch.optim.Adam([{'params': [q]} for q in twins], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    gen = torch.Generator().manual_seed(3)
    ref = [dict(p=q.detach().clone(), m=torch.zeros_like(q), v=torch.zeros_like(q), bp=torch.zeros_like(q), bm=torch.zeros_like(q),
                bv=torch.zeros_like(q)) for q in twins]

    def one_step(t, tag, quiet):
        _fill_grads(params, gen)
        for p, q in zip(params, twins):
            q.grad = p.grad.detach().double().clone()
        opt.step()
        topt.step()
        views = {i: (m_, v_) for i, m_, v_ in opt._moment_views()}
        hyp = Hyper.of_torch(lr, betas[0], betas[1], eps, wd, t)
        for i, (p, q, r) in enumerate(zip(params, twins, ref)):
            r['p'], r['m'], r['v'], r['bp'], r['bm'], r['bv'] = adam_ref(r['p'], q.grad, r['m'], r['v'], r['bp'], r['bm'], r['bv'], hyp)
            # the float64 formula of this file IS torch's Adam (to float64 rounding)
            assert float((r['p'] - q.detach()).abs().max()) <= 1e-12 * float(q.detach().abs().max()) + 1e-18, (tag, i)
            assert float((r['m'] - topt.state[q]['exp_avg']).abs().max()) <= 1e-12 * float(r['m'].abs().max()) + 1e-30
            within(p.detach(), q.detach(), r['bp'], f'clf.p {tag} tensor {i}', quiet=True)
            within(views[i][0], topt.state[q]['exp_avg'], r['bm'], f'clf.m {tag} tensor {i}', quiet=True)
            within(views[i][1], topt.state[q]['exp_avg_sq'], r['bv'], f'clf.v {tag} tensor {i}', quiet=True)
        if not quiet:
            print(f'    {tag}: ' + '  '.join(f'{k} {RATIO[k]:.3f}' for k in ('clf.p', 'clf.m', 'clf.v')))

    for t in (1, 2, 3):
        one_step(t, f'{mode} step {t}', quiet=t < 3)
    assert st._dirty and st._cast_done and st.pending_backward == 0
    for k, v in frozen.items():
        assert torch.equal(c.state_dict()[k], v), k + ': a frozen tensor changed'
    ranges = st.trainable_ranges()
    keep = torch.ones(st.total, dtype=torch.bool, device=gpu)
    for a, n in ranges:
        keep[a:a + n] = False
    assert torch.equal(st.master[keep].view(torch.int32), master0[keep].view(torch.int32)), 'elements outside the trainable runs changed'
    assert len(ranges) == 1 and (mode == 'last') == bool(keep.any())
    if dtype == DV_BF16:
        for a, n in ranges:
            assert torch.equal(st.cc[a:a + n].view(torch.int16), st.master[a:a + n].to(torch.bfloat16).view(torch.int16))

    # ---- state interchange, ours -> torch: a fresh torch Adam on the CURRENT fp32 values continues as we do
    sd = opt.state_dict()
    assert all(int(e['step']) == 3 for e in sd['state'].values()) and len(sd['state']) == len(params)
    twins = [torch.nn.Parameter(p.detach().double().clone()) for p in params]
    topt = torch.optim.Adam([{'params': [q]} for q in twins], lr=0.5, foreach=False)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == lr and topt.param_groups[0]['weight_decay'] == wd
    for q in twins:                                    # torch keeps the moments in the parameter's dtype
        assert topt.state[q]['exp_avg'].dtype == F64 and float(topt.state[q]['step']) == 3
    ref = [dict(p=q.detach().clone(), m=topt.state[q]['exp_avg'].clone(), v=topt.state[q]['exp_avg_sq'].clone(),
                bp=torch.zeros_like(q), bm=torch.zeros_like(q), bv=torch.zeros_like(q)) for q in twins]
    one_step(4, f'{mode} ours->torch step 4', quiet=False)

    # ---- torch -> ours: a second model with a fresh Adam takes torch's float64 state (cast to fp32: u |x| to start with)
    c2 = _classifier(gpu, mode, dtype)
    params2 = [p for p in c2.parameters() if p.requires_grad]
    with torch.no_grad():
        for p, q in zip(params2, twins):
            p.copy_(q.detach().float())
    opt2 = Adam([{'params': [p]} for p in params2], lr=0.5, stores=c2.stores())
    assert opt2.load_state_dict(topt.state_dict()) == len(params2) and opt2._step == 4 and opt2.param_groups[0]['lr'] == lr
    ref = [dict(p=q.detach().clone(), m=topt.state[q]['exp_avg'].clone(), v=topt.state[q]['exp_avg_sq'].clone(),
                bp=U * q.detach().abs(), bm=U * topt.state[q]['exp_avg'].abs(), bv=U * topt.state[q]['exp_avg_sq'].abs())
           for q in twins]
    params, opt = params2, opt2
    one_step(5, f'{mode} torch->ours step 5', quiet=False)
