"""What the optimizer suites (SGD / EMA, Adam, LARS) share: parameter arenas in sentinel buffers, the compute-copy checks, the
one-rounding bound and a LinearClassifier on materialised arenas."""
import torch

from dualvar_amd._lib import DV_BF16, DV_F32
from tests.checks import U, bits, is_sent, sent


def rnd(x, prop):
    """one rounding of a value within prop of x"""
    return prop + U * (x.abs() + prop)


def arena(vals64, dtype=torch.float32):
    n = vals64.numel()
    t = sent((n + 8,), vals64.device, dtype)
    t[:n] = vals64.to(dtype)
    return t


def check_copy(copy, p, n, dtype, what):
    if dtype is None:
        assert is_sent(copy), what + ': copy = NULL but the copy buffer changed'
        return
    assert torch.equal(bits(copy[:n]), bits(p[:n].to(dtype))), what + ': the copy is not the round-to-nearest-even cast of the new value'
    assert is_sent(copy[n:]), what + ': copy written past n'


def copy_buffer(n, copy, dev):
    """copy case -> (torch dtype or None, DV code, the whole sentinel buffer, the [n + 8] view the entry writes).  'bf16-odd': the
    view starts one element (2 bytes) past the allocation, so no 8-byte store of four bf16 is possible"""
    dt = {'bf16': torch.bfloat16, 'bf16-odd': torch.bfloat16, 'f32': torch.float32, 'none': None}[copy]
    off = 1 if copy == 'bf16-odd' else 0
    whole = sent((n + 8 + off,), dev, dt or torch.float32)
    cp = whole[off:]
    assert cp.data_ptr() % 8 == 2 * off
    return dt, DV_BF16 if dt == torch.bfloat16 else DV_F32, whole, cp


def _classifier(gpu, mode, dtype):
    from dualvar_amd.model import LinearClassifier
    torch.manual_seed(0)
    kw = dict(use_dropout=False) if mode == 'ft' else dict(use_dropout=True, use_l2_norm=True, use_final_bn=True)
    c = LinearClassifier(num_class=10, network='r3d', **kw)
    if mode == 'last':
        for n_, p_ in c.named_parameters():
            if 'backbone' in n_:
                p_.requires_grad = False
    c.set_compute_dtype('fp32' if dtype == DV_F32 else 'bf16')
    for st in c.stores():
        st.materialize(gpu, dtype)
    return c


def _fill_grads(params, gen, scale=1e-2):
    for p in params:
        p.grad.copy_((torch.randn(p.shape, generator=gen) * scale).to(p.device))
