"""What the float64 suites share: sentinel buffers, bit views, the comparisons against float64, the err / bound recorder
and its report, channel-slice views and a few small helpers.  Written once so that a name means one thing in every suite;
tests/test_checks_host.py pins it on CPU tensors.  (The models of the kernels' summation orders are in tests/chains.py.)"""
import subprocess
import sys

import numpy as np
import pytest
import torch

from dualvar_amd._lib import DV_BF16, DV_F32

U = 2.0 ** -24                     # unit roundoff of fp32
BF16_U = 2.0 ** -8                 # unit roundoff of a bf16 store (8 significant bits)
F64 = torch.float64
TDT = {DV_F32: torch.float32, DV_BF16: torch.bfloat16}
# storage dtype -> (integer view, a NaN bit pattern no kernel produces; int32 buffers take the fp32 pattern as it is)
SENT = {torch.float32: (torch.int32, 0x7fb12345), torch.bfloat16: (torch.int16, 0x7fb1),
        torch.float64: (torch.int64, 0x7ff8123456789abc), torch.int32: (torch.int32, 0x7fb12345)}


# ----------------------------------------------------------------------------------------------------------- small helpers
def f32(x):
    """the fp32 value a C float argument receives"""
    return float(np.float32(x))


def cp8(c):
    return (c + 7) & ~7


def vec(dtype):
    return 4 if dtype == DV_F32 else 8


def ceil_div(a, b):
    return -(-a // b)


def dev_gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def lib():
    from dualvar_amd import _lib
    return _lib.load()


def launch(name, *args):
    """one entry of the C ABI on the current stream; a non-zero return code raises"""
    from dualvar_amd import _lib, ops
    _lib.check(getattr(_lib.load(), name)(*args, ops.stream_ptr()), name)


def chan(vals, CP, dev, junk=0.625):
    """per-channel fp32 array readable up to CP (16-byte loads), junk in the pad lanes"""
    t = torch.full((CP,), junk, dtype=torch.float32, device=dev)
    t[:vals.numel()] = vals.float().to(dev)
    return t


CHAIN = {}


def child(argv, cwd, timeout):
    """one GPU child process under its own timeout; a failure marks the chain as broken, for every suite of the run"""
    assert not CHAIN.get('broken'), 'an earlier child failed or died: no further GPU child is started'
    CHAIN['broken'] = True
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    CHAIN['broken'] = False
    return out


# ----------------------------------------------------------------------------------------------------- sentinels, bit views
def _torch_dtype(dtype):
    return TDT.get(dtype, dtype) if isinstance(dtype, int) else dtype


def bits(t):
    """the integer view of a tensor's bits (a copy where t is not contiguous); integer tensors as they are"""
    return t.contiguous().view(SENT[t.dtype][0]) if t.dtype.is_floating_point else t


def sent(shape, dev, dtype=torch.float32):
    """a buffer of the sentinel pattern; dtype a torch dtype or a DV_* code"""
    dt = _torch_dtype(dtype)
    it, pattern = SENT[dt]
    return torch.full(shape, pattern, dtype=it, device=dev).view(dt)


def is_sent(t, where=None):
    """every element of t (of t[where]: a bool mask) still holds the sentinel bits; True for no elements"""
    same = bits(t) == SENT[t.dtype][1]
    return bool((same if where is None else same[where]).all())


# -------------------------------------------------------------------------------------------------------------- comparisons
class Ratios(dict):
    """quantity -> largest err / bound of the run.  A suite makes one, checks through its `within` / `ratio`, and prints it
    from a module fixture (`report_fixture`), so that its figures appear under its own heading."""

    def within(self, got, ref64, bound, what, key=None, quiet=False):
        return within(got, ref64, bound, what, self, key, quiet)

    def ratio(self, err, bound, what, key=None, quiet=True):
        return err_within(err, bound, what, self, key, quiet)

    def report(self, width=20, title='largest err / bound per quantity:'):
        print('\n' + title)
        for k in sorted(self):
            print('  %-*s %.3f' % (width, k, self[k]))


def report_fixture(ratios, width=20):
    """the module-scoped autouse fixture that prints `ratios` after the module's last test"""
    @pytest.fixture(scope='module', autouse=True)
    def _report():
        yield
        ratios.report(width)
    return _report


def err_within(err, bound, what, ratios=None, key=None, quiet=True):
    """err <= bound elementwise, no element left out: a NaN on either side and a non-finite error fail, and where the bound is
    0 the error must be 0.  Returns the largest err / bound over bound > 0 and records it in `ratios` under `key` (default: the first word of
    `what`).  err, bound: tensors, arrays or numbers that broadcast."""
    err = torch.as_tensor(err, dtype=F64)
    bound = torch.as_tensor(bound, dtype=F64, device=err.device)
    err, bound = torch.broadcast_tensors(err, bound)
    bad = ~(err <= bound) | ~torch.isfinite(err)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if ratios is not None:
        key = what.split(' ')[0] if key is None else key
        ratios[key] = max(ratios.get(key, 0.0), ratio)
    if not quiet:
        worst = float(err.max()) if err.numel() else 0.0
        print(f'    {what}: max err {worst:.3e}  err/bound {ratio:.3f}')
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} values outside the bound, err / bound = {ratio:.3f}, '
                                 f'first at {bad.nonzero()[0].tolist() if bad.dim() else []}')
    return ratio


def within(got, ref64, bound, what, ratios=None, key=None, quiet=False):
    """got is finite and |got - ref| <= bound elementwise (`err_within`); records and prints err / bound"""
    g = torch.as_tensor(got).double()
    assert bool(torch.isfinite(g).all()), f'{what}: non-finite output'
    ref64 = torch.as_tensor(ref64, dtype=F64, device=g.device)
    return err_within((g - ref64).abs(), bound, what, ratios, key, quiet)


def same_bits(got, ref64, what, *, ref_exact_in, signed_zeros):
    """got equals the float64 reference bit for bit.  Both differences between the suites are spelt out by the caller:
      ref_exact_in  torch.float32: the reference must be an fp32 number, and a bf16 `got` is held to its round-to-nearest-even
                    bf16; 'storage': the reference must be representable in got's own dtype
      signed_zeros  True: -0 and +0 are different bits; False: both sides get + 0.0 first, which only folds -0 into +0"""
    ref64 = torch.as_tensor(ref64).double().to(got.device)
    r = ref64.to(got.dtype if ref_exact_in == 'storage' else ref_exact_in)
    assert bool((r.double() == ref64).all()), f'{what}: the float64 reference is not representable in {r.dtype} (test data)'
    g, r = got.contiguous(), r.to(got.dtype).contiguous()
    if not signed_zeros:
        g, r = g + 0.0, r + 0.0
    bad = bits(g) != bits(r)
    if bool(bad.any()):
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64; first at '
                             f'{bad.nonzero()[0].tolist()}: got {g[bad][0].item()!r} want {r[bad][0].item()!r}')


def equal_bits(a, b):
    """two tensors hold the same bits (same shape and dtype; -0 and +0, and two NaN patterns, differ)"""
    return torch.equal(bits(a), bits(b))


# -------------------------------------------------------------------------------------------------------------------- views
class View:
    """[M][C] values as columns [off, off + CP) of an [M][ld] buffer (row pitch ld), CP = cp8(C).  The buffer starts as the
    sentinel pattern everywhere: an output keeps it outside the view.  `set` writes the values and fills the pad lanes
    [C, CP) with `pad` (None: leaves them as they are); an input read outside the view then reads a NaN."""

    def __init__(self, dtype, M, C_, off, ld, dev, values=None, pad=None):
        self.dtype, self.M, self.C, self.CP, self.off, self.ld = dtype, M, C_, cp8(C_), off, ld
        assert off % 8 == 0 and ld % 8 == 0 and off + self.CP <= ld
        self.buf = sent((M, ld), dev, dtype)
        if values is not None:
            self.set(values, pad)

    @classmethod
    def sliced(cls, dtype, M, C_, dev, sliced=False, values=None, pitch_pad=0):
        """zero pad lanes; sliced: at column 8 of a buffer 24 columns wider than the view, else dense (+ pitch_pad)"""
        return cls(dtype, M, C_, 8 if sliced else 0, cp8(C_) + (24 if sliced else pitch_pad), dev, values, pad=0)

    def set(self, values, pad):
        self.buf[:, self.off:self.off + self.C] = values.reshape(self.M, -1)[:, :self.C].to(self.buf.dtype).to(self.buf.device)
        if pad is not None:
            self.buf[:, self.off + self.C:self.off + self.CP] = pad

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def val(self):
        return self.buf[:, self.off:self.off + self.C].double()

    def cols(self):
        """the CP columns of the view, storage dtype"""
        return self.buf[:, self.off:self.off + self.CP]

    def check_frame(self, what):
        """outside [off, off+CP): sentinel bits; pad lanes: exactly 0"""
        assert is_sent(self.buf[:, :self.off]) and is_sent(self.buf[:, self.off + self.CP:]), \
            f'{what}: a column outside the view was written'
        assert bool((self.buf[:, self.off + self.C:self.off + self.CP] == 0).all()), f'{what}: pad lanes [C, CP) not zero'

    def untouched(self):
        return is_sent(self.buf)
