"""A plain float64 convolution (forward, data gradient, weight gradient) and the Gaussian-data bound of the convolution
kernels: a loop over the kernel taps, each a shifted, zero-padded, strided slice of the NDHWC input times the [Cin, Cout]
weight slice, summed in float64 by torch.  The same loops over |x|, |w| give S = sum|terms| per element and over the non-zero
masks the number of terms.  It never calls the library under test; tests/test_conv_float64_gpu.py checks it against
torch.nn.functional.conv3d and its autograd in float64 on the CPU."""
import torch
import torch.nn.functional as F

from dualvar_amd._lib import DV_F32
from tests.chains import gamma

F64 = torch.float64


def _slices(dims_out, k3, s3, tap):
    return tuple(slice(d, d + (o - 1) * s + 1, s) for d, o, s in zip(tap, dims_out, s3))


def _taps(k3):
    return [(a, b, c) for a in range(k3[0]) for b in range(k3[1]) for c in range(k3[2])]


def ref_fwd(x, w, s3, p3):
    """x [N,T,H,W,Cin], w [Cout,kt,kh,kw,Cin] float64 -> y [N,To,Ho,Wo,Cout]"""
    k3 = tuple(w.shape[1:4])
    xp = F.pad(x, (0, 0, p3[2], p3[2], p3[1], p3[1], p3[0], p3[0]))
    do = tuple((i + 2 * p - k) // s + 1 for i, k, s, p in zip(x.shape[1:4], k3, s3, p3))
    y = torch.zeros((x.shape[0],) + do + (w.shape[0],), dtype=F64, device=x.device)
    for tap in _taps(k3):
        st, sh, sw = _slices(do, k3, s3, tap)
        y += xp[:, st, sh, sw, :] @ w[:, tap[0], tap[1], tap[2], :].t()
    return y


def ref_dgrad(dy, w, xdims, s3, p3):
    """dy [N,To,Ho,Wo,Cout], w as above -> dx [N,T,H,W,Cin]: scatter over the taps"""
    k3 = tuple(w.shape[1:4])
    do = tuple(dy.shape[1:4])
    dxp = torch.zeros((dy.shape[0],) + tuple(i + 2 * p for i, p in zip(xdims, p3)) + (w.shape[4],), dtype=F64, device=dy.device)
    for tap in _taps(k3):
        st, sh, sw = _slices(do, k3, s3, tap)
        dxp[:, st, sh, sw, :] += dy @ w[:, tap[0], tap[1], tap[2], :]
    return dxp[:, p3[0]:p3[0] + xdims[0], p3[1]:p3[1] + xdims[1], p3[2]:p3[2] + xdims[2], :].contiguous()


def ref_wgrad(x, dy, k3, s3, p3):
    """-> dw [Cout,kt,kh,kw,Cin] = x_slice^T dy per tap"""
    xp = F.pad(x, (0, 0, p3[2], p3[2], p3[1], p3[1], p3[0], p3[0]))
    do = tuple(dy.shape[1:4])
    dw = torch.zeros((dy.shape[4],) + tuple(k3) + (x.shape[4],), dtype=F64, device=x.device)
    dy2 = dy.reshape(-1, dy.shape[4])
    for tap in _taps(k3):
        st, sh, sw = _slices(do, k3, s3, tap)
        dw[:, tap[0], tap[1], tap[2], :] = dy2.t() @ xp[:, st, sh, sw, :].reshape(-1, x.shape[4])
    return dw


def fold_adds(c, mode):
    """fp32 additions that follow the accumulator: the 4-wave fold of the K-split kernel; the slab additions and `+=` of dw"""
    if mode == 'wgrad':
        return (c.wgrad.splits if c.wgrad.splits > 1 else 0) + 1
    r = c.fwd if mode == 'fwd' else c.dgrad
    return 3 if r.path == 'KS' else 0


def gauss_bound(c, mode, S, cnt, ref, extra_adds=0):
    """the bound (B) of tests/test_conv_float64_gpu.py for a row c of tests/conv_cases.py: S = sum|terms|, cnt the number of
    terms per element"""
    if c.dtype == DV_F32:
        n = 6 * cnt + fold_adds(c, mode) + extra_adds
        d = 2.0 ** -23 if mode == 'wgrad' else 2.0 ** -24
        return gamma((n - 1).clamp_min(0)) * (1 + 2.0 ** -7) * S + d * S
    n = cnt + fold_adds(c, mode) + extra_adds
    b = gamma((n - 1).clamp_min(0)) * S
    return b if mode == 'wgrad' else b + 2.0 ** -8 * (ref.abs() + b)
