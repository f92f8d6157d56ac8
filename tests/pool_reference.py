"""Float64 references of MaxPool3d on the CPU: the forward's values and first-maximum taps from F.max_pool3d, and the
backward's sum in ascending tap order (in float64: the exact reference; in float32: the kernels' promised sum)."""
import torch
import torch.nn.functional as F

from tests import pool_cases as T


def ref_pool_fwd(x5, c):
    """x5 [N, T, H, W, CP] float64 (CPU) -> pooled values [N, To, Ho, Wo, CP] and the tap (dt*kh + dh)*kw + dw of the first
    maximum in (t, h, w) scan order, from F.max_pool3d's flat input index"""
    y, flat = F.max_pool3d(x5.permute(0, 4, 1, 2, 3).contiguous(), c.k, c.s, c.p, return_indices=True)
    To, Ho, Wo = y.shape[2:]
    t, h, w = flat // (c.H * c.W), (flat // c.W) % c.H, flat % c.W
    ar = lambda n, s, p: torch.arange(n) * s - p      # noqa: E731
    dt = t - ar(To, c.s[0], c.p[0]).view(1, 1, To, 1, 1)
    dh = h - ar(Ho, c.s[1], c.p[1]).view(1, 1, 1, Ho, 1)
    dw = w - ar(Wo, c.s[2], c.p[2]).view(1, 1, 1, 1, Wo)
    assert bool(((dt >= 0) & (dt < c.k[0]) & (dh >= 0) & (dh < c.k[1]) & (dw >= 0) & (dw < c.k[2])).all())
    tap = (dt * c.k[1] + dh) * c.k[2] + dw
    return y.permute(0, 2, 3, 4, 1).contiguous(), tap.permute(0, 2, 3, 4, 1).contiguous().to(torch.uint8)


def ref_pool_bwd(gy5, tap5, c, start, acc_dtype=torch.float64):
    """dx [N, T, H, W, CP] = start + the contributions gy of the windows that chose each element, added in ASCENDING TAP ORDER
    in acc_dtype: float64 is the exact reference, float32 the kernels' promised sum (distinct windows reach an element
    through distinct taps, so the order is total).  Also the number of windows and sum |gy| per element."""
    To, Ho, Wo = T.out_dims(c)
    acc = start.to(acc_dtype).clone()
    cnt = torch.zeros(start.shape, dtype=torch.int32)
    mag = torch.zeros(start.shape, dtype=torch.float64)
    gy5 = gy5.to(acc_dtype)
    for tp in range(c.k[0] * c.k[1] * c.k[2]):
        dt, dh, dw = tp // (c.k[1] * c.k[2]), (tp // c.k[2]) % c.k[1], tp % c.k[2]
        sel = []
        for o, s, p, d, n in ((To, c.s[0], c.p[0], dt, c.T), (Ho, c.s[1], c.p[1], dh, c.H), (Wo, c.s[2], c.p[2], dw, c.W)):
            i = torch.arange(o) * s - p + d
            sel.append((i >= 0) & (i < n))
        ot, oh, ow = (m.nonzero().flatten() for m in sel)
        if not (len(ot) and len(oh) and len(ow)):
            continue
        it, ih, iw = ot * c.s[0] - c.p[0] + dt, oh * c.s[1] - c.p[1] + dh, ow * c.s[2] - c.p[2] + dw
        O = (slice(None), ot[:, None, None], oh[None, :, None], ow[None, None, :])
        I = (slice(None), it[:, None, None], ih[None, :, None], iw[None, None, :])
        hit = tap5[O] == tp
        contrib = torch.where(hit, gy5[O], torch.zeros((), dtype=acc_dtype))
        add = torch.zeros(start.shape, dtype=acc_dtype)
        add[I] = contrib
        acc = torch.where(add != 0, acc + add, acc)        # (an element no window chose keeps its bits, -0.0 included)
        c1 = torch.zeros(start.shape, dtype=torch.int32)
        c1[I] = hit.to(torch.int32)
        cnt += c1
        mag += add.double().abs()
    return acc, cnt, mag
