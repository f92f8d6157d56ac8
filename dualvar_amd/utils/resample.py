"""PIL-exact Scale on the GPU: the host side of dv_resample_u8 (include/dualvar_hip.h).

The reference scales every decoded frame with `A.Scale((128, 171))` (utils/augmentation.py:125-146), i.e. PIL
`Image.resize((128, 171), BICUBIC)`: 128 columns x 171 rows.  Pillow's resample (src/libImaging/Resample.c) computes, per
output column (row), a coefficient table in float64 -- `precompute_coeffs` -- and quantises it to 22-bit integers
(`normalize_coeffs_8bpc`); the pixels are then pure int32 arithmetic.  `coeffs` below restates that float64 code step for
step, so the integer kernel reproduces PIL byte for byte; `resize_u8` is a numpy mirror of the kernel for the tests.

Tables are laid out for the kernel as {in, out, ksize, 0} followed by `out` entries {xmin, n, w[ksize]} (int32)."""
import functools

import numpy as np

PRECISION_BITS = 22
MAX_KSIZE = 32                                                    # DV_RESAMPLE_MAX_KSIZE
DESC = np.dtype([('src_offset', '<i8'), ('Hs', '<i4'), ('Ws', '<i4'), ('h_coef', '<i4'), ('v_coef', '<i4')])   # dv_resample_desc
SUPPORT = {'bicubic': 2.0, 'bilinear': 1.0}


def _bicubic(x):                    # Resample.c: bicubic_filter, a = -0.5
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(in_size, out_size, filter='bicubic'):
    """precompute_coeffs + normalize_coeffs_8bpc for a whole axis (box = [0, in_size)) -> (ksize, xmin[out], n[out],
    w[out, ksize] int32); the arrays are shared through the cache and must not be written"""
    if in_size <= 0 or out_size <= 0:
        raise ValueError('sizes must be positive, got %d -> %d' % (in_size, out_size))
    fn = {'bicubic': _bicubic, 'bilinear': _bilinear}[filter]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = SUPPORT[filter] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmins = np.zeros(out_size, np.int32)
    ns = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            w[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins[xx], ns[xx] = xmin, xmax
    for a in (xmins, ns, w):
        a.setflags(write=False)
    return ksize, xmins, ns, w


@functools.lru_cache(maxsize=None)
def table_words(in_size, out_size, filter='bicubic'):
    """one coefficient table in the kernel's layout (int32 words)"""
    ksize, xmin, n, w = coeffs(in_size, out_size, filter)
    if ksize > MAX_KSIZE:
        raise ValueError('%d -> %d needs %d taps, the kernel takes at most %d' % (in_size, out_size, ksize, MAX_KSIZE))
    body = np.concatenate([xmin[:, None], n[:, None], w], axis=1)
    t = np.concatenate([np.array([in_size, out_size, ksize, 0], np.int32), body.reshape(-1)]).astype(np.int32)
    t.setflags(write=False)
    return t


def _pass(a, axis_len_out, table, axis):
    """one pass of the integer mirror over `axis` (1 = columns, 0 = rows) of a [H, W, 3] uint8 array"""
    ksize, xmin, n, w = table
    x = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((axis_len_out,) + x.shape[1:], np.uint8)
    for o in range(axis_len_out):
        acc = np.full(x.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(n[o]):
            acc += x[xmin[o] + k] * int(w[o, k])
        acc = acc.astype(np.int32).astype(np.int64)                     # Pillow accumulates in INT32
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, size, filter='bicubic'):
    """numpy mirror of dv_resample_u8 (and of PIL's Image.resize): img uint8 [Hs, Ws, 3] -> [Ho, Wo, 3]; size = (Ho, Wo)"""
    Ho, Wo = size
    Hs, Ws = img.shape[:2]
    out = np.ascontiguousarray(img)
    if Wo != Ws:
        out = _pass(out, Wo, coeffs(Ws, Wo, filter), 1)
    if Ho != Hs:
        out = _pass(out, Ho, coeffs(Hs, Ho, filter), 0)
    return out.copy() if out is img else out


def pack(frames, size, filter='bicubic'):
    """decoded frames (uint8 [Hs_i, Ws_i, 3], any mix of sizes) -> (src uint8 [bytes], desc DESC[n], coef int32[words]): every
    frame at a 16-byte aligned offset of one buffer, one descriptor per frame, each distinct coefficient table once"""
    Ho, Wo = size
    offs, pos = [], 0
    for f in frames:
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError('frames must be uint8 [H, W, 3], got %s %s' % (f.dtype, f.shape))
        offs.append(pos)
        pos += (f.nbytes + 15) // 16 * 16
    src = np.zeros(max(pos, 16), np.uint8)
    desc = np.zeros(len(frames), DESC)
    tables, words = {}, []

    def table(in_size, out_size):
        if in_size == out_size:
            return -1                                     # Pillow's skip rule: that pass does not run
        key = (in_size, out_size)
        if key not in tables:
            tables[key] = sum(len(t) for t in words)
            words.append(table_words(in_size, out_size, filter))
        return tables[key]

    for i, (f, o) in enumerate(zip(frames, offs)):
        src[o:o + f.nbytes] = f.reshape(-1)
        desc[i] = (o, f.shape[0], f.shape[1], table(f.shape[1], Wo), table(f.shape[0], Ho))
    coef = np.concatenate(words).astype(np.int32) if words else np.zeros(4, np.int32)
    return src, desc, coef


def resample_u8(src, desc, coef, host_desc, host_coef, size, out=None):
    """dv_resample_u8 on the current stream: src uint8 device tensor, desc / coef device tensors (any dtype, the bytes of the
    DESC / int32 tables), host_desc / host_coef the same tables as numpy arrays (validated by the entry) -> uint8 [n, Ho, Wo, 3]"""
    import torch
    from .. import _lib as L
    from ..ops import stream_ptr
    Ho, Wo = size
    n = len(host_desc)
    host_desc = np.ascontiguousarray(host_desc, dtype=DESC)
    host_coef = np.ascontiguousarray(host_coef, dtype=np.int32)
    if desc.numel() * desc.element_size() != host_desc.nbytes or coef.numel() * coef.element_size() != host_coef.nbytes:
        raise ValueError('device and host resample tables differ in size')
    if out is None:
        out = torch.empty((n, Ho, Wo, 3), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n * Ho * Wo * 3:
        raise ValueError('out must be a contiguous uint8 tensor of at least %d bytes' % (n * Ho * Wo * 3))
    lib = L.load()
    L.check(lib.dv_resample_u8(src.data_ptr(), src.numel(), desc.data_ptr(), host_desc.ctypes.data, n, coef.data_ptr(),
                               host_coef.ctypes.data, host_coef.size, out.data_ptr(), Ho, Wo, stream_ptr()), 'dv_resample_u8')
    return out
