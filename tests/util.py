"""Shared test helpers (not the product)."""
import ctypes
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CLIP = dict(T=8, H=112, W=112)


def header_functions(header):
    """include/<header> -> (its text, {entry: (return type, [argument declarations])}) of the dv_* entries it declares"""
    hdr = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|int64_t)\s+(dv_\w+)\s*\((.*?)\)\s*;', src, flags=re.S):
        out[m.group(1)] = (m.group(0).split()[0], [a.strip() for a in m.group(2).split(',') if a.strip() and a.strip() != 'void'])
    return hdr, out


def _ctype_matches(typ, arg):
    """the ctypes type of a table against one argument declaration of the header"""
    if '*' in arg:
        return typ is ctypes.c_void_p or issubclass(typ, ctypes._Pointer)
    for word, want in (('int64_t', ctypes.c_int64), ('double', ctypes.c_double), ('float', ctypes.c_float)):
        if arg.startswith(word):
            return typ is want
    return typ is ctypes.c_int32


def check_header_binding(header):
    """include/<header>, its table in _lib.HEADERS and the loaded library agree: the same entries, each exported, with the same
    argument count and, per argument, the ctypes type its declaration asks for (a pointer: c_void_p or a POINTER type; int64_t,
    double, float: their ctypes; any other integer: c_int32); argtypes and restype are bound as the table and the declared
    return type say, and RETURNS_INT64 lists exactly the int64_t entries.  -> (the header's text, its declarations)"""
    from dualvar_amd import _lib
    table = _lib.HEADERS[header]
    hdr, decl = header_functions(header)
    assert set(decl) == set(table), (header, sorted(set(decl) ^ set(table)))
    lib = _lib.load()
    for name, (ret, args) in decl.items():
        assert hasattr(lib, name), '%s declared in %s but not exported' % (name, header)
        assert len(table[name]) == len(args), (name, len(table[name]), args)
        for typ, arg in zip(table[name], args):
            assert _ctype_matches(typ, arg), (name, arg, typ)
        fn = getattr(lib, name)
        assert fn.argtypes == table[name], name
        assert fn.restype is (ctypes.c_int64 if ret == 'int64_t' else ctypes.c_int), name
        assert (name in _lib.RETURNS_INT64) == (ret == 'int64_t'), name
    return hdr, decl


def gold(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def rel_err(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) + 1e-12))


def _hue_matches(q, want_u8):
    """floor(255 * x) == the reference's uint8 result; a float within rounding of an integer may truncate either way"""
    diff = np.abs(np.floor(q) - want_u8.astype(np.float64))
    near = np.abs(q - np.round(q)) < 2e-3
    return int(((diff > 0) & ~((diff <= 1) & near)).sum()), int(((diff > 0) & near).sum())


def grad_summary(model, P):
    sd = model.state_dict(keep_vars=True)
    out = {}
    for key in sorted(P.canonical_groups(model)):
        t = sd[key]
        if getattr(t, 'grad', None) is not None:
            g = t.grad.double()
            out[key] = np.array([g.abs().sum().item(), g.sum().item()])
    return out


def param_checksum(model, P):
    sd = model.state_dict()
    return {k: np.array([sd[k].double().abs().sum().item(), sd[k].double().sum().item()])
            for k in sorted(P.canonical_groups(model)) if sd[k].dtype.is_floating_point}


def total_loss(ret):
    """pretrain.py:402-445: clip loss + every other '*loss' entry."""
    loss = 0
    if 'clip_contrast_loss' in ret:
        loss = ret['clip_contrast_loss']
    for key in ret:
        if 'loss' in key and 'clip' not in key:
            loss = loss + ret[key]
    return loss
