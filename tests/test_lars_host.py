"""CPU: the host side of dualvar_amd.optim.LARS -- argument validation of dv_lars_norms / dv_lars_step (refused before any
launch, so safe without a device), the segment table and block map built from a ParamStore, and the state_dict format.
(Header <-> ctypes <-> .so agreement of the new entries is tests/test_abi_and_host.py::test_library_exports_every_declared_symbol.)"""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

ADAPT, DECAY = 1, 2


def test_lars_argument_validation_without_gpu():
    from dualvar_amd import _lib
    lib = _lib.load()
    assert lib.dv_lars_chunk() > 0 and lib.dv_lars_chunk() % 8 == 0
    assert C.sizeof(_lib.LarsSeg) == 32 and (_lib.DV_LARS_ADAPT, _lib.DV_LARS_DECAY) == (ADAPT, DECAY)
    ok = 4096                                                    # a 16-byte aligned address that is never dereferenced
    norms = dict(p=ok, g=ok, segs=ok, block_seg=ok, n_segs=1, total_blocks=1, wd=0.0, gs=1.0, partials=ok, stream=0)
    step = dict(p=ok, g=ok, buf=ok, segs=ok, block_seg=ok, n_segs=1, total_blocks=1, lr=0.1, mu=0.9, wd=0.0, eta=1e-3, gs=1.0,
                partials=ok, copy_dtype=0, p_copy=0, q_out=0, stream=0)
    for fn, good, ptrs in ((lib.dv_lars_norms, norms, ('p', 'g', 'segs', 'block_seg', 'partials')),
                           (lib.dv_lars_step, step, ('p', 'g', 'buf', 'segs', 'block_seg', 'partials'))):
        for k in ptrs:
            assert fn(*dict(good, **{k: 0}).values()) == -1, k                      # DV_EINVAL
        for k in ('n_segs', 'total_blocks'):
            for v in (0, -3):
                assert fn(*dict(good, **{k: v}).values()) == -1, (k, v)
        for k in ('p', 'g') + (('buf',) if 'buf' in good else ()):
            assert fn(*dict(good, **{k: ok + 4}).values()) == -2, k                 # DV_EALIGN
    # invalid AND misaligned: still refused
    assert lib.dv_lars_step(*dict(step, p=ok + 4, n_segs=0).values()) < 0


def test_lars_seg_mirror_matches_the_header(tmp_path):
    """_lib.LarsSeg against sizeof / offsetof of struct dv_lars_seg as a C compiler lays out include/dualvar_hip.h"""
    from dualvar_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'no host C compiler'
    fields = [f[0] for f in _lib.LarsSeg._fields_]
    assert fields == ['off', 'n', 'flags', 'first_block', 'n_blocks', 'pad']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dualvar_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(struct dv_lars_seg));']
    lines += [f'  printf("%zu\\n", offsetof(struct dv_lars_seg, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    (tmp_path / 'probe.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'probe')
    subprocess.run([cc, '-std=c11', '-I', os.path.join(root, 'include'), str(tmp_path / 'probe.c'), '-o', exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.LarsSeg)] + [getattr(_lib.LarsSeg, f).offset for f in fields] == [32, 0, 8, 16, 20, 24, 28]


def _models():
    from dualvar_amd import model as M
    from dualvar_amd.model import LinearClassifier
    from dualvar_amd.ops import DV_F32
    torch.manual_seed(0)
    a = M.SimCLR_TimeSeriesV4('r21d', 128, 0.07, False)
    b = LinearClassifier(num_class=10, network='r3d', use_dropout=True, use_l2_norm=True, use_final_bn=True)
    for n_, p_ in b.named_parameters():
        if 'backbone' in n_:
            p_.requires_grad = False
    for m in (a, b):
        for st in m.stores():
            st.materialize(torch.device('cpu'), DV_F32)
    return a, b


@pytest.fixture(scope='module')
def models():
    return _models()


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('exclude_vec', [True, False])
def test_lars_segment_table(models, which, exclude_vec):
    from dualvar_amd import _lib
    from dualvar_amd.optim import LARS
    m = models[which]
    chunk = _lib.load().dv_lars_chunk()
    params = [p for p in m.parameters() if p.requires_grad]
    opt = LARS([{'params': [p]} for p in params], lr=0.1, weight_decay=1e-4, exclude_vec=exclude_vec, stores=m.stores())
    seen = 0
    for st in m.stores():
        segs = opt.segments(st)
        trainable = [s for s in st.slots if s.tensor.requires_grad]
        frozen = [s for s in st.slots if not s.tensor.requires_grad]
        assert [e[0] for e in segs] == trainable                               # one per trainable slot, none for a frozen one
        assert (which == 1) == bool(frozen)
        end, first = 0, 0
        for s, off, n, flags, fb, nb in segs:
            assert off == s.off and off % 8 == 0 and off >= end and n % 8 == 0 and n >= s.size > 0
            assert off + n <= st.total
            end = off + n
            want = (ADAPT | DECAY) if (s.kind == 'conv' or not exclude_vec) else 0
            assert flags == want, (s.kind, flags)
            assert s.kind in ('conv', 'vec')
            assert fb == first and nb == (n + chunk - 1) // chunk and nb >= 1
            first += nb
        for s in frozen:                                                       # no segment reaches into a frozen slot
            assert all(off + n <= s.off or off >= s.off + s.size for _, off, n, _, _, _ in segs)
        kinds = {s.kind for s in trainable}
        assert kinds == {'conv', 'vec'}
        # the uploaded table and block map say the same
        t = opt._table(st)
        assert t.n_segs == len(segs) and t.total_blocks == first
        raw = bytes(t.segs.numpy().tobytes())
        arr = (_lib.LarsSeg * len(segs)).from_buffer_copy(raw)
        assert [(a.off, a.n, a.flags, a.first_block, a.n_blocks) for a in arr] == [e[1:] for e in segs]
        assert t.block_seg.tolist() == [i for i, e in enumerate(segs) for _ in range(e[5])]
        assert t.partials.numel() == 2 * first and t.q_out.numel() == len(segs)
        assert opt._table(st) is t                                             # cached ...
        seen += len(segs)
    assert seen == len(params)
    if which == 1:
        assert seen == 4
        # ... on the requires_grad signature: thawing a tensor rebuilds it
        st = m.stores()[0]
        t = opt._table(st)
        p0 = next(p for p in m.parameters() if not p.requires_grad)
        p0.requires_grad = True
        try:
            assert opt._table(st) is not t and opt._table(st).n_segs == 5
        finally:
            p0.requires_grad = False
    else:
        assert any(nb > 1 for st in m.stores() for *_, nb in opt.segments(st))        # tensors of more than one block


def test_lars_refuses_bad_eta_and_missing_stores(models):
    from dualvar_amd.optim import LARS
    m = models[1]
    params = [p for p in m.parameters() if p.requires_grad]
    for eta in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='eta'):
            LARS(params, lr=0.1, eta=eta, stores=m.stores())
    with pytest.raises(ValueError, match='stores='):
        LARS(params, lr=0.1)


def test_lars_state_dict_is_torch_sgd_format(models):
    """the momentum buffer has SGD's meaning: torch.optim.SGD loads our state_dict (its groups tolerate the two extra keys) and
    ours loads torch's"""
    from dualvar_amd.optim import LARS
    m = models[1]
    params = [p for p in m.parameters() if p.requires_grad]
    opt = LARS([{'params': [p]} for p in params], lr=0.2, momentum=0.9, weight_decay=1e-4, eta=2e-3, exclude_vec=False, stores=m.stores())
    g = torch.Generator().manual_seed(1)
    for i, v in opt._momentum_views():
        v.copy_(torch.randn(v.shape, generator=g))
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and len(sd['state']) == len(params) == len(sd['param_groups'])
    assert all(gr['eta'] == 2e-3 and gr['exclude_vec'] is False and gr['lr'] == 0.2 for gr in sd['param_groups'])
    assert sd['param_groups'][3]['params'] == [3]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.SGD([{'params': [q]} for q in twins], lr=0.5, momentum=0.9)
    topt.load_state_dict(sd)
    views = dict(opt._momentum_views())
    for i, q in enumerate(twins):
        assert torch.equal(topt.state[q]['momentum_buffer'], views[i])
    assert topt.param_groups[0]['lr'] == 0.2 and topt.param_groups[0]['weight_decay'] == 1e-4
    # and back into a LARS with other settings: the groups' values travel, eta and exclude_vec included
    opt2 = LARS([{'params': [p]} for p in params], lr=0.7, eta=5e-3, stores=m.stores())
    before = {i: v.clone() for i, v in views.items()}
    assert opt2.load_state_dict(topt.state_dict()) == len(params)
    assert opt2.param_groups[0]['eta'] == 2e-3 and opt2.param_groups[0]['exclude_vec'] is False and opt2.param_groups[0]['lr'] == 0.2
    for i, v in opt2._momentum_views():
        assert torch.equal(v, before[i])
    # trust_ratios() before any step: 1 for every stepped tensor, keyed by the flat parameter index
    assert opt.trust_ratios() == [(i, 1.0) for i in range(len(params))]
