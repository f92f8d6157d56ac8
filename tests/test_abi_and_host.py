"""CPU: the C-ABI library loads and exports every symbol include/dualvar_hip.h declares (no compute calls),
the ctypes table matches the header, and the host-side logic (parameter arenas, plan bookkeeping,
fail-loudly behaviour, CLI) works without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import check_header_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from dualvar_amd import _lib
    lib = _lib.load()
    hdr, decl = check_header_binding('dualvar_hip.h')
    assert len(decl) >= 35 and _lib.HEADERS['dualvar_hip.h'] is _lib.SIGNATURES
    declared = int(re.search(r'#define\s+DV_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert lib.dv_abi_version() == declared == _lib.ABI_VERSION >= 2


def test_binding_tables_are_disjoint_and_cover_every_header():
    """_lib.HEADERS lists exactly the headers of include/, and no entry is declared in two of its tables (each header's own
    test file checks its table against the header with tests/util.py check_header_binding)"""
    from dualvar_amd import _lib
    assert set(_lib.HEADERS) == {f for f in os.listdir(os.path.join(ROOT, 'include')) if f.endswith('.h')}
    tables = list(_lib.HEADERS.items())
    for i, (ha, a) in enumerate(tables):
        for hb, b in tables[i + 1:]:
            assert not set(a) & set(b), (ha, hb, sorted(set(a) & set(b)))
    assert sum(len(t) for _, t in tables) == len({n for _, t in tables for n in t})


def test_no_kernel_of_the_library_spills():
    """Every kernel of libdualvar_hip.so keeps its working set in registers: the build keeps hipcc's resource report next to
    each object (dualvar_amd/build.py: csrc/<name>.res) and any `ScratchSize > 0` fails here.  Round 3 shipped two BatchNorm
    backward reduce kernels that spilled 112 B per lane after an unroll change (bf16 leg -4.4 %, traffic 1.08x -> 1.55x)
    and nobody saw it."""
    from dualvar_amd import build as B
    B.build_lib()
    seen = 0
    for src in B.SOURCES:
        assert os.path.exists(B.res_path(src)), f'no resource report for {src}'
        rows = B.parse_resources(open(B.res_path(src)).read())
        assert rows, f'empty resource report for {src}'
        for r in rows:
            assert int(r.get('ScratchSize', '0')) == 0, f"{src}: {r['name']} spills {r['ScratchSize']} B/lane"
            seen += 1
    assert seen >= 250          # conv 170+, elementwise 80+, loss, augment


def test_argument_validation_without_gpu():
    """rejected arguments return DV_E* before anything is launched, so this is safe on a CPU-only host"""
    from dualvar_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc()
    assert lib.dv_conv3d_fwd(None, 0, 0, 0, 0, 0, 0) == -1
    d.dtype = 7
    assert lib.dv_conv3d_stat_tiles(None) == -1
    assert lib.dv_bn_apply(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == -1
    assert lib.dv_gemm_f32(0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0) == -1


def test_product_fails_loudly_without_gpu():
    from dualvar_amd import _lib
    from dualvar_amd.backbone import select_backbone
    from dualvar_amd import functional as DF
    m, param = select_backbone('r3d')
    assert param == {'feature_size': 512}
    with pytest.raises(_lib.DualVarHipError):
        m(torch.zeros(1, 3, 8, 32, 32))
    with pytest.raises(_lib.DualVarHipError):
        DF.l2_normalize(torch.zeros(2, 8))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.DualVarHipError):
            _lib.require_device()


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'dualvar_amd')):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M), f
    assert not re.search(r'^\s*(from|import)\s+oracle\b', open(os.path.join(ROOT, 'pretrain.py')).read(), flags=re.M)


@pytest.mark.parametrize('net', ['s3dg', 'r21d', 'r50'])
def test_state_dict_matches_oracle_names(net):
    from dualvar_amd.backbone import select_backbone
    from oracle import torch_ref as O
    a, _ = select_backbone(net)
    b, _ = O.select_backbone(net)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(sa[k].shape == sb[k].shape for k in sa)


def test_param_store_arena_views_cpu():
    """nn.Parameters become strided views of one [Cout][taps][Cin_pad] arena; state_dict round-trips."""
    from dualvar_amd import model as M
    from dualvar_amd.ops import DV_F32
    from oracle import procedural as P
    m = M.SimCLR_TimeSeriesV4('r21d', 128, 0.07, False)
    P.procedural_init(m)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    st = m.store
    st.materialize(torch.device('cpu'), DV_F32)
    assert st.ready(torch.device('cpu'), DV_F32)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    w = m.encoder_q[0].conv2.block1.conv1.spatial_conv.weight          # [144, 64, 1, 3, 3]
    s = st.slot(w)
    assert w.data_ptr() == st.master.data_ptr() + 4 * s.off and w.stride(1) == 1
    packed = st.master[s.off:s.off + s.size].view(s.Cout, s.taps, s.cin_pitch)
    assert torch.equal(packed[:, :, :s.Cin], w.detach().reshape(s.Cout, s.Cin, s.taps).permute(0, 2, 1))
    # odd channel count (83) is zero padded to 88 in the consumer's weight rows
    w2 = m.encoder_q[0].conv1.temporal_conv.weight                     # [64, 83, 3, 1, 1]
    s2 = st.slot(w2)
    assert s2.cin_pitch == 88 and float(st.master[s2.off:s2.off + s2.size].view(64, 3, 88)[:, :, 83:].abs().max()) == 0
    # gradients are views of the twin arena; an in-place load keeps the aliasing
    assert w.grad is not None and w.grad.data_ptr() == st.grad.data_ptr() + 4 * s.off
    m.load_state_dict(before)
    assert st.ready(torch.device('cpu'), DV_F32)
    # S3D registers its stem twice: one slot per tensor
    m2 = M.SimCLR_Naked('s3dg', 128, 0.07, False)
    assert len(m2.store.slots) == len(list(m2.parameters())) == 307
    assert sum(p.numel() for p in m2.parameters()) == 9098000 + 1024 * 1024 + 1024 + 128 * 1024 + 128


def test_moco_query_and_key_arenas_have_identical_layout():
    from dualvar_amd import model as M
    from dualvar_amd.ops import DV_F32
    m = M.MoCo_TimeSeriesV4('r3d', 128, 64, 0.999, 0.07, False)
    m.store.materialize(torch.device('cpu'), DV_F32)
    m.store_k.materialize(torch.device('cpu'), DV_F32)
    assert m.store.total == m.store_k.total
    assert [(a.off, a.size) for a in m.store.slots] == [(b.off, b.size) for b in m.store_k.slots]
    assert torch.equal(m.store.master, m.store_k.master)               # key encoder starts as a copy
    assert all(not p.requires_grad for p in m.encoder_k.parameters())


def test_pretrain_cli_parses_reference_flags():
    import pretrain
    a = pretrain.parse_args(['--net', 's3dg', '--model', 'simclr_timeseriesv4', '--series_mode', 'clip-sr', '--moco-k', '16384',
                             '--seq_len', '8', '--num_seq', '3', '--batch_size', '8', '--lr', '0.003', '--wd', '1e-4',
                             '--local_rank', '0', '--schedule', '120', '160'])
    assert a.mode == 'clip-sr' and a.moco_k == 16384 and a.n_proto == 1 and a.schedule == [120, 160]
    a.distributed = False
    m = pretrain.get_model(a)
    assert type(m).__name__ == 'SimCLR_TimeSeriesV4' and not m.with_tc
    ds = pretrain.SyntheticClips(a, 4)
    assert ds[0]['seq'].shape == (3, 24, 112, 112)


def test_bench_cli_and_bucket_ranges():
    from dualvar_amd.parallel import bucket_ranges
    r = bucket_ranges(100, 32)
    assert r[0] == (68, 100) and r[-1] == (0, 4) and sum(b - a for a, b in r) == 100
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True)
    assert out.returncode == 0 and '--gpus' in out.stdout and '--warmup' in out.stdout


def test_checkpoint_interchange_with_reference_format(tmp_path):
    """a reference-format checkpoint ({'epoch','state_dict',...}, reference key names) loads into
    the HIP model and back, also after the parameters have been moved into the arena."""
    import torch
    from dualvar_amd import model as M
    from dualvar_amd.ops import DV_F32
    from dualvar_amd.utils.utils import neq_load_customized, save_checkpoint
    from oracle import procedural as P, torch_ref as O
    ref = O.SimCLR_TimeSeriesV4('s3dg', 128, 0.07, False)
    P.procedural_init(ref)
    ck = {'epoch': 3, 'state_dict': ref.state_dict(), 'best_acc': 0.0, 'iteration': 7}
    mine = M.SimCLR_TimeSeriesV4('s3dg', 128, 0.07, False)
    mine.store.materialize(torch.device('cpu'), DV_F32)
    mine.load_state_dict(ck['state_dict'])                       # strict: identical key set
    assert mine.store.ready(torch.device('cpu'), DV_F32)         # still views of the arena
    for k, v in ref.state_dict().items():
        assert torch.equal(mine.state_dict()[k], v), k
    path = str(tmp_path / 'model' / 'epoch3.pth.tar')
    os.makedirs(os.path.dirname(path))
    save_checkpoint({'epoch': 4, 'state_dict': mine.state_dict(), 'best_acc': 0.0, 'iteration': 8}, filename=path)
    back = torch.load(path, map_location='cpu', weights_only=True)
    assert back['state_dict']['encoder_q.0.Conv_1a.conv1.weight'].is_contiguous()
    ref2 = O.SimCLR_TimeSeriesV4('s3dg', 128, 0.07, False)
    ref2.load_state_dict(back['state_dict'])
    # the downstream rename of classifier.py:362-366 (encoder_q.0. -> backbone.) finds its keys
    assert any(k.startswith('encoder_q.0.') for k in back['state_dict'])
    # partial load helper
    sub = {k: v for k, v in back['state_dict'].items() if 'series_proj_head' not in k}
    neq_load_customized(M.SimCLR_TimeSeriesV4('s3dg', 128, 0.07, False), sub, verbose=False)


def test_pretrain_host_flags_follow_the_reference():
    """pretrain.py:225 / :290-292,343 -- who logs and saves, and where a resumed run starts"""
    import importlib
    pt = importlib.import_module('pretrain')
    assert pt.is_printing_rank(False, 0) and pt.is_printing_rank(True, 0) and not pt.is_printing_rank(True, 3)
    # a single-process run on --gpu 1 still logs and saves its checkpoints (args.rank is 0 there, but so would any rank be)
    assert pt.is_printing_rank(False, 5)
    # the reference saves 'epoch' = the epoch just finished and resumes at the next one
    assert pt.resume_position({'epoch': 4, 'iteration': 77, 'best_acc': 0.5}) == (5, 77, 0.5)
    assert pt.resume_position({'epoch': 0}) == (1, 1, 0.0)


def test_optimizer_state_interchange_with_torch_sgd():
    """The checkpoint's 'optimizer' entry is torch.optim.SGD's state_dict in the reference (pretrain.py:343-349): ours
    has the same format, a torch state loads into the momentum arena through the parameter views, and back."""
    import warnings
    import torch
    from dualvar_amd import model as M
    from dualvar_amd.ops import DV_F32
    from dualvar_amd.optim import SGD
    from oracle import procedural as P, torch_ref as O
    ref = O.SimCLR_Naked('r3d', 128, 0.07, False)
    P.procedural_init(ref)
    rparams = [p for p in ref.parameters() if p.requires_grad]
    ropt = torch.optim.SGD([{'params': [p]} for p in rparams], lr=0.003, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(5)
    for p in rparams:
        p.grad = torch.randn(p.shape, generator=g)
    ropt.step()                                              # creates the momentum buffers
    ropt.param_groups[0]['lr'] = 0.0003                      # e.g. after a MultiStepLR milestone
    mine = M.SimCLR_Naked('r3d', 128, 0.07, False)
    for st in mine.stores():
        st.materialize(torch.device('cpu'), DV_F32)
    mparams = [p for p in mine.parameters() if p.requires_grad]
    assert [tuple(p.shape) for p in mparams] == [tuple(p.shape) for p in rparams]
    opt = SGD([{'params': [p]} for p in mparams], lr=0.003, momentum=0.9, weight_decay=1e-4, stores=mine.stores())
    assert opt.load_state_dict(ropt.state_dict()) == len(rparams)
    assert opt.param_groups[0]['lr'] == 0.0003 and opt.param_groups[1]['lr'] == 0.003
    views = dict(opt._momentum_views())
    for i, p in enumerate(rparams):
        assert torch.equal(views[i], ropt.state[p]['momentum_buffer']), i
    # ... and back: torch's SGD takes our state_dict
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and sd['param_groups'][3]['params'] == [3]
    ropt2 = torch.optim.SGD([{'params': [p]} for p in rparams], lr=0.1, momentum=0.9, weight_decay=1e-4)
    ropt2.load_state_dict(sd)
    for p in rparams:
        assert torch.equal(ropt2.state[p]['momentum_buffer'], ropt.state[p]['momentum_buffer'])
    # a state without momentum (fresh torch optimizer) is loaded with a warning, not silently
    fresh = torch.optim.SGD([{'params': [p]} for p in rparams], lr=0.1, momentum=0.9).state_dict()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        assert opt.load_state_dict(fresh) == 0
    assert any('momentum buffers restored' in str(x.message) for x in w)
    assert all(float(v.abs().sum()) == 0.0 for v in dict(opt._momentum_views()).values())


def test_backward_list_reorder_hides_syncbn_exchange_behind_weight_gradients():
    """engine.overlap_bn_exchange: wgrads issued since the previous exchange move between START and WAIT; everything
    else keeps its relative order (dgrad -> bn reduce -> START -> [wgrads] -> WAIT -> bn apply)."""
    from dualvar_amd.engine import overlap_bn_exchange

    class L_:
        def __init__(self, name, tag):
            self.name, self.tag = name, tag

    names = [('bn_bwd_reduce', 'r3'), ('syncbn_allreduce_start', 's3'), ('syncbn_allreduce_wait', 'w3'), ('bn_bwd_apply', 'a3'),
             ('conv_wgrad', 'wg3a'), ('conv_dgrad', 'dg3a'), ('conv_wgrad', 'wg3b'), ('conv_dgrad', 'dg3b'), ('maxpool_bwd', 'p'),
             ('bn_bwd_reduce', 'r2'), ('syncbn_allreduce_start', 's2'), ('syncbn_allreduce_wait', 'w2'), ('bn_bwd_apply', 'a2'),
             ('conv_wgrad', 'wg2'), ('conv_dgrad', 'dg2')]
    out = [x.tag for x in overlap_bn_exchange([L_(n, t) for n, t in names])]
    assert out == ['r3', 's3', 'w3', 'a3', 'dg3a', 'dg3b', 'p', 'r2', 's2', 'wg3a', 'wg3b', 'w2', 'a2', 'wg2', 'dg2']
    # single-GPU lists (no exchange steps) are untouched
    plain = [L_(n, t) for n, t in names if not n.startswith('syncbn')]
    assert [x.tag for x in overlap_bn_exchange(plain)] == [x.tag for x in plain]


def _run_bench(argv, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=env, timeout=timeout, cwd=ROOT)


def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher on the command line must start two ranks itself (the reference's scripts launch
    their 8 workers the same way, pretrain.py:205-220) and print n_gpus == 2 -- not silently time one rank.  --launch-check keeps
    it to the launch / rendezvous / report plumbing so that it runs on a CPU-only host; the full 2-rank bench runs in
    tests/test_distributed_gpu.py."""
    import json
    r = _run_bench(['--gpus', '2', '--launch-check'])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout.decode()
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['sum'] == 2.0


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    r = _run_bench(['--gpus', '2', '--launch-check'], {'WORLD_SIZE': '1', 'RANK': '0'})
    assert r.returncode != 0 and b'WORLD_SIZE is 1' in r.stderr


def test_bench_watchdog_names_the_stuck_phase():
    """a collective one rank never joins ends as a named phase and a non-zero exit code within the deadline, not as a silent hang"""
    r = _run_bench(['--gpus', '2', '--launch-check', '--hang-check', '3'], timeout=200)
    assert r.returncode != 0
    assert b'WATCHDOG' in r.stderr and b'launch-check all-reduce' in r.stderr
    assert not [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]


@pytest.mark.parametrize('kind,net', [('SimCLR_TimeSeriesV4', 's3dg'), ('MoCo_Naked', 'r3d')])
def test_optimizer_load_state_dict_is_all_or_nothing(kind, net):
    """A state whose k-th momentum buffer has the wrong shape must leave the optimizer untouched -- lr / param_groups and every
    momentum view as before (the reference's --resume path logs the failure and trains on, pretrain.py:287-306) -- and the
    positional mapping torch index -> arena view holds for an S3D-G model and a MoCo model as well."""
    import types
    import torch
    from dualvar_amd import model as M
    from dualvar_amd.ops import DV_F32
    from dualvar_amd.optim import SGD
    from oracle import torch_ref as O
    a = types.SimpleNamespace(shufflerank_theta=0.05)
    mk = (lambda mod: mod.SimCLR_TimeSeriesV4(net, 128, 0.07, False, args=a)) if kind.startswith('SimCLR') else \
         (lambda mod: mod.MoCo_Naked(net, 128, 256, 0.999, 0.07, False))
    torch.manual_seed(0)
    ref, mine = mk(O), mk(M)
    for st in mine.stores():
        st.materialize(torch.device('cpu'), DV_F32)
    rparams = [p for p in ref.parameters() if p.requires_grad]
    mparams = [p for p in mine.parameters() if p.requires_grad]
    assert [tuple(p.shape) for p in mparams] == [tuple(p.shape) for p in rparams]     # same order, same shapes as the reference
    ropt = torch.optim.SGD([{'params': [p]} for p in rparams], lr=0.003, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(5)
    for p in rparams:
        p.grad = torch.randn(p.shape, generator=g)
    ropt.step()
    opt = SGD([{'params': [p]} for p in mparams], lr=0.01, momentum=0.9, weight_decay=1e-4, stores=mine.stores())
    for _, v in opt._momentum_views():
        v.fill_(0.25)
    import copy
    sd = copy.deepcopy(ropt.state_dict())            # (state_dict() hands out the optimizer's own per-parameter dicts)
    k = len(rparams) // 2
    sd['state'][k]['momentum_buffer'] = torch.zeros(3, 5)                                # wrong shape in the MIDDLE
    sd['param_groups'][0]['lr'] = 123.0
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    assert opt.param_groups[0]['lr'] == 0.01
    assert all(bool((v == 0.25).all()) for _, v in opt._momentum_views()), 'a failed load must not touch the momentum'
    # the intact state maps index for index
    assert opt.load_state_dict(ropt.state_dict()) == len(rparams)
    views = dict(opt._momentum_views())
    for i, p in enumerate(rparams):
        assert torch.equal(views[i], ropt.state[p]['momentum_buffer']), i


def test_f32_exact_switch_is_parsed_like_the_library(monkeypatch):
    from dualvar_amd import _lib
    for v, want in [('1', True), ('2', True), ('01', True), ('0', False), ('', False), ('yes', False), (' 3', True)]:
        monkeypatch.setenv('DUALVAR_F32_EXACT', v)
        assert _lib.f32_exact() is want, (v, want)


def test_failed_launch_rezeroes_ticket_workspaces():
    from dualvar_amd import _lib
    t = _lib.register_ticket_workspace(torch.ones(16))
    with pytest.raises(_lib.DualVarHipError):
        _lib.check(-1, 'rejected arguments: nothing was launched')
    assert float(t.sum()) == 16.0
    with pytest.raises(_lib.DualVarHipError):
        _lib.check(700, 'a launch that failed')
    assert float(t.sum()) == 0.0


def test_overlapped_gradient_sync_refuses_a_second_backward():
    """GradSync.attach starts bucket all-reduces from inside the backward pass; a further backward into the same arena before the
    optimizer step would mix local gradients into cross-rank sums: the encoder's backward raises instead."""
    from dualvar_amd.backbone.base import _BackboneFn

    class _Store:
        _sync_started = True

    class _Plan:
        store = _Store()

    class _Ctx:
        plan = _Plan()
    with pytest.raises(RuntimeError, match='overlapped all-reduce'):
        _BackboneFn.backward(_Ctx(), None)


def test_zero_grad_rearms_an_arena_whose_overlapped_sync_was_never_finished():
    """backward (bucket all-reduces started from inside it) -> no optimizer step (exception / skipped step) -> zero_grad():
    the pending works are waited for and dropped, the flag is cleared and the next backward is accepted."""
    from dualvar_amd.engine import ParamStore
    from dualvar_amd.parallel import GradSync

    class _Work:
        waited = 0

        def wait(self):
            _Work.waited += 1
    st = ParamStore.__new__(ParamStore)
    st.grad = torch.ones(8)
    st.pending_backward = 2
    gs = GradSync.__new__(GradSync)
    gs._works, gs._stream = {id(st.grad): {0: _Work(), 4: None}}, None
    st._sync_started, st._sync_owner = True, gs
    st.zero_grad()
    assert st._sync_started is False and st.pending_backward == 2 and _Work.waited == 1
    assert gs._works == {} and float(st.grad.abs().sum()) == 0.0
    st.zero_grad()                       # idempotent


def test_ticket_workspace_registry_drops_dead_references():
    from dualvar_amd import _lib
    before = len(_lib._ticket_ws)
    for _ in range(200):
        _lib.register_ticket_workspace(torch.zeros(1))          # freed at once
    assert len(_lib._ticket_ws) <= before + 130


def test_worker_side_augmentation_rows_equal_the_in_line_build():
    """pretrain.py --dataset synthetic-frames: the DataLoader workers draw every view's augmentation and ship it as table rows; the
    collate moves the rows' source-frame indices to the sample's place in the batch.  Same seeds, same order of draws ->
    byte-identical tables to FrameBatch.build on the stacked frames (the in-line path the GPU fixtures pin)."""
    import random
    import pretrain
    from dualvar_amd.utils.transforms import FrameBatch
    a = pretrain.parse_args(['--net', 's3dg', '--model', 'simclr_naked', '--batch_size', '4', '--seq_len', '8', '--img_dim', '112',
                             '--dataset', 'synthetic-frames', '--rand_flip'])
    tr = pretrain.gpu_transform(a)
    ds = pretrain.SyntheticFrames(a, 16, transform=tr, views=2)
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    batch = pretrain.collate_frames([ds[i] for i in range(4)])
    fr = batch['frames']
    assert fr.shape == (4, 8, 128, 171, 3) and fr.dtype == torch.uint8
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    ref = FrameBatch.build(fr.view(-1, 128, 171, 3), [list(range(b * 8, b * 8 + 8)) for b in range(4)], tr, (112, 112), views=2, device='cpu')
    assert torch.equal(batch['aug'].view(-1), ref.table.view(-1))
    if ref.blur is not None:
        assert batch['has_blur'] and torch.equal(batch['blur'].view(-1), ref.blur.view(-1))
    else:
        assert not batch['has_blur']
    got = FrameBatch(fr.view(-1, 128, 171, 3), batch['aug'].view(-1), (4, 2, 3, 8, 112, 112),
                     blur=batch['blur'].view(-1) if batch['has_blur'] else None)
    assert tuple(got.shape) == tuple(ref.shape)


def test_kernel_choice_queries_on_the_host():
    """dv_conv3d_ksplit_cols / dv_conv3d_tile_shape are pure host logic: the few-row layers of S3D-G at the headline batch
    (128 clips of 8x112x112: Mixed_5 = 1 152 rows, Mixed_4 = 12 544 rows) go to the K-split kernel when K is long, the big layers
    do not, and neither do the cases the kernel does not implement (bf16, no pre-split weights, strided, short K)."""
    import ctypes as C
    from dualvar_amd import _lib as L
    lib = L.load()

    def desc(N, T, H, W, Cin, Cout, k, s=(1, 1, 1), p=None, dtype=L.DV_F32, flags=L.DV_W3):
        p = p if p is not None else tuple(kk // 2 for kk in k)
        d = L.ConvDesc()
        d.dtype, d.N, d.Ti, d.Hi, d.Wi, d.Cin = dtype, N, T, H, W, Cin
        d.To, d.Ho, d.Wo = [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((T, H, W), k, s, p)]
        d.Cout = Cout
        d.kt, d.kh, d.kw = k
        d.st, d.sh, d.sw = s
        d.pt, d.ph, d.pw = p
        d.cin_pitch, d.cout_pitch = (Cin + 7) & ~7, (Cout + 7) & ~7
        d.ldx, d.ldy, d.flags = d.cin_pitch, d.cout_pitch, flags
        return d

    ks = lambda d, dg=0: lib.dv_conv3d_ksplit_cols(C.byref(d), dg)      # noqa: E731
    m5 = desc(128, 1, 3, 3, 192, 384, (1, 3, 3))               # Mixed_5c 1x3x3: 1 152 rows, K = 1 728
    assert ks(m5, 0) == 32 and ks(m5, 1) == 32
    m5t = desc(128, 1, 3, 3, 384, 384, (3, 1, 1))              # its 3x1x1 on ONE frame: two taps trimmed, K = 384 left
    assert ks(m5t, 0) == 32
    m4 = desc(128, 2, 7, 7, 512, 64, (1, 1, 1))                # Mixed_4 entry piece: 12 544 rows, 64 columns -> the 64-column form
    assert ks(m4, 0) == 64
    assert ks(desc(128, 2, 7, 7, 160, 320, (1, 3, 3)), 0) == 0      # 12 544 rows x 320 columns: too many tiles for one round
    assert ks(desc(128, 4, 28, 28, 64, 192, (1, 3, 3)), 0) == 0     # Conv_2c: 401 408 rows
    assert ks(desc(128, 1, 3, 3, 64, 64, (3, 1, 1)), 0) == 0        # short K (after trimming: 4 tiles)
    assert ks(desc(128, 1, 3, 3, 192, 384, (1, 3, 3), dtype=L.DV_BF16, flags=0), 0) == 0
    assert ks(desc(128, 1, 3, 3, 192, 384, (1, 3, 3), flags=0), 0) == 0               # no pre-split weights
    assert ks(desc(128, 2, 6, 6, 192, 384, (1, 3, 3), s=(1, 2, 2)), 1) == 0            # strided data gradient
    r, c = C.c_int32(), C.c_int32()
    assert lib.dv_conv3d_tile_shape(C.byref(desc(128, 4, 28, 28, 64, 192, (1, 3, 3))), 0, C.byref(r), C.byref(c)) == 0
    assert (r.value, c.value) == (256, 64)

    # Every query reads the one route the launch takes.  Mixed_4's 64 -> 64 1x3x3 runs on the LDS-staged kernel, so it reports no
    # K-split column tile; over a sweep of the backbones' windows, map sizes and ragged channel counts the queries agree with
    # each other: one kernel per problem, the forward's BatchNorm partials are that kernel's tiles, and they cover M.
    tk = lambda d, dg=0: lib.dv_conv3d_tap_kind(C.byref(d), dg)       # noqa: E731
    m4s = desc(128, 2, 7, 7, 64, 64, (1, 3, 3))
    assert tk(m4s) == 1 and ks(m4s) == 0
    wins = [((1, 1, 1), (1, 1, 1)), ((1, 3, 3), (1, 1, 1)), ((3, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 1, 1)),
            ((1, 7, 7), (1, 2, 2)), ((7, 1, 1), (2, 1, 1)), ((3, 3, 3), (2, 2, 2))]
    maps = [(4, 56, 56), (4, 28, 28), (2, 14, 14), (2, 7, 7), (1, 3, 3), (8, 6, 6), (8, 56, 56)]     # (the last: the 7x1x1 stem)
    chans = [(64, 64), (64, 192), (192, 96), (20, 48), (832, 256), (512, 64), (384, 384), (160, 320)]
    descs = [desc(N, T, H, W, ci, co, k, s, dtype=dt, flags=fl)
             for dt, fl in [(L.DV_F32, 0), (L.DV_F32, L.DV_W3), (L.DV_F32, L.DV_W3 | L.DV_STATS), (L.DV_F32, L.DV_W3 | L.DV_ACCUM),
                            (L.DV_BF16, 0)]
             for N in (128, 2) for T, H, W in maps for ci, co in chans for k, s in wins]
    for N, Ho, Wo in [(128, 56, 56), (128, 28, 28), (2, 56, 56), (2, 7, 64)]:    # the pixel-pair stem form: 1x7x4, stride (1, 2, 1)
        d = desc(N, 8, 2 * Ho + 5, Wo + 3, 6, 64, (1, 7, 4), (1, 2, 1), (0, 0, 0), flags=L.DV_W3 | L.DV_STATS)
        d.cin_pitch = d.ldx = 8
        assert (d.Ho, d.Wo) == (Ho, Wo)
        descs.append(d)
    vals = lambda d: [getattr(d, f) for f, _ in d._fields_]           # noqa: E731
    seen = set()
    for d in descs:
        for dg in (0, 1):
            assert not (tk(d, dg) and ks(d, dg)), (vals(d), dg)
            seen.add((dg, tk(d, dg) != 0, ks(d, dg) != 0))
        rows, tiles = lib.dv_conv3d_tile_rows(C.byref(d)), lib.dv_conv3d_stat_tiles(C.byref(d))
        if tk(d):
            assert rows == lib.dv_conv3d_tap_rows(C.byref(d), 0), vals(d)
        M = d.N * d.To * d.Ho * d.Wo
        assert rows > 0 and 0 <= tiles * rows - M < rows, (vals(d), rows, tiles)
    assert {(0, True, False), (0, False, True), (1, True, False), (1, False, True)} <= seen      # (the sweep reaches both kernels)

    # The weight gradient has one plan as well (plan_wgrad): the tile, the row splits, the workspace and the two fused-form
    # answers are reads of it and agree with each other on every problem of the sweep (its own descriptor has no flags;
    # dv_conv3d_bn_in_ok also asks the forward, which needs the pre-split weights).
    r, c, sp = C.c_int32(), C.c_int32(), C.c_int32()
    wseen, wdone = set(), set()
    for d in descs:
        key = tuple(vals(d)[:-1])                         # (all but the flags, the descriptor's last field)
        if key in wdone:
            continue
        wdone.add(key)
        flags, d.flags = d.flags, 0
        assert lib.dv_conv3d_wgrad_tile(C.byref(d), C.byref(r), C.byref(c), C.byref(sp)) == 0, vals(d)
        tile, splits = (r.value, c.value), sp.value
        ws, bn_ok = lib.dv_conv3d_wgrad_workspace(C.byref(d)), lib.dv_conv3d_wgrad_bn_ok(C.byref(d))
        d.flags = L.DV_W3
        bn_in = lib.dv_conv3d_bn_in_ok(C.byref(d))
        d.flags = flags
        S = (d.Cout * d.kt * d.kh * d.kw * d.cin_pitch + 63) // 64 * 64
        assert splits >= 1 and ws == (splits * S * 4 if splits > 1 else 0), (vals(d), tile, splits, ws)
        if bn_ok:
            assert d.dtype == L.DV_F32 and tile in ((64, 128), (64, 224)), (vals(d), tile)
        if bn_in:
            assert tile in ((64, 192), (64, 224)), (vals(d), tile, bn_in)
        wseen.add((d.dtype, tile, bn_in, bn_ok))
    assert len(wdone) == 1572
    tiles_of = lambda dt: {t for dd, t, _, _ in wseen if dd == dt}      # noqa: E731
    assert {(128, 128), (64, 256), (128, 256), (192, 256)} <= tiles_of(L.DV_BF16)       # the bf16 DMA list ...
    assert {(128, 128), (64, 128)} <= tiles_of(L.DV_F32)                                # ... the fp32 one ...
    assert {(64, 128), (128, 64)} <= tiles_of(L.DV_BF16)      # ... conv_wgrad_kernel's two (no bf16 DMA tile is 64 x 128)
    assert {(L.DV_F32, (64, 192), 0, 0), (L.DV_F32, (64, 192), 1, 0), (L.DV_F32, (64, 224), 2, 0),
            (L.DV_F32, (64, 224), 0, 1)} <= wseen             # the LDS-staged forms, with and without their fused variants


@pytest.mark.skipif(torch.cuda.is_available(), reason='a library without the check would launch: CPU-only hosts only')
def test_single_tensor_bn_backward_refuses_mask_from_x():
    """DV_MASK_FROM_X needs the item's scale / shift: only the multi-tensor entries carry them.  The single-tensor entries
    must refuse the flag (their kernels would read scale / shift through null pointers, and the apply kernel's LDS table
    has no room for them).  Every other argument is valid, so the flag is the only reason to refuse."""
    from dualvar_amd import _lib as L
    lib = L.load()
    M, C_ = 64, 16
    p = 1 << 20                                  # any non-null, 16-byte aligned value: nothing may be dereferenced
    for fl in (L.DV_MASK_FROM_X, L.DV_MASK_FROM_X | L.DV_ACCUM):
        assert lib.dv_bn_bwd_reduce(L.DV_F32, p, C_, p, C_, p, C_, p, p, M, C_, fl, p, 1, p, None) == -1
        assert lib.dv_bn_bwd_apply(L.DV_BF16, p, C_, p, C_, p, C_, p, p, p, p, 1, 1.0 / M, 1.0, p, p, p, C_, p, C_,
                                   M, C_, fl, None) == -1
    # with DV_NO_RELU_MASK there is no mask to take from x: the flag is ignored, as in the multi-tensor kernels (not called
    # here: it would launch)


def _header_structs():
    """{name: [field, ...]} of every `typedef struct` in include/dualvar_hip.h, in declaration order"""
    src = open(os.path.join(ROOT, 'include', 'dualvar_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for m in re.finditer(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', src, flags=re.S):
        assert m.group(1) == m.group(3), m.group(0)
        fields = []
        for decl in m.group(2).split(';'):
            decl = re.sub(r'\[[^\]]*\]', '', decl.replace('*', ' ')).strip()
            if not decl:
                continue
            head, *rest = [d.strip() for d in decl.split(',')]
            fields += [head.split()[-1]] + rest
        out[m.group(1)] = fields
    return out


def test_ctypes_and_numpy_struct_mirrors_match_the_header(tmp_path):
    """The host builds the structs of include/dualvar_hip.h by hand (ctypes in dualvar_amd/_lib.py, numpy row dtypes for the
    ingest tables in dualvar_amd/utils/transforms.py).  A C probe compiled against the header prints sizeof and offsetof of
    every field; the mirrors must agree field by field, and every struct of the header must have a mirror."""
    import ctypes
    import shutil
    from dualvar_amd import _lib as L
    from dualvar_amd.utils import transforms as TR
    mirrors = {'dv_conv_desc': L.ConvDesc, 'dv_bn_reduce': L.BnReduce, 'dv_bn_bwd': L.BnBwd, 'dv_bn_in': L.BnIn,
               'dv_w3_desc': L.W3Desc, 'dv_pack_desc': L.PackDesc, 'dv_aug_frame': TR.AUG_ROW, 'dv_aug_blur': TR.AUG_BLUR,
               'dv_aug_patch': TR.AUG_PATCH, 'dv_bn_item': L.BnItem, 'dv_pool_desc': L.PoolDesc, 'dv_gemm_desc': L.GemmDesc}
    structs = _header_structs()
    assert set(structs) == set(mirrors)
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'no host C compiler'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dualvar_hip.h"', 'int main(void) {']
    for s, fields in structs.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    (tmp_path / 'probe.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'probe')
    subprocess.run([cc, '-std=c11', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'probe.c'), '-o', exe], check=True)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    for s, fields in structs.items():
        m = mirrors[s]
        if isinstance(m, np.dtype):
            names, size = list(m.names), m.itemsize
            offs = {f: m.fields[f][1] for f in names}
        else:
            names, size = [f[0] for f in m._fields_], ctypes.sizeof(m)
            offs = {f: getattr(m, f).offset for f in names}
        assert names == fields, (s, names, fields)
        assert size == got[s], (s, size, got[s])
        for f in fields:
            assert offs[f] == got[f'{s}.{f}'], (s, f, offs[f], got[f'{s}.{f}'])
    assert got['dv_bn_item'] == 256 and got['dv_aug_frame'] == 64 and got['dv_aug_patch'] == 40


def test_act_slice_refuses_misaligned_channel_offsets():
    """the multi-tensor BatchNorm and conv kernels load 16 bytes at the view's first channel: a slice must start at a multiple
    of 8 channels even when it fits inside the parent's C"""
    from dualvar_amd import ops
    a = ops.Act(torch.zeros(4, 48), 1, 1, 2, 2, 40, 48, 0, ops.DV_F32)
    s = a.slice(8, 24)
    assert (s.off, s.C, s.ld) == (8, 24, 48)
    assert a.slice(16, 32).off == 16                  # up to the end of the pitch
    with pytest.raises(AssertionError):
        a.slice(4, 8)                                 # inside C, misaligned
    with pytest.raises(AssertionError):
        a.slice(12, 24)
    with pytest.raises(AssertionError):
        a.slice(24, 32)                               # aligned, but runs past the pitch and past C


CONV_TABLE_ROWS = [
    'pw_c64_m294', 'pw_c24_m16384', 'sp3_c40_m16384', 'sp3_c128_c40_m16384', 'pw_c24_m131072', 'pw_c256_m65536', 'pw_c64_m131072',
    'rgb_stem_sp7', 'w5x7x7_c8', 'tap_sp_m12544', 'tap_tm_m12544', 'tap_sp_m50176', 'tap_sp_c192_m100352', 'tap_tm_t2', 'tap_tm_t8', 'ks32_m72', 'ks64_m6080',
    'ks_trim_t', 'ks_trim_hw', 'gemm_trim_t', 'gemm_trim_hw', 'stem_tm7_m12544', 'stem_tm7_m131072', 'pair_stem_pp',
    'pair_stem_small', 'c83_tm3', 'c144_c230_sp3', 'c1_c1_sp3', 'c40_c3_sp3', 'w1x9x9_c16', 'now3_stem_tm7', 'now3_full3_s2',
    'now3_sp3_s2_c83', 'now3_full3_s2_t1', 'now3_pw_s2', 'now3_sp3_c24', 'bf_rgb_stem', 'bf_sp3_c24', 'bf_sp3_c64',
    'bf_pw_c64_m131072', 'bf_sp3_c192_m100352', 'bf_sp3_c320_m3136', 'bf_pw_c512_m1568', 'bf_sp3_c64_m25088', 'bf_w1x9x9_c16']

CONV_TILES = ('64x32', '64x64', '64x128', '128x32', '128x64', '128x128', '256x64')
# every member the table must reach (members are derived per row by conv_cases.members from the row's literals)
CONV_REQUIRED = (
    ['%s:path:%s' % (m, p) for m in ('fwd', 'dgrad') for p in ('GEMM', 'KS', 'TAP')] +
    ['fwd:path:PP', 'dgrad:path:GEMM_CLASSES', 'dgrad:path:TAP_CLASSES'] +
    ['%s:tile:%s' % (m, t) for m in ('fwd', 'dgrad') for t in CONV_TILES] +
    ['f32:w3:generic:cp4', 'f32:w3:generic:cp8', 'f32:w3:generic:cp24', 'f32:w3:generic:cp40', 'f32:w3:generic:taps>32',
     'f32:w3:uniform-tap', 'f32:plain-split',
     'bf16:gather8', 'bf16:gather16', 'bf16:cp%32==0', 'bf16:cp%32!=0', 'bf16:stages2', 'bf16:stages4',
     'trim:t:GEMM', 'trim:hw:GEMM', 'trim:t:KS', 'trim:hw:KS',
     'fwd:ks32', 'fwd:ks64', 'dgrad:ks32', 'dgrad:ks64',
     'dgrad:classes:2', 'dgrad:classes:4', 'dgrad:classes:8', 'dgrad:classes:empty-class', 'dgrad:classes:w3',
     'dgrad:classes:no-w3', 'dgrad:strided-generic(k<s)',
     'tap:kind1', 'tap:kind2', 'tap:rows128', 'tap:rows256',
     'bn-on-load:1', 'bn-on-load:2', 'dgrad-bn:ordered', 'wgrad:bn-ok',
     'wgrad:bf16:conv_wgrad_kernel:no-16-byte-gather', 'wgrad:bf16:conv_wgrad_kernel:window>8',
     'wgrad:f32:conv_wgrad_kernel:window>8',
     'wgrad:bf16:dma:128x128', 'wgrad:bf16:dma:64x256', 'wgrad:bf16:dma:128x256', 'wgrad:bf16:dma:192x256',
     'wgrad:f32:dma:128x128', 'wgrad:f32:dma:64x128',
     'wgrad:tm1', 'wgrad:tm2', 'wgrad:tm3', 'wgrad:tm4', 'wgrad:splits=1', 'wgrad:splits>1'] +
    ['channels:%d' % ch for ch in (1, 3, 24, 40, 83, 144, 230)])


def test_conv_case_table_routes_and_coverage():
    """tests/conv_cases.py, the table tests/test_conv_float64_gpu.py runs: every row still takes the route it was written for
    (the host-side kernel-choice queries against the literals of the row), and the table as a whole reaches every member of
    CONV_REQUIRED above -- the route_conv paths, the conv_gemm tiles in both modes, the gather / weight forms of gemm_form,
    trimmed windows, the K-split column tiles, the parity-class counts of the strided data gradients, the LDS-staged tile
    heights, every weight-gradient kernel and table row -- and every row listed above.  A routing threshold that moves a
    case, or a row taken out, is named here."""
    from tests import conv_cases as T
    moved, seen = [], set()
    for c in T.CASES:
        got = T.query(c)
        want = (c.fwd, c.dgrad, c.wgrad, c.bn_in, c.dgrad_bn_ws)
        for what, g, w in zip(('fwd', 'dgrad', 'wgrad', 'bn_in_ok', 'dgrad_bn_workspace'), got, want):
            if g != w:
                moved.append('%s %s: expected %r, the library reports %r' % (c.name, what, w, g))
        seen |= set(T.members(c))
    assert not moved, '\n'.join(moved)
    assert len({c.name for c in T.CASES}) == len(T.CASES)
    need = list(CONV_REQUIRED) + ['row:' + n for n in CONV_TABLE_ROWS]
    missing = [m for m in need if m not in seen]
    assert not missing, 'not covered by the table: %s' % ', '.join(missing)


POOL_TABLE_ROWS = [
    'st_5x5_t2_c4', 'g_4x6_t2', 'st_8x15_t1_c36', 'st_15x8_t5_c72_n3', 'st_6x6_t2_sliced', 'q_133_7x8', 'q_133_1x2', 'q_333s2_8x7',
    'q_333s122_2x1', 'q_333s122_7x7', 'g_222_odd', 'g_311_s2', 'g_333_p0']
POOL_REQUIRED = (
    ['%s:%s:route2' % (w, dt) for w in ('fwd', 'bwd') for dt in ('f32', 'bf16')] +
    ['fwd:f32:route0', 'fwd:bf16:route0', 'bwd:f32:route0', 'bwd:bf16:route0', 'bwd:f32:route1', 'bwd:bf16:route1',
     'fwd:f32:tw14', 'fwd:f32:tw7', 'fwd:bf16:tw7', 'bwd:f32:tw7', 'bwd:bf16:tw7',
     'tile:boundary25', 'staged-shape:below25->gather', 'tile:tw14-one-pixel-last-tile', 'tile:three-tiles-w',
     'tile:tiles-along-h', 'tile:T1', 'tile:T2', 'tile:T5', 'tile:cpv<CV', 'tile:partial-last-chunk',
     'tile:bf16-chunks-differ-fwd-bwd', 'tile:groups%8!=0',
     'quad:k133/s122', 'quad:k333/s222', 'quad:k333/s122', 'quad:pad-lanes',
     'gather:k222/s222/p000', 'gather:k311/s211/p100', 'gather:k333/s111/p000',
     'sliced:route2', 'idx+4:route1', 'idx+4:route2'] +
    ['quad:%s%d' % (a, v) for a in 'HW' for v in (1, 2, 7, 8)])


def test_pool_case_table_routes_and_coverage():
    """tests/pool_cases.py, the tables tests/test_pool_gate_float64_gpu.py runs: through dv_maxpool3d_route and
    dv_spatial_chunks -- the planning functions the launches call -- every row still takes the route, tile width, chunk width
    and channel-chunk count it was written for, the tables reach every member of POOL_REQUIRED (gather / quad / staged in both
    directions and dtypes, the staged boundary and its tile geometries, the three quad geometries, channel chunks: one because
    S < 128, partial last chunk, capped by N, the gate-fold level), and every capped grid-stride launch has a case just over
    its cap with a ragged last block."""
    from dualvar_amd import _lib
    from tests import pool_cases as T
    lib = _lib.load()
    moved, seen = [], set()
    for c in T.POOL_CASES + T.BN_POOL_CASES + list(T.WRAP_POOLS.values()):
        for i, dt in enumerate((_lib.DV_F32, _lib.DV_BF16)):
            for bwd, want in ((0, c.fwd[i]), (1, c.bwd[i])):
                got = T.query(c, dt, bwd)
                if got != want:
                    moved.append('%s dtype %d bwd %d: expected %r, the library reports %r' % (c.name, dt, bwd, want, got))
    for c in T.POOL_CASES:
        seen |= set(T.members(c))
    assert len({c.name for c in T.POOL_CASES}) == len(T.POOL_CASES)
    # channel chunks
    tags = set()
    for c in T.CHUNK_CASES:
        for i, dt in enumerate((_lib.DV_F32, _lib.DV_BF16)):
            got = lib.dv_spatial_chunks(dt, c.N, c.S, c.C[i])
            if got != c.chunks:
                moved.append('%s dtype %d: expected %d channel chunks, the library reports %d' % (c.name, dt, c.chunks, got))
        tags.add(c.tag)
    g = T.GATE_LEVEL
    for i, dt in enumerate((_lib.DV_F32, _lib.DV_BF16)):
        got = lib.dv_spatial_chunks(dt, g['N'], g['S'], g['Ct'])
        if got != g['chunks'][i]:
            moved.append('gate level dtype %d: expected %d channel chunks, the library reports %d' % (dt, g['chunks'][i], got))
    assert not moved, '\n'.join(moved)
    assert tags >= {'S<128', 'partial-last-chunk', 'capped-by-N', 'CV<=16', 'C%V!=0'}
    pl = [c for c in T.CHUNK_CASES if c.tag == 'partial-last-chunk'][0]
    for i, v in enumerate((4, 8)):
        cvn = T.cp8(pl.C[i]) // v
        assert cvn % -(-cvn // pl.chunks) != 0 and pl.S == 128
    cn = [c for c in T.CHUNK_CASES if c.tag == 'capped-by-N'][0]
    assert -(-1024 // cn.N) < -(-(T.cp8(cn.C[0]) // 4) // 16)
    assert sum(g['widths']) == g['Ct'] == 256 and g['S'] == 128 and g['N'] == 3 and len(g['sliced']) == 2
    need = list(POOL_REQUIRED) + ['row:' + n for n in POOL_TABLE_ROWS]
    missing = [m for m in need if m not in seen]
    assert not missing, 'not covered by the table: %s' % ', '.join(missing)
    # the queries reject what the launches reject
    bad = T.desc(T.POOL_CASES[0], _lib.DV_F32)
    bad.To += 1
    assert lib.dv_maxpool3d_route(bad, 0, None, None) == -1 and lib.dv_maxpool3d_route(None, 0, None, None) == -1
    assert lib.dv_spatial_chunks(_lib.DV_F32, 0, 128, 8) == -1 and lib.dv_spatial_chunks(5, 1, 128, 8) == -1
    # grid wrap: every capped launch has a case with more than cap * 256 work items and a ragged last block
    assert set(T.WRAP_CAPS) == {'rowscale0', 'rowscale1', 'rowscale2', 'relu_bwd', 'ingest'} | set(T.WRAP_POOLS)
    for name, cap in T.WRAP_CAPS.items():
        items = T.wrap_items(name)
        assert cap * 256 < items < cap * 256 * 1.01 and items % 256 != 0, (name, items)


BN_TABLE_ROWS = [
    't1_r64_full', 't255_r128_one', 't257_r256_full', 't257_r224_one_sliced', 't2047_r224_one', 't2047_r64_full_sliced',
    't2048_r64_full', 't2048_r224_one_sliced', 't2049_r128_one', 't5000_r64_full_sliced', 't5000_r64_one', 'bn1d_m2_c8',
    'bn1d_m7_c136', 'bn1d_m128_c128', 'bn1d_m7_c512',
    'r1_c1', 'r2_c127', 'r3_c128_wide', 'r8_c129_wide', 'r3_c230', 'r2_c2048_wide',
    'c1', 'c3_res_views', 'c24_norelu_res', 'c83_views', 'c230_norelu', 'c2048_res', 'overcap_m220000_c40',
    'm1_c3', 'm31_c8_nomask', 'm33_c83_accum', 'm2048_c3', 'm2049_c8_nomask_noparams', 'm20480_c83', 'm20481_c8_r2',
    'm300000_c3_nomask', 'm300033_c8', 'c2048_m300', 'overcap_bwd_m220000_c40', 'c5120_m40_nomask_noparams']


def test_bn_case_table_blocks_and_coverage():
    """tests/bn_cases.py, the tables tests/test_batchnorm_single_gpu.py runs: every literal of every row against the host
    queries (dv_bn_bwd_blocks, dv_bn_bwd_reduce_workspace) and against the launch rules the table quotes from
    csrc/batchnorm.hip (the max-pool twin of the reduce: csrc/pool.hip; kThreads, column_reduce: csrc/streaming.hpp; the fold's group size:
    csrc/ordered_fold.hpp; grid_for: csrc/common.hpp) -- each of which is found in its home as often as quoted, and in no other file listed here --
    and the tables as a whole reach every member of bn_cases.REQUIRED and every row listed above.  A retune of dv_bn_bwd_blocks, of the 2048-tile threshold or of a grid cap
    that moves a row off its edge is named here."""
    from tests import bn_cases as T
    homes = ('batchnorm.hip', 'pool.hip', 'gate.hip', 'elementwise.hip', 'streaming.hpp', 'ordered_fold.hpp', 'common.hpp')
    src = {f: open(os.path.join(ROOT, 'dualvar_amd', 'csrc', f)).read() for f in homes}
    for text, where in T.QUOTED_RULES:
        assert where and set(where) <= set(homes), (text, where)
        for f in homes:                 # as often as quoted in the file(s) the rule lives in, and not in the others
            want = where.get(f, 0)
            assert src[f].count(text) == want, 'csrc/%s no longer reads %r %d time(s): tests/bn_cases.py quotes it' % (f, text, want)
    assert (T.BLOCK, T.APPLY_CAP, T.BAPPLY_CAP, T.FOLD_GROUP, T.STATS_WIDE_FROM, T.BAPPLY_MAX_C) == (256, 4096, 2048, 32, 2048, 5120)
    moved, seen = [], set()
    for c in T.STATS_CASES:
        if T.stats_threads(c.n_tiles) != c.threads:
            moved.append('%s: expected %d threads, the rule gives %d' % (c.name, c.threads, T.stats_threads(c.n_tiles)))
        assert 1 <= c.last_rows <= c.tile_rows and -(-T.stats_rows(c) // c.tile_rows) == c.n_tiles, c.name
    for c in T.FINALIZE_CASES:
        assert c.blocks == -(-c.C // 128) and c.base <= c.stride_extra and len(c.counts) >= 1, c.name
    for c in T.APPLY_CASES:
        for i, v in enumerate((4, 8)):
            got = T.stride_trip(c.M, c.C, v, T.APPLY_CAP)
            if got != (c.trip[i], c.wraps[i]):
                moved.append('%s apply, %d-wide vectors: expected %r, the rule gives %r' % (c.name, v, (c.trip[i], c.wraps[i]), got))
    for c in T.BWD_CASES:
        got = T.reduce_query(c.M, c.C)
        if got[:5] != c.red:
            moved.append('%s reduce: expected %r, the library reports %r' % (c.name, c.red, got[:5]))
        assert got[5] == T.workspace_bytes(got[0], c.C), (c.name, 'dv_bn_bwd_reduce_workspace')
        for i, v in enumerate((4, 8)):
            got = T.stride_trip(c.M, c.C, v, T.BAPPLY_CAP)
            if got != (c.bapply[0][i], c.bapply[1][i]):
                moved.append('%s bwd_apply, %d-wide vectors: expected %r, the rule gives %r'
                             % (c.name, v, (c.bapply[0][i], c.bapply[1][i]), got))
        assert T.cp8(c.C) <= T.BAPPLY_MAX_C and c.R in (1, 2) and c.res in (None, 'plain', 'accum'), c.name
    assert not moved, '\n'.join(moved)
    rows = T.STATS_CASES + T.FINALIZE_CASES + T.APPLY_CASES + T.BWD_CASES
    for c in rows:
        seen |= set(T.members(c))
    names = [c.name for c in rows]
    assert len(set(names)) == len(names)
    assert names == BN_TABLE_ROWS, 'rows added, removed or reordered: list them in BN_TABLE_ROWS'
    need = list(T.REQUIRED) + ['row:' + n for n in BN_TABLE_ROWS]
    missing = [m for m in need if m not in seen]
    assert not missing, 'not covered by the table: %s' % ', '.join(missing)
    # the two rows the issue of the empty trailing blocks was written around
    by = {c.name: c for c in T.BWD_CASES}
    assert by['m20481_c8_r2'].red[:3] == (320, 65, 316) and by['m300033_c8'].red[:3] == (1024, 294, 1021)
    # the host queries refuse what the launches refuse
    from dualvar_amd import _lib
    lib = _lib.load()
    assert lib.dv_bn_bwd_reduce_workspace(0, 8) == 0 and lib.dv_bn_bwd_reduce_workspace(8, 0) == 0
    assert lib.dv_bn_bwd_blocks(0, 8) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason='a library without the check would launch: CPU-only hosts only')
def test_single_tensor_bn_entries_refuse_bad_arguments():
    """every refusal of the single-tensor BatchNorm entries and their helpers that launches nothing: in each call every other
    argument is valid, so the named argument is the only reason to refuse (-1 DV_EINVAL, -2 DV_EALIGN, -3 DV_EUNSUPPORTED)"""
    from dualvar_amd import _lib as L
    lib = L.load()
    p, q = 1 << 20, (1 << 20) + 4                # non-null and 16-byte aligned / 4-byte aligned only: nothing is dereferenced
    M, C_, CP, eps, mom = 64, 12, 16, 1e-5, 0.1
    F, B = L.DV_F32, L.DV_BF16

    def stats(n_tiles=4, tile_rows=16, pitch=C_, M_=M, c=C_, part=p, local=p):
        return lib.dv_bn_reduce_stats(part, n_tiles, tile_rows, pitch, M_, c, local, None)

    def stats_fin(n_tiles=4, pitch=C_, M_=M, c=C_, gamma=p, rm=p, rv=p, shift=p):
        return lib.dv_bn_stats_finalize(p, n_tiles, 16, pitch, M_, c, p, gamma, p, eps, mom, rm, rv, p, p, p, shift, None)

    def fin(R=2, stride=2 * C_ + 1, c=C_, stats_=p, rm=p, rv=p, mean=p):
        return lib.dv_bn_finalize(stats_, R, stride, c, p, p, eps, mom, rm, rv, mean, p, p, p, None)

    def app(dt=F, x=p, ldx=CP, scale=p, shift=p, res=p, ldr=CP, y=p, ldy=CP, M_=M, c=C_):
        return lib.dv_bn_apply(dt, x, ldx, scale, shift, res, ldr, y, ldy, M_, c, 0, None)

    def red(dt=F, dy=p, lddy=CP, y=p, ldy=CP, x=p, ldx=CP, mean=p, M_=M, c=C_, flags=0, sums=p, n_rep=1, ws=p):
        return lib.dv_bn_bwd_reduce(dt, dy, lddy, y, ldy, x, ldx, mean, p, M_, c, flags, sums, n_rep, ws, None)

    def bapp(dt=F, dy=p, lddy=CP, y=p, ldy=CP, x=p, ldx=CP, rep=1, dgamma=p, dbeta=p, dx=p, lddx=CP, dres=p, lddres=CP, M_=M,
             c=C_, flags=0):
        return lib.dv_bn_bwd_apply(dt, dy, lddy, y, ldy, x, ldx, p, p, p, p, rep, 1.0 / M, 1.0, dgamma, dbeta, dx, lddx, dres,
                                   lddres, M_, c, flags, None)

    inval = [
        # non-positive sizes, missing pointers
        stats(n_tiles=0), stats(c=0), stats(M_=0), stats(part=None), stats(local=None),
        stats_fin(n_tiles=0), stats_fin(c=0), stats_fin(M_=0), stats_fin(gamma=None), stats_fin(shift=None),
        fin(R=0), fin(c=0), fin(stats_=None), fin(mean=None),
        app(M_=0), app(c=0), app(x=None), app(y=None), app(scale=None),
        red(M_=0), red(c=0), red(n_rep=0), red(n_rep=-1), red(dy=None), red(y=None), red(sums=None), red(mean=None),
        bapp(M_=0), bapp(c=0), bapp(rep=0), bapp(dx=None), bapp(y=None),
        lib.dv_bn_eval_coeffs(p, p, p, p, eps, 0, p, p, None), lib.dv_bn_eval_coeffs(p, p, p, None, eps, C_, p, p, None),
        lib.dv_bn_eval_coeffs(p, p, p, p, eps, C_, None, p, None),
        lib.dv_bn_rows_partials_f32(p, C_, 0, C_, p, None), lib.dv_bn_rows_partials_f32(p, C_, M, 0, p, None),
        lib.dv_bn_rows_partials_f32(None, C_, M, C_, p, None), lib.dv_bn_rows_partials_f32(p, C_, M, C_, None, None),
        lib.dv_addcmul_f32(p, p, p, 1.0, 0, None), lib.dv_addcmul_f32(None, p, p, 1.0, 8, None),
        lib.dv_addcmul_f32(p, None, None, 1.0, 8, None),
        lib.dv_fill_cols_f32(p, 0, 8, 0, 8, 0.0, None), lib.dv_fill_cols_f32(p, 4, 8, 0, 0, 0.0, None),
        lib.dv_fill_cols_f32(None, 4, 8, 0, 8, 0.0, None), lib.dv_fill_cols_f32(p, 4, 8, -1, 4, 0.0, None),
        # pitch < C, stride < 2C + 1, col0 + ncols > pitch
        stats(pitch=C_ - 1), stats_fin(pitch=C_ - 1), fin(stride=2 * C_), lib.dv_bn_rows_partials_f32(p, C_ - 1, M, C_, p, None),
        lib.dv_fill_cols_f32(p, 4, 8, 5, 4, 0.0, None), lib.dv_fill_cols_f32(p, 4, 8, 0, 9, 0.0, None),
        # exactly one of running_mean / running_var, of dgamma / dbeta
        stats_fin(rm=None), stats_fin(rv=None), fin(rm=None), fin(rv=None), bapp(dgamma=None), bapp(dbeta=None),
        # pitches below CP (C = 12: CP = 16)
        app(ldx=C_), app(ldy=C_), app(ldr=C_), red(lddy=C_), red(ldx=C_), red(ldy=C_), bapp(lddy=C_), bapp(ldx=C_),
        bapp(ldy=C_), bapp(lddx=C_), bapp(lddres=C_),
    ]
    assert all(rc == -1 for rc in inval), [i for i, rc in enumerate(inval) if rc != -1]
    # (a pitch below CP is not asked of what is not read: the residual / y / dres that is absent)
    align = [
        # pitches that are no multiple of the vector width (4 fp32, 8 bf16 values)
        app(ldx=CP + 2), app(ldy=CP + 2), app(ldr=CP + 2), app(dt=B, ldx=CP + 4), app(dt=B, ldy=CP + 4), app(dt=B, ldr=CP + 4),
        red(lddy=CP + 2), red(ldx=CP + 2), red(ldy=CP + 2), red(dt=B, lddy=CP + 4), red(dt=B, ldx=CP + 4), red(dt=B, ldy=CP + 4),
        bapp(lddy=CP + 2), bapp(ldx=CP + 2), bapp(ldy=CP + 2), bapp(lddx=CP + 2), bapp(lddres=CP + 2), bapp(dt=B, lddx=CP + 4),
        bapp(dt=B, lddres=CP + 4),
        # misaligned pointers
        app(x=q), app(y=q), app(res=q), app(scale=q), app(shift=q), red(dy=q), red(x=q), red(y=q), red(mean=q), red(ws=p + 2),
        bapp(dy=q), bapp(x=q), bapp(y=q), bapp(dx=q), bapp(dres=q),
    ]
    assert all(rc == -2 for rc in align), [i for i, rc in enumerate(align) if rc != -2]
    unsupported = [app(dt=7), red(dt=7), bapp(dt=7),
                   # C = 5121: 3 * 5128 floats of LDS are more than 60 KiB (C = 5120 launches: tests/test_batchnorm_single_gpu.py)
                   bapp(c=5121, lddy=5128, ldy=5128, ldx=5128, lddx=5128, lddres=5128)]
    assert all(rc == -3 for rc in unsupported), unsupported
    # with DV_NO_RELU_MASK y is not read: a missing, short or misaligned y is no reason to refuse (not called: it would launch)


def test_bn_float64_references_match_torch():
    """tests/bn_reference.py -- the references tests/test_batchnorm_single_gpu.py adds to those of the multi-tensor file -- against
    torch's own float64 modules and autograd on the CPU: the eval-mode layer behind a biased conv, training-mode BatchNorm1d
    with its backward and running statistics, and the R-rank combine against the statistics of the pooled rows"""
    from tests import bn_reference as REF
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)           # noqa: E731
    eps, mom = 1e-5, 0.1
    # eval mode: BatchNorm3d(conv(x) + b) with running statistics, some of them zero
    N, C_, T_, H, W = 2, 7, 3, 4, 5
    x, b = rnd(N, C_, T_, H, W), rnd(C_)
    bn = torch.nn.BatchNorm3d(C_, eps=eps).double().eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * rnd(C_))
        bn.bias.copy_(rnd(C_))
        bn.running_mean.copy_(rnd(C_))
        bn.running_var.copy_(torch.rand(C_, generator=g, dtype=torch.float64))
        bn.running_var[::3] = 0
        want = bn(x + b.view(1, C_, 1, 1, 1))
    rows = x.permute(0, 2, 3, 4, 1).reshape(-1, C_)                              # the kernels' [M][C] view
    got = REF.eval_reference(rows, b, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), eps)
    assert torch.allclose(got, want.permute(0, 2, 3, 4, 1).reshape(-1, C_), rtol=1e-12, atol=1e-12)
    got = REF.eval_reference(rows, None, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), eps)
    assert torch.allclose(got, bn(x).detach().permute(0, 2, 3, 4, 1).reshape(-1, C_), rtol=1e-12, atol=1e-12)
    # training-mode BatchNorm1d, M = 2 and a head-sized batch
    for M in (2, 37):
        C_ = 9
        x, dy = rnd(M, C_) * 1.5 + 0.4, rnd(M, C_)
        bn1 = torch.nn.BatchNorm1d(C_, eps=eps, momentum=mom).double().train()
        with torch.no_grad():
            bn1.weight.copy_(1 + 0.3 * rnd(C_))
            bn1.bias.copy_(rnd(C_))
            bn1.running_mean.copy_(rnd(C_))
            bn1.running_var.copy_(1 + torch.rand(C_, generator=g, dtype=torch.float64))
        rm0, rv0 = bn1.running_mean.clone(), bn1.running_var.clone()
        xr = x.clone().requires_grad_(True)
        out = bn1(xr)
        out.backward(dy)
        r = REF.bn1d_reference(x, bn1.weight.detach(), bn1.bias.detach(), rm0, rv0, dy, eps, mom)
        for k, w in (('y', out.detach()), ('rm', bn1.running_mean), ('rv', bn1.running_var), ('dx', xr.grad),
                     ('dgamma', bn1.weight.grad), ('dbeta', bn1.bias.grad)):
            assert torch.allclose(r[k], w, rtol=1e-9, atol=1e-11), (M, k)
        assert torch.allclose(r['S'], x.sum(0)) and torch.allclose(r['M2'], x.var(0, unbiased=False) * M, rtol=1e-12)
        assert torch.allclose(r['invstd'], (x.var(0, unbiased=False) + eps).rsqrt(), rtol=1e-12)
    # the R-rank combine: ranks of unequal row counts (one of a single row) against the pooled rows
    counts = (64, 65, 1, 300, 2)
    x = rnd(sum(counts), 6) * 2 + 1
    parts = torch.split(x, counts)
    S_r = torch.stack([q.sum(0) for q in parts])
    Q_r = torch.stack([((q - q.mean(0)) ** 2).sum(0) for q in parts])
    cnt, S, mean, M2 = REF.combine(S_r, Q_r, torch.tensor(counts))
    assert cnt == sum(counts) and torch.allclose(S, x.sum(0), rtol=1e-13) and torch.allclose(mean, x.mean(0), rtol=1e-12, atol=1e-14)
    assert torch.allclose(M2, x.var(0, unbiased=False) * cnt, rtol=1e-12)


def test_every_abi_entry_names_its_strongest_test():
    """tests/abi_coverage.py maps every entry of _lib.SIGNATURES to the test file that holds its strongest reference test and
    to the kind of that reference; each file mentions its entry.  (dv_check_device and dv_quantize_fp8_workspace are checked
    here only to be exported with the declared signature; dv_bn_bwd_blocks and dv_bn_bwd_reduce_workspace by the case-table
    test above.)  No entry is 'torch fp32 only' any more: the fp8 trio, the last one, has tests/test_fp8_float64_gpu.py."""
    from dualvar_amd import _lib
    from tests import abi_coverage as A
    assert set(A.ENTRY_COVERAGE) == set(_lib.SIGNATURES), sorted(set(A.ENTRY_COVERAGE) ^ set(_lib.SIGNATURES))
    here = os.path.join(ROOT, 'tests')
    text = {}
    for name, (fname, kind) in A.ENTRY_COVERAGE.items():
        assert kind in A.KINDS, (name, kind)
        if fname not in text:
            text[fname] = open(os.path.join(here, fname)).read()
        assert re.search(r'\b%s\b' % name, text[fname]), '%s is not mentioned in tests/%s' % (name, fname)
    weak = sorted(n for n, (_, k) in A.ENTRY_COVERAGE.items() if k == A.TORCH_FP32)
    assert not [n for n in weak if n.startswith('dv_bn_') or n in ('dv_addcmul_f32', 'dv_fill_cols_f32')], weak
    assert weak == [], weak


def test_ordered_fold_protocol_has_one_home():
    """The ticketed hand-off of the ordered reductions (sc1 stores, drained counter, agent-scope ticket, sc1 loads) lies outside
    the HIP memory model and is guarded for gfx950 in csrc/ordered_fold.hpp; its three users (streaming.hpp, for the BatchNorm
    backward of batchnorm.hip; conv_tap.hip; loss.hip) call that header.  So no other source spells an agent-scope atomic of its own, and loss.hip no longer carries
    a bare drain: a fourth copy of the protocol would fail here."""
    csrc = os.path.join(ROOT, 'dualvar_amd', 'csrc')
    files = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.hpp')))
    assert 'ordered_fold.hpp' in files and len(files) >= 14
    holders = [f for f in files if '__HIP_MEMORY_SCOPE_AGENT' in open(os.path.join(csrc, f)).read()]
    assert holders == ['ordered_fold.hpp'], holders
    loss = open(os.path.join(csrc, 'loss.hip')).read()
    assert not re.search(r's_waitcnt\s+vmcnt\(0\)"\s*:\s*:\s*:\s*"memory"', loss)
    assert '#include "ordered_fold.hpp"' in loss


def test_conv_interface_has_one_home():
    """The conv sources talk across translation units through plain C++ functions (dvt_ conv_tap.hip, dvg_ conv_gemm_fwd.hip / conv_gemm_dgrad.hip, dvwg_
    conv_wgrad.hip, dvw_ conv_tap_wgrad.hip, dvx_ conv_experiments.hip).  Each is declared exactly once, in the interface section
    that ends csrc/conv_common.hpp, and nowhere else; every conv source includes that header, so the compiler checks each
    definition against the declaration its callers see; and no definition takes an argument block (or anything else) as void*.
    A prototype copied back into a .hip, a crossing function without a declaration in the header, or a type-erased argument
    fails here."""
    csrc = os.path.join(ROOT, 'dualvar_amd', 'csrc')
    convs = sorted(f for f in os.listdir(csrc) if f.startswith('conv') and f.endswith('.hip'))
    assert convs == ['conv.hip', 'conv_experiments.hip', 'conv_gemm_dgrad.hip', 'conv_gemm_fwd.hip', 'conv_tap.hip', 'conv_tap_wgrad.hip',
                     'conv_wgrad.hip']
    from dualvar_amd.build import SOURCES
    assert set(convs) <= set(SOURCES)
    text = {f: open(os.path.join(csrc, f)).read() for f in convs}
    hdr = open(os.path.join(csrc, 'conv_common.hpp')).read()
    cut = hdr.index("// ==== the conv translation units' interface")
    before, iface = hdr[:cut], hdr[cut:]

    def proto(name):      # a declaration: return type, name, parameter list, semicolon
        return re.compile(r'^[ \t]*(?!return\b|else\b)[\w<>]+[\w<>\s*&]*?[\s*&]' + name + r'\s*\([^;{]*\)\s*;', re.M)

    def definition(name):
        return re.compile(r'^[\w<>]+[\w<>\s*&]*?[\s*&]' + name + r'\s*\(([^;{]*)\)\s*\{', re.M)

    # what crosses: every function with C++ linkage that a conv source defines outside its anonymous namespaces ...
    external = {}
    for f in convs:
        anon = 0
        for line in text[f].split('\n'):
            if line.startswith('namespace {'):
                anon += 1
            elif line.startswith('}  // namespace'):
                anon -= 1
            elif not anon:
                m = re.match(r'(?!static\b|extern\b|template\b|struct\b|enum\b|typedef\b|constexpr\b|using\b)[\w<>]+[\w<>\s*&]*?[\s*&]'
                             r'(\w+)\s*\((?:[^;{]*\)\s*\{|[^;{)]*$)', line)
                if m:
                    assert m.group(1) not in external, m.group(1)
                    external[m.group(1)] = f
        assert anon == 0, f
    # ... which is every dvt_ / dvg_ / ... name that any of them mentions
    called = set(n for t in text.values() for n in re.findall(r'\bdv[a-z]+_\w+', t))
    assert set(external) == called and len(called) >= 20, (sorted(set(external) ^ called), len(called))
    for name, home in sorted(external.items()):
        assert len(proto(name).findall(iface)) == 1, name
        assert not proto(name).search(before), name
        for f in convs:
            assert not proto(name).search(text[f]), (name, f)
        users = [f for f in convs if f != home and re.search(r'\b' + name + r'\b', text[f])]
        assert users, name
        defs = definition(name).findall(text[home])
        assert len(defs) == 1 and not re.search(r'\bvoid\s*\*', defs[0]), (name, defs)
    gemm_hpp = open(os.path.join(csrc, 'conv_gemm.hpp')).read()      # (the two conv_gemm_*.hip include the header through it)
    assert '#include "conv_common.hpp"' in gemm_hpp and not any(proto(n).search(gemm_hpp) for n in external)
    for f in convs:
        assert '#include "conv_common.hpp"' in text[f] or (f.startswith('conv_gemm_') and '#include "conv_gemm.hpp"' in text[f]), f
