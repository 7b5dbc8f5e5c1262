"""GradientDescentOptimizer and MomentumOptimizer on the CPU (no GPU): the numpy restatement of the update rules, argument
validation of the new C-ABI entry points, optimiser selection from the conf, slot memory, launch plans and their label coverage,
checkpoints, and the data-parallel schedules (gloo, world 2) with the optimiser emulated on the flat buffers."""
import ctypes as C
import importlib
import inspect
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dynamic_multiview_3d_amd import _lib

E_INVAL = -1


# ---------------------------------------------------------------- the oracle: TF 1.3 training_ops, fp32, in TF's order
def sgd_rule(p, g, a, lr, mu=0.0, nesterov=False, gscale=1.0):
    """ApplyGradientDescent (a is None) or ApplyMomentum on float32 arrays; returns (p, a)."""
    f = np.float32
    g = g * f(gscale)
    if a is None:
        return p - g * f(lr), None
    a = a * f(mu) + g
    if nesterov:
        return p - (g * f(lr) + (a * f(mu)) * f(lr)), a
    return p - a * f(lr), a


def test_rule_matches_float64():
    rng = np.random.default_rng(0)
    p, g, a = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    for mom, nest in ((False, False), (True, False), (True, True)):
        pf, af = sgd_rule(p, g, a if mom else None, 1e-2, 0.9 if mom else 0.0, nest, 0.5)
        assert pf.dtype == np.float32 and (af is None or af.dtype == np.float32)
        p64, g64, a64 = p.astype(np.float64), g.astype(np.float64) * 0.5, a.astype(np.float64)
        if not mom:
            ref = p64 - g64 * 1e-2
        else:
            a64 = a64 * 0.9 + g64
            ref = p64 - (g64 * 1e-2 + a64 * 0.9 * 1e-2) if nest else p64 - a64 * 1e-2
            np.testing.assert_allclose(af, a64, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(pf, ref, rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------- C ABI: validation before any launch
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def test_sgd_step_validation(lib):
    A = 4096                                        # 16-byte aligned stand-ins: nothing is dereferenced on a rejected call
    assert lib.raw_sgd_step(0, A, A, A, 1e-2, 0.9, 0, 1.0, None) == E_INVAL
    assert lib.raw_sgd_step(8, None, A, A, 1e-2, 0.9, 0, 1.0, None) == E_INVAL
    assert lib.raw_sgd_step(8, A, None, None, 1e-2, 0.0, 0, 1.0, None) == E_INVAL
    assert lib.raw_sgd_step(8, A + 4, A, A, 1e-2, 0.9, 0, 1.0, None) == E_INVAL
    assert 'aligned' in lib.last_error()
    assert lib.raw_sgd_step(8, A, A, A + 8, 1e-2, 0.9, 0, 1.0, None) == E_INVAL
    assert lib.raw_sgd_step(8, A, A, None, 1e-2, 0.0, 1, 1.0, None) == E_INVAL          # nesterov without accum
    assert 'accum' in lib.last_error()
    assert lib.raw_sgd_step(8, A, A, None, 1e-2, 0.9, 0, 1.0, None) == E_INVAL          # momentum without accum


def test_sgd_step_dev_validation(lib):
    A = 4096
    lo, hi = (_lib.C.c_int64 * 2)(0, 16), (_lib.C.c_int64 * 2)(8, 32)
    assert lib.raw_sgd_step_dev(6, A, A, A, A, 0, None, None, None) == E_INVAL            # count not a multiple of 4
    assert lib.raw_sgd_step_dev(8, None, A, A, A, 0, None, None, None) == E_INVAL
    assert lib.raw_sgd_step_dev(8, A, A, A, None, 0, None, None, None) == E_INVAL         # no state
    assert lib.raw_sgd_step_dev(8, A, A + 4, None, A, 0, None, None, None) == E_INVAL
    assert lib.raw_sgd_step_dev(64, A, A, A, A, 9, lo, hi, None) == E_INVAL               # more than 8 ranges
    assert lib.raw_sgd_step_dev(64, A, A, A, A, 2, None, None, None) == E_INVAL
    bad = (_lib.C.c_int64 * 2)(0, 4)
    assert lib.raw_sgd_step_dev(64, A, A, A, A, 2, lo, (_lib.C.c_int64 * 2)(8, 30), None) == E_INVAL      # not a multiple of 4
    assert lib.raw_sgd_step_dev(64, A, A, A, A, 2, bad, hi, None) == E_INVAL              # overlapping
    assert 'sorted and disjoint' in lib.last_error()
    assert lib.raw_sgd_step_dev(64, A, A, A, A, 2, (_lib.C.c_int64 * 2)(16, 0), (_lib.C.c_int64 * 2)(32, 8), None) == E_INVAL  # unsorted
    assert lib.raw_sgd_step_dev(16, A, A, A, A, 2, lo, hi, None) == E_INVAL               # beyond count


def test_fc_wgrad_sgd_validation(lib):
    A = 4096
    args = [64, 4096, 4096, A, 4096, A, 4096, A, A, A, A, None]
    assert lib.raw_fc_wgrad_sgd(*args[:7], A, A, A, None, None) == E_INVAL                 # no state
    assert lib.raw_fc_wgrad_sgd(*args[:7], None, A, A, A, None) == E_INVAL                 # no matrix
    assert lib.raw_fc_wgrad_sgd(64, 4096, 4096, None, 4096, A, 4096, A, A, A, A, None) == E_INVAL
    assert lib.raw_fc_wgrad_sgd(64, 4096, 4096, A, 4000, A, 4096, A, A, A, A, None) == E_INVAL      # x_ld < in
    assert lib.raw_fc_wgrad_sgd(*args[:7], A, A + 4, A, A, None) == E_INVAL                # misaligned accum
    assert lib.raw_fc_wgrad_sgd(0, 4096, 4096, A, 4096, A, 4096, A, A, A, A, None) == E_INVAL


def test_grad_finalize_commit_sgd_validation(lib):
    A = 4096
    assert lib.raw_grad_finalize_commit_sgd(None, 0, A, A, A, A, None) == E_INVAL           # no open collection
    assert 'no open collection' in lib.last_error()
    for grads, params, accum, state in ((None, A, A, A), (A, None, A, A), (A, A, A, None), (A + 4, A, A, A), (A, A, A + 4, A)):
        lib.grad_finalize_begin()
        lib.grad_finalize_add(A, 16)
        assert lib.raw_grad_finalize_commit_sgd(None, 0, grads, params, accum, state, None) == E_INVAL
    lib.grad_finalize_begin()                       # a rejected commit closed its collection
    lib.grad_finalize_abort()


# ---------------------------------------------------------------- conf -> optimiser -> plans
B64 = {'batch_size': 64, 'learning_rate': 1e-4}
KINDS = {'momentum': dict(optimizer='momentum', momentum=0.9), 'sgd': dict(optimizer='sgd')}
NEW_LABELS = {
    'fc_wgrad_momentum_b3': 'tests/test_gpu_optimizers.py::test_fused_fc_wgrad_sgd_equals_wgrad_then_sgd_step',
    'fc_wgrad_sgd_b3': 'tests/test_gpu_optimizers.py::test_fused_fc_wgrad_sgd_equals_wgrad_then_sgd_step',
    'grad_finalize_momentum': 'tests/test_gpu_optimizers.py::test_grad_finalize_sgd_equals_per_layer_reduction_and_sgd_step',
    'grad_finalize_sgd': 'tests/test_gpu_optimizers.py::test_grad_finalize_sgd_equals_per_layer_reduction_and_sgd_step',
    'momentum': 'tests/test_gpu_optimizers.py::test_sgd_step_bit_exact_vs_numpy',
    'sgd': 'tests/test_gpu_optimizers.py::test_sgd_step_bit_exact_vs_numpy',
}


def _appflow(conf):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cpu')


@pytest.fixture(scope="module")
def b64_models():
    return {k: _appflow(dict(B64, **extra)) for k, extra in [('absent', {}), ('adam', {'optimizer': 'adam'})] + list(KINDS.items())}


def _labels(plan):
    return [o[0] for o in _lib.plan_ops(plan)]


class _Counter:
    """Records the calls run_backward_fused makes outside the recorded plan (none of them runs: no device)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append(name)


def _launches_per_step(g):
    real, g.lib = g.lib, _Counter()
    g._stream_ptr = lambda: None
    try:
        g.run_backward_fused()
    finally:
        calls, g.lib = g.lib.calls, real
        del g._stream_ptr
    direct = [c for c in calls if not c.startswith('plan_')]
    return g.n_launch_fwd + g.n_launch_bwd_fused + len(direct), direct


def test_absent_optimizer_key_is_the_adam_plan(b64_models):
    a, b = b64_models['absent'].graph, b64_models['adam'].graph
    assert a.optimizer == 'adam' and a.adam_m is not None and a.accum is None
    for pa, pb in ((a.plan_fwd, b.plan_fwd), (a.plan_bwd, b.plan_bwd), (a.plan_bwd_fused, b.plan_bwd_fused)):
        assert _labels(pa) == _labels(pb)
    fused = _labels(a.plan_bwd_fused)
    assert fused.count('fc_wgrad_adam_b3') == 4 and 'grad_finalize_adam' in fused
    n, direct = _launches_per_step(a)
    assert direct == ['adam_step_dev', 'adam_advance', 'adam_advance']


def test_fused_fc_optimiser_closes_the_reverse_pass(lib, monkeypatch):
    """LinearNode.record_fused_update: the four fused fc launches go on side class 2 behind every class-1 launch of the fused
    reverse pass (conv / fc filter gradients, chunked finalisations), and only the last grad_finalize follows them."""
    monkeypatch.delenv('MV3D_SIDE_STREAMS', raising=False)          # the default: two side streams
    marks, cur = [], [None]
    begin, side = lib.plan_begin, lib.plan_side

    def plan_begin(p):
        cur[0] = p
        return begin(p)

    def plan_side(k):
        marks.append((cur[0], lib.plan_size(cur[0]), k))
        return side(k)

    monkeypatch.setattr(lib, 'plan_begin', plan_begin)
    monkeypatch.setattr(lib, 'plan_side', plan_side)
    g = _appflow(dict(B64)).graph
    labels = _labels(g.plan_bwd_fused)
    cls = [0] * len(labels)                 # the side class each launch was recorded under
    for p, i, k in marks:
        if p == g.plan_bwd_fused:
            cls[i:] = [k] * (len(labels) - i)
    fc = [i for i, k in enumerate(cls) if k == 2]
    assert [labels[i] for i in fc] == ['fc_wgrad_adam_b3'] * 4
    assert labels[fc[-1] + 1:] == ['grad_finalize_adam']
    side1 = [i for i, k in enumerate(cls[:fc[-1] + 1]) if k == 1]
    assert side1 and max(side1) < fc[0]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_conf_selects_the_fused_plan_of_the_optimizer(b64_models, kind):
    g, adam = b64_models[kind].graph, b64_models['adam'].graph
    assert g.optimizer == kind and g.plan_bwd_fused is not None
    fused = _labels(g.plan_bwd_fused)
    assert fused.count('fc_wgrad_%s_b3' % kind) == 4
    assert fused.count('grad_finalize_%s' % kind) == _labels(adam.plan_bwd_fused).count('grad_finalize_adam') >= 1
    every = fused + _labels(g.plan_fwd) + _labels(g.plan_bwd)
    assert not [l for l in every if 'adam' in l]
    n, direct = _launches_per_step(g)
    n_adam, _ = _launches_per_step(adam)
    assert direct == ['sgd_step_dev'] and n <= n_adam - 2
    np.testing.assert_array_equal(g.opt_state.numpy()[:8], g.opt_state.numpy()[8:])
    st = g.opt_state.numpy()
    assert st[0] == np.float32(1e-4) and st[1] == np.float32(0.9 if kind == 'momentum' else 0.0) and st[2] == 0.0 and st[6] == 1.0


def test_slot_memory_follows_the_optimizer(b64_models):
    mom, gd, adam = b64_models['momentum'].graph, b64_models['sgd'].graph, b64_models['adam'].graph
    assert mom.accum is not None and mom.accum.numel() == mom.flat_size and mom.adam_m is None and mom.adam_v is None
    assert gd.accum is None and gd.adam_m is None and gd.adam_v is None
    assert adam.accum is None and adam.adam_m.numel() == adam.adam_v.numel() == adam.flat_size
    assert adam.flat_size > 69e6


def test_new_labels_are_parity_tested(b64_models):
    """In the spirit of test_label_coverage.py: a Momentum or GD plan of the benchmarked configuration launches only kernels the
    Adam plan already launches, or the new ones, each held bit-exact by a GPU test."""
    def labels(g):
        return set(_labels(g.plan_fwd)) | set(_labels(g.plan_bwd)) | set(_labels(g.plan_bwd_fused))
    adam = labels(b64_models['adam'].graph)
    for kind in KINDS:
        new = labels(b64_models[kind].graph) - adam
        assert new and not new - set(NEW_LABELS), new - set(NEW_LABELS)
    for label, where in NEW_LABELS.items():
        path, name = where.split('::')
        mod = importlib.import_module(path[:-3].replace('/', '.'))
        assert inspect.isfunction(getattr(mod, name)), where


@pytest.mark.parametrize("conf", [dict(optimizer='rmsprop'), dict(optimizer='momentum'), dict(optimizer='momentum', momentum=None)])
def test_bad_conf_raises_value_error(conf):
    with pytest.raises(ValueError):
        _appflow(dict({'batch_size': 2, 'learning_rate': 1e-4}, **conf))


def test_conf_helper_and_optimizer_classes():
    from dynamic_multiview_3d_amd import model_base as mb
    assert isinstance(mb.optimizer_from_conf({}, 1e-3), mb.AdamOptimizer)
    o = mb.optimizer_from_conf({'optimizer': 'momentum', 'momentum': 0.5, 'use_nesterov': True}, 1e-3)
    assert isinstance(o, mb.MomentumOptimizer) and (o.lr, o.momentum, o.use_nesterov) == (1e-3, 0.5, True)
    assert isinstance(mb.optimizer_from_conf({'optimizer': 'sgd'}, 1e-3), mb.GradientDescentOptimizer)
    m = _appflow({'batch_size': 2, 'learning_rate': 1e-3, 'optimizer': 'momentum', 'momentum': 0.5, 'use_nesterov': True})
    st = m.graph.opt_state.numpy()
    assert (st[0], st[1], st[2], st[6]) == (np.float32(1e-3), 0.5, 1.0, 1.0)


# ---------------------------------------------------------------- checkpoints
def _lowdim(conf, seed=7):
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    return AppFlowLowDimAngle(dict({'batch_size': 2, 'learning_rate': 1e-4}, **conf), load_tfrec=False, device='cpu', seed=seed)


def test_momentum_checkpoint_names_and_round_trip(tmp_path):
    from dynamic_multiview_3d_amd import tf_checkpoint
    m = _lowdim(KINDS['momentum'])
    g = m.graph
    g.accum.copy_(torch.randn(g.flat_size, generator=torch.Generator().manual_seed(1)))
    prefix = m.saver.save(None, str(tmp_path / 'model'), global_step=3)
    sd = tf_checkpoint.read_checkpoint(prefix)
    with_grad = [k for k, v in g.variables.items() if v.has_grad]
    assert with_grad
    assert set(sd) == set(g.variables) | {k + '/Momentum' for k in with_grad}
    for k in with_grad:
        v = g.variables[k]
        np.testing.assert_array_equal(sd[k + '/Momentum'], g.accum[v.offset:v.offset + v.size].view(v.shape).numpy())
    m2 = _lowdim(KINDS['momentum'], seed=8)
    assert not torch.equal(m2.graph.params, g.params)
    m2.saver.restore(None, prefix)
    for k, v in g.variables.items():
        sl = slice(v.offset, v.offset + v.size)
        assert torch.equal(m2.graph.params[sl], g.params[sl])
        if v.has_grad:
            assert torch.equal(m2.graph.accum[sl], g.accum[sl])
    gd = _lowdim(KINDS['sgd'])
    assert set(gd.graph.state_dict()) == set(gd.graph.variables)


def test_cross_optimizer_restore_raises_key_error(tmp_path):
    ckpt = {k: _lowdim(conf).saver.save(None, str(tmp_path / k)) for k, conf in (('adam', {}), ('momentum', KINDS['momentum']),
                                                                                 ('sgd', KINDS['sgd']))}
    with pytest.raises(KeyError, match='/Adam'):
        _lowdim(KINDS['momentum']).saver.restore(None, ckpt['adam'])
    with pytest.raises(KeyError, match='/Momentum'):
        _lowdim({}).saver.restore(None, ckpt['momentum'])
    with pytest.raises(KeyError, match='/Momentum'):                   # GD checkpoint: no accumulators to restore
        _lowdim(KINDS['momentum']).saver.restore(None, ckpt['sgd'])
    with pytest.raises(KeyError, match='/Momentum'):
        _lowdim(KINDS['sgd']).saver.restore(None, ckpt['momentum'])
    _lowdim(KINDS['sgd']).saver.restore(None, ckpt['sgd'])


# ---------------------------------------------------------------- data parallel (gloo, world 2)
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _SgdCpuLib:
    """Stands in for libmv3d_hip.so: segments are no-ops (the test supplies the gradients), mv3d_sgd_step_dev is the rule
    above on the flat buffers (read through the device-state record it is given)."""

    def __init__(self, g):
        self.g = g
        self.calls = []

    def plan_run_range_multi(self, plan, begin, end, stream, side_streams, nside, flags):
        pass

    def sgd_step_dev(self, count, p, gr, accum, state, nskip, slo, shi, stream):
        g = self.g
        assert nskip == 0 and (accum is None) == (g.accum is None)
        lo = (p - g.params.data_ptr()) // 4
        rec = (state - g.opt_state.data_ptr()) // 4
        st = g.opt_state.numpy()[rec:rec + 8]
        sl = slice(lo, lo + count)
        a = g.accum.numpy()[sl] if accum is not None else None
        pn, an = sgd_rule(g.params.numpy()[sl], g.grads.numpy()[sl], a, st[0], st[1], st[2] != 0, st[6])
        g.params.numpy()[sl] = pn
        if a is not None:
            a[...] = an
        self.calls.append((lo, count))


def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from dynamic_multiview_3d_amd import parallel
    parallel.init_from_env('gloo')
    conf = dict(optimizer='momentum', momentum=0.9, use_nesterov=True)
    out = {}
    for mode in ('allreduce', 'sharded', 'single'):
        m = _lowdim(conf)
        g = m.graph
        if mode != 'single':
            m.enable_data_parallel(world, mode=mode)
        fake = _SgdCpuLib(g)
        g.lib = fake
        g._stream_ptr = lambda: None
        gens = [torch.Generator().manual_seed(1000 + r) for r in range(world)]
        for step in range(3):
            per_rank = [torch.randn(g.flat_size, generator=gen) * 1e-2 for gen in gens]
            if mode == 'single':        # one process, the global batch: the mean of the ranks' gradients
                g.grads.copy_((per_rank[0] + per_rank[1]) * np.float32(1.0 / world))
                g.apply_optimizer()
            else:
                g.grads.copy_(per_rank[rank])
                g.run_backward_overlapped(with_adam=True)
        refused = True
        if mode == 'sharded':
            try:
                g.state_dict()
                refused = False
            except RuntimeError:
                pass
            g.gather_optimizer_state()
        out[mode] = (g.params.clone(), g.accum.clone(), sum(c for _, c in fake.calls), g.flat_size, refused)
    import torch.distributed as dist
    (pa, aa, na, flat, _), (ps, as_, ns, _, refused), (p1, a1, n1, _, _) = out['allreduce'], out['sharded'], out['single']
    other = ps.clone()
    dist.broadcast(other, src=0)
    q.put((rank, bool(torch.equal(pa, ps)), bool(torch.equal(aa, as_)), bool(torch.equal(pa, p1)), bool(torch.equal(aa, a1)),
           bool(torch.equal(other, ps)), refused, na, ns, n1, flat, float(aa.abs().sum())))
    dist.destroy_process_group()


def test_sharded_momentum_equals_allreduce_and_single_process_two_ranks():
    """'sharded' (reduce-scatter -> Momentum on 1/world -> all-gather) and 'allreduce' (SUM + redundant Momentum) leave identical
    weights and accumulators on both ranks after three Nesterov steps, equal to one process stepping on the global batch;
    gather_optimizer_state completes the sharded accumulators (state_dict refuses until then)."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, p_same, a_same, p_single, a_single, ranks_equal, refused, na, ns, n1, flat, asum in res:
        assert p_same and a_same, "sharded and all-reduce modes diverged on rank %d" % rank
        assert p_single and a_single, "data-parallel step differs from the single-process global-batch step on rank %d" % rank
        assert ranks_equal and refused and asum > 0
        assert na == 3 * flat and ns * 2 == na and n1 == na
