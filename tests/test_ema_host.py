"""EMA weights on the CPU (no GPU): the numpy twins of mv3d_ema_step against the float64 closed form, the conf switch, argument
validation of the two new C-ABI entry points, where the EMA launches sit in the single-GPU and data-parallel schedules (gloo,
world 2, the rule emulated on the flat buffers), checkpoints, and Graph.ema_weights() on a CPU graph."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import EMA_COUNTER, EMA_SLOT
from dynamic_multiview_3d_amd.model_base import ema_from_conf, ema_one_minus_decay, ema_rule
from tests.test_dist_cpu import _CpuLib
from tests.test_optimizers_host import B64, _Counter, _appflow, _free_port, _labels, _lowdim

E_INVAL = -1


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
def test_ema_rule_follows_the_closed_form(decay):
    """p constant: s_k = p + (s_0 - p)(1 - w)^k.  Three fp32 roundings per step, each <= 2^-24 of a magnitude <= 2 max(|s_0|, |p|):
    the error after k steps stays below k * 4e-7 * max(|s_0|, |p|) per element."""
    rng = np.random.default_rng(5)
    s0 = (rng.standard_normal(4096) * 10.0 ** rng.integers(-4, 4, 4096)).astype(np.float32)
    p = (rng.standard_normal(4096) * 10.0 ** rng.integers(-4, 4, 4096)).astype(np.float32)
    w = ema_one_minus_decay(decay)
    assert w.dtype == np.float32
    s = s0.copy()
    s064, p64, w64 = s0.astype(np.float64), p.astype(np.float64), float(w)
    bound = 4e-7 * np.maximum(np.abs(s064), np.abs(p64))
    worst = 0.0
    for k in range(1, 201):
        s = ema_rule(s, p, w)
        assert s.dtype == np.float32
        ref = p64 + (s064 - p64) * (1.0 - w64) ** k
        err = np.abs(s.astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) / k)
        assert (err <= k * bound).all(), (k, float((err / bound).max()))
    print("decay %g: worst error / (k * 4e-7 * max) = %.3g" % (decay, worst))
    assert ema_rule(p, p, w).tobytes() == p.tobytes()          # s == p: d = 0, s stays as it is, bit for bit


def test_ema_one_minus_decay():
    for decay in (0.5, 0.9, 0.999, 0.9999):
        w = ema_one_minus_decay(decay)
        assert w.dtype == np.float32 and w == np.float32(1 - decay)
    assert ema_one_minus_decay(0.999, 0) == np.float32(0.9)                 # min(0.999, 1 / 10)
    assert ema_one_minus_decay(0.999, 10) == np.float32(0.45)               # min(0.999, 11 / 20)
    assert ema_one_minus_decay(0.999, 8989) != np.float32(1 - 0.999)
    for n in (8990, 8991, 10 ** 6):                                         # (1 + n) / (10 + n) reaches 0.999 at n = 8990
        assert ema_one_minus_decay(0.999, n) == np.float32(1 - 0.999)
    assert ema_one_minus_decay(0.5, 0) == np.float32(0.9) and ema_one_minus_decay(0.5, 8) == np.float32(0.5)


def test_ema_from_conf():
    assert ema_from_conf({}) == (None, False)
    assert ema_from_conf({'ema_decay': None}) == (None, False)
    assert ema_from_conf({'ema_decay': 0}) == (None, False) and ema_from_conf({'ema_decay': 0.0})[0] is None
    assert ema_from_conf({'ema_decay': 0.999}) == (0.999, False)
    assert ema_from_conf({'ema_decay': 0.5, 'ema_num_updates': True}) == (0.5, True)
    for bad in (-0.1, 1, 1.0, 1.5, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError):
            ema_from_conf({'ema_decay': bad})
    from dynamic_multiview_3d_amd import mv3d
    with pytest.raises(ValueError):                 # every model class reads the key, before it builds anything
        mv3d.mv3d_nobg_nodm({'batch_size': 2, 'ema_decay': 1.0}, device='cpu')
    with pytest.raises(ValueError):
        _lowdim({'ema_decay': float('nan')})


# ---------------------------------------------------------------- C ABI: validation before any launch
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def test_ema_step_validation(lib):
    A, B = 4096, 1 << 20                            # 16-byte aligned stand-ins: nothing is dereferenced on a rejected call
    assert lib.raw_ema_step(0, A, B, 0.5, None) == E_INVAL
    assert lib.raw_ema_step(-4, A, B, 0.5, None) == E_INVAL
    assert lib.raw_ema_step(8, None, B, 0.5, None) == E_INVAL
    assert lib.raw_ema_step(8, A, None, 0.5, None) == E_INVAL
    assert lib.raw_ema_step(8, A + 4, B, 0.5, None) == E_INVAL
    assert lib.raw_ema_step(8, A, B + 8, 0.5, None) == E_INVAL
    for w in (-1e-3, 1.0 + 1e-6, 2.0, float('nan'), float('inf'), -float('inf')):
        assert lib.raw_ema_step(8, A, B, w, None) == E_INVAL, w
    assert 'one_minus_decay' in lib.last_error()


def test_swap_f32_validation(lib):
    A, B = 4096, 1 << 20
    assert lib.raw_swap_f32(0, A, B, None) == E_INVAL
    assert lib.raw_swap_f32(-1, A, B, None) == E_INVAL
    assert lib.raw_swap_f32(8, None, B, None) == E_INVAL
    assert lib.raw_swap_f32(8, A, None, None) == E_INVAL
    assert lib.raw_swap_f32(8, A + 4, B, None) == E_INVAL
    assert lib.raw_swap_f32(8, A, B + 4, None) == E_INVAL
    assert lib.raw_swap_f32(8, A, A, None) == E_INVAL                      # a == b
    assert lib.raw_swap_f32(8, A, A + 16, None) == E_INVAL                 # overlapping, either order
    assert lib.raw_swap_f32(8, A + 16, A, None) == E_INVAL
    assert 'overlap' in lib.last_error()


# ---------------------------------------------------------------- where the launches sit: the fused single-GPU step
class _ArgCounter(_Counter):
    """_Counter that also keeps the arguments of every call."""

    def __init__(self):
        super().__init__()
        self.args = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            self.args.append((name, a))
        return call


def _direct_calls(g, run):
    real, g.lib = g.lib, _ArgCounter()
    g._stream_ptr = lambda: None
    try:
        run()
    finally:
        fake, g.lib = g.lib, real
        del g._stream_ptr
    return [c for c in fake.args if not c[0].startswith('plan_')]


def _ema_tiles(g, calls, w):
    """The mv3d_ema_step calls of one step cover [0, flat_size) exactly once, shadow and parameter pointers at the same offset."""
    ranges = []
    for name, a in calls:
        if name == 'ema_step':
            count, shadow, params, wk, _ = a
            lo = (params - g.params.data_ptr()) // 4
            assert (shadow - g.ema.data_ptr()) // 4 == lo and lo % 4 == 0 and wk == float(w)
            ranges.append((lo, lo + count))
    ranges.sort()
    assert ranges and ranges[0][0] == 0 and ranges[-1][1] == g.flat_size
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), ranges
    return ranges


@pytest.fixture(scope="module")
def b64_pair():
    return _appflow(dict(B64)).graph, _appflow(dict(B64, ema_decay=0.999)).graph


def test_fused_step_launch_list_with_and_without_the_switch(b64_pair):
    off, on = b64_pair
    assert off.ema is None and on.ema is not None and on.ema.numel() == on.flat_size and torch.equal(on.ema, on.params)
    for a, b in ((off.plan_fwd, on.plan_fwd), (off.plan_bwd, on.plan_bwd), (off.plan_bwd_fused, on.plan_bwd_fused)):
        assert a is not None and _labels(a) == _labels(b)          # the switch records nothing
    assert [c[0] for c in _direct_calls(off, off.run_backward_fused)] == ['adam_step_dev', 'adam_advance', 'adam_advance']
    calls = _direct_calls(on, on.run_backward_fused)
    names = [c[0] for c in calls]
    assert [n for n in names if n != 'ema_step'] == ['adam_step_dev', 'adam_advance', 'adam_advance']
    ranges = _ema_tiles(on, calls, ema_one_minus_decay(0.999))
    # the fc stream's share is what the fused kernels and their layers' bias launch update: the ranges the main optimiser skips
    skips = list(zip(on._skip_lo, on._skip_hi))
    assert on._fc_ranges == skips and all(r in ranges for r in skips)
    lo, hi = on._bias_span
    assert skips[0][0] <= lo and hi <= skips[-1][1]
    assert on.ema_updates == 1 and off.ema_updates == 0
    on.ema_updates = 0


def test_unfused_steps_cover_the_flat_buffer_once(b64_pair):
    _, on = b64_pair
    calls = _direct_calls(on, on.apply_optimizer)
    assert [c[0] for c in calls] == ['adam_step_dev', 'adam_advance', 'adam_advance', 'ema_step']
    assert _ema_tiles(on, calls, ema_one_minus_decay(0.999)) == [(0, on.flat_size)]
    on.ema_updates = 0
    # the bucketed optimiser of run_backward_with_adam: the buckets tile the buffer, so do the EMA launches behind them
    buckets = sorted((lo, hi) for _, lo, hi in on.grad_buckets if hi > lo)
    assert buckets[0][0] == 0 and buckets[-1][1] == on.flat_size and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))


# ---------------------------------------------------------------- data parallel (gloo, world 2)
class _EmaCpuLib(_CpuLib):
    """tests/test_dist_cpu.py's stand-in with mv3d_ema_step = the numpy rule on the flat buffers."""

    def __init__(self, g):
        super().__init__(g)
        self.ema_calls = []

    def ema_step(self, count, shadow, params, w, stream):
        g = self.g
        lo = (params - g.params.data_ptr()) // 4
        assert (shadow - g.ema.data_ptr()) // 4 == lo
        sl = slice(lo, lo + count)
        g.ema.numpy()[sl] = ema_rule(g.ema.numpy()[sl], g.params.numpy()[sl], np.float32(w))
        self.ema_calls.append((lo, count))


def _dp_ema_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from dynamic_multiview_3d_amd import parallel
    parallel.init_from_env('gloo')
    out = {}
    for mode in ('allreduce', 'sharded'):
        m = _lowdim({'ema_decay': 0.5, 'ema_num_updates': True})
        g = m.graph
        m.enable_data_parallel(world, mode=mode)
        fake = _EmaCpuLib(g)
        g.lib = fake
        g._stream_ptr = lambda: None
        gen = torch.Generator().manual_seed(1000 + rank)
        want = g.params.numpy().copy()
        follows, once = True, True
        for step in range(3):
            g.grads.copy_(torch.randn(g.flat_size, generator=gen) * 1e-2)
            fake.ema_calls = []
            g.run_backward_overlapped(with_adam=True)
            want = ema_rule(want, g.params.numpy(), ema_one_minus_decay(0.5, step))      # the parameters this step left
            follows = follows and want.tobytes() == g.ema.numpy().tobytes()
            once = once and fake.ema_calls == [(0, g.flat_size)]
        g.gather_optimizer_state()
        sd = g.state_dict()
        out[mode] = (g.ema.clone(), g.params.clone(), follows, once, g.ema_updates, float(sd[EMA_COUNTER]))
    ea, pa, fa, oa, na, ca = out['allreduce']
    es, ps, fs, os_, ns, cs = out['sharded']
    other = es.clone()
    dist.broadcast(other, src=0)
    q.put((rank, bool(torch.equal(ea, es)), bool(torch.equal(other, es)), fa and fs, oa and os_, (na, ns, ca, cs),
           bool(torch.equal(pa, ps)), not torch.equal(es, ps)))
    dist.destroy_process_group()


def test_data_parallel_shadows_two_ranks():
    """Three steps in 'allreduce' and 'sharded' mode: one EMA launch over the whole flat buffer per step, behind the last
    all-gather; the shadows follow the rule over the parameters each step left and are bit-identical between modes and ranks."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_ema_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, modes_equal, ranks_equal, follows, once, counters, params_equal, moved in res:
        assert params_equal and modes_equal, "sharded and all-reduce shadows diverged on rank %d" % rank
        assert ranks_equal, "ranks hold different shadows"
        assert follows, "shadows do not follow the rule over the recorded parameters on rank %d" % rank
        assert once, "a step's EMA launches do not cover the flat buffer exactly once on rank %d" % rank
        assert counters == (3, 3, 3.0, 3.0) and moved


# ---------------------------------------------------------------- checkpoints
def _stepped(conf, seed=7, steps=2):
    """An EMA model whose shadows differ from its variables: `steps` emulated updates on perturbed parameters."""
    m = _lowdim(conf, seed=seed)
    g = m.graph
    gen = torch.Generator().manual_seed(3)
    mask = torch.zeros(g.flat_size)             # the padding between variables stays zero (it is in no checkpoint)
    for v in g.variables.values():
        mask[v.offset:v.offset + v.size] = 1.0
    for _ in range(steps):
        g.params.add_(torch.randn(g.flat_size, generator=gen) * 1e-2 * mask)
        w = ema_one_minus_decay(g.ema_decay, g.ema_updates if g.ema_num_updates else None)
        g.ema.copy_(torch.from_numpy(ema_rule(g.ema.numpy(), g.params.numpy(), w)))
        g.ema_updates += 1
    return m


def test_checkpoint_names_and_round_trip(tmp_path):
    from dynamic_multiview_3d_amd import tf_checkpoint
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    m = _stepped({'ema_decay': 0.9, 'ema_num_updates': True})
    g = m.graph
    plain = _lowdim({})
    assert plain.graph.ema is None and not any(EMA_SLOT in k for k in plain.graph.state_dict())
    shadows = {k + '/' + EMA_SLOT for k in g.variables}
    assert set(g.state_dict()) == set(plain.graph.state_dict()) | shadows | {EMA_COUNTER}
    assert EMA_SLOT == 'ExponentialMovingAverage' and EMA_COUNTER == 'ExponentialMovingAverage/num_updates'
    prefix = m.saver.save(None, str(tmp_path / 'model'), global_step=2)
    sd = tf_checkpoint.read_checkpoint(prefix)
    assert shadows <= set(sd) and sd[EMA_COUNTER].dtype == np.float32 and float(sd[EMA_COUNTER]) == 2.0
    for k, v in g.variables.items():
        np.testing.assert_array_equal(sd[k + '/' + EMA_SLOT], g.ema[v.offset:v.offset + v.size].view(v.shape).numpy())
        assert not np.array_equal(sd[k + '/' + EMA_SLOT], sd[k]) or not np.abs(sd[k]).sum()
    # restore reproduces variables, shadows and the counter
    m2 = _lowdim({'ema_decay': 0.9, 'ema_num_updates': True}, seed=8)
    assert not torch.equal(m2.graph.params, g.params) and m2.graph.ema_updates == 0
    m2.saver.restore(None, prefix)
    assert torch.equal(m2.graph.params, g.params) and torch.equal(m2.graph.ema, g.ema) and m2.graph.ema_updates == 2
    assert list(m2.graph.get_ema_variables()) == list(g.variables)
    for k, a in m2.graph.get_ema_variables().items():
        np.testing.assert_array_equal(a, sd[k + '/' + EMA_SLOT])
    # a checkpoint without shadows: a resume that turns the switch on
    bare = plain.saver.save(None, str(tmp_path / 'bare'))
    m3 = _stepped({'ema_decay': 0.9}, seed=9)
    m3.saver.restore(None, bare)
    assert torch.equal(m3.graph.params, plain.graph.params) and torch.equal(m3.graph.ema, m3.graph.params) and m3.graph.ema_updates == 0
    # some of the shadows: KeyError; shadows into a model without the switch: unexpected keys, as ever
    for drop in ('fc1/Matrix/' + EMA_SLOT, EMA_COUNTER):
        part = {k: v for k, v in sd.items() if k != drop}
        tf_checkpoint.write_checkpoint(str(tmp_path / 'part'), part)
        with pytest.raises(KeyError, match=EMA_SLOT):
            _lowdim({'ema_decay': 0.9}).saver.restore(None, str(tmp_path / 'part'))
    with pytest.raises(KeyError, match=EMA_SLOT):
        _lowdim({}).saver.restore(None, prefix)
    # a variable without a gradient has a shadow too, equal to it
    h = AppFlowHighDimAngle({'batch_size': 2, 'learning_rate': 1e-4, 'ema_decay': 0.9}, load_tfrec=False, device='cpu')
    dead = [k for k, v in h.graph.variables.items() if not v.has_grad]
    assert dead and all(k.split('/')[0] in ('a0', 'a1') for k in dead)
    hs = h.graph.state_dict()
    for k in dead:
        assert torch.equal(hs[k + '/' + EMA_SLOT], hs[k]) and k + '/Adam' not in hs
    # a model built without a loss holds the shadows as well
    r = _lowdim_noloss({'ema_decay': 0.9})
    assert r.graph.ema is not None
    r.saver.restore(None, prefix)
    assert torch.equal(r.graph.ema, g.ema)


def _lowdim_noloss(conf):
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    return AppFlowLowDimAngle(dict({'batch_size': 2, 'learning_rate': 1e-4}, **conf), load_tfrec=False, build_loss=False, device='cpu')


# ---------------------------------------------------------------- ema_weights() on a CPU graph
def test_ema_weights_context_on_a_cpu_graph():
    m = _stepped({'ema_decay': 0.9})
    g = m.graph
    p0, e0 = g.params.clone(), g.ema.clone()
    assert not torch.equal(p0, e0)
    with m.ema_weights() as inner:
        assert inner is g
        assert torch.equal(g.params, e0) and torch.equal(g.ema, p0)
        for call in (g.train_step, m.train_step, g.state_dict, g.ema_weights().__enter__):
            with pytest.raises(RuntimeError, match='ema_weights'):
                call()
    assert torch.equal(g.params.view(torch.int32), p0.view(torch.int32)) and torch.equal(g.ema.view(torch.int32), e0.view(torch.int32))
    with pytest.raises(ZeroDivisionError):
        with g.ema_weights():
            1 / 0
    assert torch.equal(g.params.view(torch.int32), p0.view(torch.int32)) and torch.equal(g.ema.view(torch.int32), e0.view(torch.int32))
    assert not g._ema_swapped
    with pytest.raises(RuntimeError):
        _lowdim({}).graph.ema_weights().__enter__()
    with pytest.raises(RuntimeError):
        _lowdim({}).graph.get_ema_variables()


def test_evaluate_selects_the_weights():
    import types
    on, off = _stepped({'ema_decay': 0.9}), _lowdim({})
    seen = []
    for m in (on, off):
        m._evaluate = types.MethodType(lambda self, data, n: {'swapped': seen.append(self.graph._ema_swapped) or self.graph._ema_swapped}, m)
    assert on.evaluate(None, 1) == {'swapped': True, 'weights': 'ema'}
    assert on.evaluate(None, 1, weights='raw') == {'swapped': False, 'weights': 'raw'}
    assert on.evaluate(None, 1, weights='ema')['weights'] == 'ema'
    assert off.evaluate(None, 1) == {'swapped': False} and off.evaluate(None, 1, weights='raw') == {'swapped': False}
    with pytest.raises(ValueError):
        off.evaluate(None, 1, weights='ema')
    with pytest.raises(ValueError):
        on.evaluate(None, 1, weights='best')
    assert seen == [True, False, True, False, False]
