"""Decoupled weight decay on the CPU (no GPU): the numpy twin of mv3d_weight_decay_step against the closed form, argument
validation of the two new C-ABI entry points, the model's decay table, where the decay launches sit in the schedules, and two
gloo ranks against a single-process twin."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.model_base import ema_one_minus_decay, ema_rule, weight_decay_factor, weight_decay_rule
from tests.test_dist_cpu import _CpuLib
from tests.test_ema_host import _direct_calls
from tests.test_optimizers_host import B64, _appflow, _free_port, _lowdim

E_INVAL = -1


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("f", [1e-6, 1e-3, 0.5])
def test_weight_decay_rule_follows_the_closed_form(f):
    """p_k = p_0 (1 - f)^k.  Two fp32 roundings per step (the product, the difference), each <= 2^-24 of a magnitude <= |p_0|: the
    bound argued in test_ema_rule_follows_the_closed_form for its three roundings of magnitudes <= 2 max, k * 4e-7 * |p_0| after
    k steps, holds here with room."""
    rng = np.random.default_rng(3)
    p0 = (rng.standard_normal(4096) * 10.0 ** rng.integers(-4, 4, 4096)).astype(np.float32)
    f = np.float32(f)
    p, p64 = p0.copy(), p0.astype(np.float64)
    bound = 4e-7 * np.abs(p64)
    worst = 0.0
    for k in range(1, 201):
        p = weight_decay_rule(p, [(0, p.size)], f)
        assert p.dtype == np.float32
        err = np.abs(p.astype(np.float64) - p64 * (1.0 - float(f)) ** k)
        worst = max(worst, float((err / bound).max()) / k)
        assert (err <= k * bound).all(), (k, float((err / bound).max()))
    print("f %g: worst error / (k * 4e-7 * |p0|) = %.3g" % (float(f), worst))


def test_weight_decay_rule_leaves_the_rest_alone():
    rng = np.random.default_rng(4)
    p = rng.standard_normal(256).astype(np.float32)
    p[[8, 40, 100]] = 0.0
    p[[9, 41, 101]] = -0.0
    ranges = [(8, 16), (32, 64), (128, 132)]
    out = weight_decay_rule(p, ranges, np.float32(0.25))
    inside = np.zeros(256, bool)
    for a, b in ranges:
        inside[a:b] = True
    assert out[~inside].tobytes() == p[~inside].tobytes()                   # outside the ranges: the same bits
    zero = p == 0
    assert out.view(np.int32)[zero].tobytes() == p.view(np.int32)[zero].tobytes()       # +0 and -0 keep their bits, inside and outside
    moved = inside & ~zero
    assert (out[moved] == p[moved] - p[moved] * np.float32(0.25)).all() and (out[moved] != p[moved]).all()
    assert weight_decay_rule(p, ranges, np.float32(0.0)).tobytes() == p.tobytes()       # f = 0: the identity, -0 included
    assert weight_decay_rule(p, [], np.float32(0.5)).tobytes() == p.tobytes()
    assert weight_decay_rule(p, [(248, 300)], np.float32(0.5)).size == 256              # a range past the end is clipped
    q = p.copy()
    weight_decay_rule(p, ranges, np.float32(0.25))
    assert p.tobytes() == q.tobytes()                                       # the input is left alone


def test_fused_rule_is_decay_then_ema():
    rng = np.random.default_rng(5)
    p, s = rng.standard_normal(512).astype(np.float32), rng.standard_normal(512).astype(np.float32)
    ranges = [(0, 4), (64, 260)]
    f, w = np.float32(0.01), ema_one_minus_decay(0.9)
    p2, s2 = weight_decay_rule(p, ranges, f, shadow=s, one_minus_decay=w)
    want_p = weight_decay_rule(p, ranges, f)
    assert p2.tobytes() == want_p.tobytes() and s2.tobytes() == ema_rule(s, want_p, w).tobytes()
    assert s2[300:].tobytes() == ema_rule(s, p, w)[300:].tobytes()          # outside the ranges the EMA sees p itself


def test_weight_decay_factor_is_rounded_once():
    f = weight_decay_factor(np.float32(1e-4), 0.01)
    assert f.dtype == np.float32 and f == np.float32(float(np.float32(1e-4)) * 0.01)


# ---------------------------------------------------------------- C ABI: validation before any launch
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def test_weight_decay_step_validation(lib):
    P, S, T = 4096, 1 << 20, 1 << 22                # aligned stand-ins: nothing is dereferenced on a rejected call
    wd = lib.raw_weight_decay_step
    assert _lib.DECAY_MAX_RANGES == 1024
    assert wd(None, None, 0, 8, T, 1, 0.1, 0.0, None) == E_INVAL
    assert wd(P + 4, None, 0, 8, T, 1, 0.1, 0.0, None) == E_INVAL           # misaligned parameters, shadows, table
    assert wd(P, S + 8, 0, 8, T, 1, 0.1, 0.5, None) == E_INVAL
    assert wd(P, None, 0, 8, T + 4, 1, 0.1, 0.0, None) == E_INVAL
    assert wd(P, None, 0, 8, None, 1, 0.1, 0.0, None) == E_INVAL            # ranges announced, no table
    assert wd(P, None, 2, 8, T, 1, 0.1, 0.0, None) == E_INVAL               # lo not a multiple of 4, with and without a shadow
    assert wd(P, S, 2, 8, T, 1, 0.1, 0.5, None) == E_INVAL
    assert wd(P, None, 0, 6, T, 1, 0.1, 0.0, None) == E_INVAL               # hi: only the fused form takes the buffers' unaligned end
    assert 'multiple of 4' in lib.last_error()
    assert wd(P, None, -4, 8, T, 1, 0.1, 0.0, None) == E_INVAL
    assert wd(P, None, 8, 8, T, 1, 0.1, 0.0, None) == E_INVAL and wd(P, None, 8, 4, T, 1, 0.1, 0.0, None) == E_INVAL
    assert wd(P, None, 0, 8, T, 1025, 0.1, 0.0, None) == E_INVAL            # above the cap
    assert '1024' in lib.last_error()
    assert wd(P, None, 0, 8, T, -1, 0.1, 0.0, None) == E_INVAL
    for f in (-1e-6, 1.0, 1.5, float('nan'), float('inf'), -float('inf')):
        assert wd(P, None, 0, 8, T, 1, f, 0.0, None) == E_INVAL, f
        assert wd(P, S, 0, 8, T, 1, f, 0.5, None) == E_INVAL, f
    for w in (-1e-3, 1.0 + 1e-6, 2.0, float('nan'), float('inf')):
        assert wd(P, S, 0, 8, T, 1, 0.1, w, None) == E_INVAL, w
    assert 'one_minus_decay' in lib.last_error()


def test_opt_set_lr_validation(lib):
    A = 4096
    assert lib.raw_opt_set_lr(None, 1e-3, None) == E_INVAL
    assert lib.raw_opt_set_lr(A + 2, 1e-3, None) == E_INVAL
    for lr in (-1e-6, float('nan'), float('inf'), -float('inf')):
        assert lib.raw_opt_set_lr(A, lr, None) == E_INVAL, lr
    assert 'lr' in lib.last_error()


# ---------------------------------------------------------------- the model's table
def _check_table(g):
    r = g._decay_ranges
    assert r and g._decay_table.dtype == torch.int64 and g._decay_table.tolist() == [x for ab in r for x in ab]
    assert all(a % 4 == 0 and b % 4 == 0 and a < b for a, b in r)
    assert all(x[1] <= y[0] for x, y in zip(r, r[1:])) and r[0][0] >= 0 and r[-1][1] <= g.flat_size      # sorted, disjoint
    assert len(r) <= _lib.DECAY_MAX_RANGES
    want = sorted((v.offset, v.offset + -(-v.size // 4) * 4) for k, v in g.variables.items()
                  if v.has_grad and (k.endswith('/w') or k.endswith('/Matrix')))
    assert r == want
    return r


def test_table_holds_the_weights_with_a_gradient():
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    h = AppFlowHighDimAngle({'batch_size': 2, 'learning_rate': 1e-4, 'weight_decay': 0.01}, load_tfrec=False, device='cpu').graph
    r = _check_table(h)
    dead = [v for k, v in h.variables.items() if not v.has_grad]
    assert dead and {v.name.split('/')[0] for v in dead} == {'a0', 'a1'} and any(v.name.endswith('/Matrix') or v.name.endswith('/w') for v in dead)
    assert not any(a <= v.offset < b for v in dead for a, b in r)
    biases = [v for k, v in h.variables.items() if v.has_grad and not (k.endswith('/w') or k.endswith('/Matrix'))]
    assert biases and not any(a <= v.offset < b for v in biases for a, b in r)
    off = AppFlowHighDimAngle({'batch_size': 2, 'learning_rate': 1e-4}, load_tfrec=False, device='cpu').graph
    assert off.weight_decay is None and off._decay_table is None and off._decay_ranges == []
    del h, off
    from tests.layer_cases import MULTIOBJ_256_CONF
    m = MultiObjectAppFlow(dict(MULTIOBJ_256_CONF, batch_size=2, learning_rate=1e-4, weight_decay=0.01), load_tfrec=False, device='cpu').graph
    assert 26 < len(_check_table(m)) <= _lib.DECAY_MAX_RANGES            # the largest model fits the cap
    with pytest.raises(RuntimeError):
        m.enable_weight_decay(0.1)                  # after compile()
    with pytest.raises(RuntimeError):
        m.enable_lr_schedule({'kind': None, 'base': 1e-3, 'warmup': 2})


def test_too_many_ranges_are_refused(monkeypatch):
    monkeypatch.setattr(_lib, 'DECAY_MAX_RANGES', 3)
    with pytest.raises(ValueError, match='at most 3'):
        _lowdim({'weight_decay': 0.01})


# ---------------------------------------------------------------- where the launches sit
def _decay_tiles(g, calls, f, w):
    """The mv3d_weight_decay_step calls of one update cover [0, flat_size) exactly once, every one with the flat bases, the table
    and the step's scalars."""
    spans = []
    for name, a in calls:
        if name == 'weight_decay_step':
            params, shadow, lo, hi, table, n, fk, wk, _ = a
            assert params == g.params.data_ptr() and shadow == (g.ema.data_ptr() if g.ema is not None else None)
            assert table == g._decay_table.data_ptr() and n == len(g._decay_ranges) and lo % 4 == 0 and hi % 4 == 0
            assert np.float32(fk).tobytes() == np.float32(f).tobytes() and wk == (float(w) if g.ema is not None else 0.0)
            spans.append((lo, hi))
    spans.sort()
    assert spans and spans[0][0] == 0 and spans[-1][1] == g.flat_size
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
    return spans


@pytest.mark.parametrize("ema", [False, True])
def test_decay_calls_cover_the_flat_buffer_once(ema):
    g = _appflow(dict(B64, weight_decay=0.1, **({'ema_decay': 0.999} if ema else {}))).graph
    assert g.plan_bwd_fused is not None and len(g._decay_ranges) == 26
    f, w = weight_decay_factor(np.float32(1e-4), 0.1), ema_one_minus_decay(0.999)
    # the fused step: the fc ranges go out in front of everything on the main stream (the event is recorded behind them)
    calls = _direct_calls(g, g.run_backward_fused)
    names = [c[0] for c in calls]
    assert 'ema_step' not in names                                          # with EMA on the fused form replaces it, one for one
    assert [n for n in names if n != 'weight_decay_step'] == ['adam_step_dev', 'adam_advance', 'adam_advance']
    spans = _decay_tiles(g, calls, f, w)
    assert all(tuple(r) in spans for r in g._fc_ranges)
    nfc = len(g._fc_ranges)
    assert names[:2 + nfc] == ['adam_step_dev', 'adam_advance'] + ['weight_decay_step'] * nfc
    assert [(c[1][2], c[1][3]) for c in calls[2:2 + nfc]] == [tuple(r) for r in g._fc_ranges]
    assert g.global_step == 1 and g.ema_updates == (1 if ema else 0)
    # plain / clipped / accumulation: one launch over the whole buffer
    calls = _direct_calls(g, g.apply_optimizer)
    assert [c[0] for c in calls] == ['adam_step_dev', 'adam_advance', 'adam_advance', 'weight_decay_step']
    assert _decay_tiles(g, calls, f, w) == [(0, g.flat_size)]
    # the bucketed optimiser issues it per slice: the buckets tile the buffer
    buckets = sorted((lo, hi) for _, lo, hi in g.grad_buckets if hi > lo)
    assert buckets[0][0] == 0 and buckets[-1][1] == g.flat_size and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
    # f >= 1 raises when the step is issued, before any launch
    g.weight_decay = 2e4
    for run in (g.train_step, g.apply_optimizer):
        with pytest.raises(ValueError, match='below 1'):
            _direct_calls(g, run)


# ---------------------------------------------------------------- data parallel (gloo, world 2)
WD = 100.0          # f = float32(1e-4 * 100) = 0.01: moves bits in three steps


class _DecayCpuLib(_CpuLib):
    """tests/test_dist_cpu.py's stand-in with mv3d_weight_decay_step = the numpy rule on the flat buffers."""

    def __init__(self, g):
        super().__init__(g)
        self.decay_calls = []

    def weight_decay_step(self, params, shadow, lo, hi, table, n, f, w, stream):
        g = self.g
        assert params == g.params.data_ptr() and shadow is None and table == g._decay_table.data_ptr() and n == len(g._decay_ranges)
        ranges = [(max(a, lo), min(b, hi)) for a, b in g._decay_ranges if min(b, hi) > max(a, lo)]
        g.params.numpy()[:] = weight_decay_rule(g.params.numpy(), ranges, np.float32(f))
        self.decay_calls.append((lo, hi))


def _dp_decay_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from dynamic_multiview_3d_amd import parallel
    parallel.init_from_env('gloo')
    gens = [torch.Generator().manual_seed(1000 + r) for r in range(world)]
    flat = _lowdim({}).graph.flat_size
    grads = [[torch.randn(flat, generator=gen) * 1e-2 for gen in gens] for _ in range(3)]       # [step][rank]: every rank knows them all

    def twin(decay_ranges):
        """Single process, no decay key: both ranks' gradients summed on the host (gradient scale 1 / world), and with
        decay_ranges the rule applied on the host after every update."""
        t = _lowdim({}).graph
        t.world_size = world
        t.upload_optimizer_state()
        t.lib = _CpuLib(t)
        t._stream_ptr = lambda: None
        for step in range(3):
            t.grads.copy_(grads[step][0] + grads[step][1])
            t.apply_optimizer()
            if decay_ranges:
                t.params.numpy()[:] = weight_decay_rule(t.params.numpy(), decay_ranges, weight_decay_factor(np.float32(1e-4), WD))
        return t.params.clone()

    out = {}
    for mode in ('allreduce', 'sharded'):
        m = _lowdim({'weight_decay': WD})
        g = m.graph
        m.enable_data_parallel(world, mode=mode)
        fake = _DecayCpuLib(g)
        g.lib = fake
        g._stream_ptr = lambda: None
        once = True
        for step in range(3):
            g.grads.copy_(grads[step][rank])
            fake.decay_calls = []
            g.run_backward_overlapped(with_adam=True)
            once = once and fake.decay_calls == [(0, g.flat_size)]
        out[mode] = (g.params.clone(), once, g.global_step)
    want, undecayed = twin(g._decay_ranges), twin(None)
    pa, oa, na = out['allreduce']
    ps, os_, ns = out['sharded']
    other = ps.clone()
    dist.broadcast(other, src=0)
    q.put((rank, bool(torch.equal(pa, ps)), bool(torch.equal(other, ps)), bool(torch.equal(ps, want)), oa and os_, (na, ns),
           not torch.equal(ps, undecayed)))
    dist.destroy_process_group()


def test_data_parallel_decay_two_ranks():
    """Three steps in 'allreduce' and 'sharded' mode: one decay launch over the whole flat buffer per step; the weights are
    bit-identical between modes and ranks and equal a single-process twin without the key that applies the rule on the host."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_decay_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, modes_equal, ranks_equal, twin_equal, once, counters, moved in res:
        assert modes_equal, "sharded and all-reduce weights diverged on rank %d" % rank
        assert ranks_equal, "ranks hold different weights"
        assert twin_equal, "the weights differ from the single-process twin's on rank %d" % rank
        assert once, "a step's decay launches do not cover the flat buffer exactly once on rank %d" % rank
        assert counters == (3, 3) and moved
