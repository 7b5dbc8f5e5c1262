"""Global-norm gradient clipping on the CPU (no GPU): the numpy twin of mv3d_grad_clip_scale against a plain float64 restatement,
the conf switch, argument validation of the two C-ABI entry points, what a step launches with and without the switch, the
data-parallel schedule on gloo (world 2, the twin in place of the kernel) and the train driver's log line."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import GN_CHUNK
from dynamic_multiview_3d_amd.model_base import grad_clip_from_conf, grad_clip_rule
from tests.test_dist_cpu import _CpuLib
from tests.test_optimizers_host import B64, _appflow, _free_port, _labels, _lowdim

E_INVAL, E_WORKSPACE = -1, -3
INF = math.inf


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------- the rule
def _plain(g, pre_scale, clip):
    """The rule in plain float64, no order contract: the reference the twin is within an fp32 ulp of."""
    n = math.sqrt(float((np.asarray(g, np.float64) ** 2).sum())) * float(pre_scale)
    return n, (clip / n if n > clip else 1.0)


@pytest.mark.parametrize("count", [1, 3, 1000, GN_CHUNK - 1, GN_CHUNK + 1, 3 * GN_CHUNK + 7, 257 * GN_CHUNK + 5])
def test_rule_against_plain_float64(count):
    """The double sum of exact squares carries a relative error of at most count * 2^-53 (below 1e-9 here), the root and the
    product with pre_scale round to fp32 once each: the twin's norm is within 1 fp32 ulp of the float64 value.  Not clipped (the
    norm at or below the clip, or clip = inf): scale exactly 1 and gscale exactly pre_scale; clipped: norm * scale within 1 ulp
    of the clip (one rounding of the quotient, relative 2^-24, the product is then taken in float64)."""
    rng = np.random.default_rng(count)
    g = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(np.float32)
    for pre in (np.float32(1.0), np.float32(0.5), np.float32(1.0 / 3.0)):
        n, s, gs = grad_clip_rule(g, pre, INF)
        assert n.dtype == s.dtype == gs.dtype == np.float32
        want, _ = _plain(g, pre, INF)
        assert abs(float(n) - want) <= _ulp(want), (count, float(pre), float(n), want)
        assert s == 1.0 and gs == pre
        for clip in (float(n), float(n) * 2.0, float(np.nextafter(n, np.float32(INF)))):      # n == clip, n < clip
            n2, s2, gs2 = grad_clip_rule(g, pre, clip)
            assert n2 == n and s2 == 1.0 and gs2.tobytes() == pre.tobytes()
        for clip in (float(n) / 2.0, float(n) * 0.999, float(np.nextafter(n, np.float32(0))), 1e-3 * float(n)):
            n2, s2, gs2 = grad_clip_rule(g, pre, clip)
            c32 = np.float32(clip)
            assert n2 == n and s2 < 1.0 and s2 == c32 / n and gs2 == pre * s2
            assert abs(float(n2) * float(s2) - float(c32)) <= _ulp(c32), (count, clip)


def test_rule_range():
    n, s, gs = grad_clip_rule(np.full(4096, 1e30, np.float32), 1.0, 1.0)           # fp32 squares would overflow
    assert np.isfinite(n) and abs(float(n) - 6.4e31) <= _ulp(6.4e31) and s == np.float32(1.0) / n and gs == s
    n, s, _ = grad_clip_rule(np.full(4096, -1e30, np.float32), 1.0, INF)
    assert np.isfinite(n) and s == 1.0
    g = np.ones(100, np.float32)
    g[37] = np.nan
    n, s, gs = grad_clip_rule(g, 0.5, 1.0)
    assert np.isnan(n) and s == 1.0 and gs == np.float32(0.5)                      # the NaN stays visible, the scale stays 1
    g[37] = -np.inf
    n, s, gs = grad_clip_rule(g, 0.5, 1.0)
    assert n == np.float32(INF) and s == 0.0 and gs == 0.0                          # the step is dropped
    n, s, _ = grad_clip_rule(g, 0.5, INF)
    assert n == np.float32(INF) and s == 1.0                                        # measure only: never a scale
    n, s, _ = grad_clip_rule(np.zeros(5, np.float32), 1.0, 1.0)
    assert n == 0.0 and s == 1.0


def test_grad_clip_from_conf():
    assert grad_clip_from_conf({}) is None
    for off in (None, 0, 0.0):
        assert grad_clip_from_conf({'grad_clip_norm': off}) is None
    assert grad_clip_from_conf({'grad_norm_log': False}) is None and grad_clip_from_conf({'grad_norm_log': None}) is None
    assert grad_clip_from_conf({'grad_clip_norm': 5}) == 5.0 and grad_clip_from_conf({'grad_clip_norm': 1e-3}) == 1e-3
    assert grad_clip_from_conf({'grad_norm_log': True}) == INF
    assert grad_clip_from_conf({'grad_norm_log': True, 'grad_clip_norm': None}) == INF
    assert grad_clip_from_conf({'grad_norm_log': True, 'grad_clip_norm': 2.0}) == 2.0
    for bad in (True, False, -1.0, -1e-9, float('nan'), INF, -INF, 1e39):
        with pytest.raises(ValueError):
            grad_clip_from_conf({'grad_clip_norm': bad})
    from dynamic_multiview_3d_amd import mv3d
    with pytest.raises(ValueError):                 # every model class reads the key, before it builds anything
        mv3d.mv3d_nobg_nodm({'batch_size': 2, 'grad_clip_norm': -1.0}, device='cpu')
    with pytest.raises(ValueError):
        _lowdim({'grad_clip_norm': float('nan')})


def test_graph_methods_and_the_switch():
    off, on, log = _lowdim({}).graph, _lowdim({'grad_clip_norm': 2.5}).graph, _lowdim({'grad_norm_log': True}).graph
    assert off.clip_norm is None and off.clip_buf is None and off._clip_ws is None
    for call in (off.grad_norm, off.clip_gradients):
        with pytest.raises(RuntimeError):
            call()
    assert on.clip_norm == 2.5 and log.clip_norm == INF
    for g in (on, log):
        assert g.grad_norm() is g.clip_buf and g.clip_buf.numel() == 2
        assert g._clip_ws.numel() * 8 >= g._clip_ws_bytes >= 8 * -(-g.flat_size // GN_CHUNK)
        assert g.plan_bwd_fused is None
    with pytest.raises(RuntimeError):
        on.enable_grad_clip(1.0)                    # after compile()
    from dynamic_multiview_3d_amd.graph import Graph
    for bad in (0, -1.0, float('nan'), True, 1e39, 1e-60):
        with pytest.raises(ValueError):
            Graph(device='cpu').enable_grad_clip(bad)
    # the gradient buffer is zero wherever no gradient is written: what lets clip_gradients() sum the whole flat buffer
    assert off.grads.abs().sum() == 0 and on.grads.numel() == on.flat_size


# ---------------------------------------------------------------- C ABI: validation before any launch
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def test_workspace_bytes(lib):
    assert lib.grad_clip_workspace_bytes(0) == 0 and lib.grad_clip_workspace_bytes(-5) == 0
    last = 0
    for count in (1, 2, GN_CHUNK - 1, GN_CHUNK, GN_CHUNK + 1, 31 * GN_CHUNK, 32 * GN_CHUNK + 1, 1000 * GN_CHUNK, 69535232, 1 << 33):
        need = lib.grad_clip_workspace_bytes(count)
        assert need >= 8 * -(-count // GN_CHUNK) and need >= last, count
        last = need


def test_grad_clip_scale_validation(lib):
    G, OUT, ST, WS = 4096, 1 << 16, 1 << 17, 1 << 20        # aligned stand-ins: nothing is dereferenced on a rejected call
    n = 3 * GN_CHUNK
    need = lib.grad_clip_workspace_bytes(n)

    def call(count=n, g=G, pre=1.0, clip=1.0, out=OUT, sa=ST, sb=ST + 32, ws=WS, nbytes=need):
        return lib.raw_grad_clip_scale(count, g, pre, clip, out, sa, sb, ws, nbytes, None)
    assert call(count=0) == E_INVAL and call(count=-8) == E_INVAL
    assert call(g=None) == E_INVAL and call(out=None) == E_INVAL and call(ws=None) == E_INVAL
    for g in (G + 4, G + 8):
        assert call(g=g) == E_INVAL
    assert '16-byte' in lib.last_error()
    assert call(out=OUT + 2) == E_INVAL and call(sa=ST + 1) == E_INVAL and call(sb=ST + 34) == E_INVAL
    for clip in (0.0, -0.0, -1.0, float('nan'), -INF):
        assert call(clip=clip) == E_INVAL, clip
    assert 'clip_norm' in lib.last_error()
    for pre in (0.0, -0.5, float('nan'), INF, -INF):
        assert call(pre=pre) == E_INVAL, pre
    assert 'pre_scale' in lib.last_error()
    assert call(nbytes=need - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
    assert call(ws=WS + 8) == E_WORKSPACE


# ---------------------------------------------------------------- what a step launches
class _Recorder:
    """Keeps every call the graph makes on its library, with the arguments (none of them runs: no device)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, a))


def _calls(g, run):
    real, g.lib = g.lib, _Recorder()
    g._stream_ptr = lambda: None
    try:
        run()
    finally:
        fake, g.lib = g.lib, real
        del g._stream_ptr
    return fake.calls


@pytest.fixture(scope="module")
def b64_trio():
    return _appflow(dict(B64)).graph, _appflow(dict(B64, grad_clip_norm=None)).graph, _appflow(dict(B64, grad_clip_norm=1.5)).graph


def test_step_launch_list_with_and_without_the_switch(b64_trio):
    absent, none, on = b64_trio
    # keys absent or None: nothing allocated, the same three plans, the same direct calls
    assert none.clip_norm is None and none.clip_buf is None and none._clip_ws is None
    for a, b in ((absent.plan_fwd, none.plan_fwd), (absent.plan_bwd, none.plan_bwd), (absent.plan_bwd_fused, none.plan_bwd_fused)):
        assert a is not None and _labels(a) == _labels(b)
    names = lambda calls: [c[0] for c in calls]
    want = names(_calls(absent, absent.train_step))
    assert names(_calls(none, none.train_step)) == want and 'grad_clip_scale' not in want
    assert [n for n in want if not n.startswith('plan_')] == ['adam_step_dev', 'adam_advance', 'adam_advance']
    # switch on: the recorded forward and plain reverse plans are the parent's; the fused plan is not recorded
    assert _labels(on.plan_fwd) == _labels(absent.plan_fwd) and _labels(on.plan_bwd) == _labels(absent.plan_bwd)
    assert on.plan_bwd_fused is None
    assert not any('grad_sumsq' in l or 'grad_clip' in l for l in _labels(on.plan_fwd) + _labels(on.plan_bwd))
    calls = _calls(on, on.train_step)
    assert names(calls) == ['plan_run', 'plan_run_range_multi', 'grad_clip_scale', 'adam_step_dev', 'adam_advance', 'adam_advance']
    assert calls[0][1][0] == on.plan_fwd
    plan, begin, end = calls[1][1][:3]
    assert plan == on.plan_bwd and (begin, end) == (0, on.n_launch_bwd) and calls[1][1][-1] == 0       # plan_bwd whole, joined
    count, gptr, pre, clip, out, sa, sb, ws, nbytes, _ = calls[2][1]
    assert count == on.flat_size and gptr == on.grads.data_ptr() and pre == 1.0 and clip == 1.5
    assert out == on.clip_buf.data_ptr() and (sa, sb) == (on.opt_state.data_ptr(), on.opt_state.data_ptr() + 32)
    assert ws == on._clip_ws.data_ptr() and nbytes == on._clip_ws_bytes >= _lib.lib().grad_clip_workspace_bytes(on.flat_size)
    count, p, gr, m, v, state, nskip = calls[3][1][:7]
    assert count == on.flat_size and nskip == 0 and state == on.opt_state.data_ptr()
    assert (p, gr, m, v) == (on.params.data_ptr(), on.grads.data_ptr(), on.adam_m.data_ptr(), on.adam_v.data_ptr())


# ---------------------------------------------------------------- data parallel (gloo, world 2)
class _ClipCpuLib(_CpuLib):
    """tests/test_dist_cpu.py's stand-in with mv3d_grad_clip_scale = the numpy twin on the flat gradient buffer."""

    def __init__(self, g):
        super().__init__(g)
        self.clip_calls = []

    def grad_clip_scale(self, count, gptr, pre, clip, out, sa, sb, ws, nbytes, stream):
        g = self.g
        assert gptr == g.grads.data_ptr() and count == g.flat_size and out == g.clip_buf.data_ptr()
        assert (sa, sb) == (g.opt_state.data_ptr(), g.opt_state.data_ptr() + 32)
        n, s, gs = grad_clip_rule(g.grads.numpy(), pre, clip)
        g.clip_buf.numpy()[:] = (n, s)
        g.opt_state.numpy()[[6, 14]] = gs
        self.clip_calls.append((float(pre), float(np.float32(clip))))       # what the C ABI's float argument holds


STEPS = 2


def _dp_clip_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from dynamic_multiview_3d_amd import parallel
    parallel.init_from_env('gloo')
    flat = _lowdim({}).graph.flat_size
    gens = [torch.Generator().manual_seed(1000 + r) for r in range(world)]
    per_rank = [[torch.randn(flat, generator=gen) * 1e-2 for gen in gens] for _ in range(STEPS)]
    norm0 = float(grad_clip_rule((per_rank[0][0] + per_rank[0][1]).numpy(), np.float32(0.5), INF)[0])
    clip = norm0 / 2                                    # the clip is active in the first step
    out = {}
    for mode in ('allreduce', 'sharded', 'single'):
        m = _lowdim({'grad_clip_norm': clip})
        g = m.graph
        if mode != 'single':
            m.enable_data_parallel(world, mode=mode)
        else:
            g.world_size = world                        # one process on the summed gradients: pre_scale = 1 / world, no exchange
        fake = _ClipCpuLib(g)
        g.lib = fake
        g._stream_ptr = lambda: None
        seen = []
        for step in range(STEPS):
            if mode == 'single':
                g.grads.copy_(per_rank[step][0] + per_rank[step][1])
                g.clip_gradients()
                g.apply_optimizer()
            else:
                g.grads.copy_(per_rank[step][rank])
                g.run_backward_clipped()
            seen.append(g.grad_norm().clone())
        ok = fake.adam_calls == [(0, g.flat_size)] * STEPS and fake.clip_calls == [(0.5, float(np.float32(clip)))] * STEPS \
            and not getattr(g, '_slots_sharded', False) and float(g.opt_state[6]) == float(g.opt_state[14])
        g.state_dict()                                  # complete slots on every rank: no gather needed
        out[mode] = (g.params.clone(), g.adam_m.clone(), g.adam_v.clone(), torch.stack(seen), ok)
    pa, ma, va, na, oka = out['allreduce']
    ps, ms, vs, ns, oks = out['sharded']
    p1, m1, v1, n1, ok1 = out['single']
    other = ps.clone()
    dist.broadcast(other, src=0)
    bits = lambda a, b: bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    q.put((rank, bits(pa, ps) and bits(ma, ms) and bits(va, vs) and bits(na, ns), bits(other, ps),
           bits(pa, p1) and bits(ma, m1) and bits(va, v1) and bits(na, n1), oka and oks and ok1,
           float(na[0, 0]), norm0, float(na[0, 1])))
    dist.destroy_process_group()


def test_data_parallel_clip_two_ranks():
    """Both dp_modes run the bucketed all-reduce, one norm over the summed buffer and one optimiser launch over the whole buffer:
    bit-identical parameters, slots and [norm, scale] on both ranks and in both modes, equal to one process stepping on the summed
    gradients with pre_scale = 0.5; the clip (half the first step's norm) is active."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_clip_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, modes_equal, ranks_equal, single_equal, ok, norm, norm0, scale in res:
        assert modes_equal, "sharded and all-reduce modes diverged on rank %d" % rank
        assert ranks_equal, "ranks hold different weights"
        assert single_equal, "data-parallel step differs from the single-process step on the summed gradients on rank %d" % rank
        assert ok, "launches, records or slots are not what the clipped schedule states on rank %d" % rank
        assert norm == norm0 and scale == float(np.float32(np.float32(norm0 / 2) / np.float32(norm0))) and scale < 1.0


# ---------------------------------------------------------------- the train driver's log line
def test_train_log_row_carries_the_norm_only_with_the_switch():
    import json
    from dynamic_multiview_3d_amd import train
    off, on, log = _lowdim({}), _lowdim({'grad_clip_norm': 2.0}), _lowdim({'grad_norm_log': True})
    assert train.training_log_row(off, 10, 0.25) == {'itr': 10, 'training_loss': 0.25}
    on.graph.clip_buf.copy_(torch.tensor([8.0, 0.25]))
    row = train.training_log_row(on, 20, 0.5)
    assert row == {'itr': 20, 'training_loss': 0.5, 'grad_norm': 8.0, 'grad_clip_scale': 0.25}
    assert json.loads(json.dumps(row)) == row
    log.graph.clip_buf.copy_(torch.tensor([3.0, 1.0]))
    assert train.training_log_row(log, 0, 1.0) == {'itr': 0, 'training_loss': 1.0, 'grad_norm': 3.0, 'grad_clip_scale': 1.0}
