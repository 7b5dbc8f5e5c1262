"""Gradient accumulation on the CPU (no GPU): the numpy twin of mv3d_grad_accumulate against plain float64 sums, the conf switch,
the graph's methods, argument validation of the two new C-ABI entry points, what the micro-steps of a cycle launch with and
without the switch, the data-parallel schedule on gloo (world 2, the twins in place of the kernels) and the train driver's loop."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import GN_CHUNK, Graph
from dynamic_multiview_3d_amd.model_base import grad_accum_from_conf, grad_accum_rule, grad_clip_rule
from tests.test_grad_clip_host import _calls, _ClipCpuLib
from tests.test_optimizers_host import B64, _appflow, _free_port, _labels, _lowdim

E_INVAL, E_WORKSPACE = -1, -3
STORE, ADD, FINISH = 0, 1, 2
U = 2.0 ** -24                      # unit roundoff of float32


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_rule_against_plain_float64(n):
    """((g1 + g2) + g3) .. in float32 makes n - 1 roundings per element, each relative U = 2^-24 of a partial sum that is at most
    sum |g_i| (1 + U)^(n - 2) in magnitude: |twin - exact| <= gamma_(n-1) * sum |g_i| with gamma_k = k U / (1 - k U) (Higham,
    Accuracy and Stability, 4.4).  The loss mean adds the rounding of 1 / n and of the product: gamma_(n+1) * sum |l_i| / n.  One
    gradient is returned as it is; denormal results are exact (fp32 addition of denormals does not round)."""
    rng = np.random.default_rng(n)
    gs = [(rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 6, 5000)).astype(np.float32) for _ in range(n)]
    for g in gs:
        g[:4] = (0.0, -0.0, 1e-40, -3e-45)
    losses = [np.float32(v) for v in rng.uniform(0.01, 3.0, n)]
    total, mean = grad_accum_rule(gs, losses)
    assert total.dtype == np.float32 and mean.dtype == np.float32 and total.shape == gs[0].shape
    exact = np.sum([g.astype(np.float64) for g in gs], axis=0)
    mag = np.sum([np.abs(g.astype(np.float64)) for g in gs], axis=0)
    gamma = lambda k: k * U / (1 - k * U)
    assert np.all(np.abs(total.astype(np.float64) - exact) <= gamma(n - 1) * mag)
    lsum = float(np.sum([float(l) for l in losses]))
    assert abs(float(mean) - lsum / n) <= gamma(n + 1) * lsum / n
    if n == 1:
        assert total.tobytes() == gs[0].tobytes() and total is not gs[0] and mean == losses[0]
    assert grad_accum_rule(gs)[1] is None and grad_accum_rule(gs)[0].tobytes() == total.tobytes()
    # left to right, not pairwise and not in float64: the restatement gives the same bits
    want = gs[0]
    for g in gs[1:]:
        want = (want + g).astype(np.float32)
    assert total.tobytes() == want.tobytes()


def test_rule_range_and_arguments():
    a = np.array([1e38, np.inf, np.nan, 1.0, 3e38], np.float32)
    b = np.array([3e38, -np.inf, 1.0, np.inf, -3e38], np.float32)
    total, _ = grad_accum_rule([a, b])
    assert total[0] == np.inf and np.isnan(total[1]) and np.isnan(total[2]) and total[3] == np.inf and total[4] == 0.0
    with pytest.raises(ValueError):
        grad_accum_rule([])
    with pytest.raises(ValueError):
        grad_accum_rule([a, b], [1.0])


def test_grad_accum_from_conf():
    assert grad_accum_from_conf({}) is None
    for off in (None, 0, 1, np.int64(1)):
        assert grad_accum_from_conf({'grad_accum_steps': off}) is None
    for n in (2, 3, 64, np.int32(4)):
        got = grad_accum_from_conf({'grad_accum_steps': n})
        assert got == int(n) and type(got) is int
    for bad in (True, False, -1, -2, 2.0, 1.5, 0.0, '2', float('nan'), [2]):
        with pytest.raises(ValueError):
            grad_accum_from_conf({'grad_accum_steps': bad})
    from dynamic_multiview_3d_amd import mv3d
    with pytest.raises(ValueError):                 # every model class reads the key, before it builds anything
        mv3d.mv3d_nobg_nodm({'batch_size': 2, 'grad_accum_steps': -1}, device='cpu')
    with pytest.raises(ValueError):
        _lowdim({'grad_accum_steps': 2.5})
    with pytest.raises(ValueError):
        _appflow({'batch_size': 2, 'grad_accum_steps': True})


def test_graph_methods_and_the_switch():
    off, one, on = _lowdim({}).graph, _lowdim({'grad_accum_steps': 1}).graph, _lowdim({'grad_accum_steps': 3}).graph
    for g in (off, one):
        assert g.accum_steps == 0 and g.grad_sum is None and g._accum_loss is None and g.micro_step == 0
        for call in (g.accum_loss, g.accumulate_gradients):
            with pytest.raises(RuntimeError):
                call()
        assert float(g.opt_state[6]) == 1.0 and float(g.opt_state[14]) == 1.0
    assert on.accum_steps == 3 and on.micro_step == 0 and on.plan_bwd_fused is None
    assert on.grad_sum.shape == on.grads.shape and on.grad_sum.dtype == torch.float32 and on.grad_sum.data_ptr() != on.grads.data_ptr()
    assert on._accum_loss.numel() == 2 and float(on.accum_loss()) == 0.0
    third = np.float32(1.0 / 3.0)
    assert on.opt_state[[6, 14]].numpy().tobytes() == np.array([third, third]).tobytes()       # the mean's 1 / N, without clipping
    assert on.accum is None                         # the momentum slot keeps its name and its meaning
    with pytest.raises(RuntimeError):
        on.enable_grad_accum(2)                     # after compile()
    on.enable_grad_accum(1)                         # off values are accepted any time: nothing changes
    assert on.accum_steps == 3
    for bad in (True, False, -1, 2.0, 1.5, '3', float('nan')):
        with pytest.raises(ValueError):
            Graph(device='cpu').enable_grad_accum(bad)
    fresh = Graph(device='cpu')
    for none in (None, 0, 1):
        fresh.enable_grad_accum(none)
        assert fresh.accum_steps == 0
    fresh.enable_grad_accum(4)
    assert fresh.accum_steps == 4 and fresh.grad_sum is None            # allocated when the graph is finalised
    # a model without a loss has no train step: the key is validated and otherwise left alone
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    noloss = AppFlowLowDimAngle({'batch_size': 2, 'grad_accum_steps': 3}, load_tfrec=False, build_loss=False, device='cpu').graph
    assert noloss.accum_steps == 0 and noloss.grad_sum is None
    # the mv3d networks take the key like the others
    from dynamic_multiview_3d_amd import mv3d
    g = mv3d.mv3d_nobg_nodm({'batch_size': 2, 'grad_accum_steps': 2}, device='cpu').graph
    assert g.accum_steps == 2 and g.grad_sum.numel() == g.flat_size and float(g.opt_state[6]) == 0.5


def test_state_dict_refuses_the_middle_of_a_cycle_and_load_resets_it():
    g = _lowdim({'grad_accum_steps': 3}).graph
    sd = g.state_dict()
    g.micro_step = 1
    with pytest.raises(RuntimeError, match='accumulation cycle'):
        g.state_dict()
    g.load_state_dict(sd)
    assert g.micro_step == 0
    g.state_dict()


# ---------------------------------------------------------------- C ABI: validation before any launch
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def test_grad_accumulate_validation(lib):
    n = 3 * GN_CHUNK + 5
    S, G, L, LS, WS = 1 << 20, 1 << 22, 1 << 12, (1 << 12) + 4, 1 << 16     # aligned stand-ins: nothing is dereferenced on a rejected call
    need = lib.grad_clip_workspace_bytes(n)
    assert (_lib.ACCUM_STORE, _lib.ACCUM_ADD, _lib.ACCUM_FINISH) == (STORE, ADD, FINISH)

    def call(count=n, s=S, g=G, mode=FINISH, loss=L, lsum=LS, scale=0.5, part=WS, nbytes=need):
        return lib.raw_grad_accumulate(count, s, g, mode, loss, lsum, scale, part, nbytes, None)
    assert call(count=0) == E_INVAL and call(count=-4) == E_INVAL
    assert 'count' in lib.last_error()
    assert call(s=None) == E_INVAL and call(g=None) == E_INVAL
    for off in (4, 8, 12):
        assert call(s=S + off) == E_INVAL and call(g=G + off) == E_INVAL
    assert '16-byte' in lib.last_error()
    # overlapping buffers: the same, g inside sum, sum inside g, and the last element of one on the first of the other
    for s, g in ((S, S), (S, S + 16), (S + 16, S), (S, S + 4 * n - 16), (S + 4 * (n + 3) - 16, S)):
        assert call(s=s, g=g) == E_INVAL, (s, g)
    assert 'overlap' in lib.last_error()
    for mode in (-1, 3, 7):
        assert call(mode=mode) == E_INVAL
    assert 'mode' in lib.last_error()
    assert call(loss=None) == E_INVAL and call(lsum=None) == E_INVAL            # one without the other
    assert call(loss=L + 2) == E_INVAL and call(lsum=LS + 1) == E_INVAL
    for mode in (STORE, ADD):
        assert call(mode=mode) == E_INVAL                                       # partials outside FINISH
        assert 'FINISH' in lib.last_error()
    assert call(nbytes=need - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
    assert call(part=WS + 8) == E_WORKSPACE


def test_grad_clip_finish_validation(lib):
    OUT, ST, WS = 1 << 16, 1 << 17, 1 << 20
    n = 3 * GN_CHUNK
    need = lib.grad_clip_workspace_bytes(n)

    def call(count=n, pre=1.0, clip=1.0, out=OUT, sa=ST, sb=ST + 32, ws=WS, nbytes=need):
        return lib.raw_grad_clip_finish(count, pre, clip, out, sa, sb, ws, nbytes, None)
    assert call(count=0) == E_INVAL and call(count=-8) == E_INVAL
    assert call(out=None) == E_INVAL and call(ws=None) == E_INVAL
    assert call(out=OUT + 2) == E_INVAL and call(sa=ST + 1) == E_INVAL and call(sb=ST + 34) == E_INVAL
    for clip in (0.0, -0.0, -1.0, float('nan'), -np.inf):
        assert call(clip=clip) == E_INVAL, clip
    assert 'clip_norm' in lib.last_error() and 'mv3d_grad_clip_finish' in lib.last_error()
    for pre in (0.0, -0.5, float('nan'), np.inf, -np.inf):
        assert call(pre=pre) == E_INVAL, pre
    assert 'pre_scale' in lib.last_error()
    assert call(nbytes=need - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
    assert call(ws=WS + 8) == E_WORKSPACE


# ---------------------------------------------------------------- what the micro-steps of a cycle launch
def test_step_launch_list_with_and_without_the_switch():
    names = lambda calls: [c[0] for c in calls]
    absent = _appflow(dict(B64)).graph
    want_plans = [_labels(p) for p in (absent.plan_fwd, absent.plan_bwd, absent.plan_bwd_fused)]
    want = names(_calls(absent, absent.train_step))
    assert 'grad_accumulate' not in want
    assert [n for n in want if not n.startswith('plan_')] == ['adam_step_dev', 'adam_advance', 'adam_advance']
    del absent
    # key None, 0 or 1: nothing allocated, the same three plans, the same direct calls
    for value in (None, 0, 1):
        g = _appflow(dict(B64, grad_accum_steps=value)).graph
        assert g.accum_steps == 0 and g.grad_sum is None and g._accum_loss is None
        assert [_labels(p) for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)] == want_plans
        assert names(_calls(g, g.train_step)) == want
        assert float(g.opt_state[6]) == 1.0 and float(g.opt_state[14]) == 1.0
        del g
    # switch on: the recorded forward and plain reverse plans are the parent's; the fused plan is not recorded
    on = _appflow(dict(B64, grad_accum_steps=3)).graph
    assert [_labels(on.plan_fwd), _labels(on.plan_bwd)] == want_plans[:2] and on.plan_bwd_fused is None
    assert not any('grad_accum' in l for l in _labels(on.plan_fwd) + _labels(on.plan_bwd))
    third = float(np.float32(1.0 / 3.0))
    for cycle in range(2):
        slot = on._accum_loss.data_ptr() + 4 * (cycle % 2)                     # the two loss floats alternate between cycles
        for k, mode in enumerate((STORE, ADD, FINISH)):
            assert on.micro_step == k
            calls = _calls(on, on.train_step)
            micro = ['plan_run', 'plan_run_range_multi', 'grad_accumulate']
            assert names(calls) == (micro if k < 2 else micro + ['adam_step_dev', 'adam_advance', 'adam_advance'])
            assert calls[0][1][0] == on.plan_fwd
            plan, begin, end = calls[1][1][:3]
            assert plan == on.plan_bwd and (begin, end) == (0, on.n_launch_bwd) and calls[1][1][-1] == 0   # plan_bwd whole, joined
            count, s, gr, md, loss, lsum, scale, part, nbytes, _ = calls[2][1]
            assert (count, s, gr, md) == (on.flat_size, on.grad_sum.data_ptr(), on.grads.data_ptr(), mode)
            assert (loss, lsum, scale, part, nbytes) == (on.loss_buf.data_ptr(), slot, third, None, 0)
            if k == 2:
                count, p, gr, m, v, state, nskip = calls[3][1][:7]
                assert count == on.flat_size and nskip == 0 and state == on.opt_state.data_ptr()
                assert (p, gr, m, v) == (on.params.data_ptr(), on.grads.data_ptr(), on.adam_m.data_ptr(), on.adam_v.data_ptr())
        assert on.micro_step == 0 and on.accum_loss().data_ptr() == slot
    del on
    # with clipping: FINISH writes the norm's partials and pass 2 alone follows, with pre_scale = float32(1 / N)
    both = _appflow(dict(B64, grad_accum_steps=2, grad_clip_norm=1.5)).graph
    assert names(_calls(both, both.train_step)) == ['plan_run', 'plan_run_range_multi', 'grad_accumulate']
    calls = _calls(both, both.train_step)
    assert names(calls) == ['plan_run', 'plan_run_range_multi', 'grad_accumulate', 'grad_clip_finish', 'adam_step_dev', 'adam_advance',
                            'adam_advance']
    assert calls[2][1][3] == FINISH and calls[2][1][7:9] == (both._clip_ws.data_ptr(), both._clip_ws_bytes)
    count, pre, clip, out, sa, sb, ws, nbytes, _ = calls[3][1]
    assert (count, pre, clip, out) == (both.flat_size, 0.5, 1.5, both.clip_buf.data_ptr())
    assert (sa, sb) == (both.opt_state.data_ptr(), both.opt_state.data_ptr() + 32)
    assert (ws, nbytes) == (both._clip_ws.data_ptr(), both._clip_ws_bytes)


# ---------------------------------------------------------------- data parallel (gloo, world 2)
class _AccumCpuLib(_ClipCpuLib):
    """tests/test_grad_clip_host.py's stand-in with mv3d_grad_accumulate = the twin's additions on the flat buffers."""

    def __init__(self, g):
        super().__init__(g)
        self.modes = []

    def plan_run(self, plan, stream):
        pass

    def grad_accumulate(self, count, s, gr, mode, loss, lsum, scale, part, nbytes, stream):
        g = self.g
        assert (count, s, gr, loss) == (g.flat_size, g.grad_sum.data_ptr(), g.grads.data_ptr(), g.loss_buf.data_ptr())
        assert part is None and nbytes == 0         # data parallel: the all-reduce changes the buffer, no partials
        slot = g._accum_loss.numpy()[(lsum - g._accum_loss.data_ptr()) // 4:][:1]
        l = g.loss_buf.numpy()[0]
        if mode == STORE:
            g.grad_sum.copy_(g.grads)
            slot[0] = l
        elif mode == ADD:
            g.grad_sum.add_(g.grads)
            slot[0] = slot[0] + l
        else:
            g.grads.add_(g.grad_sum)
            slot[0] = np.float32(slot[0] + l) * np.float32(scale)
        self.modes.append(mode)


class _CountingComm:
    def __init__(self, comm):
        self.comm, self.rank, self.world, self.reduces = comm, comm.rank, comm.world, 0

    def allreduce_sum_(self, buf, lo, n, stream=None):
        assert (lo, n) == (0, buf.numel())
        self.reduces += 1
        self.comm.allreduce_sum_(buf, lo, n, stream)


N_ACC, CYCLES = 3, 2


def _dp_accum_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from dynamic_multiview_3d_amd import parallel
    parallel.init_from_env('gloo')
    flat = _lowdim({}).graph.flat_size
    gens = [torch.Generator().manual_seed(2000 + r) for r in range(world)]
    # [cycle][micro-step][rank]: that rank's gradient and loss
    grads = [[[torch.randn(flat, generator=gen) * 1e-2 for gen in gens] for _ in range(N_ACC)] for _ in range(CYCLES)]
    losses = [[[np.float32(0.1 * (1 + c) + 0.01 * k + 0.001 * r) for r in range(world)] for k in range(N_ACC)] for c in range(CYCLES)]
    pre = np.float32(1.0 / (world * N_ACC))
    summed = [sum(torch.from_numpy(grad_accum_rule([grads[c][k][r].numpy() for k in range(N_ACC)])[0]) for r in range(world))
              for c in range(CYCLES)]
    norm0 = float(grad_clip_rule(summed[0].numpy(), pre, np.inf)[0])
    out = {}
    for clip in (None, norm0 / 2):
        conf = {'grad_accum_steps': N_ACC}
        if clip is not None:
            conf['grad_clip_norm'] = clip
        for mode in ('allreduce', 'sharded', 'single'):
            m = _lowdim(conf)
            g = m.graph
            if mode != 'single':
                m.enable_data_parallel(world, mode=mode)
                g.comm = _CountingComm(g.comm)
            else:
                g.world_size = world                # one process on the summed gradients: scale 1 / (world * N), no exchange
                g.upload_optimizer_state()
            fake = _AccumCpuLib(g)
            g.lib = fake
            g._stream_ptr = lambda: None
            reduces, untouched, mean_ok = [], True, True
            for c in range(CYCLES):
                if mode == 'single':
                    g.grads.copy_(summed[c])
                    if clip is not None:
                        g.clip_gradients()
                    g.apply_optimizer()
                    continue
                for k in range(N_ACC):
                    before = (g.params.clone(), g.adam_m.clone(), g.adam_v.clone(), g.opt_state.clone())
                    g.grads.copy_(grads[c][k][rank])
                    g.loss_buf[0] = float(losses[c][k][rank])
                    got = g.train_step()
                    assert float(got) == float(losses[c][k][rank])             # the micro-batch's loss, as ever
                    reduces.append(g.comm.reduces)
                    if k < N_ACC - 1:
                        untouched = untouched and all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                      for a, b in zip(before, (g.params, g.adam_m, g.adam_v, g.opt_state)))
                        try:
                            g.state_dict()
                            untouched = False
                        except RuntimeError:
                            pass
                want_mean = grad_accum_rule([grads[c][0][rank].numpy()] * N_ACC, [losses[c][k][rank] for k in range(N_ACC)])[1]
                mean_ok = mean_ok and np.float32(float(g.accum_loss())).tobytes() == want_mean.tobytes()
            ok = fake.adam_calls == [(0, g.flat_size)] * CYCLES and not getattr(g, '_slots_sharded', False)
            if mode != 'single':
                ok = ok and reduces == [0, 0, 1, 1, 1, 2] and fake.modes == [STORE, ADD, FINISH] * CYCLES and untouched and mean_ok
            if clip is not None:
                ok = ok and fake.clip_calls == [(float(pre), float(np.float32(clip)))] * CYCLES
            else:
                ok = ok and g.opt_state[[6, 14]].numpy().tobytes() == np.array([pre, pre]).tobytes()
            b1 = np.float32(0.9)
            for _ in range(CYCLES):
                b1 = np.float32(b1 * np.float32(0.9))
            ok = ok and g.beta1_power == b1 and np.float32(float(g.opt_state[4])) == b1      # advanced once per update
            g.state_dict()                          # a boundary: complete slots on every rank, no gather needed
            out[(clip is not None, mode)] = (g.params.clone(), g.adam_m.clone(), g.adam_v.clone(), bool(ok),
                                             g.clip_buf.clone() if clip is not None else torch.ones(2))
    bits = lambda a, b: bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    res = []
    for clipped in (False, True):
        pa, ma, va, oka, na = out[(clipped, 'allreduce')]
        ps, ms, vs, oks, ns = out[(clipped, 'sharded')]
        p1, m1, v1, ok1, n1 = out[(clipped, 'single')]
        other = ps.clone()
        dist.broadcast(other, src=0)
        res.append((bits(pa, ps) and bits(ma, ms) and bits(va, vs) and bits(na, ns), bits(other, ps),
                    bits(pa, p1) and bits(ma, m1) and bits(va, v1) and bits(na, n1), oka and oks and ok1, float(na[1])))
    q.put((rank, res))
    dist.destroy_process_group()


def test_data_parallel_accumulation_two_ranks():
    """Two ranks, N = 3, two cycles, with and without clipping, in both dp_modes: only the last micro-step of a cycle has an
    all-reduce (one, over the whole buffer); parameters, slots and records keep their bits through micro-steps 1 and 2 and
    state_dict() refuses there; both ranks end with bit-identical weights, equal in both modes and equal to one process stepping
    on the sum of the ranks' accumulated gradients with the scale float32(1 / 6); the clip (half the first cycle's norm) is active."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_accum_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, per_clip in res:
        for clipped, (modes_equal, ranks_equal, single_equal, ok, scale) in zip((False, True), per_clip):
            assert modes_equal, "sharded and all-reduce modes diverged on rank %d (clip %s)" % (rank, clipped)
            assert ranks_equal, "ranks hold different weights (clip %s)" % clipped
            assert single_equal, "accumulated data-parallel update differs from the single-process one on rank %d (clip %s)" % (rank, clipped)
            assert ok, "launches, all-reduces, records or the loss mean are not what the schedule states on rank %d (clip %s)" % (rank, clipped)
            assert (scale < 1.0) == clipped


# ---------------------------------------------------------------- the train driver
class _Batches:
    def __init__(self):
        self.drawn = 0

    def next(self):
        self.drawn += 1
        return {}


class _NullLib:
    def __getattr__(self, name):
        return lambda *a: 0


@pytest.mark.parametrize("n", [None, 2])
def test_train_loop_draws_n_batches_per_iteration(tmp_path, n, capsys):
    """num_iterations = 10 is 11 iterations (0 .. 10 inclusive): 11 batches without the key, 22 with N = 2; rows for iterations
    0 and 10 either way; with the key every iteration ends at an update boundary and the logged loss is accum_loss()."""
    from dynamic_multiview_3d_amd import train
    model = _lowdim({} if n is None else {'grad_accum_steps': n})
    g = model.graph
    g.lib = _NullLib()
    g._stream_ptr = lambda: None
    steps = []
    real = model.train_step
    model.train_step = lambda **kw: (steps.append(g.micro_step), real(**kw))[1]
    if n is not None:
        g._accum_loss.copy_(torch.tensor([0.75, 0.25]))     # what the kernel would leave: the slots alternate between cycles
    g.loss_buf[0] = 0.5
    data, val = _Batches(), _Batches()
    with open(tmp_path / 'train_log.jsonl', 'w') as log:
        train.train_loop(model, {'num_iterations': 10, 'output_dir': str(tmp_path)}, data, val, model.saver, log=log)
    rows = [json.loads(l) for l in open(tmp_path / 'train_log.jsonl')]
    assert [r['itr'] for r in rows] == [0, 10] and all(set(r) == {'itr', 'training_loss'} for r in rows)
    assert val.drawn == 0
    if n is None:
        assert data.drawn == 11 and steps == [0] * 11 and [r['training_loss'] for r in rows] == [0.5, 0.5]
    else:
        assert data.drawn == 22 and steps == [0, 1] * 11 and g.micro_step == 0
        assert [r['training_loss'] for r in rows] == [0.75, 0.75]           # cycles 0 and 10 both ran on slot 0
    assert 'time per iteration' in capsys.readouterr().out


def test_train_docstring_names_the_key():
    from dynamic_multiview_3d_amd import train
    assert "conf['grad_accum_steps']" in train.__doc__
