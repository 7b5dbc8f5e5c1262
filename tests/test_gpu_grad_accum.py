"""Gradient accumulation on the MI355X: mv3d_grad_accumulate bit-exact against the numpy twin grad_accum_rule in its three modes,
on a slice, with the fused sum of squares against grad_clip_rule and mv3d_grad_clip_scale; and the model: the off switch, one cycle
by hand against the oracle's Adam, two micro-batches against one larger batch, clipping, EMA, the data-parallel schedule through
RCCL at world size 1, checkpoints, and the train driver."""
import json
import math

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import GN_CHUNK
from dynamic_multiview_3d_amd.model_base import ema_one_minus_decay, ema_rule, grad_accum_rule, grad_clip_rule
from tests.gpu_utils import Ws, dev, stream

pytestmark = pytest.mark.gpu

INF = math.inf
STORE, ADD, FINISH = _lib.ACCUM_STORE, _lib.ACCUM_ADD, _lib.ACCUM_FINISH
GRID_CAP = 2048                     # GN_MAX_BLOCKS: more chunks than that and the workgroups walk them with a grid stride
# 257 chunks: more than 256 partials for pass 2 of the norm
COUNTS = [1, 3, 4, 5, 1023, GN_CHUNK - 1, GN_CHUNK, GN_CHUNK + 1, 3 * GN_CHUNK + 7, 257 * GN_CHUNK + 5]
GUARD = 64


def L():
    return _lib.lib()


def _values(rng, n, special=True):
    """Normals of magnitudes 1e-20 .. 1e10 with denormals, +0 and -0 among them and, with `special`, 1e30, -1e30 (their sum of
    two overflows no float32, their squares would), +-inf and NaN."""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 10, n)).astype(np.float32)
    k = max(n // 16, 1)
    fixed = [1e-40, -3e-45, 0.0, -0.0] + ([1e30, -1e30, np.inf, -np.inf, np.nan] if special else [])
    for value in fixed:
        x[rng.integers(0, n, k)] = np.float32(value)
    return x


def _bits(t):
    torch.cuda.synchronize()
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same(got_bits, want):
    """Bit equality of float32 data, NaNs comparing as NaN (not by payload)."""
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    got = got_bits.reshape(-1).view(np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and \
        bool(np.array_equal(got_bits.reshape(-1)[~nan], want.view(np.int32)[~nan]))


def _accumulate(count, s, g, mode, loss=None, lsum=None, scale=1.0, ws=None):
    L().grad_accumulate(count, s, g, mode, loss, lsum, float(scale), ws.ptr if ws else None, ws.bytes if ws else 0, stream())


def _cycle(count, gs, losses, rng):
    """STORE, ADD, FINISH over three gradients with guards behind both buffers; every property of the three modes is asserted."""
    guard = rng.standard_normal(GUARD).astype(np.float32)
    sum_buf = dev(np.concatenate([np.full(count, np.nan, np.float32), guard]))      # STORE needs no memset: garbage underneath
    lbuf = dev(np.array([0.0, -7.0], np.float32))                                   # [loss, loss_sum]
    lp, sp = lbuf.data_ptr(), lbuf.data_ptr() + 4
    third = np.float32(1.0 / 3.0)
    for k, mode in enumerate((STORE, ADD, FINISH)):
        g_buf = dev(np.concatenate([gs[k], guard]))
        g_before, s_before = _bits(g_buf).copy(), _bits(sum_buf).copy()
        lbuf[0] = float(losses[k])
        _accumulate(count, sum_buf.data_ptr(), g_buf.data_ptr(), mode, lp, sp, third)
        want, _ = grad_accum_rule(gs[:k + 1])
        g_after, s_after = _bits(g_buf), _bits(sum_buf)
        if mode == FINISH:
            assert _same(g_after[:count], want), (count, 'FINISH')
            assert s_after.tobytes() == s_before.tobytes(), "FINISH wrote into sum"
        else:
            assert _same(s_after[:count], want), (count, mode)
            assert g_after.tobytes() == g_before.tobytes(), "STORE / ADD wrote into g"
        assert g_after[count:].tobytes() == guard.view(np.int32).tobytes() and s_after[count:].tobytes() == guard.view(np.int32).tobytes()
        # the loss scalar: the twin's bits in every mode (the mean only behind FINISH)
        run = np.float32(losses[0])
        for l in losses[1:k + 1]:
            run = np.float32(run + np.float32(l))
        want_l = grad_accum_rule(gs, losses)[1] if mode == FINISH else run
        got_l = _bits(lbuf)
        assert got_l[1] == np.float32(want_l).view(np.int32) and got_l[0] == np.float32(losses[k]).view(np.int32), (count, mode)
        # again: the same bits (one writer per element, no atomics) -- ADD and FINISH from the same inputs
        if mode != STORE:
            sum_buf.view(torch.int32).copy_(torch.from_numpy(s_before).cuda())
            g_buf.view(torch.int32).copy_(torch.from_numpy(g_before).cuda())
            _accumulate(count, sum_buf.data_ptr(), g_buf.data_ptr(), mode)           # without the loss: both pointers NULL
            assert _bits(g_buf).tobytes() == g_after.tobytes() and _bits(sum_buf).tobytes() == s_after.tobytes()
            assert _bits(lbuf).tobytes() == got_l.tobytes()


@pytest.mark.parametrize("count", COUNTS)
def test_grad_accumulate_bit_exact_vs_numpy(count):
    rng = np.random.default_rng(count)
    gs = [_values(rng, count) for _ in range(3)]
    if count > 8:
        gs[1][5], gs[2][5] = np.float32(1e30), np.float32(1e30)         # a finite sum of three next to an overflowing one
        gs[0][6] = gs[1][6] = gs[2][6] = np.float32(3e38)
    losses = [np.float32(v) for v in (0.3712, 1.25e-3, 7.5)]
    _cycle(count, gs, losses, rng)


def test_grad_accumulate_grid_stride_walk():
    """More chunks than the launch has workgroups: the workgroups walk the chunks with a grid stride, in every mode.  The values
    repeat a block of 2^20 (what is tested here is the walk, not the values)."""
    count = (GRID_CAP + 1) * GN_CHUNK + 1
    rng = np.random.default_rng(7)
    gs = [np.resize(_values(rng, 1 << 20), count) for _ in range(3)]
    _cycle(count, gs, [np.float32(1.0), np.float32(2.0), np.float32(4.0)], rng)


def test_grad_accumulate_on_a_slice_writes_only_its_range():
    rng = np.random.default_rng(12)
    total, off, count = 8 * GN_CHUNK, 4 * 1021, 2 * GN_CHUNK + 3           # 16-byte aligned, aligned to no chunk
    g1, g2 = _values(rng, count), _values(rng, count)
    sentinel_s, sentinel_g = rng.standard_normal(total).astype(np.float32), rng.standard_normal(total).astype(np.float32)
    for mode in (STORE, ADD, FINISH):
        hs, hg = sentinel_s.copy(), sentinel_g.copy()
        hs[off:off + count], hg[off:off + count] = g1, g2
        s_buf, g_buf = dev(hs), dev(hg)
        ws = Ws(int(L().grad_clip_workspace_bytes(count))) if mode == FINISH else None
        _accumulate(count, s_buf.data_ptr() + 4 * off, g_buf.data_ptr() + 4 * off, mode, ws=ws)
        want_s, want_g = hs.copy(), hg.copy()
        if mode == STORE:
            want_s[off:off + count] = g2
        elif mode == ADD:
            want_s[off:off + count] = grad_accum_rule([g1, g2])[0]
        else:
            want_g[off:off + count] = grad_accum_rule([g1, g2])[0]
        assert _same(_bits(s_buf), want_s) and _same(_bits(g_buf), want_g), mode
        outside = np.ones(total, bool)
        outside[off:off + count] = False
        assert _bits(s_buf)[outside].tobytes() == sentinel_s.view(np.int32)[outside].tobytes()
        assert _bits(g_buf)[outside].tobytes() == sentinel_g.view(np.int32)[outside].tobytes()


def _f32_bits(*values):
    return np.array(values, np.float32).view(np.int32)


@pytest.mark.parametrize("count", COUNTS + [(GRID_CAP + 1) * GN_CHUNK + 1])
def test_finish_with_partials_gives_the_norm_of_what_it_stored(count):
    """FINISH with sumsq_part, then mv3d_grad_clip_finish: [norm, scale] and slot 6 of both records have the bits of
    grad_clip_rule(stored, pre, clip), and of mv3d_grad_clip_scale run on the stored buffer -- for a clip that is not active, one
    that is, and inf."""
    rng = np.random.default_rng(count + 1)
    big = count > 300 * GN_CHUNK
    draw = (lambda: np.resize(_values(rng, 1 << 20, special=False), count)) if big else (lambda: _values(rng, count, special=False))
    g1, g2 = draw(), draw()
    g1[0] = np.float32(1.5e-3)                      # the norm of even one element is a valid clip
    stored, _ = grad_accum_rule([g1, g2])
    ws = Ws(int(L().grad_clip_workspace_bytes(count)))
    s_buf, g_buf = dev(g1), dev(g2)
    _accumulate(count, s_buf.data_ptr(), g_buf.data_ptr(), FINISH, ws=ws)
    assert _same(_bits(g_buf), stored)
    pre = np.float32(0.5)
    n = grad_clip_rule(stored, pre, INF)[0]
    assert np.isfinite(n) and n > 0
    rec = rng.standard_normal(16).astype(np.float32)
    ws2 = Ws(ws.bytes)
    for clip in ((INF,) if big else (INF, 2.0 * float(n), float(n) / 2.0)):
        want_n, want_s, want_gs = grad_clip_rule(stored, pre, clip)
        out, state = torch.full((2,), -7.0, device='cuda'), dev(rec)
        L().grad_clip_finish(count, float(pre), float(clip), out.data_ptr(), state.data_ptr(), state.data_ptr() + 32, ws.ptr, ws.bytes, stream())
        want_rec = rec.copy()
        want_rec[[6, 14]] = want_gs
        print(count, clip, _bits(out).view(np.float32), (want_n, want_s), want_gs)
        assert _bits(out).tobytes() == _f32_bits(want_n, want_s).tobytes(), (count, clip)
        assert _bits(state).tobytes() == want_rec.view(np.int32).tobytes(), (count, clip)
        out2, state2 = torch.full((2,), -7.0, device='cuda'), dev(rec)
        L().grad_clip_scale(count, g_buf.data_ptr(), float(pre), float(clip), out2.data_ptr(), state2.data_ptr(), state2.data_ptr() + 32,
                            ws2.ptr, ws2.bytes, stream())
        assert _bits(out2).tobytes() == _bits(out).tobytes() and _bits(state2).tobytes() == _bits(state).tobytes()
    nchunk = -(-count // GN_CHUNK)
    torch.cuda.synchronize()
    assert ws.t.view(torch.int32)[:2 * nchunk].cpu().numpy().tobytes() == ws2.t.view(torch.int32)[:2 * nchunk].cpu().numpy().tobytes()


# ---------------------------------------------------------------- the model
B = 2
PLAIN = {'MV3D_FUSE_FC_ADAM': '0', 'MV3D_FUSE_FINALIZE': '0', 'MV3D_OVERLAP_ADAM': '0'}      # the plain unfused schedule
SWITCHES = list(PLAIN)


def _model(monkeypatch, env, batch=B, **conf):
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for k in SWITCHES:
        monkeypatch.setenv(k, env.get(k, '1'))
    return AppFlowLowDimAngle(dict({'batch_size': batch, 'learning_rate': 1e-4}, **conf), load_tfrec=False, build_loss=True, device='cuda')


@pytest.fixture(scope="module")
def feeds():
    from tests.synth import appflow_feeds
    rng = np.random.default_rng(4)
    return [{k: torch.from_numpy(v).cuda() for k, v in appflow_feeds(rng, B).items()} for _ in range(3)]


def _flat_gradients(model, feed):
    """(flat gradient buffer, loss) of forward and plain reverse pass on `feed`: no update, no accumulation."""
    g = model.graph
    model.feed(**feed)
    g.run_forward()
    g.run_backward()
    g.settle()
    torch.cuda.synchronize()
    return g.grads.cpu().numpy().copy(), np.float32(float(g.loss_buf[0]))


@pytest.fixture(scope="module")
def first(feeds):
    """([gradient of feeds[k]], [loss of feeds[k]]) at the initial weights (the models of this file start from the same seed):
    computed once by a model without the key and left unchanged."""
    mp = pytest.MonkeyPatch()
    try:
        model = _model(mp, PLAIN)
        pairs = [_flat_gradients(model, f) for f in feeds]
    finally:
        mp.undo()
    del model
    torch.cuda.empty_cache()
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _state(g):
    g.settle()
    torch.cuda.synchronize()
    return {k: _bits(t).copy() for k, t in (('params', g.params), ('m', g.adam_m), ('v', g.adam_v))}


def test_steps_of_one_keep_the_default_schedule_and_its_bits(monkeypatch, feeds):
    """(a) grad_accum_steps = 1 is off: the fused plan is recorded, nothing is allocated, and four steps leave parameters and Adam
    slots bit-equal to a model without the key."""
    twin = _model(monkeypatch, {})
    assert twin.graph.plan_bwd_fused is not None
    for step in range(4):
        twin.train_step(**feeds[step % 3])
    want = _state(twin.graph)
    del twin
    model = _model(monkeypatch, {}, grad_accum_steps=1)
    g = model.graph
    assert g.accum_steps == 0 and g.grad_sum is None and g.plan_bwd_fused is not None
    for step in range(4):
        model.train_step(**feeds[step % 3])
    got = _state(g)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert float(g.opt_state[6]) == 1.0 and float(g.opt_state[14]) == 1.0


def test_one_cycle_by_hand_equals_the_oracle_on_the_mean_gradient(monkeypatch, feeds, first):
    """(b) N = 3 on three feeds, the flat gradients read after each reverse pass.  Micro-steps 1 and 2 leave parameters, slots and
    records bit-unchanged; after micro-step 3 grads holds the twin's sum, slots 6 and 14 are float32(1 / 3), the beta powers
    advanced once, accum_loss() has the twin's bits, and parameters, m and v are oracle.ops.adam_step on sum * float32(1 / 3),
    element for element."""
    from oracle import ops
    model = _model(monkeypatch, {}, grad_accum_steps=3)
    g = model.graph
    assert g.accum_steps == 3 and g.plan_bwd_fused is None
    start = _state(g)
    rec0 = _bits(g.opt_state).copy()
    p = g.params.cpu().numpy().copy()
    grads, losses = [], []
    for k in range(3):
        assert g.micro_step == k
        flat, loss = _flat_gradients(model, feeds[k])            # the pass train_step repeats: it is deterministic
        assert flat.tobytes() == first[0][k].tobytes() and loss == first[1][k]
        got_loss = model.train_step(**feeds[k])
        assert np.float32(float(got_loss)) == loss              # the micro-batch's loss, as ever
        grads.append(flat)
        losses.append(loss)
        if k < 2:
            now = _state(g)
            for key in start:
                assert now[key].tobytes() == start[key].tobytes(), (k, key)
            assert _bits(g.opt_state).tobytes() == rec0.tobytes() and g.beta1_power == np.float32(0.9)
            assert _bits(g.grads).tobytes() == flat.view(np.int32).tobytes()     # STORE and ADD leave g as it is
    assert g.micro_step == 0
    want_sum, want_loss = grad_accum_rule(grads, losses)
    assert _same(_bits(g.grads), want_sum) and not np.isnan(want_sum).any()
    for name, got in g.get_gradients().items():                 # the unscaled sum, per variable
        v = g.variables[name]
        assert got.tobytes() == want_sum[v.offset:v.offset + v.size].tobytes(), name
    third = np.float32(1.0 / 3.0)
    rec = _bits(g.opt_state)
    assert rec[[6, 14]].tobytes() == _f32_bits(third, third).tobytes()
    b1, b2 = np.float32(np.float32(0.9) * np.float32(0.9)), np.float32(np.float32(0.999) * np.float32(0.999))
    assert rec[[4, 5, 12, 13]].tobytes() == _f32_bits(b1, b2, b1, b2).tobytes() and g.beta1_power == b1 and g.beta2_power == b2
    assert _bits(g.accum_loss()).tobytes() == _f32_bits(want_loss).tobytes()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ops.adam_step(p, want_sum * third, m, v, np.float32(0.9), np.float32(0.999), 1e-4)
    got = _state(g)
    diff = np.flatnonzero(got['params'] != p.view(np.int32))
    print("params: %d of %d elements differ from the oracle" % (diff.size, p.size))
    assert got['m'].tobytes() == m.view(np.int32).tobytes()
    assert got['v'].tobytes() == v.view(np.int32).tobytes()
    assert diff.size == 0, (diff.size, diff[:4])
    assert not np.array_equal(m, grads[2] * (np.float32(1) - np.float32(0.9)))      # not the last micro-batch's step alone


def test_two_micro_batches_against_one_batch_of_four(monkeypatch):
    """(c) Two micro-batches of 2 against ONE step of the path without the key at batch 4: the same variables, the same four
    images.  Per variable, ||0.5 * sum - g4||_2 / ||g4||_2 <= 1e-3, the project's whole-model gradient bar.  At initialisation the
    sampling coordinates sit on the `floor` kinks of the sampler, so both models get generic variables first, as
    tools/precision_ladder.py sets them: biases perturbed by N(0, 0.05) and the flow head scaled to flows of 1.5 pixels.
    Measured on one MI355X: worst ratio 1.27e-7 (variable e1/b), a factor of 7900 inside the bar."""
    from tests.synth import appflow_feeds
    host = appflow_feeds(np.random.default_rng(9), 4)
    whole = _model(monkeypatch, PLAIN, batch=4)
    halves = _model(monkeypatch, {}, grad_accum_steps=2)
    variables = whole.graph.get_variables()
    rng = np.random.default_rng(5)
    for k, v in variables.items():
        if k.endswith('/b'):
            variables[k] = v + rng.normal(0, 0.05, v.shape).astype(np.float32)
    whole.graph.set_variables(variables)
    whole.forward(**{k: torch.from_numpy(v).cuda() for k, v in host.items()})
    std = float(whole.flow_field.numpy().std())
    variables['flow_field/w'] = (variables['flow_field/w'] * (1.5 / max(std, 1e-12))).astype(np.float32)
    whole.graph.set_variables(variables)
    halves.graph.set_variables(variables)
    g4, loss4 = _flat_gradients(whole, {k: torch.from_numpy(v).cuda() for k, v in host.items()})
    assert abs(float(whole.flow_field.numpy().std()) - 1.5) < 0.5
    micro = []
    for half in range(2):
        loss = halves.train_step(**{k: torch.from_numpy(v[2 * half:2 * half + 2]).cuda() for k, v in host.items()})
        micro.append(np.float32(float(loss)))
    hg = halves.graph
    hg.settle()
    torch.cuda.synchronize()
    assert hg.micro_step == 0 and float(hg.opt_state[6]) == 0.5
    acc = hg.grads.cpu().numpy().astype(np.float64) * 0.5
    worst, name = 0.0, None
    for k, v in hg.variables.items():
        if not v.has_grad:
            continue
        a, b = acc[v.offset:v.offset + v.size], g4[v.offset:v.offset + v.size].astype(np.float64)
        ratio = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print("%-24s %.3e" % (k, ratio))
        if ratio > worst:
            worst, name = ratio, k
    mean_loss = float(hg.accum_loss())
    print("worst relative L2 %.3e (%s); loss batch 4 %.9g, mean of the halves %.9g" % (worst, name, float(loss4), mean_loss))
    assert worst <= 1e-3, (worst, name)
    assert abs(mean_loss - float(loss4)) <= 1e-5 * abs(float(loss4))       # a mean over the batch: the two means average to it


def test_clipping_sees_the_mean_accumulated_gradient(monkeypatch, feeds, first):
    """(d) N = 2, clip at half the twin's norm of the summed gradient: grad_norm() has the bits of grad_clip_rule(sum, float32(1 /
    2), clip), slot 6 its gscale, and the update is the oracle's on sum * gscale."""
    from oracle import ops
    want_sum, _ = grad_accum_rule(first[0][:2])
    half = np.float32(0.5)
    clip = float(grad_clip_rule(want_sum, half, INF)[0]) / 2
    model = _model(monkeypatch, {}, grad_accum_steps=2, grad_clip_norm=clip)
    g = model.graph
    p = g.params.cpu().numpy().copy()
    for k in range(2):
        model.train_step(**feeds[k])
    want_n, want_s, want_gs = grad_clip_rule(want_sum, half, clip)
    assert want_s < 1.0
    assert _same(_bits(g.grads), want_sum)
    assert _bits(g.grad_norm()).tobytes() == _f32_bits(want_n, want_s).tobytes()
    assert _bits(g.opt_state)[[6, 14]].tobytes() == _f32_bits(want_gs, want_gs).tobytes()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ops.adam_step(p, want_sum * want_gs, m, v, np.float32(0.9), np.float32(0.999), 1e-4)
    got = _state(g)
    assert got['m'].tobytes() == m.view(np.int32).tobytes() and got['v'].tobytes() == v.view(np.int32).tobytes()
    assert got['params'].tobytes() == p.view(np.int32).tobytes()


def test_ema_counts_updates_not_micro_steps(monkeypatch, feeds):
    """(e) N = 2 with EMA over two cycles: the shadows move once per update (not at micro-step 1) and equal ema_rule iterated once
    per update; ema_updates counts 2."""
    model = _model(monkeypatch, {}, grad_accum_steps=2, ema_decay=0.5)
    g = model.graph
    g.settle()
    torch.cuda.synchronize()
    want = g.params.cpu().numpy().copy()
    for cycle in range(2):
        model.train_step(**feeds[(2 * cycle) % 3])
        assert g.ema_updates == cycle and _bits(g.ema).tobytes() == want.view(np.int32).tobytes()
        model.train_step(**feeds[(2 * cycle + 1) % 3])
        g.settle()
        torch.cuda.synchronize()
        want = ema_rule(want, g.params.cpu().numpy(), ema_one_minus_decay(0.5))
        assert g.ema_updates == cycle + 1
    assert _bits(g.ema).tobytes() == want.view(np.int32).tobytes()
    assert not np.array_equal(g.ema.cpu().numpy(), g.params.cpu().numpy())


@pytest.mark.parametrize("clipped", [False, True])
def test_data_parallel_schedule_world_one_equals_single_gpu(monkeypatch, feeds, first, clipped):
    """(f) The data-parallel cycle (FINISH, one all-reduce over the whole buffer, with clipping the ordinary norm behind it, the
    optimiser) with a world-size-1 RCCL communicator equals the single-GPU one bit for bit over two cycles."""
    from dynamic_multiview_3d_amd import parallel
    conf = {'grad_accum_steps': 2}
    if clipped:
        conf['grad_clip_norm'] = float(grad_clip_rule(grad_accum_rule(first[0][:2])[0], np.float32(0.5), INF)[0]) / 2
    res = []
    for dp in (False, True):
        model = _model(monkeypatch, {}, **conf)
        g = model.graph
        if dp:
            comm = parallel.RcclComm(0, 1)
            model.enable_data_parallel(1, comm=comm)
        for step in range(4):
            model.feed(**feeds[step % 3])
            if dp:
                g.run_forward()
                g.run_micro_step(data_parallel=True)
            else:
                g.train_step()
        state = _state(g)
        state['grads'] = _bits(g.grads).copy()
        state['loss'] = _bits(g.accum_loss()).copy()
        if clipped:
            state['norm'] = _bits(g.grad_norm()).copy()
        assert g.micro_step == 0 and not getattr(g, '_slots_sharded', False)
        res.append(state)
        if dp:
            comm.close()
        del model, g
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k
    if clipped:
        assert res[0]['norm'].view(np.float32)[1] <= 1.0


def test_state_dict_raises_inside_a_cycle_and_works_at_the_boundary(monkeypatch, feeds):
    """(g) and forward() in the middle of a cycle touches no gradient: the cycle ends on the sum it would have had without it."""
    model = _model(monkeypatch, {}, grad_accum_steps=2)
    g = model.graph
    sd0 = g.state_dict()
    model.train_step(**feeds[0])
    with pytest.raises(RuntimeError, match='accumulation cycle'):
        g.state_dict()
    kept = _bits(g.grad_sum).copy()
    model.forward(**feeds[2])
    assert _bits(g.grad_sum).tobytes() == kept.tobytes()
    model.train_step(**feeds[1])
    sd = g.state_dict()
    assert float(sd['beta1_power']) == float(np.float32(np.float32(0.9) * np.float32(0.9)))
    model.train_step(**feeds[0])
    g.load_state_dict(sd0)                          # resets the cycle
    assert g.micro_step == 0 and float(g.opt_state[6]) == 0.5
    g.state_dict()


# ---------------------------------------------------------------- the driver
def test_train_driver_updates_once_per_iteration(tmp_path):
    """(h) --synthetic, N = 2, num_iterations = 10: rows for iterations 0 and 10 with finite losses, and 11 updates -- the beta1
    power, 0.9 before the first update, has been multiplied by 0.9 eleven times in float32 (22 micro-steps would make it 22)."""
    from dynamic_multiview_3d_amd import train
    out = tmp_path / 'modeldata'
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 10, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle,\n"
        "  'grad_accum_steps': 2}\n" % str(out))
    model = train.main(['--hyper', str(conf_py), '--synthetic'])
    g = model.graph
    assert g.accum_steps == 2 and g.micro_step == 0
    rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
    assert [r['itr'] for r in rows] == [0, 10]
    for r in rows:
        assert set(r) == {'itr', 'training_loss'} and math.isfinite(r['training_loss']) and r['training_loss'] > 0
    b1 = np.float32(0.9)
    for _ in range(11):
        b1 = np.float32(b1 * np.float32(0.9))
    assert g.beta1_power == b1 and _bits(g.opt_state)[4] == b1.view(np.int32)
    assert rows[1]['training_loss'] == float(g.accum_loss())
