"""Global-norm gradient clipping on the MI355X: mv3d_grad_clip_scale bit-exact against the numpy twin grad_clip_rule, its range,
a slice of a larger buffer, and the model: the clipped schedule against the plain unfused step, one step by hand against the
oracle's Adam on the scaled gradients, the length of a gradient-descent step, EMA on top of it, the data-parallel schedule through
RCCL at world size 1, and the train driver's log."""
import glob
import json
import math

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import GN_CHUNK
from dynamic_multiview_3d_amd.model_base import ema_one_minus_decay, ema_rule, grad_clip_rule
from tests.gpu_utils import Ws, dev, stream

pytestmark = pytest.mark.gpu

INF = math.inf
# 257 chunks: the final kernel's strided loop wraps (thread 0 adds partials 0 and 256)
COUNTS = [1, 3, 4, 5, 1023, GN_CHUNK - 1, GN_CHUNK, GN_CHUNK + 1, 3 * GN_CHUNK + 7, 257 * GN_CHUNK + 5]


def L():
    return _lib.lib()


def _values(rng, n):
    """Normals of magnitudes 1e-20 .. 1e10 with denormals, +0 and -0 among them; element 0 is a normal number, so that the norm
    of even one element is a valid clip."""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 10, n)).astype(np.float32)
    k = max(n // 16, 1)
    for value in (np.float32(1e-40), np.float32(-3e-45), np.float32(0.0), np.float32(-0.0)):
        x[rng.integers(0, n, k)] = value
    x[0] = np.float32(1.5e-3)
    return x


def _bits(t):
    torch.cuda.synchronize()
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _f32_bits(*values):
    return np.array(values, np.float32).view(np.int32)


def _run(count, gptr, pre, clip, ws, state=None):
    """One call; (out bits, state bits) read back."""
    out = torch.full((2,), -7.0, device='cuda')
    sa = state.data_ptr() if state is not None else None
    sb = state.data_ptr() + 32 if state is not None else None
    L().grad_clip_scale(count, gptr, float(pre), float(clip), out.data_ptr(), sa, sb, ws.ptr, ws.bytes, stream())
    return _bits(out), (_bits(state) if state is not None else None)


@pytest.mark.parametrize("count", COUNTS)
def test_grad_clip_scale_bit_exact_vs_numpy(count):
    """out[0], out[1] and slot 6 of both records equal the twin's bits for clip = inf, 2 n and n / 2 (n: the twin's norm); every
    other float of the records, g and the floats behind it are untouched; a second call gives the same bits."""
    rng = np.random.default_rng(count)
    x = _values(rng, count)
    guard = rng.standard_normal(64).astype(np.float32)
    buf = dev(np.concatenate([x, guard]))
    before = _bits(buf).copy()
    ws = Ws(int(L().grad_clip_workspace_bytes(count)))
    rec = rng.standard_normal(16).astype(np.float32)
    for pre in (np.float32(1.0), np.float32(0.5), np.float32(1.0 / 3.0)):
        n = grad_clip_rule(x, pre, INF)[0]
        assert np.isfinite(n) and n > 0
        for clip in (INF, 2.0 * float(n), float(n) / 2.0):
            want_n, want_s, want_gs = grad_clip_rule(x, pre, clip)
            assert (want_s < 1.0) == (clip < float(n)) and want_n == n
            state = dev(rec)
            got, st = _run(count, buf.data_ptr(), pre, clip, ws, state)
            want_rec = rec.copy()
            want_rec[[6, 14]] = want_gs
            print(count, float(pre), clip, got.view(np.float32), (want_n, want_s), st.view(np.float32)[[6, 14]], want_gs)
            assert got.tobytes() == _f32_bits(want_n, want_s).tobytes(), (count, float(pre), clip)
            assert st.tobytes() == want_rec.view(np.int32).tobytes(), (count, float(pre), clip)
            again, st2 = _run(count, buf.data_ptr(), pre, clip, ws, dev(rec))
            assert again.tobytes() == got.tobytes() and st2.tobytes() == st.tobytes()
            assert _bits(buf).tobytes() == before.tobytes()
    # without records: the same two floats
    got, _ = _run(count, buf.data_ptr(), 1.0, INF, ws)
    assert got.tobytes() == _f32_bits(*grad_clip_rule(x, 1.0, INF)[:2]).tobytes()


def test_grad_clip_scale_grid_stride_walk():
    """More chunks than the launch has workgroups (2048): the workgroups walk the chunks with a grid stride, and the result is
    still the twin's.  The values repeat a block of 2^20 (what is tested here is the walk, not the values)."""
    count = 2049 * GN_CHUNK + 1
    x = np.resize(_values(np.random.default_rng(7), 1 << 20), count)
    buf = dev(x)
    ws = Ws(int(L().grad_clip_workspace_bytes(count)))
    want = grad_clip_rule(x, 1.0, INF)
    got, _ = _run(count, buf.data_ptr(), 1.0, INF, ws)
    print(got.view(np.float32), want)
    assert got.tobytes() == _f32_bits(want[0], want[1]).tobytes()


def test_grad_clip_scale_on_a_slice_reads_only_its_range():
    rng = np.random.default_rng(12)
    total, off, count = 8 * GN_CHUNK, 4 * 1021, 2 * GN_CHUNK + 3           # 16-byte aligned, aligned to no chunk
    x = np.full(total, np.nan, np.float32)                                  # NaN sentinels on both sides
    x[off:off + count] = _values(rng, count)
    buf = dev(x)
    ws = Ws(int(L().grad_clip_workspace_bytes(count)))
    want_n, want_s, _ = grad_clip_rule(x[off:off + count], 1.0, INF)
    clip = float(want_n) / 2
    want = grad_clip_rule(x[off:off + count], 1.0, clip)
    got, _ = _run(count, buf.data_ptr() + 4 * off, 1.0, clip, ws)
    assert np.isfinite(got.view(np.float32)).all()
    assert got.tobytes() == _f32_bits(want[0], want[1]).tobytes()
    assert np.isnan(x[off - 1]) and np.isnan(x[off + count])


def test_grad_clip_scale_range():
    ws = Ws(int(L().grad_clip_workspace_bytes(4096)))
    big = dev(np.full(4096, 1e30, np.float32))
    got, _ = _run(4096, big.data_ptr(), 1.0, 1.0, ws)
    n, s = got.view(np.float32)
    assert np.isfinite(n) and abs(float(n) - 6.4e31) <= float(np.spacing(np.float32(6.4e31)))      # fp32 squares would overflow
    assert s == np.float32(1.0) / n
    assert got.tobytes() == _f32_bits(*grad_clip_rule(np.full(4096, 1e30, np.float32), 1.0, 1.0)[:2]).tobytes()
    x = np.ones(4096, np.float32)
    x[1234] = np.inf
    state = dev(np.arange(16, dtype=np.float32))
    dx = dev(x)
    got, st = _run(4096, dx.data_ptr(), 0.5, 1.0, ws, state)
    assert got.tobytes() == _f32_bits(np.inf, 0.0).tobytes() and st.view(np.float32)[6] == 0.0 and st.view(np.float32)[14] == 0.0
    x[1234] = np.nan
    dx = dev(x)
    got, st = _run(4096, dx.data_ptr(), 0.5, 1.0, ws, state)
    n, s = got.view(np.float32)
    assert np.isnan(n) and s == 1.0 and st.view(np.float32)[6] == 0.5 and st.view(np.float32)[14] == 0.5


# ---------------------------------------------------------------- the model
B = 2
PLAIN = {'MV3D_FUSE_FC_ADAM': '0', 'MV3D_FUSE_FINALIZE': '0', 'MV3D_OVERLAP_ADAM': '0'}      # the plain unfused schedule
SWITCHES = list(PLAIN)


def _model(monkeypatch, env, **conf):
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for k in SWITCHES:
        monkeypatch.setenv(k, env.get(k, '1'))
    return AppFlowLowDimAngle(dict({'batch_size': B, 'learning_rate': 1e-4}, **conf), load_tfrec=False, build_loss=True, device='cuda')


@pytest.fixture(scope="module")
def feeds():
    from tests.synth import appflow_feeds
    rng = np.random.default_rng(4)
    return [{k: torch.from_numpy(v).cuda() for k, v in appflow_feeds(rng, B).items()} for _ in range(2)]


def _flat_gradients(model, feed):
    """The flat gradient buffer of the model's first step on `feed` (forward and plain reverse pass, no update)."""
    g = model.graph
    model.feed(**feed)
    g.run_forward()
    g.run_backward()
    g.settle()
    torch.cuda.synchronize()
    return g.grads.cpu().numpy().copy()


@pytest.fixture(scope="module")
def first_norm(feeds):
    """The twin's norm of the first step's gradient on feeds[0] (the models of this file start from the same seed)."""
    mp = pytest.MonkeyPatch()
    try:
        model = _model(mp, PLAIN)
        flat = _flat_gradients(model, feeds[0])
    finally:
        mp.undo()
    n = float(grad_clip_rule(flat, 1.0, INF)[0])
    assert math.isfinite(n) and n > 0
    del model
    torch.cuda.empty_cache()
    return n


def _state(g):
    g.settle()
    torch.cuda.synchronize()
    return {k: _bits(t).copy() for k, t in (('params', g.params), ('m', g.adam_m), ('v', g.adam_v))}


def test_unclipped_steps_keep_the_bits_of_the_plain_schedule(monkeypatch, feeds):
    """(a) grad_clip_norm = 1e30 never clips: four unsynchronised train steps leave parameters and Adam slots bit-equal to a model
    without the key on the plain unfused schedule, and the scale is exactly 1."""
    twin = _model(monkeypatch, PLAIN)
    assert twin.graph.clip_norm is None and twin.graph.plan_bwd_fused is None
    for step in range(4):
        twin.train_step(**feeds[step % 2])
    want = _state(twin.graph)
    del twin
    model = _model(monkeypatch, {}, grad_clip_norm=1e30)
    g = model.graph
    assert g.clip_norm == 1e30 and g.plan_bwd_fused is None
    for step in range(4):
        model.train_step(**feeds[step % 2])
    got = _state(g)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    n, s = g.grad_norm().tolist()
    assert s == 1.0 and math.isfinite(n) and n > 0
    assert float(g.opt_state[6]) == 1.0 and float(g.opt_state[14]) == 1.0


def test_one_clipped_step_by_hand_equals_the_oracle_on_the_scaled_gradients(monkeypatch, feeds, first_norm):
    """(b) forward, reverse pass, read the flat gradients, clip_gradients(), apply_optimizer() with clip = half the twin's norm:
    grad_norm() has the twin's bits, and parameters and slots are oracle.ops.adam_step on g * gscale from the same start."""
    from oracle import ops
    clip = first_norm / 2
    model = _model(monkeypatch, {}, grad_clip_norm=clip)
    g = model.graph
    flat = _flat_gradients(model, feeds[0])
    p = g.params.cpu().numpy().copy()
    # what lets clip_gradients() sum the whole buffer: the padding between variables and variables without a gradient are zero
    outside = np.ones(flat.size, bool)
    for var in g.variables.values():
        if var.has_grad:
            outside[var.offset:var.offset + var.size] = False
    assert outside.any() and not flat[outside].any() and flat[~outside].any()
    want_n, want_s, want_gs = grad_clip_rule(flat, 1.0, clip)
    assert float(want_n) == first_norm and want_s < 1.0
    g.clip_gradients()
    g.apply_optimizer()
    assert _bits(g.grad_norm()).tobytes() == _f32_bits(want_n, want_s).tobytes()
    assert _bits(g.opt_state)[[6, 14]].tobytes() == _f32_bits(want_gs, want_gs).tobytes()
    assert _bits(g.grads).tobytes() == flat.view(np.int32).tobytes()                   # the gradients are not rewritten
    m, v = np.zeros_like(p), np.zeros_like(p)
    ops.adam_step(p, flat * want_gs, m, v, np.float32(0.9), np.float32(0.999), 1e-4)
    got = _state(g)
    gp = got['params'].view(np.float32)
    diff = np.flatnonzero(got['params'] != p.view(np.int32))
    print("params: %d of %d elements differ from the oracle, max |diff| %.3g" % (diff.size, p.size, float(np.abs(gp - p).max())))
    assert got['m'].tobytes() == m.view(np.int32).tobytes()
    assert got['v'].tobytes() == v.view(np.int32).tobytes()
    assert diff.size == 0, (diff.size, diff[:4])
    # an implementation that computes the norm but never lets it reach the optimiser would have made the unclipped step
    assert not np.array_equal(m, flat * (np.float32(1) - np.float32(0.9)))


@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_gradient_descent_step_has_the_clipped_length(monkeypatch, feeds, factor):
    """(c) gradient descent, p -= lr * gscale * g: ||delta p||_2 = lr * clip where the clip is active (clip = n / 2) and lr * n
    where it is not (clip = 2 n), to 1e-5 relative.  What the measured length adds to lr * clip is what fp32 storage of p rounds
    away: an error e of up to half an ulp of p per element, independent of the update, so ||dp + e|| = ||dp|| (1 + ||e||^2 /
    (2 ||dp||^2)).  The 69 M parameters are mostly fc weights of magnitude 0.02 (ulp 1.9e-9): ||e|| is about sqrt(69e6) * 1.9e-9
    / sqrt(12) = 4.5e-6.  The gradient of this model at initialisation is small (n = 2.4e-3), so the learning rate is chosen
    for the step, not for training: lr = 10 gives ||dp|| >= 1.2e-2 and a relative excess below 1e-7, while an element still
    moves by 1e-6, far below its own magnitude.  (At lr = 0.1 the same step measures 4.8e-4 long of lr * clip, all of it e.)
    The two fp32 products per element are good to 2^-23 relative."""
    lr = 10.0
    conf = {'optimizer': 'sgd', 'learning_rate': lr}
    n = float(grad_clip_rule(_flat_gradients(_model(monkeypatch, PLAIN, **conf), feeds[0]), 1.0, INF)[0])
    clip = factor * n
    model = _model(monkeypatch, {}, grad_clip_norm=clip, **conf)
    g = model.graph
    p0 = g.params.double().clone()
    model.train_step(**feeds[0])
    g.settle()
    torch.cuda.synchronize()
    step = float((g.params.double() - p0).norm())
    norm, scale = g.grad_norm().tolist()
    want = lr * min(clip, n)
    print("factor %g: n %.9g, grad_norm %.9g, scale %.9g, ||dp|| %.9g, want %.9g, rel %.3g" % (factor, n, norm, scale, step, want,
                                                                                             abs(step - want) / want))
    assert norm == n and (scale < 1.0) == (factor < 1.0)
    assert abs(step - want) <= 1e-5 * want


def test_ema_follows_the_clipped_parameters(monkeypatch, feeds, first_norm):
    """(d) EMA and clipping together: the EMA launch follows apply_optimizer as ever, the shadows equal ema_rule iterated over the
    clipped run's parameters."""
    model = _model(monkeypatch, {}, grad_clip_norm=first_norm / 2, ema_decay=0.5)
    g = model.graph
    g.settle()
    torch.cuda.synchronize()
    want = g.params.cpu().numpy().copy()
    assert _bits(g.ema).tobytes() == want.view(np.int32).tobytes()
    scales = []
    for step in range(3):
        model.train_step(**feeds[step % 2])
        g.settle()
        torch.cuda.synchronize()
        scales.append(float(g.grad_norm()[1]))
        want = ema_rule(want, g.params.cpu().numpy(), ema_one_minus_decay(0.5))
    assert scales[0] < 1.0 and g.ema_updates == 3
    assert _bits(g.ema).tobytes() == want.view(np.int32).tobytes()
    assert not np.array_equal(g.ema.cpu().numpy(), g.params.cpu().numpy())


@pytest.mark.parametrize("mode", ['sharded', 'allreduce'])
def test_data_parallel_clip_schedule_world_one_equals_single_gpu(monkeypatch, feeds, first_norm, mode):
    """The data-parallel clipped schedule (bucketed all-reduce on the communication stream, then norm and optimiser on the main
    stream) with a world-size-1 RCCL communicator equals the single-GPU one bit for bit over three steps, in either dp_mode."""
    from dynamic_multiview_3d_amd import parallel
    res = []
    for dp in (False, True):
        model = _model(monkeypatch, {}, grad_clip_norm=first_norm / 2)
        g = model.graph
        if dp:
            comm = parallel.RcclComm(0, 1)
            model.enable_data_parallel(1, comm=comm, mode=mode)
        for step in range(3):
            model.feed(**feeds[step % 2])
            if dp:
                g.run_forward()
                g.run_backward_clipped(data_parallel=True)
            else:
                g.train_step()
        state = _state(g)
        state['norm'] = _bits(g.grad_norm()).copy()
        assert not getattr(g, '_slots_sharded', False)
        res.append(state)
        if dp:
            comm.close()
        del model, g
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k
    assert res[0]['norm'].view(np.float32)[1] <= 1.0


# ---------------------------------------------------------------- the driver
def test_train_driver_logs_the_norm_and_the_scale(tmp_path):
    from dynamic_multiview_3d_amd import summary, train
    out = tmp_path / 'modeldata'
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 10, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle,\n"
        "  'grad_clip_norm': 1e-3}\n" % str(out))
    model = train.main(['--hyper', str(conf_py), '--synthetic', '--event_log'])
    assert model.graph.clip_norm == 1e-3
    rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
    assert [r['itr'] for r in rows] == [0, 10]
    for r in rows:
        assert set(r) == {'itr', 'training_loss', 'grad_norm', 'grad_clip_scale'}
        assert math.isfinite(r['grad_norm']) and r['grad_norm'] > 0 and 0 < r['grad_clip_scale'] <= 1
        if r['grad_norm'] > 1e-3:
            assert r['grad_clip_scale'] == float(np.float32(1e-3) / np.float32(r['grad_norm']))
    files = glob.glob(str(out / 'events.out.tfevents*'))
    assert len(files) == 1
    got = [(e['step'], e['scalars'][0]) for e in summary.read_events(files[0])[1:]]
    want = [(r['itr'], (key, float(np.float32(r[key])))) for r in rows for key in ('training_loss', 'grad_norm', 'grad_clip_scale')]
    assert got == want
