"""EMA weights on the MI355X: mv3d_ema_step bit-exact against the numpy rule, mv3d_swap_f32 bit-exact on arbitrary patterns, the
model's shadows after unsynchronised steps in every single-GPU schedule against the rule iterated over a twin's parameters,
ema_weights() against a model that carries the shadows as variables, and train.py's checkpoints / --evaluate / --raw_weights."""
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.graph import EMA_COUNTER, EMA_SLOT
from dynamic_multiview_3d_amd.model_base import ema_one_minus_decay, ema_rule
from tests.gpu_utils import dev, stream

pytestmark = pytest.mark.gpu

# (1 << 24) + 6: two sweeps of the launch's 2048 workgroups x 4 x 256 lanes x 16 B (2^23 floats per sweep, the same as the
# 8192 x 256-lane x 16 B grid of the element-wise kernels), a partial chunk and a scalar tail
COUNTS = [1, 3, 4, 5, 4099, (1 << 24) + 6]
GUARD = 64


def L():
    return _lib.lib()


def _values(rng, n):
    """Finite floats of magnitudes 1e-4 .. 1e3, with +0 and -0 among them."""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 3, n)).astype(np.float32)
    z = rng.integers(0, max(n, 2), max(n // 16, 1))
    x[z[z < n]] = 0.0
    x[z[(z < n) & (z % 2 == 1)]] = -0.0
    return x


def _bits(t):
    torch.cuda.synchronize()
    return t.detach().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("count", COUNTS)
def test_ema_step_bit_exact_vs_numpy(count):
    """Three consecutive updates with a fresh p each, for w = 1, 0.5 and float32(1 - 0.999): the shadows equal ema_rule bit for
    bit, p and the 64 floats behind the shadows are bitwise untouched."""
    rng = np.random.default_rng(count)
    s0 = _values(rng, count)
    ps = [_values(rng, count) for _ in range(3)]
    guard = rng.integers(0, 2 ** 31, GUARD).astype(np.int32)
    dps = [dev(p) for p in ps]
    for w in (np.float32(1.0), np.float32(0.5), ema_one_minus_decay(0.999)):
        buf = torch.empty(count + GUARD, dtype=torch.float32, device='cuda')
        buf[:count].copy_(torch.from_numpy(s0))
        buf[count:].view(torch.int32).copy_(torch.from_numpy(guard))
        s = s0.copy()
        for k in range(3):
            if k == 1:                                      # every 7th element: s == p exactly
                p = ps[1].copy()
                p[::7] = s[::7]
                dp = dev(p)
            else:
                p, dp = ps[k], dps[k]
            L().ema_step(count, buf.data_ptr(), dp.data_ptr(), float(w), stream())
            s_new = ema_rule(s, p, w)
            if k == 1:
                assert s_new[::7].tobytes() == s[::7].tobytes()
            s = s_new
            got = _bits(buf)
            assert got[:count].tobytes() == s.view(np.int32).tobytes(), (count, float(w), k)
            assert got[count:].tobytes() == guard.tobytes()
            assert _bits(dp).tobytes() == p.view(np.int32).tobytes()
        del buf


def test_ema_step_on_a_slice_touches_only_its_range():
    rng = np.random.default_rng(11)
    n, off, count = 8192, 1028, 4099
    s, p = _values(rng, n), _values(rng, n)
    ds, dp = dev(s), dev(p)
    w = np.float32(0.25)
    L().ema_step(count, ds.data_ptr() + 4 * off, dp.data_ptr() + 4 * off, float(w), stream())
    want = s.copy()
    want[off:off + count] = ema_rule(s[off:off + count], p[off:off + count], w)
    assert _bits(ds).tobytes() == want.view(np.int32).tobytes()
    assert _bits(dp).tobytes() == p.view(np.int32).tobytes()
    assert not np.array_equal(want, s)


@pytest.mark.parametrize("count", COUNTS)
def test_swap_f32_exchanges_bit_patterns(count):
    rng = np.random.default_rng(count + 1)
    a, b = (rng.integers(0, 2 ** 32, count + GUARD, dtype=np.uint64).astype(np.uint32).view(np.int32) for _ in range(2))
    a[:min(count, 3)] = np.array([0x7fc00001, 0xffa5a5a5 - (1 << 32), 0x7f800001], np.int64).astype(np.int32)[:min(count, 3)]   # NaN payloads
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    L().swap_f32(count, da.data_ptr(), db.data_ptr(), stream())
    torch.cuda.synchronize()
    ga, gb = da.cpu().numpy(), db.cpu().numpy()
    assert ga[:count].tobytes() == b[:count].tobytes() and gb[:count].tobytes() == a[:count].tobytes()
    assert ga[count:].tobytes() == a[count:].tobytes() and gb[count:].tobytes() == b[count:].tobytes()


# ---------------------------------------------------------------- the model: every single-GPU schedule
SCHEDULES = {
    'pipelined': {},
    'joined': {'MV3D_PIPELINE_FCADAM': '0'},
    'bucketed': {'MV3D_FUSE_FC_ADAM': '0'},
    'plain': {'MV3D_OVERLAP_ADAM': '0', 'MV3D_FUSE_FC_ADAM': '0'},
}
B = 64          # the fused fc kernels (plan_bwd_fused) and the pipelined fc optimiser apply at this batch
STEPS = 4


def _model(monkeypatch, env, **conf):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    for k in ('MV3D_FUSE_FC_ADAM', 'MV3D_PIPELINE_FCADAM', 'MV3D_OVERLAP_ADAM'):
        monkeypatch.setenv(k, env.get(k, '1'))
    return AppearanceFlowModel(dict({'batch_size': B, 'learning_rate': 1e-3}, **conf), load_tfrec=False, build_loss=True, device='cuda')


@pytest.fixture(scope="module")
def feeds():
    from tests.synth import appflow_feeds
    rng = np.random.default_rng(4)
    return [{k: torch.from_numpy(v).cuda() for k, v in appflow_feeds(rng, B).items()} for _ in range(2)]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_model_shadows_follow_the_rule_in_every_schedule(monkeypatch, feeds, schedule):
    """A twin without the switch runs 4 steps, its parameters read back after each.  The EMA model runs the same steps with no
    host synchronisation in between: its parameters equal the twin's and its shadows equal ema_rule iterated over the twin's
    snapshots, bit for bit.  A mis-ordered EMA launch (before its range's optimiser, or racing the next step's) gives other bits."""
    env = SCHEDULES[schedule]
    twin = _model(monkeypatch, env)
    g = twin.graph
    assert g.ema is None
    assert (g.plan_bwd_fused is not None) == (schedule in ('pipelined', 'joined'))
    snaps = []
    g.settle()
    torch.cuda.synchronize()
    snaps.append(g.params.cpu().numpy().copy())
    for step in range(STEPS):
        twin.train_step(**feeds[step % 2])
        g.settle()
        torch.cuda.synchronize()
        snaps.append(g.params.cpu().numpy().copy())
    assert not np.array_equal(snaps[0], snaps[-1])
    del twin, g
    variants = [False, True] if schedule == 'pipelined' else [False]        # ema_num_updates once: it only changes the scalar
    for num_updates in variants:
        model = _model(monkeypatch, env, ema_decay=0.5, ema_num_updates=num_updates)
        g = model.graph
        torch.cuda.synchronize()
        for step in range(STEPS):
            model.train_step(**feeds[step % 2])
            if schedule == 'pipelined':
                assert g._fc_pending and g._ema_pending             # both left running under the next step's encoder
        assert g.ema_updates == STEPS
        g.settle()
        torch.cuda.synchronize()
        params, shadows = g.params.cpu().numpy(), g.ema.cpu().numpy()
        want = snaps[0]
        for k in range(STEPS):
            want = ema_rule(want, snaps[k + 1], ema_one_minus_decay(0.5, k if num_updates else None))
        assert params.tobytes() == snaps[-1].tobytes(), (schedule, num_updates)
        bad = np.flatnonzero(shadows.view(np.int32) != want.view(np.int32))
        assert bad.size == 0, (schedule, num_updates, bad.size, bad[:4], bad[-4:])
        assert not np.array_equal(shadows, params)
        del model, g
    torch.cuda.empty_cache()


def test_ema_weights_runs_the_forward_pass_on_the_shadows(monkeypatch, feeds):
    """Inside ema_weights() the loss and the generated image are bitwise those of a second model whose variables were set to
    get_ema_variables(); after exit params, ema and the next train_step() loss are bitwise an undisturbed twin's."""
    def trained():
        m = _model(monkeypatch, {}, ema_decay=0.5)
        for step in range(2):
            m.train_step(**feeds[step % 2])
        return m
    model, twin = trained(), trained()
    g = model.graph
    carrier = _model(monkeypatch, {})
    carrier.graph.set_variables(g.get_ema_variables())
    want_loss = np.float32(float(carrier.forward(**feeds[1]))).view(np.uint32)
    want_gen = carrier.gen.numpy()
    raw_loss = np.float32(float(model.forward(**feeds[1]))).view(np.uint32)
    with model.ema_weights():
        got_loss = np.float32(float(model.forward(**feeds[1]))).view(np.uint32)
        got_gen = model.gen.numpy()
        with pytest.raises(RuntimeError):
            model.train_step(**feeds[0])
    assert got_loss == want_loss and got_gen.tobytes() == want_gen.tobytes()
    assert raw_loss != got_loss                                      # the shadows are not the weights
    g.settle()
    twin.graph.settle()
    torch.cuda.synchronize()
    assert _bits(g.params).tobytes() == _bits(twin.graph.params).tobytes()
    assert _bits(g.ema).tobytes() == _bits(twin.graph.ema).tobytes()
    la, lb = float(model.train_step(**feeds[0])), float(twin.train_step(**feeds[0]))
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    g.settle()
    twin.graph.settle()
    assert _bits(g.params).tobytes() == _bits(twin.graph.params).tobytes()
    assert _bits(g.ema).tobytes() == _bits(twin.graph.ema).tobytes()


# ---------------------------------------------------------------- the driver
def test_train_driver_saves_resumes_and_evaluates_the_shadows(tmp_path):
    """train.py with conf['ema_decay']: the checkpoint holds <var>/ExponentialMovingAverage and the counter; a resume that runs
    no step rewrites them unchanged; --evaluate scores the averaged weights (it equals model.evaluate of a model carrying the
    shadows as its variables) and differs from --evaluate --raw_weights."""
    from dynamic_multiview_3d_amd import train, tf_checkpoint
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    out = tmp_path / 'modeldata'
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 2, 'batch_size': 2, 'learning_rate': 1e-3, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle,\n"
        "  'ema_decay': 0.9}\n" % str(out))
    model = train.main(['--hyper', str(conf_py)])
    names = list(model.graph.variables)
    sd = tf_checkpoint.read_checkpoint(str(out / 'model'))
    assert all(k + '/' + EMA_SLOT in sd for k in names) and float(sd[EMA_COUNTER]) == 3.0       # iterations 0, 1, 2
    assert not np.array_equal(sd['fc1/Matrix/' + EMA_SLOT], sd['fc1/Matrix'])
    for ext in ('.index', '.data-00000-of-00001'):
        os.replace(str(out / 'model') + ext, str(out / 'model2') + ext)
    train.main(['--hyper', str(conf_py), '--pretrained', str(out / 'model2'), '--num_iterations', '1'])      # no step
    same = tf_checkpoint.read_checkpoint(str(out / 'model'))
    assert set(same) == set(sd) and all(np.array_equal(same[k], sd[k]) for k in sd)
    ema = train.main(['--hyper', str(conf_py), '--synthetic', '--evaluate', 'model2', '--eval_batches', '2'])
    raw = train.main(['--hyper', str(conf_py), '--synthetic', '--evaluate', 'model2', '--eval_batches', '2', '--raw_weights'])
    assert ema.pop('weights') == 'ema' and raw.pop('weights') == 'raw'
    assert ema['loss'] != raw['loss'] and ema['image/l1'] != raw['image/l1']
    m = AppFlowLowDimAngle({'batch_size': 2, 'learning_rate': 1e-3}, load_tfrec=False, device='cuda')
    m.graph.set_variables({k: sd[k + '/' + EMA_SLOT] for k in names})
    want = m.evaluate(train.SyntheticData(m, seed=0), 2)
    assert 'weights' not in want
    for key, value in want.items():
        assert ema[key] == value, (key, ema[key], value)
