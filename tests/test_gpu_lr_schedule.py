"""Learning-rate schedules and decoupled weight decay in the model on the MI355X: unsynchronised steps in every single-GPU
schedule against twins that set the rate / apply the rule from the host between synchronised steps, and train.py's log rows,
checkpoint counter, resume and event file."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd.graph import GLOBAL_STEP
from dynamic_multiview_3d_amd.model_base import (ema_one_minus_decay, ema_rule, learning_rate_at, lr_schedule_from_conf,
                                                 weight_decay_factor, weight_decay_rule)
from tests.test_gpu_ema import SCHEDULES, STEPS, _model, feeds      # noqa: F401  (feeds: the module's fixture)

pytestmark = pytest.mark.gpu

LR = 1e-3
SCHED = dict(lr_schedule='exponential', lr_decay_steps=2, lr_decay_rate=0.5, lr_warmup_steps=2)
WD = 0.1            # f = float32(1e-3 * 0.1) = 1e-4: moves bits in 4 steps
# (environment, extra conf, train_step() calls per update)
CASES = dict({k: (env, {}, 1) for k, env in SCHEDULES.items()}, clipped=({}, {'grad_clip_norm': 1.0}, 1),
             accumulation=({}, {'grad_accum_steps': 2}, 2))


def _update(model, feeds, k, n):
    for j in range(n):
        model.train_step(**feeds[(k * n + j) % 2])


def _snapshot(g):
    g.settle()
    torch.cuda.synchronize()
    return g.params.cpu().numpy().copy()


@pytest.mark.parametrize("case", list(CASES))
def test_scheduled_rate_equals_a_twin_that_uploads_it_before_every_step(monkeypatch, feeds, case):
    """The twin has a constant rate; before update k its graph.lr is set to learning_rate_at(k) and uploaded, and it is
    synchronised between steps.  The scheduled model runs the same updates with no host synchronisation: the same bits, and both
    optimiser records end at learning_rate_at(4).  A rate written in front of a step, or on another stream than its record's last
    reader, races the fused fc launches and gives other bits."""
    env, extra, n = CASES[case]
    spec = lr_schedule_from_conf(dict({'learning_rate': LR}, **SCHED))
    twin = _model(monkeypatch, env, **extra)
    g = twin.graph
    assert g.lr_spec is None and (g.plan_bwd_fused is not None) == (case in ('pipelined', 'joined'))
    first = _snapshot(g)
    for k in range(STEPS):
        g.lr = float(learning_rate_at(spec, k))
        g.upload_optimizer_state()
        _update(twin, feeds, k, n)
        g.settle()
        torch.cuda.synchronize()
    want = _snapshot(g)
    assert not np.array_equal(first, want)
    del twin, g
    model = _model(monkeypatch, env, **dict(extra, **SCHED))
    g = model.graph
    torch.cuda.synchronize()
    assert g.opt_state[0].item() == float(learning_rate_at(spec, 0)) == g.opt_state[8].item()
    for k in range(STEPS):
        assert g.learning_rate() == learning_rate_at(spec, k)
        _update(model, feeds, k, n)
        if case == 'pipelined':
            assert g._fc_pending
    assert g.global_step == STEPS
    got = _snapshot(g)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (case, bad.size, bad[:4], bad[-4:])
    state = g.opt_state.cpu().numpy()
    assert state[0].tobytes() == learning_rate_at(spec, STEPS).tobytes() == state[8].tobytes()
    del model, g
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", list(CASES))
def test_decay_equals_a_twin_that_applies_the_rule_on_the_host(monkeypatch, feeds, case):
    """The twin has no weight_decay key; after every update it synchronises, applies weight_decay_rule to a download of params and
    uploads the result.  The decayed model runs the same updates unsynchronised: the same bits; with ema_decay as well its shadows
    equal ema_rule iterated over the twin's snapshots.  A decay launch the next forward pass does not wait for (the fc matrices
    under the pipelined optimiser) gives other bits."""
    env, extra, n = CASES[case]
    f = weight_decay_factor(np.float32(LR), WD)
    assert 0 < f < 1e-3
    snaps, ranges = None, None
    for ema in (False, True):
        model = _model(monkeypatch, env, **dict(extra, weight_decay=WD, **({'ema_decay': 0.5} if ema else {})))
        g = model.graph
        assert g.weight_decay == WD and len(g._decay_ranges) == 26
        if snaps is None:                                   # the twin, once: it needs the decayed model's table
            ranges = list(g._decay_ranges)
            twin = _model(monkeypatch, env, **extra)
            tg = twin.graph
            assert tg.weight_decay is None and tg._decay_table is None
            snaps = [_snapshot(tg)]
            for k in range(STEPS):
                _update(twin, feeds, k, n)
                new = weight_decay_rule(_snapshot(tg), ranges, f)
                tg.params.copy_(torch.from_numpy(new))
                torch.cuda.synchronize()
                snaps.append(new)
            assert not np.array_equal(snaps[0], snaps[-1])
            del twin, tg
        torch.cuda.synchronize()
        for k in range(STEPS):
            _update(model, feeds, k, n)
            if case == 'pipelined':
                assert g._fc_pending                        # left running under the next step's encoder
        assert g.global_step == STEPS
        got = _snapshot(g)
        bad = np.flatnonzero(got.view(np.int32) != snaps[-1].view(np.int32))
        assert bad.size == 0, (case, ema, bad.size, bad[:4], bad[-4:])
        if ema:
            assert g.ema_updates == STEPS
            shadows = g.ema.cpu().numpy()
            want = snaps[0]
            for k in range(STEPS):
                want = ema_rule(want, snaps[k + 1], ema_one_minus_decay(0.5))
            bad = np.flatnonzero(shadows.view(np.int32) != want.view(np.int32))
            assert bad.size == 0, (case, bad.size, bad[:4], bad[-4:])
            assert not np.array_equal(shadows, got)
        del model, g
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the driver
def test_train_driver_logs_saves_and_resumes_the_schedule(tmp_path):
    """train.py --synthetic, 12 iterations with a schedule: the learning_rate rows equal the rule, the checkpoint carries
    global_step, a resumed run's next row continues the schedule (from the checkpoint's counter, and for a checkpoint without it
    from the file name's iteration), and the tag is in the event file."""
    from dynamic_multiview_3d_amd import summary, tf_checkpoint, train
    out = tmp_path / 'modeldata'
    conf_py = tmp_path / 'conf.py'
    sched = dict(lr_schedule='cosine', lr_decay_steps=40, lr_alpha=0.1, lr_warmup_steps=3)

    def write_conf(iterations):
        conf_py.write_text(
            "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
            "configuration = dict({'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
            "  'num_iterations': %d, 'batch_size': 2, 'learning_rate': 1e-3, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle},\n"
            "  **%r)\n" % (str(out), iterations, sched))
    write_conf(12)
    spec = lr_schedule_from_conf(dict({'learning_rate': 1e-3}, **sched))
    model = train.main(['--hyper', str(conf_py), '--synthetic', '--event_log'])
    assert model.graph.global_step == 13                                   # iterations 0 .. 12
    rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
    assert [r['itr'] for r in rows] == [0, 10]
    for r in rows:
        assert set(r) == {'itr', 'training_loss', 'learning_rate'} and r['learning_rate'] == float(learning_rate_at(spec, r['itr']))
    assert rows[0]['learning_rate'] != rows[1]['learning_rate']
    files = glob.glob(str(out / 'events.out.tfevents*'))
    assert len(files) == 1
    got = [(e['step'], e['scalars'][0]) for e in summary.read_events(files[0])[1:]]
    assert got == [(r['itr'], (key, float(np.float32(r[key])))) for r in rows for key in ('training_loss', 'learning_rate')]
    sd = tf_checkpoint.read_checkpoint(str(out / 'model'))
    assert sd[GLOBAL_STEP].dtype == np.int64 and int(sd[GLOBAL_STEP]) == 13
    # resume at iteration 13, to 20: from the counter, and from the file name where the checkpoint has none
    for ext in ('.index', '.data-00000-of-00001'):
        os.replace(str(out / 'model') + ext, str(out / 'model13') + ext)
    tf_checkpoint.write_checkpoint(str(out / 'bare13'), {k: v for k, v in sd.items() if k != GLOBAL_STEP})
    write_conf(20)
    for name in ('model13', 'bare13'):
        os.remove(out / 'train_log.jsonl')
        resumed = train.main(['--hyper', str(conf_py), '--synthetic', '--pretrained', str(out / name)])
        assert resumed.graph.global_step == 21
        rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
        assert [r['itr'] for r in rows] == [20] and rows[0]['learning_rate'] == float(learning_rate_at(spec, 20)), name
    state = resumed.graph.opt_state.cpu().numpy()
    assert state[0].tobytes() == learning_rate_at(spec, 21).tobytes() == state[8].tobytes()
