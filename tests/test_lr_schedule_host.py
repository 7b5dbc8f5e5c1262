"""Learning-rate schedules on the CPU (no GPU): learning_rate_at() against known answers and a second float64 formulation, the
conf keys in every model class, where mv3d_opt_set_lr sits in the schedules a CPU graph can issue, and the update counter in
checkpoints."""
import math

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd.graph import GLOBAL_STEP
from dynamic_multiview_3d_amd.lr_schedule import learning_rate_at, lr_schedule_from_conf, weight_decay_from_conf
from tests.test_ema_host import _direct_calls
from tests.test_optimizers_host import B64, _appflow, _labels, _lowdim

BASE = 1e-3


def _spec(**conf):
    return lr_schedule_from_conf(dict({'learning_rate': BASE}, **conf))


# ---------------------------------------------------------------- the rule
def test_exponential_known_answers():
    s = _spec(lr_schedule='exponential', lr_decay_steps=1000, lr_decay_rate=0.96)
    assert learning_rate_at(s, 0) == np.float32(BASE) and learning_rate_at(s, 1000) == np.float32(BASE * 0.96)
    assert learning_rate_at(s, 0).dtype == np.float32
    rates = [learning_rate_at(s, k) for k in range(0, 5000, 37)]
    assert all(a > b for a, b in zip(rates, rates[1:]))                     # strictly decreasing where float32 resolves it
    st = _spec(lr_schedule='exponential', lr_decay_steps=1000, lr_decay_rate=0.96, lr_staircase=True)
    for k in (0, 1, 500, 999):
        assert learning_rate_at(st, k) == np.float32(BASE)
    for k in (1000, 1001, 1999):
        assert learning_rate_at(st, k) == np.float32(BASE * 0.96)
    assert learning_rate_at(st, 2000) == np.float32(BASE * 0.96 ** 2)
    up = _spec(lr_schedule='exponential', lr_decay_steps=10, lr_decay_rate=1.5)
    assert learning_rate_at(up, 10) == np.float32(BASE * 1.5) and learning_rate_at(up, 5) > learning_rate_at(up, 4)


def test_piecewise_known_answers():
    bounds, values = [0, 10, 11, 500], [0.1, 0.05, 0.02, 0.01, 0.001]
    s = lr_schedule_from_conf({'lr_schedule': 'piecewise', 'lr_boundaries': bounds, 'lr_values': values, 'learning_rate': 123.0})
    for i, b in enumerate(bounds):                                          # TF's <=: the boundary step still has the earlier value
        if b > 0:
            want = values[i] if i == 0 or b - 1 > bounds[i - 1] else values[i - 1]
            assert learning_rate_at(s, b - 1) == np.float32(want), b
        assert learning_rate_at(s, b) == np.float32(values[i]), b
        assert learning_rate_at(s, b + 1) == np.float32(values[i + 1]), b
    assert learning_rate_at(s, 10 ** 9) == np.float32(values[-1])
    assert lr_schedule_from_conf({'lr_schedule': 'piecewise', 'lr_boundaries': [5], 'lr_values': [1.0, 0.5]}) is not None     # no base needed
    assert all(learning_rate_at(s, k).dtype == np.float32 for k in (0, 10, 600))


def test_cosine_known_answers():
    for alpha in (0.0, 0.1, 1.0):
        s = _spec(lr_schedule='cosine', lr_decay_steps=1000, **({'lr_alpha': alpha} if alpha else {}))
        assert learning_rate_at(s, 0) == np.float32(BASE)
        assert learning_rate_at(s, 500) == np.float32(BASE * (1 + alpha) / 2)           # cos(pi / 2) = 6e-17: invisible
        for k in (1000, 1001, 10 ** 7):
            assert learning_rate_at(s, k) == np.float32(BASE * alpha)
        rates = [learning_rate_at(s, k) for k in range(0, 1001, 50)]
        assert all(a >= b for a, b in zip(rates, rates[1:])) and (alpha == 1.0 or rates[0] > rates[-1])


def test_warmup_known_answers():
    W = 8
    s = _spec(lr_warmup_steps=W)                                            # with no kind at all
    assert s['kind'] is None
    assert learning_rate_at(s, 0) == np.float32(BASE / W)
    for k in (W - 1, W, W + 1, 10 ** 6):
        assert learning_rate_at(s, k) == np.float32(BASE)
    rates = [learning_rate_at(s, k) for k in range(W)]
    assert all(a < b for a, b in zip(rates, rates[1:]))
    e = _spec(lr_schedule='exponential', lr_decay_steps=2, lr_decay_rate=0.5, lr_warmup_steps=2)
    assert [learning_rate_at(e, k) for k in range(4)] == [np.float32(BASE * 0.5), np.float32(BASE * 0.5 ** 0.5), np.float32(BASE * 0.5),
                                                          np.float32(BASE * 0.5 ** 1.5)]
    assert _spec() is None and _spec(lr_warmup_steps=0) is None and _spec(lr_schedule=None, lr_alpha=None) is None


def _second_opinion(spec, step):
    """The same rules written differently, in float64: exp(log(rate) * x), the half-angle form of the cosine."""
    kind = spec['kind']
    if kind == 'exponential':
        x = float(step // spec['decay_steps']) if spec['staircase'] else step / spec['decay_steps']
        lr = spec['base'] * math.exp(math.log(spec['rate']) * x)
    elif kind == 'cosine':
        t = min(step, spec['decay_steps']) / spec['decay_steps']
        # (1 + cos x) / 2 = cos^2(x / 2) = sin^2((pi - x) / 2): the sine keeps its relative accuracy where the rate goes to 0
        lr = spec['base'] * ((1.0 - spec['alpha']) * math.sin(0.5 * math.pi * (1.0 - t)) ** 2 + spec['alpha'])
    elif kind == 'piecewise':
        lr = spec['values'][int(np.searchsorted(np.asarray(spec['boundaries']), step, side='left'))]
    else:
        lr = spec['base']
    if step < spec['warmup']:
        lr = lr * (step + 1) / spec['warmup']
    return lr


def test_agrees_with_a_second_float64_formulation_over_random_specs():
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(1000):
        kind = [None, 'exponential', 'piecewise', 'cosine'][int(rng.integers(0, 4))]
        conf = {'learning_rate': float(10.0 ** rng.uniform(-6, 0)), 'lr_warmup_steps': int(rng.integers(0 if kind else 1, 2000))}
        if kind:
            conf['lr_schedule'] = kind
        if kind in ('exponential', 'cosine'):
            conf['lr_decay_steps'] = int(rng.integers(1, 100000))
        if kind == 'exponential':
            conf['lr_decay_rate'] = float(rng.uniform(0.05, 1.0))
            conf['lr_staircase'] = bool(rng.integers(0, 2))
        if kind == 'cosine':
            conf['lr_alpha'] = float(rng.uniform(0, 1)) if rng.integers(0, 2) else 0.0
        if kind == 'piecewise':
            n = int(rng.integers(1, 6))
            conf['lr_boundaries'] = sorted(int(b) for b in rng.choice(200000, n, replace=False))
            conf['lr_values'] = [float(10.0 ** rng.uniform(-6, 0)) for _ in range(n + 1)]
        spec = lr_schedule_from_conf(conf)
        step = int(rng.integers(0, 200000)) if rng.integers(0, 4) else int(rng.integers(0, 50))
        got = learning_rate_at(spec, step)
        assert got.dtype == np.float32 and np.isfinite(got) and got >= 0
        want = np.float32(_second_opinion(spec, step))
        ulp = float(np.spacing(np.float32(max(abs(float(want)), float(np.finfo(np.float32).tiny)))))
        err = abs(float(got) - float(want)) / ulp
        worst = max(worst, err)
        assert err <= 1.0, (conf, step, got, want)
    print("worst disagreement: %.3g ulp" % worst)


# ---------------------------------------------------------------- conf validation, in every model class
GOOD = {
    'exponential': dict(lr_schedule='exponential', lr_decay_steps=100, lr_decay_rate=0.9),
    'piecewise': dict(lr_schedule='piecewise', lr_boundaries=[10, 20], lr_values=[1e-3, 1e-4, 1e-5]),
    'cosine': dict(lr_schedule='cosine', lr_decay_steps=100),
}
NAN, INF = float('nan'), float('inf')
BAD_LR = [
    dict(lr_schedule='linear'), dict(lr_schedule=True), dict(lr_schedule=3),                             # unknown kind
    dict(lr_schedule='exponential', lr_decay_steps=100), dict(lr_schedule='exponential', lr_decay_rate=0.9),      # required key missing
    dict(lr_schedule='piecewise', lr_boundaries=[10]), dict(lr_schedule='piecewise', lr_values=[1e-3, 1e-4]),
    dict(lr_schedule='cosine'),
    dict(GOOD['exponential'], lr_alpha=0.1), dict(GOOD['exponential'], lr_boundaries=[5]),                # a key of another kind
    dict(GOOD['cosine'], lr_decay_rate=0.5), dict(GOOD['cosine'], lr_staircase=True), dict(GOOD['piecewise'], lr_decay_steps=10),
    dict(lr_decay_steps=100), dict(lr_decay_rate=0.5), dict(lr_alpha=0.0), dict(lr_staircase=False), dict(lr_values=[1e-3]),      # ... or of none
    dict(lr_warmup_steps=5, lr_decay_steps=100),
    dict(lr_warmup=5), dict(GOOD['cosine'], lr_decay_step=5), dict(lr_shedule='cosine'),                  # typos
    dict(GOOD['exponential'], lr_decay_steps=True), dict(GOOD['exponential'], lr_decay_steps=0), dict(GOOD['exponential'], lr_decay_steps=-3),
    dict(GOOD['exponential'], lr_decay_steps=10.0), dict(GOOD['exponential'], lr_decay_steps=NAN),
    dict(GOOD['exponential'], lr_decay_rate=True), dict(GOOD['exponential'], lr_decay_rate=0), dict(GOOD['exponential'], lr_decay_rate=-0.5),
    dict(GOOD['exponential'], lr_decay_rate=NAN), dict(GOOD['exponential'], lr_decay_rate=INF), dict(GOOD['exponential'], lr_decay_rate='0.5'),
    dict(GOOD['exponential'], lr_staircase=1), dict(GOOD['exponential'], lr_staircase='yes'),
    dict(GOOD['cosine'], lr_alpha=-0.1), dict(GOOD['cosine'], lr_alpha=1.5), dict(GOOD['cosine'], lr_alpha=NAN), dict(GOOD['cosine'], lr_alpha=True),
    dict(GOOD['piecewise'], lr_boundaries=[20, 10]), dict(GOOD['piecewise'], lr_boundaries=[10, 10]), dict(GOOD['piecewise'], lr_boundaries=[-1, 10]),
    dict(GOOD['piecewise'], lr_boundaries=[1.5, 10]), dict(GOOD['piecewise'], lr_boundaries=[True, 10]), dict(GOOD['piecewise'], lr_boundaries=[]),
    dict(GOOD['piecewise'], lr_boundaries=10),
    dict(GOOD['piecewise'], lr_values=[1e-3, 1e-4]), dict(GOOD['piecewise'], lr_values=[1e-3, 1e-4, 0.0]), dict(GOOD['piecewise'], lr_values=[1e-3, -1e-4, 1e-5]),
    dict(GOOD['piecewise'], lr_values=[1e-3, NAN, 1e-5]), dict(GOOD['piecewise'], lr_values=[1e-3, INF, 1e-5]), dict(GOOD['piecewise'], lr_values=[1e-3, True, 1e-5]),
    dict(lr_warmup_steps=-1), dict(lr_warmup_steps=True), dict(lr_warmup_steps=2.5), dict(lr_warmup_steps=NAN),
]
BAD_WD = [dict(weight_decay=True), dict(weight_decay=False), dict(weight_decay=-0.1), dict(weight_decay=NAN), dict(weight_decay=INF),
          dict(weight_decay=-INF), dict(weight_decay='0.1')]


@pytest.mark.parametrize("extra", BAD_LR + BAD_WD, ids=lambda d: ','.join('%s=%r' % kv for kv in d.items())[:60])
def test_bad_conf_raises_value_error(extra):
    conf = dict({'learning_rate': BASE, 'batch_size': 2}, **extra)
    with pytest.raises(ValueError):
        lr_schedule_from_conf(conf)
        weight_decay_from_conf(conf)


def _model_classes():
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    from tests.layer_cases import MULTIOBJ_256_CONF
    return [lambda c: AppearanceFlowModel(c, load_tfrec=False, device='cpu'), lambda c: Base_Prediction_Model(c, load_tfrec=False, device='cpu'),
            lambda c: MultiObjectAppFlow(dict(MULTIOBJ_256_CONF, **c), load_tfrec=False, device='cpu'), lambda c: mv3d.mv3d_nobg_nodm(c, device='cpu')]


def test_every_model_class_checks_the_keys():
    """Every ValueError case of the schedule keys and of weight_decay, in each of the four classes: the keys are read before
    anything is built, so a case costs nothing."""
    for build in _model_classes():
        for extra in BAD_LR + BAD_WD:
            with pytest.raises(ValueError):
                build(dict({'learning_rate': BASE, 'batch_size': 2}, **extra))


def test_graph_switch_checks_the_value_like_the_conf_key():
    g = _lowdim({}).graph
    for bad in [d['weight_decay'] for d in BAD_WD]:
        with pytest.raises(ValueError):
            g.enable_weight_decay(bad)
    g.enable_weight_decay(None)
    g.enable_weight_decay(0)
    assert g.weight_decay is None


def test_weight_decay_from_conf():
    assert weight_decay_from_conf({}) is None and weight_decay_from_conf({'weight_decay': None}) is None
    assert weight_decay_from_conf({'weight_decay': 0}) is None and weight_decay_from_conf({'weight_decay': 0.0}) is None
    assert weight_decay_from_conf({'weight_decay': 0.01}) == 0.01 and weight_decay_from_conf({'weight_decay': 1}) == 1.0


# ---------------------------------------------------------------- where the launches sit
SCHED = dict(lr_schedule='exponential', lr_decay_steps=2, lr_decay_rate=0.5, lr_warmup_steps=2)
ADAM3 = ['adam_step_dev', 'adam_advance', 'adam_advance']


class _NoComm:
    rank = 0

    def allreduce_sum_(self, *a):
        pass


def _steps(g):
    """[(name, callable)]: every schedule a CPU graph can issue; each callable makes exactly one optimiser update."""
    out = [('plain', g.apply_optimizer)]
    if g.plan_bwd_fused is not None:
        out.append(('fused', g.run_backward_fused))
    if g.clip_norm is not None:
        out.append(('clipped', lambda: g.run_backward_clipped(data_parallel=False)))
    if not g.accum_steps:
        def dp():
            g.comm, mode, g.dp_mode = _NoComm(), g.dp_mode, 'allreduce'
            try:
                g.run_backward_overlapped(with_adam=True)
            finally:
                g.comm, g.dp_mode = None, mode
        out.append(('data parallel', dp))
    return out


@pytest.fixture(scope="module")
def graphs():
    class Lazy(dict):                   # the B = 64 pair (the fused plan exists there) is kept; the others are built where used
        def __missing__(self, k):
            c = {'clip': {'grad_clip_norm': 1.0}, 'accum': {'grad_accum_steps': 2}}[k]
            return _lowdim(c).graph, _lowdim(dict(c, **SCHED)).graph
    return Lazy(default=(_appflow(dict(B64)).graph, _appflow(dict(B64, **SCHED)).graph))


def test_keys_absent_the_launch_lists_are_the_parents(graphs):
    """The expected lists are written out here (what the parent commit's code issues, read off its schedules), not taken from a
    run of the parent.  The bucketed schedule (run_backward_with_adam) needs streams and is not issued on a CPU graph: there the
    GPU tests hold the keys-absent twins' bits (tests/test_gpu_lr_schedule.py, tests/test_gpu_ema.py)."""
    for kind in ('default', 'clip', 'accum'):
        off, on = graphs[kind]
        assert off.lr_spec is None and off.weight_decay is None and off._decay_table is None and on.lr_spec is not None
        for a, b in ((off.plan_fwd, on.plan_fwd), (off.plan_bwd, on.plan_bwd), (off.plan_bwd_fused, on.plan_bwd_fused)):
            assert (a is None) == (b is None) and (a is None or _labels(a) == _labels(b))      # the switch records nothing
    off = graphs['default'][0]
    nb = sum(1 for _, lo, hi in off.grad_buckets if hi > lo)
    want = {'plain': ADAM3, 'fused': ADAM3, 'data parallel': ['adam_step_dev'] * nb + ADAM3[1:]}
    for name, run in _steps(off):
        assert [c[0] for c in _direct_calls(off, run)] == want[name], name
    off = graphs['clip'][0]
    assert off.plan_bwd_fused is None
    assert [c[0] for c in _direct_calls(off, lambda: off.run_backward_clipped(data_parallel=False))] == ['grad_clip_scale'] + ADAM3
    off = graphs['accum'][0]
    assert [c[0] for c in _direct_calls(off, off.run_micro_step)] == ['grad_accumulate']
    assert [c[0] for c in _direct_calls(off, off.run_micro_step)] == ['grad_accumulate'] + ADAM3
    assert off.micro_step == 0 and off.global_step == 1


def _check_set_lr(g, calls, k):
    """Exactly one mv3d_opt_set_lr per record, with learning_rate_at(k + 1) bit for bit, behind that record's last optimiser /
    advance call."""
    recs = {g.opt_state.data_ptr(): [], g.opt_state.data_ptr() + 32: []}
    sets = {r: [] for r in recs}
    for i, (name, a) in enumerate(calls):
        if name == 'opt_set_lr':
            sets[a[0]].append((i, a[1]))
        elif name == 'adam_advance':
            recs[a[0]].append(i)
        elif name == 'adam_step_dev':
            recs[a[5]].append(i)
    want = learning_rate_at(g.lr_spec, k + 1)
    for r in recs:
        assert len(sets[r]) == 1, (r, sets)
        i, lr = sets[r][0]
        assert np.float32(lr).tobytes() == want.tobytes() and lr == float(want)
        assert recs[r] and i > max(recs[r]), (calls, r)


def test_schedule_on_one_set_lr_per_record_behind_its_last_reader(graphs):
    on = graphs['default'][1]
    assert on.learning_rate() == learning_rate_at(on.lr_spec, 0) and on.learning_rate().dtype == np.float32
    assert on.opt_state[0].item() == float(on.learning_rate()) and on.opt_state[8].item() == float(on.learning_rate())
    for name, run in _steps(on):
        k = on.global_step
        calls = _direct_calls(on, run)
        _check_set_lr(on, calls, k)
        assert on.global_step == k + 1 and on.learning_rate() == learning_rate_at(on.lr_spec, k + 1), name
    # the fused step: the fc record's write sits behind the bias-span launch and its advance, in front of the main record's
    names = [c[0] for c in _direct_calls(on, on.run_backward_fused)]
    assert names == ['adam_step_dev', 'adam_advance', 'opt_set_lr', 'adam_advance', 'opt_set_lr']
    on = graphs['clip'][1]
    k = on.global_step
    _check_set_lr(on, _direct_calls(on, lambda: on.run_backward_clipped(data_parallel=False)), k)
    on = graphs['accum'][1]
    k = on.global_step
    first = _direct_calls(on, on.run_micro_step)                            # micro-step 1 of 2: no update, no write
    assert [c[0] for c in first] == ['grad_accumulate'] and on.global_step == k
    _check_set_lr(on, _direct_calls(on, on.run_micro_step), k)
    assert on.global_step == k + 1


def test_momentum_and_gd_write_the_rate_too():
    for extra in (dict(optimizer='momentum', momentum=0.9), dict(optimizer='sgd')):
        g = _lowdim(dict(extra, **SCHED)).graph
        calls = _direct_calls(g, g.apply_optimizer)
        assert [c[0] for c in calls] == ['sgd_step_dev', 'opt_set_lr', 'opt_set_lr']
        assert {c[1][0] for c in calls[1:]} == {g.opt_state.data_ptr(), g.opt_state.data_ptr() + 32}
        assert all(c[1][1] == float(learning_rate_at(g.lr_spec, 1)) for c in calls[1:])


# ---------------------------------------------------------------- the counter in checkpoints
def test_global_step_in_checkpoints(tmp_path):
    from dynamic_multiview_3d_amd import tf_checkpoint
    plain = _lowdim({})
    assert GLOBAL_STEP == 'global_step' and GLOBAL_STEP not in plain.graph.state_dict()
    want_keys = set(plain.graph.variables) | {'beta1_power', 'beta2_power'} | {k + s for k, v in plain.graph.variables.items()
                                                                               if v.has_grad for s in ('/Adam', '/Adam_1')}
    assert set(plain.graph.state_dict()) == want_keys                       # everything off: exactly today's keys
    plain.graph.global_step = 5
    assert GLOBAL_STEP not in plain.graph.state_dict()
    for conf in (SCHED, {'lr_warmup_steps': 3}, {'weight_decay': 0.01}):
        m = _lowdim(conf)
        g = m.graph
        assert set(g.state_dict()) == want_keys | {GLOBAL_STEP}
        g.set_global_step(7)
        assert g.opt_state[0].item() == float(g.learning_rate()) == g.opt_state[8].item()
        prefix = m.saver.save(None, str(tmp_path / 'model'), global_step=7)
        sd = tf_checkpoint.read_checkpoint(prefix)
        assert sd[GLOBAL_STEP].dtype == np.int64 and int(sd[GLOBAL_STEP]) == 7 and sd[GLOBAL_STEP].shape == ()
        m2 = _lowdim(conf, seed=8)
        assert m2.graph.global_step == 0
        m2.saver.restore(None, prefix)
        assert m2.graph.global_step == 7 and m2.graph.global_step_restored and torch.equal(m2.graph.params, g.params)
        assert m2.graph.opt_state[0].item() == float(g.learning_rate()) and m2.graph.opt_state[8].item() == float(g.learning_rate())
        # a checkpoint without the counter: 0, and the caller's set_global_step re-uploads the rate
        bare = plain.saver.save(None, str(tmp_path / 'bare'))
        m2.saver.restore(None, bare)
        assert m2.graph.global_step == 0 and not m2.graph.global_step_restored
        assert m2.graph.opt_state[0].item() == float(learning_rate_at(g.lr_spec, 0)) if g.lr_spec else True
        m2.graph.set_global_step(3)
        if g.lr_spec:
            assert m2.graph.opt_state[8].item() == float(learning_rate_at(g.lr_spec, 3))
        # the counter into a model with everything off: unexpected, like any other entry
        with pytest.raises(KeyError):
            _lowdim({}).saver.restore(None, prefix)
    for bad in (-1, True, 2.5):
        with pytest.raises(ValueError):
            plain.graph.set_global_step(bad)
    a = _lowdim(dict(SCHED, grad_accum_steps=2)).graph
    a.micro_step = 1                                                        # inside a cycle
    with pytest.raises(RuntimeError):
        a.state_dict()
    with pytest.raises(RuntimeError):
        a.set_global_step(4)
    a.micro_step = 0
    assert int(a.state_dict()[GLOBAL_STEP]) == 0
