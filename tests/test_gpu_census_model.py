"""conf['census_loss_weight'] through whole models on the GPU: loss and every parameter gradient against the float64 oracle graph
of the same model with the census term added from the test side (metrics.census_loss_host in float64 registered on the oracle's
tape), train steps that are finite, move every variable and repeat bit for bit (alone and combined with conf['ssim_loss_weight'],
where the census gradient is added onto the L2 + SSIM gradient), evaluate() reporting the term and the combined loss, and a
switch at 0.0 that changes nothing.  Bar: relative L2 at most 1e-3 per variable (the project's parity bar); measured values are
printed.  Decisions at the kinks of lrelu / relu / floor follow the device, as in tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics
from oracle import models as omodels
from oracle.graph import Node
from tests.synth import appflow_feeds
from tests.test_gpu_model import _activation_pattern_override, _perturb_biases, _sampling_cell_override

pytestmark = pytest.mark.gpu

WEIGHT = 0.5


def _with_census(builder, pred, target, weight, max_val):
    """The oracle builder with weight * census_loss(out[pred], feed[target]) (radius 3, eps 0.01: the defaults) added to its loss: value and gradient come from the
    float64 numpy twin and enter the reverse pass through the tape's recording hook."""
    def build(t, n):
        out = builder(t, n)
        a = out[pred]
        loss, grad = metrics.census_loss_host(a.v, n[target].v, max_val, np.float64, weight, 3, 0.01)
        y = Node(np.asarray(loss, dtype=t.dtype))
        t._rec([y], lambda: a.acc((grad * float(y.g)).astype(t.dtype)))
        out['loss'] = t.add(out['loss'], y)
        return out
    return build


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _models():
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    return {'appflow': (AppearanceFlowModel, {'batch_size': 2, 'learning_rate': 1e-4}, omodels.appearance_flow_builder('base'), 'gen', 'gen'),
            'base_prediction': (Base_Prediction_Model, bp, omodels.base_prediction_builder(bp), 'gen_image1', 'gen_image1')}


def _feeds(name, seed=3):
    f = appflow_feeds(np.random.default_rng(seed), 2)
    if name == 'base_prediction':
        f['dimage0'] = f['image0'][..., :1].copy()
        f['dimage1'] = f['image1'][..., :1].copy()
    return f


@pytest.mark.parametrize("name", ['appflow', 'base_prediction'])
def test_loss_and_gradients_match_the_float64_oracle_with_the_term_added(name):
    cls, conf, plain_builder, attr, key = _models()[name]
    model = cls(dict(conf, census_loss_weight=WEIGHT), load_tfrec=False, device='cuda')
    g = model.graph
    variables = _perturb_biases(g)
    feeds = _feeds(name)
    builder = _with_census(plain_builder, key, 'image1', WEIGHT, 1.0)
    run = lambda **kw: omodels.run(builder, {k: v.copy() for k, v in variables.items()}, feeds, dtype=np.float64, **kw)
    out, grads, tape = run()
    model.feed(**feeds)
    g.run_forward()
    g.run_backward()
    torch.cuda.synchronize()
    override, flips = _activation_pattern_override(model, tape)
    woverride, moved = _sampling_cell_override(model, tape)
    if flips or moved:
        out, grads, tape = run(sign_override=override, warp_override=woverride)
    plain = float(omodels.run(plain_builder, {k: v.copy() for k, v in variables.items()}, feeds, dtype=np.float64, backward=False)[0]['loss'])
    loss, want = float(g.loss_buf[0]), float(out['loss'])
    print('%s: loss %.8f oracle %.8f (of which census term %.6f); kink overrides: %d signs, %d cells' % (name, loss, want, want - plain, flips, moved))
    assert want - plain > 0.05                                           # the term is a real part of what is compared
    assert abs(loss - want) <= 2e-5 * abs(want)
    assert _rel_l2(getattr(model, attr).numpy(), out[key]) <= 1e-4
    got = g.get_gradients()
    assert set(got) == set(grads)
    errs = {k: _rel_l2(got[k], grads[k]) for k in grads}
    worst = max(errs, key=errs.get)
    print('%s: %d variables, worst relative L2 %.2e (%s), median %.2e' % (name, len(errs), errs[worst], worst, np.median(list(errs.values()))))
    assert errs[worst] <= 1e-3, (worst, errs[worst])


def _state_bits(model):
    model.graph.settle()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.graph.state_dict().items()}


def _five_steps(conf, feeds):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    model = AppearanceFlowModel(conf, load_tfrec=False, device='cuda')
    start = model.graph.get_variables()
    losses = [model.train_step(**feeds).clone()] + [model.train_step().clone() for _ in range(4)]      # the step returns a view of the loss word
    losses = torch.stack(losses).cpu().numpy()
    return model, start, losses, _state_bits(model)


@pytest.mark.parametrize("extra", [{}, {'ssim_loss_weight': 0.25}], ids=['alone', 'with_ssim'])
def test_train_steps_are_finite_move_every_variable_and_repeat_bit_for_bit(extra):
    conf = dict({'batch_size': 2, 'learning_rate': 1e-4, 'census_loss_weight': WEIGHT}, **extra)
    feeds = _feeds('appflow', seed=6)
    model, start, losses, state = _five_steps(conf, feeds)
    print('losses with the census term%s:' % (' and the SSIM term' if extra else ''), losses)
    assert np.all(np.isfinite(losses)) and np.all(losses > 0)
    end = model.graph.get_variables()
    assert set(end) == set(model.t_vars)
    for k in end:
        assert np.all(np.isfinite(end[k])) and not np.array_equal(end[k], start[k]), k
    _, _, losses2, state2 = _five_steps(conf, feeds)
    assert losses.tobytes() == losses2.tobytes()
    assert state.keys() == state2.keys()
    for k in state:
        assert state[k].tobytes() == state2[k].tobytes(), k

    # evaluate() on that model: one batch; 'image/census' is the unweighted term, and loss = L2 + weight * census (+ the SSIM term)
    class OneBatch:
        def next(self):
            return feeds
    res = model.evaluate(OneBatch(), 1)
    gen, tgt = model.gen.numpy().astype(np.float64), feeds['image1'].astype(np.float64)
    l2 = ((gen - tgt) ** 2).sum(axis=3).mean()
    want = l2 + WEIGHT * res['image/census'] + extra.get('ssim_loss_weight', 0.0) * (1.0 - res['image/ssim'])
    twin = float(metrics.census_loss_host(gen, tgt, 1.0, np.float64, 1.0, 3, 0.01)[0])
    print('evaluate: loss %.8f, L2 %.8f + %.2f * census %.8f (twin on the downloaded image %.8f) -> %.8f' % (res['loss'], l2, WEIGHT, res['image/census'], twin, want))
    assert abs(res['loss'] - want) <= 1e-5
    assert abs(res['image/census'] - twin) <= 2e-6 + 1e-5 * twin      # the kernel tests hold the value to the twin; this is the wiring
    if not extra:                                                     # without the key evaluate() reports no such figure
        from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
        plain = AppearanceFlowModel({'batch_size': 2, 'learning_rate': 1e-4}, load_tfrec=False, device='cuda')
        assert 'image/census' not in plain.evaluate(OneBatch(), 1)


def test_switch_at_zero_is_the_model_without_the_key():
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    feeds = _feeds('appflow', seed=8)
    res = []
    for extra in ({}, {'census_loss_weight': 0.0}):
        model = AppearanceFlowModel(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cuda')
        loss = model.train_step(**feeds)
        res.append((loss.cpu().numpy().tobytes(), _state_bits(model)))
    (l0, s0), (l1, s1) = res
    assert l0 == l1 and s0.keys() == s1.keys()
    for k in s0:
        assert s0[k].tobytes() == s1[k].tobytes(), k
