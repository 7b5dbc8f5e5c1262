"""conf['flow_smoothness_weight'] through whole models on the GPU, in the manner of tests/test_gpu_ssim_model.py: loss, the flow
gradient and every parameter gradient against the float64 oracle graph of the same model with the smoothness term added from
the test side (metrics.flow_smoothness_host in float64 registered on the oracle's tape), in the three schedules the graph has
for the term (fused head; MV3D_FUSE_RESAMPLE=0; SSIM on), a graph whose loss is the term alone, the per-head terms of the
multi-object model, train steps that are finite, move every variable and repeat bit for bit, a switch at 0 that changes nothing,
and evaluate()'s 'flow/smoothness'.  Bar: relative L2 at most 1e-3 per variable and for the flow gradient (the project's parity
bar); measured values are printed.  Decisions at the kinks of lrelu / relu / floor follow the device, as in
tests/test_gpu_model.py.  Beside the oracle, the merge itself is checked exactly: the flow gradient with the switch on is the
flow gradient with the switch off plus the kernel's own gradient, one fp32 addition per element."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics
from oracle import models as omodels
from oracle.graph import Node
from tests.synth import appflow_feeds, multiobj_feeds
from tests.test_gpu_model import _activation_pattern_override, _perturb_biases, _sampling_cell_override

pytestmark = pytest.mark.gpu

WEIGHT, ALPHA, EPS = 0.2, 10.0, 1e-3
BASE = {'batch_size': 2, 'learning_rate': 1e-4}


def _with_smoothness(builder, weight, alpha, eps, captured, alone=False, ssim_weight=0.0):
    """The oracle builder with weight * S(out['flow_field'], guide = feed['image1']) added to its loss (or as its whole loss):
    value and gradient come from the float64 numpy twin and enter the reverse pass through the tape's recording hook."""
    def build(t, n):
        out = builder(t, n)
        f = out['flow_field']
        captured['flow'] = f
        loss, grad = metrics.flow_smoothness_host(f.v, n['image1'].v if alpha else None, alpha, eps, np.float64, weight)
        y = Node(np.asarray(loss, dtype=t.dtype))
        t._rec([y], lambda: f.acc((grad * float(y.g)).astype(t.dtype)))
        captured['term'] = float(loss)
        if ssim_weight:
            a = out['gen']
            sl, sg = metrics.ssim_loss_host(a.v, n['image1'].v, 1.0, np.float64, ssim_weight)
            z = Node(np.asarray(sl, dtype=t.dtype))
            t._rec([z], lambda: a.acc((sg * float(z.g)).astype(t.dtype)))
            out['loss'] = t.add(out['loss'], z)
        out['loss'] = t.scale(y, 1.0) if alone else t.add(out['loss'], y)
        return out
    return build


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict(BASE, **extra), load_tfrec=False, device='cuda')


def _against_oracle(model, builder, captured, feeds, label):
    g = model.graph
    variables = _perturb_biases(g)
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
    loss, want = float(g.loss_buf[0]), float(out['loss'])
    flow_err = _rel_l2(model.flow_field.grad_value().cpu().numpy(), captured['flow'].g)
    print('%s: loss %.8f oracle %.8f (of which smoothness term %.6f); flow gradient rel L2 %.2e; kink overrides: %d signs, %d cells'
          % (label, loss, want, captured['term'], flow_err, flips, moved))
    assert captured['term'] > 0.01 * want                                # the term is a real part of what is compared
    assert abs(loss - want) <= 2e-5 * abs(want)
    assert _rel_l2(model.flow_field.numpy(), out['flow_field']) <= 1e-4
    assert flow_err <= 1e-3
    got = g.get_gradients()
    assert set(got) == set(grads)
    errs = {k: _rel_l2(got[k], grads[k]) for k in grads}
    worst = max(errs, key=errs.get)
    print('%s: %d variables, worst relative L2 %.2e (%s), flow_field/w %.2e, median %.2e'
          % (label, len(errs), errs[worst], worst, errs['flow_field/w'], np.median(list(errs.values()))))
    assert errs[worst] <= 1e-3, (worst, errs[worst])
    return variables


def _flow_gradient_is_the_sum(model_on, variables, feeds, extra, heads=None):
    """Exact check of the merge: same variables and feeds in the model without the switch give the consumer's flow gradient; the
    kernel alone (store) gives the term's; the model with the switch on must hold their fp32 sum, element for element."""
    off = type(model_on)(dict(model_on.conf, flow_smoothness_weight=0.0), load_tfrec=False, device='cuda')
    off.graph.set_variables(variables)
    off.feed(**feeds)
    off.graph.run_forward()
    off.graph.run_backward()
    torch.cuda.synchronize()
    heads = heads or [('flow', model_on.flow_field, off.flow_field, model_on.image1)]
    for name, f_on, f_off, guide in heads:
        assert np.array_equal(f_on.numpy(), f_off.numpy()), name
        own = torch.zeros(f_on.shape, dtype=torch.float32, device='cuda')
        metrics.flow_smoothness(f_on, guide, ALPHA, EPS, weight=WEIGHT, grad=own)
        want = f_off.grad_value() + own
        assert own.abs().max() > 0
        assert np.array_equal(f_on.grad_value().cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), (name, extra)


@pytest.mark.parametrize("schedule", ['fused', 'unfused', 'ssim'])
def test_loss_and_gradients_match_the_float64_oracle_with_the_term_added(schedule, monkeypatch):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    if schedule == 'unfused':
        monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    extra = {'ssim_loss_weight': 0.5} if schedule == 'ssim' else {}
    model = _appflow(flow_smoothness_weight=WEIGHT, **extra)
    fused = [n.fused_loss is not None for n in model.graph.nodes if isinstance(n, ResampleNode)]
    assert fused == [schedule == 'fused']
    captured = {}
    builder = _with_smoothness(omodels.appearance_flow_builder('base'), WEIGHT, ALPHA, EPS, captured, ssim_weight=extra.get('ssim_loss_weight', 0.0))
    feeds = appflow_feeds(np.random.default_rng(3), 2)
    variables = _against_oracle(model, builder, captured, feeds, schedule)
    _flow_gradient_is_the_sum(model, variables, feeds, schedule)


def test_smoothness_alone_stores_the_gradient_and_the_producer_runs_from_it():
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf

    class SmoothOnly(AppearanceFlowModel):
        def build_loss(self):
            self.loss = tf_utils.flow_smoothness_loss(self.flow_field, self.image1, ALPHA, EPS) * WEIGHT
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    model = _appflow(SmoothOnly)
    model.flow_field.grad_value().fill_(123.0)                           # stale contents the store must replace
    captured = {}
    builder = _with_smoothness(omodels.appearance_flow_builder('base'), WEIGHT, ALPHA, EPS, captured, alone=True)
    feeds = appflow_feeds(np.random.default_rng(4), 2)
    _against_oracle(model, builder, captured, feeds, 'alone')
    own = torch.zeros(model.flow_field.shape, dtype=torch.float32, device='cuda')
    metrics.flow_smoothness(model.flow_field, model.image1, ALPHA, EPS, weight=WEIGHT, grad=own)
    assert torch.equal(model.flow_field.grad_value(), own)              # stored: nothing of the stale buffer is left


def test_two_terms_alone_on_one_flow_give_the_sum_of_the_two_kernel_gradients():
    """No other writer of the flow gradient and two terms on it: the first stores, the second adds -- the buffer holds the fp32 sum
    of the two kernel gradients element for element, and the loss both values."""
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf
    wa, wb = 0.75, 0.25

    class TwoTerms(AppearanceFlowModel):
        def build_loss(self):
            self.loss = (tf_utils.flow_smoothness_loss(self.flow_field, self.image1, ALPHA, EPS) * wa
                         + tf_utils.flow_smoothness_loss(self.flow_field, None, 0.0, EPS) * wb)
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    model = _appflow(TwoTerms)
    model.flow_field.grad_value().fill_(123.0)
    feeds = appflow_feeds(np.random.default_rng(9), 2)
    model.feed(**feeds)
    for _ in range(2):                                                   # replayed: the first launch stores every time
        model.graph.run_forward()
        model.graph.run_backward()
        torch.cuda.synchronize()
        ga = torch.zeros(model.flow_field.shape, dtype=torch.float32, device='cuda')
        gb = torch.zeros(model.flow_field.shape, dtype=torch.float32, device='cuda')
        la = metrics.flow_smoothness(model.flow_field, model.image1, ALPHA, EPS, weight=wa, grad=ga)
        lb = metrics.flow_smoothness(model.flow_field, None, 0.0, EPS, weight=wb, grad=gb)
        assert ga.abs().max() > 0 and gb.abs().max() > 0 and not torch.equal(ga, gb)
        got = model.flow_field.grad_value()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), (ga + gb).cpu().numpy().view(np.uint32))
        assert float(model.graph.loss_buf[0]) == float(la + lb)           # the first term stores the loss word, the second adds
    flow = model.flow_field.numpy()
    g64 = (metrics.flow_smoothness_host(flow, feeds['image1'], ALPHA, EPS, np.float64, wa)[1]
           + metrics.flow_smoothness_host(flow, None, 0.0, EPS, np.float64, wb)[1])
    rel = _rel_l2(got.cpu().numpy(), g64)
    print('two terms alone: flow gradient against the float64 sum of the twins, relative L2 %.2e' % rel)
    assert rel <= 1e-3


def test_multiobject_per_head_terms_add_up():
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = dict(BASE, use_color='', combination_image='', gen_sep_images='', masked_image_loss='', fully_conv='')
    feeds = multiobj_feeds(np.random.default_rng(5), 2)
    on = MultiObjectAppFlow(dict(conf, flow_smoothness_weight=WEIGHT), load_tfrec=False, device='cuda')
    assert len(on.flow_heads) == 3
    variables = _perturb_biases(on.graph)
    on.feed(**feeds)
    on.graph.run_forward()
    on.graph.run_backward()
    torch.cuda.synchronize()
    off = MultiObjectAppFlow(conf, load_tfrec=False, device='cuda')
    off.graph.set_variables(variables)
    off.feed(**feeds)
    off.graph.run_forward()
    off.graph.run_backward()
    torch.cuda.synchronize()
    image1 = feeds['image1']
    terms = [float(metrics.flow_smoothness_host(f.numpy(), image1, ALPHA, EPS, np.float64, WEIGHT)[0]) for _, f in on.flow_heads]
    l_on, l_off = float(on.graph.loss_buf[0]), float(off.graph.loss_buf[0])
    print('multi-object: loss on %.8f off %.8f, difference %.8f, sum of the %d head terms %.8f' % (l_on, l_off, l_on - l_off, len(terms), sum(terms)))
    assert min(terms) > 0
    # both losses are fp32 words built by one fp32 addition per term (7 and 4 of them): at most half an ulp, 6e-8 of the word,
    # per addition, 11 in all -> 6.6e-7 of the larger word; plus the kernels' own 2e-6 floor on the three terms
    assert abs((l_on - l_off) - sum(terms)) <= 1e-6 * l_on + 2e-6
    for (name, f_on), (_, f_off) in zip(on.flow_heads, off.flow_heads):
        assert np.array_equal(f_on.numpy(), f_off.numpy()), name
        own = torch.zeros(f_on.shape, dtype=torch.float32, device='cuda')
        metrics.flow_smoothness(f_on, on.image1, ALPHA, EPS, weight=WEIGHT, grad=own)
        want = f_off.grad_value() + own
        assert np.array_equal(f_on.grad_value().cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), name
    g_on, g_off = on.graph.get_gradients(), off.graph.get_gradients()
    assert set(g_on) == set(g_off)
    assert all(not np.array_equal(g_on[k], g_off[k]) for k in g_on if k.startswith('dec_image1') and k.endswith('d0/w'))


def _state_bits(model):
    model.graph.settle()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.graph.state_dict().items()}


def _five_steps(conf, feeds):
    model = _appflow(**conf)
    start = model.graph.get_variables()
    losses = [model.train_step(**feeds).clone()] + [model.train_step().clone() for _ in range(4)]      # the step returns a view of the loss word
    losses = torch.stack(losses).cpu().numpy()
    return model, start, losses, _state_bits(model)


def test_train_steps_are_finite_move_every_variable_and_repeat_bit_for_bit():
    conf = {'flow_smoothness_weight': WEIGHT}
    feeds = appflow_feeds(np.random.default_rng(6), 2)
    model, start, losses, state = _five_steps(conf, feeds)
    print('losses with the smoothness term:', losses)
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

    # evaluate() on that model: one batch; 'flow/smoothness' is the unweighted twin on the downloaded flow, by the kernel tests' rule
    class OneBatch:
        def next(self):
            return feeds
    res = model.evaluate(OneBatch(), 1)
    flow = model.flow_field.numpy()
    s64 = float(metrics.flow_smoothness_host(flow, feeds['image1'], ALPHA, EPS, np.float64)[0])
    s32 = float(metrics.flow_smoothness_host(flow, feeds['image1'], ALPHA, EPS, np.float32)[0])
    gen, tgt = model.gen.numpy().astype(np.float64), feeds['image1'].astype(np.float64)
    l2 = ((gen - tgt) ** 2).sum(axis=3).mean()
    print('evaluate: flow/smoothness %.8f twin %.8f (float32 gap %.2e); loss %.8f = L2 %.8f + %.2f * S'
          % (res['flow/smoothness'], s64, abs(s32 - s64), res['loss'], l2, WEIGHT))
    assert abs(res['flow/smoothness'] - s64) <= max(4 * abs(s32 - s64), 2e-6)
    assert abs(res['loss'] - (l2 + WEIGHT * s64)) <= 1e-5


def test_switch_at_zero_is_the_model_without_the_key():
    feeds = appflow_feeds(np.random.default_rng(8), 2)
    res = []
    for extra in ({}, {'flow_smoothness_weight': 0.0}):
        model = _appflow(**extra)
        loss = model.train_step(**feeds)
        res.append((loss.cpu().numpy().tobytes(), _state_bits(model)))
        if extra:
            class OneBatch:
                def next(self):
                    return feeds
            assert 'flow/smoothness' not in model.evaluate(OneBatch(), 1)
    (l0, s0), (l1, s1) = res
    assert l0 == l1 and s0.keys() == s1.keys()
    for k in s0:
        assert s0[k].tobytes() == s1[k].tobytes(), k
