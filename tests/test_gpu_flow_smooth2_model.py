"""conf['flow_smoothness_order'] = 2 through whole models on the GPU, in the manner of tests/test_gpu_flow_smooth_model.py: loss,
the flow gradient and every parameter gradient against the float64 oracle graph of the same model with the second-order term added
from the test side (metrics.flow_smoothness_host(order=2) in float64 registered on the oracle's tape), in the three schedules the
graph has for the term (fused head; MV3D_FUSE_RESAMPLE=0; one more term on gen), the fused step's flow gradient against the unfused
step's bit for bit, the per-head terms of the multi-object model, a train step at order 1 that is the step without the key, and
evaluate()'s 'flow/smoothness2'.  Bar: relative L2 at most 1e-3 per variable and for the flow gradient (the project's parity bar);
measured values are printed.  Beside the oracle, the merge itself is checked exactly: the flow gradient with the switch on is the
flow gradient with the switch off plus the kernel's own gradient, one fp32 addition per element."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics
from oracle import models as omodels
from oracle.graph import Node
from tests.synth import appflow_feeds, multiobj_feeds
from tests.test_gpu_flow_smooth_model import ALPHA, BASE, EPS, WEIGHT, _against_oracle, _appflow, _state_bits
from tests.test_gpu_model import _perturb_biases

pytestmark = pytest.mark.gpu

ON = {'flow_smoothness_weight': WEIGHT, 'flow_smoothness_order': 2}


def _with_smoothness2(builder, captured, ssim_weight=0.0):
    """The oracle builder with WEIGHT * S2(out['flow_field'], guide = feed['image1']) added to its loss: value and gradient come
    from the float64 numpy twin and enter the reverse pass through the tape's recording hook."""
    def build(t, n):
        out = builder(t, n)
        f = out['flow_field']
        captured['flow'] = f
        loss, grad = metrics.flow_smoothness_host(f.v, n['image1'].v, ALPHA, EPS, np.float64, WEIGHT, order=2)
        y = Node(np.asarray(loss, dtype=t.dtype))
        t._rec([y], lambda: f.acc((grad * float(y.g)).astype(t.dtype)))
        captured['term'] = float(loss)
        if ssim_weight:
            a = out['gen']
            sl, sg = metrics.ssim_loss_host(a.v, n['image1'].v, 1.0, np.float64, ssim_weight)
            z = Node(np.asarray(sl, dtype=t.dtype))
            t._rec([z], lambda: a.acc((sg * float(z.g)).astype(t.dtype)))
            out['loss'] = t.add(out['loss'], z)
        out['loss'] = t.add(out['loss'], y)
        return out
    return build


def _fwd_bwd(model, variables, feeds):
    model.graph.set_variables(variables)
    model.feed(**feeds)
    model.graph.run_forward()
    model.graph.run_backward()
    torch.cuda.synchronize()


def _flow_gradient_is_the_sum(model_on, variables, feeds, label):
    """Exact check of the merge: same variables and feeds in the model without the switch give the consumer's flow gradient; the
    second-order kernel alone (store) gives the term's; the model with the switch on must hold their fp32 sum, element for element."""
    off = type(model_on)(dict(model_on.conf, flow_smoothness_weight=0.0), load_tfrec=False, device='cuda')
    _fwd_bwd(off, variables, feeds)
    assert np.array_equal(model_on.flow_field.numpy(), off.flow_field.numpy()), label
    own = torch.zeros(model_on.flow_field.shape, dtype=torch.float32, device='cuda')
    metrics.flow_smoothness(model_on.flow_field, model_on.image1, ALPHA, EPS, weight=WEIGHT, grad=own, order=2)
    first = torch.zeros_like(own)
    metrics.flow_smoothness(model_on.flow_field, model_on.image1, ALPHA, EPS, weight=WEIGHT, grad=first)
    want = off.flow_field.grad_value() + own
    assert own.abs().max() > 0 and not torch.equal(own, first)            # the second-order gradient, not the first-order one
    assert np.array_equal(model_on.flow_field.grad_value().cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), label


@pytest.mark.parametrize("schedule", ['fused', 'unfused', 'ssim'])
def test_loss_and_gradients_match_the_float64_oracle_with_the_term_added(schedule, monkeypatch):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    if schedule == 'unfused':
        monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    extra = {'ssim_loss_weight': 0.5} if schedule == 'ssim' else {}
    model = _appflow(**ON, **extra)
    fused = [n.fused_loss is not None for n in model.graph.nodes if isinstance(n, ResampleNode)]
    assert fused == [schedule == 'fused']
    assert [t.second_order for _, t in model.graph.loss_expr.terms if hasattr(t, 'second_order')] == [True]
    captured = {}
    builder = _with_smoothness2(omodels.appearance_flow_builder('base'), captured, ssim_weight=extra.get('ssim_loss_weight', 0.0))
    feeds = appflow_feeds(np.random.default_rng(3), 2)
    variables = _against_oracle(model, builder, captured, feeds, 'order 2, ' + schedule)
    _flow_gradient_is_the_sum(model, variables, feeds, schedule)


def test_the_fused_steps_flow_gradient_equals_the_unfused_steps_bit_for_bit(monkeypatch):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    feeds = appflow_feeds(np.random.default_rng(5), 2)
    fused = _appflow(**ON)
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    unfused = _appflow(**ON)
    monkeypatch.delenv('MV3D_FUSE_RESAMPLE')
    for m, want in ((fused, True), (unfused, False)):
        assert [n.fused_loss is not None for n in m.graph.nodes if isinstance(n, ResampleNode)] == [want]
    variables = _perturb_biases(fused.graph)
    for m in (fused, unfused):
        _fwd_bwd(m, variables, feeds)
    assert np.array_equal(fused.flow_field.numpy(), unfused.flow_field.numpy())
    gf, gu = fused.flow_field.grad_value().cpu().numpy(), unfused.flow_field.grad_value().cpu().numpy()
    assert np.abs(gf).max() > 0
    assert np.array_equal(gf.view(np.uint32), gu.view(np.uint32))
    lf, lu = float(fused.graph.loss_buf[0]), float(unfused.graph.loss_buf[0])
    print('loss fused %.9g unfused %.9g' % (lf, lu))
    assert abs(lf - lu) <= 3e-6 * lu                                      # the unfused head's loss comes from another kernel


def test_multiobject_per_head_terms_add_up():
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = dict(BASE, use_color='', combination_image='', gen_sep_images='', masked_image_loss='', fully_conv='')
    feeds = multiobj_feeds(np.random.default_rng(5), 2)
    on = MultiObjectAppFlow(dict(conf, **ON), load_tfrec=False, device='cuda')
    assert len(on.flow_heads) == 3 and [s[0] for s in on.smoothness2_terms] == [name for name, _ in on.flow_heads]
    variables = _perturb_biases(on.graph)
    _fwd_bwd(on, variables, feeds)
    off = MultiObjectAppFlow(conf, load_tfrec=False, device='cuda')
    _fwd_bwd(off, variables, feeds)
    image1 = feeds['image1']
    terms = [float(metrics.flow_smoothness_host(f.numpy(), image1, ALPHA, EPS, np.float64, WEIGHT, order=2)[0]) for _, f in on.flow_heads]
    l_on, l_off = float(on.graph.loss_buf[0]), float(off.graph.loss_buf[0])
    print('multi-object: loss on %.8f off %.8f, difference %.8f, sum of the %d head terms %.8f' % (l_on, l_off, l_on - l_off, len(terms), sum(terms)))
    assert min(terms) > 0
    # both losses are fp32 words built by one fp32 addition per term (7 and 4 of them): at most half an ulp, 6e-8 of the word,
    # per addition, 11 in all -> 6.6e-7 of the larger word; plus the kernels' own 2e-6 floor on the three terms
    assert abs((l_on - l_off) - sum(terms)) <= 1e-6 * l_on + 2e-6
    for (name, f_on), (_, f_off) in zip(on.flow_heads, off.flow_heads):
        assert np.array_equal(f_on.numpy(), f_off.numpy()), name
        own = torch.zeros(f_on.shape, dtype=torch.float32, device='cuda')
        metrics.flow_smoothness(f_on, on.image1, ALPHA, EPS, weight=WEIGHT, grad=own, order=2)
        want = f_off.grad_value() + own
        assert own.abs().max() > 0
        assert np.array_equal(f_on.grad_value().cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), name


class _OneBatch:
    def __init__(self, feeds):
        self.feeds = feeds

    def next(self):
        return self.feeds


def test_a_train_step_at_order_1_is_the_step_without_the_key():
    feeds = appflow_feeds(np.random.default_rng(8), 2)
    res = []
    for extra in ({}, {'flow_smoothness_order': 1}):
        model = _appflow(flow_smoothness_weight=WEIGHT, **extra)
        loss = model.train_step(**feeds)
        res.append((loss.cpu().numpy().tobytes(), _state_bits(model)))
    (l0, s0) = res[0]
    for l1, s1 in res[1:]:
        assert l0 == l1 and s0.keys() == s1.keys()
        for k in s0:
            assert s0[k].tobytes() == s1[k].tobytes(), k
    # ... and order 2 is another step
    model = _appflow(**ON)
    assert model.train_step(**feeds).cpu().numpy().tobytes() != l0


def test_evaluate_reports_the_second_order_term_under_its_own_key():
    feeds = appflow_feeds(np.random.default_rng(6), 2)
    model = _appflow(**ON)
    _perturb_biases(model.graph)
    res = model.evaluate(_OneBatch(feeds), 1)
    assert 'flow/smoothness2' in res and 'flow/smoothness' not in res
    eager = float(metrics.flow_smoothness(model.flow_field, model.image1, ALPHA, EPS, order=2))
    s64 = float(metrics.flow_smoothness_host(model.flow_field.numpy(), feeds['image1'], ALPHA, EPS, np.float64, order=2)[0])
    gen, tgt = model.gen.numpy().astype(np.float64), feeds['image1'].astype(np.float64)
    l2 = ((gen - tgt) ** 2).sum(axis=3).mean()
    print('evaluate: flow/smoothness2 %.9g eager %.9g twin %.9g; loss %.8f = L2 %.8f + %.2f * S2' % (res['flow/smoothness2'], eager, s64, res['loss'], l2, WEIGHT))
    assert eager > 0 and abs(res['flow/smoothness2'] - eager) <= 2e-6 * eager
    assert abs(eager - s64) <= max(1e-5 * s64, 2e-6)
    assert abs(res['loss'] - (l2 + WEIGHT * s64)) <= 1e-5
    # with the key at 1 the report is the first-order one
    first = _appflow(flow_smoothness_weight=WEIGHT, flow_smoothness_order=1).evaluate(_OneBatch(feeds), 1)
    assert 'flow/smoothness' in first and 'flow/smoothness2' not in first
