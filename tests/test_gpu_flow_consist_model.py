"""conf['flow_consistency_weight'] with conf['pair_swap'] through AppearanceFlowModel on the GPU, in the manner of
tests/test_gpu_flow_smooth_model.py: B = 4, 128 x 128, pair-swapped synthetic feeds (two pairs and their reverses).  Loss, the flow
gradient and every parameter gradient against the float64 oracle graph of the same model with the consistency term added from the
test side (metrics.flow_consistency_host in float64 registered on the oracle's tape), with the fused and the unfused head and once
together with the smoothness and multi-scale terms; train steps that are finite, move every variable and repeat bit for bit; a
weight of 0 that changes nothing; evaluate()'s two names.  Bars as in that file: relative L2 at most 1e-3 per variable and for the
flow gradient, the loss to 2e-5; measured values are printed.  Decisions at the kinks of lrelu / floor follow the device, by the
overrides of tests/test_gpu_model.py.  Beside the oracle the merge is checked exactly: the flow gradient with the switch on is the
flow gradient with the switch off plus the kernel's own gradient, one fp32 addition per element."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics, pair_swap
from oracle import models as omodels
from oracle.graph import Node
from tests.synth import appflow_feeds, car_like_batch
from tests.test_gpu_flow_smooth_model import _rel_l2, _state_bits
from tests.test_gpu_model import _activation_pattern_override, _perturb_biases, _sampling_cell_override

pytestmark = pytest.mark.gpu

WEIGHT, EPS = 0.5, 1e-3
BASE = {'batch_size': 4, 'learning_rate': 1e-4, 'pair_swap': True}
ON = {'flow_consistency_weight': WEIGHT}


def _feeds(seed):
    """Two synthetic pairs and their reverses: the layout conf['pair_swap'] gives every batch."""
    rng = np.random.default_rng(seed)
    rec = appflow_feeds(rng, 2)
    rec['depth_image0'], rec['depth_image1'] = car_like_batch(rng, 2, 128, 1), car_like_batch(rng, 2, 128, 1)
    return pair_swap.mirror_host(rec)


def _appflow(**extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return AppearanceFlowModel(dict(BASE, **extra), load_tfrec=False, device='cuda')


def _with_terms(builder, captured, smooth=0.0, multiscale=0):
    """The oracle builder with WEIGHT * C(out['flow_field']) added to its loss, and optionally the smoothness and multi-scale terms
    the model adds in front of it: values and gradients come from the float64 numpy twins through the tape's recording hook."""
    def build(t, n):
        out = builder(t, n)
        f = out['flow_field']
        captured['flow'] = f

        def add(loss, grad):
            y = Node(np.asarray(loss, dtype=t.dtype))
            t._rec([y], lambda: f.acc((grad * float(y.g)).astype(t.dtype)))
            out['loss'] = t.add(out['loss'], y)
        if smooth:
            add(*metrics.flow_smoothness_host(f.v, n['image1'].v, 10.0, 1e-3, np.float64, smooth))
        if multiscale:
            value, grad, _ = metrics.multiscale_warp_loss_host(n['image0'].v, f.v, n['image1'].v, multiscale, None, 2, np.float64)
            add(value, grad)
        loss, grad, _, share = metrics.flow_consistency_host(_at_device_cells(f.v, captured), EPS, np.float64, WEIGHT)
        captured['term'], captured['share'] = float(loss), float(share)
        add(loss, grad)
        return out
    return build


def _coords(flow):
    """(flow[..., 0] + row, flow[..., 1] + column) in the flow's own dtype: the term's and the sampler's coordinates.  The device
    forms them in float32, where a flow of -1e-9 at row 5 gives exactly 5."""
    n, h, w, _ = flow.shape
    ii, jj = np.meshgrid(np.arange(h, dtype=flow.dtype), np.arange(w, dtype=flow.dtype), indexing='ij')
    return flow + np.stack([ii, jj], axis=-1)[None]


def _at_device_cells(flow, captured):
    """The rule of tests/test_gpu_model.py's _sampling_cell_override for the term's own sampler, whose coordinates are the warp
    points of the model's sampler: the warp gradient jumps where a coordinate crosses an integer, so for the pixels whose cell
    differs between device and oracle the twin is evaluated at the device's flow.  The flows themselves must agree to 1e-4 of their
    range, and only a handful of pixels may sit that close to an integer."""
    dev = captured.get('device_flow')
    if dev is None:
        return flow
    assert np.abs(dev - flow).max() <= 1e-4 * max(np.abs(flow).max(), 1.0)
    dev_xy, xy = _coords(dev).astype(np.float64), _coords(flow)
    diff = (np.floor(dev_xy) != np.floor(xy)).any(axis=-1, keepdims=True)
    captured['term_cells_moved'] = int(diff.sum())
    assert captured['term_cells_moved'] <= 4 + 1e-3 * diff.size, captured['term_cells_moved']
    return np.where(diff, flow + (dev_xy - xy), flow)                    # the flow that puts the float64 coordinate where the device's is


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
        captured['device_flow'] = model.flow_field.numpy()                  # float32: the coordinates are formed as the device forms them
        out, grads, tape = run(sign_override=override, warp_override=woverride)
    loss, want = float(g.loss_buf[0]), float(out['loss'])
    flow_err = _rel_l2(model.flow_field.grad_value().cpu().numpy(), captured['flow'].g)
    print('%s: loss %.8f oracle %.8f (of which consistency term %.6f, valid share %.3f); flow gradient rel L2 %.2e; kink overrides: '
          '%d signs, %d cells, %d cells of the term' % (label, loss, want, captured['term'], captured['share'], flow_err, flips, moved,
                                                        captured.get('term_cells_moved', 0)))
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


def _flow_gradient_is_the_sum(model_on, variables, feeds, label):
    """Same variables and feeds in the model with a weight of 0 give the flow gradient of everything else; the kernel alone (store)
    gives the term's; the model with the switch on must hold their fp32 sum, element for element."""
    off = type(model_on)(dict(model_on.conf, flow_consistency_weight=0.0), load_tfrec=False, device='cuda')
    off.graph.set_variables(variables)
    off.feed(**feeds)
    off.graph.run_forward()
    off.graph.run_backward()
    torch.cuda.synchronize()
    assert np.array_equal(model_on.flow_field.numpy(), off.flow_field.numpy()), label
    own = torch.zeros(model_on.flow_field.shape, dtype=torch.float32, device='cuda')
    metrics.flow_consistency(model_on.flow_field, EPS, WEIGHT, grad=own)
    want = off.flow_field.grad_value() + own
    assert own.abs().max() > 0
    assert np.array_equal(model_on.flow_field.grad_value().cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), label


@pytest.mark.parametrize("schedule", ['fused', 'unfused', 'with-smoothness-and-multiscale'])
def test_loss_and_gradients_match_the_float64_oracle_with_the_term_added(schedule, monkeypatch):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    if schedule == 'unfused':
        monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    others = schedule == 'with-smoothness-and-multiscale'
    extra = {'flow_smoothness_weight': 0.2, 'multiscale_loss_levels': 2} if others else {}
    model = _appflow(**dict(ON, **extra))
    fused = [n.fused_loss is not None for n in model.graph.nodes if isinstance(n, ResampleNode)]
    assert fused == [schedule != 'unfused']
    captured = {}
    builder = _with_terms(omodels.appearance_flow_builder('base'), captured, smooth=0.2 if others else 0.0, multiscale=2 if others else 0)
    feeds = _feeds(3)
    variables = _against_oracle(model, builder, captured, feeds, schedule)
    _flow_gradient_is_the_sum(model, variables, feeds, schedule)


def _steps(conf, feeds, count=3):
    model = _appflow(**conf)
    start = model.graph.get_variables()
    losses = [model.train_step(**feeds).clone()] + [model.train_step().clone() for _ in range(count - 1)]
    return model, start, torch.stack(losses).cpu().numpy(), _state_bits(model)


class _OneBatch:
    def __init__(self, feeds):
        self.feeds = feeds

    def next(self):
        return self.feeds


def test_train_steps_are_finite_move_every_variable_repeat_bit_for_bit_and_evaluate_reports_the_term():
    feeds = _feeds(6)
    model, start, losses, state = _steps(ON, feeds)
    print('losses with the consistency term:', losses)
    assert np.all(np.isfinite(losses)) and np.all(losses > 0)
    end = model.graph.get_variables()
    assert set(end) == set(model.t_vars)
    for k in end:
        assert np.all(np.isfinite(end[k])) and not np.array_equal(end[k], start[k]), k
    _, _, losses2, state2 = _steps(ON, feeds)
    assert losses.tobytes() == losses2.tobytes()
    assert state.keys() == state2.keys()
    for k in state:
        assert state[k].tobytes() == state2[k].tobytes(), k

    # evaluate() on that model, one batch: the two names are the unweighted twin on the downloaded flow, by the kernel tests' rule
    res = model.evaluate(_OneBatch(feeds), 1)
    flow = model.flow_field.numpy()
    _, _, c64, s64 = metrics.flow_consistency_host(flow, EPS, np.float64)
    _, _, c32, s32 = metrics.flow_consistency_host(flow, EPS, np.float32)
    gen, tgt = model.gen.numpy().astype(np.float64), feeds['image1'].astype(np.float64)
    l2 = ((gen - tgt) ** 2).sum(axis=3).mean()
    print('evaluate: flow/consistency %.9g twin %.9g (float32 twin off by %.2e); valid %.6f twin %.6f; loss %.8f = L2 %.8f + %.1f * C'
          % (res['flow/consistency'], c64, abs(float(c32) - float(c64)), res['flow/consistency_valid'], s64, res['loss'], l2, WEIGHT))
    assert abs(res['flow/consistency'] - float(c64)) <= 4 * abs(float(c32) - float(c64))
    assert res['flow/consistency_valid'] == float(np.float32(s64)) == float(s32)
    assert abs(res['loss'] - (l2 + WEIGHT * float(c64))) <= 1e-5 * max(1.0, res['loss'])


def test_weight_zero_is_the_model_without_the_key():
    feeds = _feeds(8)
    res = []
    for extra in ({}, {'flow_consistency_weight': 0.0}, {'flow_consistency_weight': None, 'flow_consistency_eps': 0.5}):
        model = _appflow(**extra)
        loss = model.train_step(**feeds)
        res.append((loss.cpu().numpy().tobytes(), _state_bits(model)))
        assert not any('consistency' in k for k in model.evaluate(_OneBatch(feeds), 1))
    for l1, s1 in res[1:]:
        assert res[0][0] == l1 and res[0][1].keys() == s1.keys()
        for k in s1:
            assert res[0][1][k].tobytes() == s1[k].tobytes(), k
