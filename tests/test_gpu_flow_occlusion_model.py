"""conf['occlusion_mask'] with conf['pair_swap'] through AppearanceFlowModel on the GPU, in the manner of
tests/test_gpu_flow_consist_model.py.  The decoder fixes the flow at 128 x 128, so the class does not allow a smaller image: B = 2 at
128 x 128, one synthetic pair and its reverse.

The flow head of an untrained model gives flows of a small fraction of a pixel, for which every pixel is visible.  The head's
filter is therefore scaled (the head has no bias, so the flow is linear in it) until the median |r|^2 of the inside pixels sits at alpha2: the
coordinates are generic and the mask is mixed, which is asserted from the float64 twin.

Loss and every gradient, for the fused head and for MV3D_FUSE_RESAMPLE=0, against the float64 oracle graph of the same model whose
loss is replaced from the test side by the masked L2 with the mask held constant.  The mask is the device's own, which must equal
the float32 twin on the device's flow at every pixel and the float64 twin everywhere but at pixels within 1e-4 (relative) of the
threshold.  Bars as in that file: relative L2 at most 1e-3 per variable and for the flow gradient, the loss to 2e-5; measured
values are printed.  Decisions at the kinks of lrelu / floor follow the device, by the overrides of tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics, pair_swap
from oracle import models as omodels
from oracle.graph import Node
from tests.synth import appflow_feeds, car_like_batch
from tests.test_gpu_flow_smooth_model import _rel_l2, _state_bits
from tests.test_gpu_model import _activation_pattern_override, _perturb_biases, _sampling_cell_override

pytestmark = pytest.mark.gpu

BASE = {'batch_size': 2, 'learning_rate': 1e-4, 'pair_swap': True}
ON = {'occlusion_mask': True}
A1, A2 = 0.01, 0.5


def _feeds(seed):
    """One synthetic pair and its reverse: the layout conf['pair_swap'] gives every batch."""
    rng = np.random.default_rng(seed)
    rec = appflow_feeds(rng, 1)
    rec['depth_image0'], rec['depth_image1'] = car_like_batch(rng, 1, 128, 1), car_like_batch(rng, 1, 128, 1)
    return pair_swap.mirror_host(rec)


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict(BASE, **extra), load_tfrec=False, device='cuda')


def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _scaled_head(model, feeds):
    """Variables with perturbed biases and a flow head scaled so that the mask is mixed; returns them (they are set on the model)."""
    g = model.graph
    variables = _perturb_biases(g)
    for _ in range(3):
        model.feed(**feeds)
        g.run_forward()
        torch.cuda.synchronize()
        _, _, (lhs, _, inside) = metrics.flow_occlusion_mask_host(model.flow_field.numpy(), A1, A2, True, np.float64, details=True)
        c = np.float32(np.sqrt(A2 / np.median(lhs[inside])))
        variables['flow_field/w'] = variables['flow_field/w'] * c          # the head has no bias: the flow is linear in its filter
        g.set_variables(variables)
    return variables


def _twins(flow):
    """(float32 twin mask, float64 twin mask, shares, smallest relative margin of a pixel where the two differ or 1)."""
    m32, s32 = metrics.flow_occlusion_mask_host(flow, A1, A2, True, np.float32)
    m64, s64, (lhs, rhs, inside) = metrics.flow_occlusion_mask_host(flow, A1, A2, True, np.float64, details=True)
    diff = m32.astype(np.float64) != m64
    rel = np.abs(lhs - rhs) / np.maximum(lhs, rhs)
    return m32, m64, s64, (float(rel[diff].max()) if diff.any() else 0.0), int(diff.sum())


def _masked_loss(builder, mask, captured):
    """The oracle builder with its loss replaced by mean_{n,h,w} sum_c ((gen - image1) mask)^2, the mask a constant."""
    m = np.asarray(mask, np.float64)[..., None]

    def build(t, n):
        out = builder(t, n)
        captured['flow'] = out['flow_field']
        gen, tgt = out['gen'], n['image1']
        d = (gen.v - tgt.v) * m
        npix = float(np.prod(m.shape))
        y = Node(np.asarray((d * d).sum() / npix, dtype=t.dtype))
        t._rec([y], lambda: gen.acc((d * m * (2.0 / npix) * float(y.g)).astype(t.dtype)))
        out['loss'] = y
        return out
    return build


def _run_device(model, variables, feeds):
    g = model.graph
    g.set_variables(variables)
    model.feed(**feeds)
    g.run_forward()
    g.run_backward()
    torch.cuda.synchronize()


def test_loss_and_gradients_match_the_float64_oracle_for_both_schedules(monkeypatch):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    feeds = _feeds(3)
    fused = _appflow(**ON)
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    unfused = _appflow(**ON)
    monkeypatch.delenv('MV3D_FUSE_RESAMPLE')
    for m, want in ((fused, True), (unfused, False)):
        (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
        assert (node.fused_loss is not None) == want and (node.fused_occlusion is not None) == want
    assert 'occl_head_tile' in _labels(fused)[0] and 'occl_mask' in _labels(unfused)[0] and 'occl_head_tile' not in _labels(unfused)[0]
    variables = _scaled_head(fused, feeds)
    _run_device(fused, variables, feeds)
    _run_device(unfused, variables, feeds)

    # the mask: the device's equals the float32 twin on the device's flow, and the float64 twin but for pixels at the threshold
    flow = fused.flow_field.numpy()
    mask = fused.occlusion_mask().cpu().numpy()[..., 0]
    m32, m64, shares, margin, differ = _twins(flow)
    print('mask: visible %.3f occluded %.3f outside %.3f; float32 and float64 twins differ at %d pixels (largest margin there %.1e); '
          'flow rms %.3f max %.3f' % (shares + (differ, margin, float(np.sqrt((flow ** 2).mean())), float(np.abs(flow).max()))))
    assert 0.2 < shares[0] < 0.8 and shares[1] > 0.1                       # mixed
    assert np.array_equal(mask, m32) and margin < 1e-4 and differ <= 4
    x = flow[..., 0] + np.arange(128, dtype=np.float32)[None, :, None]
    assert np.mean(np.abs(x - np.rint(x)) > 1e-3) > 0.99                   # generic coordinates

    # the two schedules against each other: everything in front of the head is the same launch list
    assert np.array_equal(unfused.flow_field.numpy(), flow) and np.array_equal(unfused.occlusion_mask().cpu().numpy()[..., 0], mask)
    assert np.array_equal(unfused.gen.numpy().view(np.uint32), fused.gen.numpy().view(np.uint32))
    gf, gu = fused.flow_field.grad_value().cpu().numpy(), unfused.flow_field.grad_value().cpu().numpy()
    assert np.array_equal(gf.view(np.uint32), gu.view(np.uint32)) and np.abs(gf).max() > 0
    lf, lu = float(fused.graph.loss_buf[0]), float(unfused.graph.loss_buf[0])
    print('loss fused %.9g unfused %.9g (rel %.2e)' % (lf, lu, abs(lf - lu) / lu))
    assert abs(lf - lu) <= 3e-6 * lu

    # the oracle, with the device's mask held constant
    captured = {}
    builder = _masked_loss(omodels.appearance_flow_builder('base'), mask, captured)
    run = lambda **kw: omodels.run(builder, {k: v.copy() for k, v in variables.items()}, feeds, dtype=np.float64, **kw)
    out, grads, tape = run()
    override, flips = _activation_pattern_override(fused, tape)
    woverride, moved = _sampling_cell_override(fused, tape)
    if flips or moved:
        out, grads, tape = run(sign_override=override, warp_override=woverride)
    want = float(out['loss'])
    plain = float(((fused.gen.numpy().astype(np.float64) - feeds['image1']) ** 2).sum(axis=3).mean())
    print('oracle loss %.9g (unmasked L2 of the same images %.9g); kink overrides: %d signs, %d cells' % (want, plain, flips, moved))
    assert want < 0.95 * plain                                             # the mask takes a real part of the loss away
    assert _rel_l2(flow, out['flow_field']) <= 1e-4
    flow_err = _rel_l2(gf, captured['flow'].g)
    print('flow gradient rel L2 %.2e (largest element %.3e, %d of %d elements exactly 0)'
          % (flow_err, np.abs(gf).max(), int(np.count_nonzero(gf == 0)), gf.size))
    assert flow_err <= 1e-3
    assert not np.any(gf[mask == 0])                                       # an occluded pixel pulls nothing
    for label, m in (('fused', fused), ('unfused', unfused)):
        loss = float(m.graph.loss_buf[0])
        got = m.graph.get_gradients()
        assert set(got) == set(grads)
        errs = {k: _rel_l2(got[k], grads[k]) for k in grads}
        worst = max(errs, key=errs.get)
        print('%s: loss %.9g oracle %.9g; %d variables, worst relative L2 %.2e (%s), flow_field/w %.2e, median %.2e'
              % (label, loss, want, len(errs), errs[worst], worst, errs['flow_field/w'], np.median(list(errs.values()))))
        assert abs(loss - want) <= 2e-5 * abs(want)
        assert errs[worst] <= 1e-3, (label, worst, errs[worst])


class _OneBatch:
    def __init__(self, feeds):
        self.feeds = feeds

    def next(self):
        return self.feeds


def _steps(conf, feeds, variables=None, count=3):
    model = _appflow(**conf)
    if variables is not None:
        model.graph.set_variables(variables)
    start = model.graph.get_variables()
    losses = [model.train_step(**feeds).clone()] + [model.train_step().clone() for _ in range(count - 1)]
    return model, start, torch.stack(losses).cpu().numpy(), _state_bits(model)


def test_train_steps_repeat_bit_for_bit_and_evaluate_and_the_accessor_report_the_mask():
    from dynamic_multiview_3d_amd.train import training_log_row
    feeds = _feeds(6)
    variables = _scaled_head(_appflow(**ON), feeds)
    model, start, losses, state = _steps(ON, feeds, variables)
    print('losses with the occlusion mask:', losses)
    assert np.all(np.isfinite(losses)) and np.all(losses > 0)
    end = model.graph.get_variables()
    for k in end:
        assert np.all(np.isfinite(end[k])) and not np.array_equal(end[k], start[k]), k
    _, _, losses2, state2 = _steps(ON, feeds, variables)
    assert losses.tobytes() == losses2.tobytes() and state.keys() == state2.keys()
    for k in state:
        assert state[k].tobytes() == state2[k].tobytes(), k

    # the log row reads the mask of the step that has just run; evaluate() one batch; the accessor holds that batch's mask
    row = training_log_row(model, 10, float(losses[-1]))
    m32, _, shares, _, _ = _twins(model.flow_field.numpy())
    assert row['flow_visible'] == float(np.float32(np.count_nonzero((m32 == 1) & _inside(model.flow_field.numpy())) / m32.size))
    res = model.evaluate(_OneBatch(feeds), 1)
    flow = model.flow_field.numpy()
    m32, m64, shares, margin, differ = _twins(flow)
    inside = _inside(flow)
    counts = [np.count_nonzero((m32 == 1) & inside), np.count_nonzero((m32 == 0) & inside), np.count_nonzero(~inside)]
    got = [res['flow/visible'], res['flow/occluded'], res['flow/outside']]
    print('evaluate: shares %s; float64 twin %s (%d pixels at the threshold)' % (got, shares, differ))
    assert got == [float(np.float32(c / float(m32.size))) for c in counts]
    assert abs(sum(got) - 1.0) < 1e-6 and min(got[:2]) > 0
    assert np.array_equal(model.occlusion_mask().cpu().numpy()[..., 0], m32) and differ <= 4 and margin < 1e-4
    gen, tgt = model.gen.numpy().astype(np.float64), feeds['image1'].astype(np.float64)
    l2 = (((gen - tgt) * m32[..., None]) ** 2).sum(axis=3).mean()
    assert abs(res['loss'] - l2) <= 1e-5 * max(1.0, l2)


def _inside(flow):
    return metrics.flow_occlusion_mask_host(flow, A1, A2, True, np.float32, details=True)[2][2]


def test_switch_off_is_the_model_without_the_key():
    feeds = _feeds(8)
    res = []
    for extra in ({}, {'occlusion_mask': False}, {'occlusion_mask': None, 'occlusion_alpha2': 2.0, 'occlusion_outside': 'mask'}):
        model = _appflow(**extra)
        loss = model.train_step(**feeds)
        res.append((loss.cpu().numpy().tobytes(), _state_bits(model), _labels(model), model.graph.activation_bytes))
        assert not any(k.endswith(('/visible', '/occluded', '/outside')) for k in model.evaluate(_OneBatch(feeds), 1))
        assert not hasattr(model, 'occlusion_terms')
    for l1, s1, p1, a1 in res[1:]:
        assert res[0][0] == l1 and res[0][1].keys() == s1.keys() and res[0][2] == p1 and res[0][3] == a1
        for k in s1:
            assert res[0][1][k].tobytes() == s1[k].tobytes(), k


def test_unsupported_classes_and_combinations_raise():
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    on = dict(BASE, **ON)
    with pytest.raises(ValueError, match='pair_swap'):
        _appflow(occlusion_mask=True, pair_swap=False)
    for combo in (dict(ssim_loss_weight=0.2), dict(census_loss_weight=0.2), dict(multiscale_loss_levels=2), dict(occlusion_alpha2=0.0),
                  dict(occlusion_alpha1=float('nan')), dict(occlusion_outside='drop'), dict(occlusion_mask=1)):
        with pytest.raises(ValueError, match='occlusion'):
            _appflow(**dict(ON, **combo))
    bp = dict(on, use_color='', use_depth='', depth_lr_factor=0.1)
    with pytest.raises(ValueError, match='occlusion_mask'):
        Base_Prediction_Model(bp, load_tfrec=False, device='cuda')
    with pytest.raises(ValueError):
        mv3d.mv3d_nobg_nodm(dict(on), device='cuda')
    # the family takes it, with the fused head
    assert _labels(_appflow(AppearanceFlowTinghui, **ON))[0][-2:] == ['occl_head_tile', 'occl_head_final']
