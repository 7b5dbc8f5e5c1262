"""conf['occlusion_mask_multiscale'] through AppearanceFlowModel on the GPU, in the manner of tests/test_gpu_flow_occlusion_model.py
and tests/test_gpu_multiscale_model.py: B = 4 at 128 x 128, two synthetic pairs and their reverses, the flow head scaled until the
mask is mixed.

The step's loss word is built by fp32 additions, one per term, in launch order: the head stores, the multi-scale term adds.  So the
loss with the key on must be the loss of the same model without the multi-scale term plus the kernel's own value, one fp32
addition, bit for bit; the kernel's value and gradient on the step's flow and mask are held to the float64 masked twin by
tests/multiscale_cases.within_rule, and the difference of the two loss words to the twin's value by that rule's value bound.  The
flow gradient of the fused step (one tiled head launch that writes the mask, the multi-scale launches behind it) must equal the
MV3D_FUSE_RESAMPLE=0 step's bit for bit.  Every figure is printed before it is asserted."""
import json
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics, pair_swap
from tests import multiscale_cases as MC
from tests.synth import appflow_feeds, car_like_batch
from tests.test_gpu_flow_occlusion_model import _labels, _scaled_head

pytestmark = pytest.mark.gpu

BASE = {'batch_size': 4, 'learning_rate': 1e-4, 'pair_swap': True}
WEIGHTS = [1.0, 0.5, 0.25]
OCCL = {'occlusion_mask': True}
ON = dict(OCCL, multiscale_loss_levels=3, multiscale_loss_weight=WEIGHTS, occlusion_mask_multiscale=True)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'appflow_plan_labels_b4.json')


def _feeds(seed):
    """Two synthetic pairs and their reverses: the layout conf['pair_swap'] gives every batch."""
    rng = np.random.default_rng(seed)
    rec = appflow_feeds(rng, 2)
    rec['depth_image0'], rec['depth_image1'] = car_like_batch(rng, 2, 128, 1), car_like_batch(rng, 2, 128, 1)
    return pair_swap.mirror_host(rec)


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict(BASE, **extra), load_tfrec=False, device='cuda')


def _fwd_bwd(model, feeds, variables):
    model.graph.set_variables(variables)
    model.feed(**feeds)
    model.graph.run_forward()
    model.graph.run_backward()
    torch.cuda.synchronize()
    return model.graph.loss_buf[0].cpu().numpy()


def _twin(flow, src, target, mask, levels=3, weights=WEIGHTS, kind=2):
    """(value64, grad64, levels64, value32, grad32, levels32): the reference tuple of MC.within_rule."""
    out = []
    for dt in (np.float64, np.float32):
        v, g, lv = metrics.multiscale_warp_loss_host(src, flow, target, levels, weights, kind, dt, mask=mask)
        out += [float(v), g, lv]
    return tuple(out)


class _OneBatch:
    def __init__(self, feeds):
        self.feeds = feeds

    def next(self):
        return self.feeds


def test_loss_is_head_plus_masked_term_and_the_fused_step_equals_the_unfused_one(monkeypatch):
    from dynamic_multiview_3d_amd.graph import MultiscaleTerm, OcclusionMaskNode, ResampleNode
    feeds = _feeds(3)
    fused = _appflow(**ON)
    head = _appflow(**OCCL)                                                   # the same model without the multi-scale term
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    unfused = _appflow(**ON)
    monkeypatch.delenv('MV3D_FUSE_RESAMPLE')
    for m, want in ((fused, True), (unfused, False)):
        (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
        (occl,) = [n for n in m.graph.nodes if isinstance(n, OcclusionMaskNode)]
        assert (node.fused_loss is not None) == want and (node.fused_occlusion is occl) == want
        (term,) = [t for _, t in m.graph.loss_expr.terms if isinstance(t, MultiscaleTerm)]
        assert term.mask is occl.mask
    fwd, bwd, _ = _labels(fused)
    assert fwd[-5:] == ['occl_head_tile', 'occl_head_final', 'multiscale_pyramid', 'multiscale_loss_masked_tile', 'multiscale_loss_final']
    assert fwd[:-3] == _labels(head)[0] and bwd == _labels(head)[1]
    ufwd, ubwd, _ = _labels(unfused)
    assert 'occl_mask' in ufwd and 'occl_head_tile' not in ufwd and ufwd[-3:] == fwd[-3:]
    assert sum(l == 'multiscale_loss_masked_tile' for l in ufwd + ubwd) == 2 and (ufwd + ubwd).count('multiscale_pyramid') == 1
    assert not any(l == 'multiscale_loss_tile' for l in fwd + bwd + ufwd + ubwd)

    variables = _scaled_head(fused, feeds)
    l_on, l_head, l_un = (_fwd_bwd(m, feeds, variables) for m in (fused, head, unfused))
    flow, mask = fused.flow_field.numpy(), fused.occlusion_mask().cpu().numpy()
    visible = float(mask.mean())
    print('mask: visible share %.3f; flow rms %.3f' % (visible, float(np.sqrt((flow ** 2).mean()))))
    assert 0.2 < visible < 0.8                                                 # mixed
    for other in (head, unfused):
        assert np.array_equal(other.flow_field.numpy(), flow) and np.array_equal(other.occlusion_mask().cpu().numpy(), mask)

    # the kernel on the step's own flow and mask against the masked twin
    ref = _twin(flow, feeds['image0'], feeds['image1'], mask)
    own = torch.zeros(fused.flow_field.shape, dtype=torch.float32, device='cuda')
    value, _ = metrics.multiscale_warp_loss(fused.image0, fused.flow_field, fused.image1, 3, WEIGHTS, 2, grad=own, mask=fused.occlusion_mask())
    MC.within_rule('the masked term on the model\'s flow', float(value), own.cpu().numpy(), ref)
    plain = float(metrics.multiscale_warp_loss(fused.image0, fused.flow_field, fused.image1, 3, WEIGHTS, 2)[0])
    print('loss on %.8f head %.8f difference %.8f masked twin %.8f (float32 gap %.2e); unmasked term %.8f'
          % (l_on, l_head, float(l_on) - float(l_head), ref[0], abs(ref[3] - ref[0]), plain))
    assert ref[0] > 0.01 * float(l_head) and ref[0] < 0.95 * plain               # a real part of the loss, and the mask takes a real part away
    assert l_on.tobytes() == (l_head + value.cpu().numpy()).astype(np.float32).tobytes()      # one fp32 addition onto the head's word
    assert abs((float(l_on) - float(l_head)) - ref[0]) <= max(4 * abs(ref[3] - ref[0]), 2e-6)

    # the flow gradient: the head's plus the kernel's own, one fp32 addition per element; fused and unfused bit for bit
    gf, gu = fused.flow_field.grad_value().cpu().numpy(), unfused.flow_field.grad_value().cpu().numpy()
    want = (head.flow_field.grad_value() + own).cpu().numpy()
    assert np.abs(own.cpu().numpy()).max() > 0
    assert np.array_equal(gf.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(gf.view(np.uint32), gu.view(np.uint32))
    print('loss fused %.9g unfused %.9g' % (float(l_on), float(l_un)))
    assert abs(float(l_on) - float(l_un)) <= 3e-6 * float(l_un)                   # the unfused head's loss comes from another kernel
    g_on, g_head = fused.graph.get_gradients(), head.graph.get_gradients()
    assert not np.array_equal(g_on['flow_field/w'], g_head['flow_field/w'])


def test_evaluate_reports_the_masked_and_the_unmasked_level_terms():
    feeds = _feeds(7)
    model = _appflow(**ON)
    _scaled_head(model, feeds)
    res = model.evaluate(_OneBatch(feeds), 1)
    flow, mask = model.flow_field.numpy(), model.occlusion_mask().cpu().numpy()
    assert 0.05 < mask.mean() < 0.95
    masked = _twin(flow, feeds['image0'], feeds['image1'], mask)
    plain = _twin(flow, feeds['image0'], feeds['image1'], None)
    for l, key in enumerate(('flow/photo_x2', 'flow/photo_x4', 'flow/photo_x8')):
        for name, ref in ((key, plain), (key + '_masked', masked)):
            gap = abs(float(ref[5][l]) - float(ref[2][l]))
            print('%s %.8f twin %.8f (float32 gap %.2e)' % (name, res[name], ref[2][l], gap))
            assert abs(res[name] - float(ref[2][l])) <= max(4 * gap, 2e-6)
        assert 0 < res[key + '_masked'] < res[key]
    assert list(res)[-4:] == ['flow/photo_x2_masked', 'flow/photo_x4_masked', 'flow/photo_x8_masked', 'images']
    assert not any(k.endswith('_masked') for k in _appflow(**OCCL).evaluate(_OneBatch(feeds), 1))


def test_a_class_of_the_family_builds_and_steps_with_the_key():
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    feeds = _feeds(2)
    model = _appflow(AppearanceFlowTinghui, multiscale_loss_kind='l1', **ON)
    fwd = _labels(model)[0]
    assert fwd[-5:] == ['occl_head_tile', 'occl_head_final', 'multiscale_pyramid', 'multiscale_loss_masked_tile', 'multiscale_loss_final']
    losses = [float(model.train_step(**feeds)), float(model.train_step())]
    print('AppearanceFlowTinghui with the key: losses', losses)
    assert all(np.isfinite(l) and l > 0 for l in losses)


def test_with_the_key_absent_the_recorded_plans_are_the_ones_from_before_the_key():
    """tests/golden/appflow_plan_labels_b4.json holds the plan labels AppearanceFlowModel recorded on the device at B = 4 before
    conf['occlusion_mask_multiscale'] existed: the default conf and the occlusion conf."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    for name, conf, off in (('default', {}, False), ('occlusion', OCCL, None)):
        for key in ({}, {'occlusion_mask_multiscale': off}):
            assert _labels(_appflow(**dict(conf, **key))) == golden[name], (name, key)
