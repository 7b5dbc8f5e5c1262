"""conf['occlusion_mask_image_terms'] through AppearanceFlowModel on the GPU, in the manner of
tests/test_gpu_flow_occlusion_model.py: B = 2 at 128 x 128, one synthetic pair and its reverse, the flow head scaled until the
occlusion mask is mixed.

The step's loss is the head term plus the weighted masked SSIM and census terms.  The two masked terms are recomputed through
metrics.ssim_loss / metrics.census_loss(..., mask=model.occlusion_mask()) on the tensors the step left behind, and held to the
float64 twins by the parity rule of tests/test_gpu_masked_census_loss.py (4 x the float32 twin's own gap, floor 2e-6).  The head
term is the float64 masked L2 of the same tensors, which tests/test_gpu_flow_occlusion_model.py holds the device to within 2e-5
relative.  The loss word is the fp32 sum of the three, so it may differ from the float64 sum of the recomputed terms by 2e-5 of the
head term, 2e-6 per masked term (their floor) and 3 roundings of the total (3 x 6e-8 relative)."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics
from tests import masked_image_cases as MC
from tests.test_gpu_flow_occlusion_model import ON, _OneBatch, _appflow, _feeds, _labels, _scaled_head
from tests.test_gpu_flow_smooth_model import _state_bits

pytestmark = pytest.mark.gpu

KEY = 'occlusion_mask_image_terms'
WS, WC, RADIUS, EPS = 0.25, 0.5, 3, 0.01
TERMS = dict(ssim_loss_weight=WS, census_loss_weight=WC)
MASKED = dict(ON, **TERMS, **{KEY: True})


def test_the_step_loss_is_the_head_term_plus_the_weighted_masked_terms():
    feeds = _feeds(3)
    model = _appflow(**MASKED)
    fwd = _labels(model)[0]
    assert fwd[-7:] == ['resample_fwd', 'occl_mask', 'pixel_loss', 'ssim_loss_masked_tile', 'ssim_loss_masked_final', 'census_loss_masked_tile',
                        'census_loss_masked_final']
    _scaled_head(model, feeds)
    loss = float(model.train_step(**feeds))
    mask = model.occlusion_mask()
    m = mask.cpu().numpy()
    visible = float(m.mean())
    assert set(np.unique(m)) == {0.0, 1.0} and 0.2 < visible < 0.8                        # mixed
    gen, tgt = model.gen.numpy(), feeds['image1']

    # the masked terms through the device mirrors, weighted as the step weighs them, and unweighted against the twins
    ssim_w = float(metrics.ssim_loss(model.gen, model.image1, 1.0, WS, mask=mask))
    census_w = float(metrics.census_loss(model.gen, model.image1, 1.0, WC, RADIUS, EPS, mask=mask))
    ssim_m = float(metrics.ssim_loss(model.gen, model.image1, 1.0, 1.0, mask=mask))
    census_m = float(metrics.census_loss(model.gen, model.image1, 1.0, 1.0, RADIUS, EPS, mask=mask))
    ssim_u, census_u = float(metrics.ssim_loss(model.gen, model.image1, 1.0)), float(metrics.census_loss(model.gen, model.image1, 1.0, 1.0, RADIUS, EPS))
    for name, got, twin in (('ssim', ssim_m, lambda dt: metrics.ssim_loss_host(gen, tgt, 1.0, dt, 1.0, mask=m)),
                            ('census', census_m, lambda dt: metrics.census_loss_host(gen, tgt, 1.0, dt, 1.0, RADIUS, EPS, mask=m))):
        (l64, g64), (l32, g32) = twin(np.float64), twin(np.float32)
        allowed = MC.allowed(float(l64), g64, float(l32), g32, False)[0]
        print('%s masked term %.8f float64 twin %.8f err %.2e allowed %.2e' % (name, got, float(l64), abs(got - float(l64)), allowed))
        assert abs(got - float(l64)) <= allowed
    print('visible %.3f; ssim masked %.6f unmasked %.6f; census masked %.6f unmasked %.6f' % (visible, ssim_m, ssim_u, census_m, census_u))
    assert 0 < ssim_m < ssim_u and 0 < census_m < census_u                                # the mask takes a real part of both terms away

    head = float((((gen.astype(np.float64) - tgt) * m) ** 2).sum(axis=3).mean())
    want = head + ssim_w + census_w
    allowed = 2e-5 * head + 2 * 2e-6 + 3 * 6e-8 * want
    print('step loss %.9g; head %.9g + %.2f ssim %.9g + %.2f census %.9g = %.9g; err %.2e allowed %.2e'
          % (loss, head, WS, ssim_w, WC, census_w, want, abs(loss - want), allowed))
    assert abs(loss - want) <= allowed
    assert ssim_w + census_w > 100 * allowed                                              # the terms are far above what the bound forgives

    # evaluate(): the unmasked figures stay, the masked rows are the terms as trained
    res = model.evaluate(_OneBatch(feeds), 1)
    mask = model.occlusion_mask()
    assert list(res)[-3:] == ['image/ssim_loss_masked', 'image/census_masked', 'images']
    assert res['image/census_masked'] == float(metrics.census_loss(model.gen, model.image1, 1.0, 1.0, RADIUS, EPS, mask=mask))
    assert res['image/ssim_loss_masked'] == float(metrics.ssim_loss(model.gen, model.image1, 1.0, 1.0, mask=mask))
    assert res['image/census'] == float(metrics.census_loss(model.gen, model.image1, 1.0, 1.0, RADIUS, EPS))
    assert 0 < res['image/census_masked'] < res['image/census'] and 0 < res['image/ssim_loss_masked'] < 1 - res['image/ssim'] + 1e-6


def test_two_identical_models_give_identical_state_bits_after_a_step():
    feeds = _feeds(6)
    runs = []
    for _ in range(2):
        model = _appflow(**MASKED)
        start = model.graph.get_variables()
        losses = torch.stack([model.train_step(**feeds).clone(), model.train_step().clone()]).cpu().numpy()
        end = model.graph.get_variables()
        assert np.all(np.isfinite(losses)) and np.all(losses > 0)
        for k in end:
            assert np.all(np.isfinite(end[k])) and not np.array_equal(end[k], start[k]), k
        runs.append((losses.tobytes(), _state_bits(model)))
        del model
    assert runs[0][0] == runs[1][0] and runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k


def test_key_absent_none_or_false_is_the_model_without_it():
    feeds = _feeds(8)
    for base in (dict(TERMS), dict(ON)):
        res = []
        for extra in ({}, {KEY: None}, {KEY: False}):
            model = _appflow(**dict(base, **extra))
            loss = model.train_step(**feeds)
            res.append((loss.cpu().numpy().tobytes(), _state_bits(model), _labels(model), model.graph.activation_bytes))
            assert not hasattr(model, 'masked_image_terms')
            assert not any(l.endswith(('_masked_tile', '_masked_final')) for plan in res[-1][2] if plan for l in plan)
            del model
        for l1, s1, p1, a1 in res[1:]:
            assert res[0][0] == l1 and res[0][1].keys() == s1.keys() and res[0][2] == p1 and res[0][3] == a1
            for k in s1:
                assert res[0][1][k].tobytes() == s1[k].tobytes(), k
    for combo in (dict(ssim_loss_weight=0.2), dict(census_loss_weight=0.2)):                  # ... and still refuses what it refused
        with pytest.raises(ValueError, match='occlusion_mask'):
            _appflow(**dict(ON, **combo))
