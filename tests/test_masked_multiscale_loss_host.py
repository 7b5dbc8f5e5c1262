"""CPU-side checks of the occlusion-masked multi-scale loss: the numpy twin (metrics.multiscale_warp_loss_host with mask=) against
the unmasked twin, against linearity in the mask and against central differences; the refusals of
mv3d_multiscale_warp_loss_masked (they come before any launch, so they need no device); the graph op;
conf['occlusion_mask_multiscale'] on recorded plans; and evaluate()'s host path.  Cases: tests/masked_multiscale_cases.py."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import masked_multiscale_cases as MM

ON = dict(pair_swap=True, occlusion_mask=True)
KEY = 'occlusion_mask_multiscale'
IMAGE_KEY = 'occlusion_mask_image_terms'
MS_LABELS = ['multiscale_pyramid', 'multiscale_loss_masked_tile', 'multiscale_loss_final']


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()


def _twin(case, family, c, kind, dtype, m):
    src, tgt = MM.images(case)
    return metrics.multiscale_warp_loss_host(src[..., :c], MM.flow(case, family), tgt[..., :c], MM.dims(case)[3], MM.weights(case), kind, dtype,
                                             mask=m)


# ------------------------------------------------------------------------------------------------ numpy twin
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", sorted(MM.SHAPES))
def test_a_mask_of_ones_gives_the_unmasked_twin_bit_for_bit(case, dtype):
    for family in MM.FAMILIES:
        for c in (1, 3):
            for kind in MM.KINDS:
                plain = _twin(case, family, c, kind, dtype, None)
                ones = _twin(case, family, c, kind, dtype, MM.mask(case, 'ones'))
                for a, b in zip(plain, ones):
                    assert a.dtype == b.dtype == np.dtype(dtype) and a.tobytes() == b.tobytes(), (case, family, c, kind)


@pytest.mark.parametrize("case", sorted(MM.SHAPES))
def test_a_mask_of_zeros_gives_exact_zeros(case):
    for dtype in (np.float32, np.float64):
        for family in MM.FAMILIES:
            for kind in MM.KINDS:
                v, g, lv = _twin(case, family, 3, kind, dtype, MM.mask(case, 'zeros'))
                assert float(v) == 0.0 and not np.signbit(v) and not np.any(g) and not np.any(lv), (case, family, kind)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_flow_on_a_transposed_pair_is_exactly_zero_under_any_mask(dtype):
    for side, levels in ((8, 3), (96, 2), (32, 3)):
        a, b = MM.transposed_pair(side)
        for mf in MM.MASKS:
            m = MM.mask_of(mf, 2, side, side, side)
            for kind in MM.KINDS:
                v, g, t = metrics.multiscale_warp_loss_host(a, np.zeros((2, side, side, 2), np.float32), b, levels, None, kind, dtype, mask=m)
                assert v == 0 and not np.any(g) and not np.any(t), (side, mf, kind)
                assert v.dtype == dtype and g.dtype == dtype and t.shape == (levels,)


@pytest.mark.parametrize("case", sorted(MM.SHAPES))
def test_float64_twin_is_linear_in_the_mask(case):
    m1, m2 = MM.mask(case, 'fraction').astype(np.float64), MM.mask(case, 'blocks').astype(np.float64)
    for family in MM.FAMILIES:
        for kind in MM.KINDS:
            v1, g1, t1 = _twin(case, family, 3, kind, np.float64, m1)
            v2, g2, t2 = _twin(case, family, 3, kind, np.float64, m2)
            v12, g12, t12 = _twin(case, family, 3, kind, np.float64, m1 + m2)
            vs, gs, ts = _twin(case, family, 3, kind, np.float64, 2.5 * m1)
            print('%s %s kind %d: |value(m1 + m2) - value(m1) - value(m2)| %.1e, gradient max %.1e'
                  % (case, family, kind, abs(v12 - v1 - v2), np.abs(g12 - g1 - g2).max()))
            assert abs(float(v12) - float(v1) - float(v2)) <= 1e-12 and np.abs(g12 - g1 - g2).max() <= 1e-12
            assert np.abs(t12 - t1 - t2).max() <= 1e-12
            assert abs(float(vs) - 2.5 * float(v1)) <= 1e-12 and np.abs(gs - 2.5 * g1).max() <= 1e-12


@pytest.mark.parametrize("kind", MM.KINDS)
def test_gradient_matches_central_finite_differences(kind):
    """float64 on one3 (every flow element), edge and nonsq (64 elements each, drawn once, plus the four corners).  The bound is 10 x
    what test_gradient_matches_central_finite_differences of tests/test_multiscale_loss_host.py allows for the unmasked twin with
    the same step: 10 * (1e-8 + 1e-6 * largest |grad|).  The mask is a constant factor per coarse pixel, so the twin stays piecewise
    polynomial in the flow and the generator keeps every coordinate 1e-3 from a kink."""
    h = 1e-6
    for case, mf in (('one3', 'fraction'), ('edge', 'blocks'), ('nonsq', 'sparse')):
        src, tgt = MM.images(case)
        levels, flow = MM.dims(case)[3], MM.flow(case, 'random').astype(np.float64)
        m = MM.mask(case, mf)
        value = lambda f: float(metrics.multiscale_warp_loss_host(src, f, tgt, levels, MM.weights(case), kind, mask=m)[0])
        _, g, _ = metrics.multiscale_warp_loss_host(src, flow, tgt, levels, MM.weights(case), kind, mask=m)
        every = list(np.ndindex(flow.shape))
        if case != 'one3':
            n, hh, ww, _ = flow.shape
            rng = np.random.default_rng(5)
            every = [every[k] for k in rng.choice(len(every), 64, replace=False)] + [(0, 0, 0, 0), (n - 1, hh - 1, ww - 1, 1), (0, hh - 1, 0, 1),
                                                                                       (n - 1, 0, ww - 1, 0)]
        worst = 0.0
        for idx in every:
            fp, fm = flow.copy(), flow.copy()
            fp[idx] += h
            fm[idx] -= h
            worst = max(worst, abs((value(fp) - value(fm)) / (2 * h) - g[idx]))
        print('%s %s kind %d: largest |fd - grad| %.2e over %d elements, largest |grad| %.2e' % (case, mf, kind, worst, len(every), np.abs(g).max()))
        assert np.abs(g).max() > 0
        assert worst <= 10 * (1e-8 + 1e-6 * np.abs(g).max())


def test_bad_masks_are_refused():
    src, tgt = MM.images('edge')
    fl, m = MM.flow('edge', 'random'), MM.mask('edge', 'fraction')
    args = (src[..., :3], fl, tgt[..., :3], 3)
    for bad in (m[:, :-8], m[:, :, :-8], np.concatenate([m, m], axis=3), m[:1], m[..., 0], np.ones((2, 40, 24, 3), np.float32)):
        with pytest.raises(ValueError, match='mask'):
            metrics.multiscale_warp_loss_host(*args, mask=bad)
    wide = np.full(m.shape[:3] + (4,), np.nan, np.float32)
    wide[..., 2:3] = m
    want, got = metrics.multiscale_warp_loss_host(*args, mask=m), metrics.multiscale_warp_loss_host(*args, mask=wide[..., 2:3])
    assert want[0] == got[0] and np.array_equal(want[1], got[1])
    z = torch.zeros((2, 40, 24, 3))                                                 # the device mirror: the same refusals, before the device
    f2 = torch.zeros((2, 40, 24, 2))
    for bad in (torch.zeros((2, 40, 24, 2)), torch.zeros((1, 40, 24, 1)), torch.zeros((2, 32, 24, 1)),
                torch.zeros((2, 40, 24, 1), dtype=torch.float64)):
        with pytest.raises(ValueError, match='mask'):
            metrics.multiscale_warp_loss(z, f2, z, 3, mask=bad)


@pytest.mark.parametrize("case", sorted(MM.SHAPES))
def test_float32_masked_twin_stays_inside_the_parity_bar(case):
    """The GPU test lets the kernel differ from the float64 twin by 4 x the float32 twin's own gap (tests/multiscale_cases.within_rule):
    the float32 masked twin itself must pass the rule on every case of that test."""
    for family in MM.FAMILIES:
        for c in MM.channels_of(case):
            for kind in MM.KINDS:
                for mf in MM.PARITY_MASKS:
                    ref = MM.reference(case, family, c, kind, mf)
                    MM.within_rule('%s %s C %d kind %d %s' % (case, family, c, kind, mf), ref[3], ref[4], ref)
                    assert np.abs(ref[5].astype(np.float64) - ref[2]).max() <= 1e-5 * max(ref[2].max(), 1e-30) + 1e-7


# ------------------------------------------------------------------------------------------------ C ABI
OK = dict(N=2, H=16, W=16, Hs=16, Ws=16, C=3, src=0x1000, src_ld=3, flow=0x2000, flow_ld=2, target=0x3000, target_ld=3, mask=0x7000, mask_ld=1,
          levels=2, kind=2, loss=0x4000, lv=0x4100, grad=0x5000, grad_ld=2, acc=0, ready=0, ws=0x6000, ws_bytes=1 << 20)


def _call(lib, stream=None, weights=(1.0, 0.5, 0.25), **kw):
    v = dict(OK, **kw)
    w = (ctypes.c_float * len(weights))(*weights)
    return lib.raw_multiscale_warp_loss_masked(v['N'], v['H'], v['W'], v['Hs'], v['Ws'], v['C'], v['src'], v['src_ld'], v['flow'], v['flow_ld'],
                                               v['target'], v['target_ld'], v['mask'], v['mask_ld'], v['levels'], w, v['kind'], v['loss'], v['lv'],
                                               v['grad'], v['grad_ld'], v['acc'], v['ready'], v['ws'], v['ws_bytes'], stream)


def test_the_entry_is_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    name = 'mv3d_multiscale_warp_loss_masked'
    assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.multiscale_warp_loss_masked) and callable(lib.raw_multiscale_warp_loss_masked)


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns MV3D_E_INVAL (or _WORKSPACE) and names the argument; none touches a pointer, so made-up addresses do."""
    nan = float('nan')
    for kw, code, word in [(dict(mask=None), -1, 'mask is null'), (dict(mask_ld=0), -1, 'mask_ld'), (dict(mask_ld=-1), -1, 'mask_ld'),
                           (dict(mask=0x7002), -1, 'aligned'), (dict(N=0), -1, 'N'), (dict(C=5), -1, 'C'), (dict(levels=4), -1, 'levels'),
                           (dict(H=18), -1, 'H'), (dict(src_ld=2), -1, 'src_ld'), (dict(flow_ld=1), -1, 'flow_ld'), (dict(grad_ld=1), -1, 'grad_ld'),
                           (dict(kind=3), -1, 'kind'), (dict(acc=2), -1, 'grad_accumulate'), (dict(ready=2), -1, 'pyramid_ready'),
                           (dict(src=None), -1, 'src is null'), (dict(loss=None, lv=None, grad=None), -1, 'both null'),
                           (dict(weights=(1.0, nan)), -1, 'level_weights[1]'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(N=4, H=32768, W=32768, mask_ld=1 << 30), -1, 'overflow'),     # 2^62 mask elements; the others fit
                           (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x6008), -3, 'aligned')]:
        assert _call(lib, **kw) == code, kw
        assert word in lib.last_error() and 'mv3d_multiscale_warp_loss_masked' in lib.last_error(), (kw, lib.last_error())
    assert _call(lib, mask_ld=0, kind=3) == -1 and 'mask_ld' in lib.last_error()            # strides before values before pointers
    assert _call(lib, mask=None, ws=None) == -1 and 'mask is null' in lib.last_error()


def test_recorded_calls_carry_the_masked_label_and_bytes(lib):
    """Recording launches nothing, so made-up addresses do: the labels, the same workspace, and the unmasked tile launch's bytes plus
    4 B per flow pixel."""
    n, h, w, c, levels = 2, 40, 24, 3, 3
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, w, h, w, c, levels))
    wts = (ctypes.c_float * 3)(1.0, 0.5, 0.25)
    plans = {}
    for masked in (False, True):
        plan = lib.plan_create()
        lib.plan_begin(plan)
        try:
            if masked:
                assert _call(lib, N=n, H=h, W=w, Hs=h, Ws=w, levels=levels, ws_bytes=nb) == 0
                assert _call(lib, N=n, H=h, W=w, Hs=h, Ws=w, levels=levels, ws_bytes=nb, loss=None, lv=None, ready=1, acc=1) == 0
            else:
                lib.multiscale_warp_loss(n, h, w, h, w, c, 0x1000, 3, 0x2000, 2, 0x3000, 3, levels, wts, 2, 0x4000, 0x4100, 0x5000, 2, 0, 0, 0x6000,
                                         nb, None)
                lib.multiscale_warp_loss(n, h, w, h, w, c, 0x1000, 3, 0x2000, 2, 0x3000, 3, levels, wts, 2, None, None, 0x5000, 2, 1, 1, 0x6000,
                                         nb, None)
        finally:
            lib.plan_end()
        plans[masked] = _lib.plan_ops(plan)
        lib.plan_destroy(plan)
    assert [o[0] for o in plans[False]] == ['multiscale_pyramid', 'multiscale_loss_tile', 'multiscale_loss_final', 'multiscale_loss_tile']
    assert [o[0] for o in plans[True]] == MS_LABELS + ['multiscale_loss_masked_tile']          # the reverse-pass call: the tile launch alone
    for k in (0, 2):
        assert plans[True][k][1:3] == plans[False][k][1:3]
    for k in (1, 3):
        assert plans[True][k][1] == plans[False][k][1] and plans[True][k][2] == plans[False][k][2] + n * h * w * 4.0
    assert _call(lib, N=n, H=h, W=w, Hs=h, Ws=w, levels=levels, ws_bytes=nb - 1) == -3          # the same workspace size function


# ------------------------------------------------------------------------------------------------ graph op
def test_the_op_takes_a_constant_one_channel_mask_and_refuses_everything_else(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, LOSS_MULTISCALE, MultiscaleTerm
    with Graph(device='cpu') as g:
        img, tgt = g.placeholder([2, 16, 16, 3], 'img'), g.placeholder([2, 16, 16, 3], 'tgt')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'f')                                   # differentiated
        m = g.placeholder([2, 16, 16, 1], 'm')
        m3, small, other_n = g.placeholder([2, 16, 16, 3], 'm3'), g.placeholder([2, 8, 16, 1], 'small'), g.placeholder([4, 16, 16, 1], 'n4')
        learned = tf_utils.conv2d_msra(tgt, 1, 3, 3, 1, 1, 'm')                                  # requires a gradient
        (w, t), = tf_utils.multiscale_photometric_loss(flow, img, tgt, 2, [1.0, 0.5], 'l1', mask=m).terms
        assert isinstance(t, MultiscaleTerm) and (w, t.kind, t.a, t.b, t.src, t.mask, t.levels) == (1.0, LOSS_MULTISCALE, flow, tgt, img, m, 2)
        plain = tf_utils.multiscale_photometric_loss(flow, img, tgt, 2).terms[0][1]
        assert plain.mask is None and plain.workspace_bytes(lib) == t.workspace_bytes(lib) > 0
        for bad in (m3, small, other_n, learned, np.ones((2, 16, 16, 1), np.float32), 1.0):
            with pytest.raises(ValueError, match='mask'):
                tf_utils.multiscale_photometric_loss(flow, img, tgt, 2, mask=bad)
        with pytest.raises(NotImplementedError):
            tf_utils.multiscale_photometric_loss(flow, img, tgt, 2, mask=tf_utils.multiply(m, m))
        with pytest.raises(NotImplementedError):
            tf_utils.multiscale_photometric_loss(flow, img, tgt, 2, mask=tf_utils.scale(m, 0.5))
        with pytest.raises(NotImplementedError):
            tf_utils.multiscale_photometric_loss(flow, tf_utils.multiply(img, m), tgt, 2, mask=m)


# ------------------------------------------------------------------------------------------------ conf and recorded plans
def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


_SUMMARIES = {}


def _summary(**extra):
    """(labels, tensor count, activation bytes) of a model that is dropped at once (a CPU model holds over a gigabyte); computed once
    per conf."""
    key = repr(sorted(extra.items()))
    if key not in _SUMMARIES:
        m = _appflow(**extra)
        _SUMMARIES[key] = (_labels(m), len(m.graph.tensors), m.graph.activation_bytes)
        del m
        gc.collect()
    return _SUMMARIES[key]


def test_conf_parsing():
    from dynamic_multiview_3d_amd.model_base import occlusion_from_conf, occlusion_image_terms_from_conf, occlusion_multiscale_from_conf
    on = dict(ON, batch_size=4)
    for off in ({}, {KEY: None}, {KEY: False}):
        assert occlusion_multiscale_from_conf(off) is False and occlusion_multiscale_from_conf(dict(on, **off)) is False
    assert occlusion_multiscale_from_conf(dict(on, **{KEY: True})) is True
    assert occlusion_multiscale_from_conf(dict(on, **{KEY: np.bool_(True)})) is True
    for bad in (1, 0, 'yes', 1.0, 'True'):                                  # not a bool: refused with the switches off as well
        for base in ({}, on, {'occlusion_mask': False}, dict(on, multiscale_loss_levels=2)):
            with pytest.raises(ValueError, match=KEY):
                occlusion_multiscale_from_conf(dict(base, **{KEY: bad}))
    for base in ({}, {'occlusion_mask': False}, {'occlusion_mask': None, 'pair_swap': True}, {'multiscale_loss_levels': 2}):
        with pytest.raises(ValueError, match='needs conf\\[\'occlusion_mask\'\\]'):
            occlusion_multiscale_from_conf(dict(base, **{KEY: True}))
    # occlusion_from_conf keeps its 3-tuple and its refusals; the key lifts the multi-scale one only
    for off in ({}, {KEY: None}, {KEY: False}):
        for image in ({}, {IMAGE_KEY: True}):
            with pytest.raises(ValueError, match='multiscale_loss_levels'):
                occlusion_from_conf(dict(on, multiscale_loss_levels=2, **off, **image))
    assert occlusion_from_conf(dict(on, multiscale_loss_levels=2, **{KEY: True})) == (0.01, 0.5, True)
    assert occlusion_from_conf(dict(on, **{KEY: True})) == (0.01, 0.5, True)
    with pytest.raises(ValueError, match='census_loss_weight'):              # the image terms keep their own key
        occlusion_from_conf(dict(on, multiscale_loss_levels=2, census_loss_weight=0.5, **{KEY: True}))
    both = dict(on, multiscale_loss_levels=2, census_loss_weight=0.5, **{KEY: True, IMAGE_KEY: True})
    assert occlusion_from_conf(both) == (0.01, 0.5, True) and occlusion_image_terms_from_conf(both) and occlusion_multiscale_from_conf(both)


def test_the_key_puts_the_masked_term_behind_the_fused_head(lib):
    """The conf the parent refuses.  The head stays the one fused tiled launch, which writes the mask on the way; the three
    multi-scale launches come behind it and the reverse plans are those of occlusion_mask alone (the fused head has stored the
    flow's gradient, so the term's one call gives the value and adds its gradient)."""
    from dynamic_multiview_3d_amd.graph import LOSS_MULTISCALE, MultiscaleTerm, OcclusionMaskNode, ResampleNode
    alone = _summary(**ON)
    assert alone[0][0][-2:] == ['occl_head_tile', 'occl_head_final']
    m = _appflow(multiscale_loss_levels=2, **dict(ON, **{KEY: True}))
    fwd, bwd, bwd_fused = _labels(m)
    assert fwd == alone[0][0] + MS_LABELS and 'multiscale_loss_tile' not in fwd + (bwd or []) + (bwd_fused or [])
    assert [bwd, bwd_fused] == alone[0][1:]
    (occl,) = [n for n in m.graph.nodes if isinstance(n, OcclusionMaskNode)]
    (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
    assert node.fused_loss is not None and node.fused_occlusion is occl and occl.fused_into is node
    (w2, t2), (wm, tm) = m.graph.loss_expr.terms
    assert (w2, t2.kind, t2.mask) == (1.0, 2, occl.mask)
    assert isinstance(tm, MultiscaleTerm) and (wm, tm.kind, tm.a, tm.b, tm.src, tm.levels) == (1.0, LOSS_MULTISCALE, m.flow_field, m.image1, m.image0, 2)
    assert tm.mask is occl.mask
    assert tm.ws.numel() == lib.multiscale_warp_loss_workspace_bytes(2, 128, 128, 128, 128, 3, 2)
    assert m.multiscale_terms == [('flow', m.flow_field, m.image0, m.image1, 2, 'l2')]
    assert m.masked_multiscale_terms == [('flow', m.flow_field, m.image0, m.image1, 2, 'l2', occl.mask)]
    del m, occl, node, t2, tm
    gc.collect()
    # the unmasked conf records the same launches behind its own head, under the unmasked label
    plain = _labels(_appflow(multiscale_loss_levels=2))[0]
    assert plain[-4:] == ['resample_loss', 'multiscale_pyramid', 'multiscale_loss_tile', 'multiscale_loss_final']


def test_the_key_combines_with_the_other_flow_terms_and_the_image_terms(lib):
    conf = dict(ON, multiscale_loss_levels=3, multiscale_loss_kind='l1', flow_smoothness_weight=0.1, flow_consistency_weight=0.2,
                census_loss_weight=0.5, **{KEY: True, IMAGE_KEY: True})
    m = _appflow(**conf)
    fwd = _labels(m)[0]
    masks = [t.mask for _, t in m.graph.loss_expr.terms]
    del m
    gc.collect()
    assert 'multiscale_loss_masked_tile' in fwd and 'census_loss_masked_tile' in fwd and 'multiscale_loss_tile' not in fwd
    assert fwd.index('occl_mask') < fwd.index('multiscale_loss_masked_tile')          # the census term keeps the head unfused
    # head, census and multi-scale carry the one mask; smoothness and consistency stay unmasked
    assert [x is not None for x in masks] == [True, True, False, True, False] and masks[0] is masks[1] is masks[3]


def test_the_key_without_the_multiscale_switch_records_the_plans_of_occlusion_mask_alone(lib):
    alone = _summary(**ON)
    assert _summary(**dict(ON, **{KEY: True})) == alone
    assert _summary(multiscale_loss_levels=0, **dict(ON, **{KEY: True})) == alone
    assert _summary(multiscale_loss_levels=2, multiscale_loss_weight=0.0, **dict(ON, **{KEY: True})) == alone
    m = _appflow(**dict(ON, **{KEY: True}))
    assert not hasattr(m, 'masked_multiscale_terms') and not hasattr(m, 'multiscale_terms')


@pytest.mark.parametrize("conf", [{}, dict(multiscale_loss_levels=2), ON], ids=['default', 'multiscale', 'occlusion'])
def test_key_absent_none_or_false_changes_nothing(lib, conf):
    """Plans, tensor count and activation bytes are those of the same conf without the key."""
    absent = _summary(**conf)
    assert _summary(**dict(conf, **{KEY: None})) == absent and _summary(**dict(conf, **{KEY: False})) == absent
    assert absent[0][0][-1] == {0: 'resample_loss', 1: 'multiscale_loss_final', 2: 'occl_head_final'}[len(conf)]


def test_without_the_key_the_refusal_of_the_combination_is_still_made(lib):
    for image in ({}, {IMAGE_KEY: True}):
        for off in ({}, {KEY: None}, {KEY: False}):
            with pytest.raises(ValueError, match='occlusion_mask'):
                _appflow(multiscale_loss_levels=2, **dict(ON, **off, **image))


def test_refusals_of_the_key(lib):
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    for bad in (1, 'yes', 0.0):
        for base in ({}, ON, dict(ON, multiscale_loss_levels=2), dict(multiscale_loss_levels=2)):
            with pytest.raises(ValueError, match=KEY):
                _appflow(**dict(base, **{KEY: bad}))
    with pytest.raises(ValueError, match=KEY):                              # True needs occlusion_mask
        _appflow(**{KEY: True})
    with pytest.raises(ValueError, match=KEY):
        _appflow(multiscale_loss_levels=2, pair_swap=True, occlusion_mask=False, **{KEY: True})
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    for conf in ({KEY: True}, dict(ON, **{KEY: True}), {KEY: 'yes'}):     # classes without supports_occlusion_mask
        with pytest.raises(ValueError, match='occlusion_mask'):
            Base_Prediction_Model(dict(bp, **conf), load_tfrec=False, device='cpu')
    assert not MultiObjectAppFlow.supports_occlusion_mask
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError):
            cls(dict({'batch_size': 2}, **{KEY: True}), device='cpu')
    # multiscale_term() before head_loss(): there is no mask for the flow yet
    stub = object.__new__(AppearanceFlowModel)
    stub.conf = dict(ON, batch_size=2, multiscale_loss_levels=2, **{KEY: True})
    with pytest.raises(RuntimeError, match='head_loss'):
        stub.multiscale_term(object(), object(), object())


def test_the_family_takes_the_key(lib):
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for cls in (AppearanceFlowTinghui, AppFlowHighDimAngle, AppFlowLowDimAngle):
        m = _appflow(cls, multiscale_loss_levels=3, **dict(ON, **{KEY: True}))
        fwd = _labels(m)[0]
        del m
        gc.collect()
        assert fwd[-5:] == ['occl_head_tile', 'occl_head_final'] + MS_LABELS, cls.__name__


# ------------------------------------------------------------------------------------------------ evaluate(), host path
def test_evaluate_reports_the_masked_rows_on_a_cpu_graph_only_when_the_key_is_on(lib, monkeypatch):
    """A CPU graph cannot run a forward pass, so forward() is replaced by one that fills the tensors evaluate() reads; the numpy
    forms then score them.  flow/photo_x* stay the unmasked figures."""
    rng = np.random.default_rng(12)
    shape = (2, 128, 128, 3)
    src, target = rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32)
    flow = rng.uniform(-3, 3, (2, 128, 128, 2)).astype(np.float32)
    mask = (rng.uniform(0, 1, (2, 128, 128, 1)) < 0.6).astype(np.float32)

    class Data:
        def next(self):
            return {}

    def run(m):
        def forward(**feeds):
            m.flow_field.set(flow.copy())
            m.gen.set(src.copy())
            m.image0.set(src.copy())
            m.image1.set(target.copy())
            for term in getattr(m, 'occlusion_terms', []):
                term[2].set(mask.copy())
            return torch.zeros(())
        monkeypatch.setattr(m, 'forward', forward)
        return m.evaluate(Data(), num_batches=1)
    plain = run(_appflow(pair_swap=True, multiscale_loss_levels=3))
    assert 'flow/photo_x8' in plain and not any(k.endswith('_masked') for k in plain)
    gc.collect()
    alone = run(_appflow(**dict(ON, **{KEY: True})))
    assert 'flow/visible' in alone and not any('photo' in k for k in alone)
    gc.collect()
    on = run(_appflow(multiscale_loss_levels=3, multiscale_loss_kind='l1', multiscale_loss_weight=[1.0, 0.5, 0.25], **dict(ON, **{KEY: True})))
    names = ['flow/photo_x2_masked', 'flow/photo_x4_masked', 'flow/photo_x8_masked']
    assert list(on)[-4:] == names + ['images']
    assert set(on) == set(plain) | {'flow/visible', 'flow/occluded', 'flow/outside'} | set(names)
    want_plain = metrics.multiscale_warp_loss_host(src, flow, target, 3, None, 1)[2]
    want = metrics.multiscale_warp_loss_host(src, flow, target, 3, None, 1, mask=mask)[2]
    for l, name in enumerate(names):
        assert on[name] == float(want[l]) and on[name[:-7]] == float(want_plain[l])
        assert 0 < on[name] < on[name[:-7]]
