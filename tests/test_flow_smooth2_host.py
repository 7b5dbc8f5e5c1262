"""CPU-side checks of the second-order flow smoothness (conf['flow_smoothness_order'] = 2): the numpy twin
(metrics.flow_smoothness_host(order=2)) against central differences of its own float64 value, its exact zeros on constant and
dyadic affine flows, what it is for (an affine flow costs nothing, where the first-order term charges it), the stencil weight as
the product of two first-order edge weights, order=1 bit for bit what the function was, the conf parser, the graph op's
refusals, the plans a CPU graph records with the key absent, 1 and 2, the argument lists SmoothTerm hands to the library (the
check of tests/test_loss_calls_host.py) and the device-less refusals of mv3d_flow_smoothness2."""
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from dynamic_multiview_3d_amd import graph as G
from tests.test_flow_smooth_host import SHAPES, _appflow, _inputs, _labels, _recorded
from tests.test_loss_calls_host import Recorder, _converts


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _affine(n, h, w, a, b):
    """[n,h,w,2] float32: channel c = a[c] + b[c][0] x + b[c][1] y."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([a[c] + b[c][0] * x + b[c][1] * y for c in range(2)], -1)
    return np.broadcast_to(f, (n, h, w, 2)).astype(np.float32)


DYADIC = ((0.75, -1.5), ((0.125, -0.25), (0.5, 0.0625)))
GENERIC = ((0.37, -2.1), ((0.013, -0.021), (0.017, 0.009)))


# ------------------------------------------------------------------------------------------------ the numpy twin
def test_gradient_matches_central_differences_of_the_float64_value():
    rng = np.random.default_rng(11)
    flow = rng.uniform(-3, 3, (2, 5, 7, 2))
    guide = rng.uniform(0, 1, (2, 5, 7, 3))
    _, grad = metrics.flow_smoothness_host(flow, guide, 10.0, 1e-3, np.float64, 0.75, order=2)
    assert grad.shape == flow.shape and grad.dtype == np.float64
    step = 1e-6
    numeric = np.empty_like(flow)
    for at in np.ndindex(*flow.shape):
        up, down = flow.copy(), flow.copy()
        up[at] += step
        down[at] -= step
        numeric[at] = (float(metrics.flow_smoothness_host(up, guide, 10.0, 1e-3, np.float64, 0.75, order=2)[0])
                       - float(metrics.flow_smoothness_host(down, guide, 10.0, 1e-3, np.float64, 0.75, order=2)[0])) / (2 * step)
    rel = np.linalg.norm(grad - numeric) / np.linalg.norm(numeric)
    print('second-order twin against central differences: relative L2 %.2e' % rel)
    assert np.linalg.norm(numeric) > 0 and rel <= 1e-6


@pytest.mark.parametrize("hw", [(3, 3), (21, 70), (35, 131)])
def test_constant_and_dyadic_affine_flows_give_exactly_zero_at_float32(hw):
    """First differences that are exact and equal along each axis: d == 0, sqrt(eps * eps) == eps, so (+0, zeros) under any guide."""
    h, w = hw
    rng = np.random.default_rng(h * w)
    const = np.broadcast_to(np.array([0.37, -2.125], np.float32), (2, h, w, 2))
    for flow in (const, _affine(2, h, w, *DYADIC)):
        for guide in (None, rng.uniform(0, 1, (2, h, w, 3)).astype(np.float32)):
            for eps in (1e-3, 0.3):
                loss, grad = metrics.flow_smoothness_host(flow, guide, 10.0, eps, np.float32, 0.5, order=2)
                assert isinstance(loss, np.float32) and grad.dtype == np.float32
                assert float(loss) == 0.0 and not np.signbit(loss) and not np.any(grad)


def test_a_generic_affine_flow_costs_nothing_at_order_2_and_something_at_order_1():
    flow = _affine(1, 35, 131, *GENERIC)
    second = float(metrics.flow_smoothness_host(flow, None, 10.0, 1e-3, np.float64, order=2)[0])
    second32 = float(metrics.flow_smoothness_host(flow, None, 10.0, 1e-3, np.float32, order=2)[0])
    first = float(metrics.flow_smoothness_host(flow, None, 10.0, 1e-3, np.float64)[0])
    print('affine flow on 35 x 131: order 1 %.4f, order 2 %.2e in float64, %.2e in float32' % (first, second, second32))
    assert 0 <= second < 1e-9 and 0 <= second32 < 1e-9           # rounding of the float32 flow values only
    assert first > 1e-3


def test_the_stencil_weight_is_the_product_of_the_two_first_order_edge_weights():
    rng = np.random.default_rng(3)
    guide = rng.uniform(0, 1, (2, 9, 11, 3))
    alpha = 10.0
    for axis in (1, 2):
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        edge = np.exp(-(alpha / 3) * np.abs(guide[tuple(hi)] - guide[tuple(lo)]).sum(axis=3))       # the first-order weights
        first, second = [slice(None)] * 3, [slice(None)] * 3
        first[axis], second[axis] = slice(None, -1), slice(1, None)
        want = edge[tuple(first)] * edge[tuple(second)]
        got = metrics._smooth2_weights(guide, alpha, axis, np.float64)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12
    # ... and it is what the twin applies: with a guide the value is the weighted sum of the unguided penalties
    flow = rng.uniform(-3, 3, (2, 9, 11, 2))
    eps = float(np.float32(1e-3))
    total = 0.0
    for axis in (2, 1):
        lo, mid, hi = metrics._smooth2_slices(axis)
        d = (flow[hi] - flow[mid]) - (flow[mid] - flow[lo])
        v = metrics._smooth2_weights(guide, alpha, axis, np.float64)[..., None] * (np.sqrt(d * d + eps * eps) - eps)
        total += v.sum() / v.size
    assert abs(float(metrics.flow_smoothness_host(flow, guide, alpha, 1e-3, np.float64, order=2)[0]) - total) <= 1e-12 * total


def test_value_and_gradient_are_linear_in_the_weight():
    flow, guide = _inputs((2, 9, 11), 3, 5)
    l1, g1 = metrics.flow_smoothness_host(flow, guide, 10.0, 1e-3, np.float64, 1.0, order=2)
    for weight in (0.25, -2.0, 0.0):                              # exact in float32, so the float64 results scale exactly
        lw, gw = metrics.flow_smoothness_host(flow, guide, 10.0, 1e-3, np.float64, weight, order=2)
        assert abs(float(lw) - weight * float(l1)) <= 1e-15 * abs(float(l1))
        assert np.abs(gw - weight * g1).max() <= 1e-15 * np.abs(g1).max()
    plain = metrics.flow_smoothness_host(flow, order=2)
    zero = metrics.flow_smoothness_host(flow, guide, 0.0, order=2)
    assert float(plain[0]) == float(zero[0]) and np.array_equal(plain[1], zero[1])       # alpha 0: no guide is read
    assert 0 < float(l1) < float(plain[0])


def _first_order_float32(flow, guide, alpha, eps, weight):
    """What flow_smoothness_host computed at float32 before it took `order`, written out again."""
    t = np.float32
    f = np.asarray(flow).astype(t)
    g = None if guide is None else np.asarray(guide).astype(t)
    alpha, eps, weight = (float(t(v)) for v in (alpha, eps, weight))
    n, h, w, _ = f.shape
    eps_t = t(eps)
    eps2 = eps_t * eps_t
    zx, zy = float(n) * h * (w - 1) * 2.0, float(n) * (h - 1) * w * 2.0
    e, v = {}, {}
    for axis in (2, 1):
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        d = f[tuple(hi)] - f[tuple(lo)]
        wgt = np.ones(d.shape[:3] + (1,), t)
        if g is not None:
            ad = np.abs(g[tuple(hi)] - g[tuple(lo)])
            s = np.zeros(ad.shape[:3], t)
            for k in range(ad.shape[3]):
                s = s + ad[..., k]
            wgt = np.exp(-(t(alpha / g.shape[3]) * s))[..., None].astype(t)
        r = np.sqrt(d * d + eps2)
        e[axis], v[axis] = wgt * (d / r), wgt * (r - eps_t)
    loss = t(weight * (float(v[2].sum(dtype=t)) / zx + float(v[1].sum(dtype=t)) / zy))
    px = np.zeros((n, h, w + 1, 2), t)
    px[:, :, 1:w] = e[2]
    py = np.zeros((n, h + 1, w, 2), t)
    py[:, 1:h] = e[1]
    return loss, (px[:, :, :-1] - px[:, :, 1:]) * t(weight / zx) + (py[:, :-1] - py[:, 1:]) * t(weight / zy)


@pytest.mark.parametrize("shape", SHAPES)
def test_order_1_is_bit_for_bit_what_the_function_returned_before(shape):
    for cg, alpha in ((0, 10.0), (1, 10.0), (3, 0.0), (3, 10.0)):
        flow, guide = _inputs(shape, cg, seed=sum(shape) + cg)
        for eps, weight in ((1e-3, 1.0), (0.05, 0.25)):
            want_l, want_g = _first_order_float32(flow, guide, alpha, eps, weight)
            for got_l, got_g in (metrics.flow_smoothness_host(flow, guide, alpha, eps, np.float32, weight),
                                 metrics.flow_smoothness_host(flow, guide, alpha, eps, np.float32, weight, order=1)):
                assert isinstance(got_l, np.float32) and got_g.dtype == np.float32
                assert got_l.tobytes() == want_l.tobytes() and got_g.tobytes() == want_g.tobytes()


def test_operand_checks_of_the_twin():
    f = np.zeros((1, 4, 4, 2), np.float32)
    for bad in (0, 3, True, 2.5, None, '2'):
        with pytest.raises(ValueError, match='order'):
            metrics.flow_smoothness_host(f, order=bad)
    for small in (f[:, :2], f[:, :, :2]):
        metrics.flow_smoothness_host(small)                              # order 1 takes a side of 2
        with pytest.raises(ValueError, match='H, W >= 3'):
            metrics.flow_smoothness_host(small, order=2)
    with pytest.raises(ValueError, match='guide'):
        metrics.flow_smoothness_host(f, np.zeros((1, 4, 5, 3), np.float32), order=2)
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_smoothness_host(f, eps=0.0, order=2)
    # the device mirror makes the same checks before it calls the library: no device is needed to see them
    t = torch.zeros((1, 4, 4, 2))
    with pytest.raises(ValueError, match='order'):
        metrics.flow_smoothness(t, order=3)
    with pytest.raises(ValueError, match='H, W >= 3'):
        metrics.flow_smoothness(torch.zeros((1, 2, 4, 2)), order=2)


# ------------------------------------------------------------------------------------------------ conf
def test_conf_parser_accepts_and_refuses_what_it_should():
    from dynamic_multiview_3d_amd.model_base import flow_smoothness_from_conf, flow_smoothness_order_from_conf
    assert flow_smoothness_order_from_conf({}) == 1
    assert flow_smoothness_order_from_conf({'flow_smoothness_order': None}) == 1
    assert flow_smoothness_order_from_conf({'flow_smoothness_order': 1}) == 1
    assert flow_smoothness_order_from_conf({'flow_smoothness_order': 2}) == 2
    assert flow_smoothness_order_from_conf({'flow_smoothness_order': np.int64(2), 'flow_smoothness_weight': 0.1}) == 2
    for bad in (True, False, 0, 3, -1, 2.0, 1.5, '2', [2]):
        for weight in ({}, {'flow_smoothness_weight': 0.1}):             # whether or not the weight is set
            with pytest.raises(ValueError, match='flow_smoothness_order'):
                flow_smoothness_order_from_conf(dict(weight, flow_smoothness_order=bad))
    assert flow_smoothness_from_conf({'flow_smoothness_weight': 0.5, 'flow_smoothness_order': 2}) == (0.5, 10.0, 1e-3)       # its 3-tuple
    with pytest.raises(ValueError, match='flow_smoothness_order'):
        _appflow(flow_smoothness_order=3)                                # a constructor refuses it before it builds anything
    with pytest.raises(ValueError, match='flow_smoothness_order'):
        _appflow(flow_smoothness_order=True, flow_smoothness_weight=0.1)


# ------------------------------------------------------------------------------------------------ graph op
def test_op_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    with G.Graph(device='cpu') as g:
        img = g.placeholder([2, 16, 16, 3], 'img')
        mask = g.placeholder([2, 16, 16, 1], 'mask')
        thin = g.placeholder([2, 2, 16, 3], 'thin')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
        three = tf_utils.conv2d_msra(img, 3, 3, 3, 1, 1, 'three')
        thin_flow = tf_utils.conv2d_msra(thin, 2, 3, 3, 1, 1, 'thin_flow')
        for bad in (0, 3, True, 2.0):
            with pytest.raises(ValueError, match='order'):
                tf_utils.flow_smoothness_loss(flow, img, order=bad)
        tf_utils.flow_smoothness_loss(thin_flow)                         # H = 2 is enough for first differences
        with pytest.raises(ValueError, match='H, W >= 3'):
            tf_utils.flow_smoothness_loss(thin_flow, order=2)
        with pytest.raises(ValueError, match='not differentiated'):
            tf_utils.flow_smoothness_loss(g.placeholder([2, 16, 16, 2], 'fed'), order=2)
        with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
            tf_utils.flow_smoothness_loss(three, order=2)
        with pytest.raises(NotImplementedError, match='guide'):
            tf_utils.flow_smoothness_loss(flow, three, order=2)
        with pytest.raises(NotImplementedError):
            tf_utils.flow_smoothness_loss(flow, tf_utils.multiply(img, mask), order=2)
        with pytest.raises(NotImplementedError):
            tf_utils.flow_smoothness_loss(tf_utils.scale(flow, 0.5), order=2)
        e = tf_utils.flow_smoothness_loss(flow, img, 5.0, 1e-2, order=2) * 0.5 + tf_utils.flow_smoothness_loss(flow)
        (w2, t2), (w1, t1) = e.terms
        assert (w2, t2.kind, t2.order, t2.on_flow, t2.second_order) == (0.5, G.LOSS_SMOOTH, 3, True, True)
        assert (w1, t1.kind, t1.order, t1.on_flow, t1.second_order) == (1.0, G.LOSS_SMOOTH, 3, True, False)
        assert (t2.a, t2.b, t2.edge_alpha, t2.eps) == (flow, img, 5.0, 1e-2)
    # the library's own answer for a flow it does not take reaches the caller as a ValueError that names the entry
    term = G.SmoothTerm(thin_flow, None, second_order=True)
    with pytest.raises(ValueError, match='mv3d_flow_smoothness2'):
        term.workspace_bytes(lib)
    assert G.SmoothTerm(thin_flow, None).workspace_bytes(lib) == 256


# ------------------------------------------------------------------------------------------------ conf switch on recorded plans
def _second(labels):
    return [[{'flow_smooth_tile': 'flow_smooth2_tile', 'flow_smooth_final': 'flow_smooth2_final'}.get(l, l) for l in plan]
            if plan is not None else None for plan in labels]


@pytest.mark.parametrize("extra", [{}, {'ssim_loss_weight': 0.5}], ids=['fused', 'ssim'])
def test_cpu_graph_records_the_second_order_labels_in_the_first_order_places(lib, extra):
    first = _labels(_appflow(flow_smoothness_weight=0.25, **extra))
    assert any('flow_smooth_tile' in plan for plan in first if plan)
    assert first == _labels(_appflow(flow_smoothness_weight=0.25, flow_smoothness_order=1, **extra))
    assert first == _labels(_appflow(flow_smoothness_weight=0.25, flow_smoothness_order=None, **extra))
    m = _appflow(flow_smoothness_weight=0.25, flow_smoothness_order=2, **extra)
    assert _labels(m) == _second(first) != first
    # the term is the same one, in the same place, with the flag set; evaluate() will report it under its own key
    ts = [t for _, t in m.graph.loss_expr.terms if t.kind == G.LOSS_SMOOTH]
    assert len(ts) == 1 and ts[0].second_order and ts[0].a is m.flow_field and ts[0].b is m.image1
    assert ts[0].ws.numel() == lib.flow_smoothness2_workspace_bytes(2, 128, 128)
    assert m.smoothness2_terms == [('flow', m.flow_field, m.image1, 10.0, 1e-3)] and not hasattr(m, 'smoothness_terms')
    off = _labels(_appflow(**extra))
    for weight in ({}, {'flow_smoothness_weight': 0.0}, {'flow_smoothness_weight': None}):
        m = _appflow(flow_smoothness_order=2, **weight, **extra)
        assert _labels(m) == off                                         # order 2 without a weight: no smoothness term at all
        assert not hasattr(m, 'smoothness2_terms') and not hasattr(m, 'smoothness_terms')


def test_multiobject_heads_take_the_order_with_no_code_of_their_own(lib):
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': 0.1, 'combination_image': '', 'gen_sep_images': '',
            'masked_image_loss': '', 'fully_conv': '', 'flow_smoothness_weight': 0.5}
    first = _labels(MultiObjectAppFlow(conf, load_tfrec=False, device='cpu'))
    m = MultiObjectAppFlow(dict(conf, flow_smoothness_order=2), load_tfrec=False, device='cpu')
    assert _labels(m) == _second(first) and _labels(m)[0].count('flow_smooth2_tile') == 3
    assert [s[0] for s in m.smoothness2_terms] == [name for name, _ in m.flow_heads]


# ------------------------------------------------------------------------------------------------ the library call
@pytest.fixture(scope='module')
def terms():
    with G.Graph(device='cpu') as g:
        from dynamic_multiview_3d_amd import tf_utils
        img = g.placeholder([2, 16, 16, 3], 'img')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
    g.finalize()
    assert flow.requires_grad
    return g, {'unguided': G.SmoothTerm(flow, None, second_order=True), 'guided': G.SmoothTerm(flow, img, 10.0, second_order=True)}


@pytest.mark.parametrize('value, grad, accumulate', [(True, False, False), (True, True, False), (True, True, True), (False, True, True)])
@pytest.mark.parametrize('case', ['unguided', 'guided'])
def test_launch_calls_the_second_entry_alone_with_the_declared_arguments(terms, case, value, grad, accumulate):
    g, by_case = terms
    term = by_case[case]
    term.ws = torch.empty(64, dtype=torch.uint8)
    rec, real = Recorder(), g.lib
    g.lib = rec
    try:
        term.launch(g, 0.5, value, grad, accumulate)
    finally:
        g.lib = real
    (name, args), = rec.calls                               # exactly one entry
    assert name == 'flow_smoothness2'
    _converts(_lib.STATUS_FUNCS['mv3d_flow_smoothness2'], args)
    assert args[6] == (3 if case == 'guided' else 0) and (args[11] is not None) == value and (args[12] is not None) == grad
    assert args[14] == (1 if grad and accumulate else 0)


@pytest.mark.parametrize('case', ['unguided', 'guided'])
def test_workspace_bytes_calls_the_second_size_entry_alone(terms, case):
    rec = Recorder()
    assert terms[1][case].workspace_bytes(rec) == 64
    (name, args), = rec.calls
    assert name == 'flow_smoothness2_workspace_bytes' and args == (2, 16, 16)
    _converts(_lib.OTHER_FUNCS['mv3d_flow_smoothness2_workspace_bytes'][1], args)


def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_flow_smoothness2', 'mv3d_flow_smoothness2_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.flow_smoothness2) and callable(lib.raw_flow_smoothness2)
    assert _lib.STATUS_FUNCS['mv3d_flow_smoothness2'] == _lib.STATUS_FUNCS['mv3d_flow_smoothness']
    assert lib.flow_smoothness2_workspace_bytes(1, 3, 3) == 256                    # one tile x 2 sums x 8 bytes, rounded up to 256
    assert lib.flow_smoothness2_workspace_bytes(64, 128, 128) == lib.flow_smoothness_workspace_bytes(64, 128, 128) == 64 * 8 * 2 * 16
    for n, h, w in ((2, 2, 77), (2, 77, 2), (1, 2, 2), (0, 4, 4)):
        assert lib.flow_smoothness2_workspace_bytes(n, h, w) == 0


def test_the_library_refuses_a_side_of_2_without_a_device_and_names_the_argument(lib):
    ok = dict(N=2, H=16, W=16, flow=0x1000, flow_ld=2, guide=0x2000, gc=3, guide_ld=3, alpha=10.0, eps=1e-3, weight=1.0, loss=0x3000,
              grad=0x5000, grad_ld=2, acc=0, ws=0x4000, ws_bytes=4096)

    def call(**kw):
        v = dict(ok, **kw)
        return _recorded(lib, lambda: lib.raw_flow_smoothness2(
            v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['guide'], v['gc'], v['guide_ld'], v['alpha'], v['eps'], v['weight'],
            v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], None))
    inf, nan = float('inf'), float('nan')
    for kw, code, word in [(dict(H=2), -1, 'H (2)'), (dict(W=2), -1, 'W (2)'), (dict(H=1), -1, 'H (1)'), (dict(N=0), -1, 'N'),
                           (dict(N=1 << 30, H=1 << 20, W=1 << 20), -1, 'tiles'), (dict(N=1 << 10, H=1 << 15, W=1 << 15, flow_ld=1 << 30), -1, 'overflow'),
                           (dict(flow_ld=1), -1, 'flow_ld'), (dict(gc=5), -1, 'guide_c'), (dict(gc=-1), -1, 'guide_c'),
                           (dict(guide=None), -1, 'guide'), (dict(guide_ld=2), -1, 'guide_ld'), (dict(grad_ld=1), -1, 'grad_ld'),
                           (dict(acc=2), -1, 'grad_accumulate'), (dict(eps=0.0), -1, 'eps'), (dict(eps=nan), -1, 'eps'),
                           (dict(alpha=-1.0), -1, 'edge_alpha'), (dict(alpha=inf), -1, 'edge_alpha'), (dict(weight=nan), -1, 'weight'),
                           (dict(flow=None), -1, 'flow is null'), (dict(loss=None, grad=None), -1, 'both null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(flow=0x1002), -1, 'aligned'), (dict(guide=0x2001), -1, 'aligned'),
                           (dict(grad=0x5001), -1, 'aligned'), (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x4008), -3, 'aligned')]:
        rc, labels = call(**kw)
        assert rc == code and labels == [], (kw, rc, labels)
        assert word in lib.last_error() and 'mv3d_flow_smoothness2:' in lib.last_error(), (kw, lib.last_error())
    assert call(H=3, W=3) == (0, ['flow_smooth2_tile', 'flow_smooth2_final'])
    assert call(grad=None) == (0, ['flow_smooth2_tile', 'flow_smooth2_final'])            # value only
    assert call(loss=None) == (0, ['flow_smooth2_tile'])                                  # gradient only: one launch
    assert call(guide=None, gc=0, guide_ld=0) == (0, ['flow_smooth2_tile', 'flow_smooth2_final'])
    assert call(flow=0x1004, flow_ld=4, grad=0x5004, grad_ld=4, guide_ld=4)[0] == 0       # channel-slice views
