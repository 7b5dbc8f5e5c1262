"""CPU-side checks of the edge-aware flow smoothness loss: the numpy twin (metrics.flow_smoothness_host) against float64 torch
autograd over an independent restatement (slicing differences, torch.exp, torch.sqrt), the exact zeros of a constant flow, the
refusals of mv3d_flow_smoothness (they come before any launch, so they need no device), the refusals of the graph op, and the
scheduling of conf['flow_smoothness_weight'] on recorded plans: fused head, unfused resampler, smoothness alone."""
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics

SHAPES = [(1, 2, 2), (3, 5, 2), (2, 2, 7), (2, 45, 77)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _inputs(shape, cg, seed):
    rng = np.random.default_rng(seed)
    flow = rng.uniform(-3, 3, shape + (2,)).astype(np.float32)
    flow[0, 0, 1] = flow[0, 0, 0]                             # one exact repeat: d == 0 on an edge
    guide = rng.uniform(0, 1, shape + (cg,)).astype(np.float32) if cg else None
    return flow, guide


def torch_flow_smoothness(flow, guide, alpha, eps, weight):
    """(loss, d loss / d flow) in float64 by autograd, written from the definition."""
    f = torch.tensor(flow, dtype=torch.float64, requires_grad=True)
    eps = float(np.float32(eps))
    total = 0.0
    for axis in (2, 1):
        d = f.narrow(axis, 1, f.shape[axis] - 1) - f.narrow(axis, 0, f.shape[axis] - 1)
        phi = torch.sqrt(d * d + eps * eps) - eps
        if guide is not None:
            g = torch.tensor(guide, dtype=torch.float64)
            dg = g.narrow(axis, 1, g.shape[axis] - 1) - g.narrow(axis, 0, g.shape[axis] - 1)
            phi = phi * torch.exp(-alpha * dg.abs().mean(dim=3, keepdim=True))
        total = total + phi.sum() / phi.numel()
    loss = float(np.float32(weight)) * total
    loss.backward()
    return float(loss.detach()), f.grad.numpy()


@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("cg", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_twin_matches_autograd(shape, cg, alpha):
    flow, guide = _inputs(shape, cg, seed=sum(shape) + cg)
    for eps, weight in ((1e-3, 1.0), (0.05, 0.25)):
        loss, grad = metrics.flow_smoothness_host(flow, guide, alpha, eps, np.float64, weight)
        assert grad.shape == flow.shape and grad.dtype == np.float64
        tl, tg = torch_flow_smoothness(flow, guide, alpha, eps, weight)
        rel_l = abs(float(loss) - tl) / abs(tl)
        rel_g = np.linalg.norm(grad - tg) / np.linalg.norm(tg)
        print('%s Cg %d alpha %g eps %g: loss %.8f rel %.1e, gradient rel L2 %.1e' % (shape, cg, alpha, eps, loss, rel_l, rel_g))
        assert rel_l <= 1e-10
        assert rel_g <= 1e-10


def test_alpha_zero_and_no_guide_agree_and_the_guide_lowers_the_penalty():
    flow, guide = _inputs((2, 9, 11), 3, 5)
    plain = metrics.flow_smoothness_host(flow)
    zero = metrics.flow_smoothness_host(flow, guide, 0.0)
    assert float(plain[0]) == float(zero[0]) and np.array_equal(plain[1], zero[1])
    assert 0 < float(metrics.flow_smoothness_host(flow, guide, 10.0)[0]) < float(plain[0])


def test_float32_twin_is_close_to_float64():
    flow, guide = _inputs(SHAPES[-1], 3, 7)
    l64, g64 = metrics.flow_smoothness_host(flow, guide, 10.0, 1e-3, np.float64)
    l32, g32 = metrics.flow_smoothness_host(flow, guide, 10.0, 1e-3, np.float32)
    assert g32.dtype == np.float32 and isinstance(l32, np.float32)
    assert abs(float(l32) - float(l64)) <= 1e-5 * float(l64)
    assert np.linalg.norm(g32 - g64) / np.linalg.norm(g64) <= 1e-5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_flow_gives_exactly_zero_loss_and_gradient(dtype):
    """sqrt(eps * eps) == eps with a correctly rounded root: phi(0) == 0 and phi'(0) == 0 whatever the guide and the weight."""
    rng = np.random.default_rng(1)
    for eps in (1e-3, 0.3, 7e-5):
        flow = np.empty((2, 6, 9, 2), np.float32)
        flow[..., 0], flow[..., 1] = 0.37, -2.125
        for guide in (None, rng.uniform(0, 1, (2, 6, 9, 3)).astype(np.float32)):
            loss, grad = metrics.flow_smoothness_host(flow, guide, 10.0, eps, dtype, 0.5)
            assert float(loss) == 0.0 and not np.any(grad)


def test_operand_checks():
    f = np.zeros((1, 4, 4, 2), np.float32)
    with pytest.raises(ValueError, match='flow'):
        metrics.flow_smoothness_host(f[..., :1])
    with pytest.raises(ValueError, match='H, W'):
        metrics.flow_smoothness_host(f[:, :1])
    with pytest.raises(ValueError, match='guide'):
        metrics.flow_smoothness_host(f, np.zeros((1, 4, 5, 3), np.float32))
    with pytest.raises(ValueError, match='guide'):
        metrics.flow_smoothness_host(f, np.zeros((1, 4, 4, 5), np.float32))
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_smoothness_host(f, eps=0.0)
    with pytest.raises(ValueError, match='edge_alpha'):
        metrics.flow_smoothness_host(f, edge_alpha=-1.0)
    with pytest.raises(ValueError, match='weight'):
        metrics.flow_smoothness_host(f, weight=float('nan'))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_flow_smoothness', 'mv3d_flow_smoothness_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.flow_smoothness) and callable(lib.raw_flow_smoothness)
    assert lib.flow_smoothness_workspace_bytes(1, 2, 2) == 256                     # one tile x 2 sums x 8 bytes, rounded up to 256
    assert lib.flow_smoothness_workspace_bytes(64, 128, 128) == 64 * 8 * 2 * 16
    assert lib.flow_smoothness_workspace_bytes(2, 1, 77) == 0 and lib.flow_smoothness_workspace_bytes(0, 4, 4) == 0


def _recorded(lib, fn):
    """Device-less recording: the labels a call appends to a plan (nothing is launched)."""
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        rc = fn()
    finally:
        lib.plan_end()
    labels = [o[0] for o in _lib.plan_ops(plan)]
    lib.plan_destroy(plan)
    return rc, labels


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns its code, names the argument and records nothing; none touches a pointer, so made-up addresses do."""
    ok = dict(N=2, H=16, W=16, flow=0x1000, flow_ld=2, guide=0x2000, gc=3, guide_ld=3, alpha=10.0, eps=1e-3, weight=1.0, loss=0x3000,
              grad=0x5000, grad_ld=2, acc=0, ws=0x4000, ws_bytes=4096)

    def call(**kw):
        v = dict(ok, **kw)
        return _recorded(lib, lambda: lib.raw_flow_smoothness(
            v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['guide'], v['gc'], v['guide_ld'], v['alpha'], v['eps'], v['weight'],
            v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], None))
    inf, nan = float('inf'), float('nan')
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(H=1), -1, 'H'), (dict(W=1), -1, 'W'),
                           (dict(N=1 << 30, H=1 << 20, W=1 << 20), -1, 'tiles'), (dict(N=1 << 10, H=1 << 15, W=1 << 15, flow_ld=1 << 30), -1, 'overflow'),
                           (dict(flow_ld=1), -1, 'flow_ld'), (dict(gc=5), -1, 'guide_c'), (dict(gc=-1), -1, 'guide_c'),
                           (dict(guide=None), -1, 'guide'), (dict(guide_ld=2), -1, 'guide_ld'), (dict(grad_ld=1), -1, 'grad_ld'),
                           (dict(acc=2), -1, 'grad_accumulate'), (dict(acc=-1), -1, 'grad_accumulate'),
                           (dict(eps=0.0), -1, 'eps'), (dict(eps=-1.0), -1, 'eps'), (dict(eps=inf), -1, 'eps'), (dict(eps=nan), -1, 'eps'),
                           (dict(alpha=-1.0), -1, 'edge_alpha'), (dict(alpha=inf), -1, 'edge_alpha'), (dict(alpha=nan), -1, 'edge_alpha'),
                           (dict(weight=inf), -1, 'weight'), (dict(weight=nan), -1, 'weight'),
                           (dict(flow=None), -1, 'flow is null'), (dict(loss=None, grad=None), -1, 'both null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(flow=0x1002), -1, 'aligned'), (dict(guide=0x2001), -1, 'aligned'),
                           (dict(grad=0x5001), -1, 'aligned'), (dict(loss=0x3002), -1, 'aligned'),
                           (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x4008), -3, 'aligned')]:
        rc, labels = call(**kw)
        assert rc == code and labels == [], (kw, rc, labels)
        assert word in lib.last_error() and 'mv3d_flow_smoothness' in lib.last_error(), (kw, lib.last_error())
    # what is accepted, and what each form records
    assert call() == (0, ['flow_smooth_tile', 'flow_smooth_final'])
    assert call(grad=None) == (0, ['flow_smooth_tile', 'flow_smooth_final'])            # value only
    assert call(loss=None) == (0, ['flow_smooth_tile'])                                 # gradient only: one launch
    assert call(guide=None, gc=0, guide_ld=0) == (0, ['flow_smooth_tile', 'flow_smooth_final'])
    assert call(flow=0x1004, flow_ld=4, grad=0x5004, grad_ld=4, guide_ld=4)[0] == 0      # channel-slice views


# ------------------------------------------------------------------------------------------------ graph op
def test_op_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, LOSS_SMOOTH
    with Graph(device='cpu') as g:
        img = g.placeholder([2, 16, 16, 3], 'img')
        mask = g.placeholder([2, 16, 16, 1], 'mask')
        other = g.placeholder([2, 16, 8, 3], 'other')
        wide = g.placeholder([2, 16, 16, 5], 'wide')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
        three = tf_utils.conv2d_msra(img, 3, 3, 3, 1, 1, 'three')
        with pytest.raises(ValueError, match='not differentiated'):
            tf_utils.flow_smoothness_loss(g.placeholder([2, 16, 16, 2], 'fed'))
        with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
            tf_utils.flow_smoothness_loss(three)
        with pytest.raises(ValueError, match='guide'):
            tf_utils.flow_smoothness_loss(flow, other)
        with pytest.raises(ValueError, match='guide'):
            tf_utils.flow_smoothness_loss(flow, wide)
        with pytest.raises(NotImplementedError, match='guide'):
            tf_utils.flow_smoothness_loss(flow, three)                   # a guide that requires a gradient
        with pytest.raises(NotImplementedError):
            tf_utils.flow_smoothness_loss(flow, tf_utils.multiply(img, mask))
        with pytest.raises(NotImplementedError):
            tf_utils.flow_smoothness_loss(tf_utils.scale(flow, 0.5))
        with pytest.raises(ValueError, match='eps'):
            tf_utils.flow_smoothness_loss(flow, img, eps=0.0)
        with pytest.raises(ValueError, match='edge_alpha'):
            tf_utils.flow_smoothness_loss(flow, img, edge_alpha=-1.0)
        e = tf_utils.flow_smoothness_loss(flow, img, 5.0, 1e-2) * 0.5 + tf_utils.euclidean_loss(three, img) + tf_utils.flow_smoothness_loss(flow)
        assert [(w, t.kind) for w, t in e.terms] == [(0.5, LOSS_SMOOTH), (1.0, 2), (1.0, LOSS_SMOOTH)]
        t0, t2 = e.terms[0][1], e.terms[2][1]
        assert (t0.a, t0.b, t0.edge_alpha, t0.eps) == (flow, img, 5.0, 1e-2) and (t2.b, t2.edge_alpha, t2.eps) == (None, 10.0, 1e-3)


# ------------------------------------------------------------------------------------------------ conf switch on recorded plans
def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def _smooth(plan):
    return [l for l in plan if l.startswith('flow_smooth')]


def test_switch_absent_zero_or_none_records_the_same_plans(lib):
    absent = _labels(_appflow())
    assert absent == _labels(_appflow(flow_smoothness_weight=0.0)) == _labels(_appflow(flow_smoothness_weight=None))
    assert absent == _labels(_appflow(flow_smoothness_weight=0, flow_smoothness_edge=3.0, flow_smoothness_eps=0.1))
    assert 'resample_loss' in absent[0] and not any(_smooth(plan) for plan in absent if plan)


def test_switch_on_keeps_the_head_fused_and_adds_one_combined_launch_behind_it(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_SMOOTH, ResampleNode
    absent = _labels(_appflow())
    m = _appflow(flow_smoothness_weight=0.25)
    fwd, bwd, fused = _labels(m)
    assert fwd == absent[0] + ['flow_smooth_tile', 'flow_smooth_final'] and fwd[-3] == 'resample_loss'
    assert bwd == absent[1] and fused == absent[2]                       # nothing is added to the reverse plans
    assert [n.fused_loss is not None for n in m.graph.nodes if isinstance(n, ResampleNode)] == [True]
    (w2, t2), (ws, ts) = m.graph.loss_expr.terms
    assert (w2, t2.kind) == (1.0, 2) and (ws, ts.kind, ts.edge_alpha, ts.eps) == (0.25, LOSS_SMOOTH, 10.0, 1e-3)
    assert ts.a is m.flow_field and ts.b is m.image1                     # the term reads the flow, not gen
    assert ts.ws.numel() == lib.flow_smoothness_workspace_bytes(2, 128, 128) and t2.ws is None
    assert m.smoothness_terms == [('flow', m.flow_field, m.image1, 10.0, 1e-3)]
    # edge 0 / None: unguided, no guide is read
    for edge in (0, None):
        m = _appflow(flow_smoothness_weight=0.25, flow_smoothness_edge=edge, flow_smoothness_eps=0.01)
        ts = m.graph.loss_expr.terms[1][1]
        assert ts.b is None and ts.eps == 0.01


def _expect_unfused(m, between):
    """Value in the forward plan behind the other terms; one gradient launch in both reverse plans right behind the resampler's
    backward and in front of the flow_field deconvolution's backward (its filter gradient is the next launch)."""
    fwd, bwd, fused = _labels(m)
    assert 'resample_loss' not in fwd
    assert fwd[-2 - len(between) - 2:] == ['resample_fwd', 'pixel_loss'] + between + ['flow_smooth_tile', 'flow_smooth_final']
    for plan in (bwd, fused):
        assert plan[:3] == ['resample_bwd', 'flow_smooth_tile', 'thin_wgrad'] and _smooth(plan) == ['flow_smooth_tile']


def test_with_ssim_or_an_unfused_head_the_gradient_follows_the_resamplers_backward(lib, monkeypatch):
    _expect_unfused(_appflow(flow_smoothness_weight=0.25, ssim_loss_weight=0.5), ['ssim_loss_tile', 'ssim_loss_final'])
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    plain = _labels(_appflow())
    m = _appflow(flow_smoothness_weight=0.25)
    _expect_unfused(m, [])
    fwd, bwd, fused = _labels(m)
    assert fwd == plain[0] + ['flow_smooth_tile', 'flow_smooth_final']
    assert bwd == plain[1][:1] + ['flow_smooth_tile'] + plain[1][1:] and fused == plain[2][:1] + ['flow_smooth_tile'] + plain[2][1:]
    # the data-parallel step replays plan_bwd in segments: the gradient launch lies inside the first one
    assert m.graph.grad_buckets[0][0] >= 3


def test_smoothness_alone_stores_the_gradient_in_front_of_the_producer(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf

    class SmoothOnly(AppearanceFlowModel):
        def build_loss(self):
            self.loss = tf_utils.flow_smoothness_loss(self.flow_field, self.image1) * 2.0
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    m = _appflow(SmoothOnly)
    fwd, bwd, fused = _labels(m)
    assert 'resample_loss' not in fwd and 'pixel_loss' not in fwd and 'fill' not in fwd
    assert fwd[-3:] == ['resample_fwd', 'flow_smooth_tile', 'flow_smooth_final']
    for plan in (bwd, fused):                                            # no resampler backward: the term's store comes first
        assert plan[:2] == ['flow_smooth_tile', 'thin_wgrad'] and 'resample_bwd' not in plan and _smooth(plan) == ['flow_smooth_tile']
    assert m.graph.variables['flow_field/w'].has_grad and m.graph.variables['e0/w'].has_grad


def test_two_terms_alone_on_one_flow_store_then_add(lib, monkeypatch):
    """Two smoothness terms on the same flow and no other writer of its gradient: the first launch of each reverse plan stores
    (grad_accumulate 0), the second adds (1).  A spy on the library call reads the argument itself."""
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf
    calls = []
    real = lib.flow_smoothness

    def spy(*args):
        # (N, H, W, flow, flow_ld, guide, guide_c, guide_ld, alpha, eps, weight, loss, grad, grad_ld, grad_accumulate, ws, ws_bytes, stream)
        calls.append(dict(guide_c=args[6], weight=args[10], loss=args[11], grad=args[12], acc=args[14]))
        return real(*args)
    monkeypatch.setattr(lib, 'flow_smoothness', spy)

    class TwoTerms(AppearanceFlowModel):
        def build_loss(self):
            self.loss = tf_utils.flow_smoothness_loss(self.flow_field, self.image1) * 2.0 + tf_utils.flow_smoothness_loss(self.flow_field) * 0.5
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    m = _appflow(TwoTerms)
    fwd, bwd, fused = _labels(m)
    assert fwd[-5:] == ['resample_fwd', 'flow_smooth_tile', 'flow_smooth_final', 'flow_smooth_tile', 'flow_smooth_final']
    for plan in (bwd, fused):
        assert plan[:3] == ['flow_smooth_tile', 'flow_smooth_tile', 'thin_wgrad'] and _smooth(plan) == ['flow_smooth_tile'] * 2
    value = [c for c in calls if c['grad'] is None]
    grads = [c for c in calls if c['grad'] is not None]
    assert [(c['guide_c'], c['weight']) for c in value] == [(3, 2.0), (0, 0.5)] and all(c['loss'] is not None for c in value)
    # two reverse recordings (plain and fused-optimiser plan), each: store, then add, into one gradient buffer
    assert [(c['guide_c'], c['weight'], c['acc']) for c in grads] == [(3, 2.0, 0), (0, 0.5, 1)] * 2
    assert all(c['loss'] is None and c['grad'] == m.flow_field.grad_ptr for c in grads)

    # the same two terms beside the L2 term: the fused head has stored the flow gradient, both add in the forward plan
    del calls[:]

    class TwoTermsAndL2(AppearanceFlowModel):
        def build_loss(self):
            self.loss = (tf_utils.euclidean_loss(self.gen, self.image1) + tf_utils.flow_smoothness_loss(self.flow_field, self.image1) * 2.0
                         + tf_utils.flow_smoothness_loss(self.flow_field) * 0.5)
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    m = _appflow(TwoTermsAndL2)
    assert [(c['guide_c'], c['acc'], c['loss'] is not None, c['grad'] == m.flow_field.grad_ptr) for c in calls] == [(3, 1, True, True), (0, 1, True, True)]
    assert not any(_smooth(plan) for plan in _labels(m)[1:])


def test_a_term_without_a_place_in_the_reverse_pass_is_an_error(lib):
    """A deferred term whose tensor no node of the graph produces must not vanish silently."""
    m = _appflow(flow_smoothness_weight=0.25, ssim_loss_weight=0.5)
    g = m.graph
    term = [t for _, t in g.loss_expr.terms if t.a is m.flow_field][0]
    pending = [(0.25, term)]
    g._flow_terms_all_placed([])
    with pytest.raises(RuntimeError, match='no place'):
        g._flow_terms_all_placed(pending)


def test_tinghui_and_the_angle_variants_take_the_switch(lib):
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for cls in (AppearanceFlowTinghui, AppFlowHighDimAngle, AppFlowLowDimAngle):
        fwd = _labels(_appflow(cls, flow_smoothness_weight=0.1))[0]
        assert fwd[-3:] == ['resample_loss', 'flow_smooth_tile', 'flow_smooth_final'], cls.__name__


def test_multiobject_adds_one_term_per_flow_head(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_SMOOTH
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': 0.1, 'combination_image': '', 'gen_sep_images': '',
            'masked_image_loss': '', 'fully_conv': ''}
    plain = _labels(MultiObjectAppFlow(conf, load_tfrec=False, device='cpu'))
    m = MultiObjectAppFlow(dict(conf, flow_smoothness_weight=0.5, flow_smoothness_edge=4.0), load_tfrec=False, device='cpu')
    heads = [name for name, _ in m.flow_heads]
    assert heads == ['dec_image1', 'dec_image1_only0', 'dec_image1_only1']
    terms = [(w, t) for w, t in m.graph.loss_expr.terms if t.kind == LOSS_SMOOTH]
    assert [w for w, _ in terms] == [0.5] * 3 and [t.a for _, t in terms] == [f for _, f in m.flow_heads]
    assert all(t.b is m.image1 and t.edge_alpha == 4.0 for _, t in terms)
    assert [s[0] for s in m.smoothness_terms] == heads
    fwd, bwd, _ = _labels(m)
    # dec_image1 keeps its fused head (one combined launch in the forward plan); the two masked heads run unfused: value in the
    # forward plan, gradient behind each resampler's backward
    assert fwd.count('flow_smooth_tile') == 3 and fwd.count('flow_smooth_final') == 3
    assert fwd.count('resample_loss') == plain[0].count('resample_loss') == 1
    assert bwd.count('flow_smooth_tile') == 2 and 'flow_smooth_final' not in bwd
    at = [i for i, l in enumerate(bwd) if l == 'flow_smooth_tile']
    assert all(bwd[i - 1] == 'resample_bwd' for i in at)
    assert [l for l in bwd if not l.startswith('flow_smooth')] == plain[1]


def test_models_without_a_flow_refuse_the_key_and_bad_values_are_refused(lib):
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd import multiobject_main_model
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError, match='flow_smoothness_weight'):
            cls({'batch_size': 2, 'flow_smoothness_weight': 0.5}, device='cpu')
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1, 'flow_smoothness_weight': 0.5}
    with pytest.raises(ValueError, match='flow_smoothness_weight'):
        Base_Prediction_Model(bp, load_tfrec=False, device='cpu')
    mo = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'combination_image': '', 'fully_conv': '', 'flow_smoothness_weight': 0.5}
    with pytest.raises(ValueError, match='flow_smoothness_weight'):
        multiobject_main_model.Base_Prediction_Model(mo, load_tfrec=False, device='cpu')
    # a multi-object configuration that builds no flow head must not swallow the key either
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    for conf in ({'use_depth': 0.1, 'combination_image': ''}, {'predict_target_masks': 1.0}):
        with pytest.raises(ValueError, match='flow_smoothness_weight'):
            MultiObjectAppFlow(dict({'batch_size': 2, 'learning_rate': 1e-4, 'fully_conv': '', 'flow_smoothness_weight': 0.5}, **conf),
                               load_tfrec=False, device='cpu')
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='flow_smoothness_weight'):
            _appflow(flow_smoothness_weight=bad)
        with pytest.raises(ValueError, match='flow_smoothness_edge'):
            _appflow(flow_smoothness_weight=0.1, flow_smoothness_edge=bad)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='flow_smoothness_eps'):
            _appflow(flow_smoothness_weight=0.1, flow_smoothness_eps=bad)


def test_evaluate_reports_the_unweighted_term_on_a_cpu_graph_only_when_the_switch_is_on(lib):
    """evaluate() needs forward passes, which a CPU graph cannot run: check the bookkeeping it reads."""
    assert not hasattr(_appflow(), 'smoothness_terms')
    assert [t[0] for t in _appflow(flow_smoothness_weight=0.1).smoothness_terms] == ['flow']
