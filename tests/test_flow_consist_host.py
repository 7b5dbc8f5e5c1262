"""Forward-backward flow consistency without a GPU: the numpy twin against autograd and against the oracle's sampler, the C ABI's
refusals, the graph op, the conf switches on recorded plans, and evaluate()'s bookkeeping on a CPU graph.

Measured on the CPU (tests/flow_consist_cases.py, seed 7, eps 1e-3, weight 0.7): the float32 twin's gradient deviates from the float64
twin's by 6e-10 .. 2.5e-8 absolute (max |grad| 5e-5 .. 2.4e-2, i.e. 1e-6 .. 1e-4 of it: the residual is a difference of numbers 20 to
1000 times its size); the value by 2.5e-9 .. 9e-7 (values 0.11 .. 22)."""
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import flow_consist_cases as FC
from tests.test_flow_smooth_host import _labels, _recorded

EPS, WEIGHT = 1e-3, 0.7


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    return FC.all_cases()


# ------------------------------------------------------------------------------------------------ numpy twin
def torch_consistency(flow, eps, weight):
    """The definition restated in plain torch float64 with explicit floor, gather and weights: (loss, grad, value, valid share)."""
    f = torch.tensor(np.asarray(flow, np.float64), requires_grad=True)
    n, h, w, _ = f.shape
    eps = float(np.float32(eps))
    partner = torch.roll(f, -(n // 2), 0)                                       # partner[n] = f[(n + N/2) mod N]
    ii = torch.arange(h, dtype=torch.float64)[None, :, None]
    jj = torch.arange(w, dtype=torch.float64)[None, None, :]
    x, y = f[..., 0] + ii, f[..., 1] + jj                                       # x: the column, from the ROW index; y: the row
    valid = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    xs, ys = torch.where(valid, x, torch.zeros_like(x)), torch.where(valid, y, torch.zeros_like(y))
    fx, fy = torch.floor(xs).detach(), torch.floor(ys).detach()
    dx, dy = ((fx + 1) - xs)[..., None], ((fy + 1) - ys)[..., None]
    ix, iy = fx.long(), fy.long()
    b = torch.arange(n)[:, None, None].expand(n, h, w)

    def tap(yy, xx):                                                            # index W or H: weight 0, reads 0
        ok = ((yy < h) & (xx < w))[..., None]
        return partner[b, yy.clamp(max=h - 1), xx.clamp(max=w - 1)] * ok
    s = dx * dy * tap(iy, ix) + (1 - dx) * (1 - dy) * tap(iy + 1, ix + 1) + dx * (1 - dy) * tap(iy + 1, ix) + (1 - dx) * dy * tap(iy, ix + 1)
    r0, r1 = f[..., 0] + s[..., 1], f[..., 1] + s[..., 0]
    phi = torch.sqrt(r0 * r0 + r1 * r1 + eps * eps) - eps
    value = (phi * valid).sum() / (n * h * w)
    loss = float(np.float32(weight)) * value
    loss.backward()
    return float(loss.detach()), f.grad.numpy(), float(value.detach()), float(valid.double().mean())


def test_float64_twin_matches_autograd(cases):
    for name, flow in cases:
        loss, grad, value, share = metrics.flow_consistency_host(flow, EPS, np.float64, WEIGHT)
        tl, tg, tv, ts = torch_consistency(flow, EPS, WEIGHT)
        scale = np.abs(tg).max()
        assert scale > 0, name
        assert np.abs(grad - tg).max() <= 1e-9 * scale, (name, np.abs(grad - tg).max() / scale)
        assert abs(float(value) - tv) <= 1e-12 * max(tv, 1.0) and abs(float(loss) - tl) <= 1e-12 * max(tl, 1.0), name
        assert float(share) == ts == FC.valid_fraction(flow), name


def test_float32_twin_is_close_to_float64(cases):
    for name, flow in cases:
        l64, g64, v64, s64 = metrics.flow_consistency_host(flow, EPS, np.float64, WEIGHT)
        l32, g32, v32, s32 = metrics.flow_consistency_host(flow, EPS, np.float32, WEIGHT)
        assert g32.dtype == np.float32 and type(l32) is np.float32 and type(v32) is np.float32
        # the measured deviations are in the module docstring; the bars leave a factor of 10 above the largest of them
        assert np.abs(g32 - g64).max() <= 1e-3 * np.abs(g64).max(), (name, np.abs(g32 - g64).max() / np.abs(g64).max())
        assert abs(float(v32) - float(v64)) <= 1e-6 * float(v64), name
        assert float(s32) == float(np.float32(s64)), name                      # the cell and the validity are the same in both


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_convention_anchor(dtype):
    """F = (a, b) against G = (-b, -a) is an exact inverse pair under the transposed convention -- the oracle's sampler says so on
    an image -- and the term is exactly 0 there; G = -F is not."""
    from oracle import ops
    n, h, a, b = 2, 16, 3.0, -2.0
    flow = np.zeros((n, h, h, 2), dtype)
    flow[0], flow[1] = (a, b), (-b, -a)
    loss, grad, value, share = metrics.flow_consistency_host(flow, EPS, dtype, 2.0)
    assert float(loss) == 0.0 and float(value) == 0.0 and not grad.any()
    assert 0.4 < float(share) < 1.0                                             # the offsets push a margin of pixels out of the image
    img = np.random.default_rng(3).uniform(0, 1, (1, h, h, 3)).astype(dtype)
    there = ops.resampler_fwd(img, ops.warp_pts_layer(flow[:1]))
    back = ops.resampler_fwd(there, ops.warp_pts_layer(flow[1:]))
    m = 4                                                                       # |a|, |b| < m: the interior never left the image
    assert np.array_equal(back[:, m:-m, m:-m], img[:, m:-m, m:-m])
    wrong = flow.copy()
    wrong[1] = (-a, -b)
    back = ops.resampler_fwd(there, ops.warp_pts_layer(wrong[1:]))
    assert np.abs(back[:, m:-m, m:-m] - img[:, m:-m, m:-m]).max() > 0.5
    assert float(metrics.flow_consistency_host(wrong, EPS, dtype)[2]) > 1.0     # |r| = |(a - b, b - a)| ~ 7 pixels


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_all_invalid_input_gives_zero(dtype):
    flow = np.full((2, 8, 8, 2), 100.0, dtype)
    flow[1, 2, 3] = (np.nan, np.inf)
    loss, grad, value, share = metrics.flow_consistency_host(flow, EPS, dtype)
    assert float(loss) == 0.0 and float(value) == 0.0 and float(share) == 0.0 and not grad.any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_non_finite_partner_value_stays_visible_and_is_not_scattered(dtype):
    """NaN in flow[m] at a tap of a valid pixel: that pixel's phi and psi are NaN, so the value and its own gradient are; the
    entries it would scatter are dropped, so nothing else turns NaN."""
    flow = np.zeros((2, 8, 8, 2), dtype)
    flow[0] += 0.5                                                              # every pixel samples the four pixels around it
    flow[1, 3, 4, 0] = np.nan                                                   # own flow NaN: that pixel is invalid
    loss, grad, value, share = metrics.flow_consistency_host(flow, EPS, dtype)
    assert np.isnan(float(value)) and np.isnan(float(loss)) and 0 < float(share) < 1
    bad = np.isnan(grad).any(axis=-1)
    assert not bad[1].any()                                                     # nothing non-finite was scattered into the partner
    assert sorted(zip(*np.nonzero(bad[0]))) == [(3, 2), (3, 3), (4, 2), (4, 3)]  # x = i + 0.5 is the column, y = j + 0.5 the row


def test_operand_checks():
    f = np.zeros((2, 4, 4, 2), np.float32)
    with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
        metrics.flow_consistency_host(f[..., :1])
    with pytest.raises(ValueError, match='even N'):
        metrics.flow_consistency_host(np.zeros((3, 4, 4, 2), np.float32))
    with pytest.raises(ValueError, match='even N'):
        metrics.flow_consistency_host(f[:0])
    with pytest.raises(ValueError, match='H == W'):
        metrics.flow_consistency_host(np.zeros((2, 4, 5, 2), np.float32))
    with pytest.raises(ValueError, match='H == W'):
        metrics.flow_consistency_host(f[:, :1, :1])
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_consistency_host(f, eps=0.0)
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_consistency_host(f, eps=float('nan'))
    with pytest.raises(ValueError, match='weight'):
        metrics.flow_consistency_host(f, weight=float('inf'))
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_consistency_host(f, eps=1e-20)                             # eps * eps underflows in float32
    assert float(metrics.flow_consistency_host(f, eps=2.0 ** -63, dtype=np.float32)[0]) == 0.0
    with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
        metrics.flow_consistency(torch.zeros(2, 4, 4, 3))                       # the device mirror makes the same checks first
    with pytest.raises(ValueError, match='even N'):
        metrics.flow_consistency(torch.zeros(3, 4, 4, 2))
    with pytest.raises(ValueError, match='eps'):
        metrics.flow_consistency(torch.zeros(2, 4, 4, 2), eps=-1.0)
    with pytest.raises(_lib.Mv3dError, match='GPU'):
        metrics.flow_consistency(torch.zeros(2, 4, 4, 2))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_flow_consistency', 'mv3d_flow_consistency_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.flow_consistency) and callable(lib.raw_flow_consistency)
    assert 'mv3d_flow_consistency' in header.split('int mv3d_loss_overwrite_next(void);')[0].rsplit('/*', 1)[1]
    # the int64 plane [N,H,W,2], the float plane [N,H,W,2] of the gathered part and 2 sums x 8 bytes per 16 x 64 tile, each
    # rounded up to 256
    assert lib.flow_consistency_workspace_bytes(2, 2, 2) == 256 + 256 + 256
    assert lib.flow_consistency_workspace_bytes(64, 128, 128) == 64 * 128 * 128 * 16 + 64 * 128 * 128 * 8 + 64 * 8 * 2 * 16
    for bad in ((1, 4, 4), (3, 4, 4), (0, 4, 4), (2, 4, 5), (2, 1, 1), (2, 40000, 40000)):
        assert lib.flow_consistency_workspace_bytes(*bad) == 0, bad


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns its code, names the argument and records nothing; none touches a pointer, so made-up addresses do."""
    ok = dict(N=2, H=16, W=16, flow=0x1000, flow_ld=2, eps=1e-3, weight=1.0, loss=0x3000, stats=0x3100, grad=0x5000, grad_ld=2, acc=0,
              ws=0x10000, ws_bytes=1 << 16)

    def call(**kw):
        v = dict(ok, **kw)
        return _recorded(lib, lambda: lib.raw_flow_consistency(
            v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['eps'], v['weight'], v['loss'], v['stats'], v['grad'], v['grad_ld'],
            v['acc'], v['ws'], v['ws_bytes'], None))
    inf, nan = float('inf'), float('nan')
    need = lib.flow_consistency_workspace_bytes(2, 16, 16)
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(N=1), -1, 'N'), (dict(N=3), -1, 'N'), (dict(W=17), -1, 'differ'), (dict(H=1, W=1), -1, 'H'),
                           (dict(H=40000, W=40000), -1, 'H'), (dict(N=1 << 30, H=1 << 15, W=1 << 15), -1, 'tiles'),
                           (dict(N=1 << 10, H=1 << 15, W=1 << 15, flow_ld=1 << 30), -1, 'overflow'),
                           (dict(flow_ld=1), -1, 'flow_ld'), (dict(grad_ld=1), -1, 'grad_ld'),
                           (dict(acc=2), -1, 'grad_accumulate'), (dict(acc=-1), -1, 'grad_accumulate'),
                           (dict(eps=0.0), -1, 'eps'), (dict(eps=-1.0), -1, 'eps'), (dict(eps=inf), -1, 'eps'), (dict(eps=nan), -1, 'eps'), (dict(eps=1e-20), -1, 'underflows'),
                           (dict(weight=inf), -1, 'weight'), (dict(weight=nan), -1, 'weight'),
                           (dict(flow=None), -1, 'flow is null'), (dict(loss=None, stats=None, grad=None), -1, 'both null'),
                           (dict(loss=None), -1, 'stats without loss_accum'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(flow=0x1002), -1, 'aligned'), (dict(stats=0x3101), -1, 'aligned'),
                           (dict(grad=0x5001), -1, 'aligned'), (dict(loss=0x3002), -1, 'aligned'),
                           (dict(ws_bytes=need - 1), -3, 'workspace'), (dict(ws=0x10008), -3, 'aligned')]:
        rc, labels = call(**kw)
        assert rc == code and labels == [], (kw, rc, labels)
        assert word in lib.last_error() and 'mv3d_flow_consistency' in lib.last_error(), (kw, lib.last_error())
    # what is accepted, and what each form records
    three = ['flow_consist_tile', 'flow_consist_scatter', 'flow_consist_final']
    assert call(ws_bytes=need) == (0, three)
    assert call(stats=None) == (0, three)
    assert call(grad=None) == (0, ['flow_consist_tile', 'flow_consist_final'])          # value only: no scatter
    assert call(loss=None, stats=None) == (0, three)                                    # gradient only: the final launch converts
    assert call(flow=0x1004, flow_ld=3, grad=0x5004, grad_ld=4)[0] == 0                 # channel-slice views


# ------------------------------------------------------------------------------------------------ graph op
def test_op_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, LOSS_CONSIST, FLOW_TERMS
    assert LOSS_CONSIST in FLOW_TERMS
    with Graph(device='cpu') as g:
        img = g.placeholder([2, 16, 16, 3], 'img')
        odd = g.placeholder([3, 16, 16, 3], 'odd')
        wide = g.placeholder([2, 16, 8, 3], 'wide')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
        with pytest.raises(ValueError, match='not differentiated'):
            tf_utils.flow_consistency_loss(g.placeholder([2, 16, 16, 2], 'fed'))
        with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
            tf_utils.flow_consistency_loss(tf_utils.conv2d_msra(img, 3, 3, 3, 1, 1, 'three'))
        with pytest.raises(ValueError, match='even N'):
            tf_utils.flow_consistency_loss(tf_utils.conv2d_msra(odd, 2, 3, 3, 1, 1, 'oddflow'))
        with pytest.raises(ValueError, match='H == W'):
            tf_utils.flow_consistency_loss(tf_utils.conv2d_msra(wide, 2, 3, 3, 1, 1, 'wideflow'))
        with pytest.raises(NotImplementedError):
            tf_utils.flow_consistency_loss(tf_utils.scale(flow, 0.5))
        with pytest.raises(ValueError, match='eps'):
            tf_utils.flow_consistency_loss(flow, eps=0.0)
        e = tf_utils.flow_consistency_loss(flow, 1e-2) * 0.5 + tf_utils.flow_consistency_loss(flow)
        assert [(w, t.kind) for w, t in e.terms] == [(0.5, LOSS_CONSIST), (1.0, LOSS_CONSIST)]
        t0, t1 = e.terms[0][1], e.terms[1][1]
        assert (t0.a, t0.b, t0.eps) == (flow, None, float(np.float32(1e-2))) and t1.eps == float(np.float32(1e-3))


# ------------------------------------------------------------------------------------------------ conf switches on recorded plans
ON = dict(pair_swap=True, flow_consistency_weight=0.25)
THREE = ['flow_consist_tile', 'flow_consist_scatter', 'flow_consist_final']


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def _consist(plan):
    return [l for l in plan if l.startswith('flow_consist')]


def test_switch_absent_zero_or_none_records_the_same_plans(lib):
    absent = _labels(_appflow())
    assert absent == _labels(_appflow(flow_consistency_weight=0.0)) == _labels(_appflow(flow_consistency_weight=None))
    assert absent == _labels(_appflow(flow_consistency_weight=0, flow_consistency_eps=0.1)) == _labels(_appflow(pair_swap=True))
    assert absent == _labels(_appflow(pair_swap=True, flow_consistency_weight=0)) == _labels(_appflow(pair_swap=False)) == _labels(_appflow(pair_swap=None))
    assert 'resample_loss' in absent[0] and not any(_consist(plan) for plan in absent if plan)
    m = _appflow(pair_swap=True, flow_consistency_weight=0)
    assert not hasattr(m, 'consistency_terms') and all(t.ws is None for _, t in m.graph.loss_expr.terms)


def test_switch_on_keeps_the_head_fused_and_adds_the_terms_launches_behind_it(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_CONSIST, ResampleNode
    absent = _labels(_appflow())
    m = _appflow(**ON)
    fwd, bwd, fused = _labels(m)
    assert fwd == absent[0] + THREE and fwd[-4] == 'resample_loss'
    assert bwd == absent[1] and fused == absent[2]                       # nothing is added to the reverse plans
    assert [n.fused_loss is not None for n in m.graph.nodes if isinstance(n, ResampleNode)] == [True]
    (w2, t2), (wc, tc) = m.graph.loss_expr.terms
    assert (w2, t2.kind) == (1.0, 2) and (wc, tc.kind, tc.eps) == (0.25, LOSS_CONSIST, float(np.float32(1e-3)))
    assert tc.a is m.flow_field and tc.b is None
    assert tc.ws.numel() == lib.flow_consistency_workspace_bytes(2, 128, 128) and t2.ws is None
    assert m.consistency_terms == [('flow', m.flow_field, 1e-3)]
    assert _appflow(flow_consistency_eps=0.01, **ON).graph.loss_expr.terms[1][1].eps == float(np.float32(0.01))


def test_an_unfused_head_defers_the_gradient_into_the_reverse_plan(lib, monkeypatch):
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    plain = _labels(_appflow())
    m = _appflow(**ON)
    fwd, bwd, fused = _labels(m)
    assert 'resample_loss' not in fwd
    assert fwd == plain[0] + ['flow_consist_tile', 'flow_consist_final']           # the value only
    # the gradient call right behind the resampler's backward, in front of the flow_field deconvolution's backward
    assert bwd == plain[1][:1] + THREE + plain[1][1:] and fused == plain[2][:1] + THREE + plain[2][1:]
    assert bwd[0] == 'resample_bwd' and bwd[4] == 'thin_wgrad'
    assert m.graph.grad_buckets[0][0] >= 5


def test_the_order_with_the_smoothness_and_multiscale_terms(lib, monkeypatch):
    both = dict(flow_smoothness_weight=0.25, multiscale_loss_levels=2)
    base = _labels(_appflow(**both))
    fwd, bwd, fused = _labels(_appflow(**dict(both, **ON)))
    assert fwd == base[0] + THREE and bwd == base[1] and fused == base[2]
    flow_terms = [l for l in fwd if l.startswith(('flow_smooth', 'multiscale', 'flow_consist'))]
    assert flow_terms[:2] == ['flow_smooth_tile', 'flow_smooth_final'] and flow_terms[-3:] == THREE
    assert all(l.startswith('multiscale') for l in flow_terms[2:-3]) and len(flow_terms) > 5
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    base = _labels(_appflow(**both))
    fwd, bwd, fused = _labels(_appflow(**dict(both, **ON)))
    assert fwd == base[0] + ['flow_consist_tile', 'flow_consist_final']
    for plan, ref in ((bwd, base[1]), (fused, base[2])):
        at = plan.index('flow_consist_tile')
        assert plan[at:at + 3] == THREE and plan[:at] + plan[at + 3:] == ref
        assert plan[0] == 'resample_bwd' and plan[at - 1].startswith('multiscale') and plan[1] == 'flow_smooth_tile'


def test_the_family_takes_the_switch(lib):
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for cls in (AppearanceFlowTinghui, AppFlowHighDimAngle, AppFlowLowDimAngle):
        fwd = _labels(_appflow(cls, **ON))[0]
        assert fwd[-4:] == ['resample_loss'] + THREE, cls.__name__


def test_conf_refusals(lib):
    from dynamic_multiview_3d_amd import mv3d, multiobject_main_model
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    with pytest.raises(ValueError, match='pair_swap'):
        _appflow(flow_consistency_weight=0.25)                           # the weight without the pair-swapped feed
    with pytest.raises(ValueError, match='pair_swap'):
        _appflow(flow_consistency_weight=0.25, pair_swap=False)
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError, match='pair_swap'):
            cls(dict({'batch_size': 2}, **ON), device='cpu')
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    with pytest.raises(ValueError, match='flow_consistency_weight'):
        Base_Prediction_Model(dict(bp, **ON), load_tfrec=False, device='cpu')
    Base_Prediction_Model(dict(bp, pair_swap=True), load_tfrec=False, device='cpu')       # the key alone is an augmentation
    mo = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'combination_image': '', 'fully_conv': ''}
    for cls in (multiobject_main_model.Base_Prediction_Model, MultiObjectAppFlow):
        with pytest.raises(ValueError, match='pair_swap'):
            cls(dict(mo, **ON), load_tfrec=False, device='cpu')
    for bad in (True, False, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='flow_consistency_weight'):
            _appflow(pair_swap=True, flow_consistency_weight=bad)
    for bad in (0.0, -1.0, float('nan'), True, 1e-20):
        with pytest.raises(ValueError, match='flow_consistency_eps'):
            _appflow(flow_consistency_eps=bad, **ON)


def test_evaluate_reports_the_two_names_on_a_cpu_graph_only_when_the_switch_is_on(lib, monkeypatch):
    """A CPU graph cannot run a forward pass, so forward() is replaced by one that fills the tensors evaluate() reads; the numpy
    form then scores them."""
    flow = np.zeros((2, 128, 128, 2), np.float32)
    flow[0], flow[1] = (3.0, -2.0), (-1.0, 2.0)                          # r = (3 + 2, -2 - 1) wherever the pixel is valid

    class Data:
        def next(self):
            return {}

    def run(m):
        def forward(**feeds):
            m.flow_field.set(flow)
            m.gen.set(np.zeros(m.gen.shape, np.float32))
            m.image1.set(np.full(m.image1.shape, 0.5, np.float32))
            return torch.zeros(())
        monkeypatch.setattr(m, 'forward', forward)
        return m.evaluate(Data(), num_batches=2)
    off = run(_appflow(pair_swap=True))
    assert not any('consistency' in k for k in off)
    on = run(_appflow(**ON))
    assert set(on) == set(off) | {'flow/consistency', 'flow/consistency_valid'}
    _, _, value, share = metrics.flow_consistency_host(flow, 1e-3)
    assert on['flow/consistency'] == float(value) and on['flow/consistency_valid'] == float(share)
    assert 0.9 < on['flow/consistency_valid'] < 1.0 and abs(on['flow/consistency'] - np.sqrt(34.0) * on['flow/consistency_valid']) < 1e-2
