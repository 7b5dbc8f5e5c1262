"""CPU-side checks of the SSIM training loss: the numpy twin (metrics.ssim_loss_host) against the metric it is defined from and
against float64 torch autograd over an independent F.conv2d restatement, the refusals of mv3d_ssim_loss (they come before any
launch, so they need no device), and the graph bookkeeping of conf['ssim_loss_weight'] on recorded plans."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamic_multiview_3d_amd import _lib, metrics

SHAPES = [(2, 45, 77, 3), (1, 11, 11, 2), (3, 40, 23, 1)]
FAMILIES = ('random', 'shift', 'blur')


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _pair(family, shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, shape).astype(np.float32)
    if family == 'random':
        return a, rng.uniform(0, 1, shape).astype(np.float32)
    if family == 'shift':
        return a, np.roll(a, 1, axis=2)
    p = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge')          # the 5-point blur
    b = (p[:, 1:-1, 1:-1] + p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:]) / np.float32(5)
    return a, b.astype(np.float32)


def torch_ssim_loss(a, b, max_val, weight=1.0):
    """(loss, d loss / d a) in float64 by autograd: the 11x11 outer-product window as one grouped F.conv2d."""
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64)
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    c = ta.shape[3]
    k = (g[:, None] * g[None, :])[None, None].repeat(c, 1, 1, 1)
    f = lambda x: F.conv2d(x.permute(0, 3, 1, 2), k, groups=c)
    mx, my, sab, s2 = f(ta), f(tb), f(ta * tb), f(ta * ta + tb * tb)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    s = ((2 * mx * my + c1) / (mx * mx + my * my + c1)) * ((2 * sab - 2 * mx * my + c2) / (s2 - mx * mx - my * my + c2))
    loss = weight * (1 - s.mean())
    loss.backward()
    return float(loss.detach()), ta.grad.numpy()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_value_is_one_minus_the_ssim_metric_and_gradient_matches_autograd(shape, family):
    a, b = _pair(family, shape, seed=sum(shape) + len(family))
    for max_val, weight in ((1.0, 1.0), (1.5, 0.25)):
        if max_val == 1.5:
            a, b = (a - np.float32(0.5)) * np.float32(1.5), (b - np.float32(0.5)) * np.float32(1.5)
        loss, grad = metrics.ssim_loss_host(a, b, max_val, np.float64, weight)
        assert grad.shape == shape and grad.dtype == np.float64
        want = weight * (1.0 - metrics.image_metrics_host(a, b, max_val)[:, metrics.SSIM].mean())
        assert abs(float(loss) - want) <= 1e-12
        tl, tg = torch_ssim_loss(a, b, max_val, weight)
        rel = np.linalg.norm(grad - tg) / np.linalg.norm(tg)
        print('%s %s max_val %.1f: loss %.6f, |loss - autograd| %.1e, gradient rel L2 %.1e' % (shape, family, max_val, loss, abs(loss - tl), rel))
        assert abs(float(loss) - tl) <= 1e-12
        assert rel <= 1e-10


def test_float32_twin_is_close_to_float64():
    """The float32 restatement -- the kernel's operation order -- stays near the float64 one on every family."""
    for family in FAMILIES:
        a, b = _pair(family, SHAPES[0], 7)
        l64, g64 = metrics.ssim_loss_host(a, b, 1.0, np.float64)
        l32, g32 = metrics.ssim_loss_host(a, b, 1.0, np.float32)
        assert g32.dtype == np.float32
        assert abs(float(l32) - float(l64)) <= 1e-5
        assert np.linalg.norm(g32 - g64) / np.linalg.norm(g64) <= 1e-4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_images_give_zero_loss_and_no_gradient(dtype):
    from dynamic_multiview_3d_amd.train import SyntheticData
    weight = 0.5
    for a in (np.random.default_rng(1).uniform(0, 1, (2, 19, 23, 3)).astype(np.float32),
              SyntheticData._images(np.random.default_rng(2), (2, 40, 33, 3)).astype(np.float32)):      # flat regions: B2 ~ c2
        loss, grad = metrics.ssim_loss_host(a, a.copy(), 1.0, dtype, weight)
        assert float(loss) == 0.0
        assert np.abs(grad).max() <= 4e-6 * weight


def test_operand_checks():
    a = np.zeros((1, 12, 12, 1), np.float32)
    with pytest.raises(ValueError, match='shape'):
        metrics.ssim_loss_host(a, a[:, :11])
    with pytest.raises(ValueError, match='window'):
        metrics.ssim_loss_host(a[:, :10], a[:, :10])
    with pytest.raises(ValueError, match='max_val'):
        metrics.ssim_loss_host(a, a, max_val=0.0)
    with pytest.raises(ValueError, match='weight'):
        metrics.ssim_loss_host(a, a, weight=float('nan'))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_ssim_loss', 'mv3d_ssim_loss_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.ssim_loss) and callable(lib.raw_ssim_loss)
    assert lib.ssim_loss_workspace_bytes(2, 45, 77, 3) == 256                  # 2 x 2 x 3 tiles x 8 bytes, rounded up to 256
    assert lib.ssim_loss_workspace_bytes(64, 128, 128, 3) == 64 * 16 * 8
    assert lib.ssim_loss_workspace_bytes(2, 10, 77, 3) == 0 and lib.ssim_loss_workspace_bytes(2, 45, 77, 5) == 0


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns its code and names the argument; none of them touches a pointer, so made-up addresses do."""
    ok = dict(N=2, H=16, W=16, C=3, a=0x1000, a_ld=3, b=0x2000, b_ld=3, max_val=1.0, weight=1.0, loss=0x3000, grad=0x5000, grad_ld=3,
              acc=0, ws=0x4000, ws_bytes=4096)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_ssim_loss(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['max_val'], v['weight'],
                                 v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], None)
    inf, nan = float('inf'), float('nan')
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(H=10), -1, 'H'), (dict(W=10), -1, 'W'), (dict(C=5), -1, 'C'), (dict(C=0), -1, 'C'),
                           (dict(H=32769), -1, 'H'), (dict(W=32769), -1, 'W'), (dict(N=1 << 21, H=32768, W=32768), -1, 'tiles'),
                           (dict(a_ld=2), -1, 'a_ld'), (dict(b_ld=2), -1, 'b_ld'), (dict(grad_ld=2), -1, 'grad_ld'),
                           (dict(acc=2), -1, 'grad_accumulate'), (dict(acc=-1), -1, 'grad_accumulate'),
                           (dict(max_val=0.0), -1, 'max_val'), (dict(max_val=inf), -1, 'max_val'), (dict(max_val=nan), -1, 'max_val'),
                           (dict(weight=inf), -1, 'weight'), (dict(weight=nan), -1, 'weight'),
                           (dict(a=None), -1, 'a is null'), (dict(b=None), -1, 'b is null'), (dict(loss=None), -1, 'loss_accum is null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(a=0x1002), -1, 'aligned'), (dict(grad=0x5001), -1, 'aligned'),
                           (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x4008), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error() and 'mv3d_ssim_loss' in lib.last_error(), (kw, lib.last_error())
    # the order of the checks: shape before strides before values before pointers before the workspace
    assert call(N=0, a_ld=2) == -1 and 'N' in lib.last_error()
    assert call(a_ld=2, max_val=0.0) == -1 and 'a_ld' in lib.last_error()
    assert call(weight=nan, a=None) == -1 and 'weight' in lib.last_error()
    assert call(a=None, ws_bytes=0) == -1 and 'a is null' in lib.last_error()


# ------------------------------------------------------------------------------------------------ graph bookkeeping (recorded plans)
def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _appflow(**extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return AppearanceFlowModel(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def test_switch_absent_or_zero_records_the_same_plans(lib):
    absent, zero = _labels(_appflow()), _labels(_appflow(ssim_loss_weight=0.0))
    assert absent == zero
    assert 'resample_loss' in absent[0] and not any(l.startswith('ssim_loss') for plan in absent if plan for l in plan)


def test_switch_on_adds_the_ssim_launches_after_the_pixel_loss(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_SSIM, ResampleNode
    m = _appflow(ssim_loss_weight=0.5)
    fwd, bwd, _ = _labels(m)
    assert 'resample_loss' not in fwd                                  # gen now feeds two terms: the fused head is gone
    assert fwd[-4:] == ['resample_fwd', 'pixel_loss', 'ssim_loss_tile', 'ssim_loss_final']
    assert bwd[0] == 'resample_bwd'
    assert [n.fused_loss for n in m.graph.nodes if isinstance(n, ResampleNode)] == [None]
    (w2, t2), (ws, ts) = m.graph.loss_expr.terms
    assert (w2, t2.kind) == (1.0, 2) and (ws, ts.kind, ts.max_val) == (0.5, LOSS_SSIM, 1.0)
    assert ts.a is m.gen and ts.b is m.image1
    assert ts.ws.numel() == lib.ssim_loss_workspace_bytes(2, 128, 128, 3) and t2.ws is None


def test_base_prediction_and_multiobject_add_the_term_to_the_colour_image_only(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_SSIM
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    plain = _labels(Base_Prediction_Model(conf, load_tfrec=False, device='cpu'))
    m = Base_Prediction_Model(dict(conf, ssim_loss_weight=0.25), load_tfrec=False, device='cpu')
    fwd = _labels(m)[0]
    assert fwd == plain[0] + ['ssim_loss_tile', 'ssim_loss_final']    # both pixel losses first, then the SSIM term
    ssim = [(w, t) for w, t in m.graph.loss_expr.terms if t.kind == LOSS_SSIM]
    assert len(ssim) == 1 and ssim[0][0] == 0.25 and ssim[0][1].a is m.gen_image1 and ssim[0][1].b is m.image1
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': 0.1, 'combination_image': '', 'gen_sep_images': '',
            'masked_image_loss': '', 'fully_conv': '', 'ssim_loss_weight': 0.5}
    m = MultiObjectAppFlow(conf, load_tfrec=False, device='cpu')
    ssim = [(w, t) for w, t in m.graph.loss_expr.terms if t.kind == LOSS_SSIM]
    assert len(ssim) == 1 and ssim[0][1].a is m.gen_image1 and ssim[0][1].b is m.image1
    assert _labels(m)[0].count('ssim_loss_tile') == 1


def test_ssim_alone_on_a_sampled_image_does_not_fuse(lib):
    """A gen that feeds only an SSIM term must not go to the fused sampler + pixel-loss launch."""
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf

    class SsimOnly(AppearanceFlowModel):
        def build_loss(self):
            self.loss = tf_utils.ssim_loss(self.image1, self.gen, 1.0) * 2.0       # target first: the op swaps the operands
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    m = SsimOnly({'batch_size': 2, 'learning_rate': 1e-4}, load_tfrec=False, device='cpu')
    fwd = _labels(m)[0]
    assert 'resample_loss' not in fwd and 'pixel_loss' not in fwd and 'fill' not in fwd
    assert fwd[-3:] == ['resample_fwd', 'ssim_loss_tile', 'ssim_loss_final']
    (w, t), = m.graph.loss_expr.terms
    assert w == 2.0 and t.a is m.gen and t.b is m.image1


def test_op_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph
    with Graph(device='cpu') as g:
        x = g.placeholder([2, 16, 16, 3], 'x')
        y = g.placeholder([2, 16, 16, 3], 'y')
        m = g.placeholder([2, 16, 16, 1], 'm')
        small = g.placeholder([2, 10, 16, 3], 's')
        with pytest.raises(NotImplementedError):
            tf_utils.ssim_loss(tf_utils.multiply(x, m), y)
        with pytest.raises(NotImplementedError):
            tf_utils.ssim_loss(x, tf_utils.scale(y, 0.75))
        with pytest.raises(ValueError):
            tf_utils.ssim_loss(small, small)
        with pytest.raises(ValueError):
            tf_utils.ssim_loss(x, m)
        e = tf_utils.ssim_loss(x, y, 1.5) * 0.5 + tf_utils.euclidean_loss(x, y)
        assert [(w, t.kind) for w, t in e.terms] == [(0.5, 3), (1.0, 2)] and e.terms[0][1].max_val == 1.5


def test_models_without_the_term_refuse_the_key(lib):
    from dynamic_multiview_3d_amd import mv3d
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError, match='ssim_loss_weight'):
            cls({'batch_size': 2, 'ssim_loss_weight': 0.5}, device='cpu')
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='ssim_loss_weight'):
            _appflow(ssim_loss_weight=bad)
