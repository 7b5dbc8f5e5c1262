"""CPU-side checks of the census training loss: the numpy twin (metrics.census_loss_host) against central finite differences and
against float64 torch autograd over an independent restatement, its properties, the guard of the GPU parity rule, the refusals of
mv3d_census_loss (they come before any launch, so they need no device), conf['census_loss_*'] and the graph bookkeeping on
recorded plans, and evaluate()'s host path.

A graph built without a GPU records its plans but cannot run them, so what a model's loss becomes with the key set is checked
here on the recorded plans and terms (what is launched, in which order, with which weight and arguments) and in numbers on the
GPU (tests/test_gpu_census_model.py)."""
import os
import types

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import census_cases

RADII = (1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, shape), rng.uniform(0, 1, shape)


def torch_census_loss(a, b, max_val, weight, radius, eps):
    """(loss, d loss / d a) in float64 by autograd, from the formulas for g, t, dist and rho only."""
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64)
    n, h, w, c = ta.shape
    r = radius
    hv, wv = h - 2 * r, w - 2 * r
    ga, gb = ta.mean(dim=3) * (255.0 / max_val), tb.mean(dim=3) * (255.0 / max_val)

    def t(g, dy, dx):
        d = g[:, r + dy:r + dy + hv, r + dx:r + dx + wv] - g[:, r:r + hv, r:r + wv]
        return d / torch.sqrt(0.81 + d ** 2)
    terms = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy or dx:
                e = (t(ga, dy, dx) - t(gb, dy, dx)) ** 2
                terms.append(e / (0.1 + e))
    dist = torch.stack(terms).mean(dim=0)
    rho = torch.sqrt(dist + eps ** 2) - eps
    loss = weight * rho.mean()
    loss.backward()
    return float(loss.detach()), ta.grad.numpy()


@pytest.mark.parametrize("radius", RADII)
def test_float64_twin_matches_central_finite_differences(radius):
    shape = (1, 12, 13, 2)
    a, b = _random_pair(shape, 10 + radius)
    eps32 = float(np.float32(0.01))
    loss, grad = metrics.census_loss_host(a, b, 1.0, np.float64, 1.0, radius, eps32)
    value = lambda x: float(metrics.census_loss_host(x, b, 1.0, np.float64, 1.0, radius, eps32)[0])
    h = 1e-6
    fd = np.zeros(shape)
    for idx in np.ndindex(shape):
        hi, lo = a.copy(), a.copy()
        hi[idx] += h
        lo[idx] -= h
        fd[idx] = (value(hi) - value(lo)) / (2 * h)
    rel = np.linalg.norm(fd - grad) / np.linalg.norm(fd)
    print('radius %d: loss %.6f, gradient against central differences rel L2 %.1e' % (radius, loss, rel))
    assert grad.shape == shape and grad.dtype == np.float64
    assert rel <= 1e-6


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", [(2, 15, 19, 3), (1, 7, 7, 2), (3, 20, 9, 1), (1, 9, 8, 4)])
def test_float64_twin_matches_autograd_over_an_independent_restatement(shape, radius):
    a, b = _random_pair(shape, sum(shape) + radius)
    a, b = a.astype(np.float32), b.astype(np.float32)
    for max_val, weight, eps in ((1.0, 1.0, 0.01), (1.5, 0.25, 0.05)):
        if max_val == 1.5:
            a, b = (a - np.float32(0.5)) * np.float32(1.5), (b - np.float32(0.5)) * np.float32(1.5)
        loss, grad = metrics.census_loss_host(a, b, max_val, np.float64, weight, radius, eps)
        tl, tg = torch_census_loss(a, b, max_val, weight, radius, float(np.float32(eps)))
        rel = np.linalg.norm(grad - tg) / np.linalg.norm(tg)
        print('%s r %d max_val %.1f: loss %.6f, |loss - autograd| / loss %.1e, gradient rel L2 %.1e' % (shape, radius, max_val, loss, abs(loss - tl) / tl, rel))
        assert abs(float(loss) - tl) <= 1e-10 * abs(tl)
        assert rel <= 1e-10


def test_default_dtype_is_float32_and_defaults_are_radius_3_eps_001():
    a, b = _random_pair((1, 9, 9, 3), 5)
    loss, grad = metrics.census_loss_host(a, b)
    assert loss.dtype == np.float32 and grad.dtype == np.float32
    want = metrics.census_loss_host(a, b, 1.0, np.float32, 1.0, 3, 0.01)
    assert loss == want[0] and np.array_equal(grad, want[1])
    assert [len(metrics.census_offsets(r)) for r in RADII] == [8, 24, 48]
    assert metrics.census_offsets(1)[:4] == [(-1, -1), (-1, 0), (-1, 1), (0, -1)]        # row-major: dy outer, dx inner


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_images_give_exactly_zero(dtype):
    from dynamic_multiview_3d_amd.train import SyntheticData
    for radius in RADII:
        for a in (np.random.default_rng(1).uniform(0, 1, (2, 19, 23, 3)).astype(np.float32),
                  SyntheticData._images(np.random.default_rng(2), (2, 40, 33, 3)).astype(np.float32)):
            loss, grad = metrics.census_loss_host(a, a.copy(), 1.0, dtype, 0.5, radius)
            assert float(loss) == 0.0 and not np.any(grad)


def test_properties_of_the_float64_twin():
    a, b = _random_pair((2, 17, 14, 3), 21)
    for radius in RADII:
        loss, grad = metrics.census_loss_host(a, b, 1.0, np.float64, 1.0, radius)
        assert 0.0 <= float(loss) < 1.0
        # exactly invariant to an additive brightness change (up to the rounding of a + const)
        shifted = float(metrics.census_loss_host(a + 0.125, b, 1.0, np.float64, 1.0, radius)[0])
        assert abs(shifted - float(loss)) <= 1e-12
        # the gradient is the same for every channel
        assert np.array_equal(grad[..., 0], grad[..., 1]) and np.array_equal(grad[..., 0], grad[..., 2])
    # Pixels outside the valid region receive a gradient as neighbours of valid pixels, and only so: every pixel of an image lies
    # within r of the valid region, so the border ring is not zero ...
    a, b = _random_pair((1, 9, 11, 2), 22)
    for radius in RADII:
        _, grad = metrics.census_loss_host(a, b, 1.0, np.float64, 1.0, radius)
        ring = np.ones((9, 11), bool)
        ring[radius:9 - radius, radius:11 - radius] = False
        assert np.any(grad[0][ring] != 0)
    # ... and a gradient reaches no further than the patches allow: with a != b at the single pixel z only the valid pixels within
    # r of z see a difference, and their patches end r further out, so every pixel more than 2r from z gets exactly zero
    for radius in RADII:
        a = np.random.default_rng(23).uniform(0, 1, (1, 6 * radius + 4, 6 * radius + 5, 1))
        b = a.copy()
        zy, zx = radius, radius + 1
        b[0, zy, zx, 0] = 1.0 - b[0, zy, zx, 0]
        _, grad = metrics.census_loss_host(a, b, 1.0, np.float64, 1.0, radius)
        yy, xx = np.meshgrid(np.arange(a.shape[1]), np.arange(a.shape[2]), indexing='ij')
        far = np.maximum(np.abs(yy - zy), np.abs(xx - zx)) > 2 * radius
        assert np.any(far) and not np.any(grad[0, ..., 0][far]) and np.any(grad[0, ..., 0][~far])


def test_operand_checks():
    a = np.zeros((1, 12, 12, 1), np.float32)
    with pytest.raises(ValueError, match='shape'):
        metrics.census_loss_host(a, a[:, :11])
    with pytest.raises(ValueError, match='patch'):
        metrics.census_loss_host(a[:, :6], a[:, :6])
    metrics.census_loss_host(a[:, :6], a[:, :6], radius=2)
    with pytest.raises(ValueError, match='C in 1..4'):
        metrics.census_loss_host(np.zeros((1, 12, 12, 5)), np.zeros((1, 12, 12, 5)))
    with pytest.raises(ValueError, match='max_val'):
        metrics.census_loss_host(a, a, max_val=0.0)
    with pytest.raises(ValueError, match='weight'):
        metrics.census_loss_host(a, a, weight=float('nan'))
    with pytest.raises(ValueError, match='eps'):
        metrics.census_loss_host(a, a, eps=0.0)
    for bad in (0, 4, 1.0, True):
        with pytest.raises(ValueError, match='radius'):
            metrics.census_loss_host(a, a, radius=bad)


# ------------------------------------------------------------------------------------------------ the GPU tolerance rule
@pytest.mark.parametrize("case", sorted(census_cases.CASES))
def test_reference_alone_stays_inside_the_gpu_cap(case):
    """tests/test_gpu_census_loss.py lets the kernel differ from the float64 twin by 4 x the float32 twin's own gap and caps the
    gradient's relative L2 error at 1e-3: 4 x the gap must itself stay below that cap on every case of that test."""
    worst = 0.0
    for family in census_cases.FAMILIES:
        if family == 'same':
            continue
        for max_val in census_cases.MAX_VALS:
            for off, c in census_cases.views_of(case):
                _, g64, _, g32 = census_cases.reference(case, family, max_val, off, c, 1.0)
                n2 = np.linalg.norm(g64)
                assert n2 > 0, (case, family)
                rel = np.linalg.norm(g32.astype(np.float64) - g64) / n2
                worst = max(worst, rel)
                assert 4 * rel < 1e-3, (case, family, max_val, rel)
    print('%s: float32-to-float64 gap of the gradient at most %.1e relative L2' % (case, worst))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_census_loss', 'mv3d_census_loss_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.census_loss) and callable(lib.raw_census_loss)
    assert lib.census_loss_workspace_bytes(2, 45, 77, 3, 3) == 256                  # 2 x 2 x 3 tiles x 8 bytes, rounded up to 256
    assert lib.census_loss_workspace_bytes(64, 128, 128, 3, 2) == 64 * 16 * 8
    assert lib.census_loss_workspace_bytes(1, 3, 3, 1, 1) == 256 and lib.census_loss_workspace_bytes(1, 4, 5, 1, 2) == 0
    assert lib.census_loss_workspace_bytes(2, 6, 77, 3, 3) == 0 and lib.census_loss_workspace_bytes(2, 45, 77, 5, 3) == 0
    assert lib.census_loss_workspace_bytes(2, 45, 77, 3, 0) == 0 and lib.census_loss_workspace_bytes(2, 45, 77, 3, 4) == 0


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns its code and names the argument; none of them touches a pointer, so made-up addresses do."""
    ok = dict(N=2, H=16, W=16, C=3, a=0x1000, a_ld=3, b=0x2000, b_ld=3, radius=3, max_val=1.0, eps=0.01, weight=1.0, loss=0x3000,
              grad=0x5000, grad_ld=3, acc=0, ws=0x4000, ws_bytes=4096)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_census_loss(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['radius'], v['max_val'], v['eps'],
                                   v['weight'], v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], None)
    inf, nan = float('inf'), float('nan')
    lib.loss_overwrite_next()
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(H=6), -1, 'H'), (dict(W=6), -1, 'W'), (dict(H=4, radius=2), -1, 'H'),
                           (dict(W=2, radius=1), -1, 'W'), (dict(C=5), -1, 'C'), (dict(C=0), -1, 'C'),
                           (dict(radius=0), -1, 'radius'), (dict(radius=4), -1, 'radius'), (dict(radius=-1), -1, 'radius'),
                           (dict(H=32769), -1, 'H'), (dict(W=32769), -1, 'W'), (dict(N=1 << 21, H=32768, W=32768), -1, 'tiles'),
                           (dict(a_ld=2), -1, 'a_ld'), (dict(b_ld=2), -1, 'b_ld'), (dict(grad_ld=2), -1, 'grad_ld'),
                           (dict(acc=2), -1, 'grad_accumulate'), (dict(acc=-1), -1, 'grad_accumulate'),
                           (dict(max_val=0.0), -1, 'max_val'), (dict(max_val=inf), -1, 'max_val'), (dict(max_val=nan), -1, 'max_val'),
                           (dict(eps=0.0), -1, 'eps'), (dict(eps=-1.0), -1, 'eps'), (dict(eps=inf), -1, 'eps'), (dict(eps=nan), -1, 'eps'),
                           (dict(weight=inf), -1, 'weight'), (dict(weight=nan), -1, 'weight'),
                           (dict(a=None), -1, 'a is null'), (dict(b=None), -1, 'b is null'), (dict(loss=None), -1, 'loss_accum is null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(a=0x1002), -1, 'aligned'), (dict(grad=0x5001), -1, 'aligned'),
                           (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x4008), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error() and 'mv3d_census_loss' in lib.last_error(), (kw, lib.last_error())
    # the order of the checks: shape before strides before values before pointers before the workspace
    assert call(N=0, a_ld=2) == -1 and 'N' in lib.last_error()
    assert call(radius=9, H=2) == -1 and 'radius' in lib.last_error()
    assert call(a_ld=2, max_val=0.0) == -1 and 'a_ld' in lib.last_error()
    assert call(weight=nan, a=None) == -1 and 'weight' in lib.last_error()
    assert call(a=None, ws_bytes=0) == -1 and 'a is null' in lib.last_error()
    # the overwrite flag stayed pending through every refusal: a recorded pixel loss still sees it (and consumes it)
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        lib.pixel_loss_strided(4, 3, 0x1000, 3, 0x2000, 3, 1.0, None, 1, 2, 1.0, 0x3000, None, 3, None)
    finally:
        lib.plan_end()
    lib.plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ conf
def test_census_from_conf_defaults_and_refusals():
    from dynamic_multiview_3d_amd.model_base import census_from_conf
    assert census_from_conf({}) == (0.0, 3, 0.01)
    assert census_from_conf({'census_loss_weight': None, 'census_loss_radius': None, 'census_loss_eps': None}) == (0.0, 3, 0.01)
    assert census_from_conf({'census_loss_weight': 0}) == (0.0, 3, 0.01)
    assert census_from_conf({'census_loss_weight': 0.5, 'census_loss_radius': 1, 'census_loss_eps': 0.1}) == (0.5, 1, 0.1)
    assert census_from_conf({'census_loss_weight': 2, 'census_loss_radius': np.int64(2)}) == (2.0, 2, 0.01)
    for bad in (-1.0, float('nan'), float('inf'), -0.5):
        with pytest.raises(ValueError, match='census_loss_weight'):
            census_from_conf({'census_loss_weight': bad})
    for bad in (0, 4, -1, 2.0, '3', True):
        with pytest.raises(ValueError, match='census_loss_radius'):
            census_from_conf({'census_loss_weight': 0.5, 'census_loss_radius': bad})
    for bad in (0.0, -0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='census_loss_eps'):
            census_from_conf({'census_loss_weight': 0.5, 'census_loss_eps': bad})


# ------------------------------------------------------------------------------------------------ graph bookkeeping (recorded plans)
def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _appflow(**extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return AppearanceFlowModel(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def test_switch_absent_none_or_zero_records_the_same_plans(lib):
    absent = _labels(_appflow())
    m = _appflow(census_loss_weight=0.0, census_loss_radius=1, census_loss_eps=0.5)
    assert absent == _labels(m) == _labels(_appflow(census_loss_weight=None))
    assert 'resample_loss' in absent[0] and not any(l.startswith('census_loss') for plan in absent if plan for l in plan)
    assert not hasattr(m, 'census_terms') and [t.kind for _, t in m.graph.loss_expr.terms] == [2]


def test_switch_on_adds_weight_times_the_term_after_the_pixel_loss(lib):
    """The loss with the key is the loss without it plus weight x the census term: the same pixel term, and one more term that
    carries the weight, the pair, max_val, radius and eps the launches are recorded with."""
    from dynamic_multiview_3d_amd.graph import LOSS_CENSUS, ResampleNode
    m = _appflow(census_loss_weight=0.5, census_loss_radius=2, census_loss_eps=0.02)
    fwd, bwd, _ = _labels(m)
    assert 'resample_loss' not in fwd                                  # gen now feeds two terms: the fused head is gone
    assert fwd[-4:] == ['resample_fwd', 'pixel_loss', 'census_loss_tile', 'census_loss_final']
    assert bwd[0] == 'resample_bwd'
    assert [n.fused_loss for n in m.graph.nodes if isinstance(n, ResampleNode)] == [None]
    (w2, t2), (wc, tc) = m.graph.loss_expr.terms
    assert (w2, t2.kind) == (1.0, 2) and (wc, tc.kind, tc.max_val, tc.radius, tc.eps) == (0.5, LOSS_CENSUS, 1.0, 2, float(np.float32(0.02)))
    assert tc.a is m.gen and tc.b is m.image1
    assert tc.ws.numel() == lib.census_loss_workspace_bytes(2, 128, 128, 3, 2) and t2.ws is None
    assert m.census_terms == [('image', m.gen, m.image1, 1.0, 2, 0.02)]


def test_combines_with_the_other_switches_in_the_stated_order(lib):
    m = _appflow(census_loss_weight=0.5, ssim_loss_weight=0.25, flow_smoothness_weight=0.1, multiscale_loss_levels=2)
    fwd = _labels(m)[0]
    tail = ['pixel_loss', 'ssim_loss_tile', 'ssim_loss_final', 'census_loss_tile', 'census_loss_final', 'flow_smooth_tile', 'flow_smooth_final',
            'multiscale_pyramid', 'multiscale_loss_tile', 'multiscale_loss_final']
    assert fwd[-len(tail):] == tail
    without = _labels(_appflow(ssim_loss_weight=0.25, flow_smoothness_weight=0.1, multiscale_loss_levels=2))
    assert [l for l in fwd if not l.startswith('census_loss')] == without[0] and _labels(m)[1] == without[1]


def test_base_prediction_and_multiobject_add_the_term_to_the_colour_image_only(lib):
    from dynamic_multiview_3d_amd.graph import LOSS_CENSUS
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    plain = _labels(Base_Prediction_Model(conf, load_tfrec=False, device='cpu'))
    m = Base_Prediction_Model(dict(conf, census_loss_weight=0.25), load_tfrec=False, device='cpu')
    fwd = _labels(m)[0]
    assert fwd == plain[0] + ['census_loss_tile', 'census_loss_final']    # both pixel losses first, then the census term
    census = [(w, t) for w, t in m.graph.loss_expr.terms if t.kind == LOSS_CENSUS]
    assert len(census) == 1 and census[0][0] == 0.25 and census[0][1].a is m.gen_image1 and census[0][1].b is m.image1
    assert (census[0][1].radius, census[0][1].eps) == (3, float(np.float32(0.01)))
    conf = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': 0.1, 'combination_image': '', 'gen_sep_images': '',
            'masked_image_loss': '', 'fully_conv': '', 'census_loss_weight': 0.5}
    m = MultiObjectAppFlow(conf, load_tfrec=False, device='cpu')
    census = [(w, t) for w, t in m.graph.loss_expr.terms if t.kind == LOSS_CENSUS]
    assert len(census) == 1 and census[0][1].a is m.gen_image1 and census[0][1].b is m.image1
    assert _labels(m)[0].count('census_loss_tile') == 1


def test_census_alone_on_a_sampled_image_does_not_fuse(lib):
    """A gen that feeds only a census term must not go to the fused sampler + pixel-loss launch."""
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.model_base import optimizer_from_conf

    class CensusOnly(AppearanceFlowModel):
        def build_loss(self):
            self.loss = tf_utils.census_loss(self.image1, self.gen, 1.0) * 2.0       # target first: the op swaps the operands
            self.train_op = optimizer_from_conf(self.conf, self.conf['learning_rate']).minimize(self.loss, self.graph)
    m = CensusOnly({'batch_size': 2, 'learning_rate': 1e-4}, load_tfrec=False, device='cpu')
    fwd = _labels(m)[0]
    assert 'resample_loss' not in fwd and 'pixel_loss' not in fwd and 'fill' not in fwd
    assert fwd[-3:] == ['resample_fwd', 'census_loss_tile', 'census_loss_final']
    (w, t), = m.graph.loss_expr.terms
    assert w == 2.0 and t.a is m.gen and t.b is m.image1


def test_op_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, LOSS_CENSUS
    with Graph(device='cpu') as g:
        x = g.placeholder([2, 16, 16, 3], 'x')
        y = g.placeholder([2, 16, 16, 3], 'y')
        m = g.placeholder([2, 16, 16, 1], 'm')
        small = g.placeholder([2, 6, 16, 3], 's')
        with pytest.raises(NotImplementedError):
            tf_utils.census_loss(tf_utils.multiply(x, m), y)
        with pytest.raises(NotImplementedError):
            tf_utils.census_loss(x, tf_utils.scale(y, 0.75))
        with pytest.raises(ValueError, match='patch'):
            tf_utils.census_loss(small, small)                              # smaller than 2r+1 = 7
        tf_utils.census_loss(small, small, radius=2)
        with pytest.raises(ValueError, match='shape'):
            tf_utils.census_loss(x, m)
        with pytest.raises(ValueError, match='max_val'):
            tf_utils.census_loss(x, y, max_val=0.0)
        with pytest.raises(ValueError, match='radius'):
            tf_utils.census_loss(x, y, radius=4)
        with pytest.raises(ValueError, match='eps'):
            tf_utils.census_loss(x, y, eps=float('nan'))
        e = tf_utils.census_loss(x, y, 1.5, 1, 0.05) * 0.5 + tf_utils.euclidean_loss(x, y)
        assert [(w, t.kind) for w, t in e.terms] == [(0.5, LOSS_CENSUS), (1.0, 2)]
        assert (e.terms[0][1].max_val, e.terms[0][1].radius) == (1.5, 1)


def test_models_without_the_term_refuse_the_key_and_bad_values_are_refused(lib):
    from dynamic_multiview_3d_amd import mv3d
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError, match='census_loss_weight'):
            cls({'batch_size': 2, 'census_loss_weight': 0.5}, device='cpu')
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='census_loss_weight'):
            _appflow(census_loss_weight=bad)
    with pytest.raises(ValueError, match='census_loss_radius'):
        _appflow(census_loss_weight=0.5, census_loss_radius=4)
    with pytest.raises(ValueError, match='census_loss_eps'):
        _appflow(census_loss_weight=0.5, census_loss_eps=0.0)


# ------------------------------------------------------------------------------------------------ evaluate(), host path
class _Arr:
    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def numpy(self):
        return self.a


def test_evaluate_reports_the_unweighted_term_on_a_cpu_graph_only_when_the_switch_is_on():
    """ModelBase.evaluate on a graph without a GPU scores each batch with the twin; the figure is unweighted and averaged over
    the batches."""
    from dynamic_multiview_3d_amd.model_base import ModelBase
    rng = np.random.default_rng(3)
    batches = [(rng.uniform(0, 1, (2, 14, 12, 3)).astype(np.float32), rng.uniform(0, 1, (2, 14, 12, 3)).astype(np.float32)) for _ in range(2)]

    class M(ModelBase):
        def __init__(self, on):
            self.graph = types.SimpleNamespace(device=torch.device('cpu'), loss_expr=object())
            self.pred, self.target, self.i = _Arr(batches[0][0]), _Arr(batches[0][1]), 0
            if on:
                self.census_terms = [('image', self.pred, self.target, 1.0, 2, 0.01)]

        def forward(self, **feeds):
            self.pred.a, self.target.a = batches[self.i]
            self.i += 1
            return 0.5

        def eval_pairs(self):
            return [('image', self.pred, self.target, 1.0)]

    data = types.SimpleNamespace(next=lambda: {})
    res = M(True).evaluate(data, 2)
    want = np.mean([float(metrics.census_loss_host(p, t, 1.0, np.float64, 1.0, 2, 0.01)[0]) for p, t in batches])
    assert abs(res['image/census'] - want) <= 1e-15 and 0 < want < 1
    assert 'image/census' not in M(False).evaluate(data, 2)
    assert not hasattr(_appflow(), 'census_terms')
