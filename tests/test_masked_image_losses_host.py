"""CPU-side checks of the occlusion-masked census and SSIM losses: the numpy twins (metrics.census_loss_host / ssim_loss_host with
mask=) against the unmasked twins, against linearity in the mask and against float64 torch autograd over an independent
restatement multiplied by the mask; the guard of the GPU parity rule; the refusals of mv3d_census_loss_masked and
mv3d_ssim_loss_masked (they come before any launch, so they need no device); the graph ops; conf['occlusion_mask_image_terms'] on
recorded plans; and evaluate()'s host path.

Measured on the CPU for the shapes and mask families of tests/masked_image_cases.py: the float32 twin's gradient is at most 7.5e-5
(census) and 5.5e-5 (SSIM) relative L2 away from the float64 twin's, so 4 x that gap stays inside the 1e-3 cap of the GPU tests."""
import gc
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamic_multiview_3d_amd import _lib, metrics
from tests import census_cases
from tests import masked_image_cases as MC

ON = dict(pair_swap=True, occlusion_mask=True)
KEY = 'occlusion_mask_image_terms'


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


def _cases(kind):
    return MC.CENSUS_CASES if kind == 'census' else sorted(MC.SSIM_CASES)


KIND_CASES = [(kind, case) for kind in ('census', 'ssim') for case in _cases(kind)]


# ------------------------------------------------------------------------------------------------ numpy twins
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,case", KIND_CASES)
def test_a_mask_of_ones_gives_the_unmasked_twin_bit_for_bit(kind, case, dtype):
    for family in MC.FAMILIES:
        a, b = MC.inputs(kind, case, family)
        for off, c in MC.views_of(kind, case):
            va, vb = a[..., off:off + c], b[..., off:off + c]
            plain = MC.twin(kind, case, va, vb, dtype, 0.75, None)
            ones = MC.twin(kind, case, va, vb, dtype, 0.75, MC.mask(kind, case, 'ones'))
            assert ones[0].dtype == plain[0].dtype == np.dtype(dtype) and ones[1].dtype == np.dtype(dtype)
            assert ones[0].tobytes() == plain[0].tobytes(), (case, family)
            assert np.array_equal(ones[1].view(np.uint8), plain[1].view(np.uint8)), (case, family)


@pytest.mark.parametrize("kind,case", KIND_CASES)
def test_zero_mask_gives_zero_and_equal_images_give_zero_under_any_mask(kind, case):
    for dtype in (np.float32, np.float64):
        for family in MC.FAMILIES:
            a, b = MC.inputs(kind, case, family)
            loss, grad = MC.twin(kind, case, a, b, dtype, 1.0, MC.mask(kind, case, 'zeros'))
            assert float(loss) == 0.0 and not np.signbit(loss) and not np.any(grad), (case, family)
        a, b = MC.inputs(kind, case, 'same')
        for mf in MC.MASKS:
            loss, grad = MC.twin(kind, case, a, b, dtype, 1.0, MC.mask(kind, case, mf))
            assert float(loss) == 0.0, (case, mf)
            assert np.abs(grad).max() <= (0.0 if kind == 'census' else 4e-6), (case, mf)


@pytest.mark.parametrize("kind,case", KIND_CASES)
def test_float64_twins_are_linear_in_the_mask(kind, case):
    a, b = MC.inputs(kind, case, 'random')
    m1, m2 = MC.mask(kind, case, 'fraction').astype(np.float64), MC.mask(kind, case, 'blocks').astype(np.float64)
    l1, g1 = MC.twin(kind, case, a, b, np.float64, 1.0, m1)
    l2, g2 = MC.twin(kind, case, a, b, np.float64, 1.0, m2)
    l12, g12 = MC.twin(kind, case, a, b, np.float64, 1.0, m1 + m2)
    ls, gs = MC.twin(kind, case, a, b, np.float64, 1.0, 2.5 * m1)
    print('%s %s: |loss(m1 + m2) - loss(m1) - loss(m2)| %.1e, gradient max %.1e' % (kind, case, abs(l12 - l1 - l2), np.abs(g12 - g1 - g2).max()))
    assert abs(float(l12) - float(l1) - float(l2)) <= 1e-12 and np.abs(g12 - g1 - g2).max() <= 1e-12
    assert abs(float(ls) - 2.5 * float(l1)) <= 1e-12 and np.abs(gs - 2.5 * g1).max() <= 1e-12


def torch_masked_census(a, b, m, radius, eps):
    """(loss, d loss / d a) in float64 by autograd, from the formulas for g, t, dist and rho only, times the mask."""
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb, tm = torch.tensor(b, dtype=torch.float64), torch.tensor(m, dtype=torch.float64)[..., 0]
    n, h, w, c = ta.shape
    r = radius
    hv, wv = h - 2 * r, w - 2 * r
    ga, gb = ta.mean(dim=3) * 255.0, tb.mean(dim=3) * 255.0

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
    loss = (tm[:, r:r + hv, r:r + wv] * rho).sum() / (n * hv * wv)
    loss.backward()
    return float(loss.detach()), ta.grad.numpy()


def torch_masked_ssim(a, b, m):
    """(loss, d loss / d a) in float64 by autograd: the 11x11 outer-product window as one grouped F.conv2d, the map times the mask
    at the window centres."""
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb, tm = torch.tensor(b, dtype=torch.float64), torch.tensor(m, dtype=torch.float64)
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    c = ta.shape[3]
    k = (g[:, None] * g[None, :])[None, None].repeat(c, 1, 1, 1)
    f = lambda x: F.conv2d(x.permute(0, 3, 1, 2), k, groups=c)
    mx, my, sab, s2 = f(ta), f(tb), f(ta * tb), f(ta * ta + tb * tb)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mx * my + c1) / (mx * mx + my * my + c1)) * ((2 * sab - 2 * mx * my + c2) / (s2 - mx * mx - my * my + c2))
    mw = tm[:, 5:-5, 5:-5, :].permute(0, 3, 1, 2)                          # [N,1,Hv,Wv]: the centre of the window with origin (oy, ox)
    loss = (mw * (1 - s)).sum() / s.numel()
    loss.backward()
    return float(loss.detach()), ta.grad.numpy()


@pytest.mark.parametrize("kind,case", KIND_CASES)
def test_float64_twins_match_autograd_over_an_independent_restatement_times_the_mask(kind, case):
    for family, mf in (('random', 'fraction'), ('shift', 'blocks'), ('noise', 'sparse')):
        a, b = MC.inputs(kind, case, family)
        m = MC.mask(kind, case, mf)
        loss, grad = MC.twin(kind, case, a, b, np.float64, 1.0, m)
        if kind == 'census':
            tl, tg = torch_masked_census(a, b, m, census_cases.CASES[case][0], float(np.float32(MC.EPS)))
        else:
            tl, tg = torch_masked_ssim(a, b, m)
        scale = max(np.linalg.norm(tg), 1e-300)
        print('%s %s %s %s: loss %.6f, |loss - autograd| %.1e, gradient L2 error %.1e of %.1e'
              % (kind, case, family, mf, loss, abs(loss - tl), np.linalg.norm(grad - tg), scale))
        assert abs(float(loss) - tl) <= 1e-10 * max(abs(tl), 1e-3)
        assert np.linalg.norm(grad - tg) <= 1e-10 * scale if np.any(tg) else not np.any(grad)


def test_the_mask_may_be_a_channel_of_a_wider_array_and_bad_masks_are_refused():
    a, b = MC.inputs('ssim', 'row', 'random')
    m = MC.mask('ssim', 'row', 'fraction')
    wide = np.full(m.shape[:3] + (4,), np.nan, np.float32)
    wide[..., 2:3] = m
    for fn, args in ((metrics.ssim_loss_host, (a, b, 1.0, np.float32, 1.0)), (metrics.census_loss_host, (a, b, 1.0, np.float32, 1.0, 2, 0.01))):
        want = fn(*args, mask=m)
        got = fn(*args, mask=wide[..., 2:3])
        squeezed = fn(*args, mask=m[..., 0])
        assert want[0] == got[0] == squeezed[0] and np.array_equal(want[1], got[1]) and np.array_equal(want[1], squeezed[1])
        with pytest.raises(ValueError, match='mask'):
            fn(*args, mask=m[:, :-1])
        with pytest.raises(ValueError, match='mask'):
            fn(*args, mask=wide)
        with pytest.raises(ValueError, match='finite'):
            fn(*args, mask=wide[..., 1:2])


# ------------------------------------------------------------------------------------------------ the GPU tolerance rule
@pytest.mark.parametrize("kind,case", KIND_CASES)
def test_reference_alone_stays_inside_the_gpu_cap(kind, case):
    """tests/test_gpu_masked_*_loss.py let the kernel differ from the float64 twin by 4 x the float32 twin's own gap and cap the
    gradient's relative L2 error at 1e-3 wherever the float64 gradient is non-zero: 4 x the gap must itself stay below that cap on
    every case of those tests.  Where the float64 gradient is exactly zero (a mask that hides every valid pixel or window) the
    float32 twin's is zero too, inside the absolute floor."""
    worst, zero = 0.0, []
    for family in MC.FAMILIES:
        if family == 'same':
            continue
        for mf in MC.MASKS:
            for off, c in MC.views_of(kind, case):
                _, g64, _, g32 = MC.reference(kind, case, family, mf, off, c)
                n2 = np.linalg.norm(g64)
                if n2 == 0:
                    zero.append((family, mf))
                    assert np.abs(g32).max() <= 4e-6, (case, family, mf)
                    continue
                rel = np.linalg.norm(g32.astype(np.float64) - g64) / n2
                worst = max(worst, rel)
                assert 4 * rel < 1e-3, (case, family, mf, rel)
    print('%s %s: float32-to-float64 gap of the gradient at most %.1e relative L2; zero float64 gradient under %s'
          % (kind, case, worst, sorted(set(mf for _, mf in zero))))
    assert all(mf == 'zeros' for _, mf in zero) or case in ('r1_smallest', 'one', 'smallest'), zero


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_census_loss_masked', 'mv3d_ssim_loss_masked', 'mv3d_ssim_loss_masked_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.census_loss_masked) and callable(lib.raw_census_loss_masked)
    assert callable(lib.ssim_loss_masked) and callable(lib.raw_ssim_loss_masked)
    assert lib.ssim_loss_masked_workspace_bytes(2, 45, 77, 3) == 256               # 2 x 2 x 3 tiles x 16 bytes, rounded up to 256
    assert lib.ssim_loss_masked_workspace_bytes(64, 128, 128, 3) == 64 * 16 * 16
    assert lib.ssim_loss_masked_workspace_bytes(2, 10, 77, 3) == 0 and lib.ssim_loss_masked_workspace_bytes(2, 45, 77, 5) == 0


CENSUS_OK = dict(N=2, H=16, W=16, C=3, a=0x1000, a_ld=3, b=0x2000, b_ld=3, mask=0x6000, mask_ld=1, radius=3, max_val=1.0, eps=0.01, weight=1.0,
                 loss=0x3000, grad=0x5000, grad_ld=3, acc=0, ws=0x4000, ws_bytes=4096)


def census_call(lib, stream=None, ok=CENSUS_OK, **kw):
    v = dict(ok, **kw)
    return lib.raw_census_loss_masked(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['mask'], v['mask_ld'], v['radius'],
                                      v['max_val'], v['eps'], v['weight'], v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], stream)


def ssim_call(lib, stream=None, ok=CENSUS_OK, **kw):
    v = dict(ok, **kw)
    return lib.raw_ssim_loss_masked(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['mask'], v['mask_ld'], v['max_val'],
                                    v['weight'], v['loss'], v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], stream)


inf, nan = float('inf'), float('nan')
SHARED_REFUSALS = [(dict(N=0), -1, 'N'), (dict(C=5), -1, 'C'), (dict(C=0), -1, 'C'), (dict(H=32769), -1, 'H'), (dict(W=32769), -1, 'W'),
                   (dict(N=1 << 21, H=32768, W=32768), -1, 'tiles'), (dict(a_ld=2), -1, 'a_ld'), (dict(b_ld=2), -1, 'b_ld'),
                   (dict(mask_ld=0), -1, 'mask_ld'), (dict(mask_ld=-1), -1, 'mask_ld'), (dict(grad_ld=2), -1, 'grad_ld'),
                   (dict(acc=2), -1, 'grad_accumulate'), (dict(acc=-1), -1, 'grad_accumulate'),
                   (dict(max_val=0.0), -1, 'max_val'), (dict(max_val=inf), -1, 'max_val'), (dict(max_val=nan), -1, 'max_val'),
                   (dict(weight=inf), -1, 'weight'), (dict(weight=nan), -1, 'weight'),
                   (dict(a=None), -1, 'a is null'), (dict(b=None), -1, 'b is null'), (dict(loss=None), -1, 'loss_accum is null'),
                   (dict(mask=None), -1, 'mask is null'), (dict(ws=None), -1, 'workspace is null'), (dict(a=0x1002), -1, 'aligned'),
                   (dict(mask=0x6002), -1, 'aligned'), (dict(grad=0x5001), -1, 'aligned'),
                   (dict(ws_bytes=255), -3, 'workspace'), (dict(ws=0x4008), -3, 'aligned')]
CENSUS_REFUSALS = SHARED_REFUSALS + [(dict(H=6), -1, 'H'), (dict(W=6), -1, 'W'), (dict(H=4, radius=2), -1, 'H'), (dict(radius=0), -1, 'radius'),
                                     (dict(radius=4), -1, 'radius'), (dict(eps=0.0), -1, 'eps'), (dict(eps=inf), -1, 'eps'), (dict(eps=nan), -1, 'eps')]
SSIM_REFUSALS = SHARED_REFUSALS + [(dict(H=10), -1, 'H'), (dict(W=10), -1, 'W')]


def test_refusals_come_before_any_launch(lib):
    """Every refusal returns its code and names the argument; none of them touches a pointer, so made-up addresses do.  The
    overwrite flag stays pending through all of them."""
    lib.loss_overwrite_next()
    for call, name, table in ((census_call, 'mv3d_census_loss_masked', CENSUS_REFUSALS), (ssim_call, 'mv3d_ssim_loss_masked', SSIM_REFUSALS)):
        for kw, code, word in table:
            assert call(lib, **kw) == code, (name, kw)
            assert word in lib.last_error() and name in lib.last_error(), (kw, lib.last_error())
        # the order of the checks: shape before strides before values before pointers before the workspace
        assert call(lib, N=0, mask_ld=0) == -1 and 'N' in lib.last_error()
        assert call(lib, mask_ld=0, max_val=0.0) == -1 and 'mask_ld' in lib.last_error()
        assert call(lib, weight=nan, mask=None) == -1 and 'weight' in lib.last_error()
        assert call(lib, mask=None, ws_bytes=0) == -1 and 'mask is null' in lib.last_error()
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:                                    # a recorded pixel loss still sees the flag (and consumes it)
        lib.pixel_loss_strided(4, 3, 0x1000, 3, 0x2000, 3, 1.0, None, 1, 2, 1.0, 0x3000, None, 3, None)
    finally:
        lib.plan_end()
    lib.plan_destroy(plan)


def test_recorded_calls_carry_the_masked_labels_and_bytes(lib):
    """Recording launches nothing, so made-up addresses do: the labels, and the unmasked entry's bytes plus 4 B per pixel."""
    n, h, w, c = 2, 45, 77, 3
    plans = {}
    for masked in (False, True):
        plan = lib.plan_create()
        lib.plan_begin(plan)
        try:
            if masked:
                assert census_call(lib, N=n, H=h, W=w) == 0 and ssim_call(lib, N=n, H=h, W=w) == 0
            else:
                lib.census_loss(n, h, w, c, 0x1000, 3, 0x2000, 3, 3, 1.0, 0.01, 1.0, 0x3000, 0x5000, 3, 0, 0x4000, 4096, None)
                lib.ssim_loss(n, h, w, c, 0x1000, 3, 0x2000, 3, 1.0, 1.0, 0x3000, 0x5000, 3, 0, 0x4000, 4096, None)
        finally:
            lib.plan_end()
        plans[masked] = _lib.plan_ops(plan)
        lib.plan_destroy(plan)
    assert [o[0] for o in plans[False]] == ['census_loss_tile', 'census_loss_final', 'ssim_loss_tile', 'ssim_loss_final']
    assert [o[0] for o in plans[True]] == ['census_loss_masked_tile', 'census_loss_masked_final', 'ssim_loss_masked_tile', 'ssim_loss_masked_final']
    tiles = n * 2 * 3
    assert plans[True][0][2] == plans[False][0][2] + n * h * w * 4.0 and plans[True][0][1] == plans[False][0][1]
    assert plans[True][1][2] == plans[False][1][2]
    assert plans[True][2][2] == plans[False][2][2] + n * h * w * 4.0 + tiles * 8.0          # ... and the second sum of every tile
    assert plans[True][3][2] == plans[False][3][2] + tiles * 8.0


# ------------------------------------------------------------------------------------------------ graph ops
def test_ops_take_a_constant_one_channel_mask_and_refuse_everything_else(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, LOSS_CENSUS, LOSS_SSIM
    with Graph(device='cpu') as g:
        x = tf_utils.conv2d_msra(g.placeholder([2, 16, 16, 3], 'x'), 3, 3, 3, 1, 1, 'c')        # differentiated
        y = g.placeholder([2, 16, 16, 3], 'y')
        m = g.placeholder([2, 16, 16, 1], 'm')
        m3 = g.placeholder([2, 16, 16, 3], 'm3')
        small = g.placeholder([2, 8, 16, 1], 'small')
        learned = tf_utils.conv2d_msra(y, 1, 3, 3, 1, 1, 'm')                                    # requires a gradient
        for op, kind in ((tf_utils.ssim_loss, LOSS_SSIM), (tf_utils.census_loss, LOSS_CENSUS)):
            (w, t), = op(x, y, mask=m).terms
            assert (w, t.kind, t.a, t.b, t.mask) == (1.0, kind, x, y, m)
            (w, t), = op(y, x, 1.0, mask=m).terms                                               # the op swaps the operands, the mask stays
            assert (t.a, t.b, t.mask) == (x, y, m)
            assert op(x, y).terms[0][1].mask is None
            for bad in (m3, small, learned, np.ones((2, 16, 16, 1), np.float32), 1.0):
                with pytest.raises(ValueError, match='mask'):
                    op(x, y, mask=bad)
            with pytest.raises(NotImplementedError):
                op(x, y, mask=tf_utils.multiply(m, m))
            with pytest.raises(NotImplementedError):
                op(tf_utils.multiply(x, m), y, mask=m)
            with pytest.raises(NotImplementedError):
                op(x, tf_utils.scale(y, 0.75), mask=m)


# ------------------------------------------------------------------------------------------------ conf and recorded plans
def _labels(model):
    g = model.graph
    return [[o[0] for o in _lib.plan_ops(p)] if p is not None else None for p in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused)]


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def _summary(**extra):
    """(labels, tensor count, activation bytes) of a model that is dropped at once (a CPU model holds over a gigabyte)."""
    m = _appflow(**extra)
    out = (_labels(m), len(m.graph.tensors), m.graph.activation_bytes)
    del m
    gc.collect()
    return out


def test_conf_parsing():
    from dynamic_multiview_3d_amd.model_base import occlusion_from_conf, occlusion_image_terms_from_conf
    on = dict(ON, batch_size=4)
    assert occlusion_image_terms_from_conf({}) is False and occlusion_image_terms_from_conf({KEY: None}) is False
    assert occlusion_image_terms_from_conf({KEY: False}) is False and occlusion_image_terms_from_conf(dict(on, **{KEY: False})) is False
    assert occlusion_image_terms_from_conf(dict(on, **{KEY: True})) is True
    assert occlusion_image_terms_from_conf(dict(on, **{KEY: np.bool_(True)})) is True
    for bad in (1, 0, 'yes', 1.0, 'True'):                                  # not a bool: refused with the switches off as well
        for base in ({}, on, {'occlusion_mask': False}):
            with pytest.raises(ValueError, match=KEY):
                occlusion_image_terms_from_conf(dict(base, **{KEY: bad}))
    for base in ({}, {'occlusion_mask': False}, {'occlusion_mask': None, 'pair_swap': True}):
        with pytest.raises(ValueError, match='needs conf\\[\'occlusion_mask\'\\]'):
            occlusion_image_terms_from_conf(dict(base, **{KEY: True}))
    # occlusion_from_conf keeps its 3-tuple and its refusals; the key lifts the SSIM and census ones only
    for combo in (dict(ssim_loss_weight=0.1), dict(census_loss_weight=0.1), dict(ssim_loss_weight=0.1, census_loss_weight=0.2)):
        for off in ({}, {KEY: None}, {KEY: False}):
            with pytest.raises(ValueError, match='occlusion_mask'):
                occlusion_from_conf(dict(on, **combo, **off))
        assert occlusion_from_conf(dict(on, **combo, **{KEY: True})) == (0.01, 0.5, True)
    for key in ({}, {KEY: True}):
        with pytest.raises(ValueError, match='multiscale_loss_levels'):
            occlusion_from_conf(dict(on, multiscale_loss_levels=2, **key))
    assert occlusion_from_conf(dict(on, **{KEY: True})) == (0.01, 0.5, True)


def test_the_key_builds_the_masked_terms_on_the_head_mask(lib):
    """The case the parent refuses: occlusion_mask + census_loss_weight (+ ssim_loss_weight) + the key builds a model whose SSIM
    and census terms carry the head's mask, in front of which the head stays unfused with the mask node's own launch."""
    from dynamic_multiview_3d_amd.graph import LOSS_CENSUS, LOSS_SSIM, OcclusionMaskNode, ResampleNode
    m = _appflow(census_loss_weight=0.5, **dict(ON, **{KEY: True}))
    fwd, bwd, _ = _labels(m)
    assert fwd[-5:] == ['resample_fwd', 'occl_mask', 'pixel_loss', 'census_loss_masked_tile', 'census_loss_masked_final']
    assert bwd[0] == 'resample_bwd'
    del m
    gc.collect()
    m = _appflow(ssim_loss_weight=0.25, census_loss_weight=0.5, census_loss_radius=2, **dict(ON, **{KEY: True}))
    fwd, bwd, _ = _labels(m)
    assert fwd[-7:] == ['resample_fwd', 'occl_mask', 'pixel_loss', 'ssim_loss_masked_tile', 'ssim_loss_masked_final', 'census_loss_masked_tile',
                        'census_loss_masked_final']
    assert not any(l in ('ssim_loss_tile', 'census_loss_tile', 'occl_head_tile', 'resample_loss') for l in fwd) and bwd[0] == 'resample_bwd'
    (occl,) = [n for n in m.graph.nodes if isinstance(n, OcclusionMaskNode)]
    (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
    assert node.fused_loss is None and node.fused_occlusion is None and occl.fused_into is None
    (w2, t2), (ws, ts), (wc, tc) = m.graph.loss_expr.terms
    assert (w2, t2.kind, t2.mask) == (1.0, 2, occl.mask)
    assert (ws, ts.kind, ts.a, ts.b, ts.mask, ts.max_val) == (0.25, LOSS_SSIM, m.gen, m.image1, occl.mask, 1.0)
    assert (wc, tc.kind, tc.a, tc.b, tc.mask, tc.radius) == (0.5, LOSS_CENSUS, m.gen, m.image1, occl.mask, 2)
    assert ts.ws.numel() == lib.ssim_loss_masked_workspace_bytes(2, 128, 128, 3) and tc.ws.numel() == lib.census_loss_workspace_bytes(2, 128, 128, 3, 2)
    assert m.census_terms == [('image', m.gen, m.image1, 1.0, 2, 0.01)]
    assert m.masked_image_terms == [('image', 'ssim_loss_masked', m.gen, m.image1, occl.mask, 1.0, None, None),
                                    ('image', 'census_masked', m.gen, m.image1, occl.mask, 1.0, 2, 0.01)]
    # without the masked terms the same conf records the unmasked launches behind the same head
    del m, occl, node, t2, ts, tc
    gc.collect()
    plain = _labels(_appflow(ssim_loss_weight=0.25, census_loss_weight=0.5, census_loss_radius=2))[0]
    assert [l.replace('_masked', '') for l in fwd if l != 'occl_mask'] == plain


def test_the_key_with_neither_weight_records_the_plans_of_occlusion_mask_alone(lib):
    alone = _summary(**ON)
    assert _summary(**dict(ON, **{KEY: True})) == alone
    assert _summary(ssim_loss_weight=0, census_loss_weight=None, **dict(ON, **{KEY: True})) == alone
    m = _appflow(**dict(ON, **{KEY: True}))
    assert not hasattr(m, 'masked_image_terms') and not hasattr(m, 'census_terms')


def test_key_absent_none_or_false_changes_nothing(lib):
    """Plans, tensor count and activation bytes are those of the same conf without the key, and the refusals are still made."""
    for conf in ({}, dict(ssim_loss_weight=0.25, census_loss_weight=0.5), ON):
        absent = _summary(**conf)
        assert _summary(**dict(conf, **{KEY: None})) == absent and _summary(**dict(conf, **{KEY: False})) == absent
    fwd = _summary(ssim_loss_weight=0.25, census_loss_weight=0.5)[0][0]
    assert fwd[-6:] == ['resample_fwd', 'pixel_loss', 'ssim_loss_tile', 'ssim_loss_final', 'census_loss_tile', 'census_loss_final']
    assert _summary()[0][0][-1] == 'resample_loss' and _summary(**ON)[0][0][-2:] == ['occl_head_tile', 'occl_head_final']
    for combo in (dict(ssim_loss_weight=0.2), dict(census_loss_weight=0.2)):
        for off in ({}, {KEY: None}, {KEY: False}):
            with pytest.raises(ValueError, match='occlusion_mask'):
                _appflow(**dict(ON, **combo, **off))


def test_refusals_of_the_key(lib):
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    for bad in (1, 'yes', 0.0):
        for base in ({}, ON, dict(ON, census_loss_weight=0.5)):
            with pytest.raises(ValueError, match=KEY):
                _appflow(**dict(base, **{KEY: bad}))
    with pytest.raises(ValueError, match=KEY):                              # True needs occlusion_mask
        _appflow(**{KEY: True})
    with pytest.raises(ValueError, match=KEY):
        _appflow(census_loss_weight=0.5, pair_swap=True, occlusion_mask=False, **{KEY: True})
    for key in ({}, {KEY: True}):                                           # the multi-scale term stays refused
        with pytest.raises(ValueError, match='occlusion_mask'):
            _appflow(multiscale_loss_levels=2, **dict(ON, **key))
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    for conf in ({KEY: True}, dict(ON, **{KEY: True}), dict(ON, census_loss_weight=0.5, **{KEY: True})):
        with pytest.raises(ValueError, match='occlusion_mask'):
            Base_Prediction_Model(dict(bp, **conf), load_tfrec=False, device='cpu')
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError):
            cls(dict({'batch_size': 2}, **{KEY: True}), device='cpu')


def test_the_family_takes_the_key(lib):
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for cls in (AppearanceFlowTinghui, AppFlowHighDimAngle, AppFlowLowDimAngle):
        m = _appflow(cls, census_loss_weight=0.5, **dict(ON, **{KEY: True}))
        fwd = _labels(m)[0]
        del m
        gc.collect()
        assert fwd[-5:] == ['resample_fwd', 'occl_mask', 'pixel_loss', 'census_loss_masked_tile', 'census_loss_masked_final'], cls.__name__


# ------------------------------------------------------------------------------------------------ evaluate(), host path
def test_evaluate_reports_the_masked_rows_on_a_cpu_graph_only_when_the_terms_are_on(lib, monkeypatch):
    """A CPU graph cannot run a forward pass, so forward() is replaced by one that fills the tensors evaluate() reads; the numpy
    forms then score them.  image/census and image/ssim stay the unmasked figures."""
    rng = np.random.default_rng(11)
    shape = (2, 128, 128, 3)
    gen, target = rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32)
    mask = (rng.uniform(0, 1, (2, 128, 128, 1)) < 0.6).astype(np.float32)

    class Data:
        def next(self):
            return {}

    def run(m):
        def forward(**feeds):
            m.flow_field.set(np.zeros(m.flow_field.shape, np.float32))
            m.gen.set(gen.copy())
            m.image1.set(target.copy())
            for term in getattr(m, 'occlusion_terms', []):
                term[2].set(mask.copy())
            return torch.zeros(())
        monkeypatch.setattr(m, 'forward', forward)
        return m.evaluate(Data(), num_batches=1)
    conf = dict(ssim_loss_weight=0.25, census_loss_weight=0.5, census_loss_radius=1)
    plain = run(_appflow(pair_swap=True, **conf))
    assert 'image/census' in plain and not any(k.endswith('_masked') for k in plain)
    gc.collect()
    alone = run(_appflow(**dict(ON, **{KEY: True})))
    assert 'flow/visible' in alone and not any(k.endswith('_masked') for k in alone)
    gc.collect()
    on = run(_appflow(**dict(ON, **conf, **{KEY: True})))
    assert list(on)[-3:] == ['image/ssim_loss_masked', 'image/census_masked', 'images']
    assert set(on) == set(plain) | {'flow/visible', 'flow/occluded', 'flow/outside', 'image/ssim_loss_masked', 'image/census_masked'}
    assert on['image/census'] == plain['image/census'] and on['image/ssim'] == plain['image/ssim']
    want_c = float(metrics.census_loss_host(gen, target, 1.0, np.float64, 1.0, 1, 0.01, mask=mask)[0])
    want_s = float(metrics.ssim_loss_host(gen, target, 1.0, np.float64, 1.0, mask=mask)[0])
    assert on['image/census_masked'] == want_c and on['image/ssim_loss_masked'] == want_s
    assert 0 < want_c < on['image/census'] and 0 < want_s < 1 - on['image/ssim']
