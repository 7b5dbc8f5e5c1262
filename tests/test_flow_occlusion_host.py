"""Occlusion masking of the head loss without a GPU: the numpy twin against a per-pixel float64 loop and against constructed
flows, the masked head's gradient against central differences, the C ABI's refusals, the graph op, the conf switch on recorded plans
and evaluate()'s bookkeeping on a CPU graph.

Measured on the CPU (tests/flow_occlusion_cases.py, seed 7, alphas 0.01 / 0.5): the smallest relative margin |lhs - rhs| / max(lhs, rhs)
of an inside pixel is 1.27e-4 (smooth 4 x 72); the float32 twin's mask equals the float64 twin's at every pixel of every case."""
import gc
import math
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import flow_occlusion_cases as OC
from tests.test_flow_smooth_host import _labels, _recorded


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ numpy twin
def loop_mask(flow, alpha1, alpha2, outside_visible):
    """The definition as a direct per-pixel float64 loop: (mask [N,H,W], (visible, occluded, outside) counts)."""
    f = np.asarray(flow, np.float64)
    n, h, w, _ = f.shape
    a1, a2 = float(np.float32(alpha1)), float(np.float32(alpha2))
    mask = np.zeros((n, h, w))
    counts = [0, 0, 0]
    for b in range(n):
        partner = f[(b + n // 2) % n]
        for i in range(h):
            for j in range(w):
                f0, f1 = f[b, i, j]
                x, y = f0 + i, f1 + j
                if not (0 <= x <= w - 1 and 0 <= y <= h - 1):          # a NaN fails the comparisons
                    mask[b, i, j] = 1.0 if outside_visible else 0.0
                    counts[2] += 1
                    continue
                fx, fy = int(math.floor(x)), int(math.floor(y))
                dx, dy = (fx + 1) - x, (fy + 1) - y

                def tap(r, c):
                    return partner[r, c] if (r < h and c < w) else np.zeros(2)
                s = dx * dy * tap(fy, fx) + (1 - dx) * (1 - dy) * tap(fy + 1, fx + 1) + dx * (1 - dy) * tap(fy + 1, fx) + (1 - dx) * dy * tap(fy, fx + 1)
                r0, r1 = f0 + s[1], f1 + s[0]
                lhs = r0 * r0 + r1 * r1
                rhs = a1 * ((f0 * f0 + f1 * f1) + (s[0] * s[0] + s[1] * s[1])) + a2
                visible = lhs < rhs
                mask[b, i, j] = 1.0 if visible else 0.0
                counts[0 if visible else 1] += 1
    return mask, counts


@pytest.mark.parametrize("family,n,h", OC.CASES[:4])
def test_twin_matches_a_per_pixel_loop(family, n, h):
    flow = OC.flow(family, n, h)
    for keep in (True, False):
        mask, counts = loop_mask(flow, OC.ALPHA1, OC.ALPHA2, keep)
        got, shares = metrics.flow_occlusion_mask_host(flow, OC.ALPHA1, OC.ALPHA2, keep)
        assert got.dtype == np.float64 and np.array_equal(got, mask)
        assert shares == tuple(c / float(n * h * h) for c in counts) and abs(sum(shares) - 1.0) < 1e-15


def test_every_case_has_both_values_and_the_float32_twin_decides_alike():
    for name, flow in OC.all_cases():
        m64, s64 = metrics.flow_occlusion_mask_host(flow)
        m32, s32 = metrics.flow_occlusion_mask_host(flow, dtype=np.float32)
        assert m32.dtype == np.float32 and np.array_equal(m64, m32.astype(np.float64)), name
        assert s64 == s32 and min(s64[:2]) > 0, name
        rel, inside = OC.margins(flow)
        print('%-14s smallest margin %.3e shares %.3f %.3f %.3f' % ((name, rel[inside].min()) + s64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_integer_inverse_flows_are_visible_at_every_inside_pixel(dtype):
    n, h, a, b = 4, 24, 3.0, -2.0
    f = np.zeros((n, h, h, 2), np.float32)
    f[0], f[2] = (a, b), (-b, -a)
    f[1], f[3] = (-5.0, 1.0), (-1.0, 5.0)
    for keep in (True, False):
        mask, shares, (lhs, rhs, inside) = metrics.flow_occlusion_mask_host(f, 0.0, 1e-6, keep, dtype, details=True)
        assert np.all(lhs[inside] == 0) and np.all(mask[inside] == 1)         # the residual is exactly 0: visible at any alpha2 > 0
        assert np.all(mask[~inside] == (1 if keep else 0))
        assert shares[1] == 0 and 0 < shares[2] < 0.5


def test_a_shifted_block_is_occluded_exactly_where_its_interior_is_sampled():
    """Zero flows see each other everywhere.  The partner's flow is (3, 0) on a block: a pixel of sample 0 samples the partner at
    (row j, column i), so it is occluded exactly where (j, i) lies in the block (|r|^2 = 9 against 0.01 * 9 + 0.5); the partner's
    own pixels of the block follow their flow to a pixel of sample 0 whose flow is 0 and are occluded as well."""
    h = 16
    f = np.zeros((2, h, h, 2), np.float32)
    rows, cols = slice(4, 9), slice(6, 12)
    f[1, rows, cols, 0] = 3.0
    mask, shares = metrics.flow_occlusion_mask_host(f)
    want0 = np.ones((h, h))
    want0[cols, rows] = 0.0                                                    # pixel (i, j) reads partner[j, i]
    assert np.array_equal(mask[0], want0)
    want1 = np.ones((h, h))
    want1[rows, cols] = 0.0
    assert np.array_equal(mask[1], want1) and shares[2] == 0


def test_outside_visible_flips_only_the_outside_pixels():
    for name, flow in OC.all_cases()[:6]:
        keep, sk = metrics.flow_occlusion_mask_host(flow, outside_visible=True)
        drop, sd = metrics.flow_occlusion_mask_host(flow, outside_visible=False)
        _, inside = OC.margins(flow)
        assert sk == sd and np.array_equal(keep[inside], drop[inside]), name
        assert np.all(keep[~inside] == 1) and np.all(drop[~inside] == 0) and np.count_nonzero(~inside) > 0, name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_in_the_partner_occludes_and_nan_in_f_is_outside(dtype):
    base = np.zeros((2, 8, 8, 2), np.float32)
    clean, _ = metrics.flow_occlusion_mask_host(base, dtype=dtype)
    assert np.all(clean == 1)
    f = base.copy()
    f[1, 3, 5, 0] = np.nan                      # sampled by pixel (5, 3) of sample 0; the pixel itself has no coordinate
    f[0, 6, 6, 1] = np.inf                      # no coordinate either; sampled by pixel (6, 6) of sample 1
    for keep in (True, False):
        mask, shares, (_, _, inside) = metrics.flow_occlusion_mask_host(f, outside_visible=keep, dtype=dtype, details=True)
        assert not inside[1, 3, 5] and not inside[0, 6, 6] and np.count_nonzero(~inside) == 2
        assert mask[1, 3, 5] == mask[0, 6, 6] == (1 if keep else 0)
        # pixel (i, j) reads the partner at rows j, j + 1 and columns i, i + 1, and a weight of 0 does not hide a NaN (0 * NaN):
        # the four pixels whose footprint holds the value are occluded, and only they
        want = np.ones((2, 8, 8))
        want[0, 4:6, 2:4] = 0
        want[1, 5:7, 5:7] = 0
        assert np.array_equal(mask[inside], want[inside]) and np.all(inside[want == 0]) and np.all(np.isfinite(mask))
        assert shares == (118 / 128.0, 8 / 128.0, 2 / 128.0)


def test_operand_checks():
    f = np.zeros((2, 4, 4, 2), np.float32)
    for bad in (np.zeros((3, 4, 4, 2)), np.zeros((2, 4, 5, 2)), np.zeros((2, 4, 4, 3)), np.zeros((2, 1, 1, 2))):
        with pytest.raises(ValueError):
            metrics.flow_occlusion_mask_host(bad)
    for kw in (dict(alpha1=-1e-3), dict(alpha1=float('nan')), dict(alpha1=float('inf')), dict(alpha2=0.0), dict(alpha2=-1.0),
               dict(alpha2=float('nan')), dict(alpha1=True), dict(outside_visible=1), dict(outside_visible=None)):
        with pytest.raises(ValueError):
            metrics.flow_occlusion_mask_host(f, **kw)
    with pytest.raises(_lib.Mv3dError, match='GPU'):
        metrics.flow_occlusion_mask(torch.zeros(2, 4, 4, 2))


# ------------------------------------------------------------------------------------------------ the masked head's gradient
@pytest.mark.parametrize("kind", [2, 1])
@pytest.mark.parametrize("n,h", OC.SHAPES[:2])
def test_masked_head_gradient_matches_central_differences(n, h, kind):
    """Twin mask -> oracle sampler -> masked L2 / L1, in float64: the analytic dflow (mask held constant) against central
    differences of the whole chain with the mask recomputed at every step.  The step crosses no margin: every perturbed mask is
    asserted equal to the unperturbed one, so the two derivatives are of one function."""
    flow = OC.flow('smooth', n, h).astype(np.float64)
    src, target = OC.head_images(n, h, 3)
    weight, step = 0.7, 1e-6
    loss, dflow, _, mask = OC.head_chain_host(src, flow, target, kind, weight)
    assert 0 < mask.mean() < 1 and loss > 0
    rel, inside = OC.margins(flow)
    assert rel[inside].min() > 100 * step
    num = np.zeros_like(flow)
    picked = list(np.ndindex(*flow.shape))[::1 if h <= 8 else 9]              # every element at 8 x 8, every 9th (both channels occur) at 20 x 20
    for idx in picked:
        vals = []
        for sgn in (1.0, -1.0):
            p = flow.copy()
            p[idx] += sgn * step
            l, _, _, m = OC.head_chain_host(src, p, target, kind, weight)
            assert np.array_equal(m, mask), idx                                # no margin is crossed
            vals.append(float(l))
        num[idx] = (vals[0] - vals[1]) / (2 * step)
    sel = np.zeros(flow.shape, bool)
    sel[tuple(np.array(picked).T)] = True
    worst = np.abs(num - dflow)[sel].max()
    print('masked head %dx%d kind %d: max |dflow| %.3e, against central differences %.2e' % (n, h, kind, np.abs(dflow).max(), worst))
    assert np.abs(dflow).max() > 1e-5
    assert worst <= 1e-6 * np.abs(dflow).max() + 1e-10
    # an occluded pixel has no gradient at all, and the mask itself contributes none
    assert not np.any(dflow[mask == 0])


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_flow_occlusion_mask', 'mv3d_flow_occlusion_mask_workspace_bytes', 'mv3d_warp_resample_occlusion_loss',
                 'mv3d_warp_resample_occlusion_loss_workspace_bytes'):
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert callable(lib.flow_occlusion_mask) and callable(lib.raw_warp_resample_occlusion_loss)
    # 4 doubles per 32 x 32 tile, rounded up to 256
    for fn in (lib.flow_occlusion_mask_workspace_bytes, lib.warp_resample_occlusion_loss_workspace_bytes):
        assert fn(2, 2, 2) == 256 and fn(64, 128, 128) == 64 * 16 * 32
        for bad in ((1, 4, 4), (3, 4, 4), (0, 4, 4), (2, 4, 5), (2, 1, 1), (2, 40000, 40000)):
            assert fn(*bad) == 0, bad


def test_mask_refusals_come_before_any_launch(lib):
    ok = dict(N=2, H=16, W=16, flow=0x1000, flow_ld=2, a1=0.01, a2=0.5, keep=1, mask=0x3000, mask_ld=1, stats=0x5000, ws=0x10000, ws_bytes=1 << 16)

    def call(**kw):
        v = dict(ok, **kw)
        return _recorded(lib, lambda: lib.raw_flow_occlusion_mask(v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['a1'], v['a2'], v['keep'],
                                                                  v['mask'], v['mask_ld'], v['stats'], v['ws'], v['ws_bytes'], None))
    inf, nan = float('inf'), float('nan')
    need = lib.flow_occlusion_mask_workspace_bytes(2, 16, 16)
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(N=3), -1, 'N'), (dict(W=17), -1, 'differ'), (dict(H=1, W=1), -1, 'H'),
                           (dict(H=40000, W=40000), -1, 'H'), (dict(N=1 << 30, H=1 << 15, W=1 << 15), -1, 'tiles'),
                           (dict(N=1 << 10, H=1 << 15, W=1 << 15, flow_ld=1 << 30), -1, 'overflow'),
                           (dict(flow_ld=1), -1, 'flow_ld'), (dict(mask_ld=0), -1, 'mask_ld'),
                           (dict(a1=-0.1), -1, 'alpha1'), (dict(a1=nan), -1, 'alpha1'), (dict(a1=inf), -1, 'alpha1'),
                           (dict(a2=0.0), -1, 'alpha2'), (dict(a2=-1.0), -1, 'alpha2'), (dict(a2=nan), -1, 'alpha2'), (dict(a2=inf), -1, 'alpha2'),
                           (dict(keep=2), -1, 'outside_visible'), (dict(flow=None), -1, 'flow is null'),
                           (dict(mask=None, stats=None), -1, 'both null'), (dict(flow=0x1002), -1, 'aligned'), (dict(mask=0x3001), -1, 'aligned'),
                           (dict(stats=0x5002), -1, 'aligned'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(ws_bytes=need - 1), -3, 'workspace'), (dict(ws=0x10008), -3, 'aligned')]:
        rc, labels = call(**kw)
        assert rc == code and labels == [], (kw, rc, labels)
        assert word in lib.last_error() and 'mv3d_flow_occlusion_mask' in lib.last_error(), (kw, lib.last_error())
    assert call() == (0, ['occl_mask', 'occl_mask_stats'])
    assert call(stats=None, ws=None, ws_bytes=0) == (0, ['occl_mask'])           # only the shares need the workspace
    assert call(mask=None) == (0, ['occl_mask', 'occl_mask_stats'])
    assert call(a1=0.0, flow=0x1004, flow_ld=3, mask=0x3004, mask_ld=4)[0] == 0  # channel-slice views


def test_head_refusals_come_before_any_launch_and_keep_the_overwrite_pending(lib):
    ok = dict(N=2, H=16, W=16, Hs=16, Ws=16, C=3, src=0x1000, flow=0x2000, flow_ld=2, tgt=0x3000, tgt_ld=3, kind=2, weight=1.0, a1=0.01, a2=0.5,
              keep=1, warp=0x4000, gen=0x5000, dflow=0x6000, dflow_ld=2, mask=0x7000, mask_ld=1, loss=0x8000, stats=0x8100, ws=0x10000,
              ws_bytes=1 << 16)

    def call(**kw):
        v = dict(ok, **kw)
        return _recorded(lib, lambda: lib.raw_warp_resample_occlusion_loss(
            v['N'], v['H'], v['W'], v['Hs'], v['Ws'], v['C'], v['src'], v['flow'], v['flow_ld'], v['tgt'], v['tgt_ld'], v['kind'], v['weight'],
            v['a1'], v['a2'], v['keep'], v['warp'], v['gen'], v['dflow'], v['dflow_ld'], v['mask'], v['mask_ld'], v['loss'], v['stats'],
            v['ws'], v['ws_bytes'], None))
    nan = float('nan')
    need = lib.warp_resample_occlusion_loss_workspace_bytes(2, 16, 16)
    two = ['occl_head_tile', 'occl_head_final']
    for kw, code, word in [(dict(N=3), -1, 'N'), (dict(W=17, Ws=17), -1, 'differ'), (dict(Hs=8), -1, 'source'), (dict(Ws=32), -1, 'source'),
                           (dict(H=1, W=1, Hs=1, Ws=1), -1, 'H'), (dict(C=0), -1, 'C'), (dict(C=5, tgt_ld=5), -1, 'C'), (dict(flow_ld=1), -1, 'flow_ld'),
                           (dict(tgt_ld=2), -1, 'target_ld'), (dict(dflow_ld=1), -1, 'dflow_ld'), (dict(mask_ld=0), -1, 'mask_ld'),
                           (dict(kind=3), -1, 'kind'), (dict(weight=nan), -1, 'weight'), (dict(a1=-1.0), -1, 'alpha1'), (dict(a2=0.0), -1, 'alpha2'),
                           (dict(keep=-1), -1, 'outside_visible'), (dict(src=None), -1, 'src is null'), (dict(flow=None), -1, 'flow is null'),
                           (dict(tgt=None), -1, 'target is null'), (dict(gen=None), -1, 'gen is null'), (dict(loss=None), -1, 'loss_accum is null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(gen=0x5002), -1, 'aligned'), (dict(mask=0x7001), -1, 'aligned'),
                           (dict(ws_bytes=need - 1), -3, 'workspace'), (dict(ws=0x10008), -3, 'aligned')]:
        lib.loss_overwrite_next()
        rc, labels = call(**kw)
        assert rc == code and labels == [], (kw, rc, labels)
        assert word in lib.last_error() and 'mv3d_warp_resample_occlusion_loss' in lib.last_error(), (kw, lib.last_error())
        # the flag is still pending: the next loss entry consumes it (recorded, nothing runs)
        assert _recorded(lib, lambda: lib.raw_pixel_loss(4, 1, 0x1000, 0x2000, None, 2, 1.0, 0x3000, None, None))[0] == 0
    assert call() == (0, two)
    assert call(warp=None, dflow=None, mask=None, stats=None) == (0, two)
    assert call(C=1, tgt_ld=4, kind=1, keep=0, flow=0x2004, flow_ld=3, mask=0x7004, mask_ld=4, dflow=0x6004, dflow_ld=3) == (0, two)


# ------------------------------------------------------------------------------------------------ graph op
def test_op_makes_a_constant_one_channel_tensor_and_refuses_what_it_cannot_do(lib):
    from dynamic_multiview_3d_amd import tf_utils
    from dynamic_multiview_3d_amd.graph import Graph, OcclusionMaskNode, LOSS_L2
    with Graph(device='cpu') as g:
        img = g.placeholder([2, 16, 16, 3], 'img')
        tgt = g.placeholder([2, 16, 16, 3], 'tgt')
        odd = g.placeholder([3, 16, 16, 3], 'odd')
        wide = g.placeholder([2, 16, 8, 3], 'wide')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
        with pytest.raises(ValueError, match=r'\[N,H,W,2\]'):
            tf_utils.occlusion_mask(tf_utils.conv2d_msra(img, 3, 3, 3, 1, 1, 'three'))
        with pytest.raises(ValueError, match='even N'):
            tf_utils.occlusion_mask(tf_utils.conv2d_msra(odd, 2, 3, 3, 1, 1, 'oddflow'))
        with pytest.raises(ValueError, match='H == W'):
            tf_utils.occlusion_mask(tf_utils.conv2d_msra(wide, 2, 3, 3, 1, 1, 'wideflow'))
        with pytest.raises(NotImplementedError):
            tf_utils.occlusion_mask(tf_utils.scale(flow, 0.5))
        for kw in (dict(alpha1=-1.0), dict(alpha2=0.0), dict(alpha2=float('nan')), dict(outside_visible='keep')):
            with pytest.raises(ValueError):
                tf_utils.occlusion_mask(flow, **kw)
        before = len(g.nodes)
        mask = tf_utils.occlusion_mask(flow)
        assert mask.shape == (2, 16, 16, 1) and mask.requires_grad is False and len(g.nodes) == before + 1
        node = mask.producer
        assert isinstance(node, OcclusionMaskNode) and node.flow is flow and node.mask is mask
        assert (node.alpha1, node.alpha2, node.outside_visible) == (float(np.float32(0.01)), 0.5, True)
        # it composes with what exists
        gen = tf_utils.resample_layer(img, tf_utils.warp_pts_layer(flow))
        e = tf_utils.masked_euclidean_loss(gen, tgt, mask)
        (w, t), = e.terms
        assert (w, t.kind, t.a, t.b, t.mask) == (1.0, LOSS_L2, gen, tgt, mask)
        (w, t), = tf_utils.l1_loss(tf_utils.multiply(gen, mask), tf_utils.multiply(tgt, mask)).terms
        assert t.mask is mask and t.a is gen


# ------------------------------------------------------------------------------------------------ conf switch on recorded plans
ON = dict(pair_swap=True, occlusion_mask=True)
HEAD = ['occl_head_tile', 'occl_head_final']


def _appflow(cls=None, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    return (cls or AppearanceFlowModel)(dict({'batch_size': 2, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cpu')


def _plans(cls=None, **extra):
    """The three label lists of a model that is dropped at once: a CPU model holds over a gigabyte of buffers, and its graph is
    full of reference cycles, so it is collected here and not whenever the collector next runs."""
    m = _appflow(cls, **extra)
    out = _labels(m)
    del m
    gc.collect()
    return out


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()


def test_conf_parsing():
    from dynamic_multiview_3d_amd.model_base import occlusion_from_conf
    assert occlusion_from_conf({}) is None and occlusion_from_conf({'occlusion_mask': None}) is None
    assert occlusion_from_conf({'occlusion_mask': False, 'pair_swap': True, 'batch_size': 2}) is None
    assert occlusion_from_conf({'occlusion_alpha1': 0.2}) is None                 # the parameters alone switch nothing on
    on = {'occlusion_mask': True, 'pair_swap': True, 'batch_size': 4}
    assert occlusion_from_conf(on) == (0.01, 0.5, True)
    assert occlusion_from_conf(dict(on, occlusion_alpha1=0, occlusion_alpha2=2, occlusion_outside='mask')) == (0.0, 2.0, False)
    assert occlusion_from_conf(dict(on, occlusion_alpha1=None, occlusion_alpha2=None, occlusion_outside=None)) == (0.01, 0.5, True)
    assert occlusion_from_conf(dict(on, occlusion_outside='keep'))[2] is True
    for bad in (dict(occlusion_mask=1), dict(occlusion_mask='yes'), dict(occlusion_mask=0.0),
                dict(occlusion_alpha1=float('nan')), dict(occlusion_alpha1=float('inf')), dict(occlusion_alpha1=-0.01), dict(occlusion_alpha1=True),
                dict(occlusion_alpha2=0.0), dict(occlusion_alpha2=-1.0), dict(occlusion_alpha2=float('nan')), dict(occlusion_alpha2=float('inf')),
                dict(occlusion_alpha2=1e-60), dict(occlusion_outside='drop'), dict(occlusion_outside=True),
                dict(pair_swap=False), dict(pair_swap=None),
                dict(ssim_loss_weight=0.1), dict(census_loss_weight=0.1), dict(multiscale_loss_levels=2)):
        with pytest.raises(ValueError):
            occlusion_from_conf(dict(on, **bad))
    # the bad parameters raise with the switch off as well: a misspelt value is never ignored silently
    for bad in (dict(occlusion_alpha1=-1.0), dict(occlusion_alpha2=0.0), dict(occlusion_outside='drop'), dict(occlusion_mask='on')):
        with pytest.raises(ValueError):
            occlusion_from_conf(bad)
    with pytest.raises(ValueError, match='pair_swap'):
        occlusion_from_conf({'occlusion_mask': True})
    # a weight of 0 leaves the other switches off: no conflict
    assert occlusion_from_conf(dict(on, ssim_loss_weight=0, census_loss_weight=None, multiscale_loss_levels=0)) == (0.01, 0.5, True)


def test_key_absent_none_or_false_records_the_same_plans_and_allocates_nothing(lib):
    from dynamic_multiview_3d_amd.graph import OcclusionMaskNode, ResampleNode
    absent = _plans()
    assert absent == _plans(occlusion_mask=None) == _plans(occlusion_mask=False)
    assert absent == _plans(pair_swap=True, occlusion_mask=False, occlusion_alpha1=0.3, occlusion_outside='mask')
    assert 'resample_loss' in absent[0] and not any(l.startswith('occl') for plan in absent if plan for l in plan)
    plain = _appflow()
    size = (len(plain.graph.tensors), plain.graph.activation_bytes)
    del plain
    gc.collect()
    m = _appflow(pair_swap=True, occlusion_mask=False)
    assert not hasattr(m, 'occlusion_terms') and not any(isinstance(n, OcclusionMaskNode) for n in m.graph.nodes)
    assert (len(m.graph.tensors), m.graph.activation_bytes) == size
    (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
    assert node.fused_occlusion is None and node.occlusion_ws is None
    (w, t), = m.graph.loss_expr.terms
    assert t.mask is None
    with pytest.raises(RuntimeError, match='occlusion_mask'):
        m.occlusion_mask()


def test_key_on_fuses_the_head_into_one_tiled_launch(lib):
    from dynamic_multiview_3d_amd.graph import OcclusionMaskNode, ResampleNode
    absent = _plans()
    m = _appflow(**ON)
    fwd, bwd, fused = _labels(m)
    at = absent[0].index('resample_loss')
    assert fwd == absent[0][:at] + HEAD + absent[0][at + 1:] and 'occl_mask' not in fwd         # the node's own launch is not recorded
    assert bwd == absent[1] and fused == absent[2]
    (node,) = [n for n in m.graph.nodes if isinstance(n, ResampleNode)]
    (occl,) = [n for n in m.graph.nodes if isinstance(n, OcclusionMaskNode)]
    assert node.fused_occlusion is occl and occl.fused_into is node and occl.flow is m.flow_field
    assert node.occlusion_ws.numel() == lib.warp_resample_occlusion_loss_workspace_bytes(2, 128, 128)
    (w, t), = m.graph.loss_expr.terms
    assert (w, t.kind, t.a, t.b, t.mask) == (1.0, 2, m.gen, m.image1, occl.mask)
    assert m.occlusion_terms == [('flow', m.flow_field, occl.mask, 0.01, 0.5, True)]
    assert tuple(m.occlusion_mask().shape) == (2, 128, 128, 1)
    del m, node, occl, t
    gc.collect()
    other = _appflow(occlusion_alpha1=0.05, occlusion_alpha2=1.5, occlusion_outside='mask', **ON)
    (occl,) = [n for n in other.graph.nodes if isinstance(n, OcclusionMaskNode)]
    assert (occl.alpha1, occl.alpha2, occl.outside_visible) == (float(np.float32(0.05)), 1.5, False)


def test_an_unfused_head_keeps_the_four_separate_launches(lib, monkeypatch):
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    plain = _plans()
    fwd, bwd, fused = _plans(**ON)
    at = plain[0].index('resample_fwd')
    assert plain[0][at:] == ['resample_fwd', 'pixel_loss']
    assert fwd == plain[0][:at] + ['resample_fwd', 'occl_mask', 'pixel_loss']
    assert bwd == plain[1] and fused == plain[2] and bwd[0] == 'resample_bwd'


def test_the_flow_terms_stay_behind_the_head(lib, monkeypatch):
    terms = dict(flow_smoothness_weight=0.25, flow_consistency_weight=0.5)
    base = _plans(pair_swap=True, **terms)
    fwd, bwd, fused = _plans(**dict(terms, **ON))
    at = base[0].index('resample_loss')
    assert fwd == base[0][:at] + HEAD + base[0][at + 1:] and bwd == base[1] and fused == base[2]
    assert fwd[at + 2] == 'flow_smooth_tile' and fwd[-1] == 'flow_consist_final'
    monkeypatch.setenv('MV3D_FUSE_RESAMPLE', '0')
    base = _plans(pair_swap=True, **terms)
    fwd, bwd, fused = _plans(**dict(terms, **ON))
    at = base[0].index('pixel_loss')
    assert fwd == base[0][:at] + ['occl_mask'] + base[0][at:] and bwd == base[1] and fused == base[2]


def test_the_family_takes_the_switch(lib):
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    for cls in (AppearanceFlowTinghui, AppFlowHighDimAngle, AppFlowLowDimAngle):
        fwd = _plans(cls, **ON)[0]
        assert fwd[-2:] == HEAD, cls.__name__


def test_every_other_class_and_combination_is_refused(lib):
    from dynamic_multiview_3d_amd import mv3d, multiobject_main_model
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    with pytest.raises(ValueError, match='pair_swap'):
        _appflow(occlusion_mask=True)
    with pytest.raises(ValueError, match='pair_swap'):
        _appflow(occlusion_mask=True, pair_swap=False)
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        with pytest.raises(ValueError):
            cls(dict({'batch_size': 2}, **ON), device='cpu')
    bp = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1}
    with pytest.raises(ValueError, match='occlusion_mask'):
        Base_Prediction_Model(dict(bp, **ON), load_tfrec=False, device='cpu')
    mo = {'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'combination_image': '', 'fully_conv': ''}
    for cls in (multiobject_main_model.Base_Prediction_Model, MultiObjectAppFlow):
        with pytest.raises(ValueError):
            cls(dict(mo, **ON), load_tfrec=False, device='cpu')
    for combo in (dict(ssim_loss_weight=0.2), dict(census_loss_weight=0.2), dict(multiscale_loss_levels=2)):
        with pytest.raises(ValueError, match='occlusion_mask'):
            _appflow(**dict(ON, **combo))
    for bad in (dict(occlusion_mask=1), dict(occlusion_alpha1=float('nan')), dict(occlusion_alpha1=-1.0), dict(occlusion_alpha2=0.0),
                dict(occlusion_alpha2=float('inf')), dict(occlusion_outside='drop')):
        with pytest.raises(ValueError, match='occlusion'):
            _appflow(**dict(ON, **bad))


def test_evaluate_and_the_log_row_report_the_shares_on_a_cpu_graph_only_when_the_switch_is_on(lib, monkeypatch):
    """A CPU graph cannot run a forward pass, so forward() is replaced by one that fills the tensors evaluate() reads; the numpy
    form then scores them."""
    from dynamic_multiview_3d_amd.train import training_log_row
    flow = OC.flow('smooth', 2, 128)

    class Data:
        def next(self):
            return {}

    def run(m):
        def forward(**feeds):
            m.flow_field.set(flow.copy())
            m.gen.set(np.zeros(m.gen.shape, np.float32))
            m.image1.set(np.full(m.image1.shape, 0.5, np.float32))
            return torch.zeros(())
        monkeypatch.setattr(m, 'forward', forward)
        return m.evaluate(Data(), num_batches=2)
    plain = _appflow(pair_swap=True)
    off = run(plain)
    assert not any(k.split('/')[-1] in ('visible', 'occluded', 'outside') for k in off)
    assert 'flow_visible' not in training_log_row(plain, 10, 0.5)
    m = _appflow(**ON)
    on = run(m)
    assert set(on) == set(off) | {'flow/visible', 'flow/occluded', 'flow/outside'}
    _, shares = metrics.flow_occlusion_mask_host(flow)
    assert (on['flow/visible'], on['flow/occluded'], on['flow/outside']) == shares
    assert abs(on['flow/visible'] + on['flow/occluded'] + on['flow/outside'] - 1.0) < 1e-12
    row = training_log_row(m, 10, 0.5)
    assert row['flow_visible'] == shares[0] and row['training_loss'] == 0.5
