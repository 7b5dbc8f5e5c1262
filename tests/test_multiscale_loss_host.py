"""metrics.multiscale_warp_loss_host, the numpy statement of mv3d_multiscale_warp_loss, on the CPU: against an independent
composition from the oracle, against finite differences, on known answers, and float32 against float64 on every case of the GPU
test (tests/multiscale_cases.py), which is where the reference alone is shown to stay inside the GPU parity bar."""
import numpy as np
import pytest

from dynamic_multiview_3d_amd import metrics
from oracle import ops
from tests import multiscale_cases as MC


def _oracle_composition(src, flow, target, levels, weights, kind):
    """(value, grad, [T_l]) in float64 from oracle/ops.py: pooling by reshape / mean, warp_pts_layer, resampler_fwd / _bwd, the
    pixel losses; the coarse warp gradient repeated over the block and divided by f^3."""
    n, h, w, _ = flow.shape
    value, grad, ts = 0.0, np.zeros(flow.shape, np.float64), []

    def pool(x, f):
        return x.astype(np.float64).reshape(n, x.shape[1] // f, f, x.shape[2] // f, f, x.shape[3]).mean(axis=(2, 4))
    for l in range(1, levels + 1):
        f = 1 << l
        s, t = pool(src, f), pool(target, f)
        warp = ops.warp_pts_layer(pool(flow, f) / f)
        gen = ops.resampler_fwd(s, warp)
        if kind == 2:
            T, dgen = ops.euclidean_loss_fwd(gen, t), ops.euclidean_loss_bwd(gen, t)
        else:
            T, dgen = ops.l1_loss_fwd(gen, t), ops.l1_loss_bwd(gen, t)
        _, dwarp = ops.resampler_bwd(s, warp, dgen, need_ddata=False)
        ts.append(float(T))
        value += weights[l - 1] * float(T)
        grad += weights[l - 1] * np.repeat(np.repeat(dwarp, f, axis=1), f, axis=2) / f ** 3
    return value, grad, ts


@pytest.mark.parametrize("kind", MC.KINDS)
@pytest.mark.parametrize("case", sorted(MC.SHAPES))
def test_float64_twin_matches_the_oracle_composition(case, kind):
    src, tgt = MC.images(case)
    levels = MC.dims(case)[3]
    for family in MC.FAMILIES:
        for c in MC.channels_of(case):
            flow = MC.flow(case, family)
            want_v, want_g, want_t = _oracle_composition(src[..., :c], flow, tgt[..., :c], levels, MC.weights(case), kind)
            v64, g64, t64 = MC.reference(case, family, c, kind)[:3]
            scale = max(np.abs(want_g).max(), 1e-300)
            print('%s %s C %d kind %d: value %.12g rel %.2e | grad max rel %.2e' % (case, family, c, kind, want_v, abs(v64 - want_v) / max(abs(want_v), 1e-300),
                                                                                   np.abs(g64 - want_g).max() / scale))
            assert abs(v64 - want_v) <= 1e-12 * abs(want_v)
            assert np.abs(g64 - want_g).max() <= 1e-12 * scale
            assert np.allclose(t64, want_t, rtol=1e-12, atol=0)
            assert g64.dtype == np.float64 and g64.shape == flow.shape


@pytest.mark.parametrize("kind", MC.KINDS)
def test_gradient_matches_central_finite_differences(kind):
    """float64, the smallest cases: every flow element of one1 and one3 is perturbed."""
    for case in ('one1', 'one3'):
        src, tgt = MC.images(case)
        levels, flow = MC.dims(case)[3], MC.flow(case, 'random').astype(np.float64)
        _, g, _ = metrics.multiscale_warp_loss_host(src, flow, tgt, levels, MC.weights(case), kind)
        h = 1e-6                                             # the generator keeps every coordinate 1e-3 from a kink
        worst = 0.0
        for idx in np.ndindex(flow.shape):
            fp, fm = flow.copy(), flow.copy()
            fp[idx] += h
            fm[idx] -= h
            fd = (float(metrics.multiscale_warp_loss_host(src, fp, tgt, levels, MC.weights(case), kind)[0]) -
                  float(metrics.multiscale_warp_loss_host(src, fm, tgt, levels, MC.weights(case), kind)[0])) / (2 * h)
            worst = max(worst, abs(fd - g[idx]))
        print('%s kind %d: largest |fd - grad| %.2e, largest |grad| %.2e' % (case, kind, worst, np.abs(g).max()))
        assert np.abs(g).max() > 0
        assert worst <= 1e-8 + 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_flow_on_a_transposed_pair_is_exactly_zero(dtype):
    for side, levels in ((8, 3), (96, 2), (32, 3)):
        a, b = MC.transposed_pair(side)
        for kind in MC.KINDS:
            v, g, t = metrics.multiscale_warp_loss_host(a, np.zeros((2, side, side, 2), np.float32), b, levels, None, kind, dtype)
            assert v == 0 and not np.any(g) and not np.any(t), (side, kind)
            assert v.dtype == dtype and g.dtype == dtype and t.shape == (levels,)


def test_a_displaced_dot_reaches_more_pixels_at_level_2():
    """A 2 x 2 dot displaced by 5 pixels, zero flow: the full-resolution euclidean loss moves the flow at a handful of pixels
    (the sampler's gradient sees four source pixels), the pooled term at level 2 at strictly more."""
    src, tgt = np.zeros((1, 32, 32, 1)), np.zeros((1, 32, 32, 1))
    src[0, 10:12, 10:12] = 1.0
    tgt[0, 10:12, 15:17] = 1.0
    flow = np.zeros((1, 32, 32, 2))
    warp = ops.warp_pts_layer(flow)
    gen = ops.resampler_fwd(src, warp)
    _, dflow = ops.resampler_bwd(src, warp, ops.euclidean_loss_bwd(gen, tgt), need_ddata=False)
    full = int(np.count_nonzero(np.abs(dflow).sum(-1)))
    counts = []
    for l in (1, 2, 3):
        w = [0.0] * 3
        w[l - 1] = 1.0
        _, g, _ = metrics.multiscale_warp_loss_host(src, flow, tgt, 3, w, 2)
        counts.append(int(np.count_nonzero(np.abs(g).sum(-1))))
    print('pixels with a non-zero flow gradient: full resolution %d, levels 1..3 %s' % (full, counts))
    assert full > 0 and counts[1] > full


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("case", sorted(MC.SHAPES))
def test_float32_twin_stays_inside_the_parity_bar(case, family):
    for c in MC.channels_of(case):
        for kind in MC.KINDS:
            ref = MC.reference(case, family, c, kind)
            MC.within_rule('%s %s C %d kind %d' % (case, family, c, kind), ref[3], ref[4], ref)
            assert ref[4].dtype == np.float32
            assert np.abs(ref[5].astype(np.float64) - ref[2]).max() <= 1e-5 * max(ref[2].max(), 1e-30) + 1e-7


def test_generated_flows_keep_clear_of_the_kinks():
    for case in MC.SHAPES:
        for family in ('smooth', 'random'):
            cmin, dmin, bad = MC.clearance(case, MC.flow(case, family))
            print('%s %s: closest coordinate to an integer %.2e, smallest |difference| %.2e' % (case, family, cmin, dmin))
            assert cmin >= 1e-3 and dmin >= 1e-5 and not bad.any()
        f = MC.flow(case, 'dyadic').astype(np.float64)
        top = 1 << MC.dims(case)[3]
        assert np.all(f * 4 / top == np.round(f * 4 / top))


def test_refusals():
    src, tgt = MC.images('edge')
    flow = MC.flow('edge', 'random')
    ok = dict(src=src[..., :3], flow=flow, target=tgt[..., :3], levels=3)
    for kw, word in [(dict(levels=0), 'levels'), (dict(levels=4), 'levels'), (dict(level_weights=[1.0, 1.0]), 'level_weights'),
                     (dict(level_weights=[1.0, float('nan'), 1.0]), 'finite'), (dict(kind=3), 'kind'), (dict(flow=flow[..., :1]), 'flow'),
                     (dict(target=tgt[:, :-8, :, :3]), 'target'), (dict(src=src[..., :2]), 'src'), (dict(src=src[:, :-4, :, :3]), 'Hs'),
                     (dict(flow=flow[:, :36], target=tgt[:, :36, :, :3]), 'H ')]:
        with pytest.raises(ValueError, match=word):
            metrics.multiscale_warp_loss_host(**dict(ok, **kw))
