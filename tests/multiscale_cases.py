"""Shapes, operands and references shared by tests/test_multiscale_loss_host.py and tests/test_gpu_multiscale_loss.py.

Shapes (N, H, W, L[, Hs, Ws]); the kernel's tiles are 32 x 32 flow pixels:
  one1, one3   one coarse pixel at the top level
  edge         crosses one tile edge in H, below a tile in W
  inner        a tile with neighbours on all eight sides
  nonsq        a source that is not the target's size (and not square)
  views        run as channel-slice views: flow = channels 1..2 of a 4-channel tensor, src / target = the first C of 4 channels

Flow families:
  smooth, random   a few pixels / uniform in [-3, 3].  The generator checks in float64, on the fp32 flow, that every coarse sampling
                   coordinate at every level is at least 1e-3 away from an integer (the validity bounds -1, Ws/f, Hs/f are
                   integers) and that every coarse difference gen_l - pool_l(target) of the 4-channel pair is at least 1e-5
                   away from 0 (the absolute value's kink; channels 0..C-1 of the pair are the C-channel operands, so this covers
                   every C).  Top-level blocks that miss are drawn again with the next seed until all hold; then it is asserted.
                   No element is left out of any comparison.
  dyadic           constant over each 2^L x 2^L block, values multiples of 2^L / 4: every coarse coordinate is a multiple of 1/4, so
                   floors and validity decisions are the same in fp32 and fp64.  Exact integers, exactly -1, exactly Ws/f and
                   points far outside are included (forced where the shape has four blocks or more)."""
import functools

import numpy as np

from dynamic_multiview_3d_amd import metrics

SHAPES = {'one1': (1, 2, 2, 1), 'one3': (1, 8, 8, 3), 'edge': (2, 40, 24, 3), 'inner': (2, 96, 96, 2), 'nonsq': (2, 24, 40, 3, 40, 24),
          'views': (2, 16, 48, 1)}
FAMILIES = ('smooth', 'random', 'dyadic')
CHANNELS = (1, 3, 4)
KINDS = (2, 1)
WEIGHTS = (1.0, 0.5, 0.25)              # w_1 .. w_3; a case with fewer levels takes the first L


def dims(case):
    s = SHAPES[case]
    n, h, w, levels = s[:4]
    hs, ws = s[4:] if len(s) == 6 else (h, w)
    return n, h, w, levels, hs, ws


def channels_of(case):
    return (1, 3) if case == 'views' else CHANNELS


@functools.lru_cache(maxsize=None)
def images(case):
    """(src [N,Hs,Ws,4], target [N,H,W,4]) float32: a smooth pattern plus noise, in [0, 1]; a C-channel operand is the first C
    channels."""
    n, h, w, _, hs, ws = dims(case)
    seed = sum(map(ord, case))

    def image(rng, hh, ww):
        y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
        base = 0.5 + 0.25 * np.sin(x / 5.0 + np.arange(4)[:, None, None]) * np.cos(y / 7.0)
        return (0.6 * base.transpose(1, 2, 0)[None] + 0.4 * rng.uniform(0, 1, (n, hh, ww, 4))).astype(np.float32)
    src, tgt = image(np.random.default_rng(seed), hs, ws), image(np.random.default_rng(seed + 1), h, w)
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt


def _pool(x, f):
    n, h, w, c = x.shape
    return x.astype(np.float64).reshape(n, h // f, f, w // f, f, c).mean(axis=(2, 4))


def clearance(case, flow):
    """(smallest distance of a coarse coordinate from an integer, smallest |coarse difference|, mask of the top-level blocks that
    hold a coordinate closer than 1e-3 or a difference smaller than 1e-5), in float64 on the given fp32 flow."""
    n, h, w, levels, hs, ws = dims(case)
    src, tgt = images(case)
    top = 1 << levels
    bad = np.zeros((n, h // top, w // top), bool)
    cmin, dmin = np.inf, np.inf
    for l in range(1, levels + 1):
        f = 1 << l
        fl = _pool(flow, f) / f
        ii, jj = np.meshgrid(np.arange(h // f, dtype=np.float64), np.arange(w // f, dtype=np.float64), indexing='ij')
        x, y = fl[..., 0] + ii, fl[..., 1] + jj
        dist = np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y)))
        s = _pool(src, f)
        valid, dx, dy, iff, icc, ifc, icf = metrics._bilinear_taps(s, x, y)
        gen = np.where(valid[..., None], dx * dy * iff + (1 - dx) * (1 - dy) * icc + dx * (1 - dy) * ifc + (1 - dx) * dy * icf, 0.0)
        diff = np.abs(gen - _pool(tgt, f)).min(axis=3)
        cmin, dmin = min(cmin, dist.min()), min(dmin, diff.min())
        miss = (dist < 1e-3) | (diff < 1e-5)
        r = top // f
        bad |= miss.reshape(n, h // top, r, w // top, r).any(axis=(2, 4))
    return cmin, dmin, bad


@functools.lru_cache(maxsize=None)
def flow(case, family):
    """[N,H,W,2] float32, read-only."""
    n, h, w, levels, hs, ws = dims(case)
    top = 1 << levels
    seed = sum(map(ord, case + family))

    def draw(k):
        rng = np.random.default_rng(seed + k)
        if family == 'smooth':
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            f = np.stack([2.0 * np.sin(x / 17.0 + 0.3) * np.cos(y / 23.0) + 0.3, 1.5 * np.cos(x / 29.0) + 0.5 * np.sin(y / 11.0 + 1.0)], -1)
            return (f[None] * np.linspace(1.0, 0.6, n)[:, None, None, None] + rng.normal(0, 0.05, (n, h, w, 2))).astype(np.float32)
        return rng.uniform(-3, 3, (n, h, w, 2)).astype(np.float32)

    if family == 'dyadic':
        rng = np.random.default_rng(seed)
        q = top / 4.0
        span = int(max(h, w, hs, ws) / q) // 2 + 2            # about half of the draws land inside the source
        blocks = rng.integers(-span, span + 1, (n, h // top, w // top, 2)).astype(np.float64) * q
        if blocks[0, :, :, 0].size >= 4:
            flat = blocks[0].reshape(-1, 2)
            bi = lambda k: (k // (w // top), k % (w // top))          # block k -> its (I, J) at the top level
            flat[0] = (-1.0 - bi(0)[0]) * top, 0.0                        # x exactly -1
            flat[1] = (ws / top - bi(1)[0]) * top, 0.0                    # x exactly Ws / f
            flat[2] = 0.0, (hs / top - bi(2)[1]) * top                    # y exactly Hs / f
            flat[3] = 1000.0 * top, -1000.0 * top                         # far outside
        out = np.repeat(np.repeat(blocks, top, axis=1), top, axis=2).astype(np.float32)
    else:
        out = draw(0)
        for k in range(1, 200):
            bad = clearance(case, out)[2]
            if not bad.any():
                break
            mask = np.repeat(np.repeat(bad, top, axis=1), top, axis=2)
            out[mask] = draw(k)[mask]
        cmin, dmin, bad = clearance(case, out)
        assert not bad.any() and cmin >= 1e-3 and dmin >= 1e-5, (case, family, cmin, dmin)
    out.setflags(write=False)
    return out


def weights(case):
    return list(WEIGHTS[:dims(case)[3]])


@functools.lru_cache(maxsize=None)
def reference(case, family, c, kind):
    """(value64, grad64, levels64, value32, grad32, levels32) of the twin, computed once and shared; the arrays are read-only."""
    src, tgt = images(case)
    levels = dims(case)[3]
    out = []
    for dt in (np.float64, np.float32):
        v, g, lv = metrics.multiscale_warp_loss_host(src[..., :c], flow(case, family), tgt[..., :c], levels, weights(case), kind, dt)
        g.setflags(write=False)
        lv.setflags(write=False)
        out += [float(v), g, lv]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def transposed_pair(side):
    """(src, target) [2,side,side,3] float32 with values that are multiples of 1/256 and target = src transposed: zero flow then
    gives gen_l == pool_l(target) at every level, and pooling is exact in any order."""
    a = np.random.default_rng(side).integers(0, 257, (2, side, side, 3)).astype(np.float32) / np.float32(256)
    b = np.ascontiguousarray(a.transpose(0, 2, 1, 3))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def within_rule(label, got_v, got_g, ref):
    """Prints every figure, then asserts the tolerance rule: at most 4 x the float32-twin-to-float64 gap, floors 2e-6 absolute
    (value) and 2e-6 of the float64 gradient's L2 norm / largest magnitude; the gradient's relative L2 error at most 1e-3."""
    v64, g64, _, v32, g32, _ = ref
    got_g = np.asarray(got_g, np.float64)
    v_err, v_gap = abs(float(got_v) - v64), abs(v32 - v64)
    err, gap = got_g - g64, g32.astype(np.float64) - g64
    e2, g2, n2 = np.linalg.norm(err), np.linalg.norm(gap), np.linalg.norm(g64)
    em, gm, nm = np.abs(err).max(), np.abs(gap).max(), np.abs(g64).max()
    print('%-30s value %.8f err %.2e gap %.2e | grad L2 err %.2e gap %.2e norm %.2e rel %.2e | max err %.2e gap %.2e max %.2e'
          % (label, v64, v_err, v_gap, e2, g2, n2, e2 / n2 if n2 else 0.0, em, gm, nm))
    assert np.all(np.isfinite(got_g)) and np.isfinite(got_v), label
    assert v_err <= max(4 * v_gap, 2e-6), (label, v_err, v_gap)
    assert e2 <= max(4 * g2, 2e-6 * n2), (label, e2, g2)
    assert em <= max(4 * gm, 2e-6 * nm), (label, em, gm)
    assert e2 <= 1e-3 * n2, (label, e2, n2)
