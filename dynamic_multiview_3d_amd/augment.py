"""Colour augmentation of training batches: brightness, saturation, hue and contrast, ONE pointwise colour map per sample applied to
all of the sample's colour views (source view, target view, the per-object target renders: they show the same surfaces, so they
must get the same map, the contrast stage's pivot included); masks, depth maps and displacements are never touched.

The reference has no augmentation of any kind and TensorFlow cannot be run here, so nothing below was ever compared with
tf.image.random_*: the contract is the project's own (include/mv3d_hip.h, DESIGN.md input path), `color_augment_host` restates it
in numpy float32 and is the authority for the device code (csrc/color_augment.hip, mv3d_color_augment), which it equals bitwise --
the pivot's summation order included.

conf keys (absent, None or 0 = that stage is off; with all of them off nothing is built, allocated or launched):
    augment_brightness  b          finite, 0 < b <= 1       db ~ U[-b, b)       c = c + db
    augment_saturation  (lo, hi)   finite, 0 <= lo < hi     fs ~ U[lo, hi)      s = clip(s * fs) in HSV
    augment_hue         h          finite, 0 < h <= 0.5     dh ~ U[-h, h)       h = frac(h + dh) in HSV
    augment_contrast    (lo, hi)   finite, 0 <= lo < hi     fc ~ U[lo, hi)      c = (c - pivot) * fc + pivot
    augment_seed        int        default 0                the generator is np.random.default_rng([augment_seed, rank])
The order is brightness, saturation and hue (one HSV round trip), contrast, clip to [0, 1]; a stage that is off is skipped, not run
with a neutral value (the HSV round trip is not the identity in fp32).  The clip happens whenever any stage runs, so a bicubic
overshoot of the reader's resize is clipped, too.

Geometric augmentation (the second half of this file): ONE left-right flip, centred zoom-in and window shift per sample, applied
to ALL of the sample's views, masks and depth maps included, and the displacement's azimuth negated under a flip.  These three are
exact for a pinhole camera on a turntable (the mirrored scene, a longer focal length, a moved principal point): the relative pose
disp = (el1 - el0, az1 - az0) the network is told stays true, as (el1 - el0, -(az1 - az0)) under the mirror; fixed lights are not
reflected, the approximation the colour stage makes, too.  In-plane rotation is NOT in the set (rolling both cameras changes their
relative rotation to something disp cannot express), nor is zoom-out (it would need pixels outside the render).  The contract is
include/mv3d_hip.h's (mv3d_geom_augment), `geom_augment_host` its numpy twin and the authority, which the device equals bitwise.
    augment_flip   p       finite, 0 < p <= 1       m = u0 < p
    augment_zoom   zmax    finite, 1 < zmax <= 4    s = 1 + (zmax - 1) * u1
    augment_shift  t       finite, 0 < t <= 1       ox = (2 u2 - 1) * t * cx * (1 - 1/s), oy likewise with cy and u3; needs augment_zoom
The generator is the stage's own, np.random.default_rng([augment_seed, rank, 1]): the colour stage's stream does not depend on
these keys.  Order in the input path: conversion / resize, colour, geometry, pair swap.
"""
import ctypes as C

import numpy as np

from . import _lib
from .graph import _block_sum_rule

BRIGHTNESS, SATURATION, HUE, CONTRAST = _lib.AUG_BRIGHTNESS, _lib.AUG_SATURATION, _lib.AUG_HUE, _lib.AUG_CONTRAST
ALL_STAGES = BRIGHTNESS | SATURATION | HUE | CONTRAST
KEYS = ('augment_brightness', 'augment_saturation', 'augment_hue', 'augment_contrast')
NEUTRAL = np.array([0.0, 1.0, 0.0, 1.0], np.float32)        # [brightness delta, saturation factor, hue delta, contrast factor]
CHUNK = 4096                # pixels per chunk of the pivot's sums (CA_CHUNK of csrc/color_augment.hip): 256 threads x 4 quads x 4 pixels
MAX_VIEWS = 8

_f = np.float32


# ---------------------------------------------------------------------------- conf
def _off(v):
    return v is None or (not isinstance(v, (bool, tuple, list, np.ndarray)) and v == 0)


def _scalar(conf, key, hi):
    v = conf.get(key)
    if _off(v):
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("conf[%r] must be a number in (0, %g] (or 0 / None for off), got %r" % (key, hi, v))
    v = float(v)
    if not np.isfinite(v) or not 0.0 < v <= hi:
        raise ValueError("conf[%r] must be finite and in (0, %g] (or 0 / None for off), got %r" % (key, hi, conf[key]))
    return v


def _range(conf, key):
    v = conf.get(key)
    if _off(v):
        return None
    ok = isinstance(v, (tuple, list, np.ndarray)) and len(v) == 2 and \
        all(isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) for x in v)
    if not ok:
        raise ValueError("conf[%r] must be (lo, hi), two numbers (or 0 / None for off), got %r" % (key, v))
    lo, hi = float(v[0]), float(v[1])
    if not (np.isfinite(lo) and np.isfinite(hi)) or not 0.0 <= lo < hi:
        raise ValueError("conf[%r] must be finite with 0 <= lo < hi, got %r" % (key, v))
    return lo, hi


def _seed(conf):
    seed = conf.get('augment_seed')
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("conf['augment_seed'] must be a non-negative integer, got %r" % (seed,))
    return int(seed)


class AugmentSpec:
    """The parsed keys: stages (the MV3D_AUG_* mask), lo / hi (float64 [4]: the range each column is drawn from) and seed."""

    def __init__(self, stages, lo, hi, seed):
        self.stages, self.lo, self.hi, self.seed = stages, lo, hi, seed

    @property
    def enabled(self):
        return self.stages != 0


def augment_from_conf(conf):
    """conf -> AugmentSpec; raises ValueError on a bool, a wrong arity, NaN / inf or a value out of range, before any device work."""
    if isinstance(conf, AugmentSpec):
        return conf
    b, s, h, c = _scalar(conf, 'augment_brightness', 1.0), _range(conf, 'augment_saturation'), _scalar(conf, 'augment_hue', 0.5), \
        _range(conf, 'augment_contrast')
    seed = _seed(conf)
    lo, hi = NEUTRAL.astype(np.float64), NEUTRAL.astype(np.float64)
    stages = 0
    for col, bit, rng in ((0, BRIGHTNESS, None if b is None else (-b, b)), (1, SATURATION, s), (2, HUE, None if h is None else (-h, h)),
                          (3, CONTRAST, c)):
        if rng is not None:
            stages |= bit
            lo[col], hi[col] = rng
    return AugmentSpec(stages, lo, hi, int(seed))


def draw_params(rng, n, conf):
    """float32 [n, 4] = [brightness delta, saturation factor, hue delta, contrast factor] per sample.  One rng.random((n, 4)) per
    call whatever the stages, so switching one stage on or off never changes another stage's values; column j is lo_j + (hi_j -
    lo_j) * u in double, rounded to float32 once; a column whose stage is off holds its neutral value (0 or 1)."""
    spec = augment_from_conf(conf)
    u = rng.random((n, 4))
    return (spec.lo + (spec.hi - spec.lo) * u).astype(np.float32)


# ---------------------------------------------------------------------------- the numpy twin
def _clip01(x):
    return np.where(x < 0, _f(0), np.where(x > 1, _f(1), x))


def is_color(a):
    return getattr(a, 'ndim', 0) == 4 and a.shape[-1] == 3


def joint_pivots(colour):
    """float32 [n, 3]: the contrast stage's pivot, the per-channel mean over ALL the given float32 [n, h, w, 3] arrays together, in
    the device's order: per (sample, view, chunk of 4096 pixels) thread t of 256 adds the pixels of its quads t + 256 k, k = 0 .. 3,
    in ascending order to one double per channel (pixels past the image count as 0), the 256 sums go through block_sum / block_total
    (csrc/sum_common.h); the chunk sums are added views ascending, chunks ascending within a view, divided by views * h * w in
    double and rounded to float32 once."""
    n, h, w, _ = colour[0].shape
    P = h * w
    nchunk = -(-P // CHUNK)
    total = np.zeros((n, 3), np.float64)
    for x in colour:
        pad = np.zeros((n, nchunk * CHUNK, 3), np.float64)
        pad[:, :P] = x.reshape(n, P, 3)
        pad = pad.reshape(n, nchunk, 4, 256, 4, 3)          # [sample, chunk, k, thread, pixel of the quad, channel]
        acc = np.zeros((n, nchunk, 256, 3), np.float64)
        for k in range(4):
            for j in range(4):
                acc = acc + pad[:, :, k, :, j, :]
        part = _block_sum_rule(np.ascontiguousarray(acc.transpose(0, 1, 3, 2)))      # [sample, chunk, channel]
        for c in range(nchunk):
            total = total + part[:, c]
    return (total / float(len(colour) * P)).astype(np.float32)


def color_map_host(x, params, stages, pivot=None):
    """The colour map of the contract on one float32 array [n, ..., 3] with params float32 [n, 4] (and pivot float32 [n, 3] for
    the contrast stage): every operation a float32 operation in the device's order."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    bc = (n,) + (1,) * (x.ndim - 2)
    p = np.asarray(params, np.float32).reshape(n, 4)
    db, fs, dh, fc = (p[:, j].reshape(bc) for j in range(4))
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if stages & BRIGHTNESS:
            r, g, b = r + db, g + db, b + db
        if stages & (SATURATION | HUE):
            r, g, b = _clip01(r), _clip01(g), _clip01(b)
            v = np.where(r > g, r, g)
            v = np.where(v > b, v, b)
            mn = np.where(r < g, r, g)
            mn = np.where(mn < b, mn, b)
            rng = v - mn
            s = np.where(v > 0, rng / v, _f(0))
            norm = _f(1) / (_f(6) * rng)
            h = np.where(r == v, (g - b) * norm, np.where(g == v, (b - r) * norm + _f(2) / _f(6), (r - g) * norm + _f(4) / _f(6)))
            h = np.where(rng <= 0, _f(0), h)
            h = np.where(h < 0, h + _f(1), h)
            if stages & SATURATION:
                s = _clip01(s * fs)
            if stages & HUE:
                h = h + dh
            h = h - np.floor(h)
            c = s * v
            m = v - c
            d = h * _f(6)
            k = np.minimum(d.astype(np.int32), 5)           # h can round to exactly 1.0
            f = d - _f(2) * np.floor(d / _f(2))
            xx = c * (_f(1) - np.abs(f - _f(1)))
            zero = np.zeros_like(c)
            r = m + np.where((k == 0) | (k == 5), c, np.where((k == 1) | (k == 4), xx, zero))
            g = m + np.where((k == 1) | (k == 2), c, np.where((k == 0) | (k == 3), xx, zero))
            b = m + np.where((k == 3) | (k == 4), c, np.where((k == 2) | (k == 5), xx, zero))
        if stages & CONTRAST:
            pv = np.asarray(pivot, np.float32).reshape(n, 3)
            pr, pg, pb = (pv[:, j].reshape(bc) for j in range(3))
            r, g, b = (r - pr) * fc + pr, (g - pg) * fc + pg, (b - pb) * fc + pb
        out = np.stack([_clip01(r), _clip01(g), _clip01(b)], axis=-1)
    assert out.dtype == np.float32
    return out


def color_augment_host(views, params, stages):
    """The numpy twin of mv3d_color_augment.  views: a list of arrays; the float32 [n, h, w, 3] ones are the colour views and come
    back as new arrays, every other array (single-channel images, 2-D inputs) comes back as the same object.  params: float32
    [n, 4]; stages: the MV3D_AUG_* mask (not 0).  Bitwise the device's result."""
    stages = int(stages)
    if stages == 0 or stages & ~ALL_STAGES:
        raise ValueError("color_augment_host: stage mask %#x (no stage, or unknown bits)" % stages)
    colour = [np.asarray(v) for v in views if is_color(v)]
    if not colour:
        raise ValueError("color_augment_host: no colour view (float32 [n, h, w, 3]) among the inputs")
    if any(c.dtype != np.float32 or c.shape != colour[0].shape for c in colour):
        raise ValueError("color_augment_host: the colour views must be float32 arrays of one shape")
    if len(colour) > MAX_VIEWS:
        raise ValueError("color_augment_host: %d colour views, 1 .. %d supported" % (len(colour), MAX_VIEWS))
    pivot = joint_pivots(colour) if stages & CONTRAST else None
    return [color_map_host(v, params, stages, pivot) if is_color(v) else v for v in views]


# ---------------------------------------------------------------------------- the stage of the input path
class ColorAugment:
    """The colour stage of a training input: parses conf's keys, picks the colour views out of input_shapes ({name: (n, ...)}: every
    4-D input with exactly 3 channels, in input_shapes order), owns the generator, the device workspace and a pinned ring for the
    parameters.  `apply(batch, stream)` draws one parameter row per sample, uploads it and launches mv3d_color_augment in place on
    the batch's colour tensors; with device='cpu' it calls the twin and replaces the tensors in `batch`.  One instance serves one
    stream: the workspace is reused from call to call in stream order.  `enabled` is false when no stage key is set (apply is then
    a no-op and nothing is allocated).  seed overrides conf['augment_seed']."""

    def __init__(self, conf, input_shapes, device='cpu', seed=None, rank=0, ring=4):
        self.spec = augment_from_conf(conf)
        self.stages = self.spec.stages
        self.enabled = self.spec.enabled
        self.names = []
        self.params = None                  # the last call's float32 [n, 4], for logs and tests
        if not self.enabled:
            return
        for name, shape in input_shapes.items():
            if len(shape) == 4:
                if shape[-1] == 3:
                    self.names.append(name)
                elif shape[-1] != 1:
                    raise ValueError("colour augmentation (conf['augment_*']) does not fit input %r with %d channels: image inputs "
                                     "must have 1 (left alone) or 3 (colour) channels" % (name, shape[-1]))
        if not self.names:
            raise ValueError("colour augmentation (conf['augment_*']) needs an input of shape [n, h, w, 3]; have %s"
                             % {k: tuple(s) for k, s in input_shapes.items()})
        shapes = {tuple(input_shapes[k]) for k in self.names}
        if len(shapes) != 1:
            raise ValueError("colour augmentation (conf['augment_*']): the colour inputs differ in shape: %s" % sorted(shapes))
        if len(self.names) > MAX_VIEWS:
            raise ValueError("colour augmentation (conf['augment_*']): %d colour inputs, at most %d supported" % (len(self.names), MAX_VIEWS))
        self.n, self.h, self.w, _ = shapes.pop()
        self.rng = np.random.default_rng([self.spec.seed if seed is None else int(seed), int(rank)])
        import torch
        self.device = torch.device(device)
        self.cuda = self.device.type == 'cuda'
        if self.cuda:
            self.lib = _lib.lib()
            self.ws_bytes = int(self.lib.color_augment_workspace_bytes(self.n, len(self.names), self.h, self.w))
            self.ws = torch.empty(max(self.ws_bytes // 8, 2), dtype=torch.float64, device=self.device)
            # [pinned params, device params, event of the upload]: a pinned row is rewritten only after its upload has completed
            self.ring = [[torch.empty((self.n, 4), dtype=torch.float32).pin_memory(),
                          torch.empty((self.n, 4), dtype=torch.float32, device=self.device), None] for _ in range(max(int(ring), 2))]
            self.slot = 0

    def draw(self):
        self.params = draw_params(self.rng, self.n, self.spec)
        return self.params

    def apply(self, batch, stream=None):
        """batch: {input name: tensor}; the colour tensors (float32, contiguous, [n, h, w, 3]) are changed in place on the device,
        replaced in the dict on the CPU.  stream: a torch.cuda.Stream, None = the current one.  Returns batch."""
        if not self.enabled:
            return batch
        import torch
        params = self.draw()
        tensors = [batch[k] for k in self.names]
        for k, t in zip(self.names, tensors):
            if tuple(t.shape) != (self.n, self.h, self.w, 3) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("colour augmentation: input %r is not a contiguous float32 [%d, %d, %d, 3] tensor" % (k, self.n, self.h, self.w))
        if not self.cuda:
            for k, a in zip(self.names, color_augment_host([t.numpy() for t in tensors], params, self.stages)):
                batch[k] = torch.from_numpy(a)
            return batch
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        host, dev, ev = slot = self.ring[self.slot % len(self.ring)]
        self.slot += 1
        if ev is not None:
            ev.synchronize()
        host.numpy()[...] = params
        with torch.cuda.stream(stream):
            dev.copy_(host, non_blocking=True)
            slot[2] = torch.cuda.Event()
            slot[2].record(stream)
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        self.lib.color_augment(ptrs, len(tensors), self.n, self.h, self.w, dev.data_ptr(), self.stages, self.ws.data_ptr(), self.ws_bytes,
                               stream.cuda_stream)
        return batch


class AugmentedData:
    """A batch source whose next() hands out an augmented COPY of source.next(): the colour inputs are copied into buffers of this
    object's own (allocated once) and augmented there on the current stream; everything else is passed through.  The source's own
    tensors stay as they are -- train.SyntheticData cycles a small pool, which would otherwise be augmented over and over."""

    def __init__(self, source, augment):
        self.source, self.augment = source, augment
        self.bufs = {}

    def next(self):
        batch = dict(self.source.next())
        if not self.augment.enabled:
            return batch
        for k in self.augment.names:
            if k not in self.bufs:
                import torch
                self.bufs[k] = torch.empty_like(batch[k])
            self.bufs[k].copy_(batch[k])
            batch[k] = self.bufs[k]
        return self.augment.apply(batch)

    def __getattr__(self, name):
        return getattr(self.source, name)


# ============================================================================ geometric augmentation: flip, zoom, shift
GEOM_KEYS = ('augment_flip', 'augment_zoom', 'augment_shift')
GEOM_MAX_VIEWS = 16
GEOM_MAX_ZOOM = 4.0
DISP_NAMES = ('disp', 'displacement')


class GeomSpec:
    """The parsed keys: flip (the probability p), zoom (zmax), shift (t) -- None for a stage that is off -- and seed."""

    def __init__(self, flip, zoom, shift, seed):
        self.flip, self.zoom, self.shift, self.seed = flip, zoom, shift, seed

    @property
    def enabled(self):
        return self.flip is not None or self.zoom is not None


def geom_from_conf(conf):
    """conf -> GeomSpec; raises ValueError on a bool, NaN / inf, a value out of range or augment_shift without augment_zoom (without
    zoom the window has no slack to move in), before any device work."""
    if isinstance(conf, GeomSpec):
        return conf
    flip, shift = _scalar(conf, 'augment_flip', 1.0), _scalar(conf, 'augment_shift', 1.0)
    zoom = conf.get('augment_zoom')
    if _off(zoom):
        zoom = None
    else:
        if isinstance(zoom, bool) or not isinstance(zoom, (int, float, np.integer, np.floating)):
            raise ValueError("conf['augment_zoom'] must be a number in (1, %g] (or 0 / None for off), got %r" % (GEOM_MAX_ZOOM, zoom))
        zoom = float(zoom)
        if not np.isfinite(zoom) or not 1.0 < zoom <= GEOM_MAX_ZOOM:
            raise ValueError("conf['augment_zoom'] must be finite and in (1, %g] (zoom-in only; 0 / None for off), got %r"
                             % (GEOM_MAX_ZOOM, conf['augment_zoom']))
    if shift is not None and zoom is None:
        raise ValueError("conf['augment_shift'] needs conf['augment_zoom']: without zoom the window fills the image and cannot move")
    return GeomSpec(flip, zoom, shift, _seed(conf))


def draw_geom_params(rng, n, spec, h, w):
    """float32 [n, 4] = [m, inv, cxo, cyo] per sample (include/mv3d_hip.h, mv3d_geom_augment).  One rng.random((n, 4)) per call
    whatever the stages, so switching one stage never changes another's draws; float64 arithmetic, rounded to float32 once.  A stage
    that is off gives its neutral value: m = 0, inv = 1, cxo = cx, cyo = cy.  |ox| <= cx (1 - 1/s) keeps the unclamped window inside
    the image; the kernel's clamp only absorbs rounding."""
    spec = geom_from_conf(spec)
    u = rng.random((n, 4))
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    m = (u[:, 0] < spec.flip).astype(np.float64) if spec.flip is not None else np.zeros(n)
    s = 1.0 + (spec.zoom - 1.0) * u[:, 1] if spec.zoom is not None else np.ones(n)
    inv = 1.0 / s
    t = spec.shift if spec.shift is not None else 0.0
    ox = (2.0 * u[:, 2] - 1.0) * t * cx * (1.0 - inv)
    oy = (2.0 * u[:, 3] - 1.0) * t * cy * (1.0 - inv)
    return np.stack([m, inv, cx + ox, cy + oy], axis=1).astype(np.float32)


def geom_source_coords(params, size, axis, clamp=True):
    """float32 [n, size]: the source coordinate of every output coordinate along x (axis 1; mirrored where m is set) or y (axis 0),
    in the contract's fp32 order; clamp=False leaves out the clamp to [0, size - 1] (for tests of the offset bound)."""
    p = np.asarray(params, np.float32)
    n = p.shape[0]
    c = _f(0.5) * _f(size - 1)
    o = np.arange(size, dtype=np.float32)[None, :].repeat(n, 0)
    if axis == 1:
        o = np.where(p[:, 0:1] != 0, _f(size - 1) - o, o)
    s = (o - c) * p[:, 1:2] + p[:, 2:3] if axis == 1 else (o - c) * p[:, 1:2] + p[:, 3:4]
    if clamp:
        s = np.minimum(np.maximum(s, _f(0)), _f(size - 1))
    assert s.dtype == np.float32
    return s


def geom_augment_host(views, disp, params):
    """The numpy twin of mv3d_geom_augment.  views: a list of float32 arrays [n, h, w, c], c = 3 (bilinear) or 1 (nearest), one
    (n, h, w) for all; disp: float32 [n, 2] or None; params: finite float32 [n, 4] = [m, inv, cxo, cyo].  Returns (new views, new
    disp); the inputs are left alone.  Every operation is a float32 operation in the contract's order: bitwise the device's result."""
    views = [np.asarray(v) for v in views]
    if not 1 <= len(views) <= GEOM_MAX_VIEWS:
        raise ValueError("geom_augment_host: %d views, 1 .. %d supported" % (len(views), GEOM_MAX_VIEWS))
    if any(v.ndim != 4 or v.dtype != np.float32 or v.shape[:3] != views[0].shape[:3] or v.shape[3] not in (1, 3) for v in views):
        raise ValueError("geom_augment_host: the views must be float32 [n, h, w, 1 or 3] arrays of one (n, h, w)")
    n, h, w, _ = views[0].shape
    p = np.asarray(params, np.float32)
    if p.shape != (n, 4) or not np.isfinite(p).all():
        raise ValueError("geom_augment_host: params must be finite float32 [%d, 4]" % n)
    xs, ys = geom_source_coords(p, w, 1), geom_source_coords(p, h, 0)
    x0f, y0f = np.floor(xs), np.floor(ys)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (xs - x0f)[:, None, :, None], (ys - y0f)[:, :, None, None]
    xi = np.minimum(np.floor(xs + _f(0.5)).astype(np.int64), w - 1)
    yi = np.minimum(np.floor(ys + _f(0.5)).astype(np.int64), h - 1)
    i = np.arange(n)[:, None, None]
    outs = []
    for v in views:
        if v.shape[3] == 1:
            out = v[i, yi[:, :, None], xi[:, None, :]]
        else:
            a, b = v[i, y0[:, :, None], x0[:, None, :]], v[i, y0[:, :, None], x1[:, None, :]]
            c, d = v[i, y1[:, :, None], x0[:, None, :]], v[i, y1[:, :, None], x1[:, None, :]]
            with np.errstate(over='ignore', invalid='ignore'):
                top = a + (b - a) * fx
                bot = c + (d - c) * fx
                out = top + (bot - top) * fy
        assert out.dtype == np.float32 and out.shape == v.shape
        outs.append(np.ascontiguousarray(out))
    if disp is not None:
        d = np.asarray(disp)
        if d.shape != (n, 2) or d.dtype != np.float32:
            raise ValueError("geom_augment_host: disp must be float32 [%d, 2]" % n)
        disp = d.copy()
        disp[:, 1] = np.where(p[:, 0] != 0, np.negative(d[:, 1]), d[:, 1])
    return outs, disp


class GeomAugment:
    """The geometric stage of a training input, modelled on ColorAugment: parses conf's keys, picks every 4-D input of
    input_shapes ({name: (n, ...)}) with 1 or 3 channels, in input_shapes order (any other channel count is refused), and the one
    [n, 2] input named `disp` or `displacement`; owns the generator, np.random.default_rng([seed, rank, 1]), and a pinned ring for
    the parameters.  `apply(batch, stream)` draws one parameter row per sample, uploads it and launches mv3d_geom_augment: the views
    are replaced in `batch` by freshly written tensors, the displacement is changed in place; with device='cpu' it calls the twin.
    `enabled` is false when no stage key is set (apply is then a no-op and nothing is allocated).  seed overrides
    conf['augment_seed']."""

    def __init__(self, conf, input_shapes, device='cpu', seed=None, rank=0, ring=4):
        self.spec = geom_from_conf(conf)
        self.enabled = self.spec.enabled
        self.names, self.channels, self.disp_name = [], [], None
        self.params = None                  # the last call's float32 [n, 4], for logs and tests
        if not self.enabled:
            return
        for name, shape in input_shapes.items():
            if len(shape) == 4:
                if shape[-1] not in (1, 3):
                    raise ValueError("geometric augmentation (conf['augment_flip' / '_zoom' / '_shift']) does not fit input %r with %d "
                                     "channels: image inputs must have 1 or 3 channels" % (name, shape[-1]))
                self.names.append(name)
                self.channels.append(int(shape[-1]))
        if not self.names:
            raise ValueError("geometric augmentation (conf['augment_flip' / '_zoom' / '_shift']) needs an image input; have %s"
                             % {k: tuple(s) for k, s in input_shapes.items()})
        if len(self.names) > GEOM_MAX_VIEWS:
            raise ValueError("geometric augmentation: %d image inputs, at most %d supported" % (len(self.names), GEOM_MAX_VIEWS))
        sizes = {tuple(input_shapes[k][:3]) for k in self.names}
        if len(sizes) != 1:
            raise ValueError("geometric augmentation: the image inputs differ in shape: %s" % sorted(sizes))
        self.n, self.h, self.w = sizes.pop()
        found = [k for k in DISP_NAMES if k in input_shapes]
        if len(found) != 1 or tuple(input_shapes[found[0]]) != (self.n, 2):
            raise ValueError("geometric augmentation needs exactly one [%d, 2] input named %s (a flip negates its azimuth); have %s"
                             % (self.n, ' or '.join(DISP_NAMES), {k: tuple(s) for k, s in input_shapes.items()}))
        self.disp_name = found[0]
        self.rng = np.random.default_rng([self.spec.seed if seed is None else int(seed), int(rank), 1])
        import torch
        self.device = torch.device(device)
        self.cuda = self.device.type == 'cuda'
        if self.cuda:
            self.lib = _lib.lib()
            self.c_channels = (C.c_int * len(self.names))(*self.channels)
            # [pinned params, device params, event of the upload]: a pinned row is rewritten only after its upload has completed
            self.ring = [[torch.empty((self.n, 4), dtype=torch.float32).pin_memory(),
                          torch.empty((self.n, 4), dtype=torch.float32, device=self.device), None] for _ in range(max(int(ring), 2))]
            self.slot = 0

    def draw(self):
        self.params = draw_geom_params(self.rng, self.n, self.spec, self.h, self.w)
        return self.params

    def apply(self, batch, stream=None):
        """batch: {input name: tensor}; the views (float32, contiguous, [n, h, w, 1 or 3]) are replaced in the dict by new tensors,
        the displacement (float32, contiguous, [n, 2]) is changed in place.  stream: a torch.cuda.Stream, None = the current one.
        Returns batch."""
        if not self.enabled:
            return batch
        import torch
        params = self.draw()
        tensors = [batch[k] for k in self.names]
        disp = batch[self.disp_name]
        for k, t, c in zip(self.names + [self.disp_name], tensors + [disp], [(self.h, self.w, c) for c in self.channels] + [(2,)]):
            if tuple(t.shape) != (self.n,) + c or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("geometric augmentation: input %r is not a contiguous float32 %s tensor" % (k, [self.n] + list(c)))
        if not self.cuda:
            outs, d = geom_augment_host([t.numpy() for t in tensors], disp.numpy(), params)
            for k, a in zip(self.names, outs):
                batch[k] = torch.from_numpy(a)
            disp.numpy()[...] = d
            return batch
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        host, dev, ev = slot = self.ring[self.slot % len(self.ring)]
        self.slot += 1
        if ev is not None:
            ev.synchronize()
        host.numpy()[...] = params
        with torch.cuda.stream(stream):
            dev.copy_(host, non_blocking=True)
            slot[2] = torch.cuda.Event()
            slot[2].record(stream)
            outs = [torch.empty_like(t) for t in tensors]        # on `stream`: a source's block is reused only behind the kernel
        src = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        dst = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in outs])
        self.lib.geom_augment(src, dst, self.c_channels, len(tensors), self.n, self.h, self.w, dev.data_ptr(), disp.data_ptr(),
                              stream.cuda_stream)
        for k, t in zip(self.names, outs):
            batch[k] = t
        return batch


class GeomAugmentedData:
    """A batch source whose next() hands out a geometrically augmented COPY of source.next(): the views come out of place anyway,
    the displacement is copied into a buffer of this object's own before it is changed.  It runs behind AugmentedData (colour
    first: its contrast pivot is a sum in pixel order) and in front of PairSwappedData; the source's tensors stay as they are."""

    def __init__(self, source, augment):
        self.source, self.augment = source, augment
        self.disp = None

    def next(self):
        batch = dict(self.source.next())
        if not self.augment.enabled:
            return batch
        k = self.augment.disp_name
        if self.disp is None:
            import torch
            self.disp = torch.empty_like(batch[k])
        self.disp.copy_(batch[k])
        batch[k] = self.disp
        return self.augment.apply(batch)

    def __getattr__(self, name):
        return getattr(self.source, name)
