"""Shared by tests/test_geom_augment_host.py and tests/test_gpu_geom_augment.py: the shapes, view lists and crafted parameter rows
of mv3d_geom_augment (include/mv3d_hip.h), images and masks, and the conf of the reader tests.  The shard helpers and the input sets
are the colour stage's (tests/color_augment_cases.py)."""
import numpy as np

from dynamic_multiview_3d_amd import augment as A

CONF = {'augment_flip': 0.5, 'augment_zoom': 2.0, 'augment_shift': 1.0}
WIDE = {'augment_flip': 0.5, 'augment_zoom': 4.0, 'augment_shift': 1.0}        # the whole zoom range, for the random rows
# (n, h, w): odd sides and a row shorter than one lane's four pixels; a small square; a width that is no multiple of 4 and spans
# several lanes (and rows that start off a 16-byte boundary); the model's size
SHAPES = [(2, 5, 7), (3, 8, 8), (2, 33, 130), (1, 128, 128)]
VIEW_LISTS = [[3], [3, 1]]
MULTIOBJECT = [3, 1, 1, 3, 3, 3, 1, 1, 1, 1, 1, 1]             # multiobject_appflow.INPUTS, at 16 x 16
CORNERS = [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def row(m, s, tx, ty, h, w):
    """[m, inv, cxo, cyo] of a zoom s with the window moved by the fractions tx, ty in [-1, 1] of its slack: float64, rounded once"""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    inv = 1.0 / s
    return np.array([m, inv, cx + tx * cx * (1.0 - inv), cy + ty * cy * (1.0 - inv)], np.float64).astype(np.float32)


def identity(n, h, w):
    return np.tile(row(0, 1, 0, 0, h, w), (n, 1))


def flip_only(n, h, w):
    return np.tile(row(1, 1, 0, 0, h, w), (n, 1))


def corner(n, h, w, which, m=0):
    """s = zmax = 4 with the window pushed into one corner (t = 1)"""
    tx, ty = CORNERS[which]
    return np.tile(row(m, 4, tx, ty, h, w), (n, 1))


def param_rows(n, h, w, seed=0):
    """[(name, float32 [n, 4])]: identity, flip only, the four corner shifts at s = 4 (the last two mirrored as well), random draws"""
    rng = np.random.default_rng([seed, n, h, w])
    rows = [('identity', identity(n, h, w)), ('flip', flip_only(n, h, w))]
    rows += [('corner %d' % k, corner(n, h, w, k, m=k // 2)) for k in range(4)]
    rows += [('random %d' % k, A.draw_geom_params(rng, n, WIDE, h, w)) for k in range(2)]
    return rows


def images(seed, shape):
    """float32 with overshoot, uniform in [-0.25, 1.25]: what the colour stage's input may hold behind a bicubic resize"""
    return np.random.default_rng(seed).uniform(-0.25, 1.25, shape).astype(np.float32)


def masks(seed, shape):
    return np.random.default_rng(seed).integers(0, 2, shape).astype(np.float32)


def views(seed, n, h, w, channels):
    """one array per entry of `channels`: colour views with overshoot, single-channel views alternately masks and depth-like"""
    out = []
    for k, c in enumerate(channels):
        out.append(images(seed + k, (n, h, w, 3)) if c == 3 else masks(seed + k, (n, h, w, 1)) if k % 2 else images(seed + k, (n, h, w, 1)))
    return out


def disp(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 2)).astype(np.float32)
