"""The cases of the occlusion-masked multi-scale loss, shared by tests/test_masked_multiscale_loss_host.py and
tests/test_gpu_masked_multiscale_loss.py.

Shapes, images, flows, weights and the tolerance rule are those of tests/multiscale_cases.py, unchanged: one1 1x2x2, one3 1x8x8,
edge 2x40x24, inner 2x96x96, nonsq and views are the smallest that reach one coarse pixel, a tile edge, a tile with eight
neighbours, a non-square source and channel-slice views.  Their generators assert that no coarse coordinate is within 1e-3 of an
integer and no coarse difference within 1e-5 of 0; the mask moves neither, so no element is left out of any comparison.

The mask families are those of tests/masked_image_cases.py: ones, zeros, blocks (zero rectangles across the 32-pixel tile edges
and touching the image border, clipped to small images), sparse (30 % ones) and fraction (uniform in [0, 1)).  References come
from the masked twin (metrics.multiscale_warp_loss_host with mask=) at float64 and float32, computed once and read-only."""
import functools

import numpy as np

from dynamic_multiview_3d_amd import metrics
from tests import multiscale_cases as MC

SHAPES, FAMILIES, KINDS = MC.SHAPES, MC.FAMILIES, MC.KINDS
dims, channels_of, images, flow, weights, within_rule, transposed_pair = (MC.dims, MC.channels_of, MC.images, MC.flow, MC.weights,
                                                                          MC.within_rule, MC.transposed_pair)
MASKS = ('ones', 'zeros', 'blocks', 'sparse', 'fraction')
PARITY_MASKS = ('blocks', 'sparse', 'fraction')


def mask_of(family, n, h, w, seed):
    """float32 [n,h,w,1], read-only."""
    rng = np.random.default_rng(seed)
    if family == 'ones':
        m = np.ones((n, h, w, 1), np.float32)
    elif family == 'zeros':
        m = np.zeros((n, h, w, 1), np.float32)
    elif family == 'blocks':
        m = np.ones((n, h, w, 1), np.float32)
        m[:, 27:37, 20:45] = 0              # across the tile edges at 32 in y and x
        m[:, 0:5, max(w - 6, 0):w] = 0      # the top right corner of the image
        m[:, max(h - 4, 0):h, 0:9] = 0      # the bottom left corner
        m[n - 1, :, 60:66] = 0              # a column band across the tile edge at 64, the last image only
        if h <= 8 and w <= 8:               # the corners would cover all of the smallest images: keep one pixel in four
            m[:, 0::2, 0::2] = 1
    elif family == 'sparse':
        m = (rng.uniform(0, 1, (n, h, w, 1)) < 0.3).astype(np.float32)
    elif family == 'fraction':
        m = rng.uniform(0, 1, (n, h, w, 1)).astype(np.float32)
    else:
        raise KeyError(family)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def mask(case, family):
    n, h, w = dims(case)[:3]
    return mask_of(family, n, h, w, sum(map(ord, 'multiscale' + case + family)))


@functools.lru_cache(maxsize=None)
def reference(case, family, c, kind, mask_family):
    """(value64, grad64, levels64, value32, grad32, levels32) of the masked twin (mask_family None: the unmasked twin's, shared with
    tests/multiscale_cases.py), computed once; the arrays are read-only."""
    if mask_family is None:
        return MC.reference(case, family, c, kind)
    src, tgt = images(case)
    levels = dims(case)[3]
    out = []
    for dt in (np.float64, np.float32):
        v, g, lv = metrics.multiscale_warp_loss_host(src[..., :c], flow(case, family), tgt[..., :c], levels, weights(case), kind, dt,
                                                     mask=mask(case, mask_family))
        g.setflags(write=False)
        lv.setflags(write=False)
        out += [float(v), g, lv]
    return tuple(out)
