"""The cases of the masked census and SSIM losses, shared by the GPU parity tests (tests/test_gpu_masked_census_loss.py,
tests/test_gpu_masked_ssim_loss.py) and the CPU guard of their tolerance rule (tests/test_masked_image_losses_host.py): shapes,
input families, mask families, and the references, computed once and read-only.

Census reuses the shapes and inputs of tests/census_cases.py at max_val 1.  The SSIM shapes: the smallest image (one window), one
window row with W crossing a tile edge, ragged edges, a tile with neighbours on several sides."""
import functools

import numpy as np

from dynamic_multiview_3d_amd import metrics
from tests import census_cases
from tests.test_gpu_metrics import _pair

CENSUS_CASES = ('one', 'rows', 'ragged', 'inner', 'views', 'r1_smallest', 'r2_ragged')
SSIM_CASES = {'smallest': (1, 11, 11, 1), 'row': (2, 12, 43, 3), 'ragged': (2, 45, 77, 3), 'inner': (1, 75, 70, 2)}
FAMILIES = ('noise', 'shift', 'random', 'same')
MASKS = ('ones', 'zeros', 'blocks', 'sparse', 'fraction')
MAX_VAL = 1.0
EPS = census_cases.EPS


def shape_of(kind, case):
    """[N,H,W,ld] of the operands."""
    return census_cases.CASES[case][1] if kind == 'census' else SSIM_CASES[case]


def views_of(kind, case):
    """[(channel offset, C)] of the views the case runs."""
    return census_cases.views_of(case) if kind == 'census' else [(0, SSIM_CASES[case][3])]


@functools.lru_cache(maxsize=None)
def inputs(kind, case, family):
    if kind == 'census':
        return census_cases.inputs(case, family, MAX_VAL)
    a, b = _pair(family, SSIM_CASES[case], seed=sum(map(ord, case + family)))
    for x in (a, b):
        x.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def mask(kind, case, family):
    """float32 [N,H,W,1], read-only.  blocks: ones with zero rectangles (clipped to the image) that cross the 32-pixel tile edges
    in both directions and touch the image border; sparse: 30 % ones; fraction: uniform in [0, 1)."""
    n, h, w, _ = shape_of(kind, case)
    rng = np.random.default_rng(sum(map(ord, kind + case + family)))
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
    elif family == 'sparse':
        m = (rng.uniform(0, 1, (n, h, w, 1)) < 0.3).astype(np.float32)
    elif family == 'fraction':
        m = rng.uniform(0, 1, (n, h, w, 1)).astype(np.float32)
    else:
        raise KeyError(family)
    m.setflags(write=False)
    return m


def twin(kind, case, a, b, dtype, weight, m):
    """The numpy twin of the kind on operands that are already the view's channels."""
    if kind == 'census':
        return metrics.census_loss_host(a, b, MAX_VAL, dtype, weight, census_cases.CASES[case][0], EPS, mask=m)
    return metrics.ssim_loss_host(a, b, MAX_VAL, dtype, weight, mask=m)


@functools.lru_cache(maxsize=None)
def reference(kind, case, family, mask_family, off, c, weight=1.0):
    """(loss64, grad64, loss32, grad32) of the view's channels under the mask family (None: the unmasked twin)."""
    a, b = inputs(kind, case, family)
    m = mask(kind, case, mask_family) if mask_family is not None else None
    l64, g64 = twin(kind, case, a[..., off:off + c], b[..., off:off + c], np.float64, weight, m)
    l32, g32 = twin(kind, case, a[..., off:off + c], b[..., off:off + c], np.float32, weight, m)
    for x in (g64, g32):
        x.setflags(write=False)
    return float(l64), g64, float(l32), g32


def allowed(l64, g64, l32, g32, same, weight=1.0):
    """The parity rule of tests/test_gpu_census_loss.py for one case: (loss, gradient L2, gradient max-abs) bounds on the kernel's
    distance from the float64 twin -- 4 x the float32 twin's own gap, with floors of 2e-6 absolute for the loss and 2e-6 of the
    float64 gradient's L2 norm / largest magnitude; 4e-6 * weight absolute for a == b and wherever the float64 gradient is exactly
    zero (a mask that hides every valid pixel: there is no norm to be relative to)."""
    gap = g32.astype(np.float64) - g64
    n2, nm = np.linalg.norm(g64), np.abs(g64).max()
    flat = same or n2 == 0
    return (max(4 * abs(l32 - l64), 4e-6 * weight if flat else 2e-6),
            max(4 * np.linalg.norm(gap), 4e-6 * weight if flat else 2e-6 * n2),
            max(4 * np.abs(gap).max(), 4e-6 * weight if flat else 2e-6 * nm))
