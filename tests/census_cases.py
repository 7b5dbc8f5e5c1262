"""The cases of the GPU parity test of the census loss (tests/test_gpu_census_loss.py), shared with the CPU guard of its tolerance
rule (tests/test_census_loss_host.py): shapes per radius, input families, dynamic ranges, and the references, computed once."""
import functools

import numpy as np

from dynamic_multiview_3d_amd import metrics
from tests.test_gpu_metrics import _pair

# (case name) -> (radius, shape [N,H,W,ld])
CASES = {
    'one': (3, (1, 7, 7, 2)),             # one valid pixel
    'rows': (3, (2, 8, 37, 3)),           # two valid rows, W crosses a tile edge
    'narrow': (3, (3, 40, 23, 1)),
    'ragged': (3, (2, 45, 77, 3)),
    'inner': (3, (2, 75, 70, 3)),         # a tile with neighbours on all eight sides
    'views': (3, (2, 33, 43, 4)),         # as the views C=3 at channel 0 and C=1 at channel 3
    'r1_smallest': (1, (1, 3, 3, 1)),
    'r1_ragged': (1, (2, 45, 77, 3)),
    'r2_smallest': (2, (1, 5, 5, 1)),
    'r2_ragged': (2, (2, 45, 77, 3)),
}
FAMILIES = ('noise', 'shift', 'random', 'same')
MAX_VALS = (1.0, 1.5)
EPS = 0.01


def views_of(case):
    return [(0, 3), (3, 1)] if case == 'views' else [(0, CASES[case][1][3])]


@functools.lru_cache(maxsize=None)
def inputs(case, family, max_val):
    a, b = _pair(family, CASES[case][1], seed=sum(map(ord, case + family)))
    if max_val == 1.5:                                        # the mv3d range: (x - 0.5) * 1.5 in [-0.75, 0.75]
        a, b = ((a - np.float32(0.5)) * np.float32(1.5)).astype(np.float32), ((b - np.float32(0.5)) * np.float32(1.5)).astype(np.float32)
    for x in (a, b):
        x.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(case, family, max_val, off, c, weight):
    """(loss64, grad64, loss32, grad32) of the view's channels, computed once and shared; the arrays are read-only."""
    a, b = inputs(case, family, max_val)
    r = CASES[case][0]
    l64, g64 = metrics.census_loss_host(a[..., off:off + c], b[..., off:off + c], max_val, np.float64, weight, r, EPS)
    l32, g32 = metrics.census_loss_host(a[..., off:off + c], b[..., off:off + c], max_val, np.float32, weight, r, EPS)
    for x in (g64, g32):
        x.setflags(write=False)
    return float(l64), g64, float(l32), g32
