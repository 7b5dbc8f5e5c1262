"""Shared by tests/test_color_augment_host.py and tests/test_gpu_color_augment.py: crafted pixels with the value the contract of
mv3d_color_augment (include/mv3d_hip.h) gives by hand, the conf of the issue's parameter ranges, and tiny TFRecord shards.

The hand values.  S|H below is the HSV round trip with saturation factor fs and hue delta dh; 1/6, 2/6 and 4/6 are the float32
quotients 0.16666667, 0.33333334 and 0.6666667.
  black, white, grey     range = 0: s = 0, h = 0, c = 0, m = v, x = 0 -> (v, v, v)
  primaries, secondaries s = 1, c = 1, m = 0; h = 0, 1/6, 2/6, 1/6 + 2/6 = 0.5, 4/6, 1 - 1/6 = 0.8333333; d = h * 6 rounds to exactly
                         0, 1, 2, 3, 4, 5 (the products are 1.00000003, 2.00000006, 4.00000012 and 4.99999988: all within half an
                         ulp of the integer), so f = 0 or 1, x = 0 or c, and every one of them is a fixed point
  (0.75, 0.75, 0.25)     r == g == max takes the r branch: h = 0.5 * (1 / 3) = 1/6, s = 0.5 / 0.75 = 0.6666667, c = 0.5 (0.50000001
                         rounds), m = 0.25, d = 1, x = c -> (0.75, 0.75, 0.25)
  (1, 0.5 - 2^-24, 0.5)  h = -2^-24 * 0.3333333 = -2e-8, h + 1 rounds to 1.0, h - floor(h) = 0: k = 0, x = 0, s = c = 0.5 + 2^-24,
                         m = 0.5 - 2^-24 -> (1, m, m)
  (1, 0.5, 0.5 - 2^-24)  with dh = -2^-25: h = +2e-8 - 3e-8 = -1e-8, floor = -1, h + 1 rounds to 1.0 and stays: d = 6, (int)d = 6, which
                         without the min would select nothing and give (m, m, m); with it k = 5, f = 6 - 2 * 3 = 0, x = 0 -> (1, m, m)
  red with dh = +-0.5    h = 0.5 (-0.5 - floor(-0.5) = 0.5): d = 3, k = 3, f = 1, x = c = 1 -> (0, 1, 1)
  (0.8, 0.4, 0.2), fs 0  s = 0: c = 0, x = 0, m = v -> (0.8, 0.8, 0.8)
  brightness +-0.25 on (0.125, 0.5, 0.875): exact sums, clipped -> (0.375, 0.75, 1) and (0, 0.25, 0.625)
"""
import numpy as np

from dynamic_multiview_3d_amd import augment as A
from dynamic_multiview_3d_amd import read_tf_records as R

CONF = {'augment_brightness': 0.3, 'augment_saturation': (0.3, 2), 'augment_hue': 0.5, 'augment_contrast': (0.4, 1.8)}
SH = A.SATURATION | A.HUE
E = 2.0 ** -24
_M = 0.5 - E

# (name, pixel, [db, fs, dh, fc], want) -- all under the stage mask SATURATION | HUE
CRAFTED_SH = [
    ('black', (0, 0, 0), (0, 1, 0, 1), (0, 0, 0)),
    ('white', (1, 1, 1), (0, 1, 0, 1), (1, 1, 1)),
    ('grey', (0.5, 0.5, 0.5), (0, 1, 0, 1), (0.5, 0.5, 0.5)),
    ('red', (1, 0, 0), (0, 1, 0, 1), (1, 0, 0)),
    ('green', (0, 1, 0), (0, 1, 0, 1), (0, 1, 0)),
    ('blue', (0, 0, 1), (0, 1, 0, 1), (0, 0, 1)),
    ('yellow', (1, 1, 0), (0, 1, 0, 1), (1, 1, 0)),
    ('cyan', (0, 1, 1), (0, 1, 0, 1), (0, 1, 1)),
    ('magenta', (1, 0, 1), (0, 1, 0, 1), (1, 0, 1)),
    ('r == g == max', (0.75, 0.75, 0.25), (0, 1, 0, 1), (0.75, 0.75, 0.25)),
    ('tiny negative hue', (1, _M, 0.5), (0, 1, 0, 1), (1, _M, _M)),
    ('hue that wraps to exactly 1.0', (1, 0.5, _M), (0, 1, -2.0 ** -25, 1), (1, _M, _M)),
    ('hue + 0.5', (1, 0, 0), (0, 1, 0.5, 1), (0, 1, 1)),
    ('hue - 0.5', (1, 0, 0), (0, 1, -0.5, 1), (0, 1, 1)),
    ('saturation 0', (0.8, 0.4, 0.2), (0, 0, 0, 1), (0.8, 0.8, 0.8)),
]
# under the stage mask BRIGHTNESS
CRAFTED_B = [
    ('brightness above 1', (0.125, 0.5, 0.875), (0.25, 1, 0, 1), (0.375, 0.75, 1)),
    ('brightness below 0', (0.125, 0.5, 0.875), (-0.25, 1, 0, 1), (0, 0.25, 0.625)),
]


def crafted_batch(cases, h=16, w=16, seed=0):
    """(images float32 [len(cases), h, w, 3], params float32 [len(cases), 4], positions): sample i carries case i's parameters;
    EVERY crafted pixel is scattered into every sample's image (random elsewhere), case j at positions[j]."""
    rng = np.random.default_rng(seed)
    n = len(cases)
    x = rng.integers(0, 256, (n, h, w, 3)).astype(np.float32) / np.float32(255)
    pos = rng.choice(h * w, n, replace=False)
    flat = x.reshape(n, h * w, 3)
    for j, (_, px, _, _) in enumerate(cases):
        flat[:, pos[j]] = np.asarray(px, np.float32)
    params = np.array([c[2] for c in cases], np.float32)
    return x, params, pos


def check_crafted(cases, out, pos):
    flat = out.reshape(out.shape[0], -1, 3)
    for i, (name, _, _, want) in enumerate(cases):
        np.testing.assert_array_equal(flat[i, pos[i]], np.asarray(want, np.float32), err_msg=name)


def images(kind, seed, shape):
    """'u8': uint8 / 255; 'over': float32 with overshoot, uniform in [-0.25, 1.25] (where the pivot's summation order matters)"""
    rng = np.random.default_rng(seed)
    if kind == 'u8':
        return rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    return rng.uniform(-0.25, 1.25, shape).astype(np.float32)


APPFLOW = (('image0', 3), ('image1', 3), ('depth_image0', 1), ('depth_image1', 1))      # + disp: the appearance-flow input set


def appflow_shapes(batch, size):
    shapes = {name: (batch, size, size, ch) for name, ch in APPFLOW}
    shapes['disp'] = (batch, 2)
    return shapes


def multiobject_shapes(batch, size):
    from dynamic_multiview_3d_amd.multiobject_appflow import INPUTS
    shapes = {name: (batch, size, size, ch) for name, ch in INPUTS}
    shapes['displacement'] = (batch, 2)
    return shapes


def write_shards(data, shapes, size, nfiles=2, per_file=3, seed=0):
    """nfiles shards of per_file records with every feature of `shapes` at size x size (uint8) or as floats"""
    rng = np.random.default_rng(seed)
    for f in range(nfiles):
        with R.TFRecordWriter(str(data / ('%d.tfrecords' % f))) as wr:
            for _ in range(per_file):
                rec = {}
                for name, shape in shapes.items():
                    key = R.RECORD_NAME.get(name, name)
                    if len(shape) == 2:
                        rec[key] = rng.uniform(-1, 1, shape[1]).astype(np.float32)
                    else:
                        rec[key] = rng.integers(0, 256, (size, size, shape[3]), dtype=np.uint8).tobytes()
                wr.write(R.serialize_example(rec))
