"""The reader's process_image restated for the tests, independently of the package: uint8 [N, Hs, Ws, C] -> central square
crop -> TensorFlow 1.3 ResizeBicubic (align_corners = False) -> / 255, float32 [N, Ho, Wo, C], as DESIGN.md (input path) pins it.

`reference` is the numpy float32 statement of the whole rule.  `identity`, `half` and `double` are pure-integer statements of
the three ratios where the rule degenerates: out == S copies the source (weights 0, 1, 0, 0), out == S / 2 takes every second
pixel, out == 2 S has weights (-3, 19, 19, -3) / 32 on odd outputs and (0, 1, 0, 0) on even ones, so the fp32 result equals
integer arithmetic in any summation order.  CASES is the list the host and the GPU tests share."""
import numpy as np

f32 = np.float32

# (record H, record W, output side)
CASES = [(128, 128, 128), (128, 128, 64), (128, 128, 256), (128, 128, 96), (128, 128, 200), (100, 100, 128), (96, 128, 64)]
CHANNELS = (1, 3)
MAX_ABS_WEIGHT_SUM = 1.375           # largest sum of |weights| over the table (asserted in test_input_resize_host.py)


def table():
    """tab[2i] = near(i / 1024), tab[2i + 1] = far(i / 1024 + 1), A = -0.75, i = 0 .. 1024, every step rounded to float32"""
    A = f32(-0.75)
    tab = np.zeros(2 * 1025, f32)
    for i in range(1025):
        x = f32(i / 1024.0)
        tab[2 * i] = ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)
        x = x + f32(1)
        tab[2 * i + 1] = ((A * x - f32(5) * A) * x + f32(8) * A) * x - f32(4) * A
    return tab


_TAB = table()


def taps(S, out, o):
    """the four clamped source indices and weights of output coordinate o on an axis S -> out"""
    scale = f32(S) / f32(out)
    loc = scale * f32(o)
    fl = np.floor(loc)
    off = int(np.rint((loc - fl) * f32(1024)))                    # np.rint: round half to even
    fl = int(fl)
    idx = [min(max(fl + k, 0), S - 1) for k in (-1, 0, 1, 2)]
    w = [_TAB[2 * off + 1], _TAB[2 * off], _TAB[2 * (1024 - off)], _TAB[2 * (1024 - off) + 1]]
    return idx, w


def _resize_axis(v, out, axis):
    """v float32; `axis` of length S -> out.  ((v0*w0 + v1*w1) + v2*w2) + v3*w3 per output coordinate."""
    v = np.moveaxis(v, axis, 0)
    S = v.shape[0]
    res = np.empty((out,) + v.shape[1:], f32)
    for o in range(out):
        (i0, i1, i2, i3), (w0, w1, w2, w3) = taps(S, out, o)
        acc = v[i0] * w0 + v[i1] * w1
        acc = acc + v[i2] * w2
        res[o] = acc + v[i3] * w3
    return np.moveaxis(res, 0, axis)


def crop(src):
    hs, ws = src.shape[-3:-1]
    S = min(hs, ws)
    y0, x0 = (hs - S) // 2, (ws - S) // 2
    return src[..., y0:y0 + S, x0:x0 + S, :]


def reference(src, ho, wo):
    assert src.dtype == np.uint8 and src.ndim == 4
    v = crop(src).astype(f32)
    h = _resize_axis(v, wo, 2)                                    # horizontal first
    o = _resize_axis(h, ho, 1)
    assert o.dtype == f32
    return o / f32(255.0)


def identity(src):
    return crop(src).astype(f32) / f32(255.0)


def half(src):
    return crop(src)[:, ::2, ::2, :].astype(f32) / f32(255.0)


def _double_axis(v, axis):
    """int64 in, int64 out scaled by 32: even outputs 32 v[k], odd ones -3 v[k-1] + 19 v[k] + 19 v[k+1] - 3 v[k+2] (clamped)"""
    v = np.moveaxis(v, axis, 0)
    S = v.shape[0]
    k = np.arange(S)
    at = lambda d: v[np.clip(k + d, 0, S - 1)]
    res = np.empty((2 * S,) + v.shape[1:], np.int64)
    res[0::2] = 32 * v
    res[1::2] = -3 * at(-1) + 19 * at(0) + 19 * at(1) - 3 * at(2)
    return np.moveaxis(res, 0, axis)


def double(src):
    q = _double_axis(_double_axis(crop(src).astype(np.int64), 2), 1)            # integers, scaled by 1024, |q| < 2^24
    assert np.abs(q).max() < (1 << 24)
    return (q.astype(f32) / f32(1024.0)) / f32(255.0)


def integer_version(hs, ws, out):
    S = min(hs, ws)
    return identity if out == S else half if 2 * out == S else double if out == 2 * S else None


def random_u8(seed, n, hs, ws, c):
    return np.random.default_rng(seed).integers(0, 256, (n, hs, ws, c), dtype=np.uint8)
