"""Seeded flow batches for the forward-backward consistency tests, shared by the CPU and the GPU files.

A case is a float32 array [N,H,H,2] whose second half plays the reversed pairs of the first (the partner of sample n is
(n + N/2) mod N).  Two families:

  smooth_case   smooth random flows of a few pixels; the partner is the approximate inverse plus noise, so the residuals are small
                and not zero
  large_case    smooth flows of a good part of the image side: many pixels leave the image

Every generator asserts what makes float32 and float64 agree on the cell and on the validity of every pixel: every sampling
coordinate x = f0 + i, y = f1 + j (formed in float32, as the kernel forms it) is at least 1e-3 away from every integer, and so from
the bounds 0 and H-1 as well.  The flows are built that way (the fractional part of every coordinate is moved into [0.01, 0.99]
before the flow is rounded to float32) and the assertion checks the result; no case is dropped.  The large family also asserts a
valid fraction strictly between 0.2 and 0.9.
"""
import numpy as np

MARGIN = 1e-3


def _smooth_field(rng, n, h, amplitude, knots=4):
    """[n,h,h,2] float64: bilinear interpolation of a knots x knots grid of N(0, amplitude^2) values."""
    grid = rng.normal(0.0, amplitude, (n, knots, knots, 2))
    t = np.linspace(0.0, knots - 1.0, h)
    i0 = np.minimum(np.floor(t).astype(np.int64), knots - 2)
    a = (t - i0)[None, :, None, None]
    rows = grid[:, i0] * (1.0 - a) + grid[:, i0 + 1] * a                       # [n,h,knots,2]
    b = (t - i0)[None, None, :, None]
    return rows[:, :, i0] * (1.0 - b) + rows[:, :, i0 + 1] * b


def _settle(flow64):
    """Moves the fractional part of every sampling coordinate into [0.01, 0.99], rounds the flow to float32 and asserts the margin
    on the float32 coordinates.  Returns the float32 flow."""
    n, h, w, _ = flow64.shape
    ii, jj = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    base = np.stack([ii, jj], axis=-1)[None]
    x = flow64 + base
    fl = np.floor(x)
    x = fl + np.clip(x - fl, 0.01, 0.99)
    flow = (x - base).astype(np.float32)
    check_margins(flow)
    return flow


def coordinates(flow):
    """(x, y) as the kernel forms them: float32 flow + float32 index."""
    f = np.asarray(flow, np.float32)
    n, h, w, _ = f.shape
    ii, jj = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    return f[..., 0] + ii[None], f[..., 1] + jj[None]


def check_margins(flow):
    h = flow.shape[1]
    for c in coordinates(flow):
        c = c.astype(np.float64)
        assert np.all(np.abs(c - np.rint(c)) >= MARGIN), "a sampling coordinate within 1e-3 of an integer"
        assert np.all(np.abs(c) >= MARGIN) and np.all(np.abs(c - (h - 1)) >= MARGIN), "a sampling coordinate within 1e-3 of a bound"


def valid_fraction(flow):
    h = flow.shape[1]
    x, y = coordinates(flow)
    return float(np.mean((x >= 0) & (x <= h - 1) & (y >= 0) & (y <= h - 1)))


def _with_partner(first, rng, noise):
    """first [n/2,h,h,2] float64 -> [n,h,h,2] float64: the partner's flow at (row r, column c) is about what takes the point back,
    (-F1, -F0) of the pixel (c, r) that lands near it (the transposed sampler convention), plus noise."""
    inverse = -np.transpose(first, (0, 2, 1, 3))[..., ::-1]
    return np.concatenate([first, inverse + rng.normal(0.0, noise, first.shape)], axis=0)


def smooth_case(n, h, seed):
    """Flows of a few pixels with small non-zero residuals: [n,h,h,2] float32."""
    assert n % 2 == 0 and n >= 2
    rng = np.random.default_rng([seed, n, h, 1])
    first = _smooth_field(rng, n // 2, h, amplitude=min(2.0, h / 8.0))
    return _settle(_with_partner(first, rng, noise=0.05))


def large_case(n, h, seed):
    """Flows of a good part of the image side: many pixels leave the image.  [n,h,h,2] float32."""
    assert n % 2 == 0 and n >= 2
    rng = np.random.default_rng([seed, n, h, 2])
    first = _smooth_field(rng, n // 2, h, amplitude=0.35 * h)
    flow = _settle(_with_partner(first, rng, noise=0.25))
    vf = valid_fraction(flow)
    assert 0.2 < vf < 0.9, "valid fraction %.3f of the large-flow case (n=%d, h=%d, seed=%d) outside (0.2, 0.9)" % (vf, n, h, seed)
    return flow


# the shapes of the GPU tests: below one tile; no multiple of 16; N/2 odd and an odd image size; across a 64-wide tile edge; the
# model's own size
SHAPES = [(2, 8), (2, 20), (6, 33), (4, 72), (2, 128)]
SEED = 7


def all_cases():
    """[(name, flow)] of both families at every shape of SHAPES."""
    out = []
    for n, h in SHAPES:
        out.append(('smooth-%dx%d' % (n, h), smooth_case(n, h, SEED)))
        out.append(('large-%dx%d' % (n, h), large_case(n, h, SEED)))
    return out
