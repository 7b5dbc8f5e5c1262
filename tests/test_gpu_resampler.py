"""The plain resampler (mv3d_resampler_*, tf.contrib.resampler.resampler) on the GPU against oracle/ops.py evaluated in float64
on the same fp32 inputs: the reference's own rotation case, random and edge warps over strided operands, a scatter pile-up,
the bitwise reproducibility of the data gradient, and graphs that route through every resample_layer path."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from oracle import ops
from oracle import models as omodels
from tests import resampler_cases as RC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu


def _oracle(data, warp, g=None):
    with np.errstate(invalid='ignore', over='ignore'):
        d64, w64 = data.astype(np.float64), warp.astype(np.float64)
        out = ops.resampler_fwd(d64, w64)
        if g is None:
            return out
        ddata, dwarp = ops.resampler_bwd(d64, w64, g.astype(np.float64))
    return out, ddata, dwarp


def _valid(warp, hs, ws):
    x, y = warp[..., 0], warp[..., 1]
    with np.errstate(invalid='ignore'):
        return (x > -1) & (y > -1) & (x < ws) & (y < hs)


class _Buf:
    """A [rows, ld] fp32 device buffer holding a [..., C] tensor at channel offset `off`; the rest is a sentinel."""
    SENTINEL = 7.25

    def __init__(self, arr, ld=None, off=0):
        self.shape, self.C = arr.shape, arr.shape[-1]
        self.ld, self.off = ld or self.C, off
        rows = int(np.prod(arr.shape[:-1]))
        host = np.full((rows, self.ld), self.SENTINEL, np.float32)
        host[:, off:off + self.C] = arr.reshape(rows, self.C)
        self.t = torch.from_numpy(host).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    def get(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        rest = np.delete(h, np.s_[self.off:self.off + self.C], axis=1)
        assert np.all(rest == self.SENTINEL), "a channel outside the slice was written"
        return h[:, self.off:self.off + self.C].reshape(self.shape)


def _ws(lib, n, p, hs, ws, c):
    nb = lib.resampler_bwd_workspace_bytes(n, p, hs, ws, c)
    t = torch.empty(nb // 4 + 4, dtype=torch.float32, device=DEV)
    return t, nb


def _run(lib, data, warp, dout, strided=False, want=('dwarp', 'ddata')):
    """fwd + bwd through the C ABI; returns (out, ddata, dwarp) as numpy (None for what was not requested)."""
    n, hs, ws, c = data.shape
    p = int(np.prod(warp.shape[1:-1]))
    pad = 4 if c % 4 == 0 else 1
    d = _Buf(data, c + 2 * pad, pad) if strided else _Buf(data)
    w = _Buf(warp, 5, 1) if strided else _Buf(warp)
    o = _Buf(np.zeros(warp.shape[:-1] + (c,), np.float32), c + pad, pad) if strided else _Buf(np.zeros(warp.shape[:-1] + (c,), np.float32))
    g = _Buf(dout, c + 3, 2) if strided else _Buf(dout)
    dw = _Buf(np.zeros(warp.shape, np.float32), 3, 1) if strided else _Buf(np.zeros(warp.shape, np.float32))
    dd = _Buf(np.zeros(data.shape, np.float32), c + 1, 0) if strided else _Buf(np.zeros(data.shape, np.float32))
    wst, nb = _ws(lib, n, p, hs, ws, c)
    st = stream()
    lib.resampler_fwd(n, p, hs, ws, c, d.ptr, d.ld, w.ptr, w.ld, o.ptr, o.ld, st)
    lib.resampler_bwd(n, p, hs, ws, c, d.ptr, d.ld, w.ptr, w.ld, g.ptr, g.ld,
                      dw.ptr if 'dwarp' in want else None, dw.ld, dd.ptr if 'ddata' in want else None, dd.ld,
                      wst.data_ptr(), nb, st)
    return o.get(), (dd.get() if 'ddata' in want else None), (dw.get() if 'dwarp' in want else None)


def _max_err(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


# ------------------------------------------------------------------------------------------------ 1. the reference's case
@pytest.fixture(scope="module")
def rotation():
    img = RC.rectangle_image()
    assert img.shape == (1500, 2100, 3) and img.dtype == np.uint8
    colours = np.unique(img.reshape(-1, 3), axis=0)
    assert colours.tolist() == [[2, 0, 0], [255, 255, 255]], colours
    rows, cols = np.nonzero((img == (2, 0, 0)).all(-1))
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (499, 1183, 431, 1668)
    data = img[None].astype(np.float32)
    warp = RC.rotation_warp()
    dout = np.random.default_rng(0).normal(0, 1, (1, 1500, 2100, 3)).astype(np.float32)
    return data, warp, dout


def test_reference_rotation_case(rotation):
    lib = _lib.lib()
    data, warp, dout = rotation
    out, ddata, dwarp = _run(lib, data, warp, dout)
    ref_out, ref_dd, ref_dw = _oracle(data, warp, dout)
    valid = _valid(warp, 1500, 2100)
    assert 0.03 < 1 - valid.mean() < 0.07, 1 - valid.mean()             # the points clipped to x = 2100
    assert np.all(out[~valid] == 0)
    assert np.abs(out - ref_out).max() <= 4e-6 * 255
    assert _max_err(dwarp, ref_dw) <= 2e-5
    assert _max_err(ddata, ref_dd) <= 1e-5
    # bitwise reproducible data gradient
    for _ in range(2):
        _, dd2, _ = _run(lib, data, warp, dout, want=('ddata',))
        assert np.array_equal(dd2.view(np.uint32), ddata.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. random and edge warps
def _edge_warp(rng, n, pshape, hs, ws):
    x = rng.uniform(-2.0, ws + 1.0, (n,) + pshape).astype(np.float32)
    y = rng.uniform(-2.0, hs + 1.0, (n,) + pshape).astype(np.float32)
    f32 = np.float32
    specials_x = [0.0, 1.0, ws - 1.0, -1.0, np.nextafter(f32(-1), f32(0)), float(ws), np.nextafter(f32(ws), f32(0)),
                  1e30, -1e30, np.inf, -np.inf, np.nan, 2.0, 0.5]
    specials_y = [0.0, 2.0, hs - 1.0, 0.5, -1.0, np.nextafter(f32(-1), f32(0)), float(hs), np.nextafter(f32(hs), f32(0)),
                  np.nan, 1e30, -np.inf, np.inf, -1e30, 3.0]
    fx, fy = x.reshape(-1), y.reshape(-1)
    ix, iy = rng.random(fx.shape) < 0.15, rng.random(fy.shape) < 0.15           # exact integer coordinates
    fx[ix], fy[iy] = np.round(fx[ix]), np.round(fy[iy])
    k = 0
    for sx in specials_x:
        for sy in specials_y:
            if k < fx.size:
                fx[k], fy[k] = sx, sy
                k += 3
    return np.stack([x, y], -1).astype(np.float32)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 7, 32])
@pytest.mark.parametrize("n,pshape", [(1, (37,)), (3, (9, 11))])
def test_random_and_edge_warps(n, pshape, c, strided):
    lib = _lib.lib()
    rng = np.random.default_rng(100 * c + n + strided)
    hs, ws = 6, 9
    data = rng.normal(0, 1, (n, hs, ws, c)).astype(np.float32)
    warp = _edge_warp(rng, n, pshape, hs, ws)
    dout = rng.normal(0, 1, warp.shape[:-1] + (c,)).astype(np.float32)
    out, ddata, dwarp = _run(lib, data, warp, dout, strided=strided)
    ref_out, ref_dd, ref_dw = _oracle(data, warp, dout)
    valid = _valid(warp, hs, ws)
    assert np.all(out[~valid] == 0) and np.all(dwarp[~valid] == 0)
    assert np.isfinite(out).all() and np.isfinite(dwarp).all() and np.isfinite(ddata).all()
    assert _max_err(out, ref_out) <= 2e-6
    assert _max_err(dwarp, ref_dw) <= 1e-5
    assert _max_err(ddata, ref_dd) <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. pile-up
def test_every_point_on_one_2x2_block():
    lib = _lib.lib()
    rng = np.random.default_rng(7)
    data = rng.normal(0, 1, (1, 16, 16, 3)).astype(np.float32)
    warp = np.stack([rng.uniform(3.0, 4.0, (1, 512, 512)), rng.uniform(5.0, 6.0, (1, 512, 512))], -1).astype(np.float32)
    dout = rng.normal(0, 1, (1, 512, 512, 3)).astype(np.float32)
    _, ddata, _ = _run(lib, data, warp, dout, want=('ddata',))
    _, ref_dd, _ = _oracle(data, warp, dout)
    assert _max_err(ddata, ref_dd) <= 1e-5
    assert np.count_nonzero(ddata) == np.count_nonzero(ref_dd) <= 12
    _, again, _ = _run(lib, data, warp, dout, want=('ddata',))
    assert np.array_equal(again.view(np.uint32), ddata.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4. partial calls, workspace
@pytest.mark.parametrize("c", [3, 32])
def test_partial_calls_equal_the_combined_call(c):
    lib = _lib.lib()
    rng = np.random.default_rng(11)
    data = rng.normal(0, 1, (2, 20, 24, c)).astype(np.float32)
    warp = _edge_warp(rng, 2, (15, 17), 20, 24)
    dout = rng.normal(0, 1, (2, 15, 17, c)).astype(np.float32)
    _, dd, dw = _run(lib, data, warp, dout)
    _, dd1, dw1 = _run(lib, data, warp, dout, want=('dwarp',))
    _, dd2, dw2 = _run(lib, data, warp, dout, want=('ddata',))
    assert dd1 is None and dw2 is None
    assert np.array_equal(dw1.view(np.uint32), dw.view(np.uint32))
    assert np.array_equal(dd2.view(np.uint32), dd.view(np.uint32))
    d, w, g = (torch.from_numpy(a).to(DEV) for a in (data, warp, dout))
    dd_t = torch.zeros_like(d)
    wst, nb = _ws(lib, 2, 15 * 17, 20, 24, c)
    rc = lib.raw_resampler_bwd(2, 15 * 17, 20, 24, c, d.data_ptr(), c, w.data_ptr(), 2, g.data_ptr(), c, None, 2,
                               dd_t.data_ptr(), c, wst.data_ptr(), nb - 8, stream())
    assert rc == -3 and 'workspace' in lib.last_error()


# ------------------------------------------------------------------------------------------------ 5. graphs
def _device_graph(case, seed):
    from dynamic_multiview_3d_amd import tf_utils as tf
    from dynamic_multiview_3d_amd.graph import Graph
    with Graph(device=DEV, seed=seed) as g:
        t = RC.build_graph(tf, g, case)
    g.compile()
    return g, t


def _sample_points_override(dev_warps, tape):
    """As tests/test_gpu_model.py does: where the device's sampling coordinates sit in another cell than the oracle's (they
    must agree to rounding), the oracle is evaluated at the device's coordinates."""
    override, moved = [], 0
    for dev, w in zip(dev_warps, tape.warp_inputs):
        dev = dev.reshape(w.shape)
        assert np.abs(dev - w).max() <= 1e-4 * max(np.abs(w).max(), 1.0)
        diff = (np.floor(dev) != np.floor(w)).any(axis=-1, keepdims=True)
        moved += int(diff.sum())
        override.append(np.where(diff, dev, w) if diff.any() else None)
    return override, moved


@pytest.mark.parametrize("case", ['conv_warp', 'conv_src', 'warp_pts_src'])
def test_graph_against_the_oracle(case):
    rng = np.random.default_rng(21)
    g, t = _device_graph(case, 5)
    var = RC.graph_variables(rng, case)
    if var is not None:
        g.set_variables(var)
    variables = g.get_variables()
    feeds = RC.graph_feeds(rng, case)
    for k, v in feeds.items():
        g.inputs[k].set(v)
    g.run_forward()
    g.run_backward()
    torch.cuda.synchronize()
    builder = RC.oracle_builder(case)
    out, grads, tape = omodels.run(builder, {k: v.copy() for k, v in variables.items()}, feeds)
    override, moved = _sample_points_override([t['warp'].numpy()], tape)
    if moved:
        out, grads, tape = omodels.run(builder, {k: v.copy() for k, v in variables.items()}, feeds, warp_override=override)
    if case == 'conv_warp':
        w = t['warp'].numpy()
        assert (w[..., 0] < 0).any() and (w[..., 0] > RC.WS - 1).any() and np.ptp(w[..., 1]) > RC.HS   # all over the image
    for k in ('gen', 'warp') + (('src',) if 'src' in t else ()):
        assert _max_err(t[k].numpy(), out[k]) <= 1e-4, k
    np.testing.assert_allclose(float(g.loss_buf[0]), float(out['loss']), rtol=1e-4)
    got = g.get_gradients()
    assert set(got) == set(grads) and grads
    for k in grads:
        assert _max_err(got[k], grads[k]) <= 1e-3, k
    # the optimiser step runs on top of these gradients
    loss = float(g.train_step())
    assert np.isfinite(loss)
