"""Colour augmentation on the CPU (no GPU): the numpy twin of mv3d_color_augment against an independent float64 formulation
(colorsys) and against hand-computed pixels, its properties, draw_params, the conf keys, the CPU reader and the argument checks
of the C-ABI entry point.  The reference has no augmentation and TensorFlow cannot be run here: the twin is the authority."""
import colorsys
import ctypes as C

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import augment as A
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import color_augment_cases as CC

E_INVAL, E_WORKSPACE = -1, -3
ALL = A.ALL_STAGES


# ---------------------------------------------------------------- the twin
def _colorsys_version(views, params, stages):
    """brightness, clip, colorsys HSV round trip with s * fs clipped and h + dh wrapped, contrast about the float64 joint mean,
    clip: per pixel, in float64, from the float32 parameters"""
    pivot = np.mean(np.stack([v.astype(np.float64) for v in views], 1), axis=(1, 2, 3))
    clip = lambda c: min(max(c, 0.0), 1.0)
    out = []
    for x in views:
        o = np.empty(x.shape, np.float64)
        for i in range(x.shape[0]):
            db, fs, dh, fc = (float(v) for v in params[i])
            for y, xx in np.ndindex(x.shape[1:3]):
                r, g, b = (float(c) for c in x[i, y, xx])
                if stages & A.BRIGHTNESS:
                    r, g, b = r + db, g + db, b + db
                if stages & (A.SATURATION | A.HUE):
                    h, s, v = colorsys.rgb_to_hsv(clip(r), clip(g), clip(b))
                    if stages & A.SATURATION:
                        s = clip(s * fs)
                    if stages & A.HUE:
                        h = (h + dh) % 1.0
                    r, g, b = colorsys.hsv_to_rgb(h, s, v)
                if stages & A.CONTRAST:
                    r, g, b = ((c - p) * fc + p for c, p in zip((r, g, b), pivot[i]))
                o[i, y, xx] = clip(r), clip(g), clip(b)
        out.append(o)
    return out


def test_twin_against_colorsys_float64():
    """48 images of 40 x 40 (6 samples x 2 views, u8 / 255 and overshooting, all four stages and each HSV stage alone), parameters
    drawn from b = 0.3, saturation (0.3, 2), h = 0.5, contrast (0.4, 1.8); rows of grey pixels, rows with two equal channels.  The bar
    is 1e-5: a wrong hue sector, a swapped channel or a missing wrap shows at >= 1e-2, and the fp32 twin's own rounding (some ten
    operations of 2^-24 relative error on values <= 1, the hue's multiplied by 6 and the contrast's by <= 1.8) stays near 1e-6.
    Measured: 1.1e-06."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for kind, stages in (('u8', ALL), ('over', ALL), ('over', A.SATURATION), ('u8', A.HUE)):
        views = [CC.images(kind, rng.integers(1 << 30), (6, 40, 40, 3)) for _ in range(2)]
        for v in views:
            v[:, 3] = v[:, 3, :, :1]                    # a row of grey pixels
            v[:, 5, :, 1] = v[:, 5, :, 0]               # r == g
            v[:, 7, :, 2] = v[:, 7, :, 1]               # g == b
            v[:, 9, :, 2] = v[:, 9, :, 0]               # r == b
        params = A.draw_params(rng, 6, CC.CONF)
        got = A.color_augment_host(views, params, stages)
        want = _colorsys_version(views, params, stages)
        worst = max(worst, max(np.abs(g.astype(np.float64) - w).max() for g, w in zip(got, want)))
    print("twin against colorsys (float64): max abs difference %.3g" % worst)
    assert worst <= 1e-5


def test_crafted_pixels_have_the_hand_computed_values():
    for cases, stages in ((CC.CRAFTED_SH, CC.SH), (CC.CRAFTED_B, A.BRIGHTNESS)):
        for name, px, params, want in cases:
            x = np.asarray(px, np.float32).reshape(1, 1, 1, 3)
            got = A.color_augment_host([x], np.asarray(params, np.float32)[None], stages)[0]
            np.testing.assert_array_equal(got.reshape(3), np.asarray(want, np.float32), err_msg=name)
        x, params, pos = CC.crafted_batch(cases)
        CC.check_crafted(cases, A.color_augment_host([x], params, stages)[0], pos)
    # the neutral HSV round trip alone leaves none of the first ten crafted pixels changed, and a saturation-only or hue-only
    # mask gives the same values as the joint mask with the other parameter neutral
    for name, px, params, want in CC.CRAFTED_SH:
        x = np.asarray(px, np.float32).reshape(1, 1, 1, 3)
        p = np.asarray(params, np.float32)[None]
        if p[0, 2] == 0:
            np.testing.assert_array_equal(A.color_augment_host([x], p, A.SATURATION)[0].reshape(3), np.asarray(want, np.float32), err_msg=name)
        if p[0, 1] == 1:
            np.testing.assert_array_equal(A.color_augment_host([x], p, A.HUE)[0].reshape(3), np.asarray(want, np.float32), err_msg=name)


def test_outputs_in_range_and_passthrough():
    rng = np.random.default_rng(1)
    a, b = CC.images('over', 1, (3, 9, 11, 3)), CC.images('over', 2, (3, 9, 11, 3))
    mask = rng.uniform(-1, 2, (3, 9, 11, 1)).astype(np.float32)
    disp = rng.uniform(-1, 2, (3, 2)).astype(np.float32)
    keep = [a.copy(), mask.copy(), b.copy(), disp.copy()]
    for stages in (A.BRIGHTNESS, A.SATURATION, A.HUE, A.CONTRAST, CC.SH, ALL):
        out = A.color_augment_host([a, mask, b, disp], A.draw_params(rng, 3, CC.CONF), stages)
        assert out[1] is mask and out[3] is disp
        for o, src in ((out[0], a), (out[2], b)):
            assert o is not src and o.dtype == np.float32 and o.shape == src.shape
            assert o.min() >= 0.0 and o.max() <= 1.0 and np.isfinite(o).all()
    for got, want in zip([a, mask, b, disp], keep):                  # the inputs are left alone
        assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        A.color_augment_host([mask, disp], np.zeros((3, 4), np.float32), ALL)
    for bad in (0, 16, 31):
        with pytest.raises(ValueError):
            A.color_augment_host([a], np.zeros((3, 4), np.float32), bad)


def test_equal_views_come_out_equal():
    a = CC.images('over', 3, (2, 20, 20, 3))
    params = A.draw_params(np.random.default_rng(3), 2, CC.CONF)
    o0, o1, o2 = A.color_augment_host([a, a.copy(), a.copy()], params, ALL)
    assert o0.tobytes() == o1.tobytes() == o2.tobytes()


def test_pivot_is_the_joint_mean():
    """view A all 0.25, view B all 0.75: the joint pivot is 0.5 (exact sums), so with factor 2 A becomes 0 and B becomes 1; a
    per-view pivot would leave both as they are"""
    a, b = np.full((2, 8, 8, 3), 0.25, np.float32), np.full((2, 8, 8, 3), 0.75, np.float32)
    params = np.tile(np.array([0, 1, 0, 2], np.float32), (2, 1))
    np.testing.assert_array_equal(A.joint_pivots([a, b]), np.full((2, 3), 0.5, np.float32))
    oa, ob = A.color_augment_host([a, b], params, A.CONTRAST)
    np.testing.assert_array_equal(oa, np.zeros_like(a))
    np.testing.assert_array_equal(ob, np.ones_like(b))
    per_view = [A.color_augment_host([v], params, A.CONTRAST)[0] for v in (a, b)]
    np.testing.assert_array_equal(per_view[0], a)
    np.testing.assert_array_equal(per_view[1], b)
    # different means per sample and channel, hand-computed: pivot = (mean A + mean B) / 2
    rng = np.random.default_rng(5)
    a, b = CC.images('u8', 5, (3, 12, 12, 3)), CC.images('u8', 6, (3, 12, 12, 3))
    fc = rng.uniform(0.4, 1.8, 3).astype(np.float32)
    params = np.stack([np.zeros(3), np.ones(3), np.zeros(3), fc], 1).astype(np.float32)
    pivot = np.float32((a.astype(np.float64).sum((1, 2)) + b.astype(np.float64).sum((1, 2))) / (2 * 144))
    want = np.clip((a - pivot[:, None, None]) * fc[:, None, None, None] + pivot[:, None, None], 0, 1)
    np.testing.assert_array_equal(A.color_augment_host([a, b], params, A.CONTRAST)[0], want)


@pytest.mark.parametrize("shape,views", [((2, 128, 128, 3), 2), ((3, 67, 61, 3), 3), ((1, 1, 1, 3), 1), ((2, 5, 7, 3), 1)])
def test_pivot_of_u8_images_is_the_plain_float64_mean(shape, views):
    """for uint8 / 255 inputs the double sums are exact whatever the order: every term has 24 significant bits with its lowest at
    2^-31 or above, and a sum of 2^14 of them needs 45 bits -- at most 2^17 terms here, 48 bits"""
    xs = [CC.images('u8', 10 + v, shape) for v in range(views)]
    count = views * shape[1] * shape[2]
    want = np.float32(np.sum(np.stack(xs, 1), axis=(1, 2, 3), dtype=np.float64) / count)
    np.testing.assert_array_equal(A.joint_pivots(xs), want)


# ---------------------------------------------------------------- draw_params and the conf keys
def test_draw_params():
    seed = [3, 0]
    full = A.draw_params(np.random.default_rng(seed), 64, CC.CONF)
    assert full.dtype == np.float32 and full.shape == (64, 4)
    assert full.tobytes() == A.draw_params(np.random.default_rng(seed), 64, CC.CONF).tobytes()
    lo, hi = np.array([-0.3, 0.3, -0.5, 0.4]), np.array([0.3, 2, 0.5, 1.8])
    assert np.all(full >= lo.astype(np.float32)) and np.all(full <= hi.astype(np.float32))
    assert np.all(full.max(0) - full.min(0) > 0.8 * (hi - lo))                # the whole range is used
    for col, key in enumerate(A.KEYS):                                        # one stage off: its column neutral, the others as before
        conf = {k: v for k, v in CC.CONF.items() if k != key}
        got = A.draw_params(np.random.default_rng(seed), 64, conf)
        assert np.all(got[:, col] == A.NEUTRAL[col])
        others = [c for c in range(4) if c != col]
        assert got[:, others].tobytes() == full[:, others].tobytes()
    assert np.all(A.draw_params(np.random.default_rng(seed), 5, {}) == A.NEUTRAL)
    # ranks differ, and so do seeds
    shapes = CC.appflow_shapes(4, 16)
    r0, r1 = (A.ColorAugment(CC.CONF, shapes, rank=r).draw() for r in (0, 1))
    s1 = A.ColorAugment(dict(CC.CONF, augment_seed=1), shapes).draw()
    assert not np.any(r0 == r1) and not np.any(r0 == s1)
    assert r0.tobytes() == A.draw_params(np.random.default_rng([0, 0]), 4, CC.CONF).tobytes()
    assert s1.tobytes() == A.ColorAugment(CC.CONF, shapes, seed=1).draw().tobytes()


def test_conf_keys():
    spec = A.augment_from_conf({})
    assert spec.stages == 0 and not spec.enabled and spec.seed == 0
    for key, bit in zip(A.KEYS, (A.BRIGHTNESS, A.SATURATION, A.HUE, A.CONTRAST)):
        for off in (None, 0, 0.0):
            assert not A.augment_from_conf({key: off}).enabled
        assert A.augment_from_conf({key: CC.CONF[key]}).stages == bit
    assert A.augment_from_conf(CC.CONF).stages == ALL
    assert A.augment_from_conf({'augment_brightness': 1, 'augment_hue': 0.5, 'augment_saturation': [0, 1], 'augment_contrast': (0, 0.1)}).stages == ALL
    nan, inf = float('nan'), float('inf')
    bad = {'augment_brightness': (True, False, -0.1, 1.5, nan, inf, '0.1', (0.1, 0.2)),
           'augment_hue': (True, -0.1, 0.51, nan, inf, [0.1]),
           'augment_saturation': (True, 0.5, (1,), (0.5, 1, 2), (-0.1, 1), (1, 1), (2, 1), (nan, 1), (0, inf), (True, 2), ('a', 'b')),
           'augment_contrast': (False, 1.5, (1,), (0.5, 1, 2), (-0.1, 1), (1, 1), (2, 1), (0, nan), (0, inf), (0, True))}
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError):
                A.augment_from_conf({key: v})
    for seed in (True, -1, 1.5, '3'):
        with pytest.raises(ValueError):
            A.augment_from_conf(dict(CC.CONF, augment_seed=seed))
    assert A.augment_from_conf(dict(CC.CONF, augment_seed=np.int64(5))).seed == 5


def test_color_augment_object_and_model_classes():
    shapes = CC.appflow_shapes(4, 16)
    off = A.ColorAugment({'batch_size': 4}, shapes)
    assert not off.enabled and off.names == []
    batch = {'image0': torch.zeros(4, 16, 16, 3)}
    assert off.apply(batch) is batch and float(batch['image0'].sum()) == 0
    on = A.ColorAugment(CC.CONF, shapes)
    assert on.enabled and on.names == ['image0', 'image1'] and on.stages == ALL
    assert A.ColorAugment(CC.CONF, CC.multiobject_shapes(2, 16)).names == ['image0', 'image1', 'image1_only0', 'image1_only1']
    with pytest.raises(ValueError, match='augment'):                 # no colour input
        A.ColorAugment(CC.CONF, {'depth': (4, 16, 16, 1), 'labels': (4, 5)})
    with pytest.raises(ValueError, match='augment'):                 # an image input that is neither colour nor single-channel
        A.ColorAugment(CC.CONF, {'image0': (4, 16, 16, 3), 'flow': (4, 16, 16, 2)})
    with pytest.raises(ValueError, match='augment'):
        A.ColorAugment(CC.CONF, {'image0': (4, 16, 16, 3), 'rgbd': (4, 16, 16, 4)})
    with pytest.raises(ValueError):
        A.ColorAugment({'augment_hue': 0.7}, shapes)
    # every model class reads the keys, before it builds anything
    from dynamic_multiview_3d_amd import mv3d
    from tests.test_optimizers_host import _appflow, _lowdim
    with pytest.raises(ValueError):
        mv3d.mv3d_nobg_nodm({'batch_size': 2, 'augment_brightness': 2.0}, device='cpu')
    with pytest.raises(ValueError):
        _lowdim({'augment_contrast': (2, 1)})
    with pytest.raises(ValueError):
        _appflow({'batch_size': 2, 'augment_saturation': True})
    m = _appflow(dict(CC.CONF, batch_size=2, learning_rate=1e-4))
    aug = A.ColorAugment(m.conf, {k: tuple(t.shape) for k, t in m.graph.inputs.items()})
    assert aug.names == ['image0', 'image1']


def test_augmented_data_hands_out_copies():
    class Pool:
        def __init__(self):
            self.b = {'image0': torch.from_numpy(CC.images('u8', 1, (4, 16, 16, 3))), 'image1': torch.from_numpy(CC.images('u8', 2, (4, 16, 16, 3))),
                      'depth_image0': torch.rand(4, 16, 16, 1), 'disp': torch.rand(4, 2)}

        def next(self):
            return self.b
    pool = Pool()
    keep = {k: v.clone() for k, v in pool.b.items()}
    data = A.AugmentedData(pool, A.ColorAugment(CC.CONF, CC.appflow_shapes(4, 16)))
    rng = np.random.default_rng([0, 0])
    for _ in range(2):
        got = data.next()
        want = A.color_augment_host([keep['image0'].numpy(), keep['image1'].numpy()], A.draw_params(rng, 4, CC.CONF), ALL)
        np.testing.assert_array_equal(got['image0'].numpy(), want[0])
        np.testing.assert_array_equal(got['image1'].numpy(), want[1])
        assert got['depth_image0'] is pool.b['depth_image0'] and got['disp'] is pool.b['disp']
        for k in keep:
            assert torch.equal(pool.b[k], keep[k])


# ---------------------------------------------------------------- the CPU reader
def _read(conf, shapes, batches, **kw):
    inp = R.TFRecordInput(conf, shapes, device='cpu', **kw)
    try:
        return [{k: v.numpy().copy() for k, v in inp.next().items()} for _ in range(batches)]
    finally:
        inp.close()


def test_cpu_reader(tmp_path):
    shapes = CC.appflow_shapes(4, 16)
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0}
    conf = dict(base, **CC.CONF)
    plain = _read(base, shapes, 3, seed=4)
    got = _read(conf, shapes, 3, seed=4)
    rng = np.random.default_rng([0, 0])
    for p, g in zip(plain, got):
        want = A.color_augment_host([p['image0'], p['image1']], A.draw_params(rng, 4, CC.CONF), ALL)
        np.testing.assert_array_equal(g['image0'], want[0])
        np.testing.assert_array_equal(g['image1'], want[1])
        assert not np.array_equal(g['image0'], p['image0'])
        for k in ('depth_image0', 'depth_image1', 'disp'):          # same records in the same order, untouched
            assert g[k].tobytes() == p[k].tobytes()
    # rank and augment_seed select the generator
    got = _read(dict(conf, augment_seed=9), shapes, 1, seed=4, rank=1, world=1)
    want = A.color_augment_host([plain[0]['image0'], plain[0]['image1']], A.draw_params(np.random.default_rng([9, 1]), 4, CC.CONF), ALL)
    np.testing.assert_array_equal(got[0]['image1'], want[1])
    # validation inputs and test_mode are never augmented; with the keys absent (or off) the reader is the plain one
    for c, kw in ((dict(conf, train_val_split=0.0), {'training': False}), (dict(conf, test_mode=''), {}), (dict(base, augment_hue=0, augment_contrast=None), {})):
        ref = dict(base, **{k: c[k] for k in ('train_val_split', 'test_mode') if k in c})
        for a, b in zip(_read(ref, shapes, 2, seed=4, **kw), _read(c, shapes, 2, seed=4, **kw)):
            assert set(a) == set(b)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes()
    inp = R.TFRecordInput(base, shapes, device='cpu')
    assert inp.augment is None
    inp.close()
    with pytest.raises(ValueError):
        R.TFRecordInput(dict(base, augment_hue=0.6), shapes, device='cpu')
    with pytest.raises(ValueError, match='augment'):
        R.TFRecordInput(conf, {'depth_image0': (4, 16, 16, 1), 'disp': (4, 2)}, device='cpu')


# ---------------------------------------------------------------- the entry point's argument checks (nothing is launched)
def test_abi_argument_checks():
    lib = _lib.lib()
    assert (_lib.AUG_BRIGHTNESS, _lib.AUG_SATURATION, _lib.AUG_HUE, _lib.AUG_CONTRAST) == (1, 2, 4, 8)
    n, h, w = 2, 67, 61
    nbytes = 4 * n * h * w * 3
    need = int(lib.color_augment_workspace_bytes(n, 3, h, w))
    assert need == n * 3 * 1 * 24 and int(lib.color_augment_workspace_bytes(2, 4, 128, 128)) == 2 * 4 * 4 * 24
    assert int(lib.color_augment_workspace_bytes(1, 1, 1, 1)) == 24 and int(lib.color_augment_workspace_bytes(1, 1, 64, 65)) == 48
    V0, P, WS = 0x10000000, 0x30000000, 0x40000000              # never dereferenced: every call below fails its checks

    def views(k, stride=0x1000000):
        return [V0 + i * stride for i in range(k)]

    def call(ptrs=None, nv=None, n=n, h=h, w=w, params=P, stages=15, ws=WS, nb=need, null_array=False):
        ptrs = views(3) if ptrs is None else ptrs
        arr = None if null_array else (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        return lib.raw_color_augment(arr, len(ptrs) if nv is None else nv, n, h, w, params, stages, ws, nb, None)
    assert call(null_array=True) == E_INVAL and call(params=None) == E_INVAL and call(ws=None) == E_INVAL
    assert 'null' in lib.last_error() and 'mv3d_color_augment' in lib.last_error()
    assert call(ptrs=[V0, None, V0 + 0x1000000]) == E_INVAL
    assert call(ptrs=[], nv=0) == E_INVAL and call(ptrs=views(9)) == E_INVAL and call(nv=-1) == E_INVAL
    assert 'views' in lib.last_error()
    for kw in ({'n': 0}, {'h': 0}, {'w': -1}, {'n': 1 << 20, 'h': 1 << 10, 'w': 1 << 10}, {'n': 1, 'h': 1 << 15, 'w': 1 << 15}):
        assert call(**kw) == E_INVAL, kw
    assert call(stages=0) == E_INVAL and call(stages=16) == E_INVAL and call(stages=15 | 32) == E_INVAL
    assert 'stage' in lib.last_error()
    for off in (4, 8, 12):
        assert call(ptrs=[V0, V0 + 0x1000000 + off]) == E_INVAL
    assert '16-byte' in lib.last_error()
    assert call(params=P + 4) == E_INVAL
    assert call(ptrs=[V0, V0 + 0x1000000, V0]) == E_INVAL and call(ptrs=[V0, V0]) == E_INVAL            # duplicates
    assert 'overlap' in lib.last_error()
    assert call(ptrs=[V0, V0 + 0x10000]) == E_INVAL and 0x10000 < nbytes and call(ptrs=[V0 + 16, V0]) == E_INVAL        # overlapping ranges
    assert call(nb=need - 1) == E_WORKSPACE and call(nb=0) == E_WORKSPACE
    assert call(ws=WS + 8) == E_WORKSPACE
