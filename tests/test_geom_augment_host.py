"""Geometric augmentation on the CPU (no GPU): the numpy twin of mv3d_geom_augment and its properties, draw_geom_params, the conf
keys, the model classes, the CPU reader, the synthetic feed's wrapper and the argument checks of the C-ABI entry point.  The
reference has no augmentation and TensorFlow cannot be run here: the twin is the authority, and every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import augment as A
from dynamic_multiview_3d_amd import pair_swap as PS
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import color_augment_cases as CC
from tests import geom_augment_cases as GC

E_INVAL = -1


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize("n,h,w", GC.SHAPES)
def test_identity_flip_and_flip_twice(n, h, w):
    x = GC.views(1, n, h, w, [3, 1])
    d = GC.disp(2, n)
    keep = [v.copy() for v in x] + [d.copy()]
    outs, dd = A.geom_augment_host(x, d, GC.identity(n, h, w))
    assert all(_same(o, v) and o is not v for o, v in zip(outs, x)) and _same(dd, d) and dd is not d
    outs, dd = A.geom_augment_host(x, d, GC.flip_only(n, h, w))
    for o, v in zip(outs, x):                                       # both channel counts
        assert _same(o, np.ascontiguousarray(v[:, :, ::-1]))
    assert _same(dd[:, 0], d[:, 0]) and _same(dd[:, 1], -d[:, 1])
    again, ddd = A.geom_augment_host(outs, dd, GC.flip_only(n, h, w))
    assert all(_same(o, v) for o, v in zip(again, x)) and _same(ddd, d)
    # one sample flipped, the others not
    p = GC.identity(n, h, w)
    p[n - 1] = GC.flip_only(1, h, w)[0]
    outs, dd = A.geom_augment_host(x, d, p)
    assert _same(outs[0][n - 1], x[0][n - 1, :, ::-1]) and _same(outs[0][:n - 1], x[0][:n - 1])
    assert _same(dd[:n - 1], d[:n - 1]) and dd[n - 1, 1] == -d[n - 1, 1]
    assert A.geom_augment_host(x, None, p)[1] is None
    for got, want in zip(x + [d], keep):                            # the inputs are left alone
        assert _same(got, want)


@pytest.mark.parametrize("n,h,w", GC.SHAPES)
def test_constant_image_and_mask_range(n, h, w):
    """a constant image stays constant to the bit under any parameters (a + (b - a) * f with b == a), a {0, 1} mask stays in
    {0, 1} (nearest sampling), and every output value of a single-channel view is one of its sample's input values"""
    const = [np.full((n, h, w, 3), np.float32(0.3)), np.full((n, h, w, 1), np.float32(0.7))]
    mask = GC.masks(5, (n, h, w, 1))
    depth = GC.images(6, (n, h, w, 1))
    for name, p in GC.param_rows(n, h, w):
        outs, _ = A.geom_augment_host(const + [mask, depth], None, p)
        assert _same(outs[0], const[0]) and _same(outs[1], const[1]), name
        assert np.all((outs[2] == 0) | (outs[2] == 1)), name
        for i in range(n):
            assert np.isin(outs[3][i], depth[i]).all(), name


@pytest.mark.parametrize("n,h,w", GC.SHAPES)
def test_corner_shifts_stay_inside_the_image(n, h, w):
    """t = 1 at s = zmax = 4, all four corners, both mirrors: the UNCLAMPED coordinates lie in [0, size - 1] up to the four roundings
    of the chain (inv, the product, cxo, the sum: each at most 2^-24 of a value no larger than size - 1), so the clamp only absorbs
    rounding; the window touches the image's edge on the side it was pushed to; the twin reads in bounds (numpy would raise)."""
    x = GC.views(3, n, h, w, [3, 1])
    for k, (tx, ty) in enumerate(GC.CORNERS):
        for m in (0, 1):
            p = GC.corner(n, h, w, k, m)
            for size, axis, t in ((w, 1, tx), (h, 0, ty)):
                raw = A.geom_source_coords(p, size, axis, clamp=False).astype(np.float64)
                slack = 4 * 2.0 ** -24 * (size - 1)
                assert raw.min() >= -slack and raw.max() <= size - 1 + slack, (k, m, axis)
                edge = raw.min() if t < 0 else size - 1 - raw.max()
                assert abs(edge) <= slack, (k, m, axis)
                got = A.geom_source_coords(p, size, axis)
                assert got.min() >= 0 and got.max() <= size - 1 and np.abs(got - raw).max() <= slack
            outs, _ = A.geom_augment_host(x, None, p)
            assert np.isfinite(outs[0]).all()
    # parameters far outside the contract's ranges still read in bounds: the clamp holds whatever they hold
    wild = np.array([[1, 50, -1e6, 1e6]] * n, np.float32)
    outs, _ = A.geom_augment_host(x, None, wild)
    assert _same(outs[1], np.broadcast_to(x[1][:, h - 1:h, 0:1], x[1].shape).copy())
    with pytest.raises(ValueError):
        A.geom_augment_host(x, None, np.full((n, 4), np.nan, np.float32))


def test_zoom_by_two_has_the_hand_computed_values():
    """s = 2 on an 8-wide ramp, no shift: xs = (x - 3.5) / 2 + 3.5 = 1.75, 2.25, .. 5.25: bilinear gives the ramp's value at xs
    (exact in fp32 here), nearest rounds xs + 0.5 down: 2 2 3 3 4 4 5 5"""
    ramp = np.arange(8, dtype=np.float32)
    rgb = np.broadcast_to(ramp[None, None, :, None], (1, 8, 8, 3)).copy()
    one = rgb[..., :1].copy()
    outs, _ = A.geom_augment_host([rgb, one], None, GC.row(0, 2, 0, 0, 8, 8)[None])
    np.testing.assert_array_equal(outs[0][0, 3, :, 1], np.float32([1.75, 2.25, 2.75, 3.25, 3.75, 4.25, 4.75, 5.25]))
    np.testing.assert_array_equal(outs[1][0, 3, :, 0], np.float32([2, 2, 3, 3, 4, 4, 5, 5]))
    outs, _ = A.geom_augment_host([rgb.transpose(0, 2, 1, 3).copy()], None, GC.row(1, 2, 0, 0, 8, 8)[None])     # rows, and mirrored
    np.testing.assert_array_equal(outs[0][0, :, 2, 0], np.float32([1.75, 2.25, 2.75, 3.25, 3.75, 4.25, 4.75, 5.25]))


def test_twin_refuses_what_it_cannot_take():
    x = GC.views(1, 2, 5, 7, [3, 1])
    p = GC.identity(2, 5, 7)
    for bad in ([], x * 9, [x[0][..., :2]], [x[0].astype(np.float64)], [x[0], x[1][:, :4]], [x[0][0]]):
        with pytest.raises(ValueError):
            A.geom_augment_host(bad, None, p)
    with pytest.raises(ValueError):
        A.geom_augment_host(x, None, p[:1])
    with pytest.raises(ValueError):
        A.geom_augment_host(x, np.zeros((2, 3), np.float32), p)


# ---------------------------------------------------------------- draw_geom_params and the conf keys
def test_draw_geom_params():
    n, h, w = 64, 33, 130
    cx, cy = np.float32((w - 1) / 2), np.float32((h - 1) / 2)
    seed = [3, 0, 1]
    full = A.draw_geom_params(np.random.default_rng(seed), n, GC.WIDE, h, w)
    assert full.dtype == np.float32 and full.shape == (n, 4)
    assert _same(full, A.draw_geom_params(np.random.default_rng(seed), n, GC.WIDE, h, w))
    assert set(np.unique(full[:, 0])) == {0.0, 1.0}
    assert np.all(full[:, 1] >= np.float32(0.25)) and np.all(full[:, 1] <= 1) and full[:, 1].max() - full[:, 1].min() > 0.5
    # the float64 formula, rounded once
    u = np.random.default_rng(seed).random((n, 4))
    s = 1 + 3 * u[:, 1]
    want = np.stack([u[:, 0] < 0.5, 1 / s, (w - 1) / 2 + (2 * u[:, 2] - 1) * ((w - 1) / 2) * (1 - 1 / s),
                     (h - 1) / 2 + (2 * u[:, 3] - 1) * ((h - 1) / 2) * (1 - 1 / s)], 1).astype(np.float32)
    assert _same(full, want)
    # neutral columns for stages that are off; a stage switched on leaves the other columns as they were
    assert np.all(A.draw_geom_params(np.random.default_rng(seed), 5, {}, h, w) == np.float32([0, 1, cx, cy]))
    flip = A.draw_geom_params(np.random.default_rng(seed), n, {'augment_flip': 0.5}, h, w)
    assert _same(flip[:, 0], full[:, 0]) and np.all(flip[:, 1:] == np.float32([1, cx, cy]))
    zoom = A.draw_geom_params(np.random.default_rng(seed), n, {'augment_zoom': 4}, h, w)
    assert np.all(zoom[:, 0] == 0) and _same(zoom[:, 1], full[:, 1]) and np.all(zoom[:, 2:] == np.float32([cx, cy]))
    noflip = A.draw_geom_params(np.random.default_rng(seed), n, {'augment_zoom': 4, 'augment_shift': 1}, h, w)
    assert np.all(noflip[:, 0] == 0) and _same(noflip[:, 1:], full[:, 1:])
    assert np.all(A.draw_geom_params(np.random.default_rng(seed), n, {'augment_flip': 1}, h, w)[:, 0] == 1)
    # the window stays inside the image: |ox| <= cx (1 - inv) up to the rounding of cxo
    assert np.all(np.abs(full[:, 2].astype(np.float64) - (w - 1) / 2) <= (w - 1) / 2 * (1 - full[:, 1].astype(np.float64)) + 2.0 ** -24 * w)
    # same seed, same rows; ranks and seeds differ; the generator is [seed, rank, 1]
    shapes = CC.appflow_shapes(16, 16)
    r0, r1 = (A.GeomAugment(GC.WIDE, shapes, rank=r).draw() for r in (0, 1))
    s1 = A.GeomAugment(dict(GC.WIDE, augment_seed=1), shapes).draw()
    assert not np.any(r0[:, 1:] == r1[:, 1:]) and not np.any(r0[:, 1:] == s1[:, 1:])
    assert _same(r0, A.draw_geom_params(np.random.default_rng([0, 0, 1]), 16, GC.WIDE, 16, 16))
    assert _same(r0, A.GeomAugment(GC.WIDE, shapes, rank=0).draw())
    assert _same(s1, A.GeomAugment(GC.WIDE, shapes, seed=1).draw())


def test_colour_parameter_stream_does_not_depend_on_the_new_keys():
    shapes = CC.appflow_shapes(4, 16)
    plain = A.ColorAugment(CC.CONF, shapes, rank=2)
    both = A.ColorAugment(dict(CC.CONF, **GC.CONF), shapes, rank=2)
    geom = A.GeomAugment(dict(CC.CONF, **GC.CONF), shapes, rank=2)
    rng = np.random.default_rng([0, 2])
    for _ in range(3):
        geom.draw()
        want = A.draw_params(rng, 4, CC.CONF)
        assert _same(plain.draw(), want) and _same(both.draw(), want)
    assert A.augment_from_conf(GC.CONF).stages == 0 and not A.geom_from_conf(CC.CONF).enabled


def test_conf_keys_and_every_refusal():
    spec = A.geom_from_conf({})
    assert not spec.enabled and (spec.flip, spec.zoom, spec.shift, spec.seed) == (None, None, None, 0)
    for key in A.GEOM_KEYS:
        for off in (None, 0, 0.0):
            assert not A.geom_from_conf({key: off}).enabled
    spec = A.geom_from_conf(dict(GC.CONF, augment_seed=3))
    assert spec.enabled and (spec.flip, spec.zoom, spec.shift, spec.seed) == (0.5, 2.0, 1.0, 3)
    assert A.geom_from_conf({'augment_flip': 1}).enabled and A.geom_from_conf({'augment_zoom': 4}).zoom == 4.0
    assert A.geom_from_conf({'augment_zoom': np.float32(1.5), 'augment_shift': np.float64(0.25)}).shift == 0.25
    nan, inf = float('nan'), float('inf')
    refused = [
        {'augment_flip': True},                                     # a bool where a number belongs
        {'augment_zoom': True},
        {'augment_zoom': 2.0, 'augment_shift': True},
        {'augment_flip': False},
        {'augment_flip': 1.5},                                      # p > 1
        {'augment_flip': -0.1},
        {'augment_zoom': 1.0},                                      # zmax <= 1
        {'augment_zoom': 0.5},
        {'augment_zoom': 4.5},                                      # zmax > 4
        {'augment_shift': 0.5},                                     # shift without zoom
        {'augment_shift': 0.5, 'augment_zoom': 0},
        {'augment_shift': 0.5, 'augment_flip': 0.5},
        {'augment_zoom': 2.0, 'augment_shift': 1.5},
        {'augment_flip': nan},                                      # NaN and inf
        {'augment_zoom': nan},
        {'augment_zoom': 2.0, 'augment_shift': nan},
        {'augment_flip': inf},
        {'augment_zoom': inf},
        {'augment_flip': '0.5'},
        {'augment_zoom': (1, 2)},
        {'augment_flip': 0.5, 'augment_seed': -1},
    ]
    for conf in refused:
        with pytest.raises(ValueError):
            A.geom_from_conf(conf)


def test_geom_augment_object():
    shapes = CC.appflow_shapes(4, 16)
    off = A.GeomAugment({'batch_size': 4}, shapes)
    assert not off.enabled and off.names == [] and off.disp_name is None
    batch = {'image0': torch.zeros(4, 16, 16, 3)}
    assert off.apply(batch) is batch
    on = A.GeomAugment(GC.CONF, shapes)
    assert on.names == ['image0', 'image1', 'depth_image0', 'depth_image1'] and on.channels == [3, 3, 1, 1] and on.disp_name == 'disp'
    mo = A.GeomAugment(GC.CONF, CC.multiobject_shapes(2, 16))
    assert mo.channels == GC.MULTIOBJECT and mo.disp_name == 'displacement' and len(mo.names) == 12
    for bad in ({'image0': (4, 16, 16, 3), 'flow': (4, 16, 16, 2), 'disp': (4, 2)},          # a channel count other than 1 or 3
                {'image0': (4, 16, 16, 3), 'rgbd': (4, 16, 16, 4), 'disp': (4, 2)},
                {'image0': (4, 16, 16, 3)},                                                   # no displacement
                {'image0': (4, 16, 16, 3), 'labels': (4, 5)},
                {'image0': (4, 16, 16, 3), 'disp': (4, 2), 'displacement': (4, 2)},           # two of them
                {'image0': (4, 16, 16, 3), 'disp': (4, 3)},
                {'image0': (4, 16, 16, 3), 'image1': (4, 8, 8, 3), 'disp': (4, 2)},           # views of two sizes
                {'disp': (4, 2)},                                                             # no view
                dict({'v%d' % k: (4, 8, 8, 1) for k in range(17)}, disp=(4, 2))):             # 17 views
        with pytest.raises(ValueError, match='geometric'):
            A.GeomAugment(GC.CONF, bad)
    # apply on the CPU is the twin; a tensor of another shape is refused
    raw = {k: torch.from_numpy(v) for k, v in zip(on.names, GC.views(7, 4, 16, 16, on.channels))}
    raw['disp'] = torch.from_numpy(GC.disp(8, 4))
    keep = {k: v.clone() for k, v in raw.items()}
    got = on.apply(dict(raw))
    outs, d = A.geom_augment_host([keep[k].numpy() for k in on.names], keep['disp'].numpy(), on.params)
    assert _same(on.params, A.draw_geom_params(np.random.default_rng([0, 0, 1]), 4, GC.CONF, 16, 16))
    for k, o in zip(on.names, outs):
        assert _same(got[k].numpy(), o) and torch.equal(raw[k], keep[k])
    assert _same(got['disp'].numpy(), d) and got['disp'] is raw['disp']                       # in place
    with pytest.raises(ValueError, match='geometric'):
        on.apply(dict(raw, image1=torch.zeros(4, 16, 16, 1)))


def test_model_classes():
    """every mv3d class refuses each key (its labels are an absolute pose of a single view); every supporting class builds with them;
    a bad value is refused by every class before it builds anything"""
    from dynamic_multiview_3d_amd import mv3d, multiobject_main_model
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.appearance_flow_tinghui import AppearanceFlowTinghui
    from dynamic_multiview_3d_amd.lowdim_angle import AppFlowLowDimAngle
    from dynamic_multiview_3d_amd.highdim_angle import AppFlowHighDimAngle
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    from dynamic_multiview_3d_amd.model_base import ModelBase
    assert ModelBase.supports_geom_augment is False
    keys = ({'augment_flip': 0.5}, {'augment_zoom': 2.0}, {'augment_zoom': 2.0, 'augment_shift': 0.5})
    for cls in (mv3d.mv3d_nobg_nodm, mv3d.mv3d_nobg_dm, mv3d.mv3d_bg_nodm):
        assert cls.supports_geom_augment is False
        for k in keys:
            with pytest.raises(ValueError, match='augment_flip'):
                cls(dict({'batch_size': 2}, **k), device='cpu')
        with pytest.raises(ValueError):
            cls({'batch_size': 2, 'augment_shift': 0.5}, device='cpu')
    af = {'batch_size': 2, 'learning_rate': 1e-4}
    bp = dict(af, use_color='', use_depth='', depth_lr_factor=0.1)
    mo = dict(af, use_color='', combination_image='', fully_conv='')
    for cls, base in ((AppearanceFlowModel, af), (AppearanceFlowTinghui, af), (AppFlowLowDimAngle, af), (AppFlowHighDimAngle, af),
                      (Base_Prediction_Model, bp), (MultiObjectAppFlow, mo), (multiobject_main_model.Base_Prediction_Model, mo)):
        assert cls.supports_geom_augment is True
        with pytest.raises(ValueError, match='augment_zoom'):
            cls(dict(base, augment_zoom=5.0), load_tfrec=False, device='cpu')
    for cls, base in ((AppearanceFlowModel, af), (Base_Prediction_Model, bp), (MultiObjectAppFlow, mo),
                      (multiobject_main_model.Base_Prediction_Model, mo)):
        m = cls(dict(base, **GC.CONF), load_tfrec=False, device='cpu')
        stage = A.GeomAugment(m.conf, {k: tuple(t.shape) for k, t in m.graph.inputs.items()})
        assert stage.enabled and len(stage.names) == (12 if 'combination_image' in base else 4)


def test_geom_augmented_data_hands_out_copies():
    """the synthetic feed's wrapper: transformed copies, the pool untouched, behind the colour wrapper and in front of the mirror"""
    class Pool:
        def __init__(self):
            self.b = {'image0': torch.from_numpy(CC.images('u8', 1, (4, 16, 16, 3))), 'image1': torch.from_numpy(CC.images('u8', 2, (4, 16, 16, 3))),
                      'depth_image0': torch.rand(4, 16, 16, 1), 'depth_image1': torch.rand(4, 16, 16, 1), 'disp': torch.rand(4, 2)}

        def next(self):
            return self.b
    pool = Pool()
    keep = {k: v.clone() for k, v in pool.b.items()}
    shapes = CC.appflow_shapes(4, 16)
    conf = dict(CC.CONF, batch_size=4, pair_swap=True, **GC.CONF)
    names = [k for k in shapes if k != 'disp']
    data = A.AugmentedData(pool, A.ColorAugment(conf, shapes))
    data = A.GeomAugmentedData(data, A.GeomAugment(conf, shapes))
    data = PS.PairSwappedData(data, PS.PairSwap(conf, 4))
    crng, grng = np.random.default_rng([0, 0]), np.random.default_rng([0, 0, 1])
    for _ in range(2):
        got = data.next()
        col = A.color_augment_host([keep[k].numpy() for k in names], A.draw_params(crng, 4, CC.CONF), A.ALL_STAGES)
        outs, d = A.geom_augment_host(col, keep['disp'].numpy(), A.draw_geom_params(grng, 4, GC.CONF, 16, 16))
        want = PS.mirror_host(dict({k: o[:2] for k, o in zip(names, outs)}, disp=d[:2]))
        for k in shapes:
            assert _same(got[k].numpy(), want[k]), k
        for k in keep:
            assert torch.equal(pool.b[k], keep[k]), k
    off = A.GeomAugmentedData(pool, A.GeomAugment({}, shapes))
    assert off.next()['disp'] is pool.b['disp']
    assert off.b is pool.b                                           # attributes of the source show through


# ---------------------------------------------------------------- the CPU reader
def _read(conf, shapes, batches, **kw):
    inp = R.TFRecordInput(conf, shapes, device='cpu', **kw)
    try:
        return [{k: v.numpy().copy() for k, v in inp.next().items()} for _ in range(batches)]
    finally:
        inp.close()


def _want(raw, names, disp, crng, grng, n, size, colour=True):
    views = [raw[k] for k in names]
    if colour:
        views = A.color_augment_host(views, A.draw_params(crng, n, CC.CONF), A.ALL_STAGES)
    outs, d = A.geom_augment_host(views, raw[disp], A.draw_geom_params(grng, n, GC.CONF, size, size))
    return dict(zip(names, outs), **{disp: d})


@pytest.mark.parametrize("inputs", ['appflow', 'multiobject'])
def test_cpu_reader(tmp_path, inputs):
    shapes = (CC.appflow_shapes if inputs == 'appflow' else CC.multiobject_shapes)(4, 16)
    disp = 'disp' if inputs == 'appflow' else 'displacement'
    names = [k for k in shapes if k != disp]
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0}
    plain = _read(base, shapes, 3, seed=4)
    # geometry alone, and behind the colour stage: geom_augment_host(color_augment_host(raw))
    for colour in (False, True):
        conf = dict(base, **GC.CONF)
        if colour:
            conf.update(CC.CONF)
        got = _read(conf, shapes, 3, seed=4)
        crng, grng = np.random.default_rng([0, 0]), np.random.default_rng([0, 0, 1])
        for p, g in zip(plain, got):
            want = _want(p, names, disp, crng, grng, 4, 16, colour)
            assert set(g) == set(shapes)
            for k in shapes:
                assert _same(g[k], want[k]), k
            assert not np.array_equal(g['image0'], p['image0'])
    # rank and augment_seed select the generator
    got = _read(dict(base, augment_seed=9, **GC.CONF), shapes, 1, seed=4, rank=1, world=1)
    want = _want(plain[0], names, disp, None, np.random.default_rng([9, 1, 1]), 4, 16, colour=False)
    assert all(_same(got[0][k], want[k]) for k in shapes)
    # with the keys absent (or off) the reader is the plain one; validation inputs and test_mode are never transformed
    conf = dict(base, **GC.CONF)
    for c, kw in ((dict(base, augment_flip=0, augment_zoom=None, augment_shift=0.0), {}), (dict(conf, train_val_split=0.0), {'training': False}),
                  (dict(conf, test_mode=''), {})):
        ref = dict(base, **{k: c[k] for k in ('train_val_split', 'test_mode') if k in c})
        for a, b in zip(_read(ref, shapes, 2, seed=4, **kw), _read(c, shapes, 2, seed=4, **kw)):
            assert list(a) == list(b)
            for k in a:
                assert _same(a[k], b[k]), k
    for c, kw in ((base, {}), (dict(conf, test_mode=''), {}), (dict(conf, train_val_split=0.0), {'training': False})):
        inp = R.TFRecordInput(c, shapes, device='cpu', **kw)
        assert inp.geom is None and inp.augment is None
        inp.close()
    with pytest.raises(ValueError):
        R.TFRecordInput(dict(base, augment_shift=0.5), shapes, device='cpu')
    with pytest.raises(ValueError, match='geometric'):
        R.TFRecordInput(conf, {'image0': (4, 16, 16, 3), 'labels': (4, 5)}, device='cpu')


def test_cpu_reader_with_pair_swap(tmp_path):
    """one parameter row per RECORD, the mirror behind it: image0[n + B/2] == image1[n] bit for bit, disp[n + B/2] == -disp[n], and the
    batch is mirror_host(geom_augment_host(color_augment_host(records)))"""
    shapes = CC.appflow_shapes(4, 16)
    names = [k for k in shapes if k != 'disp']
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'pair_swap': True}
    plain = _read(base, shapes, 3, seed=4)
    got = _read(dict(base, **CC.CONF, **GC.CONF), shapes, 3, seed=4)
    crng, grng = np.random.default_rng([0, 0]), np.random.default_rng([0, 0, 1])
    flipped = 0
    for p, g in zip(plain, got):
        for a, b in (('image0', 'image1'), ('depth_image0', 'depth_image1')):
            assert _same(g[a][2:], g[b][:2]) and _same(g[b][2:], g[a][:2])
        assert _same(g['disp'][2:], -g['disp'][:2])
        records = {k: v[:2] for k, v in p.items()}
        want = PS.mirror_host(_want(records, names, 'disp', crng, grng, 2, 16))
        for k in shapes:
            assert _same(g[k], want[k]), k
        flipped += int(np.sum(g['disp'][:2, 1] == -p['disp'][:2, 1]))
    assert 0 < flipped < 6                                           # some records mirrored, some not
    inp = R.TFRecordInput(dict(base, **GC.CONF), shapes, device='cpu')
    assert inp.geom.n == 2                                           # built with nrec rows
    inp.close()


# ---------------------------------------------------------------- the entry point's argument checks (nothing is launched)
def test_abi_argument_checks():
    lib = _lib.lib()
    n, h, w = 2, 33, 130
    big = 4 * n * h * w * 3
    S0, D0, P, DSP = 0x10000000, 0x20000000, 0x30000000, 0x31000000     # never dereferenced: every call below fails its checks

    def call(src=None, dst=None, ch=(3, 1, 3), nv=None, n=n, h=h, w=w, params=P, disp=DSP, null=()):
        src = [S0 + i * 0x1000000 for i in range(len(ch))] if src is None else src
        dst = [D0 + i * 0x1000000 for i in range(len(ch))] if dst is None else dst
        a_src = None if 'src' in null else (C.c_void_p * max(len(src), 1))(*src)
        a_dst = None if 'dst' in null else (C.c_void_p * max(len(dst), 1))(*dst)
        a_ch = None if 'ch' in null else (C.c_int * max(len(ch), 1))(*ch)
        return lib.raw_geom_augment(a_src, a_dst, a_ch, len(ch) if nv is None else nv, n, h, w, params, disp, None)
    for null in ('src', 'dst', 'ch'):
        assert call(null=(null,)) == E_INVAL
    assert call(params=None) == E_INVAL and 'null' in lib.last_error() and 'mv3d_geom_augment' in lib.last_error()
    assert call(src=[S0, None, S0 + 0x2000000]) == E_INVAL and call(dst=[D0, D0 + 0x1000000, None]) == E_INVAL
    assert call(ch=(), nv=0) == E_INVAL and call(ch=(1,) * 17) == E_INVAL and call(nv=-1) == E_INVAL
    assert 'views' in lib.last_error()
    for c in (0, 2, 4, -1):
        assert call(ch=(3, c)) == E_INVAL
    assert 'channels' in lib.last_error()
    for kw in ({'n': 0}, {'h': 0}, {'w': -1}, {'n': 1 << 20, 'h': 1 << 10, 'w': 1 << 10}, {'n': 1, 'h': 1 << 15, 'w': 1 << 15}):
        assert call(**kw) == E_INVAL, kw
    for off in (4, 8, 12):
        assert call(src=[S0 + off], dst=[D0], ch=(3,)) == E_INVAL and call(src=[S0], dst=[D0 + off], ch=(1,)) == E_INVAL
        assert call(params=P + off) == E_INVAL and call(disp=DSP + off) == E_INVAL
    assert '16-byte' in lib.last_error()
    # equal or overlapping buffers: a source with a destination, two destinations, two sources; a 1-channel view is a third as long
    assert call(src=[S0], dst=[S0], ch=(3,)) == E_INVAL and 'overlap' in lib.last_error()
    assert call(src=[S0], dst=[S0 + big - 16], ch=(3,)) == E_INVAL and call(src=[S0 + 16], dst=[S0], ch=(3,)) == E_INVAL
    assert call(src=[S0, S0 + 0x1000000], dst=[D0, D0 + 64], ch=(3, 1)) == E_INVAL
    assert call(src=[S0, S0], dst=[D0, D0 + 0x1000000], ch=(3, 3)) == E_INVAL
    assert call(src=[S0, D0 + big // 3 - 16], dst=[D0, D0 + 0x1000000], ch=(3, 1)) == E_INVAL          # inside destination 0 ...
    assert call(src=[S0, D0 + big // 3 - 16], dst=[D0, D0 + 0x1000000], ch=(1, 3)) == E_INVAL          # ... also when it is short
