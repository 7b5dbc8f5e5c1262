"""mv3d_geom_augment on the GPU against its numpy twin (augment.geom_augment_host), and the reader and the train driver on top of
it (conf['augment_flip' / '_zoom' / '_shift']).

Every comparison is bitwise, no tolerance: each operation of the transform is an fp32 subtract, multiply, add, min, max or floor,
the unit is built without contraction, and the twin restates the order.  Every buffer carries a sentinel tail that must stay
untouched, the destinations are pre-filled with the sentinel (a pixel the kernel skipped would show), and the sources must come
back as they went in."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import augment as A
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import color_augment_cases as CC
from tests import geom_augment_cases as GC
from tests.gpu_utils import DEV

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
TAIL = 64


def _buf(a):
    t = torch.full((a.size + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)
    return t


def _run(views, disp, params, stream=None, repeat=1):
    """the entry point on float32 [n, h, w, c] arrays, out of place on separate allocations; returns (results, disp)"""
    lib = _lib.lib()
    n, h, w, _ = views[0].shape
    src = [_buf(v) for v in views]
    dst = [torch.full((v.size + TAIL,), SENTINEL, dtype=torch.float32, device=DEV) for v in views]
    d_par = torch.from_numpy(np.ascontiguousarray(params, np.float32)).to(DEV)
    d_disp = None if disp is None else _buf(disp)
    channels = (C.c_int * len(views))(*[v.shape[3] for v in views])
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    for r in range(repeat):
        if r:
            torch.cuda.synchronize()
            d_disp[:disp.size] = torch.from_numpy(disp.reshape(-1)).to(DEV)
            torch.cuda.synchronize()
        a_src = (C.c_void_p * len(views))(*[b.data_ptr() for b in src])
        a_dst = (C.c_void_p * len(views))(*[b.data_ptr() for b in dst])
        lib.geom_augment(a_src, a_dst, channels, len(views), n, h, w, d_par.data_ptr(), None if d_disp is None else d_disp.data_ptr(),
                         st.cuda_stream)
    torch.cuda.synchronize()
    outs = []
    for s, d, v in zip(src, dst, views):
        o = d.cpu().numpy()
        assert np.all(o[v.size:] == SENTINEL), "wrote past a destination"
        assert s.cpu().numpy()[:v.size].tobytes() == v.tobytes() and np.all(s.cpu().numpy()[v.size:] == SENTINEL), "changed a source"
        outs.append(o[:v.size].reshape(v.shape))
    if d_disp is not None:
        o = d_disp.cpu().numpy()
        assert np.all(o[disp.size:] == SENTINEL), "wrote past disp"
        d_disp = o[:disp.size].reshape(disp.shape)
    return outs, d_disp


def _check(views, disp, params, name=''):
    got, gd = _run(views, disp, params)
    want, wd = A.geom_augment_host(views, disp, params)
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g.tobytes() == w_.tobytes(), "%s: view %d differs from the twin at %d elements" % (name, k, int(np.sum(g != w_)))
    if disp is not None:
        assert gd.tobytes() == wd.tobytes(), name
    return got, gd


@pytest.mark.parametrize("n,h,w", GC.SHAPES)
def test_kernel_equals_twin_bitwise(n, h, w):
    for channels in GC.VIEW_LISTS:
        x = GC.views(10 * h + w, n, h, w, channels)
        d = GC.disp(h, n)
        for name, p in GC.param_rows(n, h, w):
            got, gd = _check(x, d, p, '%s %s' % (channels, name))
            if name == 'identity':
                assert all(g.tobytes() == v.tobytes() for g, v in zip(got, x)) and gd.tobytes() == d.tobytes()
            if name == 'flip':
                assert all(g.tobytes() == np.ascontiguousarray(v[:, :, ::-1]).tobytes() for g, v in zip(got, x))
                assert gd[:, 0].tobytes() == d[:, 0].tobytes() and gd[:, 1].tobytes() == (-d[:, 1]).tobytes()
    _check(x, None, p, 'without disp')


def test_multiobject_views_equal_twin_bitwise():
    """the twelve image inputs of the multi-object model in one launch"""
    n, h, w = 2, 16, 16
    x = GC.views(50, n, h, w, GC.MULTIOBJECT)
    d = GC.disp(51, n)
    for name, p in GC.param_rows(n, h, w):
        got, _ = _check(x, d, p, name)
        for g, v in zip(got, x):
            if v.shape[3] == 1 and set(np.unique(v)) <= {0.0, 1.0}:
                assert set(np.unique(g)) <= {0.0, 1.0}                   # a mask stays a mask
    # sixteen views, and a call whose work items exceed the 2048-workgroup cap: every workgroup walks several samples
    x = GC.views(60, 300, 6, 6, [3, 1] * 8)
    _check(x, GC.disp(61, 300), A.draw_geom_params(np.random.default_rng(5), 300, GC.WIDE, 6, 6), 'grid stride')


def test_constant_image_stays_constant():
    n, h, w = 2, 33, 130
    const = [np.full((n, h, w, 3), np.float32(0.3)), np.full((n, h, w, 1), np.float32(0.7))]
    for name, p in GC.param_rows(n, h, w, seed=1):
        got, _ = _run(const, None, p)
        assert got[0].tobytes() == const[0].tobytes() and got[1].tobytes() == const[1].tobytes(), name


def test_result_does_not_depend_on_the_grid_or_the_stream():
    """the unit has no grid override (it keeps no state): two calls on different streams; the last sample of an n = 3 call against
    the same sample as an n = 1 call (another grid, another block index, and at 33 x 130 another row alignment: 16-byte stores
    against scalar ones)"""
    n, h, w = 3, 33, 130
    x = GC.views(70, n, h, w, [3, 1, 3])
    d = GC.disp(71, n)
    p = A.draw_geom_params(np.random.default_rng(6), n, GC.WIDE, h, w)
    p[n - 1, 0] = 1
    first, fd = _run(x, d, p)
    other, od = _run(x, d, p, stream=torch.cuda.Stream())
    one, sd = _run([v[n - 1:].copy() for v in x], d[n - 1:].copy(), p[n - 1:])
    for a, b, c in zip(first, other, one):
        assert a.tobytes() == b.tobytes() and a[n - 1:].tobytes() == c.tobytes()
    assert fd.tobytes() == od.tobytes() and fd[n - 1:].tobytes() == sd.tobytes()


def test_same_bits_twice():
    n, h, w = 2, 33, 130
    x = GC.views(80, n, h, w, [3, 1])
    d = GC.disp(81, n)
    p = A.draw_geom_params(np.random.default_rng(7), n, GC.WIDE, h, w)
    first, fd = _run(x, d, p)
    second, sd = _run(x, d, p, repeat=2)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    assert fd.tobytes() == sd.tobytes()


def test_recorded_into_a_plan():
    """the three host arrays are read at call time and travel by value: the call records like any other dispatch, as one launch
    declaring 8 bytes per element, and the replay gives the twin's bits after the arrays are gone"""
    lib = _lib.lib()
    n, h, w = 2, 16, 16
    x = GC.views(90, n, h, w, [3, 1])
    d = GC.disp(91, n)
    p = GC.corner(n, h, w, 1, m=1)
    src = [torch.from_numpy(v).to(DEV) for v in x]
    dst = [torch.full_like(t, SENTINEL) for t in src]
    d_par, d_disp = torch.from_numpy(p).to(DEV), torch.from_numpy(d).to(DEV)
    plan = lib.plan_create()
    lib.plan_begin(plan)
    a_src = (C.c_void_p * 2)(*[t.data_ptr() for t in src])
    a_dst = (C.c_void_p * 2)(*[t.data_ptr() for t in dst])
    channels = (C.c_int * 2)(3, 1)
    lib.geom_augment(a_src, a_dst, channels, 2, n, h, w, d_par.data_ptr(), d_disp.data_ptr(), None)
    lib.plan_end()
    a_src[0] = a_src[1] = a_dst[0] = a_dst[1] = None
    channels[0] = channels[1] = 0
    del a_src, a_dst, channels
    assert lib.plan_size(plan) == 1
    ops = _lib.plan_ops(plan)
    assert ops[0][0] == 'geom_augment_kernel' and ops[0][2] == 8.0 * n * h * w * 4
    torch.cuda.synchronize()
    assert all(float((t != SENTINEL).sum()) == 0 for t in dst)           # recording launched nothing
    np.testing.assert_array_equal(d_disp.cpu().numpy(), d)
    lib.plan_run(plan, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want, wd = A.geom_augment_host(x, d, p)
    for t, w_ in zip(dst, want):
        assert t.cpu().numpy().tobytes() == w_.tobytes()
    assert d_disp.cpu().numpy().tobytes() == wd.tobytes()
    lib.plan_destroy(plan)


def test_entry_point_refuses_what_the_header_says():
    lib = _lib.lib()
    n, h, w = 2, 8, 8
    count = n * h * w * 3
    s = torch.zeros(count + 8, dtype=torch.float32, device=DEV)
    t = torch.zeros(2 * count + 8, dtype=torch.float32, device=DEV)
    par = torch.zeros(n + 1, 4, device=DEV)
    disp = torch.zeros(n + 2, 2, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(src, dst, ch, views=None, params=par.data_ptr(), dsp=disp.data_ptr()):
        k = len(src)
        return lib.raw_geom_augment((C.c_void_p * k)(*src), (C.c_void_p * k)(*dst), (C.c_int * k)(*ch), k if views is None else views,
                                    n, h, w, params, dsp, st)
    S, T = s.data_ptr(), t.data_ptr()
    assert call([S], [S], [3]) == -1                                     # a source is a destination
    assert call([S], [S + 16], [3]) == -1 and 'overlap' in lib.last_error()
    assert call([S, T], [T + 4 * count, T + 4 * count - 16], [3, 3]) == -1       # a destination overlaps a source
    assert call([S], [T], [2]) == -1 and 'channels' in lib.last_error()  # channel count 2
    assert call([S] * 17, [T] * 17, [1] * 17) == -1 and 'views' in lib.last_error()       # 17 views
    assert call([S + 4], [T], [3]) == -1 and call([S], [T + 8], [1]) == -1       # misalignment
    assert call([S], [T], [3], params=par.data_ptr() + 4) == -1 and call([S], [T], [3], dsp=disp.data_ptr() + 8) == -1
    assert '16-byte' in lib.last_error()
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0 and float(s.abs().sum()) == 0.0
    assert call([S], [T], [3]) == 0 and call([S], [T], [3], dsp=None) == 0       # and takes what it should
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the reader
def _batches(conf, shapes, device, count=3):
    inp = R.TFRecordInput(conf, shapes, device=device, seed=5)
    try:
        out = []
        for _ in range(count):
            b = inp.next()
            if device != 'cpu':
                torch.cuda.synchronize()
            out.append({k: v.cpu().numpy().copy() for k, v in b.items()})
        return out
    finally:
        inp.close()


@pytest.mark.parametrize("inputs,swap", [('appflow', False), ('appflow', True), ('multiobject', False)])
def test_gpu_reader_equals_cpu_reader(tmp_path, inputs, swap):
    """three batches of 4 over two files of three records (a file boundary and a second epoch), behind the colour stage: the device
    reader's batches equal the CPU reader's (whose views are the twins': tests/test_geom_augment_host.py); with pair_swap (the
    appearance-flow set only: a multi-object sample has no reverse) one transform per record and the mirror identities"""
    shapes = (CC.appflow_shapes if inputs == 'appflow' else CC.multiobject_shapes)(4, 16)
    disp = 'disp' if inputs == 'appflow' else 'displacement'
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0}
    if swap:
        base['pair_swap'] = True
    conf = dict(base, **CC.CONF, **GC.CONF)
    cpu, gpu, plain = _batches(conf, shapes, 'cpu'), _batches(conf, shapes, 'cuda:0'), _batches(base, shapes, 'cuda:0')
    nrec = 2 if swap else 4
    crng, grng = np.random.default_rng([0, 0]), np.random.default_rng([0, 0, 1])
    names = [k for k in shapes if k != disp]
    for c, g, p in zip(cpu, gpu, plain):
        assert set(g) == set(shapes)
        for k in shapes:
            assert g[k].tobytes() == c[k].tobytes(), k
        assert not np.array_equal(g['image0'], p['image0'])
        col = A.color_augment_host([p[k][:nrec] for k in names], A.draw_params(crng, nrec, CC.CONF), A.ALL_STAGES)
        want, wd = A.geom_augment_host(col, p[disp][:nrec], A.draw_geom_params(grng, nrec, GC.CONF, 16, 16))
        for k, w_ in zip(names, want):
            assert g[k][:nrec].tobytes() == w_.tobytes(), k
        assert g[disp][:nrec].tobytes() == wd.tobytes()
        if swap:
            assert g['image0'][2:].tobytes() == g['image1'][:2].tobytes() and g['image1'][2:].tobytes() == g['image0'][:2].tobytes()
            assert g['depth_image0'][2:].tobytes() == g['depth_image1'][:2].tobytes()
            assert g['disp'][2:].tobytes() == (-g['disp'][:2]).tobytes()


def test_gpu_reader_leaves_validation_and_test_mode_alone(tmp_path):
    shapes = CC.appflow_shapes(4, 16)
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': ''}
    for a, b in zip(_batches(base, shapes, 'cuda:0', 2), _batches(dict(base, **GC.CONF), shapes, 'cuda:0', 2)):
        for k in shapes:
            assert a[k].tobytes() == b[k].tobytes(), k
    inp = R.TFRecordInput(dict(base, **GC.CONF), shapes, training=False, device='cuda:0')
    assert inp.geom is None
    inp.close()
    del base['test_mode']
    inp = R.TFRecordInput(dict(base, train_val_split=0.0, **GC.CONF), shapes, training=False, device='cuda:0')
    assert inp.geom is None
    inp.close()
    inp = R.TFRecordInput(base, shapes, device='cuda:0')                 # keys absent: nothing is built
    assert inp.geom is None and inp.augment is None
    inp.close()


# ---------------------------------------------------------------- the train driver
def test_train_driver_transforms_copies_of_the_synthetic_pool(tmp_path, monkeypatch):
    """iterations 0 .. 3 are four steps: the batch the model holds after the last one is pool[3] through the twin with the FOURTH
    parameter table of default_rng([0, 0, 1]); the pool is as it was built"""
    from dynamic_multiview_3d_amd import train
    plain_source = train.SyntheticData
    made = []

    class Spy(plain_source):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(train, 'SyntheticData', Spy)
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "from appearance_flow_model import AppearanceFlowModel\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 3, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.95, 'model': AppearanceFlowModel,\n"
        "  %s}\n" % (str(tmp_path / 'modeldata'), ', '.join('%r: %r' % kv for kv in GC.CONF.items())))
    model = train.main(['--hyper', str(conf_py), '--synthetic', '--num_iterations', '3'])
    torch.cuda.synchronize()
    rows = [json.loads(l) for l in open(tmp_path / 'modeldata' / 'train_log.jsonl')]
    assert len(rows) == 1 and np.isfinite(rows[0]['training_loss'])
    fresh = plain_source(model, seed=0).pool
    for a, b in zip(made[0].pool, fresh):                                # pristine
        for k in b:
            assert torch.equal(a[k], b[k]), k
    last = {k: v.cpu().numpy() for k, v in fresh[3].items()}
    names = ['image0', 'image1', 'depth_image0', 'depth_image1']
    size = last['image0'].shape[1]
    rng = np.random.default_rng([0, 0, 1])
    for _ in range(4):
        params = A.draw_geom_params(rng, 2, GC.CONF, size, size)
    want, wd = A.geom_augment_host([last[k] for k in names], last['disp'], params)
    assert not np.array_equal(want[0], last['image0'])
    for k, w_ in zip(names, want):
        assert getattr(model, k).numpy().tobytes() == w_.tobytes(), k
    assert model.disp.numpy().tobytes() == wd.tobytes()
