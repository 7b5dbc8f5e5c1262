"""mv3d_color_augment on the GPU against its numpy twin (augment.color_augment_host), and the reader and the train driver on top
of it (conf['augment_*']).

Every comparison is by value with assert_array_equal, no tolerance: each operation of the map is an fp32 add, multiply, compare,
floor, truncation or correctly rounded division, the unit is built without contraction, and the contrast pivot's double sums have a
fixed order that the twin restates.  Every buffer carries a sentinel tail that must stay untouched."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import augment as A
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import color_augment_cases as CC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
WS_SENTINEL = -3.5
ALL = A.ALL_STAGES
MASKS = (A.BRIGHTNESS, A.SATURATION, A.HUE, A.CONTRAST, CC.SH, ALL)
SHAPES = [(1, 1, 1, 1), (3, 5, 7, 1), (2, 16, 16, 2), (2, 67, 61, 3), (2, 128, 128, 4)]       # (n, h, w, views)


def _run(views, params, stages, repeat=1):
    """the entry point on float32 [n, h, w, 3] arrays, in place on separate allocations; returns (results, workspace doubles).  The
    words behind every view and behind the workspace must stay untouched, and so must the workspace without the contrast bit."""
    lib = _lib.lib()
    n, h, w, _ = views[0].shape
    count = views[0].size
    bufs = []
    for v in views:
        t = torch.full((count + 64,), SENTINEL, dtype=torch.float32, device=DEV)
        t[:count] = torch.from_numpy(v.reshape(-1)).to(DEV)
        bufs.append(t)
    need = int(lib.color_augment_workspace_bytes(n, len(views), h, w))
    assert need == n * len(views) * (-(-h * w // A.CHUNK)) * 24
    ws = torch.full((need // 8 + 8,), WS_SENTINEL, dtype=torch.float64, device=DEV)
    d_par = torch.from_numpy(np.ascontiguousarray(params, np.float32)).to(DEV)
    ptrs = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
    for r in range(repeat):
        if r:
            for b, v in zip(bufs, views):
                b[:count] = torch.from_numpy(v.reshape(-1)).to(DEV)
        lib.color_augment(ptrs, len(bufs), n, h, w, d_par.data_ptr(), stages, ws.data_ptr(), need, stream())
    torch.cuda.synchronize()
    outs = []
    for b, v in zip(bufs, views):
        o = b.cpu().numpy()
        assert np.all(o[count:] == SENTINEL), "wrote past a view"
        outs.append(o[:count].reshape(v.shape))
    wsh = ws.cpu().numpy()
    written = need // 8 if stages & A.CONTRAST else 0
    assert np.all(wsh[written:] == WS_SENTINEL), "wrote past the workspace (or into it without the contrast bit)"
    assert not np.any(wsh[:written] == WS_SENTINEL)
    return outs, wsh[:need // 8]


def _check(views, params, stages):
    got, _ = _run(views, params, stages)
    want = A.color_augment_host(views, params, stages)
    for g, w_ in zip(got, want):
        np.testing.assert_array_equal(g, w_)
    return got


@pytest.mark.parametrize("kind", ['u8', 'over'])
@pytest.mark.parametrize("n,h,w,views", SHAPES)
def test_kernel_equals_twin_bitwise(n, h, w, views, kind):
    rng = np.random.default_rng(n * h + w + views)
    x = [CC.images(kind, 100 * v + h, (n, h, w, 3)) for v in range(views)]
    for stages in MASKS:
        _check(x, A.draw_params(rng, n, CC.CONF), stages)


def test_crafted_pixels():
    for cases, stages in ((CC.CRAFTED_SH, CC.SH), (CC.CRAFTED_B, A.BRIGHTNESS)):
        x, params, pos = CC.crafted_batch(cases)
        CC.check_crafted(cases, _check([x], params, stages)[0], pos)
    # scattered into one image of the all-stages run, too (parameters drawn: the twin is the expectation)
    x, _, _ = CC.crafted_batch(CC.CRAFTED_SH + CC.CRAFTED_B, h=23, w=19)
    _check([x, x[::-1].copy()], A.draw_params(np.random.default_rng(0), x.shape[0], CC.CONF), ALL)


def test_chunk_sums_and_pivot_order():
    """the workspace holds the chunk sums [sample, view, chunk, channel] of the twin's order; on overshooting float32 images a
    plain float64 sum in another order differs in the last bits of some of them, which is what makes this a test of the order"""
    n, h, w, views = 2, 67, 61, 3
    x = [CC.images('over', 40 + v, (n, h, w, 3)) for v in range(views)]
    _, ws = _run(x, A.draw_params(np.random.default_rng(1), n, CC.CONF), A.CONTRAST)
    part = ws.reshape(n, views, 1, 3)
    total = np.zeros((n, 3))
    for v in range(views):
        total = total + part[:, v, 0]
    np.testing.assert_array_equal(np.float32(total / (views * h * w)), A.joint_pivots(x))


def test_result_does_not_depend_on_the_grid():
    """the unit has no grid override (it keeps no state): the last sample of an n = 3 call against the same sample as an n = 1 call
    (another grid, another block index, and at 67 x 61 another alignment: 16-byte accesses against scalar ones), and a call whose
    2400 work items exceed the 2048-workgroup cap, so that every workgroup walks two items of different samples"""
    rng = np.random.default_rng(2)
    x = [CC.images('over', 60 + v, (3, 67, 61, 3)) for v in range(2)]
    params = A.draw_params(rng, 3, CC.CONF)
    for stages in (ALL, CC.SH):
        full, _ = _run(x, params, stages)
        one, _ = _run([v[2:3].copy() for v in x], params[2:3], stages)
        for f, o in zip(full, one):
            np.testing.assert_array_equal(f[2:3], o)
    x = [CC.images('over', 70 + v, (300, 6, 6, 3)) for v in range(8)]
    _check(x, A.draw_params(rng, 300, CC.CONF), ALL)


def test_same_bits_twice():
    x = [CC.images('over', 80 + v, (2, 67, 61, 3)) for v in range(3)]
    params = A.draw_params(np.random.default_rng(3), 2, CC.CONF)
    first, ws1 = _run(x, params, ALL)
    second, ws2 = _run(x, params, ALL, repeat=2)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    assert ws1.tobytes() == ws2.tobytes()


def test_recorded_into_a_plan():
    """the pointer array is read at call time and travels by value: the call records like any other dispatch (two launches with
    the contrast bit, one without), and the replay gives the twin's bits after the array is gone"""
    lib = _lib.lib()
    x = [CC.images('over', 90 + v, (2, 16, 16, 3)) for v in range(2)]
    params = A.draw_params(np.random.default_rng(4), 2, CC.CONF)
    bufs = [torch.from_numpy(v).to(DEV) for v in x]
    d_par = torch.from_numpy(params).to(DEV)
    need = int(lib.color_augment_workspace_bytes(2, 2, 16, 16))
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    plans = []
    for stages in (ALL, CC.SH):
        plan = lib.plan_create()
        lib.plan_begin(plan)
        ptrs = (C.c_void_p * 2)(*[b.data_ptr() for b in bufs])
        lib.color_augment(ptrs, 2, 2, 16, 16, d_par.data_ptr(), stages, ws.data_ptr(), need, None)
        lib.plan_end()
        ptrs[0] = ptrs[1] = None
        del ptrs
        plans.append(plan)
    assert [lib.plan_size(p) for p in plans] == [2, 1]
    assert [o[0] for o in _lib.plan_ops(plans[0])] == ['color_augment_sums_kernel', 'color_augment_apply_kernel']
    torch.cuda.synchronize()
    for b, v in zip(bufs, x):                                            # recording launched nothing
        np.testing.assert_array_equal(b.cpu().numpy(), v)
    lib.plan_run(plans[0], stream())
    torch.cuda.synchronize()
    for b, want in zip(bufs, A.color_augment_host(x, params, ALL)):
        np.testing.assert_array_equal(b.cpu().numpy(), want)
    for p in plans:
        lib.plan_destroy(p)


def test_entry_point_refuses_device_buffers_it_cannot_take():
    lib = _lib.lib()
    t = torch.zeros(2 * 8 * 8 * 3 + 8, dtype=torch.float32, device=DEV)
    par = torch.zeros(2, 4, device=DEV)
    ws = torch.zeros(16, dtype=torch.float64, device=DEV)
    need = int(lib.color_augment_workspace_bytes(2, 2, 8, 8))
    for a, b in ((t.data_ptr(), t.data_ptr()), (t.data_ptr(), t.data_ptr() + 16), (t.data_ptr() + 4, ws.data_ptr())):
        ptrs = (C.c_void_p * 2)(a, b)
        assert lib.raw_color_augment(ptrs, 2, 2, 8, 8, par.data_ptr(), ALL, ws.data_ptr(), need, stream()) == -1
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


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


@pytest.mark.parametrize("inputs,record", [('appflow', 16), ('appflow', 8), ('multiobject', 16), ('multiobject', 8)])
def test_gpu_reader_equals_cpu_reader(tmp_path, inputs, record):
    """three batches of 4 over two files of three records (a file boundary and a second epoch), the record size the model's (16) or
    resized on the way (record_image_size 8 -> 16): the device reader's batches equal the CPU reader's, whose colour views are the
    twin's; depth maps, masks and displacements equal the unaugmented reader's"""
    shapes = (CC.appflow_shapes if inputs == 'appflow' else CC.multiobject_shapes)(4, 16)
    CC.write_shards(tmp_path, shapes, record)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0}
    if record != 16:
        base['record_image_size'] = record
    conf = dict(base, **CC.CONF)
    cpu, gpu, plain = _batches(conf, shapes, 'cpu'), _batches(conf, shapes, 'cuda:0'), _batches(base, shapes, 'cuda:0')
    colour = [k for k, s in shapes.items() if len(s) == 4 and s[3] == 3]
    assert len(colour) == (2 if inputs == 'appflow' else 4)
    rng = np.random.default_rng([0, 0])
    for c, g, p in zip(cpu, gpu, plain):
        assert set(g) == set(shapes)
        for k in shapes:
            np.testing.assert_array_equal(g[k], c[k], err_msg=k)
            if k not in colour:
                assert g[k].tobytes() == p[k].tobytes(), k
        want = A.color_augment_host([p[k] for k in colour], A.draw_params(rng, 4, CC.CONF), ALL)
        for k, w_ in zip(colour, want):
            np.testing.assert_array_equal(g[k], w_, err_msg=k)
            assert not np.array_equal(g[k], p[k])


def test_gpu_reader_leaves_validation_and_test_mode_alone(tmp_path):
    shapes = CC.appflow_shapes(4, 16)
    CC.write_shards(tmp_path, shapes, 16)
    base = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': ''}
    for a, b in zip(_batches(base, shapes, 'cuda:0', 2), _batches(dict(base, **CC.CONF), shapes, 'cuda:0', 2)):
        for k in shapes:
            assert a[k].tobytes() == b[k].tobytes(), k
    inp = R.TFRecordInput(dict(base, **CC.CONF), shapes, training=False, device='cuda:0')
    assert inp.augment is None
    inp.close()


# ---------------------------------------------------------------- the train driver
def _conf_file(tmp_path, extra):
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "from appearance_flow_model import AppearanceFlowModel\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 3, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.95, 'model': AppearanceFlowModel,\n"
        "  %s}\n" % (str(tmp_path / 'modeldata'), extra))
    return str(conf_py)


@pytest.mark.parametrize("keys", [True, False])
def test_train_driver_augments_copies_of_the_synthetic_pool(tmp_path, monkeypatch, keys):
    """iterations 0 .. 3 are four steps: the batch the model holds after the last one is pool[3] through the twin with the FOURTH
    parameter table of default_rng([0, 0]) -- or, with the keys absent, pool[3] itself; the pool is as it was built"""
    from dynamic_multiview_3d_amd import train
    plain_source = train.SyntheticData
    made = []

    class Spy(plain_source):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(train, 'SyntheticData', Spy)
    extra = ', '.join('%r: %r' % kv for kv in CC.CONF.items()) if keys else "'augment_hue': None"
    model = train.main(['--hyper', _conf_file(tmp_path, extra), '--synthetic', '--num_iterations', '3'])
    torch.cuda.synchronize()
    rows = [json.loads(l) for l in open(tmp_path / 'modeldata' / 'train_log.jsonl')]
    assert len(rows) == 1 and np.isfinite(rows[0]['training_loss'])
    pool = made[0].pool
    fresh = plain_source(model, seed=0).pool
    for a, b in zip(pool, fresh):                                        # pristine
        for k in b:
            assert torch.equal(a[k], b[k]), k
    last = {k: v.cpu().numpy() for k, v in fresh[3].items()}
    if keys:
        rng = np.random.default_rng([0, 0])
        for _ in range(4):
            params = A.draw_params(rng, 2, CC.CONF)
        want = A.color_augment_host([last['image0'], last['image1']], params, ALL)
        assert not np.array_equal(want[0], last['image0'])
    else:
        want = [last['image0'], last['image1']]
    np.testing.assert_array_equal(model.image0.numpy(), want[0])
    np.testing.assert_array_equal(model.image1.numpy(), want[1])
    for k in ('depth_image0', 'depth_image1', 'disp'):
        np.testing.assert_array_equal(getattr(model, k).numpy(), last[k])
