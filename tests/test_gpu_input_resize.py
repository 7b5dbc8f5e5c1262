"""mv3d_u8_process_image on the GPU -- central square crop + TF 1.3 bicubic + / 255 of uint8 record images -- and the reader and
train driver on top of it (conf['record_image_size']).

Every comparison is bitwise against tests/resize_cases.py: each operation is an fp32 multiply, add, floor, round-to-even or
correctly rounded division, the order is fixed and the unit is built without contraction; three of the ratios (1, 1/2, 2) are
exact in integers whatever the order."""
import json

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import resize_cases as RC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25


def _run(src, ho, wo):
    """the entry point on a uint8 [N, Hs, Ws, C] array; the words behind the output must stay untouched"""
    n, hs, ws, c = src.shape
    count = n * ho * wo * c
    d_src = torch.from_numpy(src).to(DEV)
    d_dst = torch.full((count + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.lib().u8_process_image(d_src.data_ptr(), n, hs, ws, c, d_dst.data_ptr(), ho, wo, stream())
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    assert np.all(out[count:] == SENTINEL), "wrote past the output"
    return out[:count].reshape(n, ho, wo, c)


def _check(src, ho, wo):
    got = _run(src, ho, wo)
    np.testing.assert_array_equal(got, RC.reference(src, ho, wo))
    exact = RC.integer_version(src.shape[1], src.shape[2], ho) if ho == wo else None
    if exact is not None:
        np.testing.assert_array_equal(got, exact(src))
    return got


@pytest.mark.parametrize("c", RC.CHANNELS)
@pytest.mark.parametrize("n", [1, 32])
@pytest.mark.parametrize("hs,ws,out", RC.CASES)
def test_sizes_bitwise(hs, ws, out, n, c):
    _check(RC.random_u8(hs + out + 7 * n + c, n, hs, ws, c), out, out)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_and_unequal_sides(c):
    _check(RC.random_u8(40 + c, 3, 40, 52, c), 24, 56)


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("out", [64, 200, 256])
def test_all_black_and_all_white(out, value):
    got = _check(np.full((2, 128, 128, 3), value, np.uint8), out, out)
    bound = 255 * RC.MAX_ABS_WEIGHT_SUM ** 2 * 12 * 2.0 ** -24           # see test_input_resize_host.py
    assert np.abs(got * np.float32(255) - np.float32(value)).max() <= bound


@pytest.mark.parametrize("c", RC.CHANNELS)
@pytest.mark.parametrize("hs,ws,out", [(128, 128, 75), (100, 100, 75), (1400, 1400, 64)])
def test_fallback_path(hs, ws, out, c):
    """rows of 75 * c floats are no multiple of 16 bytes (c = 1, 3); 1400 -> 64 at c = 3 needs a window beyond the tile's LDS
    budget even at one output row per tile (at c = 1 it is the one-row tile that runs)"""
    _check(RC.random_u8(out + c, 2, hs, ws, c), out, out)


def test_upper_bound_of_the_sides():
    """both sides of the record and of the output at the limit the entry point admits (4096)"""
    _check(RC.random_u8(1, 1, 4096, 24, 1), 4096, 4096)               # tall record: rows 2036 .. 2059
    _check(RC.random_u8(2, 1, 16, 4096, 1), 4096, 8)                  # wide record: columns 2040 .. 2055


def test_one_pixel_and_tiny_records():
    _check(RC.random_u8(3, 2, 1, 1, 3), 8, 8)
    _check(RC.random_u8(4, 2, 2, 3, 4), 5, 7)
    _check(RC.random_u8(5, 1, 37, 37, 4), 1, 1)


@pytest.mark.parametrize("c", RC.CHANNELS)
def test_identity_equals_u8_to_unit_f32(c):
    src = RC.random_u8(11 + c, 32, 128, 128, c)
    d_src = torch.from_numpy(src).to(DEV)
    want = torch.empty(src.shape, dtype=torch.float32, device=DEV)
    _lib.lib().u8_to_unit_f32(src.size, d_src.data_ptr(), want.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_run(src, 128, 128), want.cpu().numpy())


def _write_multiobject_shards(data, nfiles=2, per_file=6, size=128, seed=0):
    from dynamic_multiview_3d_amd.multiobject_appflow import INPUTS
    rng = np.random.default_rng(seed)
    recs = []
    for f in range(nfiles):
        with R.TFRecordWriter(str(data / ('%d.tfrecords' % f))) as w:
            for _ in range(per_file):
                s = {name: rng.integers(0, 256, (size, size, ch), dtype=np.uint8) for name, ch in INPUTS}
                s['displacement'] = rng.uniform(-1, 1, 2).astype(np.float32)
                recs.append(s)
                w.write(R.serialize_example({k: (v.tobytes() if v.dtype == np.uint8 else v) for k, v in s.items()}))
    return recs


def test_gpu_reader_equals_cpu_reader(tmp_path):
    from dynamic_multiview_3d_amd.multiobject_appflow import INPUTS
    recs = _write_multiobject_shards(tmp_path, nfiles=2, per_file=3)
    conf = {'batch_size': 4, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': '', 'record_image_size': 128}
    shapes = {name: (4, 256, 256, ch) for name, ch in INPUTS}
    shapes['displacement'] = (4, 2)
    cpu = R.TFRecordInput(conf, shapes, device='cpu')
    gpu = R.TFRecordInput(conf, shapes, device='cuda:0')
    try:
        for b in range(3):                                               # 12 records out of 6: file boundary and a second epoch
            want, got = cpu.next(), gpu.next()
            torch.cuda.synchronize()
            assert set(got) == set(shapes)
            for k in shapes:
                assert got[k].device.type == 'cuda' and got[k].dtype == torch.float32 and tuple(got[k].shape) == shapes[k]
                np.testing.assert_array_equal(got[k].cpu().numpy(), want[k].numpy())
            np.testing.assert_array_equal(got['image0'][0].cpu().numpy(), RC.double(recs[(4 * b) % 6]['image0'][None])[0])
            np.testing.assert_array_equal(got['displacement'][1].cpu().numpy(), recs[(4 * b + 1) % 6]['displacement'])
    finally:
        cpu.close()
        gpu.close()


def test_train_driver_resizes_128_shards_to_256(tmp_path):
    """BASELINE config 5's model (MultiObjectAppFlow, fully_conv, 256 x 256) trains from 128 x 128 shards through train.py: the
    batch the model holds after the last step is the first two records of the only training file, resized."""
    from dynamic_multiview_3d_amd import train
    data = tmp_path / 'data'
    data.mkdir()
    recs = _write_multiobject_shards(data, nfiles=2, per_file=6)
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom multiobject_appflow import MultiObjectAppFlow\n"
        "configuration = {'experiment_name': 't', 'data_dir': %r, 'output_dir': os.path.dirname(os.path.realpath(__file__)) + '/modeldata',\n"
        "  'num_iterations': 6, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.5, 'model': MultiObjectAppFlow,\n"
        "  'use_color': '', 'use_depth': 0.1, 'combination_image': '', 'gen_sep_images': '', 'fully_conv': '',\n"
        "  'image_size': 256, 'record_image_size': 128}\n" % str(data))
    model = train.main(['--hyper', str(conf_py)])
    rows = [json.loads(l) for l in open(tmp_path / 'modeldata' / 'train_log.jsonl')]
    losses = [r['training_loss'] for r in rows if 'training_loss' in r]
    assert len(losses) == 1 and all(np.isfinite(losses))
    # 7 steps x 2 records over a 6-record training file: the 7th batch wraps to records 0, 1 of file 0 again
    first = recs[:2]
    assert tuple(model.image0.shape) == (2, 256, 256, 3)
    np.testing.assert_array_equal(model.image0.numpy(), RC.reference(np.stack([r['image0'] for r in first]), 256, 256))
    np.testing.assert_array_equal(model.image1_mask1.numpy(), RC.double(np.stack([r['image1_mask1'] for r in first])))
    np.testing.assert_array_equal(model.displacement.numpy(), np.stack([r['displacement'] for r in first]))
