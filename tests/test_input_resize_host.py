"""Record images that are not the model's size (conf['record_image_size']): the host side of the reader's process_image --
crop + TF 1.3 bicubic + / 255 (read_tf_records.process_image) against the tests' own restatement (tests/resize_cases.py),
the CPU reader end to end, and the argument validation of mv3d_u8_process_image.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import resize_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
P = 0x10000          # a fake, aligned device address: every call below must fail validation before it would launch


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _weights(tab, off):
    return [tab[2 * off + 1], tab[2 * off], tab[2 * (1024 - off)], tab[2 * (1024 - off) + 1]]


@pytest.mark.parametrize("tab", [R.bicubic_table, RC.table], ids=['package', 'restatement'])
def test_table_known_answers(tab):
    tab = tab()
    assert tab.dtype == np.float32 and tab.shape == (2050,)
    assert (tab[0], tab[1]) == (1.0, 0.0)
    assert (tab[2048], tab[2049]) == (0.0, 0.0)
    assert _weights(tab, 512) == [-3 / 32, 19 / 32, 19 / 32, -3 / 32]
    assert _weights(tab, 0) == [0.0, 1.0, 0.0, 0.0]
    sums = [float(np.abs(np.array(_weights(tab, off), np.float64)).sum()) for off in range(1025)]
    assert max(sums) == RC.MAX_ABS_WEIGHT_SUM and int(np.argmax(sums)) == 512


def test_package_table_is_the_restatement():
    np.testing.assert_array_equal(R.bicubic_table(), RC.table())


@pytest.mark.parametrize("c", RC.CHANNELS)
@pytest.mark.parametrize("hs,ws,out", RC.CASES)
def test_host_matches_restatement_bitwise(hs, ws, out, c):
    src = RC.random_u8(hs * 1000 + out + c, 2, hs, ws, c)
    got = R.process_image(src, (out, out))
    assert got.dtype == np.float32 and got.shape == (2, out, out, c)
    np.testing.assert_array_equal(got, RC.reference(src, out, out))
    exact = RC.integer_version(hs, ws, out)
    if exact is not None:
        np.testing.assert_array_equal(got, exact(src))


def test_integer_versions_cover_their_ratios():
    assert [RC.integer_version(*k) for k in RC.CASES[:3]] == [RC.identity, RC.half, RC.double]
    assert RC.integer_version(96, 128, 64) is None and RC.integer_version(100, 100, 128) is None


def test_non_square_record_crops_the_middle():
    src = RC.random_u8(5, 1, 96, 128, 3)
    np.testing.assert_array_equal(R.process_image(src, (64, 64)), R.process_image(np.ascontiguousarray(src[:, :, 16:112]), (64, 64)))
    tall = np.ascontiguousarray(src.transpose(0, 2, 1, 3))                         # 128 x 96: rows 16 .. 111
    np.testing.assert_array_equal(R.process_image(tall, (64, 64)), R.process_image(np.ascontiguousarray(tall[:, 16:112]), (64, 64)))
    np.testing.assert_array_equal(R.process_image(tall, (64, 64)), RC.reference(tall, 64, 64))


def test_unequal_output_sides_and_leading_axes():
    src = RC.random_u8(6, 2, 40, 40, 3)
    np.testing.assert_array_equal(R.process_image(src, (24, 56)), RC.reference(src, 24, 56))
    np.testing.assert_array_equal(R.process_image(src[0], (24, 56)), RC.reference(src[:1], 24, 56)[0])
    with pytest.raises(ValueError):
        R.process_image(src.astype(np.float32), (24, 56))


@pytest.mark.parametrize("hs,ws,out", RC.CASES)
def test_constant_image_stays_constant(hs, ws, out):
    """Weights sum to 1 only to rounding.  Twelve roundings (two four-term passes, the division, this test's multiply) on the
    largest possible magnitude, 255 times the squared largest sum of absolute weights: about 3.4e-4."""
    bound = 255 * RC.MAX_ABS_WEIGHT_SUM ** 2 * 12 * 2.0 ** -24
    for v in (0, 1, 127, 200, 255):
        got = R.process_image(np.full((1, hs, ws, 3), v, np.uint8), (out, out))
        err = np.abs(got * np.float32(255) - np.float32(v)).max()
        assert err <= bound, (v, err, bound)


# ------------------------------------------------------------------------------------------------- the reader on the CPU
def _write_shards(tmp_path, nfiles=2, per_file=3, seed=0, size=128):
    rng = np.random.default_rng(seed)
    recs = []
    for f in range(nfiles):
        with R.TFRecordWriter(str(tmp_path / ('%d.tfrecords' % f))) as w:
            for _ in range(per_file):
                a = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
                m = rng.integers(0, 256, (size, size, 1), dtype=np.uint8)
                d = rng.uniform(-1, 1, 2).astype(np.float32)
                recs.append((a, m, d))
                w.write(R.serialize_example({'image0': a.tobytes(), 'depth0': m.tobytes(), 'displacement': d}))
    return recs


def _shapes(b, side):
    return {'image0': (b, side, side, 3), 'depth_image0': (b, side, side, 1), 'disp': (b, 2)}


@pytest.mark.parametrize("side", [256, 64])
def test_cpu_reader_resizes_in_file_order_across_a_file_boundary(tmp_path, side):
    recs = _write_shards(tmp_path)
    conf = {'batch_size': 2, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': '', 'record_image_size': 128}
    inp = R.TFRecordInput(conf, _shapes(2, side), device='cpu')
    try:
        for b in range(3):                                       # the second batch takes record 2 of file 0 and record 0 of file 1
            out = inp.next()
            assert out['image0'].shape == (2, side, side, 3) and out['depth_image0'].shape == (2, side, side, 1)
            assert out['image0'].dtype == out['depth_image0'].dtype
            for i in range(2):
                a, m, d = recs[2 * b + i]
                np.testing.assert_array_equal(out['image0'][i].numpy(), RC.reference(a[None], side, side)[0])
                np.testing.assert_array_equal(out['depth_image0'][i].numpy(), RC.reference(m[None], side, side)[0])
                np.testing.assert_array_equal(out['disp'][i].numpy(), d)
    finally:
        inp.close()


def test_record_size_forms_and_the_identity_case(tmp_path):
    recs = _write_shards(tmp_path, nfiles=1, per_file=2)
    base = {'batch_size': 2, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': ''}
    outs = []
    for conf in (base, {**base, 'record_image_size': 128}, {**base, 'record_image_size': (128, 128)}):
        inp = R.TFRecordInput(conf, _shapes(2, 128), device='cpu')            # the key equal to the model's size: today's path
        assert inp.rspec == inp.spec
        outs.append(inp.next())
        inp.close()
    for o in outs:
        np.testing.assert_array_equal(o['image0'].numpy(), np.stack([r[0] for r in recs]).astype(np.float32) / np.float32(255))
    inp = R.TFRecordInput({**base, 'record_image_size': [128, 128]}, _shapes(2, 96), device='cpu')
    np.testing.assert_array_equal(inp.next()['image0'].numpy(), RC.reference(np.stack([r[0] for r in recs]), 96, 96))
    inp.close()
    for bad in (0, (128,), (128, 0), 'big', 12.5):
        with pytest.raises(ValueError, match='record_image_size'):
            R.TFRecordInput({**base, 'record_image_size': bad}, _shapes(2, 96), device='cpu')
    with pytest.raises(ValueError, match='Unequal height and width unsupported'):
        R.TFRecordInput({**base, 'record_image_size': 128}, {'image0': (2, 64, 96, 3)}, device='cpu')


@pytest.mark.parametrize("side", [256, 64])
def test_without_the_key_a_size_mismatch_still_raises(tmp_path, side):
    _write_shards(tmp_path, nfiles=1, per_file=2)
    conf = {'batch_size': 2, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': ''}
    inp = R.TFRecordInput(conf, {'image0': (2, side, side, 3), 'disp': (2, 2)}, device='cpu')
    with pytest.raises(RuntimeError, match='has %d bytes, expected %d' % (128 * 128 * 3, side * side * 3)):
        inp.next()
    inp.close()
    rec = next(R.read_records(str(tmp_path / '0.tfrecords')))
    with pytest.raises(ValueError, match='has 49152 bytes'):
        R.decode_record(rec, {'image0': (side, side, 3)})


def test_decode_record_with_a_record_size(tmp_path):
    recs = _write_shards(tmp_path, nfiles=1, per_file=1)
    rec = next(R.read_records(str(tmp_path / '0.tfrecords')))
    a, m, d = recs[0]
    got = R.decode_record(rec, {'image0': (256, 256, 3), 'depth_image0': (256, 256, 1), 'disp': (2,)}, record_size=128)
    np.testing.assert_array_equal(got['image0'], RC.reference(a[None], 256, 256)[0])
    np.testing.assert_array_equal(got['depth_image0'], RC.reference(m[None], 256, 256)[0])
    np.testing.assert_array_equal(got['disp'], d)
    same = R.decode_record(rec, {'image0': (128, 128, 3)}, record_size=(128, 128))
    np.testing.assert_array_equal(same['image0'], a.astype(np.float32) / np.float32(255))
    with pytest.raises(ValueError, match='has 49152 bytes, expected 100x100x3'):
        R.decode_record(rec, {'image0': (256, 256, 3)}, record_size=100)


def test_build_tfrecord_input_passes_the_key_through(tmp_path):
    recs = _write_shards(tmp_path, nfiles=1, per_file=2)

    class _T:
        def __init__(self, shape):
            self.shape = shape

    class _G:
        device = 'cpu'
        inputs = {k: _T(s) for k, s in _shapes(2, 64).items()}

    class _M:
        graph = _G()

    conf = {'batch_size': 2, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': '', 'record_image_size': 128}
    inp = R.build_tfrecord_input(conf, _M())
    np.testing.assert_array_equal(inp.next()['image0'].numpy(), RC.half(np.stack([r[0] for r in recs])))
    inp.close()


# ------------------------------------------------------------------------------------------------- the C entry point
def _call(lib, src=P, n=2, hs=128, ws=128, c=3, dst=P, ho=256, wo=256):
    return lib.raw_u8_process_image(src, n, hs, ws, c, dst, ho, wo, None)


def test_validation_without_device(lib):
    assert _call(lib, src=None) == E_INVAL and 'null' in lib.last_error()
    assert _call(lib, dst=None) == E_INVAL and 'null' in lib.last_error()
    for k in ('n', 'hs', 'ws', 'ho', 'wo'):
        assert _call(lib, **{k: 0}) == E_INVAL and 'shape' in lib.last_error(), k
        assert _call(lib, **{k: -3}) == E_INVAL, k
    for c in (0, 5, -1):
        assert _call(lib, c=c) == E_INVAL and 'channels' in lib.last_error()
    for k in ('hs', 'ws', 'ho', 'wo'):
        assert _call(lib, n=1, c=1, **{k: 4097}) == E_INVAL and '4096' in lib.last_error(), k
    for off in (4, 8, 12, 1):
        assert _call(lib, dst=P + off) == E_INVAL and 'aligned' in lib.last_error()
    assert _call(lib, n=1 << 20, hs=8, ws=8, c=1, ho=64, wo=64) == E_INVAL and '32-bit' in lib.last_error()     # 2^32 outputs
    assert _call(lib, n=1 << 20, hs=64, ws=64, c=1, ho=8, wo=8) == E_INVAL and '32-bit' in lib.last_error()     # 2^32 inputs
    assert _call(lib, n=128, hs=8, ws=8, c=1, ho=4096, wo=4096) == E_INVAL                                      # 2^31 outputs
    with pytest.raises(_lib.Mv3dError, match='mv3d_u8_process_image failed'):
        lib.u8_process_image(None, 1, 8, 8, 1, P, 8, 8, None)


def test_symbol_is_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'mv3d_hip.h')).read()
    assert re.search(r'\bint\s+mv3d_u8_process_image\s*\(const void\* src, int n, int hs, int ws, int c, void\* dst, int ho, int wo, '
                     r'void\* stream\);', hdr)
    assert 'mv3d_u8_process_image' in _lib.EXPORTS and len(_lib.STATUS_FUNCS['mv3d_u8_process_image']) == 9
    assert hasattr(lib.dll, 'mv3d_u8_process_image')
    from dynamic_multiview_3d_amd import build
    assert build.UNITS['process_image.hip'] == ['-ffp-contract=off']
