"""CPU-side checks of the image metrics and the event-file writer: closed forms of the numpy definition (metrics.py
image_metrics_host), the bytes of a scalar event derived by hand from the Event / Summary field numbers, a file read back
through the package's record framing, and the new C-ABI entries declared, exported and bound."""
import ctypes as C
import math
import os
import struct
import types

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics, summary
from dynamic_multiview_3d_amd import read_tf_records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the definition
def test_window_is_the_normalised_11_tap_gaussian():
    w = metrics.ssim_window()
    assert w.shape == (11,) and w.dtype == np.float64
    assert abs(w.sum() - 1.0) <= 2e-16
    assert np.array_equal(w, w[::-1]) and np.all(np.diff(w[:6]) > 0)
    assert abs(w[4] / w[5] - math.exp(-1 / 4.5)) <= 1e-15 and abs(w[0] / w[5] - math.exp(-25 / 4.5)) <= 1e-15
    w32 = metrics.ssim_window(np.float32)
    assert w32.dtype == np.float32 and abs(float(w32.astype(np.float64).sum()) - 1.0) <= 11 * 2.0 ** -25


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_images_give_exactly_one_and_zero(dtype):
    rng = np.random.default_rng(0)
    a = rng.uniform(0, 1, (2, 19, 23, 3)).astype(np.float32)
    out = metrics.image_metrics_host(a, a.copy(), 1.0, dtype)
    assert out.shape == (2, 3) and out.dtype == dtype
    assert np.all(out[:, metrics.SSIM] == 1.0) and np.all(out[:, metrics.L1] == 0.0) and np.all(out[:, metrics.MSE] == 0.0)
    assert np.all(np.isinf(metrics.psnr(out[:, metrics.MSE], 1.0)))
    b = (a - 0.5) * 1.5
    assert np.all(metrics.image_metrics_host(b, b, 1.5, dtype)[:, metrics.SSIM] == 1.0)


@pytest.mark.parametrize("p,q,max_val,ch", [(0.25, 0.75, 1.0, 3), (0.5, 0.5625, 1.0, 1), (-0.375, 0.75, 1.5, 4), (0.0, 1.0, 1.0, 2)])
def test_constant_images_closed_form(p, q, max_val, ch):
    a = np.full((2, 16, 21, ch), p, np.float32)
    b = np.full((2, 16, 21, ch), q, np.float32)
    out = metrics.image_metrics_host(a, b, max_val)
    c1 = (0.01 * max_val) ** 2
    want = (2 * p * q + c1) / (p * p + q * q + c1)              # the contrast term is c2 / c2
    assert np.abs(out[:, metrics.SSIM] - want).max() <= 1e-12
    assert np.abs(out[:, metrics.L1] - ch * abs(p - q)).max() <= 1e-15
    assert np.abs(out[:, metrics.MSE] - (p - q) ** 2).max() <= 1e-15
    assert abs(metrics.psnr((p - q) ** 2, max_val) - 10 * math.log10(max_val ** 2 / (p - q) ** 2)) <= 1e-12


def test_single_bright_pixel_by_hand():
    """One pixel of value v at (py, px) of an otherwise black image against a black image: a window with origin (oy, ox) sees it
    with weight w[py-oy] * w[px-ox] when both differences lie in 0..10, and every other one of the (H-10)(W-10) windows gives 1."""
    H, W, py, px, v = 20, 17, 3, 9, 0.8
    a = np.zeros((1, H, W, 1), np.float32)
    a[0, py, px, 0] = v
    b = np.zeros_like(a)
    m = metrics.ssim_map(a, b, 1.0)
    assert m.shape == (1, H - 10, W - 10, 1)
    w = metrics.ssim_window()
    v = float(np.float32(v))
    c1, c2 = 1e-4, 9e-4
    total, touched = 0.0, 0
    for oy in range(H - 10):
        for ox in range(W - 10):
            dy, dx = py - oy, px - ox
            if 0 <= dy <= 10 and 0 <= dx <= 10:
                g = w[dy] * w[dx]
                mx, s2 = v * g, v * v * g
                value = (c1 / (mx * mx + c1)) * (c2 / (s2 - mx * mx + c2))
                assert abs(m[0, oy, ox, 0] - value) <= 1e-13
                touched += 1
            else:
                value = 1.0
                assert m[0, oy, ox, 0] == 1.0
            total += value
    assert touched == 4 * 7                                          # oy in 0..3, ox in 0..6
    out = metrics.image_metrics_host(a, b, 1.0)
    assert abs(out[0, metrics.SSIM] - total / ((H - 10) * (W - 10))) <= 1e-13
    assert abs(out[0, metrics.L1] - v / (H * W)) <= 1e-15 and abs(out[0, metrics.MSE] - v * v / (H * W)) <= 1e-15


def test_host_metrics_refuse_bad_operands():
    a = np.zeros((1, 10, 12, 3), np.float32)
    with pytest.raises(ValueError, match='window'):
        metrics.image_metrics_host(a, a)
    with pytest.raises(ValueError, match='shape'):
        metrics.image_metrics_host(np.zeros((1, 12, 12, 3)), np.zeros((1, 12, 12, 1)))
    with pytest.raises(ValueError, match='max_val'):
        metrics.image_metrics_host(np.zeros((1, 12, 12, 3)), np.zeros((1, 12, 12, 3)), 0.0)


# ------------------------------------------------------------------------------------------------ the C ABI entries
def test_metrics_entries_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, 'include', 'mv3d_hip.h')).read()
    for name in ('mv3d_image_metrics', 'mv3d_image_metrics_workspace_bytes'):
        assert name + '(' in hdr and name in _lib.EXPORTS and hasattr(lib.dll, name)
    assert len(_lib.STATUS_FUNCS['mv3d_image_metrics']) == 13
    assert _lib.OTHER_FUNCS['mv3d_image_metrics_workspace_bytes'] == (C.c_size_t, [C.c_int] * 4)
    # one double triple per 32x32 tile, rounded up to 256 bytes; 0 for a refused shape
    assert lib.image_metrics_workspace_bytes(64, 128, 128, 3) == 64 * 16 * 24
    assert lib.image_metrics_workspace_bytes(1, 11, 11, 2) == 256
    assert lib.image_metrics_workspace_bytes(2, 45, 77, 3) == 256 * -(-2 * 2 * 3 * 24 // 256)
    for bad in ((0, 16, 16, 3), (1, 10, 16, 3), (1, 16, 10, 3), (1, 16, 16, 5), (1, 16, 16, 0), (1, 32769, 16, 1)):
        assert lib.image_metrics_workspace_bytes(*bad) == 0


def test_metrics_validation_without_device(lib):
    """Argument errors come back before any launch, so they need no device: the code, and the argument named."""
    ok = dict(N=2, H=16, W=16, C=3, a=0x1000, a_ld=3, b=0x2000, b_ld=3, max_val=1.0, out=0x3000, ws=0x4000, ws_bytes=4096)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_image_metrics(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['max_val'], v['out'],
                                     v['ws'], v['ws_bytes'], None)
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(H=10), -1, 'H'), (dict(W=10), -1, 'W'), (dict(C=5), -1, 'C'), (dict(C=0), -1, 'C'),
                           (dict(a_ld=2), -1, 'a_ld'), (dict(b_ld=2), -1, 'b_ld'), (dict(max_val=0.0), -1, 'max_val'),
                           (dict(max_val=-1.0), -1, 'max_val'), (dict(max_val=float('inf')), -1, 'max_val'),
                           (dict(max_val=float('nan')), -1, 'max_val'), (dict(a=None), -1, 'a is null'), (dict(b=None), -1, 'b is null'),
                           (dict(out=None), -1, 'out is null'), (dict(ws=None), -1, 'workspace is null'), (dict(H=32769), -1, 'H'),
                           (dict(N=1 << 21, H=32768, W=32768), -1, 'tiles'), (dict(ws_bytes=255), -3, 'workspace'),
                           (dict(ws=0x4008), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error() and 'mv3d_image_metrics' in lib.last_error(), (kw, lib.last_error())


# ------------------------------------------------------------------------------------------------ event files
def _crc32c(data):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), bit by bit: independent of the library's implementation."""
    crc = 0xFFFFFFFF
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def _masked(data):
    c = _crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def _frame(payload):
    hdr = struct.pack('<Q', len(payload))
    return hdr + struct.pack('<I', _masked(hdr)) + payload + struct.pack('<I', _masked(payload))


def test_log_value_bytes_by_hand(lib, tmp_path):
    """Event{wall_time (1, double), step (2, varint), summary (5) {value (1) {tag (1), simple_value (2, float)}}}:
    key bytes are (field << 3) | wire type -> 0x09, 0x10, 0x2a; inside 0x0a, 0x0a, 0x15."""
    wall = 1500000000.25
    w = summary.FileWriter(str(tmp_path), clock=lambda: wall, hostname='host')
    assert os.path.basename(w.path) == 'events.out.tfevents.1500000000.host'
    summary.log_value(w, 0.25, 'loss', 300)
    w.close()
    wall_bytes = struct.pack('<d', wall)
    version = b'\x09' + wall_bytes + b'\x1a\x0d' + b'brain.Event:2'
    value = b'\x0a\x04loss' + b'\x15' + bytes.fromhex('0000803e')           # 0.25f little endian
    assert len(value) == 11
    event = b'\x09' + wall_bytes + b'\x10\xac\x02' + b'\x2a\x0d' + b'\x0a\x0b' + value        # 300 = 0b10_0101100 -> ac 02
    assert summary.encode_event(wall, step=300, scalars=[('loss', 0.25)]) == event
    assert open(w.path, 'rb').read() == _frame(version) + _frame(event)


def test_event_file_round_trip_and_corruption(lib, tmp_path):
    ticks = iter(range(100, 200))
    w = summary.FileWriter(str(tmp_path / 'logs'), clock=lambda: float(next(ticks)))
    rows = [('training_loss', 0.5, 0), ('training_loss', 0.125, 10), ('val_loss', 3.0e-3, 500), ('image/ssim', 0.75, 12000),
            ('image/psnr', float('inf'), 12000), ('big', 1.0, (1 << 40) + 3)]
    for tag, value, step in rows:
        summary.log_value(w, value, tag, step)
    w.flush()
    w.close()
    with pytest.raises(ValueError):
        w.add_scalar('late', 1.0, 1)
    events = summary.read_events(w.path)
    assert events[0]['file_version'] == 'brain.Event:2' and events[0]['scalars'] == [] and events[0]['wall_time'] == 100.0
    got = [(e['scalars'][0][0], e['scalars'][0][1], e['step']) for e in events[1:]]
    assert got == [(t, float(np.float32(v)), s) for t, v, s in rows]
    assert [e['wall_time'] for e in events[1:]] == [101.0 + i for i in range(len(rows))]
    # the records are plain TFRecords: the package's reader frames them, and a flipped byte fails a checksum
    payloads = list(R.read_records(w.path))
    assert len(payloads) == 1 + len(rows) and payloads[1] == summary.encode_event(101.0, step=0, scalars=[('training_loss', 0.5)])
    raw = bytearray(open(w.path, 'rb').read())
    for pos in (3, 12 + 5, len(raw) - 9):                         # a length byte, a payload byte of the first record, one of the last
        bad = bytearray(raw)
        bad[pos] ^= 0x40
        p = tmp_path / ('bad%d' % pos)
        p.write_bytes(bytes(bad))
        with pytest.raises(IOError):
            summary.read_events(str(p))


def test_log_value_is_exported_from_tf_utils():
    from dynamic_multiview_3d_amd import tf_utils
    assert tf_utils.log_value is summary.log_value


# ------------------------------------------------------------------------------------------------ evaluate(), host path
class _Arr:
    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def numpy(self):
        return self.a


def test_evaluate_aggregates_per_image_on_a_cpu_graph():
    """ModelBase.evaluate on a graph without a GPU scores each batch with image_metrics_host: means over the images, PSNR
    averaged per image, the loss averaged over the batches."""
    from dynamic_multiview_3d_amd.model_base import ModelBase
    rng = np.random.default_rng(3)
    batches = [(rng.uniform(0, 1, (2, 14, 12, 3)).astype(np.float32), rng.uniform(0, 1, (2, 14, 12, 3)).astype(np.float32)) for _ in range(3)]
    losses = [0.5, 0.25, 1.0]

    class M(ModelBase):
        def __init__(self):
            self.graph = types.SimpleNamespace(device=torch.device('cpu'), loss_expr=object())
            self.pred, self.target, self.i = _Arr(batches[0][0]), _Arr(batches[0][1]), 0

        def forward(self, **feeds):
            self.pred.a, self.target.a = batches[self.i]
            self.i += 1
            return losses[self.i - 1]

        def eval_pairs(self):
            return [('image', self.pred, self.target, 1.0)]

    data = types.SimpleNamespace(next=lambda: {})
    res = M().evaluate(data, 3)
    per = np.concatenate([metrics.image_metrics_host(p, t, 1.0) for p, t in batches])
    assert res['images'] == 6 and abs(res['loss'] - np.mean(losses)) <= 1e-15
    assert abs(res['image/l1'] - per[:, 0].mean()) <= 1e-15 and abs(res['image/ssim'] - per[:, 2].mean()) <= 1e-15
    assert abs(res['image/psnr'] - (10 * np.log10(1.0 / per[:, 1])).mean()) <= 1e-12
    with pytest.raises(NotImplementedError):
        ModelBase.eval_pairs(M())


def test_eval_pairs_of_the_model_classes(lib):
    """Each class names its pairs from the tensors its graph built; the mv3d colour / fourth-channel pairs are channel views."""
    from dynamic_multiview_3d_amd import mv3d
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    m = AppearanceFlowModel({'batch_size': 2, 'learning_rate': 1e-4}, load_tfrec=False, device='cpu')
    assert m.eval_pairs() == [('image', m.gen, m.image1, 1.0)]
    m = Base_Prediction_Model({'batch_size': 2, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 1.0}, device='cpu')
    assert [(p[0], p[1].C, p[3]) for p in m.eval_pairs()] == [('image', 3, 1.0), ('depth', 1, 1.0)]
    m = mv3d.mv3d_nobg_nodm({'batch_size': 2}, device='cpu')
    assert m.eval_pairs() == [('image', m.gen, m.images2, 1.5)]
    for cls, fourth in ((mv3d.mv3d_nobg_dm, ('depth', 1.5)), (mv3d.mv3d_bg_nodm, ('mask', 1.0))):
        m = cls({'batch_size': 2}, device='cpu')
        n_tensors = len(m.graph.tensors)
        (n0, p0, t0, v0), (n1, p1, t1, v1) = m.eval_pairs()
        assert (n0, v0, n1, v1) == ('image', 1.5) + fourth
        assert (p0.C, p0.ld, t0.C, t0.ld, p1.C, p1.ld, t1.C, t1.ld) == (3, 4, 3, 4, 1, 4, 1, 4)
        assert p0.ptr == m.gen.ptr and p1.ptr == m.gen.ptr + 12 and t1.ptr == m.images2.ptr + 12
        assert len(m.graph.tensors) == n_tensors                        # views only: the compiled graph is not touched
