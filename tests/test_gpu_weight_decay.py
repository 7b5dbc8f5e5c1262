"""Decoupled weight decay on the MI355X: mv3d_weight_decay_step, alone and with the EMA fused behind it, bit-exact against the
numpy twin over every table shape the kernel's range lookup can meet, and mv3d_opt_set_lr."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from dynamic_multiview_3d_amd.model_base import ema_one_minus_decay, ema_rule, weight_decay_rule
from tests.gpu_utils import stream
from tests.test_gpu_ema import GUARD, _values

pytestmark = pytest.mark.gpu

# hi - lo.  (1 << 24) + 8: two sweeps of the launch's 2048 workgroups x 4 x 256 lanes x 16 B (2^23 floats per sweep) plus a
# partial chunk, as COUNTS of tests/test_gpu_ema.py; 3 * 4096 + 12: whole chunks and a partial one; 4100: one chunk and a float4
SPANS = [4, 8, 4100, 3 * 4096 + 12, (1 << 24) + 8]
LO = 4096 + 64          # the span starts inside the buffer, off the chunk grid of absolute indices
TAIL = 192              # floats of the buffer behind hi (and then the guard words)
FS = [np.float32(0.0), np.float32(1e-4 * 0.01), np.float32(0.5)]


def L():
    return _lib.lib()


def _table(kind, lo, hi):
    if kind == 'all':                       # one range over everything
        return [(0, -(-(hi + TAIL) // 4) * 4)]
    if kind == 'none':                      # no range inside [lo, hi)
        return [(0, 64), (lo - 8, lo), (-(-hi // 4) * 4, -(-hi // 4) * 4 + 64)]
    if kind == 'rotating':                  # 21 ranges: bounds inside chunks and inside one wave
        out, at = [], lo + 4
        for i in range(21):
            n = (4, 60, 1028, 4100)[i % 4]
            out.append((at, at + n))
            at += n + (4, 68)[i % 2]
        return out
    if kind == 'straddle':                  # starts before lo, ends after hi
        return [(lo - 32, -(-hi // 4) * 4 + 32)]
    if kind == 'dense':                     # the cap: 1024 ranges of 4 floats, 4 apart
        return [(lo + 8 * i, lo + 8 * i + 4) for i in range(_lib.DECAY_MAX_RANGES)]
    raise KeyError(kind)


TABLES = ['all', 'none', 'rotating', 'straddle', 'dense']
_cache = {}


def _data(n):
    """(params, shadows, guard words) for a buffer of n floats: made once per size."""
    if n not in _cache:
        _cache.clear()
        rng = np.random.default_rng(n)
        _cache[n] = (_values(rng, n), _values(rng, n), rng.integers(0, 2 ** 31, GUARD).astype(np.int32))
    return _cache[n]


def _upload(x, guard):
    buf = torch.empty(x.size + GUARD, dtype=torch.float32, device='cuda')
    buf[:x.size].copy_(torch.from_numpy(x))
    buf[x.size:].view(torch.int32).copy_(torch.from_numpy(guard))
    return buf


def _same(buf, x, guard):
    want = _upload(x, guard)
    return bool(torch.equal(buf.view(torch.int32), want.view(torch.int32)))


def _twin(p, s, lo, hi, ranges, f, w, fused):
    """The rule over [lo, hi) of whole buffers: ranges clipped to the span, the EMA (fused form) over every element of it."""
    clipped = [(max(a, lo), min(b, hi)) for a, b in ranges if min(b, hi) > max(a, lo)]
    p2 = weight_decay_rule(p, clipped, f)
    s2 = s.copy()
    if fused:
        s2[lo:hi] = ema_rule(s[lo:hi], p2[lo:hi], w)
    return p2, s2, clipped


def _run_case(lo, hi, ranges, n):
    p, s, guard = _data(n)
    table = torch.tensor(ranges, dtype=torch.int64, device='cuda').reshape(-1)
    w = ema_one_minus_decay(0.9)
    for fused in (False, True):
        for f in FS:
            dp, ds = _upload(p, guard), _upload(s, guard)
            L().weight_decay_step(dp.data_ptr(), ds.data_ptr() if fused else None, lo, hi, table.data_ptr(), len(ranges), float(f),
                                  float(w) if fused else 0.0, stream())
            torch.cuda.synchronize()
            p2, s2, clipped = _twin(p, s, lo, hi, ranges, f, w, fused)
            assert _same(dp, p2, guard), (lo, hi, fused, float(f))          # the span, the rest of the buffer and the guard words
            assert _same(ds, s2, guard), (lo, hi, fused, float(f))          # shadow == NULL: the companion buffer is untouched
            if f > 0 and clipped:
                assert not np.array_equal(p2, p)                            # the case decays something
            if not clipped or f == 0:
                assert p2.tobytes() == p.tobytes()                          # no range inside the span, or f = 0: all bits untouched
            if fused:
                assert not np.array_equal(s2[lo:hi], s[lo:hi])
            del dp, ds


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("span", SPANS)
def test_weight_decay_step_bit_exact_vs_numpy(span, table):
    lo, hi = LO, LO + span
    _run_case(lo, hi, _table(table, lo, hi), hi + TAIL)


@pytest.mark.parametrize("table", ['all', 'rotating', 'none'])
@pytest.mark.parametrize("span", [5, 4099, 3 * 4096 + 14])
def test_fused_form_takes_the_unaligned_end_of_the_buffers(span, table):
    """hi is the end of the buffers and no multiple of 4: the scalar tail decays where its float4's range says so (a range's padded
    end lies past hi) and its shadows move; the guard words behind the buffers keep their bits."""
    lo, hi = LO, LO + span
    p, s, guard = _data(hi)
    ranges = _table(table, lo, hi)
    table_dev = torch.tensor(ranges, dtype=torch.int64, device='cuda').reshape(-1)
    w = ema_one_minus_decay(0.5)
    for f in FS:
        dp, ds = _upload(p, guard), _upload(s, guard)
        L().weight_decay_step(dp.data_ptr(), ds.data_ptr(), lo, hi, table_dev.data_ptr(), len(ranges), float(f), float(w), stream())
        torch.cuda.synchronize()
        p2, s2, _ = _twin(p, s, lo, hi, ranges, f, w, True)
        assert _same(dp, p2, guard) and _same(ds, s2, guard), (span, table, float(f))
        assert not np.array_equal(s2[hi - (span & 3):hi], s[hi - (span & 3):hi])
    assert L().raw_weight_decay_step(dp.data_ptr(), None, lo, hi, table_dev.data_ptr(), len(ranges), 0.5, 0.0, stream()) == -1


def test_opt_set_lr_writes_float_0_of_the_chosen_record():
    rng = np.random.default_rng(1)
    init = rng.standard_normal(16).astype(np.float32)
    state = torch.from_numpy(init).cuda()
    want = init.copy()
    for rec, lr in ((0, np.float32(3e-4)), (1, np.float32(7.5e-6)), (0, np.float32(0.0))):
        L().opt_set_lr(state.data_ptr() + 32 * rec, float(lr), stream())
        torch.cuda.synchronize()
        want[8 * rec] = lr
        assert state.cpu().numpy().tobytes() == want.tobytes(), (rec, float(lr))     # the other 15 floats keep their bits
