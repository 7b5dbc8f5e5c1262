"""mv3d_flow_consistency on the GPU, through the C ABI, against metrics.flow_consistency_host evaluated in float64 on the same fp32
inputs (tests/flow_consist_cases.py: both families at every shape).

Tolerance: for every case the numpy twin is also evaluated in float32, and the kernel may differ from the float64 result by at most
4 x the float32 twin's own deviation from the float64 twin on that case, for the weighted value, for both stats and for the
gradient (largest element error).  The factor covers what the float32 twin does not share with the kernel: the double sums and the
fixed-point scatter.  The gradient's floor is the header's fixed-point bound, H W 2^-(K+1) |k| with K = 62 - ceil(log2(H W)) and
k = weight / (N H W).  The count of valid pixels must be exact.  Every figure is printed before it is asserted.

The float32 twin's deviations, measured on the CPU (seed 7, eps 1e-3, weight 0.7), gradient (largest element) / value:
  smooth  2x8 2.5e-08 / 1.4e-08   2x20 7.7e-09 / 6.5e-08   6x33 2.5e-09 / 7.8e-09   4x72 4.1e-09 / 4.4e-09   2x128 4.3e-09 / 2.5e-09
  large   2x8 1.4e-08 / 2.3e-08   2x20 1.4e-08 / 3.4e-07   6x33 2.3e-09 / 8.0e-07   4x72 6.6e-10 / 5.3e-07   2x128 5.6e-10 / 9.0e-07

Shapes (tiles are 16 rows x 64 columns): below one tile; no multiple of 16; N/2 odd with an odd image size; across a 64-wide tile
edge; the model's own size; and channel-slice views with flow_ld 3 and grad_ld 4 (the scalar load and store paths)."""
import functools

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import flow_consist_cases as FC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
EPS, WEIGHT = 1e-3, 0.7
THREE = ['flow_consist_tile', 'flow_consist_scatter', 'flow_consist_final']
CASES = [(family, n, h) for n, h in FC.SHAPES for family in ('smooth', 'large')]


@functools.lru_cache(maxsize=None)
def _flow(family, n, h):
    f = (FC.smooth_case if family == 'smooth' else FC.large_case)(n, h, FC.SEED)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _reference(family, n, h, weight):
    """((loss, grad, value, share) in float64, the same in float32), computed once and shared; the arrays are read-only."""
    out = []
    for dtype in (np.float64, np.float32):
        l, g, v, s = metrics.flow_consistency_host(_flow(family, n, h), EPS, dtype, weight)
        g.setflags(write=False)
        out.append((float(l), g, float(v), float(s)))
    return tuple(out)


def _fixed_point_bound(n, h, weight):
    bits = int(np.ceil(np.log2(h * h)))
    return h * h * 2.0 ** -(62 - bits + 1) * abs(weight) / (n * h * h)


def _run(lib, tf, weight=WEIGHT, loss=None, stats=None, grad=None, accumulate=0, ws=None, want_loss=True, off=0, goff=0):
    """One call on the flow view [off, off + 2) of tf [N,H,H,ld]; grad (optional) is [N,H,H,grad_ld], view [goff, goff + 2)."""
    n, h, w, ld = tf.shape
    nb = int(lib.flow_consistency_workspace_bytes(n, h, w))
    assert nb >= n * h * w * (16 + 8) + 16 * n * -(-h // 16) * -(-w // 64)
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if loss is None and want_loss:
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib.flow_consistency(n, h, w, tf.data_ptr() + 4 * off, ld, EPS, weight, loss.data_ptr() if loss is not None else None,
                         stats.data_ptr() if stats is not None else None, grad.data_ptr() + 4 * goff if grad is not None else None,
                         grad.shape[3] if grad is not None else 2, accumulate, ws.data_ptr(), nb, stream())
    return loss


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _check_parity(label, family, n, h, got_l, got_stats, got_grad):
    (l64, g64, v64, s64), (l32, g32, v32, s32) = _reference(family, n, h, WEIGHT)
    figures = [('loss', got_l, l64, l32), ('C', float(got_stats[0]), v64, v32), ('valid', float(got_stats[1]), s64, s32)]
    for what, got, r64, r32 in figures:
        print('%-16s %-5s %.9g err %.2e float32 twin %.2e' % (label, what, r64, abs(got - r64), abs(r32 - r64)))
    err, gap = np.abs(got_grad.astype(np.float64) - g64).max(), np.abs(g32.astype(np.float64) - g64).max()
    floor = _fixed_point_bound(n, h, WEIGHT)
    print('%-16s grad  max %.3e err %.2e float32 twin %.2e fixed-point bound %.1e | != float32 twin: %d of %d'
          % (label, np.abs(g64).max(), err, gap, floor, int(np.count_nonzero(got_grad != g32)), g32.size))
    assert np.all(np.isfinite(got_grad)) and np.isfinite(got_l)
    for what, got, r64, r32 in figures:
        assert abs(got - r64) <= 4 * abs(r32 - r64), (label, what, got, r64, r32)
    assert err <= max(4 * gap, floor), (label, err, gap)
    count = int(round(s64 * n * h * h))
    assert got_stats[1] == np.float32(count / float(n * h * h)), (label, got_stats[1], count)       # the count is exact
    assert 0 < count < n * h * h


@pytest.mark.parametrize("family,n,h", CASES)
def test_parity_with_the_numpy_definition(family, n, h):
    lib = _lib.lib()
    tf = torch.from_numpy(_flow(family, n, h).copy()).to(DEV)
    grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
    only = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV)
    loss = _run(lib, tf, stats=stats, grad=grad)
    loss_only = _run(lib, tf)
    _run(lib, tf, grad=only, want_loss=False)
    torch.cuda.synchronize()
    assert np.array_equal(tf.cpu().numpy(), _flow(family, n, h))
    _check_parity('%s-%dx%d' % (family, n, h), family, n, h, float(loss.cpu()[0]), stats.cpu().numpy(), grad.cpu().numpy())
    # value only, gradient only and the combined call agree bit for bit
    assert _bits(loss)[0] == _bits(loss_only)[0]
    assert np.array_equal(_bits(grad), _bits(only))


def test_channel_slice_views_and_the_torch_mirror():
    """flow = channels 1..2 of a 3-channel tensor (flow_ld 3), gradient = channels 1..2 of a 4-channel buffer (grad_ld 4): the
    scalar load and store paths; every channel outside the views keeps its bits."""
    family, n, h = 'smooth', 2, 20
    f3 = np.full((n, h, h, 3), SENTINEL, np.float32)
    f3[..., 1:3] = _flow(family, n, h)
    tf = torch.from_numpy(f3).to(DEV)
    grad = torch.full((n, h, h, 4), SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.zeros(2, dtype=torch.float32, device=DEV)
    loss = metrics.flow_consistency(tf[..., 1:3], EPS, WEIGHT, grad=grad[..., 1:3], stats=stats)
    assert loss.shape == () and loss.device.type == 'cuda'
    got = grad.cpu().numpy()
    assert np.all(got[..., 0] == SENTINEL) and np.all(got[..., 3] == SENTINEL) and np.array_equal(tf.cpu().numpy(), f3)
    _check_parity('views-2x20', family, n, h, float(loss), stats.cpu().numpy(), got[..., 1:3])
    # the dense call computes the same bits
    dense = torch.from_numpy(_flow(family, n, h).copy()).to(DEV)
    dgrad = torch.empty(dense.shape, dtype=torch.float32, device=DEV)
    dloss = _run(_lib.lib(), dense, grad=dgrad)
    torch.cuda.synchronize()
    assert _bits(dloss)[0] == _bits(loss.reshape(1))[0] and np.array_equal(_bits(dgrad), got[..., 1:3].copy().view(np.uint32))
    metrics.flow_consistency(tf[..., 1:3], EPS, WEIGHT, grad=grad[..., 1:3], accumulate=True)
    assert np.array_equal(grad.cpu().numpy()[..., 1:3], got[..., 1:3] + got[..., 1:3])
    with pytest.raises(ValueError, match='grad'):
        metrics.flow_consistency(tf[..., 1:3], grad=grad[:, :-1, :, 1:3])
    with pytest.raises(ValueError, match='stats'):
        metrics.flow_consistency(tf[..., 1:3], stats=torch.zeros(3, device=DEV))


def test_integer_inverse_flows_give_exactly_zero():
    """flow[n] = (a, b) against flow[m] = (-b, -a): value, gathered and scattered gradient are exactly 0, over several tiles."""
    lib = _lib.lib()
    n, h, a, b = 4, 72, 3.0, -2.0
    f = np.zeros((n, h, h, 2), np.float32)
    f[0], f[2] = (a, b), (-b, -a)
    f[1], f[3] = (-5.0, 1.0), (-1.0, 5.0)
    tf = torch.from_numpy(f).to(DEV)
    grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV)
    loss = _run(lib, tf, weight=2.0, stats=stats, grad=grad)
    base = torch.from_numpy(np.random.default_rng(5).normal(0, 1e-3, f.shape).astype(np.float32)).to(DEV)
    accum = base.clone()
    _run(lib, tf, weight=2.0, grad=accum, accumulate=1, want_loss=False)
    torch.cuda.synchronize()
    _, _, value, share = metrics.flow_consistency_host(f, EPS, np.float64, 2.0)
    assert float(value) == 0.0 and 0.5 < float(share) < 1.0
    got = stats.cpu().numpy()
    assert loss.cpu().numpy()[0] == 0.0 and got[0] == 0.0 and got[1] == np.float32(share)
    assert not np.any(grad.cpu().numpy())                                # stored zeros over the sentinel, in both halves of the batch
    assert np.array_equal(_bits(accum), _bits(base))                     # adding exactly 0 changes no bit


def test_a_non_finite_partner_value_gives_what_the_twin_gives():
    """NaN and inf in the partner flow: NaN in the value and in the gathered gradient of the pixels that sample them, nothing
    non-finite scattered; the same elements as in the float32 twin, and the finite ones by the parity rule's 4 x."""
    lib = _lib.lib()
    f = _flow('smooth', 2, 20).copy()
    f[1, 5, 7, 0], f[1, 12, 3, 1], f[0, 9, 9, 1] = np.nan, np.inf, np.nan
    tf = torch.from_numpy(f).to(DEV)
    grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
    loss = _run(lib, tf, grad=grad)
    torch.cuda.synchronize()
    with np.errstate(invalid='ignore'):
        _, g64, _, _ = metrics.flow_consistency_host(f, EPS, np.float64, WEIGHT)
        l32, g32, _, _ = metrics.flow_consistency_host(f, EPS, np.float32, WEIGHT)
    got = grad.cpu().numpy()
    assert np.isnan(loss.cpu().numpy()[0]) and np.isnan(l32)
    assert np.array_equal(np.isnan(got), np.isnan(g32)) and np.array_equal(np.isnan(got), np.isnan(g64)) and not np.isinf(got).any()
    ok = ~np.isnan(got)
    assert 0 < np.count_nonzero(~ok) < 40
    err, gap = np.abs(got[ok] - g64[ok]).max(), np.abs(g32[ok] - g64[ok]).max()
    print('non-finite partner: %d NaN elements, finite ones err %.2e float32 twin %.2e' % (np.count_nonzero(~ok), err, gap))
    assert err <= max(4 * gap, _fixed_point_bound(2, 20, WEIGHT))


def test_loss_adds_by_default_and_stores_after_overwrite_next():
    lib = _lib.lib()
    tf = torch.from_numpy(_flow('smooth', 6, 33).copy()).to(DEV)
    term = _run(lib, tf, weight=0.25)
    acc = torch.full((1,), 3.5, dtype=torch.float32, device=DEV)
    _run(lib, tf, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    t = np.float32(term.cpu().numpy()[0])
    assert t > 0 and acc.cpu().numpy()[0] == np.float32(3.5) + t          # one fp32 addition onto what was there
    lib.loss_overwrite_next()
    grad = torch.empty(tf.shape, dtype=torch.float32, device=DEV)
    _run(lib, tf, weight=0.25, grad=grad, want_loss=False)               # a gradient-only call is no loss entry: the flag stays
    _run(lib, tf, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t                                      # stored
    _run(lib, tf, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t + t                                  # the flag was consumed: this call adds again
    # the flag is one flag for every loss entry point: a pixel loss consumes it just the same
    lib.loss_overwrite_next()
    lib.pixel_loss_strided(tf.numel() // 2, 2, tf.data_ptr(), 2, tf.data_ptr(), 2, 1.0, None, 1, 2, 1.0, acc.data_ptr(), None, 2, stream())
    _run(lib, tf, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == np.float32(0.0) + t


def test_grad_accumulate_adds_onto_what_is_there_bit_for_bit():
    """Onto random contents: contents + the stored gradient, one fp32 addition per element; onto zeros: the stored gradient."""
    lib = _lib.lib()
    for family, n, h in (('large', 4, 72), ('smooth', 6, 33), ('smooth', 2, 8)):
        tf = torch.from_numpy(_flow(family, n, h).copy()).to(DEV)
        stored = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
        _run(lib, tf, weight=0.5, grad=stored, want_loss=False)
        onto_zero = torch.zeros(tf.shape, dtype=torch.float32, device=DEV)
        _run(lib, tf, weight=0.5, grad=onto_zero, accumulate=1, want_loss=False)
        base = torch.from_numpy(np.random.default_rng(4).normal(0, 1e-4, tuple(tf.shape)).astype(np.float32)).to(DEV)
        accum = base.clone()
        _run(lib, tf, weight=0.5, grad=accum, accumulate=1, want_loss=False)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(onto_zero), _bits(stored)), (family, n, h)
        want = base.cpu().numpy() + stored.cpu().numpy()                  # one fp32 addition per element
        assert np.array_equal(accum.cpu().numpy().view(np.uint32), want.view(np.uint32)), (family, n, h)


def test_two_runs_and_a_replayed_plan_give_the_same_bits():
    lib = _lib.lib()
    tf = torch.from_numpy(_flow('large', 4, 72).copy()).to(DEV)
    n, h, w, _ = tf.shape
    nb = int(lib.flow_consistency_workspace_bytes(n, h, w))
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    losses = [torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    stats = [torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    grads = [torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    for l, s, g in zip(losses[:2], stats[:2], grads[:2]):
        lib.loss_overwrite_next()
        _run(lib, tf, loss=l, stats=s, grad=g, ws=ws)
        ws.fill_(255)                                                       # no state survives in the workspace between calls
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        lib.loss_overwrite_next()                                           # a recorded call keeps the flag it saw
        lib.flow_consistency(n, h, w, tf.data_ptr(), 2, EPS, WEIGHT, losses[2].data_ptr(), stats[2].data_ptr(), grads[2].data_ptr(), 2, 0,
                             ws.data_ptr(), nb, None)
    finally:
        lib.plan_end()
    assert [o[0] for o in _lib.plan_ops(plan)] == THREE
    torch.cuda.synchronize()
    assert losses[2].cpu().numpy()[0] == SENTINEL and np.all(grads[2].cpu().numpy() == SENTINEL)      # recording launches nothing
    for _ in range(2):                                                      # replayed twice: it stores both times
        lib.plan_run(plan, stream())
    torch.cuda.synchronize()
    lib.plan_destroy(plan)
    lb, sb, gb = [_bits(l)[0] for l in losses], [_bits(s) for s in stats], [_bits(g) for g in grads]
    assert lb[0] == lb[1] == lb[2]
    assert np.array_equal(sb[0], sb[1]) and np.array_equal(sb[0], sb[2])
    assert np.array_equal(gb[0], gb[1]) and np.array_equal(gb[0], gb[2])
    assert not np.any(grads[0].cpu().numpy() == SENTINEL)


def test_argument_errors_leave_loss_stats_and_grad_untouched():
    lib = _lib.lib()
    n, h = 2, 20
    tf = torch.from_numpy(_flow('smooth', n, h).copy()).to(DEV)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV)
    grad = torch.full((n, h, h, 2), SENTINEL, dtype=torch.float32, device=DEV)
    nb = int(lib.flow_consistency_workspace_bytes(n, h, h))
    ws = torch.empty(nb + 64, dtype=torch.uint8, device=DEV)
    ok = dict(N=n, H=h, W=h, flow=tf.data_ptr(), flow_ld=2, eps=EPS, weight=1.0, loss=loss.data_ptr(), stats=stats.data_ptr(),
              grad=grad.data_ptr(), grad_ld=2, acc=0, ws=ws.data_ptr(), ws_bytes=nb)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_flow_consistency(v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['eps'], v['weight'], v['loss'], v['stats'],
                                        v['grad'], v['grad_ld'], v['acc'], v['ws'], v['ws_bytes'], stream())
    nan = float('nan')
    lib.loss_overwrite_next()                                  # stays pending through every refusal
    for kw, code, word in [(dict(N=1), -1, 'N'), (dict(N=3), -1, 'N'), (dict(W=h + 1), -1, 'differ'), (dict(H=1, W=1), -1, 'H'),
                           (dict(flow_ld=1), -1, 'flow_ld'), (dict(grad_ld=1), -1, 'grad_ld'), (dict(acc=2), -1, 'grad_accumulate'),
                           (dict(eps=0.0), -1, 'eps'), (dict(eps=nan), -1, 'eps'), (dict(weight=nan), -1, 'weight'),
                           (dict(flow=None), -1, 'flow is null'), (dict(loss=None, stats=None, grad=None), -1, 'both null'),
                           (dict(loss=None), -1, 'stats without'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(grad=grad.data_ptr() + 2), -1, 'aligned'), (dict(ws_bytes=nb - 1), -3, 'workspace'),
                           (dict(ws=ws.data_ptr() + 8), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    torch.cuda.synchronize()
    assert loss.cpu().numpy()[0] == SENTINEL and np.all(stats.cpu().numpy() == SENTINEL) and np.all(grad.cpu().numpy() == SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    got = loss.cpu().numpy()[0]
    assert 0 < got < 10.0 and not np.any(grad.cpu().numpy() == SENTINEL)          # stored over the sentinel: the flag was still pending
    assert got == stats.cpu().numpy()[0]                                          # weight 1: the loss word holds C itself
