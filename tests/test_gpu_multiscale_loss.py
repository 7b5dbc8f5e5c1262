"""mv3d_multiscale_warp_loss on the GPU, through the C ABI, against metrics.multiscale_warp_loss_host evaluated in float64 on the
same fp32 inputs.

Tolerance (the rule of tests/test_gpu_flow_smooth.py, stated in tests/multiscale_cases.within_rule): the kernel may differ from
the float64 result by at most 4 x the float32-twin-to-float64 gap on the same inputs, with floors of 2e-6 absolute for the value
and 2e-6 of the float64 gradient's L2 norm / largest magnitude for the gradient's L2 / max-abs error; whatever the gap says, the
gradient's relative L2 error may not exceed 1e-3.  Every figure is printed before it is asserted.  Shapes and flow families:
tests/multiscale_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import multiscale_cases as MC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25


def _weights(w):
    return (ctypes.c_float * len(w))(*w)


def _operands(case, family, c):
    """(src, flow, target, flow channel offset) on the device.  'views' keeps 4-channel tensors with sentinels around the views;
    every other case gets dense copies (so the vector paths run there and the scalar ones in 'views')."""
    src, tgt = MC.images(case)
    fl = MC.flow(case, family)
    if case == 'views':
        s4, t4 = np.full(src.shape, SENTINEL, np.float32), np.full(tgt.shape, SENTINEL, np.float32)
        s4[..., :c], t4[..., :c] = src[..., :c], tgt[..., :c]
        f4 = np.full(fl.shape[:3] + (4,), SENTINEL, np.float32)
        f4[..., 1:3] = fl
        return torch.from_numpy(s4).to(DEV), torch.from_numpy(f4).to(DEV), torch.from_numpy(t4).to(DEV), 1
    return (torch.from_numpy(src[..., :c].copy()).to(DEV), torch.from_numpy(fl.copy()).to(DEV), torch.from_numpy(tgt[..., :c].copy()).to(DEV), 0)


def _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=None, lv=None, grad=None, accumulate=0, ready=0, ws=None, want_loss=True):
    """One call on the views [0, c) of ts / tt and [off, off + 2) of tf; grad (optional) has tf's layout."""
    n, h, wd, _ = tf.shape
    hs, wsd = ts.shape[1:3]
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, wd, hs, wsd, c, levels))
    assert nb > 0
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if loss is None and want_loss:
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib.multiscale_warp_loss(n, h, wd, hs, wsd, c, ts.data_ptr(), ts.shape[3], tf.data_ptr() + 4 * off, tf.shape[3], tt.data_ptr(), tt.shape[3],
                             levels, _weights(w), kind, loss.data_ptr() if loss is not None else None,
                             lv.data_ptr() if lv is not None else None, grad.data_ptr() + 4 * off if grad is not None else None,
                             tf.shape[3], accumulate, ready, ws.data_ptr(), nb, stream())
    return loss


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("case", sorted(MC.SHAPES))
def test_parity_with_the_numpy_definition(case, family):
    lib = _lib.lib()
    levels, w = MC.dims(case)[3], MC.weights(case)
    for c in MC.channels_of(case):
        for kind in MC.KINDS:
            ts, tf, tt, off = _operands(case, family, c)
            before = [t.cpu().numpy() for t in (ts, tf, tt)]
            grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
            only = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
            ready = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
            lv = torch.full((levels,), SENTINEL, dtype=torch.float32, device=DEV)
            n, h, wd, _ = tf.shape
            ws = torch.empty(int(lib.multiscale_warp_loss_workspace_bytes(n, h, wd, ts.shape[1], ts.shape[2], c, levels)), dtype=torch.uint8, device=DEV)
            loss = _run(lib, ts, tf, tt, off, c, levels, w, kind, lv=lv, grad=grad)
            _run(lib, ts, tf, tt, off, c, levels, w, kind, grad=only, want_loss=False)
            loss_only = _run(lib, ts, tf, tt, off, c, levels, w, kind, ws=ws)                            # leaves the pyramids in ws
            _run(lib, ts, tf, tt, off, c, levels, w, kind, grad=ready, ready=1, ws=ws, want_loss=False)  # ... which this call uses
            torch.cuda.synchronize()
            label = '%s %s C %d kind %d' % (case, family, c, kind)
            got_full = grad.cpu().numpy()
            outside = np.ones(tf.shape[3], bool)
            outside[off:off + 2] = False
            assert np.all(got_full[..., outside] == SENTINEL), label                    # channels outside the view are untouched
            for t, b in zip((ts, tf, tt), before):
                assert np.array_equal(t.cpu().numpy(), b), label                          # ... and so are the operands and their sentinels
            got32 = got_full[..., off:off + 2]
            ref = MC.reference(case, family, c, kind)
            MC.within_rule(label, float(loss.cpu()[0]), got32, ref)
            print('    != float32 twin: %d of %d gradient elements' % (int(np.count_nonzero(got32 != ref[4])), got32.size))
            # the unweighted T_l
            got_lv = lv.cpu().numpy().astype(np.float64)
            lv_gap = np.abs(ref[5].astype(np.float64) - ref[2])
            print('    T_l %s err %s gap %s' % (ref[2], np.abs(got_lv - ref[2]), lv_gap))
            assert np.all(np.abs(got_lv - ref[2]) <= np.maximum(4 * lv_gap, 2e-6)), label
            # value only, gradient only, gradient from ready pyramids and the combined call agree bit for bit
            assert _bits(loss)[0] == _bits(loss_only)[0], label
            assert np.array_equal(_bits(grad), _bits(only)), label
            assert np.array_equal(_bits(grad), _bits(ready)), label


def test_zero_flow_on_a_transposed_pair_is_exactly_zero():
    lib = _lib.lib()
    for side, levels in ((8, 3), (96, 2)):
        a, b = MC.transposed_pair(side)
        ts, tt = torch.from_numpy(a.copy()).to(DEV), torch.from_numpy(b.copy()).to(DEV)
        tf = torch.zeros((2, side, side, 2), dtype=torch.float32, device=DEV)
        for kind in MC.KINDS:
            grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
            lv = torch.full((levels,), SENTINEL, dtype=torch.float32, device=DEV)
            loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
            lib.loss_overwrite_next()
            _run(lib, ts, tf, tt, 0, 3, levels, [1.0] * levels, kind, loss=loss, lv=lv, grad=grad)
            torch.cuda.synchronize()
            assert loss.cpu().numpy()[0] == 0.0 and not np.any(lv.cpu().numpy()) and not np.any(grad.cpu().numpy()), (side, kind)


def test_loss_adds_by_default_and_stores_after_overwrite_next():
    lib = _lib.lib()
    case, c, kind = 'edge', 3, 2
    levels, w = MC.dims(case)[3], MC.weights(case)
    ts, tf, tt, off = _operands(case, 'smooth', c)
    term = _run(lib, ts, tf, tt, off, c, levels, w, kind)
    acc = torch.full((1,), 3.5, dtype=torch.float32, device=DEV)
    _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=acc)
    torch.cuda.synchronize()
    t = np.float32(term.cpu().numpy()[0])
    assert t > 0 and acc.cpu().numpy()[0] == np.float32(3.5) + t                       # one fp32 addition onto what was there
    lib.loss_overwrite_next()
    grad = torch.empty(tf.shape, dtype=torch.float32, device=DEV)
    _run(lib, ts, tf, tt, off, c, levels, w, kind, grad=grad, want_loss=False)       # a gradient-only call is no loss entry: the flag stays
    _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t                                                    # stored
    _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t + t                                                # the flag was consumed: this call adds again


def test_grad_accumulate_adds_onto_what_is_there_bit_for_bit():
    lib = _lib.lib()
    for case, c, kind in (('inner', 4, 2), ('views', 3, 1), ('edge', 1, 2)):
        levels, w = MC.dims(case)[3], MC.weights(case)
        ts, tf, tt, off = _operands(case, 'random', c)
        stored = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
        _run(lib, ts, tf, tt, off, c, levels, w, kind, grad=stored)
        base = torch.from_numpy(np.random.default_rng(4).normal(0, 1e-4, tuple(tf.shape)).astype(np.float32)).to(DEV)
        accum = base.clone()
        _run(lib, ts, tf, tt, off, c, levels, w, kind, grad=accum, accumulate=1)
        torch.cuda.synchronize()
        want = base.cpu().numpy().copy()
        want[..., off:off + 2] = want[..., off:off + 2] + stored.cpu().numpy()[..., off:off + 2]       # one fp32 addition per element
        assert np.array_equal(accum.cpu().numpy().view(np.uint32), want.view(np.uint32)), case


def test_two_runs_and_a_replayed_plan_give_the_same_bits():
    lib = _lib.lib()
    case, c, kind = 'inner', 3, 2
    levels, w = MC.dims(case)[3], MC.weights(case)
    ts, tf, tt, off = _operands(case, 'smooth', c)
    n, h, wd, _ = tf.shape
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, wd, h, wd, c, levels))
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    losses = [torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    grads = [torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    for l, g in zip(losses[:2], grads[:2]):
        lib.loss_overwrite_next()
        _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=l, grad=g, ws=ws)
        ws.zero_()                                                          # nothing a call needs survives in the workspace
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        lib.loss_overwrite_next()                                           # a recorded call keeps the flag it saw
        _run(lib, ts, tf, tt, off, c, levels, w, kind, loss=losses[2], grad=grads[2], ws=ws)
    finally:
        lib.plan_end()
    ops = _lib.plan_ops(plan)
    assert [o[0] for o in ops] == ['multiscale_pyramid', 'multiscale_loss_tile', 'multiscale_loss_final']
    px, pyr = n * h * wd, 2 * n * h * wd * (1 / 4 + 1 / 16)
    assert ops[0][2] == (2 * px + pyr) * 4 * c                              # src and target read once, the levels written once
    assert ops[1][2] == px * (8 + 8) + pyr * 4 * c + n * 9 * 24             # flow, gradient, the levels re-read, the tile sums
    torch.cuda.synchronize()
    assert losses[2].cpu().numpy()[0] == SENTINEL and np.all(grads[2].cpu().numpy() == SENTINEL)      # recording launches nothing
    for _ in range(2):                                                      # replayed twice: it stores both times
        lib.plan_run(plan, stream())
    torch.cuda.synchronize()
    lib.plan_destroy(plan)
    lb = [_bits(l)[0] for l in losses]
    gb = [_bits(g) for g in grads]
    assert lb[0] == lb[1] == lb[2]
    assert np.array_equal(gb[0], gb[1]) and np.array_equal(gb[0], gb[2])
    assert not np.any(grads[0].cpu().numpy() == SENTINEL)


def test_level_one_matches_the_existing_sampler_and_loss_kernel():
    """Level 1 on 'edge' against mv3d_warp_resample_loss run at the coarse size on operands pooled on the host with the
    hierarchical fp32 rule: the same value, and the coarse dflow repeated over 2 x 2 blocks and divided by 8."""
    lib = _lib.lib()
    case, c = 'edge', 3
    src, tgt = MC.images(case)
    fl = MC.flow(case, 'random')
    n, h, w = fl.shape[:3]
    ps, pt, pf = (metrics._pool2(x) for x in (src[..., :c], tgt[..., :c], fl))
    assert ps.dtype == np.float32
    for kind in MC.KINDS:
        tps, ptt = torch.from_numpy(ps.copy()).to(DEV), torch.from_numpy(pt.copy()).to(DEV)
        tpf = torch.from_numpy((pf * np.float32(0.5)).copy()).to(DEV)
        gen = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=DEV)
        dflow = torch.empty((n, h // 2, w // 2, 2), dtype=torch.float32, device=DEV)
        coarse = torch.zeros(1, dtype=torch.float32, device=DEV)
        lib.warp_resample_loss(n, h // 2, w // 2, h // 2, w // 2, c, tps.data_ptr(), tpf.data_ptr(), 2, ptt.data_ptr(), c, kind, 1.0,
                               None, gen.data_ptr(), dflow.data_ptr(), 2, coarse.data_ptr(), stream())
        ts, tf, tt, off = _operands(case, 'random', c)
        grad = torch.empty(tf.shape, dtype=torch.float32, device=DEV)
        loss = _run(lib, ts, tf, tt, off, c, 1, [1.0], kind, grad=grad)
        torch.cuda.synchronize()
        want_g = np.repeat(np.repeat(dflow.cpu().numpy().astype(np.float64), 2, axis=1), 2, axis=2) / 8.0
        ref = list(metrics.multiscale_warp_loss_host(src[..., :c], fl, tgt[..., :c], 1, [1.0], kind, np.float64))
        r32 = metrics.multiscale_warp_loss_host(src[..., :c], fl, tgt[..., :c], 1, [1.0], kind, np.float32)
        full = (float(ref[0]), ref[1], ref[2], float(r32[0]), r32[1], r32[2])
        MC.within_rule('new entry, kind %d' % kind, float(loss.cpu()[0]), grad.cpu().numpy(), full)
        MC.within_rule('existing kernel, kind %d' % kind, float(coarse.cpu()[0]), want_g, full)
        # ... and against each other: the existing kernel's result in the reference's place, the twin's gap around it
        both = (float(coarse.cpu()[0]), want_g, None, float(r32[0]) - float(ref[0]) + float(coarse.cpu()[0]),
                (want_g + (r32[1].astype(np.float64) - ref[1])).astype(np.float64), None)
        MC.within_rule('new against existing, kind %d' % kind, float(loss.cpu()[0]), grad.cpu().numpy(), both)


def test_host_mirror_takes_torch_tensors_and_channel_views():
    case, c, kind = 'views', 3, 2
    ts, tf, tt, off = _operands(case, 'random', c)
    grad = torch.full(tf.shape, SENTINEL, dtype=torch.float32, device=DEV)
    value, lv = metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, MC.weights(case), kind, grad=grad[..., 1:3])
    assert value.shape == () and lv.shape == (1,) and value.device.type == 'cuda'
    ref = MC.reference(case, 'random', c, kind)
    got = grad.cpu().numpy()
    MC.within_rule('mirror', float(value), got[..., 1:3], ref)
    assert np.all(got[..., 0] == SENTINEL) and np.all(got[..., 3] == SENTINEL)
    metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, MC.weights(case), kind, grad=grad[..., 1:3], accumulate=True)
    assert np.array_equal(grad.cpu().numpy()[..., 1:3], got[..., 1:3] + got[..., 1:3])
    with pytest.raises(ValueError, match='flow'):
        metrics.multiscale_warp_loss(ts[..., :c], tf, tt[..., :c], 1)
    with pytest.raises(ValueError, match='levels'):
        metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 4)
    with pytest.raises(ValueError, match='multiple'):
        z = torch.zeros((1, 12, 16, 3), device=DEV)                                      # 12 is no multiple of 8
        metrics.multiscale_warp_loss(z, z[..., :2].contiguous(), z, 3)
    with pytest.raises(ValueError, match='level_weights'):
        metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, [1.0, 2.0])
    with pytest.raises(ValueError, match='finite'):
        metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, [float('inf')])
    with pytest.raises(ValueError, match='kind'):
        metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, kind=0)
    with pytest.raises(ValueError, match='grad'):
        metrics.multiscale_warp_loss(ts[..., :c], tf[..., 1:3], tt[..., :c], 1, grad=grad[:, :-1, :, 1:3])


def test_argument_errors_leave_loss_and_grad_untouched():
    lib = _lib.lib()
    n, h, w, c, levels = 2, 16, 20, 3, 2
    ts, tt = torch.rand((n, h, w, c), device=DEV), torch.rand((n, h, w, c), device=DEV)
    tf = torch.rand((n, h, w, 2), device=DEV)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
    lv = torch.full((levels,), SENTINEL, dtype=torch.float32, device=DEV)
    grad = torch.full((n, h, w, 2), SENTINEL, dtype=torch.float32, device=DEV)
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, w, h, w, c, levels))
    assert lib.multiscale_warp_loss_workspace_bytes(n, h, w, h, w, c, 3) == 0          # 20 is no multiple of 8
    ws = torch.empty(nb + 64, dtype=torch.uint8, device=DEV)
    inf, nan = float('inf'), float('nan')
    ok = dict(N=n, H=h, W=w, Hs=h, Ws=w, C=c, src=ts.data_ptr(), src_ld=c, flow=tf.data_ptr(), flow_ld=2, target=tt.data_ptr(), target_ld=c,
              levels=levels, weights=_weights([1.0, 0.5]), kind=2, loss=loss.data_ptr(), lv=lv.data_ptr(), grad=grad.data_ptr(), grad_ld=2,
              acc=0, ready=0, ws=ws.data_ptr(), ws_bytes=nb)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_multiscale_warp_loss(v['N'], v['H'], v['W'], v['Hs'], v['Ws'], v['C'], v['src'], v['src_ld'], v['flow'], v['flow_ld'],
                                            v['target'], v['target_ld'], v['levels'], v['weights'], v['kind'], v['loss'], v['lv'], v['grad'],
                                            v['grad_ld'], v['acc'], v['ready'], v['ws'], v['ws_bytes'], stream())
    lib.loss_overwrite_next()                                  # stays pending through every refusal
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(C=0), -1, 'C'), (dict(C=5), -1, 'C'), (dict(levels=0), -1, 'levels'),
                           (dict(levels=4), -1, 'levels'), (dict(H=18), -1, 'H'), (dict(W=22), -1, 'W'), (dict(Hs=10), -1, 'Hs'),
                           (dict(Ws=0), -1, 'Ws'), (dict(levels=3), -1, 'W'), (dict(src_ld=2), -1, 'src_ld'), (dict(flow_ld=1), -1, 'flow_ld'),
                           (dict(target_ld=2), -1, 'target_ld'), (dict(grad_ld=1), -1, 'grad_ld'), (dict(kind=0), -1, 'kind'),
                           (dict(kind=3), -1, 'kind'), (dict(acc=2), -1, 'grad_accumulate'), (dict(ready=2), -1, 'pyramid_ready'),
                           (dict(src=None), -1, 'src is null'), (dict(flow=None), -1, 'flow is null'), (dict(target=None), -1, 'target is null'),
                           (dict(weights=None), -1, 'level_weights is null'), (dict(weights=_weights([1.0, nan])), -1, 'level_weights[1]'),
                           (dict(weights=_weights([inf, 1.0])), -1, 'level_weights[0]'), (dict(loss=None, lv=None, grad=None), -1, 'both null'),
                           (dict(loss=None), -1, 'level_values'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(grad=grad.data_ptr() + 2), -1, 'aligned'), (dict(ws_bytes=nb - 1), -3, 'workspace'),
                           (dict(ws=ws.data_ptr() + 8), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    torch.cuda.synchronize()
    assert loss.cpu().numpy()[0] == SENTINEL and np.all(grad.cpu().numpy() == SENTINEL) and np.all(lv.cpu().numpy() == SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    got = loss.cpu().numpy()[0]
    assert 0 < got < 10.0 and not np.any(grad.cpu().numpy() == SENTINEL)          # stored over the sentinel: the flag was still pending
    want = np.float32(np.float64(lv.cpu().numpy()[0]) * 1.0 + np.float64(lv.cpu().numpy()[1]) * 0.5)
    assert abs(got - want) <= 2e-6
