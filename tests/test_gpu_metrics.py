"""mv3d_image_metrics on the GPU, through the C ABI, against metrics.image_metrics_host evaluated in float64 on the same fp32 inputs.

Tolerance: for every case the numpy restatement is also evaluated in float32, and the kernel may differ from the float64 value
by at most 4 x the float32-to-float64 gap of that restatement on the same inputs (the kernel's arithmetic is the same fp32, its
sum order differs), with a floor of 2e-6 absolute for SSIM (16 fp32 ulps at 1.0) and 2e-6 relative for the L1 and MSE means.
Every figure is printed before it is asserted.

Inputs: the car-like synthetic renders of train.SyntheticData._images at noise 0 and 2, a copy shifted by one pixel, a
uniform-random pair, and a == b (SSIM from about 0.003 to exactly 1)."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from dynamic_multiview_3d_amd.train import SyntheticData
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
SHAPES = {'a': (64, 128, 128, 3), 'b': (2, 256, 256, 3), 'c': (64, 128, 128, 4), 'd': (3, 40, 23, 1), 'e': (1, 11, 11, 2),
          'f': (2, 45, 77, 3)}
FAMILIES = ('noise', 'shift', 'random', 'same')


def _render_clean(rng, shape):
    """SyntheticData._images without its noise term (noise 0): the same ellipse on the same grey, quantised to uint8 / 255."""
    b, h, w, c = shape
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.full(shape, 127.0, np.float32)
    for i in range(b):
        cy, cx = rng.uniform(0.3 * h, 0.7 * h, 2)
        ay, ax = rng.uniform(0.12 * h, 0.35 * h, 2)
        img[i][((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1] = rng.uniform(0, 255, c)
    return np.clip(np.rint(img), 0, 255) / 255.0


def _pair(family, shape, seed):
    """(a, b) float32 in [0, 1]."""
    if family == 'noise':                  # the same scene without noise and with the renders' noise of 2 grey levels
        clean = _render_clean(np.random.default_rng(seed), shape)
        noisy = SyntheticData._images(np.random.default_rng(seed), shape)
        return clean.astype(np.float32), noisy.astype(np.float32)
    if family == 'shift':
        a = SyntheticData._images(np.random.default_rng(seed), shape).astype(np.float32)
        return a, np.roll(a, 1, axis=2)
    if family == 'random':
        rng = np.random.default_rng(seed)
        return rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32)
    a = SyntheticData._images(np.random.default_rng(seed), shape).astype(np.float32)
    return a, a.copy()


def _device_metrics(lib, a, b, max_val, views):
    """Upload a, b [N,H,W,ld] once; per (channel offset, C) view run the kernel.  Returns [view][N,3] float32."""
    n, h, w, ld = a.shape
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    outs = []
    for off, c in views:
        nb = int(lib.image_metrics_workspace_bytes(n, h, w, c))
        assert nb >= n * 24
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        out = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=DEV)
        lib.image_metrics(n, h, w, c, ta.data_ptr() + 4 * off, ld, tb.data_ptr() + 4 * off, ld, max_val, out.data_ptr(), ws.data_ptr(), nb, stream())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return outs


def check_against_host(got, a, b, max_val, label):
    """The tolerance rule of the module docstring on one [N,3] result; returns (kernel error, float32 gap) maxima per column."""
    h64 = metrics.image_metrics_host(a, b, max_val, np.float64)
    h32 = metrics.image_metrics_host(a, b, max_val, np.float32).astype(np.float64)
    gap = np.abs(h32 - h64)
    err = np.abs(got.astype(np.float64) - h64)
    floor = np.stack([2e-6 * np.abs(h64[:, 0]), 2e-6 * np.abs(h64[:, 1]), np.full(len(h64), 2e-6)], axis=1)
    allowed = np.maximum(4 * gap, floor)
    print('%-34s ssim %.6f..%.6f | kernel err l1 %.2e mse %.2e ssim %.2e | float32 gap l1 %.2e mse %.2e ssim %.2e'
          % (label, h64[:, 2].min(), h64[:, 2].max(), err[:, 0].max(), err[:, 1].max(), err[:, 2].max(),
             gap[:, 0].max(), gap[:, 1].max(), gap[:, 2].max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= allowed), (label, err.max(axis=0), allowed.min(axis=0), np.argwhere(err > allowed)[:4])
    return err.max(axis=0), gap.max(axis=0)


@pytest.mark.parametrize("max_val", [1.0, 1.5])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_parity_with_the_numpy_definition(case, family, max_val):
    lib = _lib.lib()
    shape = SHAPES[case]
    a, b = _pair(family, shape, seed=sum(map(ord, case + family)))
    if max_val == 1.5:                                        # the mv3d range: (x - 0.5) * 1.5 in [-0.75, 0.75]
        a, b = ((a - np.float32(0.5)) * np.float32(1.5)).astype(np.float32), ((b - np.float32(0.5)) * np.float32(1.5)).astype(np.float32)
    views = [(0, 3), (3, 1)] if case == 'c' else [(0, shape[3])]        # c: colour view C=3 ld=4 and the channel-3 view C=1 ld=4
    outs = _device_metrics(lib, a, b, max_val, views)
    for (off, c), got in zip(views, outs):
        sa, sb = a[..., off:off + c], b[..., off:off + c]
        if family == 'same':
            assert np.all(got[:, metrics.SSIM] == 1.0) and np.all(got[:, metrics.L1] == 0.0) and np.all(got[:, metrics.MSE] == 0.0)
        check_against_host(got, sa, sb, max_val, '%s %s max_val %.1f ch %d+%d' % (case, family, max_val, off, c))


def test_ssim_spans_the_range():
    """The input families cover what the parity test claims: from nearly unrelated to nearly equal."""
    shape = SHAPES['f']
    lo = metrics.image_metrics_host(*_pair('random', shape, 1), 1.0)[:, 2]
    hi = metrics.image_metrics_host(*_pair('noise', shape, 1), 1.0)[:, 2]
    assert lo.max() < 0.02 and hi.min() > 0.9, (lo, hi)


def test_two_runs_and_a_replayed_plan_give_the_same_bits():
    lib = _lib.lib()
    for case in ('a', 'f'):
        n, h, w, c = SHAPES[case]
        a, b = _pair('noise', SHAPES[case], 5)
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        nb = int(lib.image_metrics_workspace_bytes(n, h, w, c))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        outs = [torch.full((n, 3), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
        for o in outs[:2]:
            lib.image_metrics(n, h, w, c, ta.data_ptr(), c, tb.data_ptr(), c, 1.0, o.data_ptr(), ws.data_ptr(), nb, stream())
        plan = lib.plan_create()
        lib.plan_begin(plan)
        try:
            lib.image_metrics(n, h, w, c, ta.data_ptr(), c, tb.data_ptr(), c, 1.0, outs[2].data_ptr(), ws.data_ptr(), nb, None)
        finally:
            lib.plan_end()
        assert [o[0] for o in _lib.plan_ops(plan)] == ['image_metrics_tile', 'image_metrics_final']
        torch.cuda.synchronize()
        assert np.all(outs[2].cpu().numpy() == SENTINEL)                    # recording launches nothing
        ws.zero_()                                                          # no state survives in the workspace between calls
        lib.plan_run(plan, stream())
        torch.cuda.synchronize()
        lib.plan_destroy(plan)
        r = [o.cpu().numpy().view(np.uint32) for o in outs]
        assert np.array_equal(r[0], r[1]) and np.array_equal(r[0], r[2])


def test_host_mirror_takes_torch_tensors_and_channel_views():
    a, b = _pair('shift', SHAPES['c'], 9)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = metrics.image_metrics(ta[..., :3], tb[..., :3], 1.0)
    assert got.shape == (64, 3) and got.device.type == 'cuda'
    check_against_host(got.cpu().numpy(), a[..., :3], b[..., :3], 1.0, 'mirror colour view')
    out = torch.empty((64, 3), dtype=torch.float32, device=DEV)
    assert metrics.image_metrics(ta[..., 3:], tb[..., 3:], 1.0, out=out) is out
    check_against_host(out.cpu().numpy(), a[..., 3:], b[..., 3:], 1.0, 'mirror channel-3 view')
    with pytest.raises(ValueError, match='shape'):
        metrics.image_metrics(ta, tb[..., :3])
    with pytest.raises(ValueError, match='NHWC'):
        metrics.image_metrics(ta.permute(0, 2, 1, 3), tb.permute(0, 2, 1, 3))
    with pytest.raises(_lib.Mv3dError, match='max_val'):
        metrics.image_metrics(ta, tb, max_val=0.0)


def test_argument_errors_leave_out_untouched():
    lib = _lib.lib()
    n, h, w, c = 2, 16, 20, 3
    ta = torch.rand((n, h, w, c), device=DEV)
    tb = torch.rand((n, h, w, c), device=DEV)
    out = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=DEV)
    nb = int(lib.image_metrics_workspace_bytes(n, h, w, c))
    ws = torch.empty(nb + 64, dtype=torch.uint8, device=DEV)
    ok = dict(N=n, H=h, W=w, C=c, a=ta.data_ptr(), a_ld=c, b=tb.data_ptr(), b_ld=c, max_val=1.0, out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=nb)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_image_metrics(v['N'], v['H'], v['W'], v['C'], v['a'], v['a_ld'], v['b'], v['b_ld'], v['max_val'], v['out'],
                                     v['ws'], v['ws_bytes'], stream())
    for kw, code, word in [(dict(N=0), -1, 'N'), (dict(H=10), -1, 'H'), (dict(W=10), -1, 'W'), (dict(C=5), -1, 'C'), (dict(C=0), -1, 'C'),
                           (dict(a_ld=2), -1, 'a_ld'), (dict(b_ld=2), -1, 'b_ld'), (dict(max_val=0.0), -1, 'max_val'),
                           (dict(max_val=float('inf')), -1, 'max_val'), (dict(max_val=float('nan')), -1, 'max_val'),
                           (dict(a=None), -1, 'a is null'), (dict(b=None), -1, 'b is null'), (dict(out=None), -1, 'out is null'),
                           (dict(ws=None), -1, 'workspace is null'), (dict(H=32769), -1, 'H'),
                           (dict(N=1 << 21, H=32768, W=32768), -1, 'tiles'),
                           (dict(ws_bytes=nb - 1), -3, 'workspace'), (dict(ws=ws.data_ptr() + 8), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() != SENTINEL)
