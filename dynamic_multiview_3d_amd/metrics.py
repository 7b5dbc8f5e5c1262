"""Per-image quality metrics of a prediction against its target: L1, MSE / PSNR and SSIM.

`image_metrics` is the host mirror of mv3d_image_metrics (include/mv3d_hip.h, csrc/metrics.hip): it runs on device memory and
returns a device tensor, so a test split can be scored without copying a prediction to the host.  `image_metrics_host` is the
numpy restatement of the same definition; `ModelBase.evaluate` uses it on a machine without a GPU.

Definition (per image n of [N,H,W,C] operands a, b):
  l1   = mean over the H*W pixels of sum_c |a-b|            -- the per-image form of l1_loss, mv3d/utils/tf_utils.py:22-23
  mse  = mean over the H*W*C elements of (a-b)^2;  psnr = 10 log10(max_val^2 / mse), inf when mse == 0
  ssim = Wang et al. 2004 in the form tf.image.ssim computes it.  F is the 11-tap Gaussian (sigma 1.5, normalised to sum 1)
         applied separably over fully-inside windows, so the map is (H-10) x (W-10) per channel; c1 = (0.01 max_val)^2,
         c2 = (0.03 max_val)^2, mx = F(a), my = F(b),
           lum = (2 mx my + c1) / (mx^2 + my^2 + c1)
           cs  = (2 F(a b) - 2 mx my + c2) / (F(a a + b b) - (mx^2 + my^2) + c2)
         ssim = mean of lum * cs over the windows and the channels.
"""
import math

import numpy as np

WINDOW_TAPS = 11
WINDOW_SIGMA = 1.5
K1, K2 = 0.01, 0.03
L1, MSE, SSIM = 0, 1, 2         # columns of the [N,3] result


def ssim_window(dtype=np.float64):
    """The 11 normalised Gaussian weights.  Computed in double with the C library's exp and an in-order sum -- the same steps as
    mv3d_image_metrics takes -- then rounded to `dtype` once."""
    g = [math.exp(-float((k - WINDOW_TAPS // 2) ** 2) / (2.0 * WINDOW_SIGMA * WINDOW_SIGMA)) for k in range(WINDOW_TAPS)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], np.float64).astype(dtype)


def _valid_filter(x, w):
    """F over [N,H,W,C]: horizontal pass, then vertical pass, taps added in index order (the kernel's order)."""
    taps = len(w)
    wo, ho = x.shape[2] - taps + 1, x.shape[1] - taps + 1
    h = w[0] * x[:, :, 0:wo]
    for k in range(1, taps):
        h = h + w[k] * x[:, :, k:k + wo]
    v = w[0] * h[:, 0:ho]
    for k in range(1, taps):
        v = v + w[k] * h[:, k:k + ho]
    return v


def _ssim_operands(a, b, max_val, dtype):
    """The operand checks of the SSIM functions: (a, b) in `dtype` and max_val as the float the C ABI takes."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    if a.shape != b.shape or a.ndim != 4:
        raise ValueError("ssim: operands must be [N,H,W,C] of one shape, got %s and %s" % (a.shape, b.shape))
    if a.shape[1] < WINDOW_TAPS or a.shape[2] < WINDOW_TAPS:
        raise ValueError("ssim: images of %d x %d are smaller than the %d-tap window" % (a.shape[1], a.shape[2], WINDOW_TAPS))
    max_val = float(np.float32(max_val))                     # the C ABI takes a float
    if not math.isfinite(max_val) or max_val <= 0:
        raise ValueError("ssim: max_val must be finite and positive")
    return a, b, max_val


def ssim_map(a, b, max_val, dtype=np.float64):
    """lum * cs at every fully-inside window: [N, H-10, W-10, C] in `dtype` arithmetic."""
    dtype = np.dtype(dtype).type
    a, b, max_val = _ssim_operands(a, b, max_val, dtype)
    return _ssim_parts(a, b, max_val, dtype)[-1]


def _ssim_parts(a, b, max_val, dtype):
    """(mx, my, A1, B1, A2, B2, lum, S = lum * cs) of the SSIM expression, each [N, H-10, W-10, C] in `dtype`."""
    k1, k2 = K1 * max_val, K2 * max_val
    c1, c2 = dtype(k1 * k1), dtype(k2 * k2)
    w = ssim_window(dtype)
    two = dtype(2)
    mx, my = _valid_filter(a, w), _valid_filter(b, w)
    sab = _valid_filter(a * b, w)
    s2 = _valid_filter(a * a + b * b, w)
    num0 = (mx * my) * two
    den0 = mx * mx + my * my
    A1, B1 = num0 + c1, den0 + c1
    A2, B2 = (sab * two - num0) + c2, (s2 - den0) + c2
    lum = A1 / B1
    cs = A2 / B2
    return mx, my, A1, B1, A2, B2, lum, lum * cs


def _transposed_filter(d, w):
    """Ft over [N,Hv,Wv,C]: the transpose of _valid_filter.  The window is symmetric, so it is the same pass (horizontal, then
    vertical, taps added in index order) over the map zero-padded by taps-1 on every side; the result is [N,Hv+10,Wv+10,C]."""
    pad = len(w) - 1
    n, hv, wv, c = d.shape
    p = np.zeros((n, hv + 2 * pad, wv + 2 * pad, c), d.dtype)
    p[:, pad:pad + hv, pad:pad + wv] = d
    return _valid_filter(p, w)


def _host_mask(op, mask, shape, dtype):
    """The mask of a masked image loss as [N,H,W] in `dtype`: [N,H,W,1] (or [N,H,W]) over the operands' N, H, W, finite."""
    m = np.asarray(mask)
    if m.ndim == 4 and m.shape[3] == 1:
        m = m[..., 0]
    if m.shape != tuple(shape[:3]):
        raise ValueError("%s: mask must be [N,H,W,1] over the operands' %s, got %s" % (op, tuple(shape[:3]), np.asarray(mask).shape))
    m = m.astype(dtype)
    if not np.all(np.isfinite(m)):
        raise ValueError("%s: mask must be finite" % op)
    return m


def ssim_loss_host(pred, target, max_val=1.0, dtype=np.float64, weight=1.0, mask=None):
    """(loss, grad): loss = weight * (1 - mean of ssim_map over images, windows and channels), a scalar of `dtype`, and grad =
    d loss / d pred, [N,H,W,C] in `dtype`; every step in `dtype` arithmetic.  At float32 this states mv3d_ssim_loss's own
    operation order (csrc/ssim_loss.hip); only the sum behind the mean differs (the kernel keeps it in double).

    Per window:  Dm = dS/dmx = 2 (my (A2 - A1) - mx S (B2 - B1)) / (B1 B2),  Ds = dS/dsab = 2 lum / B2,  Dq = dS/ds2 = -S / B2
    grad = -weight / count * (Ft(Dm) + target * Ft(Ds) + 2 pred * Ft(Dq));  pred == target gives exactly (0, zeros).

    mask (None = the code above, untouched): m [N,H,W,1], any finite values, never differentiated, indexed by the pixel of pred
    (mv3d_ssim_loss_masked).  A window with origin (oy, ox) takes the mask at its centre, m_w = m(oy + 5, ox + 5), the same for
    every channel:
      loss = weight * (mean(m_w broadcast over C) - mean(m_w * S)),   both means over the N Hv Wv C windows (a masked window still
      counts: masked_euclidean_loss keeps its mean over all pixels the same way); the kernel keeps the two sums in double;
      Dm, Ds, Dq are each multiplied by m_w (one multiply each) before the transposed passes.
    m == 1 gives the unmasked numbers bit for bit, m == 0 gives (0, zeros), pred == target gives exactly 0 under any mask, and
    both results are linear in m."""
    dtype = np.dtype(dtype).type
    a, b, max_val = _ssim_operands(pred, target, max_val, dtype)
    weight = float(np.float32(weight))                       # the C ABI takes a float
    if not math.isfinite(weight):
        raise ValueError("ssim_loss: weight must be finite")
    w = ssim_window(dtype)
    two = dtype(2)
    mx, my, A1, B1, A2, B2, lum, S = _ssim_parts(a, b, max_val, dtype)
    count = S.size
    dm = ((my * (A2 - A1) - (mx * S) * (B2 - B1)) * two) / (B1 * B2)
    ds = (lum / B2) * two
    dq = -(S / B2)
    if mask is None:
        loss = dtype(weight * float(dtype(1) - S.mean(dtype=dtype)))
    else:
        half = WINDOW_TAPS // 2
        mw = _host_mask('ssim_loss', mask, a.shape, dtype)[:, half:half + S.shape[1], half:half + S.shape[2], None]
        loss = dtype(weight * float(np.broadcast_to(mw, S.shape).mean(dtype=dtype) - (mw * S).mean(dtype=dtype)))
        dm, ds, dq = dm * mw, ds * mw, dq * mw
    g = (_transposed_filter(dm, w) + b * _transposed_filter(ds, w)) + (a * two) * _transposed_filter(dq, w)
    return loss, g * dtype(-weight / count)


def image_metrics_host(pred, target, max_val=1.0, dtype=np.float64):
    """[N,3] = (l1, mse, ssim) per image, every step in `dtype` arithmetic (see the module docstring)."""
    dt = np.dtype(dtype).type
    m = ssim_map(pred, target, max_val, dt)
    a, b = np.asarray(pred).astype(dt), np.asarray(target).astype(dt)
    d = a - b
    out = np.empty((a.shape[0], 3), dt)
    out[:, L1] = np.abs(d).sum(axis=3, dtype=dt).mean(axis=(1, 2), dtype=dt)
    out[:, MSE] = (d * d).mean(axis=(1, 2, 3), dtype=dt)
    out[:, SSIM] = m.mean(axis=(1, 2, 3), dtype=dt)
    return out


def psnr(mse, max_val=1.0):
    """10 log10(max_val^2 / mse), elementwise in float64; inf where mse == 0."""
    mse = np.asarray(mse, np.float64)
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(float(max_val) ** 2 / mse)


# ---------------------------------------------------------------------------------------------- device side
def channel_view(t, offset, channels):
    """Channels [offset, offset + channels) of a graph Tensor as a view (what tf.split / tf.slice give); usable after the graph
    is compiled, adds no node."""
    from .graph import Tensor
    if offset < 0 or channels < 1 or offset + channels > t.C:
        raise ValueError("channels [%d, %d) of a %d-channel tensor" % (offset, offset + channels, t.C))
    return Tensor(t.graph, t.shape[:-1] + (channels,), storage=t.storage, ch_off=t.ch_off + offset, act=t.act, leak=t.leak)


def _operand(x, what):
    """(data pointer, shape, pixel stride, torch device or None) of a graph Tensor or a torch device tensor."""
    import torch
    if torch.is_tensor(x):
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError("image_metrics: %s must be float32 [N,H,W,C], got %s %s" % (what, x.dtype, tuple(x.shape)))
        n, h, w, c = x.shape
        ld = x.stride(2)
        if x.stride(3) != 1 or x.stride(1) != w * ld or x.stride(0) != h * w * ld or ld < c:
            raise ValueError("image_metrics: %s must be NHWC with one pixel stride (a channel slice of a dense tensor), "
                             "strides %s" % (what, x.stride()))
        return x.data_ptr(), (n, h, w, c), ld, x.device
    if len(x.shape) != 4:
        raise ValueError("image_metrics: %s must be [N,H,W,C], got %s" % (what, x.shape))
    return x.ptr, tuple(x.shape), x.ld, x.graph.device


def _same_device(a, b):
    """A graph Tensor names its device as the graph was given it ('cuda'), a torch tensor with its index ('cuda:0')."""
    import torch
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index is None or b.index is None or a.index == b.index)


def _mask_operand(op, mask, shape, dev):
    """(data pointer, pixel stride) of the mask of a masked image loss: a graph Tensor or a torch device tensor [N,H,W,1] over the
    operands' N, H, W on their device (a channel of a wider tensor works); None for no mask."""
    if mask is None:
        return None
    pm, shape_m, m_ld, dev_m = _operand(mask, 'mask')
    if shape_m != tuple(shape[:3]) + (1,):
        raise ValueError("%s: mask must be [N,H,W,1] over the operands' %s, got %s" % (op, tuple(shape[:3]), shape_m))
    if not _same_device(dev_m, dev):
        raise ValueError("%s: mask on %s, operands on %s" % (op, dev_m, dev))
    return pm, m_ld


# The preamble of the eager wrappers below, in the order each of them takes it: operands, the GPU check, grad, the launch resources.
def _gpu_device(op, dev, *others):
    """`dev` as a torch.device; Mv3dError unless it and `others` are GPU devices."""
    import torch
    from . import _lib
    dev = torch.device(dev)
    if any(torch.device(d).type != 'cuda' for d in (dev,) + others):
        raise _lib.Mv3dError("%s runs on the GPU (operands are on %s); %s_host is the numpy form" % (op, dev, op))
    return dev


def _image_pair(op, pred, target):
    """((address, pixel stride) of pred, the same of target, their one shape, their GPU device) of an image operation."""
    pa, shape, a_ld, dev = _operand(pred, 'pred')
    pb, shape_b, b_ld, dev_b = _operand(target, 'target')
    if shape != shape_b:
        raise ValueError("%s: pred %s and target %s differ in shape" % (op, shape, shape_b))
    return (pa, a_ld), (pb, b_ld), shape, _gpu_device(op, dev, dev_b)


def _grad_operand(op, grad, of, shape, dev):
    """(address, pixel stride) of `grad`, a torch tensor of the shape and on the device of the operand named `of`; None for None."""
    import torch
    if grad is None:
        return None
    if not torch.is_tensor(grad):
        raise ValueError("%s: grad must be a torch device tensor" % op)
    pg, shape_g, g_ld, dev_g = _operand(grad, 'grad')
    if shape_g != shape or not _same_device(dev_g, dev):
        raise ValueError("%s: grad %s on %s does not match %s %s on %s" % (op, shape_g, dev_g, of, shape, dev))
    return pg, g_ld


def _stats_operand(op, stats, count, dev):
    """The address of `stats`, a dense float32 [count] tensor on `dev`; None for None."""
    import torch
    if stats is None:
        return None
    if (not torch.is_tensor(stats) or tuple(stats.shape) != (count,) or stats.dtype != torch.float32 or not stats.is_contiguous()
            or not _same_device(stats.device, dev)):
        raise ValueError("%s: stats must be a dense float32 [%d] tensor on the flow's device" % (op, count))
    return stats.data_ptr()


_workspaces = {}        # torch device -> uint8 workspace tensor, grown on demand (calls on one stream share it in order)


def _workspace(device, nbytes):
    import torch
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 4096), dtype=torch.uint8, device=device)
        _workspaces[device] = ws
    return ws


def _launch(dev, nbytes, stream):
    """(a zeroed 0-d result on dev, (address, bytes) of a workspace of nbytes, `stream` or torch's current one of dev)."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    return torch.zeros((), dtype=torch.float32, device=dev), (_workspace(dev, nbytes).data_ptr(), nbytes), stream


def image_metrics(pred, target, max_val=1.0, out=None, stream=None):
    """mv3d_image_metrics on device memory.  pred / target: graph Tensors (channel views from split included) or torch device
    tensors, [N,H,W,C] float32.  out: an optional dense float32 [N,3] device tensor to write into.  Asynchronous on `stream`
    (a raw stream handle; default: torch's current stream of the operands' device).  Returns the [N,3] device tensor with
    columns (l1, mse, ssim)."""
    import torch
    from . import _lib
    a, b, shape, dev = _image_pair('image_metrics', pred, target)
    n, h, w, c = shape
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("image_metrics: out must be a dense float32 [%d,3] tensor" % n)
    lib = _lib.lib()
    nbytes = int(lib.image_metrics_workspace_bytes(n, h, w, c))
    ws = _workspace(out.device, nbytes)
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    lib.image_metrics(n, h, w, c, *a, *b, float(max_val), out.data_ptr(), ws.data_ptr(), nbytes, stream)
    return out


def ssim_loss(pred, target, max_val=1.0, weight=1.0, grad=None, accumulate=False, stream=None, mask=None):
    """mv3d_ssim_loss on device memory: weight * (1 - mean SSIM) of pred against target, and optionally its gradient with
    respect to pred.  mask (None = mv3d_ssim_loss, exactly as before): a float32 [N,H,W,1] graph Tensor or torch device tensor
    (a channel of a wider tensor works); the call is then mv3d_ssim_loss_masked (ssim_loss_host states the definition).  pred / target: graph Tensors (channel views included) or torch device tensors, [N,H,W,C] float32, with
    the operand rules of image_metrics.  grad: an optional float32 device tensor of pred's shape with one pixel stride (a
    channel slice of a dense tensor works); it is overwritten, or added to when accumulate is true.  Asynchronous on `stream`
    (default: torch's current stream of the operands' device).  Returns the loss as a 0-d device tensor."""
    from . import _lib, loss_calls
    a, b, shape, dev = _image_pair('ssim_loss', pred, target)
    grad = _grad_operand('ssim_loss', grad, 'pred', shape, dev)
    mask = _mask_operand('ssim_loss', mask, shape, dev)
    lib = _lib.lib()
    out, ws, stream = _launch(dev, loss_calls.ssim_workspace_bytes(lib, shape, mask is not None), stream)
    loss_calls.ssim(lib, shape, a, b, mask, max_val, weight, out.data_ptr(), grad, accumulate, ws, stream)
    return out


# ------------------------------------------------------------------------------------------------ flow smoothness
def _smooth_scalars(edge_alpha, eps, weight):
    """(edge_alpha, eps, weight) as the floats the C ABI takes; ValueError on what mv3d_flow_smoothness would refuse."""
    edge_alpha, eps, weight = (float(np.float32(v)) for v in (edge_alpha, eps, weight))
    if not math.isfinite(edge_alpha) or edge_alpha < 0:
        raise ValueError("flow_smoothness: edge_alpha must be finite and not negative")
    if not math.isfinite(eps) or eps <= 0:
        raise ValueError("flow_smoothness: eps must be finite and positive")
    if not math.isfinite(weight):
        raise ValueError("flow_smoothness: weight must be finite")
    return edge_alpha, eps, weight


def _smooth_order(order):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order not in (1, 2):
        raise ValueError("flow_smoothness: order must be 1 or 2, got %r" % (order,))
    return int(order)


def _smooth_shape(shape, order=1):
    if len(shape) != 4 or shape[3] != 2:
        raise ValueError("flow_smoothness: flow must be [N,H,W,2], got %s" % (tuple(shape),))
    side = order + 1                                         # a difference of this order spans order + 1 pixels
    if shape[0] < 1 or shape[1] < side or shape[2] < side:
        raise ValueError("flow_smoothness: flow %s needs N >= 1 and H, W >= %d" % (tuple(shape), side))


def _smooth_operands(flow, guide, edge_alpha, eps, weight, dtype, order=1):
    """The operand checks of the flow-smoothness functions: (flow, guide or None) in `dtype`, and edge_alpha, eps, weight as the
    floats the C ABI takes."""
    f = np.asarray(flow).astype(dtype)
    _smooth_shape(f.shape, order)
    g = None
    if guide is not None:
        g = np.asarray(guide).astype(dtype)
        if g.ndim != 4 or g.shape[:3] != f.shape[:3] or not 1 <= g.shape[3] <= 4:
            raise ValueError("flow_smoothness: guide must be [N,H,W,1..4] over the flow's %s, got %s" % (f.shape[:3], g.shape))
    edge_alpha, eps, weight = _smooth_scalars(edge_alpha, eps, weight)
    return f, g, edge_alpha, eps, weight


def flow_smoothness_host(flow, guide=None, edge_alpha=10.0, eps=1e-3, dtype=np.float64, weight=1.0, order=1):
    """(loss, grad) of the edge-aware first-order smoothness of a flow [N,H,W,2]: loss = weight * S, a scalar of `dtype`, and
    grad = d loss / d flow, [N,H,W,2] in `dtype`; every step in `dtype` arithmetic.  At float32 this states mv3d_flow_smoothness's
    own operation order (csrc/flow_smooth.hip); only the two sums behind S (the kernel keeps them in double) and exp differ.

      dx = f[:, :, 1:] - f[:, :, :-1]      wx = exp(-(edge_alpha / Cg) * sum_k |I[:, :, 1:, k] - I[:, :, :-1, k]|)   (1 without a guide)
      dy = f[:, 1:] - f[:, :-1]            wy the same along rows
      r = sqrt(d * d + eps * eps)          phi = r - eps (Charbonnier)          phi' = d / r
      S = sum(wx * phi(dx)) / Zx + sum(wy * phi(dy)) / Zy,      Zx = N H (W-1) 2,  Zy = N (H-1) W 2
      grad[i, j] = (ex[i, j-1] - ex[i, j]) * (weight / Zx) + (ey[i-1, j] - ey[i, j]) * (weight / Zy),   e = w * phi', 0 out of range
    The guide is not differentiated.  sqrt(eps * eps) == eps, so a constant flow gives exactly (0, zeros).

    order=2 is the second-order term, the twin of mv3d_flow_smoothness2 (H, W >= 3): _smooth2_host states it."""
    dtype = np.dtype(dtype).type
    order = _smooth_order(order)
    f, g, edge_alpha, eps, weight = _smooth_operands(flow, guide, edge_alpha, eps, weight, dtype, order)
    if order == 2:
        return _smooth2_host(f, g, edge_alpha, eps, weight, dtype)
    n, h, w, _ = f.shape
    eps_t = dtype(eps)
    eps2 = eps_t * eps_t
    zx, zy = float(n) * h * (w - 1) * 2.0, float(n) * (h - 1) * w * 2.0

    def edges(axis):
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        d = f[tuple(hi)] - f[tuple(lo)]
        if g is None:
            wgt = np.ones(d.shape[:3] + (1,), dtype)
        else:
            ad = np.abs(g[tuple(hi)] - g[tuple(lo)])
            s = np.zeros(ad.shape[:3], dtype)
            for k in range(ad.shape[3]):                     # channels added in index order
                s = s + ad[..., k]
            wgt = np.exp(-(dtype(edge_alpha / g.shape[3]) * s))[..., None].astype(dtype)
        r = np.sqrt(d * d + eps2)
        return wgt * (d / r), wgt * (r - eps_t)

    ex, vx = edges(2)
    ey, vy = edges(1)
    loss = dtype(weight * (float(vx.sum(dtype=dtype)) / zx + float(vy.sum(dtype=dtype)) / zy))
    px = np.zeros((n, h, w + 1, 2), dtype)
    px[:, :, 1:w] = ex
    py = np.zeros((n, h + 1, w, 2), dtype)
    py[:, 1:h] = ey
    grad = (px[:, :, :-1] - px[:, :, 1:]) * dtype(weight / zx) + (py[:, :-1] - py[:, 1:]) * dtype(weight / zy)
    return loss, grad


def _smooth2_slices(axis):
    """The index tuples of the -, c and + pixels of every three-pixel stencil along `axis` of an [N,H,W,C] array."""
    lo, mid, hi = ([slice(None)] * 4 for _ in range(3))
    lo[axis], mid[axis], hi[axis] = slice(None, -2), slice(1, -1), slice(2, None)
    return tuple(lo), tuple(mid), tuple(hi)


def _smooth2_weights(g, edge_alpha, axis, dtype):
    """The stencil weights of _smooth2_host along `axis` for the guide g (in `dtype`), one per stencil centre."""
    lo, mid, hi = _smooth2_slices(axis)
    below, above = np.abs(g[mid] - g[lo]), np.abs(g[hi] - g[mid])
    s = np.zeros(below.shape[:3], dtype)
    for k in range(below.shape[3]):                          # channels in index order, the lower edge before the upper one
        s = s + below[..., k]
        s = s + above[..., k]
    return np.exp(-(dtype(edge_alpha / g.shape[3]) * s)).astype(dtype)


def _smooth2_host(f, g, edge_alpha, eps, weight, dtype):
    """flow_smoothness_host at order 2 on checked operands: the penalty of the second differences, which is minimal for an affine
    flow.  Along an axis, with c the centre of a three-pixel stencil and -, + its neighbours (x centres j = 1..W-2, y centres
    i = 1..H-2):

      d = (f[+] - f[c]) - (f[c] - f[-])                           per flow channel
      s = 0;  for k: s = s + |I[c,k] - I[-,k]|;  s = s + |I[+,k] - I[c,k]|
      w = exp(-((edge_alpha / Cg) * s))                            1 without a guide or with edge_alpha == 0 (no guide is read):
                                                                   the product of the first-order weights of the two edges spanned
      r = sqrt(d * d + eps * eps)      v = w * (r - eps)           e = w * (d / r)
      S2 = sum(vx) / Z2x + sum(vy) / Z2y,      Z2x = N H (W-2) 2,  Z2y = N (H-2) W 2
      grad[i, j] = ((ex[i, j-1] - ex[i, j]) - (ex[i, j] - ex[i, j+1])) * (weight / Z2x)
                 + ((ey[i-1, j] - ey[i, j]) - (ey[i, j] - ey[i+1, j])) * (weight / Z2y),      e = 0 where no stencil is centred
    A flow whose first differences are exact and equal along each axis (constant, affine with dyadic coefficients) gives exactly
    (0, zeros) under any guide."""
    n, h, w, _ = f.shape
    eps_t = dtype(eps)
    eps2 = eps_t * eps_t
    zx, zy = float(n) * h * (w - 2) * 2.0, float(n) * (h - 2) * w * 2.0

    def stencils(axis):
        lo, mid, hi = _smooth2_slices(axis)
        d = (f[hi] - f[mid]) - (f[mid] - f[lo])
        if g is None or edge_alpha == 0:
            wgt = np.ones(d.shape[:3] + (1,), dtype)
        else:
            wgt = _smooth2_weights(g, edge_alpha, axis, dtype)[..., None]
        r = np.sqrt(d * d + eps2)
        return wgt * (d / r), wgt * (r - eps_t)

    ex, vx = stencils(2)
    ey, vy = stencils(1)
    loss = dtype(weight * (float(vx.sum(dtype=dtype)) / zx + float(vy.sum(dtype=dtype)) / zy))
    px = np.zeros((n, h, w + 2, 2), dtype)                   # ex at centre j sits at column j + 1
    px[:, :, 2:w] = ex
    py = np.zeros((n, h + 2, w, 2), dtype)
    py[:, 2:h] = ey
    grad = (((px[:, :, :-2] - px[:, :, 1:-1]) - (px[:, :, 1:-1] - px[:, :, 2:])) * dtype(weight / zx)
            + ((py[:, :-2] - py[:, 1:-1]) - (py[:, 1:-1] - py[:, 2:])) * dtype(weight / zy))
    return loss, grad


def flow_smoothness(flow, guide=None, edge_alpha=10.0, eps=1e-3, weight=1.0, grad=None, accumulate=False, stream=None, order=1):
    """mv3d_flow_smoothness on device memory (order=2: mv3d_flow_smoothness2, H, W >= 3): weight * S of flow_smoothness_host at that
    order, and optionally its gradient with respect to the flow.  flow / guide: graph Tensors (channel views included) or torch device tensors, float32 [N,H,W,2] / [N,H,W,1..4].  grad: an
    optional float32 device tensor of the flow's shape with one pixel stride (a channel slice of a dense tensor works); it is
    overwritten, or added to when accumulate is true.  Asynchronous on `stream` (default: torch's current stream of the operands'
    device).  Returns the loss as a 0-d device tensor."""
    from . import _lib, loss_calls
    pf, shape, f_ld, dev = _operand(flow, 'flow')
    order = _smooth_order(order)
    _smooth_shape(shape, order)
    edge_alpha, eps, weight = _smooth_scalars(edge_alpha, eps, weight)      # the twin's checks: the same ValueError for the same argument
    if guide is not None:
        pgd, shape_g, gd_ld, dev_g = _operand(guide, 'guide')
        if shape_g[:3] != shape[:3] or not 1 <= shape_g[3] <= 4:
            raise ValueError("flow_smoothness: guide must be [N,H,W,1..4] over the flow's %s, got shape %s" % (shape[:3], shape_g))
        if not _same_device(dev_g, dev):
            raise ValueError("flow_smoothness: guide on %s, flow on %s" % (dev_g, dev))
        guide = (pgd, shape_g[3], gd_ld)
    dev = _gpu_device('flow_smoothness', dev)
    grad = _grad_operand('flow_smoothness', grad, 'flow', shape, dev)
    lib = _lib.lib()
    out, ws, stream = _launch(dev, loss_calls.flow_smoothness_workspace_bytes(lib, shape[:3], order), stream)
    loss_calls.flow_smoothness(lib, shape[:3], (pf, f_ld), guide, edge_alpha, eps, weight, out.data_ptr(), grad, accumulate, ws, stream,
                               order)
    return out


# ------------------------------------------------------------------------------------------------ forward-backward flow consistency
def _consist_scalars(eps, weight):
    """(eps, weight) as the floats the C ABI takes; ValueError on what mv3d_flow_consistency would refuse."""
    eps, weight = (float(np.float32(v)) for v in (eps, weight))
    if not math.isfinite(eps) or eps <= 0:
        raise ValueError("flow_consistency: eps must be finite and positive")
    if not float(np.float32(eps) * np.float32(eps)) >= float(np.finfo(np.float32).tiny):
        raise ValueError("flow_consistency: eps (%g) is below 2^-63: eps * eps underflows in float32, and with it the exact zeros" % eps)
    if not math.isfinite(weight):
        raise ValueError("flow_consistency: weight must be finite")
    return eps, weight


def _consist_shape(shape):
    if len(shape) != 4 or shape[3] != 2:
        raise ValueError("flow_consistency: flow must be [N,H,W,2], got %s" % (tuple(shape),))
    if shape[0] < 2 or shape[0] % 2:
        raise ValueError("flow_consistency: flow %s needs an even N >= 2 (the second half holds the reversed pairs)" % (tuple(shape),))
    if shape[1] != shape[2] or shape[1] < 2:
        raise ValueError("flow_consistency: flow %s needs H == W >= 2 (the transposed sampler convention)" % (tuple(shape),))


def flow_consistency_host(flow, eps=1e-3, dtype=np.float64, weight=1.0):
    """(loss, grad, value, valid_fraction) of the forward-backward consistency of a pair-swapped batch of flows [N,H,W,2] (N even,
    H == W): loss = weight * C and value = C are scalars of `dtype`, grad = d loss / d flow is [N,H,W,2] in `dtype`; every step in
    `dtype` arithmetic.  At float32 this states mv3d_flow_consistency's own operation order (csrc/flow_consist.hip); only the sum
    behind C (the kernel keeps it in double) and the scatter (the kernel sums it in 64-bit fixed point) differ.

      partner of sample n: m = (n + N/2) mod N
      x = f[..., 0] + i (the ROW index),  y = f[..., 1] + j: the sampler reads x as the column and y as the row (the transposed
          convention of warp_pts_layer + resample_layer)
      valid = 0 <= x <= W-1 and 0 <= y <= H-1 (NaN, inf: not valid); stricter than the sampler's window, so no tap with a non-zero
          weight is outside the image.  A tap at index W or H has weight 0, reads 0 and receives nothing
      w = (dx dy, (1-dx)(1-dy), dx (1-dy), (1-dx) dy) for the taps ff cc fc cf of flow[m];  s = ((w0 ff + w1 cc) + w2 fc) + w3 cf
      r0 = f0 + s1,  r1 = f1 + s0 (the channel swap belongs to the convention),  d = sqrt((r0 r0 + r1 r1) + eps eps)
      phi = d - eps,  psi = (r0 / d, r1 / d);   C = sum over valid of phi / (N H W);  valid_fraction = count(valid) / (N H W)
      k = weight / (N H W);  gx = psi1 (dy (cf0 - ff0) + (1-dy) (cc0 - fc0)) + psi0 (the same of channel 1), gy with dx and
          (fc - ff), (cc - cf): the sampler's warp gradient for dgen = (psi1, psi0)
      grad[n,i,j] = ((psi0 + gx) k, (psi1 + gy) k) where valid;   grad[m, tap q] += (w_q psi1, w_q psi0) summed, then times k
    Flows that invert each other on integer offsets, (a, b) against (-b, -a), give exactly (0, zeros, 0, .)."""
    dtype = np.dtype(dtype).type
    f = np.asarray(flow).astype(dtype)
    _consist_shape(f.shape)
    eps, weight = _consist_scalars(eps, weight)
    n, h, w, _ = f.shape
    half = n // 2
    npix = float(n) * h * w
    one, zero = dtype(1), dtype(0)
    eps_t = dtype(eps)
    eps2 = eps_t * eps_t
    partner = np.roll(f, -half, axis=0)                      # partner[n] = f[(n + N/2) mod N]
    ii, jj = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing='ij')
    x = f[..., 0] + ii[None]
    y = f[..., 1] + jj[None]
    with np.errstate(invalid='ignore'):
        valid = (x >= 0) & (y >= 0) & (x <= w - 1) & (y <= h - 1)
    xs, ys = np.where(valid, x, zero), np.where(valid, y, zero)
    fxf, fyf = np.floor(xs), np.floor(ys)
    dx, dy = (fxf + one) - xs, (fyf + one) - ys
    fx, fy = fxf.astype(np.int64), fyf.astype(np.int64)
    b = np.broadcast_to(np.arange(n).reshape(n, 1, 1), x.shape)

    taps = []                                                # (ok, row, column, values) of ff, cc, fc, cf
    for yy, xx in ((fy, fx), (fy + 1, fx + 1), (fy + 1, fx), (fy, fx + 1)):
        ok = valid & (xx < w) & (yy < h)
        yc, xc = np.minimum(yy, h - 1), np.minimum(xx, w - 1)
        taps.append((ok, yc, xc, np.where(ok[..., None], partner[b, yc, xc], zero)))
    wq = (dx * dy, (one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy)
    iff, icc, ifc, icf = (t[3] for t in taps)
    s = ((wq[0][..., None] * iff + wq[1][..., None] * icc) + wq[2][..., None] * ifc) + wq[3][..., None] * icf
    r0, r1 = f[..., 0] + s[..., 1], f[..., 1] + s[..., 0]
    d = np.sqrt((r0 * r0 + r1 * r1) + eps2)
    phi = np.where(valid, d - eps_t, zero)
    psi0, psi1 = np.where(valid, r0 / d, zero), np.where(valid, r1 / d, zero)
    c = float(phi.sum(dtype=dtype)) / npix
    value, loss = dtype(c), dtype(weight * c)
    valid_fraction = dtype(float(np.count_nonzero(valid)) / npix)
    k = dtype(weight / npix)

    gx = np.zeros(x.shape, dtype)
    gy = np.zeros(x.shape, dtype)
    for ch, g in ((0, psi1), (1, psi0)):                     # channels added in index order
        gx = gx + g * (dy * (icf[..., ch] - iff[..., ch]) + (one - dy) * (icc[..., ch] - ifc[..., ch]))
        gy = gy + g * (dx * (ifc[..., ch] - iff[..., ch]) + (one - dx) * (icc[..., ch] - icf[..., ch]))
    grad = np.where(valid[..., None], np.stack(((psi0 + gx) * k, (psi1 + gy) * k), axis=-1), zero).astype(dtype)
    scat = np.zeros(f.shape, dtype)
    mb = (b + half) % n
    def finite(v):                                           # a non-finite entry (a non-finite partner flow) is dropped, as by the kernel
        return np.where(np.isfinite(v), v, zero)
    for q, (ok, yc, xc, _) in enumerate(taps):
        np.add.at(scat, (mb[ok], yc[ok], xc[ok], 0), finite(wq[q] * psi1)[ok])
        np.add.at(scat, (mb[ok], yc[ok], xc[ok], 1), finite(wq[q] * psi0)[ok])
    grad = grad + scat * k
    return loss, grad, value, valid_fraction


def flow_consistency(flow, eps=1e-3, weight=1.0, grad=None, accumulate=False, stats=None, stream=None):
    """mv3d_flow_consistency on device memory: weight * C of flow_consistency_host, and optionally its gradient with respect to the
    flow.  flow: a graph Tensor (channel views included) or a torch device tensor, float32 [N,H,W,2], N even, H == W.  grad: an
    optional float32 device tensor of the flow's shape with one pixel stride (a channel slice of a dense tensor works); it is
    overwritten, or added to when accumulate is true.  stats: an optional dense float32 [2] device tensor that receives the
    unweighted C and the valid fraction.  Asynchronous on `stream` (default: torch's current stream of the operands' device).
    Returns the loss as a 0-d device tensor."""
    from . import _lib, loss_calls
    pf, shape, f_ld, dev = _operand(flow, 'flow')
    _consist_shape(shape)
    eps, weight = _consist_scalars(eps, weight)              # the twin's checks: the same ValueError for the same argument
    dev = _gpu_device('flow_consistency', dev)
    grad = _grad_operand('flow_consistency', grad, 'flow', shape, dev)
    ps = _stats_operand('flow_consistency', stats, 2, dev)
    lib = _lib.lib()
    out, ws, stream = _launch(dev, loss_calls.flow_consistency_workspace_bytes(lib, shape[:3]), stream)
    loss_calls.flow_consistency(lib, shape[:3], (pf, f_ld), eps, weight, out.data_ptr(), ps, grad, accumulate, ws, stream)
    return out


# ------------------------------------------------------------------------------------------------ occlusion mask of the head loss
def _occlusion_scalars(alpha1, alpha2, outside_visible):
    """(alpha1, alpha2, outside_visible) as the values the C ABI takes; ValueError on what mv3d_flow_occlusion_mask would refuse."""
    if isinstance(alpha1, bool) or isinstance(alpha2, bool):
        raise ValueError("flow_occlusion_mask: alpha1 and alpha2 must be numbers")
    alpha1, alpha2 = (float(np.float32(v)) for v in (alpha1, alpha2))
    if not math.isfinite(alpha1) or alpha1 < 0:
        raise ValueError("flow_occlusion_mask: alpha1 must be finite and >= 0")
    if not math.isfinite(alpha2) or alpha2 <= 0:
        raise ValueError("flow_occlusion_mask: alpha2 must be finite and positive")
    if not isinstance(outside_visible, (bool, np.bool_)):
        raise ValueError("flow_occlusion_mask: outside_visible must be True or False, got %r" % (outside_visible,))
    return alpha1, alpha2, bool(outside_visible)


def flow_occlusion_mask_host(flow, alpha1=0.01, alpha2=0.5, outside_visible=True, dtype=np.float64, details=False):
    """(mask [N,H,W] of `dtype`, (visible, occluded, outside) shares of N H W as floats) of a pair-swapped batch of flows [N,H,W,2]
    (N even, H == W): the forward-backward occlusion test of UnFlow in the conventions of flow_consistency_host, every step in
    `dtype` arithmetic.  At float32 this states mv3d_flow_occlusion_mask's own operation order (csrc/flow_occlusion.hip).

      partner of sample n: m = (n + N/2) mod N;   x = f[..., 0] + i (the ROW index),  y = f[..., 1] + j
      inside = 0 <= x <= W-1 and 0 <= y <= H-1 (NaN, inf: not inside): the consistency term's strict window
      w = (dx dy, (1-dx)(1-dy), dx (1-dy), (1-dx) dy) for the taps ff cc fc cf of flow[m];  s = ((w0 ff + w1 cc) + w2 fc) + w3 cf
      r0 = f0 + s1,  r1 = f1 + s0;   lhs = r0 r0 + r1 r1;   rhs = alpha1 ((f0 f0 + f1 f1) + (s0 s0 + s1 s1)) + alpha2
      visible = inside and lhs < rhs (a NaN on either side: not visible, the pixel counts as occluded)
      mask = 1 where visible, 0 where inside and not visible, and (1 if outside_visible else 0) where not inside
    The mask has no gradient.  With details=True a third result (lhs, rhs, inside) is returned, for tests that need the margins."""
    dtype = np.dtype(dtype).type
    f = np.asarray(flow).astype(dtype)
    _consist_shape(f.shape)
    alpha1, alpha2, outside_visible = _occlusion_scalars(alpha1, alpha2, outside_visible)
    n, h, w, _ = f.shape
    half = n // 2
    one, zero = dtype(1), dtype(0)
    a1, a2 = dtype(np.float32(alpha1)), dtype(np.float32(alpha2))
    partner = np.roll(f, -half, axis=0)                      # partner[n] = f[(n + N/2) mod N]
    ii, jj = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing='ij')
    x = f[..., 0] + ii[None]
    y = f[..., 1] + jj[None]
    with np.errstate(invalid='ignore'):
        inside = (x >= 0) & (y >= 0) & (x <= w - 1) & (y <= h - 1)
    xs, ys = np.where(inside, x, zero), np.where(inside, y, zero)
    fxf, fyf = np.floor(xs), np.floor(ys)
    dx, dy = (fxf + one) - xs, (fyf + one) - ys
    fx, fy = fxf.astype(np.int64), fyf.astype(np.int64)
    b = np.broadcast_to(np.arange(n).reshape(n, 1, 1), x.shape)
    taps = []                                                # values of ff, cc, fc, cf
    for yy, xx in ((fy, fx), (fy + 1, fx + 1), (fy + 1, fx), (fy, fx + 1)):
        ok = inside & (xx < w) & (yy < h)
        yc, xc = np.minimum(yy, h - 1), np.minimum(xx, w - 1)
        taps.append(np.where(ok[..., None], partner[b, yc, xc], zero))
    wq = (dx * dy, (one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy)
    with np.errstate(invalid='ignore', over='ignore'):
        s = ((wq[0][..., None] * taps[0] + wq[1][..., None] * taps[1]) + wq[2][..., None] * taps[2]) + wq[3][..., None] * taps[3]
        f0, f1 = f[..., 0], f[..., 1]
        r0, r1 = f0 + s[..., 1], f1 + s[..., 0]
        lhs = r0 * r0 + r1 * r1
        rhs = a1 * ((f0 * f0 + f1 * f1) + (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1])) + a2
        visible = inside & (lhs < rhs)
    mask = np.where(inside, np.where(visible, one, zero), one if outside_visible else zero).astype(dtype)
    npix = float(n) * h * w
    shares = (np.count_nonzero(visible) / npix, np.count_nonzero(inside & ~visible) / npix, np.count_nonzero(~inside) / npix)
    if details:
        return mask, shares, (lhs, rhs, inside)
    return mask, shares


def flow_occlusion_mask(flow, alpha1=0.01, alpha2=0.5, outside_visible=True, out=None, stats=None, stream=None):
    """mv3d_flow_occlusion_mask on device memory: the mask of flow_occlusion_mask_host.  flow: a graph Tensor (channel views
    included) or a torch device tensor, float32 [N,H,W,2], N even, H == W.  out: an optional float32 device tensor [N,H,W] or
    [N,H,W,1] with one pixel stride (a channel of a wider tensor works); a dense [N,H,W,1] tensor is made when it is None.  stats:
    an optional dense float32 [3] device tensor that receives the visible, occluded and outside shares.  Asynchronous on `stream`
    (default: torch's current stream of the operands' device).  Returns the mask tensor."""
    import torch
    from . import _lib
    pf, shape, f_ld, dev = _operand(flow, 'flow')
    _consist_shape(shape)
    alpha1, alpha2, outside_visible = _occlusion_scalars(alpha1, alpha2, outside_visible)
    dev = _gpu_device('flow_occlusion_mask', dev)
    n, h, w, _ = shape
    if out is None:
        out = torch.empty((n, h, w, 1), dtype=torch.float32, device=dev)
    if not torch.is_tensor(out):
        raise ValueError("flow_occlusion_mask: out must be a torch device tensor")
    view = out if out.dim() == 4 else out.unsqueeze(-1)
    po, shape_o, o_ld, dev_o = _operand(view, 'out')
    if shape_o != (n, h, w, 1) or not _same_device(dev_o, dev):
        raise ValueError("flow_occlusion_mask: out %s on %s does not match flow %s on %s" % (tuple(out.shape), dev_o, shape, dev))
    ps = _stats_operand('flow_occlusion_mask', stats, 3, dev)
    lib = _lib.lib()
    nbytes = int(lib.flow_occlusion_mask_workspace_bytes(n, h, w)) if ps is not None else 0
    ws = _workspace(dev, nbytes) if nbytes else None
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    lib.flow_occlusion_mask(n, h, w, pf, f_ld, float(alpha1), float(alpha2), 1 if outside_visible else 0, po, o_ld, ps,
                            ws.data_ptr() if ws is not None else None, nbytes, stream)
    return out


# ------------------------------------------------------------------------------------------------ multi-scale photometric loss
MULTISCALE_MAX_LEVELS = 3


def _multiscale_scalars(levels, level_weights, kind):
    """(levels, [w_l] as the floats the C ABI takes, kind); ValueError on what mv3d_multiscale_warp_loss would refuse."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MULTISCALE_MAX_LEVELS:
        raise ValueError("multiscale_warp_loss: levels must be an integer in 1..%d, got %r" % (MULTISCALE_MAX_LEVELS, levels))
    levels = int(levels)
    if level_weights is None:
        level_weights = [1.0] * levels
    weights = [float(np.float32(v)) for v in np.asarray(level_weights, np.float64).reshape(-1)]
    if len(weights) != levels:
        raise ValueError("multiscale_warp_loss: %d level_weights for %d levels" % (len(weights), levels))
    if not all(math.isfinite(v) for v in weights):
        raise ValueError("multiscale_warp_loss: level_weights must be finite, got %r" % (weights,))
    if kind not in (1, 2):
        raise ValueError("multiscale_warp_loss: kind must be 1 (absolute value) or 2 (square), got %r" % (kind,))
    return levels, weights, int(kind)


def _multiscale_shapes(src, flow, target, levels):
    """Checks [N,Hs,Ws,C], [N,H,W,2], [N,H,W,C] with C in 1..4 and every side a multiple of 2^levels."""
    src, flow, target = tuple(src), tuple(flow), tuple(target)
    if len(flow) != 4 or flow[3] != 2:
        raise ValueError("multiscale_warp_loss: flow must be [N,H,W,2], got %s" % (flow,))
    if len(target) != 4 or target[:3] != flow[:3] or not 1 <= target[3] <= 4:
        raise ValueError("multiscale_warp_loss: target must be [N,H,W,1..4] over the flow's %s, got %s" % (flow[:3], target))
    if len(src) != 4 or src[0] != flow[0] or src[3] != target[3]:
        raise ValueError("multiscale_warp_loss: src must be [N,Hs,Ws,C] with the target's N and C, got %s for target %s" % (src, target))
    f = 1 << levels
    for name, v in (('N', flow[0]), ('H', flow[1]), ('W', flow[2]), ('Hs', src[1]), ('Ws', src[2])):
        if v < 1 or (name != 'N' and v % f):
            raise ValueError("multiscale_warp_loss: %s (%d) must be a positive multiple of 2^levels = %d" % (name, v, 1 if name == 'N' else f))


def _multiscale_mask_shape(mask, flow):
    """Checks the mask's shape [N,H,W,1] over the flow's N, H, W."""
    if tuple(mask) != tuple(flow[:3]) + (1,):
        raise ValueError("multiscale_warp_loss: mask must be [N,H,W,1] over the flow's %s, got %s" % (tuple(flow[:3]), tuple(mask)))


def _pool2(x):
    """One pyramid step over [N,H,W,C]: 0.25 * ((p00 + p01) + (p10 + p11)) of every 2 x 2 block, in x's dtype."""
    return x.dtype.type(0.25) * ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))


def _bilinear_taps(data, x, y):
    """(valid, dx, dy, iff, icc, ifc, icf) of the sampler at (x = column, y = row) over data [N,Hs,Ws,C], in data's dtype: valid iff
    -1 < x < Ws and -1 < y < Hs; dx = (floor(x) + 1) - x; a tap outside the image, and every tap of an invalid point, is 0.  The
    expressions of mv3d_warp_resample_fwd / _bwd."""
    n, hs, ws, _ = data.shape
    one = data.dtype.type(1)
    valid = (x > -1) & (y > -1) & (x < ws) & (y < hs)
    fxf, fyf = np.floor(x), np.floor(y)
    dx, dy = ((fxf + one) - x)[..., None], ((fyf + one) - y)[..., None]
    fx = np.clip(fxf, -2, ws).astype(np.int64)          # the clip keeps the conversion defined for far-away points (not valid)
    fy = np.clip(fyf, -2, hs).astype(np.int64)
    b = np.broadcast_to(np.arange(n).reshape(n, 1, 1), x.shape)

    def tap(yy, xx):
        ok = valid & (xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)
        return np.where(ok[..., None], data[b, np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)], data.dtype.type(0))
    return valid, dx, dy, tap(fy, fx), tap(fy + 1, fx + 1), tap(fy + 1, fx), tap(fy, fx + 1)


def multiscale_warp_loss_host(src, flow, target, levels, level_weights=None, kind=2, dtype=np.float64, mask=None):
    """(value, grad, level_values) of the multi-scale photometric loss of a flow [N,H,W,2] that warps src [N,Hs,Ws,C] onto target
    [N,H,W,C]: value = sum_l w_l T_l, a scalar of `dtype`; grad = d value / d flow, [N,H,W,2]; level_values = [T_1 .. T_L], the
    unweighted terms; every step in `dtype` arithmetic.  At float32 this states mv3d_multiscale_warp_loss's own operation order
    (csrc/multiscale_loss.hip); only the sums behind T_l differ (the kernel keeps them in double).  For level l = 1..L, f = 2^l:

      pool_l   halves level l-1 (level 0 = the input): 0.25 * ((p00 + p01) + (p10 + p11)) of the 2 x 2 block p00 p01 / p10 p11
               (row-major); applied to src, to target and to both channels of the flow
      flow_l = pool_l(flow) * (1 / f);   x = flow_l[..., 0] + I (the ROW index),  y = flow_l[..., 1] + J: the sampler reads x as
               the column and y as the row (the transposed convention of warp_pts_layer + resample_layer).  Pooling with aligned
               pixel centres maps x to (x - (f-1)/2) / f, so the block mean is the coarse flow and no other offset appears
      gen_l  = ((dx dy iff + (1-dx)(1-dy) icc) + dx (1-dy) ifc) + (1-dx) dy icf over pool_l(src), 0 where the point is not valid
      d = gen_l - pool_l(target);   T_l = mean over (n,I,J) of sum_c phi(d),  phi = d d (kind 2) or |d| (kind 1)
      s_l = w_l k / (N H_l W_l) / f^3  (k = 2 or 1), formed in double and rounded once;  g = d s_l (kind 2) or sign(d) s_l (kind 1)
      G_l[..., 0] = sum_c g (dy (icf - iff) + (1-dy) (icc - ifc)),  G_l[..., 1] = sum_c g (dx (ifc - iff) + (1-dx) (icc - icf)),
               channels added in index order, 0 where the point is not valid
      grad[n,i,j] = (G_1[n, i>>1, j>>1] + G_2[n, i>>2, j>>2]) + G_3[n, i>>3, j>>3]      (1 / f^2 from the mean, 1 / f from the scaling)
    src and target are not differentiated.  gen_l == pool_l(target) at every level gives exactly (0, zeros, zeros).

    mask (optional): [N,H,W,1] over the flow's grid, not differentiated; the statement of mv3d_multiscale_warp_loss_masked:
      m_l    = pool_l(mask), the same pooling, level by level: a coarse pixel counts by its visible share, a 0/1 mask pools exactly
      T_l    = (1 / (N H_l W_l)) sum over (n,I,J) of m_l sum_c phi(d): the count stays that of the unmasked term, as in the masked
               census and SSIM terms
      g      = (d s_l) m_l (kind 2) or (sign(d) s_l) m_l (kind 1): s_l unchanged, the mask multiplies last; G_l and grad as above
    A mask of ones gives the unmasked result bit for bit, a mask of zeros exact zeros, gen_l == pool_l(target) exactly 0 under any
    mask; value and gradient are linear in the mask.  mask=None is the unmasked code, untouched."""
    dtype = np.dtype(dtype).type
    levels, weights, kind = _multiscale_scalars(levels, level_weights, kind)
    s, fl, t = (np.asarray(v).astype(dtype) for v in (src, flow, target))
    _multiscale_shapes(s.shape, fl.shape, t.shape, levels)
    ml = None
    if mask is not None:
        ml = np.asarray(mask).astype(dtype)
        _multiscale_mask_shape(ml.shape, fl.shape)
    n, h, w, _ = fl.shape
    one, zero = dtype(1), dtype(0)
    value, grad, level_values = 0.0, None, []
    for l in range(1, levels + 1):
        f = 1 << l
        s, fl, t = _pool2(s), _pool2(fl), _pool2(t)
        hl, wl = h >> l, w >> l
        ii, jj = np.meshgrid(np.arange(hl, dtype=dtype), np.arange(wl, dtype=dtype), indexing='ij')
        x = fl[..., 0] * dtype(1.0 / f) + ii[None]
        y = fl[..., 1] * dtype(1.0 / f) + jj[None]
        valid, dx, dy, iff, icc, ifc, icf = _bilinear_taps(s, x, y)
        gen = np.where(valid[..., None], ((dx * dy * iff + (one - dx) * (one - dy) * icc) + dx * (one - dy) * ifc) + (one - dx) * dy * icf, zero)
        d = gen - t
        count = float(n) * hl * wl
        scale = dtype(weights[l - 1] * (2.0 if kind == 2 else 1.0) / count / float(f * f * f))
        phi, g = (d * d, d * scale) if kind == 2 else (np.abs(d), np.sign(d) * scale)
        if ml is not None:
            ml = _pool2(ml)
            phi, g = phi * ml, g * ml
        T = dtype(float(phi.sum(dtype=dtype)) / count)
        level_values.append(T)
        value += weights[l - 1] * float(T)
        tx = g * (dy * (icf - iff) + (one - dy) * (icc - ifc))
        ty = g * (dx * (ifc - iff) + (one - dx) * (icc - icf))
        G = np.zeros((n, hl, wl, 2), dtype)
        for c in range(d.shape[3]):                          # channels added in index order
            G[..., 0] = G[..., 0] + tx[..., c]
            G[..., 1] = G[..., 1] + ty[..., c]
        G = np.where(valid[..., None], G, zero)
        G = np.repeat(np.repeat(G, f, axis=1), f, axis=2)
        grad = G if grad is None else grad + G
    return dtype(value), grad, np.array(level_values, dtype)


def multiscale_warp_loss(src, flow, target, levels, level_weights=None, kind=2, grad=None, accumulate=False, stream=None, mask=None):
    """mv3d_multiscale_warp_loss on device memory: the value of multiscale_warp_loss_host and the unweighted T_l, and optionally
    the gradient with respect to the flow.  src / flow / target: graph Tensors (channel views included) or torch device tensors,
    float32 [N,Hs,Ws,C] / [N,H,W,2] / [N,H,W,C].  grad: an optional float32 device tensor of the flow's shape with one pixel stride
    (a channel slice of a dense tensor works); it is overwritten, or added to when accumulate is true.  Asynchronous on `stream`
    (default: torch's current stream of the operands' device).  mask (optional): a graph Tensor or torch device tensor, float32
    [N,H,W,1] over the flow's grid on the flow's device (a channel of a wider tensor works): mv3d_multiscale_warp_loss_masked, the
    masked form multiscale_warp_loss_host states.  Returns (value, level_values): a 0-d and a [levels] device tensor.
    Raises ValueError on what the C entry would refuse."""
    import torch
    from . import _lib, loss_calls
    levels, weights, kind = _multiscale_scalars(levels, level_weights, kind)       # the twin's checks: the same ValueError
    pf, shape, f_ld, dev = _operand(flow, 'flow')
    ps, shape_s, s_ld, dev_s = _operand(src, 'src')
    pt, shape_t, t_ld, dev_t = _operand(target, 'target')
    _multiscale_shapes(shape_s, shape, shape_t, levels)
    if not _same_device(dev_s, dev) or not _same_device(dev_t, dev):
        raise ValueError("multiscale_warp_loss: src on %s, target on %s, flow on %s" % (dev_s, dev_t, dev))
    mask = _mask_operand('multiscale_warp_loss', mask, shape, dev)
    dev = _gpu_device('multiscale_warp_loss', dev)
    grad = _grad_operand('multiscale_warp_loss', grad, 'flow', shape, dev)
    level_values = torch.zeros((levels,), dtype=torch.float32, device=dev)
    lib = _lib.lib()
    src_hwc = (shape_s[1], shape_s[2], shape_t[3])
    out, ws, stream = _launch(dev, loss_calls.multiscale_workspace_bytes(lib, shape[:3], src_hwc, levels), stream)
    loss_calls.multiscale(lib, shape[:3], src_hwc, (ps, s_ld), (pf, f_ld), (pt, t_ld), mask, levels, weights, kind, out.data_ptr(),
                          level_values.data_ptr(), grad, accumulate, False, ws, stream)
    return out, level_values


# ------------------------------------------------------------------------------------------------ census (ternary) loss
CENSUS_MAX_RADIUS = 3


def _census_scalars(max_val, weight, radius, eps):
    """(max_val, weight, radius, eps) with the floats as the C ABI takes them; ValueError on what mv3d_census_loss would refuse."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= CENSUS_MAX_RADIUS:
        raise ValueError("census_loss: radius must be an integer in 1..%d, got %r" % (CENSUS_MAX_RADIUS, radius))
    max_val, weight, eps = (float(np.float32(v)) for v in (max_val, weight, eps))
    if not math.isfinite(max_val) or max_val <= 0:
        raise ValueError("census_loss: max_val must be finite and positive")
    if not math.isfinite(eps) or eps <= 0:
        raise ValueError("census_loss: eps must be finite and positive")
    if not math.isfinite(weight):
        raise ValueError("census_loss: weight must be finite")
    return max_val, weight, int(radius), eps


def _census_shape(shape, shape_b, radius):
    shape, shape_b = tuple(shape), tuple(shape_b)
    if len(shape) != 4 or shape != shape_b:
        raise ValueError("census_loss: operands must be [N,H,W,C] of one shape, got %s and %s" % (shape, shape_b))
    if shape[0] < 1 or not 1 <= shape[3] <= 4:
        raise ValueError("census_loss: needs N >= 1 and C in 1..4, got %s" % (shape,))
    side = 2 * radius + 1
    if shape[1] < side or shape[2] < side:
        raise ValueError("census_loss: images of %d x %d are smaller than the %d x %d patch" % (shape[1], shape[2], side, side))


def census_offsets(radius):
    """The K = (2r+1)^2 - 1 offsets (dy, dx) of the patch, centre excluded, row-major: dy outer, dx inner."""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def census_loss_host(a, b, max_val=1.0, dtype=np.float32, weight=1.0, radius=3, eps=0.01, mask=None):
    """(loss, grad) of the soft census (ternary) loss of Meister et al. ("UnFlow") / Liu et al. ("DDFlow"): loss = weight *
    census_loss, a scalar of `dtype`, and grad = d loss / d a, [N,H,W,C] in `dtype`; every step in `dtype` arithmetic.  At float32
    this states mv3d_census_loss's own operation order (csrc/census_loss.hip); only the sum behind the mean differs (the kernel
    keeps it in double).

    a (prediction) and b (target) [N,H,W,C], C in 1..4; radius r in {1, 2, 3}; K = (2r+1)^2 - 1 offsets o of the (2r+1)^2 patch,
    centre excluded, row-major (dy outer, dx inner); Hv = H - 2r, Wv = W - 2r; a pixel is valid when its whole patch is inside the
    image.
      g_x(p)   = (255 / max_val) (1/C) sum_c x(p,c)        intensity on the 0..255 scale: the constants mean what they mean in the
                                                           literature
      d_x(p,o) = g_x(p+o) - g_x(p)       R_x(p,o) = sqrt(0.81 + d_x^2)       t_x(p,o) = d_x / R_x
      u(p,o)   = t_a - t_b               e = u^2
      dist(p)  = (1/K) sum_o e / (0.1 + e)                 in [0, 1)
      root(p)  = sqrt(dist + eps^2)      rho(p) = dist / (root + eps)        the Charbonnier penalty root - eps, written so that
                                                                             dist == 0 gives exactly 0 whatever the rounding
      census_loss = (1 / (N Hv Wv)) sum over n and the valid p of rho(p)
    Gradient:
      phi(p,o) = [0.1 / (0.1 + e)^2] 2 u 0.81 / R_a^3      rho'(p) = 1 / (2 root(p))
      dL/dg_a(q) = (1 / (K N Hv Wv)) ( sum_{o : q-o valid} rho'(q-o) phi(q-o, o) - [q valid] rho'(q) sum_o phi(q, o) )
      grad(q,c)  = weight (255 / (max_val C)) dL/dg_a(q)   the same for every channel c
    Pixels outside the valid region still receive a gradient as neighbours.  a == b gives a loss of exactly 0 and a gradient of
    exactly 0, because u == 0.

    Order of the steps: the channels of g are added in index order and scaled by 255 / (max_val C) rounded once; dist adds its K
    terms in offset order and multiplies by 1/K rounded once; phi = (0.162 u) / ((0.1 + e)^2 (R_a R_a R_a)); the second sum of
    the bracket runs in offset order and the first in reverse offset order (the order in which a kernel that gathers at q meets
    them: phi(q-o, o) == -phi(q, -o) exactly); the bracket is first - rho'(q) * second, times weight 255 / (max_val C K N Hv Wv)
    rounded once.

    mask (None = the code above, untouched): m [N,H,W,1], any finite values, never differentiated, indexed by the pixel of a and
    read only at valid pixels (mv3d_census_loss_masked):
      census_loss_masked = (1 / (N Hv Wv)) sum over n and the valid p of m(p) rho(p)     the count stays N Hv Wv, as
                                                                                         masked_euclidean_loss keeps its mean
    The product m(p) * rho(p) is formed first, then summed (the kernel adds it into its double sum).  In the gradient rho'(p)
    becomes (0.5 / root(p)) * m(p), one multiply; everything behind it is unchanged, so a masked pixel still receives a gradient
    as the neighbour of a visible one.  m == 1 gives the unmasked numbers bit for bit, m == 0 gives (0, zeros), a == b gives
    exactly 0 under any mask, and both results are linear in m."""
    dtype = np.dtype(dtype).type
    max_val, weight, r, eps = _census_scalars(max_val, weight, radius, eps)
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    _census_shape(a.shape, b.shape, r)
    n, h, w, c = a.shape
    hv, wv = h - 2 * r, w - 2 * r
    offsets = census_offsets(r)
    k = len(offsets)
    count = float(n) * hv * wv
    gs = dtype(255.0 / (max_val * c))
    c81, c01, c162, half = dtype(0.81), dtype(0.1), dtype(0.162), dtype(0.5)

    def gray(x):
        s = x[..., 0]
        for ch in range(1, c):                               # channels added in index order
            s = s + x[..., ch]
        return s * gs

    ga, gb = gray(a), gray(b)
    ca, cb = ga[:, r:r + hv, r:r + wv], gb[:, r:r + hv, r:r + wv]
    acc = np.zeros((n, hv, wv), dtype)
    phi = []
    for dy, dx in offsets:
        da = ga[:, r + dy:r + dy + hv, r + dx:r + dx + wv] - ca
        db = gb[:, r + dy:r + dy + hv, r + dx:r + dx + wv] - cb
        ra, rb = np.sqrt(da * da + c81), np.sqrt(db * db + c81)
        u = da / ra - db / rb
        e = u * u
        den = c01 + e
        acc = acc + e / den
        phi.append((u * c162) / ((den * den) * ((ra * ra) * ra)))
    dist = acc * dtype(1.0 / k)
    eps_t = dtype(eps)
    root = np.sqrt(dist + eps_t * eps_t)
    rho = dist / (root + eps_t)
    dr = half / root
    if mask is not None:
        mv = _host_mask('census_loss', mask, a.shape, dtype)[:, r:r + hv, r:r + wv]
        rho = mv * rho
        dr = dr * mv
    loss = dtype(weight * (float(rho.sum(dtype=dtype)) / count))
    second = np.zeros((n, hv, wv), dtype)
    for f in phi:
        second = second + f
    first = np.zeros((n, h, w), dtype)
    for (dy, dx), f in reversed(list(zip(offsets, phi))):
        first[:, r + dy:r + dy + hv, r + dx:r + dx + wv] = first[:, r + dy:r + dy + hv, r + dx:r + dx + wv] + dr * f
    first[:, r:r + hv, r:r + wv] = first[:, r:r + hv, r:r + wv] - dr * second
    grad = first * dtype(weight * 255.0 / (max_val * c) / (k * count))
    return loss, np.ascontiguousarray(np.broadcast_to(grad[..., None], a.shape))


def census_loss(a, b, max_val=1.0, weight=1.0, radius=3, eps=0.01, grad=None, accumulate=False, stream=None, mask=None):
    """mv3d_census_loss on device memory: weight * census_loss of a (the prediction) against b (the target), and optionally its
    gradient with respect to a.  mask (None = mv3d_census_loss, exactly as before): a float32 [N,H,W,1] graph Tensor or torch
    device tensor (a channel of a wider tensor works); the call is then mv3d_census_loss_masked (census_loss_host states the
    definition).  a / b: graph Tensors (channel views included) or torch device tensors, [N,H,W,C] float32, with the
    operand rules of image_metrics.  grad: an optional float32 device tensor of a's shape with one pixel stride (a channel slice of
    a dense tensor works); it is overwritten, or added to when accumulate is true.  Asynchronous on `stream` (default: torch's
    current stream of the operands' device).  Returns the loss as a 0-d device tensor."""
    from . import _lib, loss_calls
    pa, pb, shape, dev = _image_pair('census_loss', a, b)
    grad = _grad_operand('census_loss', grad, 'pred', shape, dev)
    mask = _mask_operand('census_loss', mask, shape, dev)
    lib = _lib.lib()
    out, ws, stream = _launch(dev, loss_calls.census_workspace_bytes(lib, shape, radius), stream)
    loss_calls.census(lib, shape, pa, pb, mask, radius, max_val, eps, weight, out.data_ptr(), grad, accumulate, ws, stream)
    return out
