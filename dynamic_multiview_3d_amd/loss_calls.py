"""The library calls of the loss kernels that have a recorded caller (the LossTerm classes of graph.py) and an eager one (the
wrappers of metrics.py): one function per family, the only place that lays out the positional arguments of its entry
(include/mv3d_hip.h) and that chooses between an entry and its masked form (for the flow smoothness: between the first- and the second-order entry).

Operands arrive resolved.  `lib` is _lib.lib().  An operand is its (address, pixel stride) pair, or None where it is optional and
absent: `mask` (None = the unmasked entry; a pair is spliced into the same argument list, behind the operands, for the masked entry),
`grad` (None = no gradient; the stride passed is then the dense one), `guide`, a (address, channels, pixel stride) triple.  `loss`,
`level_values` and `stats` are addresses or None, `ws` is the (address, bytes) pair of the workspace and `stream` a raw handle.
"""
import ctypes


def _grad(grad, dense_ld):
    return grad if grad is not None else (None, dense_ld)


def ssim_workspace_bytes(lib, shape, masked):
    return int((lib.ssim_loss_masked_workspace_bytes if masked else lib.ssim_loss_workspace_bytes)(*shape))


def ssim(lib, shape, a, b, mask, max_val, weight, loss, grad, accumulate, ws, stream):
    """mv3d_ssim_loss / mv3d_ssim_loss_masked over a, b of shape (N, H, W, C)."""
    head, tail = (*shape, *a, *b), (float(max_val), float(weight), loss, *_grad(grad, shape[3]), 1 if accumulate else 0, *ws, stream)
    return lib.ssim_loss(*head, *tail) if mask is None else lib.ssim_loss_masked(*head, *mask, *tail)


def census_workspace_bytes(lib, shape, radius):
    return int(lib.census_loss_workspace_bytes(*shape, int(radius)))            # the masked form takes the same workspace


def census(lib, shape, a, b, mask, radius, max_val, eps, weight, loss, grad, accumulate, ws, stream):
    """mv3d_census_loss / mv3d_census_loss_masked over a, b of shape (N, H, W, C)."""
    head = (*shape, *a, *b)
    tail = (int(radius), float(max_val), float(eps), float(weight), loss, *_grad(grad, shape[3]), 1 if accumulate else 0, *ws, stream)
    return lib.census_loss(*head, *tail) if mask is None else lib.census_loss_masked(*head, *mask, *tail)


def flow_smoothness_workspace_bytes(lib, nhw, order=1):
    return int((lib.flow_smoothness2_workspace_bytes if order == 2 else lib.flow_smoothness_workspace_bytes)(*nhw))


def flow_smoothness(lib, nhw, flow, guide, edge_alpha, eps, weight, loss, grad, accumulate, ws, stream, order=1):
    """mv3d_flow_smoothness (order 1) / mv3d_flow_smoothness2 (order 2) of a flow over (N, H, W): one argument list."""
    entry = lib.flow_smoothness2 if order == 2 else lib.flow_smoothness
    entry(*nhw, *flow, *(guide if guide is not None else (None, 0, 0)), float(edge_alpha), float(eps), float(weight),
          loss, *_grad(grad, 2), 1 if accumulate else 0, *ws, stream)


def multiscale_workspace_bytes(lib, nhw, src_hwc, levels):
    return int(lib.multiscale_warp_loss_workspace_bytes(*nhw, *src_hwc, int(levels)))       # the masked form takes the same workspace


def multiscale(lib, nhw, src_hwc, src, flow, target, mask, levels, weights, kind, loss, level_values, grad, accumulate, reuse, ws, stream):
    """mv3d_multiscale_warp_loss / mv3d_multiscale_warp_loss_masked of a flow over (N, H, W) that warps src, (Hs, Ws, C), onto
    target; `weights`: one float per level; reuse: the workspace already holds this call's pyramids."""
    head = (*nhw, *src_hwc, *src, *flow, *target)
    tail = (int(levels), (ctypes.c_float * levels)(*weights), int(kind), loss, level_values, *_grad(grad, 2), 1 if accumulate else 0,
            1 if reuse else 0, *ws, stream)
    return lib.multiscale_warp_loss(*head, *tail) if mask is None else lib.multiscale_warp_loss_masked(*head, *mask, *tail)


def flow_consistency_workspace_bytes(lib, nhw):
    return int(lib.flow_consistency_workspace_bytes(*nhw))


def flow_consistency(lib, nhw, flow, eps, weight, loss, stats, grad, accumulate, ws, stream):
    """mv3d_flow_consistency of a pair-swapped batch of flows over (N, H, W)."""
    lib.flow_consistency(*nhw, *flow, float(eps), float(weight), loss, stats, *_grad(grad, 2), 1 if accumulate else 0, *ws, stream)
