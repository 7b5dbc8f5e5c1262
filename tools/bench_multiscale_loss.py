"""Times mv3d_multiscale_warp_loss at the training shape (B = 64, 128 x 128, C = 3, L = 3) in its three modes, and the B = 64
train step of AppearanceFlowModel with conf['multiscale_loss_levels'] = 3 against the same step without it.

Algorithmic bytes of one call, px = B H W full-resolution pixels, r = 1/4 + 1/16 + 1/64 the pyramid's share of an image:
  flow read once                       8 px
  grad read and written once           16 px  (8 px when it is stored; 0 for a value-only call)
  src and target read once             2 * 4 C px             (not with pyramid_ready)
  the pyramids written                 2 * 4 C r px           (not with pyramid_ready)
  ... and read again by the loss pass  2 * 4 C r px
The per-tile sums (24 bytes per 32 x 32 tile) are left out.

usage: python tools/bench_multiscale_loss.py [--iters 200] [--no-step]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from dynamic_multiview_3d_amd import _lib      # noqa: E402


def call_bytes(px, c, levels, value, grad, accumulate, ready):
    r = sum(0.25 ** l for l in range(1, levels + 1))
    b = 8.0 * px + (16.0 if accumulate else 8.0) * px * (1 if grad else 0) + 2 * 4.0 * c * r * px
    if not ready:
        b += 2 * 4.0 * c * px + 2 * 4.0 * c * r * px
    return b


def time_us(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    lib = _lib.lib()
    n, h, w, c, levels = 64, 128, 128, 3, 3
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.uniform(0, 1, (n, h, w, c)).astype(np.float32)).cuda()
    tgt = torch.from_numpy(rng.uniform(0, 1, (n, h, w, c)).astype(np.float32)).cuda()
    flow = torch.from_numpy(rng.uniform(-3, 3, (n, h, w, 2)).astype(np.float32)).cuda()
    grad = torch.zeros_like(flow)
    loss = torch.zeros(1, device='cuda')
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, w, h, w, c, levels))
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    wts = (ctypes.c_float * levels)(1.0, 0.5, 0.25)
    stream = torch.cuda.current_stream().cuda_stream

    def run(value, g, accumulate, ready):
        lib.multiscale_warp_loss(n, h, w, h, w, c, src.data_ptr(), c, flow.data_ptr(), 2, tgt.data_ptr(), c, levels, wts, 2,
                                 loss.data_ptr() if value else None, None, grad.data_ptr() if g else None, 2, 1 if accumulate else 0,
                                 1 if ready else 0, ws.data_ptr(), nb, stream)
    px = float(n * h * w)
    for name, mode in (('value + gradient (added)', (True, True, True, False)), ('value only', (True, False, False, False)),
                       ('gradient only, pyramid_ready', (False, True, True, True))):
        run(True, False, False, False)          # the pyramids are in the workspace
        us = time_us(lambda: run(*mode), args.iters)
        by = call_bytes(px, c, levels, *mode)
        print('%-32s %8.2f us  %7.2f MB  %7.1f GB/s' % (name, us, by / 1e6, by / us / 1e3))
    if args.no_step:
        return
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.train import SyntheticData
    for label, extra in (('step, switch off', {}), ('step, L = 3', {'multiscale_loss_levels': 3, 'multiscale_loss_weight': [1.0, 0.5, 0.25]})):
        model = AppearanceFlowModel(dict({'batch_size': 64, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cuda')
        data = SyntheticData(model, seed=1)
        model.train_step(**data.next())
        us = time_us(lambda: model.train_step(), max(args.iters // 4, 20))
        print('%-32s %8.1f us' % (label, us))


if __name__ == '__main__':
    main()
