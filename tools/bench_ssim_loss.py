#!/usr/bin/env python
"""Micro-benchmark of the SSIM training loss (mv3d_ssim_loss; GPU only): python tools/bench_ssim_loss.py [--iters K] [--repeats R]

Per workload shape three calls are timed side by side: mv3d_ssim_loss with its gradient, mv3d_ssim_loss value only, and
mv3d_image_metrics -- the forward half alone -- as the yardstick.  After 10 warm-up calls each, R rounds run; a round times K
back-to-back calls of each of the three between device events, one after the other, so that a drift of the machine hits all
three alike.  The figure is the median round's time per call (one call = the tile launch + the final launch).  GB/s is over the
algorithmic bytes: the two images read once (2*N*H*W*C*4), plus the gradient written once (N*H*W*C*4) when it is asked for.

Then one AppearanceFlowModel step at batch 64 is timed with and without conf['ssim_loss_weight'], alternating groups of steps of
the two models in the same way, with a host clock around a device synchronise.  With the term the appearance-flow head runs unfused (resample forward, pixel loss, SSIM loss,
resample backward instead of one launch), so the difference is more than the loss kernel's own time."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dynamic_multiview_3d_amd import _lib


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed_us_host(fn, iters):
    """A host clock around work that ends in a device synchronise: a train step uses side streams, which events on the main
    stream do not cover."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def alternating(fns, iters, repeats, warmup=10, timer=timed_us):
    """{name: (median, min, max) us per call}; every round times each entry once, in order."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(timer(fn, iters))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--step-repeats', type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim_loss needs a GPU"
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for n, h, w, c in [(64, 128, 128, 3), (32, 256, 256, 3)]:
        a, b = torch.rand((n, h, w, c), device='cuda'), torch.rand((n, h, w, c), device='cuda')
        grad = torch.empty((n, h, w, c), device='cuda')
        loss = torch.zeros(1, device='cuda')
        out = torch.empty((n, 3), device='cuda')
        nb = int(lib.ssim_loss_workspace_bytes(n, h, w, c))
        ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
        nbm = int(lib.image_metrics_workspace_bytes(n, h, w, c))
        wsm = torch.empty(nbm, dtype=torch.uint8, device='cuda')
        image_bytes = 2.0 * n * h * w * c * 4
        fns = {
            'ssim_loss+grad': lambda: lib.ssim_loss(n, h, w, c, a.data_ptr(), c, b.data_ptr(), c, 1.0, 1.0, loss.data_ptr(), grad.data_ptr(), c, 0,
                                                    ws.data_ptr(), nb, st),
            'ssim_loss value': lambda: lib.ssim_loss(n, h, w, c, a.data_ptr(), c, b.data_ptr(), c, 1.0, 1.0, loss.data_ptr(), None, c, 0,
                                                     ws.data_ptr(), nb, st),
            'image_metrics': lambda: lib.image_metrics(n, h, w, c, a.data_ptr(), c, b.data_ptr(), c, 1.0, out.data_ptr(), wsm.data_ptr(), nbm, st),
        }
        nbytes = {'ssim_loss+grad': image_bytes * 1.5, 'ssim_loss value': image_bytes, 'image_metrics': image_bytes}
        for k, (med, lo, hi) in alternating(fns, args.iters, args.repeats).items():
            print(json.dumps({'op': k, 'shape': [n, h, w, c], 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                              'MB': round(nbytes[k] / 1e6, 2), 'GB/s': round(nbytes[k] / med / 1e3, 1)}), flush=True)

    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.train import SyntheticData
    models = {}
    for name, extra in (('L2', {}), ('L2 + 0.5 SSIM', {'ssim_loss_weight': 0.5})):
        m = AppearanceFlowModel(dict({'batch_size': 64, 'learning_rate': 1e-4}, **extra), load_tfrec=False, device='cuda')
        m.feed(**SyntheticData(m, pool=1).next())
        models[name] = m
    res = alternating({k: m.graph.train_step for k, m in models.items()}, args.step_iters, args.step_repeats, warmup=5, timer=timed_us_host)
    for k, (med, lo, hi) in res.items():
        g = models[k].graph
        print(json.dumps({'op': 'AppearanceFlowModel.train_step', 'loss': k, 'batch': 64, 'us': round(med, 1), 'us_min': round(lo, 1),
                          'us_max': round(hi, 1), 'launches': [g.n_launch_fwd, g.n_launch_bwd]}), flush=True)
    d = res['L2 + 0.5 SSIM'][0] - res['L2'][0]
    print(json.dumps({'op': 'step delta', 'us': round(d, 1), 'percent': round(100.0 * d / res['L2'][0], 2)}), flush=True)


if __name__ == '__main__':
    main()
