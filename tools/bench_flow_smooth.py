#!/usr/bin/env python
"""Micro-benchmark of the flow smoothness loss (mv3d_flow_smoothness; GPU only): python tools/bench_flow_smooth.py [--iters K] [--repeats R]

Per workload shape the calls are timed side by side: mv3d_flow_smoothness guided by a 3-channel image and unguided, each with
value + gradient (store), value + gradient (accumulate), value only and gradient only, and mv3d_pixel_loss (L2 with gradient) on
a same-sized two-channel tensor as the yardstick of an HBM-bound single-pass loss.  After 10 warm-up calls each, R rounds run; a
round times K back-to-back calls of each entry between device events, one after the other, so that a drift of the machine hits
all alike.  The figure is the median round's time per call (one call = the tile launch + the final launch where there is a
value).  GB/s is over the algorithmic bytes per pixel: 8 of flow, 4 * Cg of guide, 8 of gradient written (16 when it accumulates);
for the pixel loss 16 read and 8 written.

Then one AppearanceFlowModel step at batch 64 is timed with and without conf['flow_smoothness_weight'], with a host clock around
a device synchronise.  Each model runs in a child process of its own (one at a time, each under --step-timeout), the two kinds
alternating (--step-rounds of each): identical models built in one process differ in step time by more than the two short
launches the term adds at the end of the forward plan (measured: 1657 and 1803 us).  The head stays fused."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dynamic_multiview_3d_amd import _lib
from tools.bench_ssim_loss import alternating, timed_us_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--step-iters', type=int, default=10)
    ap.add_argument('--step-repeats', type=int, default=15)
    ap.add_argument('--step-rounds', type=int, default=4)
    ap.add_argument('--step-timeout', type=float, default=180.0, help="seconds one child process may take (a run takes about 10)")
    ap.add_argument('--step-weight', type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--no-step', action='store_true', help="kernels only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flow_smooth needs a GPU"
    if args.step_weight is not None:
        return step_child(args.step_weight, args.step_iters, args.step_repeats)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for n, h, w in [(64, 128, 128), (32, 256, 256)]:
        flow = torch.rand((n, h, w, 2), device='cuda') * 6 - 3
        other = torch.rand((n, h, w, 2), device='cuda')
        guide = torch.rand((n, h, w, 3), device='cuda')
        grad = torch.zeros((n, h, w, 2), device='cuda')
        loss = torch.zeros(1, device='cuda')
        nb = int(lib.flow_smoothness_workspace_bytes(n, h, w))
        ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
        px = float(n * h * w)

        def smooth(cg, want_loss, want_grad, acc):
            return lambda: lib.flow_smoothness(n, h, w, flow.data_ptr(), 2, guide.data_ptr() if cg else None, cg, cg, 10.0, 1e-3, 1e-6,
                                               loss.data_ptr() if want_loss else None, grad.data_ptr() if want_grad else None, 2, acc,
                                               ws.data_ptr(), nb, st)
        fns, nbytes = {}, {}
        for cg in (3, 0):
            tag = 'guided Cg=3' if cg else 'unguided'
            for name, (wl, wg, acc) in (('value+grad', (True, True, 0)), ('value+grad accumulate', (True, True, 1)),
                                        ('value', (True, False, 0)), ('grad', (False, True, 0))):
                fns['flow_smoothness %s %s' % (tag, name)] = smooth(cg, wl, wg, acc)
                nbytes['flow_smoothness %s %s' % (tag, name)] = px * (8 + 4 * cg + (0 if not wg else 16 if acc else 8))
        fns['pixel_loss L2+grad'] = lambda: lib.pixel_loss(n * h * w, 2, flow.data_ptr(), other.data_ptr(), None, 2, 1.0, loss.data_ptr(),
                                                           grad.data_ptr(), st)
        nbytes['pixel_loss L2+grad'] = px * 24
        for k, (med, lo, hi) in alternating(fns, args.iters, args.repeats).items():
            print(json.dumps({'op': k, 'shape': [n, h, w], 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                              'MB': round(nbytes[k] / 1e6, 2), 'GB/s': round(nbytes[k] / med / 1e3, 1)}), flush=True)
    if args.no_step:
        return

    import subprocess
    times = {0.0: [], 0.1: []}
    launches = {}
    for _ in range(args.step_rounds):
        for w in times:                          # one child at a time: a fresh process, a fresh device context
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--step-weight', str(w), '--step-iters', str(args.step_iters),
                                  '--step-repeats', str(args.step_repeats)], check=True, capture_output=True, text=True,
                                 timeout=args.step_timeout).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            times[w].append(rec['us'])
            launches[w] = rec['launches']
    med = {w: float(np.median(v)) for w, v in times.items()}
    for w, v in times.items():
        print(json.dumps({'op': 'AppearanceFlowModel.train_step', 'loss': 'L2 + %g smoothness' % w if w else 'L2', 'batch': 64,
                          'us': round(med[w], 1), 'us_min': round(min(v), 1), 'us_max': round(max(v), 1), 'processes': len(v),
                          'launches': launches[w]}), flush=True)
    d = med[0.1] - med[0.0]
    print(json.dumps({'op': 'step delta', 'us': round(d, 1), 'percent': round(100.0 * d / med[0.0], 2)}), flush=True)


def step_child(weight, iters, repeats):
    """One model, one process: the median over `repeats` groups of `iters` steps."""
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.train import SyntheticData
    conf = dict({'batch_size': 64, 'learning_rate': 1e-4}, **({'flow_smoothness_weight': weight} if weight else {}))
    m = AppearanceFlowModel(conf, load_tfrec=False, device='cuda')
    m.feed(**SyntheticData(m, pool=1).next())
    med, lo, hi = alternating({'step': m.graph.train_step}, iters, repeats, warmup=10, timer=timed_us_host)['step']
    print(json.dumps({'us': med, 'us_min': lo, 'us_max': hi, 'launches': [m.graph.n_launch_fwd, m.graph.n_launch_bwd_fused]}), flush=True)


if __name__ == '__main__':
    main()
