#!/usr/bin/env python
"""Train-step rate of the headline configuration (AppearanceFlowModel, 128 x 128, batch 64, one GPU) under each optimiser:
Adam, Momentum, Momentum + Nesterov, gradient descent.  bench.py's method -- synthetic batch resident in HBM, warm-up steps, then
timed steps between HIP events on the main stream, no cyclic GC in the timed region -- and one JSON line per optimiser.

    python tools/bench_optimizers.py [--steps 30] [--warmup 5] [--batch 64]
"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synth_batch

OPTIMIZERS = [('adam', {}), ('momentum', dict(optimizer='momentum', momentum=0.9)),
              ('momentum_nesterov', dict(optimizer='momentum', momentum=0.9, use_nesterov=True)), ('sgd', dict(optimizer='sgd'))]


def run(name, extra, args):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    conf = dict({'batch_size': args.batch, 'learning_rate': 1e-4, 'experiment_name': 'appflow_offset'}, **extra)
    model = AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda', seed=1234)
    g = model.graph
    model.feed(**synth_batch(np.random.default_rng(0), args.batch))
    for _ in range(args.warmup):
        g.train_step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(args.steps):
        g.train_step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc.enable()
    step_ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
    slots = sum(t.numel() for t in (g.adam_m, g.adam_v, g.accum) if t is not None)
    out = {"optimizer": name, "value": round(args.batch * args.steps / elapsed, 2), "unit": "images/sec",
           "step_ms": {"mean": round(1e3 * elapsed / args.steps, 4), "median": round(step_ms[len(step_ms) // 2], 4),
                       "min": round(step_ms[0], 4), "max": round(step_ms[-1], 4)},
           "launches_per_step": g.n_launch_fwd + g.n_launch_bwd_fused + (3 if g.optimizer == 'adam' else 1),
           "slot_bytes": 4 * slots, "loss": round(float(g.loss_buf[0]), 6), "batch": args.batch, "steps": args.steps,
           "warmup": args.warmup}
    del model, g
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--only', default='', help='comma-separated list (run in that order, repeats allowed) of ' +
                    ', '.join(n for n, _ in OPTIMIZERS))
    args = ap.parse_args()
    kinds = dict(OPTIMIZERS)
    for name in [s for s in args.only.split(',') if s] or list(kinds):
        print(json.dumps(run(name, kinds[name], args)), flush=True)


if __name__ == '__main__':
    main()
