#!/usr/bin/env python
"""What the EMA of the weights costs on one GPU, against what the project already ships.

kernel: mv3d_ema_step and, in the same process and alternating with it, mv3d_sgd_step without a momentum slot (gradient descent:
        the same 12 B/param -- two loads, one store -- and the same access pattern) over the benchmarked model's 69 535 232 floats:
        warm-up, then --launches launches per sample between two HIP events, --samples samples each.  Bar: median EMA time <=
        median GD time + the GD samples' own max - min.
step:   AppearanceFlowModel at batch 64 with and without conf['ema_decay'], two models in one process, alternating blocks of
        --steps train steps, --samples blocks each.  Bar: (on - off) <= the summed alone-time of the step's EMA launches (each
        range timed like the kernel above) + the off blocks' max - min: the placement must not cost more than running the
        launches serially would.

    python tools/bench_ema.py [--only kernel,step] [--launches 200] [--steps 200] [--samples 5] [--batch 64]

One JSON line per measurement.
"""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synth_batch

FLAT = 69535232             # AppearanceFlowModel's flat parameter buffer
COPY_TBS = 6.29             # measured float4 copy rate of the MI355X, TB/s


def _timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def _stats(ms, count):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    gbs = 12.0 * count / (med * 1e-3) / 1e9
    return {"ms": {"median": round(med, 5), "min": round(ms[0], 5), "max": round(ms[-1], 5)}, "GB/s": round(gbs, 1),
            "share_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3)}


def time_kernels(lib, count, launches, samples, with_gd=True):
    """[ema samples], [gd samples] in ms per launch, alternating sample by sample."""
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device='cuda').manual_seed(0)
    s, p, g = (torch.randn(count, device='cuda', generator=gen) for _ in range(3))
    g.mul_(1e-3)
    w = float(np.float32(1 - 0.999))
    ema = lambda: lib.ema_step(count, s.data_ptr(), p.data_ptr(), w, st)
    gd = lambda: lib.sgd_step(count, p.data_ptr(), g.data_ptr(), None, 1e-4, 0.0, 0, 1.0, st)
    for fn in (ema, gd):
        _timed(fn, 20)
    t_ema, t_gd = [], []
    for _ in range(samples):
        t_ema.append(_timed(ema, launches))
        if with_gd:
            t_gd.append(_timed(gd, launches))
    return t_ema, t_gd


def bench_kernel(args):
    from dynamic_multiview_3d_amd import _lib
    t_ema, t_gd = time_kernels(_lib.lib(), FLAT, args.launches, args.samples)
    ema, gd = _stats(t_ema, FLAT), _stats(t_gd, FLAT)
    spread = gd["ms"]["max"] - gd["ms"]["min"]
    return {"bench": "ema_kernel", "floats": FLAT, "bytes": 12 * FLAT, "launches": args.launches, "samples": args.samples,
            "ema": ema, "gd": gd, "bar_ms": round(gd["ms"]["median"] + spread, 5),
            "bar_met": bool(ema["ms"]["median"] <= gd["ms"]["median"] + spread)}


def _ema_ranges(g):
    out, at = [], 0
    for a, b in g._fc_ranges:
        if a > at:
            out.append((at, a))
        out.append((a, b))
        at = b
    if at < g.flat_size:
        out.append((at, g.flat_size))
    return out


def bench_step(args):
    from dynamic_multiview_3d_amd import _lib
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    models = {}
    for name, extra in (('off', {}), ('on', {'ema_decay': 0.999})):
        conf = dict({'batch_size': args.batch, 'learning_rate': 1e-4, 'experiment_name': 'appflow_offset'}, **extra)
        m = AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda', seed=1234)
        m.feed(**synth_batch(np.random.default_rng(0), args.batch))
        for _ in range(10):
            m.graph.train_step()
        models[name] = m
    ranges = _ema_ranges(models['on'].graph)
    alone = []
    for lo, hi in ranges:
        t, _ = time_kernels(_lib.lib(), hi - lo, args.launches, args.samples, with_gd=False)
        alone.append(sorted(t)[len(t) // 2])
    gc.collect()
    gc.disable()
    ms = {'off': [], 'on': []}
    for _ in range(args.samples):
        for name in ('off', 'on'):
            ms[name].append(_timed(models[name].graph.train_step, args.steps))
    gc.enable()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    spread = max(ms['off']) - min(ms['off'])
    over = med['on'] - med['off']
    return {"bench": "ema_step", "batch": args.batch, "steps_per_block": args.steps, "blocks": args.samples,
            "step_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
            "images_per_sec": {k: round(args.batch / (med[k] * 1e-3), 1) for k in ms},
            "overhead_ms": round(over, 4), "ema_ranges": [hi - lo for lo, hi in ranges],
            "ema_alone_ms": [round(t, 5) for t in alone], "bar_ms": round(sum(alone) + spread, 4),
            "bar_met": bool(over <= sum(alone) + spread)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--only', default='kernel,step')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    for name in [s for s in args.only.split(',') if s]:
        print(json.dumps({'kernel': bench_kernel, 'step': bench_step}[name](args)), flush=True)


if __name__ == '__main__':
    main()
