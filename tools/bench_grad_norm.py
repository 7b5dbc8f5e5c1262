#!/usr/bin/env python
"""What global-norm gradient clipping costs on one GPU, against what the project already ships.

kernel: both launches of mv3d_grad_clip_scale together and, in the same process and alternating with them, mv3d_ema_step over the
        same count -- the benchmarked model's 69 535 232 floats: warm-up, then --launches calls per sample between two HIP events,
        --samples samples each.  The norm pass reads 4 B/element, the EMA moves 12.  Bar: median norm time <= median EMA time +
        the EMA samples' own max - min (slower than a kernel that moves three times the bytes means it is not streaming).
step:   AppearanceFlowModel at batch 64, three models in one process, alternating blocks of --steps train steps, --samples blocks
        each: `on` (conf['grad_clip_norm']), `plain` (no key, MV3D_FUSE_FC_ADAM=0 MV3D_FUSE_FINALIZE=0 MV3D_OVERLAP_ADAM=0: the
        same launches without the norm) and `fused` (no key, the default schedule: what a user gives up by switching clipping on).
        Bar: (on - plain) <= the kernel-alone time + the plain blocks' max - min.

    python tools/bench_grad_norm.py [--only kernel,step] [--launches 200] [--steps 200] [--samples 5] [--batch 64]

One JSON line per measurement.
"""
import argparse
import gc
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synth_batch

FLAT = 69535232             # AppearanceFlowModel's flat parameter buffer
COPY_TBS = 6.29             # measured float4 copy rate of the MI355X, TB/s
PLAIN = {'MV3D_FUSE_FC_ADAM': '0', 'MV3D_FUSE_FINALIZE': '0', 'MV3D_OVERLAP_ADAM': '0'}


def _timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def _stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    gbs = nbytes / (med * 1e-3) / 1e9
    return {"ms": {"median": round(med, 5), "min": round(ms[0], 5), "max": round(ms[-1], 5)}, "GB/s": round(gbs, 1),
            "share_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3)}


def time_kernels(lib, count, launches, samples, with_ema=True):
    """[norm samples], [ema samples] in ms per call, alternating sample by sample."""
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device='cuda').manual_seed(0)
    s, p, g = (torch.randn(count, device='cuda', generator=gen) for _ in range(3))
    g.mul_(1e-3)
    out = torch.zeros(2, device='cuda')
    state = torch.zeros(16, device='cuda')
    nbytes = int(lib.grad_clip_workspace_bytes(count))
    ws = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device='cuda')
    w = float(np.float32(1 - 0.999))
    norm = lambda: lib.grad_clip_scale(count, g.data_ptr(), 1.0, 1.0, out.data_ptr(), state.data_ptr(), state.data_ptr() + 32,
                                       ws.data_ptr(), nbytes, st)
    ema = lambda: lib.ema_step(count, s.data_ptr(), p.data_ptr(), w, st)
    for fn in (norm, ema):
        _timed(fn, 20)
    t_norm, t_ema = [], []
    for _ in range(samples):
        t_norm.append(_timed(norm, launches))
        if with_ema:
            t_ema.append(_timed(ema, launches))
    return t_norm, t_ema


def bench_kernel(args):
    from dynamic_multiview_3d_amd import _lib
    t_norm, t_ema = time_kernels(_lib.lib(), FLAT, args.launches, args.samples)
    norm, ema = _stats(t_norm, 4 * FLAT), _stats(t_ema, 12 * FLAT)
    spread = ema["ms"]["max"] - ema["ms"]["min"]
    return {"bench": "grad_norm_kernel", "floats": FLAT, "bytes": 4 * FLAT, "launches": args.launches, "samples": args.samples,
            "norm": norm, "ema": ema, "bar_ms": round(ema["ms"]["median"] + spread, 5),
            "bar_met": bool(norm["ms"]["median"] <= ema["ms"]["median"] + spread)}


def bench_step(args):
    from dynamic_multiview_3d_amd import _lib
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    models = {}
    for name, env, extra in (('plain', PLAIN, {}), ('on', {}, {'grad_clip_norm': args.clip}), ('fused', {}, {})):
        for k in PLAIN:
            os.environ[k] = env.get(k, '1')
        conf = dict({'batch_size': args.batch, 'learning_rate': 1e-4, 'experiment_name': 'appflow_offset'}, **extra)
        m = AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda', seed=1234)
        m.feed(**synth_batch(np.random.default_rng(0), args.batch))
        for _ in range(10):
            m.graph.train_step()
        models[name] = m
    g = models['on'].graph
    t, _ = time_kernels(_lib.lib(), g.flat_size, args.launches, args.samples, with_ema=False)
    alone = sorted(t)[len(t) // 2]
    gc.collect()
    gc.disable()
    ms = {k: [] for k in models}
    for _ in range(args.samples):
        for name in models:
            ms[name].append(_timed(models[name].graph.train_step, args.steps))
    gc.enable()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    spread = max(ms['plain']) - min(ms['plain'])
    over = med['on'] - med['plain']
    norm, scale = g.grad_norm().tolist()
    return {"bench": "grad_norm_step", "batch": args.batch, "steps_per_block": args.steps, "blocks": args.samples,
            "step_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
            "images_per_sec": {k: round(args.batch / (med[k] * 1e-3), 1) for k in ms},
            "overhead_ms": round(over, 4), "norm_alone_ms": round(alone, 5), "bar_ms": round(alone + spread, 4),
            "bar_met": bool(over <= alone + spread), "given_up_vs_fused_ms": round(med['on'] - med['fused'], 4),
            "last_grad_norm": norm if math.isfinite(norm) else str(norm), "last_clip_scale": scale}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--only', default='kernel,step')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--clip', type=float, default=1.0, help="conf['grad_clip_norm'] of the clipped model")
    args = ap.parse_args()
    for name in [s for s in args.only.split(',') if s]:
        print(json.dumps({'kernel': bench_kernel, 'step': bench_step}[name](args)), flush=True)


if __name__ == '__main__':
    main()
