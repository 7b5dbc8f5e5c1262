#!/usr/bin/env python
"""What gradient accumulation costs on one GPU, against what the project already ships.

kernel: mv3d_grad_accumulate in its three modes and, in the same process and alternating with them sample by sample,
        mv3d_ema_step over the same count -- the benchmarked model's 69 535 232 floats: warm-up, then --launches calls per
        sample between two HIP events, --samples samples each.  ADD, FINISH and the EMA move 12 B/element, STORE 8.  Bar: median
        ADD and FINISH time <= median EMA time + the EMA samples' own max - min.
norm:   FINISH with partials + mv3d_grad_clip_finish against FINISH without partials + mv3d_grad_clip_scale, alternating.  The
        fused pair must be faster; the difference is what the norm's 4 B/element read pass cost.
step:   AppearanceFlowModel at micro-batch 64, three models in one process, alternating blocks, --samples blocks each: `accum`
        (conf['grad_accum_steps'] = --accum: a block is --steps cycles), `plain` (no key, MV3D_FUSE_FC_ADAM=0
        MV3D_FUSE_FINALIZE=0 MV3D_OVERLAP_ADAM=0: the same reverse pass with an update per batch; a block is --steps * --accum
        steps) and `fused` (no key, the default schedule).  Reported per image.

    python tools/bench_grad_accum.py [--only kernel,norm,step] [--launches 200] [--steps 50] [--samples 5] [--batch 64] [--accum 4]

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
PLAIN = {'MV3D_FUSE_FC_ADAM': '0', 'MV3D_FUSE_FINALIZE': '0', 'MV3D_OVERLAP_ADAM': '0'}
STORE, ADD, FINISH = 0, 1, 2


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


def _buffers(count):
    gen = torch.Generator(device='cuda').manual_seed(0)
    # small values: thousands of ADD / FINISH launches in a row keep the sums finite
    return [torch.randn(count, device='cuda', generator=gen).mul_(1e-6) for _ in range(4)]


def bench_kernel(args):
    from dynamic_multiview_3d_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    count = FLAT
    total, g, s, p = _buffers(count)
    loss = torch.zeros(2, device='cuda')
    w = float(np.float32(1 - 0.999))
    acc = lambda mode: (lambda: lib.grad_accumulate(count, total.data_ptr(), g.data_ptr(), mode, loss.data_ptr(), loss.data_ptr() + 4,
                                                    0.25, None, 0, st))
    fns = {'store': acc(STORE), 'add': acc(ADD), 'finish': acc(FINISH), 'ema': lambda: lib.ema_step(count, s.data_ptr(), p.data_ptr(), w, st)}
    for fn in fns.values():
        _timed(fn, 20)
    ms = {k: [] for k in fns}
    for _ in range(args.samples):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, args.launches))
    out = {k: _stats(v, (8 if k == 'store' else 12) * count) for k, v in ms.items()}
    spread = out['ema']['ms']['max'] - out['ema']['ms']['min']
    bar = out['ema']['ms']['median'] + spread
    return dict({"bench": "grad_accum_kernel", "floats": count, "launches": args.launches, "samples": args.samples}, **out,
                bar_ms=round(bar, 5), bar_met={k: bool(out[k]['ms']['median'] <= bar) for k in ('add', 'finish')})


def bench_norm(args):
    from dynamic_multiview_3d_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    count = FLAT
    total, g, _, _ = _buffers(count)
    out = torch.zeros(2, device='cuda')
    state = torch.zeros(16, device='cuda')
    nbytes = int(lib.grad_clip_workspace_bytes(count))
    ws = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device='cuda')
    rec = (out.data_ptr(), state.data_ptr(), state.data_ptr() + 32, ws.data_ptr(), nbytes, st)

    def fused():
        lib.grad_accumulate(count, total.data_ptr(), g.data_ptr(), FINISH, None, None, 0.25, ws.data_ptr(), nbytes, st)
        lib.grad_clip_finish(count, 0.25, 1.0, *rec)

    def split():
        lib.grad_accumulate(count, total.data_ptr(), g.data_ptr(), FINISH, None, None, 0.25, None, 0, st)
        lib.grad_clip_scale(count, g.data_ptr(), 0.25, 1.0, *rec)
    ms = {'fused': [], 'split': []}
    for fn in (fused, split):
        _timed(fn, 20)
    for _ in range(args.samples):
        for k, fn in (('fused', fused), ('split', split)):
            ms[k].append(_timed(fn, args.launches))
    res = {k: _stats(v, (12 if k == 'fused' else 16) * count) for k, v in ms.items()}
    saved = res['split']['ms']['median'] - res['fused']['ms']['median']
    return {"bench": "grad_accum_norm", "floats": count, "launches": args.launches, "samples": args.samples, "fused": res['fused'],
            "split": res['split'], "saved_ms": round(saved, 5), "fused_is_faster": bool(saved > 0)}


def bench_step(args):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    n = args.accum
    models = {}
    for name, env, extra in (('plain', PLAIN, {}), ('accum', {}, {'grad_accum_steps': n}), ('fused', {}, {})):
        for k in PLAIN:
            os.environ[k] = env.get(k, '1')
        conf = dict({'batch_size': args.batch, 'learning_rate': 1e-4, 'experiment_name': 'appflow_offset'}, **extra)
        m = AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda', seed=1234)
        m.feed(**synth_batch(np.random.default_rng(0), args.batch))
        for _ in range(2 * n):
            m.graph.train_step()
        models[name] = m
    assert models['accum'].graph.micro_step == 0
    gc.collect()
    gc.disable()
    calls = args.steps * n                          # train_step() calls per block: the same number of images in every arm
    ms = {k: [] for k in models}
    for _ in range(args.samples):
        for name in models:
            ms[name].append(_timed(models[name].graph.train_step, calls))
    gc.enable()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"bench": "grad_accum_step", "micro_batch": args.batch, "accum_steps": n, "calls_per_block": calls, "blocks": args.samples,
            "ms_per_micro_batch": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
            "images_per_sec": {k: round(args.batch / (med[k] * 1e-3), 1) for k in ms},
            "accum_vs_plain": round(med['plain'] / med['accum'], 4), "accum_vs_fused": round(med['fused'] / med['accum'], 4),
            "last_accum_loss": float(models['accum'].graph.accum_loss())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--only', default='kernel,norm,step')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=50, help='accumulation cycles per block of the step measurement')
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--accum', type=int, default=4, help="conf['grad_accum_steps'] of the accumulating model")
    args = ap.parse_args()
    for name in [s for s in args.only.split(',') if s]:
        print(json.dumps({'kernel': bench_kernel, 'norm': bench_norm, 'step': bench_step}[name](args)), flush=True)


if __name__ == '__main__':
    main()
