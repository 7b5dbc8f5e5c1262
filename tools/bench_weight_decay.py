#!/usr/bin/env python
"""What decoupled weight decay and a learning-rate schedule cost on one GPU, against what the project already ships.

kernel: over the benchmarked model's flat buffer (69 535 424 floats) and its decay table (26 ranges), in one process and
        alternating sample by sample: mv3d_weight_decay_step alone, mv3d_grad_accumulate in STORE mode over the same count (the
        project's 8 B/element stream), the fused decay + EMA, mv3d_ema_step, and decay-only + mv3d_ema_step back to back.
        Every launch takes the next of four buffer sets, so none finds its operands in the Infinity Cache.  Warm-up, then
        --launches launches per sample (0.2-0.5 s) between two HIP events, --samples samples each.
        Bars: decay-only <= STORE + STORE's max - min; fused <= EMA * 16 / 12 + EMA's max - min; fused < decay-only + EMA.
step:   AppearanceFlowModel at batch 64, every variant in a fresh process of its own (three blocks of --steps train steps),
        --samples rounds with the variants alternating: default, a schedule alone, ema_decay alone, weight_decay alone,
        weight_decay + ema_decay (the fused launch in front of the fc event).

    python tools/bench_weight_decay.py [--only kernel,step] [--launches 2000] [--steps 100] [--samples 3] [--batch 64]

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

ROTATE = 4
SCHED = dict(lr_schedule='cosine', lr_decay_steps=200000, lr_warmup_steps=1000)


def _timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def _model(batch, **extra):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    conf = dict({'batch_size': batch, 'learning_rate': 1e-4, 'experiment_name': 'appflow_offset'}, **extra)
    m = AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda', seed=1234)
    m.feed(**synth_batch(np.random.default_rng(0), batch))
    return m


def _ms(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def bench_kernel(args):
    from dynamic_multiview_3d_amd import _lib
    lib = _lib.lib()
    m = _model(2, weight_decay=0.01)
    g = m.graph
    n, ranges = g.flat_size, list(g._decay_ranges)
    table = g._decay_table.clone()
    decayed = sum(b - a for a, b in ranges)
    del m, g
    torch.cuda.empty_cache()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device='cuda').manual_seed(0)
    # every launch takes the next of ROTATE buffer sets (4 x 278 MB per operand): a launch then never finds its operands in the
    # 256 MB Infinity Cache from the launch before, as a launch inside a train step does not
    ps, ss, as_, bs = ([torch.randn(n, device='cuda', generator=gen) for _ in range(ROTATE)] for _ in range(4))
    loss = torch.zeros(4, device='cuda')
    f, w = float(np.float32(1e-4 * 0.01)), float(np.float32(1 - 0.999))
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % ROTATE
            fn(turn[0])
        return call
    decay = rotating(lambda i: lib.weight_decay_step(ps[i].data_ptr(), None, 0, n, table.data_ptr(), len(ranges), f, 0.0, st))
    fused = rotating(lambda i: lib.weight_decay_step(ps[i].data_ptr(), ss[i].data_ptr(), 0, n, table.data_ptr(), len(ranges), f, w, st))
    ema = rotating(lambda i: lib.ema_step(n, ss[i].data_ptr(), ps[i].data_ptr(), w, st))
    store = rotating(lambda i: lib.grad_accumulate(n, as_[i].data_ptr(), bs[i].data_ptr(), _lib.ACCUM_STORE, loss.data_ptr(),
                                                   loss.data_ptr() + 4, 0.5, None, 0, st))
    both = lambda: (decay(), ema())
    fns = {'decay': decay, 'store': store, 'fused': fused, 'ema': ema, 'decay_then_ema': both}
    for fn in fns.values():
        _timed(fn, 10)
    t = {k: [] for k in fns}
    for _ in range(args.samples):
        for k, fn in fns.items():
            t[k].append(_timed(fn, args.launches))
    ms = {k: _ms(v) for k, v in t.items()}
    spread = lambda k: ms[k]["max"] - ms[k]["min"]
    bar_decay = ms['store']["median"] + spread('store')
    bar_fused = ms['ema']["median"] * 16.0 / 12.0 + spread('ema')
    return {"bench": "weight_decay_kernel", "floats": n, "ranges": len(ranges), "decayed_floats": decayed, "launches": args.launches, "rotating_buffer_sets": ROTATE,
            "samples": args.samples, "ms": ms,
            "decay_GB/s": round(8.0 * decayed / (ms['decay']["median"] * 1e-3) / 1e9, 1),
            "fused_GB/s": round((16.0 * decayed + 12.0 * (n - decayed)) / (ms['fused']["median"] * 1e-3) / 1e9, 1),
            "decay_bar_ms": round(bar_decay, 5), "decay_bar_met": bool(ms['decay']["median"] <= bar_decay),
            "fused_bar_ms": round(bar_fused, 5), "fused_bar_met": bool(ms['fused']["median"] <= bar_fused),
            "fused_beats_two_launches": bool(ms['fused']["median"] < ms['decay_then_ema']["median"])}


VARIANTS = {                       # name: extra conf
    'default': {},
    'schedule': SCHED,
    'ema': {'ema_decay': 0.999},
    'decay': {'weight_decay': 0.01},
    'decay_ema': {'weight_decay': 0.01, 'ema_decay': 0.999},
}


def bench_variant(args, name):
    """One variant, alone in this process (a process that holds several models has more streams than hardware queues, and which
    streams then share a queue -- not the variant -- decides the step time): three blocks of --steps train steps."""
    m = _model(args.batch, **VARIANTS[name])
    for _ in range(20):
        m.graph.train_step()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    ms = [_timed(m.graph.train_step, args.steps) for _ in range(3)]
    return {"variant": name, "ms": _ms(ms)}


def bench_step(args):
    """Every variant in a fresh child process of its own, --samples rounds, the variants alternating within a round."""
    import subprocess
    ms = {k: [] for k in VARIANTS}
    for _ in range(args.samples):
        for name in VARIANTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--only', 'variant:' + name, '--steps', str(args.steps),
                                  '--batch', str(args.batch)], check=True, capture_output=True, text=True, timeout=300).stdout
            ms[name].append(json.loads(out.strip().splitlines()[-1])["ms"]["median"])
            print(name, ms[name][-1], file=sys.stderr, flush=True)
    out = {k: _ms(v) for k, v in ms.items()}
    med = {k: v["median"] for k, v in out.items()}
    return {"bench": "weight_decay_step", "batch": args.batch, "steps_per_block": args.steps, "rounds": args.samples, "step_ms": out,
            "schedule_minus_default_ms": round(med['schedule'] - med['default'], 4),
            "decay_minus_ema_ms": round(med['decay'] - med['ema'], 4),
            "decay_ema_minus_ema_ms": round(med['decay_ema'] - med['ema'], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--only', default='kernel,step')
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--samples', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    for name in [s for s in args.only.split(',') if s]:
        if name.startswith('variant:'):
            print(json.dumps(bench_variant(args, name.split(':', 1)[1])), flush=True)
        else:
            print(json.dumps({'kernel': bench_kernel, 'step': bench_step}[name](args)), flush=True)


if __name__ == '__main__':
    main()
