#!/usr/bin/env python
"""What the colour stage of the input path costs on one GPU, against the project's existing 8-bytes-per-element stream.

mv3d_color_augment at the benchmarked input (n = 64, 128 x 128, two colour views, all four stages) and at a large case (n = 512),
where the HBM rate is visible: the call is recorded into a plan, so that its two launches can be timed on their own --
    sums    color_augment_sums_kernel alone (4 B/element read)
    apply   color_augment_apply_kernel alone (4 B read + 4 B written per element)
    call    both, as conf['augment_contrast'] makes the reader launch them
    nocontrast   the call without the contrast bit (one launch)
    store   mv3d_grad_accumulate in MV3D_ACCUM_STORE mode over the same number of floats, in the same process and alternating with
            the others sample by sample: the yardstick of the apply pass
warm-up, then --launches calls per sample between two HIP events, --samples samples each; median, min and max.  Bar: median apply
time <= median store time + the store samples' own max - min; reported as MET, or MISSED by how much.

    python tools/bench_color_augment.py [--n 64,512] [--size 128] [--views 2] [--launches 200] [--samples 7]

One JSON line per case.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

COPY_TBS = 6.29             # measured float4 copy rate of the MI355X, TB/s


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
    return {"us": {"median": round(med * 1e3, 3), "min": round(ms[0] * 1e3, 3), "max": round(ms[-1] * 1e3, 3)}, "GB/s": round(gbs, 1),
            "share_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3)}


def bench_case(args, n):
    from dynamic_multiview_3d_amd import _lib, augment as A
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    h = w = args.size
    gen = torch.Generator(device='cuda').manual_seed(0)
    views = [torch.rand((n, h, w, 3), device='cuda', generator=gen) for _ in range(args.views)]
    conf = {'augment_brightness': 0.3, 'augment_saturation': (0.3, 2), 'augment_hue': 0.5, 'augment_contrast': (0.4, 1.8)}
    params = torch.from_numpy(A.draw_params(np.random.default_rng(0), n, conf)).cuda()
    nbytes = int(lib.color_augment_workspace_bytes(n, args.views, h, w))
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device='cuda')
    ptrs = (C.c_void_p * args.views)(*[v.data_ptr() for v in views])
    count = args.views * n * h * w * 3
    src, dst = torch.rand(count, device='cuda', generator=gen), torch.empty(count, device='cuda')

    def call(stages):
        return lambda: lib.color_augment(ptrs, args.views, n, h, w, params.data_ptr(), stages, ws.data_ptr(), nbytes, st)
    plan = lib.plan_create()
    lib.plan_begin(plan)
    call(A.ALL_STAGES)()
    lib.plan_end()
    assert lib.plan_size(plan) == 2                 # the sums, then the map
    fns = {'store': lambda: lib.grad_accumulate(count, dst.data_ptr(), src.data_ptr(), _lib.ACCUM_STORE, None, None, 1.0, None, 0, st),
           'sums': lambda: lib.plan_run_range(plan, 0, 1, st), 'apply': lambda: lib.plan_run_range(plan, 1, 2, st),
           'call': call(A.ALL_STAGES), 'nocontrast': call(A.ALL_STAGES & ~A.CONTRAST)}
    for fn in fns.values():
        _timed(fn, 20)
    ms = {k: [] for k in fns}
    for _ in range(args.samples):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, args.launches))
    lib.plan_destroy(plan)
    traffic = {'store': 8, 'sums': 4, 'apply': 8, 'call': 12, 'nocontrast': 8}
    out = {k: _stats(v, traffic[k] * count) for k, v in ms.items()}
    spread = out['store']['us']['max'] - out['store']['us']['min']
    bar = out['store']['us']['median'] + spread
    miss = out['apply']['us']['median'] - bar
    return dict({"bench": "color_augment", "n": n, "size": h, "views": args.views, "floats": count, "launches": args.launches,
                 "samples": args.samples}, **out, bar_us=round(bar, 3),
                apply_bar="MET" if miss <= 0 else "MISSED by %.3f us (%.1f %%)" % (miss, 100 * miss / bar))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', default='64,512')
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--views', type=int, default=2)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--samples', type=int, default=7)
    args = ap.parse_args()
    for n in [int(s) for s in args.n.split(',') if s]:
        print(json.dumps(bench_case(args, n)), flush=True)


if __name__ == '__main__':
    main()
