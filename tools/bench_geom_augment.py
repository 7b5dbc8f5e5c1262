#!/usr/bin/env python
"""What the geometric stage of the input path costs on one GPU, against the project's existing 8-bytes-per-element stream.

mv3d_geom_augment at the benchmarked input (n = 64, two 3-channel and two 1-channel views of 128 x 128) and at a large case
(n = 512), where the HBM rate is visible --
    flip    the call with flip-only parameters (p = 0.5: a permutation of every second sample's rows, no interpolation weight)
    all     the call with flip, zoom (zmax = 2) and shift (t = 1) drawn per sample
    store   mv3d_grad_accumulate in MV3D_ACCUM_STORE mode over the same number of floats, in the same process and alternating with
            the others sample by sample: the yardstick (4 B read + 4 B written per element, as the call)
The operands rotate over four buffer sets (sources, destinations, parameters, displacement), so no call finds its lines where the
previous one left them.  Warm-up, then --launches calls per sample between two HIP events, --samples samples each; median, min
and max.  Bar: median call time <= median store time + the larger of the two min-max spreads; reported as MET, or MISSED by how
much.

    python tools/bench_geom_augment.py [--n 64,512] [--size 128] [--channels 3,3,1,1] [--launches 200] [--samples 7]

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
SETS = 4


def _timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def _stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    gbs = nbytes / (med * 1e-3) / 1e9
    return {"us": {"median": round(med * 1e3, 3), "min": round(ms[0] * 1e3, 3), "max": round(ms[-1] * 1e3, 3)}, "GB/s": round(gbs, 1),
            "share_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3)}


def bench_case(args, n, channels):
    from dynamic_multiview_3d_amd import _lib, augment as A
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    h = w = args.size
    nv = len(channels)
    gen = torch.Generator(device='cuda').manual_seed(0)
    count = n * h * w * sum(channels)
    c_ch = (C.c_int * nv)(*channels)
    confs = {'flip': {'augment_flip': 0.5}, 'all': {'augment_flip': 0.5, 'augment_zoom': 2.0, 'augment_shift': 1.0}}
    rng = np.random.default_rng(0)
    sets = []
    for _ in range(SETS):
        src = [torch.rand((n, h, w, c), device='cuda', generator=gen) for c in channels]
        dst = [torch.empty_like(t) for t in src]
        sets.append({'keep': (src, dst), 'src': (C.c_void_p * nv)(*[t.data_ptr() for t in src]), 'dst': (C.c_void_p * nv)(*[t.data_ptr() for t in dst]),
                     'disp': torch.rand((n, 2), device='cuda', generator=gen),
                     'params': {k: torch.from_numpy(A.draw_geom_params(rng, n, c, h, w)).cuda() for k, c in confs.items()},
                     'flat': (torch.rand(count, device='cuda', generator=gen), torch.empty(count, device='cuda'))})

    def call(kind):
        def fn(i):
            s = sets[i % SETS]
            lib.geom_augment(s['src'], s['dst'], c_ch, nv, n, h, w, s['params'][kind].data_ptr(), s['disp'].data_ptr(), st)
        return fn

    def store(i):
        a, b = sets[i % SETS]['flat']
        lib.grad_accumulate(count, b.data_ptr(), a.data_ptr(), _lib.ACCUM_STORE, None, None, 1.0, None, 0, st)
    fns = {'store': store, 'flip': call('flip'), 'all': call('all')}
    for fn in fns.values():
        _timed(fn, 20)
    ms = {k: [] for k in fns}
    for _ in range(args.samples):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, args.launches))
    out = {k: _stats(v, 8 * count) for k, v in ms.items()}
    res = dict({"bench": "geom_augment", "n": n, "size": h, "channels": list(channels), "floats": count, "launches": args.launches,
                "samples": args.samples}, **out)
    spread = lambda k: out[k]['us']['max'] - out[k]['us']['min']
    for k in ('flip', 'all'):
        bar = out['store']['us']['median'] + max(spread('store'), spread(k))
        miss = out[k]['us']['median'] - bar
        res[k + '_bar_us'] = round(bar, 3)
        res[k + '_bar'] = "MET" if miss <= 0 else "MISSED by %.3f us (%.1f %%)" % (miss, 100 * miss / bar)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', default='64,512')
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--channels', default='3,3,1,1')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--samples', type=int, default=7)
    args = ap.parse_args()
    channels = [int(s) for s in args.channels.split(',') if s]
    for n in [int(s) for s in args.n.split(',') if s]:
        print(json.dumps(bench_case(args, n, channels)), flush=True)


if __name__ == '__main__':
    main()
