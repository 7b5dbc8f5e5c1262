#!/usr/bin/env python
"""Micro-benchmark of the reader's device-side resize (mv3d_u8_process_image; GPU only) against the plain uint8 -> float32 / 255
kernel (mv3d_u8_to_unit_f32) writing the same number of floats: python tools/bench_process_image.py [--iters K] [--rounds R]

Per shape both kernels are timed alternately, R rounds of K back-to-back calls between device events after a warm-up; the
calls rotate through enough output buffers to exceed the 256 MiB Infinity Cache, so the stores reach HBM.  Reported: the
median round's microseconds per call and the output rate (4 bytes per output float over that time)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dynamic_multiview_3d_amd import _lib

SHAPES = [(32, 128, 128, 3, 256), (32, 128, 128, 1, 256), (32, 128, 128, 3, 64), (32, 128, 128, 3, 200), (32, 128, 128, 3, 75)]


def timed(fn, nbuf, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % nbuf)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_process_image needs a GPU"
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    for n, hs, ws, c, out in SHAPES:
        count = n * out * out * c
        nbuf = max(2, -(-(320 << 20) // (4 * count)))
        src = torch.from_numpy(rng.integers(0, 256, (n, hs, ws, c), dtype=np.uint8)).cuda()
        flat = torch.from_numpy(rng.integers(0, 256, count, dtype=np.uint8)).cuda()           # the plain kernel's input: one byte per output
        dst = [torch.empty(count, dtype=torch.float32, device='cuda') for _ in range(nbuf)]
        calls = {'u8_process_image': lambda i: lib.u8_process_image(src.data_ptr(), n, hs, ws, c, dst[i].data_ptr(), out, out, st),
                 'u8_to_unit_f32': lambda i: lib.u8_to_unit_f32(count, flat.data_ptr(), dst[i].data_ptr(), st)}
        for fn in calls.values():
            timed(fn, nbuf, 2 * nbuf)
        us = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                us[k].append(timed(fn, nbuf, args.iters))
        row = {'shape': '%dx%dx%dx%d -> %d' % (n, hs, ws, c, out), 'output_MB': round(4e-6 * count, 2), 'buffers': nbuf}
        for k in calls:
            med = float(np.median(us[k]))
            row[k] = {'us': round(med, 2), 'min_us': round(min(us[k]), 2), 'max_us': round(max(us[k]), 2), 'out_GBps': round(4e-3 * count / med, 1)}
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
