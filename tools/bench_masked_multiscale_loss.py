#!/usr/bin/env python
"""Micro-benchmark of the masked multi-scale loss against the unmasked entry (GPU only):
python tools/bench_masked_multiscale_loss.py [--iters K] [--repeats R]

At the training shape (B = 64, 128 x 128, C = 3, L = 3), value plus stored gradient, mv3d_multiscale_warp_loss_masked is timed beside
mv3d_multiscale_warp_loss in one process.  Both rotate over four buffer sets (images, flow, mask, gradient, workspace), so that a
call does not find its own operands of the call before in the nearest cache.  After 10 warm-up calls each, R rounds run; a round
times K back-to-back calls of each entry between device events, one after the other, so that a drift of the machine hits both
alike.  The figure is the median round's time per call (one call = the pyramid, tile and final launches), with the smallest and
the largest round.  The bytes are the algorithmic bytes of tools/bench_multiscale_loss.py, plus the mask's 4 B per pixel.

The masked form adds one load per flow pixel, 336 pooled values per tile in LDS and two multiplies per coarse pixel.  Its bar: the
unmasked median, plus the time of the extra 4 B per pixel at the byte rate the unmasked call itself achieves, plus the larger of
the two min-max spreads.  The last row states the bar and MET or MISSED."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dynamic_multiview_3d_amd import _lib
from tools.bench_multiscale_loss import call_bytes
from tools.bench_ssim_loss import alternating

SETS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_masked_multiscale_loss needs a GPU"
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, h, w, c, levels = 64, 128, 128, 3, 3
    nb = int(lib.multiscale_warp_loss_workspace_bytes(n, h, w, h, w, c, levels))
    wts = (ctypes.c_float * levels)(1.0, 0.5, 0.25)
    sets = []
    for _ in range(SETS):
        sets.append(dict(src=torch.rand((n, h, w, c), device='cuda'), tgt=torch.rand((n, h, w, c), device='cuda'),
                         flow=torch.empty((n, h, w, 2), device='cuda').uniform_(-3, 3), m=(torch.rand((n, h, w, 1), device='cuda') < 0.7).float(),
                         grad=torch.empty((n, h, w, 2), device='cuda'), ws=torch.empty(nb, dtype=torch.uint8, device='cuda')))
    loss = torch.zeros(1, device='cuda')

    def rotating(call):
        state = [0]

        def fn():
            s = sets[state[0] % SETS]
            state[0] += 1
            call(s)
        return fn
    fns = {
        'multiscale_warp_loss +grad': rotating(lambda s: lib.multiscale_warp_loss(
            n, h, w, h, w, c, s['src'].data_ptr(), c, s['flow'].data_ptr(), 2, s['tgt'].data_ptr(), c, levels, wts, 2, loss.data_ptr(), None,
            s['grad'].data_ptr(), 2, 0, 0, s['ws'].data_ptr(), nb, st)),
        'multiscale_warp_loss_masked +grad': rotating(lambda s: lib.multiscale_warp_loss_masked(
            n, h, w, h, w, c, s['src'].data_ptr(), c, s['flow'].data_ptr(), 2, s['tgt'].data_ptr(), c, s['m'].data_ptr(), 1, levels, wts, 2,
            loss.data_ptr(), None, s['grad'].data_ptr(), 2, 0, 0, s['ws'].data_ptr(), nb, st)),
    }
    plain, masked = list(fns)
    mask_bytes = 4.0 * n * h * w
    plain_bytes = call_bytes(float(n * h * w), c, levels, True, True, False, False)
    nbytes = {plain: plain_bytes, masked: plain_bytes + mask_bytes}
    res = alternating(fns, args.iters, args.repeats)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({'op': k, 'shape': [n, h, w, c], 'levels': levels, 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                          'MB': round(nbytes[k] / 1e6, 2), 'GB/s': round(nbytes[k] / med / 1e3, 1)}), flush=True)
    (pm, pl, ph), (mm, ml, mh) = res[plain], res[masked]
    extra = mask_bytes / (nbytes[plain] / pm)               # us for the mask's bytes at the unmasked call's own byte rate
    spread = max(ph - pl, mh - ml)
    bar = pm + extra + spread
    print(json.dumps({'op': masked + ' against ' + plain, 'masked us': round(mm, 2), 'unmasked us': round(pm, 2), 'ratio': round(mm / pm, 4),
                      'extra bytes us': round(extra, 2), 'spread us': round(spread, 2), 'bar us': round(bar, 2),
                      'verdict': 'MET' if mm <= bar else 'MISSED'}), flush=True)


if __name__ == '__main__':
    main()
