#!/usr/bin/env python
"""Micro-benchmark of the masked census and SSIM losses against their unmasked entries (GPU only):
python tools/bench_masked_image_losses.py [--iters K] [--repeats R]

At the benchmarked image shape [64,128,128,3], value plus gradient, mv3d_census_loss_masked (radius 3) is timed beside
mv3d_census_loss and mv3d_ssim_loss_masked beside mv3d_ssim_loss, in one process.  Every entry rotates over four buffer sets
(images, mask, gradient, workspace), so that a call does not find its own operands of the call before in the nearest cache.  After
10 warm-up calls each, R rounds run; a round times K back-to-back calls of each entry between device events, one after the other,
so that a drift of the machine hits all alike.  The figure is the median round's time per call (one call = the tile launch + the
final launch), with the smallest and the largest round.

The masked form adds one load and at most three multiplies per pixel or window.  Its bar: the unmasked median, plus the time of the
extra 4 B per pixel at the byte rate the unmasked call itself achieves, plus the larger of the two min-max spreads.  The last rows
state the bar and MET or MISSED."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dynamic_multiview_3d_amd import _lib
from tools.bench_ssim_loss import alternating

SETS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_masked_image_losses needs a GPU"
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, h, w, c, radius = 64, 128, 128, 3, 3
    nb_census = int(lib.census_loss_workspace_bytes(n, h, w, c, radius))
    nb_ssim = int(lib.ssim_loss_workspace_bytes(n, h, w, c))
    nb_ssim_masked = int(lib.ssim_loss_masked_workspace_bytes(n, h, w, c))
    sets = []
    for _ in range(SETS):
        sets.append(dict(a=torch.rand((n, h, w, c), device='cuda'), b=torch.rand((n, h, w, c), device='cuda'),
                         m=(torch.rand((n, h, w, 1), device='cuda') < 0.7).float(), grad=torch.empty((n, h, w, c), device='cuda'),
                         ws=torch.empty(max(nb_census, nb_ssim_masked), dtype=torch.uint8, device='cuda')))
    loss = torch.zeros(1, device='cuda')

    def rotating(call):
        state = [0]

        def fn():
            s = sets[state[0] % SETS]
            state[0] += 1
            call(s)
        return fn
    fns = {
        'census_loss r=3 +grad': rotating(lambda s: lib.census_loss(
            n, h, w, c, s['a'].data_ptr(), c, s['b'].data_ptr(), c, radius, 1.0, 0.01, 1.0, loss.data_ptr(), s['grad'].data_ptr(), c, 0,
            s['ws'].data_ptr(), nb_census, st)),
        'census_loss_masked r=3 +grad': rotating(lambda s: lib.census_loss_masked(
            n, h, w, c, s['a'].data_ptr(), c, s['b'].data_ptr(), c, s['m'].data_ptr(), 1, radius, 1.0, 0.01, 1.0, loss.data_ptr(),
            s['grad'].data_ptr(), c, 0, s['ws'].data_ptr(), nb_census, st)),
        'ssim_loss +grad': rotating(lambda s: lib.ssim_loss(
            n, h, w, c, s['a'].data_ptr(), c, s['b'].data_ptr(), c, 1.0, 1.0, loss.data_ptr(), s['grad'].data_ptr(), c, 0, s['ws'].data_ptr(),
            nb_ssim, st)),
        'ssim_loss_masked +grad': rotating(lambda s: lib.ssim_loss_masked(
            n, h, w, c, s['a'].data_ptr(), c, s['b'].data_ptr(), c, s['m'].data_ptr(), 1, 1.0, 1.0, loss.data_ptr(), s['grad'].data_ptr(), c, 0,
            s['ws'].data_ptr(), nb_ssim_masked, st)),
    }
    image_bytes = 3.0 * n * h * w * c * 4                  # both images read once, the gradient written once
    mask_bytes = 4.0 * n * h * w
    nbytes = {k: image_bytes + (mask_bytes if 'masked' in k else 0.0) for k in fns}
    res = alternating(fns, args.iters, args.repeats)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({'op': k, 'shape': [n, h, w, c], 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                          'MB': round(nbytes[k] / 1e6, 2), 'GB/s': round(nbytes[k] / med / 1e3, 1)}), flush=True)
    for plain, masked in (('census_loss r=3 +grad', 'census_loss_masked r=3 +grad'), ('ssim_loss +grad', 'ssim_loss_masked +grad')):
        (pm, pl, ph), (mm, ml, mh) = res[plain], res[masked]
        extra = mask_bytes / (nbytes[plain] / pm)           # us for the mask's bytes at the unmasked call's own byte rate
        spread = max(ph - pl, mh - ml)
        bar = pm + extra + spread
        print(json.dumps({'op': masked + ' against ' + plain, 'masked us': round(mm, 2), 'unmasked us': round(pm, 2),
                          'ratio': round(mm / pm, 4), 'extra bytes us': round(extra, 2), 'spread us': round(spread, 2), 'bar us': round(bar, 2),
                          'verdict': 'MET' if mm <= bar else 'MISSED'}), flush=True)


if __name__ == '__main__':
    main()
