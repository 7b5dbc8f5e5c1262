#!/usr/bin/env python
"""Micro-benchmark of the occlusion-aware head (mv3d_warp_resample_occlusion_loss, mv3d_flow_occlusion_mask; GPU only):
python tools/bench_occlusion_head.py [--iters K] [--repeats R] [--sets S]

At N = 64, 128 x 128, C = 3, in one process, four things are timed:
  (a) mv3d_warp_resample_loss, the unmasked fused head
  (b) mv3d_flow_occlusion_mask alone
  (c) mv3d_warp_resample_occlusion_loss, the fused occlusion-aware head (its tile and final launches)
  (d) the four-launch chain (c) replaces: the mask, mv3d_warp_resample_fwd, mv3d_pixel_loss_strided with the mask,
      mv3d_warp_resample_bwd
Every call takes the next of S buffer sets (images, flow, outputs and workspace of its own), so a call does not find its operands
where the previous one left them.  After 10 warm-up calls each, R rounds run; a round times K back-to-back calls of each entry
between device events, one after the other, so that a drift of the machine hits all alike.  The figures are the median round's time
per call with the fastest and the slowest round.  The bar for (c) is (a) + (b) plus the larger of their spreads, and (c) must beat
(d); the verdict line says MET or MISSED for each.

Then one AppearanceFlowModel step at batch 64 is timed with conf['pair_swap'] + conf['occlusion_mask'] against the default step,
with a host clock around a device synchronise.  Each model runs in a child process of its own (one at a time, each under
--step-timeout), the two kinds alternating (--step-rounds of each)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dynamic_multiview_3d_amd import _lib
from tools.bench_flow_consistency import paired_flows
from tools.bench_ssim_loss import alternating, timed_us_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--sets', type=int, default=4, help="buffer sets the calls rotate over")
    ap.add_argument('--step-iters', type=int, default=10)
    ap.add_argument('--step-repeats', type=int, default=15)
    ap.add_argument('--step-rounds', type=int, default=3)
    ap.add_argument('--step-timeout', type=float, default=180.0, help="seconds one child process may take")
    ap.add_argument('--step-on', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--no-step', action='store_true', help="kernels only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_occlusion_head needs a GPU"
    if args.step_on is not None:
        return step_child(bool(args.step_on), args.step_iters, args.step_repeats)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, h, c = 64, 128, 3
    a1, a2 = 0.01, 0.5
    nb = int(lib.warp_resample_occlusion_loss_workspace_bytes(n, h, h))
    sets = []
    for i in range(max(args.sets, 1)):
        g = torch.Generator(device='cuda').manual_seed(i)
        sets.append(dict(flow=torch.from_numpy(paired_flows(n, h, i)).cuda(),
                         src=torch.rand((n, h, h, c), device='cuda', generator=g), tgt=torch.rand((n, h, h, c), device='cuda', generator=g),
                         warp=torch.zeros((n, h, h, 2), device='cuda'), gen=torch.zeros((n, h, h, c), device='cuda'),
                         dgen=torch.zeros((n, h, h, c), device='cuda'), dflow=torch.zeros((n, h, h, 2), device='cuda'),
                         mask=torch.zeros((n, h, h, 1), device='cuda'), loss=torch.zeros(1, device='cuda'),
                         ws=torch.empty(nb, dtype=torch.uint8, device='cuda')))

    def rotating(fn):
        state = [0]

        def call():
            fn(sets[state[0] % len(sets)])
            state[0] += 1
        return call
    p = lambda t: t.data_ptr()

    def chain(s):
        lib.flow_occlusion_mask(n, h, h, p(s['flow']), 2, a1, a2, 1, p(s['mask']), 1, None, None, 0, st)
        lib.warp_resample_fwd(n, h, h, h, h, c, p(s['src']), p(s['flow']), 2, p(s['warp']), p(s['gen']), st)
        lib.pixel_loss_strided(n * h * h, c, p(s['gen']), c, p(s['tgt']), c, 1.0, p(s['mask']), 1, 2, 1.0, p(s['loss']), p(s['dgen']), c, st)
        lib.warp_resample_bwd(n, h, h, h, h, c, p(s['src']), p(s['flow']), 2, p(s['dgen']), p(s['dflow']), 2, st)
    fns = {
        'a warp_resample_loss (unmasked head)': rotating(lambda s: lib.warp_resample_loss(
            n, h, h, h, h, c, p(s['src']), p(s['flow']), 2, p(s['tgt']), c, 2, 1.0, p(s['warp']), p(s['gen']), p(s['dflow']), 2, p(s['loss']), st)),
        'b flow_occlusion_mask': rotating(lambda s: lib.flow_occlusion_mask(
            n, h, h, p(s['flow']), 2, a1, a2, 1, p(s['mask']), 1, None, None, 0, st)),
        'c warp_resample_occlusion_loss (fused)': rotating(lambda s: lib.warp_resample_occlusion_loss(
            n, h, h, h, h, c, p(s['src']), p(s['flow']), 2, p(s['tgt']), c, 2, 1.0, a1, a2, 1, p(s['warp']), p(s['gen']), p(s['dflow']), 2,
            p(s['mask']), 1, p(s['loss']), None, p(s['ws']), nb, st)),
        'd chain: mask, resample_fwd, pixel_loss(mask), resample_bwd': rotating(chain),
    }
    res = alternating(fns, args.iters, args.repeats)
    for k, (med, lo, hi) in res.items():
        print(json.dumps({'op': k, 'shape': [n, h, h, c], 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                          'buffer_sets': len(sets)}), flush=True)
    (a, alo, ahi), (b, blo, bhi), (cc, _, _), (d, _, _) = (res[k] for k in fns)
    bar = a + b + max(ahi - alo, bhi - blo)
    print(json.dumps({'op': 'verdict', 'c_us': round(cc, 2), 'bar_a_plus_b_plus_spread_us': round(bar, 2),
                      'against_a_plus_b': 'MET' if cc <= bar else 'MISSED', 'chain_us': round(d, 2),
                      'against_chain': 'MET' if cc < d else 'MISSED'}), flush=True)
    if args.no_step:
        return

    import subprocess
    times = {0: [], 1: []}
    launches = {}
    for _ in range(args.step_rounds):
        for on in times:                         # one child at a time: a fresh process, a fresh device context
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--step-on', str(on), '--step-iters', str(args.step_iters),
                                  '--step-repeats', str(args.step_repeats)], check=True, capture_output=True, text=True,
                                 timeout=args.step_timeout).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            times[on].append(rec['us'])
            launches[on] = rec['launches']
    med = {on: float(np.median(v)) for on, v in times.items()}
    for on, v in times.items():
        print(json.dumps({'op': 'AppearanceFlowModel.train_step', 'loss': 'occlusion-masked L2, pair_swap' if on else 'L2', 'batch': 64,
                          'us': round(med[on], 1), 'us_min': round(min(v), 1), 'us_max': round(max(v), 1), 'processes': len(v),
                          'launches': launches[on]}), flush=True)
    d = med[1] - med[0]
    print(json.dumps({'op': 'step delta', 'us': round(d, 1), 'percent': round(100.0 * d / med[0], 2)}), flush=True)


def step_child(on, iters, repeats):
    """One model, one process: the median over `repeats` groups of `iters` steps."""
    from dynamic_multiview_3d_amd import pair_swap
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.train import SyntheticData
    conf = dict({'batch_size': 64, 'learning_rate': 1e-4}, **({'pair_swap': True, 'occlusion_mask': True} if on else {}))
    m = AppearanceFlowModel(conf, load_tfrec=False, device='cuda')
    data = SyntheticData(m, pool=1)
    if on:
        data = pair_swap.PairSwappedData(data, pair_swap.PairSwap(conf))
    m.feed(**data.next())
    med, lo, hi = alternating({'step': m.graph.train_step}, iters, repeats, warmup=10, timer=timed_us_host)['step']
    print(json.dumps({'us': med, 'us_min': lo, 'us_max': hi, 'launches': [m.graph.n_launch_fwd, m.graph.n_launch_bwd_fused]}), flush=True)


if __name__ == '__main__':
    main()
