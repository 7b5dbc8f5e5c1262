#!/usr/bin/env python
"""Micro-benchmark of the forward-backward consistency loss (mv3d_flow_consistency; GPU only):
python tools/bench_flow_consistency.py [--iters K] [--repeats R] [--sets S]

At N = 64, 128 x 128 the entry (value + gradient: the tile, scatter and final launches) is timed against mv3d_flow_smoothness
(unguided, value + gradient: its two launches) at the same shape in the same process.  Every call takes the next of S buffer sets
(flow, gradient and workspace of its own), so a call does not find its operands where the previous one left them.  After 10
warm-up calls each, R rounds run; a round times K back-to-back calls of each entry between device events, one after the other, so
that a drift of the machine hits both alike.  The figures are the median round's time per call with the fastest and the slowest
round.  The flows are smooth fields of a few pixels with an approximate inverse in the second half of the batch, the layout
conf['pair_swap'] produces.

Then one AppearanceFlowModel step at batch 64 is timed with conf['pair_swap'] + conf['flow_consistency_weight'] against the default
step, with a host clock around a device synchronise.  Each model runs in a child process of its own (one at a time, each under
--step-timeout), the two kinds alternating (--step-rounds of each).  The head stays fused: the term adds its three launches at
the end of the forward plan."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dynamic_multiview_3d_amd import _lib
from tools.bench_ssim_loss import alternating, timed_us_host


def paired_flows(n, h, seed):
    """[n,h,h,2] float32: low-frequency flows of a few pixels; sample n + n/2 holds about the inverse of sample n."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:h].astype(np.float64)
    first = np.stack([2.0 * np.sin(x / 17.0 + 0.3) * np.cos(y / 23.0), 1.5 * np.cos(x / 29.0) + 0.5 * np.sin(y / 11.0 + 1.0)], -1)
    first = first[None] * rng.uniform(0.5, 1.5, (n // 2, 1, 1, 1)) + rng.normal(0, 0.05, (n // 2, h, h, 2))
    inverse = -np.transpose(first, (0, 2, 1, 3))[..., ::-1] + rng.normal(0, 0.05, first.shape)
    return np.concatenate([first, inverse], axis=0).astype(np.float32)


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
    assert torch.cuda.is_available(), "bench_flow_consistency needs a GPU"
    if args.step_on is not None:
        return step_child(bool(args.step_on), args.step_iters, args.step_repeats)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, h = 64, 128
    nb_c, nb_s = int(lib.flow_consistency_workspace_bytes(n, h, h)), int(lib.flow_smoothness_workspace_bytes(n, h, h))
    sets = []
    for i in range(max(args.sets, 1)):
        sets.append(dict(flow=torch.from_numpy(paired_flows(n, h, i)).cuda(), grad=torch.zeros((n, h, h, 2), device='cuda'),
                         loss=torch.zeros(1, device='cuda'), ws=torch.empty(max(nb_c, nb_s), dtype=torch.uint8, device='cuda')))

    def rotating(fn):
        state = [0]

        def call():
            fn(sets[state[0] % len(sets)])
            state[0] += 1
        return call
    fns = {
        'flow_consistency value+grad': rotating(lambda s: lib.flow_consistency(
            n, h, h, s['flow'].data_ptr(), 2, 1e-3, 1e-6, s['loss'].data_ptr(), None, s['grad'].data_ptr(), 2, 0, s['ws'].data_ptr(), nb_c, st)),
        'flow_consistency value+grad accumulate': rotating(lambda s: lib.flow_consistency(
            n, h, h, s['flow'].data_ptr(), 2, 1e-3, 1e-6, s['loss'].data_ptr(), None, s['grad'].data_ptr(), 2, 1, s['ws'].data_ptr(), nb_c, st)),
        'flow_consistency value': rotating(lambda s: lib.flow_consistency(
            n, h, h, s['flow'].data_ptr(), 2, 1e-3, 1e-6, s['loss'].data_ptr(), None, None, 2, 0, s['ws'].data_ptr(), nb_c, st)),
        'flow_smoothness unguided value+grad': rotating(lambda s: lib.flow_smoothness(
            n, h, h, s['flow'].data_ptr(), 2, None, 0, 0, 10.0, 1e-3, 1e-6, s['loss'].data_ptr(), s['grad'].data_ptr(), 2, 0,
            s['ws'].data_ptr(), nb_s, st)),
    }
    for k, (med, lo, hi) in alternating(fns, args.iters, args.repeats).items():
        print(json.dumps({'op': k, 'shape': [n, h, h], 'us': round(med, 2), 'us_min': round(lo, 2), 'us_max': round(hi, 2),
                          'buffer_sets': len(sets)}), flush=True)
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
        print(json.dumps({'op': 'AppearanceFlowModel.train_step', 'loss': 'L2 + 0.1 consistency, pair_swap' if on else 'L2', 'batch': 64,
                          'us': round(med[on], 1), 'us_min': round(min(v), 1), 'us_max': round(max(v), 1), 'processes': len(v),
                          'launches': launches[on]}), flush=True)
    d = med[1] - med[0]
    print(json.dumps({'op': 'step delta', 'us': round(d, 1), 'percent': round(100.0 * d / med[0], 2)}), flush=True)


def step_child(on, iters, repeats):
    """One model, one process: the median over `repeats` groups of `iters` steps."""
    from dynamic_multiview_3d_amd import pair_swap
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.train import SyntheticData
    conf = dict({'batch_size': 64, 'learning_rate': 1e-4}, **({'pair_swap': True, 'flow_consistency_weight': 0.1} if on else {}))
    m = AppearanceFlowModel(conf, load_tfrec=False, device='cuda')
    data = SyntheticData(m, pool=1)
    if on:
        data = pair_swap.PairSwappedData(data, pair_swap.PairSwap(conf))
    m.feed(**data.next())
    med, lo, hi = alternating({'step': m.graph.train_step}, iters, repeats, warmup=10, timer=timed_us_host)['step']
    print(json.dumps({'us': med, 'us_min': lo, 'us_max': hi, 'launches': [m.graph.n_launch_fwd, m.graph.n_launch_bwd_fused]}), flush=True)


if __name__ == '__main__':
    main()
