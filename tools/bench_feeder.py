#!/usr/bin/env python
"""Train-step rate with the TFRecord feeder in the loop (host decode + PCIe upload overlapped with the step) against the
device-resident rate of bench.py (GPU box only): python tools/bench_feeder.py [steps] [--record-size S]

Without --record-size: AppearanceFlowModel, B = 64, 128 x 128 records of the model's own size.  With --record-size S: BASELINE
config 5 -- MultiObjectAppFlow, fully_conv, 256 x 256, B = 32, 13 features -- fed from S x S records that the reader resizes on
the device (conf['record_image_size'], mv3d_u8_process_image), and additionally the rate of the feeder alone (next() in a loop,
nothing consuming the batches but a device synchronise at the end), which has to stay above the step's.
--augment sets the four conf['augment_*'] keys (augment.py): the reader then runs the colour stage on its stream on every batch.
--geom sets conf['augment_flip' / '_zoom' / '_shift'] (0.5, 2, 1): the reader then runs the geometric stage behind it."""
import argparse
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from dynamic_multiview_3d_amd import read_tf_records as R
ap = argparse.ArgumentParser()
ap.add_argument('steps', nargs='?', type=int, default=40)
ap.add_argument('--record-size', type=int, default=None, help='time config 5 (256 x 256 multi-object) fed from records of this size')
ap.add_argument('--augment', action='store_true', help='switch on all four colour-augmentation stages of the reader')
ap.add_argument('--geom', action='store_true', help='switch on flip, zoom and shift: the geometric stage of the reader')
args = ap.parse_args()
steps = args.steps
tmp = tempfile.mkdtemp(prefix='mv3d_feed_')
rng = np.random.default_rng(0)
t0 = time.perf_counter()
if args.record_size is None:
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel as Model
    B, nfiles, per_file = 64, 4, 64 * 5
    conf = {'batch_size': B, 'learning_rate': 1e-4, 'data_dir': tmp, 'train_val_split': 1.0}

    def sample():
        img0 = rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)
        img1 = rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)
        return {'image0': img0.tobytes(), 'image1': img1.tobytes(), 'depth0': img0[..., :1].tobytes(), 'depth1': img1[..., :1].tobytes(),
                'displacement': rng.uniform(-1, 1, 2).astype(np.float32)}
else:
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow as Model, INPUTS
    B, nfiles, per_file, S = 32, 2, 32 * 4, args.record_size
    conf = {'batch_size': B, 'learning_rate': 1e-4, 'data_dir': tmp, 'train_val_split': 1.0, 'use_color': '', 'use_depth': 0.1,
            'combination_image': '', 'gen_sep_images': '', 'fully_conv': '', 'image_size': 256, 'record_image_size': S}

    def sample():
        s = {name: rng.integers(0, 256, (S, S, ch), dtype=np.uint8).tobytes() for name, ch in INPUTS}
        s['displacement'] = rng.uniform(-10, 10, 2).astype(np.float32)
        return s
if args.augment:
    conf.update({'augment_brightness': 0.3, 'augment_saturation': (0.3, 2), 'augment_hue': 0.5, 'augment_contrast': (0.4, 1.8)})
if args.geom:
    conf.update({'augment_flip': 0.5, 'augment_zoom': 2.0, 'augment_shift': 1.0})
for f in range(nfiles):
    with R.TFRecordWriter(os.path.join(tmp, '%d.tfrecords' % f)) as w:
        for i in range(per_file):
            w.write(R.serialize_example(sample()))
print('wrote %d records in %.1f s' % (nfiles * per_file, time.perf_counter() - t0), flush=True)
m = Model(conf, load_tfrec=True, build_loss=True, device='cuda:0', seed=1234)
for verify in (True, False):
    if args.record_size is not None:
        data = R.build_tfrecord_input(conf, m, training=True, seed=0, verify=verify)
        for _ in range(3):
            data.next()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            data.next()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print('feeder alone (crc verify %s): %.2f ms/batch  %.1f batches/s  %.0f images/s' % (verify, dt * 1e3 / steps, steps / dt, B * steps / dt), flush=True)
        data.close()
    data = R.build_tfrecord_input(conf, m, training=True, seed=0, verify=verify)
    for _ in range(3):
        m.train_step(**data.next())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.train_step(**data.next())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print('feeder in the loop (crc verify %s): %.2f ms/step  %.1f batches/s  %.0f images/s' % (verify, dt * 1e3 / steps, steps / dt, B * steps / dt), flush=True)
    data.close()
batch = {k: torch.rand(t.shape, device='cuda:0') for k, t in m.graph.inputs.items()}
m.feed(**batch)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    m.graph.train_step()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print('device-resident batch: %.2f ms/step  %.1f batches/s  %.0f images/s' % (dt * 1e3 / steps, steps / dt, B * steps / dt))
