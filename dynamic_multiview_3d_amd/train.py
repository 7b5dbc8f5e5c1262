"""Train driver -- drop-in for dyn_mult_view/multi_view_model/train.py:34-156.

Same flags (--hyper, --visualize, --device, --pretrained), same conf files (a python module with a
`configuration` dict; reference-style confs that `from appearance_flow_model import ...` load
unchanged), same model selection (conf['model'], default Base_Prediction_Model: train.py:57-60), same
loop cadence (iterations itr_0..num_iterations inclusive, log every 10, validation every 500,
checkpoint every 10 000 to output_dir/model<itr> as a TensorFlow V2 bundle (tf_checkpoint.py), resume iteration
parsed from the checkpoint name: train.py:95-103,117-154).  sess.run([loss, train_op]) is model.train_step().

Input: the TFRecord shards under conf['data_dir'] (read_tf_records.py); when that directory holds no files, or with
--synthetic, seeded synthetic batches shaped like the reader's tensors.

--visualize <checkpoint name> restores output_dir/<name> and writes the model's qualitative outputs (visualize.py).
--evaluate <checkpoint name> [--eval_batches N] restores output_dir/<name>, scores N batches (default 19, the reference's
test_iter, mv3d/nobg_dm.py:118) of the `test` split -- or of synthetic batches with --synthetic -- with model.evaluate()
(loss, per-image L1 / PSNR / SSIM), prints the result and writes it to output_dir/eval_<name>.json.
--event_log additionally writes TensorFlow event files (summary.py, the counterpart of mv3d/utils/tf_utils.py:11-15) under
conf['event_log_dir'] (default output_dir): `training_loss` and `val_loss` where the JSON-lines log gets them, and with
--evaluate `test_loss` and the metrics at the checkpoint's iteration.  Without the flag only the JSON-lines log is written.
Not ported: image and histogram summaries.
With conf['ema_decay'] the checkpoints carry the averaged weights (<var>/ExponentialMovingAverage), and --evaluate and --visualize
run on them; --raw_weights opts out.  The periodic val_loss during training stays on the raw weights.
With conf['grad_clip_norm'] (or conf['grad_norm_log']) the lines written every 10th iteration also carry `grad_norm` and
`grad_clip_scale` of that step, in the JSON-lines log and, with --event_log, as scalars.
With conf['grad_accum_steps'] = N an iteration is one optimiser update: N batches of conf['batch_size'] drawn from the input and N
model.train_step() calls (micro-steps).  The logged `training_loss` is then the mean over the update's micro-batches, `grad_norm`
and `grad_clip_scale` belong to the averaged accumulated gradient, the printed time per iteration is per update, and checkpoints
are written at update boundaries only.
With conf['augment_brightness' / '_saturation' / '_hue' / '_contrast'] (augment.py) the training batches go through the colour stage,
one colour map per sample over all of its colour views: the TFRecord reader runs it on its own stream, and synthetic training batches
are handed out as augmented copies (the cycled pool stays pristine).  Validation, --evaluate and --visualize batches are never augmented;
under data parallelism every rank draws from np.random.default_rng([augment_seed, rank]).
With conf['augment_flip' / '_zoom' / '_shift'] the training batches then go through the geometric stage (augment.GeomAugment: one flip,
zoom-in and window shift per sample for all of its views, disp's azimuth negated under a flip), behind the colour stage and in front
of the pair swap, under the same rules; its generator is np.random.default_rng([augment_seed, rank, 1]).
With conf['pair_swap'] (pair_swap.py) every batch is conf['batch_size'] / 2 pairs and their reverses, for every input of the graph;
conf['flow_consistency_weight'] adds the forward-backward consistency term that layout makes possible, and conf['occlusion_mask']
takes the pixels that term's residual marks as occluded out of the head's photometric loss (`flow_visible` is then logged next to
`training_loss`).
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np
import torch

from .summary import log_value

SUMMARY_INTERVAL = 400      # train.py:24
VAL_INTERVAL = 500          # train.py:27
SAVE_INTERVAL = 10000       # train.py:30

_ALIASES = ('appearance_flow_model', 'highdim_angle', 'lowdim_angle', 'appearance_flow_tinghui', 'main_model',
            'multiobject_appflow', 'multiobject_main_model')


def load_conf(conf_file):
    """imp.load_source('hyperparams', conf_file).configuration (train.py:44-45), with the reference's
    bare module names resolved to this package."""
    if not os.path.exists(conf_file):
        sys.exit("Experiment configuration not found")
    from . import compat
    compat.install()                               # bare model-module names and dyn_mult_view.* (confs use dyn_mult_view.__file__)
    spec = importlib.util.spec_from_file_location('hyperparams', conf_file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.configuration


def select_model(conf):
    if 'model' in conf:
        return conf['model']
    from .main_model import Base_Prediction_Model
    return Base_Prediction_Model


class SyntheticData:
    """Seeded stand-in for build_tfrecord_input (multi_view_model/utils/read_tf_records.py:15-85):
    uint8-quantised car-like renders / 255, masks in {0,1}, displacement ranges of the datasets
    (SURVEY 8d).  A small pool of device-resident batches is cycled."""

    def __init__(self, model, seed=0, pool=4):
        self.model = model
        rng = np.random.default_rng(seed)
        self.pool = []
        for _ in range(pool):
            batch = {}
            for name, t in model.graph.inputs.items():
                if len(t.shape) == 2:
                    if name == 'displacement':
                        a = rng.normal(10, 10, t.shape) * rng.choice([-1, 1], t.shape)
                    elif name == 'labels':          # mv3d: [radius, sin / cos elevation, sin / cos azimuth] (mv3d/utils/tf_utils.py:184-190)
                        rad, el, az = rng.uniform(0.5, 1.5, t.shape[0]), rng.uniform(0, 0.7, t.shape[0]), rng.uniform(-3.14, 3.14, t.shape[0])
                        a = np.stack([rad, np.sin(el), np.cos(el), np.sin(az), np.cos(az)], 1)
                    else:
                        a = np.stack([rng.uniform(-1, 1, t.shape[0]), rng.uniform(-6.28, 6.28, t.shape[0])], 1)
                else:
                    a = self._images(rng, t.shape)
                    if 'mask' in name:
                        a = (a[..., :1] > 0.55).astype(np.float32) * np.ones(t.shape, np.float32)
                batch[name] = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(model.graph.device)
            self.pool.append(batch)
        self.i = 0

    @staticmethod
    def _images(rng, shape):
        b, h, w, c = shape
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.full(shape, 127.0, np.float32)
        for i in range(b):
            cy, cx = rng.uniform(0.3 * h, 0.7 * h, 2)
            ay, ax = rng.uniform(0.12 * h, 0.35 * h, 2)
            img[i][((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1] = rng.uniform(0, 255, c)
        img += rng.normal(0, 2, shape).astype(np.float32)
        return np.clip(np.rint(img), 0, 255) / 255.0

    def next(self):
        b = self.pool[self.i % len(self.pool)]
        self.i += 1
        return b


def training_log_row(model, itr, cost, learning_rate=None):
    """The train_log.jsonl line of iteration itr: the loss, and with conf['grad_clip_norm'] / conf['grad_norm_log'] on the last
    step's gradient norm (of the averaged gradient, before clipping) and clip scale, and with conf['occlusion_mask'] on the visible
    share of the last step's occlusion mask as `flow_visible`.  Reading them synchronises, like float(cost).
    learning_rate: the rate that iteration's update used (the host mirror, read before the update: no synchronisation), given
    whenever a schedule, a warm-up or weight decay is on."""
    row = {'itr': itr, 'training_loss': cost}
    if model.graph.clip_norm is not None:
        norm, scale = model.graph.grad_norm().tolist()
        row['grad_norm'], row['grad_clip_scale'] = norm, scale
    if learning_rate is not None:
        row['learning_rate'] = float(learning_rate)
    if getattr(model, 'occlusion_terms', None):      # conf['occlusion_mask']: the visible share of the step's mask, so that a collapse shows
        row['flow_visible'] = float(model.flow_visible())
    return row


def train_iteration(model, train_data):
    """One iteration of the training loop = one optimiser update; returns the device loss scalar to log.  Without gradient
    accumulation one batch and one model.train_step(); with conf['grad_accum_steps'] = N, N batches and N micro-steps, and the loss
    is Graph.accum_loss(), the mean over them."""
    n = model.graph.accum_steps
    if not n:
        return model.train_step(**train_data.next())
    for _ in range(n):
        model.train_step(**train_data.next())
    return model.graph.accum_loss()


def train_loop(model, conf, train_data, val_data, saver, itr_0=0, rank=0, log=None, events=None):
    """Iterations itr_0 .. conf['num_iterations'] inclusive (train.py:117): a log line every 10th, validation every 500th, a
    checkpoint every 10 000th.  log (a text file) and events (a summary.FileWriter or None) are rank 0's."""
    starttime = time.time()
    t_iter = []
    for itr in range(itr_0, conf['num_iterations'] + 1, 1):         # inclusive, train.py:117
        t_startiter = time.time()
        lr = model.graph.learning_rate() if model.graph.counts_updates() else None      # the rate this iteration's update uses
        cost = train_iteration(model, train_data)
        if itr % 10 == 0:
            c = float(cost)
            if rank == 0:
                print(str(itr) + ' ' + str(c))
                row = training_log_row(model, itr, c, lr)
                log.write(json.dumps(row) + '\n')
                if events is not None:
                    for key in ('training_loss', 'grad_norm', 'grad_clip_scale', 'learning_rate', 'flow_visible'):
                        if key in row:
                            log_value(events, row[key], key, itr)
        if itr % VAL_INTERVAL == 0 and itr != 0:
            vc = float(model.forward(**val_data.next()))
            if rank == 0:
                log.write(json.dumps({'itr': itr, 'val_loss': vc}) + '\n')
                if events is not None:
                    log_value(events, vc, 'val_loss', itr)
        if itr % SAVE_INTERVAL == 0 and itr != 0:
            model.graph.gather_optimizer_state()        # collective: the sharded optimiser's slots, complete on every rank
            if rank == 0:
                print('Saving model to' + conf['output_dir'])
                saver.save(None, conf['output_dir'] + '/model' + str(itr))
        t_iter.append(time.time() - t_startiter)
        if itr % 100 == 1 and rank == 0:
            if model.graph.device.type == 'cuda':
                torch.cuda.synchronize()
            avg_t_iter = (time.time() - starttime) / (itr - itr_0 + 1)
            print('time per iteration: {0}'.format(avg_t_iter))
            print('expected for complete training: {0}h '.format(avg_t_iter / 3600 * conf['num_iterations']))
            log.flush()
            if events is not None:
                events.flush()


def _event_writer(conf):
    from .summary import FileWriter
    return FileWriter(conf.get('event_log_dir') or conf['output_dir'])


def evaluate_checkpoint(model, conf, name, data, num_batches, event_log=False, write=True, weights=None):
    """--evaluate: restore output_dir/<name>, model.evaluate() over num_batches batches of `data`, print the result and write
    output_dir/eval_<name>.json; with event_log also `test_loss` (mv3d/nobg_dm.py:148-149) and every metric as scalars at the
    iteration the checkpoint's name ends in (0 when it ends in none, like the final `model`).  weights: model.evaluate()'s
    (None = the averaged weights when conf['ema_decay'] is on, 'raw' = the variables)."""
    import re
    path = conf['output_dir'] + '/' + name
    model.saver.restore(None, path)
    print('restore done.')
    result = model.evaluate(data, num_batches) if weights is None else model.evaluate(data, num_batches, weights=weights)
    m = re.match('.*?([0-9]+)$', name)
    result['iteration'] = int(m.group(1)) if m else 0
    result['checkpoint'] = name
    print(json.dumps(result))
    if write:
        with open(os.path.join(conf['output_dir'], 'eval_%s.json' % name), 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
        if event_log:
            events = _event_writer(conf)
            for key, value in result.items():
                if key in ('images', 'iteration', 'checkpoint', 'weights'):
                    continue
                log_value(events, value, 'test_loss' if key == 'loss' else key, result['iteration'])
            events.close()
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--hyper', default='../../tensorflowdata/appflow_offset/conf.py', help='hyperparameters configuration file')
    ap.add_argument('--visualize', default='', help='model within hyperparameter folder from which to create gifs')
    ap.add_argument('--device', default='0', help='GPU index (the reference sets CUDA_VISIBLE_DEVICES)')
    ap.add_argument('--pretrained', default=None, help='path to model file from which to resume training')
    ap.add_argument('--num_iterations', type=int, default=None, help='override conf["num_iterations"]')
    ap.add_argument('--synthetic', action='store_true', help='ignore conf["data_dir"] and train on synthetic batches')
    ap.add_argument('--evaluate', default='', help='model within hyperparameter folder to score on the test split (loss, L1, PSNR, SSIM)')
    ap.add_argument('--eval_batches', type=int, default=19, help='batches --evaluate scores (the reference tests 19)')
    ap.add_argument('--event_log', action='store_true', help='also write the scalars as TensorFlow event files')
    ap.add_argument('--raw_weights', action='store_true',
                    help="--evaluate / --visualize on the variables themselves, not on the averaged weights of conf['ema_decay'] "
                         "(the periodic val_loss during training is always computed on the raw weights)")
    FLAGS = ap.parse_args(argv)
    if FLAGS.visualize and FLAGS.evaluate:
        ap.error('--visualize and --evaluate exclude each other')

    conf = load_conf(FLAGS.hyper)
    if FLAGS.visualize:                                               # train.py:47-55
        print('creating visualizations ...')
        conf['data_dir'] = '/'.join(str.split(conf.get('data_dir') or '', '/')[:-1] + ['test'])
        conf['visualize'] = conf['output_dir'] + '/' + FLAGS.visualize
        conf['event_log_dir'] = '/tmp'
        conf['batch_size'] = 10
        conf['test_mode'] = ''
    if FLAGS.evaluate:                                                # the test split, as --visualize selects it
        conf['data_dir'] = '/'.join(str.split(conf.get('data_dir') or '', '/')[:-1] + ['test'])
        conf['test_mode'] = ''
    if FLAGS.num_iterations is not None:
        conf['num_iterations'] = FLAGS.num_iterations

    from . import parallel
    rank, world, local_rank = parallel.init_from_env()
    dev = 'cuda:%d' % (local_rank if world > 1 else int(FLAGS.device))
    torch.cuda.set_device(torch.device(dev))

    Model = select_model(conf)
    model = Model(conf, load_tfrec=True, build_loss=not FLAGS.visualize, device=dev)
    if world > 1:
        comm = parallel.make_comm(rank, world, 'rccl' if torch.cuda.is_available() else 'gloo')
        model.enable_data_parallel(world, comm=comm)
    saver = model.saver
    data_dir = conf.get('data_dir')
    if not FLAGS.synthetic and data_dir and os.path.isdir(data_dir) and os.listdir(data_dir):
        # the reference's shards (multi_view_model/utils/read_tf_records.py:15-85), read without TensorFlow
        from .read_tf_records import build_tfrecord_input
        train_data = build_tfrecord_input(conf, model, training=True, seed=rank, rank=rank, world=world)
        val_data = build_tfrecord_input(conf, model, training=False, seed=10_000 + rank)
        if rank == 0:
            print('reading TFRecord shards from', data_dir)
    else:
        if rank == 0:
            print('no TFRecord shards at conf["data_dir"] = %r: training on synthetic batches' % (data_dir,))
        train_data = SyntheticData(model, seed=rank)
        val_data = SyntheticData(model, seed=10_000 + rank, pool=1)
        from . import augment
        if augment.augment_from_conf(conf).enabled and 'test_mode' not in conf:
            # the pool is cycled: without this the same four batches would repeat forever.  Copies, so that the pool stays pristine
            shapes = {k: tuple(t.shape) for k, t in model.graph.inputs.items()}
            train_data = augment.AugmentedData(train_data, augment.ColorAugment(conf, shapes, device=model.graph.device, rank=rank))
        if augment.geom_from_conf(conf).enabled and 'test_mode' not in conf:
            # behind the colour stage (its contrast pivot is a sum in pixel order), in front of the mirror; copies, as above
            shapes = {k: tuple(t.shape) for k, t in model.graph.inputs.items()}
            train_data = augment.GeomAugmentedData(train_data, augment.GeomAugment(conf, shapes, device=model.graph.device, rank=rank))
        from . import pair_swap
        if pair_swap.pair_swap_from_conf(conf):
            # the first half of every synthetic batch and its reverses, behind the colour stage: the layout the graph's batch has
            # for training, validation, --evaluate and --visualize alike
            stage = pair_swap.PairSwap(conf, next(iter(model.graph.inputs.values())).shape[0])       # the graph's batch, as the reader takes it
            train_data, val_data = pair_swap.PairSwappedData(train_data, stage), pair_swap.PairSwappedData(val_data, stage)

    if FLAGS.visualize:                                               # train.py:80-92
        print('-------------------------------------------------------------------')
        print('verify current settings!! ')
        for key in conf.keys():
            print(key, ': ', conf[key])
        print('-------------------------------------------------------------------')
        saver.restore(None, conf['visualize'])
        print('restore done.')
        if model.graph.ema is not None and not FLAGS.raw_weights:
            with model.ema_weights():
                model.visualize(None, **train_data.next())
        else:
            model.visualize(None, **train_data.next())
        return model

    if FLAGS.evaluate:
        return evaluate_checkpoint(model, conf, FLAGS.evaluate, train_data, FLAGS.eval_batches, FLAGS.event_log and rank == 0,
                                   write=rank == 0, weights='raw' if FLAGS.raw_weights else None)

    itr_0 = 0
    if FLAGS.pretrained is not None:
        conf['pretrained_model'] = FLAGS.pretrained
        saver.restore(None, conf['pretrained_model'])
        from .model_base import iteration_from_checkpoint_name
        itr_0 = iteration_from_checkpoint_name(conf['pretrained_model'])      # train.py:99-101
        print('resuming training at iteration:  ', itr_0)
        g = model.graph
        if g.counts_updates() and not g.global_step_restored:
            g.set_global_step(itr_0)            # a checkpoint from before the switch: the schedule continues at the file name's iteration

    if rank == 0:
        print('-------------------------------------------------------------------')
        print('verify current settings!! ')
        for key in conf.keys():
            print(key, ': ', conf[key])
        print('-------------------------------------------------------------------')
        os.makedirs(conf['output_dir'], exist_ok=True)
        log = open(os.path.join(conf['output_dir'], 'train_log.jsonl'), 'a')
    events = _event_writer(conf) if FLAGS.event_log and rank == 0 else None

    # The launch thread runs tens of milliseconds ahead of the GPU; a full cyclic-GC pass over everything the imports and
    # the graph construction left behind takes longer than that and drains the queues.  Move those objects to the
    # permanent generation: later collections only look at what the loop itself allocates.
    import gc
    gc.collect()
    gc.freeze()

    train_loop(model, conf, train_data, val_data, saver, itr_0, rank, log if rank == 0 else None, events)
    model.graph.gather_optimizer_state()
    if rank == 0:
        print('Saving model.')
        saver.save(None, conf['output_dir'] + '/model')
        log.close()
        if events is not None:
            events.close()
        print('Training complete')
    return model


if __name__ == '__main__':
    main()
