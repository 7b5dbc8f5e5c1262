"""Pair-swapped batches: every rendered pair is used in both directions inside one batch.

A record holds image0, image1, depth0, depth1 and displacement = (el1 - el0, az1 - az0) (the reference's
utils/render_multiobj.py:364,386).  The reversed pair is the same record read backwards: the images exchanged, the depths
exchanged, the displacement negated.  With conf['pair_swap'] = True a batch of B = conf['batch_size'] samples is made out of B/2
records:

  samples 0 .. B/2-1      the records as read
  sample  n + B/2         record n reversed: image0 <-> image1, depth_image0 <-> depth_image1, disp -> -disp

This doubles the supervision per rendered pair and puts both flows of a pair into one forward pass, which is what the
forward-backward consistency term (tf_utils.flow_consistency_loss, conf['flow_consistency_weight']) needs: the partner of sample n
is sample (n + B/2) mod B.  The layout is a property of the graph's batch, not of training: the TFRecord reader and the synthetic
feed build it for training, validation, --evaluate and --visualize alike; under data parallelism every rank mirrors its own batch,
and with gradient accumulation every micro-batch is mirrored.  The mirror runs BEHIND the colour augmentation (augment.py), which
draws one colour map per record: image0[n + B/2] equals image1[n] bit for bit after augmentation.

The key alone, without the consistency weight, is a valid augmentation for every model whose inputs are exactly the five reader
tensors (the appearance-flow family and Base_Prediction_Model, which names its depth pair dimage0 / dimage1: the stage takes the
pairs it exchanges from the batch's own names, swapped_pairs()).  The multi-object models (13 reader tensors, image1_only0/1 have
no reverse) and the mv3d networks refuse it (ModelBase._check_conf).  Absent, None or False: the batches are what they were.
"""
import numpy as np

IMAGES = ('image0', 'image1')
DEPTHS = (('depth_image0', 'depth_image1'), ('dimage0', 'dimage1'))     # the appearance-flow family's names, Base_Prediction_Model's
SWAPPED = (IMAGES, DEPTHS[0])
NEGATED = ('disp',)
NAMES = tuple(n for pair in SWAPPED for n in pair) + NEGATED


def swapped_pairs(names):
    """The pairs of inputs that a reverse exchanges, for a model's input names: the two views and ONE depth pair, under either of
    its names, beside `disp`.  ValueError for any other set of inputs: a sample of such a model has no reverse."""
    names = set(names)
    for depth in DEPTHS:
        if names == set(IMAGES) | set(depth) | set(NEGATED):
            return (IMAGES, depth)
    raise ValueError("pair_swap: a batch must hold exactly the inputs %s (the depth pair may be named %s instead; a sample of any "
                     "other model has no reverse), got %s" % (sorted(NAMES), list(DEPTHS[1]), sorted(names)))


def pair_swap_from_conf(conf):
    """conf['pair_swap'] as a bool: False when the key is absent, None or False.  Raises ValueError for a value that is no bool and,
    with the switch on, for a conf['batch_size'] that is odd (or smaller than 2), before any device work."""
    v = conf.get('pair_swap')
    if v is None:
        return False
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("conf['pair_swap'] must be True or False (or None for off), got %r" % (v,))
    if not v:
        return False
    b = conf.get('batch_size')
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 2 or b % 2:
        raise ValueError("conf['pair_swap'] needs an even conf['batch_size'] >= 2 (a batch is B/2 records and their reverses), got %r" % (b,))
    return True


def _check_names(batch):
    swapped_pairs(batch)
    rows = {int(v.shape[0]) for v in batch.values()}
    if len(rows) != 1:
        raise ValueError("pair_swap: the inputs of a batch differ in their number of samples: %s" % sorted(rows))
    return rows.pop()


def mirror_host(batch):
    """The numpy statement: {name: array of h records} -> {name: array of 2 h samples}, the records followed by their reverses."""
    _check_names(batch)
    b = {k: np.asarray(v) for k, v in batch.items()}
    out = {}
    for x, y in swapped_pairs(batch):
        out[x] = np.concatenate([b[x], b[y]], axis=0)
        out[y] = np.concatenate([b[y], b[x]], axis=0)
    for k in NEGATED:
        out[k] = np.concatenate([b[k], np.negative(b[k])], axis=0)
    return {k: out[k] for k in batch}


class PairSwap:
    """The mirror stage of an input: `apply(batch, stream)` turns {name: torch tensor of h records} into {name: tensor of 2 h
    samples} on the tensors' device with device-to-device copies and one negation (torch plumbing, no kernel of its own), on
    `stream` (a torch.cuda.Stream; None = the current one).  On the CPU the same with host copies."""

    def __init__(self, conf, batch=None):
        if not pair_swap_from_conf(conf):
            raise ValueError("PairSwap: conf['pair_swap'] is off")
        batch = int(conf['batch_size'] if batch is None else batch)     # the graph's batch where the caller knows it
        if batch < 2 or batch % 2:
            raise ValueError("pair_swap needs an even batch of at least 2 samples, got %d" % batch)
        self.half = batch // 2

    def apply(self, batch, stream=None):
        import torch
        h = _check_names(batch)
        if h != self.half:
            raise ValueError("pair_swap: a batch of %d records for conf['batch_size'] = %d (expected %d)" % (h, 2 * self.half, self.half))

        def run():
            out = {}
            for x, y in swapped_pairs(batch):
                for dst, first, second in ((x, batch[x], batch[y]), (y, batch[y], batch[x])):
                    full = torch.empty((2 * h,) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
                    full[:h].copy_(first, non_blocking=True)
                    full[h:].copy_(second, non_blocking=True)
                    out[dst] = full
            for k in NEGATED:
                v = batch[k]
                full = torch.empty((2 * h,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
                full[:h].copy_(v, non_blocking=True)
                torch.neg(v, out=full[h:])
                out[k] = full
            return {k: out[k] for k in batch}
        if stream is not None:
            with torch.cuda.stream(stream):
                return run()
        return run()


class PairSwappedData:
    """A batch source whose next() hands out the mirrored form of the first half of source.next(): what the synthetic feed (and any
    source of full batches) goes through with conf['pair_swap'] on.  It runs behind the source's own stages (an augmented copy is
    mirrored after its colour maps were applied), so both directions of a pair carry the same colours."""

    def __init__(self, source, stage):
        self.source, self.stage = source, stage

    def next(self):
        h = self.stage.half
        return self.stage.apply({k: v[:h] for k, v in self.source.next().items()})

    def __getattr__(self, name):
        return getattr(self.source, name)
