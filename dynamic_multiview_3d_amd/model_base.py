"""Shared machinery of the model classes: graph ownership, feeding, stepping, checkpoints.

The reference classes own a TF graph + placeholders and are driven by
sess.run([model.loss, model.train_op], {model.train_cond: 1}) (multi_view_model/train.py:120-123).
Here `train_step(**feeds)` / `forward(**feeds)` are the explicit replacements of those
sess.run calls; everything else keeps the reference attribute names.
"""
import os
import re

import numpy as np
import torch

from . import tf_checkpoint
from .graph import Graph, ema_one_minus_decay, ema_rule      # noqa: F401  (the numpy twins of mv3d_ema_step are part of this module's interface)
from .graph import grad_clip_rule                            # noqa: F401  (... and the twin of mv3d_grad_clip_scale)
from .graph import grad_accum_rule                           # noqa: F401  (... and the twin of mv3d_grad_accumulate)
from .graph import weight_decay_rule, weight_decay_factor    # noqa: F401  (... and the twin of mv3d_weight_decay_step)
from .lr_schedule import learning_rate_at, lr_schedule_from_conf, weight_decay_from_conf      # noqa: F401


class Saver:
    """tf.train.Saver stand-in (train.py:70-71,134-136; mv3d/utils/tf_utils.py:199-212): variables + the optimiser's slots
    (Adam: m, v and the beta powers; Momentum: the accumulator; GD: none) under their TF names, written as a TensorFlow V2 checkpoint (`<prefix>.index`,
    `<prefix>.data-00000-of-00001`, and the `checkpoint` state file next to them) -- see tf_checkpoint.py."""

    def __init__(self, graph):
        self.graph = graph

    def save(self, sess, save_path, global_step=None):
        prefix = save_path if global_step is None else '%s-%d' % (save_path, int(global_step))
        prefix = os.path.abspath(prefix)
        tf_checkpoint.write_checkpoint(prefix, {k: v.numpy() for k, v in self.graph.state_dict().items()})
        tf_checkpoint.update_checkpoint_state(os.path.dirname(prefix), prefix)
        return prefix

    def restore(self, sess, save_path):
        if tf_checkpoint.checkpoint_exists(save_path):
            arrays = tf_checkpoint.read_checkpoint(save_path)
            self.graph.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in arrays.items()})
        elif os.path.isfile(save_path):                      # state dict written by torch.save (pre-bundle snapshots)
            self.graph.load_state_dict(torch.load(save_path, map_location='cpu', weights_only=True))      # tensors only: never unpickle objects
        else:
            raise FileNotFoundError("no checkpoint at %r (expected %s.index)" % (save_path, save_path))


class AdamOptimizer:
    """tf.train.AdamOptimizer(lr).minimize(loss) (appearance_flow_model.py:77): TF defaults
    beta1=0.9, beta2=0.999, epsilon=1e-8; the update itself is mv3d_adam_step."""

    def __init__(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.beta1, self.beta2, self.eps = learning_rate, beta1, beta2, epsilon

    def minimize(self, loss, graph):
        graph.loss_expr = loss
        graph.lr = self.lr
        graph.optimizer = 'adam'
        graph.beta1, graph.beta2, graph.eps = self.beta1, self.beta2, self.eps
        return 'train_op'


class GradientDescentOptimizer:
    """tf.train.GradientDescentOptimizer(lr).minimize(loss): ApplyGradientDescent, p -= g*lr (mv3d_sgd_step); no slots."""

    def __init__(self, learning_rate):
        self.lr = learning_rate

    def minimize(self, loss, graph):
        graph.loss_expr = loss
        graph.lr = self.lr
        graph.optimizer = 'sgd'
        graph.momentum, graph.use_nesterov = 0.0, False
        return 'train_op'


class MomentumOptimizer:
    """tf.train.MomentumOptimizer(lr, momentum, use_nesterov=False).minimize(loss): ApplyMomentum (mv3d_sgd_step with the
    accumulator); one slot, <var>/Momentum."""

    def __init__(self, learning_rate, momentum, use_nesterov=False):
        self.lr, self.momentum, self.use_nesterov = learning_rate, momentum, bool(use_nesterov)

    def minimize(self, loss, graph):
        graph.loss_expr = loss
        graph.lr = self.lr
        graph.optimizer = 'momentum'
        graph.momentum, graph.use_nesterov = self.momentum, self.use_nesterov
        return 'train_op'


def optimizer_from_conf(conf, learning_rate, **adam_kw):
    """The optimiser a configuration asks for: conf['optimizer'] in {'adam' (default when absent), 'momentum', 'sgd'};
    'momentum' needs conf['momentum'] (TF has no default) and takes conf['use_nesterov'] (default False).  adam_kw: the model's
    own AdamOptimizer arguments.  Raises ValueError on anything else, before any device work."""
    name = conf.get('optimizer', 'adam')
    if name == 'adam':
        return AdamOptimizer(learning_rate, **adam_kw)
    if name == 'sgd':
        return GradientDescentOptimizer(learning_rate)
    if name == 'momentum':
        if conf.get('momentum') is None:
            raise ValueError("conf['optimizer'] = 'momentum' needs conf['momentum']")
        return MomentumOptimizer(learning_rate, float(conf['momentum']), bool(conf.get('use_nesterov', False)))
    raise ValueError("unknown conf['optimizer'] %r (have 'adam', 'momentum', 'sgd')" % (name,))


def ema_from_conf(conf):
    """(decay or None, num_updates) of the EMA-weights switch: conf['ema_decay'] absent, None or 0 = off (the graph then records
    and launches exactly what it did without the key); otherwise tf.train.ExponentialMovingAverage's decay, finite and in (0, 1).
    conf['ema_num_updates'] (default False) hands TF's num_updates to it: decay_t = min(decay, (1 + n) / (10 + n)).  Raises
    ValueError on a value out of range, before any device work."""
    decay = conf.get('ema_decay')
    num_updates = bool(conf.get('ema_num_updates', False))
    if decay is None or (not isinstance(decay, bool) and decay == 0):
        return None, num_updates
    if isinstance(decay, bool):
        raise ValueError("conf['ema_decay'] must be a number in (0, 1), got %r" % (decay,))
    decay = float(decay)
    if not np.isfinite(decay) or not 0.0 < decay < 1.0:
        raise ValueError("conf['ema_decay'] must be finite and in (0, 1) (or 0 / None for off), got %r" % (conf['ema_decay'],))
    return decay, num_updates


def grad_clip_from_conf(conf):
    """The clip norm Graph.enable_grad_clip takes, or None for off (the graph then allocates, records and launches exactly what it
    did without the keys).  conf['grad_clip_norm'] = c, finite and > 0, clips every step's gradient to the global L2 norm c;
    conf['grad_norm_log'] = True without a clip norm only measures (math.inf); absent, None, 0 or False is off.  A bool, a
    negative value, NaN or inf for grad_clip_norm raises ValueError, before any device work."""
    import math
    c = conf.get('grad_clip_norm')
    if isinstance(c, bool):
        raise ValueError("conf['grad_clip_norm'] must be a number > 0 (or 0 / None for off), got %r" % (c,))
    if c is None or c == 0:
        return math.inf if conf.get('grad_norm_log') else None
    c = float(c)
    with np.errstate(over='ignore', under='ignore'):
        c32 = float(np.float32(c))                  # what the kernel is handed
    if not math.isfinite(c) or not c > 0.0 or not 0.0 < c32 < math.inf:
        raise ValueError("conf['grad_clip_norm'] must be finite (as a float32) and > 0 (or 0 / None for off), got %r" % (conf['grad_clip_norm'],))
    return c


def grad_accum_from_conf(conf):
    """The N Graph.enable_grad_accum takes, or None for off (the graph then allocates, records and launches exactly what it did
    without the key).  conf['grad_accum_steps'] = N, an integer >= 2, makes one optimiser update out of N train steps
    (micro-batches of conf['batch_size'] each); absent, None, 0 or 1 is off.  A bool, a non-integer or a negative value raises
    ValueError, before any device work."""
    n = conf.get('grad_accum_steps')
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError("conf['grad_accum_steps'] must be an integer >= 2 (or None / 0 / 1 for off), got %r" % (n,))
    return int(n) if n >= 2 else None


def ssim_weight_from_conf(conf):
    """conf['ssim_loss_weight'] as a float: 0.0 when the key is absent (or None), which leaves the loss as the reference
    defines it.  Raises ValueError on a negative or non-finite value, before any device work."""
    w = conf.get('ssim_loss_weight')
    if w is None:
        return 0.0
    w = float(w)
    if not np.isfinite(w) or w < 0:
        raise ValueError("conf['ssim_loss_weight'] must be finite and >= 0, got %r" % (conf['ssim_loss_weight'],))
    return w


def census_from_conf(conf):
    """(weight, radius, eps) of the census-loss switch: conf['census_loss_weight'] (0.0 when absent or None, which leaves the loss
    and the recorded plans as they are), conf['census_loss_radius'] (default 3, an int in 1..3) and conf['census_loss_eps'] (the
    Charbonnier epsilon, default 0.01).  Raises ValueError on a value out of range, before any device work."""
    w = conf.get('census_loss_weight')
    w = 0.0 if w is None else float(w)
    if not np.isfinite(w) or w < 0:
        raise ValueError("conf['census_loss_weight'] must be finite and >= 0, got %r" % (conf['census_loss_weight'],))
    radius = conf.get('census_loss_radius')
    radius = 3 if radius is None else radius
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= 3:
        raise ValueError("conf['census_loss_radius'] must be an integer in 1..3, got %r" % (radius,))
    eps = conf.get('census_loss_eps')
    eps = 0.01 if eps is None else float(eps)
    if not np.isfinite(eps) or eps <= 0:
        raise ValueError("conf['census_loss_eps'] must be finite and > 0, got %r" % (conf['census_loss_eps'],))
    return w, int(radius), eps


def flow_smoothness_from_conf(conf):
    """(weight, edge_alpha, eps) of the flow-smoothness switch: conf['flow_smoothness_weight'] (0.0 when absent or None, which
    leaves the loss and the recorded plans as they are), conf['flow_smoothness_edge'] (default 10; 0 or None = unguided: no guide
    is read) and conf['flow_smoothness_eps'] (default 1e-3 pixels).  Raises ValueError on a value out of range, before any
    device work."""
    w = conf.get('flow_smoothness_weight')
    w = 0.0 if w is None else float(w)
    if not np.isfinite(w) or w < 0:
        raise ValueError("conf['flow_smoothness_weight'] must be finite and >= 0, got %r" % (conf['flow_smoothness_weight'],))
    alpha = conf.get('flow_smoothness_edge', 10.0)
    alpha = 0.0 if alpha is None else float(alpha)
    if not np.isfinite(alpha) or alpha < 0:
        raise ValueError("conf['flow_smoothness_edge'] must be finite and >= 0, got %r" % (conf['flow_smoothness_edge'],))
    eps = conf.get('flow_smoothness_eps')
    eps = 1e-3 if eps is None else float(eps)
    if not np.isfinite(eps) or eps <= 0:
        raise ValueError("conf['flow_smoothness_eps'] must be finite and > 0, got %r" % (conf['flow_smoothness_eps'],))
    return w, alpha, eps


def flow_smoothness_order_from_conf(conf):
    """1 or 2: conf['flow_smoothness_order'], the order of the differences conf['flow_smoothness_weight'] penalises.  1 (absent,
    None or 1): first differences, minimal for a constant flow, exactly as without the key.  2: second differences
    (mv3d_flow_smoothness2), minimal for an affine flow, with the same edge and eps keys.  Raises ValueError on a bool, a
    non-integer or any other value, whether or not the weight is set, before any device work."""
    order = conf.get('flow_smoothness_order')
    if order is None:
        return 1
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order not in (1, 2):
        raise ValueError("conf['flow_smoothness_order'] must be 1 or 2, got %r" % (order,))
    return int(order)


def flow_consistency_from_conf(conf):
    """(weight, eps) of the forward-backward consistency switch: conf['flow_consistency_weight'] (0.0 when absent, None or 0, which
    leaves the loss and the recorded plans as they are) and conf['flow_consistency_eps'] (the Charbonnier epsilon in pixels,
    default 1e-3).  A positive weight needs conf['pair_swap'] (pair_swap.py): without it the two halves of a batch are unrelated
    samples and the term means nothing.  Raises ValueError on a bool, a negative or non-finite weight, a bad eps, or a positive
    weight without conf['pair_swap'], before any device work."""
    from .pair_swap import pair_swap_from_conf
    w = conf.get('flow_consistency_weight')
    if isinstance(w, bool):
        raise ValueError("conf['flow_consistency_weight'] must be a number >= 0 (or None for off), got %r" % (w,))
    w = 0.0 if w is None else float(w)
    if not np.isfinite(w) or w < 0:
        raise ValueError("conf['flow_consistency_weight'] must be finite and >= 0, got %r" % (conf['flow_consistency_weight'],))
    eps = conf.get('flow_consistency_eps')
    if isinstance(eps, bool):
        raise ValueError("conf['flow_consistency_eps'] must be a number > 0, got %r" % (eps,))
    eps = 1e-3 if eps is None else float(eps)
    if not np.isfinite(eps) or eps <= 0:
        raise ValueError("conf['flow_consistency_eps'] must be finite and > 0, got %r" % (conf['flow_consistency_eps'],))
    if not float(np.float32(eps) * np.float32(eps)) >= float(np.finfo(np.float32).tiny):
        raise ValueError("conf['flow_consistency_eps'] must be at least 2^-63 (its square must not underflow in float32), got %r" % (eps,))
    if w > 0 and not pair_swap_from_conf(conf):
        raise ValueError("conf['flow_consistency_weight'] needs conf['pair_swap'] = True: the term pairs sample n of a batch with "
                         "sample n + batch_size / 2, which the pair-swapped feed makes the reversed pair")
    return w, eps


def occlusion_from_conf(conf):
    """None, or (alpha1, alpha2, outside_visible) of the occlusion-mask switch: conf['occlusion_mask'] (absent, None or False = off,
    which leaves the loss and the recorded plans as they are), conf['occlusion_alpha1'] (default 0.01), conf['occlusion_alpha2']
    (default 0.5, in pixels squared) and conf['occlusion_outside'] ('keep', the default: a pixel whose flow leaves the image keeps
    its loss, or 'mask': it loses it, UnFlow's choice).  The switch needs conf['pair_swap'] (pair_swap.py): the mask comes from the
    forward-backward residual of sample n against sample n + batch_size / 2.  Combined with conf['ssim_loss_weight'] or
    conf['census_loss_weight'] the switch is refused unless conf['occlusion_mask_image_terms'] opts into their masked forms
    (occlusion_image_terms_from_conf), and combined with conf['multiscale_loss_levels'] unless conf['occlusion_mask_multiscale']
    opts into the masked multi-scale term (occlusion_multiscale_from_conf).  Raises ValueError on a non-bool switch, a bool, negative or non-finite alpha1, an alpha2 <= 0, an unknown
    conf['occlusion_outside'], a missing conf['pair_swap'] or one of those combinations, before any device work."""
    from .pair_swap import pair_swap_from_conf
    on = conf.get('occlusion_mask')
    if on is not None and not isinstance(on, (bool, np.bool_)):
        raise ValueError("conf['occlusion_mask'] must be True or False (or None for off), got %r" % (on,))
    alphas = []
    for key, default in (('occlusion_alpha1', 0.01), ('occlusion_alpha2', 0.5)):
        v = conf.get(key)
        if isinstance(v, (bool, np.bool_)) or isinstance(v, str):
            raise ValueError("conf[%r] must be a number, got %r" % (key, v))
        v = default if v is None else float(v)
        if not np.isfinite(v) or not np.isfinite(np.float32(v)):
            raise ValueError("conf[%r] must be finite, got %r" % (key, conf[key]))
        alphas.append(v)
    if alphas[0] < 0:
        raise ValueError("conf['occlusion_alpha1'] must be >= 0, got %r" % (conf['occlusion_alpha1'],))
    if alphas[1] <= 0 or not float(np.float32(alphas[1])) > 0:
        raise ValueError("conf['occlusion_alpha2'] must be > 0, got %r" % (conf['occlusion_alpha2'],))
    outside = conf.get('occlusion_outside')
    outside = 'keep' if outside is None else outside
    if outside not in ('keep', 'mask'):
        raise ValueError("conf['occlusion_outside'] must be 'keep' or 'mask', got %r" % (outside,))
    if not on:
        return None
    if not pair_swap_from_conf(conf):
        raise ValueError("conf['occlusion_mask'] needs conf['pair_swap'] = True: the mask pairs sample n of a batch with sample "
                         "n + batch_size / 2, which the pair-swapped feed makes the reversed pair")
    image_terms = _occlusion_image_terms_switch(conf)
    if ssim_weight_from_conf(conf) > 0 and not image_terms:
        raise ValueError("conf['occlusion_mask'] does not combine with conf['ssim_loss_weight']: the SSIM loss has no masked form "
                         "unless conf['occlusion_mask_image_terms'] = True asks for it")
    if census_from_conf(conf)[0] > 0 and not image_terms:
        raise ValueError("conf['occlusion_mask'] does not combine with conf['census_loss_weight']: the census loss has no masked form "
                         "unless conf['occlusion_mask_image_terms'] = True asks for it")
    if multiscale_loss_from_conf(conf)[0] > 0 and not _occlusion_multiscale_switch(conf):
        raise ValueError("conf['occlusion_mask'] does not combine with conf['multiscale_loss_levels']: the multi-scale loss has no masked form "
                         "unless conf['occlusion_mask_multiscale'] = True asks for it")
    return alphas[0], alphas[1], outside == 'keep'


def _occlusion_image_terms_switch(conf):
    """conf['occlusion_mask_image_terms'] as a bool (absent, None or False = off); ValueError on anything that is not a bool."""
    on = conf.get('occlusion_mask_image_terms')
    if on is not None and not isinstance(on, (bool, np.bool_)):
        raise ValueError("conf['occlusion_mask_image_terms'] must be True or False (or None for off), got %r" % (on,))
    return bool(on)


def occlusion_image_terms_from_conf(conf):
    """True when the SSIM and census terms take the head's occlusion mask: conf['occlusion_mask_image_terms'] (absent, None or
    False = off, which leaves every conf behaving, raising and recording as it did without the key).  True needs
    conf['occlusion_mask']: ssim_term() and census_term() then pass the mask head_loss() created (UnFlow's data term is the census
    loss under the forward-backward mask; DDFlow and ARFlow mask census and SSIM the same way), and conf['occlusion_mask']
    combines with conf['ssim_loss_weight'] and conf['census_loss_weight'].  With neither weight set the key changes nothing.
    Raises ValueError on a value that is not a bool (with the switch off as well) and on True without conf['occlusion_mask'], before
    any device work."""
    on = _occlusion_image_terms_switch(conf)
    if on and occlusion_from_conf(conf) is None:
        raise ValueError("conf['occlusion_mask_image_terms'] needs conf['occlusion_mask'] = True: the masked SSIM and census "
                         "terms take the occlusion_mask of the head loss")
    return on


def _occlusion_multiscale_switch(conf):
    """conf['occlusion_mask_multiscale'] as a bool (absent, None or False = off); ValueError on anything that is not a bool."""
    on = conf.get('occlusion_mask_multiscale')
    if on is not None and not isinstance(on, (bool, np.bool_)):
        raise ValueError("conf['occlusion_mask_multiscale'] must be True or False (or None for off), got %r" % (on,))
    return bool(on)


def occlusion_multiscale_from_conf(conf):
    """True when the multi-scale term takes the head's occlusion mask: conf['occlusion_mask_multiscale'] (absent, None or False =
    off, which leaves every conf behaving, raising and recording as it did without the key).  True needs conf['occlusion_mask']:
    multiscale_term() then passes the mask head_loss() created for its flow, pooled level by level like the images (UnFlow, DDFlow
    and ARFlow apply the forward-backward mask at every pyramid level), and conf['occlusion_mask'] combines with
    conf['multiscale_loss_levels'].  With the multi-scale switch off the key changes nothing.  The smoothness and consistency
    terms stay unmasked.  Raises ValueError on a value that is not a bool (with the switches off as well) and on True without
    conf['occlusion_mask'], before any device work."""
    on = _occlusion_multiscale_switch(conf)
    if on and occlusion_from_conf(conf) is None:
        raise ValueError("conf['occlusion_mask_multiscale'] needs conf['occlusion_mask'] = True: the masked multi-scale term takes "
                         "the occlusion_mask of the head loss")
    return on


def multiscale_loss_from_conf(conf):
    """(levels, [w_1 .. w_levels], kind) of the multi-scale photometric switch: conf['multiscale_loss_levels'] (1..3; absent, None
    or 0 = off), conf['multiscale_loss_weight'] (a scalar applied to every level or a list of one weight per level, default 1.0)
    and conf['multiscale_loss_kind'] ('l2', the default, or 'l1').  levels is 0 when the switch is off or every weight is 0, which
    leaves the loss and the recorded plans as they are.  Raises ValueError on a value out of range, before any device work."""
    levels = conf.get('multiscale_loss_levels')
    if levels is None or (not isinstance(levels, bool) and levels == 0):
        return 0, [], 'l2'
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= 3:
        raise ValueError("conf['multiscale_loss_levels'] must be an integer in 1..3 (or 0 / None for off), got %r" % (levels,))
    levels = int(levels)
    w = conf.get('multiscale_loss_weight')
    w = 1.0 if w is None else w
    if isinstance(w, (list, tuple, np.ndarray)):
        weights = [float(v) for v in w]
        if len(weights) != levels:
            raise ValueError("conf['multiscale_loss_weight'] lists %d weights for %d levels" % (len(weights), levels))
    else:
        weights = [float(w)] * levels
    if not all(np.isfinite(v) and v >= 0 for v in weights):
        raise ValueError("conf['multiscale_loss_weight'] must be finite and >= 0, got %r" % (conf['multiscale_loss_weight'],))
    kind = conf.get('multiscale_loss_kind')
    kind = 'l2' if kind is None else kind
    if kind not in ('l1', 'l2'):
        raise ValueError("conf['multiscale_loss_kind'] must be 'l2' or 'l1', got %r" % (kind,))
    if not any(weights):
        return 0, [], kind
    return levels, weights, kind


class ModelBase(object):
    input_names = ()
    supports_ssim_loss = False      # the classes whose build_loss() adds ssim_term() and census_term() set it
    supports_flow_smoothness = False        # the classes whose build_loss() adds flow_smoothness_term() set it
    supports_multiscale_loss = False        # the classes whose build_loss() adds multiscale_term() set it
    supports_flow_consistency = False       # the classes whose build_loss() adds flow_consistency_term() set it
    supports_pair_swap = False              # the classes whose inputs are exactly the reader's five tensors (pair_swap.py)
    supports_occlusion_mask = False         # the classes whose build_loss() takes its photometric term from head_loss()
    supports_geom_augment = False           # the classes whose pose input is the RELATIVE pose disp of a pair (augment.GeomAugment)

    def _check_conf(self):
        """Keys that would otherwise be ignored silently; called by a constructor before it builds the graph."""
        if ssim_weight_from_conf(self.conf) > 0 and not self.supports_ssim_loss:
            raise ValueError("%s does not support conf['ssim_loss_weight']" % type(self).__name__)
        if census_from_conf(self.conf)[0] > 0 and not self.supports_ssim_loss:
            raise ValueError("%s does not support conf['census_loss_weight']" % type(self).__name__)
        if flow_smoothness_from_conf(self.conf)[0] > 0 and not self.supports_flow_smoothness:
            raise ValueError("%s does not support conf['flow_smoothness_weight']" % type(self).__name__)
        flow_smoothness_order_from_conf(self.conf)          # a bad order is refused whether or not the weight is set
        if multiscale_loss_from_conf(self.conf)[0] > 0 and not self.supports_multiscale_loss:
            raise ValueError("%s has no flow: it does not support conf['multiscale_loss_levels']" % type(self).__name__)
        from .pair_swap import pair_swap_from_conf
        if pair_swap_from_conf(self.conf) and not self.supports_pair_swap:
            raise ValueError("%s does not support conf['pair_swap']: its inputs are not the five reader tensors of one pair, so "
                             "a sample has no reverse" % type(self).__name__)
        if flow_consistency_from_conf(self.conf)[0] > 0 and not self.supports_flow_consistency:
            raise ValueError("%s does not support conf['flow_consistency_weight']" % type(self).__name__)
        if occlusion_from_conf(self.conf) is not None and not self.supports_occlusion_mask:
            raise ValueError("%s does not support conf['occlusion_mask']" % type(self).__name__)
        if occlusion_image_terms_from_conf(self.conf) and not self.supports_occlusion_mask:
            raise ValueError("%s does not support conf['occlusion_mask_image_terms']" % type(self).__name__)
        if occlusion_multiscale_from_conf(self.conf) and not self.supports_occlusion_mask:
            raise ValueError("%s does not support conf['occlusion_mask_multiscale']" % type(self).__name__)
        from .augment import geom_from_conf, GEOM_KEYS
        if geom_from_conf(self.conf).enabled and not self.supports_geom_augment:
            raise ValueError("%s does not support conf[%s]: its pose input is the absolute pose of a single view, under which no "
                             "flip, zoom or shift is exact" % (type(self).__name__, ' / '.join(repr(k) for k in GEOM_KEYS)))

    def _note_term(self, attr, entry):
        """One more entry of a per-term list that evaluate() reports from (_report); the list exists only once a term was added."""
        self.__dict__.setdefault(attr, []).append(entry)

    def head_loss(self, gen, target, flow, name='flow'):
        """The photometric term of an appearance-flow head: euclidean_loss(gen, target), exactly the reference's, when
        conf['occlusion_mask'] is absent, None or False (the graph then records what it recorded without the key); with the key on,
        masked_euclidean_loss(gen, target, occlusion_mask(flow, alpha1, alpha2, outside)) with the mask held constant.  The
        consistency term (conf['flow_consistency_weight']) stays unmasked: it is what keeps 'every pixel occluded' from being a
        minimum of the masked loss.  evaluate() reports the mask's shares as '<name>/visible', '<name>/occluded', '<name>/outside'."""
        from .tf_utils import euclidean_loss, masked_euclidean_loss, occlusion_mask
        occl = occlusion_from_conf(self.conf)
        if occl is None:
            return euclidean_loss(gen, target)
        mask = occlusion_mask(flow, *occl)
        self._note_term('occlusion_terms', (name, flow, mask) + tuple(occl))      # (name, flow, mask tensor, alpha1, alpha2, outside_visible)
        self._note_term('_head_masks', (gen, mask))
        return masked_euclidean_loss(gen, target, mask)

    def _image_term_mask(self, op, pred):
        """The mask ssim_term() / census_term() pass on: None unless conf['occlusion_mask_image_terms'] is on, then the occlusion
        mask head_loss() created for this prediction."""
        if not occlusion_image_terms_from_conf(self.conf):
            return None
        for gen, mask in getattr(self, '_head_masks', []):
            if gen is pred:
                return mask
        raise RuntimeError("%s: conf['occlusion_mask_image_terms'] is on, but head_loss() made no occlusion mask for this prediction "
                           "(call head_loss() first)" % op)

    def occlusion_mask(self, name='flow'):
        """The occlusion mask [B,H,W,1] of the last step (forward, train or evaluate) as a device tensor: a view of the graph's
        own buffer, overwritten by the next step.  Needs conf['occlusion_mask']."""
        for term in getattr(self, 'occlusion_terms', []):
            if term[0] == name:
                return term[2].value()
        raise RuntimeError("occlusion_mask: the model was built without conf['occlusion_mask'] (or without a loss)")

    def flow_visible(self, name='flow'):
        """The visible share of the last step's mask as a 0-d device tensor (train.py logs it: a mask that collapses shows here).
        One extra launch pair on the current flow; not part of the step."""
        from . import metrics
        for term in getattr(self, 'occlusion_terms', []):
            if term[0] == name:
                if self.graph.device.type != 'cuda':        # a CPU graph: the numpy form
                    return metrics.flow_occlusion_mask_host(term[1].numpy(), term[3], term[4], term[5])[1][0]
                stats = torch.zeros(3, dtype=torch.float32, device=self.graph.device)
                metrics.flow_occlusion_mask(term[1], term[3], term[4], term[5], stats=stats)
                return stats[0]
        raise RuntimeError("flow_visible: the model was built without conf['occlusion_mask'] (or without a loss)")

    def flow_consistency_term(self, flow, name='flow'):
        """conf['flow_consistency_weight'] * flow_consistency_loss(flow, eps) on one flow head, or 0 when the switch is absent or 0
        (the graph then records exactly what it recorded without the key).  evaluate() reports the unweighted term as
        '<name>/consistency' and the share of valid pixels as '<name>/consistency_valid'."""
        from .tf_utils import flow_consistency_loss
        w, eps = flow_consistency_from_conf(self.conf)
        if w == 0:
            return 0
        self._note_term('consistency_terms', (name, flow, eps))
        return flow_consistency_loss(flow, eps) * w

    def multiscale_term(self, flow, src, target, name='flow'):
        """multiscale_photometric_loss(flow, src, target) with the levels, weights and kind of conf['multiscale_loss_*'] on one flow
        head, or 0 when the switch is off (the graph then records exactly what it recorded without the keys).  Raises ValueError
        for an image size that is no multiple of 2^levels.  evaluate() reports the unweighted level terms as '<name>/photo_x2',
        '<name>/photo_x4', '<name>/photo_x8'.  With conf['occlusion_mask_multiscale'] the term takes the occlusion mask head_loss()
        made for this flow (multiscale_photometric_loss(..., mask=)); '<name>/photo_x*' stay the unmasked figures, comparable across
        runs, and '<name>/photo_x2_masked', '_x4_masked', '_x8_masked' are the unweighted level terms as trained."""
        from .tf_utils import multiscale_photometric_loss
        levels, weights, kind = multiscale_loss_from_conf(self.conf)
        if levels == 0:
            return 0
        mask = None
        if occlusion_multiscale_from_conf(self.conf):
            for term in getattr(self, 'occlusion_terms', []):
                if term[1] is flow:
                    mask = term[2]
            if mask is None:
                raise RuntimeError("multiscale_term: conf['occlusion_mask_multiscale'] is on, but head_loss() made no occlusion mask "
                                   "for this flow (call head_loss() first)")
        self._note_term('multiscale_terms', (name, flow, src, target, levels, kind))
        if mask is not None:
            self._note_term('masked_multiscale_terms', (name, flow, src, target, levels, kind, mask))
        return multiscale_photometric_loss(flow, src, target, levels, weights, kind, mask=mask)

    def flow_smoothness_term(self, flow, guide, name='flow'):
        """conf['flow_smoothness_weight'] * flow_smoothness_loss(flow, guide, edge, eps) on one flow head, or 0 when the switch is
        absent or 0 (the graph then records exactly what it recorded without the key).  The guide (the target view's colour
        image: the flow is indexed by output pixel) is dropped when conf['flow_smoothness_edge'] is 0 or None.  evaluate()
        reports the unweighted term as '<name>/smoothness'.  With conf['flow_smoothness_order'] = 2 the term is the second-order
        one (flow_smoothness_loss(..., order=2)) and evaluate() reports it as '<name>/smoothness2' and no '<name>/smoothness': the
        two figures are not comparable."""
        from .tf_utils import flow_smoothness_loss
        w, alpha, eps = flow_smoothness_from_conf(self.conf)
        order = flow_smoothness_order_from_conf(self.conf)
        if w == 0:
            return 0
        if alpha == 0:
            guide = None
        # (name, flow, guide or None, edge_alpha, eps)
        self._note_term('smoothness2_terms' if order == 2 else 'smoothness_terms', (name, flow, guide, alpha, eps))
        return flow_smoothness_loss(flow, guide, alpha, eps, order) * w

    def _eval_pair(self, op, pred, target):
        """(name, max_val) of this model's eval_pairs() entry for the pair."""
        for name, p, t, max_val in self.eval_pairs():
            if p is pred and t is target:
                return name, max_val
        raise RuntimeError("%s: eval_pairs() of %s has no entry for this pair" % (op, type(self).__name__))

    def ssim_term(self, pred, target):
        """conf['ssim_loss_weight'] * ssim_loss(pred, target, max_val) with max_val from this model's eval_pairs() entry of the
        pair, or 0 when the switch is absent or 0 (the graph then records exactly what it recorded without the key).  With
        conf['occlusion_mask_image_terms'] the term takes the head's occlusion mask (ssim_loss(..., mask=)), and evaluate() reports
        the unweighted masked term as '<pair>/ssim_loss_masked' ('<pair>/ssim' stays the unmasked figure)."""
        from .tf_utils import ssim_loss
        w = ssim_weight_from_conf(self.conf)
        if w == 0:
            return 0
        name, max_val = self._eval_pair('ssim_term', pred, target)
        mask = self._image_term_mask('ssim_term', pred)
        term = ssim_loss(pred, target, max_val, mask=mask) * w
        if mask is not None:
            self._note_term('masked_image_terms', (name, 'ssim_loss_masked', pred, target, mask, max_val, None, None))
        return term

    def census_term(self, pred, target):
        """conf['census_loss_weight'] * census_loss(pred, target, max_val, radius, eps) with max_val from this model's eval_pairs()
        entry of the pair and radius, eps from conf['census_loss_radius' / '_eps'], or 0 when the switch is absent or 0 (the graph
        then records exactly what it recorded without the key).  Raises ValueError for an image smaller than the patch.
        evaluate() reports the unweighted term as '<pair>/census'.  With conf['occlusion_mask_image_terms'] the term takes the head's
        occlusion mask (census_loss(..., mask=)); '<pair>/census' stays the unmasked figure, comparable across runs, and
        '<pair>/census_masked' is the unweighted term as trained."""
        from .tf_utils import census_loss
        w, radius, eps = census_from_conf(self.conf)
        if w == 0:
            return 0
        name, max_val = self._eval_pair('census_term', pred, target)
        mask = self._image_term_mask('census_term', pred)
        term = census_loss(pred, target, max_val, radius, eps, mask=mask) * w
        self._note_term('census_terms', (name, pred, target, max_val, radius, eps))        # name: the pair's
        if mask is not None:
            self._note_term('masked_image_terms', (name, 'census_masked', pred, target, mask, max_val, radius, eps))
        return term

    def _make_graph(self, device, seed):
        self._check_conf()
        ema_from_conf(self.conf)        # a bad conf['ema_decay'] raises here, before any device work
        grad_clip_from_conf(self.conf)  # ... and a bad conf['grad_clip_norm']
        grad_accum_from_conf(self.conf)  # ... and a bad conf['grad_accum_steps']
        from .augment import augment_from_conf, geom_from_conf
        augment_from_conf(self.conf)     # ... and a bad conf['augment_*'] (the input path's colour stage: augment.py)
        geom_from_conf(self.conf)        # ... and a bad conf['augment_flip' / '_zoom' / '_shift'] (its geometric stage)
        lr_schedule_from_conf(self.conf)  # ... and a bad, stray or misspelt conf['lr_*']
        weight_decay_from_conf(self.conf)  # ... and a bad conf['weight_decay']
        self.graph = Graph(device=device, seed=seed)
        return self.graph

    def _finish(self, build_loss):
        self.t_vars = list(self.graph.variables.keys())
        self.saver = Saver(self.graph)
        # EMA weights are a property of the graph, not of the loss: a build_loss=False model holds the shadows too, so that a
        # checkpoint can be restored and rendered with them
        decay, num_updates = ema_from_conf(self.conf)
        if decay is not None:
            self.graph.enable_ema(decay, num_updates)
        clip = grad_clip_from_conf(self.conf)
        if clip is not None and build_loss:     # a property of the train step: a model without a loss has no gradient
            self.graph.enable_grad_clip(clip)
        accum = grad_accum_from_conf(self.conf)
        if accum is not None and build_loss:    # likewise a property of the train step
            self.graph.enable_grad_accum(accum)
        if build_loss:                          # the rate and the decay belong to the optimiser's update
            self.graph.enable_lr_schedule(lr_schedule_from_conf(self.conf))
            self.graph.enable_weight_decay(weight_decay_from_conf(self.conf))
        self.graph.compile()

    def ema_weights(self):
        """Context manager: forward passes inside run on the averaged weights (Graph.ema_weights)."""
        return self.graph.ema_weights()

    # ---- sess.run replacements
    def feed(self, **feeds):
        for k, v in feeds.items():
            if v is None:
                continue
            if k not in self.graph.inputs:
                raise KeyError("unknown input %r (have %s)" % (k, list(self.graph.inputs)))
            self.graph.inputs[k].set(v)

    def train_step(self, **feeds):
        """One sess.run([model.loss, model.train_op], {train_cond: 1}); returns the loss as a
        0-d device tensor (call float() on it to synchronise).  With conf['grad_accum_steps'] = N one micro-step: the N-th call
        in a row updates the weights (Graph.run_micro_step)."""
        if self.graph.loss_expr is None:
            raise RuntimeError("model was built with build_loss=False")
        self.feed(**feeds)
        return self.graph.train_step()

    def forward(self, **feeds):
        """One forward pass (the train_cond: 0 / visualize path, train.py:130, appearance_flow_model.py:134)."""
        self.feed(**feeds)
        self.graph.run_forward()
        return self.graph.loss_buf[0]

    # ---- quantitative evaluation
    def eval_pairs(self):
        """[(name, prediction tensor, target tensor, max_val)]: what evaluate() scores.  max_val is the dynamic range of the
        TARGET as the reader / the reference's loader produces it; each model class states where its value comes from."""
        raise NotImplementedError("%s defines no eval_pairs()" % type(self).__name__)

    def evaluate(self, data, num_batches=19, weights=None):
        """_evaluate() on the weights asked for: 'raw' (the variables), 'ema' (the averaged weights, conf['ema_decay'] must be on)
        or None = 'ema' when the switch is on, else 'raw'.  With the switch on the result also names them: 'weights': 'ema' | 'raw';
        with it off the result is _evaluate()'s alone."""
        have = getattr(self.graph, 'ema', None) is not None
        if weights is None:
            weights = 'ema' if have else 'raw'
        if weights not in ('ema', 'raw'):
            raise ValueError("evaluate: weights must be 'ema', 'raw' or None, got %r" % (weights,))
        if weights == 'ema' and not have:
            raise ValueError("evaluate: weights='ema' needs conf['ema_decay']")
        if int(num_batches) < 1:
            raise ValueError("evaluate: num_batches must be at least 1")
        if weights == 'ema':
            with self.graph.ema_weights():
                result = self._evaluate(data, num_batches)
        else:
            result = self._evaluate(data, num_batches)
        if have:
            result['weights'] = weights
        return result

    def _evaluate(self, data, num_batches=19):
        """The quantitative counterpart of mv3d.test() (mv3d/nobg_dm.py:117-149): forward(**data.next()) num_batches times
        (19 = the reference's test_iter), the loss averaged over the batches (:143-145), and per-image L1 / PSNR / SSIM of every
        eval_pairs() entry averaged over the images (metrics.py; PSNR is averaged per image, an image with mse == 0 makes it inf).
        Every loss switch that is on adds its unweighted figures, averaged over the batches, under the keys its *_term() method or
        head_loss() names: _report() below is the table of everything reported.
        On the GPU every batch writes its figures (the device kernels') into its row of one device buffer and the host synchronises
        once, after the last batch.  On a CPU graph the numpy forms score each batch.
        Only forward passes run: parameters, optimiser slots and the step counter are left as they were.
        Returns {'loss': .., '<pair>/l1': .., '<pair>/psnr': .., '<pair>/ssim': .., 'images': count}."""
        g = self.graph
        num_batches = int(num_batches)
        if num_batches < 1:
            raise ValueError("evaluate: num_batches must be at least 1")
        pairs = self.eval_pairs()
        if not pairs:
            raise RuntimeError("evaluate: the built graph has no prediction / target pair")
        n = pairs[0][1].shape[0]
        report = self._report(pairs, n)
        on_gpu = g.device.type == 'cuda'
        starts = np.cumsum([0] + [e[0] for e in report])        # entry k owns columns starts[k] .. starts[k + 1] of every batch's row
        shape = (num_batches, int(starts[-1]))
        buf = torch.empty(shape, dtype=torch.float32, device=g.device) if on_gpu else np.empty(shape, np.float64)
        for i in range(num_batches):
            loss = self.forward(**data.next())
            for k, (_, device, host, _) in enumerate(report):
                if on_gpu:
                    device(buf[i, starts[k]:starts[k + 1]], loss)
                else:
                    buf[i, starts[k]:starts[k + 1]] = host(loss)
        if on_gpu:
            buf = buf.cpu().numpy().astype(np.float64)          # the one synchronisation
        result = {}
        for k, entry in enumerate(report):
            result.update(entry[3](buf[:, starts[k]:starts[k + 1]]))
        result['images'] = num_batches * n
        return result

    def _report(self, pairs, n):
        """What _evaluate() reports, in the order of the result's keys: one entry (columns, device, host, result) per quantity.
        `columns` float32 values per batch; device(out, loss) writes them into the dense device vector `out`, asynchronously;
        host(loss) returns them on a CPU graph (the numpy forms); result(block) turns the float64 [num_batches, columns] block into
        [(key, value)].  `loss` is what forward() returned for the batch."""
        from . import metrics
        ms_kind = {'l1': 1, 'l2': 2}

        def means(*keys):               # one key per column: the mean over the batches
            return lambda block: [(key, float(block[:, c].mean())) for c, key in enumerate(keys)]
        def into(value):                # a 0-d or [columns] device tensor -> out
            return lambda out, loss: out.copy_(value(loss).reshape(-1), non_blocking=True)
        def pair(name, pred, target, max_val):
            def result(block):          # per image, not per batch: PSNR is averaged over the images
                s = block.reshape(-1, 3)
                return [(name + '/l1', float(s[:, metrics.L1].mean())), (name + '/psnr', float(metrics.psnr(s[:, metrics.MSE], max_val).mean())),
                        (name + '/ssim', float(s[:, metrics.SSIM].mean()))]
            return (3 * n, lambda out, loss: metrics.image_metrics(pred, target, max_val, out=out.view(n, 3)),
                    lambda loss: metrics.image_metrics_host(pred.numpy(), target.numpy(), max_val).reshape(-1), result)
        def smoothness(name, flow, guide, alpha, eps, order=1):
            return (1, into(lambda loss: metrics.flow_smoothness(flow, guide, alpha, eps, order=order)),
                    lambda loss: float(metrics.flow_smoothness_host(flow.numpy(), guide.numpy() if guide is not None else None, alpha, eps,
                                                                    order=order)[0]),
                    means(name + ('/smoothness2' if order == 2 else '/smoothness')))
        def smoothness2(*term):         # a smoothness2_terms tuple: the second-order term under its own key
            return smoothness(*term, order=2)
        def host_mask(mask):
            return mask.numpy() if mask is not None else None
        def multiscale(name, flow, src, target, levels, kind, mask=None, suffix=''):     # suffix '_masked': the masked level terms as trained
            return (levels, into(lambda loss: metrics.multiscale_warp_loss(src, flow, target, levels, None, ms_kind[kind], mask=mask)[1]),
                    lambda loss: metrics.multiscale_warp_loss_host(src.numpy(), flow.numpy(), target.numpy(), levels, None, ms_kind[kind],
                                                                   mask=host_mask(mask))[2],
                    means(*['%s/photo_x%d%s' % (name, 2 << l, suffix) for l in range(levels)]))
        def census(name, pred, target, max_val, radius, eps, mask=None, suffix=''):
            return (1, into(lambda loss: metrics.census_loss(pred, target, max_val, 1.0, radius, eps, mask=mask)),
                    lambda loss: float(metrics.census_loss_host(pred.numpy(), target.numpy(), max_val, np.float64, 1.0, radius, eps,
                                                                mask=host_mask(mask))[0]),
                    means(name + '/census' + suffix))
        def consistency(name, flow, eps):
            return (2, lambda out, loss: metrics.flow_consistency(flow, eps, 1.0, stats=out),
                    lambda loss: [float(v) for v in metrics.flow_consistency_host(flow.numpy(), eps)[2:]],
                    means(name + '/consistency', name + '/consistency_valid'))
        def occlusion(name, flow, _, a1, a2, keep):
            return (3, lambda out, loss: metrics.flow_occlusion_mask(flow, a1, a2, keep, stats=out),
                    lambda loss: metrics.flow_occlusion_mask_host(flow.numpy(), a1, a2, keep)[1],
                    means(*['%s/%s' % (name, what) for what in ('visible', 'occluded', 'outside')]))
        def masked_image(name, what, pred, target, mask, max_val, radius, eps):       # the masked SSIM / census term as trained
            if what == 'census_masked':
                return census(name, pred, target, max_val, radius, eps, mask, '_masked')
            return (1, into(lambda loss: metrics.ssim_loss(pred, target, max_val, 1.0, mask=mask)),
                    lambda loss: float(metrics.ssim_loss_host(pred.numpy(), target.numpy(), max_val, np.float64, 1.0, mask=mask.numpy())[0]),
                    means(name + '/ssim_loss_masked'))
        def masked_multiscale(*term):   # a multiscale_terms tuple with the mask behind it
            return multiscale(*term, suffix='_masked')
        report = [(1, into(lambda loss: loss), float, means('loss'))] if self.graph.loss_expr is not None else []
        report += [pair(*p) for p in pairs]
        for make, attr in ((smoothness, 'smoothness_terms'), (smoothness2, 'smoothness2_terms'), (multiscale, 'multiscale_terms'), (census, 'census_terms'),
                           (consistency, 'consistency_terms'), (occlusion, 'occlusion_terms'), (masked_image, 'masked_image_terms'),
                           (masked_multiscale, 'masked_multiscale_terms')):
            report += [make(*term) for term in getattr(self, attr, [])]
        return report

    # ---- data-parallel hook
    def enable_data_parallel(self, world_size, group=None, comm=None, mode=None):
        """comm: parallel.RcclComm (the product path: RCCL through the C ABI) or parallel.TorchComm (default: torch.distributed
        on `group`; gloo in the CPU rehearsals).  mode: 'sharded' (default) or 'allreduce' -- Graph.run_backward_overlapped."""
        from .parallel import TorchComm
        g = self.graph
        g.world_size = int(world_size)
        g.dist_group = group
        g.comm = comm if comm is not None else TorchComm(group)
        if mode is not None:
            g.dp_mode = mode
        g.upload_optimizer_state()     # gradient scale 1 / world size for the SUM


def iteration_from_checkpoint_name(path):
    """train.py:99-101: resume iteration = trailing digits of the checkpoint file name."""
    return int(re.match('.*?([0-9]+)$', path).group(1))
