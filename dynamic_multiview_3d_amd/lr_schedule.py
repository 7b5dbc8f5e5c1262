"""Learning-rate schedules (tf.train.exponential_decay, piecewise_constant, cosine_decay, with an optional linear warm-up) and the
conf keys of decoupled weight decay.

learning_rate_at() IS THE AUTHORITY for the scheduled rate: TensorFlow cannot be run next to this project and the evaluation
order of its float32 graph ops is not reproducible bit for bit, so the rule is defined here -- in float64 with Python's math,
rounded ONCE to float32 -- and the device only ever stores the float32 this function returns (mv3d_opt_set_lr).
"""
import math

import numpy as np

KINDS = ('exponential', 'piecewise', 'cosine')
# conf key -> the kinds it belongs to (lr_warmup_steps goes with every kind and with none)
_KEYS = {
    'lr_schedule': None,
    'lr_warmup_steps': None,
    'lr_decay_steps': ('exponential', 'cosine'),
    'lr_decay_rate': ('exponential',),
    'lr_staircase': ('exponential',),
    'lr_boundaries': ('piecewise',),
    'lr_values': ('piecewise',),
    'lr_alpha': ('cosine',),
}
_REQUIRED = {'exponential': ('lr_decay_steps', 'lr_decay_rate'), 'piecewise': ('lr_boundaries', 'lr_values'), 'cosine': ('lr_decay_steps',)}


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _number(conf, key, lo=None, lo_open=False, hi=None):
    """conf[key] as a finite float inside the stated interval; a bool, NaN, inf or a value outside it raises ValueError."""
    v = conf[key]
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("conf[%r] must be a number, got %r" % (key, v))
    x = float(v)
    if not math.isfinite(x) or (lo is not None and (x <= lo if lo_open else x < lo)) or (hi is not None and x > hi):
        raise ValueError("conf[%r] is out of range: %r" % (key, v))
    return x


def lr_schedule_from_conf(conf):
    """The spec learning_rate_at() and Graph.enable_lr_schedule() take, or None when conf asks for neither a schedule nor a
    warm-up (the graph then records and launches exactly what it did without the keys).

      lr_schedule       None | 'exponential' | 'piecewise' | 'cosine'
      lr_decay_steps    integer > 0                           exponential, cosine (required)
      lr_decay_rate     finite, > 0                           exponential (required)
      lr_staircase      bool (default False)                  exponential
      lr_boundaries     strictly increasing integers >= 0     piecewise (required)
      lr_values         len(boundaries) + 1 finite floats > 0 piecewise (required); absolute rates, conf['learning_rate'] is ignored
      lr_alpha          in [0, 1] (default 0)                 cosine
      lr_warmup_steps   integer >= 0 (default 0)              any kind, or none

    ValueError, before any device work: an unknown kind; a key the kind requires that is missing; a key of another kind or of no
    schedule at all, and any other key that starts with 'lr_' (a typo must not train silently at a constant rate); a bool where
    a number is wanted, NaN, inf, or a value out of range.  A key whose value is None counts as absent."""
    present = {k for k, v in conf.items() if isinstance(k, str) and k.startswith('lr_') and v is not None}
    unknown = sorted(present - set(_KEYS))
    if unknown:
        raise ValueError("unknown learning-rate key(s) %s (have %s)" % (unknown, sorted(_KEYS)))
    kind = conf.get('lr_schedule')
    if kind is not None and (not isinstance(kind, str) or kind not in KINDS):
        raise ValueError("conf['lr_schedule'] must be None or one of %s, got %r" % (KINDS, kind))
    stray = sorted(k for k in present if _KEYS[k] is not None and kind not in _KEYS[k])
    if stray:
        raise ValueError("conf key(s) %s do not belong to conf['lr_schedule'] = %r" % (stray, kind))
    missing = [k for k in _REQUIRED.get(kind, ()) if k not in present]
    if missing:
        raise ValueError("conf['lr_schedule'] = %r needs %s" % (kind, missing))
    warmup = 0
    if 'lr_warmup_steps' in present:
        warmup = conf['lr_warmup_steps']
        if not _is_int(warmup) or warmup < 0:
            raise ValueError("conf['lr_warmup_steps'] must be an integer >= 0, got %r" % (warmup,))
        warmup = int(warmup)
    if kind is None and warmup == 0:
        return None
    spec = {'kind': kind, 'warmup': warmup}
    if kind != 'piecewise':
        if conf.get('learning_rate') is None:
            raise ValueError("a learning-rate schedule needs conf['learning_rate'] (the base rate)")
        spec['base'] = _number(conf, 'learning_rate', 0.0, lo_open=True)
    if kind in ('exponential', 'cosine'):
        n = conf['lr_decay_steps']
        if not _is_int(n) or n <= 0:
            raise ValueError("conf['lr_decay_steps'] must be an integer > 0, got %r" % (n,))
        spec['decay_steps'] = int(n)
    if kind == 'exponential':
        spec['rate'] = _number(conf, 'lr_decay_rate', 0.0, lo_open=True)
        stair = conf.get('lr_staircase')
        if stair is not None and not isinstance(stair, (bool, np.bool_)):
            raise ValueError("conf['lr_staircase'] must be a bool, got %r" % (stair,))
        spec['staircase'] = bool(stair)
    elif kind == 'cosine':
        spec['alpha'] = _number(conf, 'lr_alpha', 0.0, hi=1.0) if 'lr_alpha' in present else 0.0
    elif kind == 'piecewise':
        bounds, values = conf['lr_boundaries'], conf['lr_values']
        if not isinstance(bounds, (list, tuple, np.ndarray)) or not isinstance(values, (list, tuple, np.ndarray)):
            raise ValueError("conf['lr_boundaries'] and conf['lr_values'] must be lists")
        bounds = list(bounds)
        if not bounds or not all(_is_int(b) and b >= 0 for b in bounds) or any(b <= a for a, b in zip(bounds, bounds[1:])):
            raise ValueError("conf['lr_boundaries'] must be strictly increasing integers >= 0, got %r" % (conf['lr_boundaries'],))
        if len(values) != len(bounds) + 1:
            raise ValueError("conf['lr_values'] must hold len(lr_boundaries) + 1 = %d rates, got %d" % (len(bounds) + 1, len(values)))
        spec['boundaries'] = [int(b) for b in bounds]
        spec['values'] = [_number({'lr_values': v}, 'lr_values', 0.0, lo_open=True) for v in values]
    return spec


def learning_rate_at(spec, step):
    """np.float32 rate of optimiser update number `step` (0-based: the number of updates already made).  spec: what
    lr_schedule_from_conf() returns.  THE AUTHORITY for the scheduled rate (see the module docstring): evaluated in float64 with
    Python's math and rounded once to float32.

      exponential   base * rate ** (step / decay_steps)           staircase: the exponent is step // decay_steps
      piecewise     values[0] for step <= boundaries[0]; values[i] for boundaries[i-1] < step <= boundaries[i]; values[-1] beyond
      cosine        base * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)
      None          base
      warm-up W     for step < W the rate above times (step + 1) / W"""
    if isinstance(step, (bool, np.bool_)) or not isinstance(step, (int, np.integer)) or step < 0:
        raise ValueError("learning_rate_at: step must be an integer >= 0, got %r" % (step,))
    step = int(step)
    kind = spec['kind']
    if kind == 'exponential':
        n = spec['decay_steps']
        x = float(step // n) if spec['staircase'] else step / n
        lr = spec['base'] * math.pow(spec['rate'], x)
    elif kind == 'piecewise':
        i = 0
        while i < len(spec['boundaries']) and step > spec['boundaries'][i]:
            i += 1
        lr = spec['values'][i]
    elif kind == 'cosine':
        n, alpha = spec['decay_steps'], spec['alpha']
        lr = spec['base'] * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * min(step, n) / n)) + alpha)
    elif kind is None:
        lr = spec['base']
    else:
        raise ValueError("learning_rate_at: unknown kind %r" % (kind,))
    w = spec.get('warmup', 0)
    if step < w:
        lr = lr * ((step + 1) / w)
    with np.errstate(over='ignore', under='ignore'):
        out = np.float32(lr)
    if not np.isfinite(out) or out < 0:
        raise ValueError("learning_rate_at: the rate of step %d is %r: not a finite float32 >= 0" % (step, lr))
    return out


def check_weight_decay(wd, what="conf['weight_decay']"):
    """wd as a float, finite and > 0, or None for off (None or 0).  A bool, anything that is not a number (a string included), a
    negative value, NaN or inf raises ValueError.  The one check of conf['weight_decay'] and of Graph.enable_weight_decay()."""
    if wd is None:
        return None
    if isinstance(wd, (bool, np.bool_)) or not isinstance(wd, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number > 0 (or 0 / None for off), got %r" % (what, wd))
    x = float(wd)
    if not math.isfinite(x) or x < 0:
        raise ValueError("%s must be finite and > 0 (or 0 / None for off), got %r" % (what, wd))
    return x if x > 0 else None


def weight_decay_from_conf(conf):
    """conf['weight_decay'] = wd as a float, finite and > 0, or None for off (absent, None or 0: nothing is allocated, the same
    plans and launches).  After update k every decayed weight loses float32(float64(lr_k) * wd) of itself
    (Graph.enable_weight_decay).  A bool, a string, a negative value, NaN or inf raises ValueError, before any device work."""
    return check_weight_decay(conf.get('weight_decay'))
