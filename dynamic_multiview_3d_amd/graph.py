"""Static graph of the appearance-flow train step, executed by libmv3d_hip.so.

The reference builds a TensorFlow-1.3 graph once (buildModel/build_loss) and then calls
sess.run([loss, train_op]) per iteration (multi_view_model/train.py:122).  This module is the
MI355X-side counterpart: the tf_utils-named functions (tf_utils.py of this package) append nodes
to the current Graph; `finalize()` lays every activation, gradient and variable out in HBM once;
`compile()` records the forward and the hand-scheduled reverse launch sequences into native plans
(mv3d_plan_*), so a step is two native calls plus one fused Adam kernel -- no autograd, no
per-op Python in the steady state.

Data layout in HBM
  * activations: NHWC fp32, one allocation per root Storage [rows, channels]; tf.concat /
    tf.split on the channel axis and tf.reshape are views (channel offset + pixel stride `ld`).
  * gradients: one buffer per root Storage with identical layout.  The gradient buffer of a
    tensor that is an activation output holds dL/d(pre-activation): the consumer's dgrad kernel
    multiplies by act'(output) in its epilogue (slope at 0 is f1).
  * variables: ONE flat fp32 buffer (TF variable order), plus flat grad / Adam m / Adam v buffers
    of the same layout -> Adam is one kernel launch and the data-parallel all-reduce runs on
    contiguous bucket views.
PyTorch is used for device memory (torch.empty), streams and torch.distributed only.
"""
import contextlib
import ctypes as C
import os
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, loss_calls
from ._lib import ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH

_current = []

EMA_SLOT = 'ExponentialMovingAverage'           # TF's shadow-variable name: <var>/ExponentialMovingAverage
EMA_COUNTER = EMA_SLOT + '/num_updates'


# =============================================================================================== EMA host twins
def ema_one_minus_decay(decay, n=None):
    """float32(1 - decay_t), the scalar mv3d_ema_step takes: decay_t = decay, or with tf.train.ExponentialMovingAverage's
    num_updates = n (the zero-based index of the update) min(decay, (1 + n) / (10 + n)).  Evaluated in double, rounded once."""
    d = float(decay)
    if n is not None:
        d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
    return np.float32(1.0 - d)


def ema_rule(shadow, params, one_minus_decay):
    """numpy twin of mv3d_ema_step: assign_moving_average(zero_debias=False) on float32 arrays, in TF's order and with one
    rounding per operation -- d = s - p; u = d * w; s = s - u.  Returns the new shadows (the inputs are left alone)."""
    s, p = np.asarray(shadow, np.float32), np.asarray(params, np.float32)
    d = s - p
    u = d * np.float32(one_minus_decay)
    return s - u


GLOBAL_STEP = 'global_step'                     # the checkpoint's count of optimiser updates (TF's global_step variable)


def weight_decay_factor(lr, weight_decay):
    """f = float32(float64(lr) * weight_decay), the scalar mv3d_weight_decay_step takes: rounded once."""
    return np.float32(float(np.float32(lr)) * float(weight_decay))


def weight_decay_rule(params, ranges, f, shadow=None, one_minus_decay=None):
    """numpy twin of mv3d_weight_decay_step over whole flat float32 arrays: inside the [begin, end) index pairs of `ranges`
    t = p * f; p = p - t with one rounding per operation, an element whose t is 0 keeping its bits (only p = -0 tells the
    difference: its sign stays); outside them nothing.  Returns the new parameters, or with `shadow` (new parameters, new
    shadows): the EMA of every element behind the decay, ema_rule(shadow, new parameters, one_minus_decay).  The inputs are
    left alone; ranges that reach past the array are clipped."""
    p = np.array(params, np.float32)
    f = np.float32(f)
    for a, b in np.asarray(ranges, np.int64).reshape(-1, 2):
        a, b = max(int(a), 0), min(int(b), p.size)
        if b > a:
            with np.errstate(under='ignore'):
                t = p[a:b] * f
                p[a:b] = np.where(t == 0, p[a:b], p[a:b] - t)
    if shadow is None:
        return p
    return p, ema_rule(shadow, p, one_minus_decay)


# =============================================================================================== gradient-clipping host twin
GN_CHUNK = 16384                                # floats per chunk of mv3d_grad_clip_scale (csrc/grad_norm.hip): 256 threads x 16 float4


def _block_sum_rule(v):
    """block_sum / block_total of csrc/sum_common.h over the last axis (256 doubles, one per thread): the xor butterfly inside each
    wave of 64 (lane 0's value: the halves added pairwise, offsets 32 .. 1), then ((w0 + w1) + w2) + w3."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def grad_clip_rule(g, pre_scale, clip_norm):
    """numpy twin of mv3d_grad_clip_scale, in the order include/mv3d_hip.h states: (norm, scale, gscale) as float32, the device's
    out[0], out[1] and slot 6 of the optimiser records, bit for bit.  g: the flat float32 gradient buffer; pre_scale: float32(1 /
    world size); clip_norm: > 0, inf = measure only."""
    g = np.asarray(g, np.float32).reshape(-1)
    pre, clip = np.float32(pre_scale), np.float32(clip_norm)
    nchunk = -(-g.size // GN_CHUNK)
    x = np.zeros(nchunk * GN_CHUNK, np.float64)             # elements past the count are 0
    x[:g.size] = g
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        x *= x                                              # exact: 24 x 24 bits
        x = np.ascontiguousarray(x.reshape(nchunk, 16, 256, 4).transpose(1, 3, 0, 2))   # [chunk, float4 k, thread, component] -> [k, component, chunk, thread]
        acc = np.zeros((nchunk, 256), np.float64)
        for k in range(16):                                 # 64 sequential adds per thread: k = 0 .. 15, then x, y, z, w
            for c in range(4):
                acc = acc + x[k, c]
        part = _block_sum_rule(acc)                         # one double per chunk
        rounds = -(-nchunk // 256)                          # final kernel: thread t adds partials t, t + 256, ..
        p = np.zeros(rounds * 256, np.float64)
        p[:nchunk] = part
        acc = np.zeros(256, np.float64)
        for row in p.reshape(rounds, 256):
            acc = acc + row
        S = _block_sum_rule(acc)
        n = np.float32(np.sqrt(S)) * pre
        s = clip / n if n > clip else np.float32(1.0)       # NaN compares false; n = inf gives 0
        return np.float32(n), np.float32(s), np.float32(pre * s)


def grad_accum_rule(grads_list, losses=None):
    """numpy twin of mv3d_grad_accumulate over one cycle: (sum, loss mean).  sum = ((g1 + g2) + g3) .. in float32, left to right
    -- what MV3D_ACCUM_STORE, then ADD .., then FINISH leave in the gradient buffer, bit for bit (the optimiser multiplies it by
    float32(1 / (world size * N)) through its gradient-scale slot); loss mean = ((l1 + l2) + ..) * float32(1 / N), or None
    without losses."""
    gs = [np.asarray(g, np.float32) for g in grads_list]
    if not gs:
        raise ValueError("grad_accum_rule: no gradients")
    with np.errstate(over='ignore', invalid='ignore'):
        total = gs[0].copy()
        for g in gs[1:]:
            total = total + g
        if losses is None:
            return total, None
        if len(losses) != len(gs):
            raise ValueError("grad_accum_rule: %d losses for %d gradients" % (len(losses), len(gs)))
        mean = np.float32(losses[0])
        for l in losses[1:]:
            mean = np.float32(mean + np.float32(l))
        return total, np.float32(mean * np.float32(1.0 / len(gs)))


def current_graph():
    if not _current:
        raise RuntimeError("no Graph is active: build models inside `with Graph(...) as g:`")
    return _current[-1]


# =============================================================================================== storage / tensors
class Storage:
    """[rows, ch] fp32 region.  Either a root allocation, a channel slice of `parent`
    (set when tf.concat adopts it), or a reshaped alias of a dense root (`alias_of`)."""

    def __init__(self, rows, ch, alias_of=None):
        self.rows, self.ch = rows, ch
        self.parent, self.ch_off = None, 0
        self.alias_of = alias_of
        self.has_alias = False
        self.data = None
        self.grad = None
        self.needs_grad = False
        self.external = False
        if alias_of is not None:
            alias_of.has_alias = True

    def resolve(self):
        s, off = self, 0
        while s.parent is not None:
            off += s.ch_off
            s = s.parent
        return s, off

    def can_be_adopted(self):
        return self.parent is None and self.alias_of is None and not self.has_alias and not self.external


class Tensor:
    def __init__(self, graph, shape, storage=None, ch_off=0, producer=None, act=ACT_NONE, leak=0.2,
                 requires_grad=False, name=None):
        self.graph = graph
        self.shape = tuple(int(s) for s in shape)
        self.C = self.shape[-1]
        self.rows = int(np.prod(self.shape[:-1])) if len(self.shape) > 1 else 1
        self.storage = storage if storage is not None else Storage(self.rows, self.C)
        self.ch_off = ch_off
        self.producer = producer
        self.act, self.leak = act, leak          # activation these VALUES are the output of
        self.requires_grad = requires_grad
        self.name = name
        self.fused_into = None                   # set on a pre-activation tensor once lrelu()/tanh() fused it
        self.grad_consumers = 0
        # backward-emission state
        self.grad_written = False
        self.grad_masked = False
        if requires_grad:
            self.storage.needs_grad = True

    # ---- TF-like surface
    def get_shape(self):
        return list(self.shape)

    # ---- resolved addressing (valid after Graph.finalize())
    def _root(self):
        s = self.storage
        if s.alias_of is not None:
            root, off = s.alias_of.resolve()
            assert off == 0 and root.ch == s.alias_of.ch
            return root, 0, s.ch
        root, off = s.resolve()
        return root, off, root.ch

    @property
    def ld(self):
        return self._root()[2]

    @property
    def ptr(self):
        root, off, _ = self._root()
        return root.data.data_ptr() + 4 * (off + self.ch_off)

    @property
    def grad_ptr(self):
        root, off, _ = self._root()
        return root.grad.data_ptr() + 4 * (off + self.ch_off)

    def _view(self, buf):
        root, off, ld = self._root()
        v = buf.view(-1, ld)[:, off + self.ch_off: off + self.ch_off + self.C]
        return v.reshape(self.shape) if v.is_contiguous() else v.unflatten(0, self.shape[:-1])

    def value(self):
        """torch view of the activation (device)."""
        return self._view(self._root()[0].data)

    def grad_value(self):
        return self._view(self._root()[0].grad)

    def numpy(self):
        return self.value().detach().cpu().numpy().copy()

    def set(self, array):
        t = torch.as_tensor(np.ascontiguousarray(array, dtype=np.float32)) if not torch.is_tensor(array) else array
        self.value().copy_(t.reshape(self.shape), non_blocking=True)


class Variable:
    def __init__(self, name, shape, init):
        self.name, self.shape, self.init = name, tuple(shape), init
        self.size = int(np.prod(shape))
        self.offset = None
        self.graph = None
        self.has_grad = False

    @property
    def ptr(self):
        return self.graph.params.data_ptr() + 4 * self.offset

    @property
    def grad_ptr(self):
        return self.graph.grads.data_ptr() + 4 * self.offset

    def value(self):
        self.graph._settle()
        return self.graph.params[self.offset:self.offset + self.size].view(self.shape)

    def grad_value(self):
        self.graph._settle()
        return self.graph.grads[self.offset:self.offset + self.size].view(self.shape)


class ScalarExpr:
    """Weighted sum of loss terms; supports the arithmetic the reference applies to losses
    (main_model.py:144-152: `self.loss = 0.; self.loss += euclidean_loss(...) * factor`)."""

    def __init__(self, terms=()):
        self.terms = list(terms)          # [(weight, LossTerm)]

    def __add__(self, o):
        if isinstance(o, (int, float)):
            if o != 0:
                raise NotImplementedError("adding a non-zero constant to a loss")
            return ScalarExpr(self.terms)
        return ScalarExpr(self.terms + o.terms)

    __radd__ = __add__

    def __mul__(self, c):
        return ScalarExpr([(w * float(c), t) for w, t in self.terms])

    __rmul__ = __mul__


LOSS_L1, LOSS_L2, LOSS_SSIM, LOSS_SMOOTH, LOSS_MULTISCALE, LOSS_CENSUS, LOSS_CONSIST = 1, 2, 3, 4, 5, 6, 7


def _at(t):
    """(address, pixel stride) of a Tensor for loss_calls, or None for an absent operand."""
    return (t.ptr, t.ld) if t is not None else None


class LossTerm:
    """One term of the loss on the differentiated tensor a against b.  A class states its `kind` (LOSS_*), its `order` (the terms
    of a step are launched in this order: Graph._emit_losses) and `on_flow`: a term on a flow, usually an INTERMEDIATE tensor whose
    gradient also arrives from its consumer, so that its gradient launch can be deferred into the reverse plans
    (Graph._flow_term_before / _flow_term_after merge the two).  `ws` is the term's own workspace, allocated by Graph.compile()."""
    kind, order, on_flow = None, None, False

    def __init__(self, a, b, mask=None):
        self.a, self.b, self.mask, self.ws = a, b, mask, None

    def workspace_bytes(self, lib):
        """Bytes of the workspace this term needs (ValueError where the kernel does not take its operands), or None for none."""
        return None

    @staticmethod
    def _nonzero(nbytes, message):
        """The workspace size the library answers, or ValueError(message) where it answers 0."""
        if not int(nbytes):
            raise ValueError(message)
        return int(nbytes)

    def launch(self, g, w, value, grad, accumulate):
        """Record the term's library call at weight w: the value into the loss word and / or the gradient stored into (or, with
        accumulate, added onto) a's gradient buffer.  The terms with an eager twin in metrics.py call through loss_calls, which
        owns the argument layout and the choice of the masked entry."""
        raise NotImplementedError

    def _grad_at(self, grad):
        """(address, pixel stride) of a's gradient for loss_calls, or None without `grad`."""
        return (self.a.grad_ptr, self.a.ld) if grad else None

    def _ws_at(self):
        return self.ws.data_ptr(), self.ws.numel()


class PixelTerm(LossTerm):
    """kind LOSS_L1 / LOSS_L2: the pixel losses (mv3d_pixel_loss*), with an optional one-channel mask and a scale on b; no workspace."""
    order = 0

    def __init__(self, a, b, kind, mask=None, b_scale=1.0):
        LossTerm.__init__(self, a, b, mask)
        self.kind, self.b_scale = kind, float(b_scale)

    def launch(self, g, w, value, grad, accumulate):
        a, b, m = self.a, self.b, self.mask
        g.lib.pixel_loss_strided(a.rows, a.C, a.ptr, a.ld, b.ptr, b.ld, self.b_scale, m.ptr if m is not None else None,
                                 m.ld if m is not None else 1, self.kind, float(w), g.loss_buf.data_ptr(), a.grad_ptr if grad else None, a.ld, g.stream)


class SsimTerm(LossTerm):
    """1 - mean SSIM at dynamic range max_val (mv3d_ssim_loss), or with a one-channel mask its masked form
    (mv3d_ssim_loss_masked).  The workspace holds the per-tile sums (not the shared scratch: the term's two launches must find it
    untouched whatever runs beside them)."""
    kind, order = LOSS_SSIM, 1

    def __init__(self, a, b, max_val=1.0, mask=None):
        LossTerm.__init__(self, a, b, mask)
        self.max_val = float(max_val)

    def workspace_bytes(self, lib):
        return self._nonzero(loss_calls.ssim_workspace_bytes(lib, self.a.shape, self.mask is not None),
                             "ssim_loss: operands of shape %s are outside what mv3d_ssim_loss takes" % (self.a.shape,))

    def launch(self, g, w, value, grad, accumulate):
        loss_calls.ssim(g.lib, self.a.shape, _at(self.a), _at(self.b), _at(self.mask), self.max_val, w, g.loss_buf.data_ptr(),
                        self._grad_at(grad), accumulate, self._ws_at(), g.stream)


class CensusTerm(LossTerm):
    """The soft census loss over (2 radius + 1)^2 patches at dynamic range max_val with Charbonnier eps (mv3d_census_loss), or with
    a one-channel mask its masked form (mv3d_census_loss_masked; the same workspace)."""
    kind, order = LOSS_CENSUS, 2

    def __init__(self, a, b, max_val=1.0, radius=3, eps=1e-3, mask=None):
        LossTerm.__init__(self, a, b, mask)
        self.max_val, self.radius, self.eps = float(max_val), int(radius), float(eps)

    def workspace_bytes(self, lib):
        return self._nonzero(loss_calls.census_workspace_bytes(lib, self.a.shape, self.radius),
                             "census_loss: operands of shape %s at radius %d are outside what mv3d_census_loss takes" % (self.a.shape, self.radius))

    def launch(self, g, w, value, grad, accumulate):
        loss_calls.census(g.lib, self.a.shape, _at(self.a), _at(self.b), _at(self.mask), self.radius, self.max_val, self.eps, w,
                          g.loss_buf.data_ptr(), self._grad_at(grad), accumulate, self._ws_at(), g.stream)


class SmoothTerm(LossTerm):
    """The edge-aware smoothness of the flow a (mv3d_flow_smoothness) with b the guide image or None, edge parameter edge_alpha
    and Charbonnier eps; with second_order the penalty of the second differences (mv3d_flow_smoothness2), which takes the same
    operands (`order` is the launch position, hence the keyword's name).  The workspace holds 2 sums per tile."""
    kind, order, on_flow = LOSS_SMOOTH, 3, True

    def __init__(self, a, b, edge_alpha=0.0, eps=1e-3, second_order=False):
        LossTerm.__init__(self, a, b)
        self.edge_alpha, self.eps, self.second_order = float(edge_alpha), float(eps), bool(second_order)

    def workspace_bytes(self, lib):
        difference = 2 if self.second_order else 1
        return self._nonzero(loss_calls.flow_smoothness_workspace_bytes(lib, self.a.shape[:3], difference),
                             "flow_smoothness_loss: a flow of shape %s is outside what mv3d_flow_smoothness%s takes"
                             % (self.a.shape, '2' if self.second_order else ''))

    def launch(self, g, w, value, grad, accumulate):
        b = self.b
        loss_calls.flow_smoothness(g.lib, self.a.shape[:3], _at(self.a), (b.ptr, b.C, b.ld) if b is not None else None, self.edge_alpha,
                                   self.eps, w, g.loss_buf.data_ptr() if value else None, self._grad_at(grad), grad and accumulate,
                                   self._ws_at(), g.stream, 2 if self.second_order else 1)


class MultiscaleTerm(LossTerm):
    """The multi-scale photometric loss (mv3d_multiscale_warp_loss) of the flow a, which warps `src` onto the target b over `levels`
    pyramid levels with weights `level_weights` and pixel loss `pixel_kind` (LOSS_L1 / LOSS_L2); neither image is differentiated.
    The workspace holds the tile sums and both pyramids: a call without the value is the reverse-pass call, which reuses them.
    With a one-channel mask over the flow's grid both calls are the masked form's (mv3d_multiscale_warp_loss_masked; the same
    workspace: the mask is pooled inside the tile launch)."""
    kind, order, on_flow = LOSS_MULTISCALE, 4, True

    def __init__(self, a, b, src, levels, level_weights, pixel_kind=LOSS_L2, mask=None):
        LossTerm.__init__(self, a, b, mask)
        self.src, self.levels, self.level_weights, self.pixel_kind = src, int(levels), tuple(float(v) for v in level_weights), pixel_kind

    def workspace_bytes(self, lib):
        return self._nonzero(loss_calls.multiscale_workspace_bytes(lib, self.a.shape[:3], self.src.shape[1:], self.levels),
                             "multiscale_photometric_loss: a flow of shape %s over a source of shape %s at %d levels is outside "
                             "what mv3d_multiscale_warp_loss takes" % (self.a.shape, self.src.shape, self.levels))

    def launch(self, g, w, value, grad, accumulate):
        loss_calls.multiscale(g.lib, self.a.shape[:3], self.src.shape[1:], _at(self.src), _at(self.a), _at(self.b), _at(self.mask),
                              self.levels, [float(w) * v for v in self.level_weights], self.pixel_kind,
                              g.loss_buf.data_ptr() if value else None, None, self._grad_at(grad), grad and accumulate, not value,
                              self._ws_at(), g.stream)


class ConsistTerm(LossTerm):
    """The forward-backward consistency (mv3d_flow_consistency) of the flow a over a pair-swapped batch with Charbonnier eps; b is
    None.  The workspace holds the int64 scatter plane, the float plane of the gathered part and the tile sums."""
    kind, order, on_flow = LOSS_CONSIST, 5, True

    def __init__(self, a, eps=1e-3):
        LossTerm.__init__(self, a, None)
        self.eps = float(eps)

    def workspace_bytes(self, lib):
        return self._nonzero(loss_calls.flow_consistency_workspace_bytes(lib, self.a.shape[:3]),
                             "flow_consistency_loss: a flow of shape %s is outside what mv3d_flow_consistency takes" % (self.a.shape,))

    def launch(self, g, w, value, grad, accumulate):
        loss_calls.flow_consistency(g.lib, self.a.shape[:3], _at(self.a), self.eps, w, g.loss_buf.data_ptr() if value else None, None,
                                    self._grad_at(grad), grad and accumulate, self._ws_at(), g.stream)


FLOW_TERMS = tuple(c.kind for c in LossTerm.__subclasses__() if c.on_flow)      # (LOSS_SMOOTH, LOSS_MULTISCALE, LOSS_CONSIST)


# =============================================================================================== nodes
class Node:
    def forward(self, g):
        raise NotImplementedError

    def backward(self, g):
        pass


def _epi(bias=None, act=ACT_NONE, leak=0.2, mask_of=None):
    """Epilogue for a kernel; mask_of = tensor whose activation derivative multiplies the result."""
    if mask_of is not None and mask_of.act != ACT_NONE:
        return _lib.epilogue(bias, act, leak, mask_of.act, mask_of.leak, mask_of.ptr, mask_of.ld)
    return _lib.epilogue(bias, act, leak)


def _ensure_premasked(g, t):
    """Make t's gradient buffer hold dL/d(pre-activation) if t is an activation output."""
    if t.act != ACT_NONE and not t.grad_masked:
        g.lib.act_bwd(t.rows, t.C, t.grad_ptr, t.ld, t.ptr, t.ld, t.grad_ptr, t.ld, t.act, t.leak, g.stream)
        t.grad_masked = True


def _note_grad_written(x, masked):
    x.grad_written = True
    x.grad_masked = masked


class ConvNode(Node):
    """conv2d_msra (tf_utils.py:70-84) / deconv2d_msra (tf_utils.py:87-98) with the following
    lrelu/relu/tanh fused into the epilogue."""

    def __init__(self, x, y, w, b, kh, kw, sh, sw, transposed):
        self.x, self.y, self.w, self.b = x, y, w, b
        self.k = (kh, kw, sh, sw)
        self.transposed = transposed
        self.act, self.leak = ACT_NONE, 0.2

    def geom(self):
        kh, kw, sh, sw = self.k
        img, feat = (self.y, self.x) if self.transposed else (self.x, self.y)
        n, h, w, c = img.shape
        return _lib.conv_geom(n, h, w, c, feat.shape[3], kh, kw, sh, sw, img.ld, feat.ld)

    def workspace_bytes(self, g):
        return g.lib.conv_workspace_bytes(C.byref(self.geom()))

    def wgrad_partial_bytes(self, g):
        return int(g.lib.conv_wgrad_workspace_bytes(C.byref(self.geom())))

    def forward(self, g):
        geom = self.geom()
        epi = _epi(self.b.ptr if self.b is not None else None, self.act, self.leak)
        fn = g.lib.deconv2d_fwd if self.transposed else g.lib.conv2d_fwd
        fn(C.byref(geom), self.x.ptr, self.w.ptr, self.y.ptr, C.byref(epi), g.ws_ptr, g.ws_bytes, g.stream)

    def backward(self, g):
        y, x = self.y, self.x
        if not y.grad_written:
            return
        _ensure_premasked(g, y)
        geom = self.geom()
        # filter / bias gradients are side work (only Adam reads them): own scratch, may run on the side stream
        ws_side = g.begin_side()
        ws_len = g.ws_bytes
        if g._finalizing:
            # mv3d_grad_finalize_*: the per-slab partial sums stay in THIS layer's region of the arena until the one batched
            # reduction (+ optimiser) at the end of the pass has read them
            ws_side, ws_len = g._part_arena.data_ptr() + self._part_off, self._part_bytes
        if self.transposed:
            g.lib.deconv2d_wgrad(C.byref(geom), x.ptr, y.grad_ptr, self.w.grad_ptr, ws_side, ws_len, g.stream)
        else:
            g.lib.conv2d_wgrad(C.byref(geom), x.ptr, y.grad_ptr, self.w.grad_ptr,
                               self.b.grad_ptr if self.b is not None else None, ws_side, ws_len, g.stream)
        g.end_side()
        self.w.has_grad = True
        if self.b is not None:
            self.b.has_grad = True
        if x.requires_grad:
            epi = _epi(mask_of=x)
            fn = g.lib.deconv2d_dgrad if self.transposed else g.lib.conv2d_dgrad
            fn(C.byref(geom), y.grad_ptr, self.w.ptr, x.grad_ptr, C.byref(epi), g.ws_ptr, g.ws_bytes, g.stream)
            _note_grad_written(x, x.act != ACT_NONE)


class LinearNode(Node):
    """linear_msra (tf_utils.py:54-67)."""

    def __init__(self, x, y, m, b):
        self.x, self.y, self.m, self.b = x, y, m, b
        self.act, self.leak = ACT_NONE, 0.2

    def workspace_bytes(self, g):
        return g.lib.fc_workspace_bytes(self.x.shape[0], self.x.C, self.y.C)

    chain = None        # Graph._find_fc_chains: the list of small layers this one is part of (one launch for all of them)

    def forward(self, g):
        x, y = self.x, self.y
        if self.chain is not None:
            # a chain of small layers (the angle MLP a0 -> a1 -> a2): ONE launch, recorded at the position of the LAST layer (the
            # first launch that touches its output: the fc hazard of the pipelined optimiser looks at that position)
            if self is not self.chain[-1]:
                return
            c = _lib.FcChain()
            first = self.chain[0]
            c.B, c.nlayers, c.in_, c.x_ld, c.x = first.x.shape[0], len(self.chain), first.x.C, first.x.ld, first.x.ptr
            for k, n in enumerate(self.chain):
                c.l[k].M, c.l[k].bias, c.l[k].y, c.l[k].y_ld, c.l[k].out = n.m.ptr, n.b.ptr, n.y.ptr, n.y.ld, n.y.C
                c.l[k].act, c.l[k].leak = n.act, n.leak
            g.lib.fc_chain_fwd(C.byref(c), g.stream)
            return
        epi = _epi(self.b.ptr, self.act, self.leak)
        g.lib.fc_fwd(x.shape[0], x.C, y.C, x.ptr, x.ld, self.m.ptr, y.ptr, y.ld, C.byref(epi), g.ws_ptr, g.ws_bytes, g.stream)

    def backward(self, g):
        x, y = self.x, self.y
        if not y.grad_written:
            return
        _ensure_premasked(g, y)
        B, fin, fout = x.shape[0], x.C, y.C
        # the fused kernel reads x and dy with 16-byte loads: a channel slice at an odd offset takes fc_wgrad + adam_step_dev
        if g._fusing and g.lib.fc_wgrad_adam_supported(B, fin, fout, x.ld, y.ld) and x.ptr % 16 == 0 and y.grad_ptr % 16 == 0:
            # Single-GPU step: the matrix gradient never goes to HBM -- ApplyAdam runs in the epilogue of the filter-gradient
            # kernel (mv3d_fc_wgrad_adam), recorded by record_fused_update() at the end of the reverse pass.
            if x.requires_grad:
                epi = _epi(mask_of=x)
                g.lib.fc_dgrad(B, fin, fout, y.grad_ptr, y.ld, self.m.ptr, x.grad_ptr, x.ld, C.byref(epi), g.ws_ptr, g.ws_bytes, g.stream)
                _note_grad_written(x, x.act != ACT_NONE)
            g._fused_vars.append(self.m)
            g._fused_nodes.append(self)
            self.m.has_grad = self.b.has_grad = True
            return
        # The angle MLP (a0 -> a1 -> a2, appearance_flow_model.py:101-103): nothing on the main stream reads the input gradient of a
        # small fc layer whose input comes from another small fc layer, so its data gradient rides the filter-gradient stream too
        # (two 5 us launches off the dependent chain of the reverse pass)
        side_dgrad = (x.requires_grad and fin <= 128 and fout <= 128 and x.grad_consumers <= 1 and
                      any(isinstance(n, LinearNode) and n.y.storage is x.storage and n.y.ch_off == x.ch_off and n.x.C <= 128
                          for n in g.nodes))
        ws_side = g.begin_side()
        if side_dgrad:
            epi = _epi(mask_of=x)       # both gradients read dy: one launch (mv3d_fc_wgrad_dgrad)
            g.lib.fc_wgrad_dgrad(B, fin, fout, x.ptr, x.ld, y.grad_ptr, y.ld, self.m.ptr, self.m.grad_ptr, self.b.grad_ptr,
                                 x.grad_ptr, x.ld, C.byref(epi), ws_side, g.ws_bytes, g.stream)
            _note_grad_written(x, x.act != ACT_NONE)
        else:
            g.lib.fc_wgrad(B, fin, fout, x.ptr, x.ld, y.grad_ptr, y.ld, self.m.grad_ptr, self.b.grad_ptr,
                           ws_side, g.ws_bytes, g.stream)
        g.end_side()
        self.m.has_grad = self.b.has_grad = True
        if x.requires_grad and not side_dgrad:
            epi = _epi(mask_of=x)
            g.lib.fc_dgrad(B, fin, fout, y.grad_ptr, y.ld, self.m.ptr, x.grad_ptr, x.ld, C.byref(epi),
                           g.ws_ptr, g.ws_bytes, g.stream)
            _note_grad_written(x, x.act != ACT_NONE)

    def record_fused_update(self, g):
        """The fused filter gradient + optimiser of a matrix whose backward() left it out.  Graph.compile records it at the
        end of the reverse pass, behind the layer's data gradient (the last reader of the old weights).  It streams 400 MB:
        next to the other fc layers' weight streams and the latency-bound 8x8 / 4x4 convolutions it only fights for HBM,
        next to the MFMA-bound tail of the filter-gradient chain it is free (measured at B = 64: right behind the layer
        26.56k, 6 nodes behind 26.65k, end of the pass 26.83k images/s)."""
        x, y = self.x, self.y
        B, fin, fout = x.shape[0], x.C, y.C
        g.begin_side(cls=2)         # its own stream: it must not hold up the conv filter gradients
        off = 4 * self.m.offset
        if g.optimizer == 'adam':
            g.lib.fc_wgrad_adam(B, fin, fout, x.ptr, x.ld, y.grad_ptr, y.ld, self.m.ptr, g.adam_m.data_ptr() + off,
                                g.adam_v.data_ptr() + off, self.b.grad_ptr, g.opt_state.data_ptr() + 32, g.stream)
        else:                       # Momentum (slot) or GD (none): mv3d_fc_wgrad_sgd
            g.lib.fc_wgrad_sgd(B, fin, fout, x.ptr, x.ld, y.grad_ptr, y.ld, self.m.ptr,
                               g.accum.data_ptr() + off if g.accum is not None else None, self.b.grad_ptr,
                               g.opt_state.data_ptr() + 32, g.stream)
        g.end_side()


class ActNode(Node):
    """Stand-alone activation (only when it could not be fused into its producer)."""

    def __init__(self, x, y, act, leak):
        self.x, self.y, self.act, self.leak = x, y, act, leak

    def forward(self, g):
        x, y = self.x, self.y
        g.lib.act_fwd(x.rows, x.C, x.ptr, x.ld, y.ptr, y.ld, self.act, self.leak, g.stream)

    def backward(self, g):
        x, y = self.x, self.y
        if not y.grad_written or not x.requires_grad:
            return
        _ensure_premasked(g, y)          # y.grad now holds dL/dx
        g.lib.copy2d(x.rows, x.C, y.grad_ptr, y.ld, 1, x.grad_ptr, x.ld, 0, g.stream)
        _note_grad_written(x, False)


class ViewNode(Node):
    """tf.reshape / tf.split / zero-copy tf.concat: no kernels; only gradient bookkeeping."""

    def __init__(self, ins, outs):
        self.ins, self.outs = ins, outs

    def forward(self, g):
        pass

    def backward(self, g):
        written = [o for o in self.outs if o.grad_written]
        if not written:
            return
        if len(written) != len(self.outs):
            # a slice nobody differentiated through: its gradient is zero
            for o in self.outs:
                if not o.grad_written and o.requires_grad:
                    g.lib.copy2d(o.rows, o.C, g.zero_ptr, 0, max(o.rows, 1) * 4, o.grad_ptr, o.ld, 0, g.stream)
                    _note_grad_written(o, o.act != ACT_NONE)
        masked = [o.grad_masked for o in self.outs if o.requires_grad]
        want_mask = any(masked)
        if want_mask and not all(masked):
            for o in self.outs:
                if o.requires_grad:
                    _ensure_premasked(g, o)
        for i in self.ins:
            if i.requires_grad:
                if want_mask and i.act == ACT_NONE:
                    raise RuntimeError("view of mixed activation / linear tensors cannot carry a masked gradient")
                _note_grad_written(i, want_mask)


class CopyConcatNode(Node):
    """tf.concat fallback when an input cannot be adopted as a slice (copies)."""

    def __init__(self, ins, out):
        self.ins, self.out = ins, out

    def forward(self, g):
        off = 0
        for t in self.ins:
            g.lib.copy2d(t.rows, t.C, t.ptr, t.ld, 1, self.out.ptr + 4 * off, self.out.ld, 0, g.stream)
            off += t.C

    def backward(self, g):
        o = self.out
        if not o.grad_written:
            return
        off = 0
        for t in self.ins:
            if t.requires_grad:
                g.lib.copy2d(t.rows, t.C, o.grad_ptr + 4 * off, o.ld, 1, t.grad_ptr, t.ld, 0, g.stream)
                _note_grad_written(t, o.grad_masked and t.act != ACT_NONE)
                if o.grad_masked and t.act == ACT_NONE:
                    raise RuntimeError("masked gradient reached a linear tensor through concat")
            off += t.C


class TileNode(Node):
    """tf.tile of a [B,1,1,C] code over [B,h,w,C] (multiobject_appflow.py:148-149)."""

    def __init__(self, x, y, reps):
        self.x, self.y, self.reps = x, y, reps

    def forward(self, g):
        x, y = self.x, self.y
        g.lib.copy2d(y.rows, y.C, x.ptr, x.ld, self.reps, y.ptr, y.ld, 0, g.stream)

    def backward(self, g):
        x, y = self.x, self.y
        if not y.grad_written or not x.requires_grad:
            return
        g.lib.group_sum(x.rows, self.reps, x.C, y.grad_ptr, y.ld, x.grad_ptr, x.ld, g.stream)
        _note_grad_written(x, y.grad_masked)


class ResampleNode(Node):
    """warp_pts_layer + resample_layer (tf_utils.py:35-42) fused: flow -> (warp_pts, gen).  When the source image needs a
    gradient, the reverse pass scatters it with mv3d_resampler_bwd against the warp the forward pass materialised."""

    def __init__(self, src, flow, warp, gen):
        self.src, self.flow, self.warp, self.gen = src, flow, warp, gen
        self.fused_loss = None      # (weight, LossTerm) when gen feeds exactly one plain pixel loss (Graph._fuse_resample_losses)
        self.fused_occlusion = None     # the OcclusionMaskNode whose mask that loss carries: the occlusion-aware head in one launch
        self.occlusion_ws = None        # ... and its workspace (the per-tile sums)

    def workspace_bytes(self, g):
        if not self.src.requires_grad:
            return 0
        n, h, w, _ = self.flow.shape
        _, hs, ws, c = self.src.shape
        return g.lib.resampler_bwd_workspace_bytes(n, h * w, hs, ws, c)

    def forward(self, g):
        n, h, w, _ = self.flow.shape
        _, hs, ws, c = self.src.shape
        if self.fused_loss is not None:
            # sampler + loss + sampler gradient in one pass: the loss gradient d(gen) never goes to HBM
            wgt, term = self.fused_loss
            want_grad = self.flow.requires_grad
            if self.fused_occlusion is not None:
                # ... and the occlusion mask of that loss is made on the way (mv3d_warp_resample_occlusion_loss)
                o = self.fused_occlusion
                g.lib.warp_resample_occlusion_loss(n, h, w, hs, ws, c, self.src.ptr, self.flow.ptr, self.flow.ld, term.b.ptr, term.b.ld,
                                                   term.kind, float(wgt), o.alpha1, o.alpha2, 1 if o.outside_visible else 0,
                                                   self.warp.ptr, self.gen.ptr, self.flow.grad_ptr if want_grad else None, self.flow.ld,
                                                   o.mask.ptr, o.mask.ld, g.loss_buf.data_ptr(), None, self.occlusion_ws.data_ptr(),
                                                   self.occlusion_ws.numel(), g.stream)
                if want_grad:
                    _note_grad_written(self.flow, False)
                return
            g.lib.warp_resample_loss(n, h, w, hs, ws, c, self.src.ptr, self.flow.ptr, self.flow.ld, term.b.ptr, term.b.ld,
                                     term.kind, float(wgt), self.warp.ptr, self.gen.ptr,
                                     self.flow.grad_ptr if want_grad else None, self.flow.ld, g.loss_buf.data_ptr(), g.stream)
            if want_grad:
                _note_grad_written(self.flow, False)
            return
        g.lib.warp_resample_fwd(n, h, w, hs, ws, c, self.src.ptr, self.flow.ptr, self.flow.ld,
                                self.warp.ptr, self.gen.ptr, g.stream)

    def backward(self, g):
        if self.fused_loss is not None or not self.gen.grad_written:
            return
        n, h, w, _ = self.flow.shape
        _, hs, ws, c = self.src.shape
        if self.flow.requires_grad:
            g.lib.warp_resample_bwd(n, h, w, hs, ws, c, self.src.ptr, self.flow.ptr, self.flow.ld,
                                    self.gen.grad_ptr, self.flow.grad_ptr, self.flow.ld, g.stream)
            _note_grad_written(self.flow, False)
        if self.src.requires_grad:
            g.lib.resampler_bwd(n, h * w, hs, ws, c, self.src.ptr, self.src.ld, self.warp.ptr, 2, self.gen.grad_ptr, self.gen.ld,
                                None, 0, self.src.grad_ptr, self.src.ld, g.ws_ptr, g.ws_bytes, g.stream)
            _note_grad_written(self.src, False)


class OcclusionMaskNode(Node):
    """tf_utils.occlusion_mask: flow [N,H,W,2] of a pair-swapped batch -> the one-channel occlusion mask [N,H,W,1]
    (mv3d_flow_occlusion_mask; metrics.flow_occlusion_mask_host states the definition).  The mask is a constant of the step: it has
    no gradient.  `fused_into` is the ResampleNode whose fused launch (mv3d_warp_resample_occlusion_loss) writes the mask instead
    of this node's own launch (Graph._fuse_resample_losses)."""

    def __init__(self, flow, mask, alpha1, alpha2, outside_visible):
        self.flow, self.mask = flow, mask
        self.alpha1, self.alpha2, self.outside_visible = float(alpha1), float(alpha2), bool(outside_visible)
        self.fused_into = None

    def forward(self, g):
        if self.fused_into is not None:
            return
        n, h, w, _ = self.flow.shape
        g.lib.flow_occlusion_mask(n, h, w, self.flow.ptr, self.flow.ld, self.alpha1, self.alpha2, 1 if self.outside_visible else 0,
                                  self.mask.ptr, self.mask.ld, None, None, 0, g.stream)


class ResamplerNode(Node):
    """resample_layer / tf.contrib.resampler.resampler(src, warp) with any warp tensor [N, ..., 2] (tf_utils.py:40-42):
    out [N, ..., C]; gradients w.r.t. the warp and / or the source (mv3d_resampler_*)."""

    def __init__(self, src, warp, out):
        self.src, self.warp, self.out = src, warp, out

    def _dims(self):
        n, hs, ws, c = self.src.shape
        return n, self.warp.rows // n, hs, ws, c

    def workspace_bytes(self, g):
        return g.lib.resampler_bwd_workspace_bytes(*self._dims()) if self.src.requires_grad else 0

    def forward(self, g):
        src, warp, out = self.src, self.warp, self.out
        g.lib.resampler_fwd(*self._dims(), src.ptr, src.ld, warp.ptr, warp.ld, out.ptr, out.ld, g.stream)

    def backward(self, g):
        src, warp, out = self.src, self.warp, self.out
        if not out.grad_written or not (warp.requires_grad or src.requires_grad):
            return
        g.lib.resampler_bwd(*self._dims(), src.ptr, src.ld, warp.ptr, warp.ld, out.grad_ptr, out.ld,
                            warp.grad_ptr if warp.requires_grad else None, warp.ld,
                            src.grad_ptr if src.requires_grad else None, src.ld, g.ws_ptr, g.ws_bytes, g.stream)
        for t in (warp, src):
            if t.requires_grad:
                _note_grad_written(t, False)


# =============================================================================================== graph
class Graph:
    """Build with the tf_utils functions inside `with Graph(...)`, then finalize() + compile()."""

    ALIGN = 64          # variables start on 256-byte boundaries of the flat buffer

    def __init__(self, device=None, seed=1234):
        self.device = torch.device(device if device is not None else 'cuda')
        self.rng = np.random.default_rng(seed)
        self.nodes = []
        self.tensors = []
        self.inputs = OrderedDict()
        self.variables = OrderedDict()
        self._scope = []
        self.loss_expr = None
        self.lr = None
        self.finalized = False
        self.lib = None
        self.stream = None
        self.ws = None
        self.ws_ptr, self.ws_bytes = None, 0
        self.n_side = max(0, min(4, int(os.environ.get('MV3D_SIDE_STREAMS', '2'))))      # 0: single-stream reverse pass; class 1 conv filter gradients, class 2 fused fc optimiser
        self.ws_side = []
        self.side_streams = None
        self.adam_stream = None
        self.adam_timing = None         # list of (start, end) events per optimiser launch when a bench wants them
        self.overlap_adam = os.environ.get('MV3D_OVERLAP_ADAM', '1') != '0'
        self.fuse_fc_adam = os.environ.get('MV3D_FUSE_FC_ADAM', '1') != '0'      # single-GPU step: Adam of the fc matrices inside their filter-gradient kernels
        self._fusing = False
        # single-GPU step: the slab reductions of all conv filter gradients and the optimiser of everything that is not a fused fc
        # matrix in ONE launch at the end of the reverse pass (mv3d_grad_finalize_*) instead of one reduction per layer + Adam
        self.fuse_finalize = os.environ.get('MV3D_FUSE_FINALIZE', '1') != '0'
        self.finalize_chunk_bytes = int(float(os.environ.get('MV3D_FINALIZE_CHUNK_MB', '48')) * 1e6)
        self._finalizing = False
        self._finalized_in_plan = False
        self._part_arena = self._fin_table = None
        self._fused_vars = []
        # The fused fc optimiser (4 x 400 MB of HBM streaming) is not joined at the end of the step: it keeps running on its side
        # stream under the NEXT step's encoder, and the forward pass waits for it in front of the first launch that touches an fc
        # matrix or an fc layer's saved input (Graph._fwd_wait_idx).  Every other reader of the weights settles first (_settle()).
        self.pipeline_fc = os.environ.get('MV3D_PIPELINE_FCADAM', '1') != '0'
        # data parallel, sharded optimiser: all-gathers of buckets first read at forward launch >= pipeline_dp_min_idx are deferred
        self.pipeline_dp = os.environ.get('MV3D_PIPELINE_DP', '1') != '0'
        self.pipeline_dp_min_idx = 8
        self._fused_nodes = []
        self._fwd_wait_idx = 0
        self._fc_event = None
        self._fc_pending = False
        self._pending_idx = 0           # forward launch index the pending event is waited for in front of
        self.plan_bwd_fused = None
        self.opt_state = None
        self.plan_fwd = self.plan_bwd = None
        self._flow_terms_deferred = []      # [(weight, LossTerm)]: terms on a flow whose gradient launch goes into the reverse plans
        # the update rule (model_base: AdamOptimizer, MomentumOptimizer, GradientDescentOptimizer); slots and state follow it
        self.optimizer = 'adam'
        self.momentum, self.use_nesterov = 0.0, False
        self.adam_m = self.adam_v = self.accum = None
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8
        self.beta1_power = np.float32(self.beta1)
        self.beta2_power = np.float32(self.beta2)
        self.world_size, self.dist_group = 1, None
        self.comm = None                # parallel.TorchComm / parallel.RcclComm once data parallel is enabled
        self.dp_mode = 'sharded'        # 'sharded': reduce-scatter -> Adam on 1/world of every bucket -> all-gather; 'allreduce': SUM + redundant Adam
        self.comm_stream = None
        self.bucket_elems = 16 * 1024 * 1024        # 64 MB of fp32 gradients per all-reduce bucket
        # tf.train.ExponentialMovingAverage of every variable (enable_ema): one flat shadow buffer with the layout of params,
        # updated by mv3d_ema_step behind each optimiser launch of a train step, on that launch's stream
        self.ema = None
        self.ema_decay, self.ema_num_updates, self.ema_updates = None, False, 0
        self._ema_event = None          # recorded behind an EMA launch the step leaves running on a side stream
        self._ema_pending = False
        self._ema_swapped = False       # inside ema_weights(): params holds the shadows and ema the weights
        self._fc_ranges = []            # flat ranges the fused fc optimiser's stream updates (run_backward_fused)
        # global-norm gradient clipping (enable_grad_clip): mv3d_grad_clip_scale over the flat gradient buffer writes the gradient
        # scale of both optimiser records just before the optimiser runs; inf = measure the norm only
        self.clip_norm = None
        self.clip_buf = None            # device [norm, scale] of the last step
        self._clip_ws, self._clip_ws_bytes = None, 0
        # gradient accumulation (enable_grad_accum): accum_steps micro-batches per optimiser update, their gradients summed by
        # mv3d_grad_accumulate into grad_sum (a second flat buffer) and, by the last micro-step, back into grads
        self.accum_steps = 0            # N >= 2, or 0 = off
        self.grad_sum = None
        self.micro_step = 0             # position in the cycle, 0 .. N - 1
        self._accum_loss = None         # two floats: the running loss sum of the current cycle and the mean of the last completed one
        self._accum_slot, self._accum_done = 0, 1
        # the count of optimiser updates made so far; update number k uses learning_rate_at(lr_spec, k).  A schedule
        # (enable_lr_schedule) writes the next update's rate into the optimiser records behind each update; decoupled weight decay
        # (enable_weight_decay) runs where the EMA launches run, over one device table of the decayed variables' flat ranges
        self.global_step = 0
        self.global_step_restored = False       # the last load_state_dict() found the counter in the checkpoint
        self.lr_spec = None
        self.weight_decay = None
        self._decay_ranges = []         # [(begin, end)]: sorted, disjoint, multiples of 4
        self._decay_table = None        # the same as int64 pairs on the device

    OPTIMIZERS = ('adam', 'momentum', 'sgd')

    @property
    def adam_state(self):
        """The device optimiser state under its original name (an Adam graph's MV3D_ADAM_* records)."""
        return self.opt_state

    def __enter__(self):
        _current.append(self)
        return self

    def __exit__(self, *a):
        _current.pop()

    # ---------------------------------------------------------------- construction helpers
    def scope_name(self, name):
        return '/'.join(self._scope + [name])

    def variable(self, name, shape, init):
        full = self.scope_name(name)
        if full in self.variables:
            raise ValueError("variable %s already exists" % full)
        v = Variable(full, shape, init)
        v.graph = self
        self.variables[full] = v
        return v

    def placeholder(self, shape, name):
        t = Tensor(self, shape, name=name)
        t.storage.external = True
        self.inputs[name] = t
        self.tensors.append(t)
        return t

    def new_tensor(self, shape, **kw):
        t = Tensor(self, shape, **kw)
        self.tensors.append(t)
        return t

    def add(self, node):
        self.nodes.append(node)
        return node

    # ---------------------------------------------------------------- memory layout
    def finalize(self):
        if self.finalized:
            return
        self.lib = _lib.lib()
        dev = self.device
        roots = []
        for t in self.tensors:
            s = t.storage
            base = s.alias_of if s.alias_of is not None else s
            root, _ = base.resolve()
            if s.needs_grad:
                root.needs_grad = True
            if root not in roots:
                roots.append(root)
        act_bytes = 0
        for r in roots:
            r.data = torch.zeros(r.rows * r.ch, dtype=torch.float32, device=dev)
            act_bytes += r.rows * r.ch * 4
            if r.needs_grad:
                r.grad = torch.zeros(r.rows * r.ch, dtype=torch.float32, device=dev)
                act_bytes += r.rows * r.ch * 4
        self.activation_bytes = act_bytes
        # variables: flat buffer in creation order (= TF trainable_variables order)
        off = 0
        for v in self.variables.values():
            v.offset = off
            off += -(-v.size // self.ALIGN) * self.ALIGN
        self.flat_size = off
        host = np.zeros(off, dtype=np.float32)
        for v in self.variables.values():
            host[v.offset:v.offset + v.size] = v.init(self.rng, v.shape).reshape(-1)
        self.params = torch.from_numpy(host).to(dev)
        self.grads = torch.zeros(off, dtype=torch.float32, device=dev)
        if self.ema_decay is not None:      # the shadows start as a copy of the variables, as TF initialises them
            self.ema = self.params.clone()
        if self.clip_norm is not None:
            self._alloc_grad_clip()
        if self.accum_steps:
            self._alloc_grad_accum()
        # optimiser slots: Adam m and v, one momentum accumulator, or none (gradient descent)
        if self.optimizer not in self.OPTIMIZERS:
            raise ValueError("unknown optimizer %r (have %s)" % (self.optimizer, ', '.join(self.OPTIMIZERS)))
        if self.optimizer == 'adam':
            self.adam_m = torch.zeros(off, dtype=torch.float32, device=dev)
            self.adam_v = torch.zeros(off, dtype=torch.float32, device=dev)
        elif self.optimizer == 'momentum':
            self.accum = torch.zeros(off, dtype=torch.float32, device=dev)
        # two records (include/mv3d_hip.h MV3D_ADAM_* / MV3D_SGD_*): [0:8] main stream, [8:16] the fused fc optimiser's stream
        self.opt_state = torch.zeros(16, dtype=torch.float32, device=dev)
        self.loss_buf = torch.zeros(4, dtype=torch.float32, device=dev)
        self.zero_buf = torch.zeros(1024, dtype=torch.float32, device=dev)
        self.zero_ptr = self.zero_buf.data_ptr()
        self.finalized = True       # pointers are valid from here on (workspace queries need them)
        # (Measured and dropped, round 2 and again round 3: spreading the LAST filter gradients of the pass -- the first layers' --
        # over all 256 CUs, or issuing them on the main stream once the data-gradient chain has ended: +-0.3 % on the step.)
        need = 0
        for n in self.nodes:
            if hasattr(n, 'workspace_bytes'):
                need = max(need, int(n.workspace_bytes(self)))
        self.ws_bytes = need
        self.ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=dev)
        self.ws_ptr = self.ws.data_ptr()
        # one scratch buffer per side-work class (classes may run concurrently)
        self.ws_side = [torch.empty(max(need // 4, 4), dtype=torch.float32, device=dev) for _ in range(self.n_side)]

    # ---------------------------------------------------------------- plans
    def _fuse_resample_losses(self):
        """A resampler output that is consumed by exactly one unmasked, unscaled pixel loss and by no other node (the
        appearance-flow head, appearance_flow_model.py:127-130 + build_loss) is computed together with that loss and
        the flow gradient by mv3d_warp_resample_loss.  A loss whose mask is the occlusion mask of the resampler's own flow
        (OcclusionMaskNode) fuses too, into mv3d_warp_resample_occlusion_loss, which writes the mask in place of the node's own
        launch.  MV3D_FUSE_RESAMPLE=0 keeps the separate launches."""
        self.fused_terms = set()
        enabled = os.environ.get('MV3D_FUSE_RESAMPLE', '1') != '0'
        for n in self.nodes:
            if isinstance(n, OcclusionMaskNode):
                n.fused_into = None
        for n in self.nodes:
            if not isinstance(n, ResampleNode):
                continue
            n.fused_loss = None
            n.fused_occlusion = None
            if not enabled or self.loss_expr is None or n.src.requires_grad:
                continue            # the sampled image's gradient has to exist when the source needs one
            gen = n.gen
            # (a smoothness term sits on the flow, not on gen: it leaves the head fused and adds to the flow gradient behind it)
            uses = [(w, t) for w, t in self.loss_expr.terms if t.a is gen or t.b is gen or t.mask is gen]
            if len(uses) != 1:
                continue
            w, t = uses[0]
            if not isinstance(t, PixelTerm):
                continue            # the SSIM and census losses need gen and write their gradient in HBM: they never fuse
            # (A masked SSIM or census term beside the masked pixel loss is a second use of gen: the head stays unfused, so the
            # mask node's own occl_mask launch sits in the forward plan in front of every loss launch that reads the mask.)
            if t.a is not gen or t.b_scale != 1.0 or t.b.requires_grad or t.b.rows != gen.rows or t.b.C != gen.C:
                continue
            occl = None
            if t.mask is not None:
                # A masked loss fuses only when the mask is the occlusion mask of the resampler's own flow: the fused launch then
                # makes it (mv3d_warp_resample_occlusion_loss).  The mask node has to come behind the resampler, so that nothing in
                # front of the fused launch can have read the mask.  (A masked multi-scale term is a second reader of the mask: it
                # sits on the flow, not on gen, and its launches go with the losses behind every node's, so the head stays fused.)
                occl = t.mask.producer
                if not (isinstance(occl, OcclusionMaskNode) and occl.mask is t.mask and occl.flow is n.flow and occl.fused_into is None
                        and self.nodes.index(occl) > self.nodes.index(n)):
                    continue
                bn, bh, bw, _ = n.flow.shape
                if tuple(n.src.shape[:3]) != (bn, bh, bw) or bh != bw or bn % 2 or bn < 2:
                    continue
            if gen.C > 4 or gen.ld != gen.C or gen.storage.has_alias or gen.storage.alias_of is not None:
                continue
            read_elsewhere = False
            for m in self.nodes:
                if m is n:
                    continue
                for v in vars(m).values():
                    vs = v if isinstance(v, (list, tuple)) else (v,)
                    if any(x is gen for x in vs):
                        read_elsewhere = True
            if read_elsewhere:
                continue
            if occl is not None:
                nbytes = int(self.lib.warp_resample_occlusion_loss_workspace_bytes(*n.flow.shape[:3]))
                if not nbytes:
                    continue
                if n.occlusion_ws is None or n.occlusion_ws.numel() != nbytes:
                    n.occlusion_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                n.fused_occlusion = occl
                occl.fused_into = n
            n.fused_loss = (w, t)
            self.fused_terms.add(id(t))

    def _find_fc_chains(self):
        """Chains of small linear layers (every width <= 64) whose intermediate outputs nobody else reads: one forward launch each
        (mv3d_fc_chain_fwd).  MV3D_FC_CHAINS=0 keeps one launch per layer."""
        for n in self.nodes:
            if isinstance(n, LinearNode):
                n.chain = None
        cur = self.lib.set_diagnostics(0)          # the live mask (mv3d_set_diagnostics returns the previous one)
        self.lib.set_diagnostics(cur)
        if os.environ.get('MV3D_FC_CHAINS', '1') == '0' or (cur & 4):       # bit 4: no small-fc kernels
            return
        def tensors_of(node):
            for val in vars(node).values():
                for t in (val if isinstance(val, (list, tuple)) else (val,)):
                    if isinstance(t, Tensor):
                        yield t
        users = {}          # root storage -> nodes that touch it
        for n in self.nodes:
            for t in tensors_of(n):
                users.setdefault(id(t._root()[0]), set()).add(id(n))
        small = lambda n: isinstance(n, LinearNode) and n.x.C <= 64 and n.y.C <= 64 and n.b is not None
        nxt = {}
        for n in self.nodes:
            if not small(n):
                continue
            root = id(n.y._root()[0])
            if len(users.get(root, ())) != 2:
                continue
            for m in self.nodes:
                if m is not n and small(m) and id(m.x._root()[0]) == root and m.x.ptr == n.y.ptr and m.x.C == n.y.C and m.x.ld == n.y.ld:
                    nxt[id(n)] = m
        heads = [n for n in self.nodes if id(n) in nxt and not any(v is n for v in nxt.values())]
        for h in heads:
            chain = [h]
            while id(chain[-1]) in nxt and len(chain) < 4:
                chain.append(nxt[id(chain[-1])])
            if len(chain) >= 2:
                for n in chain:
                    n.chain = chain

    def _emit_losses(self, with_grad):
        if self.loss_expr is None:
            return
        # A pixel loss stores its gradient, the SSIM and census losses can add to one: the terms go in their classes' `order`, and an
        # SSIM or census term accumulates when an earlier term of this step has written the gradient of the same tensor (L2 + SSIM +
        # census on one prediction).  A term on a flow sits on an intermediate tensor.  Where the forward plan has already stored that
        # tensor's gradient (the fused head, mv3d_warp_resample_loss), one launch gives the value and adds the gradient.  Otherwise
        # only the value is recorded here and the gradient launch is deferred to the reverse plan (_flow_term_before / _after).
        written = set()             # gradient addresses written by the terms so far
        self._flow_terms_deferred = []
        for w, term in sorted(self.loss_expr.terms, key=lambda wt: wt[1].order):       # stable: the terms of a kind keep their order
            if id(term) in self.fused_terms:
                continue
            a, b = term.a, term.b
            if term.on_flow:
                both = with_grad and a.requires_grad and a.grad_written
                self._flow_term_launch(w, term, value=True, grad=both, accumulate=both)
                if with_grad and a.requires_grad and not both:
                    self._flow_terms_deferred.append((w, term))
                continue
            if a.C != b.C or a.rows != b.rows:
                raise ValueError("loss operands of different shapes")
            grad = with_grad and a.requires_grad
            term.launch(self, w, value=True, grad=grad, accumulate=grad and a.grad_ptr in written)
            if grad:
                written.add(a.grad_ptr)
                _note_grad_written(a, False)

    def _flow_term_launch(self, w, term, value, grad, accumulate):
        """One call of a term on a flow (LossTerm.launch), refused where the add would land on a masked gradient."""
        if grad and accumulate and term.a.grad_masked:
            raise NotImplementedError("a loss term on a flow whose gradient buffer already holds d/d(pre-activation)")
        term.launch(self, w, value, grad, accumulate)
        if grad:
            _note_grad_written(term.a, False)

    def _flow_term_before(self, n, pending):
        """Reverse plan, in front of node n's backward: a deferred term on a tensor n produces whose gradient nobody
        has written STORES it (the term is that tensor's only source of gradient); the producer's backward then runs from it.
        Store or add is decided per term at its launch: of several terms on one tensor the first stores and the others add."""
        for wt in [wt for wt in pending if wt[1].a.producer is n]:
            self._flow_term_launch(wt[0], wt[1], value=False, grad=True, accumulate=wt[1].a.grad_written)
            pending.remove(wt)

    def _flow_term_after(self, pending):
        """Reverse plan, behind a node's backward: a deferred term whose tensor has just received its gradient from
        a consumer (the resampler's backward) ADDS its own, one fp32 addition per element, before the tensor's producer runs."""
        for wt in [wt for wt in pending if wt[1].a.grad_written]:
            self._flow_term_launch(wt[0], wt[1], value=False, grad=True, accumulate=True)
            pending.remove(wt)

    def _backward_node(self, n, pending):
        self._flow_term_before(n, pending)
        n.backward(self)
        self._flow_term_after(pending)

    @staticmethod
    def _flow_terms_all_placed(pending):
        """End of a reverse recording: a deferred term that found no place is an error, not a silently missing gradient."""
        if pending:
            raise RuntimeError("a loss term on a flow: the reverse pass has no place for the gradient of %d term(s): no node of "
                               "this graph produces the tensor" % len(pending))

    def compile(self, stream=None):
        """Record the forward (+loss, +loss gradient) and backward launch sequences."""
        self.finalize()
        self.stream = stream        # None = the null stream; plans take the stream at run time
        lib = self.lib
        for t in self.tensors:
            t.grad_written = t.grad_masked = False
        self._flow_terms_deferred = []
        self._bind_prepared_filters()
        self._fuse_resample_losses()
        # every term that needs a workspace keeps one of its own (not the shared scratch: see SsimTerm)
        for _, term in (self.loss_expr.terms if self.loss_expr is not None else ()):
            nbytes = term.workspace_bytes(lib) if term.ws is None else None
            if nbytes is not None:
                term.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._find_fc_chains()
        self.plan_fwd = lib.plan_create()
        lib.plan_begin(self.plan_fwd)
        try:
            lib.filter_cache_refresh(None)      # first launch of the step: convert every conv filter once
            # loss terms accumulate into loss_buf[0]; the first one recorded stores instead (no launch to clear the accumulator)
            if self.loss_expr is not None and self.loss_expr.terms:
                lib.loss_overwrite_next()
            else:
                lib.fill(self.loss_buf.data_ptr(), 1, 0.0, self.stream)
            self._fwd_first_op = {}
            for n in self.nodes:
                self._fwd_first_op[id(n)] = lib.plan_size(self.plan_fwd)
                n.forward(self)
            self._emit_losses(with_grad=True)
        finally:
            lib.plan_end()
        flags_after_forward = [(t.grad_written, t.grad_masked) for t in self.tensors]
        self.plan_bwd = lib.plan_create()
        lib.plan_begin(self.plan_bwd)
        self.grad_buckets = []          # [(plan op end index, lo, hi)]: grads[lo:hi] are final once ops [.., end) ran
        try:
            done = set()
            order = list(self.variables.values())
            suffix = len(order)         # variables[suffix:] are complete
            cut_hi = self.flat_size
            gate = 0
            pending = list(self._flow_terms_deferred)
            for n in reversed(self.nodes):
                self._backward_node(n, pending)
                if isinstance(n, LinearNode):
                    gate = lib.plan_size(self.plan_bwd)
                for v in (getattr(n, 'w', None), getattr(n, 'b', None), getattr(n, 'm', None)):
                    if isinstance(v, Variable):
                        done.add(v.name)
                # the completed variables form a growing suffix of the flat buffer when the backward
                # order mirrors the creation order (true for every sequential model of the reference)
                while suffix > 0 and order[suffix - 1].name in done:
                    suffix -= 1
                lo = order[suffix].offset if suffix < len(order) else self.flat_size
                # also cut where the reverse pass moves from convolutions to an fc layer: conv filters are read by the first
                # launch of the next step (filter conversion), fc matrices much later -- their buckets' all-gathers can run
                # under the next step's encoder (run_backward_overlapped), a mixed bucket could not
                boundary = False
                if isinstance(n, ConvNode) and cut_hi > lo:
                    for prev in reversed(self.nodes[:self.nodes.index(n)]):      # the next node of the reverse pass that owns parameters
                        if any(isinstance(v, Variable) for v in vars(prev).values()):
                            boundary = isinstance(prev, LinearNode)
                            break
                if cut_hi - lo >= self.bucket_elems or boundary:
                    self.grad_buckets.append((lib.plan_size(self.plan_bwd), lo, cut_hi))
                    cut_hi = lo
            self._flow_terms_all_placed(pending)
        finally:
            lib.plan_end()
        nbwd = lib.plan_size(self.plan_bwd)
        if cut_hi > 0 or not self.grad_buckets:
            self.grad_buckets.append((nbwd, 0, cut_hi))
        else:
            end, lo, hi = self.grad_buckets[-1]
            self.grad_buckets[-1] = (nbwd, lo, hi)
        # Extra (empty) segment boundary: the optimiser launches of the early (fc) buckets are held back until the main
        # stream is past the fc layers and the small-spatial convolutions -- kernels that stream HBM or wait on it like
        # Adam does and slow down 3-10x next to it -- and overlap the encoder's large MFMA-bound layers instead
        # (measured: 0.85-0.92 of the backward launch list beats 0.5-0.8 by ~1.5 %: the optimiser then runs next to the two
        # largest data-gradient kernels and the tail of the filter-gradient chain; 'fc' = right behind the last fc layer).
        mode = os.environ.get('MV3D_ADAM_GATE', '0.9')      # 'fc', 'none' or a fraction of the backward launch list
        if mode == 'none':
            gate = 0
        elif mode != 'fc':
            gate = int(float(mode) * nbwd)
        self.adam_gate = gate if 0 < gate < nbwd else 0
        if self.adam_gate and all(b[0] != self.adam_gate for b in self.grad_buckets):
            i = next(j for j, b in enumerate(self.grad_buckets) if b[0] > self.adam_gate)
            hi = self.grad_buckets[i][2]
            self.grad_buckets.insert(i, (self.adam_gate, hi, hi))
        # Adam runs over the prefix of the flat buffer that holds variables with a gradient path;
        # variables without one (highdim_angle.py:8-9) keep zero gradients and are never touched.
        self.n_launch_fwd = lib.plan_size(self.plan_fwd)
        self.n_launch_bwd = lib.plan_size(self.plan_bwd)
        self._bucket_first_use = [self._first_param_use(lo, hi) for _, lo, hi in self.grad_buckets]
        # Second recording of the reverse pass for the single-GPU step, with the optimiser of the large fc matrices fused into
        # their filter-gradient kernels (LinearNode.backward); the plain plan above stays for run_backward() (tests read the
        # gradients) and for the data-parallel step (the all-reduce needs them).
        self.plan_bwd_fused = None
        self._fused_vars = []
        self._fused_nodes = []
        # (not with gradient clipping: the fused kernels never write the fc gradients to memory, and the norm needs all of them;
        # not with gradient accumulation either: the sum needs them, and only the last micro-step updates)
        if self.fuse_fc_adam and self.clip_norm is None and not self.accum_steps and self.lr is not None and any(isinstance(n, LinearNode) for n in self.nodes):
            for t, (gw, gm) in zip(self.tensors, flags_after_forward):
                t.grad_written, t.grad_masked = gw, gm
            plan = lib.plan_create()
            self._finalized_in_plan = False
            if self.fuse_finalize:
                # every conv layer gets its own region for its per-slab partial filters (they live until the end of the pass)
                off = 0
                for n in self.nodes:
                    if isinstance(n, ConvNode):
                        n._part_off, n._part_bytes = off, n.wgrad_partial_bytes(self)
                        off += -(-n._part_bytes // 256) * 256
                self._part_arena = torch.empty(max(off // 4, 4), dtype=torch.float32, device=self.device)
                lib.grad_finalize_begin()
                self._finalizing = True
                self._fin_pending, self._fin_vars, self._fin_done, self._fin_tables = 0, [], set(), []
            lib.plan_begin(plan)
            self._fusing = True
            pending = list(self._flow_terms_deferred)
            try:
                for n in reversed(self.nodes):
                    self._backward_node(n, pending)
                    if self._finalizing and isinstance(n, ConvNode) and n.w.has_grad:
                        # the reduction (+ optimiser) of what has piled up goes out as soon as it is worth a launch: it then runs
                        # beside the rest of the pass instead of in its tail
                        self._fin_pending += n._part_bytes
                        self._fin_vars += [n.w] + ([n.b] if n.b is not None else [])
                        if self._fin_pending >= self.finalize_chunk_bytes:
                            self._finalize_commit()
                            lib.grad_finalize_begin()
                self._flow_terms_all_placed(pending)
                for n in self._fused_nodes:         # the fused fc optimiser goes behind the whole reverse pass
                    n.record_fused_update(self)
                if self._finalizing and self._fused_vars:
                    # everything else the optimiser owns: gradients that are already final in the flat buffer (the angle MLP, conv
                    # layers whose filter gradient is a single slab); the fused fc matrices and their biases are updated on the
                    # fused kernels' own stream (run_backward_fused).  Ranges a slab segment produces are dropped by the library.
                    fused = {id(v) for v in self._fused_vars} | {id(n.b) for n in self._fused_nodes}
                    for v in self.variables.values():
                        if v.has_grad and id(v) not in fused and id(v) not in self._fin_done:
                            lib.grad_finalize_add(v.grad_ptr, -(-v.size // 4) * 4)
                    self._finalize_commit()
                    self._finalizing = False
                    self._finalized_in_plan = True
            finally:
                self._fusing = False
                if self._finalizing:
                    lib.grad_finalize_abort()
                    self._finalizing = False
                lib.plan_end()
            if self._fused_vars:
                self.plan_bwd_fused = plan
                self.n_launch_bwd_fused = lib.plan_size(plan)
                # ranges of the flat buffers the main stream's optimiser launch leaves alone: the fused matrices, and their layers'
                # biases (whose gradients the fused kernels produce: their Adam runs behind those kernels, on their stream)
                def merged(ranges):
                    out = []
                    for lo, hi in sorted(ranges):
                        if out and lo <= out[-1][1]:
                            out[-1][1] = max(out[-1][1], hi)
                        else:
                            out.append([lo, hi])
                    return out
                pad4 = lambda v: (v.offset, v.offset + -(-v.size // 4) * 4)
                biases = merged(pad4(n.b) for n in self._fused_nodes)
                skips = merged([pad4(v) for v in self._fused_vars] + [tuple(b) for b in biases])
                assert len(skips) <= 8, "mv3d_adam_step_dev leaves at most 8 ranges untouched"
                self._skip_lo = (C.c_int64 * len(skips))(*[a for a, _ in skips])
                self._skip_hi = (C.c_int64 * len(skips))(*[b for _, b in skips])
                # the biases: ONE launch over [first bias, last bias end) that skips what lies between them
                self._bias_span = (biases[0][0], biases[-1][1])
                gaps = [(biases[i][1] - biases[0][0], biases[i + 1][0] - biases[0][0]) for i in range(len(biases) - 1)]
                assert len(gaps) <= 8
                self._bias_skip = (len(gaps), (C.c_int64 * max(1, len(gaps)))(*[a for a, _ in gaps] or [0]),
                                   (C.c_int64 * max(1, len(gaps)))(*[b for _, b in gaps] or [0]))
                self._fwd_wait_idx = self._first_fc_hazard()
                self._fc_ranges = [tuple(r) for r in skips]      # what the fused kernels and the bias launch update, on their stream
            else:
                lib.plan_destroy(plan)
        self._build_decay_table()
        self.upload_optimizer_state()
        self.reset_ema()
        return self

    # ---------------------------------------------------------------- learning-rate schedule, weight decay
    def enable_lr_schedule(self, spec):
        """Update number k (0-based, Graph.global_step) uses lr_schedule.learning_rate_at(spec, k): call before compile() with
        what lr_schedule_from_conf() returns; None leaves the switch off (the same plans, launches and bits).  Behind the last
        launch of an update that reads an optimiser record, on that launch's stream, mv3d_opt_set_lr writes the NEXT update's
        rate into it: a write in front of a step could race the previous update's fused fc launches still in flight."""
        if spec is None:
            return
        if self.plan_fwd is not None:
            raise RuntimeError("enable_lr_schedule: call it before compile()")
        from .lr_schedule import learning_rate_at
        learning_rate_at(spec, 0)           # a malformed spec raises here
        self.lr_spec = dict(spec)

    def enable_weight_decay(self, weight_decay):
        """Decoupled weight decay: after update k, on the updated weights, p -= p * f_k with f_k = float32(float64(lr_k) *
        weight_decay) -- the decay follows the scheduled rate, as torch.optim.AdamW scales it by the rate; it is applied BEHIND the
        update rather than in front of it, which differs from AdamW's order by O(f * update).  Only variables with a gradient
        whose name ends in /w or /Matrix decay; biases and variables without a gradient keep their bits.  Call before compile();
        None or 0 leave the switch off (nothing allocated, the same plans and launches)."""
        from .lr_schedule import check_weight_decay
        wd = check_weight_decay(weight_decay, "enable_weight_decay: weight_decay")      # the conf key's own check
        if wd is None:
            return
        if self.plan_fwd is not None:
            raise RuntimeError("enable_weight_decay: call it before compile()")
        self.weight_decay = wd

    def counts_updates(self):
        """True when a schedule, a warm-up or weight decay is on: checkpoints then carry `global_step`."""
        return self.lr_spec is not None or self.weight_decay is not None

    def learning_rate(self):
        """The host float32 the next update will use (the device records hold the same bits)."""
        if self.lr_spec is None:
            return None if self.lr is None else np.float32(self.lr)
        from .lr_schedule import learning_rate_at
        return learning_rate_at(self.lr_spec, self.global_step)

    def set_global_step(self, step):
        """The count of updates made so far (a resume from a checkpoint that does not carry it: train.py hands in the iteration of
        the file name); re-uploads the optimiser records with the rate of that update."""
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 0:
            raise ValueError("set_global_step: step must be an integer >= 0, got %r" % (step,))
        if self.accum_steps and self.micro_step:
            raise RuntimeError("set_global_step() in the middle of an accumulation cycle (micro-step %d of %d)"
                               % (self.micro_step, self.accum_steps))
        self.global_step = int(step)
        self.upload_optimizer_state()

    def _build_decay_table(self):
        """The decay set as ONE device table: the [begin, end) flat ranges of every variable with a gradient whose name ends in /w
        or /Matrix, each padded to a multiple of 4 (the padding floats are zero and p - p * f keeps them zero)."""
        self._decay_ranges, self._decay_table = [], None
        if self.weight_decay is None:
            return
        pad4 = lambda v: (v.offset, v.offset + -(-v.size // 4) * 4)
        self._decay_ranges = sorted(pad4(v) for k, v in self.variables.items()
                                    if v.has_grad and k.rsplit('/', 1)[-1] in ('w', 'Matrix'))
        n = len(self._decay_ranges)
        if n > _lib.DECAY_MAX_RANGES:
            raise ValueError("weight decay: %d decayed variables, mv3d_weight_decay_step takes at most %d ranges" % (n, _lib.DECAY_MAX_RANGES))
        assert all(a % 4 == 0 and b % 4 == 0 and a < b for a, b in self._decay_ranges)
        assert all(r[1] <= s[0] for r, s in zip(self._decay_ranges, self._decay_ranges[1:])) and (not n or self._decay_ranges[-1][1] <= self.flat_size)
        self._decay_table = torch.tensor(self._decay_ranges or [(0, 0)], dtype=torch.int64).reshape(-1).to(self.device)

    def _decay_factor(self):
        """f_k of the update being issued (k = global_step): raises when it reaches 1."""
        f = weight_decay_factor(self.learning_rate(), self.weight_decay)
        if not f < 1.0:
            raise ValueError("weight decay: f = float32(lr * weight_decay) = %r at update %d must stay below 1" % (float(f), self.global_step))
        return float(f)

    def _post_range(self, lo, hi, stream):
        """What follows the optimiser over the flat range [lo, hi), on its stream: mv3d_weight_decay_step (with EMA on, its fused
        form in place of the EMA launch, one for one), else mv3d_ema_step, else nothing."""
        if self.weight_decay is not None:
            ema = self.ema is not None
            w = float(ema_one_minus_decay(self.ema_decay, self.ema_updates if self.ema_num_updates else None)) if ema else 0.0
            self.lib.weight_decay_step(self.params.data_ptr(), self.ema.data_ptr() if ema else None, lo, hi,
                                       self._decay_table.data_ptr(), len(self._decay_ranges), self._decay_factor(), w, stream)
        elif self.ema is not None:
            self._ema_range(lo, hi, stream)

    def _lr_next(self, stream, main=True, fc=True):
        """mv3d_opt_set_lr with the rate of update global_step + 1 into the main and / or the fused fc optimiser's record, behind
        the last launch of update global_step that reads it, on that launch's stream.  Nothing without a schedule."""
        if self.lr_spec is None:
            return
        from .lr_schedule import learning_rate_at
        lr = float(learning_rate_at(self.lr_spec, self.global_step + 1))
        if main:
            self.lib.opt_set_lr(self.opt_state.data_ptr(), lr, stream)
        if fc:
            self.lib.opt_set_lr(self.opt_state.data_ptr() + 32, lr, stream)

    def _update_done(self):
        """Host bookkeeping of one optimiser update, once everything of it has been issued."""
        if self.ema is not None:
            self.ema_updates += 1
        self.global_step += 1

    # ---------------------------------------------------------------- EMA weights
    def enable_ema(self, decay, num_updates=False):
        """tf.train.ExponentialMovingAverage(decay, num_updates).apply(every variable), run behind each train step's optimiser:
        call before compile().  Graph.ema (flat, the layout of params) holds the shadows, Graph.ema_updates the number of updates
        made so far (the `num_updates` TF is handed when the switch is on: decay_t = min(decay, (1 + n) / (10 + n)))."""
        decay = float(decay)
        if not np.isfinite(decay) or not 0.0 < decay < 1.0:
            raise ValueError("enable_ema: decay must be finite and in (0, 1), got %r" % (decay,))
        if self.plan_fwd is not None:
            raise RuntimeError("enable_ema: call it before compile()")
        self.ema_decay, self.ema_num_updates = decay, bool(num_updates)
        if self.finalized and self.ema is None:
            self.ema = self.params.clone()

    def reset_ema(self):
        """Shadows := the variables as they are now, update counter := 0 (TF's initial state; call it after set_variables()
        when the new values are a fresh start rather than a step of this run).  No-op with EMA off."""
        if self.ema is None:
            return
        self._check_not_swapped('reset_ema')
        self._settle()
        self.ema.copy_(self.params)
        self.ema_updates = 0

    def _check_not_swapped(self, what):
        if self._ema_swapped:
            raise RuntimeError("%s inside ema_weights(): the parameter buffer holds the averaged weights" % what)

    def _ema_range(self, lo, hi, stream):
        """mv3d_ema_step over the flat range [lo, hi) on `stream`, behind the optimiser launch that updated it there."""
        w = float(ema_one_minus_decay(self.ema_decay, self.ema_updates if self.ema_num_updates else None))
        self.lib.ema_step(hi - lo, self.ema.data_ptr() + lo * 4, self.params.data_ptr() + lo * 4, w, stream)

    def _ema_side(self, stream):
        """The step leaves an EMA launch running on `stream` (a torch stream other than the current one): readers of Graph.ema
        and the next writers of params on other streams wait for this event (_settle()); the forward pass does not."""
        if self._ema_event is None:
            self._ema_event = torch.cuda.Event()
        self._ema_event.record(stream)
        self._ema_pending = True

    def get_ema_variables(self):
        """The shadows, like get_variables(): one host array per variable (a variable without a gradient equals its shadow)."""
        if self.ema is None:
            raise RuntimeError("get_ema_variables: EMA is off (Graph.enable_ema / conf['ema_decay'])")
        self._check_not_swapped('get_ema_variables')
        self._settle()
        return OrderedDict((k, self.ema[v.offset:v.offset + v.size].view(v.shape).detach().cpu().numpy().copy())
                           for k, v in self.variables.items())

    def _swap_ema(self):
        self._settle()
        if torch.device(self.device).type == 'cuda':
            self.lib.swap_f32(self.flat_size, self.params.data_ptr(), self.ema.data_ptr(), self._stream_ptr())
        else:
            tmp = self.params.clone()
            self.params.copy_(self.ema)
            self.ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """with g.ema_weights(): forward passes (evaluate, visualize) run on the averaged weights.  params and ema are exchanged
        in place (mv3d_swap_f32: no third buffer) and exchanged back on exit, also when the body raises; train_step() and the
        checkpoint calls raise RuntimeError inside.  Conv filters are re-converted by the first launch of every forward pass
        and fc matrices at each use, so nothing else has to be invalidated."""
        if self.ema is None:
            raise RuntimeError("ema_weights: EMA is off (Graph.enable_ema / conf['ema_decay'])")
        self._check_not_swapped('ema_weights')
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            self._swap_ema()

    # ---------------------------------------------------------------- global-norm gradient clipping
    def enable_grad_clip(self, clip_norm):
        """Clip the gradient of every train step to the global L2 norm clip_norm (finite, > 0), or with math.inf only measure the
        norm: call before compile().  A step then runs the schedule in which the whole gradient exists before the first update
        (train_step); grad_norm() reads the step's [norm, scale]."""
        c = float(clip_norm)
        with np.errstate(over='ignore', under='ignore'):
            c32 = float(np.float32(c))                  # what the kernel is handed
        if isinstance(clip_norm, bool) or not c > 0.0 or (math.isfinite(c) and not 0.0 < c32 < math.inf):
            raise ValueError("enable_grad_clip: clip_norm must be > 0 and a finite float32, or inf to measure only, got %r" % (clip_norm,))
        if self.plan_fwd is not None:
            raise RuntimeError("enable_grad_clip: call it before compile()")
        self.clip_norm = c
        if self.finalized and self.clip_buf is None:
            self._alloc_grad_clip()

    def _alloc_grad_clip(self):
        self.clip_buf = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._clip_ws_bytes = int(self.lib.grad_clip_workspace_bytes(self.flat_size))
        self._clip_ws = torch.empty(max(self._clip_ws_bytes // 8, 2), dtype=torch.float64, device=self.device)

    def clip_gradients(self):
        """mv3d_grad_clip_scale over the whole flat gradient buffer on the main stream, between the reverse pass (and the
        all-reduce) and the optimiser: the norm of the averaged gradient (pre_scale = float32(1 / world size)) and the clip scale
        go to grad_norm(), pre_scale * scale into the gradient-scale slot of both optimiser records.  The padding between
        variables and the ranges of variables without a gradient are zero (grads is torch.zeros and nothing writes there; a SUM
        over ranks keeps them zero), so the sum over [0, flat_size) is the sum over the gradients."""
        if self.clip_norm is None:
            raise RuntimeError("clip_gradients: gradient clipping is off (Graph.enable_grad_clip / conf['grad_clip_norm'])")
        self._settle()
        self.lib.grad_clip_scale(self.flat_size, self.grads.data_ptr(), self._grad_pre_scale(), self.clip_norm,
                                 self.clip_buf.data_ptr(), self.opt_state.data_ptr(), self.opt_state.data_ptr() + 32,
                                 self._clip_ws.data_ptr(), self._clip_ws_bytes, self._stream_ptr())

    def grad_norm(self):
        """The device tensor [norm, scale] of the last clipped step: the L2 norm of the averaged gradient before clipping and the
        factor the optimiser applied (1 where it did not clip).  Converting it to Python floats is the caller's synchronisation."""
        if self.clip_buf is None:
            raise RuntimeError("grad_norm: gradient clipping is off (Graph.enable_grad_clip / conf['grad_clip_norm'])")
        return self.clip_buf

    def run_backward_clipped(self, data_parallel=None):
        """Reverse pass, norm, optimiser -- the step with gradient clipping.  The whole gradient exists before the first update:
        single GPU the plain reverse pass; data parallel (default: world size > 1) the bucketed all-reduce of
        run_backward_overlapped, overlapped with the pass as ever, in either dp_mode -- every rank then reduces the same summed
        buffer in the same order, so the scale and the weights stay bit-identical across ranks and every rank holds complete
        optimiser slots.  The fused, finalize-fused, overlapped and sharded optimiser schedules need the update inside the pass
        and are not used."""
        if self.world_size > 1 if data_parallel is None else data_parallel:
            self.run_backward_overlapped(with_adam=False)
        else:
            self.run_backward()
        self.clip_gradients()
        self.apply_optimizer()

    # ---------------------------------------------------------------- gradient accumulation
    def enable_grad_accum(self, steps):
        """One optimiser update out of `steps` train_step() calls (micro-steps), each a forward and a plain reverse pass on its own
        micro-batch: call before compile().  None, 0 or 1 leave the switch off (nothing allocated, the same plans and launches); a
        bool, a non-integer or a negative value raises ValueError.  The network has no batch statistics and every loss is a mean
        over the batch, so N micro-batches of B give the gradient of one batch of N * B, up to rounding."""
        if steps is None:
            return
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError("enable_grad_accum: steps must be an integer >= 2 (or None / 0 / 1 for off), got %r" % (steps,))
        if steps < 2:
            return
        if self.plan_fwd is not None:
            raise RuntimeError("enable_grad_accum: call it before compile()")
        self.accum_steps = int(steps)
        if self.finalized and self.grad_sum is None:
            self._alloc_grad_accum()

    def _alloc_grad_accum(self):
        self.grad_sum = torch.zeros(self.flat_size, dtype=torch.float32, device=self.device)
        self._accum_loss = torch.zeros(2, dtype=torch.float32, device=self.device)

    def _grad_pre_scale(self):
        """float32(1 / (world size * micro-steps per update)): what turns the summed gradient buffer into the mean."""
        return float(np.float32(1.0 / (self.world_size * max(self.accum_steps, 1))))

    def accum_loss(self):
        """The device scalar ((l1 + l2) + ..) * float32(1 / N) over the micro-batches of the last completed cycle (0 before the
        first).  Converting it to a Python float is the caller's synchronisation."""
        if not self.accum_steps:
            raise RuntimeError("accum_loss: gradient accumulation is off (Graph.enable_grad_accum / conf['grad_accum_steps'])")
        return self._accum_loss[self._accum_done]

    def accumulate_gradients(self, fused_norm=False):
        """mv3d_grad_accumulate on the main stream behind the reverse pass of micro-step `micro_step`: STORE into grad_sum on the
        first, ADD on those between, FINISH on the last -- which writes the sum into grads, so that everything behind it reads
        the flat gradient buffer as ever.  The loss scalar rides along.  fused_norm (last micro-step only): FINISH also writes
        the chunk sums of squares of what it stored into the clipping workspace, for mv3d_grad_clip_finish."""
        if not self.accum_steps:
            raise RuntimeError("accumulate_gradients: gradient accumulation is off (Graph.enable_grad_accum / conf['grad_accum_steps'])")
        self._settle()
        n, k = self.accum_steps, self.micro_step
        mode = _lib.ACCUM_STORE if k == 0 else (_lib.ACCUM_FINISH if k == n - 1 else _lib.ACCUM_ADD)
        if fused_norm and (mode != _lib.ACCUM_FINISH or self.clip_norm is None):
            raise RuntimeError("accumulate_gradients: fused_norm needs the last micro-step and gradient clipping")
        self.lib.grad_accumulate(self.flat_size, self.grad_sum.data_ptr(), self.grads.data_ptr(), mode, self.loss_buf.data_ptr(),
                                 self._accum_loss.data_ptr() + 4 * self._accum_slot, float(np.float32(1.0 / n)),
                                 self._clip_ws.data_ptr() if fused_norm else None, self._clip_ws_bytes if fused_norm else 0,
                                 self._stream_ptr())

    def run_micro_step(self, data_parallel=None):
        """Reverse pass and what follows it in one micro-step of an accumulation cycle (train_step() has run the forward pass).
        Micro-steps 1 .. N - 1: the plain reverse pass, then STORE or ADD; no optimiser, no EMA, no beta-power advance, no
        communication -- parameters and slots keep their bits.  Micro-step N: the plain reverse pass and FINISH; data parallel
        (default: world size > 1) ONE all-reduce over the whole buffer, N times less communication than a step per micro-batch;
        with clipping the norm of the mean gradient, pre_scale = float32(1 / (world size * N)) -- single GPU
        mv3d_grad_clip_finish over the partials FINISH wrote, data parallel the ordinary mv3d_grad_clip_scale behind the
        all-reduce (which changes the buffer); then apply_optimizer(), once per update, on every rank over the whole buffer:
        complete slots and bit-identical weights on every rank, as in the clipped schedule."""
        dp = self.world_size > 1 if data_parallel is None else data_parallel
        self.run_backward()
        last = self.micro_step == self.accum_steps - 1
        fused_norm = last and self.clip_norm is not None and not dp
        self.accumulate_gradients(fused_norm=fused_norm)
        if not last:
            self.micro_step += 1
            return
        if dp:
            # allreduce_grads() without its world-size test (it skips at world size 1): data_parallel=True runs the exchange
            # through the communicator whatever the world size, which is how a one-GPU test covers this schedule
            self.comm.allreduce_sum_(self.grads, 0, self.flat_size, self._stream_ptr())
        if fused_norm:
            self.lib.grad_clip_finish(self.flat_size, self._grad_pre_scale(), self.clip_norm, self.clip_buf.data_ptr(),
                                      self.opt_state.data_ptr(), self.opt_state.data_ptr() + 32, self._clip_ws.data_ptr(),
                                      self._clip_ws_bytes, self._stream_ptr())
        elif self.clip_norm is not None:
            self.clip_gradients()
        self.apply_optimizer()
        self.micro_step = 0
        self._accum_done, self._accum_slot = self._accum_slot, self._accum_done

    def _finalize_commit(self):
        """Close the open mv3d_grad_finalize collection: one launch on the filter-gradient stream that sums the collected layers'
        slabs and applies their optimiser update (recorded into the plan being recorded)."""
        lib = self.lib
        on_gpu = torch.device(self.device).type == 'cuda'
        tb = int(lib.grad_finalize_table_bytes())
        table = torch.empty(max(tb, 16), dtype=torch.uint8, device=self.device) if on_gpu else None
        self._fin_tables.append(table)
        self.begin_side()
        try:
            tp = table.data_ptr() if on_gpu else None
            if self.optimizer == 'adam':
                lib.grad_finalize_commit(tp, tb, self.grads.data_ptr(), self.params.data_ptr(),
                                         self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.opt_state.data_ptr(), self.stream)
            else:
                lib.grad_finalize_commit_sgd(tp, tb, self.grads.data_ptr(), self.params.data_ptr(),
                                             self.accum.data_ptr() if self.accum is not None else None, self.opt_state.data_ptr(),
                                             self.stream)
        finally:
            self.end_side()
        self._fin_done |= {id(v) for v in self._fin_vars}
        self._fin_pending, self._fin_vars = 0, []

    def _bind_prepared_filters(self):
        """Weights only change in apply_adam(), so each conv filter is converted to the kernels' operand format
        once per step (mv3d_filter_cache_*, include/mv3d_hip.h) instead of once per call.  The library's cache is
        process-global: it is reset here, the plans recorded below keep their own copy of the job table."""
        lib = self.lib
        lib.filter_cache_clear()
        self._prepared = []
        if torch.device(self.device).type != 'cuda':      # plan recording without a GPU (host-logic tests): nothing to bind
            return
        for n in self.nodes:
            if not isinstance(n, ConvNode):
                continue
            geom = n.geom()
            ops = [2 if n.transposed else 0]
            if n.x.requires_grad:
                ops.append(3 if n.transposed else 1)
            for op in ops:
                nbytes = int(lib.filter_prepared_bytes(C.byref(geom), op))
                if nbytes > 0:
                    buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                    self._prepared.append(buf)
                    lib.filter_cache_bind(C.byref(geom), op, n.w.ptr, buf.data_ptr(), nbytes)
        tb = int(lib.filter_cache_table_bytes())
        self._prepared_table = torch.empty(max(tb, 16), dtype=torch.uint8, device=self.device)
        lib.filter_cache_commit(self._prepared_table.data_ptr(), tb, None)

    # ---------------------------------------------------------------- execution
    def _stream_ptr(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _first_param_use(self, lo, hi):
        """Index of the first forward launch that reads a parameter of the flat range [lo, hi): a conv filter is read by launch 0
        (the conversion of all filters, mv3d_filter_cache_refresh), everything else by its layer's first launch."""
        first = self.n_launch_fwd
        for n in self.nodes:
            for name, val in vars(n).items():
                if isinstance(val, Variable) and val.offset is not None and lo <= val.offset < hi:
                    first = min(first, 0 if (isinstance(n, ConvNode) and name == 'w') else self._fwd_first_op[id(n)])
        return first

    def _first_fc_hazard(self):
        """Index of the first forward launch that must not run before the previous step's fused fc optimiser finished: the
        first node that reads one of those matrices or touches the storage of a fused layer's saved input (the deferred
        kernels still read it).  None (no pipelining) when such an input is fed from outside the graph."""
        roots = set()
        for n in self._fused_nodes:
            root = n.x._root()[0]
            if root.external or n.x.storage.external:
                return None
            roots.add(id(root))
        def tensors_of(node):
            for val in vars(node).values():
                for t in (val if isinstance(val, (list, tuple)) else (val,)):
                    if isinstance(t, Tensor):
                        yield t
        fused = {id(n) for n in self._fused_nodes}
        idx = self.n_launch_fwd
        for n in self.nodes:
            if id(n) in fused or any(id(t._root()[0]) in roots for t in tensors_of(n)):
                idx = min(idx, self._fwd_first_op[id(n)])
        return idx

    def _settle_fc(self):
        """Order the current stream behind a fused fc optimiser still in flight from the last train step."""
        if self._fc_pending:
            torch.cuda.current_stream(self.device).wait_event(self._fc_event)
            self._fc_pending = False

    def _settle(self):
        """_settle_fc(), and behind the EMA launch that follows that optimiser on its stream (the forward pass waits for the
        optimiser alone: it reads the weights, never the shadows)."""
        self._settle_fc()
        if self._ema_pending:
            torch.cuda.current_stream(self.device).wait_event(self._ema_event)
            self._ema_pending = False

    settle = _settle        # public name: call before touching Graph.params / adam_m / adam_v / accum / grads directly

    def run_forward(self):
        st = self._stream_ptr()
        if self._fc_pending and 0 < self._pending_idx < self.n_launch_fwd:
            self.lib.plan_run_range(self.plan_fwd, 0, self._pending_idx, st)
            self._settle_fc()
            self.lib.plan_run_range(self.plan_fwd, self._pending_idx, self.n_launch_fwd, st)
            return
        self._settle_fc()
        self.lib.plan_run(self.plan_fwd, st)

    def begin_side(self, cls=1):
        """Tag the calls recorded until end_side() as side work of class `cls` (1: conv / fc filter gradients, 2: the fused fc
        optimiser; a class maps to side stream (cls - 1) % n_side); returns the scratch pointer reserved for that class."""
        if self.n_side == 0:
            return self.ws_ptr
        k = (cls - 1) % self.n_side
        self.lib.plan_side(k + 1)
        return self.ws_side[k].data_ptr()

    def end_side(self):
        if self.n_side:
            self.lib.plan_side(0)

    def _side_ptrs(self):
        """HIP streams for the filter-gradient kernels of the reverse pass (empty on CPU / when disabled)."""
        if self.n_side == 0 or torch.device(self.device).type != 'cuda':
            return None, 0
        if self.side_streams is None:
            self.side_streams = [torch.cuda.Stream(device=self.device) for _ in range(self.n_side)]
            self._side_arr = (C.c_void_p * self.n_side)(*[st.cuda_stream for st in self.side_streams])
        return self._side_arr, self.n_side

    def run_backward(self):
        self._settle()
        sides, ns = self._side_ptrs()
        self.lib.plan_run_range_multi(self.plan_bwd, 0, self.n_launch_bwd, self._stream_ptr(), sides, ns, 0)

    def allreduce_grads(self):
        self._settle()
        if self.world_size > 1:
            self.comm.allreduce_sum_(self.grads, 0, self.flat_size, self._stream_ptr())

    def upload_optimizer_state(self):
        """The device optimiser state: Adam's lr, betas, epsilon and the two beta powers, or Momentum / GD's lr, momentum and
        Nesterov flag; then the gradient scale (1 / world size; with gradient accumulation 1 / (world size * micro-steps))."""
        if self.opt_state is None or self.lr is None:
            return
        lr = self.lr if self.lr_spec is None else self.learning_rate()      # a schedule: learning_rate_at(global_step)
        if self.optimizer == 'adam':
            vals = [lr, self.beta1, self.beta2, self.eps, self.beta1_power, self.beta2_power]
        else:
            vals = [lr, self.momentum, 1.0 if self.use_nesterov else 0.0, 0.0, 0.0, 0.0]
        vals = np.array(vals + [1.0 / (self.world_size * max(self.accum_steps, 1)), 0.0], np.float32)
        self._settle()
        self.opt_state.copy_(torch.from_numpy(np.concatenate([vals, vals])))

    upload_adam_state = upload_optimizer_state

    def _opt_range(self, lo, hi, stream, skips=None, state=None):
        """The optimiser over the flat range [lo, hi) (minus `skips`): mv3d_adam_step_dev or mv3d_sgd_step_dev."""
        off = lo * 4
        n, slo, shi = (0, None, None) if skips is None else skips
        state = self.opt_state.data_ptr() if state is None else state
        if self.optimizer == 'adam':
            self.lib.adam_step_dev(hi - lo, self.params.data_ptr() + off, self.grads.data_ptr() + off, self.adam_m.data_ptr() + off,
                                   self.adam_v.data_ptr() + off, state, n, slo, shi, stream)
        else:
            self.lib.sgd_step_dev(hi - lo, self.params.data_ptr() + off, self.grads.data_ptr() + off,
                                  self.accum.data_ptr() + off if self.accum is not None else None, state, n, slo, shi, stream)

    _adam_range = _opt_range

    def _adam_advance(self, stream=None, both=True):
        """beta powers *= betas: on the device (behind every optimiser launch of this step) and in the host mirror the
        checkpoints read.  Momentum and GD have nothing to advance."""
        if self.optimizer != 'adam':
            return
        st = self._stream_ptr() if stream is None else stream
        self.lib.adam_advance(self.opt_state.data_ptr(), st)
        if both:                                             # the fused fc optimiser's record (advanced on its own stream by run_backward_fused)
            self.lib.adam_advance(self.opt_state.data_ptr() + 32, st)
        self.beta1_power = np.float32(self.beta1_power * np.float32(self.beta1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(self.beta2))

    def apply_optimizer(self):
        self._settle()
        self._opt_range(0, self.flat_size, self._stream_ptr())
        self._adam_advance()
        self._lr_next(self._stream_ptr())
        if self.ema is not None or self.weight_decay is not None:
            self._post_range(0, self.flat_size, self._stream_ptr())
        self._update_done()

    apply_adam = apply_optimizer

    def run_backward_fused(self):
        """Single-GPU reverse pass with the fc matrices' optimiser inside their filter-gradient kernels; one small launch
        updates everything else (conv filters, biases, the angle MLP: 3 % of the parameters) once the side streams joined."""
        sides, ns = self._side_ptrs()
        st = self._stream_ptr()
        pipelined = self.pipeline_fc and ns >= 2 and self._fwd_wait_idx is not None
        self.lib.plan_run_range_multi(self.plan_bwd_fused, 0, self.n_launch_bwd_fused, st, sides, ns, 1 if pipelined else 0)
        fc_state = self.opt_state.data_ptr() + 32
        if pipelined:
            main = torch.cuda.current_stream(self.device)
            for k, q in enumerate(self.side_streams):
                if k != 1 % ns:
                    main.wait_stream(q)                      # the conv filter gradients: the launch below reads them
            fcq = self.side_streams[1 % ns]                  # class 2: the fused fc optimiser
            fc_stream = fcq.cuda_stream
        else:
            fc_stream = st
        lo, hi = self._bias_span
        self._opt_range(lo, hi, fc_stream, self._bias_skip, state=fc_state)
        if self.optimizer == 'adam':
            self.lib.adam_advance(fc_state, fc_stream)
        self._lr_next(fc_stream, main=False)     # the fc record: behind its last reader of this update, on the fc stream
        decay = self.weight_decay is not None
        if decay:
            # the decay WRITES the fc matrices: it goes in front of _fc_event, which is what the next forward pass waits for before
            # it reads them.  With EMA on it is the fused launch and the event is recorded behind it: the other placement, the
            # pure decay in front of the event and the EMA behind it, measured 0.043 ms per step slower
            for a, b in self._fc_ranges:
                self._post_range(a, b, fc_stream)
        if pipelined:
            if self._fc_event is None:
                self._fc_event = torch.cuda.Event()
            self._fc_event.record(fcq)
            self._fc_pending = True
            self._pending_idx = self._fwd_wait_idx
        if not self._finalized_in_plan:          # otherwise the plan's last launch (grad_finalize_<kind>) was the optimiser of everything else
            self._opt_range(0, self.flat_size, st, (len(self._skip_lo), self._skip_lo, self._skip_hi))
        self._adam_advance(st, both=False)
        self._lr_next(st, fc=False)
        if self.ema is not None or decay:
            # every range behind its optimiser, on that optimiser's stream: the fused matrices and their layers' biases on the fc
            # stream (EMA alone behind _fc_event: the next forward pass does not wait for it), the rest on the main stream (which
            # has joined the stream of the grad_finalize launches).  The next step's writers of params fork from the main stream or
            # sit on the fc stream, so they are behind these reads.
            at = 0
            for a, b in self._fc_ranges:
                if a > at:
                    self._post_range(at, a, st)
                if not decay:
                    self._ema_range(a, b, fc_stream)
                at = b
            if at < self.flat_size:
                self._post_range(at, self.flat_size, st)
            if pipelined and self.ema is not None and not decay:
                self._ema_side(fcq)
        self._update_done()

    def run_backward_with_adam(self):
        """Single-GPU reverse pass with the optimiser folded in: the backward plan is issued bucket by bucket
        (the same >= 64 MB suffix buckets the data-parallel path all-reduces); as soon as a bucket's gradients are
        final -- its filter-gradient kernels sit on the side streams -- Adam for that slice of the flat buffers
        starts on its own stream while the main stream continues with the data gradients of the layers below.
        Adam is pure HBM streaming (28 B per parameter), the convolution kernels it overlaps are MFMA / latency bound."""
        self._settle()
        main = torch.cuda.current_stream(self.device)
        sides, ns = self._side_ptrs()
        if self.adam_stream is None:
            self.adam_stream = torch.cuda.Stream(device=self.device)
        begin, pending = 0, []
        for end, lo, hi in self.grad_buckets:
            self.lib.plan_run_range_multi(self.plan_bwd, begin, end, main.cuda_stream, sides, ns, 1)      # no join
            begin = end
            if hi > lo:
                pending.append((lo, hi))
            if end < self.adam_gate or not pending:
                continue
            # the slices' gradients come from side-stream kernels; their weights were last read by main-stream kernels
            self.adam_stream.wait_stream(main)
            for st in (self.side_streams or []):
                self.adam_stream.wait_stream(st)
            for plo, phi in pending:
                if self.adam_timing is not None:      # bench: HIP events around the optimiser launches, on their stream
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self.adam_stream)
                self._opt_range(plo, phi, self.adam_stream.cuda_stream)
                if self.adam_timing is not None:
                    e1.record(self.adam_stream)
                    self.adam_timing.append((e0, e1))
                if self.ema is not None or self.weight_decay is not None:       # behind the slice's optimiser, on its stream (joined below)
                    self._post_range(plo, phi, self.adam_stream.cuda_stream)
            pending = []
        main.wait_stream(self.adam_stream)
        for st in (self.side_streams or []):
            main.wait_stream(st)
        self._adam_advance(main.cuda_stream)
        self._lr_next(main.cuda_stream)
        self._update_done()

    run_backward_with_optimizer = run_backward_with_adam

    def run_backward_overlapped(self, with_adam=False):
        """Data-parallel reverse pass.  The recorded backward sequence is issued in segments; after each segment the gradients
        it completed -- a contiguous suffix range of the flat buffer, >= 64 MB: the fc matrices, 97 % of the bytes, are final
        after the decoder's half of the reverse pass -- go to the communicator on its own stream while the next segment computes:
          'sharded'    reduce-scatter(SUM) of the bucket -> TF-Adam on this rank's 1/world slice of it (grad scale 1/world) ->
                       all-gather of the updated parameters, all on the communication stream.  The optimiser's 28 B/param are
                       paid once per node instead of once per GPU, and the all-gather of a bucket only overwrites weights no
                       later kernel of this step reads (a layer's data gradient precedes its bucket).
          'allreduce'  SUM all-reduce of the bucket, then Adam on all of it on every rank (identical weights by construction).
        Both leave bit-identical weights on every rank (tests/test_dist_cpu.py)."""
        self._settle()
        main = self._stream_ptr()
        sides, ns = self._side_ptrs()
        on_gpu = torch.device(self.device).type == 'cuda'
        if on_gpu and self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(device=self.device)
        cs = self.comm_stream.cuda_stream if on_gpu else None
        comm, W = self.comm, self.world_size
        begin = 0
        late = []                       # [(first forward launch that reads the bucket, lo, slice length)]
        for end, lo, hi in self.grad_buckets:
            # the segment's filter-gradient launches stay on their side streams: only the COMMUNICATION stream waits for them (the
            # main stream goes straight on with the next layers' data gradients instead of idling behind an 80 us fc filter gradient
            # at every bucket boundary)
            self.lib.plan_run_range_multi(self.plan_bwd, begin, end, main, sides, ns, 1 if on_gpu else 0)
            begin = end
            if hi <= lo:
                continue
            if on_gpu:
                self.comm_stream.wait_stream(torch.cuda.current_stream(self.device))
                for q in (self.side_streams or []):
                    self.comm_stream.wait_stream(q)
                ctx = torch.cuda.stream(self.comm_stream)      # a torch.distributed communicator takes the current stream
                ctx.__enter__()
            if self.dp_mode == 'sharded' and with_adam:
                n = (hi - lo) // W
                assert n * W == hi - lo and n % 4 == 0, "bucket not divisible by 4 * world"
                comm.reduce_scatter_sum_(self.grads, lo, n, cs)
                a = lo + comm.rank * n
                self._opt_range(a, a + n, cs)
                self._slots_sharded = bool(self._slots())      # this rank's optimiser slots are now current on its own slices only
                # the updated slices of a bucket whose parameters the next forward pass reads late (the fc matrices: 97 % of the
                # bytes) are gathered AFTER every bucket has been reduced and, on the GPU, under the next step's encoder
                use = self._bucket_first_use[self.grad_buckets.index((end, lo, hi))]
                if self.pipeline_dp and use >= self.pipeline_dp_min_idx:
                    late.append((use, lo, n))
                else:
                    comm.allgather_(self.params, lo, n, cs)
            else:
                comm.allreduce_sum_(self.grads, lo, hi - lo, cs)
                if with_adam:
                    self._opt_range(lo, hi, cs)
            if on_gpu:
                ctx.__exit__(None, None, None)
        if on_gpu:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.comm_stream)                # every reduce-scatter, Adam slice and early all-gather
            for q in (self.side_streams or []):              # (and any filter gradient behind the last bucket's boundary)
                cur.wait_stream(q)
        if late:
            late.sort()
            if on_gpu:
                ctx = torch.cuda.stream(self.comm_stream)
                ctx.__enter__()
            for _, lo, n in late:
                comm.allgather_(self.params, lo, n, cs)
            if on_gpu:
                ctx.__exit__(None, None, None)
        decay = with_adam and self.weight_decay is not None
        if decay:
            # ONE launch over the whole buffer on the communication stream, behind the last all-gather (late ones included) and IN
            # FRONT of _fc_event: the decay writes the weights the next forward pass waits for.  Every rank decays identical
            # parameters, so the weights stay bit-identical across ranks; with EMA on it is the fused form
            self._post_range(0, self.flat_size, cs)
        if late and on_gpu:
            if self._fc_event is None:
                self._fc_event = torch.cuda.Event()
            self._fc_event.record(self.comm_stream)
            self._fc_pending = True
            # (with the decay the event covers weights of EVERY bucket, the conv filters the first forward launch reads among
            # them: the next forward pass then waits in front of its first launch)
            self._pending_idx = 0 if decay else late[0][0]
        elif decay and on_gpu:
            torch.cuda.current_stream(self.device).wait_stream(self.comm_stream)
        if with_adam:
            self._adam_advance()
            self._lr_next(self._stream_ptr())
            if self.ema is not None and not decay:
                # ONE launch over the whole buffer on the communication stream, behind the last all-gather (late ones included)
                # and behind _fc_event: every rank keeps the complete shadow of its (bit-identical) parameters
                self._ema_range(0, self.flat_size, cs)
                if on_gpu:
                    self._ema_side(self.comm_stream)
            self._update_done()

    def train_step(self):
        """forward + loss + reverse pass + (all-reduce) + optimiser (+ EMA of the weights); returns the device loss scalar.  With
        gradient accumulation one micro-step (run_micro_step): every accum_steps-th call updates, and the scalar returned is the
        micro-batch's loss (accum_loss() is the cycle's mean)."""
        self._check_not_swapped('train_step')
        if self.weight_decay is not None:
            self._decay_factor()            # f >= 1 raises before anything of the step is issued
        self.run_forward()
        if self.accum_steps:
            self.run_micro_step()
        elif self.clip_norm is not None:
            self.run_backward_clipped()
        elif self.world_size > 1:
            self.run_backward_overlapped(with_adam=True)
        elif self.plan_bwd_fused is not None:
            self.run_backward_fused()
        elif self.overlap_adam and torch.device(self.device).type == 'cuda':
            self.run_backward_with_adam()
        else:
            self.run_backward()
            self.apply_optimizer()
        return self.loss_buf[0]

    # ---------------------------------------------------------------- variables I/O
    def get_variables(self):
        self._settle()
        return OrderedDict((k, v.value().detach().cpu().numpy().copy()) for k, v in self.variables.items())

    def set_variables(self, values):
        self._settle()
        for k, a in values.items():
            self.variables[k].value().copy_(torch.as_tensor(np.asarray(a, dtype=np.float32)).reshape(self.variables[k].shape))

    def get_gradients(self):
        """One host array per variable with a gradient, as the flat gradient buffer holds it.  With gradient accumulation, after
        an update that is the UNSCALED sum over the cycle's micro-batches (the optimiser applied float32(1 / (world size * N))
        through its gradient-scale slot); in the middle of a cycle it is the last micro-batch's own gradient."""
        self._settle()
        return OrderedDict((k, v.grad_value().detach().cpu().numpy().copy()) for k, v in self.variables.items() if v.has_grad)

    def _slots(self):
        """[(TF slot name, flat buffer)] of the active optimiser: tf.train.AdamOptimizer's 'Adam' (m) and 'Adam_1' (v),
        tf.train.MomentumOptimizer's 'Momentum', none for tf.train.GradientDescentOptimizer."""
        if self.optimizer == 'adam':
            return [('Adam', self.adam_m), ('Adam_1', self.adam_v)]
        if self.optimizer == 'momentum':
            return [('Momentum', self.accum)]
        return []

    def gather_optimizer_state(self):
        """COLLECTIVE (every rank calls it): after sharded data-parallel steps a rank's optimiser slots are current only on its own
        1/world slice of every bucket; all-gather them (same lo / n layout as the parameters) so that any rank can write a
        complete checkpoint.  No-op on one GPU and in 'allreduce' mode."""
        self._settle()
        if self.world_size <= 1 or not getattr(self, '_slots_sharded', False):
            return
        on_gpu = torch.device(self.device).type == 'cuda'
        if on_gpu:
            torch.cuda.synchronize(self.device)
        cs = self._stream_ptr() if on_gpu else None
        W = self.world_size
        for _, lo, hi in self.grad_buckets:
            if hi > lo:
                n = (hi - lo) // W
                for _, buf in self._slots():
                    self.comm.allgather_(buf, lo, n, cs)
        if on_gpu:
            torch.cuda.synchronize(self.device)
        self._slots_sharded = False

    def state_dict(self):
        """TF-Saver-style names: <var> and the active optimiser's slots -- <var>/Adam, <var>/Adam_1, beta1_power, beta2_power
        (Adam), <var>/Momentum (Momentum), nothing else (GD) -- (train.py:70-71 saves GLOBAL_VARIABLES).  With EMA on also
        <var>/ExponentialMovingAverage for EVERY variable (TF's shadow variables) and the update counter
        ExponentialMovingAverage/num_updates; every data-parallel rank holds the complete shadows.  With a learning-rate schedule, a
        warm-up or weight decay on also the int64 scalar global_step, the number of optimiser updates made (with all of them off
        the keys are exactly those above).  With gradient accumulation
        it raises RuntimeError in the middle of a cycle: the partial gradient sum is not part of a checkpoint."""
        self._check_not_swapped('state_dict')
        if self.accum_steps and self.micro_step:
            raise RuntimeError("state_dict() in the middle of an accumulation cycle (micro-step %d of %d): the partial gradient sum is "
                               "not checkpointed; save at an update boundary" % (self.micro_step, self.accum_steps))
        self._settle()
        if self.world_size > 1 and getattr(self, '_slots_sharded', False):
            raise RuntimeError("sharded data-parallel step: this rank holds 1/%d of the optimiser slots; call "
                               "Graph.gather_optimizer_state() on EVERY rank before state_dict() / Saver.save()" % self.world_size)
        sd = OrderedDict()
        slots = self._slots()
        for k, v in self.variables.items():
            sd[k] = v.value().detach().cpu().clone()
            if v.has_grad:
                for name, buf in slots:
                    sd[k + '/' + name] = buf[v.offset:v.offset + v.size].view(v.shape).detach().cpu().clone()
            if self.ema is not None:
                sd[k + '/' + EMA_SLOT] = self.ema[v.offset:v.offset + v.size].view(v.shape).detach().cpu().clone()
        if self.optimizer == 'adam':
            sd['beta1_power'] = torch.tensor(float(self.beta1_power))
            sd['beta2_power'] = torch.tensor(float(self.beta2_power))
        if self.ema is not None:
            sd[EMA_COUNTER] = torch.tensor(float(self.ema_updates))
        if self.counts_updates():           # only with a schedule, a warm-up or weight decay on: otherwise exactly the keys above
            sd[GLOBAL_STEP] = torch.tensor(self.global_step, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd):
        """Restores what state_dict() names; KeyError on a missing or unexpected entry.  With EMA on, a checkpoint that carries
        every shadow and the counter restores them; one that carries none is a resume that turns the switch on (shadows := the
        restored variables, counter := 0); one that carries some of them raises KeyError.  With EMA off shadow entries are
        unexpected like any other.  With a schedule, a warm-up or weight decay on, global_step comes from the checkpoint, or is 0
        where it has none (global_step_restored tells which; set_global_step() is the caller's remedy), and the optimiser records
        are re-uploaded with the rate of that update."""
        self._check_not_swapped('load_state_dict')
        self._settle()
        slots = self._slots()
        names = {n for n, _ in slots}
        step = None
        if self.counts_updates():           # with the switches off `global_step` is unexpected like any other entry
            sd = OrderedDict(sd)
            step = sd.pop(GLOBAL_STEP, None)
        ema_keys = []
        if self.ema is not None:
            ema_keys = [k + '/' + EMA_SLOT for k in self.variables] + [EMA_COUNTER]
            have = [k for k in ema_keys if k in sd]
            if have and len(have) != len(ema_keys):
                raise KeyError("checkpoint holds %d of the model's %d EMA entries (<var>/%s and %s): missing %s"
                               % (len(have), len(ema_keys), EMA_SLOT, EMA_COUNTER, [k for k in ema_keys if k not in sd][:8]))
            sd = OrderedDict(sd)
            ema_sd = {k: sd.pop(k) for k in have}
            bad_ema = [k for k, v in self.variables.items() if k + '/' + EMA_SLOT in ema_sd and
                       tuple(ema_sd[k + '/' + EMA_SLOT].shape) != tuple(v.shape)]
            if bad_ema:
                raise KeyError("checkpoint does not match the model: shape mismatch of the EMA shadows of %s" % bad_ema[:8])
        missing = [k for k in self.variables if k not in sd]
        if self.optimizer == 'momentum':        # the accumulator is what identifies a Momentum checkpoint (Adam's: the beta powers)
            missing += [k + '/Momentum' for k, v in self.variables.items() if v.has_grad and k + '/Momentum' not in sd]
        scalars = {'beta1_power', 'beta2_power'} if self.optimizer == 'adam' else set()
        unexpected = [k for k in sd if k not in scalars and k not in self.variables and
                      not (k.rsplit('/', 1)[0] in self.variables and k.rsplit('/', 1)[-1] in names)]
        bad = [k for k, v in self.variables.items() if k in sd and tuple(sd[k].shape) != tuple(v.shape)]
        if missing or unexpected or bad or not scalars <= set(sd):
            raise KeyError("checkpoint does not match the model (%s optimizer): missing %s; unexpected %s; shape mismatch %s%s"
                           % (self.optimizer, missing[:8], unexpected[:8], [(k, tuple(sd[k].shape), self.variables[k].shape) for k in bad[:8]],
                              '' if scalars <= set(sd) else '; no beta1_power / beta2_power'))
        for k, v in self.variables.items():
            v.value().copy_(sd[k])
            for name, buf in slots:
                if k + '/' + name in sd:
                    buf[v.offset:v.offset + v.size].view(v.shape).copy_(sd[k + '/' + name])
        if self.optimizer == 'adam':
            self.beta1_power = np.float32(float(sd['beta1_power']))
            self.beta2_power = np.float32(float(sd['beta2_power']))
        if self.ema is not None:
            if ema_sd:
                for k, v in self.variables.items():
                    self.ema[v.offset:v.offset + v.size].view(v.shape).copy_(ema_sd[k + '/' + EMA_SLOT])
                self.ema_updates = int(round(float(ema_sd[EMA_COUNTER])))
            else:
                self.ema.copy_(self.params)
                self.ema_updates = 0
        self.micro_step = 0             # an accumulation cycle starts afresh on the restored weights
        if self.counts_updates():       # a checkpoint without the counter: 0 (train.py then hands in the file name's iteration)
            self.global_step = 0 if step is None else int(step)
            self.global_step_restored = step is not None
        self.upload_optimizer_state()


# =============================================================================================== initialisers
def truncated_normal_init(stddev):
    """tf.truncated_normal_initializer(stddev) (tf_utils.py:77): redraw beyond 2 sigma."""
    def init(rng, shape):
        out = rng.standard_normal(shape)
        bad = np.abs(out) > 2
        while bad.any():
            out[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(out) > 2
        return (out * stddev).astype(np.float32)
    return init


def random_normal_init(stddev):
    """tf.random_normal_initializer(stddev) (tf_utils.py:63,95)."""
    return lambda rng, shape: (rng.standard_normal(shape) * stddev).astype(np.float32)


def zeros_init():
    """tf.constant_initializer(0.) (tf_utils.py:65,80)."""
    return lambda rng, shape: np.zeros(shape, np.float32)
