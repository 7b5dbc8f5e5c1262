"""Host-side mirror of the reference op library dyn_mult_view/mv3d/utils/tf_utils.py:18-98.

Same function names, argument order and variable naming ('<scope>/w', '<scope>/b',
'<scope>/Matrix'); instead of TensorFlow graph nodes the functions append launch nodes of
libmv3d_hip.so to the current Graph (graph.py).  Activations that directly follow a
conv / deconv / linear are fused into that kernel's epilogue.
"""
import math

from .graph import (current_graph, Tensor, Storage, ScalarExpr, PixelTerm, SsimTerm, CensusTerm, SmoothTerm, MultiscaleTerm, ConsistTerm,
                    LOSS_L1, LOSS_L2, ConvNode, LinearNode, ActNode, ViewNode, CopyConcatNode, TileNode, ResampleNode, ResamplerNode,
                    OcclusionMaskNode, truncated_normal_init, random_normal_init, zeros_init)
from ._lib import ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH


class variable_scope:
    """tf.variable_scope(name): prefixes variable names (main_model.py:58,69)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        current_graph()._scope.append(self.name)
        return self

    def __exit__(self, *a):
        current_graph()._scope.pop()


def _check_usable(t):
    if t.fused_into is not None:
        raise RuntimeError("pre-activation tensor was fused into its producer's epilogue; use the activation output")


def _same_out(size, s):
    return -(-size // s)


# ------------------------------------------------------------------------------------------------ losses
class _Scaled:
    """x * c for a constant c: a loss target only (mv3d/bg_nodm.py:88 `gt_sm = gt_sm * 0.75`); folded into the loss kernel."""

    def __init__(self, x, c):
        self.x, self.c = x, float(c)


class _Masked:
    """tf.multiply(x, mask) with a one-channel mask: a loss operand only (mv3d/bg_nodm.py:91); (a*m - b*m) is evaluated
    as (a - b)*m inside the loss kernel."""

    def __init__(self, x, mask):
        self.x, self.mask = x, mask


def scale(x, c):
    return _Scaled(x, c)


def multiply(x, mask):
    if mask.C != 1:
        raise NotImplementedError("multiply: only a one-channel mask is supported")
    return _Masked(x, mask)


def _loss_term(input1, input2, kind, mask=None):
    for v in (input1, input2):
        if isinstance(v, _Masked):
            if mask is not None and mask is not v.mask:
                raise NotImplementedError("loss operands multiplied by different masks")
            mask = v.mask
    a, b = (v.x if isinstance(v, _Masked) else v for v in (input1, input2))
    # the differentiated operand goes first; both reference losses are symmetric in their arguments
    a_grad = (a.x if isinstance(a, _Scaled) else a).requires_grad
    b_grad = (b.x if isinstance(b, _Scaled) else b).requires_grad
    if b_grad and not a_grad:
        a, b = b, a
    elif a_grad and b_grad:
        raise NotImplementedError("loss between two differentiated tensors")
    if isinstance(a, _Scaled):
        raise NotImplementedError("scaling the differentiated operand of a loss")
    b_scale = 1.0
    if isinstance(b, _Scaled):
        b, b_scale = b.x, b.c
    return ScalarExpr([(1.0, PixelTerm(a, b, kind, mask, b_scale))])


def _image_pair(op, input1, input2):
    """(differentiated, other) operand of the symmetric image loss `op`: plain tensors, exactly one of them differentiated."""
    for v in (input1, input2):
        if isinstance(v, (_Masked, _Scaled)):
            raise NotImplementedError("%s of a masked or scaled operand" % op)
    if input2.requires_grad and not input1.requires_grad:
        return input2, input1
    if input1.requires_grad and input2.requires_grad:
        raise NotImplementedError("loss between two differentiated tensors")
    return input1, input2


def _image_mask(op, mask, a):
    """The mask operand of the image loss `op` on the differentiated operand a, or None: a graph tensor [N,H,W,1] over a's N, H, W
    that is not differentiated (an occlusion_mask() output, or a one-channel view of a constant tensor)."""
    if mask is None:
        return None
    if isinstance(mask, (_Masked, _Scaled)):
        raise NotImplementedError("%s of a masked or scaled operand" % op)
    if not isinstance(mask, Tensor) or len(mask.shape) != 4 or tuple(mask.shape) != tuple(a.shape[:3]) + (1,):
        raise ValueError("%s: mask must be a tensor [N,H,W,1] over the operands' %s, got %s" % (op, tuple(a.shape[:3]), getattr(mask, 'shape', mask)))
    if mask.requires_grad:
        raise ValueError("%s: the mask is not differentiated; it must not require a gradient" % op)
    _check_usable(mask)
    return mask


def _check_flow(op, flow):
    """The flow operand of the op `op`: a usable tensor [N,H,W,2], neither masked nor scaled."""
    if isinstance(flow, (_Masked, _Scaled)):
        raise NotImplementedError("%s of a masked or scaled operand" % op)
    if not isinstance(flow, Tensor) or len(flow.shape) != 4 or flow.shape[3] != 2:
        raise ValueError("%s: flow must be a tensor [N,H,W,2], got %s" % (op, getattr(flow, 'shape', flow)))
    _check_usable(flow)


def euclidean_loss(input1, input2):
    """tf_utils.py:18-19: reduce_mean(reduce_sum(pow(a-b, 2), 3))."""
    return _loss_term(input1, input2, 2)


def l1_loss(input1, input2):
    """tf_utils.py:22-23: reduce_mean(reduce_sum(abs(a-b), 3))."""
    return _loss_term(input1, input2, 1)


def masked_euclidean_loss(input1, input2, mask):
    """reduce_mean(reduce_sum(pow((a-b)*mask, 2), 3)) -- the inline expression of
    multi_view_model/multiobject_appflow.py:239-242 (mask is [B,H,W,1])."""
    return _loss_term(input1, input2, 2, mask)


def ssim_loss(input1, input2, max_val=1.0, mask=None):
    """1 - reduce_mean(tf.image.ssim(a, b, max_val)) for images of one size: the mean over images, fully-inside 11x11 Gaussian
    windows and channels (mv3d_ssim_loss; metrics.py states the definition).  Operands [N,H,W,C] with H, W >= 11 and C <= 4;
    exactly one of them is differentiated.  Masked and scaled operands are not supported.  mask (optional): a graph tensor
    [N,H,W,1] that is not differentiated, usually occlusion_mask(flow); every window is then weighed by the mask at its centre and
    the mean keeps its count (mv3d_ssim_loss_masked; metrics.ssim_loss_host states the definition)."""
    a, b = _image_pair('ssim_loss', input1, input2)
    if len(a.shape) != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("ssim_loss: operands must be [N,H,W,C] of one shape, got %s and %s" % (a.shape, b.shape))
    if a.shape[1] < 11 or a.shape[2] < 11 or a.C > 4:
        raise ValueError("ssim_loss: needs H, W >= 11 and C <= 4, got %s" % (a.shape,))
    if not (math.isfinite(float(max_val)) and float(max_val) > 0):
        raise ValueError("ssim_loss: max_val must be finite and positive")
    return ScalarExpr([(1.0, SsimTerm(a, b, max_val, _image_mask('ssim_loss', mask, a)))])


def census_loss(input1, input2, max_val=1.0, radius=3, eps=0.01, mask=None):
    """The soft census (ternary) loss of the prediction against the target (mv3d_census_loss; metrics.census_loss_host states the
    definition): the mean over images and fully-inside (2 radius + 1)^2 patches of the Charbonnier penalty (parameter eps) of the
    distance between the two images' soft census signatures, computed on the channel mean scaled to 0..255 by max_val.  Operands
    [N,H,W,C] with H, W >= 2 radius + 1, C <= 4 and radius in 1..3; exactly one of them is differentiated, and it goes first (the
    value does not depend on the order, the gradient is the differentiated operand's).  Masked and scaled operands are not
    supported.  mask (optional): a graph tensor [N,H,W,1] that is not differentiated, usually occlusion_mask(flow); every valid
    pixel's penalty is then weighed by the mask there and the mean keeps its count (mv3d_census_loss_masked;
    metrics.census_loss_host states the definition)."""
    from .metrics import _census_scalars, _census_shape
    a, b = _image_pair('census_loss', input1, input2)
    max_val, _, radius, eps = _census_scalars(max_val, 1.0, radius, eps)
    _census_shape(a.shape, b.shape, radius)
    return ScalarExpr([(1.0, CensusTerm(a, b, max_val, radius, eps, _image_mask('census_loss', mask, a)))])


def flow_smoothness_loss(flow, guide=None, edge_alpha=10.0, eps=1e-3, order=1):
    """Edge-aware first-order smoothness of a flow field [N,H,W,2] (mv3d_flow_smoothness; metrics.flow_smoothness_host states the
    definition): the mean Charbonnier penalty sqrt(d^2 + eps^2) - eps of the horizontal plus that of the vertical differences,
    each difference weighted by exp(-edge_alpha * mean_k |difference of the guide|) when a guide image [N,H,W,1..4] is given.
    The flow must be differentiated (it is usually an intermediate tensor: its gradient from the consumer and this term's are
    added); the guide must not be.  Masked and scaled operands are not supported.  order=2: the same penalty of the SECOND
    differences (mv3d_flow_smoothness2; H, W >= 3), minimal for an affine flow; a stencil's weight is the product of the weights
    of the two edges it spans."""
    from .metrics import _smooth_order
    if isinstance(guide, (_Masked, _Scaled)):
        raise NotImplementedError("flow_smoothness_loss of a masked or scaled operand")
    _check_flow('flow_smoothness_loss', flow)
    order = _smooth_order(order)
    if flow.shape[1] < order + 1 or flow.shape[2] < order + 1:
        raise ValueError("flow_smoothness_loss: needs H, W >= %d, got %s" % (order + 1, flow.shape,))
    if not flow.requires_grad:
        raise ValueError("flow_smoothness_loss: the flow is not differentiated (nothing to regularise)")
    if guide is not None:
        if not isinstance(guide, Tensor) or len(guide.shape) != 4 or tuple(guide.shape[:3]) != tuple(flow.shape[:3]) or not 1 <= guide.C <= 4:
            raise ValueError("flow_smoothness_loss: guide must be [N,H,W,1..4] over the flow's %s, got %s"
                             % (flow.shape[:3], getattr(guide, 'shape', guide)))
        if guide.requires_grad:
            raise NotImplementedError("flow_smoothness_loss: the guide is not differentiated; it must not require a gradient")
    edge_alpha, eps = float(edge_alpha), float(eps)
    if not (math.isfinite(edge_alpha) and edge_alpha >= 0):
        raise ValueError("flow_smoothness_loss: edge_alpha must be finite and >= 0")
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError("flow_smoothness_loss: eps must be finite and positive")
    return ScalarExpr([(1.0, SmoothTerm(flow, guide, edge_alpha, eps, second_order=order == 2))])


def multiscale_photometric_loss(flow, src_img, target, levels=3, level_weights=None, kind='l2', mask=None):
    """Coarse-to-fine photometric loss of a flow field [N,H,W,2] (mv3d_multiscale_warp_loss; metrics.multiscale_warp_loss_host
    states the definition): sum over the levels l = 1..levels of level_weights[l-1] times the euclidean_loss ('l2') or l1_loss
    ('l1') between the 2^l-times pooled src_img, warped by the pooled and rescaled flow, and the pooled target.  level_weights: a
    list of `levels` finite weights (default: all 1).  The flow must be differentiated (it is usually an intermediate tensor: its
    gradient from the sampler and this term's are added); the images must not be.  Every side of src_img [N,Hs,Ws,C] and target
    [N,H,W,C], C <= 4, must be a multiple of 2^levels.  Masked and scaled operands are not supported.  mask (optional): a graph
    tensor [N,H,W,1] over the flow's grid that is not differentiated, usually occlusion_mask(flow); it is pooled like the images,
    every coarse pixel is weighed by its pooled mask and the means keep their counts (mv3d_multiscale_warp_loss_masked;
    metrics.multiscale_warp_loss_host states the definition)."""
    from .metrics import _multiscale_scalars, _multiscale_shapes
    for v in (flow, src_img, target):
        if isinstance(v, (_Masked, _Scaled)):
            raise NotImplementedError("multiscale_photometric_loss of a masked or scaled operand")
    if kind not in ('l1', 'l2'):
        raise ValueError("multiscale_photometric_loss: kind must be 'l2' or 'l1', got %r" % (kind,))
    levels, weights, _ = _multiscale_scalars(levels, level_weights, 2)
    for v, what in ((flow, 'flow'), (src_img, 'src_img'), (target, 'target')):
        if not isinstance(v, Tensor) or len(v.shape) != 4:
            raise ValueError("multiscale_photometric_loss: %s must be a tensor [N,H,W,C], got %s" % (what, getattr(v, 'shape', v)))
        _check_usable(v)
    _multiscale_shapes(src_img.shape, flow.shape, target.shape, levels)
    if not flow.requires_grad:
        raise ValueError("multiscale_photometric_loss: the flow is not differentiated (nothing to learn)")
    if src_img.requires_grad or target.requires_grad:
        raise NotImplementedError("multiscale_photometric_loss: the images are not differentiated; they must not require a gradient")
    mask = _image_mask('multiscale_photometric_loss', mask, flow)
    return ScalarExpr([(1.0, MultiscaleTerm(flow, target, src_img, levels, weights, LOSS_L2 if kind == 'l2' else LOSS_L1, mask))])


def flow_consistency_loss(flow, eps=1e-3):
    """Forward-backward consistency of a flow field [N,H,W,2] over a pair-swapped batch (mv3d_flow_consistency;
    metrics.flow_consistency_host states the definition): sample n + N/2 is sample n read backwards (pair_swap.py), and following
    the flow of n and then the partner's flow there should lead back to the start; the mean Charbonnier penalty
    sqrt(|r|^2 + eps^2) - eps of that residual over the pixels that stay inside the image.  N must be even and the field square.
    The flow must be differentiated (it is usually an intermediate tensor: its gradient from the consumer and this term's are
    added).  Masked and scaled operands are not supported."""
    from .metrics import _consist_scalars, _consist_shape
    _check_flow('flow_consistency_loss', flow)
    _consist_shape(flow.shape)
    if not flow.requires_grad:
        raise ValueError("flow_consistency_loss: the flow is not differentiated (nothing to regularise)")
    eps, _ = _consist_scalars(float(eps), 1.0)
    return ScalarExpr([(1.0, ConsistTerm(flow, eps))])


def occlusion_mask(flow, alpha1=0.01, alpha2=0.5, outside_visible=True):
    """The occlusion mask [B,H,W,1] of a flow field [B,H,W,2] over a pair-swapped batch (mv3d_flow_occlusion_mask;
    metrics.flow_occlusion_mask_host states the definition): 1 where following the flow of sample n and then the partner's flow
    there leads back to the start within |r|^2 < alpha1 (|f|^2 + |s|^2) + alpha2 (UnFlow's forward-backward test), 0 where it does
    not, and outside_visible where the flow leaves the image and the test cannot be made.  The mask is a constant of the step
    (requires_grad is False): use it as masked_euclidean_loss(gen, target, mask) or multiply(x, mask).  B must be even and the
    field square."""
    from .metrics import _consist_shape, _occlusion_scalars
    _check_flow('occlusion_mask', flow)
    _consist_shape(flow.shape)
    alpha1, alpha2, outside_visible = _occlusion_scalars(alpha1, alpha2, outside_visible)
    g = current_graph()
    mask = g.new_tensor(tuple(flow.shape[:3]) + (1,), requires_grad=False, name='occlusion_mask')
    mask.producer = g.add(OcclusionMaskNode(flow, mask, alpha1, alpha2, outside_visible))
    return mask


# ------------------------------------------------------------------------------------------------ activations
def _activation(x, act, leak=0.2):
    g = current_graph()
    _check_usable(x)
    p = x.producer
    if isinstance(p, (ConvNode, LinearNode)) and p.y is x and p.act == ACT_NONE and x.grad_consumers == 0:
        p.act, p.leak = act, leak
        y = g.new_tensor(x.shape, storage=x.storage, ch_off=x.ch_off, producer=p, act=act, leak=leak,
                         requires_grad=x.requires_grad)
        p.y = y
        x.fused_into = p
        return y
    y = g.new_tensor(x.shape, act=act, leak=leak, requires_grad=x.requires_grad)
    x.grad_consumers += 1
    y.producer = g.add(ActNode(x, y, act, leak))
    return y


def relu(x, name="relu"):
    """tf_utils.py:25-27: 0.5*x + 0.5*abs(x)."""
    return _activation(x, ACT_RELU)


def lrelu(x, leak=0.2, name="lrelu"):
    """tf_utils.py:29-33: f1*x + f2*abs(x), f1 = 0.5(1+leak), f2 = 0.5(1-leak)."""
    return _activation(x, ACT_LRELU, leak)


def tanh(x):
    """tf.nn.tanh (main_model.py:79)."""
    return _activation(x, ACT_TANH)


# ------------------------------------------------------------------------------------------------ warp / resample
def coords(h, w, batch_size):
    """tf_utils.py:44-52.  The grid is generated inside the resampler kernels: channel 0 = row
    index, channel 1 = column index; returned here as a description."""
    return ('coords', int(h), int(w), int(batch_size))


class _WarpPts(Tensor):
    pass


def warp_pts_layer(flow_field, name="warp_pts"):
    """tf_utils.py:35-38: flow_field + coords(...).  Materialised by resample_layer's kernel."""
    g = current_graph()
    _check_usable(flow_field)
    w = _WarpPts(g, flow_field.shape, requires_grad=False, name=name)
    w.flow = flow_field
    g.tensors.append(w)
    return w


def resample_layer(src_img, warp_pts, name="tgt_img"):
    """tf_utils.py:40-42: tf.contrib.resampler.resampler(src_img, warp_pts).

    The output of warp_pts_layer over a dense source goes through the fused warp + resampler kernels (ResampleNode; with
    a source that needs a gradient the reverse pass adds the data gradient).  Any other warp tensor [N, ..., 2] -- a
    placeholder, a layer's output, a channel slice -- takes the plain resampler (ResamplerNode), whose source may be a
    channel slice too."""
    g = current_graph()
    _check_usable(src_img)
    if len(src_img.shape) != 4:
        raise ValueError("resampler: the source must be [N,H,W,C], got %s" % (src_img.shape,))
    if isinstance(warp_pts, _WarpPts):
        flow = warp_pts.flow
        if src_img.ld != src_img.C:
            raise NotImplementedError("warp_pts_layer over a channel-sliced source")
        n, h, w, _ = flow.shape
        if n != src_img.shape[0]:
            raise ValueError("resampler: batch of the warp (%d) and of the source (%d) differ" % (n, src_img.shape[0]))
        gen = g.new_tensor((n, h, w, src_img.C), requires_grad=flow.requires_grad or src_img.requires_grad, name=name)
        flow.grad_consumers += 1
        if src_img.requires_grad:
            src_img.grad_consumers += 1
        gen.producer = g.add(ResampleNode(src_img, flow, warp_pts, gen))
        return gen
    _check_usable(warp_pts)
    if len(warp_pts.shape) < 2 or warp_pts.shape[-1] != 2:
        raise ValueError("resampler: the warp must be [N, ..., 2], got %s" % (warp_pts.shape,))
    if warp_pts.shape[0] != src_img.shape[0]:
        raise ValueError("resampler: batch of the warp (%d) and of the source (%d) differ" % (warp_pts.shape[0], src_img.shape[0]))
    out = g.new_tensor(warp_pts.shape[:-1] + (src_img.C,), requires_grad=warp_pts.requires_grad or src_img.requires_grad,
                       name=name)
    warp_pts.grad_consumers += 1
    src_img.grad_consumers += 1
    out.producer = g.add(ResamplerNode(src_img, warp_pts, out))
    return out


def resampler(data, warp, name="resampler"):
    """tf.contrib.resampler.resampler(data, warp): the same op as resample_layer."""
    return resample_layer(data, warp, name=name)


# ------------------------------------------------------------------------------------------------ layers
def linear_msra(input_, output_size, name):
    """tf_utils.py:54-67: Matrix ~ N(0, sqrt(2/fan_in)), b = 0; matmul + b."""
    g = current_graph()
    _check_usable(input_)
    fan_in = int(input_.get_shape()[-1])
    stddev = 1.0 * math.sqrt(2. / float(fan_in))
    with variable_scope(name):
        matrix = g.variable("Matrix", [fan_in, output_size], random_normal_init(stddev))
        b = g.variable("b", [output_size], zeros_init())
    y = g.new_tensor((input_.shape[0], output_size), requires_grad=True)
    input_.grad_consumers += 1
    y.producer = g.add(LinearNode(input_, y, matrix, b))
    return y


def conv2d_msra(input_, output_dim, k_h, k_w, d_h, d_w, name):
    """tf_utils.py:70-84: w ~ truncated N(0, sqrt(2/(k_h*k_w*Cin))), b = 0; SAME conv + b."""
    g = current_graph()
    _check_usable(input_)
    n, h, w, cin = input_.shape
    stddev = 1.0 * math.sqrt(2. / float(k_h * k_w * cin))
    with variable_scope(name):
        wv = g.variable('w', [k_h, k_w, cin, output_dim], truncated_normal_init(stddev))
        b = g.variable('b', [output_dim], zeros_init())
    y = g.new_tensor((n, _same_out(h, d_h), _same_out(w, d_w), output_dim), requires_grad=True)
    input_.grad_consumers += 1
    y.producer = g.add(ConvNode(input_, y, wv, b, k_h, k_w, d_h, d_w, transposed=False))
    return y


def deconv2d_msra(input_, output_shape, k_h, k_w, d_h, d_w, name):
    """tf_utils.py:87-98: w[k_h,k_w,Cout,Cin] ~ N(0, sqrt(2/(k_h*k_w*Cin)*d_h*d_w)), no bias;
    conv2d_transpose with default SAME padding."""
    g = current_graph()
    _check_usable(input_)
    n, h, w, cin = input_.shape
    out = tuple(int(s) for s in output_shape)
    if out[0] != n or _same_out(out[1], d_h) != h or _same_out(out[2], d_w) != w:
        raise ValueError("output_shape %s inconsistent with input %s and stride (%d,%d)" % (out, input_.shape, d_h, d_w))
    stddev = 1.0 * math.sqrt(2.0 / float(k_h * k_w * cin) * float(d_h) * float(d_w))
    with variable_scope(name):
        wv = g.variable('w', [k_h, k_w, out[-1], cin], random_normal_init(stddev))
    y = g.new_tensor(out, requires_grad=True)
    input_.grad_consumers += 1
    y.producer = g.add(ConvNode(input_, y, wv, None, k_h, k_w, d_h, d_w, transposed=True))
    return y


# ------------------------------------------------------------------------------------------------ glue
def _common_act(ts):
    acts = {(t.act, t.leak) for t in ts}
    return acts.pop() if len(acts) == 1 else (ACT_NONE, 0.2)


def concat(values=None, axis=None):
    """tf.concat(axis=..., values=[...]) on the channel (last) axis.  Inputs that own their storage are adopted as channel
    slices of one wider buffer, so their producers write straight into it (no copy)."""
    g = current_graph()
    values = list(values)
    for t in values:
        _check_usable(t)
    nd = len(values[0].shape)
    if axis not in (nd - 1, -1):
        raise NotImplementedError("concat on a non-channel axis")
    rows = values[0].rows
    total = sum(t.C for t in values)
    shape = values[0].shape[:-1] + (total,)
    rg = any(t.requires_grad for t in values)
    act, leak = _common_act(values)
    adoptable = all(t.storage.can_be_adopted() and t.ch_off == 0 and t.C == t.storage.ch and t.rows == rows
                    for t in values) and len({id(t.storage) for t in values}) == len(values)
    if adoptable:
        st = Storage(rows, total)
        off = 0
        for t in values:
            t.storage.parent, t.storage.ch_off = st, off
            if t.storage.needs_grad:
                st.needs_grad = True
            off += t.C
        out = g.new_tensor(shape, storage=st, act=act, leak=leak, requires_grad=rg)
        out.producer = g.add(ViewNode(values, [out]))
    else:
        out = g.new_tensor(shape, act=act, leak=leak, requires_grad=rg)
        out.producer = g.add(CopyConcatNode(values, out))
    for t in values:
        t.grad_consumers += 1
    return out


def split(value, num_or_size_splits, axis):
    """tf.split into channel slices (views): a count (equal slices) or a list of sizes -- the latter also stands in for
    the tf.slice pairs of mv3d/nobg_dm.py:85-89 (colour = channels 0..2, depth / mask = channel 3)."""
    g = current_graph()
    _check_usable(value)
    if axis not in (len(value.shape) - 1, -1):
        raise NotImplementedError("split on a non-channel axis")
    if isinstance(num_or_size_splits, (list, tuple)):
        sizes = [int(c) for c in num_or_size_splits]
        if sum(sizes) != value.C or min(sizes) < 1:
            raise ValueError("split sizes %s do not add up to %d channels" % (sizes, value.C))
    else:
        num = int(num_or_size_splits)
        if num < 1 or value.C % num:
            raise ValueError("channels not divisible")
        sizes = [value.C // num] * num
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    outs = [g.new_tensor(value.shape[:-1] + (c,), storage=value.storage, ch_off=value.ch_off + o, act=value.act,
                         leak=value.leak, requires_grad=value.requires_grad) for c, o in zip(sizes, offs)]
    node = g.add(ViewNode([value], list(outs)))
    for o in outs:
        o.producer = node
    value.grad_consumers += 1
    return outs


def reshape(tensor, shape):
    """tf.reshape between [B,h,w,c] and [B,h*w*c] (NHWC flatten order h,w,c)."""
    g = current_graph()
    _check_usable(tensor)
    shape = tuple(int(s) for s in shape)
    st = tensor.storage
    dense = st.parent is None and tensor.ch_off == 0 and tensor.C == st.ch
    if not dense:
        raise NotImplementedError("reshape of a channel-sliced tensor")
    base = st.alias_of if st.alias_of is not None else st
    rows = 1
    for s in shape[:-1]:
        rows *= s
    if rows * shape[-1] != tensor.rows * tensor.C:
        raise ValueError("reshape size mismatch")
    alias = Storage(rows, shape[-1], alias_of=base)
    alias.external = base.external
    if st.needs_grad:
        alias.needs_grad = True
    out = g.new_tensor(shape, storage=alias, act=tensor.act, leak=tensor.leak, requires_grad=tensor.requires_grad)
    out.producer = g.add(ViewNode([tensor], [out]))
    tensor.grad_consumers += 1
    return out


def tile_spatial(code, h, w):
    """reshape [B,C] -> [B,1,1,C] + tf.tile over [1,h,w,1] (multiobject_appflow.py:148-149)."""
    g = current_graph()
    _check_usable(code)
    b, c = code.shape
    out = g.new_tensor((b, h, w, c), act=code.act, leak=code.leak, requires_grad=code.requires_grad)
    code.grad_consumers += 1
    out.producer = g.add(TileNode(code, out, h * w))
    return out


# ---------------------------------------------------------------------------- snapshots (mv3d/utils/tf_utils.py:199-212)
def save_snapshot(saver, session, path, step):
    """saver.save(session, path/snapshot<step>, global_step=step): files `snapshot<step>-<step>.index|.data-*`."""
    import os
    return saver.save(session, os.path.join(path, "snapshot" + str(step)), global_step=step)


def load_snapshot(saver, session, path):
    """Restore the checkpoint the `checkpoint` state file of `path` names; returns its iteration (the digits after
    the last '-'), or None when the directory holds no checkpoint state."""
    import re
    from . import tf_checkpoint
    ckpt = tf_checkpoint.get_checkpoint_state(path)
    if ckpt is None:
        return None
    print("loading " + ckpt['model_checkpoint_path'] + "...")
    saver.restore(session, ckpt['model_checkpoint_path'])
    num_iter = int(re.match(r'.*-(\d*)$', ckpt['model_checkpoint_path']).group(1))
    print("done.")
    return num_iter


from .visualize import save_images, rescale_image, rescale_dm      # noqa: E402,F401  (tf_utils.py:101-147)
from .summary import log_value                                     # noqa: E402,F401  (tf_utils.py:11-15)
