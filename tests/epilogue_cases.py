"""Shapes, diagnostics rungs and epilogues that reach every conv / deconv / fc kernel's epilogue code, shared by the CPU
label test (tests/test_epilogue_label_coverage.py) and the GPU parity test (tests/test_gpu_epilogues.py).

Every conv, deconv and fc entry point takes an mv3d_epilogue (include/mv3d_hip.h): bias, activation and leak, plus an
activation-gradient mask with its own activation, leak, saved output and stride.  Most kernels evaluate it through
common.h act_apply / act_grad_from_out; cconv, s2conv, sconv4, smallc_band and thin_head carry a hand-written copy, and
the branch-free copies of the first four cannot do tanh: eligibility guards alone keep it away from them.  The shapes
below are the smallest that still dispatch each of those kernels (the planner picks by batch x spatial size), the rungs
(mv3d_set_diagnostics) switch in the kernels behind them, and the epilogues use leaks that are neither the
field's default 0.2 nor equal to each other.

A conv shape is (kind, n, h, w, c (image side), k (feature side), ksz, stride); an fc shape is ('fc', B, in, out).
"""
import collections
import ctypes as C
import functools
import zlib

import numpy as np

from oracle import ops

CONV, DECONV, FC = 'conv', 'deconv', 'fc'
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3

S2_5 = (CONV, 2, 16, 16, 32, 32, 5, 1)           # s2conv<5x5,s1>
S2_3 = (CONV, 2, 16, 16, 64, 64, 3, 1)           # s2conv<3x3,s1>
SC_S1 = (CONV, 4, 8, 8, 128, 128, 3, 1)          # sconv<1ph> both ways
SC_E4 = (CONV, 4, 8, 8, 128, 256, 3, 2)          # sconv<1ph> forward, sconv<4ph> data gradient
S2_E2 = (CONV, 2, 32, 32, 32, 64, 5, 2)          # s2conv<5x5,s2> forward, sconv4<gmask> data gradient
SC_D4 = (DECONV, 4, 8, 8, 128, 256, 3, 2)        # sconv<4ph> forward, sconv<1ph> data gradient
S4_D2 = (DECONV, 2, 32, 32, 32, 64, 5, 2)        # sconv4 forward, s2conv<5x5,s2,gmask> data gradient
TH_E0 = (CONV, 2, 64, 64, 3, 32, 5, 2)           # smallc_band forward, thin_deconv_s2<3> data gradient
TH_FLOW = (DECONV, 2, 64, 64, 2, 32, 5, 2)       # thin_head<2> forward, smallc_band<gmask> data gradient
TH_RGB = (DECONV, 2, 64, 64, 3, 32, 5, 2)        # thin_head<3> forward, smallc_band<gmask> data gradient
RAG_C = (CONV, 1, 7, 9, 5, 20, 3, 2)             # ragged: generic igemm
RAG_D = (DECONV, 1, 6, 10, 6, 8, 5, 2)
CC_3 = (CONV, 8, 32, 32, 64, 64, 3, 1)           # cconv<3x3,128px> behind 268435456
CC_5 = (CONV, 8, 64, 64, 32, 32, 5, 1)           # cconv<5x5,128px> behind 268435456: the largest shape here
FC_SMALL = (FC, 8, 200, 96)                      # small_fc_fwd / small_fc_dgrad
FC_STREAM = (FC, 8, 512, 384)                    # fc_stream_b3 + fc_splitk_epilogue

DEFAULT_SHAPES = [S2_5, S2_3, SC_S1, SC_E4, S2_E2, SC_D4, S4_D2, TH_E0, TH_FLOW, TH_RGB, RAG_C, RAG_D]
FAST_SHAPES = [S2_5, S2_3, SC_S1, SC_E4, S2_E2, SC_D4, S4_D2, TH_E0, TH_FLOW, TH_RGB]      # s2conv, sconv, sconv4 and thin

R_DEFAULT = 0
R_S2_OFF = 268435456                 # the rungs behind s2conv: cconv, bconvu
R_EXACT = 4096                       # the exact fp32-MFMA kernels (hconv)
R_GENERIC = 4096 | 1 | 2 | 16 | 64   # generic implicit GEMM and generic fc
R_SPLITK = 16777216                  # the kernels sconv replaced: split-K bconvu, phase-split bconv
R_HEAD_OFF = 536870912               # thin_deconv_s2 as the forward of a head
R_BAND_OFF = 33554432 | 67108864     # smallc_img2feat

# (shape, rung): one parity case each
CASES = ([(s, R_DEFAULT) for s in DEFAULT_SHAPES]
         + [(CC_3, R_S2_OFF), (CC_5, R_S2_OFF), (S2_5, R_S2_OFF)]
         + [(s, R_EXACT) for s in FAST_SHAPES]
         + [(S2_5, R_GENERIC), (FC_SMALL, R_GENERIC)]      # bit 4 is clear: the small fc kernels still take FC_SMALL here
         + [(FC_STREAM, R_GENERIC), (FC_SMALL, R_GENERIC | 4), (FC_STREAM, R_EXACT)]      # generic fc (an igemm), fc_stream
         + [(SC_S1, R_SPLITK), (S2_E2, R_SPLITK), (S4_D2, R_SPLITK)]
         + [(TH_FLOW, R_HEAD_OFF), (TH_E0, R_BAND_OFF)]
         + [(FC_SMALL, R_DEFAULT), (FC_STREAM, R_DEFAULT)])

Epi = collections.namedtuple('Epi', 'name bias act leak gact gleak')
F1 = Epi('F1', True, ACT_RELU, 0.2, ACT_NONE, 0.2)
F2 = Epi('F2', False, ACT_LRELU, 0.1, ACT_NONE, 0.2)
F3 = Epi('F3', True, ACT_NONE, 0.1, ACT_NONE, 0.2)
F4 = Epi('F4', True, ACT_TANH, 0.2, ACT_NONE, 0.2)
G1 = Epi('G1', False, ACT_NONE, 0.2, ACT_RELU, 0.2)
G2 = Epi('G2', False, ACT_NONE, 0.1, ACT_LRELU, 0.3)        # leak != gmask_leak: a swap of the two shows
G3 = Epi('G3', False, ACT_NONE, 0.2, ACT_TANH, 0.2)
H = Epi('H', True, ACT_LRELU, 0.1, ACT_LRELU, 0.3)          # v = act(acc + b) * act'(ref) in one call
FWD_EPIS = [F1, F2, F3, F4, H]          # through the forward entry of each kind
DGRAD_EPIS = [G1, G2, G3, H]            # through the data-gradient entry
# what the suite used before: the field's default leak on both sides
F_LRELU02 = Epi('F_lrelu02', True, ACT_LRELU, 0.2, ACT_NONE, 0.2)
G_LRELU02 = Epi('G_lrelu02', False, ACT_NONE, 0.2, ACT_LRELU, 0.2)

FWD, DGRAD = 'fwd', 'dgrad'


def case_id(case):
    shape, rung = case
    return '-'.join(str(v) for v in shape) + '@%d' % rung


def mate(shape):
    """The layer whose data gradient produces a tensor of the shape `shape`'s forward produces (and the other way round): the
    same geometry of the other kind; a stride-1 convolution with as many filters as channels, and a square fc layer, are
    their own mates.  A forward's output can be the saved output of its mate's data gradient."""
    if shape[0] == FC:
        return (FC, shape[1], shape[3], shape[2])
    kind, n, h, w, c, k, ksz, s = shape
    if s == 1 and c == k:
        return shape
    return (DECONV if kind == CONV else CONV,) + tuple(shape[1:])


def produced(shape, direction):
    """(shape, channels) of the tensor the forward / data-gradient call of `shape` writes"""
    if shape[0] == FC:
        _, B, fin, fout = shape
        return (B, fout if direction == FWD else fin)
    kind, n, h, w, c, k, ksz, s = shape
    image_side = (kind == DECONV) == (direction == FWD)
    return (n, h, w, c) if image_side else (n, -(-h // s), -(-w // s), k)


def consumed(shape, direction):
    return produced(shape, DGRAD if direction == FWD else FWD)


# ---------------------------------------------------------------------------------------------------------------
# recording (CPU: nothing is launched)
def _record(L, lib_mod, call):
    plan = L.plan_create()
    L.plan_begin(plan)
    try:
        call()
    finally:
        L.plan_end()
    labels = [o[0] for o in lib_mod.plan_ops(plan)]
    L.plan_destroy(plan)
    return labels


def _epi_struct(lib_mod, e, bias_ptr, ref_ptr, ref_ld):
    return lib_mod.epilogue(bias_ptr if e.bias else None, e.act, e.leak, e.gact, e.gleak,
                            ref_ptr if e.gact != ACT_NONE else None, ref_ld if e.gact != ACT_NONE else 0)


def launch(lib_mod, shape, direction, e, src, w, dst, bias, ref, ws, wsb, stream, img_ld=None, feat_ld=None, ref_ld=None):
    """One forward / data-gradient call of `shape` with epilogue `e` on the given device (or made-up, when recording) pointers."""
    L = lib_mod.lib()
    if shape[0] == FC:
        _, B, fin, fout = shape
        x_ld, y_ld = img_ld or fin, feat_ld or fout
        if direction == FWD:
            epi = _epi_struct(lib_mod, e, bias, ref, ref_ld or y_ld)
            L.fc_fwd(B, fin, fout, src, x_ld, w, dst, y_ld, C.byref(epi), ws, wsb, stream)
        else:
            epi = _epi_struct(lib_mod, e, bias, ref, ref_ld or x_ld)
            L.fc_dgrad(B, fin, fout, src, y_ld, w, dst, x_ld, C.byref(epi), ws, wsb, stream)
        return
    kind, n, h, w_, c, k, ksz, s = shape
    g = lib_mod.conv_geom(n, h, w_, c, k, ksz, ksz, s, s, img_ld, feat_ld)
    out_is_image = (kind == DECONV) == (direction == FWD)
    epi = _epi_struct(lib_mod, e, bias, ref, ref_ld or (g.img_ld if out_is_image else g.feat_ld))
    fn = {(CONV, FWD): L.conv2d_fwd, (CONV, DGRAD): L.conv2d_dgrad,
          (DECONV, FWD): L.deconv2d_fwd, (DECONV, DGRAD): L.deconv2d_dgrad}[(kind, direction)]
    fn(C.byref(g), src, w, dst, C.byref(epi), ws, wsb, stream)


def workspace_bytes(lib_mod, shape, img_ld=None, feat_ld=None):
    L = lib_mod.lib()
    if shape[0] == FC:
        return int(L.fc_workspace_bytes(shape[1], shape[2], shape[3]))
    kind, n, h, w_, c, k, ksz, s = shape
    g = lib_mod.conv_geom(n, h, w_, c, k, ksz, ksz, s, s, img_ld, feat_ld)
    return int(L.conv_workspace_bytes(C.byref(g)))


def record_case(lib_mod, case, fwd_epi=F1, dgrad_epi=G1):
    """Kernel labels of the forward call under fwd_epi and the data-gradient call under dgrad_epi of one (shape, rung):
    {'fwd': [...], 'dgrad': [...], 'calls': [[...], [...]]}.  Recorded in a plan on made-up pointers; works without a GPU."""
    shape, rung = case
    L = lib_mod.lib()
    X, W, Y, B, R, ws = 0x10000000, 0x20000000, 0x30000000, 0x50000000, 0x60000000, 0x40000000
    old = L.set_diagnostics(rung)
    try:
        wsb = workspace_bytes(lib_mod, shape)
        out = {}
        for direction, e in ((FWD, fwd_epi), (DGRAD, dgrad_epi)):
            out[direction] = _record(L, lib_mod, lambda: launch(lib_mod, shape, direction, e, X, W, Y, B, R, ws, wsb, None))
    finally:
        L.set_diagnostics(old)
    out['calls'] = [out[FWD], out[DGRAD]]
    return out


# ---------------------------------------------------------------------------------------------------------------
# data and float64 oracle of one shape (numpy only), computed once and shared
Data = collections.namedtuple('Data', 'x w dy bias_fwd bias_dgrad lin_fwd lin_dgrad')


def _per_image(fn, a):
    return np.concatenate([fn(a[i:i + 1]) for i in range(a.shape[0])], axis=0)


@functools.lru_cache(maxsize=None)
def case_data(shape, seed=0):
    """Inputs of the forward (x) and the data gradient (dy) of one shape, the filter, one bias per direction, and the float64
    results BEFORE the epilogue.  x ~ N(0, 1) and the filter ~ N(0, 1 / fan-in): a unit-variance pre-activation plus an
    N(0, 1) bias.  The arrays are shared between tests: read-only."""
    rng = np.random.default_rng([zlib.crc32(repr(shape).encode()), seed])
    f32 = np.float32
    if shape[0] == FC:
        _, B, fin, fout = shape
        x = rng.standard_normal((B, fin)).astype(f32)
        w = (rng.standard_normal((fin, fout)) / np.sqrt(fin)).astype(f32)
        dy = rng.standard_normal((B, fout)).astype(f32)
        lin_fwd = x.astype(np.float64) @ w.astype(np.float64)
        lin_dgrad = dy.astype(np.float64) @ w.astype(np.float64).T
    else:
        kind, n, h, w_, c, k, ksz, s = shape
        x = rng.standard_normal(consumed(shape, FWD)).astype(f32)
        dy = rng.standard_normal(produced(shape, FWD)).astype(f32)
        w64 = rng.standard_normal((ksz, ksz, c, k)) / np.sqrt(ksz * ksz * (c if kind == CONV else k))
        w = w64.astype(f32)
        w64 = w.astype(np.float64)
        conv = lambda a: ops.conv2d_fwd(a.astype(np.float64), w64, None, s, s)                       # image -> feature
        tconv = lambda a: ops.deconv2d_fwd(a.astype(np.float64), w64, (h, w_), s, s)                 # feature -> image
        lin_fwd = _per_image(conv if kind == CONV else tconv, x)
        lin_dgrad = _per_image(tconv if kind == CONV else conv, dy)
    d = Data(x, w, dy, rng.standard_normal(lin_fwd.shape[-1]).astype(f32), rng.standard_normal(lin_dgrad.shape[-1]).astype(f32),
             lin_fwd, lin_dgrad)
    for a in d:
        a.setflags(write=False)
    return d


def pre_activation(shape, direction, e, seed=0):
    """float64 acc + bias of one call"""
    d = case_data(shape, seed)
    lin = d.lin_fwd if direction == FWD else d.lin_dgrad
    return lin + (d.bias_fwd if direction == FWD else d.bias_dgrad).astype(np.float64) if e.bias else lin


def act_ref(pre, act, leak):
    if act == ACT_LRELU:
        return ops.absact_fwd(pre, 'lrelu', leak)
    if act == ACT_RELU:
        return ops.absact_fwd(pre, 'relu')
    return np.tanh(pre) if act == ACT_TANH else pre


def saved_output(shape_out, gact, rng):
    """A saved output for the mask `gact` (float32) and its float64 slope.
    RELU: what a relu forward writes and nothing else -- positives, -0.0 (negative pre-activation), and exact +0.0 on
    [:, ::3, ::2] (a pre-activation of exactly 0): slopes 1, 0 and 0.5.  LRELU: positives, negatives and both zeros, which
    both give f1 (sign(0) = 0).  TANH: uniform in (-1, 1), slope 1 - y^2."""
    z = rng.standard_normal(shape_out).astype(np.float32)
    idx = (slice(None), slice(None, None, 3), slice(None, None, 2)) if len(shape_out) == 4 else (slice(None, None, 3), slice(None, None, 2))
    if gact == ACT_RELU:
        y = np.where(z > 0, z, np.float32(-0.0)).astype(np.float32)
        y[idx] = 0.0
        slope = np.where(y > 0, 1.0, np.where(np.signbit(y), 0.0, 0.5))
    elif gact == ACT_LRELU:
        y = z.copy()
        y[idx] = 0.0
        neg = (slice(None),) * (len(shape_out) - 1) + (slice(None, None, 2),)
        y[idx][neg] = -0.0
        slope = None        # needs the leak: lrelu_slope
    elif gact == ACT_TANH:
        y = rng.uniform(-1, 1, shape_out).astype(np.float32)
        slope = 1.0 - y.astype(np.float64) ** 2
    else:
        raise ValueError(gact)
    return y, slope


def lrelu_slope(y, leak):
    f1, f2 = 0.5 * (1 + leak), 0.5 * (1 - leak)
    return f1 + f2 * np.sign(y.astype(np.float64))


def relu_band(pre):
    """Elements too close to the relu kink for the sign of a float32 result to be decided: |pre| <= 1e-5 max|pre| (the band of
    tests/test_gpu_model.py); and the cap on how many a case may have.  For a unit-variance pre-activation the expected
    share is 2 * 1e-5 * max / sqrt(2 pi), about 4e-5 at max = 5."""
    band = np.abs(pre) <= 1e-5 * np.abs(pre).max()
    return band, 8 + 1e-4 * pre.size
