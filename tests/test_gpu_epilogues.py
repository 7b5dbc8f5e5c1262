"""Every conv / deconv / fc kernel's epilogue against the float64 oracle: relu, tanh, leaks that are not 0.2, bias on every
forward (the deconv forward too), and the activation-gradient mask with its own activation and leak.

The suite drove the epilogue through bias + lrelu 0.2 forward and an lrelu 0.2 mask with +0.0 only; a kernel that hard-codes
0.2, swaps leak and gmask_leak, drops the -0.0 marker a relu forward leaves for pre-activations below zero, or reads that
marker wrongly passed all of it.  tests/epilogue_cases.py has the shapes, rungs and epilogues (F1 - F4 forward, G1 - G3
mask, H both in one call), tests/test_epilogue_label_coverage.py proves on the CPU which kernels they run.

Bar: 2e-5 of the tensor maximum, the per-op bar of tests/test_gpu_ops.py, for the exact-fp32 rungs as well.  The relu sign
checks leave out the elements within 1e-5 max|pre| of the kink (the band of tests/test_gpu_model.py), on the condition that
they number at most 8 + 1e-4 size.  Every test prints its figures (run with -s to see them)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from tests import epilogue_cases as EC
from tests.gpu_utils import dev, host, stream, Ws, rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
SENTINEL = 7.0


def L():
    return _lib.lib()


def _embed(a, ld, fill):
    """`a` at channel 0 of a buffer with pixel stride ld, `fill` in the channels outside the slice"""
    if ld == a.shape[-1]:
        return np.array(a, dtype=np.float32)          # a copy: the shared case data is read-only
    buf = np.full(a.shape[:-1] + (ld,), fill, np.float32)
    buf[..., :a.shape[-1]] = a
    return buf


def _strides(shape, direction, wide):
    """(img_ld, feat_ld, ld of the tensor read, ld of the tensor written); an fc layer's x side counts as the image side"""
    fc = shape[0] == EC.FC
    c_img, c_feat = (shape[2], shape[3]) if fc else (shape[4], shape[5])
    img_ld, feat_ld = (c_img + 5, c_feat + 7) if wide else (c_img, c_feat)
    out_is_image = (direction == EC.DGRAD) if fc else ((shape[0] == EC.DECONV) == (direction == EC.FWD))
    return (img_ld, feat_ld) + ((feat_ld, img_ld) if out_is_image else (img_ld, feat_ld))


def run_call(shape, rung, direction, e, ref=None, wide=False):
    """One call on the device: returns (the produced slice as numpy, the produced device buffer).  `ref` is the saved output of
    the mask: a numpy array of the produced shape (embedded at the stride of the produced tensor) or a device buffer of that
    stride.  Checks that nothing outside the slice was written."""
    d = EC.case_data(shape)
    img_ld, feat_ld, in_ld, out_ld = _strides(shape, direction, wide)
    src = d.x if direction == EC.FWD else d.dy
    bias = d.bias_fwd if direction == EC.FWD else d.bias_dgrad
    out_shape = EC.produced(shape, direction)
    assert src.shape == EC.consumed(shape, direction)
    dsrc, dw, db = dev(_embed(src, in_ld, 3.0)), dev(np.array(d.w)), dev(np.array(bias))
    out = torch.full(out_shape[:-1] + (out_ld,), SENTINEL, device='cuda')
    dref = None
    if ref is not None:
        dref = ref if isinstance(ref, torch.Tensor) else dev(_embed(ref, out_ld, -3.0))
        assert tuple(dref.shape) == tuple(out.shape)
    old = L().set_diagnostics(rung)
    try:
        ws = Ws(EC.workspace_bytes(_lib, shape, img_ld, feat_ld))
        EC.launch(_lib, shape, direction, e, dsrc.data_ptr(), dw.data_ptr(), out.data_ptr(), db.data_ptr(),
                  dref.data_ptr() if dref is not None else None, ws.ptr, ws.bytes, stream(), img_ld, feat_ld, out_ld)
        got = host(out)
    finally:
        L().set_diagnostics(old)
    assert np.all(got[..., out_shape[-1]:] == SENTINEL), "wrote outside the channel slice"
    return got[..., :out_shape[-1]], out


def _mask(shape, direction, e):
    """saved output (float32) and float64 slope of epilogue e's mask for the tensor this call produces"""
    rng = np.random.default_rng([zlib.crc32(repr((shape, direction)).encode()), e.gact])
    y, slope = EC.saved_output(EC.produced(shape, direction), e.gact, rng)
    z = y == 0
    if e.gact == EC.ACT_RELU:
        assert (z & np.signbit(y)).any() and (z & ~np.signbit(y)).any() and not (y < 0).any()      # both zeros, nothing negative
    if e.gact == EC.ACT_LRELU:
        assert (z & np.signbit(y)).any() and (z & ~np.signbit(y)).any() and (y < 0).any() and (y > 0).any()
        slope = EC.lrelu_slope(y, e.gleak)
    return y, slope


def _check_relu_marker(got, pre, what):
    """relu writes -0.0 where the pre-activation is negative and a positive value where it is positive; never a negative one"""
    band, cap = EC.relu_band(pre)
    print("%s: %d elements in the relu band, cap %.1f" % (what, band.sum(), cap))
    assert band.sum() <= cap
    assert np.all(got >= 0)
    assert np.array_equal(np.signbit(got)[~band], (pre < 0)[~band])


def check_call(case, direction, e, wide=False):
    shape, rung = case
    what = "EPI %s %s %s%s" % (EC.case_id(case), direction, e.name, " wide" if wide else "")
    pre = EC.pre_activation(shape, direction, e)
    want = EC.act_ref(pre, e.act, e.leak)
    y = None
    if e.gact != EC.ACT_NONE:
        y, slope = _mask(shape, direction, e)
        want = want * slope
    got, _ = run_call(shape, rung, direction, e, ref=y, wide=wide)
    err = rel_err(got, want)
    print("%s: rel_err %.3g" % (what, err))
    assert err < TOL
    if e.act == EC.ACT_RELU and e.gact == EC.ACT_NONE:
        _check_relu_marker(got, pre, what)


CALLS = [(EC.FWD, e) for e in EC.FWD_EPIS] + [(EC.DGRAD, e) for e in EC.DGRAD_EPIS]


@pytest.mark.parametrize('direction,e', CALLS, ids=lambda v: v if isinstance(v, str) else v.name)
@pytest.mark.parametrize('case', EC.CASES, ids=EC.case_id)
def test_epilogue_matches_the_oracle(case, direction, e):
    """One (shape, rung) x one epilogue against the float64 oracle at the per-op bar.

    The tanh forward (F4) is the tight one: tanh has slope 1 at 0 and a maximum of 1, so the accumulator's absolute error
    becomes the output's error relative to 1.  On the split-bf16 kernels that error is about 3.5e-6 of max|acc + bias|;
    through bconvu the two largest shapes (conv 8,32,32,64,64,3,1 and conv 8,64,64,32,32,5,1) came to 2.02e-5 and 2.34e-5,
    which is why try_hconv (hconv.hip) sends a tanh forward to the exact-fp32 kernels (at most 3.8e-6 with tanh).
    The tanh forwards that try_hconv does not plan stay on split-bf16 kernels and are the cases nearest the bar:
    smallc_img2feat 1.85e-5, fc_stream_b3 1.41e-5, thin_head 1.15e-5; everything without tanh is below 6.5e-6."""
    check_call(case, direction, e)


@pytest.mark.parametrize('direction,e', [(EC.FWD, EC.F1), (EC.DGRAD, EC.G1)], ids=lambda v: v if isinstance(v, str) else v.name)
@pytest.mark.parametrize('case', [c for c in EC.CASES if c[1] == EC.R_DEFAULT], ids=EC.case_id)
def test_epilogue_on_channel_slices_of_wider_buffers(case, direction, e):
    """img_ld = c + 5, feat_ld = k + 7, the mask at the stride of the tensor it belongs to, 7.0 outside the written slice"""
    check_call(case, direction, e, wide=True)


# writer (forward, relu) and reader (data gradient, relu mask): every case with the reader on the same rung, and the kernels
# with a hand-written epilogue against the exact-fp32 kernels (common.h act_apply / act_grad_from_out) in both orders
ROUND_TRIPS = ([(c, c[1]) for c in EC.CASES]
               + [((s, EC.R_DEFAULT), EC.R_EXACT) for s in EC.FAST_SHAPES] + [((s, EC.R_EXACT), EC.R_DEFAULT) for s in EC.FAST_SHAPES]
               + [((s, EC.R_S2_OFF), EC.R_EXACT) for s in (EC.CC_3, EC.CC_5)] + [((s, EC.R_EXACT), EC.R_S2_OFF) for s in (EC.CC_3, EC.CC_5)])


@pytest.mark.parametrize('case,reader_rung', ROUND_TRIPS, ids=lambda v: EC.case_id(v) if isinstance(v, tuple) else 'reader@%d' % v)
def test_relu_round_trip_on_the_device(case, reader_rung):
    """Forward with relu, then the data gradient of the layer's mate (tests/epilogue_cases.py mate) masked by the forward's
    own output, still on the device: the only place where the -0.0 one kernel writes meets the sign-bit test of another.
    The oracle decides the slope from its own pre-activation; elements inside the relu band are left out."""
    shape, rung = case
    m = EC.mate(shape)
    assert EC.produced(m, EC.DGRAD) == EC.produced(shape, EC.FWD)
    pre = EC.pre_activation(shape, EC.FWD, EC.F1)
    band, cap = EC.relu_band(pre)
    assert band.sum() <= cap
    _, saved = run_call(shape, rung, EC.FWD, EC.F1)
    got, _ = run_call(m, reader_rung, EC.DGRAD, EC.G1, ref=saved)
    want = EC.case_data(m).lin_dgrad * (pre > 0)
    err = np.abs(got - want)[~band].max() / np.abs(want).max()
    print("ROUNDTRIP %s reader@%d: rel_err %.3g, %d in the band, cap %.1f" % (EC.case_id(case), reader_rung, err, band.sum(), cap))
    assert err < TOL


# ---------------------------------------------------------------------------------------------------------------
# the small-fc entries
CHAIN_ACTS = [(EC.ACT_RELU, 0.2), (EC.ACT_TANH, 0.2), (EC.ACT_LRELU, 0.1)]


@pytest.mark.parametrize('rot', [0, 1, 2])
def test_fc_chain_with_mixed_activations_equals_per_layer_calls(rot):
    """mv3d_fc_chain_fwd on 4 -> 64 -> 64 -> 19 with relu, tanh and lrelu 0.1 in every order of layers: bit-equal to three
    mv3d_fc_fwd calls, and within the per-op bar of the oracle.  13 rows: a workgroup carries four."""
    B, widths, y_lds = 13, [4, 64, 64, 19], [64, 72, 19]
    acts = CHAIN_ACTS[rot:] + CHAIN_ACTS[:rot]
    rng = np.random.default_rng(5 + rot)
    x = rng.standard_normal((B, widths[0])).astype(np.float32)
    Ms = [(rng.standard_normal((widths[k], widths[k + 1])) / np.sqrt(widths[k])).astype(np.float32) for k in range(3)]
    bs = [rng.standard_normal(widths[k + 1]).astype(np.float32) for k in range(3)]
    dx_, dMs, dbs = dev(x), [dev(m) for m in Ms], [dev(b) for b in bs]
    ws = Ws(int(L().fc_workspace_bytes(B, 64, 64)))
    ys_ref, cur, cur_ld = [], dx_, widths[0]
    for k in range(3):
        y = torch.full((B, y_lds[k]), SENTINEL, device='cuda')
        epi = _lib.epilogue(dbs[k].data_ptr(), acts[k][0], acts[k][1])
        L().fc_fwd(B, widths[k], widths[k + 1], cur.data_ptr(), cur_ld, dMs[k].data_ptr(), y.data_ptr(), y_lds[k], C.byref(epi),
                   ws.ptr, ws.bytes, stream())
        ys_ref.append(y)
        cur, cur_ld = y, y_lds[k]
    ys = [torch.full((B, y_lds[k]), SENTINEL, device='cuda') for k in range(3)]
    c = _lib.FcChain()
    c.B, c.nlayers, c.in_, c.x_ld, c.x = B, 3, widths[0], widths[0], dx_.data_ptr()
    for k in range(3):
        c.l[k].M, c.l[k].bias, c.l[k].y, c.l[k].y_ld, c.l[k].out = dMs[k].data_ptr(), dbs[k].data_ptr(), ys[k].data_ptr(), y_lds[k], widths[k + 1]
        c.l[k].act, c.l[k].leak = acts[k]
    L().fc_chain_fwd(C.byref(c), stream())
    h = x.astype(np.float64)
    for k in range(3):
        got, per_layer = host(ys[k]), host(ys_ref[k])
        assert np.array_equal(got.view(np.uint32), per_layer.view(np.uint32))          # the bits: a relu's -0.0 included
        h = EC.act_ref(h @ Ms[k].astype(np.float64) + bs[k], acts[k][0], acts[k][1])
        err = rel_err(got[:, :widths[k + 1]], h)
        print("FCCHAIN rot %d layer %d act %d: rel_err %.3g" % (rot, k, acts[k][0], err))
        assert err < TOL
        assert np.all(got[:, widths[k + 1]:] == SENTINEL)


@pytest.mark.parametrize('e', [EC.G1, EC.G2, EC.G3], ids=lambda e: e.name)
def test_fc_wgrad_dgrad_with_each_mask_equals_the_two_calls(e):
    """mv3d_fc_wgrad_dgrad on (8, 64, 64): bit-equal to mv3d_fc_wgrad followed by mv3d_fc_dgrad under a relu, lrelu 0.3 and tanh
    mask, and within the per-op bar of the oracle."""
    B, fin, fout, x_ld, dy_ld = 8, 64, 64, 72, 64
    shape = (EC.FC, B, fin, fout)
    d = EC.case_data(shape)
    saved, slope = _mask(shape, EC.DGRAD, e)               # the saved output is the layer's input x: [B, fin]
    dxb, dM, ddy = dev(_embed(saved, x_ld, -3.0)), dev(np.array(d.w)), dev(np.array(d.dy))
    ws = Ws(int(L().fc_workspace_bytes(B, fin, fout)))
    epi = _lib.epilogue(None, e.act, e.leak, e.gact, e.gleak, dxb.data_ptr(), x_ld)
    gm1, gb1, gx1 = (torch.full(sh, SENTINEL, device='cuda') for sh in ((fin, fout), (fout,), (B, x_ld)))
    gm2, gb2, gx2 = (torch.full(sh, SENTINEL, device='cuda') for sh in ((fin, fout), (fout,), (B, x_ld)))
    L().fc_wgrad(B, fin, fout, dxb.data_ptr(), x_ld, ddy.data_ptr(), dy_ld, gm1.data_ptr(), gb1.data_ptr(), ws.ptr, ws.bytes, stream())
    L().fc_dgrad(B, fin, fout, ddy.data_ptr(), dy_ld, dM.data_ptr(), gx1.data_ptr(), x_ld, C.byref(epi), ws.ptr, ws.bytes, stream())
    L().fc_wgrad_dgrad(B, fin, fout, dxb.data_ptr(), x_ld, ddy.data_ptr(), dy_ld, dM.data_ptr(), gm2.data_ptr(), gb2.data_ptr(),
                       gx2.data_ptr(), x_ld, C.byref(epi), ws.ptr, ws.bytes, stream())
    for a, b in ((gm1, gm2), (gb1, gb2), (gx1, gx2)):
        assert np.array_equal(host(a).view(np.uint32), host(b).view(np.uint32))
    got = host(gx2)
    assert np.all(got[:, fin:] == SENTINEL)
    err = rel_err(got[:, :fin], d.lin_dgrad * slope)
    x64, dy64 = saved.astype(np.float64), d.dy.astype(np.float64)
    err_w, err_b = rel_err(host(gm2), x64.T @ dy64), rel_err(host(gb2), dy64.sum(0))
    print("FCBWD %s: rel_err dx %.3g dM %.3g db %.3g" % (e.name, err, err_w, err_b))
    assert err < TOL and err_w < TOL and err_b < TOL


# ---------------------------------------------------------------------------------------------------------------
# the standalone activation kernels on the strided [rows, ch] form
@pytest.mark.parametrize('act,leak', [(EC.ACT_TANH, 0.2), (EC.ACT_LRELU, 0.1)], ids=['tanh', 'lrelu0.1'])
def test_act_fwd_bwd_tanh_and_leak_on_strided_rows(act, leak):
    """mv3d_act_fwd / mv3d_act_bwd with ch = 5, x_ld = 8, y_ld = 7 against np.tanh, 1 - y^2 and absact_*.  tanhf is good to a
    few ulp: 1e-6 absolute on values below 1, and 1 - y * y in float32 is off by up to an ulp of 1 (1.2e-7) times |dy| < 5:
    1e-6 absolute as well; lrelu is two products and a sum, its mask one product: 1e-6 relative."""
    rows, ch, x_ld, y_ld, dx_ld = 301, 5, 8, 7, 6
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((rows, ch)) * 2).astype(np.float32)
    x[::7, 0], x[1::7, 3] = 0.0, -0.0
    dy = rng.standard_normal((rows, ch)).astype(np.float32)
    dxb, ddy = dev(_embed(x, x_ld, 3.0)), dev(dy)
    y = torch.full((rows, y_ld), SENTINEL, device='cuda')
    gx = torch.full((rows, dx_ld), SENTINEL, device='cuda')
    L().act_fwd(rows, ch, dxb.data_ptr(), x_ld, y.data_ptr(), y_ld, act, leak, stream())
    L().act_bwd(rows, ch, ddy.data_ptr(), ch, y.data_ptr(), y_ld, gx.data_ptr(), dx_ld, act, leak, stream())
    yy, gg = host(y), host(gx)
    assert np.all(yy[:, ch:] == SENTINEL) and np.all(gg[:, ch:] == SENTINEL)
    x64, dy64, y64 = x.astype(np.float64), dy.astype(np.float64), yy[:, :ch].astype(np.float64)
    if act == EC.ACT_TANH:
        np.testing.assert_allclose(yy[:, :ch], np.tanh(x64), rtol=0, atol=1e-6)
        np.testing.assert_allclose(gg[:, :ch], dy64 * (1 - y64 * y64), rtol=1e-6, atol=1e-6)
    else:
        np.testing.assert_allclose(yy[:, :ch], EC.ops.absact_fwd(x64, 'lrelu', leak), rtol=1e-6, atol=0)
        np.testing.assert_allclose(gg[:, :ch], EC.ops.absact_bwd(x64, dy64, 'lrelu', leak), rtol=1e-6, atol=0)
