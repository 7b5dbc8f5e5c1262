"""CPU-side checks of the plain resampler (mv3d_resampler_*): argument validation before any launch, the workspace size, the
routing of resample_layer / resampler into the recorded plans, and shape errors.  Nothing here needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

from dynamic_multiview_3d_amd import _lib
from tests import resampler_cases as RC

E_INVAL, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
P = 0x10000          # a fake, aligned device address: every call below must fail validation before it would launch


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dynamic_multiview_3d_amd import build
        build.build()
    return _lib.lib()


def _fwd(lib, N=1, Pn=8, Hs=4, Ws=5, Cc=3, data=P, data_ld=3, warp=P, warp_ld=2, out=P, out_ld=3):
    return lib.raw_resampler_fwd(N, Pn, Hs, Ws, Cc, data, data_ld, warp, warp_ld, out, out_ld, None)


def _bwd(lib, N=1, Pn=8, Hs=4, Ws=5, Cc=3, data=P, data_ld=3, warp=P, warp_ld=2, dout=P, dout_ld=3, dwarp=P, dwarp_ld=2,
         ddata=P, ddata_ld=3, ws=None, ws_bytes=0):
    return lib.raw_resampler_bwd(N, Pn, Hs, Ws, Cc, data, data_ld, warp, warp_ld, dout, dout_ld, dwarp, dwarp_ld, ddata, ddata_ld,
                                 ws, ws_bytes, None)


def test_validation_without_device(lib):
    assert _fwd(lib, N=0) == E_INVAL and 'shape' in lib.last_error()
    assert _fwd(lib, Cc=0) == E_INVAL
    assert _fwd(lib, data_ld=2) == E_INVAL and 'stride' in lib.last_error()
    assert _fwd(lib, warp_ld=1) == E_INVAL
    assert _fwd(lib, out_ld=2) == E_INVAL
    assert _fwd(lib, data=None) == E_INVAL and 'null' in lib.last_error()
    assert _fwd(lib, out=None) == E_INVAL
    assert _fwd(lib, warp=P + 2) == E_INVAL and 'aligned' in lib.last_error()
    assert _fwd(lib, Ws=(1 << 24) + 1) == E_UNSUPPORTED
    assert _fwd(lib, N=1 << 20, Pn=1 << 20) == E_UNSUPPORTED
    assert _bwd(lib, dwarp=None, ddata=None) == E_INVAL and 'neither' in lib.last_error()
    assert _bwd(lib, dout=None) == E_INVAL
    assert _bwd(lib, dwarp_ld=1) == E_INVAL
    assert _bwd(lib, ddata_ld=2) == E_INVAL
    need = lib.resampler_bwd_workspace_bytes(1, 8, 4, 5, 3)
    assert _bwd(lib, ws=None, ws_bytes=need) == E_WORKSPACE and 'workspace' in lib.last_error()
    assert _bwd(lib, ws=P, ws_bytes=need - 1) == E_WORKSPACE
    assert _bwd(lib, dwarp=None, ws=P, ws_bytes=need - 4) == E_WORKSPACE
    assert _bwd(lib, ws=P + 8, ws_bytes=need) == E_INVAL          # the int64 accumulator is read 16 bytes at a time


def test_workspace_formula(lib):
    for (n, p, hs, ws, c) in [(1, 3150000, 1500, 2100, 3), (64, 16384, 128, 128, 3), (8, 4096, 64, 64, 32), (3, 5, 7, 9, 7)]:
        acc = -(-n * hs * ws * c * 8 // 256) * 256
        assert lib.resampler_bwd_workspace_bytes(n, p, hs, ws, c) == acc + 4096
    assert lib.resampler_bwd_workspace_bytes(0, 1, 1, 1, 1) == 0


def test_plan_records_three_launches_for_ddata(lib):
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        need = lib.resampler_bwd_workspace_bytes(2, 100, 8, 8, 32)
        lib.resampler_fwd(2, 100, 8, 8, 32, P, 32, P, 2, P, 32, None)
        lib.resampler_bwd(2, 100, 8, 8, 32, P, 32, P, 2, P, 32, P, 2, None, 32, None, 0, None)
        lib.resampler_bwd(2, 100, 8, 8, 7, P, 7, P, 2, P, 7, P, 2, P, 7, P, need, None)
    finally:
        lib.plan_end()
    ops = _lib.plan_ops(plan)
    assert [o[0] for o in ops] == ['resampler_fwd<vec4>', 'resampler_bwd<vec4,dwarp>', 'resampler_ddata_prep',
                                   'resampler_bwd<generic,dwarp+ddata>', 'resampler_ddata_final']
    assert ops[0][2] == 200 * (8 + 4 * 32) + 2 * 8 * 8 * 4 * 32          # warp + output per point, every source element once
    lib.plan_destroy(plan)


def _graph(case):
    from dynamic_multiview_3d_amd import tf_utils as tf
    from dynamic_multiview_3d_amd.graph import Graph
    with Graph(device='cpu') as g:
        t = RC.build_graph(tf, g, case)
    g.compile()
    return g, t


def _labels(plan):
    return [o[0] for o in _lib.plan_ops(plan)]


def test_any_warp_routes_to_the_plain_resampler(lib):
    from dynamic_multiview_3d_amd.graph import ResamplerNode, ResampleNode
    g, t = _graph('conv_warp')
    assert any(isinstance(n, ResamplerNode) for n in g.nodes) and not any(isinstance(n, ResampleNode) for n in g.nodes)
    assert t['gen'].shape == (RC.N, RC.H, RC.W, 3)
    fwd, bwd = _labels(g.plan_fwd), _labels(g.plan_bwd)
    assert 'resampler_fwd<C3>' in fwd and 'pixel_loss' in fwd
    assert 'resampler_bwd<C3,dwarp>' in bwd and 'resampler_ddata_prep' not in bwd       # the image needs no gradient
    assert g.ws_bytes >= 0
    g, t = _graph('conv_src')
    fwd, bwd = _labels(g.plan_fwd), _labels(g.plan_bwd)
    assert 'resampler_fwd<C4>' in fwd
    i = bwd.index('resampler_bwd<C4,ddata>')
    assert bwd[i - 1] == 'resampler_ddata_prep' and bwd[i + 1] == 'resampler_ddata_final'
    assert g.ws_bytes >= lib.resampler_bwd_workspace_bytes(RC.N, RC.H * RC.W, RC.HS, RC.WS, 4)


def test_warp_pts_over_a_differentiated_source_keeps_the_unfused_head(lib):
    from dynamic_multiview_3d_amd.graph import ResampleNode
    g, t = _graph('warp_pts_src')
    rs = [n for n in g.nodes if isinstance(n, ResampleNode)]
    assert len(rs) == 1 and rs[0].fused_loss is None
    fwd, bwd = _labels(g.plan_fwd), _labels(g.plan_bwd)
    assert 'resample_fwd' in fwd and 'pixel_loss' in fwd and 'resample_loss' not in fwd
    i = bwd.index('resample_bwd')
    assert bwd[i + 1:i + 4] == ['resampler_ddata_prep', 'resampler_bwd<C4,ddata>', 'resampler_ddata_final']
    assert not any(l.startswith('resampler_fwd') for l in fwd)


def test_appearance_flow_plans_do_not_change(lib):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    m = AppearanceFlowModel({'batch_size': 8, 'learning_rate': 1e-4}, load_tfrec=False, build_loss=True, device='cpu')
    g = m.graph
    for plan in (g.plan_fwd, g.plan_bwd, g.plan_bwd_fused):
        assert not any(l.startswith('resampler_') for l in _labels(plan))
    assert 'resample_loss' in _labels(g.plan_fwd)
    assert g.ws_bytes == max(n.workspace_bytes(g) for n in g.nodes if hasattr(n, 'workspace_bytes'))


def test_shape_errors(lib):
    from dynamic_multiview_3d_amd import tf_utils as tf
    from dynamic_multiview_3d_amd.graph import Graph
    with Graph(device='cpu') as g:
        img = g.placeholder((2, 8, 9, 3), 'img')
        for shape in [(2, 5, 3), (3, 5, 2), (2,), (2, 4, 4, 1)]:
            w = g.placeholder(shape, 'w%d' % len(g.inputs))
            with pytest.raises(ValueError):
                tf.resampler(img, w)
        flat = g.placeholder((2, 72, 3), 'flat')
        with pytest.raises(ValueError):
            tf.resample_layer(flat, g.placeholder((2, 5, 2), 'w_ok'))
        out = tf.resampler(img, g.placeholder((2, 2), 'one_point'))             # rank 2: one point per image
        assert out.shape == (2, 3)
        out = tf.resampler(img, g.placeholder((2, 3, 4, 5, 2), 'rank5'))
        assert out.shape == (2, 3, 4, 5, 3)


def test_channel_sliced_source_and_warp(lib):
    """A channel slice of a split as the source and as the warp: strides reach the kernels, gradients reach the slices."""
    from dynamic_multiview_3d_amd import tf_utils as tf
    from dynamic_multiview_3d_amd.graph import Graph, ResamplerNode
    with Graph(device='cpu') as g:
        img = g.placeholder((2, 8, 9, 3), 'img')
        feat = tf.conv2d_msra(img, 7, 3, 3, 1, 1, 'c')
        src, warp = tf.split(feat, [5, 2], 3)
        out = tf.resampler(src, warp)
        g.loss_expr = tf.euclidean_loss(out, g.placeholder((2, 8, 9, 5), 'tgt'))
        g.lr = 1e-4
    g.compile()
    node = [n for n in g.nodes if isinstance(n, ResamplerNode)][0]
    assert node.src.ld == 7 and node.warp.ld == 7 and out.shape == (2, 8, 9, 5)
    bwd = _labels(g.plan_bwd)
    assert 'resampler_bwd<generic,dwarp+ddata>' in bwd
    assert src.grad_written and warp.grad_written
