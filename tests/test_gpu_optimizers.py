"""GradientDescentOptimizer / MomentumOptimizer on the MI355X: the element-wise step, the fused fc filter gradient and the gradient
finalisation held bit-exact to the numpy rule (tests/test_optimizers_host.py) and to the unfused calls they replace; the model's
fused, pipelined and unfused schedules bit-identical; train.py saves and resumes the Momentum slot."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib
from tests import layer_cases as LC
from tests.gpu_utils import dev, host, stream, Ws, conv_ws
from tests.test_optimizers_host import sgd_rule

pytestmark = pytest.mark.gpu

RULES = [('gd', None, False), ('momentum', 0.9, False), ('nesterov', 0.9, True)]       # name, momentum (None: no slot), nesterov


def L():
    return _lib.lib()


def _state(lr, mu, nesterov, gscale):
    return np.array([lr, mu or 0.0, 1.0 if nesterov else 0.0, 0, 0, 0, gscale, 0], np.float32)


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
def test_sgd_step_bit_exact_vs_numpy(rule):
    """mv3d_sgd_step (with a scalar tail) and mv3d_sgd_step_dev (skipped ranges left untouched) against the numpy rule, bit for
    bit, with a gradient scale that is not 1, over three steps."""
    name, mu, nest = rule
    rng = np.random.default_rng(2)
    lr, gscale = np.float32(3e-2), np.float32(1.0 / 3.0)
    for count in (4099, (1 << 20) + 2):
        p = rng.standard_normal(count).astype(np.float32)
        a = rng.standard_normal(count).astype(np.float32) if mu is not None else None
        dp, da = dev(p), (dev(a) if a is not None else None)
        for step in range(3):
            g = (rng.standard_normal(count) * 10.0 ** rng.integers(-4, 1)).astype(np.float32)
            dg = dev(g)
            L().sgd_step(count, dp.data_ptr(), dg.data_ptr(), da.data_ptr() if da is not None else None, lr, mu or 0.0, int(nest),
                         gscale, stream())
            p, a = sgd_rule(p, g, a, lr, mu or 0.0, nest, gscale)
            np.testing.assert_array_equal(host(dp), p)
            if a is not None:
                np.testing.assert_array_equal(host(da), a)
    # _dev: scalars from the state, three skipped ranges
    count = 1 << 16
    p = rng.standard_normal(count).astype(np.float32)
    a = rng.standard_normal(count).astype(np.float32) if mu is not None else None
    dp, da = dev(p), (dev(a) if a is not None else None)
    st = dev(_state(lr, mu, nest, gscale))
    skips = [(0, 64), (1000, 4096), (60000, 65536)]
    lo, hi = (C.c_int64 * 3)(*[s for s, _ in skips]), (C.c_int64 * 3)(*[e for _, e in skips])
    keep = np.ones(count, bool)
    for s, e in skips:
        keep[s:e] = False
    for step in range(2):
        g = rng.standard_normal(count).astype(np.float32)
        L().sgd_step_dev(count, dp.data_ptr(), dev(g).data_ptr(), da.data_ptr() if da is not None else None, st.data_ptr(), 3, lo, hi,
                         stream())
        pn, an = sgd_rule(p, g, a, lr, mu or 0.0, nest, gscale)
        p = np.where(keep, pn, p)
        a = np.where(keep, an, a) if a is not None else None
        np.testing.assert_array_equal(host(dp), p)
        if a is not None:
            np.testing.assert_array_equal(host(da), a)


def _wide(rng, shape, ld):
    full = np.zeros((shape[0], ld), np.float32)
    full[:, :shape[1]] = rng.standard_normal(shape).astype(np.float32)
    return full


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
@pytest.mark.parametrize("case", [c for c in LC.FC_B64 if c[0] == 64 and min(c[1], c[2]) >= 4096], ids=LC.case_id)
def test_fused_fc_wgrad_sgd_equals_wgrad_then_sgd_step(case, rule):
    """mv3d_fc_wgrad_sgd at the benchmarked fc shapes against mv3d_fc_wgrad followed by mv3d_sgd_step_dev: matrix, slot and bias
    gradient bit-identical after two steps."""
    B, fin, fout, x_ld, y_ld = case
    name, mu, nest = rule
    assert L().fc_wgrad_adam_supported(B, fin, fout, x_ld, y_ld)
    rng = np.random.default_rng(1)
    ws = Ws(int(L().fc_workspace_bytes(B, fin, fout)))
    p0 = (rng.standard_normal((fin, fout)) / np.sqrt(fin)).astype(np.float32)
    st = dev(_state(1e-2, mu, nest, 0.5))
    pa, pb = dev(p0), dev(p0)
    aa = torch.zeros(fin, fout, device='cuda') if mu is not None else None
    ab = torch.zeros(fin, fout, device='cuda') if mu is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    for step in range(2):
        dxb, ddy = dev(_wide(rng, (B, fin), x_ld)), dev(_wide(rng, (B, fout), y_ld) * np.float32(10.0 ** rng.integers(-3, 1)))
        gm = torch.empty(fin, fout, device='cuda')
        gb_a, gb_b = torch.empty(fout, device='cuda'), torch.empty(fout, device='cuda')
        L().fc_wgrad(B, fin, fout, dxb.data_ptr(), x_ld, ddy.data_ptr(), y_ld, gm.data_ptr(), gb_a.data_ptr(), ws.ptr, ws.bytes, stream())
        L().sgd_step_dev(fin * fout, pa.data_ptr(), gm.data_ptr(), ptr(aa), st.data_ptr(), 0, None, None, stream())
        L().fc_wgrad_sgd(B, fin, fout, dxb.data_ptr(), x_ld, ddy.data_ptr(), y_ld, pb.data_ptr(), ptr(ab), gb_b.data_ptr(),
                         st.data_ptr(), stream())
        np.testing.assert_array_equal(host(gb_a), host(gb_b))
        np.testing.assert_array_equal(host(pa), host(pb))
        if aa is not None:
            np.testing.assert_array_equal(host(aa), host(ab))
    assert np.abs(host(pb) - p0).max() > 0


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
def test_grad_finalize_sgd_equals_per_layer_reduction_and_sgd_step(rule):
    """mv3d_grad_finalize_commit_sgd: three filter gradients with slabs and one already-final range finished by ONE launch,
    bit-identical to the per-layer reductions followed by mv3d_sgd_step_dev over the flat buffer (parameters and slot)."""
    name, mu, nest = rule
    rng = np.random.default_rng(11)
    lib = L()
    cases = [(LC.CONV, 8, 32, 32, 32, 64, 5, 1), (LC.DECONV, 8, 16, 16, 64, 128, 3, 2), (LC.CONV, 8, 64, 64, 3, 32, 5, 2)]
    layers, off = [], 0
    for kind, n, h, w, c, k, ksz, s in cases:
        g = _lib.conv_geom(n, h, w, c, k, ksz, ksz, s, s)
        lay = dict(kind=kind, g=g, img=dev(rng.standard_normal((n, h, w, c)).astype(np.float32)),
                   feat=dev(rng.standard_normal((n, g.Ho, g.Wo, k)).astype(np.float32)), w_off=off)
        off += -(-(ksz * ksz * c * k) // 64) * 64
        if kind == LC.CONV:
            lay['b_off'] = off
            off += -(-k // 64) * 64
        layers.append(lay)
    plain_off, plain_n = off, 192
    flat = off + 256

    def wgrads(grads, ws_of):
        for i, lay in enumerate(layers):
            ws, wsb = ws_of(i)
            gw = grads.data_ptr() + 4 * lay['w_off']
            if lay['kind'] == LC.CONV:
                lib.conv2d_wgrad(C.byref(lay['g']), lay['img'].data_ptr(), lay['feat'].data_ptr(), gw, grads.data_ptr() + 4 * lay['b_off'],
                                 ws, wsb, stream())
            else:
                lib.deconv2d_wgrad(C.byref(lay['g']), lay['feat'].data_ptr(), lay['img'].data_ptr(), gw, ws, wsb, stream())

    plain = rng.standard_normal(plain_n).astype(np.float32)
    ref = torch.zeros(flat, device='cuda')
    ref[plain_off:plain_off + plain_n] = dev(plain)
    shared = [conv_ws(lay['g']) for lay in layers]
    wgrads(ref, lambda i: (shared[i].ptr, shared[i].bytes))
    own = [Ws(max(int(lib.conv_wgrad_workspace_bytes(C.byref(lay['g']))), 16)) for lay in layers]
    assert sum(int(lib.conv_wgrad_workspace_bytes(C.byref(lay['g']))) > 0 for lay in layers) >= 2
    st = dev(_state(1e-3, mu, nest, 0.25))
    p0 = rng.standard_normal(flat).astype(np.float32)
    pa, pb = dev(p0), dev(p0)
    aa = torch.zeros(flat, device='cuda') if mu is not None else None
    ab = torch.zeros(flat, device='cuda') if mu is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    for step in range(2):
        lib.sgd_step_dev(flat, pa.data_ptr(), ref.data_ptr(), ptr(aa), st.data_ptr(), 0, None, None, stream())
        gbuf = torch.zeros(flat, device='cuda')
        gbuf[plain_off:plain_off + plain_n] = dev(plain)
        lib.grad_finalize_begin()
        wgrads(gbuf, lambda i: (own[i].ptr, own[i].bytes))
        lib.grad_finalize_add(gbuf.data_ptr() + 4 * plain_off, plain_n)
        tb = int(lib.grad_finalize_table_bytes())
        table = torch.empty(tb, dtype=torch.uint8, device='cuda')
        lib.grad_finalize_commit_sgd(table.data_ptr(), tb, gbuf.data_ptr(), pb.data_ptr(), ptr(ab), st.data_ptr(), stream())
        torch.cuda.synchronize()
    np.testing.assert_array_equal(host(pa), host(pb))
    if aa is not None:
        np.testing.assert_array_equal(host(aa), host(ab))
    assert np.abs(host(pb) - p0).max() > 0


def _model(monkeypatch, nesterov, **env):
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    for k in ('MV3D_FUSE_FC_ADAM', 'MV3D_PIPELINE_FCADAM'):
        monkeypatch.setenv(k, env.get(k, '1'))
    conf = {'batch_size': 64, 'learning_rate': 1e-3, 'optimizer': 'momentum', 'momentum': 0.9, 'use_nesterov': nesterov}
    return AppearanceFlowModel(conf, load_tfrec=False, build_loss=True, device='cuda')


@pytest.mark.parametrize("nesterov", [False, True])
def test_momentum_model_schedules_agree_bit_for_bit(monkeypatch, nesterov):
    """AppearanceFlowModel at batch 64 with Momentum, three steps on alternating feeds: the fused single-GPU step (pipelined fc
    optimiser), the same with every stream joined at the end of the step, and the unfused step (plain reverse pass + bucketed
    mv3d_sgd_step_dev) leave bit-identical losses, weights and accumulators; and the unfused optimiser equals the numpy rule on
    run_backward()'s gradients."""
    from tests.synth import appflow_feeds
    rng = np.random.default_rng(4)
    feeds = [appflow_feeds(rng, 64) for _ in range(2)]
    res = {}
    for label, env in (('pipelined', {}), ('joined', {'MV3D_PIPELINE_FCADAM': '0'}), ('unfused', {'MV3D_FUSE_FC_ADAM': '0'})):
        model = _model(monkeypatch, nesterov, **env)
        g = model.graph
        assert g.accum is not None and g.adam_m is None
        assert (g.plan_bwd_fused is not None) == (label != 'unfused')
        losses = []
        for step in range(3):
            model.feed(**feeds[step % 2])
            losses.append(float(g.train_step()))
        torch.cuda.synchronize()
        g.settle()
        res[label] = (losses, g.params.cpu().numpy().copy(), g.accum.cpu().numpy().copy())
        del model, g
        torch.cuda.empty_cache()
    assert np.abs(res['pipelined'][1]).sum() > 0 and np.abs(res['pipelined'][2]).sum() > 0
    for other in ('joined', 'unfused'):
        assert res['pipelined'][0] == res[other][0], other
        np.testing.assert_array_equal(res['pipelined'][1], res[other][1])
        np.testing.assert_array_equal(res['pipelined'][2], res[other][2])
    # the unfused optimiser on the plain reverse pass's gradients, against the numpy rule
    model = _model(monkeypatch, nesterov, MV3D_FUSE_FC_ADAM='0')
    g = model.graph
    for step in range(3):
        model.feed(**feeds[step % 2])
        p, a = g.params.cpu().numpy().copy(), g.accum.cpu().numpy().copy()
        g.run_forward()
        g.run_backward()
        grads = g.grads.cpu().numpy().copy()
        g.apply_optimizer()
        pn, an = sgd_rule(p, grads, a, 1e-3, 0.9, nesterov, 1.0)
        np.testing.assert_array_equal(g.params.cpu().numpy(), pn)
        np.testing.assert_array_equal(g.accum.cpu().numpy(), an)
    np.testing.assert_array_equal(g.params.cpu().numpy(), res['unfused'][1])
    np.testing.assert_array_equal(g.accum.cpu().numpy(), res['unfused'][2])


def test_train_driver_resumes_the_momentum_slot(tmp_path):
    """train.py with conf['optimizer'] = 'momentum': three steps, the checkpoint holds <var>/Momentum and no beta powers; a resume
    from model<itr> restores the accumulators (a resume that runs no step saves them unchanged) and the continued run uses them
    (it differs from the same resume with the accumulators zeroed)."""
    from dynamic_multiview_3d_amd import train, tf_checkpoint
    out = tmp_path / 'modeldata'
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': %r,\n"
        "  'num_iterations': 2, 'batch_size': 2, 'learning_rate': 1e-3, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle,\n"
        "  'optimizer': 'momentum', 'momentum': 0.9}\n" % str(out))
    train.main(['--hyper', str(conf_py)])
    sd = tf_checkpoint.read_checkpoint(str(out / 'model'))
    assert 'a0/Matrix/Momentum' in sd and 'beta1_power' not in sd and not any(k.endswith('/Adam') for k in sd)
    assert np.abs(sd['a0/Matrix/Momentum']).sum() > 0
    for ext in ('.index', '.data-00000-of-00001'):
        os.replace(str(out / 'model') + ext, str(out / 'model2') + ext)
    zeroed = {k: (np.zeros_like(v) if k.endswith('/Momentum') else v) for k, v in sd.items()}
    tf_checkpoint.write_checkpoint(str(out / 'zero2'), zeroed)
    train.main(['--hyper', str(conf_py), '--pretrained', str(out / 'model2'), '--num_iterations', '1'])      # no step
    same = tf_checkpoint.read_checkpoint(str(out / 'model'))
    assert set(same) == set(sd) and all(np.array_equal(same[k], sd[k]) for k in sd)
    ends = {}
    for start in ('model2', 'zero2'):
        model = train.main(['--hyper', str(conf_py), '--pretrained', str(out / start), '--num_iterations', '4'])
        ends[start] = tf_checkpoint.read_checkpoint(str(out / 'model'))
        assert model.graph.optimizer == 'momentum'
    rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
    assert all(np.isfinite(r['training_loss']) for r in rows if 'training_loss' in r)
    assert not np.array_equal(ends['model2']['fc1/Matrix'], ends['zero2']['fc1/Matrix'])
    assert not np.array_equal(ends['model2']['fc1/Matrix/Momentum'], sd['fc1/Matrix/Momentum'])
