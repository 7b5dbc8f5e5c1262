"""mv3d_flow_occlusion_mask and mv3d_warp_resample_occlusion_loss on the GPU, through the C ABI (tests/flow_occlusion_cases.py: both
families at every shape, alphas 0.01 / 0.5).

The mask is compared at every pixel with metrics.flow_occlusion_mask_host in float64: the cases keep every inside pixel at least
1e-4 (relative) off the threshold, 12 x the float32 error measured there, so no pixel is left out.  The shares must be the exact
counts.  The fused head is compared bit for bit with the chain of separate launches it replaces (mask, mv3d_warp_resample_fwd,
mv3d_pixel_loss_strided with the mask, mv3d_warp_resample_bwd) for warp_out, gen, the mask and dflow.  Its loss may differ from
the float64 twin chain (tests/flow_occlusion_cases.head_chain_host) by at most 4 x the float32 twin chain's own deviation from it
(the rule of tests/test_gpu_flow_consist.py), and from the chain's loss, which sums in another order, by rtol 3e-6 (the bar
tests/test_gpu_ops.py uses for the unmasked head).  Every figure is printed before it is asserted.

Shapes (tiles are 32 x 32): below one tile; no multiple of 32; N/2 odd with an odd side; across a tile edge; the model's own size;
and channel-slice views with flow_ld 3 and mask_ld 4."""
import functools

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, metrics
from tests import flow_occlusion_cases as OC
from tests.gpu_utils import DEV, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
A1, A2 = OC.ALPHA1, OC.ALPHA2
WEIGHT = 0.7
HEAD = ['occl_head_tile', 'occl_head_final']


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _sent(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)               # a copy: the cases are read-only


@functools.lru_cache(maxsize=None)
def _mask_reference(family, n, h, keep):
    mask, shares = metrics.flow_occlusion_mask_host(OC.flow(family, n, h), A1, A2, keep, np.float64)
    mask.setflags(write=False)
    return mask, shares


@functools.lru_cache(maxsize=None)
def _head_reference(family, n, h, c, kind):
    """(loss in float64, loss in float32) of the twin chain, computed once."""
    src, tgt = OC.head_images(n, h, c)
    return tuple(float(OC.head_chain_host(src, OC.flow(family, n, h), tgt, kind, WEIGHT, A1, A2, True, dt)[0]) for dt in (np.float64, np.float32))


def _mask(lib, tf, keep=True, mask=None, stats=None, off=0, moff=0, ws=None):
    """One mask call on the flow view [off, off + 2) of tf [N,H,H,ld]; mask is [N,H,H,mask_ld], channel moff."""
    n, h, w, ld = tf.shape
    nb = int(lib.flow_occlusion_mask_workspace_bytes(n, h, w))
    assert nb >= 32 * n * (-(-h // 32)) ** 2
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if mask is None:
        mask = _sent(n, h, w, 1)
    lib.flow_occlusion_mask(n, h, w, tf.data_ptr() + 4 * off, ld, A1, A2, 1 if keep else 0, mask.data_ptr() + 4 * moff, mask.shape[3],
                            stats.data_ptr() if stats is not None else None, ws.data_ptr(), nb, stream())
    return mask


def _head(lib, src, tf, tgt, kind, weight=WEIGHT, keep=True, loss=None, stats=None, want_dflow=True, ws=None, warp=True, mask=True):
    """One fused call on dense operands: (loss, warp, gen, dflow, mask)."""
    n, h, w, c = src.shape
    nb = int(lib.warp_resample_occlusion_loss_workspace_bytes(n, h, w))
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if loss is None:
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    warp_t, gen, dflow, mask_t = (_sent(n, h, w, 2) if warp else None), _sent(n, h, w, c), (_sent(n, h, w, 2) if want_dflow else None), \
        (_sent(n, h, w, 1) if mask else None)
    ptr = lambda t: t.data_ptr() if t is not None else None
    lib.warp_resample_occlusion_loss(n, h, w, h, w, c, src.data_ptr(), tf.data_ptr(), 2, tgt.data_ptr(), c, kind, weight, A1, A2, 1 if keep else 0,
                                     ptr(warp_t), gen.data_ptr(), ptr(dflow), 2, ptr(mask_t), 1, loss.data_ptr(), ptr(stats), ws.data_ptr(), nb,
                                     stream())
    return loss, warp_t, gen, dflow, mask_t


def _chain(lib, src, tf, tgt, kind, weight=WEIGHT, keep=True):
    """The four separate launches the fused head replaces: (loss, warp, gen, dflow, mask)."""
    n, h, w, c = src.shape
    mask = _mask(lib, tf, keep)
    warp, gen, dgen, dflow = _sent(n, h, w, 2), _sent(n, h, w, c), _sent(n, h, w, c), _sent(n, h, w, 2)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib.warp_resample_fwd(n, h, w, h, w, c, src.data_ptr(), tf.data_ptr(), 2, warp.data_ptr(), gen.data_ptr(), stream())
    lib.pixel_loss_strided(n * h * w, c, gen.data_ptr(), c, tgt.data_ptr(), c, 1.0, mask.data_ptr(), 1, kind, weight, loss.data_ptr(),
                           dgen.data_ptr(), c, stream())
    lib.warp_resample_bwd(n, h, w, h, w, c, src.data_ptr(), tf.data_ptr(), 2, dgen.data_ptr(), dflow.data_ptr(), 2, stream())
    return loss, warp, gen, dflow, mask


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("family,n,h", OC.CASES)
def test_mask_equals_the_float64_twin_at_every_pixel_and_the_shares_are_the_exact_counts(family, n, h):
    lib = _lib.lib()
    tf = _dev(OC.flow(family, n, h))
    for keep in (True, False):
        stats = _sent(3)
        mask = _mask(lib, tf, keep, stats=stats)
        only = _mask(lib, tf, keep)                                        # without the shares: one launch, the same mask
        torch.cuda.synchronize()
        want, shares = _mask_reference(family, n, h, keep)
        got = mask.cpu().numpy()[..., 0]
        print('%s-%dx%d keep=%d: %d of %d pixels differ from the float64 twin; shares %s twin %s'
              % (family, n, h, keep, int(np.count_nonzero(got != want)), want.size, stats.cpu().numpy(), np.float32(shares)))
        assert np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(stats.cpu().numpy(), np.array(shares, np.float64).astype(np.float32))
        assert np.array_equal(_bits(mask), _bits(only))
    assert np.array_equal(tf.cpu().numpy(), OC.flow(family, n, h))


def test_channel_slice_views_leave_the_other_channels_alone_and_the_torch_mirror_agrees():
    family, n, h = 'smooth', 6, 33
    lib = _lib.lib()
    f3 = np.full((n, h, h, 3), SENTINEL, np.float32)
    f3[..., 1:3] = OC.flow(family, n, h)
    tf = _dev(f3)
    wide = _sent(n, h, h, 4)
    stats = _sent(3)
    _mask(lib, tf, True, mask=wide, stats=stats, off=1, moff=2)
    torch.cuda.synchronize()
    got = wide.cpu().numpy()
    want, shares = _mask_reference(family, n, h, True)
    assert np.all(got[..., [0, 1, 3]] == SENTINEL) and np.array_equal(tf.cpu().numpy(), f3)
    assert np.array_equal(got[..., 2].astype(np.float64), want) and np.array_equal(stats.cpu().numpy(), np.float32(shares))
    # the mirror: views in, a view out
    wide2 = _sent(n, h, h, 4)
    stats2 = torch.zeros(3, dtype=torch.float32, device=DEV)
    out = metrics.flow_occlusion_mask(tf[..., 1:3], A1, A2, True, out=wide2[..., 2:3], stats=stats2)
    assert out.shape == (n, h, h, 1) and np.array_equal(_bits(wide2), _bits(wide)) and np.array_equal(_bits(stats2), _bits(stats))
    made = metrics.flow_occlusion_mask(tf[..., 1:3], A1, A2, False)
    assert tuple(made.shape) == (n, h, h, 1) and np.array_equal(made.cpu().numpy()[..., 0].astype(np.float64), _mask_reference(family, n, h, False)[0])
    with pytest.raises(ValueError, match='out'):
        metrics.flow_occlusion_mask(tf[..., 1:3], out=wide2[:, :-1, :, 2:3])
    with pytest.raises(ValueError, match='stats'):
        metrics.flow_occlusion_mask(tf[..., 1:3], stats=torch.zeros(2, device=DEV))


def test_non_finite_flows_give_what_the_twin_gives():
    lib = _lib.lib()
    f = OC.flow('smooth', 2, 20).copy()
    f[1, 5, 7, 0], f[1, 12, 3, 1], f[0, 9, 9, 1] = np.nan, np.inf, np.nan
    tf = _dev(f)
    for keep in (True, False):
        stats = _sent(3)
        mask = _mask(lib, tf, keep, stats=stats)
        torch.cuda.synchronize()
        want, shares = metrics.flow_occlusion_mask_host(f, A1, A2, keep, np.float32)
        assert np.array_equal(mask.cpu().numpy()[..., 0], want) and np.array_equal(stats.cpu().numpy(), np.float32(shares))
        assert want[1, 5, 7] == want[0, 9, 9] == (1.0 if keep else 0.0)


# ------------------------------------------------------------------------------------------------ the fused head
@pytest.mark.parametrize("kind", [2, 1])
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("family,n,h", OC.CASES)
def test_fused_head_against_the_chain_and_the_twin(family, n, h, c, kind):
    lib = _lib.lib()
    src_h, tgt_h = OC.head_images(n, h, c)
    src, tgt, tf = _dev(src_h), _dev(tgt_h), _dev(OC.flow(family, n, h))
    stats = _sent(3)
    loss, warp, gen, dflow, mask = _head(lib, src, tf, tgt, kind, stats=stats)
    closs, cwarp, cgen, cdflow, cmask = _chain(lib, src, tf, tgt, kind)
    torch.cuda.synchronize()
    label = '%s-%dx%d C=%d kind=%d' % (family, n, h, c, kind)
    assert np.array_equal(_bits(warp), _bits(cwarp)), label
    assert np.array_equal(_bits(gen), _bits(cgen)), label                    # unmasked
    assert np.array_equal(_bits(mask), _bits(cmask)), label
    assert np.array_equal(_bits(dflow), _bits(cdflow)), label
    want, shares = _mask_reference(family, n, h, True)
    assert np.array_equal(mask.cpu().numpy()[..., 0].astype(np.float64), want) and np.array_equal(stats.cpu().numpy(), np.float32(shares))
    l64, l32 = _head_reference(family, n, h, c, kind)
    got, chain = float(loss.cpu()[0]), float(closs.cpu()[0])
    print('%-28s loss %.9g err %.2e float32 twin %.2e | chain %.9g rel %.2e | max |dflow| %.3e, zero where occluded: %s'
          % (label, l64, abs(got - l64), abs(l32 - l64), chain, abs(got - chain) / abs(chain), float(dflow.abs().max()),
             bool((dflow.cpu().numpy()[want == 0] == 0).all())))
    assert np.isfinite(got) and got > 0 and float(dflow.abs().max()) > 0
    assert abs(got - l64) <= 4 * abs(l32 - l64), (label, got, l64, l32)
    assert abs(got - chain) <= 3e-6 * abs(chain), (label, got, chain)
    assert not np.any(dflow.cpu().numpy()[want == 0])                        # an occluded pixel pulls nothing


def test_optional_outputs_and_the_mask_choice_do_not_change_the_others():
    lib = _lib.lib()
    family, n, h, c = 'large', 4, 72, 3
    src_h, tgt_h = OC.head_images(n, h, c)
    src, tgt, tf = _dev(src_h), _dev(tgt_h), _dev(OC.flow(family, n, h))
    full = _head(lib, src, tf, tgt, 2)
    bare = _head(lib, src, tf, tgt, 2, want_dflow=False, warp=False, mask=False)
    drop = _head(lib, src, tf, tgt, 2, keep=False)
    cdrop = _chain(lib, src, tf, tgt, 2, keep=False)
    torch.cuda.synchronize()
    assert _bits(full[0])[0] == _bits(bare[0])[0] and np.array_equal(_bits(full[2]), _bits(bare[2]))
    assert np.array_equal(_bits(drop[2]), _bits(full[2]))                   # gen does not know the mask
    assert np.array_equal(_bits(drop[4]), _bits(cdrop[4])) and np.array_equal(_bits(drop[3]), _bits(cdrop[3]))
    assert np.array_equal(drop[4].cpu().numpy()[..., 0].astype(np.float64), _mask_reference(family, n, h, False)[0])
    assert float(drop[0].cpu()[0]) < float(full[0].cpu()[0])                 # the outside pixels have left the loss


def test_a_target_equal_to_the_warped_source_gives_exactly_zero():
    lib = _lib.lib()
    family, n, h, c = 'smooth', 4, 72, 3
    src = _dev(OC.head_images(n, h, c)[0])
    tf = _dev(OC.flow(family, n, h))
    gen = _sent(n, h, h, c)
    lib.warp_resample_fwd(n, h, h, h, h, c, src.data_ptr(), tf.data_ptr(), 2, None, gen.data_ptr(), stream())
    for kind in (2, 1):
        loss, _, gen2, dflow, mask = _head(lib, src, tf, gen, kind, loss=_sent(1))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(gen2), _bits(gen))
        assert loss.cpu().numpy()[0] == np.float32(SENTINEL) + np.float32(0.0) and not np.any(dflow.cpu().numpy())
        assert 0 < mask.mean() < 1
    lib.loss_overwrite_next()
    loss = _head(lib, src, tf, gen, 2, loss=_sent(1))[0]
    torch.cuda.synchronize()
    assert _bits(loss)[0] == 0                                              # stored: exactly +0


def test_loss_adds_by_default_and_stores_after_overwrite_next():
    lib = _lib.lib()
    n, h, c = 6, 33, 3
    src_h, tgt_h = OC.head_images(n, h, c)
    src, tgt, tf = _dev(src_h), _dev(tgt_h), _dev(OC.flow('smooth', n, h))
    term = _head(lib, src, tf, tgt, 2, weight=0.25)[0]
    acc = torch.full((1,), 3.5, dtype=torch.float32, device=DEV)
    _head(lib, src, tf, tgt, 2, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    t = np.float32(term.cpu().numpy()[0])
    assert t > 0 and acc.cpu().numpy()[0] == np.float32(3.5) + t          # one fp32 addition onto what was there
    lib.loss_overwrite_next()
    _mask(lib, tf)                                                         # the mask entry is no loss entry: the flag stays
    _head(lib, src, tf, tgt, 2, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t                                      # stored
    _head(lib, src, tf, tgt, 2, weight=0.25, loss=acc)
    torch.cuda.synchronize()
    assert acc.cpu().numpy()[0] == t + t                                  # the flag was consumed: this call adds again


def test_two_runs_and_a_replayed_plan_give_the_same_bits():
    lib = _lib.lib()
    family, n, h, c = 'large', 4, 72, 3
    src_h, tgt_h = OC.head_images(n, h, c)
    src, tgt, tf = _dev(src_h), _dev(tgt_h), _dev(OC.flow(family, n, h))
    nb = int(lib.warp_resample_occlusion_loss_workspace_bytes(n, h, h))
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        lib.loss_overwrite_next()
        stats = _sent(3)
        runs.append(_head(lib, src, tf, tgt, 2, loss=_sent(1), stats=stats, ws=ws) + (stats,))
        ws.fill_(255)                                                       # no state survives in the workspace between calls
    loss, stats = _sent(1), _sent(3)
    warp, gen, dflow, mask = _sent(n, h, h, 2), _sent(n, h, h, c), _sent(n, h, h, 2), _sent(n, h, h, 1)
    plan = lib.plan_create()
    lib.plan_begin(plan)
    try:
        lib.loss_overwrite_next()                                           # a recorded call keeps the flag it saw
        lib.warp_resample_occlusion_loss(n, h, h, h, h, c, src.data_ptr(), tf.data_ptr(), 2, tgt.data_ptr(), c, 2, WEIGHT, A1, A2, 1,
                                         warp.data_ptr(), gen.data_ptr(), dflow.data_ptr(), 2, mask.data_ptr(), 1, loss.data_ptr(),
                                         stats.data_ptr(), ws.data_ptr(), nb, None)
        lib.flow_occlusion_mask(n, h, h, tf.data_ptr(), 2, A1, A2, 1, mask.data_ptr(), 1, None, None, 0, None)
    finally:
        lib.plan_end()
    assert [o[0] for o in _lib.plan_ops(plan)] == HEAD + ['occl_mask']
    torch.cuda.synchronize()
    assert loss.cpu().numpy()[0] == SENTINEL and np.all(gen.cpu().numpy() == SENTINEL)      # recording launches nothing
    for _ in range(2):                                                      # replayed twice: it stores both times
        lib.plan_run(plan, stream())
    torch.cuda.synchronize()
    lib.plan_destroy(plan)
    third = (loss, warp, gen, dflow, mask, stats)
    for a, b, c3 in zip(runs[0], runs[1], third):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c3))
    assert not np.any(dflow.cpu().numpy() == SENTINEL) and not np.any(mask.cpu().numpy() == SENTINEL)


def test_argument_errors_leave_every_output_untouched_and_the_overwrite_pending():
    lib = _lib.lib()
    n, h, c = 2, 20, 3
    src_h, tgt_h = OC.head_images(n, h, c)
    src, tgt, tf = _dev(src_h), _dev(tgt_h), _dev(OC.flow('smooth', n, h))
    loss, stats = _sent(1), _sent(3)
    warp, gen, dflow, mask = _sent(n, h, h, 2), _sent(n, h, h, c), _sent(n, h, h, 2), _sent(n, h, h, 1)
    nb = int(lib.warp_resample_occlusion_loss_workspace_bytes(n, h, h))
    ws = torch.empty(nb + 64, dtype=torch.uint8, device=DEV)
    ok = dict(N=n, H=h, W=h, Hs=h, Ws=h, C=c, src=src.data_ptr(), flow=tf.data_ptr(), flow_ld=2, tgt=tgt.data_ptr(), tgt_ld=c, kind=2, weight=1.0,
              a1=A1, a2=A2, keep=1, warp=warp.data_ptr(), gen=gen.data_ptr(), dflow=dflow.data_ptr(), dflow_ld=2, mask=mask.data_ptr(), mask_ld=1,
              loss=loss.data_ptr(), stats=stats.data_ptr(), ws=ws.data_ptr(), ws_bytes=nb)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.raw_warp_resample_occlusion_loss(
            v['N'], v['H'], v['W'], v['Hs'], v['Ws'], v['C'], v['src'], v['flow'], v['flow_ld'], v['tgt'], v['tgt_ld'], v['kind'], v['weight'],
            v['a1'], v['a2'], v['keep'], v['warp'], v['gen'], v['dflow'], v['dflow_ld'], v['mask'], v['mask_ld'], v['loss'], v['stats'],
            v['ws'], v['ws_bytes'], stream())

    def mask_call(**kw):
        v = dict(ok, **kw)
        return lib.raw_flow_occlusion_mask(v['N'], v['H'], v['W'], v['flow'], v['flow_ld'], v['a1'], v['a2'], v['keep'], v['mask'], v['mask_ld'],
                                           v['stats'], v['ws'], v['ws_bytes'], stream())
    nan, inf = float('nan'), float('inf')
    lib.loss_overwrite_next()                                  # stays pending through every refusal
    for kw, code, word in [(dict(N=1), -1, 'N'), (dict(N=3), -1, 'N'), (dict(W=h + 1, Ws=h + 1), -1, 'differ'), (dict(Hs=h - 1), -1, 'source'),
                           (dict(H=1, W=1, Hs=1, Ws=1), -1, 'H'), (dict(C=5), -1, 'C'), (dict(flow_ld=1), -1, 'flow_ld'), (dict(tgt_ld=2), -1, 'target_ld'),
                           (dict(dflow_ld=1), -1, 'dflow_ld'), (dict(mask_ld=0), -1, 'mask_ld'), (dict(kind=0), -1, 'kind'),
                           (dict(weight=inf), -1, 'weight'), (dict(a1=-1.0), -1, 'alpha1'), (dict(a1=nan), -1, 'alpha1'), (dict(a2=0.0), -1, 'alpha2'),
                           (dict(a2=inf), -1, 'alpha2'), (dict(keep=2), -1, 'outside_visible'), (dict(src=None), -1, 'src is null'),
                           (dict(gen=None), -1, 'gen is null'), (dict(loss=None), -1, 'loss_accum is null'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(dflow=dflow.data_ptr() + 2), -1, 'aligned'), (dict(ws_bytes=nb - 1), -3, 'workspace'),
                           (dict(ws=ws.data_ptr() + 8), -3, 'aligned')]:
        assert call(**kw) == code, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    for kw, code, word in [(dict(N=3), -1, 'N'), (dict(W=h + 1), -1, 'differ'), (dict(flow_ld=1), -1, 'flow_ld'), (dict(mask_ld=0), -1, 'mask_ld'),
                           (dict(a1=inf), -1, 'alpha1'), (dict(a2=-1.0), -1, 'alpha2'), (dict(keep=-1), -1, 'outside_visible'),
                           (dict(flow=None), -1, 'flow is null'), (dict(mask=None, stats=None), -1, 'both null'), (dict(ws=None), -1, 'workspace is null'),
                           (dict(ws_bytes=nb - 1), -3, 'workspace')]:
        assert mask_call(**kw) == code, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    torch.cuda.synchronize()
    for t in (loss, stats, warp, gen, dflow, mask):
        assert np.all(t.cpu().numpy() == SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    got = loss.cpu().numpy()[0]
    assert 0 < got < 10.0 and got != SENTINEL                                 # stored over the sentinel: the flag was still pending
    for t in (stats, warp, gen, dflow, mask):
        assert not np.any(t.cpu().numpy() == SENTINEL)
    assert abs(float(stats.sum().cpu()) - 1.0) < 1e-6
