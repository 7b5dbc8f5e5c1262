"""The argument lists the loss terms hand to the library (loss_calls.py), checked against the declared C signatures (_lib) without a
GPU: a recording stand-in for the library notes (entry, args); a shifted, missing or mistyped argument fails here."""
import pytest
import torch

from dynamic_multiview_3d_amd import _lib, tf_utils
from dynamic_multiview_3d_amd import graph as G


class Recorder:
    """Stands in for _lib.lib(): every attribute is an entry that notes its call; status entries answer 0, size entries 64."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 64 if name.endswith('workspace_bytes') else 0
        return entry


@pytest.fixture(scope='module')
def terms():
    """{case: LossTerm} over the tensors of one small finalized CPU graph; every differentiated tensor has a gradient buffer."""
    with G.Graph(device='cpu') as g:
        img = g.placeholder([2, 16, 16, 3], 'img')
        tgt = g.placeholder([2, 16, 16, 3], 'tgt')
        mask = g.placeholder([2, 16, 16, 1], 'mask')
        pred = tf_utils.conv2d_msra(img, 3, 3, 3, 1, 1, 'pred')
        flow = tf_utils.conv2d_msra(img, 2, 3, 3, 1, 1, 'flow')
    g.finalize()
    assert pred.requires_grad and flow.requires_grad
    return g, {
        'ssim_loss': G.SsimTerm(pred, tgt, 1.0),
        'ssim_loss_masked': G.SsimTerm(pred, tgt, 1.0, mask),
        'census_loss': G.CensusTerm(pred, tgt, 1.0, 2, 0.01),
        'census_loss_masked': G.CensusTerm(pred, tgt, 1.0, 2, 0.01, mask),
        'flow_smoothness': G.SmoothTerm(flow, None),
        'flow_smoothness guided': G.SmoothTerm(flow, tgt, 10.0),
        'multiscale_warp_loss': G.MultiscaleTerm(flow, tgt, img, 2, (1.0, 0.5)),
        'multiscale_warp_loss_masked': G.MultiscaleTerm(flow, tgt, img, 2, (1.0, 0.5), mask=mask),
        'flow_consistency': G.ConsistTerm(flow),
    }


CASES = ['ssim_loss', 'ssim_loss_masked', 'census_loss', 'census_loss_masked', 'flow_smoothness', 'flow_smoothness guided',
         'multiscale_warp_loss', 'multiscale_warp_loss_masked', 'flow_consistency']
# the size entry each term asks: only the SSIM loss has a masked one
SIZE_ENTRY = {'ssim_loss_masked': 'ssim_loss_masked', 'census_loss_masked': 'census_loss', 'multiscale_warp_loss_masked': 'multiscale_warp_loss'}


def _converts(argtypes, args):
    assert len(args) == len(argtypes)
    for k, (argtype, arg) in enumerate(zip(argtypes, args)):
        try:
            argtype.from_param(arg)
        except Exception as e:
            raise AssertionError("argument %d (%r) does not convert to %s: %s" % (k, arg, argtype.__name__, e))


@pytest.mark.parametrize('value, grad, accumulate', [(True, False, False), (True, True, False), (True, True, True), (False, True, True)])
@pytest.mark.parametrize('case', CASES)
def test_launch_calls_one_entry_with_the_declared_arguments(terms, case, value, grad, accumulate):
    g, by_case = terms
    term = by_case[case]
    term.ws = torch.empty(64, dtype=torch.uint8)
    rec, real = Recorder(), g.lib
    g.lib = rec
    try:
        term.launch(g, 0.5, value, grad, accumulate)
    finally:
        g.lib = real
    (name, args), = rec.calls                               # exactly one entry
    assert name == case.split()[0]                          # the masked entry with a mask, the unmasked one without
    _converts(_lib.STATUS_FUNCS['mv3d_' + name], args)


@pytest.mark.parametrize('case', CASES)
def test_workspace_bytes_calls_one_size_entry_with_the_declared_arguments(terms, case):
    term = terms[1][case]
    rec = Recorder()
    assert term.workspace_bytes(rec) == 64
    (name, args), = rec.calls
    assert name == SIZE_ENTRY.get(case, case.split()[0]) + '_workspace_bytes'
    _converts(_lib.OTHER_FUNCS['mv3d_' + name][1], args)


def test_the_stand_in_check_refuses_a_shifted_argument():
    """The check has teeth: an argument list one short, or with a float where an address goes, does not pass."""
    good = (2, 16, 16, 3, 0x1000, 3, 0x2000, 3, 1.0, 0.5, 0x3000, None, 3, 0, 0x4000, 64, None)
    _converts(_lib.STATUS_FUNCS['mv3d_ssim_loss'], good)
    with pytest.raises(AssertionError):
        _converts(_lib.STATUS_FUNCS['mv3d_ssim_loss'], good[:-1])
    with pytest.raises(AssertionError):
        _converts(_lib.STATUS_FUNCS['mv3d_ssim_loss'], good[:4] + (1.5,) + good[5:])
