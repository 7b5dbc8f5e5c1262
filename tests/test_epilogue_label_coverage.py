"""The epilogue parity cases of tests/epilogue_cases.py reach every kernel that evaluates an mv3d_epilogue, relu runs the
kernels lrelu runs, and tanh never reaches a kernel whose epilogue cannot do it.

Recorded on the CPU (nothing is launched), in the way of tests/test_label_coverage.py.  tests/test_gpu_epilogues.py runs the
same cases against the oracle on the GPU; this file is what keeps that test from quietly running other kernels than it
is there for after a planner change."""
import numpy as np
import pytest

from dynamic_multiview_3d_amd import _lib
from tests import epilogue_cases as EC


@pytest.fixture(scope='module')
def relu_labels():
    return {case: EC.record_case(_lib, case, EC.F1, EC.G1) for case in EC.CASES}


# One entry per epilogue code site: every label prefix here must be dispatched by some (case, rung) under F1 / G1, with the
# given suffix where one is named (the gmask instance of a kernel is another template instance).
FAMILIES = [
    ('s2conv<5x5,s1', ''), ('s2conv<5x5,s1', ',gmask>'), ('s2conv<3x3,s1', ''), ('s2conv<3x3,s1', ',gmask>'),
    ('s2conv<5x5,s2', ''), ('s2conv<5x5,s2', ',gmask>'),
    ('sconv<1ph', ''), ('sconv<4ph', ''),
    ('sconv4<', ''), ('sconv4<', ',gmask>'),
    ('smallc_band', ''), ('smallc_band', '<gmask>'),
    ('thin_head<', ''), ('thin_deconv_s2<', ''), ('smallc_img2feat<', ''),
    ('cconv<3x3', ''), ('cconv<3x3', ',gmask>'), ('cconv<5x5', ''), ('cconv<5x5', ',gmask>'),
    ('bconvu<', ''), ('bconvu<', ',ksplit>'), ('igemm_splitk_epilogue', ''),
    ('bconv<phase-split', ''),
    ('hconv<1ph', ''), ('hconv<phase-split', ''), ('hconv<small-img', ''),
    ('igemm<', ''),
    ('small_fc_fwd', ''), ('small_fc_dgrad', ''), ('fc_stream_b3<fwd>', ''), ('fc_stream_b3<dgrad>', ''),
    ('fc_stream<fwd>', ''), ('fc_stream<dgrad>', ''), ('fc_splitk_epilogue', ''),
]


def _has(labels, prefix, suffix):
    if suffix:
        return any(l.startswith(prefix) and l.endswith(suffix) for l in labels)
    return any(l.startswith(prefix) and 'gmask' not in l and 'ksplit' not in l for l in labels) or prefix in labels


@pytest.mark.parametrize('prefix,suffix', FAMILIES, ids=lambda v: v or '-')
def test_every_epilogue_code_site_is_reached(relu_labels, prefix, suffix):
    labels = set()
    for rec in relu_labels.values():
        labels.update(rec[EC.FWD] + rec[EC.DGRAD])
    assert _has(labels, prefix, suffix), "no epilogue case dispatches %s...%s: %s" % (prefix, suffix, sorted(labels))


def test_generic_fc_is_reached(relu_labels):
    """The generic fc path is the implicit GEMM on a 1 x 1 geometry: its label is an igemm label, so it is pinned per case."""
    for case in ((EC.FC_STREAM, EC.R_GENERIC), (EC.FC_SMALL, EC.R_GENERIC | 4)):
        rec = relu_labels[case]
        assert rec[EC.FWD][0].startswith('igemm<') and rec[EC.DGRAD][0].startswith('igemm<'), (case, rec)


def test_default_cases_run_the_kernels_they_are_named_for(relu_labels):
    """The table of tests/epilogue_cases.py, first column by first column: what each default-rung shape is there for."""
    want = {
        EC.S2_5: ('s2conv<5x5,s1,C32,N32>', 's2conv<5x5,s1,C32,N32,gmask>'),
        EC.S2_3: ('s2conv<3x3,s1,C64,N32>', 's2conv<3x3,s1,C64,N32,gmask>'),
        EC.SC_S1: ('sconv<1ph,32px,N32>', 'sconv<1ph,32px,N32>'),
        EC.SC_E4: ('sconv<1ph,32px,N32>', 'sconv<4ph,32px,N32>'),
        EC.S2_E2: ('s2conv<5x5,s2,C32,N32>', 'sconv4<5x5,C64,64px,gmask>'),
        EC.SC_D4: ('sconv<4ph,32px,N32>', 'sconv<1ph,32px,N32>'),
        EC.S4_D2: ('sconv4<5x5,C64,64px>', 's2conv<5x5,s2,C32,N32,gmask>'),
        EC.TH_E0: ('smallc_band', 'thin_deconv_s2<3>'),
        EC.TH_FLOW: ('thin_head<2>', 'smallc_band<gmask>'),
        EC.TH_RGB: ('thin_head<3>', 'smallc_band<gmask>'),
    }
    for shape, (fwd, dgrad) in want.items():
        rec = relu_labels[(shape, EC.R_DEFAULT)]
        assert rec[EC.FWD][-1] == fwd and rec[EC.DGRAD][-1] == dgrad, (shape, rec)
    for shape in (EC.RAG_C, EC.RAG_D):
        rec = relu_labels[(shape, EC.R_DEFAULT)]
        assert rec[EC.FWD][-1].startswith('igemm<') and rec[EC.DGRAD][-1].startswith('igemm<'), (shape, rec)


@pytest.mark.parametrize('case', EC.CASES, ids=EC.case_id)
def test_relu_runs_the_kernels_lrelu_runs(relu_labels, case):
    """RELU really goes through the hand-written epilogues: no planner branch sends it elsewhere."""
    assert relu_labels[case] == EC.record_case(_lib, case, EC.F_LRELU02, EC.G_LRELU02)


# Label prefixes of the kernels whose branch-free epilogue has no tanh (MV3D_ACT_TANH would fall into the relu coefficients):
# cconv.hip fin_group, sconv.hip sconv4_kernel and s2conv_kernel, thin.hip smallc_band.  The guards in try_cconv,
# try_smallc_band, try_sconv4 and try_s2conv are all that keeps a tanh MASK away from them, and the second line behind
# try_hconv's choice of the exact kernels for a tanh forward.  sconv<1ph / 4ph> (sconv_kernel, sconv.hip) is not one of
# them: its epilogue is common.h act_apply / act_grad_from_out.  It still takes a tanh mask, which the GPU test holds to
# 1 - y^2; a tanh FORWARD never reaches it or any other split-bf16 kernel of try_hconv (the test below), so the tanh branch of
# act_apply in sconv.hip and bconv.hip is not run by any planner path.  thin_head evaluates a tanh forward itself and is
# held to np.tanh on the GPU.
NO_TANH = ('cconv<', 's2conv<', 'sconv4<', 'smallc_band')


@pytest.mark.parametrize('case', EC.CASES, ids=EC.case_id)
def test_tanh_never_reaches_an_epilogue_without_tanh(case):
    rec = EC.record_case(_lib, case, EC.F4, EC.G3)
    for direction in (EC.FWD, EC.DGRAD):
        bad = [l for l in rec[direction] if l.startswith(NO_TANH)]
        assert not bad, "%s %s with tanh dispatches %s" % (EC.case_id(case), direction, bad)


EXACT = ('hconv<', 'hconvp<', 'igemm<', 'igemm_splitk_epilogue', 'transpose_filter')


@pytest.mark.parametrize('case', [c for c in EC.CASES if c[0][0] != EC.FC and min(EC.produced(c[0], EC.FWD)[-1], EC.consumed(c[0], EC.FWD)[-1]) >= 16],
                         ids=EC.case_id)
def test_tanh_forward_takes_the_exact_fp32_kernels(case):
    """hconv.hip try_hconv: a tanh forward of a layer with 16 or more channels on both sides runs no split-bf16 kernel, on any rung
    (tanh turns their absolute error into an error relative to 1: tests/test_gpu_epilogues.py)."""
    rec = EC.record_case(_lib, case, EC.F4, EC.G3)
    assert rec[EC.FWD] and all(l.startswith(EXACT) for l in rec[EC.FWD]), rec[EC.FWD]


def test_tanh_guards_are_exercised(relu_labels):
    """The test above means something only if, without tanh, the same calls DO reach each of the four kernels."""
    for prefix in NO_TANH:
        for direction in (EC.FWD, EC.DGRAD):
            assert any(l.startswith(prefix) for rec in relu_labels.values() for l in rec[direction]), (prefix, direction)


def _all_shapes():
    shapes = []
    for shape, _ in EC.CASES:
        if shape not in shapes:
            shapes.append(shape)
    return shapes


@pytest.mark.parametrize('shape', _all_shapes(), ids=lambda s: '-'.join(str(v) for v in s))
def test_relu_band_stays_under_its_cap(shape):
    """The GPU test leaves the elements within 1e-5 max|pre| of the relu kink out of its sign checks, on the condition that
    they are few: at most 8 + 1e-4 size.  With the oracle alone: the forward of every shape of the table satisfies it."""
    pre = EC.pre_activation(shape, EC.FWD, EC.F1)
    band, cap = EC.relu_band(pre)
    assert band.sum() <= cap, (shape, int(band.sum()), cap)
    assert not (pre == 0).any()


def test_saved_outputs_hold_the_populations_the_masks_need():
    rng = np.random.default_rng(0)
    y, slope = EC.saved_output((2, 8, 8, 6), EC.ACT_RELU, rng)
    z = y == 0
    assert (y > 0).any() and (z & np.signbit(y)).any() and (z & ~np.signbit(y)).any() and not (y < 0).any()
    assert set(np.unique(slope)) == {0.0, 0.5, 1.0} and np.all(slope[z & np.signbit(y)] == 0) and np.all(slope[z & ~np.signbit(y)] == 0.5)
    y, _ = EC.saved_output((2, 8, 8, 6), EC.ACT_LRELU, rng)
    z = y == 0
    assert (y > 0).any() and (y < 0).any() and (z & np.signbit(y)).any() and (z & ~np.signbit(y)).any()
    s = EC.lrelu_slope(y, 0.3)
    assert np.all(s[z] == 0.65) and np.allclose(s[y > 0], 1.0) and np.allclose(s[y < 0], 0.3)
    y, slope = EC.saved_output((8, 40), EC.ACT_TANH, rng)
    assert np.abs(y).max() < 1 and np.all(slope == 1 - y.astype(np.float64) ** 2)
