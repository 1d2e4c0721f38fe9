"""The small-grid cases of tests/helpers/small_grids.py without a device: what the cases claim to reach, the files they
write read back through build_problem, and the reference's fixture (tests/golden/expected_small_grids.npz) against the
CPU oracle on the same files.  The same for the metal cases (METAL_CASES, tests/golden/expected_small_metals.npz)."""
import numpy as np
import pytest

from conftest import GOLDEN
from helpers import small_grids as sg


def test_the_cases_reach_what_they_claim():
    sg.check_claims()
    assert [sg.tape_row0(n) for n in (63, 64, 65, 1296, 2500, 5000)] == [0, 0, 0, 16, 4, 8]


@pytest.mark.parametrize('case', list(sg.CASES))
def test_files_come_back_through_build_problem(case, tmp_path):
    prob = sg.build_case(tmp_path, case, GOLDEN)
    sg.check_facts(case, prob)
    exp = np.load(GOLDEN / 'expected_small_grids.npz')
    assert exp[f'{case}/chi2'].shape == (1 + sg.N_WALKERS,)
    for name, item in prob.items.items():
        assert exp[f'{case}/model/{name}'].shape == (1 + sg.N_WALKERS, item.dist_grid.size)
    if max(item.model_grid.size for item in prob.items.values()) > 1300:
        return                                              # (the oracle takes seconds on the larger grids)
    from oracle import vega_cpu as oc
    names = [str(n) for n in exp[f'{case}/param_names']]
    for w in (0, 2):
        pars = dict(zip(names, exp[f'{case}/theta'][w]))
        assert oc.chi2(prob, pars) == pytest.approx(exp[f'{case}/chi2'][w], rel=1e-6)
        model = oc.compute_model(prob, pars)
        for name in prob.items:
            ref = exp[f'{case}/model/{name}'][w]
            assert np.abs(model[name] - ref).max() <= 1e-8 * np.abs(ref).max()


def test_the_metal_cases_reach_what_they_claim():
    """Every remainder of n_rp and n_rt mod 5 (k_metal_kron's five outputs per thread), the LDS test of the Kronecker sets."""
    sg.check_metal_claims()
    rp = {f['kron'][0] % 5 for _, facts in sg.METAL_CASES.values() for f in facts}
    rt = {f['kron'][1] % 5 for _, facts in sg.METAL_CASES.values() for f in facts if f['kron'][1] is not None}
    assert rp == rt == {0, 1, 2, 3, 4}


@pytest.fixture(scope='module')
def small_metals():
    with np.load(GOLDEN / 'expected_small_metals.npz') as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('case', list(sg.METAL_CASES))
def test_metal_files_come_back_through_build_problem(case, tmp_path, small_metals):
    prob = sg.build_case(tmp_path, case, GOLDEN)
    sg.check_facts(case, prob)
    exp = small_metals
    assert exp[f'{case}/chi2'].shape == (1 + sg.N_WALKERS,) and np.all(np.isfinite(exp[f'{case}/chi2']))
    assert exp[f'{case}/theta'].shape == (1 + sg.N_WALKERS, exp[f'{case}/param_names'].size)
    for name, item in prob.items.items():
        assert exp[f'{case}/model/{name}'].shape == (1 + sg.N_WALKERS, item.dist_grid.size)
    for variant, base in sg.METAL_VARIANTS.items():
        if base == case:
            var = sg.metal_variant(prob, variant)
            sg.check_facts(case, prob)                      # (the case's own Problem is untouched)
            item = next(iter(var.items.values()))
            if variant == 'm63_mixed':
                assert [i for i, p in enumerate(item.metals) if p.matrix is None] == list(sg.MIXED_PLAIN_PAIRS)
            else:
                assert item.metal_opts['fast_metals']


@pytest.mark.parametrize('case', ['m63', 'm64_rp', 'mx1320'])
def test_metal_oracle_against_the_reference(case, tmp_path, small_metals):
    """The CPU oracle - what the Problem-level variants of m63 are compared with on the device - against the unmodified
    reference on the same files: chi2 to 1e-6, models to 1e-8 of their scale (the bars of BASELINE.json)."""
    from oracle import vega_cpu as oc
    prob = sg.build_case(tmp_path, case, GOLDEN)
    exp = small_metals
    names = [str(n) for n in exp[f'{case}/param_names']]
    for w in (0, 2):
        pars = dict(zip(names, exp[f'{case}/theta'][w]))
        assert oc.chi2(prob, pars) == pytest.approx(exp[f'{case}/chi2'][w], rel=1e-6)
        model = oc.compute_model(prob, pars)
        for name in prob.items:
            ref = exp[f'{case}/model/{name}'][w]
            assert np.abs(model[name] - ref).max() <= 1e-8 * np.abs(ref).max()
