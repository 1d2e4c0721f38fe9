"""The small-grid cases of tests/helpers/small_grids.py without a device: what the cases claim to reach, the files they
write read back through build_problem, and the reference's fixture (tests/golden/expected_small_grids.npz) against the
CPU oracle on the same files."""
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
