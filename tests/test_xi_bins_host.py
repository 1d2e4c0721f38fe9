"""The spline-bins oracle of tests/helpers/xi_bins_oracle.py without a device.

  * Tie to the reference: fed the coefficients OP_ell P_ell (vega_amd/fftlog_op.py) of oracle.vega_cpu's own multipoles, the
    longdouble restatement reproduces oracle.vega_cpu's per-component xi to 1e-10 of the vector's scale - the reference
    interpolates xi_ell with scipy's not-a-knot cubic spline, this project evaluates a uniform cubic B-spline; this test is
    what ties the two - on the golden configurations auto, joint and joint_metals_fast and on every case of
    tests/test_xi_bins_gpu.py (radiation on unrescaled and on rescaled coordinates, Croom evolution, split evolution, UV shot
    noise 1 and 2, the relativistic and asymmetry odd multipoles, the template + broadband item,
    single_ell, ell_max = 2, 4 and 6, fht_lowring = False).
  * The bound holds and bites: the float64 twin of the kernel arithmetic stays within the a-priori bound on every bin of
    every case, and each named mutation exceeds it in at least one bin of at least one case.
  * The cases' claims (sizes, which options are on) hold on the built Problems.
"""
import copy

import numpy as np
import pytest

from conftest import GOLDEN, load_problem
from helpers import small_grids as sg
from helpers import xi_bins_oracle as xo

LD = np.longdouble
TIE_RTOL = 1e-10


def _need_extended_precision():
    assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'


@pytest.fixture(scope='module')
def operands(tmp_path_factory):
    """{case: [per walker {(item, component): operands}]} of every case, built once."""
    sg.check_claims()
    out = {}
    tmp = tmp_path_factory.mktemp('xi_bins')
    for case in xo.CASES:
        prob = xo.build_case(tmp, case, GOLDEN)
        out[case] = [xo.host_operands(prob, row) for row in xo.walker_params(prob)]
    return out


def _tie(ops, what):
    for key, o in ops.items():
        xi, bound, oob, _ = xo.xi_bins(o['desc'], o['st'], o['grid'], o['sc'], o['ix'], o['coef'], terms=o['terms'])
        assert not oob.any(), (what, key)
        scale = np.abs(o['ref']).max()
        err = np.abs(xi - o['ref'].astype(LD)).max()
        assert err <= TIE_RTOL * scale, f'{what} {key}: {float(err / scale):.3e} of scale'
        assert np.all(xi[o['st']['r'] == 0] == 0)


@pytest.mark.parametrize('config', ['auto', 'joint', 'joint_metals_fast'])
def test_oracle_reproduces_the_reference_on_the_golden_configurations(config):
    _need_extended_precision()
    prob = load_problem(config)
    for w, row in enumerate(xo.walker_params(prob, n=1)):
        _tie(xo.host_operands(prob, row), f'{config} walker {w}')


@pytest.mark.parametrize('case', list(xo.CASES))
def test_oracle_reproduces_the_reference_on_the_cases(operands, case):
    _need_extended_precision()
    for w, ops in enumerate(operands[case]):
        _tie(ops, f'{case} walker {w}')


def _ratio(o, mutation=None):
    xi, bound, _, _ = xo.xi_bins(o['desc'], o['st'], o['grid'], o['sc'], o['ix'], o['coef'], terms=o['terms'])
    twin = xo.twin_bins(o['desc'], o['st'], o['grid'], o['sc'], o['ix'], o['coef'], mutation, terms=o['terms'])
    err = np.abs(twin.astype(LD) - xi)
    assert np.all((bound > 0) | (err == 0))
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), bound, xi


def test_bound_holds_for_the_float64_twin_on_every_bin(operands):
    _need_extended_precision()
    worst, rel = {}, []
    for case, walkers in operands.items():
        for w, ops in enumerate(walkers):
            for key, o in ops.items():
                ratio, bound, xi = _ratio(o)
                worst[case] = max(worst.get(case, 0.0), float(ratio.max()))
                live = xi != 0
                rel.append((bound[live] / np.abs(xi[live]) / xo.U).astype(float))
                assert np.all(ratio <= 1), f'{case} walker {w} {key}: bin {int(np.argmax(ratio))} at {float(ratio.max()):.3f} of its bound'
    rel = np.concatenate(rel)
    print('\nXIBINS_HOST twin error / bound per case:', {k: float(f'{v:.3g}') for k, v in worst.items()},
          f'; bound in u |xi|: median {np.median(rel):.0f}, 99th percentile {np.percentile(rel, 99):.0f}')
    assert np.median(rel) < 1000                     # the bound is a rounding count, not orders above one


@pytest.mark.parametrize('mutation', xo.MUTATIONS)
def test_every_mutation_exceeds_the_bound_somewhere(operands, mutation):
    _need_extended_precision()
    worst = 0.0
    for case, walkers in operands.items():
        if mutation == 'surplus_walker':
            # a batch of three through a two-walker kernel: the last walker sits alone in its block
            keys = list(walkers[0])
            for key in keys:
                o = [ops[key] for ops in walkers[:3]]
                got = xo.twin_batch(o[0]['desc'], o[0]['st'], o[0]['grid'], np.stack([q['sc'] for q in o]), o[0]['ix'],
                                    np.stack([q['coef'] for q in o]), nw=2, mutation=mutation, terms=o[0]['terms'])
                clean = xo.twin_batch(o[0]['desc'], o[0]['st'], o[0]['grid'], np.stack([q['sc'] for q in o]), o[0]['ix'],
                                      np.stack([q['coef'] for q in o]), nw=2, terms=o[0]['terms'])
                for b in range(3):
                    xi, bound, _, _ = xo.xi_bins(o[b]['desc'], o[b]['st'], o[b]['grid'], o[b]['sc'], o[b]['ix'], o[b]['coef'], terms=o[b]['terms'])
                    assert np.all(np.abs(clean[b].astype(LD) - xi) <= bound)
                    live = bound > 0
                    worst = max(worst, float((np.abs(got[b].astype(LD) - xi)[live] / bound[live]).max()))
            continue
        for ops in walkers:
            for o in ops.values():
                worst = max(worst, float(_ratio(o, mutation)[0].max()))
    print(f'\nXIBINS_HOST mutation {mutation}: largest error / bound {worst:.3g}')
    assert worst > 1, mutation


def test_scalar_names_follow_the_header():
    """Engine.BINS_SCALAR_NAMES is the Python copy of VMX_DEBUG_SCALARS (include/vegamx.h), from which the library builds tap 7."""
    import re
    from conftest import REPO
    from vega_amd.engine import Engine
    header = (REPO / 'include' / 'vegamx.h').read_text()
    macro = re.search(r'#define VMX_DEBUG_SCALARS\(X\)((?:.*\\\n)*.*)\n', header).group(1)
    assert tuple(re.findall(r'X\((\w+)\)', macro)) == Engine.BINS_SCALAR_NAMES
