"""The tiers of the mu node rule (vega_amd/mu_quadrature.py: TIERS; the engine's copy: csrc/vmx_plan.h), on the CPU.

The harness and the draws of tests/test_mu_quadrature.py: the oracle's P(k, mu) on the nodes of every tier against the
reference's 1000-point midpoint sums, 104 draws over the guard box with corners (seed 20261005), the `joint` problem, four
moments, both items, peak and smooth.  The error is a fraction of the largest k^3 M_n, per wavenumber.
  (a) every tier: <= 1e-14 at every wavenumber up to its k_max;
  (b) the composite rule - each wavenumber on the tier its k tile takes, 64-wide and 16-wide tiles - <= 1e-13 over all
      wavenumbers up to K_NODE_MAX (the main rule alone: 7.4e-14, at k = 4 .. 6 h/Mpc);
  (c) each tier's weights reproduce the 1000-point midpoint sums of mu^p, p in {0, 2, 8, 14}, to 2e-14.
Measured (worst over the draws):
  82-node tier (k_max 0.11):   4.2e-15 up to k_max; it holds 1e-14 for the first 378 wavenumbers (k <= 0.188), 1e-13 for 434
  42-node tier (k_max 0.0058): 1.1e-15 up to k_max; it holds 1e-14 for the first 220 wavenumbers (k <= 0.0080), 1e-13 for 238
  composite, 64-wide and 16-wide tiles: 7.4e-14 (the main rule's own worst, at k > 4; on the shorter tiers' wavenumbers
  2.6e-15 with 64-wide and 3.2e-15 with 16-wide tiles)
  weights: <= 1.5e-15 relative for every tier and power
The host code that builds the node lists, assigns the tiers and orders the launch (vmx_plan.h) runs under
AddressSanitizer / UBSan in tests/helpers/mu_tiers_driver.cpp; its node lists and plans are compared with this module's.
"""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_problem
from test_mu_quadrature import K_NODE_MAX, _NodeGrid, _box_draws


@pytest.fixture(scope='module')
def tier_errors():
    """(k, err [tier][k]): per wavenumber the worst |rule - midpoint sum| k^3 over the draws, items, peak / smooth and
    moments, as a fraction of the largest k^3 M_n of its case.  Computed once for the tests below."""
    from oracle import vega_cpu as oc
    from vega_amd.mu_quadrature import TIERS, tier_rule
    mp = pytest.MonkeyPatch()
    mp.setattr(oc, 'sinc', lambda x: np.sinc(np.asarray(x) / np.pi))       # (a node sits at mu = 1: sinc(0))
    try:
        prob = load_problem('joint')
        rules = [tier_rule(t) for t in range(len(TIERS))]
        offs = np.concatenate([[0], np.cumsum([mu.size for mu, _ in rules])])
        full, nodes = oc.PkGrid(prob.k, 1000), _NodeGrid(prob.k, np.concatenate([mu for mu, _ in rules]))
        weight = prob.k**3 * (prob.k <= K_NODE_MAX)
        draws, box = _box_draws(prob, 104, np.random.default_rng(20261005))
        err = np.zeros((len(TIERS), prob.k.size))
        for pars in draws:
            for item in prob.items.values():
                for peak, pk_lin in ((False, prob.pk_smooth), (True, prob.pk_full - prob.pk_smooth)):
                    pp = dict(pars, peak=peak)
                    exact = oc.power_spectrum(item.core, full, pk_lin, prob.pk_fid, pp)
                    at_nodes = oc.power_spectrum(item.core, nodes, pk_lin, prob.pk_fid, pp)
                    for n in range(4):
                        ref = np.sum(full.mu**(2 * n) * exact, axis=0)
                        scale = np.abs(ref * weight).max()
                        if not scale > 0:
                            continue
                        for t, (mu, w) in enumerate(rules):
                            sl = slice(offs[t], offs[t + 1])
                            got = np.sum(w[:, None] * nodes.mu[sl]**(2 * n) * at_nodes[sl], axis=0)
                            err[t] = np.maximum(err[t], np.abs((got - ref) * weight) / scale)
    finally:
        mp.undo()
    return prob.k, err


def test_the_tiers_are_the_issue_s_rules():
    from vega_amd.mu_quadrature import TIERS, tier_of, tier_rule
    assert [tier_rule(t)[0].size for t in range(len(TIERS))] == [178, 82, 42]
    assert TIERS[0]['k_max'] == np.inf and TIERS[1]['k_max'] > TIERS[2]['k_max'] > 0
    assert [tier_of(k) for k in (1e-4, 0.0058, 0.0059, 0.11, 0.111, 6.0, 1e3)] == [2, 2, 1, 1, 0, 0, 0]
    assert tier_of(1e-4, n_tiers=1) == 0 and tier_of(1e-4, n_tiers=2) == 1


def test_every_tier_holds_1e_14_up_to_its_k_max(tier_errors):
    from vega_amd.mu_quadrature import TIERS
    k, err = tier_errors
    for t, tier in enumerate(TIERS):
        upto = k <= min(tier['k_max'], K_NODE_MAX)
        worst = err[t][upto].max()
        prefix = np.maximum.accumulate(err[t])
        held = [int(np.argmax(prefix > bar)) if (prefix > bar).any() else k.size for bar in (1e-14, 1e-13)]
        print(f'tier {t}: {worst:.3g} up to k_max = {tier["k_max"]}; <= 1e-14 for the first {held[0]} wavenumbers '
              f'(k <= {k[held[0] - 1]:.4g}), <= 1e-13 for the first {held[1]}')
        if t > 0:
            assert upto.sum() >= 64            # (the tier serves at least a tile of this grid)
            assert worst <= 1e-14, (t, worst)


@pytest.mark.parametrize('tile', [64, 16])
def test_the_composite_rule_holds_1e_13_everywhere(tier_errors, tile):
    from vega_amd.mu_quadrature import tiers_of_grid
    k, err = tier_errors
    tiers = tiers_of_grid(k, tile)
    assert set(tiers[k <= K_NODE_MAX]) == {0, 1, 2}
    composite = err[tiers, np.arange(k.size)]
    on_short = tiers > 0
    print(f'{tile}-wide tiles: composite {composite.max():.3g}, on the shorter tiers {composite[on_short].max():.3g}, '
          f'main rule alone {err[0].max():.3g}; wavenumbers per tier {np.bincount(tiers[k <= K_NODE_MAX]).tolist()}')
    assert composite.max() <= 1e-13, composite.max()
    assert composite[on_short].max() <= 1e-14


def test_every_tier_s_weights_are_a_quadrature_of_the_midpoint_sum():
    from vega_amd.mu_quadrature import N_MU, TIERS, tier_rule
    mid = (np.arange(N_MU) + 0.5) / N_MU
    for t in range(len(TIERS)):
        mu, w = tier_rule(t)
        assert np.all((mu > 0) & (mu <= 1))
        for p in (0, 2, 8, 14):
            want = np.sum(mid**p)
            rel = abs(np.sum(w * mu**p) - want) / want
            print(f'tier {t} mu^{p}: {rel:.3g}')
            assert rel <= 2e-14, (t, p, rel)


# ---- the engine's host code (vmx_plan.h) under sanitizers, against this module -----------------------------------------
@pytest.fixture(scope='module')
def driver_output(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('mu_tiers') / 'mu_tiers_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'mu_tiers_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert 'FAIL' not in run.stdout and 'runtime error' not in run.stderr and 'AddressSanitizer' not in run.stderr
    assert 'all mu tier checks passed' in run.stdout
    return run.stdout


def test_the_engine_s_tier_nodes_are_this_module_s(driver_output):
    from vega_amd.mu_quadrature import TIERS, extra_nodes
    rows = np.array([line.split()[1:] for line in driver_output.splitlines() if line.startswith('node ')], dtype=float)
    for t, tier in enumerate(TIERS):
        mu_ref, w_ref = extra_nodes(**{key: val for key, val in tier.items() if key != 'k_max'})
        got = rows[rows[:, 0] == t]
        assert got.shape[0] == mu_ref.size == (82, 50, 34)[t]
        np.testing.assert_array_equal(got[:, 1], np.arange(mu_ref.size))
        np.testing.assert_allclose(got[:, 2], mu_ref, rtol=0, atol=2e-16)
        np.testing.assert_allclose(got[:, 3], w_ref, rtol=2e-12)


def test_the_engine_s_launch_plan_takes_this_module_s_tiers(driver_output):
    """The driver's plans of the 814-point logarithmic grid: every tile once, on the tier tier_of gives its largest
    wavenumber, main-rule tiles first, then the shorter tiers, the tiles above K_NODE_MAX last."""
    from vega_amd.mu_quadrature import tier_of
    k = 1e-4 * np.exp(0.02 * np.arange(814))
    for tile in (64, 16):
        line = next(ln for ln in driver_output.splitlines() if ln.startswith(f'plan grid814 kt={tile} tiers=3:'))
        plan = [tuple(int(v) for v in entry.split('/')) for entry in line.split(':')[1].split()]
        n_tiles = (k.size + tile - 1) // tile
        assert sorted(t for t, _ in plan) == list(range(n_tiles))
        classes = []
        for t, tier in plan:
            assert tier == tier_of(k[min((t + 1) * tile, k.size) - 1])
            classes.append(3 if k[t * tile] > K_NODE_MAX else tier)
        assert classes == sorted(classes) and set(classes) == {0, 1, 2, 3}


def test_the_library_uses_the_tested_tier_code():
    hip = (REPO / 'vega_amd' / 'csrc' / 'vegamx.hip').read_text()
    assert 'vmx_plan::build_mu_tiers(' in hip and 'vmx_plan::plan_mu_tiles(' in hip and 'vmx_plan::mu_mean_nodes(' in hip
    assert 'Fornberg' not in hip                # (no second copy of the generator)
    plan = (REPO / 'vega_amd' / 'csrc' / 'vmx_plan.h').read_text()
    from vega_amd.mu_quadrature import TIERS
    for tier in TIERS[1:]:
        assert f"{{{tier['lo']}, {tier['hi']}, {tier['panels']}, {tier['n_gl']}, {tier['k_max']}}}" in plan
