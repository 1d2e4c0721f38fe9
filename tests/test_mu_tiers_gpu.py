"""The tiers of the mu node rule in the level-2 P(k, mu) kernel (k_pk_tab2; vega_amd/mu_quadrature.py: TIERS) on the GPU.

The synthetic joint fit at B = 3 (k_pk_tab2<16,16,1>: 16-wide k tiles), B = 13 (<64,4,1>) and B = 65 (<64,4,2>: two walkers
per thread, the last block with a surplus walker slot), walkers that share their Arinyo / smoothing parameters (table level 2):
  (a) chi2 and the model with the tiers against an engine built with VMX_NO_MU_TIERS=1 (the main rule on every tile) and
      against the plain 1000-point loop (set_mu_quadrature(False)): 1e-11 of the model's scale, chi2 to 1e-11 relative -
      the bars tests/test_mu_quadrature.py uses for rule on / off;
  (b) bitwise: the same batch twice; a walker among other neighbours, in another slot and lane (the batch rolled by one: every
      pair of the two-walker kernel changes partner and slot), without neighbours (a batch of the same size that holds nothing
      but copies of it - a walker evaluated alone runs the 16-wide instantiation, whose tiles, tiers and order of summation
      are another kernel's; at B = 3 that is the batch's own instantiation: there also truly alone, on the stage's output
      P_ell(k)); a batch with one walker outside the
      guard box (a mixed block of the two-walker kernel) against the same walkers evaluated separately - those inside as in
      the all-inside batch, the one outside as with the rule switched off;
  (c) the reported mean number of nodes per wavenumber on the rule: below 178 with the tiers, exactly 178 without.
"""
import numpy as np
import pytest

from conftest import synth_joint_problem

pytestmark = pytest.mark.gpu

VARIED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd', 'beta_hcd', 'L0_hcd']
BATCHES = (3, 13, 65)
BAR = 1e-11


def _engine(max_batch=65):
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=max_batch)
    vega.engine.set_constant_nl_hint(True, gaussian=True)       # (shared Arinyo / smoothing parameters: the level-2 tables)
    return vega


@pytest.fixture(scope='module')
def tiered():
    vega = _engine()
    yield vega
    vega.close()


@pytest.fixture(scope='module')
def main_rule_only():
    mp = pytest.MonkeyPatch()
    mp.setenv('VMX_NO_MU_TIERS', '1')
    try:
        vega = _engine()
    finally:
        mp.undo()
    yield vega
    vega.close()


def _walkers(eng, n):
    from vega_amd import synthetic
    return synthetic.walkers(eng.low.theta0, eng.names, n, varied=VARIED, seed=20261018)


def _eval(eng, theta):
    # (a batch of fewer than 16 walkers runs against level-2 tables once its shared parameters have come twice in a row)
    for _ in range(2):
        chi2, status, model = eng.eval(theta, want_model=True)
        if int(eng.debug_read(4, 0, 5)[4]) == 2:
            break
    assert int(eng.debug_read(4, 0, 5)[4]) == 2         # the level-2 kernel ran
    assert not status.any()
    return chi2, model


@pytest.mark.parametrize('batch', BATCHES)
def test_tiers_against_the_main_rule_and_the_plain_loop(tiered, main_rule_only, batch):
    eng, ref = tiered.engine, main_rule_only.engine
    theta = _walkers(eng, batch)
    c_tier, m_tier = _eval(eng, theta)
    nodes_tier = float(eng.debug_read(4, 0, 5)[2])
    c_main, m_main = _eval(ref, theta)
    nodes_main = float(ref.debug_read(4, 0, 5)[2])
    assert not eng.set_mu_quadrature(False)
    try:
        c_loop, m_loop = _eval(eng, theta)
    finally:
        assert eng.set_mu_quadrature(True)
    for what, c_ref, m_ref in (('main rule', c_main, m_main), ('plain loop', c_loop, m_loop)):
        worst_m = np.abs(m_tier - m_ref).max() / np.abs(m_ref).max()
        worst_c = np.abs(c_tier / c_ref - 1.0).max()
        print(f'B = {batch} tiers against the {what}: model {worst_m:.3g} of its scale, chi2 {worst_c:.3g} relative')
        assert worst_m <= BAR, (what, worst_m)
        assert worst_c <= BAR, (what, worst_c)
    # (c) the statistic bench.py multiplies into its flop count
    print(f'B = {batch} mean nodes per wavenumber on the rule: {nodes_tier:.2f} with tiers, {nodes_main:.2f} without')
    assert 42.0 < nodes_tier < 178.0
    assert nodes_main == 178.0


@pytest.mark.parametrize('batch', BATCHES)
def test_a_walker_s_result_is_bitwise_its_own(tiered, batch):
    eng = tiered.engine
    theta = _walkers(eng, batch)
    c_1, m_1 = _eval(eng, theta)
    c_2, m_2 = _eval(eng, theta)
    np.testing.assert_array_equal(c_1, c_2)
    np.testing.assert_array_equal(m_1, m_2)
    c_r, m_r = _eval(eng, np.roll(theta, 1, axis=0))            # other neighbours, the other slot of a pair
    np.testing.assert_array_equal(np.roll(c_r, -1), c_1)
    np.testing.assert_array_equal(np.roll(m_r, -1, axis=0), m_1)
    for i in sorted({0, batch // 2, batch - 1}):
        c_a, m_a = _eval(eng, np.repeat(theta[i:i + 1], batch, axis=0))         # no neighbour but itself
        np.testing.assert_array_equal(c_a, np.full(batch, c_1[i]))
        np.testing.assert_array_equal(m_a, np.repeat(m_1[i:i + 1], batch, axis=0))
    if batch == 3:
        # truly alone (B = 1 runs the batch's own instantiation of the kernel): the stage's output P_ell(k), bit for bit.  (The
        # model and chi2 of a single walker pass through other kernels than a batch's - the streaming distortion product,
        # chi2 added up in another order - and differ in the last bits with or without tiers: not compared.)
        _eval(eng, theta)
        pl_batch = eng.pk_multipoles(batch)
        for i in range(batch):
            _eval(eng, theta[i:i + 1])
            pl_alone = eng.pk_multipoles(1)
            assert set(pl_alone) == set(pl_batch) and pl_alone
            for pid in pl_batch:
                assert np.abs(pl_batch[pid][i]).max() > 0
                np.testing.assert_array_equal(pl_alone[pid][0], pl_batch[pid][i])


@pytest.mark.parametrize('batch', BATCHES)
def test_a_mixed_block_runs_both_ways(tiered, batch):
    eng = tiered.engine
    theta = _walkers(eng, batch)
    c_in, m_in = _eval(eng, theta)
    stray = batch - 2                                           # (B = 65: the second slot of a full pair of the two-walker kernel)
    mixed = theta.copy()
    mixed[stray, eng.low.slot['L0_hcd']] = 55.0                 # beyond the validated 40 Mpc/h: the plain loop for this walker
    c_mix, m_mix = _eval(eng, mixed)
    keep = np.arange(batch) != stray
    np.testing.assert_array_equal(c_mix[keep], c_in[keep])
    np.testing.assert_array_equal(m_mix[keep], m_in[keep])
    assert c_mix[stray] != c_in[stray]
    assert not eng.set_mu_quadrature(False)
    try:
        c_loop, m_loop = _eval(eng, mixed)
    finally:
        assert eng.set_mu_quadrature(True)
    np.testing.assert_array_equal(m_mix[stray], m_loop[stray])
    np.testing.assert_array_equal(c_mix[stray], c_loop[stray])
