"""The ensemble sampler's parallel tempering on the device (include/vegamx.h: vmx_ensemble_run_pt, the kernels k_ens_half_pt and
k_ens_swap) against the NumPy restatement (the `python` driver of vega_amd/ensemble.py) on real engines: the chains of all rungs,
the counters and the swap counts bit for bit at small halves, beyond the 1024 threads of a block and for two ladders on two mocks;
the cold rung without swaps equal to the single sampler; swaps that change the chain; a chain that does not depend on the cut;
refused ladders that leave the engine as it was; the exact Gaussian posteriors of linear parameters on the cold, a warm and the
last rung with the exact evidence; the config switch end to end."""
import configparser
import math

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
ALL_THREE = [('stretch', .3), ('de', .4), ('snooker', .3)]
MIXTURE = [('de', 0.8), ('snooker', 0.2)]


def _sample_params(vega, names):
    defaults = {'bias_eta_LYA': ((-0.5, 0.0), 0.01), 'beta_LYA': ((0.5, 3.0), 0.05), 'ap': ((0.5, 1.5), 0.01), 'at': ((0.5, 1.5), 0.01)}
    return {'limits': {n: defaults[n][0] for n in names}, 'values': {n: vega.params[n] for n in names},
            'errors': {n: defaults[n][1] for n in names}}


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _pair(vega, W, steps, sp, seed=7, **kw):
    from vega_amd import TemperedEnsemble
    out = []
    for driver in ('device', 'python'):
        s = TemperedEnsemble(vega, W, seed=seed, driver=driver, sample_params=sp, **kw).run(steps)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    assert np.array_equal(dev.get_chain(rung=None), py.get_chain(rung=None))
    assert np.array_equal(dev.accepted, py.accepted) and np.array_equal(dev.x, py.x)
    assert np.array_equal(dev.per_ensemble, py.per_ensemble) and np.array_equal(dev.swaps, py.swaps)
    np.testing.assert_allclose(dev.get_log_lik(rung=None), py.get_log_lik(rung=None), rtol=1e-12, atol=0)
    np.testing.assert_allclose(dev.lnl, py.lnl, rtol=1e-12, atol=0)
    for key in ('accepted', 'rejected_outside_box', 'rejected_failed_model', 'proposals', 'swaps_proposed', 'swaps_accepted'):
        assert dev.stats[key] == py.stats[key], key
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']
    assert dev.stats['host_synchronisations'] == dev.stats['calls'] == 1


@pytest.mark.parametrize('moves', [None, ALL_THREE], ids=str)
@pytest.mark.parametrize('swap_every', [1, 3])
def test_drivers_agree_on_a_ladder_of_three(auto_vega, swap_every, moves):
    """T = 3, W = 8 (H = 4: one block of 64 threads), 12 steps."""
    dev, py = _pair(auto_vega, 8, 12, _sample_params(auto_vega, AUTO_SAMPLED), betas=[1.0, 0.3, 0.0], swap_every=swap_every, moves=moves)
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 3, 12, 8, 4)
    assert np.all(dev.swaps[:, :, 0] == 12 // swap_every * 8) and dev.stats['swaps_accepted'] > 0
    assert dev.stats['engine_calls'] == 12 * 2


def test_drivers_agree_with_the_snooker_at_a_half_of_three(auto_vega):
    """T = 2, W = 6, n = 2: the snooker's three partners are the whole other half."""
    dev, py = _pair(auto_vega, 6, 12, _sample_params(auto_vega, AUTO_SAMPLED[:2]), ntemps=2, moves='snooker')
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 2, 12, 6, 2) and np.array_equal(dev.betas, [1.0, 0.0])


def test_drivers_agree_beyond_a_block(auto_vega):
    """T = 2, W = 2112: the swap kernel's strided loop over 2112 pairs with 1024 threads, the half-step's over 1056; the 2112
    rows of a half-step in 9 chunks of max_batch = 256 (5 per rung-half, were the rungs apart)."""
    dev, py = _pair(auto_vega, 2112, 3, _sample_params(auto_vega, AUTO_SAMPLED), betas=[1.0, 0.5], moves=MIXTURE)
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 2, 3, 2112, 4) and dev.stats['engine_calls'] == 3 * 2 * 9
    assert np.array_equal(dev.swaps[0, 0], [3 * 2112, dev.stats['swaps_accepted']]) and dev.stats['swaps_accepted'] > 2112


def test_drivers_agree_on_two_ladders_with_two_mocks():
    from vega_amd import VegaInterface, synthetic
    from vega_amd.montecarlo import MonteCarlo
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=256)
    try:
        vega.freeze_metals()
        mocks = MonteCarlo(vega).create_mocks(vega.compute_model(), 3, seed=1)
        for name, pool in mocks.items():
            vega.engine.set_mock_pool(name, pool)
        kw = dict(betas=[1.0, 0.3, 0.0], ladders=2, mock_rows=[2, 0], moves=ALL_THREE)
        dev, py = _pair(vega, 8, 12, _sample_params(vega, AUTO_SAMPLED), **kw)
        _assert_same(dev, py)
        assert dev.get_chain(rung=None).shape == (2, 3, 12, 8, 4) and np.all(dev.swaps[:, :, 1] > 0)
        assert np.array_equal(dev.streams.reshape(2, 3), [[0, 1, 2], [64, 65, 66]])
        other = _pair(vega, 8, 12, _sample_params(vega, AUTO_SAMPLED), **dict(kw, mock_rows=[2, 1]))[0]
        assert np.array_equal(other.get_chain(rung=0, ladder=0), dev.get_chain(rung=0, ladder=0))
        assert not np.array_equal(other.get_log_lik(rung=0, ladder=1), dev.get_log_lik(rung=0, ladder=1))
    finally:
        vega.close()


def test_the_cold_rung_without_swaps_is_the_single_sampler_and_swaps_change_it(auto_vega):
    from vega_amd import EnsembleSampler, TemperedEnsemble
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    for moves in (None, MIXTURE):
        free = TemperedEnsemble(auto_vega, 32, betas=[1.0, 0.3, 0.0], swap_every=0, streams=[[5, 6, 7]], seed=7, sample_params=sp,
                                moves=moves).run(20)
        one = EnsembleSampler(auto_vega, 32, seed=7, stream=5, sample_params=sp, moves=moves).run(20)
        assert free.driver == one.driver == 'device'
        assert np.array_equal(free.get_chain(), one.get_chain()) and np.array_equal(free.rung(0).accepted, one.accepted)
        np.testing.assert_allclose(free.get_log_lik(), one.get_log_lik(), rtol=1e-12, atol=0)
        assert free.stats['swaps_proposed'] == free.stats['swaps_accepted'] == 0
        mixed = TemperedEnsemble(auto_vega, 32, betas=[1.0, 0.3, 0.0], swap_every=1, streams=[[5, 6, 7]], seed=7, sample_params=sp,
                                 moves=moves).run(20)
        assert not np.array_equal(mixed.get_chain(), free.get_chain()) and mixed.stats['swaps_accepted'] > 0
        assert mixed.stats['swaps_proposed'] == 2 * 20 * 32 and mixed.swap_fraction.shape == (1, 2)


def test_chain_is_independent_of_the_cut(auto_vega):
    from vega_amd import TemperedEnsemble
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    kw = dict(ntemps=4, swap_every=3, thin=2, seed=3, sample_params=sp, moves=ALL_THREE)
    one = TemperedEnsemble(auto_vega, 16, **kw).run(20)
    two = TemperedEnsemble(auto_vega, 16, segment=7, **kw).run(20)
    assert np.array_equal(one.get_chain(rung=None), two.get_chain(rung=None)) and np.array_equal(one.get_log_lik(rung=None), two.get_log_lik(rung=None))
    assert np.array_equal(one.accepted, two.accepted) and np.array_equal(one.swaps, two.swaps)
    assert one.get_chain(rung=None).shape == (1, 4, 10, 16, 4) and one.stats['calls'] == 1 and two.stats['calls'] == 3
    assert np.all(one.swaps[:, :, 0] == 6 * 16)


def _refused(eng, betas, T=None, G=1, W=8, **kw):
    from vega_amd.engine import EngineError
    T = len(betas) if T is None else T
    box = dict(cols=[eng.names.index(n) for n in ('bias_eta_LYA', 'beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0], theta_fixed=eng.low.theta0.copy())
    with pytest.raises(EngineError, match='invalid argument'):
        eng.ensemble_run_pt(**box, x=np.tile([[-0.2, 1.67]], (G, T, W, 1)), lnl=np.zeros((G, T, W)),
                            accepted=np.zeros((G, T, W), dtype=np.int64), betas=betas, streams=np.arange(G * T).reshape(G, T), step0=0,
                            n_steps=5, **kw)


def test_refused_ladders_leave_the_engine_as_it_was(auto_vega):
    import ctypes as C
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    before = EnsembleSampler(auto_vega, 16, seed=7, sample_params=sp).run(6)
    eng = auto_vega.engine
    for betas in ([0.5, 0.25], [1.0, 1.0], [1.0, 0.5, 0.5], [1.0, 0.2, 0.4], [1.0, -0.1], [1.0, np.nan], [1.0, np.inf], [np.inf, 0.5],
                  list(np.linspace(1.0, 0.0, 65))):
        _refused(eng, betas)
    _refused(eng, [1.0, 0.5], swap_every=-1)
    _refused(eng, [1.0, 0.5], W=7)                                   # (what the plain run refuses)
    _refused(eng, [1.0, 0.5], moves=dict(weights=(0.0, -1.0, 1.0), gamma0=0.8, sigma=1e-5, gamma_s=1.7))
    # through ctypes: no ladder, no rung, no ladders, and G T W beyond int32 - refused before a pointer is read
    spec, args, _, _, stats, _held = eng._ensemble_arrays(
        3, [eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0], eng.low.theta0.copy(),
        np.tile([[-0.2, 1.67]], (2, 8, 1)), np.zeros((2, 8)), np.zeros((2, 8), dtype=np.int64), 0, 5, 1, False, a=2.0, log_norm=0.0, seed=1,
        stream=0, const_hint=-1, chunk=0, lanes=0)
    betas, streams = np.array([1.0, 0.5]), np.arange(2, dtype=np.uint64)
    bp, sp_ = betas.ctypes.data_as(C.POINTER(C.c_double)), streams.ctypes.data_as(C.POINTER(C.c_uint64))
    for G, T, W, b in ((1, 2, 8, None), (1, 0, 8, bp), (0, 2, 8, bp), (1, 65, 8, bp), (2**20, 2, 2**12, bp), (2**30, 2, 8, bp)):
        rc = eng.lib.vmx_ensemble_run_pt(eng._h, C.byref(spec), G, T, W, b, sp_, None, *args[:6], 1, *args[6:], C.byref(stats), None, None,
                                         None)
        assert rc == -1 and b'invalid argument' in eng.lib.vmx_last_error(), (G, T, W)
    after = EnsembleSampler(auto_vega, 16, seed=7, sample_params=sp).run(6)
    assert np.array_equal(before.get_chain(), after.get_chain()) and np.array_equal(before.get_log_lik(), after.get_log_lik())


def _linear_box(auto_vega):
    """The box b* +- 10 sd of the four linear broadband coefficients (chi2 is exactly quadratic in them: F and b* from second
    differences), with the exact log Z over it: lnL(b*) + 1/2 log|2 pi cov| - sum log(20 sd)."""
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    cols = [auto_vega.param_names.index(n) for n in names]
    base = auto_vega._theta(None)
    b0 = base[cols].copy()

    def chi2_at(offsets):
        th = np.repeat(base[None, :], len(offsets), axis=0)
        th[:, cols] = b0 + np.asarray(offsets)
        return auto_vega.chi2_batch(th)

    def fit(delta):
        n = len(cols)
        pts = [np.zeros(n)] + [delta * np.eye(n)[i] for i in range(n)] + [2 * delta * np.eye(n)[i] for i in range(n)]
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        pts += [delta * (np.eye(n)[i] + np.eye(n)[j]) for i, j in pairs]
        c = chi2_at(pts)
        F = np.zeros((n, n))
        for i in range(n):
            F[i, i] = (c[1 + n + i] - 2 * c[1 + i] + c[0]) / (2 * delta[i] ** 2)
        for k, (i, j) in enumerate(pairs):
            F[i, j] = F[j, i] = (c[1 + 2 * n + k] - c[1 + i] - c[1 + j] + c[0]) / (2 * delta[i] * delta[j])
        g = np.array([(c[1 + i] - c[0]) / delta[i] - F[i, i] * delta[i] for i in range(n)])
        return F, g

    F, _ = fit(np.ones(len(cols)))
    sd = 1.0 / np.sqrt(np.diag(F))
    F, g = fit(sd)
    cov = np.linalg.inv(F)
    mean = b0 - 0.5 * cov @ g
    sd = np.sqrt(np.diag(cov))
    lnl_max = float(auto_vega._log_norm()) - 0.5 * float(chi2_at([mean - b0])[0])
    log_z_true = lnl_max + 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1] - np.sum(np.log(20 * sd))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)}, 'values': dict(zip(names, mean)),
          'errors': dict(zip(names, sd))}
    return sp, mean, cov, sd, log_z_true


def test_linear_parameters_sample_the_exact_posteriors_and_give_the_exact_evidence(auto_vega):
    """Four linear broadband coefficients in the box b* +- 10 sd, the ladder 1, 1/2, ..., 1/32, 0, W = 32, 600 steps, the first 150
    dropped, DE 0.8 / snooker 0.2.  The posterior of rung beta is the Gaussian of covariance cov / beta cut to the box: on the
    cold rung mean and covariance, on the rung of 1/4 the covariance 4 cov (the box at +- 5 of its sd), each within 5 standard
    errors of an effective sample size N / tau_max, tau from the rung's chain; the last rung is uniform: its variances are
    (20 sd)^2 / 12, the standard error of a uniform's sample variance being sqrt(0.8 / n_eff) of it ((mu_4 - sigma^4) / sigma^4 =
    144 / 80 - 1).  The stepping-stone evidence lands within 5 err of the exact log Z, with err <= 0.25.

    tau is that of the slots' series, as in the Gaussian tests of the plain ensemble.  On a target of one mode that is the right
    series: a swap is then a move like any other - the walker that comes down from the next rung is a draw of nearly the same
    Gaussian - and there is no weight to be carried between modes, the slow motion a slot's series cannot see on the bimodal
    target of tests/test_ensemble_pt_host.py."""
    from vega_amd import TemperedEnsemble
    sp, mean, cov, sd, log_z_true = _linear_box(auto_vega)
    betas = [1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.0]
    s = TemperedEnsemble(auto_vega, 32, betas=betas, seed=11, sample_params=sp, moves=MIXTURE).run(600)
    assert s.driver == 'device' and s.stats['host_synchronisations'] == s.stats['calls'] == 1
    print('swap fractions', np.round(s.swap_fraction[0], 3))
    assert np.all(s.swaps[:, :, 1] > 0)

    def moments(rung):
        post = s.get_chain(rung=rung, discard=150)
        tau = s.get_autocorr_time(rung=rung, discard=150)
        flat = post.reshape(-1, 4)
        n_eff = flat.shape[0] / tau.max()
        assert n_eff > 100, (rung, tau)
        return flat.mean(axis=0), np.cov(flat.T), n_eff, tau

    m0, c0, n_eff, tau = moments(0)
    print('rung 0: tau', tau, 'n_eff', n_eff, 'mean pulls', (m0 - mean) / (sd / np.sqrt(n_eff)),
          'cov pulls', np.abs(c0 - cov).max() / (np.sqrt(2.0 / n_eff) * sd.max()**2))
    assert np.all(np.abs(m0 - mean) < 5 * sd / np.sqrt(n_eff)), ((m0 - mean) / sd, n_eff)
    assert np.all(np.abs(c0 - cov) < 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)), ((c0 - cov) / np.outer(sd, sd), n_eff)
    m2, c2, n_eff, tau = moments(2)
    print('rung 1/4: tau', tau, 'n_eff', n_eff, 'cov pulls', (c2 - 4 * cov) / (np.sqrt(2.0 / n_eff) * 4 * np.outer(sd, sd)))
    assert np.all(np.abs(c2 - 4 * cov) < 5 * np.sqrt(2.0 / n_eff) * 4 * np.outer(sd, sd)), ((c2 / 4 - cov) / np.outer(sd, sd), n_eff)
    m6, c6, n_eff, tau = moments(6)
    flat_var = (20 * sd)**2 / 12
    print('last rung: tau', tau, 'n_eff', n_eff, 'variance pulls', (np.diag(c6) - flat_var) / (np.sqrt(0.8 / n_eff) * flat_var))
    assert np.all(np.abs(np.diag(c6) - flat_var) < 5 * np.sqrt(0.8 / n_eff) * flat_var), (np.diag(c6) / flat_var, n_eff)
    log_z, err = s.log_evidence(discard=150)
    ti, ti_err = s.log_evidence('ti', discard=150)
    print(f'log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}); ti {ti:.4f} +- {ti_err:.4f}')
    assert abs(log_z - log_z_true) < 5 * err and err <= 0.25


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import TemperedEnsemble, run_vega_sampler
    from vega_amd.ensemble import read_pt_stats
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Ensemble'] = {'path': str(out), 'name': 'auto_chain', 'walkers': '8', 'steps': '12', 'thin': '3', 'seed': '4', 'ntemps': '3'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    said = []
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *a: said.append(' '.join(map(str, a))))
    try:
        assert isinstance(sampler, TemperedEnsemble) and sampler.driver == 'device' and np.array_equal(sampler.betas, [1.0, 0.5, 0.0])
        assert sampler.swap_every == 1 and sampler.stats['swaps_proposed'] == 2 * 12 * 8
        table = np.loadtxt(out / 'auto_chain.txt')
        assert table.shape == (12 // 3 * 8, 2 + 2) and np.all(table[:, 0] == 1.0)
        np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True))
        np.testing.assert_array_equal(table[:, 2:], sampler.get_chain(flat=True))
        assert (out / 'auto_chain.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
        stats = read_pt_stats(out / 'auto_chain.stats')
        log_z, err = sampler.log_evidence()
        assert stats['log(Z)'] == log_z and stats['log(Z) error'] == err and math.isfinite(log_z) and err > 0
        assert stats['beta'] == [1.0, 0.5, 0.0] and stats['steps'] == 12 and len(stats['swap fraction']) == 2
        assert f'log(Z) = {log_z} +- {err}' in said
    finally:
        sampler.vega.close()
