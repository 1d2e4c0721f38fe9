"""Many ensembles in one device run (include/vegamx.h: vmx_ensemble_run_many, vega_amd/ensemble.py: EnsembleSet) on real engines:
one ensemble is the existing sampler bit for bit; the device driver makes the chains of the NumPy restatement for shared data and
for one mock per ensemble, for blocks far below a wave and beyond 1024 threads; the chains do not depend on how a run is cut; every
mock's chain samples that mock's exact Gaussian posterior; refused arguments leave the engine as it was; the config switches end
to end."""
import configparser

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
MOCK_ROWS = [4, 0, 0, 2]


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


@pytest.fixture(scope='module')
def mock_vega():
    """The auto problem with the synthetic covariance (mocks are drawn from one) and a pool of 6 mocks on its engine:
    (interface, the mocks)."""
    from vega_amd import VegaInterface, synthetic
    from vega_amd.montecarlo import MonteCarlo
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=256)
    vega.freeze_metals()
    mocks = MonteCarlo(vega).create_mocks(vega.compute_model(), 6, seed=1)
    for name, pool in mocks.items():
        vega.engine.set_mock_pool(name, pool)
    yield vega, mocks
    vega.close()


def _pair(vega, E, W, steps, sp, seed=7, **kw):
    from vega_amd import EnsembleSet
    out = []
    for driver in ('device', 'python'):
        s = EnsembleSet(vega, E, W, seed=seed, driver=driver, sample_params=sp, **kw).run(steps)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    assert np.array_equal(dev.accepted, py.accepted)
    assert np.array_equal(dev.get_chain(), py.get_chain())
    np.testing.assert_allclose(dev.get_log_lik(), py.get_log_lik(), rtol=1e-12, atol=0)
    assert np.array_equal(dev.per_ensemble, py.per_ensemble)
    assert np.array_equal(dev.per_ensemble[:, 0], dev.accepted.sum(axis=1))
    for key in ('accepted', 'rejected_outside_box', 'rejected_failed_model', 'proposals'):
        assert dev.stats[key] == py.stats[key], key
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']


def test_one_ensemble_is_the_existing_sampler(auto_vega):
    """One kernel and one host routine serve both: this holds the two exported entries (vmx_ensemble_run, vmx_ensemble_run_many
    with E = 1) and the two Python classes over them to one chain."""
    from vega_amd import EnsembleSampler, EnsembleSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    both = EnsembleSet(auto_vega, 1, 64, streams=[3], seed=7, sample_params=sp).run(30)
    one = EnsembleSampler(auto_vega, 64, stream=3, seed=7, sample_params=sp).run(30)
    assert both.driver == one.driver == 'device'
    assert both.get_chain().shape == (1, 30, 64, 4)
    assert np.array_equal(both.get_chain()[0], one.get_chain())
    assert np.array_equal(both.get_log_lik()[0], one.get_log_lik())
    assert np.array_equal(both.accepted[0], one.accepted)
    member = both.member(0)
    assert np.array_equal(member.get_chain(flat=True), one.get_chain(flat=True)) and member.stats['accepted'] == one.stats['accepted']
    assert np.array_equal(member.acceptance_fraction, one.acceptance_fraction)


def _entry_state(vega):
    """A start inside the box of two sampled columns, W = 8, with the lnL of its rows (log_norm = 0): (cols, lo, hi, theta_fixed,
    x, lnl)."""
    eng = vega.engine
    cols = [eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')]
    lo, hi = np.array([-0.5, 0.5]), np.array([0.0, 3.0])
    x = np.array([-0.2, 1.67]) + 0.01 * np.random.default_rng(2).standard_normal((8, 2))
    assert np.all(x >= lo) and np.all(x <= hi)
    theta = eng.low.theta0.copy()
    rows = np.repeat(theta[None, :], 8, axis=0)
    rows[:, cols] = x
    return cols, lo, hi, theta, x, -0.5 * np.asarray(vega.chi2_batch(rows), dtype=np.float64)


def test_the_two_entries_are_one_routine(auto_vega):
    """ctypes level: `ensemble_run(stream=3)` and `ensemble_run_many(streams=[3])` from the same start, from a step0 that is no
    multiple of thin - the same chain, state and counters bit for bit; the forwarder passes the stream on (stream 4 is another
    chain); without the chain kept the final state is the same."""
    eng = auto_vega.engine
    cols, lo, hi, theta, x0, lnl0 = _entry_state(auto_vega)
    kw = dict(step0=3, n_steps=8, thin=3)

    def single(stream, **more):
        x, lnl, acc = x0.copy(), lnl0.copy(), np.zeros(8, dtype=np.int64)
        chain, chain_lnl, st = eng.ensemble_run(cols, lo, hi, theta, x, lnl, acc, stream=stream, **kw, **more)
        return chain, chain_lnl, x, lnl, acc, st

    chain, chain_lnl, x, lnl, acc, st = single(3)
    xm, lnlm, accm = x0[None].copy(), lnl0[None].copy(), np.zeros((1, 8), dtype=np.int64)
    chain_m, chain_lnl_m, st_m = eng.ensemble_run_many(cols, lo, hi, theta, xm, lnlm, accm, streams=[3], **kw)
    # (steps 3 .. 10, thin 3: the rows after steps 6 and 9)
    assert chain.shape == (2, 8, 2) and chain_m.shape == (1, 2, 8, 2) and chain_lnl_m.shape == (1, 2, 8)
    assert np.array_equal(chain, chain_m[0]) and np.array_equal(chain_lnl, chain_lnl_m[0])
    assert np.array_equal(x, xm[0]) and np.array_equal(lnl, lnlm[0]) and np.array_equal(acc, accm[0])
    assert (st['accepted'], st['rejected_outside_box'], st['rejected_failed_model']) == tuple(st_m['per_ensemble'][0])
    assert 0 < st['accepted'] == acc.sum() and st['proposals'] == st_m['proposals'] == 8 * 8
    assert not np.array_equal(single(4)[0], chain)
    none, none_lnl, x_k, lnl_k, acc_k, _ = single(3, keep_chain=False)
    assert none is None and none_lnl is None
    assert np.array_equal(x_k, x) and np.array_equal(lnl_k, lnl) and np.array_equal(acc_k, acc)


def test_drivers_agree_on_shared_data(auto_vega):
    """E = 5, W = 64: 160 rows per half in chunks of 48 - chunk boundaries inside ensembles and a tail of 16 rows."""
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, 5, 64, 20, sp, chunk=48)
    _assert_same(dev, py)
    assert dev.stats['host_synchronisations'] == dev.stats['calls'] == 1
    assert dev.stats['engine_calls'] == 20 * 2 * 4
    assert dev.get_chain().shape == (5, 20, 64, 4) and dev.get_log_lik().shape == (5, 20, 64)
    chains = dev.get_chain()
    assert all(not np.array_equal(chains[0], chains[e]) for e in range(1, 5))


@pytest.mark.parametrize('E, W, steps', [(3, 8, 10), (2, 2112, 3)])
def test_small_and_large_blocks(auto_vega, E, W, steps):
    """H = 4, far below one wave; H = 1056, beyond the 1024 threads of a block: the strided loop."""
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, E, W, steps, sp)
    _assert_same(dev, py)
    assert dev.stats['host_synchronisations'] == 1


@pytest.fixture(scope='module')
def mock_runs(mock_vega):
    """The set of the per-mock tests, both drivers, computed once: E = 4 ensembles on the mock rows 4, 0, 0, 2."""
    vega, _ = mock_vega
    return _pair(vega, 4, 32, 15, _sample_params(vega, AUTO_SAMPLED), mock_rows=MOCK_ROWS)


def test_every_ensemble_reads_its_own_mock(mock_vega, mock_runs):
    from vega_amd import EnsembleSet
    vega, _ = mock_vega
    dev, py = mock_runs
    _assert_same(dev, py)
    chain, lnl = dev.get_chain(), dev.get_log_lik()
    assert not np.array_equal(chain[1], chain[2])               # the same mock, another stream
    again = EnsembleSet(vega, 4, 32, seed=7, streams=[0, 1, 1, 3], mock_rows=MOCK_ROWS,
                        sample_params=_sample_params(vega, AUTO_SAMPLED)).run(15)
    assert np.array_equal(again.get_chain()[1], again.get_chain()[2]) and np.array_equal(again.get_log_lik()[1], again.get_log_lik()[2])
    assert np.array_equal(again.accepted[1], again.accepted[2])
    assert np.array_equal(again.get_chain()[0], chain[0])       # (stream 0 on mock 4 in both sets)
    # the data matter: the same stream on the installed data is another chain
    plain = EnsembleSet(vega, 1, 32, seed=7, streams=[0], sample_params=_sample_params(vega, AUTO_SAMPLED)).run(15)
    assert not np.array_equal(plain.get_log_lik()[0], lnl[0])


def test_chains_are_independent_of_the_cut(mock_vega, mock_runs):
    from vega_amd import EnsembleSet
    vega, _ = mock_vega
    one = mock_runs[0]
    cut = EnsembleSet(vega, 4, 32, seed=7, mock_rows=MOCK_ROWS, segment=5, sample_params=_sample_params(vega, AUTO_SAMPLED)).run(15)
    assert np.array_equal(one.get_chain(), cut.get_chain()) and np.array_equal(one.get_log_lik(), cut.get_log_lik())
    assert np.array_equal(one.accepted, cut.accepted) and np.array_equal(one.per_ensemble, cut.per_ensemble)
    assert np.array_equal(one.x, cut.x) and np.array_equal(one.lnl, cut.lnl)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 3
    assert one.stats['host_synchronisations'] == 1 and cut.stats['host_synchronisations'] == 3


def _linear_gaussian(vega, names):
    """(mean, covariance) of the exact Gaussian posterior of parameters the model is linear in, from the engine's chi2 at unit
    offsets (second differences of a quadratic are exact up to rounding)."""
    cols = [vega.param_names.index(n) for n in names]
    base = vega._theta(None)
    b0 = base[cols].copy()

    def chi2_at(offsets):
        th = np.repeat(base[None, :], len(offsets), axis=0)
        th[:, cols] = b0 + np.asarray(offsets)
        return vega.chi2_batch(th)

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
    F, g = fit(1.0 / np.sqrt(np.diag(F)))        # (again with offsets of the posterior's own size)
    cov = np.linalg.inv(F)
    return b0 - 0.5 * cov @ g, cov


def test_every_mock_samples_its_exact_gaussian_posterior(mock_vega):
    """4 of the additive broadband coefficients, everything else fixed: chi2 against any mock is exactly quadratic in them, the
    posterior of mock m exactly Gaussian with the mean of its best fit and the covariance of its HESSE matrix (the device MIGRAD
    fits of the same pool).  Every mock's chain must agree with its own fit within 5 standard errors of an effective sample size
    N / tau_max; the best fits move by more than a posterior sd from mock to mock, so a set that read another mock's row fails."""
    from vega_amd.ensemble import integrated_time
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega[0]
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    mean, cov = _linear_gaussian(vega, names)
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 30 * s, m + 30 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    M, W, steps, burn = 8, 32, 400, 150
    before = vega.chi2_batch(vega._theta(None)[None, :])
    mc = MonteCarlo(vega)
    vega.freeze_metals()
    # (the mocks scatter about the model at the data's posterior mean: their posteriors lie well inside the box)
    mocks = mc.create_mocks(vega.compute_model(dict(zip(names, mean))), M, seed=1)
    fits = mc._fit_mocks(mocks, M, sample_params=sp)
    assert list(fits.names) == names and np.all(fits.is_valid) and not np.any(fits.hesse_failed)
    best, hesse = fits.values, fits.covariance
    assert np.max(np.ptp(best, axis=0) / sd) > 1.0, np.ptp(best, axis=0) / sd
    sampler = mc.sample_mocks(mocks=mocks, walkers=W, steps=steps, burn=burn, seed=11, sample_params=sp)
    assert sampler.driver == 'device' and sampler.stats['calls'] == 1 and sampler.stats['host_synchronisations'] == 1
    post = sampler.get_chain(discard=burn)
    assert post.shape == (M, steps - burn, W, 4)
    summary = mc.mc_posteriors
    for m in range(M):
        flat = post[m].reshape(-1, 4)
        tau = integrated_time(post[m])
        n_eff = flat.shape[0] / tau.max()
        sd_m = np.sqrt(np.diag(hesse[m]))
        print(f'mock {m}: n_eff {n_eff:.0f}, mean pulls {np.round((flat.mean(axis=0) - best[m]) / (sd_m / np.sqrt(n_eff)), 2)}, '
              f'best fit - data posterior mean {np.round((best[m] - mean) / sd, 2)} sd')
        assert n_eff > 100, (m, tau)
        assert np.all(np.abs(flat.mean(axis=0) - best[m]) < 5 * sd_m / np.sqrt(n_eff)), (m, (flat.mean(axis=0) - best[m]) / sd_m, n_eff)
        tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd_m, sd_m)
        assert np.all(np.abs(np.cov(flat.T) - hesse[m]) < tol), (m, (np.cov(flat.T) - hesse[m]) / np.outer(sd_m, sd_m), n_eff)
        np.testing.assert_allclose(summary['mean'][m], flat.mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(summary['covariance'][m], np.cov(flat.T), rtol=1e-9, atol=1e-9 * sd_m.min()**2)
        np.testing.assert_allclose(summary['n_eff'][m], n_eff, rtol=1e-12)
    assert summary['names'] == names and summary['acceptance'].shape == (M,) and np.all(summary['acceptance'] > 0.1)
    # the engine is as it was: the data's chi2, not a mock's
    np.testing.assert_array_equal(vega.chi2_batch(vega._theta(None)[None, :]), before)


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    E = changes.pop('E', 2)
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), x=np.tile([[-0.2, 1.67]], (E, 8, 1)), lnl=np.zeros((E, 8)),
                accepted=np.zeros((E, 8), dtype=np.int64), streams=np.arange(E), step0=0, n_steps=5)
    args.update(changes)
    for k in ('x', 'lnl'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.ensemble_run_many(**args)


@pytest.fixture()
def bare_vega():
    """An engine no mock pool has been installed on."""
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=16)
    yield vega
    vega.close()


def test_refused_arguments_leave_the_engine_as_it_was(bare_vega, mock_vega):
    outside = np.tile([[-0.2, 1.67]], (2, 8, 1))
    outside[1, 7, 0] = 0.2                      # (the last walker of the last ensemble)
    for name, pool in mock_vega[1].items():     # (6 mocks, whatever ran before)
        mock_vega[0].engine.set_mock_pool(name, pool)
    for vega, cases in ((bare_vega, [dict(E=0), dict(streams=None), dict(mock_rows=[0, 0]),        # (no pool on this engine)
                                     dict(x=np.tile([[-0.2, 1.67]], (2, 7, 1)), lnl=np.zeros((2, 7)),
                                          accepted=np.zeros((2, 7), dtype=np.int64)),               # W odd
                                     dict(x=outside), dict(lnl=np.where(np.arange(16).reshape(2, 8) == 15, np.nan, 0.0)),
                                     dict(thin=0), dict(a=1.0)]),
                        (mock_vega[0], [dict(E=1, mock_rows=[6]), dict(E=1, mock_rows=[-1]), dict(mock_rows=[0, 6])])):
        theta = vega._theta(None)[None, :]
        before = vega.chi2_batch(theta)
        for case in cases:
            _refused(vega.engine, **case)
            np.testing.assert_array_equal(vega.chi2_batch(theta), before)
    # (what was refused runs once the argument is mended: the pool has rows 0 .. 5)
    eng = mock_vega[0].engine
    x, lnl, acc = np.tile([[-0.2, 1.67]], (1, 8, 1)), np.zeros((1, 8)), np.zeros((1, 8), dtype=np.int64)
    _, _, st = eng.ensemble_run_many([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0],
                                     eng.low.theta0.copy(), x, lnl, acc, [0], 0, 2, mock_rows=[5])
    assert st['steps'] == 2 and st['per_ensemble'].shape == (1, 3)


def _write_config(tmp_path, tag, control, section):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control'].update(dict(control, run_sampler='True', sampler='Ensemble'))
    out = tmp_path / f'chains_{tag}'
    out.mkdir()
    cfg['Ensemble'] = dict(section, path=str(out), name='run')
    (tmp_path / 'configs' / tag).mkdir(parents=True)
    with open(tmp_path / 'configs' / tag / 'main.ini', 'w') as f:
        cfg.write(f)
    return f'configs/{tag}/main.ini', out


def test_a_posterior_for_every_mock_end_to_end(tmp_path):
    from conftest import mc_launcher_config
    from fits_standard import check_file
    from vega_amd import fitslite, run_vega_sampler
    # (the auto correlation on a data file that carries a covariance, run_montecarlo = True and a [monte carlo] section)
    config = mc_launcher_config(tmp_path)
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / config)
    cfg['control'].update(run_sampler='True', sampler='Ensemble')
    out = tmp_path / 'chains_mocks'
    out.mkdir()
    cfg['Ensemble'] = dict(path=str(out), name='run', mocks='3', walkers='8', steps='12', thin='3', seed='4')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert sampler.E == 3 and sampler.driver == 'device' and sampler.mock_rows.tolist() == [0, 1, 2]
        tables = [np.loadtxt(out / f'run_mock{m}.txt') for m in range(3)]
        for m, table in enumerate(tables):
            assert table.shape == (12 // 3 * 8, 2 + 3) and np.all(table[:, 0] == 1.0)
            np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True)[m])
            np.testing.assert_array_equal(table[:, 2:], sampler.get_chain(flat=True)[m])
        assert not np.array_equal(tables[0], tables[1])
        assert (out / 'run.paramnames').read_text().splitlines() == ['ap ap', 'at at', 'bias_eta_LYA bias_eta_LYA']
        check_file(out / 'mock_posteriors.fits')
        with fitslite.open(str(out / 'mock_posteriors.fits')) as hdus:
            data = hdus[1].data
            assert len(data) == 3
            post = sampler.vega.analysis.mc_posteriors
            np.testing.assert_array_equal(data['ap_mean'], post['mean'][:, 0])
            np.testing.assert_array_equal(data['at_sd'], post['sd'][:, 1])
            np.testing.assert_array_equal(data['at_tau'], post['tau'][:, 1])
            np.testing.assert_array_equal(data['acceptance'], post['acceptance'])
            np.testing.assert_array_equal(data['bias_eta_LYA_mean'], post['mean'][:, 2])
            np.testing.assert_array_equal(np.asarray(data['covariance']).reshape(3, 3, 3), post['covariance'])
    finally:
        sampler.vega.close()


def test_replicas_together_end_to_end(tmp_path):
    from vega_amd import replicas as rep
    from vega_amd import run_vega_sampler
    config, out = _write_config(tmp_path, 'together', {}, dict(replicas='2', together='True', walkers='8', steps='12', thin='3', seed='4'))
    run = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, rank=0, world_size=1)
    vega = run.samplers[0].vega
    try:
        config_seq, out_seq = _write_config(tmp_path, 'sequential', {}, dict(replicas='2', walkers='8', steps='12', thin='3', seed='4'))
        assert run.replicas == 2 and len(run.samplers) == 2
        recs = [rep.load_record(rep.record_path(out, 'run', r)) for r in range(2)]
        seq = run_vega_sampler(config_seq, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, rank=0, world_size=1)
        try:
            recs_seq = [rep.load_record(rep.record_path(out_seq, 'run', r)) for r in range(2)]
        finally:
            seq.samplers[0].vega.close()
        for r, (rec, want) in enumerate(zip(recs, recs_seq)):
            assert set(rec) == set(want) and set(rec['stats']) == set(want['stats'])            # the same keys as today
            assert rec['stream'] == r and rec['kind'] == 'ensemble' and rec['chain'].shape == (4, 8, 2) == want['chain'].shape
            assert rec['steps'] == 12 and rec['thin'] == 3 and rec['walkers'] == 8 and rec['seed'] == 4
        for k in range(2):
            table = np.loadtxt(out / f'run_{k + 1}.txt')
            assert table.shape == (4 * 8, 4) and np.array_equal(table[:, 2:], recs[k]['chain'].reshape(-1, 2))
        assert (out / 'run.paramnames').exists() and (out / 'run.stats').exists()
        assert np.all(np.isfinite(run.merged['rhat']))
        assert not np.array_equal(recs[0]['chain'], recs[1]['chain'])
    finally:
        vega.close()
