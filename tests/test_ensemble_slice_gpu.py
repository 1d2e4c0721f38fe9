"""Ensemble slice sampling on the GPU (vmx_ensemble_run_slice: k_ens_slice_advance, k_ens_slice_emit): the device driver against
the NumPy restatement over the same engine - positions, chain, moved counters, scale and all eight counts equal, lnL to rtol 1e-12 -
at the sizes where the kernels take another path (H = 2, a block of 64 lanes, H beyond a work-group's 1024 lanes with rows over
several chunks); a set against ``python`` and against its single runs; a run cut into calls; the exact Gaussian posterior of four
linear parameters; every refusal; the settings end to end and ``sample_mocks``."""
import configparser
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']


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
    from vega_amd import EnsembleSampler
    out = []
    for driver in ('device', 'python'):
        s = EnsembleSampler(vega, W, seed=seed, driver=driver, sample_params=sp, moves='slice', **kw).run(steps)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    assert np.array_equal(dev.x, py.x) and np.array_equal(dev.get_chain(), py.get_chain())
    assert np.array_equal(dev.accepted, py.accepted) and np.array_equal(dev.mu, py.mu)
    assert np.array_equal(dev.slice_counts, py.slice_counts), (dev.slice_counts, py.slice_counts)
    np.testing.assert_allclose(dev.get_log_lik(), py.get_log_lik(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(dev.lnl, py.lnl, rtol=1e-12, atol=0)
    for key in ('proposals', 'accepted', 'moves', 'rounds', 'steps'):
        assert dev.stats[key] == py.stats[key], key
    assert dev.stats['host_synchronisations'] == dev.stats['rounds'] + dev.stats['calls']
    sl = dev.stats['slice']
    assert sl['updates'] == dev.stats['proposals'] and sl['moved'] == dev.stats['accepted'] == int(dev.accepted.sum())
    assert 0 < sl['moved'] <= sl['updates'] and sl['rows'] > sl['updates']


def test_drivers_agree_on_auto(auto_vega):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, 64, 20, sp, tune_steps=10)
    _assert_same(dev, py)
    assert dev.stats['calls'] == 1 and dev.stats['host_synchronisations'] == dev.stats['rounds'] + 1
    assert dev.get_chain().shape == (20, 64, 4) and dev.stats['proposals'] == 20 * 64 and dev.mu[0] != 1.0
    assert dev.stats['moves'] == {'slice': dict(proposals=20 * 64, accepted=dev.stats['slice']['moved'])}
    print('auto: rows per update', dev.stats['slice']['rows_per_update'], 'mu', dev.stats['mu'], 'rounds', dev.stats['rounds'],
          {k: dev.stats['slice'][k] for k in ('expansions', 'contractions', 'box', 'failed', 'capped')})
    # the scale is tuned for the steps below tune_steps alone
    frozen = _pair(auto_vega, 64, 3, sp, tune_steps=0)[0]
    assert frozen.mu[0] == 1.0


@pytest.mark.parametrize('names, W, steps', [(AUTO_SAMPLED[:2], 4, 20), (AUTO_SAMPLED, 8, 10), (AUTO_SAMPLED, 2112, 2)])
def test_drivers_agree_at_the_edges(auto_vega, names, W, steps):
    """H = 2: the two partners are the whole other half; H = 4: a block of 64 lanes; H = 1056: beyond the 1024 lanes of a
    work-group, so the lanes stride and the numbering of the requests runs over two strides, the rows over several chunks of
    max_batch = 256."""
    dev, py = _pair(auto_vega, W, steps, _sample_params(auto_vega, names), tune_steps=steps // 2)
    _assert_same(dev, py)
    assert dev.get_chain().shape == (steps, W, len(names))
    assert dev.stats['engine_calls'] == py.stats['engine_calls']
    if W == 2112:
        assert dev.stats['engine_calls'] > dev.stats['rounds']         # (a round's rows took several chunks)


def test_a_set_against_python_and_against_its_single_runs(auto_vega):
    from vega_amd import EnsembleSampler, EnsembleSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    streams = [4, 1, 2]
    sets = [EnsembleSet(auto_vega, 3, 32, streams=streams, seed=7, sample_params=sp, moves='slice', tune_steps=6, driver=d).run(12)
            for d in ('device', 'python')]
    dev, py = sets
    assert dev.driver == 'device' and py.driver == 'python' and dev.stats['calls'] == 1
    _assert_same(dev, py)
    assert np.array_equal(dev.per_ensemble, py.per_ensemble) and len({float(m) for m in dev.mu}) == 3
    for e, stream in enumerate(streams):
        one = EnsembleSampler(auto_vega, 32, stream=stream, seed=7, sample_params=sp, moves='slice', tune_steps=6).run(12)
        member = dev.member(e)
        assert np.array_equal(member.get_chain(), one.get_chain()) and np.array_equal(member.accepted, one.accepted)
        np.testing.assert_allclose(member.get_log_lik(), one.get_log_lik(), rtol=1e-12, atol=0)
        assert np.array_equal(member.slice_counts, one.slice_counts) and member.stats['mu'] == one.stats['mu']
    solo = EnsembleSet(auto_vega, 1, 32, streams=[4], seed=7, sample_params=sp, moves='slice', tune_steps=6).run(12)
    one = EnsembleSampler(auto_vega, 32, stream=4, seed=7, sample_params=sp, moves='slice', tune_steps=6).run(12)
    assert np.array_equal(solo.get_chain()[0], one.get_chain()) and np.array_equal(solo.get_log_lik()[0], one.get_log_lik())
    assert np.array_equal(solo.accepted[0], one.accepted) and solo.mu[0] == one.mu[0]


def test_chain_is_independent_of_the_cut(auto_vega):
    """A cut inside the tuning and one after it; thinning counts from the start of the run."""
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    one = EnsembleSampler(auto_vega, 32, seed=3, thin=2, sample_params=sp, moves='slice', tune_steps=8).run(18)
    two = EnsembleSampler(auto_vega, 32, seed=3, thin=2, sample_params=sp, moves='slice', tune_steps=8, segment=5).run(11).run(7)
    assert np.array_equal(one.get_chain(), two.get_chain()) and np.array_equal(one.get_log_lik(), two.get_log_lik())
    assert np.array_equal(one.accepted, two.accepted) and one.mu[0] == two.mu[0] and one.get_chain().shape == (9, 32, 4)
    assert np.array_equal(one.slice_counts, two.slice_counts) and one.stats['calls'] == 1 and two.stats['calls'] == 5
    assert two.stats['host_synchronisations'] == two.stats['rounds'] + 5


def _linear_posterior(vega):
    """The exact Gaussian posterior of four broadband coefficients (chi2 = (b - b*)^T F (b - b*) + const, F and b* from the
    engine's chi2 at unit offsets): (names, mean, cov)."""
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
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
    F, g = fit(1.0 / np.sqrt(np.diag(F)))           # (again with offsets of the posterior's own size)
    cov = np.linalg.inv(F)
    return names, b0 - 0.5 * cov @ g, cov


def test_linear_parameters_sample_the_exact_gaussian_posterior(auto_vega):
    """W = 64, 400 steps, the first 100 tune mu, 150 discarded: mean and covariance of the chain within 5 standard errors of an
    effective sample size N / tau_max, tau from the chain; no update capped; and the engine's rows are the walkers' requests: every
    trial point is a row or a box answer, none a walker's own position."""
    from vega_amd import EnsembleSampler
    names, mean, cov = _linear_posterior(auto_vega)
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 30 * s, m + 30 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    W, steps, burn = 64, 400, 150
    s = EnsembleSampler(auto_vega, W, seed=11, sample_params=sp, moves='slice', tune_steps=100).run(steps)
    assert s.driver == 'device'
    post = s.get_chain(discard=burn)
    tau = s.get_autocorr_time(discard=burn)
    flat = post.reshape(-1, len(names))
    n_eff = flat.shape[0] / tau.max()
    sl = s.stats['slice']
    print('tau', tau, 'n_eff', n_eff, 'mu', s.stats['mu'], 'rows per update', sl['rows_per_update'], 'rounds', s.stats['rounds'],
          'seconds', s.stats['seconds'], {k: sl[k] for k in ('expansions', 'contractions', 'box', 'failed', 'capped')})
    assert n_eff > 100, tau
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - mean) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - cov) < tol), ((np.cov(flat.T) - cov) / np.outer(sd, sd), n_eff)
    assert sl['capped'] == 0 and sl['moved'] == sl['updates'] == steps * W and sl['failed'] == 0
    # every trial point is a request or a box answer: two ends and the accepted point per update, one more per expansion (no side
    # reached its cap of 32: the expansions of one update would show) and per contraction
    assert sl['rows'] + sl['box'] == 3 * sl['updates'] + sl['expansions'] + sl['contractions']
    # (a round's rows, at most 32, are one chunk, and the last round - the last half is over - has none: no other row is evaluated)
    assert s.stats['engine_calls'] == s.stats['rounds'] - 1


def _call(eng, W=8, cols=2, E=2, slice_=(1.0, 10, 32, 64, 0), mu=1.0, null_slice=False, null_mu=False, **over):
    """vmx_ensemble_run_slice at the ctypes level."""
    from vega_amd import engine
    names = ['bias_eta_LYA', 'beta_LYA'][:cols]
    x = np.tile(np.array([[-0.2, 1.67][:cols]]), (E, W, 1)) + 1e-3 * np.arange(W)[None, :, None]
    lnl, acc = np.zeros((E, W)), np.zeros((E, W), dtype=np.int64)
    kw = dict(step0=0, n_steps=3, thin=1)
    kw.update(over)
    spec, args, chain, chain_lnl, stats, _held = eng._ensemble_arrays(
        3, [eng.names.index(n) for n in names], [-0.5, 0.5][:cols], [0.0, 3.0][:cols], eng.low.theta0.copy(), x, lnl, acc, kw['step0'],
        kw['n_steps'], kw['thin'], True, a=0.5, log_norm=0.0, seed=1, stream=0, const_hint=-1, chunk=0, lanes=0)
    streams = np.arange(E, dtype=np.uint64)
    mus = np.full(E, float(mu)) if np.isscalar(mu) else np.array(mu, dtype=np.float64)
    sl = engine.EnsembleSlice(*slice_)
    counts = np.zeros((E, 8), dtype=np.int64)
    rc = eng.lib.vmx_ensemble_run_slice(eng._h, C.byref(spec), E, W, streams.ctypes.data_as(C.POINTER(C.c_uint64)), None, *args,
                                        C.byref(stats), None if null_slice else C.byref(sl), None if null_mu else engine._dp(mus),
                                        counts.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, stats, counts, mus, x


def test_refusals_leave_the_engine_as_it_was(auto_vega):
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    cases = [dict(W=2, cols=1), dict(slice_=(0.0, 10, 32, 64, 0)), dict(slice_=(-1.0, 10, 32, 64, 0)), dict(slice_=(np.inf, 10, 32, 64, 0)),
             dict(slice_=(np.nan, 10, 32, 64, 0)), dict(mu=0.0), dict(mu=[1.0, -2.0]), dict(mu=[np.nan, 1.0]), dict(mu=[1.0, np.inf]),
             dict(slice_=(1.0, -1, 32, 64, 0)), dict(slice_=(1.0, 10, 0, 64, 0)), dict(slice_=(1.0, 10, 33, 64, 0)),
             dict(slice_=(1.0, 10, 32, 0, 0)), dict(slice_=(1.0, 10, 32, 65, 0)), dict(slice_=(1.0, 10, 32, 64, 1)),
             dict(slice_=(1.0, 10, 32, 64, -1)), dict(null_slice=True), dict(null_mu=True),
             dict(W=7), dict(W=2), dict(thin=0), dict(n_steps=-1), dict(step0=-1)]       # (... and what the set refuses)
    for case in cases:
        rc, _, counts, _, _ = _call(eng, **case)
        assert rc == -1 and b'invalid argument' in eng.lib.vmx_last_error() and not counts.any(), case
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # the smallest run there is goes through, the stretch scale is not read (a = 0.5 above), and the caps may be 1
    rc, stats, counts, mus, x = _call(eng, W=4, slice_=(1.0, 2, 1, 1, 0))
    assert rc == 0 and stats.steps == 3 and stats.proposals == 2 * 3 * 4 == counts[:, 0].sum() and stats.accepted == counts[:, 1].sum()
    assert stats.host_synchronisations >= 2 and np.all(counts[:, 3] <= 2 * counts[:, 0]) and np.all(counts[:, 4] <= counts[:, 0])
    rc, stats, counts, mus, x = _call(eng, n_steps=0)
    assert rc == 0 and stats.host_synchronisations == 1 and not counts.any() and np.all(mus == 1.0)
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    from vega_amd import EnsembleSampler, TemperedEnsemble
    sp = _sample_params(auto_vega, AUTO_SAMPLED[:2])
    with pytest.raises(ValueError, match='mixture'):
        EnsembleSampler(auto_vega, 8, sample_params=sp, moves=[('slice', 0.5), ('stretch', 0.5)])
    with pytest.raises(ValueError, match='tempering'):
        TemperedEnsemble(auto_vega, 8, ntemps=3, sample_params=sp, moves='slice')


def test_sample_mocks_passes_slice_on():
    """``MonteCarlo.sample_mocks(moves='slice', ...)``: the set it runs is the ``EnsembleSet`` with those settings over the same
    mock pools, bit for bit, device and python alike, and another chain than the stretch move's."""
    from vega_amd import EnsembleSet, VegaInterface, synthetic
    from vega_amd.montecarlo import MonteCarlo
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=64)
    try:
        sp = _sample_params(vega, AUTO_SAMPLED)
        mc = MonteCarlo(vega)
        ran = mc.sample_mocks(num_mocks=2, walkers=8, steps=9, seed=3, sample_params=sp, moves='slice', mu=0.7, tune_steps=4)
        assert ran.driver == 'device' and ran.slice == dict(mu0=0.7, tune_steps=4) and mc.mc_posteriors['moves'] == 'slice'
        assert np.array_equal(mc.mc_posteriors['mu'], ran.mu) and ran.stats['slice']['updates'] == 2 * 9 * 8
        by_hand = [EnsembleSet(vega, 2, 8, mock_rows=[0, 1], seed=3, sample_params=sp, moves='slice', mu=0.7, tune_steps=4, driver=d).run(9)
                   for d in ('device', 'python')]
        assert np.array_equal(ran.get_chain(), by_hand[0].get_chain()) and np.array_equal(ran.get_log_lik(), by_hand[0].get_log_lik())
        assert by_hand[1].driver == 'python'
        _assert_same(*by_hand)
        assert not np.array_equal(ran.get_chain()[0], ran.get_chain()[1])
        plain = EnsembleSet(vega, 2, 8, mock_rows=[0, 1], seed=3, sample_params=sp).run(9)
        assert not np.array_equal(plain.get_chain(), ran.get_chain())
        with pytest.raises(ValueError, match='moves'):
            mc.sample_mocks(num_mocks=2, sampler='smc', moves='slice')
    finally:
        vega.close()


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import run_vega_sampler
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Ensemble'] = {'path': str(out), 'name': 'auto_chain', 'walkers': '8', 'steps': '12', 'thin': '3', 'seed': '4',
                       'moves': 'slice', 'slice_tune_steps': '6'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert sampler.driver == 'device' and sampler.slice == dict(mu0=1.0, tune_steps=6)
        table = np.loadtxt(out / 'auto_chain.txt')
        assert table.shape == (12 // 3 * 8, 2 + 2)
        assert np.all(table[:, 0] == 1.0)
        np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True))
        np.testing.assert_array_equal(table[:, 2:], sampler.get_chain(flat=True))
        assert (out / 'auto_chain.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
        assert sampler.stats['moves']['slice']['proposals'] == 12 * 8 and sampler.stats['accepted'] > 0
        assert sampler.stats['slice']['rows'] > 0 and sampler.stats['mu'] != 1.0
    finally:
        sampler.vega.close()
