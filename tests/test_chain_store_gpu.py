"""The chain store and its summary on a real engine (include/vegamx.h: vmx_chain_store_*, vega_amd/csrc/vmx_chain.h): a store
alone keeps the bytes it is given through uneven cuts and a ``reserve``, and its summary is ``chain_summary`` bit for bit; attached
to runs it holds the chain the host path returns, for every kind of move, both thins and both drivers; ``run_until`` stops the two
drivers at the same step; ``sample_mocks(summaries='device')`` gives the restatement's numbers without a chain on the host;
refused calls leave engine and store as they were.

The tolerance against the host path's NumPy summaries (``np.mean`` / ``np.cov`` / the FFT estimator) is the one
tests/test_chain_summary_host.py measures and fixes: 3.5e-13, the covariance held to sqrt(C_ii C_jj)."""
import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
RTOL = 3.5e-13


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
    """The auto problem with the synthetic covariance (mocks are drawn from one)."""
    from vega_amd import VegaInterface, synthetic
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=256)
    vega.freeze_metals()
    yield vega
    vega.close()


def _synthetic(E, T, W, n, seed):
    """AR(1) series around 1, phi spread over the columns, and an lnL block."""
    rng = np.random.default_rng(seed)
    phi = np.linspace(0.3, 0.9, n) if n > 1 else np.array([0.6])
    z = np.empty((E, T, W, n))
    e = rng.standard_normal((E, T, W, n))
    z[:, 0] = e[:, 0] / np.sqrt(1.0 - phi**2)
    for t in range(1, T):
        z[:, t] = phi * z[:, t - 1] + e[:, t]
    return 1.0 + 0.05 * z, rng.standard_normal((E, T, W))


def _same_summary(got, ref):
    from vega_amd.ensemble import SUMMARY_KEYS
    assert set(got) == set(SUMMARY_KEYS)
    for key in SUMMARY_KEYS:
        assert np.asarray(got[key]).shape == np.asarray(ref[key]).shape, key
        assert np.asarray(got[key]).tobytes() == np.asarray(ref[key]).tobytes(), key


# ------------------------------------------------------------------ the store alone
def test_the_store_keeps_the_bytes_it_is_given(auto_vega):
    """E = 3, W = 6, n = 3, capacity 64: rows appended in cuts of 5, 7, 1 and 51, a ``reserve`` half-way; ``fetch`` of odd
    sub-ranges returns the bytes put in, and ``summary`` is ``chain_summary`` bit for bit for first rows 0 and 13."""
    from vega_amd.ensemble import chain_summary
    eng = auto_vega.engine
    chain, lnl = _synthetic(3, 64, 6, 3, seed=1)
    store = eng.chain_store(3, 6, 3, 64)
    try:
        assert store.rows == 0
        done = 0
        for k, cut in enumerate((5, 7, 1, 51)):
            if k == 2:
                store.reserve(100)          # (a new allocation: the 12 rows move with it)
                store.reserve(10)           # (never shrinks)
                assert store.capacity == 100
            store.append(chain[:, done:done + cut], lnl[:, done:done + cut])
            done += cut
            assert store.rows == done
        for row0, rows in ((0, 64), (3, 7), (13, 1), (11, 53), (64, 0)):
            got, got_lnl = store.fetch(row0, rows)
            assert got.shape == (3, rows, 6, 3) and got.tobytes() == chain[:, row0:row0 + rows].tobytes()
            assert got_lnl.tobytes() == lnl[:, row0:row0 + rows].tobytes()
        assert store.fetch(5, 9, lnl=False)[1] is None
        for first in (0, 13):
            _same_summary(store.summary(first), chain_summary(chain, first))
        _same_summary(store.summary(13, c=3.5), chain_summary(chain, 13, c=3.5))
        part = store.summary(13, moments=False)
        assert set(part) == {'count', 'tau', 'window', 'n_eff'} and part['tau'].tobytes() == chain_summary(chain, 13)['tau'].tobytes()
        assert set(store.summary(0, tau=False)) == {'count', 'mean', 'sd', 'covariance'}
    finally:
        store.close()


@pytest.mark.parametrize('E, T, W, n', [(1, 2, 2, 1), (2, 257, 6, 64)])
def test_the_summary_at_the_edges(auto_vega, E, T, W, n):
    """The smallest chain, and n at VMX_ENS_MAXN with T one past a power of two: 2080 pairs in chunks of the tile."""
    from vega_amd.ensemble import chain_summary
    chain, lnl = _synthetic(E, T, W, n, seed=2)
    store = auto_vega.engine.chain_store(E, W, n, T)
    try:
        store.append(chain, lnl)
        for first in (0, 1, T - 1):         # (T - 1: a single row - tau = -1, window 0, and a covariance over W points)
            _same_summary(store.summary(first), chain_summary(chain, first))
        assert np.all(store.summary(T - 1)['tau'] == -1.0) and np.all(np.isfinite(store.summary(T - 1)['covariance']))
    finally:
        store.close()


def test_refused_calls_leave_engine_and_store_as_they_were(auto_vega):
    from vega_amd.engine import EngineError
    from vega_amd.ensemble import chain_summary
    eng = auto_vega.engine
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    chain, lnl = _synthetic(2, 10, 8, 2, seed=3)
    for bad in (dict(E=0), dict(W=1), dict(W=1025), dict(n=0), dict(n=65), dict(capacity=-1), dict(capacity=2**62)):
        with pytest.raises(EngineError, match='invalid argument'):
            eng.chain_store(**dict(dict(E=2, W=8, n=2, capacity=4), **bad))
    store = eng.chain_store(2, 8, 2, 12)
    other = eng.chain_store(3, 8, 2, 12)
    try:
        store.append(chain, lnl)
        with pytest.raises(EngineError, match='beyond the store\'s capacity'):
            store.append(chain[:, :3], lnl[:, :3])
        for row0, rows in ((0, 11), (10, 1), (11, 0), (-1, 2), (0, -1)):
            with pytest.raises(EngineError, match='invalid argument'):
                store.fetch(row0, rows)
        for first, c in ((10, 5), (-1, 5), (0, 0.0), (0, np.nan)):
            with pytest.raises(EngineError, match='invalid argument'):
                store.summary(first, c)
        with pytest.raises(ValueError):
            store.append(chain[:, :, :6], lnl[:, :, :6])
        # attached to a run: another (E, W, n), then too many rows - refused before anything runs
        cols = [eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')]
        x0 = np.array([-0.2, 1.67]) + 0.01 * np.random.default_rng(2).standard_normal((2, 8, 2))
        rows = np.repeat(eng.low.theta0[None, :], 16, axis=0)
        rows[:, cols] = x0.reshape(16, 2)
        lnl0 = -0.5 * np.asarray(auto_vega.chi2_batch(rows), dtype=np.float64).reshape(2, 8)

        def run(n_steps, **kw):
            x, l, acc = x0.copy(), lnl0.copy(), np.zeros((2, 8), dtype=np.int64)
            out = eng.ensemble_run_many(cols, [-0.5, 0.5], [0.0, 3.0], eng.low.theta0.copy(), x, l, acc, [0, 1], 0, n_steps, **kw)
            return out, x, acc
        eng.attach_chain_store(other)
        with pytest.raises(EngineError, match=r'another \(E, W, n\)'):
            run(2)
        eng.attach_chain_store(store)
        with pytest.raises(EngineError, match='exceed the attached chain store'):
            run(3)
        assert store.rows == 10 and other.rows == 0
        got, got_lnl = store.fetch()
        assert got.tobytes() == chain.tobytes() and got_lnl.tobytes() == lnl.tobytes()
        _same_summary(store.summary(1), chain_summary(chain, 1))
        # what was refused runs once it fits: two rows behind the ten, the same rows the host gets, and with keep_chain=False
        # the same walkers without a host chain
        (host_chain, host_lnl, st), x_a, acc_a = run(2)
        assert st['steps'] == 2 and st['host_synchronisations'] == 1 and store.rows == 12
        got, got_lnl = store.fetch(10, 2)
        assert got.tobytes() == host_chain.tobytes() and got_lnl.tobytes() == host_lnl.tobytes()
        eng.attach_chain_store(None)
        store.reserve(14)
        eng.attach_chain_store(store)
        (none_chain, none_lnl, st), x_b, acc_b = run(2, keep_chain=False)
        assert none_chain is None and none_lnl is None and st['host_synchronisations'] == 1 and store.rows == 14
        assert np.array_equal(x_a, x_b) and np.array_equal(acc_a, acc_b) and store.fetch(12, 2)[0].tobytes() == host_chain.tobytes()
        eng.attach_chain_store(None)
        with pytest.raises(ValueError, match='another engine'):
            eng.attach_chain_store(type('S', (), {'engine': None})())
    finally:
        eng.attach_chain_store(None)
        store.close()
        other.close()
    with pytest.raises(EngineError, match='closed'):
        store.rows
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


# ------------------------------------------------------------------ attached to runs
MOVES = {'stretch': {}, 'mixture': dict(moves=[('de', 0.5), ('snooker', 0.3), ('cov', 0.2)]), 'slice': dict(moves='slice', tune_steps=10)}


@pytest.mark.parametrize('thin', [1, 3])
@pytest.mark.parametrize('kind', list(MOVES))
def test_the_store_holds_the_chain_of_the_host_path(auto_vega, kind, thin):
    """EnsembleSet(E = 3, W = 8), 40 steps in segments of 7: the ``chain='device'`` fetch is the ``chain='host'`` chain and lnL
    bit for bit, ``summary()`` is ``chain_summary`` of that chain bit for bit, and the ``python`` driver gives the same summary."""
    from vega_amd import EnsembleSet
    from vega_amd.ensemble import chain_summary
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    kw = dict(seed=7, thin=thin, segment=7, sample_params=sp, **MOVES[kind])
    host = EnsembleSet(auto_vega, 3, 8, **kw).run(40)
    dev = EnsembleSet(auto_vega, 3, 8, chain='device', **kw).run(25).run(15)         # (the second call grows the store)
    assert dev.driver == 'device' and dev._store is not None and dev._chain == [] and dev._store.rows == 40 // thin
    assert auto_vega.engine._attached is None
    chain = host.get_chain()
    assert chain.shape == (3, 40 // thin, 8, 4)
    assert dev.get_chain().tobytes() == chain.tobytes() and dev.get_log_lik().tobytes() == host.get_log_lik().tobytes()
    assert np.array_equal(dev.accepted, host.accepted)
    if kind != 'slice':         # (the call's single wait stays single: nothing waits for the store)
        assert dev.stats['host_synchronisations'] == dev.stats['calls'] == 7 and host.stats['host_synchronisations'] == host.stats['calls'] == 6
    assert dev.get_chain(discard=2, thin=2, flat=True).tobytes() == host.get_chain(discard=2, thin=2, flat=True).tobytes()
    for discard in (0, 3):
        _same_summary(dev.summary(discard=discard), chain_summary(chain, discard))
    py = EnsembleSet(auto_vega, 3, 8, chain='device', driver='python', **kw).run(40)
    assert py._store is None and np.array_equal(py.get_chain(), chain)
    _same_summary(py.summary(discard=3), dev.summary(discard=3))
    if kind == 'mixture':       # (the moves' counters read the recorded rows: from the store, the same counts; thin 3: proposals)
        ours, theirs = dict(dev.stats['moves']), dict(host.stats['moves'])
        assert set(ours) == {'stretch', 'de', 'snooker', 'cov'} and ours == theirs and sum(v['proposals'] for v in ours.values()) == 3 * 8 * 40
        assert all((v['accepted'] is None) == (thin == 3) for v in ours.values())
        assert dev.stats['moves'].unseen == host.stats['moves'].unseen
    member = dev.member(1)
    assert member.get_chain().tobytes() == chain[1].tobytes()
    # closed: the device memory is released, the rows answer from the host - the same arrays and the same summary
    summ = dev.summary(discard=3)
    assert dev.close() is dev and dev._store is None
    assert dev.get_chain().tobytes() == chain.tobytes() and dev.get_log_lik().tobytes() == host.get_log_lik().tobytes()
    _same_summary(dev.summary(discard=3), summ)
    dev.reset()
    assert dev._store is None and dev.get_chain().shape == (3, 0, 8, 4)
    gone = EnsembleSet(auto_vega, 3, 8, chain='device', **kw).run(7).discard_chain()
    assert gone._store is None and gone._chain == [] and gone.get_chain().shape == (3, 0, 8, 4)


def test_the_single_sampler_is_the_set_of_one(auto_vega):
    from vega_amd import EnsembleSampler, EnsembleSet
    from vega_amd.ensemble import chain_summary
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    for extra in ({}, dict(moves='slice', tune_steps=10), dict(moves='de')):
        host = EnsembleSampler(auto_vega, 8, seed=7, stream=2, segment=7, sample_params=sp, **extra).run(30)
        one = EnsembleSampler(auto_vega, 8, seed=7, stream=2, segment=7, sample_params=sp, chain='device', **extra).run(30)
        assert one._store is not None and one._store.E == 1 and one._chain == []
        assert one.get_chain().tobytes() == host.get_chain().tobytes() and one.get_log_lik().tobytes() == host.get_log_lik().tobytes()
        summ, ref = one.summary(discard=5), chain_summary(host.get_chain(), 5)
        for key in ref:
            assert np.asarray(summ[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
        both = EnsembleSet(auto_vega, 1, 8, streams=[2], seed=7, segment=7, sample_params=sp, chain='device', **extra).run(30)
        assert both.get_chain()[0].tobytes() == one.get_chain().tobytes()
        assert both.summary(discard=5)['tau'][0].tobytes() == summ['tau'].tobytes()


def test_a_store_outlives_the_second_lane():
    """The joint problem, 6 sampled parameters, half-steps of 128 rows in chunks of 64: the quadratic form serves them, so the
    second chunk of a half runs on the engine's second lane - a clone of the engine.  Retiring the lane (``set_lanes``, a new mock
    pool: anything that changes what an evaluation computes) must leave the stores of the engine alone: the rows are still
    there, the run goes on, and the chain is the host path's."""
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSet, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    from vega_amd.ensemble import chain_summary
    names = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd']
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        vega.freeze_metals()
        sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in names}, 'values': {n: vega.params[n] for n in names},
              'errors': {n: DEFAULT_VALUES[n][1] for n in names}}
        kw = dict(seed=3, chunk=64, sample_params=sp)
        host = EnsembleSet(vega, 8, 32, **kw).run(8)
        dev = EnsembleSet(vega, 8, 32, chain='device', **kw).run(5)
        assert dev.stats['engine_calls'] == 5 * 2 * 2 and vega.engine.last_form() in ('q', 'factored')       # (two chunks a half, on the quadratic form)
        first = dev.get_chain()
        vega.engine.set_lanes(2)
        vega.engine.set_lanes(1)            # (the second lane is retired here)
        assert dev._store.rows == 5 and dev.get_chain().tobytes() == first.tobytes()
        dev.run(3)
        assert dev.get_chain().tobytes() == host.get_chain().tobytes()
        for key, val in chain_summary(host.get_chain(), 2).items():
            assert np.asarray(dev.summary(discard=2)[key]).tobytes() == np.asarray(val).tobytes(), key
        dev.reset()
    finally:
        vega.close()


# ------------------------------------------------------------------ the convergence stop
def test_run_until_stops_both_drivers_at_the_same_step(auto_vega):
    from vega_amd import EnsembleSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    runs = {}
    for driver in ('device', 'python'):
        s = EnsembleSet(auto_vega, 3, 8, seed=7, driver=driver, sample_params=sp, chain='device')
        runs[driver] = s.run_until(60, tau_factor=1, tau_rtol=1.0, check_every=10)
        assert s.driver == driver
    dev, py = runs['device'], runs['python']
    assert dev.step == py.step and dev.step < 60 and dev.step % 10 == 0
    assert np.all(dev.convergence['converged']) and dev.convergence['converged_at'].max() == dev.step
    assert set(dev.convergence) == set(py.convergence)
    for key, val in dev.convergence.items():
        assert np.asarray(val).tobytes() == np.asarray(py.convergence[key]).tobytes(), key
    assert dev.convergence['tau'].shape == (len(dev.convergence['steps']), 3, 4)
    assert np.array_equal(dev.get_chain(), py.get_chain())
    # tau_rtol = 0: tau never stops moving - the run goes to max_steps and says so
    s = EnsembleSet(auto_vega, 3, 8, seed=7, sample_params=sp, chain='device').run_until(30, tau_factor=1, tau_rtol=0.0, check_every=10)
    assert s.step == 30 and list(s.convergence['steps']) == [10, 20, 30] and not np.any(s.convergence['converged'])
    assert list(s.convergence['converged_at']) == [-1, -1, -1]


# ------------------------------------------------------------------ a posterior per mock without a chain on the host
def _rel(ours, ref, scale):
    return float(np.max(np.abs(np.asarray(ours) - ref) / scale))


def test_sample_mocks_with_device_summaries(mock_vega, tmp_path):
    from vega_amd import fitslite
    from vega_amd.ensemble import chain_summary
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega
    sp = _sample_params(vega, AUTO_SAMPLED)
    mc = MonteCarlo(vega)
    kw = dict(num_mocks=4, walkers=8, steps=30, seed=5, sample_params=sp)
    lean = mc.sample_mocks(summaries='device', keep_chains=False, **kw)
    assert mc.mc_chains is None and mc.mc_chain_lnl is None and lean._chain == [] and lean._store.rows == 30
    post = dict(mc.mc_posteriors)
    kept = mc.sample_mocks(summaries='device', keep_chains=True, **kw)
    assert mc.mc_chains.shape == (4, 30, 8, 4) and mc.mc_chain_lnl.shape == (4, 30, 8)
    ref = chain_summary(mc.mc_chains, 10)           # (burn: a third of the steps)
    for key in ('mean', 'sd', 'covariance', 'tau', 'n_eff'):
        assert post[key].tobytes() == ref[key].tobytes() == mc.mc_posteriors[key].tobytes(), key
    assert 'converged' not in post
    # the host path: NumPy over the whole chain, the numbers of ever
    mc.sample_mocks(**kw)
    old = mc.mc_posteriors
    assert set(old) == set(post) and np.array_equal(mc.mc_chains, kept.get_chain())
    sd2 = np.sqrt(np.einsum('mi,mj->mij', np.diagonal(old['covariance'], axis1=1, axis2=2), np.diagonal(old['covariance'], axis1=1, axis2=2)))
    err = dict(mean=_rel(post['mean'], old['mean'], np.abs(old['mean'])), sd=_rel(post['sd'], old['sd'], old['sd']),
               covariance=_rel(post['covariance'], old['covariance'], sd2), tau=_rel(post['tau'], old['tau'], np.abs(old['tau'])),
               n_eff=_rel(post['n_eff'], old['n_eff'], np.abs(old['n_eff'])))
    print('device summaries against the host path:', {k: f'{v:.2e}' for k, v in err.items()})
    assert max(err.values()) <= RTOL, err
    assert np.array_equal(post['acceptance'], old['acceptance'])
    # the table round-trips, with the two columns of a run that stops by itself
    mc.sample_mocks(summaries='device', keep_chains=False, converge=dict(tau_factor=1, tau_rtol=1.0, check_every=10), **kw)
    conv = mc.mc_posteriors
    assert conv['converged'].shape == (4,) and conv['converged_at'].shape == (4,) and conv['steps'] <= 30 and mc.mc_chains is None
    path = mc.write_mock_posteriors(tmp_path)
    hdu = fitslite.open(path)[1]
    table = hdu.data
    assert hdu.header['EXTNAME'] == 'POSTERIORS' and {'converged', 'converged_at'} <= set(hdu.columns.names)
    assert np.array_equal(table['converged'], conv['converged'].astype(np.int64)) and np.array_equal(table['converged_at'], conv['converged_at'])
    for j, name in enumerate(AUTO_SAMPLED):
        assert np.array_equal(table[f'{name}_mean'], conv['mean'][:, j]) and np.array_equal(table[f'{name}_tau'], conv['tau'][:, j])
    assert np.array_equal(np.asarray(table['covariance']).reshape(4, 4, 4), conv['covariance'])
    mc.mc_posteriors = post
    hdu = fitslite.open(mc.write_mock_posteriors(tmp_path / 'plain'))[1]
    assert 'converged' not in hdu.columns.names and np.array_equal(hdu.data['n_eff'], post['n_eff'])
