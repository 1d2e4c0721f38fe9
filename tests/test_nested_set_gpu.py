"""Many nested-sampling runs in one device run (include/vegamx.h: vmx_nested_run_many, vega_amd/nested.py: NestedSet) on real
engines: one run is the existing sampler bit for bit; the device driver makes the runs of the NumPy restatement - runs that stop at
iterations of their own, run boundaries inside chunks, rounds without a row, more than one thread per lane, two lanes, one mock per
run, runs entered at different iterations; a set that does not depend on how it is cut; the exact evidence of every mock; refused
arguments that leave the engine as it was; the config switches end to end."""
import configparser
import math
import time

import numpy as np
import pytest

from conftest import GOLDEN, synth_joint_problem
from test_ensemble_set_gpu import _linear_gaussian, _sample_params
from test_smc_gpu import _linear_box

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
MOCK_ROWS = [4, 0, 0, 2]
MOCK_SEED = 1           # (the mocks of the evidence test: a seed whose six MIGRAD fits lie within 2 sd of the box's centre)


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


@pytest.fixture(scope='module')
def linear_box(auto_vega):
    return _linear_box(auto_vega)[0]


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
    yield vega, mocks
    vega.close()


def _install(mock_vega):
    for name, pool in mock_vega[1].items():     # (6 mocks, whatever ran before)
        mock_vega[0].engine.set_mock_pool(name, pool)
    return mock_vega[0]


def _pair(vega, E, iterations, sp, stop_at=None, seed=7, **kw):
    """The set by both drivers; ``stop_at`` [E]: run e's termination test says yes after so many iterations (its own
    ``max_iterations``), and the sets run to termination."""
    from vega_amd import NestedSet
    out = []
    for driver in ('device', 'python'):
        s = NestedSet(vega, E, seed=seed, driver=driver, sample_params=sp, **kw)
        if stop_at is not None:
            for run, at in zip(s.runs, stop_at):
                run.max_iterations = at
        s.run(iterations)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    """u and the live counts bit for bit, lnL to 1e-12 (the drivers' chi2 come from the same engine in the same batches; the
    restatement turns them into lnL in NumPy)."""
    assert np.array_equal(dev.status, py.status) and np.array_equal(dev.iteration, py.iteration)
    assert np.array_equal(dev.finished, py.finished)
    for e in range(dev.E):
        a, b = dev.runs[e], py.runs[e]
        assert np.array_equal(a.live_u, b.live_u)
        np.testing.assert_allclose(a.live_lnl, b.live_lnl, rtol=1e-12, atol=0)
        (au, al, an), (bu, bl, bn) = a.dead(), b.dead()
        assert np.array_equal(au, bu) and np.array_equal(an, bn)
        np.testing.assert_allclose(al, bl, rtol=1e-12, atol=0)
    for key in ('iterations', 'rounds', 'rows', 'rows_own_position', 'engine_calls'):
        assert dev.stats[key] == py.stats[key], key
    assert np.array_equal(dev.stats['per_run'], py.stats['per_run'])


def test_one_run_is_the_existing_sampler(auto_vega, linear_box):
    """E = 1 has the single run's batches: live points, lnL and the dead record bit for bit."""
    from vega_amd import NestedSampler, NestedSet
    kw = dict(num_live=64, threads=16, seed=7, sample_params=linear_box)
    both = NestedSet(auto_vega, 1, streams=[3], **kw).run(6)
    one = NestedSampler(auto_vega, stream=3, **kw).run(6)
    assert both.driver == one.driver == 'device' and one.iteration == both.iteration[0] == 6
    run = both.runs[0]
    assert np.array_equal(run.live_u, one.live_u) and np.array_equal(run.live_lnl, one.live_lnl)
    for a, b in zip(both.dead(0), one.dead()):
        assert np.array_equal(a, b)
    member = both.member(0)
    assert member.log_evidence() == one.log_evidence() and np.array_equal(member.samples()[0], one.samples()[0])
    assert member.information() == one.information() and both.log_evidence()[0][0] == one.log_evidence()[0]
    for key in ('iterations', 'rows', 'rows_own_position'):
        assert member.stats[key] == one.stats[key], key
    assert set(member.stats) == set(one.stats)
    assert both.stats['engine_calls'] == one.stats['engine_calls']
    # every iteration of a set of one ends in a round of its own: rounds = the single run's + iterations, and one wait each
    assert both.stats['rounds'] == one.stats['rounds'] + 6 and both.stats['host_waits'] == both.stats['rounds'] + 2
    assert one.stats['host_waits'] == one.stats['rounds'] + 6 + 2


def test_drivers_agree_with_runs_that_stop_on_their_own(auto_vega, linear_box):
    """E = 5, nlive 40, K 12, num_repeats 4, chunk 16, streams 0 .. 4; run e stops after 2 + e iterations.  The runs' rows are packed
    behind each other, so run boundaries fall inside chunks and tails stay below the chunk; once run 4 is alone, the round that
    ends each of its iterations has no row at all."""
    stop_at = [2, 3, 4, 5, 6]
    dev, py = _pair(auto_vega, 5, None, linear_box, stop_at=stop_at, num_live=40, threads=12, num_repeats=4, chunk=16)
    _assert_same(dev, py)
    assert list(dev.iteration) == stop_at and list(dev.status) == [1] * 5 and np.all(dev.finished)
    assert dev.stats['calls'] == 1 and dev.stats['host_waits'] == dev.stats['rounds'] + 2
    per = dev.stats['per_run']
    assert np.all(np.diff(per[:, 2]) > 0) and dev.stats['rounds'] == per[4, 2]          # (nobody waits for anybody)
    assert per[:, 0].sum() == dev.stats['rows'] and 0 < dev.stats['rows_own_position'] < dev.stats['rows']
    assert all(not np.array_equal(dev.runs[0].live_u, dev.runs[e].live_u) for e in range(1, 5))


def test_more_than_one_thread_per_lane(auto_vega, linear_box):
    """K = 1100 on 1024 lanes: two threads per lane of the advance kernel, rows beyond 1024 per run."""
    dev, py = _pair(auto_vega, 2, 2, linear_box, num_live=2200, threads=1100, num_repeats=2)
    _assert_same(dev, py)
    assert list(dev.iteration) == [2, 2] and dev.stats['per_run'][:, 0].min() > 2200 + 2 * 1100


def test_two_lanes():
    """E = 4, nlive 256, K 64, chunk 64 on the synthetic joint problem: a round of up to 256 rows in chunks of 64 on two lanes."""
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        dev, py = _pair(vega, 4, 2, _sample_params(vega, AUTO_SAMPLED), num_live=256, threads=64, num_repeats=3, chunk=64, seed=3)
        _assert_same(dev, py)
        assert dev.stats['lanes'] == 2 and list(dev.iteration) == [2] * 4
        assert dev.stats['engine_calls'] > dev.stats['rounds']          # (rounds of more than one chunk: the second lane ran)
    finally:
        vega.close()


def test_every_run_reads_its_own_mock(mock_vega):
    from vega_amd import NestedSampler
    vega = _install(mock_vega)
    sp = _sample_params(vega, AUTO_SAMPLED)
    kw = dict(num_live=48, threads=12, num_repeats=3)
    dev, py = _pair(vega, 4, 3, sp, streams=[0, 1, 1, 2], mock_rows=MOCK_ROWS, **kw)
    _assert_same(dev, py)
    # equal stream, equal mock: equal runs
    assert np.array_equal(dev.runs[1].live_u, dev.runs[2].live_u) and np.array_equal(dev.runs[1].live_lnl, dev.runs[2].live_lnl)
    assert np.array_equal(dev.stats['per_run'][1], dev.stats['per_run'][2])
    assert not np.array_equal(dev.runs[0].live_u, dev.runs[1].live_u)
    # run 0's first iteration is the single run's once its mock is installed as the data
    prob = vega.problem
    try:
        for name, pool in mock_vega[1].items():
            vega.engine.set_data(name, pool[MOCK_ROWS[0]])
        one = NestedSampler(vega, seed=7, stream=0, sample_params=sp, **kw).run(1)
    finally:
        for name in mock_vega[1]:
            vega.engine.set_data(name, prob.items[name].masked_data_vec)
    du, dl, dn = dev.dead(0)
    su, sl, sn = one.dead()
    assert np.array_equal(du[:12], su) and np.array_equal(dn[:12], sn)
    np.testing.assert_allclose(dl[:12], sl, rtol=1e-12, atol=0)
    # the data matter: the same stream on the installed data dies elsewhere
    other = NestedSampler(vega, seed=7, stream=0, sample_params=sp, **kw).run(1)
    assert not np.array_equal(other.dead()[1], sl)


def test_runs_entered_at_different_iterations(auto_vega, linear_box):
    """ctypes level: run 0 enters in the state the python driver has after 3 iterations, run 1 as drawn; both are what the python
    driver makes of them alone."""
    from vega_amd import NestedSet
    kw = dict(num_live=40, threads=12, num_repeats=4, seed=5, driver='python', sample_params=linear_box)
    a = NestedSet(auto_vega, 1, streams=[5], **kw).run(3)
    b = NestedSet(auto_vega, 1, streams=[6], **kw).run(0)
    assert list(a.iteration) == [3] and list(b.iteration) == [0] and b.runs[0].live_u is not None
    u = np.ascontiguousarray(np.stack([a.runs[0].live_u, b.runs[0].live_u]))
    lnl = np.ascontiguousarray(np.stack([a.runs[0].live_lnl, b.runs[0].live_lnl]))
    it = np.array([3, 0], dtype=np.int64)
    seen = []
    dead, status, done, st = auto_vega.engine.nested_run_many(
        a.cols, a.lo, a.hi, a._theta, u, lnl, it, [5, 6], 2, 12, 4, log_norm=a.log_norm(), seed=5,
        stop=lambda run, iterations, dead_lnl, live_lnl: seen.append((run, iterations, dead_lnl.size, live_lnl.size)) or False)
    assert list(status) == [0, 0] and list(done) == [2, 2] and list(it) == [5, 2] and st['host_waits'] == st['rounds'] + 1
    assert sorted(seen) == [(0, 4, 12, 40), (0, 5, 12, 40), (1, 1, 12, 40), (1, 2, 12, 40)]
    a.run(2)
    b.run(2)
    for e, want in enumerate((a, b)):
        assert np.array_equal(u[e], want.runs[0].live_u)
        np.testing.assert_allclose(lnl[e], want.runs[0].live_lnl, rtol=1e-12, atol=0)
        wu, wl, wn = want.dead(0)
        assert np.array_equal(dead[e][0], wu[-24:]) and np.array_equal(dead[e][2], wn[-24:])
        np.testing.assert_allclose(dead[e][1], wl[-24:], rtol=1e-12, atol=0)
    assert st['iterations'] == 4 and st['per_run'][:, 0].sum() == st['rows']


def test_the_set_does_not_depend_on_the_cut(auto_vega, linear_box):
    """``run(3)`` then ``run(3)`` against ``run(6)``.  Runs do not wait for each other inside a call, but a call ends when every
    run has done its iterations and the next one heads them together: a cut regroups the rounds, and the engine's chi2 depends
    on the size of its batch in the last bits.  So: three runs on one stream move in step, a cut falls where their rounds
    already meet, the batches are the same and everything is the same bit for bit (as is a set of one); three runs on streams
    of their own make the same decisions - u and the record's live counts bit for bit - with lnL to 1e-12."""
    from vega_amd import NestedSet
    kw = dict(num_live=40, threads=12, num_repeats=4, seed=5, sample_params=linear_box)
    for streams in ([2, 2, 2], [4], [0, 1, 2]):
        E = len(streams)
        one = NestedSet(auto_vega, E, streams=streams, **kw).run(6)
        cut = NestedSet(auto_vega, E, streams=streams, **kw).run(3).run(3)
        assert one.stats['calls'] == 1 and cut.stats['calls'] == 2 and list(one.iteration) == list(cut.iteration) == [6] * E
        exact = len(set(streams)) == 1
        for e in range(E):
            assert np.array_equal(one.runs[e].live_u, cut.runs[e].live_u)
            (au, al, an), (bu, bl, bn) = one.dead(e), cut.dead(e)
            assert np.array_equal(au, bu) and np.array_equal(an, bn)
            if exact:
                assert np.array_equal(one.runs[e].live_lnl, cut.runs[e].live_lnl) and np.array_equal(al, bl)
            else:
                np.testing.assert_allclose(one.runs[e].live_lnl, cut.runs[e].live_lnl, rtol=1e-12, atol=0)
                np.testing.assert_allclose(al, bl, rtol=1e-12, atol=0)
        assert np.array_equal(one.stats['per_run'][:, :2], cut.stats['per_run'][:, :2])
        if exact:
            assert np.array_equal(one.log_evidence()[0], cut.log_evidence()[0])
        assert cut.stats['host_waits'] == cut.stats['rounds'] + 3        # (a wait per round, a copy back per call, the draw)
    assert not np.array_equal(one.runs[0].live_u, one.runs[1].live_u)


def test_exact_evidence_per_mock(mock_vega):
    """Four additive broadband coefficients, everything else fixed: chi2 against mock m is exactly quadratic, so over a box far
    wider than the posterior log Z_m = lnL_max,m + 1/2 log det(2 pi Sigma_m) - sum log width, with lnL_max,m and Sigma_m from the
    device MIGRAD fit of mock m (tests/test_smc_set_gpu.py).  nlive 256, K 64, num_repeats 8, every run to precision 1e-3."""
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega[0]
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    mean, cov = _linear_gaussian(vega, names)
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    M = 6
    before = vega.chi2_batch(vega._theta(None)[None, :])
    mc = MonteCarlo(vega)
    vega.freeze_metals()
    mocks = mc.create_mocks(vega.compute_model(dict(zip(names, mean))), M, seed=MOCK_SEED)
    fits = mc._fit_mocks(mocks, M, sample_params=sp)
    assert list(fits.names) == names and np.all(fits.is_valid) and not np.any(fits.hesse_failed)
    best, hesse = fits.values, fits.covariance
    assert np.all(np.abs(best - mean) <= 2 * sd), (best - mean) / sd
    t0 = time.perf_counter()
    sampler = mc.sample_mocks_nested(mocks=mocks, seed=11, sample_params=sp, num_live=256, threads=64, num_repeats=8, precision=1e-3)
    print(f'sample_mocks_nested: {time.perf_counter() - t0:.2f} s, rounds {sampler.stats["rounds"]}, rows {sampler.stats["rows"]}, '
          f'iterations {sampler.iteration.tolist()}')
    assert sampler.driver == 'device' and sampler.stats['calls'] == 1
    assert list(sampler.status) == [1] * M and np.all(sampler.finished)           # (no run may be left out)
    log_z, err = sampler.log_evidence()
    post = mc.mc_posteriors
    for m in range(M):
        exact = sampler.log_norm() - 0.5 * fits.fval[m] + 0.5 * np.linalg.slogdet(2 * np.pi * hesse[m])[1] - np.sum(np.log(20 * sd))
        sd_m = np.sqrt(np.diag(hesse[m]))
        pts, _, w = sampler.samples()[m]
        ess = 1.0 / np.sum(w * w)
        got = w @ pts
        print(f'mock {m}: log Z {log_z[m]:.4f} (exact {exact:.4f}, err {err[m]:.4f}, pull {(log_z[m] - exact) / err[m]:+.2f}), '
              f'iterations {sampler.iteration[m]}, ESS {ess:.0f}, mean pulls {np.round((got - best[m]) / (sd_m / math.sqrt(ess)), 2).tolist()}')
        assert math.isfinite(log_z[m]) and abs(log_z[m] - exact) <= 5 * err[m], (m, log_z[m], exact, err[m])
        assert np.all(np.abs(got - best[m]) < 5 * sd_m / math.sqrt(ess)), (m, (got - best[m]) / sd_m)
        np.testing.assert_array_equal(post['mean'][m], got)
    assert post['names'] == names and np.array_equal(post['log_z'], log_z) and np.array_equal(post['iterations'], sampler.iteration)
    assert post['sampler'] == 'nested' and np.all(post['info'] > 0) and len(mc.mc_chains) == M
    # the engine is as it was: the data's chi2, not a mock's
    np.testing.assert_array_equal(vega.chi2_batch(vega._theta(None)[None, :]), before)


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    E, nlive = changes.pop('E', 2), changes.pop('nlive', 16)
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), live_u=np.full((E, nlive, 2), 0.5), live_lnl=np.zeros((E, nlive)),
                iteration=np.zeros(E, dtype=np.int64), streams=np.arange(E), n_iterations=2, threads=4, num_repeats=3)
    args.update(changes)
    for k in ('live_u', 'live_lnl'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    args['iteration'] = np.ascontiguousarray(args['iteration'], dtype=np.int64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.nested_run_many(**args)


@pytest.fixture()
def bare_vega():
    """An engine no mock pool has been installed on."""
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=16)
    yield vega
    vega.close()


def test_refused_arguments_leave_the_engine_as_it_was(bare_vega, mock_vega):
    _install(mock_vega)
    last = np.full((2, 16, 2), 0.5)
    last[1, 15, 0] = 1.5                        # (the last live point of the last run)
    for vega, cases in ((bare_vega, [dict(E=0), dict(streams=None), dict(mock_rows=[0, 0]),        # (no pool on this engine)
                                     dict(nlive=3), dict(nlive=4097), dict(threads=0), dict(threads=14), dict(num_repeats=0),
                                     dict(lo=[0.0, 0.5]), dict(live_u=last),
                                     dict(live_lnl=np.where(np.arange(32).reshape(2, 16) == 31, np.nan, 0.0)),
                                     dict(iteration=[0, -1]), dict(draw_live=True, iteration=[0, 3]), dict(chunk=-1), dict(lanes=-1),
                                     dict(const_hint=3)]),
                        (mock_vega[0], [dict(E=1, mock_rows=[6]), dict(E=1, mock_rows=[-1]), dict(mock_rows=[0, 6])])):
        theta = vega._theta(None)[None, :]
        before = vega.chi2_batch(theta)
        for case in cases:
            _refused(vega.engine, **case)
            np.testing.assert_array_equal(vega.chi2_batch(theta), before)
    # (what was refused runs once the argument is mended: the pool has rows 0 .. 5)
    eng = mock_vega[0].engine
    u, lnl, it = np.zeros((1, 16, 2)), np.zeros((1, 16)), np.zeros(1, dtype=np.int64)
    dead, status, done, st = eng.nested_run_many([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0],
                                                 eng.low.theta0.copy(), u, lnl, it, [0], 1, 4, 3, mock_rows=[5], draw_live=True)
    assert done[0] == 1 and it[0] == 1 and status[0] == 0 and st['per_run'].shape == (1, 3) and dead[0][0].shape == (4, 2)
    assert st['per_run'][0, 0] == st['rows'] > 16 and st['host_waits'] == st['rounds'] + 2


def test_evidence_for_every_mock_end_to_end(tmp_path):
    from conftest import mc_launcher_config
    from fits_standard import check_file
    from vega_amd import fitslite, run_vega_sampler
    from vega_amd.nested import NestedSet, read_stats
    config = mc_launcher_config(tmp_path)
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / config)
    cfg['control'].update(run_sampler='True', sampler='Nested')
    out = tmp_path / 'chains_mocks'
    out.mkdir()
    cfg['Nested'] = dict(path=str(out), name='run', mocks='3', num_live='48', threads='12', num_repeats='3', seed='4', max_iterations='6')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert isinstance(sampler, NestedSet) and sampler.E == 3 and sampler.driver == 'device' and sampler.mock_rows.tolist() == [0, 1, 2]
        assert np.all(sampler.finished) and list(sampler.iteration) == [6, 6, 6] and sampler.streams.tolist() == [0, 1, 2]
        log_z, err = sampler.log_evidence()
        found = sampler.samples()
        for m in range(3):
            pts, lnl, w = found[m]
            table = np.loadtxt(out / f'run_mock{m}.txt')
            assert table.shape == (6 * 12 + 48, 2 + 3) and np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
            assert (out / f'run_mock{m}.paramnames').is_file()
            stats = read_stats(out / f'run_mock{m}.stats')
            assert (stats['log(Z)'], stats['log(Z) error']) == (log_z[m], err[m]) and stats['iterations'] == 6
        assert not np.array_equal(found[0][0], found[1][0])
        check_file(out / 'mock_posteriors.fits')
        with fitslite.open(str(out / 'mock_posteriors.fits')) as hdus:
            data = hdus[1].data
            post = sampler.vega.analysis.mc_posteriors
            assert len(data) == 3 and np.all(np.isfinite(data['log_z'])) and np.all(data['log_z_err'] > 0)
            np.testing.assert_array_equal(data['log_z'], log_z)
            np.testing.assert_array_equal(data['ap_mean'], post['mean'][:, 0])
            np.testing.assert_array_equal(data['at_sd'], post['sd'][:, 1])
            np.testing.assert_array_equal(data['iterations'], [6, 6, 6])
            np.testing.assert_array_equal(data['status'], [1, 1, 1])
            np.testing.assert_array_equal(np.asarray(data['covariance']).reshape(3, 3, 3), post['covariance'])
        raw = (out / 'mock_posteriors.fits').read_bytes()
        for word in (b'SAMPLER', b'NUMLIVE', b'NREPEATS', b'THREADS', b'PRECISN', b'SEED', b'info'):
            assert word in raw, word
    finally:
        sampler.vega.close()


def _write_config(tmp_path, tag, section):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control'].update(run_sampler='True', sampler='Nested')
    out = tmp_path / f'chains_{tag}'
    out.mkdir()
    cfg['Nested'] = dict(section, path=str(out), name='run')
    (tmp_path / 'configs' / tag).mkdir(parents=True)
    with open(tmp_path / 'configs' / tag / 'main.ini', 'w') as f:
        cfg.write(f)
    return f'configs/{tag}/main.ini', out


def test_replicas_together_end_to_end(tmp_path):
    """``together = True`` writes the files of the sequential path with the same keys; the merged run has the summed live count
    either way, and the merged evidences agree within their two errors (the samples are not compared bit for bit: the batches
    are shaped differently)."""
    from vega_amd import replicas as rep
    from vega_amd import run_vega_sampler
    section = dict(replicas='2', num_live='48', threads='12', num_repeats='3', seed='4', max_iterations='8')
    stats, records = {}, {}
    for tag, extra in (('together', dict(together='True')), ('sequential', dict())):
        config, out = _write_config(tmp_path, tag, dict(section, **extra))
        run = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, rank=0, world_size=1)
        try:
            assert run.replicas == 2 and [s.stream for s in run.samplers] == [0, 1] and all(s.driver == 'device' for s in run.samplers)
            records[tag] = [rep.load_record(rep.record_path(out, 'run', r)) for r in range(2)]
            stats[tag] = rep.read_stats(out / 'run.stats')
            assert sorted(p.name for p in out.iterdir()) == sorted(p.name for p in (tmp_path / 'chains_together').iterdir())
        finally:
            run.samplers[0].vega.close()
    for rec, want in zip(records['together'], records['sequential']):
        assert set(rec) == set(want) and set(rec['stats']) == set(want['stats'])                # the same keys as today
        assert rec['kind'] == 'nested' and rec['live_u'].shape == want['live_u'].shape == (48, 2)
        assert np.array_equal(rec['dead_nlive'], want['dead_nlive']) and rec['iteration'] == want['iteration'] == 8
    a, b = stats['together'], stats['sequential']
    assert set(a) == set(b) and a['replicas'] == 2 and a['num_live'] == b['num_live'] == 96
    assert math.isfinite(a['log(Z)']) and abs(a['log(Z)'] - b['log(Z)']) <= a['log(Z) error'] + b['log(Z) error']
