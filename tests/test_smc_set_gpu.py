"""Many SMC runs in one device run (include/vegamx.h: vmx_smc_run_many, vega_amd/smc.py: SMCSet) on real engines: one run is the
existing sampler bit for bit; the device driver makes the runs of the NumPy restatement for shared data and for one mock per run,
with chunk boundaries inside runs, beyond 1024 lanes and on two lanes; runs that leave early; a set that does not depend on how it
is cut into calls or chunks; the exact evidence of every mock; refused arguments that leave the engine as it was; the config
switches end to end."""
import configparser
import math

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


def _pair(vega, E, N, stages, sp, seed=7, **kw):
    from vega_amd import SMCSet
    out = []
    for driver in ('device', 'python'):
        s = SMCSet(vega, E, particles=N, seed=seed, driver=driver, sample_params=sp, **kw).run(stages)
        assert s.driver == driver
        out.append(s)
    return out


def _same_records(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra['anc'], rb['anc'])
        np.testing.assert_allclose(ra['lnl'], rb['lnl'], rtol=1e-12, atol=0)
        for key in ('beta_prev', 'beta', 'ess'):
            assert ra[key] == pytest.approx(rb[key], rel=1e-9), key
        assert ra['accepted'] == rb['accepted'] and ra['scale'] == rb['scale'] and ra['cholesky'] == rb['cholesky']


def _assert_same(dev, py):
    """The tolerances of tests/test_smc_gpu.py::_assert_same, run by run."""
    assert np.array_equal(dev.stage, py.stage) and np.array_equal(dev.scale, py.scale) and np.array_equal(dev.status, py.status)
    assert dev.beta == pytest.approx(py.beta, rel=1e-9)         # (beta follows lnL, which the drivers share to 1e-12)
    assert np.array_equal(dev.u, py.u)
    np.testing.assert_allclose(dev.lnl, py.lnl, rtol=1e-12, atol=0)
    for e in range(dev.E):
        _same_records(dev.record[e], py.record[e])
    for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model', 'rounds'):
        assert dev.stats[key] == py.stats[key], key
    assert np.array_equal(dev.stats['per_run'], py.stats['per_run'])


def test_one_run_is_the_existing_sampler(auto_vega):
    """E = 1 has the single run's batches: u, lnL, ancestors and the record bit for bit."""
    from vega_amd import SMCSampler, SMCSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    both = SMCSet(auto_vega, 1, particles=256, streams=[3], seed=7, sample_params=sp).run(2)
    one = SMCSampler(auto_vega, particles=256, stream=3, seed=7, sample_params=sp).run(stages=2)
    assert both.driver == one.driver == 'device' and one.stage >= 1
    assert np.array_equal(both.u[0], one.u) and np.array_equal(both.lnl[0], one.lnl)
    assert (both.stage[0], both.beta[0], both.scale[0]) == (one.stage, one.beta, one.scale)
    assert len(both.record[0]) == len(one.record)
    for a, b in zip(both.record[0], one.record):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    member = both.member(0)
    assert member.log_evidence() == one.log_evidence() and np.array_equal(member.samples()[0], one.samples()[0])
    for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model', 'engine_calls', 'host_waits'):
        assert member.stats[key] == one.stats[key], key
    assert set(member.stats) == set(one.stats)


def test_drivers_agree_with_chunk_boundaries_inside_runs(auto_vega, linear_box):
    """E = 5, N = 72, sweeps = 5, chunk = 48: 360 rows per sweep, chunk boundaries inside runs and a tail of 24 rows; the linear
    coefficients give a ladder of several stages, and the runs do not all end in the same round."""
    dev, py = _pair(auto_vega, 5, 72, None, linear_box, sweeps=5, chunk=48)
    _assert_same(dev, py)
    assert np.all(dev.finished) and list(dev.status) == [1] * 5 and dev.stats['rounds'] == dev.stage.max() >= 4
    assert dev.stats['calls'] == 1 and dev.stats['host_waits'] == dev.stats['rounds'] + 2
    assert np.array_equal(dev.stats['per_run'][:, 3], 72 * (1 + 5 * dev.stage))
    # the chunks follow the rows of the runs still going: ceil(A 72 / 48) calls per sweep
    going = [int(np.sum(dev.stage > r)) for r in range(dev.stats['rounds'])]
    assert dev.stats['engine_calls'] == py.stats['engine_calls'] == -(-5 * 72 // 48) + sum(5 * -(-a * 72 // 48) for a in going)
    assert all(not np.array_equal(dev.u[0], dev.u[e]) for e in range(1, 5))
    assert 0 < dev.stats['accepted'] < dev.stats['rows']
    np.testing.assert_allclose(dev.log_evidence(), py.log_evidence(), rtol=1e-9)


def test_beyond_1024_lanes(auto_vega):
    """N = 1100: padded to 2048, two entries per lane of the stage kernel."""
    dev, py = _pair(auto_vega, 2, 1100, 1, _sample_params(auto_vega, AUTO_SAMPLED), sweeps=2)
    _assert_same(dev, py)
    assert list(dev.stage) == [1, 1] and dev.stats['rows'] == 2 * 1100 * 3


def test_two_lanes():
    """E = 4, N = 256, max_batch = 256: 1024 rows per sweep in four chunks on two lanes."""
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        dev, py = _pair(vega, 4, 256, 2, _sample_params(vega, AUTO_SAMPLED), sweeps=3, seed=3)
        _assert_same(dev, py)
        assert dev.stats['lanes'] == 2 and list(dev.stage) == [2] * 4
        assert dev.stats['engine_calls'] == py.stats['engine_calls'] == 4 * (1 + 2 * 3)
    finally:
        vega.close()


def test_every_run_reads_its_own_mock(mock_vega):
    from vega_amd import SMCSet
    vega = _install(mock_vega)
    sp = _sample_params(vega, AUTO_SAMPLED)
    kw = dict(sweeps=4, streams=[0, 1, 1, 2], mock_rows=MOCK_ROWS)
    dev, py = _pair(vega, 4, 64, 3, sp, **kw)
    _assert_same(dev, py)
    # equal stream, equal mock: equal runs
    assert np.array_equal(dev.u[1], dev.u[2]) and np.array_equal(dev.lnl[1], dev.lnl[2]) and dev.stage[1] == dev.stage[2]
    assert np.array_equal(dev.stats['per_run'][1], dev.stats['per_run'][2])
    for a, b in zip(dev.record[1], dev.record[2]):
        assert np.array_equal(a['anc'], b['anc']) and np.array_equal(a['lnl'], b['lnl']) and a['beta'] == b['beta']
    assert not np.array_equal(dev.u[0], dev.u[1])
    # the data matter: stream 0 on mock row 0 is another run than stream 0 on mock row 4
    other = SMCSet(vega, 1, particles=64, seed=7, sweeps=4, streams=[0], mock_rows=[0], sample_params=sp).run(3)
    assert not np.array_equal(other.record[0][0]['lnl'], dev.record[0][0]['lnl'])
    assert not np.array_equal(other.lnl[0], dev.lnl[0])


def test_runs_that_end_at_different_stages(auto_vega, linear_box):
    """ctypes level: run 0 enters in the state the python driver has after 3 stages, run 1 in the state after none.  Run 0 leaves
    early; the device and the python driver agree after it has left, and the later rounds evaluate N rows, not 2 N."""
    from vega_amd import SMCSet
    N, kw = 72, dict(particles=72, sweeps=5, seed=5, driver='python', sample_params=linear_box)
    a = SMCSet(auto_vega, 1, streams=[5], **kw).run(3)
    b = SMCSet(auto_vega, 1, streams=[6], **kw).run(0)
    assert a.stage[0] == 3 and not a.finished[0] and b.stage[0] == 0 and b.u is not None
    entry = dict(u=np.concatenate([a.u, b.u]), lnl=np.concatenate([a.lnl, b.lnl]), stage=np.array([3, 0], dtype=np.int64),
                 beta=np.array([a.beta[0], 0.0]), scale=np.array([a.scale[0], b.scale[0]]))
    py = SMCSet(auto_vega, 2, streams=[5, 6], **kw)
    py.u, py.lnl, py.stage, py.beta, py.scale = (entry[k].copy() for k in ('u', 'lnl', 'stage', 'beta', 'scale'))
    py.run()
    dev = {k: v.copy() for k, v in entry.items()}
    rec, status, done, st = auto_vega.engine.smc_run_many(
        py.cols, py.lo, py.hi, py._theta, dev['u'], dev['lnl'], dev['stage'], dev['beta'], dev['scale'], [5, 6], 64, 0.5, 5,
        log_norm=py.log_norm(), seed=5)
    assert list(status) == [1, 1] and done[0] < done[1] and list(dev['stage']) == [3 + done[0], done[1]]
    assert np.array_equal(dev['u'], py.u) and np.array_equal(dev['stage'], py.stage) and np.array_equal(dev['scale'], py.scale)
    np.testing.assert_allclose(dev['lnl'], py.lnl, rtol=1e-12, atol=0)
    assert dev['beta'] == pytest.approx(py.beta, rel=1e-9)
    _same_records(rec[0], py.record[0])
    _same_records(rec[1], py.record[1])
    assert np.array_equal(st['per_run'], py.stats['per_run'])
    assert list(st['per_run'][:, 3]) == [N * 5 * done[0], N * 5 * done[1]] and st['rows'] == N * 5 * (done[0] + done[1])
    assert st['host_waits'] == done[1] + 1 and st['stages'] == done[0] + done[1]


def test_the_set_does_not_depend_on_the_cut_or_the_chunks(auto_vega, linear_box):
    from vega_amd import SMCSet
    kw = dict(particles=128, sweeps=5, seed=5, sample_params=linear_box)
    one = SMCSet(auto_vega, 3, **kw).run(4)
    cut = SMCSet(auto_vega, 3, **kw)
    for _ in range(4):
        cut.run(1)
    small = SMCSet(auto_vega, 3, chunk=16, **kw).run(4)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 4 and list(one.stage) == [4] * 3 and not np.any(one.finished)
    for other in (cut, small):
        assert np.array_equal(one.u, other.u) and np.array_equal(one.lnl, other.lnl)
        for key in ('stage', 'beta', 'scale', 'status'):
            assert np.array_equal(getattr(one, key), getattr(other, key)), key
        for e in range(3):
            for a, b in zip(one.record[e], other.record[e]):
                assert np.array_equal(a['anc'], b['anc']) and np.array_equal(a['lnl'], b['lnl'])
                assert (a['beta'], a['ess'], a['accepted'], a['scale']) == (b['beta'], b['ess'], b['accepted'], b['scale'])
        assert np.array_equal(one.stats['per_run'], other.stats['per_run'])
    # (384 rows per sweep: 256 + 128 at max_batch, 24 chunks of 16; the start and 4 rounds of 5 sweeps)
    assert one.stats['engine_calls'] == 2 * 21 and small.stats['engine_calls'] == 24 * 21
    assert one.stats['host_waits'] == 4 + 2 and cut.stats['host_waits'] == 4 + 4 + 1      # (a wait per round, a copy back per call, the start)


def test_exact_evidence_per_mock(mock_vega):
    """Four additive broadband coefficients, everything else fixed: chi2 against mock m is exactly quadratic, so over a box far
    wider than the posterior log Z_m = lnL_max,m + 1/2 log det(2 pi Sigma_m) - sum log width, with lnL_max,m and Sigma_m from the
    device MIGRAD fit of mock m.  The box is the fit of the data +- 10 sd; every mock's fit lies within 2 sd of its centre, so
    that at least 8 sd remain to every wall and the truncated mass is below 1e-14.  N = 512, the default 4 n sweeps."""
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega[0]
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    mean, cov = _linear_gaussian(vega, names)
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    M, N = 6, 512
    before = vega.chi2_batch(vega._theta(None)[None, :])
    mc = MonteCarlo(vega)
    vega.freeze_metals()
    mocks = mc.create_mocks(vega.compute_model(dict(zip(names, mean))), M, seed=MOCK_SEED)
    fits = mc._fit_mocks(mocks, M, sample_params=sp)
    assert list(fits.names) == names and np.all(fits.is_valid) and not np.any(fits.hesse_failed)
    best, hesse = fits.values, fits.covariance
    print('fits - centre, in sd:', np.round((best - mean) / sd, 2).tolist())
    assert np.all(np.abs(best - mean) <= 2 * sd), (best - mean) / sd
    sampler = mc.sample_mocks(mocks=mocks, seed=11, sample_params=sp, sampler='smc', particles=N)
    assert sampler.driver == 'device' and sampler.stats['calls'] == 1 and sampler.sweeps == 16
    assert list(sampler.status) == [1] * M and np.all(sampler.finished)           # (no run may be left out)
    log_z, err = sampler.log_evidence()
    pts, _, w = sampler.samples()
    post = mc.mc_posteriors
    for m in range(M):
        exact = sampler.log_norm() - 0.5 * fits.fval[m] + 0.5 * np.linalg.slogdet(2 * np.pi * hesse[m])[1] - np.sum(np.log(20 * sd))
        sd_m = np.sqrt(np.diag(hesse[m]))
        got = pts[m].mean(axis=0)
        print(f'mock {m}: log Z {log_z[m]:.4f} (exact {exact:.4f}, err {err[m]:.4f}, pull {(log_z[m] - exact) / err[m]:+.2f}), '
              f'stages {sampler.stage[m]}, mean pulls {np.round((got - best[m]) / (sd_m / math.sqrt(N)), 2).tolist()}')
        assert math.isfinite(log_z[m]) and abs(log_z[m] - exact) <= 5 * err[m], (m, log_z[m], exact, err[m])
        assert np.all(np.abs(got - best[m]) < 5 * sd_m / math.sqrt(N)), (m, (got - best[m]) / sd_m)
        np.testing.assert_array_equal(post['mean'][m], got)
    assert post['names'] == names and np.array_equal(post['log_z'], log_z) and np.array_equal(post['stages'], sampler.stage)
    assert mc.mc_chains.shape == (M, N, 4)
    # the engine is as it was: the data's chi2, not a mock's
    np.testing.assert_array_equal(vega.chi2_batch(vega._theta(None)[None, :]), before)


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    E, N = changes.pop('E', 2), changes.pop('N', 16)
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), u=np.full((E, N, 2), 0.5), lnl=np.zeros((E, N)), stage=np.zeros(E, dtype=np.int64),
                beta=np.zeros(E), scale=np.ones(E), streams=np.arange(E), n_stages=2, ess=0.5, sweeps=3)
    args.update(changes)
    for k in ('u', 'lnl', 'beta', 'scale'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    args['stage'] = np.ascontiguousarray(args['stage'], dtype=np.int64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.smc_run_many(**args)


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
    last[1, 15, 0] = 1.5                        # (the last particle of the last run)
    dead = np.zeros((2, 16))
    dead[1] = -np.inf                           # (no particle of run 1 has a finite lnL)
    for vega, cases in ((bare_vega, [dict(E=0), dict(streams=None), dict(mock_rows=[0, 0]),        # (no pool on this engine)
                                     dict(N=7), dict(N=4097), dict(ess=0.0), dict(ess=1.0), dict(sweeps=0), dict(lo=[0.0, 0.5]),
                                     dict(u=last), dict(lnl=np.where(np.arange(32).reshape(2, 16) == 31, np.nan, 0.0)), dict(lnl=dead),
                                     dict(beta=[0.0, 1.5]), dict(scale=[1.0, 0.0]), dict(stage=[0, -1]), dict(stage=[0, 1 << 31]),
                                     dict(draw=True, stage=[0, 3]), dict(chunk=-1), dict(const_hint=3)]),
                        (mock_vega[0], [dict(E=1, mock_rows=[6]), dict(E=1, mock_rows=[-1]), dict(mock_rows=[0, 6])])):
        theta = vega._theta(None)[None, :]
        before = vega.chi2_batch(theta)
        for case in cases:
            _refused(vega.engine, **case)
            np.testing.assert_array_equal(vega.chi2_batch(theta), before)
    # (what was refused runs once the argument is mended: the pool has rows 0 .. 5)
    eng = mock_vega[0].engine
    u, lnl = np.zeros((1, 16, 2)), np.zeros((1, 16))
    rec, status, done, st = eng.smc_run_many([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0],
                                             eng.low.theta0.copy(), u, lnl, np.zeros(1, dtype=np.int64), np.zeros(1), np.ones(1), [0], 1,
                                             0.5, 3, mock_rows=[5], draw=True)
    assert done[0] == 1 and st['per_run'].shape == (1, 4) and st['per_run'][0, 3] == 16 * 4 and status[0] in (0, 1)


def test_evidence_for_every_mock_end_to_end(tmp_path):
    from conftest import mc_launcher_config
    from fits_standard import check_file
    from vega_amd import fitslite, run_vega_sampler
    from vega_amd.smc import SMCSet, read_stats
    config = mc_launcher_config(tmp_path)
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / config)
    cfg['control'].update(run_sampler='True', sampler='SMC')
    out = tmp_path / 'chains_mocks'
    out.mkdir()
    cfg['SMC'] = dict(path=str(out), name='run', mocks='3', particles='64', sweeps='4', seed='4')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert isinstance(sampler, SMCSet) and sampler.E == 3 and sampler.driver == 'device' and sampler.mock_rows.tolist() == [0, 1, 2]
        assert np.all(sampler.finished)
        log_z, err = sampler.log_evidence()
        pts, lnl, _ = sampler.samples()
        for m in range(3):
            table = np.loadtxt(out / f'run_mock{m}.txt')
            assert table.shape == (64, 2 + 3) and np.array_equal(table[:, 1], -lnl[m]) and np.array_equal(table[:, 2:], pts[m])
            stats = read_stats(out / f'run_mock{m}.stats')
            assert (stats['log(Z)'], stats['log(Z) error']) == (log_z[m], err[m]) and stats['stages'] == sampler.stage[m]
        assert not np.array_equal(pts[0], pts[1])
        check_file(out / 'mock_posteriors.fits')
        with fitslite.open(str(out / 'mock_posteriors.fits')) as hdus:
            data = hdus[1].data
            assert len(data) == 3 and np.all(np.isfinite(data['log_z'])) and np.all(data['log_z_err'] > 0)
            post = sampler.vega.analysis.mc_posteriors
            np.testing.assert_array_equal(data['log_z'], log_z)
            np.testing.assert_array_equal(data['ap_mean'], post['mean'][:, 0])
            np.testing.assert_array_equal(data['at_sd'], post['sd'][:, 1])
            np.testing.assert_array_equal(data['stages'], sampler.stage)
            np.testing.assert_array_equal(data['status'], [1, 1, 1])
            np.testing.assert_array_equal(np.asarray(data['covariance']).reshape(3, 3, 3), post['covariance'])
    finally:
        sampler.vega.close()


def _write_config(tmp_path, tag, section):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control'].update(run_sampler='True', sampler='SMC')
    out = tmp_path / f'chains_{tag}'
    out.mkdir()
    cfg['SMC'] = dict(section, path=str(out), name='run')
    (tmp_path / 'configs' / tag).mkdir(parents=True)
    with open(tmp_path / 'configs' / tag / 'main.ini', 'w') as f:
        cfg.write(f)
    return f'configs/{tag}/main.ini', out


def test_replicas_together_end_to_end(tmp_path):
    """``together = True`` writes the files of ``together = False`` with the same keys; the merged evidences agree within 5 of
    their combined error (the samples are not compared bit for bit: the batches are shaped differently)."""
    from vega_amd import replicas as rep
    from vega_amd import run_vega_sampler
    section = dict(replicas='2', particles='64', sweeps='4', seed='4', max_stages='3')
    stats, records = {}, {}
    for tag, extra in (('together', dict(together='True')), ('sequential', dict(together='False'))):
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
        assert rec['kind'] == 'smc' and rec['u'].shape == want['u'].shape == (64, 2)
    a, b = stats['together'], stats['sequential']
    assert set(a) == set(b) and a['replicas'] == 2 and a['particles'] == 128
    assert math.isfinite(a['log(Z)']) and abs(a['log(Z)'] - b['log(Z)']) <= 5 * math.hypot(a['log(Z) error'], b['log(Z) error'])
