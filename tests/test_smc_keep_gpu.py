"""Kept populations and posterior rounds of the SMC sampler on the device (include/vegamx.h: vmx_smc_run_kept,
vmx_smc_run_many_kept) on the linear-broadband problem of tests/test_smc_gpu.py: with the options off the calls are the base
calls bit for bit; with them the device driver is the NumPy restatement by the criteria of tests/test_smc_gpu.py, the kept
positions included; cuts on the ladder, at beta = 1 and between posterior rounds; a set whose runs owe different numbers of
rounds; the recycled chain of three mocks against their exact posteriors; refused arguments; the config keys end to end."""
import configparser
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN
from test_ensemble_set_gpu import _linear_gaussian
from test_smc_gpu import _assert_same, _linear_box
from test_smc_set_gpu import _install, _same_records, mock_vega  # noqa: F401  (the fixture: the auto problem with a pool of 6 mocks)

pytestmark = pytest.mark.gpu

BB = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


@pytest.fixture(scope='module')
def linear_box(auto_vega):
    return _linear_box(auto_vega)[0]


def _mock_box(vega):
    """The box of tests/test_smc_set_gpu.py::test_exact_evidence_per_mock: the fit of the data +- 10 sd."""
    mean, cov = _linear_gaussian(vega, BB)
    sd = np.sqrt(np.diag(cov))
    return {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(BB, mean, sd)}, 'values': dict(zip(BB, mean)),
            'errors': dict(zip(BB, sd))}, mean, sd


# ------------------------------------------------------------------ off is the parent
def _raw_single(s, keep, n_stages=4):
    """vmx_smc_run (``keep`` = 'base') or vmx_smc_run_kept with ``keep`` (None: a NULL pointer) from the start of sampler ``s``:
    everything the call hands back."""
    from vega_amd import engine as G
    eng, N, n = s.vega.engine, s.particles, s.n
    u, lnl = np.zeros((N, n)), np.zeros(N)
    cols, lo, hi, theta, _ = eng._sampled_box(s.cols, s.lo, s.hi, s._fixed_row(), u=u, lnl=lnl)
    rec, rec_lnl, rec_anc = np.zeros((n_stages, G.VMX_SMC_REC)), np.zeros((n_stages, N)), np.zeros((n_stages, N), dtype=np.int32)
    spec = G.SmcSpec(eng.n_params, n, G._ip(cols), G._dp(lo), G._dp(hi), N, s.sweeps, s.ess, s.log_norm(), s.seed, s.stream, G._dp(theta))
    opt, stats = G.SmcOptions(-1, 0, 0, 1), G.SmcStats()
    st, b, sc = C.c_int64(0), C.c_double(0.0), C.c_double(1.0)
    head = (eng._h, C.byref(spec), G._dp(u), G._dp(lnl), C.byref(st), C.byref(b), C.byref(sc), n_stages, G._dp(rec), G._dp(rec_lnl),
            G._ip(rec_anc))
    if isinstance(keep, str):
        code = eng.lib.vmx_smc_run(*head, C.byref(opt), C.byref(stats))
    else:
        code = eng.lib.vmx_smc_run_kept(*head, None if keep is None else C.byref(keep), C.byref(opt), C.byref(stats))
    assert code == 0
    done = int(stats.stages)
    st_d = {k: v for k, v in G._stats_dict(stats).items() if not k.startswith('seconds')}
    return dict(u=u, lnl=lnl, rec=rec[:done], rec_lnl=rec_lnl[:done], rec_anc=rec_anc[:done], state=(st.value, b.value, sc.value), stats=st_d)


def test_off_is_the_base_call(auto_vega, linear_box):
    """vmx_smc_run_kept with keep = NULL, and with a struct of NULLs, hands back the u, lnL, rec, rec_lnl, rec_anc, state and
    statistics (but the seconds) of vmx_smc_run, bit for bit; so does the set call."""
    from vega_amd import SMCSampler, SMCSet
    from vega_amd import engine as G
    s = SMCSampler(auto_vega, particles=64, sweeps=4, seed=5, sample_params=linear_box)
    base = _raw_single(s, 'base')
    assert len(base['rec']) == 4 and base['state'][1] < 1.0         # (a ladder of more than three stages)
    for keep in (None, G.SmcKeep(None, None, 0), G.SmcKeep(None, C.pointer(C.c_int32(0)), 0)):
        got = _raw_single(s, keep)
        for key in ('u', 'lnl', 'rec', 'rec_lnl', 'rec_anc'):
            assert np.array_equal(got[key], base[key]), key
        assert got['state'] == base['state'] and got['stats'] == base['stats']
    # the set: the wrapper's keep=False path is vmx_smc_run_many; a struct of NULLs through vmx_smc_run_many_kept
    eng = auto_vega.engine
    one = SMCSet(auto_vega, 2, particles=64, sweeps=4, seed=5, sample_params=linear_box).run(4)
    E, N, n = 2, 64, 4
    u, lnl = np.zeros((E, N, n)), np.zeros((E, N))
    stage, beta, scale = np.zeros(E, dtype=np.int64), np.zeros(E), np.ones(E)
    cols, lo, hi, theta, _ = eng._sampled_box(one.cols, one.lo, one.hi, one._fixed_row(), u=u.reshape(-1, n), lnl=lnl.reshape(-1))
    rec, rec_lnl, rec_anc = np.zeros((E, 4, G.VMX_SMC_REC)), np.zeros((E, 4, N)), np.zeros((E, 4, N), dtype=np.int32)
    status, done, per = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32), np.zeros((E, 4), dtype=np.int64)
    streams = np.arange(E, dtype=np.uint64)
    spec = G.SmcSpec(eng.n_params, n, G._ip(cols), G._dp(lo), G._dp(hi), N, 4, 0.5, one.log_norm(), 5, 0, G._dp(theta))
    opt, stats, keep = G.SmcOptions(-1, 0, 0, 1), G.SmcStats(), G.SmcKeep(None, None, 0)
    assert eng.lib.vmx_smc_run_many_kept(
        eng._h, C.byref(spec), E, streams.ctypes.data_as(C.POINTER(C.c_uint64)), None, G._dp(u), G._dp(lnl),
        stage.ctypes.data_as(C.POINTER(C.c_int64)), G._dp(beta), G._dp(scale), G._ip(status), 4, G._dp(rec), G._dp(rec_lnl),
        G._ip(rec_anc), G._ip(done), C.byref(keep), C.byref(opt), C.byref(stats), per.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert np.array_equal(u, one.u) and np.array_equal(lnl, one.lnl) and np.array_equal(stage, one.stage)
    assert np.array_equal(beta, one.beta) and np.array_equal(scale, one.scale) and done.tolist() == [4, 4]
    for e in range(E):
        assert np.array_equal(rec_lnl[e], [r['lnl'] for r in one.record[e]]) and np.array_equal(rec_anc[e], [r['anc'] for r in one.record[e]])
        assert np.array_equal(rec[e, :, 1], [r['beta'] for r in one.record[e]])
    assert np.array_equal(per, one.stats['per_run'])
    for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model', 'engine_calls', 'host_waits'):
        assert getattr(stats, key) == one.stats[key], key


# ------------------------------------------------------------------ device against the restatement
def _assert_same_kept(dev, py):
    """tests/test_smc_gpu.py::_assert_same (particles and ancestors bit for bit, lnL to 1e-12), the rows of the posterior rounds by
    the same criteria, and the kept positions of every stage bit for bit."""
    _assert_same(dev, py)
    assert dev.topups_left == py.topups_left and len(dev.posterior_rounds) == len(py.posterior_rounds)
    _same_records(dev.posterior_rounds, py.posterior_rounds)
    for a, b in zip(dev.record + dev.posterior_rounds, py.record + py.posterior_rounds):
        assert np.array_equal(a['u'], b['u'])
    for r in dev.posterior_rounds:
        assert np.array_equal(r['anc'], np.arange(dev.particles)) and r['beta_prev'] == r['beta'] == 1.0
        assert r['ess'] == np.count_nonzero(r['lnl'] > -np.inf)
    for a, b in zip(dev.populations(), py.populations()):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)


@pytest.mark.parametrize('N, n_total, kw', [(40, 120, dict(chunk=16, sweeps=4)), (1100, 2200, dict(sweeps=2)),
                                            (256, 768, dict(chunk=128, sweeps=3))])
def test_drivers_agree_with_posterior_rounds(auto_vega, linear_box, N, n_total, kw):
    """N = 40 with chunk 16 (a sweep ends in a tail of 8 rows, N is not a multiple of a wave), N = 1100 (two particles per lane, an
    odd segment length), N = 256 in two chunks on two lanes: the ladder and then R posterior rounds."""
    from vega_amd import SMCSampler
    out = []
    for driver in ('device', 'python'):
        s = SMCSampler(auto_vega, driver=driver, particles=N, seed=7, n_total=n_total, recycle=True, sample_params=linear_box, **kw).run()
        assert s.driver == driver and s.finished
        out.append(s)
    dev, py = out
    R = -(-n_total // N) - 1
    assert len(dev.record) >= 3 and len(dev.posterior_rounds) == R and dev.stage == len(dev.record) + R
    _assert_same_kept(dev, py)
    # a wait per ladder stage, one for all the rounds, the start, the copy back
    assert dev.stats['host_waits'] == len(dev.record) + 3 and dev.stats['calls'] == 1
    assert dev.stats['rows'] == N * (1 + dev.stage * dev.sweeps)
    if N == 256:
        assert dev.stats['lanes'] == 2 and dev.stats['engine_calls'] == 2 * (1 + dev.stage * dev.sweeps)
    np.testing.assert_allclose(dev.n_eff(), py.n_eff(), rtol=1e-9)
    np.testing.assert_allclose(dev.recycled_log_evidence(), py.recycled_log_evidence(), rtol=1e-9)
    assert dev.samples()[0].shape == ((dev.stage + 1) * N, 4) and dev.samples(recycle=False)[0].shape == ((R + 1) * N, 4)


def test_the_run_does_not_depend_on_the_cut(auto_vega, linear_box):
    """``run(stages=1)`` repeated is ``run()`` bit for bit: cuts on the ladder, at beta = 1 and between two posterior rounds."""
    from vega_amd import SMCSampler
    kw = dict(particles=128, sweeps=5, seed=5, n_total=384, sample_params=linear_box)
    one = SMCSampler(auto_vega, **kw).run()
    cut = SMCSampler(auto_vega, **kw)
    seen = []
    while not cut.finished:
        cut.run(stages=1)
        seen.append((cut.beta, cut.topups_left))
    assert len(one.record) >= 3 and one.finished and seen[-3:] == [(1.0, 2), (1.0, 1), (1.0, 0)] and cut.stats['calls'] == one.stage
    assert np.array_equal(one.u, cut.u) and np.array_equal(one.lnl, cut.lnl) and (one.stage, one.scale) == (cut.stage, cut.scale)
    for a, b in zip(one.record + one.posterior_rounds, cut.record + cut.posterior_rounds):
        assert np.array_equal(a['anc'], b['anc']) and np.array_equal(a['lnl'], b['lnl']) and np.array_equal(a['u'], b['u'])
        assert (a['beta'], a['ess'], a['accepted'], a['scale']) == (b['beta'], b['ess'], b['accepted'], b['scale'])
    assert len(one.posterior_rounds) == len(cut.posterior_rounds) == 2 and one.log_evidence() == cut.log_evidence()
    assert one.stats['rows'] == cut.stats['rows'] and one.stats['accepted'] == cut.stats['accepted']
    assert cut.stats['host_waits'] == 2 * one.stage + 1      # (a wait per stage or round, a copy back per call, the start)


# ------------------------------------------------------------------ sets
def test_a_set_of_one_is_the_single_kept_run(auto_vega, linear_box):
    from vega_amd import SMCSampler, SMCSet
    kw = dict(particles=64, sweeps=4, seed=7, n_total=192, recycle=True, sample_params=linear_box)
    both = SMCSet(auto_vega, 1, streams=[3], **kw).run()
    one = SMCSampler(auto_vega, stream=3, **kw).run()
    assert len(one.record) >= 3 and one.finished and both.finished[0] and both.status[0] == 1 and both.topups_left[0] == 0
    assert np.array_equal(both.u[0], one.u) and np.array_equal(both.lnl[0], one.lnl)
    assert (both.stage[0], both.beta[0], both.scale[0]) == (one.stage, one.beta, one.scale)
    assert len(both.record[0]) == len(one.record) and len(both.posterior_rounds[0]) == len(one.posterior_rounds) == 2
    for a, b in zip(both.record[0] + both.posterior_rounds[0], one.record + one.posterior_rounds):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    member = both.member(0)
    for a, b in zip(member.populations(), one.populations()):
        assert np.array_equal(a, b)
    for a, b in zip(member.samples(), one.samples()):
        assert np.array_equal(a, b)
    assert member.n_eff() == one.n_eff() == both.n_eff()[0] and member.recycled_log_evidence() == both.recycled_log_evidence()[0]
    assert member.log_evidence() == one.log_evidence() and member.finished


@pytest.mark.parametrize('kept', [False, True])
def test_the_exported_entries_side_by_side(auto_vega, linear_box, kept):
    """``Engine.smc_run`` (vmx_smc_run, vmx_smc_run_kept) beside ``Engine.smc_run_many`` with E = 1 (vmx_smc_run_many,
    vmx_smc_run_many_kept) at N = 24 on stream 2: a call of two stages from the draw, then a call entered at stage 2 that ends
    the run - with ``kept``, through the two posterior rounds owed.  Every array and every statistic is equal but the seconds and
    ``host_waits``, which follows each entry's own rule (include/vegamx.h)."""
    from vega_amd import SMCSampler
    N, n, sweeps = 24, 4, 2
    s = SMCSampler(auto_vega, particles=N, sweeps=sweeps, seed=3, stream=2, sample_params=linear_box)
    eng = auto_vega.engine
    kw = dict(log_norm=s.log_norm(), seed=3)
    u1, l1 = np.zeros((N, n)), np.zeros(N)
    uE, lE = np.zeros((1, N, n)), np.zeros((1, N))
    stage, beta, scale = np.zeros(1, dtype=np.int64), np.zeros(1), np.ones(1)
    left = np.full(1, 2, dtype=np.int32)
    one = (0, 0.0, 1.0, 2)
    for call, n_stages in enumerate((2, 40)):
        draw = call == 0
        out = eng.smc_run(s.cols, s.lo, s.hi, s._fixed_row(), u1, l1, one[0], one[1], one[2], n_stages, 0.5, sweeps, stream=2, draw=draw,
                          **(dict(keep=True, topups_left=one[3]) if kept else {}), **kw)
        rec1, st1 = out[0], out[-1]
        one = out[1:4] + ((out[4],) if kept else (0,))
        recE, status, done, stE = eng.smc_run_many(s.cols, s.lo, s.hi, s._fixed_row(), uE, lE, stage, beta, scale, [2], n_stages, 0.5, sweeps,
                                                   draw=draw, **(dict(keep=True, topups_left=left) if kept else {}), **kw)
        assert np.array_equal(uE[0], u1) and np.array_equal(lE[0], l1)
        assert (int(stage[0]), float(beta[0]), float(scale[0])) == one[:3] and done[0] == len(rec1) == len(recE[0]) == st1['stages']
        assert not kept or int(left[0]) == one[3]
        for a, b in zip(rec1, recE[0]):
            assert set(a) == set(b) and ('u' in a) == kept
            for key in a:
                assert np.array_equal(a[key], b[key]), key
        for key in st1:
            if not key.startswith('seconds') and key != 'host_waits':
                assert st1[key] == stE[key], key
        assert stE['per_run'].tolist() == [[st1['accepted'], st1['rows_own_position'], st1['rejected_failed_model'], st1['rows']]]
        ladder = sum(1 for r in rec1 if r['beta_prev'] < 1.0)
        rounds = len(rec1) - ladder
        assert st1['host_waits'] == ladder + (1 if rounds else 0) + 1 + (1 if draw else 0)
        assert stE['host_waits'] == len(rec1) + 1 + (1 if draw else 0)
        if call == 0:
            assert one[0] == 2 and 0.0 < one[1] < 1.0 and status[0] == 0
    assert one[1] == 1.0 and status[0] == 1 and rounds == (2 if kept else 0) and ladder >= 1 and one[0] == 2 + ladder + rounds < 42
    assert one[3] == 0


def test_runs_that_owe_different_rounds(mock_vega):  # noqa: F811
    """E = 3 x N = 64 through the engine's call with topups_left = (2, 0, 1), streams (0, 1, 1) and mock rows (2, 0, 0), round by
    round and whole, against ``python_stages_many`` (the python driver of SMCSet): the statuses after every round, the active
    list shrinking in the right rounds, stages_done, the per-run rows, the kept positions; run 1, which owes nothing, is the run
    of the base set call on the same inputs bit for bit."""
    from vega_amd import SMCSet
    vega = _install(mock_vega)
    sp = _mock_box(vega)[0]
    N, sweeps, owed0 = 64, 4, [2, 0, 1]
    kw = dict(particles=N, sweeps=sweeps, seed=7, streams=[0, 1, 1], mock_rows=[2, 0, 0], sample_params=sp, n_total=3 * N)

    def new(driver):
        s = SMCSet(vega, 3, driver=driver, **kw)
        s.topups_left[:] = owed0
        return s

    py, dev = new('python'), new('device')
    history = []
    while not np.all(py.finished):
        py.run(1)
        dev.run(1)
        history.append(dev.status.tolist())
        assert np.array_equal(dev.status, py.status) and np.array_equal(dev.topups_left, py.topups_left)
        assert np.array_equal(dev.stage, py.stage) and np.array_equal(dev.u, py.u)
        assert dev.stats['rows'] == py.stats['rows']         # (the rows of the runs still in the list, no others)
    ladder = np.array([len(r) for r in dev.record])
    assert np.all(ladder >= 3) and [len(r) for r in dev.posterior_rounds] == owed0 and dev.topups_left.tolist() == [0, 0, 0]
    assert np.array_equal(dev.stage, ladder + owed0) and history[-1] == [1, 1, 1]
    ends = [min(k for k, h in enumerate(history) if h[e] == 1) + 1 for e in range(3)]
    assert ends == (ladder + owed0).tolist()                  # (a run is RUNNING until the round that pays its last one)
    assert np.array_equal(dev.stats['per_run'][:, 3], (ladder + owed0) * sweeps * N + N)
    np.testing.assert_allclose(dev.lnl, py.lnl, rtol=1e-12, atol=0)
    for e in range(3):
        _same_records(dev.record[e], py.record[e])
        _same_records(dev.posterior_rounds[e], py.posterior_rounds[e])
        for a, b in zip(dev.record[e] + dev.posterior_rounds[e], py.record[e] + py.posterior_rounds[e]):
            assert np.array_equal(a['u'], b['u'])
    assert np.array_equal(dev.stats['per_run'], py.stats['per_run'])
    # one call for everything is the same set; so is the engine's call
    whole = new('device').run()
    assert whole.stats['calls'] == 1 and np.array_equal(whole.u, dev.u) and np.array_equal(whole.lnl, dev.lnl)
    assert np.array_equal(whole.stage, dev.stage) and whole.stats['host_waits'] == int(dev.stage.max()) + 2
    assert whole.stats['stages'] == int(dev.stage.sum()) and np.array_equal(whole.stats['per_run'], dev.stats['per_run'])
    # run 1 against the base call
    base = SMCSet(vega, 3, driver='device', **{k: v for k, v in kw.items() if k != 'n_total'}).run()
    assert np.array_equal(base.u[1], whole.u[1]) and np.array_equal(base.lnl[1], whole.lnl[1]) and base.stage[1] == whole.stage[1]
    assert base.scale[1] == whole.scale[1] and np.array_equal(base.stats['per_run'][1], whole.stats['per_run'][1])
    for a, b in zip(base.record[1], whole.record[1]):
        assert np.array_equal(a['anc'], b['anc']) and np.array_equal(a['lnl'], b['lnl'])
        assert (a['beta'], a['ess'], a['accepted'], a['scale']) == (b['beta'], b['ess'], b['accepted'], b['scale'])
    # equal stream, equal mock: runs 1 and 2 share their ladder, and run 2 goes one round further
    assert np.array_equal(whole.record[2][-1]['anc'], whole.record[1][-1]['anc']) and np.array_equal(whole.posterior_rounds[2][0]['u'], whole.u[1])


# ------------------------------------------------------------------ physics
NEFF_FACTOR = 5.46      # n_eff / N of the restatement at n = 4, N = 256, n_total = 1024, recycle: the lowest of seeds 0 .. 5


def test_recycled_posteriors_of_three_mocks(mock_vega, tmp_path):  # noqa: F811
    """Three mocks of the linear-broadband problem at N = 256 through ``sample_mocks(sampler='smc', n_total=1024, recycle=True)``
    against the same call without the options: log_z is equal; n_eff >= 0.77 x NEFF_FACTOR x N (the restatement on a correlated
    Gaussian of that shape, n = 4, N = 256, 6 stages, seeds 0 .. 5: n_eff / N 5.46 - 5.68); every mean within 5 sd / sqrt(N) of the exact
    posterior's (the device MIGRAD fit of the mock) and every sd within 5 sd / sqrt(2 N) - the base chain's bars; the table has
    the new columns."""
    from vega_amd import fitslite
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega[0]
    sp, mean, sd = _mock_box(vega)
    M, N = 3, 256
    mc = MonteCarlo(vega)
    vega.freeze_metals()
    mocks = mc.create_mocks(vega.compute_model(dict(zip(BB, mean))), M, seed=1)
    fits = mc._fit_mocks(mocks, M, sample_params=sp)
    assert np.all(fits.is_valid) and np.all(np.abs(fits.values - mean) <= 2 * sd)
    base = mc.sample_mocks(mocks=mocks, seed=11, sample_params=sp, sampler='smc', particles=N)
    base_post = mc.mc_posteriors
    assert set(base_post) == {'sampler', 'names', 'mean', 'sd', 'covariance', 'log_z', 'log_z_err', 'stages', 'status', 'acceptance',
                              'particles', 'ess', 'sweeps', 'seed', 'driver', 'stats'}
    sampler = mc.sample_mocks(mocks=mocks, seed=11, sample_params=sp, sampler='smc', particles=N, n_total=1024, recycle=True)
    post = mc.mc_posteriors
    assert sampler.driver == 'device' and np.all(sampler.finished) and list(sampler.status) == [1] * M
    assert np.all(post['stages'] >= 3) and np.array_equal(post['stages'], base_post['stages'])
    assert np.array_equal(post['log_z'], base_post['log_z']) and np.array_equal(post['log_z_err'], base_post['log_z_err'])
    assert np.array_equal(post['points'], (post['stages'] + 4) * N) and post['n_total'] == 1024 and post['recycle'] is True
    for m in range(M):
        sd_m = np.sqrt(np.diag(fits.covariance[m]))
        mean_pull = (post['mean'][m] - fits.values[m]) / (sd_m / math.sqrt(N))
        sd_pull = (post['sd'][m] - sd_m) / (sd_m / math.sqrt(2 * N))
        print(f'mock {m}: n_eff / N {post["n_eff"][m] / N:.3f}, log Z {post["log_z"][m]:.4f} recycled {post["log_z_recycled"][m]:.4f} '
              f'(err {post["log_z_err"][m]:.4f}), mean pulls {np.round(mean_pull, 2).tolist()}, sd pulls {np.round(sd_pull, 2).tolist()}')
    for m in range(M):
        sd_m = np.sqrt(np.diag(fits.covariance[m]))
        assert post['n_eff'][m] >= 0.77 * NEFF_FACTOR * N
        assert np.all(np.abs(post['mean'][m] - fits.values[m]) <= 5 * sd_m / math.sqrt(N))
        assert np.all(np.abs(post['sd'][m] - sd_m) <= 5 * sd_m / math.sqrt(2 * N))
        pts, lnl, w = mc.mc_chains[m]
        assert pts.shape == (post['points'][m], 4) and abs(w.sum() - 1.0) <= 1e-12
    path = mc.write_mock_posteriors(tmp_path)
    with fitslite.open(str(path)) as hdus:
        data, header = hdus[1].data, hdus[1].header
        np.testing.assert_array_equal(data['points'], post['points'])
        np.testing.assert_array_equal(data['n_eff'], post['n_eff'])
        np.testing.assert_array_equal(data['log_z_recycled'], post['log_z_recycled'])
        np.testing.assert_array_equal(data['log_z'], base_post['log_z'])
        assert header['NTOTAL'] == 1024 and bool(header['RECYCLE']) is True


# ------------------------------------------------------------------ refusals
def test_refused_arguments_leave_the_engine_as_it_was(auto_vega, linear_box):
    from vega_amd import SMCSampler
    from vega_amd import engine as G
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    s = SMCSampler(auto_vega, particles=64, sweeps=4, seed=5, sample_params=linear_box)
    eng, N, n = auto_vega.engine, 64, 4
    rec_u = np.zeros((2, N, n))
    for keep in (G.SmcKeep(G._dp(rec_u), C.pointer(C.c_int32(1)), 1),              # flags
                 G.SmcKeep(G._dp(rec_u), C.pointer(C.c_int32(-1)), 0),             # a negative count
                 G.SmcKeep(None, C.pointer(C.c_int32(1)), 0)):                     # rounds owed, nowhere to keep them
        u, lnl = np.zeros((N, n)), np.zeros(N)
        cols, lo, hi, th, _ = eng._sampled_box(s.cols, s.lo, s.hi, s._fixed_row(), u=u, lnl=lnl)
        rec, rec_lnl, rec_anc = np.zeros((2, G.VMX_SMC_REC)), np.zeros((2, N)), np.zeros((2, N), dtype=np.int32)
        spec = G.SmcSpec(eng.n_params, n, G._ip(cols), G._dp(lo), G._dp(hi), N, 4, 0.5, 0.0, 5, 0, G._dp(th))
        opt, stats = G.SmcOptions(-1, 0, 0, 1), G.SmcStats()
        st, b, sc = C.c_int64(0), C.c_double(0.0), C.c_double(1.0)
        assert eng.lib.vmx_smc_run_kept(eng._h, C.byref(spec), G._dp(u), G._dp(lnl), C.byref(st), C.byref(b), C.byref(sc), 2, G._dp(rec),
                                        G._dp(rec_lnl), G._ip(rec_anc), C.byref(keep), C.byref(opt), C.byref(stats)) == -1
        assert not u.any() and st.value == 0
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
        status, done = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        stage, beta, scale, streams = np.zeros(1, dtype=np.int64), np.zeros(1), np.ones(1), np.zeros(1, dtype=np.uint64)
        assert eng.lib.vmx_smc_run_many_kept(
            eng._h, C.byref(spec), 1, streams.ctypes.data_as(C.POINTER(C.c_uint64)), None, G._dp(u), G._dp(lnl),
            stage.ctypes.data_as(C.POINTER(C.c_int64)), G._dp(beta), G._dp(scale), G._ip(status), 2, G._dp(rec), G._dp(rec_lnl),
            G._ip(rec_anc), G._ip(done), C.byref(keep), C.byref(opt), C.byref(stats), None) == -1
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    with pytest.raises(G.EngineError, match='invalid argument'):
        eng.smc_run(s.cols, s.lo, s.hi, s._fixed_row(), np.full((N, n), 0.5), np.zeros(N), 0, 1.0, 1.0, 2, 0.5, 4, topups_left=-2)
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # a run entered at beta = 1 that owes rounds is accepted: one round, the particles move
    u, lnl = np.full((N, n), 0.5), np.zeros(N)
    rec, stage, beta, scale, left, st = eng.smc_run(s.cols, s.lo, s.hi, s._fixed_row(), u, lnl, 9, 1.0, 0.1, 1, 0.5, 4, topups_left=2,
                                                    log_norm=s.log_norm())
    assert (stage, beta, left, len(rec)) == (10, 1.0, 1, 1) and st['rows'] == 4 * N and st['host_waits'] == 2
    assert rec[0]['beta_prev'] == 1.0 and rec[0]['ess'] == N and np.array_equal(rec[0]['u'], np.full((N, n), 0.5)) and rec[0]['cholesky'] is False


# ------------------------------------------------------------------ the config keys end to end
def test_mocks_with_both_keys_end_to_end(tmp_path):
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
    cfg['SMC'] = dict(path=str(out), name='run', mocks='3', particles='64', sweeps='4', seed='4', n_total='200', recycle='True')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert isinstance(sampler, SMCSet) and sampler.E == 3 and sampler.driver == 'device' and np.all(sampler.finished)
        assert sampler.rounds == 3 and sampler.recycle and all(len(r) == 3 for r in sampler.posterior_rounds)
        log_z, err = sampler.log_evidence()
        pts, lnl, w = sampler.samples()
        post = sampler.vega.analysis.mc_posteriors
        for m in range(3):
            ladder = len(sampler.record[m])
            table = np.loadtxt(out / f'run_mock{m}.txt')
            assert table.shape == ((ladder + 4) * 64, 2 + 3) and np.array_equal(table[:, 1], -lnl[m]) and np.array_equal(table[:, 2:], pts[m])
            assert ladder >= 3
            # (weights down to the subnormals, which carry few bits: an absolute floor far below any weight that counts)
            assert table[:, 0].max() == 1.0 and np.allclose(table[:, 0] * w[m].max(), w[m], rtol=1e-13, atol=1e-280)
            stats = read_stats(out / f'run_mock{m}.stats')
            assert (stats['log(Z)'], stats['log(Z) error']) == (log_z[m], err[m]) and stats['stages'] == ladder
            assert stats['posterior rounds'] == 3 and stats['posterior points'] == (ladder + 4) * 64
            assert stats['n_eff'] == post['n_eff'][m] and stats['log(Z) recycled'] == post['log_z_recycled'][m]
        check_file(out / 'mock_posteriors.fits')
        with fitslite.open(str(out / 'mock_posteriors.fits')) as hdus:
            data, header = hdus[1].data, hdus[1].header
            np.testing.assert_array_equal(data['log_z'], log_z)
            np.testing.assert_array_equal(data['n_eff'], post['n_eff'])
            np.testing.assert_array_equal(data['points'], post['points'])
            np.testing.assert_array_equal(data['stages'], [len(r) for r in sampler.record])
            assert header['NTOTAL'] == 200 and bool(header['RECYCLE']) is True
    finally:
        sampler.vega.close()
