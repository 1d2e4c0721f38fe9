"""The SMC sampler on the device (include/vegamx.h: vmx_smc_run) against its NumPy restatement (the `python` driver of
vega_amd/smc.py) on real engines: the same particles and ancestors bit for bit, a run that does not depend on how it is cut into
calls or chunks, the exact evidence and posterior of parameters the model is linear in, the evidence of the nested sampler on the
physical parameters, refused arguments that leave the engine as it was, engine groups, and the config switch end to end."""
import configparser
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN, synth_joint_problem
from test_nested_gpu import AUTO_SAMPLED, _linear_gaussian, _sample_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _assert_same(a, b):
    assert a.stage == b.stage and len(a.record) == len(b.record) and a.scale == b.scale
    assert a.beta == pytest.approx(b.beta, rel=1e-9)         # (beta follows lnL, which the drivers share to 1e-12)
    assert np.array_equal(a.u, b.u)
    np.testing.assert_allclose(a.lnl, b.lnl, rtol=1e-12, atol=0)
    for ra, rb in zip(a.record, b.record):
        assert np.array_equal(ra['anc'], rb['anc'])
        np.testing.assert_allclose(ra['lnl'], rb['lnl'], rtol=1e-12, atol=0)
        for key in ('beta_prev', 'beta', 'ess'):
            assert ra[key] == pytest.approx(rb[key], rel=1e-9), key
        assert ra['accepted'] == rb['accepted'] and ra['scale'] == rb['scale'] and ra['cholesky'] == rb['cholesky']
    for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model'):
        assert a.stats[key] == b.stats[key], key


def _pair(vega, sp, stages, **kw):
    from vega_amd import SMCSampler
    out = []
    for driver in ('device', 'python'):
        s = SMCSampler(vega, driver=driver, sample_params=sp, **kw)
        s.run(stages=stages)
        assert s.driver == driver
        out.append(s)
    return out


def test_drivers_agree_on_auto(auto_vega):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, sp, 2, particles=256, seed=7)
    _assert_same(dev, py)
    # (this problem's likelihood varies by about 0.01 in lnL over the box: the ladder may reach beta = 1 before the two stages)
    assert dev.sweeps == 16 and (dev.stage == 2 or dev.finished) and dev.stage == len(dev.record) >= 1
    assert dev.stats['rows'] == 256 * (1 + dev.stage * 16) and dev.stats['accepted'] > 0
    # one wait per stage (beta), the start (how many particles have a finite lnL), the call's copy back
    assert dev.stats['host_waits'] == dev.stats['stages'] + 2
    assert dev.stats['engine_calls'] == py.stats['engine_calls'] == 1 + dev.stage * 16
    assert np.all(np.diff(dev.stages['beta']) > 0) and np.all(dev.stages['ess'] >= 0.5 * 256 * (1 - 1e-12))
    np.testing.assert_allclose(dev.log_evidence(), py.log_evidence(), rtol=1e-9)


def test_drivers_agree_on_the_joint_problem_with_two_lanes():
    """N = 1024, max_batch = 256: sweeps of four chunks on two lanes."""
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        sp = _sample_params(vega, AUTO_SAMPLED)
        dev, py = _pair(vega, sp, 2, particles=1024, sweeps=6, seed=3)
        _assert_same(dev, py)
        assert dev.stage == 2 and not dev.finished and 0.0 < dev.beta < 1.0
        assert dev.stats['engine_calls'] == py.stats['engine_calls'] == 4 * (1 + 2 * 6)
        assert dev.stats['host_waits'] == dev.stats['stages'] + 2 and dev.stats['lanes'] == 2
    finally:
        vega.close()


def _linear_box(auto_vega):
    """The box b* +- 10 sd of the four linear broadband coefficients, with the exact log Z over it."""
    names, mean, cov, F, lnl_max = _linear_gaussian(auto_vega)
    sd = np.sqrt(np.diag(cov))
    log_z_true = lnl_max + 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1] - np.sum(np.log(20 * sd))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)}, 'values': dict(zip(names, mean)),
          'errors': dict(zip(names, sd))}
    return sp, mean, cov, sd, log_z_true


def test_the_run_does_not_depend_on_the_cut_or_the_chunks(auto_vega):
    """(On the linear coefficients: a ladder of several stages.)"""
    from vega_amd import SMCSampler
    sp = _linear_box(auto_vega)[0]
    kw = dict(particles=128, sweeps=5, seed=5, sample_params=sp)
    one = SMCSampler(auto_vega, **kw).run(stages=4)
    cut = SMCSampler(auto_vega, **kw)
    for _ in range(4):
        cut.run(stages=1)
    small = SMCSampler(auto_vega, chunk=16, **kw).run(stages=4)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 4 and one.stage == 4 and not one.finished
    for other in (cut, small):
        assert np.array_equal(one.u, other.u) and np.array_equal(one.lnl, other.lnl)
        assert (one.stage, one.beta, one.scale) == (other.stage, other.beta, other.scale)
        for a, b in zip(one.record, other.record):
            assert np.array_equal(a['anc'], b['anc']) and np.array_equal(a['lnl'], b['lnl'])
            assert (a['beta'], a['ess'], a['accepted'], a['scale']) == (b['beta'], b['ess'], b['accepted'], b['scale'])
        assert one.stats['rows'] == other.stats['rows'] and one.stats['accepted'] == other.stats['accepted']
    assert small.stats['engine_calls'] == 8 * one.stats['engine_calls']
    assert cut.stats['host_waits'] == 4 + 4 + 1       # (a wait per stage, a copy back per call, the start)


@pytest.mark.parametrize('N', [24, 1056])
def test_drivers_agree_at_awkward_sizes(auto_vega, N):
    """N = 24: fewer than a wavefront, padded to 32; N = 1056: more than one particle per lane and a segment length of 2.  Stream
    2, two stages of two sweeps on the linear coefficients."""
    sp = _linear_box(auto_vega)[0]
    dev, py = _pair(auto_vega, sp, 2, particles=N, sweeps=2, seed=3, stream=2)
    _assert_same(dev, py)
    assert dev.stage == 2 and 0.0 < dev.beta < 1.0 and dev.stats['rows'] == N * (1 + 2 * 2)
    assert dev.stats['host_waits'] == dev.stats['stages'] + 2


def test_linear_parameters_give_the_exact_evidence(auto_vega):
    """chi2 = chi2_min + (b - b*)^T F (b - b*) exactly, so over the box b* +- 10 sd: log Z = lnL(b*) + 1/2 log|2 pi cov| -
    sum log(20 sd) (tests/test_nested_gpu.py).  N = 1024 equal-weight particles: ESS = N in that test's bounds."""
    from vega_amd import SMCSampler
    sp, mean, cov, sd, log_z_true = _linear_box(auto_vega)
    s = SMCSampler(auto_vega, particles=1024, seed=11, sample_params=sp).run()
    assert s.finished and s.driver == 'device'
    log_z, err = s.log_evidence()
    pts, _, w = s.samples()
    ess = float(s.particles)
    got_mean = w @ pts
    d = pts - got_mean
    got_cov = (w[:, None] * d).T @ d
    print(f'log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}), '
          f'mean pulls {np.round((got_mean - mean) / (sd / np.sqrt(ess)), 2)}, stages {s.stage}, rows {s.stats["rows"]}, '
          f'seconds {s.stats["seconds"]:.3f}, acceptance {np.round(s.stages["acceptance"], 2)}')
    assert abs(log_z - log_z_true) <= 5 * err
    assert np.all(np.abs(got_mean - mean) < 5 * sd / np.sqrt(ess)), ((got_mean - mean) / sd, ess)
    tol = 5 * np.sqrt(2.0 / ess) * np.outer(sd, sd)
    assert np.all(np.abs(got_cov - cov) < tol), ((got_cov - cov) / np.outer(sd, sd), ess)


def test_the_evidence_agrees_with_the_nested_sampler(auto_vega):
    """The 4 physical parameters of the auto problem, where no analytic evidence exists: log Z of the two estimators differ by
    less than 5 times their combined error, the posterior means by less than 5 combined standard errors (sd / sqrt(N) here,
    sd / sqrt(ESS) there).  Measured: SMC -1461.4266, nested -1461.4267, pull +1.44, mean pulls within 1.1 - this likelihood varies
    by about 0.01 in lnL over the box, so both errors are below 1e-4 and the ladder has one stage."""
    from vega_amd import NestedSampler, SMCSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    smc = SMCSampler(auto_vega, particles=1024, seed=2, sample_params=sp).run()
    ns = NestedSampler(auto_vega, num_live=256, threads=64, seed=2, sample_params=sp).run()
    z_s, e_s = smc.log_evidence()
    z_n, e_n = ns.log_evidence()
    pts, _, w = ns.samples()
    ess = 1.0 / np.sum(w**2)
    mean_n = w @ pts
    sd_n = np.sqrt(w @ (pts - mean_n)**2)
    p = smc.samples()[0]
    mean_s, sd_s = p.mean(axis=0), p.std(axis=0, ddof=1)
    se = np.sqrt(sd_n**2 / ess + sd_s**2 / smc.particles)
    print(f'SMC log Z {z_s:.4f} +- {e_s:.4f} ({smc.stage} stages, {smc.stats["rows"]} rows, {smc.stats["seconds"]:.2f} s), nested '
          f'{z_n:.4f} +- {e_n:.4f} ({ns.iteration} iterations, {ns.stats["rows"]} rows, {ns.stats["seconds"]:.2f} s), pull '
          f'{(z_s - z_n) / math.hypot(e_s, e_n):+.2f}; means {mean_s} / {mean_n}, pulls {(mean_s - mean_n) / se}')
    assert smc.finished and ns.terminated and ess > 100
    assert abs(z_s - z_n) < 5 * math.hypot(e_s, e_n)
    assert np.all(np.abs(mean_s - mean_n) < 5 * se), (mean_s, mean_n, se)


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    N = changes.pop('N', 16)
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), u=np.full((N, 2), 0.5), lnl=np.zeros(N), stage=0, beta=0.0, scale=1.0,
                n_stages=2, ess=0.5, sweeps=3)
    args.update(changes)
    for k in ('u', 'lnl'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.smc_run(**args)


def test_refused_arguments_leave_the_engine_as_it_was(auto_vega):
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    i = eng.names.index('bias_eta_LYA')
    many = list(range(33))
    cases = [dict(cols=many, lo=[0.0] * 33, hi=[1.0] * 33, u=np.full((128, 33), 0.5), lnl=np.zeros(128)),       # n > 32
             dict(N=7), dict(N=4097),                                               # N outside max(2 n + 2, 8) .. 4096
             dict(ess=0.0), dict(ess=1.0), dict(sweeps=0),
             dict(cols=[i, eng.n_params]), dict(cols=[i, i]), dict(hi=[0.0, np.inf]), dict(lo=[0.0, 0.5]),
             dict(u=np.full((16, 2), 1.5)), dict(u=np.full((16, 2), -0.1)), dict(lnl=np.full(16, np.nan)),
             dict(lnl=np.full(16, -np.inf)), dict(beta=1.5), dict(scale=0.0), dict(draw=True, stage=3)]
    for case in cases:
        _refused(eng, **case)
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


def test_a_ladder_that_cannot_advance_fails_the_call_and_nothing_else(auto_vega):
    """N = 8 particles of which one has a finite lnL: ESS = 1 at every beta, below ess N = 4, so that the head hands back beta_t =
    beta_{t-1}.  vmx_smc_run answers -2; u, lnl and the stage are the caller's, and the next run is the run it was before."""
    from vega_amd import engine as G
    from vega_amd.smc import draw_start
    eng = auto_vega.engine
    box = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
               theta_fixed=eng.low.theta0.copy())

    def ordinary():
        u, lnl = np.zeros((16, 2)), np.zeros(16)
        rec, stage, beta, scale, st = eng.smc_run(u=u, lnl=lnl, stage=0, beta=0.0, scale=1.0, n_stages=1, ess=0.5, sweeps=3, seed=6,
                                                  stream=1, draw=True, **box)
        return u, lnl, rec[0]['lnl'], rec[0]['anc'], np.array([stage, beta, scale, rec[0]['accepted'], st['rows']])

    before = ordinary()
    u = np.ascontiguousarray(draw_start(8, 2, 1, 0))
    lnl = np.array([-np.inf] * 7 + [0.0])
    u0, lnl0 = u.copy(), lnl.copy()
    with pytest.raises(G.EngineError, match='cannot advance'):
        eng.smc_run(u=u, lnl=lnl, stage=0, beta=0.0, scale=1.0, n_stages=2, ess=0.5, sweeps=3, **box)
    assert np.array_equal(u, u0) and np.array_equal(lnl, lnl0)
    # the raw entry: the stage, beta, scale and statistics words are the caller's too
    cols, lo, hi, theta, _ = eng._sampled_box(box['cols'], box['lo'], box['hi'], box['theta_fixed'], u=u, lnl=lnl)
    rec, rec_lnl, rec_anc = np.full((2, G.VMX_SMC_REC), 7.0), np.full((2, 8), 7.0), np.full((2, 8), 7, dtype=np.int32)
    spec = G.SmcSpec(eng.n_params, 2, G._ip(cols), G._dp(lo), G._dp(hi), 8, 3, 0.5, 0.0, 0, 0, G._dp(theta))
    opt, stats = G.SmcOptions(-1, 0, 0, 0), G.SmcStats()
    stats.stages, stats.rows = -5, -5
    st, b, sc = C.c_int64(4), C.c_double(0.25), C.c_double(0.5)
    assert eng.lib.vmx_smc_run(eng._h, C.byref(spec), G._dp(u), G._dp(lnl), C.byref(st), C.byref(b), C.byref(sc), 2, G._dp(rec),
                               G._dp(rec_lnl), G._ip(rec_anc), C.byref(opt), C.byref(stats)) == -2
    assert b'cannot advance' in eng.lib.vmx_last_error() and (st.value, b.value, sc.value) == (4, 0.25, 0.5)
    assert np.array_equal(u, u0) and np.array_equal(lnl, lnl0) and (stats.stages, stats.rows) == (-5, -5)
    assert np.all(rec == 7.0) and np.all(rec_lnl == 7.0) and np.all(rec_anc == 7)
    for a, b in zip(ordinary(), before):
        assert np.array_equal(a, b)


def test_an_engine_group_takes_the_python_driver():
    from vega_amd import SMCSampler, VegaInterface
    from vega_amd.engine_group import EngineGroup
    prob = synth_joint_problem()
    name = [n for n, it in prob.items.items() if it.tracer1.name != it.tracer2.name][0]
    item = prob.items[name]
    for pipe in [item.core] + [m.pipeline for m in item.metals]:
        pipe.xi.fht_lowring = False
    vega = VegaInterface(None, problem=prob, max_batch=64)
    try:
        assert isinstance(vega.engine, EngineGroup)
        s = SMCSampler(vega, particles=32, sweeps=3, seed=1, driver='device',
                       sample_params=_sample_params(vega, AUTO_SAMPLED)).run(stages=2)
        assert s.driver == 'python'
        assert s.stage == 2 and s.stats['rows'] == 32 * 7 and np.isfinite(s.log_evidence()[0])
    finally:
        vega.close()


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import run_vega_sampler
    from vega_amd.smc import SMCSampler, read_stats
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'SMC'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['SMC'] = {'path': str(out), 'name': 'auto_smc', 'particles': '64', 'sweeps': '4', 'seed': '4', 'max_stages': '3'}
    (tmp_path / 'configs' / 'smc').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'smc' / 'main.ini', 'w') as f:
        cfg.write(f)
    printed = []
    sampler = run_vega_sampler('configs/smc/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *a: printed.append(a[0]))
    assert isinstance(sampler, SMCSampler) and sampler.driver == 'device'
    stages = sampler.stage          # (1 .. max_stages: this likelihood is nearly flat over the box)
    assert 1 <= stages <= 3 and (sampler.finished or stages == 3)
    table = np.loadtxt(out / 'auto_smc.txt')
    pts, lnl, w = sampler.samples()
    assert table.shape == (64, 2 + 2)
    assert np.all(table[:, 0] == 1.0) and np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    assert (out / 'auto_smc.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
    stats = read_stats(out / 'auto_smc.stats')
    assert math.isfinite(stats['log(Z)']) and (stats['log(Z)'], stats['log(Z) error']) == sampler.log_evidence()
    assert f'log(Z) = {stats["log(Z)"]} +- {stats["log(Z) error"]}' in printed
    assert stats['stages'] == stages and stats['particles'] == 64 and stats['sweeps'] == 4 and len(stats['beta']) == stages
    assert stats['likelihood evaluations'] == 64 * (1 + stages * 4) and stats['seed'] == 4
    sampler.vega.close()
