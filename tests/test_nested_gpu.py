"""The nested sampler on the device (include/vegamx.h: vmx_nested_run) against its NumPy restatement (the `python` driver of
vega_amd/nested.py) on real engines: the same dead record and live set bit for bit, a run that does not depend on how it is cut
into calls or chunks, the exact evidence and posterior of parameters the model is linear in, agreement with the ensemble sampler,
refused arguments that leave the engine as it was, engine groups, and the config switch end to end."""
import configparser
import math

import numpy as np
import pytest

from conftest import GOLDEN, synth_joint_problem

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
LIMITS = {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0), 'ap': (0.5, 1.5), 'at': (0.5, 1.5)}


def _sample_params(vega, names, limits=None):
    limits = limits or {}
    return {'limits': {n: limits.get(n, LIMITS[n]) for n in names}, 'values': {n: vega.params[n] for n in names}, 'errors': {}}


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _assert_same(a, b):
    for x, y in zip(a.dead(), b.dead()):
        assert x.shape == y.shape
    assert np.array_equal(a.dead()[0], b.dead()[0]) and np.array_equal(a.dead()[2], b.dead()[2])
    np.testing.assert_allclose(a.dead()[1], b.dead()[1], rtol=1e-12, atol=0)
    assert np.array_equal(a.live_u, b.live_u)
    np.testing.assert_allclose(a.live_lnl, b.live_lnl, rtol=1e-12, atol=0)
    assert a.iteration == b.iteration
    for key in ('rows', 'rounds', 'rows_own_position', 'iterations'):
        assert a.stats[key] == b.stats[key], key


def _pair(vega, sp, iterations, **kw):
    from vega_amd import NestedSampler
    out = []
    for driver in ('device', 'python'):
        s = NestedSampler(vega, driver=driver, sample_params=sp, **kw)
        s.run(iterations=iterations)
        assert s.driver == driver
        out.append(s)
    return out


def test_drivers_agree_on_auto(auto_vega):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, sp, 6, num_live=256, threads=64, seed=7)
    _assert_same(dev, py)
    assert dev.dead()[0].shape == (6 * 64, 4) and dev.num_repeats == 20
    assert np.array_equal(dev.dead()[2], np.tile(256 - np.arange(64), 6))
    assert np.all(np.diff(dev.dead()[1].reshape(6, 64), axis=1) >= 0)
    assert dev.stats['rounds'] >= 6 * 20 * 3 and dev.stats['rows'] > 256
    # one wait per round (the row count), one per iteration (nothing asked: live and dead lnL), the call's copy back, the draw
    assert dev.stats['host_waits'] == dev.stats['rounds'] + dev.stats['iterations'] + 1 + 1
    assert dev.stats['engine_calls'] == dev.stats['rounds'] + 1
    assert np.isfinite(dev.log_evidence()[0])
    np.testing.assert_allclose(dev.log_evidence(), py.log_evidence(), rtol=1e-9)


def test_drivers_agree_on_the_joint_problem_with_two_lanes():
    """K = 512 threads, max_batch = 256: rounds of two chunks on two lanes."""
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        sp = _sample_params(vega, AUTO_SAMPLED)
        dev, py = _pair(vega, sp, 2, num_live=1024, threads=512, seed=3)
        _assert_same(dev, py)
        assert dev.stats['engine_calls'] > dev.stats['rounds'] + 4
        assert dev.stats['engine_calls'] == py.stats['engine_calls']
    finally:
        vega.close()


def test_the_run_does_not_depend_on_the_cut(auto_vega):
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    kw = dict(num_live=128, threads=64, num_repeats=8, seed=5, sample_params=sp)
    one = NestedSampler(auto_vega, **kw).run(iterations=6)
    cut = NestedSampler(auto_vega, **kw)
    for _ in range(3):
        cut.run(iterations=2)
    small = NestedSampler(auto_vega, chunk=16, **kw).run(iterations=6)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 3
    for other in (cut, small):
        for a, b in zip(one.dead(), other.dead()):
            assert np.array_equal(a, b)
        assert np.array_equal(one.live_u, other.live_u) and np.array_equal(one.live_lnl, other.live_lnl)
        assert one.stats['rows'] == other.stats['rows'] and one.stats['rounds'] == other.stats['rounds']
    assert small.stats['engine_calls'] > one.stats['engine_calls']


def _linear_gaussian(auto_vega):
    """F, b*, lnL(b*) of 4 additive broadband coefficients (chi2 is exactly quadratic in them) from second differences."""
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
    chi2_min = float(chi2_at([mean - b0])[0])
    return names, mean, cov, F, float(auto_vega._log_norm()) - 0.5 * chi2_min


def test_linear_parameters_give_the_exact_evidence(auto_vega):
    """chi2 = chi2_min + (b - b*)^T F (b - b*) exactly, so lnL = lnL(b*) - 1/2 (b - b*)^T cov^-1 (b - b*) with the posterior
    covariance cov = F^-1.  Over the box b* +- 10 sd: log Z = lnL(b*) + 1/2 log|2 pi cov| - sum log(20 sd)."""
    from vega_amd import NestedSampler
    names, mean, cov, F, lnl_max = _linear_gaussian(auto_vega)
    sd = np.sqrt(np.diag(cov))
    log_z_true = lnl_max + 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1] - np.sum(np.log(20 * sd))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)}, 'values': dict(zip(names, mean)),
          'errors': dict(zip(names, sd))}
    s = NestedSampler(auto_vega, num_live=256, threads=64, seed=11, sample_params=sp).run()
    assert s.terminated and s.driver == 'device'
    log_z, err = s.log_evidence()
    pts, _, w = s.samples()
    ess = 1.0 / np.sum(w**2)
    got_mean = w @ pts
    d = pts - got_mean
    got_cov = (w[:, None] * d).T @ d
    print(f'log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}), ESS {ess:.0f}, '
          f'mean pulls {np.round((got_mean - mean) / (sd / np.sqrt(ess)), 2)}, iterations {s.iteration}, rows {s.stats["rows"]}')
    assert abs(log_z - log_z_true) <= 4 * err
    assert np.all(np.abs(got_mean - mean) < 5 * sd / np.sqrt(ess)), ((got_mean - mean) / sd, ess)
    tol = 5 * np.sqrt(2.0 / ess) * np.outer(sd, sd)
    assert np.all(np.abs(got_cov - cov) < tol), ((got_cov - cov) / np.outer(sd, sd), ess)


def test_agreement_with_the_ensemble_sampler(auto_vega):
    """The 4 physical parameters of the auto problem: posterior means of the two samplers differ by less than 5 combined standard
    errors (sd / sqrt(ESS) here, sd / sqrt(N / tau) there)."""
    from vega_amd import EnsembleSampler, NestedSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    ns = NestedSampler(auto_vega, num_live=256, threads=64, seed=2, sample_params=sp).run()
    pts, _, w = ns.samples()
    ess = 1.0 / np.sum(w**2)
    mean = w @ pts
    sd = np.sqrt(w @ (pts - mean)**2)
    sp_e = dict(sp, values=dict(zip(AUTO_SAMPLED, mean)), errors=dict(zip(AUTO_SAMPLED, sd)))
    burn = 200
    es = EnsembleSampler(auto_vega, 64, seed=3, sample_params=sp_e).run(700)
    flat = es.get_chain(discard=burn, flat=True)
    n_eff = flat.shape[0] / es.get_autocorr_time(discard=burn).max()
    se = np.sqrt(sd**2 / ess + flat.std(axis=0)**2 / n_eff)
    print(f'nested {mean} (ESS {ess:.0f}), ensemble {flat.mean(axis=0)} (N_eff {n_eff:.0f}), pulls {(mean - flat.mean(axis=0)) / se}, '
          f'log Z {ns.log_evidence()}, iterations {ns.iteration}')
    assert ns.terminated and ess > 100 and n_eff > 100
    assert np.all(np.abs(mean - flat.mean(axis=0)) < 5 * se), (mean, flat.mean(axis=0), se)


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    nlive = changes.pop('nlive', 16)
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), live_u=np.full((nlive, 2), 0.5), live_lnl=np.zeros(nlive), iteration=0,
                n_iterations=2, threads=4, num_repeats=3)
    args.update(changes)
    for k in ('live_u', 'live_lnl'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.nested_run(**args)


def test_refused_arguments_leave_the_engine_as_it_was(auto_vega):
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    i = eng.names.index('bias_eta_LYA')
    many = list(range(33))
    cases = [dict(cols=many, lo=[0.0] * 33, hi=[1.0] * 33, live_u=np.full((64, 33), 0.5), live_lnl=np.zeros(64)),   # n > 32
             dict(nlive=3), dict(nlive=4097),                                   # nlive outside n + 2 .. 4096
             dict(threads=0), dict(threads=14),                                 # K outside 1 .. nlive - n - 1
             dict(num_repeats=0), dict(cols=[i, eng.n_params]), dict(cols=[i, i]), dict(hi=[0.0, np.inf]), dict(lo=[0.0, 0.5]),
             dict(live_u=np.full((16, 2), 1.5)), dict(live_u=np.full((16, 2), -0.1)), dict(live_lnl=np.full(16, np.nan)),
             dict(draw_live=True, iteration=3)]
    for case in cases:
        _refused(eng, **case)
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


def test_an_engine_group_takes_the_python_driver():
    from vega_amd import NestedSampler, VegaInterface
    from vega_amd.engine_group import EngineGroup
    prob = synth_joint_problem()
    name = [n for n, it in prob.items.items() if it.tracer1.name != it.tracer2.name][0]
    item = prob.items[name]
    for pipe in [item.core] + [m.pipeline for m in item.metals]:
        pipe.xi.fht_lowring = False
    vega = VegaInterface(None, problem=prob, max_batch=64)
    try:
        assert isinstance(vega.engine, EngineGroup)
        s = NestedSampler(vega, num_live=32, threads=8, num_repeats=4, seed=1, driver='device',
                          sample_params=_sample_params(vega, AUTO_SAMPLED)).run(iterations=2)
        assert s.driver == 'python'
        assert s.dead()[0].shape == (16, 4) and s.stats['rows'] > 32 and np.isfinite(s.log_evidence()[0])
    finally:
        vega.close()


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import run_vega_sampler
    from vega_amd.nested import NestedSampler, read_stats
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Nested'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Nested'] = {'path': str(out), 'name': 'auto_nested', 'num_live': '64', 'num_repeats': '4', 'threads': '16', 'seed': '4',
                     'max_iterations': '5'}
    (tmp_path / 'configs' / 'ns').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ns' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ns/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    assert isinstance(sampler, NestedSampler) and sampler.driver == 'device' and sampler.iteration == 5
    table = np.loadtxt(out / 'auto_nested.txt')
    pts, lnl, w = sampler.samples()
    assert table.shape == (5 * 16 + 64, 2 + 2)
    assert np.array_equal(table[:, 0], w / w.max()) and np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    assert (out / 'auto_nested.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
    stats = read_stats(out / 'auto_nested.stats')
    assert math.isfinite(stats['log(Z)']) and (stats['log(Z)'], stats['log(Z) error']) == sampler.log_evidence()
    assert stats['iterations'] == 5 and stats['num_live'] == 64 and stats['threads'] == 16
    sampler.vega.close()
