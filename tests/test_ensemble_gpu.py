"""The ensemble sampler on the device (include/vegamx.h: vmx_ensemble_run) against its NumPy restatement (the `python` driver of
vega_amd/ensemble.py) on real engines: the same decisions and positions bit for bit, a chain that does not depend on how a run is
cut into calls, the exact Gaussian posterior of parameters the model is linear in, the box and failed models, refused arguments
that leave the engine as it was, engine groups, and the config switch end to end."""
import configparser

import numpy as np
import pytest

from conftest import GOLDEN, synth_joint_problem

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']


def _sample_params(vega, names, limits=None, scale=None):
    defaults = {'bias_eta_LYA': ((-0.5, 0.0), 0.01), 'beta_LYA': ((0.5, 3.0), 0.05), 'ap': ((0.5, 1.5), 0.01),
                'at': ((0.5, 1.5), 0.01)}
    limits = limits or {}
    return {'limits': {n: limits.get(n, defaults[n][0]) for n in names}, 'values': {n: vega.params[n] for n in names},
            'errors': {n: defaults[n][1] * (scale or 1.0) for n in names}}


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _pair(vega, W, steps, sp, seed=7, segment=1000, **kw):
    from vega_amd import EnsembleSampler
    out = []
    for driver in ('device', 'python'):
        s = EnsembleSampler(vega, W, seed=seed, driver=driver, sample_params=sp, segment=segment, **kw)
        s.run(steps)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    assert np.array_equal(dev.accepted, py.accepted)
    assert np.array_equal(dev.get_chain(), py.get_chain())
    a, b = dev.get_log_lik(), py.get_log_lik()
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    assert dev.stats['accepted'] == py.stats['accepted'] and dev.stats['rejected_outside_box'] == py.stats['rejected_outside_box']


def test_drivers_agree_on_auto(auto_vega):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, 64, 60, sp)
    _assert_same(dev, py)
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']
    assert dev.stats['host_synchronisations'] == dev.stats['calls'] == 1
    assert dev.get_chain().shape == (60, 64, 4)


def test_drivers_agree_on_the_joint_problem_with_two_lanes():
    """W = 1024: halves of 512 walkers, two chunks of max_batch = 256, two lanes."""
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=256)
    try:
        sp = _sample_params(vega, AUTO_SAMPLED)
        dev, py = _pair(vega, 1024, 6, sp)
        _assert_same(dev, py)
        assert dev.stats['engine_calls'] == 6 * 2 * 2
        assert dev.stats['accepted'] > 0
    finally:
        vega.close()


@pytest.mark.parametrize('W, steps, calls_per_half', [(8, 10, 1), (2112, 3, 5)])
def test_drivers_agree_at_both_ends_of_the_block_size(auto_vega, W, steps, calls_per_half):
    """The block of the half-step kernel follows the half: H = 4, far below one wave, a block of 64; H = 1056, beyond the 1024
    threads of a block, so the strided loop runs, its rows in 5 chunks of max_batch = 256."""
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, W, steps, sp)
    _assert_same(dev, py)
    assert dev.get_chain().shape == (steps, W, 4)
    assert 0 < dev.stats['accepted'] < dev.stats['proposals'] == steps * W
    assert dev.stats['engine_calls'] == steps * 2 * calls_per_half and dev.stats['host_synchronisations'] == 1


def test_chain_is_independent_of_the_cut(auto_vega):
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    one = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp).run(60)
    two = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp, segment=30).run(60)
    assert np.array_equal(one.get_chain(), two.get_chain()) and np.array_equal(one.get_log_lik(), two.get_log_lik())
    assert np.array_equal(one.accepted, two.accepted)
    assert one.get_chain().shape == (30, 64, 4)
    assert one.stats['calls'] == 1 and two.stats['calls'] == 2
    assert one.stats['host_synchronisations'] == 1 and two.stats['host_synchronisations'] == 2


def test_linear_parameters_sample_the_exact_gaussian_posterior(auto_vega):
    """4 of the 12 additive post-distortion broadband coefficients, everything else fixed: chi2 is exactly quadratic in them, the
    posterior exactly Gaussian with precision F (chi2 = (b - b*)^T F (b - b*) + const).  F and b* from the engine's chi2 at unit
    offsets (second differences of a quadratic are exact up to rounding).  The chain's mean and covariance must agree within
    5 standard errors of an effective sample size N / tau_max (tau from the chain)."""
    from vega_amd import EnsembleSampler
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
    F, g = fit(sd)                               # (again with offsets of the posterior's own size)
    cov = np.linalg.inv(F)
    mean = b0 - 0.5 * cov @ g
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 30 * s, m + 30 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    W, steps, burn = 64, 500, 150
    s = EnsembleSampler(auto_vega, W, seed=11, sample_params=sp).run(steps)
    post = s.get_chain(discard=burn)
    tau = s.get_autocorr_time(discard=burn)
    flat = post.reshape(-1, len(cols))
    n_eff = flat.shape[0] / tau.max()
    assert n_eff > 100, tau
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - mean) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - cov) < tol), ((np.cov(flat.T) - cov) / np.outer(sd, sd), n_eff)


def test_box_edges_and_failed_models(auto_vega):
    from vega_amd import EnsembleSampler
    # a box edge inside the posterior: nothing outside it is ever accepted
    v = auto_vega.params['beta_LYA']
    sp = _sample_params(auto_vega, AUTO_SAMPLED, limits={'beta_LYA': (v - 0.5, v + 0.002)})
    s = EnsembleSampler(auto_vega, 32, seed=5, sample_params=sp).run(80)
    chain = s.get_chain()
    assert np.all(chain[:, :, 1] <= v + 0.002) and np.all(chain[:, :, 1] >= v - 0.5)
    assert s.stats['rejected_outside_box'] > 0
    # walkers spread over a box where part of the models fail (ap up to 60: the scaled separations leave the tables): a failed
    # model is never accepted (the number of walkers at the 1e100 sentinel never grows), and is counted
    sp = _sample_params(auto_vega, ['ap', 'at'], limits={'ap': (0.9, 60.0)})
    for driver in ('device', 'python'):
        s = EnsembleSampler(auto_vega, 32, seed=9, driver=driver, sample_params=sp).run(20, start='prior')
        failed = (s.get_log_lik() < -1e98).sum(axis=1)
        assert np.all(np.diff(failed) <= 0), failed
        assert s.stats['rejected_failed_model'] > 0, s.stats


def _refused(eng, **changes):
    from vega_amd.engine import EngineError
    args = dict(cols=[eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0],
                theta_fixed=eng.low.theta0.copy(), x=np.tile([[-0.2, 1.67]], (8, 1)), lnl=np.zeros(8),
                accepted=np.zeros(8, dtype=np.int64), step0=0, n_steps=5)
    args.update(changes)
    for k in ('x', 'lnl'):
        args[k] = np.ascontiguousarray(args[k], dtype=np.float64)
    with pytest.raises(EngineError, match='invalid argument'):
        eng.ensemble_run(**args)


def test_refused_arguments_leave_the_engine_as_it_was(auto_vega):
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    i = eng.names.index('bias_eta_LYA')
    cases = [dict(x=np.tile([[-0.2, 1.67]], (7, 1)), lnl=np.zeros(7), accepted=np.zeros(7, dtype=np.int64)),   # W odd
             dict(x=np.tile([[-0.2, 1.67]], (2, 1)), lnl=np.zeros(2), accepted=np.zeros(2, dtype=np.int64)),   # W < 2 n
             dict(cols=[i, eng.n_params]), dict(cols=[i, i]), dict(hi=[0.0, np.inf]), dict(lo=[0.0, 0.5]),
             dict(a=1.0), dict(a=0.5), dict(thin=0), dict(x=np.tile([[0.2, 1.67]], (8, 1))),
             dict(lnl=np.full(8, np.nan)), dict(lnl=np.full(8, -np.inf))]
    for case in cases:
        _refused(eng, **case)
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


def test_an_engine_group_takes_the_python_driver():
    from vega_amd import EnsembleSampler, VegaInterface
    from vega_amd.engine_group import EngineGroup
    prob = synth_joint_problem()
    name = [n for n, it in prob.items.items() if it.tracer1.name != it.tracer2.name][0]
    item = prob.items[name]
    for pipe in [item.core] + [m.pipeline for m in item.metals]:
        pipe.xi.fht_lowring = False
    vega = VegaInterface(None, problem=prob, max_batch=64)
    try:
        assert isinstance(vega.engine, EngineGroup)
        s = EnsembleSampler(vega, 16, seed=1, driver='device', sample_params=_sample_params(vega, AUTO_SAMPLED)).run(5)
        assert s.driver == 'python'
        assert s.get_chain().shape == (5, 16, 4) and s.stats['accepted'] > 0
    finally:
        vega.close()


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import VegaInterface, run_vega_sampler
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Ensemble'] = {'path': str(out), 'name': 'auto_chain', 'walkers': '8', 'steps': '12', 'thin': '3', 'seed': '4'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    table = np.loadtxt(out / 'auto_chain.txt')
    assert table.shape == (12 // 3 * 8, 2 + 2)
    assert np.all(table[:, 0] == 1.0)
    np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True))
    assert (out / 'auto_chain.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
    # the config's own `sampler = True` (no run asked for) still constructs
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=4)
    assert vega.run_sampler is False and vega.sampler == 'True'
    vega.close()
