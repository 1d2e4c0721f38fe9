"""The adaptive temperature ladders on the device (include/vegamx.h: vmx_ensemble_run_pt_adapt, the kernels k_ens_half_pt with a
ladder stride and k_ens_swap_adapt) against the NumPy restatement (python_steps_pt_adapt through the `python` driver of
vega_amd/ensemble.py) on real engines: chains, counters, swap counts, the final ladders, the ladders after every sweep and the
guard's counts at small halves, for two ladders on two mocks, with the adaptation ending inside a call, beyond the 1024 threads of
a block, with the snooker move and on the longest ladder; a chain that does not depend on the cut; the fixed-ladder entry as it
was; refusals that leave the engine as it was; the config switch end to end with the exact evidence of linear parameters."""
import configparser
import math

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
ALL_THREE = [('stretch', .3), ('de', .4), ('snooker', .3)]
MIXTURE = [('de', 0.8), ('snooker', 0.2)]
FAST = dict(adapt=True, adaptation_lag=5, adaptation_time=2)         # (kappa = 1 / 2 at first: the ladder moves by tens of per cent)


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
    return names, mean, sd, log_z_true


@pytest.fixture(scope='module')
def linear(auto_vega):
    """(names, mean, sd, exact log Z) of :func:`_linear_box`: the auto problem hardly constrains its physical parameters (lnL
    varies by 1e-4 over their box, every swap is accepted and equal ratios move no ladder), so the ladders run on the four linear
    coefficients, whose posterior is narrow in their box."""
    return _linear_box(auto_vega)


def _box(linear, n=4):
    names, mean, sd, _ = linear
    return {'limits': {k: (m - 10 * s, m + 10 * s) for k, m, s in zip(names[:n], mean, sd)}, 'values': dict(zip(names[:n], mean)),
            'errors': dict(zip(names[:n], sd))}


def _pair(vega, W, steps, sp, seed=7, whole_calls=False, start='prior', **kw):
    """The same run through both drivers, from walkers drawn over the whole box.  ``whole_calls``: without the class's cut at adapt_steps, so that the adaptation ends inside a call."""
    from vega_amd import TemperedEnsemble
    from vega_amd.ensemble import StretchSampler
    out = []
    for driver in ('device', 'python'):
        s = TemperedEnsemble(vega, W, seed=seed, driver=driver, sample_params=sp, **kw)
        if whole_calls:
            StretchSampler.run(s, steps, start=start)
        else:
            s.run(steps, start=start)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py, calls=1):
    assert np.array_equal(dev.get_chain(rung=None), py.get_chain(rung=None))
    assert np.array_equal(dev.accepted, py.accepted) and np.array_equal(dev.x, py.x)
    assert np.array_equal(dev.per_ensemble, py.per_ensemble) and np.array_equal(dev.swaps, py.swaps)
    assert np.array_equal(dev.current_betas, py.current_betas) and np.array_equal(dev.beta_history, py.beta_history)
    assert np.array_equal(dev._frozen_swaps, py._frozen_swaps)
    if dev.adapt:
        assert np.array_equal(dev.stats['adapt_skipped'], py.stats['adapt_skipped'])
    # (the python driver's engine batches are shaped as the device run's: the same lnL to the bit)
    d_lnl, p_lnl = dev.get_log_lik(rung=None), py.get_log_lik(rung=None)
    print('largest relative lnL difference', float(np.max(np.abs(d_lnl / p_lnl - 1.0))))
    assert np.array_equal(d_lnl, p_lnl) and np.array_equal(dev.lnl, py.lnl)
    for key in ('accepted', 'rejected_outside_box', 'rejected_failed_model', 'proposals', 'swaps_proposed', 'swaps_accepted'):
        assert dev.stats[key] == py.stats[key], key
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']
    assert dev.stats['host_synchronisations'] == dev.stats['calls'] == calls


def _moved(s):
    return float(np.max(np.abs(s.current_betas[:, 1:-1] / s.betas[1:-1] - 1.0)))


@pytest.mark.parametrize('moves', [None, ALL_THREE], ids=str)
@pytest.mark.parametrize('swap_every', [1, 3])
def test_drivers_agree_on_a_ladder_of_four(auto_vega, linear, swap_every, moves):
    """T = 4, W = 8 (H = 4: one block of 64 threads), 40 steps, lag / time (5, 2)."""
    dev, py = _pair(auto_vega, 8, 40, _box(linear), ntemps=4, swap_every=swap_every, moves=moves, **FAST)
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 4, 40, 8, 4) and dev.beta_history.shape == (40 // swap_every, 1, 4)
    assert np.all(dev.swaps[:, :, 0] == 40 // swap_every * 8) and dev.stats['swaps_accepted'] > 0
    assert dev.stats['engine_calls'] == 40 * 2
    print('ladder', dev.current_betas[0], 'moved by', _moved(dev), 'skipped', dev.stats['adapt_skipped'])
    assert _moved(dev) > 0.1 and np.array_equal(dev.beta_history[-1], dev.current_betas)
    assert np.all(dev.current_betas[:, 0] == 1.0) and np.all(dev.current_betas[:, -1] == 0.0)
    assert np.all(np.diff(dev.beta_history, axis=2) < 0.0)


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
        kw = dict(betas=[1.0, 0.3, 0.05, 0.0], ladders=2, mock_rows=[2, 0], moves=ALL_THREE, **FAST)
        dev, py = _pair(vega, 8, 20, _sample_params(vega, AUTO_SAMPLED), **kw)
        _assert_same(dev, py)
        assert dev.get_chain(rung=None).shape == (2, 4, 20, 8, 4) and dev.beta_history.shape == (20, 2, 4)
        print('ladders', dev.current_betas)
        assert not np.array_equal(dev.current_betas[0], dev.current_betas[1])
        assert dev.rung(1, ladder=1).beta == dev.current_betas[1, 1] != dev.rung(1, ladder=0).beta
    finally:
        vega.close()


def test_drivers_agree_when_the_adaptation_ends_inside_a_call(auto_vega, linear):
    """adapt_until = 13 in one call of 30 steps with a sweep after every second step: the sweeps after the steps 1, 3, ..., 11 move
    the ladder, the later ones leave it."""
    dev, py = _pair(auto_vega, 8, 30, _box(linear), ntemps=4, swap_every=2, adapt_steps=13, moves=MIXTURE,
                    whole_calls=True, **FAST)
    _assert_same(dev, py)
    hist = dev.beta_history
    assert hist.shape == (15, 1, 4) and np.all(hist[5:] == hist[5]) and np.array_equal(hist[5], dev.current_betas)
    assert not np.array_equal(hist[5, 0], dev.betas) and sum(not np.array_equal(hist[k], hist[k + 1]) for k in range(5)) >= 2


def test_drivers_agree_beyond_a_block(auto_vega, linear):
    """T = 3, W = 2112, 6 steps: the pairs' counts gather in LDS over the strides of 1024 threads."""
    dev, py = _pair(auto_vega, 2112, 6, _box(linear), betas=[1.0, 0.5, 0.1], moves=MIXTURE, **FAST)
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 3, 6, 2112, 4) and np.all(dev.swaps[0, :, 1] > 1024)
    print('ladder', dev.current_betas[0], 'skipped', dev.stats['adapt_skipped'])
    assert dev.current_betas[0, 1] != 0.5 and dev.current_betas[0, 2] == 0.1


def test_drivers_agree_with_the_snooker_at_a_half_of_three(auto_vega, linear):
    dev, py = _pair(auto_vega, 6, 12, _box(linear, 2), ntemps=3, moves='snooker', **FAST)
    _assert_same(dev, py)
    assert dev.get_chain(rung=None).shape == (1, 3, 12, 6, 2) and dev.current_betas[0, 1] != 0.5


def test_drivers_agree_on_the_longest_ladder(auto_vega, linear):
    """T = 64 at W = 8, 4 steps: 62 exponentials in the one thread that moves the ladder."""
    dev, py = _pair(auto_vega, 8, 4, _box(linear), ntemps=64, **FAST)
    _assert_same(dev, py)
    assert dev.beta_history.shape == (4, 1, 64) and _moved(dev) > 0.01
    # (a gap that changes moves every hotter rung with it: the sum of the gaps is cumulative)
    assert int(np.sum(dev.current_betas[0, 1:-1] != dev.betas[1:-1])) > 20


def test_a_cut_run_is_the_whole_run(auto_vega, linear):
    from vega_amd import TemperedEnsemble
    sp = _box(linear)
    kw = dict(ntemps=4, swap_every=3, thin=2, seed=3, sample_params=sp, moves=ALL_THREE, adapt_steps=11, **FAST)
    one = TemperedEnsemble(auto_vega, 16, **kw).run(24, start='prior')
    two = TemperedEnsemble(auto_vega, 16, segment=7, **kw).run(24, start='prior')
    assert one.driver == two.driver == 'device'
    assert np.array_equal(one.get_chain(rung=None), two.get_chain(rung=None)) and np.array_equal(one.get_log_lik(rung=None), two.get_log_lik(rung=None))
    assert np.array_equal(one.accepted, two.accepted) and np.array_equal(one.swaps, two.swaps)
    assert np.array_equal(one.current_betas, two.current_betas) and np.array_equal(one.beta_history, two.beta_history)
    assert np.array_equal(one.frozen_swap_fraction, two.frozen_swap_fraction)
    assert one.get_chain(rung=None).shape == (1, 4, 12, 16, 4) and one.stats['calls'] == 2 and two.stats['calls'] == 4
    assert one.beta_history.shape == (3, 1, 4) and np.all(one._frozen_swaps[:, :, 0] == 5 * 16)          # sweeps after 2, 5, 8 | 11 .. 23


def test_the_fixed_ladder_entry_is_what_it_was(auto_vega, linear):
    """vmx_ensemble_run_pt, whose half-step kernel now reads its beta through a ladder stride of 0, against python_steps_pt; and
    adaptation that never fires, through the other entry and kernel, gives that chain."""
    from vega_amd import TemperedEnsemble
    sp = _box(linear)
    dev, py = _pair(auto_vega, 8, 12, sp, betas=[1.0, 0.3, 0.0], ladders=2, moves=ALL_THREE)
    _assert_same(dev, py)
    assert not dev.adapt and dev.beta_history.shape == (0, 2, 3) and np.array_equal(dev.current_betas, [[1.0, 0.3, 0.0]] * 2)
    never = TemperedEnsemble(auto_vega, 8, seed=7, sample_params=sp, betas=[1.0, 0.3, 0.0], ladders=2, moves=ALL_THREE, adapt_steps=0,
                             **FAST).run(12, start='prior')
    assert never.driver == 'device'
    assert np.array_equal(never.get_chain(rung=None), dev.get_chain(rung=None)) and np.array_equal(never.swaps, dev.swaps)
    assert np.array_equal(never.get_log_lik(rung=None), dev.get_log_lik(rung=None)) and np.array_equal(never.accepted, dev.accepted)


def _refused(eng, betas, W=8, **kw):
    from vega_amd.engine import EngineError
    betas = np.array(betas, dtype=np.float64)
    G, T = betas.shape
    box = dict(cols=[eng.names.index(n) for n in ('bias_eta_LYA', 'beta_LYA')], lo=[-0.5, 0.5], hi=[0.0, 3.0], theta_fixed=eng.low.theta0.copy())
    with pytest.raises(EngineError, match='invalid argument'):
        eng.ensemble_run_pt_adapt(**box, x=np.tile([[-0.2, 1.67]], (G, T, W, 1)), lnl=np.zeros((G, T, W)),
                                  accepted=np.zeros((G, T, W), dtype=np.int64), betas=betas, streams=np.arange(G * T).reshape(G, T),
                                  step0=0, n_steps=5, **kw)


def test_refusals_leave_the_engine_as_it_was(auto_vega, linear):
    from vega_amd import EnsembleSampler
    sp = _box(linear)
    before = EnsembleSampler(auto_vega, 16, seed=7, sample_params=sp).run(6)
    eng = auto_vega.engine
    good = [1.0, 0.5, 0.0]
    _refused(eng, [[1.0, 0.0]])                                              # T = 2
    _refused(eng, [good], swap_every=0)
    _refused(eng, [good], swap_every=-1)
    _refused(eng, [good], adaptation_lag=0.0)
    _refused(eng, [good], adaptation_time=0.0)
    _refused(eng, [good], adaptation_lag=float('nan'))
    _refused(eng, [good], adaptation_time=float('inf'))
    _refused(eng, [good, [1.0, 0.5, 0.5], good])                             # one ladder among the three is not in order
    _refused(eng, [good, good, [0.9, 0.5, 0.0]])
    _refused(eng, [good], W=7)                                               # (what the plain run refuses)
    after = EnsembleSampler(auto_vega, 16, seed=7, sample_params=sp).run(6)
    assert np.array_equal(before.get_chain(), after.get_chain()) and np.array_equal(before.get_log_lik(), after.get_log_lik())


def test_run_vega_sampler_with_adapt_end_to_end(linear, tmp_path):
    """``[Ensemble] adapt = True`` from a config on the four linear broadband coefficients in the box b* +- 10 sd: T = 7, W = 32,
    600 steps of which the first 300 adapt (the default, steps // 2), DE 0.8 / snooker 0.2.  ``name.stats`` carries the lines of
    an adaptive run, and its stepping-stone evidence lies within 5 err of the exact log Z of the box, -1471.852.  Measured: -1471.815 +- 0.058, pull
    +0.65; the ladder 1, 0.47, 0.20, 0.084, 0.029, 0.0059, 0 with frozen swap fractions 0.49 ... 0.31."""
    from vega_amd import TemperedEnsemble, run_vega_sampler
    from vega_amd.ensemble import read_pt_stats
    names, mean, sd, log_z_true = linear
    print('exact log Z', log_z_true)
    assert abs(log_z_true - -1471.852) < 2e-3
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    cfg['sample'] = {n: f'{m - 10 * s!r} {m + 10 * s!r} {m!r} {s!r}' for n, m, s in zip(names, mean.tolist(), sd.tolist())}
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Ensemble'] = {'path': str(out), 'name': 'bb', 'walkers': '32', 'steps': '600', 'seed': '11', 'ntemps': '7',
                       'moves': 'de 0.8 snooker 0.2', 'adapt': 'True', 'adaptation_lag': '100', 'adaptation_time': '10'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    said = []
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *a: said.append(' '.join(map(str, a))))
    try:
        assert isinstance(sampler, TemperedEnsemble) and sampler.driver == 'device' and list(sampler.names) == names
        assert sampler.adapt and sampler.adapt_steps == 300 and sampler.stats['calls'] == 2 and sampler.frozen_rows == (300, 300)
        assert sampler.beta_history.shape == (300, 1, 7) and not np.array_equal(sampler.current_betas[0], sampler.betas)
        stats = read_pt_stats(out / 'bb.stats')
        log_z, err = sampler.log_evidence()
        print('ladder', sampler.current_betas[0], 'swap fractions', sampler.swap_fraction[0], 'frozen', sampler.frozen_swap_fraction[0],
              'log Z', log_z, '+-', err, 'pull', (log_z - log_z_true) / err)
        assert stats['log(Z)'] == log_z and stats['log(Z) error'] == err and f'log(Z) = {log_z} +- {err}' in said
        assert stats['beta'] == list(sampler.current_betas[0]) and stats['steps'] == 600 and stats['adapt_steps'] == 300
        assert stats['adaptation_lag'] == 100.0 and stats['adaptation_time'] == 10.0
        assert stats['adapt skipped'] == int(sampler.stats['adapt_skipped'][0]) == 0
        assert stats['frozen swap fraction'] == list(sampler.frozen_swap_fraction[0]) and len(stats['swap fraction']) == 6
        assert abs(log_z - log_z_true) < 5 * err and math.isfinite(err) and err > 0.0
        table = np.loadtxt(out / 'bb.txt')
        assert table.shape == (600 * 32, 2 + 4)
    finally:
        sampler.vega.close()
