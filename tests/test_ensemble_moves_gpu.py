"""The ensemble sampler's differential-evolution and snooker moves and their mixtures on the device (include/vegamx.h:
vmx_ensemble_run_many_moves, the kernel k_ens_half_moves) against the NumPy restatement (the `python` driver of
vega_amd/ensemble.py) on real engines: the same decisions and positions bit for bit for every pure move and a mixture of the three,
at halves of 3 and 4 walkers and beyond the 1024 threads of a block; the run without moves untouched and equal to the pure stretch
mixture; a set's member equal to the single run on its stream; a chain that does not depend on the cut; the exact Gaussian
posterior of linear parameters under the DE / snooker mixture; refused arguments that leave the engine as it was; the config
switch end to end."""
import configparser
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
ALL_THREE = [('stretch', .3), ('de', .4), ('snooker', .3)]
MIXTURE = [('de', 0.8), ('snooker', 0.2)]
MOVES = ['de', 'snooker', ALL_THREE]


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


def _pair(vega, W, steps, sp, moves, seed=7, **kw):
    from vega_amd import EnsembleSampler
    out = []
    for driver in ('device', 'python'):
        s = EnsembleSampler(vega, W, seed=seed, driver=driver, sample_params=sp, moves=moves, **kw).run(steps)
        assert s.driver == driver
        out.append(s)
    return out


def _assert_same(dev, py):
    assert np.array_equal(dev.accepted, py.accepted)
    assert np.array_equal(dev.get_chain(), py.get_chain())
    np.testing.assert_allclose(dev.get_log_lik(), py.get_log_lik(), rtol=1e-12, atol=0)
    for key in ('accepted', 'rejected_outside_box', 'rejected_failed_model', 'proposals', 'moves'):
        assert dev.stats[key] == py.stats[key], key
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']
    counts = dev.stats['moves']
    assert sum(c['proposals'] for c in counts.values()) == dev.stats['proposals']
    assert sum(c['accepted'] for c in counts.values()) == dev.stats['accepted'] and counts.unseen == 0


@pytest.mark.parametrize('moves', MOVES, ids=str)
def test_drivers_agree_on_auto(auto_vega, moves):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, 64, 40, sp, moves)
    _assert_same(dev, py)
    assert dev.stats['host_synchronisations'] == dev.stats['calls'] == 1 and dev.get_chain().shape == (40, 64, 4)
    used = {name for name, c in dev.stats['moves'].items() if c['proposals'] > 0}
    assert used == ({moves} if isinstance(moves, str) else {name for name, _ in moves})
    plain = _pair(auto_vega, 64, 2, sp, None)[0]
    assert not np.array_equal(plain.get_chain(), dev.get_chain()[:2])


@pytest.mark.parametrize('moves', MOVES, ids=str)
@pytest.mark.parametrize('names, W, steps, calls_per_half', [(AUTO_SAMPLED[:2], 6, 20, 1), (AUTO_SAMPLED, 8, 10, 1), (AUTO_SAMPLED, 2112, 3, 5)])
def test_drivers_agree_at_the_edges(auto_vega, names, W, steps, calls_per_half, moves):
    """H = 3: the snooker's three partners are the whole other half; H = 4: a block of 64 threads; H = 1056: beyond the 1024
    threads of a block, so the strided loop runs, its rows in 5 chunks of max_batch = 256."""
    dev, py = _pair(auto_vega, W, steps, _sample_params(auto_vega, names), moves)
    _assert_same(dev, py)
    assert dev.get_chain().shape == (steps, W, len(names))
    assert dev.stats['engine_calls'] == steps * 2 * calls_per_half and dev.stats['host_synchronisations'] == 1


def test_without_moves_the_run_is_what_it_was(auto_vega):
    """``moves=None`` launches the kernel of ever and gives the python driver's chain without moves; the pure stretch mixture
    goes through the other kernel and the second Philox block to the same chain; the new entry without moves is the old one."""
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    none = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(30)
    pure = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp, moves='stretch').run(30)
    py = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp, driver='python').run(30)
    assert none.driver == pure.driver == 'device' and py.driver == 'python'
    assert np.array_equal(none.get_chain(), pure.get_chain()) and np.array_equal(none.get_log_lik(), pure.get_log_lik())
    assert np.array_equal(none.accepted, pure.accepted)
    assert np.array_equal(none.get_chain(), py.get_chain()) and np.array_equal(none.accepted, py.accepted)
    assert 'moves' not in none.stats and pure.stats['moves']['stretch'] == dict(proposals=30 * 64, accepted=none.stats['accepted'])
    # ctypes level: vmx_ensemble_run_many_moves(..., moves = NULL) against vmx_ensemble_run_many
    eng = auto_vega.engine
    cols = [eng.names.index(n) for n in AUTO_SAMPLED]
    start = none.get_chain()[-1][None]
    out = []
    for entry, tail in ((eng.lib.vmx_ensemble_run_many, ()), (eng.lib.vmx_ensemble_run_many_moves, (None,))):
        x, lnl, acc = start.copy(), none.get_log_lik()[-1][None].copy(), np.zeros((1, 64), dtype=np.int64)
        spec, args, chain, chain_lnl, stats, _held = eng._ensemble_arrays(
            3, cols, none.lo, none.hi, auto_vega._theta(None), x, lnl, acc, 30, 5, 1, True, a=2.0, log_norm=none.log_norm(), seed=7,
            stream=0, const_hint=-1, chunk=0, lanes=0)
        streams = np.zeros(1, dtype=np.uint64)
        assert entry(eng._h, C.byref(spec), 1, 64, streams.ctypes.data_as(C.POINTER(C.c_uint64)), None, *args, C.byref(stats), None,
                     *tail) == 0
        out.append((chain, chain_lnl, acc))
    assert all(np.array_equal(a, b) for a, b in zip(*out)) and out[0][2].sum() > 0
    again = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(35)
    assert np.array_equal(again.get_chain()[30:], out[1][0][0])


def test_a_set_member_is_the_single_run(auto_vega):
    from vega_amd import EnsembleSampler, EnsembleSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    streams = [4, 1, 2]
    both = EnsembleSet(auto_vega, 3, 32, streams=streams, seed=7, sample_params=sp, moves=ALL_THREE).run(20)
    assert both.driver == 'device' and both.stats['calls'] == 1
    for e, stream in enumerate(streams):
        one = EnsembleSampler(auto_vega, 32, stream=stream, seed=7, sample_params=sp, moves=ALL_THREE).run(20)
        member = both.member(e)
        assert np.array_equal(member.get_chain(), one.get_chain()) and np.array_equal(member.accepted, one.accepted)
        np.testing.assert_allclose(member.get_log_lik(), one.get_log_lik(), rtol=1e-12, atol=0)
        assert member.stats['moves'] == one.stats['moves'] and member.stats['accepted'] == one.stats['accepted']
    assert not np.array_equal(both.get_chain()[0], both.get_chain()[1])
    solo = EnsembleSet(auto_vega, 1, 32, streams=[4], seed=7, sample_params=sp, moves=ALL_THREE).run(20)
    one = EnsembleSampler(auto_vega, 32, stream=4, seed=7, sample_params=sp, moves=ALL_THREE).run(20)
    assert np.array_equal(solo.get_chain()[0], one.get_chain()) and np.array_equal(solo.get_log_lik()[0], one.get_log_lik())
    assert np.array_equal(solo.accepted[0], one.accepted)


def test_chain_is_independent_of_the_cut(auto_vega):
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    one = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp, moves=ALL_THREE).run(40)
    two = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp, moves=ALL_THREE, segment=21).run(40)
    assert np.array_equal(one.get_chain(), two.get_chain()) and np.array_equal(one.get_log_lik(), two.get_log_lik())
    assert np.array_equal(one.accepted, two.accepted) and one.get_chain().shape == (20, 64, 4)
    assert one.stats['calls'] == 1 and two.stats['calls'] == 2 and one.stats['moves'] == two.stats['moves']
    assert one.stats['moves']['de'] == dict(proposals=one.stats['moves']['de']['proposals'], accepted=None)


def test_linear_parameters_sample_the_exact_gaussian_posterior(auto_vega):
    """The four broadband coefficients of the stretch move's test of the same name, under the DE 0.8 / snooker 0.2 mixture: the
    posterior is exactly Gaussian with precision F (chi2 = (b - b*)^T F (b - b*) + const), F and b* from the engine's chi2 at unit
    offsets.  Mean and covariance of the chain within 5 standard errors of an effective sample size N / tau_max, tau from the
    chain."""
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
    s = EnsembleSampler(auto_vega, W, seed=11, sample_params=sp, moves=MIXTURE).run(steps)
    assert s.driver == 'device'
    post = s.get_chain(discard=burn)
    tau = s.get_autocorr_time(discard=burn)
    flat = post.reshape(-1, len(cols))
    n_eff = flat.shape[0] / tau.max()
    print('tau', tau, 'n_eff', n_eff, 'moves', s.stats['moves'])
    assert n_eff > 100, tau
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - mean) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - cov) < tol), ((np.cov(flat.T) - cov) / np.outer(sd, sd), n_eff)
    assert s.stats['moves']['de']['accepted'] > 0 and s.stats['moves']['snooker']['accepted'] > 0


GOOD = dict(weights=(0.0, 0.8, 0.2), gamma0=0.8, sigma=1e-5, gamma_s=1.7)


def _refused(eng, W=8, cols=2, single=False, **moves):
    from vega_amd.engine import EngineError
    names = ['bias_eta_LYA', 'beta_LYA'][:cols]
    box = dict(cols=[eng.names.index(n) for n in names], lo=[-0.5, 0.5][:cols], hi=[0.0, 3.0][:cols], theta_fixed=eng.low.theta0.copy())
    start = np.array([[-0.2, 1.67][:cols]])
    with pytest.raises(EngineError, match='invalid argument'):
        if single:
            eng.ensemble_run(**box, x=np.tile(start, (W, 1)), lnl=np.zeros(W), accepted=np.zeros(W, dtype=np.int64), step0=0, n_steps=5,
                             moves=dict(GOOD, **moves))
        else:
            eng.ensemble_run_many(**box, x=np.tile(start, (2, W, 1)), lnl=np.zeros((2, W)), accepted=np.zeros((2, W), dtype=np.int64),
                                  streams=[0, 1], step0=0, n_steps=5, moves=dict(GOOD, **moves))


def test_refused_moves_leave_the_engine_as_it_was(auto_vega):
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    cases = [dict(weights=(0.0, -0.1, 1.0)), dict(weights=(-1.0, 1.0, 1.0)), dict(weights=(0.0, 1.0, -1e-300)),
             dict(weights=(np.nan, 1.0, 0.0)), dict(weights=(0.0, np.inf, 0.0)), dict(weights=(0.0, 0.0, 0.0)),
             dict(W=2, cols=1, weights=(0.5, 0.5, 0.0)),             # a DE weight with H = 1
             dict(W=2, cols=1, weights=(0.0, 0.0, 1.0)),             # a snooker weight with H = 1
             dict(W=4, weights=(0.0, 0.8, 0.2)),                     # a snooker weight with H = 2
             dict(gamma0=0.0), dict(gamma0=-0.5), dict(gamma0=np.nan), dict(gamma0=np.inf),
             dict(gamma_s=0.0), dict(gamma_s=-1.7), dict(gamma_s=np.nan), dict(gamma_s=np.inf),
             dict(sigma=-1e-5), dict(sigma=np.nan), dict(sigma=np.inf), dict(flags=1), dict(flags=2**31)]
    for case in cases:
        for single in (False, True):
            _refused(eng, single=single, **case)
            np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # (what the weights' rules allow runs: DE alone with H = 2, the snooker with H = 3, sigma = 0, weights that do not add up to 1)
    for W, moves in ((4, dict(GOOD, weights=(0.0, 2.0, 0.0), sigma=0.0)), (6, dict(GOOD, weights=(0.0, 0.0, 0.5)))):
        x, lnl, acc = np.tile([[-0.2, 1.67]], (W, 1)), np.zeros(W), np.zeros(W, dtype=np.int64)
        x += 1e-3 * np.arange(W)[:, None]
        _, _, st = eng.ensemble_run([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0],
                                    eng.low.theta0.copy(), x, lnl, acc, 0, 3, moves=moves)
        assert st['steps'] == 3 and st['proposals'] == 3 * W
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


def test_sample_mocks_passes_the_moves_on():
    """``MonteCarlo.sample_mocks(moves=...)``: the set it runs is the ``EnsembleSet`` with those moves over the same mock pools,
    bit for bit, and another chain than the stretch move's."""
    from vega_amd import EnsembleSet, VegaInterface, synthetic
    from vega_amd.ensemble import resolve_moves
    from vega_amd.montecarlo import MonteCarlo
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=64)
    try:
        sp = _sample_params(vega, AUTO_SAMPLED)
        mc = MonteCarlo(vega)
        ran = mc.sample_mocks(num_mocks=2, walkers=8, steps=9, seed=3, sample_params=sp, moves=MIXTURE, gamma_s=1.5)
        want = resolve_moves(MIXTURE, 4, 8, gamma_s=1.5)
        assert ran.driver == 'device' and ran.moves == want and mc.mc_posteriors['moves'] == want
        assert ran.stats['moves']['stretch']['proposals'] == 0 and ran.stats['moves']['de']['proposals'] > 0
        by_hand = EnsembleSet(vega, 2, 8, mock_rows=[0, 1], seed=3, sample_params=sp, moves=MIXTURE, gamma_s=1.5).run(9)
        assert np.array_equal(ran.get_chain(), by_hand.get_chain()) and np.array_equal(ran.get_log_lik(), by_hand.get_log_lik())
        plain = EnsembleSet(vega, 2, 8, mock_rows=[0, 1], seed=3, sample_params=sp).run(9)
        assert not np.array_equal(plain.get_chain(), by_hand.get_chain())
        with pytest.raises(ValueError, match='moves'):
            mc.sample_mocks(num_mocks=2, sampler='smc', moves='de')
    finally:
        vega.close()


def test_run_vega_sampler_end_to_end(tmp_path):
    from vega_amd import run_vega_sampler
    from vega_amd.ensemble import resolve_moves
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(GOLDEN / 'configs' / 'auto' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Ensemble'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Ensemble'] = {'path': str(out), 'name': 'auto_chain', 'walkers': '8', 'steps': '12', 'thin': '3', 'seed': '4',
                       'moves': 'de 0.8 snooker 0.2'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert sampler.driver == 'device' and sampler.moves == resolve_moves(MIXTURE, 2, 8)
        table = np.loadtxt(out / 'auto_chain.txt')
        assert table.shape == (12 // 3 * 8, 2 + 2)
        assert np.all(table[:, 0] == 1.0)
        np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True))
        np.testing.assert_array_equal(table[:, 2:], sampler.get_chain(flat=True))
        assert (out / 'auto_chain.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
        assert sampler.stats['moves']['stretch']['proposals'] == 0 and sampler.stats['moves']['de']['proposals'] > 0
        assert sampler.stats['accepted'] > 0
    finally:
        sampler.vega.close()
