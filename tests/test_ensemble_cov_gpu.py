"""The ensemble sampler's covariance move on the device (include/vegamx.h: vmx_ensemble_run_many_cov and vmx_ensemble_cov_factor, the
kernel k_ens_half_cov) on real engines: the work-group's factor stage against the serial NumPy restatement bit for bit - the
smallest half, several ensembles, a singular half, an entry loop that wraps past the block, a half beyond the block, a constant
column; the device driver against the `python` driver bit for bit under the pure move and a mixture of all four, from the smallest
run to a half beyond the block and to sixteen sampled parameters; the paths without cov unchanged; a set's member equal to the
single run; a chain that does not depend on the cut; the exact Gaussian posterior of linear parameters; refused arguments that
leave the engine as it was; the config switch end to end."""
import configparser
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
ALL_FOUR = [('stretch', .25), ('de', .25), ('snooker', .25), ('cov', .25)]
BB = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i in (0, 1, 2) for j in (0, 2, 4, 6)]


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


# ------------------------------------------------------------------ the factor stage
def _half(rng, H, n):
    A = rng.normal(size=(n, n)) / np.sqrt(n) + np.eye(n)
    return (rng.normal(size=(H, n)) @ A.T) * 10.0 ** np.linspace(-1.5, 1.5, n) + rng.normal(size=n)


def _check_factor(eng, x):
    from vega_amd import ensemble as E
    mean, factor, flag = eng.ensemble_cov_factor(x)
    assert mean.shape == x.shape[::2] and factor.shape == (x.shape[0], x.shape[2], x.shape[2]) and flag.shape == (x.shape[0],)
    goods = []
    for e in range(x.shape[0]):
        m_ref, c_ref, good = E.half_factor(x[e])
        assert flag[e] == (1 if good else 0)
        assert np.array_equal(mean[e].view(np.uint64), m_ref.view(np.uint64)), e
        assert np.array_equal(factor[e].view(np.uint64), np.ascontiguousarray(c_ref).view(np.uint64)), e
        goods.append(good)
    return factor, goods


@pytest.mark.parametrize('E_, H, n', [(1, 2, 1), (2, 3, 2), (1, 64, 64), (3, 65, 64), (1, 1056, 64)])
def test_factor_stage_is_the_serial_factor_bitwise(auto_vega, E_, H, n):
    """(1, 2, 1): the smallest run.  (2, 3, 2): more than one ensemble.  (1, 64, 64): H = n, a singular covariance - whatever the
    last pivot rounds to, both sides agree.  (3, 65, 64): 2080 entries, so the strided entry loop wraps.  (1, 1056, 64): a half
    beyond the block."""
    rng = np.random.default_rng(1000 * E_ + H + n)
    x = np.stack([_half(rng, H, n) for _ in range(E_)])
    factor, goods = _check_factor(auto_vega.engine, x)
    if H > n:
        assert all(goods) and np.all(np.triu(factor, 1) == 0.0)
        for e in range(E_):
            cov = np.atleast_2d(np.cov(x[e].T))
            assert np.allclose(factor[e] @ factor[e].T, cov, rtol=1e-6, atol=1e-9 * np.abs(cov).max())


def test_factor_stage_falls_back_on_a_constant_column(auto_vega):
    """A column constant over the walkers has variance exactly 0: the flag is 0 and the diagonal factor is returned - in the
    ensemble that has the column, not in its neighbours."""
    rng = np.random.default_rng(5)
    x = np.stack([_half(rng, 40, 18) for _ in range(3)])
    x[1, :, 7] = 0.375
    factor, goods = _check_factor(auto_vega.engine, x)
    assert goods == [True, False, True]
    assert factor[1][7, 7] == 0.0 and np.all(factor[1] - np.diag(np.diag(factor[1])) == 0.0)
    assert np.allclose(np.delete(np.diag(factor[1]), 7), np.delete(x[1].std(axis=0, ddof=1), 7), rtol=1e-10)


# ------------------------------------------------------------------ device = python
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
    for key in ('accepted', 'rejected_outside_box', 'rejected_failed_model', 'proposals', 'moves', 'cov'):
        assert dev.stats[key] == py.stats[key], key
    assert np.array_equal(dev.cov_fallbacks, py.cov_fallbacks)
    assert 0 < dev.stats['accepted'] < dev.stats['proposals']
    counts = dev.stats['moves']
    assert list(counts) == ['stretch', 'de', 'snooker', 'cov'] and counts['cov']['proposals'] > 0
    assert sum(c['proposals'] for c in counts.values()) == dev.stats['proposals']
    assert sum(c['accepted'] for c in counts.values()) == dev.stats['accepted'] and counts.unseen == 0


def _wide_params(vega):
    """ap, at, bias_eta_LYA, beta_LYA and the twelve broadband coefficients: sixteen sampled parameters, so that a walker draws
    four further Philox blocks.  The coefficients' boxes and start balls come from the curvature of chi2 along each."""
    sp = _sample_params(vega, ['ap', 'at', 'bias_eta_LYA', 'beta_LYA'])
    base = vega._theta(None)
    cols = [vega.param_names.index(n) for n in BB]
    th = np.repeat(base[None, :], 1 + 2 * len(cols), axis=0)
    for i, c in enumerate(cols):
        th[1 + 2 * i, c] += 1.0
        th[2 + 2 * i, c] += 2.0
    c2 = np.asarray(vega.chi2_batch(th))
    for i, (name, c) in enumerate(zip(BB, cols)):
        curv = (c2[2 + 2 * i] - 2 * c2[1 + 2 * i] + c2[0]) / 2.0
        sd = 1.0 / np.sqrt(curv)
        sp['limits'][name] = (base[c] - 30 * sd, base[c] + 30 * sd)
        sp['values'][name] = base[c]
        sp['errors'][name] = sd
    return sp


@pytest.mark.parametrize('moves', ['cov', ALL_FOUR], ids=str)
@pytest.mark.parametrize('names, W, steps', [(AUTO_SAMPLED[:1], 4, 20), (AUTO_SAMPLED, 8, 10), (AUTO_SAMPLED, 64, 30), (AUTO_SAMPLED, 2112, 3),
                                            ('wide', 64, 12)])
def test_drivers_agree(auto_vega, names, W, steps, moves):
    """W = 4, n = 1: the smallest run (a half of two has no third partner and the library refuses a snooker weight there: the
    mixture is stretch, DE and cov).  W = 8, n = 4: H = n.  W = 64: a plain
    run.  W = 2112: H = 1056, the propose loop wraps and the rows come in 5 chunks of max_batch = 256.  W = 64, n = 16: several
    Philox blocks per walker."""
    if W == 4 and moves != 'cov':
        moves = [('stretch', .25), ('de', .25), ('cov', .5)]
    sp = _wide_params(auto_vega) if names == 'wide' else _sample_params(auto_vega, names)
    dev, py = _pair(auto_vega, W, steps, sp, moves)
    _assert_same(dev, py)
    n = len(sp['limits'])
    assert dev.get_chain().shape == (steps, W, n) and dev.stats['host_synchronisations'] == dev.stats['calls'] == 1
    assert dev.stats['cov']['scale'] == 2.38 / np.sqrt(n)
    if W == 2112:
        assert dev.stats['engine_calls'] == steps * 2 * 5
    if W // 2 > n:
        assert dev.stats['cov']['factor_fallbacks'] == 0
    if moves != 'cov':
        assert all(dev.stats['moves'][name]['proposals'] > 0 for name, _ in moves)


def test_a_scale_of_its_own_reaches_both_drivers(auto_vega):
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    dev, py = _pair(auto_vega, 32, 10, sp, [('cov', 0.7), ('snooker', 0.3)], cov_scale=0.6)
    _assert_same(dev, py)
    assert dev.stats['cov'] == dict(scale=0.6, factor_fallbacks=0)
    other = _pair(auto_vega, 32, 10, sp, [('cov', 0.7), ('snooker', 0.3)])[0]
    assert not np.array_equal(other.get_chain(), dev.get_chain())


# ------------------------------------------------------------------ the paths that must not change
def _run_entry(vega, entry, tail, start, moves=None, steps=5):
    eng = vega.engine
    cols = [eng.names.index(n) for n in AUTO_SAMPLED]
    x, lnl, acc = start.get_chain()[-1][None].copy(), start.get_log_lik()[-1][None].copy(), np.zeros((1, 64), dtype=np.int64)
    spec, args, chain, chain_lnl, stats, _held = eng._ensemble_arrays(
        3, cols, start.lo, start.hi, vega._theta(None), x, lnl, acc, 30, steps, 1, True, a=2.0, log_norm=start.log_norm(), seed=7,
        stream=0, const_hint=-1, chunk=0, lanes=0)
    streams = np.zeros(1, dtype=np.uint64)
    rc = entry(eng._h, C.byref(spec), 1, 64, streams.ctypes.data_as(C.POINTER(C.c_uint64)), None, *args, C.byref(stats), None, *tail)
    return rc, chain, chain_lnl, acc


def test_without_cov_the_run_is_what_it_was(auto_vega):
    """A three-move mixture through the new entry with a NULL cov struct - or a cov weight of 0 - is the chain of
    vmx_ensemble_run_many_moves; without moves it is that of vmx_ensemble_run_many; ``moves=None`` is untouched: the kernel of
    ever, equal to the python driver without moves."""
    from vega_amd import EnsembleSampler, engine
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    none = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(30)
    py = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp, driver='python').run(30)
    assert none.driver == 'device' and np.array_equal(none.get_chain(), py.get_chain()) and np.array_equal(none.accepted, py.accepted)
    assert 'moves' not in none.stats and 'cov' not in none.stats
    lib = auto_vega.engine.lib
    mv = engine.EnsembleMoves((C.c_double * 3)(0.3, 0.4, 0.3), 0.8, 1e-5, 1.7, 0, 0)
    zero = engine.EnsembleCov(0.0, 1.0, 0, 0)
    fb = np.full(1, -1, dtype=np.int64)
    i64 = C.POINTER(C.c_int64)
    old = _run_entry(auto_vega, lib.vmx_ensemble_run_many_moves, (C.byref(mv),), none)
    for tail in ((C.byref(mv), None, None), (C.byref(mv), C.byref(zero), fb.ctypes.data_as(i64))):
        new = _run_entry(auto_vega, lib.vmx_ensemble_run_many_cov, tail, none)
        assert old[0] == new[0] == 0 and all(np.array_equal(a, b) for a, b in zip(old[1:], new[1:])) and new[3].sum() > 0
    assert fb[0] == 0
    plain = _run_entry(auto_vega, lib.vmx_ensemble_run_many, (), none)
    new = _run_entry(auto_vega, lib.vmx_ensemble_run_many_cov, (None, None, None), none)
    assert plain[0] == new[0] == 0 and all(np.array_equal(a, b) for a, b in zip(plain[1:], new[1:]))
    again = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(35)
    assert np.array_equal(again.get_chain()[30:], plain[1][0])
    # with a cov weight the chain is another one
    some = engine.EnsembleCov(0.5, 1.0, 0, 0)
    new = _run_entry(auto_vega, lib.vmx_ensemble_run_many_cov, (C.byref(mv), C.byref(some), fb.ctypes.data_as(i64)), none)
    assert new[0] == 0 and not np.array_equal(new[1], old[1]) and fb[0] == 0


# ------------------------------------------------------------------ the usual sampler properties
def test_a_set_member_is_the_single_run(auto_vega):
    from vega_amd import EnsembleSampler, EnsembleSet
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    streams = [4, 1, 2]
    both = EnsembleSet(auto_vega, 3, 32, streams=streams, seed=7, sample_params=sp, moves=ALL_FOUR).run(20)
    assert both.driver == 'device' and both.stats['calls'] == 1 and both.cov_fallbacks.shape == (3,)
    for e, stream in enumerate(streams):
        one = EnsembleSampler(auto_vega, 32, stream=stream, seed=7, sample_params=sp, moves=ALL_FOUR).run(20)
        member = both.member(e)
        assert np.array_equal(member.get_chain(), one.get_chain()) and np.array_equal(member.accepted, one.accepted)
        np.testing.assert_allclose(member.get_log_lik(), one.get_log_lik(), rtol=1e-12, atol=0)
        assert member.stats['moves'] == one.stats['moves'] and member.stats['accepted'] == one.stats['accepted']
        assert member.stats['cov'] == one.stats['cov']
    assert not np.array_equal(both.get_chain()[0], both.get_chain()[1])


def test_chain_is_independent_of_the_cut(auto_vega):
    from vega_amd import EnsembleSampler
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    one = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp, moves=ALL_FOUR).run(40)
    two = EnsembleSampler(auto_vega, 64, seed=3, thin=2, sample_params=sp, moves=ALL_FOUR, segment=21).run(40)
    assert np.array_equal(one.get_chain(), two.get_chain()) and np.array_equal(one.get_log_lik(), two.get_log_lik())
    assert np.array_equal(one.accepted, two.accepted) and one.get_chain().shape == (20, 64, 4)
    assert one.stats['calls'] == 1 and two.stats['calls'] == 2 and one.stats['moves'] == two.stats['moves']
    assert one.stats['cov'] == two.stats['cov']
    assert one.stats['moves']['cov'] == dict(proposals=one.stats['moves']['cov']['proposals'], accepted=None)


def test_linear_parameters_sample_the_exact_gaussian_posterior(auto_vega):
    """The four broadband coefficients of the test of the same name in tests/test_ensemble_moves_gpu.py, under the pure covariance
    move: the posterior is exactly Gaussian with precision F (chi2 = (b - b*)^T F (b - b*) + const), F and b* from the engine's
    chi2 at unit offsets.  Mean and covariance of the chain within 5 standard errors of an effective sample size N / tau_max, tau
    from the chain; n_eff > 100 (a NumPy simulation of the rule gave tau about 10 at n = 4: n_eff about 2000)."""
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
    s = EnsembleSampler(auto_vega, W, seed=11, sample_params=sp, moves='cov').run(steps)
    assert s.driver == 'device'
    post = s.get_chain(discard=burn)
    tau = s.get_autocorr_time(discard=burn)
    flat = post.reshape(-1, len(cols))
    n_eff = flat.shape[0] / tau.max()
    print('tau', tau, 'n_eff', n_eff, 'moves', s.stats['moves'], 'cov', s.stats['cov'])
    assert n_eff > 100, tau
    assert np.all(np.abs(flat.mean(axis=0) - mean) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - mean) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - cov) < tol), ((np.cov(flat.T) - cov) / np.outer(sd, sd), n_eff)
    assert s.stats['moves']['cov']['accepted'] > 0 and s.stats['cov']['factor_fallbacks'] == 0


# ------------------------------------------------------------------ refusals and the config
GOOD = dict(weights=(0.0, 0.4, 0.2, 0.4), gamma0=0.8, sigma=1e-5, gamma_s=1.7, cov_scale=1.2)


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


def test_refused_cov_leaves_the_engine_as_it_was(auto_vega):
    """Every refusal of vmx_ensemble_run_many_cov - its own and one of each kind the moves entry makes - leaves the engine as it
    was: chi2 of a row is what it was, and a plain run afterwards gives the chain it gave before."""
    from vega_amd import EnsembleSampler, engine
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    first = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(10)
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    cases = [dict(weights=(0.0, 0.4, 0.2, -0.1)), dict(weights=(0.0, 0.4, 0.2, -1e-300)), dict(weights=(0.0, 0.4, 0.2, np.nan)),
             dict(weights=(0.0, 0.4, 0.2, np.inf)), dict(weights=(0.0, 0.0, 0.0, 0.0)),
             dict(W=2, cols=1, weights=(0.0, 0.0, 0.0, 1.0)),          # a cov weight with H = 1
             dict(W=2, cols=1, weights=(0.5, 0.0, 0.0, 0.5)),
             dict(cov_scale=0.0), dict(cov_scale=-1.2), dict(cov_scale=np.nan), dict(cov_scale=np.inf), dict(cov_flags=1),
             dict(cov_flags=2**31),
             # whatever the moves entry refuses
             dict(weights=(0.0, -0.1, 0.2, 0.4)), dict(weights=(np.nan, 0.4, 0.2, 0.4)), dict(W=4, weights=(0.0, 0.4, 0.2, 0.4)),
             dict(gamma0=0.0), dict(gamma_s=np.inf), dict(sigma=-1e-5), dict(flags=1)]
    for case in cases:
        for single in (False, True):
            _refused(eng, single=single, **case)
            np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # reserved, which the binding never sets, and a cov weight without the moves' struct
    mv = engine.EnsembleMoves((C.c_double * 3)(0.3, 0.4, 0.3), 0.8, 1e-5, 1.7, 0, 0)
    lib = eng.lib
    for tail in ((C.byref(mv), C.byref(engine.EnsembleCov(0.5, 1.0, 0, 1)), None), (None, C.byref(engine.EnsembleCov(0.5, 1.0, 0, 0)), None),
                 (C.byref(mv), C.byref(engine.EnsembleCov(0.0, 0.0, 0, 0)), None)):
        rc, chain, _, acc = _run_entry(auto_vega, lib.vmx_ensemble_run_many_cov, tail, first)
        assert rc == -1 and acc.sum() == 0 and lib.vmx_last_error()
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # the factor entry's own refusals
    from vega_amd.engine import EngineError
    for shape in ((1, 1, 1), (1, 4, 65)):
        with pytest.raises(EngineError, match='invalid argument'):
            eng.ensemble_cov_factor(np.zeros(shape))
    # (what the rules allow runs: cov alone with H = 2, weights that do not add up to 1)
    x, lnl, acc = np.tile([[-0.2, 1.67]], (4, 1)), np.zeros(4), np.zeros(4, dtype=np.int64)
    x += 1e-3 * np.arange(4)[:, None] * np.array([1.0, -2.0])
    _, _, st = eng.ensemble_run([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], [-0.5, 0.5], [0.0, 3.0],
                                eng.low.theta0.copy(), x, lnl, acc, 0, 3, moves=dict(GOOD, weights=(0.0, 0.0, 0.0, 2.5)))
    assert st['steps'] == 3 and st['proposals'] == 12 and st['cov_fallbacks'].shape == (1,)
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    again = EnsembleSampler(auto_vega, 64, seed=7, sample_params=sp).run(10)
    assert np.array_equal(first.get_chain(), again.get_chain()) and np.array_equal(first.get_log_lik(), again.get_log_lik())


def test_tempering_and_slice_refuse_cov(auto_vega):
    from vega_amd import EnsembleSampler
    from vega_amd.ensemble import TemperedEnsemble
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    with pytest.raises(ValueError, match='tempering'):
        TemperedEnsemble(auto_vega, 16, ntemps=3, sample_params=sp, moves='cov')
    with pytest.raises(ValueError, match='slice'):
        EnsembleSampler(auto_vega, 16, sample_params=sp, moves=[('cov', 0.5), ('slice', 0.5)])


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
                       'moves': 'cov 0.7 snooker 0.3', 'cov_scale': '1.3'}
    (tmp_path / 'configs' / 'ens').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ens' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ens/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert sampler.driver == 'device' and sampler.moves == resolve_moves([('cov', 0.7), ('snooker', 0.3)], 2, 8, cov_scale=1.3)
        table = np.loadtxt(out / 'auto_chain.txt')
        assert table.shape == (12 // 3 * 8, 2 + 2)
        assert np.all(table[:, 0] == 1.0)
        np.testing.assert_array_equal(table[:, 1], -sampler.get_log_lik(flat=True))
        np.testing.assert_array_equal(table[:, 2:], sampler.get_chain(flat=True))
        assert (out / 'auto_chain.paramnames').read_text().splitlines() == ['bias_eta_LYA bias_eta_LYA', 'beta_LYA beta_LYA']
        assert sampler.stats['moves']['stretch']['proposals'] == 0 and sampler.stats['moves']['cov']['proposals'] > 0
        assert sampler.stats['cov']['scale'] == 1.3 and sampler.stats['accepted'] > 0
    finally:
        sampler.vega.close()
