"""``boost_posterior`` in a set of nested-sampling runs on the device (include/vegamx.h: vmx_nested_run_many_phantoms,
k_ns_set_advance_phantoms; vega_amd/nested.py: NestedSet) on real engines: a set of one is the boosted single sampler bit for bit;
the device driver keeps the phantom records of the NumPy restatement - runs that leave the set at iterations of their own, a kept
fraction below one, two threads per lane - beside base runs that are those of the set without boost; boost off is the set of
before; a set cut into calls; refused arguments that leave the engine as it was; the boosted summaries of every mock against the
exact posterior; a member's files."""
import math

import numpy as np
import pytest

from conftest import GOLDEN
from test_ensemble_set_gpu import _linear_gaussian
from test_nested_set_gpu import _assert_same
from test_smc_gpu import _linear_box

pytestmark = pytest.mark.gpu


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
    """The auto problem with the synthetic covariance (mocks are drawn from one), as in tests/test_nested_set_gpu.py."""
    from vega_amd import VegaInterface, synthetic
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=256)
    vega.freeze_metals()
    yield vega
    vega.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _report(what, a, b):
    """The figures before anything is asserted: rows, and the largest difference of every part of two phantom records."""
    line = [f'{what}: {a["lnl"].size} / {b["lnl"].size} rows']
    if a['lnl'].shape == b['lnl'].shape:
        for key in ('u', 'lnl', 'birth'):
            same = np.array_equal(_bits(a[key]), _bits(b[key]))
            worst = float(np.max(np.abs(a[key] - b[key]) / np.maximum(np.abs(b[key]), 1e-300))) if a[key].size else 0.0
            line.append(f'{key} {"same bits" if same else f"differs, largest relative difference {worst:.3g}"}')
        line.append(f'tags {"same" if np.array_equal(a["tag"], b["tag"]) else "differ"}')
    print(', '.join(line))


def _same_bits_record(a, b):
    assert a['lnl'].shape == b['lnl'].shape and a['u'].shape == b['u'].shape and np.array_equal(a['tag'], b['tag'])
    for key in ('u', 'lnl', 'birth'):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    assert a['cluster'] is None and b['cluster'] is None


def _same_record_as_python(a, b):
    """Device against the python driver: tags and u bit for bit, lnL and birth to 1e-12 (the drivers' chi2 come from the same
    engine in the same batches; the restatement turns them into lnL in NumPy)."""
    assert a['lnl'].shape == b['lnl'].shape and np.array_equal(a['tag'], b['tag']) and np.array_equal(a['u'], b['u'])
    np.testing.assert_allclose(a['lnl'], b['lnl'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a['birth'], b['birth'], rtol=1e-12, atol=0)


def _pair(vega, E, iterations, sp, stop_at=None, seed=7, **kw):
    """The boosted set by both drivers (``stop_at`` as in tests/test_nested_set_gpu.py); the device's PhantomArrays of every call
    are kept in ``dev.seen``."""
    from vega_amd import NestedSet
    out = []
    for driver in ('device', 'python'):
        s = NestedSet(vega, E, seed=seed, driver=driver, sample_params=sp, **kw)
        if stop_at is not None:
            for run, at in zip(s.runs, stop_at):
                run.max_iterations = at
        s.seen = []
        real = vega.engine.nested_run_many

        def spy(*args, _s=s, **kwargs):
            _s.seen.append(kwargs.get('phantoms'))
            return real(*args, **kwargs)

        vega.engine.nested_run_many = spy
        try:
            s.run(iterations)
        finally:
            del vega.engine.nested_run_many
        assert s.driver == driver
        out.append(s)
    return out


def test_a_set_of_one_is_the_boosted_sampler(auto_vega, linear_box):
    """E = 1 has the single run's batches: live points, the dead record and the canonical phantom record bit for bit."""
    from vega_amd import NestedSampler, NestedSet
    kw = dict(num_live=64, threads=16, num_repeats=4, seed=7, sample_params=linear_box, boost_posterior=4)
    both = NestedSet(auto_vega, 1, streams=[3], **kw).run(6)
    one = NestedSampler(auto_vega, stream=3, **kw).run(6)
    assert both.driver == one.driver == 'device' and one.iteration == both.iteration[0] == 6
    run = both.runs[0]
    assert np.array_equal(run.live_u, one.live_u) and np.array_equal(run.live_lnl, one.live_lnl)
    for a, b in zip(both.dead(0), one.dead()):
        assert np.array_equal(a, b)
    a, b = both.phantoms(0), one.phantoms()
    _report('set of one against the single sampler', a, b)
    _same_bits_record(a, b)
    assert 0 < a['lnl'].size <= 6 * 16 * 3 and np.all(a['lnl'] > a['birth'])
    member = both.member(0)
    for x, y in zip(member.samples(), one.samples()):
        assert np.array_equal(x, y)
    assert member.boost_log_evidence() == one.boost_log_evidence() == both.boost_log_evidence()[0]
    assert np.array_equal(member.boost_index(), one.boost_index()) and member.log_evidence() == one.log_evidence()


@pytest.mark.parametrize('f', [1.0, 0.3])
def test_drivers_agree_with_runs_that_stop_on_their_own(auto_vega, linear_box, f):
    """E = 3 x (nlive 40, K 12), 4 repeats, chunk 16; run e stops after 2 + e iterations, so run 0 is OUT while the others
    record.  The base runs are held to what tests/test_nested_set_gpu.py holds the drivers to; the phantom records' tags and u are
    equal, lnL and birth to 1e-12; the count the device hands back per run is the length of its record."""
    stop_at = [2, 3, 4]
    dev, py = _pair(auto_vega, 3, None, linear_box, stop_at=stop_at, num_live=40, threads=12, num_repeats=4, chunk=16,
                    boost_posterior=4 * f)
    _assert_same(dev, py)
    assert list(dev.iteration) == stop_at and list(dev.status) == [1] * 3 and dev.stats['calls'] == 1
    assert dev.stats['host_waits'] == dev.stats['rounds'] + 2
    arrays = dev.seen[0]
    assert len(dev.seen) == 1 and arrays is not None and arrays.fraction == f and py.seen == []
    for e in range(3):
        a, b = dev.phantoms(e), py.phantoms(e)
        _report(f'f = {f}, run {e}, device against python', a, b)
        _same_record_as_python(a, b)
        assert arrays.count[e] == a['lnl'].size > 0 and a['tag'][:, 0].max() == stop_at[e] - 1
        assert np.all(a['lnl'] > a['birth']) and np.all((a['u'] >= 0) & (a['u'] <= 1))
        assert len({tuple(t) for t in a['tag']}) == a['lnl'].size <= stop_at[e] * 12 * 3
        # the birth contour is the L* of the iteration: the lnL of its last death
        lstar = dev.dead(e)[1].reshape(stop_at[e], 12)[:, -1]
        assert np.array_equal(a['birth'], lstar[a['tag'][:, 0]])
    if f == 0.3:
        share = sum(dev.phantoms(e)['lnl'].size for e in range(3)) / (9 * 12 * 3)
        assert abs(share - f) < 0.16                        # (324 draws: six standard deviations of the share)


def test_more_than_one_thread_per_lane(auto_vega, linear_box):
    """K = 1100 on 1024 lanes: two threads per lane of the advance kernel, both can accept in one round."""
    dev, py = _pair(auto_vega, 2, 2, linear_box, num_live=2200, threads=1100, num_repeats=2, boost_posterior=2)
    _assert_same(dev, py)
    for e in range(2):
        a, b = dev.phantoms(e), py.phantoms(e)
        _report(f'K = 1100, run {e}, device against python', a, b)
        _same_record_as_python(a, b)
        assert dev.seen[0].count[e] == a['lnl'].size and 0 < a['lnl'].size <= 2 * 1100
        assert a['tag'][:, 1].max() > 1024 and np.all(a['tag'][:, 2] == 1)


def _same_sets(a, b, phantoms=False, statistics=True):
    assert np.array_equal(a.status, b.status) and np.array_equal(a.iteration, b.iteration)
    for e in range(a.E):
        assert np.array_equal(a.runs[e].live_u, b.runs[e].live_u) and np.array_equal(a.runs[e].live_lnl, b.runs[e].live_lnl)
        for x, y in zip(a.dead(e), b.dead(e)):
            assert np.array_equal(x, y)
        if phantoms:
            _same_bits_record(a.phantoms(e), b.phantoms(e))
    for x, y in zip(a.log_evidence(), b.log_evidence()):
        assert np.array_equal(x, y)
    if statistics:
        for key in ('iterations', 'rounds', 'rows', 'rows_own_position', 'engine_calls', 'host_waits', 'calls', 'lanes', 'const_hint'):
            assert a.stats[key] == b.stats[key], key
        assert np.array_equal(a.stats['per_run'], b.stats['per_run'])


def test_boost_off_is_the_set_of_before_and_boost_leaves_the_base_runs(auto_vega, linear_box):
    """``boost_posterior=0`` is the set without the argument bit for bit, statistics included, through vmx_nested_run_many; at
    b > 0 the base runs - u, lnL, live counts, evidences, rows, rounds and host waits - are those of b = 0: phantoms add no engine
    row, so the batches are the same."""
    from vega_amd import NestedSet
    kw = dict(num_live=40, threads=12, num_repeats=4, seed=5, sample_params=linear_box, chunk=16)
    calls = []
    real = auto_vega.engine.nested_run_many
    auto_vega.engine.nested_run_many = lambda *a, **k: calls.append('phantoms' in k) or real(*a, **k)
    try:
        plain = NestedSet(auto_vega, 3, **kw).run(4)
        zero = NestedSet(auto_vega, 3, boost_posterior=0, **kw).run(4)
        boosted = NestedSet(auto_vega, 3, boost_posterior=2, **kw).run(4)
    finally:
        del auto_vega.engine.nested_run_many
    assert calls == [False, False, True] and plain.driver == zero.driver == boosted.driver == 'device'
    _same_sets(plain, zero)
    assert set(plain.stats) == set(zero.stats) and all(run.phantom_state is None for run in zero.runs)
    with pytest.raises(ValueError, match='keeps no phantom points'):
        zero.phantoms(0)
    _same_sets(plain, boosted)
    for e in range(3):
        base, full = boosted.samples(boost=False)[e], boosted.samples()[e]
        for x, y in zip(base, plain.samples()[e]):
            assert np.array_equal(x, y)
        assert full[0].shape[0] == base[0].shape[0] + boosted.phantoms(e)['lnl'].size > base[0].shape[0]


def test_the_boosted_set_does_not_depend_on_the_cut(auto_vega, linear_box):
    """A set of one (the batches of a cut set of one are those of the whole: tests/test_nested_set_gpu.py), ``run(3)`` then
    ``run(3)`` against ``run(6)``: the phantom records are equal bit for bit."""
    from vega_amd import NestedSet
    kw = dict(num_live=40, threads=12, num_repeats=4, seed=5, sample_params=linear_box, streams=[4], boost_posterior=1.2)
    one = NestedSet(auto_vega, 1, **kw).run(6)
    cut = NestedSet(auto_vega, 1, **kw).run(3).run(3)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 2 and len(cut.runs[0].phantom_state.calls) == 2
    _report('3 + 3 iterations against 6', one.phantoms(0), cut.phantoms(0))
    _same_sets(one, cut, phantoms=True, statistics=False)
    assert one.stats['rows'] == cut.stats['rows'] and cut.stats['host_waits'] == cut.stats['rounds'] + 3
    assert 0 < one.phantoms(0)['lnl'].size < 6 * 12 * 3
    for x, y in zip(one.samples()[0], cut.samples()[0]):
        assert np.array_equal(x, y)


def _call(eng, arrays, E=2, nlive=16):
    """vmx_nested_run_many_phantoms through ``Engine.nested_run_many`` as tests/test_nested_set_gpu.py calls the set (2
    iterations, 4 threads, 3 repeats, drawn)."""
    cols = [eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')]
    u, lnl, it = np.zeros((E, nlive, 2)), np.zeros((E, nlive)), np.zeros(E, dtype=np.int64)
    return eng.nested_run_many(cols, [-0.5, 0.5], [0.0, 3.0], eng.low.theta0.copy(), u, lnl, it, np.arange(E), 2, 4, 3,
                               draw_live=True, seed=3, phantoms=arrays)


def test_refused_arguments_leave_the_engine_as_it_was(auto_vega):
    """A capacity one below n_iterations K (num_repeats - 1), a fraction of 1.5 or NaN, non-zero flags: -1, and the engine still
    evaluates what it evaluated; the mended call runs and fraction 0 runs vmx_nested_run_many and touches nothing."""
    from vega_amd.engine import EngineError, PhantomArrays
    eng = auto_vega.engine
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    need = 2 * 4 * 2
    for arrays in (PhantomArrays(2, need - 1, 2, 1.0), PhantomArrays(2, need, 2, 1.5), PhantomArrays(2, need, 2, math.nan),
                   PhantomArrays(2, need, 2, -0.5), PhantomArrays(2, need, 2, 1.0, flags=1)):
        arrays.count[:] = -5
        with pytest.raises(EngineError, match='invalid argument'):
            _call(eng, arrays)
        assert list(arrays.count) == [-5, -5]               # (nothing was written)
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    with pytest.raises(ValueError, match='PhantomArrays'):
        _call(eng, PhantomArrays(3, need, 2, 1.0))
    good = PhantomArrays(2, need + 3, 2, 1.0)               # (a capacity above the need: the rows of run 1 begin at its own stride)
    dead, status, done, st = _call(eng, good)
    assert list(done) == [2, 2] and np.all(good.count > 0) and np.all(good.count <= need) and st['host_waits'] == st['rounds'] + 2
    for e in range(2):
        u, lnl, birth, tag = good.run(e)
        assert np.all(lnl > birth) and np.all((tag[:, 0] >= 0) & (tag[:, 0] < 2) & (tag[:, 1] < 4) & (tag[:, 2] >= 1) & (tag[:, 2] < 3))
    off = PhantomArrays(2, 0, 2, 0.0, flags=9)
    off.count[:] = -5
    dead0, _, done0, st0 = _call(eng, off)
    assert list(off.count) == [-5, -5] and list(done0) == [2, 2]
    for e in range(2):
        for x, y in zip(dead[e], dead0[e]):
            assert np.array_equal(x, y)
    for key in ('rows', 'rounds', 'host_waits', 'engine_calls'):
        assert st[key] == st0[key], key
    np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)


def test_boosted_summaries_of_every_mock(mock_vega, tmp_path):
    """The exact linear-broadband problem of tests/test_nested_set_gpu.py (four additive broadband coefficients: chi2 against
    mock m is exactly quadratic, the posterior the Gaussian of the device MIGRAD fit of mock m).  Three mocks at (nlive 128, K 32),
    8 repeats, every inner point kept (b = 8) against b = 0: the evidences are the same numbers; the Kish size n_eff of the chain
    used is at least 3 times the base chain's for every mock; the boosted weighted means lie within 5 sd / sqrt(ESS) of the exact
    ones with the ESS of the base chain - the phantoms of one walk are correlated, so the boosted chain's own Kish size overstates
    what it knows, and it is held to the bar the base chain gets (the figures with its own size are printed)."""
    from fits_standard import check_file
    from vega_amd import fitslite
    from vega_amd.montecarlo import MonteCarlo
    vega = mock_vega
    names = [f'BB-lyalya_lyalya-0 add post r,mu ({i},{j})' for i, j in ((0, 0), (0, 2), (1, 0), (2, 4))]
    mean, cov = _linear_gaussian(vega, names)
    sd = np.sqrt(np.diag(cov))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)},
          'values': dict(zip(names, mean)), 'errors': dict(zip(names, sd))}
    M = 3
    mc = MonteCarlo(vega)
    vega.freeze_metals()
    mocks = mc.create_mocks(vega.compute_model(dict(zip(names, mean))), M, seed=1)
    fits = mc._fit_mocks(mocks, M, sample_params=sp)
    assert np.all(fits.is_valid) and not np.any(fits.hesse_failed)
    best, hesse = fits.values, fits.covariance
    kw = dict(mocks=mocks, seed=11, sample_params=sp, num_live=128, threads=32, num_repeats=8, precision=1e-3)
    base = mc.sample_mocks_nested(**kw)
    post0, found0 = mc.mc_posteriors, base.samples()
    assert 'n_eff' not in post0 and 'phantoms' not in post0 and 'boost_posterior' not in post0
    boosted = mc.sample_mocks_nested(boost_posterior=8, **kw)
    post = mc.mc_posteriors
    assert boosted.driver == 'device' and list(boosted.status) == [1] * M and np.all(boosted.finished)
    assert np.array_equal(post['log_z'], post0['log_z']) and np.array_equal(post['log_z_err'], post0['log_z_err'])
    assert np.array_equal(post['iterations'], post0['iterations']) and boosted.stats['rows'] == base.stats['rows']
    assert boosted.stats['host_waits'] == base.stats['host_waits'] and post['boost_posterior'] == 8.0
    for m in range(M):
        w0 = found0[m][2]
        ess0 = 1.0 / np.sum(w0 * w0)
        pts, _, w = boosted.samples()[m]
        sd_m = np.sqrt(np.diag(hesse[m]))
        pull = (post['mean'][m] - best[m]) / (sd_m / math.sqrt(ess0))
        print(f'mock {m}: phantoms {post["phantoms"][m]}, n_eff {post["n_eff"][m]:.0f} / base {ess0:.0f} = {post["n_eff"][m] / ess0:.2f}, '
              f'mean pulls {np.round(pull, 2).tolist()} (with its own size: '
              f'{np.round((post["mean"][m] - best[m]) / (sd_m / math.sqrt(post["n_eff"][m])), 2).tolist()}; base chain '
              f'{np.round((post0["mean"][m] - best[m]) / (sd_m / math.sqrt(ess0)), 2).tolist()}), sd ratio '
              f'{np.round(post["sd"][m] / sd_m, 3).tolist()}, log Z_boost - log Z {post["log_z_boost"][m] - post["log_z"][m]:+.3f}')
        assert post['n_eff'][m] == 1.0 / np.sum(w * w) and post['phantoms'][m] == boosted.phantoms(m)['lnl'].size
        assert np.array_equal(post['mean'][m], w @ pts)
        assert post['n_eff'][m] >= 3.0 * ess0, (m, post['n_eff'][m], ess0)
        assert np.all(np.abs(pull) <= 5), (m, pull)
    path = mc.write_mock_posteriors(tmp_path)
    check_file(path)
    with fitslite.open(str(path)) as hdus:
        assert hdus[1].columns.names[-3:] == ['phantoms', 'n_eff', 'log_z_boost'] and hdus[1].header['BOOST'] == 8.0
        np.testing.assert_array_equal(hdus[1].data['n_eff'], post['n_eff'])


def test_a_member_writes_the_boosted_chain(auto_vega, linear_box, tmp_path):
    """The chain ``member(e).write()`` writes has the base run's rows plus the phantoms at or below its last death (merged among
    the deaths) and those above it (beside the live points)."""
    from vega_amd import NestedSet
    from vega_amd.nested import read_stats
    s = NestedSet(auto_vega, 2, num_live=40, threads=12, num_repeats=4, seed=5, sample_params=linear_box, boost_posterior=4).run(5)
    member = s.member(1)
    txt, _, stats = member.write(tmp_path, 'run1')
    table = np.loadtxt(txt)
    ph = s.phantoms(1)
    last = s.dead(1)[1][-1]
    early, late = int(np.sum(ph['lnl'] <= last)), int(np.sum(ph['lnl'] > last))
    print(f'member 1: {5 * 12} deaths, 40 live points, {early} phantoms at or below the last death, {late} above it')
    assert early > 0 and late > 0 and table.shape == (5 * 12 + 40 + early + late, 2 + len(member.names))
    pts, lnl, w = s.samples()[1]
    assert np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts) and np.array_equal(table[:, 0], w / w.max())
    # the last rows are the live points and the late phantoms, in that order
    assert np.array_equal(lnl[-(40 + late):-late], s.runs[1].live_lnl) and np.all(lnl[-late:] > last)
    found = read_stats(stats)
    assert found['phantom points'] == early + late and found['log(Z)'] == s.log_evidence()[0][1]
    assert found['log(Z) boosted'] == s.boost_log_evidence()[1]
