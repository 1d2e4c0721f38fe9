"""``boost_posterior`` on the device (include/vegamx.h: vmx_nested_run_phantoms; k_ns_advance_phantoms and
k_ns_advance_phantoms_clustered) against the NumPy restatement (the `python` driver of vega_amd/nested.py) on a real engine: the
same phantom record bit for bit beside an unchanged base run, several threads per lane, the record against the engine, a clustered
run, a run cut into calls, refused arguments that leave the engine as it was, and the config key end to end."""
import configparser
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN, marginalization_problem, MARGINALIZATION_CASES

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
LIMITS = {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0), 'ap': (0.5, 1.5), 'at': (0.5, 1.5)}


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _sample_params(vega, names=AUTO_SAMPLED, limits=None):
    limits = limits or {}
    return {'limits': {n: limits.get(n, LIMITS[n]) for n in names}, 'values': {n: vega.params[n] for n in names}, 'errors': {}}


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


def _assert_same_record(a, b, clusters=False):
    assert a['lnl'].shape == b['lnl'].shape and a['u'].shape == b['u'].shape
    assert np.array_equal(a['tag'], b['tag'])
    for key in ('u', 'lnl', 'birth'):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    if clusters:
        assert a['cluster'].dtype == b['cluster'].dtype == np.int32 and np.array_equal(a['cluster'], b['cluster'])
    else:
        assert a['cluster'] is None and b['cluster'] is None


def _assert_same_base(a, b):
    """The dead record and the live state of two runs on the same driver: every bit."""
    for x, y in zip(a.dead(), b.dead()):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert np.array_equal(a.live_u, b.live_u) and np.array_equal(a.live_lnl, b.live_lnl) and a.iteration == b.iteration
    for key in ('rows', 'rounds', 'rows_own_position', 'iterations', 'host_waits', 'engine_calls'):
        assert a.stats[key] == b.stats[key], key


def _complete_and_unique(rec, iterations, K, num_repeats):
    """Every (iteration, thread, repeat) of a run whose steps never give up, once, in the canonical order."""
    want = np.array([(t, k, r) for t in range(iterations) for k in range(K) for r in range(1, num_repeats)], dtype=np.int64)
    return np.array_equal(rec['tag'], want.reshape(-1, 3))


@pytest.mark.parametrize('f', [1.0, 0.3])
def test_drivers_agree_on_auto(auto_vega, f):
    """nlive 256 / K 64, 4 slice steps, 4 iterations: the phantom record of the device is that of the `python` driver in every
    bit; its dead record and live state are those of a device run without boost, on the same count of rounds, rows and waits."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    kw = dict(num_live=256, threads=64, num_repeats=4, seed=7, sample_params=sp)
    dev = NestedSampler(auto_vega, driver='device', boost_posterior=4 * f, **kw).run(iterations=4)
    py = NestedSampler(auto_vega, driver='python', boost_posterior=4 * f, **kw).run(iterations=4)
    off = NestedSampler(auto_vega, driver='device', **kw).run(iterations=4)
    assert dev.driver == off.driver == 'device' and py.driver == 'python' and dev.phantom_state.fraction == f
    a, b = dev.phantoms(), py.phantoms()
    _report(f'f = {f}, device against python', a, b)
    _assert_same_record(a, b)
    _assert_same_base(dev, off)
    assert np.all(a['lnl'] > a['birth']) and np.all((a['u'] >= 0) & (a['u'] <= 1))
    if f == 1.0:
        assert 0 < a['lnl'].size <= 4 * 64 * 3 and len({tuple(t) for t in a['tag']}) == a['lnl'].size
    else:
        assert abs(a['lnl'].size / (4 * 64 * 3) - f) < 0.1       # (768 draws: six standard deviations of the share)
    pts, lnl, w = dev.samples()
    assert pts.shape == (4 * 64 + 256 + a['lnl'].size, 4) and abs(w.sum() - 1) < 1e-12
    assert dev.log_evidence() == off.log_evidence() and math.isfinite(dev.boost_log_evidence())


def test_several_threads_per_lane(auto_vega):
    """K = 1088 threads on the work-group's 1024 lanes: a lane owns two contiguous threads and both can accept in one round."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    kw = dict(num_live=1152, threads=1088, num_repeats=2, seed=3, sample_params=sp, boost_posterior=2)
    dev = NestedSampler(auto_vega, driver='device', **kw).run(iterations=2)
    py = NestedSampler(auto_vega, driver='python', **kw).run(iterations=2)
    a, b = dev.phantoms(), py.phantoms()
    _report('K = 1088, device against python', a, b)
    _assert_same_record(a, b)
    assert _complete_and_unique(a, 2, 1088, 2)


def test_the_record_is_consistent_with_the_engine(auto_vega):
    """The recorded phantom points evaluated again through ``chi2_batch_device``: the recorded lnL in every bit, above the
    birth contour."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    s = NestedSampler(auto_vega, num_live=256, threads=64, num_repeats=4, seed=7, sample_params=sp, boost_posterior=4)
    s.run(iterations=4)
    assert s.driver == 'device'
    rec = s.phantoms()
    with s._engine_rows() as s._rows:
        again = s._evaluate(rec['u'])
    s._rows = None
    diff = np.abs(again - rec['lnl']) / np.abs(rec['lnl'])
    print(f'{rec["lnl"].size} phantom points evaluated again: {int(np.sum(_bits(again) != _bits(rec["lnl"])))} differ in a bit, '
          f'largest relative difference {diff.max():.3g}')
    assert np.array_equal(_bits(again), _bits(rec['lnl']))
    assert np.all(rec['lnl'] > rec['birth'])
    # the birth contour is the L* of the iteration: the lnL of its last death
    lstar = s.dead()[1].reshape(4, 64)[:, -1]
    assert np.array_equal(rec['birth'], lstar[rec['tag'][:, 0]])


def test_clustered_run_with_boost(auto_vega):
    """The clustered run of tests/test_nested_cluster_gpu.py (nlive 256 / K 64, 3 iterations) with boost: the device equals the
    `python` driver, the phantoms' cluster ids included; the base run is the clustered run without boost."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    kw = dict(num_live=256, threads=64, num_repeats=4, seed=7, sample_params=sp, clustering=True)
    dev = NestedSampler(auto_vega, driver='device', boost_posterior=4, **kw).run(iterations=3)
    py = NestedSampler(auto_vega, driver='python', boost_posterior=4, **kw).run(iterations=3)
    off = NestedSampler(auto_vega, driver='device', **kw).run(iterations=3)
    a, b = dev.phantoms(), py.phantoms()
    _report('clustered, device against python', a, b)
    _assert_same_record(a, b, clusters=True)
    _assert_same_base(dev, off)
    assert np.array_equal(dev.cluster_ids(), off.cluster_ids()) and np.array_equal(dev.cluster_ids(), py.cluster_ids())
    assert np.all(a['cluster'] >= 1) and np.all(a['cluster'] < dev.cluster_state.next_id)
    assert dev.samples()[0].shape[0] == 3 * 64 + 256 + a['lnl'].size
    with pytest.raises(ValueError, match='not boosted'):
        dev.samples(cluster=int(a['cluster'][0]), boost=True)


def test_the_boosted_run_does_not_depend_on_the_cut(auto_vega):
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    kw = dict(num_live=128, threads=64, num_repeats=4, seed=5, sample_params=sp, boost_posterior=1.2)
    one = NestedSampler(auto_vega, **kw).run(iterations=4)
    cut = NestedSampler(auto_vega, **kw)
    cut.run(iterations=2)
    cut.run(iterations=2)
    assert one.stats['calls'] == 1 and cut.stats['calls'] == 2 and one.driver == cut.driver == 'device'
    a, b = one.phantoms(), cut.phantoms()
    _report('2 + 2 iterations against 4', a, b)
    _assert_same_record(a, b)
    assert 0 < a['lnl'].size < 4 * 64 * 3
    for x, y in zip(one.dead(), cut.dead()):
        assert np.array_equal(x, y)
    assert np.array_equal(one.live_u, cut.live_u) and np.array_equal(one.live_lnl, cut.live_lnl)
    for x, y in zip(one.samples(), cut.samples()):
        assert np.array_equal(x, y)


def _raw_call(eng, s, fraction, capacity=None, drop=None, n_iterations=2):
    """vmx_nested_run_phantoms as a foreign caller makes it (16 live points, 4 threads, 3 slice steps): (rc, count)."""
    from vega_amd import engine as M
    n, nlive, K, R = 2, 16, 4, 3
    cols = np.array([eng.names.index('bias_eta_LYA'), eng.names.index('beta_LYA')], dtype=np.int32)
    lo, hi = np.array([-0.5, 0.5]), np.array([0.0, 3.0])
    theta = np.ascontiguousarray(eng.low.theta0, dtype=np.float64).copy()
    live_u, live_lnl = np.full((nlive, n), 0.5), np.zeros(nlive)
    rows = n_iterations * K
    cap = rows * (R - 1) if capacity is None else capacity
    size = rows * (R - 1)
    arr = dict(u=np.zeros((size, n)), lnl=np.zeros(size), birth=np.zeros(size), iteration=np.zeros(size, dtype=np.int64),
               thread=np.zeros(size, dtype=np.int32), repeat=np.zeros(size, dtype=np.int32))
    ptr = {k: (None if k == drop else v.ctypes.data_as(C.POINTER({'iteration': C.c_int64, 'thread': C.c_int32,
                                                                'repeat': C.c_int32}.get(k, C.c_double)))) for k, v in arr.items()}
    ph = M.NestedPhantoms(fraction, cap, ptr['u'], ptr['lnl'], ptr['birth'], ptr['iteration'], ptr['thread'], ptr['repeat'], None,
                          -5, 0, 0)
    spec = M.NestedSpec(eng.n_params, n, M._ip(cols), M._dp(lo), M._dp(hi), nlive, K, R, 0, float(s.log_norm()), 3, 0, M._dp(theta))
    opt = M.NestedOptions(-1, 0, 0, 1, M.NESTED_STOP(), None)
    stats, it = M.NestedStats(), C.c_int64(0)
    du, dl, dn = np.zeros((rows, n)), np.zeros(rows), np.zeros(rows, dtype=np.int32)
    rc = eng.lib.vmx_nested_run_phantoms(eng._h, C.byref(spec), M._dp(live_u), M._dp(live_lnl), C.byref(it), n_iterations, M._dp(du),
                                         M._dp(dl), M._ip(dn), C.byref(opt), C.byref(stats), None, C.byref(ph))
    return rc, int(ph.count), (du, dl, dn, live_u, live_lnl), arr


def test_refused_arguments_leave_the_engine_as_it_was(auto_vega):
    """A fraction outside [0, 1] or NaN, a capacity below n_iterations K (num_repeats - 1), a missing array: -1 with the reason,
    the struct and the engine untouched; the run that follows gives the record of the run before."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega, ['bias_eta_LYA', 'beta_LYA'])
    s = NestedSampler(auto_vega, num_live=16, threads=4, num_repeats=3, seed=3, sample_params=sp)
    theta = auto_vega._theta(None)[None, :]
    before = auto_vega.chi2_batch(theta)
    eng = auto_vega.engine
    rc, count, known, rec = _raw_call(eng, s, 1.0)
    assert rc == 0 and 0 < count <= 2 * 4 * 2 and np.all(rec['lnl'][:count] > rec['birth'][:count])
    for case in (dict(fraction=1.5), dict(fraction=math.nan), dict(fraction=-0.25), dict(fraction=1.0, capacity=2 * 4 * 2 - 1),
                 dict(fraction=1.0, drop='u'), dict(fraction=0.5, drop='birth'), dict(fraction=0.5, drop='repeat')):
        rc, count, out, _ = _raw_call(eng, s, **case)
        assert rc == -1 and 'invalid argument' in eng.lib.vmx_last_error().decode(), case
        assert count == -5 and not out[0].any() and not out[1].any(), case         # (nothing was written)
        np.testing.assert_array_equal(auto_vega.chi2_batch(theta), before)
    # fraction 0 runs vmx_nested_run and touches nothing in the struct, whatever else it holds
    rc, count, plain, rec0 = _raw_call(eng, s, 0.0, capacity=0, drop='lnl')
    assert rc == 0 and count == -5 and not rec0['u'].any()
    rc, count, again, rec1 = _raw_call(eng, s, 1.0)
    assert rc == 0
    for x, y, z in zip(known, again, plain):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    for key in rec:
        assert np.array_equal(rec[key], rec1[key]), key


def test_run_vega_sampler_end_to_end(tmp_path):
    """``[Nested] boost_posterior = 2`` (nlive 64 / K 16, 4 slice steps: half of the inner points) with ``derived = True``: the
    chain carries the phantom rows with their derived columns, the stats file the two lines."""
    from vega_amd import run_vega_sampler
    from vega_amd.nested import NestedSampler, read_stats
    prob = marginalization_problem(tmp_path, MARGINALIZATION_CASES['rtmax'])
    sampled = list(prob.sample_params['limits'])
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / 'configs' / 'marg' / 'main.ini')
    cfg['control']['run_sampler'] = 'True'
    cfg['control']['sampler'] = 'Nested'
    out = tmp_path / 'chains'
    out.mkdir()
    cfg['Nested'] = {'path': str(out), 'name': 'boosted', 'num_live': '64', 'num_repeats': '4', 'threads': '16', 'seed': '4',
                     'max_iterations': '5', 'boost_posterior': '2', 'derived': 'True'}
    (tmp_path / 'configs' / 'ns').mkdir(parents=True)
    with open(tmp_path / 'configs' / 'ns' / 'main.ini', 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler('configs/ns/main.ini', search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None, max_batch=16)
    try:
        assert isinstance(sampler, NestedSampler) and sampler.driver == 'device' and sampler.iteration == 5
        assert sampler.boost_posterior == 2.0 and sampler.phantom_state.fraction == 0.5
        n_ph = sampler.phantoms()['lnl'].size
        assert 0 < n_ph < 5 * 16 * 3
        names = sampler.vega.derived_names()
        table = np.loadtxt(out / 'boosted.txt')
        pts, lnl, w = sampler.samples()
        assert len(names) == 200 and table.shape == (5 * 16 + 64 + n_ph, 2 + len(sampled) + len(names))
        assert np.array_equal(table[:, 0], w / w.max()) and np.array_equal(table[:, 1], -lnl)
        assert np.array_equal(table[:, 2:2 + len(sampled)], pts)
        block = sampler.derived()
        assert block.shape == (pts.shape[0], len(names)) and np.array_equal(table[:, 2 + len(sampled):], block)
        stats = read_stats(out / 'boosted.stats')
        assert stats['phantom points'] == n_ph and stats['log(Z) boosted'] == sampler.boost_log_evidence()
        assert (stats['log(Z)'], stats['log(Z) error']) == sampler.log_evidence() and stats['dead points'] == 5 * 16
    finally:
        sampler.vega.close()
