"""Clustering in the nested sampler on the device: the two kernels behind vmx_nested_cluster_points (k_ns_knn, k_ns_cluster) against
the NumPy restatement of vega_amd/nested.py bit for bit; the device and `python` drivers of NestedSampler(clustering=True) on a
real engine, whole and cut; vmx_nested_run_clustered with flags 0 against vmx_nested_run."""
import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
LIMITS = {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0), 'ap': (0.5, 1.5), 'at': (0.5, 1.5)}


def _blobs(rng, n, sizes, centres, sigma):
    return np.concatenate([np.clip(c + sigma * rng.standard_normal((s, n)), 0.0, 1.0) for s, c in zip(sizes, centres)])


def _points(n, m):
    """(u [m, n], prev_id [m], next_id): (1, 70) uniform; (6, 163) one blob in a ragged single tile; (6, 600) three tiles with a
    ragged tail - two blobs, 20 of the points copies of others, and previous ids that make both blobs claim id 4; (32, 300) two
    blobs at the largest LDS tile."""
    rng = np.random.default_rng(100 * n + m)
    if (n, m) == (1, 70):
        return rng.random((70, 1)), np.zeros(70, dtype=np.int32), 1
    if (n, m) == (6, 163):
        return _blobs(rng, 6, [163], [0.5], 0.05), np.full(163, 2, dtype=np.int32), 3
    if (n, m) == (6, 600):
        u = _blobs(rng, 6, [340, 240], [0.3, 0.7], 0.02)
        prev = np.full(580, 4, dtype=np.int32)
        prev[:30], prev[340:360] = 1, 0
        extra = rng.integers(0, 580, 20)
        u, prev = np.concatenate([u, u[extra]]), np.concatenate([prev, prev[extra]])
        perm = rng.permutation(600)
        return u[perm], prev[perm], 6
    if (n, m) == (32, 300):
        return _blobs(rng, 32, [180, 120], [0.35, 0.65], 0.02), np.zeros(300, dtype=np.int32), 1
    raise KeyError((n, m))


@pytest.mark.parametrize('n, m', [(1, 70), (6, 163), (6, 600), (32, 300)])
def test_cluster_points_on_the_device_equal_the_restatement_bitwise(n, m):
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    from vega_amd import nested as N
    u, prev, next_id = _points(n, m)
    want = N.cluster_points(u, prev, next_id)
    got = engine.cluster_points(u, prev, next_id)
    assert got['k'] == want['k'] and got['n_clusters'] == want['n_clusters'] and got['next_id'] == want['next_id']
    assert np.array_equal(got['ids'], want['ids'])
    assert got['mean'].shape == want['mean'].shape and got['C'].shape == want['C'].shape
    assert np.array_equal(got['mean'].view(np.uint64), want['mean'].view(np.uint64))
    assert np.array_equal(got['C'].view(np.uint64), want['C'].view(np.uint64))
    if (n, m) == (6, 600):      # the larger blob keeps the id both claimed, the other takes a new one
        assert want['n_clusters'] == 2 and list(want['cluster_id']) == [4, 6] and want['next_id'] == 7
        nn, d2 = N.nearest_neighbours(u)
        assert np.sum(d2[np.arange(m), nn[:, 0]] == 0.0) >= 21        # (20 copies and at least one original)
    if (n, m) == (32, 300):
        assert want['n_clusters'] == 2 and list(want['sizes']) == [180, 120]


def test_cluster_points_refusals():
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    u = np.random.default_rng(0).random((20, 2))
    zero = np.zeros(20, dtype=np.int32)
    for bad in (dict(u=np.random.default_rng(0).random((20, 33)), prev_id=zero, next_id=1), dict(u=u[:1], prev_id=zero[:1], next_id=1),
                dict(u=u, prev_id=zero + 3, next_id=3), dict(u=u, prev_id=zero, next_id=0),
                dict(u=np.where(np.arange(40).reshape(20, 2) == 7, np.nan, u), prev_id=zero, next_id=1)):
        with pytest.raises(engine.EngineError, match='invalid argument'):
            engine.cluster_points(**bad)


# ------------------------------------------------------------------ the drivers
@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _sample_params(vega):
    return {'limits': dict(LIMITS), 'values': {n: vega.params[n] for n in AUTO_SAMPLED}, 'errors': {}}


def _assert_same(a, b):
    assert np.array_equal(a.dead()[0], b.dead()[0]) and np.array_equal(a.dead()[2], b.dead()[2])
    np.testing.assert_allclose(a.dead()[1], b.dead()[1], rtol=1e-12, atol=0)
    assert np.array_equal(a.live_u, b.live_u)
    np.testing.assert_allclose(a.live_lnl, b.live_lnl, rtol=1e-12, atol=0)
    assert a.iteration == b.iteration
    assert np.array_equal(a.cluster_ids(), b.cluster_ids())
    assert np.array_equal(a.cluster_state.live_cluster, b.cluster_state.live_cluster)
    assert a.cluster_state.next_id == b.cluster_state.next_id
    for key in ('rows', 'rounds', 'rows_own_position', 'iterations'):
        assert a.stats[key] == b.stats[key], key


def test_drivers_agree_with_clustering_whole_and_cut(auto_vega):
    """nlive 256 / K 64, 3 iterations: the device and `python` drivers give the same dead record with its ids, the same
    live_cluster and next_id; the device run cut 1 + 2 is the same run."""
    from vega_amd import NestedSampler
    sp = _sample_params(auto_vega)
    kw = dict(num_live=256, threads=64, seed=7, sample_params=sp, clustering=True)
    dev = NestedSampler(auto_vega, driver='device', **kw).run(iterations=3)
    py = NestedSampler(auto_vega, driver='python', **kw).run(iterations=3)
    assert dev.driver == 'device' and py.driver == 'python'
    _assert_same(dev, py)
    ids = dev.cluster_ids()
    assert ids.shape == (3 * 64 + 256,) and np.all(ids[:64] == 0) and np.all(ids[64:] >= 1)
    assert dev.cluster_state.next_id >= 2 and np.all(dev.cluster_state.live_cluster < dev.cluster_state.next_id)
    assert abs(sum(c['mass'] for c in dev.clusters()) - 1) <= 1e-12
    cut = NestedSampler(auto_vega, driver='device', **kw)
    cut.run(iterations=1)
    cut.run(iterations=2)
    assert cut.stats['calls'] == 2
    _assert_same(cut, dev)
    assert np.array_equal(cut.dead()[1], dev.dead()[1]) and np.array_equal(cut.live_lnl, dev.live_lnl)


def test_flags_zero_run_what_vmx_nested_run_runs(auto_vega):
    """vmx_nested_run_clustered with the flags word 0 against vmx_nested_run over 2 iterations: every output bit for bit, and
    the clusters' arrays untouched."""
    from vega_amd import NestedSampler
    from vega_amd import nested as N
    sp = _sample_params(auto_vega)
    s = NestedSampler(auto_vega, num_live=128, threads=32, num_repeats=6, seed=3, sample_params=sp)
    s._begin_advance(lambda: N.draw_live(1, s.n, s.seed, s.stream)[0], 'nested_run')
    assert s.driver == 'device'
    auto_vega._sync_monte_carlo()
    out = []
    for clustered in (False, True):
        live_u, live_lnl = np.zeros((128, 4)), np.zeros(128)
        state = N.ClusterState(128)
        state.live_cluster[:] = -7          # (never read, never written with flags 0)
        extra = dict(clusters=state, cluster_flags=0) if clustered else {}
        du, dl, dn, it, st = auto_vega.engine.nested_run(s.cols, s.lo, s.hi, s._theta, live_u, live_lnl, 0, 2, 32, 6,
                                                         log_norm=s.log_norm(), seed=3, stream=0, draw_live=True, **extra)
        out.append((du, dl, dn, live_u, live_lnl))
        assert it == 2 and st['iterations'] == 2
        if clustered:
            assert np.all(state.live_cluster == -7) and state.next_id == 1 and not state.dead[0].any()
    for a, b in zip(*out):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert out[0][0].shape == (64, 4)
