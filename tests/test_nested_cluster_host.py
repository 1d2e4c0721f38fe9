"""Clustering in the nested sampler without a GPU: the rule of vega_amd/csrc/vmx_nested.h ("clustering"), compiled with g++ under
AddressSanitizer / UBSan into tests/helpers/nested_cluster_driver.cpp, against the NumPy restatement of vega_amd/nested.py bit for
bit; two anisotropic modes (evidence, evaluations per slice step, rounds, what the ids hold); one mode; independence of the cut;
the settings, refusals and writers."""
import configparser
import ctypes as C
import math
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vega_amd import ensemble as E
from vega_amd import nested as N


# ------------------------------------------------------------------ header <-> NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('nested_cluster') / 'nested_cluster_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'nested_cluster_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _ask(exe, text):
    out = subprocess.run([str(exe)], input=text + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout.splitlines()


def _hx(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0].to_bytes(8, 'big').hex()


def _hexes(a):
    return ' '.join(_hx(v) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _ints(a):
    return ' '.join(str(int(v)) for v in np.asarray(a).reshape(-1))


def _doubles(tokens):
    return np.array([struct.unpack('<d', struct.pack('<Q', int(t, 16)))[0] for t in tokens])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _blobs(rng, n, sizes, centres, sigma):
    return np.concatenate([np.clip(c + sigma * rng.standard_normal((s, n)), 0.0, 1.0) for s, c in zip(sizes, centres)])


def cluster_case(name):
    """(u [m, n], prev_id [m], next_id, what the case must show) of the named point set."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'n1':
        u = rng.random((70, 1))
        return u, np.zeros(70, dtype=np.int32), 1, {}
    if name == 'n2 below 2n+2':             # m = 5 < 2 n + 2 = 6: no component can be sizeable
        return rng.random((5, 2)), np.zeros(5, dtype=np.int32), 1, dict(n_clusters=1, ids={1})
    if name == 'n6 one blob':
        u = _blobs(rng, 6, [163], [0.5], 0.05)
        return u, np.full(163, 3, dtype=np.int32), 4, dict(n_clusters=1, ids={3})
    if name == 'n6 two blobs':
        u = _blobs(rng, 6, [350, 250], [0.3, 0.7], 0.02)
        u = u[rng.permutation(600)]
        return u, np.zeros(600, dtype=np.int32), 1, dict(n_clusters=2, ids={1, 2})
    if name == 'n32':
        u = _blobs(rng, 32, [180, 120], [0.35, 0.65], 0.02)
        return u, np.zeros(300, dtype=np.int32), 7, dict(n_clusters=2, ids={7, 8})
    if name == 'duplicates':                # a slice step that gives up leaves a copy of its start
        u = _blobs(rng, 2, [40, 40], [0.25, 0.75], 0.03)
        u = np.concatenate([u, u[rng.integers(0, 80, 25)], u[:3], u[:3]])
        u = u[rng.permutation(u.shape[0])]
        return u, np.zeros(u.shape[0], dtype=np.int32), 1, {}
    if name == 'identical':
        return np.full((40, 3), 0.375), np.zeros(40, dtype=np.int32), 2, dict(n_clusters=1, cholesky=[False])
    if name == 'same id claimed twice':     # both blobs' majorities held id 5: the larger keeps it, the other gets a new one
        u = _blobs(rng, 2, [90, 60], [0.3, 0.7], 0.02)
        prev = np.full(150, 5, dtype=np.int32)
        prev[:10], prev[90:100] = 2, 0
        return u, prev, 9, dict(n_clusters=2, cluster_id=[5, 9], next_id=10)
    if name == 'ties between ids':          # equal counts of ids 4 and 2 in one cluster: the lower id
        u = _blobs(rng, 2, [60], [0.5], 0.05)
        prev = np.zeros(60, dtype=np.int32)
        prev[:20], prev[20:40] = 4, 2
        return u, prev, 6, dict(n_clusters=1, cluster_id=[2], next_id=6)
    raise KeyError(name)


CLUSTER_CASES = ['n1', 'n2 below 2n+2', 'n6 one blob', 'n6 two blobs', 'n32', 'duplicates', 'identical', 'same id claimed twice',
                 'ties between ids']


def _check_cluster_lines(lines, cl, n):
    """The driver's lines N K S I Z M F W against :func:`vega_amd.nested.cluster_points`."""
    nc = cl['n_clusters']
    assert [ln.split()[0] for ln in lines] == list('NKSIZMFW')
    tok = [ln.split()[1:] for ln in lines]
    assert [int(t) for t in tok[0]] == [int(v) for v in cl['nn'].reshape(-1)]
    assert [int(t) for t in tok[1]] == [cl['k'], nc, cl['next_id']]
    assert [int(t) for t in tok[2]] == [int(v) for v in cl['slot']]
    assert [int(t) for t in tok[3]] == [int(v) for v in cl['ids']]
    assert [int(t) for t in tok[4]] == [int(v) for v in cl['cluster_id']] + [int(v) for v in cl['sizes']]
    assert _same_bits(_doubles(tok[5]), cl['mean'])
    assert [int(t) for t in tok[6]] == [int(v) for v in cl['cholesky']]
    assert _same_bits(_doubles(tok[7]), cl['C'])


@pytest.mark.parametrize('name', CLUSTER_CASES)
def test_cluster_rule_header_equals_the_restatement_bitwise(driver, name):
    """Neighbour lists (ties by position), the level used, components, the order of the clusters, the loose points, ids, means
    and factors: the header compiled by g++ and the NumPy restatement agree in everything."""
    u, prev, next_id, want = cluster_case(name)
    m, n = u.shape
    cl = N.cluster_points(u, prev, next_id)
    lines = _ask(driver, f'C {m} {n} {next_id} {_hexes(u)} {_ints(prev)}')
    _check_cluster_lines(lines, cl, n)
    # what the rule promises, whatever computed it
    assert 3 <= cl['k'] <= N.KNN and 1 <= cl['n_clusters'] <= N.MAX_CLUSTERS
    assert cl['sizes'].sum() == m and np.all(cl['sizes'] >= 1)        # (ordered by component size; the attached points come on top)
    assert len(set(cl['cluster_id'].tolist())) == cl['n_clusters'] and np.all(cl['cluster_id'] >= 1)
    assert cl['next_id'] == max(next_id, cl['cluster_id'].max() + 1)
    kk = min(N.KNN, m - 1)
    assert np.all(cl['nn'][:, :kk] >= 0) and np.all(cl['nn'][:, kk:] == -1)
    assert np.all(cl['nn'][:, :kk] != np.arange(m)[:, None])
    for key, val in want.items():
        got = cl[key]
        if key == 'ids':
            assert set(got.tolist()) == val
        else:
            assert np.array_equal(np.asarray(got), np.asarray(val)), (key, got, val)
    if name == 'n6 two blobs':             # every blob one cluster, the larger first
        assert list(cl['sizes']) == [350, 250]
    if name == 'duplicates':               # copies are each other's nearest neighbours at distance 0, in order of position
        nn, d2 = N.nearest_neighbours(u)
        assert np.sum(d2[np.arange(m), nn[:, 0]] == 0.0) >= 50
        twins = np.flatnonzero(d2[np.arange(m), nn[:, 1]] == 0.0)
        assert twins.size and all(nn[i, 0] < nn[i, 1] for i in twins)


def _two_blob_state(n, nlive, rng):
    """Live points in two separated blobs with lnL that kills from both, and ids from an earlier iteration."""
    u = _blobs(rng, n, [nlive // 2, nlive - nlive // 2], [0.3, 0.7], 0.02)
    perm = rng.permutation(nlive)
    u = u[perm]
    in_a = perm < nlive // 2
    return u, in_a


def _two_mode_iso(n, sigma=0.02):
    def loglike(u):
        u = np.asarray(u)
        a = np.zeros(u.shape[0])
        b = np.zeros(u.shape[0])
        for i in range(n):
            a = a + (u[:, i] - 0.3) * (u[:, i] - 0.3)
            b = b + (u[:, i] - 0.7) * (u[:, i] - 0.7)
        return np.logaddexp(-0.5 * a / sigma**2, -0.5 * b / sigma**2)
    return loglike


@pytest.mark.parametrize('n, nlive, K', [(2, 96, 24), (6, 160, 32)])
def test_threads_with_per_cluster_factors_header_equals_the_restatement_bitwise(driver, n, nlive, K):
    """An iteration with clustering: the ids of the dead, the clustering of the survivors, the cluster of every start, every call
    of advance of every thread with the factor of its start's cluster, and the ids afterwards."""
    seed, stream, it, num_repeats = 5 + n, 2, 9, 3
    rng = np.random.default_rng(n)
    live_u, in_a = _two_blob_state(n, nlive, rng)
    loglike = _two_mode_iso(n)
    live_lnl = loglike(live_u)
    state = N.ClusterState(nlive)
    state.live_cluster[:] = np.where(in_a, 3, 1)
    state.live_cluster[rng.integers(0, nlive, 7)] = 0           # (points born without an id cannot occur, but the rule covers them)
    state.next_id = 4
    before = state.live_cluster.copy()
    head = N.iteration_head(live_u, live_lnl, K, it, seed, stream, clusters=state)
    assert head['cluster']['n_clusters'] == 2 and head['C_thread'].shape == (K, n, n)
    assert set(head['start_slot'].tolist()) == {0, 1}
    T = N.Threads(live_u[head['start']], live_lnl[head['start']], head['C_thread'], head['lstar'], it, num_repeats, seed, stream)
    answers, shots = [[] for _ in range(K)], [[] for _ in range(K)]

    def snap(ks, asks):
        for k in ks:
            shots[k].append((int(asks[k]), int(T.state[k]), int(T.repeat[k]), int(T.n_out[k]), int(T.n_shrink[k]),
                             int(T.inside[k]), int(T.draw[k]),
                             np.concatenate([[T.L[k], T.R[k], T.t[k], T.lnl[k]], T.x[k], T.y[k], T.d[k]])))

    asks = T.advance(np.full(K, -np.inf))
    snap(range(K), asks)
    while asks.any():
        ks, rows, _ = T.requests(asks)
        answer = np.full(K, -np.inf)
        answer[ks] = loglike(rows)
        for k in ks:
            answers[k].append(answer[k])
        asks = T.advance(answer)
        snap(ks, asks)
    after = state.live_cluster.copy()
    after[head['killed']] = head['cluster']['cluster_id'][head['start_slot']]
    text = f'I {n} {nlive} {K} {num_repeats} {it} {seed:x} {stream:x} 4 {_hexes(live_u)} {_hexes(live_lnl)} {_ints(before)} '
    text += ' '.join(f'{len(a)} {_hexes(a)}' for a in answers)
    lines = _ask(driver, text)
    assert [int(t) for t in lines[0].split()[1:]] == [int(v) for v in head['dead_cluster']] == [int(v) for v in before[head['killed']]]
    _check_cluster_lines(lines[1:9], head['cluster'], n)
    assert [int(t) for t in lines[9].split()[1:]] == [int(s) for s in head['start']]
    assert [int(t) for t in lines[10].split()[1:]] == [int(s) for s in head['start_slot']]
    rows = [ln.split() for ln in lines[11:-1]]
    assert all(r[0] == 'T' for r in rows)
    per_thread = [[r for r in rows if int(r[1]) == k] for k in range(K)]
    for k in range(K):
        assert len(per_thread[k]) == len(shots[k]) == len(answers[k]) + 1, k
        for r, s in zip(per_thread[k], shots[k]):
            assert [int(t) for t in r[2:9]] == list(s[:7]), (k, r[:9], s[:7])
            assert _same_bits(_doubles(r[9:]), s[7]), (k, r[:9])
    assert lines[-1].split()[0] == 'E'
    assert [int(t) for t in lines[-1].split()[1:]] == [int(v) for v in after] + [state.next_id]
    # the blobs keep the ids their majorities held; a thread stays in the blob it started in
    assert set(head['cluster']['cluster_id'].tolist()) == {1, 3} and state.next_id == 4
    near_a = np.sum((T.x - 0.3)**2, axis=1) < np.sum((T.x - 0.7)**2, axis=1)
    assert np.array_equal(near_a, in_a[head['start']])


# ------------------------------------------------------------------ two anisotropic modes
def _anisotropic_modes():
    """Two normalised Gaussians in n = 4 at 0.3 * 1 and 0.7 * 1 with covariance c o (s s^T): c the correlation matrix of a a^T,
    a = RandomState(11 | 12).randn(4, 4); s = 0.02 (1, 0.2, 0.2, 0.2) | 0.02 (0.2, 0.2, 0.2, 1).  log Z = log 2."""
    modes = []
    for rs, s, centre in ((11, 0.02 * np.array([1.0, 0.2, 0.2, 0.2]), 0.3), (12, 0.02 * np.array([0.2, 0.2, 0.2, 1.0]), 0.7)):
        a = np.random.RandomState(rs).randn(4, 4)
        q = a @ a.T
        d = np.sqrt(np.diag(q))
        cov = q / np.outer(d, d) * np.outer(s, s)
        modes.append((centre, np.linalg.inv(cov), -0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]))

    def loglike(u):
        u = np.asarray(u)
        parts = []
        for centre, prec, log_norm in modes:
            d = u - centre
            parts.append(log_norm - 0.5 * np.einsum('ri,ij,rj->r', d, prec, d))
        return np.logaddexp(parts[0], parts[1])

    return loglike


_TWO_MODE_RUNS = {}


def _two_mode_run(seed, clustering):
    key = (seed, clustering)
    if key not in _TWO_MODE_RUNS:
        _TWO_MODE_RUNS[key] = N.NestedRun(_anisotropic_modes(), 4, num_live=512, num_repeats=20, threads=128, seed=seed,
                                          clustering=clustering).run()
    return _TWO_MODE_RUNS[key]


def _rows_per_step(run):
    return (run.stats['rows'] - run.num_live) / (run.iteration * run.threads * run.num_repeats)


@pytest.mark.parametrize('seed', [0, 1])
def test_two_anisotropic_modes(seed):
    """Two modes that one covariance fits badly (each long along another axis), nlive 512 / K 128 / num_repeats 20.  Per seed:
    |log Z - log 2| <= 4 err; evaluations per slice step with clustering <= 0.85 x those of the same seed without (which is the
    run of before, bit for bit); fewer rounds; <= 0.01 of the mass on points whose id's majority mode (by nearest centre) is not
    their own; the two heaviest ids hold >= 0.97 of the mass; the masses sum to 1 to 1e-12.

    Measured (seed 0 | seed 1): rows per slice step 5.221 | 5.231 against 6.949 | 6.917 (ratio 0.751 | 0.756), rounds 10 723 |
    10 637 against 16 953 | 17 444, log Z pull -0.97 | -0.00, two heaviest ids 0.9905 | 1.0000, stray mass 6.4e-5 | 3.2e-4."""
    on, off = _two_mode_run(seed, True), _two_mode_run(seed, False)
    log_z, err = on.log_evidence()
    log_z_off, err_off = off.log_evidence()
    per_on, per_off = _rows_per_step(on), _rows_per_step(off)
    found = on.clusters()
    pts, _, w = on.samples()
    ids = on.cluster_ids()
    near_a = np.sum((pts - 0.3)**2, axis=1) < np.sum((pts - 0.7)**2, axis=1)
    stray = 0.0
    for c in found:
        mine = ids == c['id']
        mass_a, mass_b = w[mine & near_a].sum(), w[mine & ~near_a].sum()
        stray += min(mass_a, mass_b)
    total = sum(c['mass'] for c in found)
    top2 = found[0]['mass'] + (found[1]['mass'] if len(found) > 1 else 0.0)
    print(f'seed {seed}: clustering log Z {log_z:.4f} (true {math.log(2):.4f}, err {err:.4f}, pull {(log_z - math.log(2)) / err:+.2f}), '
          f'without {log_z_off:.4f} (pull {(log_z_off - math.log(2)) / err_off:+.2f}); rows per slice step {per_on:.3f} against '
          f'{per_off:.3f} (ratio {per_on / per_off:.3f}); rounds {on.stats["rounds"]} against {off.stats["rounds"]}; iterations '
          f'{on.iteration} against {off.iteration}; ids {[(c["id"], round(c["mass"], 5)) for c in found[:4]]} of {len(found)}; '
          f'two heaviest {top2:.5f}; stray mass {stray:.2e}; sum of masses - 1 {total - 1:.1e}')
    assert on.terminated and off.terminated
    assert abs(log_z - math.log(2)) <= 4 * err
    assert per_on <= 0.85 * per_off
    assert on.stats['rounds'] < off.stats['rounds']
    assert stray <= 0.01
    assert top2 >= 0.97
    assert abs(total - 1) <= 1e-12
    # samples(cluster=) are the rows of that id, their weights renormalised; the local evidences add up to the evidence
    p0, l0, w0 = on.samples(cluster=found[0]['id'])
    assert p0.shape[0] == found[0]['n_dead'] + found[0]['n_live'] == l0.size == w0.size and abs(w0.sum() - 1) < 1e-12
    assert np.array_equal(p0, pts[ids == found[0]['id']])
    assert abs(N._logsumexp([c['log_z'] for c in found]) - log_z) < 1e-12
    assert sum(c['n_live'] for c in found) == 512 and sum(c['n_dead'] for c in found) == on.iteration * 128
    with pytest.raises(ValueError):
        on.samples(cluster=10**6)
    with pytest.raises(ValueError):
        off.clusters()


# ------------------------------------------------------------------ one mode
def _correlated_gaussian(n, sigma=0.03):
    a = np.random.RandomState(1).randn(n, n)
    s = a @ a.T
    d = np.sqrt(np.diag(s))
    cov = s / np.outer(d, d) * sigma**2
    prec = np.linalg.inv(cov)

    def loglike(u):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ri,ij,rj->r', d, prec, d)

    return loglike, cov, 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]


def test_one_mode_with_clustering():
    """The correlated Gaussian of tests/test_nested_host.py (n = 4, nlive 512 / K 128, seed 0) with clustering on: the conditions
    of that test on log Z, H and the error.  Evaluations per slice step with clustering on and off are printed, not asserted."""
    n, nlive, K, seed = 4, 512, 128, 0
    loglike, cov, log_z_true = _correlated_gaussian(n)
    h_true = -log_z_true - n / 2
    run = N.NestedRun(loglike, n, num_live=nlive, num_repeats=5 * n, threads=K, seed=seed, clustering=True).run()
    off = N.NestedRun(loglike, n, num_live=nlive, num_repeats=5 * n, threads=K, seed=seed).run()
    log_z, err = run.log_evidence()
    info = run.information()
    pts, lnl, w = run.samples()
    ess = 1.0 / np.sum(w**2)
    pull = (w @ pts - 0.5) / (0.03 / np.sqrt(ess))
    found = run.clusters()
    print(f'one mode: log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}), H {info:.3f} '
          f'(true {h_true:.3f}); rows per slice step with clustering {_rows_per_step(run):.3f}, without {_rows_per_step(off):.3f} '
          f'(ratio {_rows_per_step(run) / _rows_per_step(off):.3f}); rounds {run.stats["rounds"]} against {off.stats["rounds"]}; '
          f'ids {[(c["id"], round(c["mass"], 4)) for c in found[:4]]} of {len(found)}')
    assert run.terminated
    assert abs(log_z - log_z_true) <= 4 * err
    assert abs(info - h_true) <= 0.1 * h_true
    assert abs(err - math.sqrt(h_true / nlive)) <= 0.1 * math.sqrt(h_true / nlive)
    assert np.all(np.abs(pull) <= 5), pull
    assert abs(w.sum() - 1) < 1e-12 and abs(sum(c['mass'] for c in found) - 1) <= 1e-12


# ------------------------------------------------------------------ smaller checks
def test_the_clustered_run_does_not_depend_on_the_cut():
    loglike = _two_mode_iso(3)
    kw = dict(num_live=128, num_repeats=4, threads=32, seed=2, clustering=True)
    one = N.NestedRun(loglike, 3, **kw)
    one.run(iterations=7)
    cut = N.NestedRun(loglike, 3, **kw)
    cut.run(iterations=3)
    cut.run(iterations=4)
    assert one.iteration == cut.iteration == 7 and cut.stats['calls'] == 2
    for a, b in zip(one.dead(), cut.dead()):
        assert a.shape == b.shape and _same_bits(a, b)
    assert _same_bits(one.live_u, cut.live_u) and _same_bits(one.live_lnl, cut.live_lnl)
    assert np.array_equal(one.cluster_ids(), cut.cluster_ids()) and one.cluster_ids().size == 7 * 32 + 128
    assert one.cluster_state.next_id == cut.cluster_state.next_id >= 3
    assert np.all(one.cluster_ids()[:32] == 0) and np.all(one.cluster_state.live_cluster >= 1)
    assert one.stats['rows'] == cut.stats['rows'] and one.stats['rounds'] == cut.stats['rounds']
    assert one.clusters() == cut.clusters()


def test_one_thread_with_clustering():
    loglike, cov, log_z_true = _correlated_gaussian(2)
    run = N.NestedRun(loglike, 2, num_live=64, num_repeats=10, threads=1, seed=0, clustering=True).run()
    _, lnl, counts = run.dead()
    assert np.all(counts == 64) and counts.size == run.iteration and np.all(np.diff(lnl) >= 0)
    log_z, err = run.log_evidence()
    print(f'K = 1 with clustering: log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}), iterations {run.iteration}')
    assert abs(log_z - log_z_true) <= 4 * err
    assert abs(sum(c['mass'] for c in run.clusters()) - 1) <= 1e-12


def test_clustering_off_is_the_run_of_before():
    """``clustering=False`` through the new arguments: python_iterations without a ClusterState, bit for bit what it was (the
    head's factor is the global one and the threads read it as a [n, n] array)."""
    loglike, _, _ = _correlated_gaussian(3)
    a = N.NestedRun(loglike, 3, num_live=96, num_repeats=6, threads=24, seed=4)
    b = N.NestedRun(loglike, 3, num_live=96, num_repeats=6, threads=24, seed=4, clustering=False)
    a.run(iterations=5)
    b.run(iterations=5)
    assert b.cluster_state is None and a.cluster_state is None
    for x, y in zip(a.dead(), b.dead()):
        assert _same_bits(x, y)
    assert _same_bits(a.live_u, b.live_u) and a.stats['rows'] == b.stats['rows']
    # ... and the head without a state is the head of before: one factor from all survivors
    head = N.iteration_head(a.live_u, a.live_lnl, 24, 5, 4, 0)
    mean, cov = N.mean_cov(a.live_u[head['surv']])
    assert _same_bits(head['cov'], cov) and head['C'].shape == (3, 3) and 'cluster' not in head
    # a single cluster's factor is the global one: same members, same sums
    state = N.ClusterState(96)
    one = N.iteration_head(a.live_u, a.live_lnl, 24, 5, 4, 0, clusters=state)
    if one['cluster']['n_clusters'] == 1:
        assert _same_bits(one['C'][0], head['C'])


def test_constructor_defaults_and_refusals():
    f = _two_mode_iso(3)
    run = N.NestedRun(f, 3)
    assert run.clustering is False and run.cluster_state is None
    on = N.NestedRun(f, 3, clustering=True)
    assert on.clustering and on.cluster_state.next_id == 1 and on.cluster_state.live_cluster.shape == (75,)
    assert on.cluster_state.live_cluster.dtype == np.int32 and not on.cluster_state.live_cluster.any()
    with pytest.raises(ValueError, match='clustering'):
        N.NestedRun(f, 3, clustering='yes')
    with pytest.raises(ValueError, match='clustering=True'):
        run.clusters()
    with pytest.raises(ValueError, match='nothing has run'):
        on.clusters()
    import inspect
    for cls in (N.NestedRun, N.NestedSampler):
        assert inspect.signature(cls.__init__).parameters['clustering'].default is False
    assert inspect.signature(N.NestedSampler.__init__).parameters['cluster_posteriors'].default is False
    assert N.KNN == 8 and N.MAX_CLUSTERS == 8


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Nested\n'


def test_cluster_settings(tmp_path):
    plain = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\n'), SAMPLE)
    assert 'do_clustering' not in plain and 'cluster_posteriors' not in plain
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ndo_clustering = True\n'), SAMPLE)
    assert s['do_clustering'] is True and 'cluster_posteriors' not in s
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ncluster_posteriors = True\n'), SAMPLE)
    assert s['do_clustering'] is True and s['cluster_posteriors'] is True
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ndo_clustering = False\ncluster_posteriors = True\n'), SAMPLE)
    assert s['do_clustering'] is True               # (cluster_posteriors implies it)
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ndo_clustering = False\ncluster_posteriors = False\n'), SAMPLE)
    assert s['do_clustering'] is False and s['cluster_posteriors'] is False
    # replicas: clustering is allowed, per-cluster chains are not (ids of different replicas are unrelated)
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ndo_clustering = True\nreplicas = 3\n'), SAMPLE)
    assert s['do_clustering'] is True and s['replicas'] == 3
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ncluster_posteriors = True\nreplicas = 1\n'), SAMPLE)
    assert s['cluster_posteriors'] is True
    with pytest.raises(ValueError, match='cluster_posteriors'):
        E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ncluster_posteriors = True\nreplicas = 2\n'), SAMPLE)
    with pytest.raises(ValueError):
        E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\ndo_clustering = perhaps\n'), SAMPLE)


def test_merged_replicas_drop_the_ids():
    from vega_amd import replicas as R
    loglike = _two_mode_iso(2)
    runs = [N.NestedRun(loglike, 2, num_live=64, num_repeats=4, threads=16, seed=1, stream=s, clustering=True, max_iterations=6).run()
            for s in range(2)]
    for run in runs:
        run.vega, run.names = None, ['a', 'b']
    rec = [R.nested_record(run) for run in runs]
    assert not any('cluster' in key for r in rec for key in r)


def test_cluster_writer_round_trip(tmp_path):
    loglike = _two_mode_iso(3)
    run = N.NestedRun(loglike, 3, num_live=128, num_repeats=4, threads=32, seed=2, clustering=True, max_iterations=10).run()
    names = ['a', 'b', 'c']
    txt, pn, stats = N.write_run(run, tmp_path, 'run', names, cluster_posteriors=True)
    found = run.clusters()
    pts, lnl, w = run.samples()
    ids = run.cluster_ids()
    back = N.read_stats(stats)
    assert (back['log(Z)'], back['log(Z) error']) == run.log_evidence() and back['threads'] == 32
    assert len(found) >= 2
    for j, c in enumerate(found, start=1):
        table = np.loadtxt(tmp_path / f'run_cluster_{j}.txt', ndmin=2)
        keep = ids == c['id']
        assert table.shape == (keep.sum(), 5) and np.array_equal(table[:, 2:], pts[keep]) and np.array_equal(table[:, 1], -lnl[keep])
        if w[keep].max() > 0:
            assert table[:, 0].max() == 1.0
            np.testing.assert_allclose(table[:, 0] / table[:, 0].sum(), w[keep] / w[keep].sum(), rtol=1e-13, atol=0)
        assert back[f'log(Z_{j})'] == c['log_z'] or (np.isneginf(back[f'log(Z_{j})']) and np.isneginf(c['log_z']))
        assert back[f'mass_{j}'] == c['mass'] and back[f'id_{j}'] == c['id']
        assert (tmp_path / f'run_cluster_{j}.paramnames').read_text() == pn.read_text()
    assert not (tmp_path / f'run_cluster_{len(found) + 1}.txt').exists()
    # without cluster_posteriors the files are those of before, byte for byte, whether the run clustered or not
    (tmp_path / 'plain').mkdir()
    txt2, pn2, stats2 = N.write_run(run, tmp_path / 'plain', 'run', names)
    assert txt2.read_text() == txt.read_text() and pn2.read_text() == pn.read_text()
    assert stats2.read_text() == ''.join(ln + '\n' for ln in stats.read_text().splitlines()
                                         if not ln.startswith(('log(Z_', 'mass_', 'id_')))
    assert sorted(p.name for p in (tmp_path / 'plain').iterdir()) == ['run.paramnames', 'run.stats', 'run.txt']
    assert set(N.read_stats(stats2)) == {'log(Z)', 'log(Z) error', 'H', 'dead points', 'likelihood evaluations', 'iterations', 'seed',
                                         'num_live', 'num_repeats', 'threads'}


def test_cluster_struct_and_symbols_match_the_library():
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(17) == C.sizeof(engine.NestedClusters)
    for sym in ('vmx_nested_run_clustered', 'vmx_nested_cluster_points'):
        assert sym in engine.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert engine.VMX_NS_KNN == N.KNN and engine.VMX_NS_MAX_CLUSTERS == N.MAX_CLUSTERS and engine.VMX_NS_CLUSTER == 1
    header = (REPO / 'include' / 'vegamx.h').read_text()
    assert '#define VMX_NS_KNN 8' in header and '#define VMX_NS_MAX_CLUSTERS 8' in header
