"""``boost_posterior`` of the nested sampler without a GPU: the boost part of vega_amd/csrc/vmx_nested.h, compiled with g++ under
AddressSanitizer / UBSan into tests/helpers/nested_boost_driver.cpp, against the NumPy restatement of vega_amd/nested.py bit for
bit (the phantom record, the thinning word, the give-up step that yields nothing); ``boosted_weights`` against its definition in
O(N^2) loops; the boosted chain's statistics on the correlated Gaussian of tests/test_nested_host.py; independence of how a run is
cut; the ``[Nested]`` key, the writer, the struct."""
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
    exe = tmp_path_factory.mktemp('nested_boost') / 'nested_boost_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'nested_boost_driver.cpp')]
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


def _doubles(tokens):
    return np.array([struct.unpack('<d', struct.pack('<Q', int(t, 16)))[0] for t in tokens])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _gauss_loglike(n, sigma=0.15, centre=0.5):
    def loglike(u):
        d = (np.asarray(u) - centre) / sigma
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return -0.5 * acc
    return loglike


def _plateau_loglike(n):
    """Terraces around the centre: 1 within 0.12 of it, 0 within 0.6, negative steps outside.  L* is the wide terrace's 0, most
    threads start on it and find lnL > L* only on the small inner one: a slice whose line misses it shrinks MAX_SHRINK times."""
    def loglike(u):
        d = np.asarray(u) - 0.5
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return np.where(acc < 0.12**2, 1.0, np.where(acc < 0.6**2, 0.0, -np.floor(40.0 * acc)))
    return loglike


HEADER_CASES = [(1, 24, 8, 3, 'plain'), (2, 48, 16, 3, 'ties'), (6, 64, 24, 3, 'plain'), (32, 80, 16, 3, 'plain'),
                (2, 48, 16, 1, 'plain'), (2, 48, 16, 4, 'plateau')]


@pytest.mark.parametrize('f', [1.0, 0.3])
@pytest.mark.parametrize('n, nlive, K, num_repeats, case', HEADER_CASES)
def test_phantom_record_of_the_header_equals_the_restatement_bitwise(driver, n, nlive, K, num_repeats, case, f):
    """One whole iteration, the recorded answers replayed round by round through the header compiled by g++: every phantom point
    it reports (thread, repeat, kept, lnL, point; birth = L*) is what ``python_iterations(boost=...)`` recorded, in every bit; the
    dead record and the end points are those of the run without boost; ``num_repeats = 1`` records nothing; a slice step that
    gives up after MAX_SHRINK (the terraces) yields no phantom, and no tag repeats."""
    seed, stream, it = 11 + n, 3, 5
    live_u = N.draw_live(nlive, n, seed, stream)
    loglike = _plateau_loglike(n) if case == 'plateau' else _gauss_loglike(n)
    live_lnl = loglike(live_u)
    order = np.argsort(live_lnl, kind='stable')
    if case == 'ties':
        live_lnl[order[3]] = live_lnl[order[1]]
        live_lnl[order[K]] = live_lnl[order[K - 1]]
        live_lnl[order[0]] = -np.inf
    rounds = []

    def evaluate(rows):
        rounds.append(loglike(rows))
        return rounds[-1]

    state = N.PhantomState(f)
    lu, ll = live_u.copy(), live_lnl.copy()
    du, dl, dn, _, st = N.python_iterations(lu, ll, it, 1, K, num_repeats, seed, stream, evaluate, boost=state)
    rec = state.record(n)
    # the base run is the run without boost
    lu0, ll0 = live_u.copy(), live_lnl.copy()
    du0, dl0, dn0, _, st0 = N.python_iterations(lu0, ll0, it, 1, K, num_repeats, seed, stream, loglike)
    assert _same_bits(du, du0) and _same_bits(dl, dl0) and np.array_equal(dn, dn0) and st == st0
    assert _same_bits(lu, lu0) and _same_bits(ll, ll0)

    text = f'B {n} {nlive} {K} {num_repeats} {it} {seed:x} {stream:x} {_hx(f)} {_hexes(live_u)} {_hexes(live_lnl)} '
    text += ' '.join(f'{len(a)} {_hexes(a)}' for a in rounds)
    lines = [ln.split() for ln in _ask(driver, text)]
    killed = [int(t) for t in lines[0][1:]]
    lstar = _doubles(lines[1][1:])[0]
    assert _same_bits(_doubles(lines[2][1:]), dl) and _same_bits(live_u[killed], du)
    P = [ln for ln in lines if ln[0] == 'P']
    G = [(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == 'G']
    Eend = [ln for ln in lines if ln[0] == 'E']
    assert [int(t) for t in lines[-1][1:]] == [st['rounds'], st['rows']]
    assert _same_bits(np.array([_doubles(ln[2:3])[0] for ln in Eend]), ll[killed])
    assert _same_bits(np.concatenate([_doubles(ln[3:]) for ln in Eend]), lu[killed])
    # every phantom the header saw, and the ones it keeps
    tags = [(int(ln[1]), int(ln[2])) for ln in P]
    assert len(set(tags)) == len(tags) and all(1 <= r < num_repeats for _, r in tags)
    assert not set(tags) & set(G)
    if num_repeats == 1:
        assert not P and rec['lnl'].size == 0
    else:
        assert len(P) > (0 if case == 'plateau' else K // 2)
    if case == 'plateau':
        assert lstar == 0.0 and len(G) >= K, 'too few slice steps gave up: the case does not reach MAX_SHRINK'
        assert len(tags) + len([g for g in G if g[1] < num_repeats]) == K * (num_repeats - 1)
    elif not G:
        assert len(tags) == K * (num_repeats - 1)
    kept = sorted((int(ln[1]), int(ln[2]), i) for i, ln in enumerate(P) if int(ln[3]) == 1)
    if f == 1.0:
        assert len(kept) == len(P)
    assert [(k, r) for k, r, _ in kept] == [(int(k), int(r)) for _, k, r in rec['tag']]
    assert np.all(rec['tag'][:, 0] == it)
    if kept:
        assert _same_bits(np.array([_doubles(P[i][4:5])[0] for _, _, i in kept]), rec['lnl'])
        assert _same_bits(np.concatenate([_doubles(P[i][5:]) for _, _, i in kept]), rec['u'])
        assert _same_bits(rec['birth'], np.full(len(kept), lstar)) and np.all(rec['lnl'] > rec['birth'])
    ks, rs = np.array([k for k, _ in tags], dtype=np.int64), np.array([r for _, r in tags], dtype=np.int64)
    if tags:
        assert np.array_equal(N.phantom_kept(ks, it, rs, f, seed, stream), np.array([int(ln[3]) == 1 for ln in P]))


# ------------------------------------------------------------------ the thinning counter
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


def test_the_thinning_word_is_the_documented_counter(driver):
    """(k, t, r) is kept iff u01(word 0 of the Philox block with counter (k, t, r, 3)) < f - against NumPy's Philox (which
    increments before it encrypts), against ``_blocks``, and against the header; the kept mask of a run is that word's, however
    the run is cut into calls."""
    seed, stream, f = 9, 2, 0.3
    ks, ts, rs = np.array([0, 1, 5, 63, 4000]), [0, 17, 17, 2, 123456], np.array([1, 2, 3, 29, 159])
    text = []
    for k, t, r in zip(ks, ts, rs):
        c = int(k) | (t << 64) | (int(r) << 128) | (3 << 192)
        w0 = np.random.Philox(key=[seed, stream], counter=c - 1).random_raw(4)[0]
        assert N._blocks(np.array([k]), t, np.array([r]), 3, seed, stream)[0, 0] == w0
        assert bool(N.phantom_kept(np.array([k]), t, np.array([r]), f, seed, stream)[0]) == bool(E.u01(np.array([w0]))[0] < f)
        text.append(f'Q {k} {t} {r} {_hx(f)} {seed:x} {stream:x}')
    got = _ask(driver, ' '.join(text))
    assert [g.split()[1] for g in got] == [str(int(N.phantom_kept(np.array([k]), t, np.array([r]), f, seed, stream)[0]))
                                           for k, t, r in zip(ks, ts, rs)]
    loglike, _, _ = _correlated_gaussian(3)
    kw = dict(num_live=96, num_repeats=6, threads=24, seed=4, stream=1)
    full = N.NestedRun(loglike, 3, boost_posterior=6, **kw).run(iterations=5).phantoms()
    thin = N.NestedRun(loglike, 3, boost_posterior=6 * f, **kw).run(iterations=5).phantoms()
    cut = N.NestedRun(loglike, 3, boost_posterior=6 * f, **kw)
    cut.run(iterations=2)
    cut.run(iterations=3)
    assert full['lnl'].size == 5 * 24 * 5                   # (no step of this run gives up: every inner point is there)
    words = N._blocks(full['tag'][:, 1], 0, full['tag'][:, 2], 3, 4, 1)
    for t in range(5):
        sel = full['tag'][:, 0] == t
        words[sel] = N._blocks(full['tag'][sel, 1], t, full['tag'][sel, 2], 3, 4, 1)
    mask = E.u01(words[:, 0]) < f
    assert 0 < mask.sum() < mask.size
    for got_rec in (thin, cut.phantoms()):
        assert np.array_equal(got_rec['tag'], full['tag'][mask])
        assert _same_bits(got_rec['u'], full['u'][mask]) and _same_bits(got_rec['lnl'], full['lnl'][mask])
        assert _same_bits(got_rec['birth'], full['birth'][mask])


# ------------------------------------------------------------------ the weights
def _brute_force_weights(dead_lnl, dead_nlive, live_lnl, ph_lnl, ph_birth):
    """The definition of ``boosted_weights`` in loops."""
    D, nl, P = len(dead_lnl), len(live_lnl), len(ph_lnl)
    l_d = dead_lnl[-1]
    events = [(dead_lnl[i], 0, i) for i in range(D)] + [(ph_lnl[p], 1, p) for p in range(P) if ph_lnl[p] <= l_d]
    events.sort()
    log_x, lw, index = 0.0, [], []
    for x, is_ph, i in events:
        if is_ph:
            b = None
            for j in range(D):
                if dead_lnl[j] >= x:
                    b = dead_nlive[j]
                    break
        else:
            b = dead_nlive[i]
        a = 0
        for p in range(P):
            if ph_birth[p] < x <= ph_lnl[p]:
                a += 1
        m = float(b + a)
        lw.append(x + log_x + math.log1p(-math.exp(-1.0 / m)))
        log_x -= 1.0 / m
        index.append(D + nl + i if is_ph else i)
    late = [p for p in range(P) if ph_lnl[p] > l_d]
    for i in range(nl):
        lw.append(live_lnl[i] + log_x - math.log(nl + len(late)))
        index.append(D + i)
    for p in late:
        lw.append(ph_lnl[p] + log_x - math.log(nl + len(late)))
        index.append(D + nl + p)
    return np.array(lw), np.array(index)


@pytest.mark.parametrize('seed', range(6))
def test_boosted_weights_against_the_definition(seed):
    """Random records with ties between deaths, phantoms tied with a death, phantoms above the last death and a failed model:
    1e-13 in every log weight; the weights sum to 1 under log Z_boost; the index map is a permutation; without phantoms the
    function is ``log_weights`` to 1e-14."""
    rng = np.random.default_rng(seed)
    nlive, K, iters = 12, 4, 9
    levels = np.sort(rng.normal(size=iters * K) * 3.0)
    levels[5] = levels[4]                                   # two deaths tie
    levels[17] = levels[16]
    if seed % 2:
        levels[0] = -np.inf
    dead_lnl = levels
    dead_nlive = np.tile(nlive - np.arange(K), iters)
    live_lnl = dead_lnl[-1] + rng.random(nlive) * 2.0
    lstars = dead_lnl[K - 1::K]
    P = 70
    ph_birth = lstars[rng.integers(0, iters, size=P)]
    ph_lnl = ph_birth + rng.random(P) * 4.0
    ph_lnl[np.isneginf(ph_birth)] = rng.normal(size=int(np.isneginf(ph_birth).sum()))
    for p, i in ((3, 20), (9, 21), (11, 35)):             # phantoms tied with a death above their birth (35: the last death)
        if dead_lnl[i] > ph_birth[p]:
            ph_lnl[p] = dead_lnl[i]
    assert np.all(ph_lnl > ph_birth) and np.any(ph_lnl > dead_lnl[-1]) and np.any(np.isin(ph_lnl, dead_lnl))
    lw, index, log_z = N.boosted_weights(dead_lnl, dead_nlive, live_lnl, ph_lnl, ph_birth)
    want, want_index = _brute_force_weights(dead_lnl, dead_nlive, live_lnl, ph_lnl, ph_birth)
    assert np.array_equal(index, want_index)
    assert np.array_equal(np.sort(index), np.arange(dead_lnl.size + nlive + P))
    finite = np.isfinite(want)
    assert np.array_equal(finite, np.isfinite(lw)) and np.all(np.abs(lw[finite] - want[finite]) <= 1e-13)
    assert abs(np.sum(np.exp(lw - log_z)) - 1.0) < 1e-12 and log_z == N._logsumexp(lw)
    # the events are in order, and a death comes before a phantom of the same lnL
    both = np.concatenate([dead_lnl, live_lnl, ph_lnl])[index]
    n_ev = dead_lnl.size + int(np.sum(ph_lnl <= dead_lnl[-1]))
    assert np.all(np.diff(both[:n_ev]) >= 0)
    for j in range(n_ev - 1):
        if both[j] == both[j + 1]:
            assert not (index[j] >= dead_lnl.size and index[j + 1] < dead_lnl.size)
    none, idx0, z0 = N.boosted_weights(dead_lnl, dead_nlive, live_lnl, np.empty(0), np.empty(0))
    base = N.log_weights(dead_lnl, dead_nlive, live_lnl)
    fin = np.isfinite(base)
    assert np.array_equal(idx0, np.arange(base.size)) and np.all(np.abs(none[fin] - base[fin]) <= 1e-14)
    assert np.array_equal(np.isfinite(none), fin) and abs(z0 - N._logsumexp(base)) <= 1e-14


# ------------------------------------------------------------------ statistics
BOOST_CASES = [(2, 256, 64, s) for s in range(5)] + [(4, 512, 128, s) for s in range(3)]


@pytest.mark.parametrize('f', [1.0, 0.2])
@pytest.mark.parametrize('n, nlive, K, seed', BOOST_CASES)
def test_the_boosted_chain_of_a_correlated_gaussian(n, nlive, K, seed, f):
    """The correlated Gaussian of tests/test_nested_host.py (sigma = 0.03 per axis), the fraction f of the inner points kept: every
    phantom has lnL > birth; the kept share is within 0.02 of f; the boosted chain's weighted mean within 5 sigma / sqrt(ESS) and
    every coordinate's weighted variance over the true one within 5 sqrt(2 / ESS) of 1, both with the ESS of the unboosted chain
    (the boosted chain may not be worse than the bar the base chain gets); |log Z_boost - true| <= 4 err; the Kish sample size
    1 / sum p^2 at least 3 times the base chain's at f = 1, 2 times at f = 0.2.  The reported evidence is the base run's."""
    loglike, cov, log_z_true = _correlated_gaussian(n)
    num_repeats = 5 * n
    run = N.NestedRun(loglike, n, num_live=nlive, num_repeats=num_repeats, threads=K, seed=seed, boost_posterior=f * num_repeats).run()
    assert run.terminated and run.phantom_state.fraction == f
    ph = run.phantoms()
    share = ph['lnl'].size / (run.iteration * K * (num_repeats - 1))
    pts, lnl, w = run.samples()
    base_pts, base_lnl, base_w = run.samples(boost=False)
    ess, ess_base = 1.0 / np.sum(w**2), 1.0 / np.sum(base_w**2)
    mean = w @ pts
    pull = (mean - 0.5) / (0.03 / np.sqrt(ess_base))
    ratio = (w @ (pts - mean)**2) / np.diag(cov)
    log_z, err = run.log_evidence()
    log_z_boost = run.boost_log_evidence()
    base_mean = base_w @ base_pts
    print(f'n {n} seed {seed} f {f}: kept {ph["lnl"].size} (share {share:.4f}), sample size {ess:.0f} / base {ess_base:.0f} = '
          f'{ess / ess_base:.2f}, mean pulls {np.round(pull, 2)}, variance ratios {np.round(ratio, 3)} '
          f'(allowed +-{5 * math.sqrt(2 / ess_base):.3f}), log Z_boost - true {(log_z_boost - log_z_true) / err:+.2f} err, '
          f'log Z - true {(log_z - log_z_true) / err:+.2f} err, base pulls '
          f'{np.round((base_mean - 0.5) / (0.03 / np.sqrt(ess_base)), 2)}')
    assert np.all(ph['lnl'] > ph['birth'])
    assert abs(share - f) <= 0.02
    assert pts.shape == (base_w.size + ph['lnl'].size, n) and abs(w.sum() - 1) < 1e-12 and lnl.shape == w.shape
    assert np.all(np.abs(pull) <= 5), pull
    assert np.all(np.abs(ratio - 1.0) <= 5 * math.sqrt(2 / ess_base)), ratio
    assert abs(log_z_boost - log_z_true) <= 4 * err
    assert ess >= (3.0 if f == 1.0 else 2.0) * ess_base
    # the reported evidence and the base chain are those of the run without boost
    assert log_z == N.evidence(*run.dead()[1:], run.live_lnl)[0]
    assert base_lnl.size == run.dead()[1].size + nlive


# ------------------------------------------------------------------ the cut, the constructor
def test_the_boosted_run_does_not_depend_on_the_cut():
    loglike, _, _ = _correlated_gaussian(3)
    kw = dict(num_live=96, num_repeats=6, threads=24, seed=4, boost_posterior=2.0)
    one = N.NestedRun(loglike, 3, **kw).run(iterations=4)
    cut = N.NestedRun(loglike, 3, **kw)
    cut.run(iterations=2)
    cut.run(iterations=2)
    off = N.NestedRun(loglike, 3, **dict(kw, boost_posterior=0.0)).run(iterations=4)
    assert one.iteration == cut.iteration == 4 and cut.stats['calls'] == 2
    a, b = one.phantoms(), cut.phantoms()
    assert a['lnl'].size > 0 and np.array_equal(a['tag'], b['tag']) and a['cluster'] is None
    for key in ('u', 'lnl', 'birth'):
        assert _same_bits(a[key], b[key])
    order = np.lexsort((a['tag'][:, 2], a['tag'][:, 1], a['tag'][:, 0]))
    assert np.array_equal(order, np.arange(order.size))                 # (the canonical order)
    for x, y, z in zip(one.dead(), cut.dead(), off.dead()):
        assert _same_bits(x, y) and _same_bits(x, z)
    assert _same_bits(one.live_u, off.live_u) and _same_bits(one.live_lnl, off.live_lnl) and one.stats['rows'] == off.stats['rows']
    for x, y in zip(one.samples(), cut.samples()):
        assert _same_bits(x, y)
    assert one.boost_log_evidence() == cut.boost_log_evidence() and one.log_evidence() == off.log_evidence()
    # with nothing kept the chain is the unboosted one
    for x, y in zip(one.samples(boost=False), off.samples()):
        assert _same_bits(x, y)
    with pytest.raises(ValueError, match='boost_posterior'):
        off.phantoms()
    for x, y in zip(off.samples(boost=None), off.samples(boost=False)):
        assert _same_bits(x, y)


def test_boost_with_clustering_and_the_refusals():
    """A clustered run records the id every phantom's thread hands its end point; the whole-run chain is boosted, a cluster's is
    not; the constructor refuses what is no boost; a call's phantom record stays under the stated budget."""
    def loglike(u):
        u = np.asarray(u)
        return np.logaddexp(-0.5 * np.sum((u - 0.3)**2, axis=1) / 0.02**2, -0.5 * np.sum((u - 0.7)**2, axis=1) / 0.02**2)

    run = N.NestedRun(loglike, 2, num_live=128, num_repeats=4, threads=32, seed=2, clustering=True, boost_posterior=4,
                      max_iterations=12).run()
    ph = run.phantoms()
    assert ph['cluster'].dtype == np.int32 and ph['cluster'].shape == ph['lnl'].shape and np.all(ph['cluster'] >= 1)
    assert set(np.unique(ph['cluster'])) <= set(np.unique(run.cluster_ids()))
    assert run.samples()[0].shape[0] == run.cluster_ids().size + ph['lnl'].size
    j = run.clusters()[0]['id']
    assert run.samples(cluster=j)[0].shape[0] == int(np.sum(run.cluster_ids() == j))
    with pytest.raises(ValueError, match='not boosted'):
        run.samples(cluster=j, boost=True)
    f = _gauss_loglike(3)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match='boost_posterior'):
            N.NestedRun(f, 3, boost_posterior=bad)
    assert N.NestedRun(f, 3).phantom_state is None and N.NestedRun(f, 3, boost_posterior=0).phantom_state is None
    assert N.NestedRun(f, 3, num_repeats=10, boost_posterior=2.5).phantom_state.fraction == 0.25
    assert N.NestedRun(f, 3, num_repeats=10, boost_posterior=50).phantom_state.fraction == 1.0       # (not above num_repeats)
    # 32 parameters with the defaults (800 live points, 384 threads, 160 repeats): 18 MB of record an iteration, 11 a call
    big = N.NestedRun(_gauss_loglike(32), 32, max_batch=4096, boost_posterior=1.0)
    assert (big.num_live, big.threads, big.num_repeats) == (800, 384, 160) and big._per_call() == 11
    assert big._per_call() * 384 * 159 * N.phantom_row_bytes(32) <= N.PHANTOM_BUDGET == 200_000_000
    assert N.NestedRun(_gauss_loglike(32), 32, max_batch=4096)._per_call() == 65536 // 384


# ------------------------------------------------------------------ config and files
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Nested\n'
MC = '[monte carlo]\nnum_mocks = 4\n'


def test_boost_posterior_setting(tmp_path):
    plain = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\n'), SAMPLE)
    assert 'boost_posterior' not in plain
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\nboost_posterior = 2.5\n'), SAMPLE)
    assert s['boost_posterior'] == 2.5 and {k: v for k, v in s.items() if k != 'boost_posterior'} == plain
    assert E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\nboost_posterior = 0\n'), SAMPLE)['boost_posterior'] == 0.0
    # off, it combines with everything
    assert E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\nboost_posterior = 0.0\nreplicas = 3\n'),
                              SAMPLE)['replicas'] == 3
    assert E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\nboost_posterior = 1\nreplicas = 1\n'),
                              SAMPLE)['boost_posterior'] == 1.0
    s = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\nboost_posterior = 3\ncluster_posteriors = True\n'), SAMPLE)
    assert s['boost_posterior'] == 3.0 and s['do_clustering'] is True


@pytest.mark.parametrize('text, match', [
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = -1\n', 'boost_posterior'),
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = nan\n', 'boost_posterior'),
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = inf\n', 'boost_posterior'),
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = much\n', 'boost_posterior'),
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = 2\nreplicas = 2\n', 'boost_posterior does not combine.*out of scope'),
    (HEAD + '[Nested]\npath = {p}\nboost_posterior = 2\nreplicas = 2\ntogether = True\n', 'boost_posterior does not combine'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Nested]\npath = {p}\nboost_posterior = 2\nmocks = 3\n',
     'boost_posterior does not combine'),
])
def test_boost_posterior_setting_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), SAMPLE)


def test_writer_round_trip_with_boost(tmp_path):
    loglike, _, _ = _correlated_gaussian(3)
    kw = dict(num_live=64, num_repeats=6, threads=16, seed=1, max_iterations=12)
    run = N.NestedRun(loglike, 3, boost_posterior=3.0, **kw).run()
    names = ['a', 'b', 'c']
    txt, pn, stats = N.write_run(run, tmp_path, 'run', names)
    table = np.loadtxt(txt)
    pts, lnl, w = run.samples()
    n_ph = run.phantoms()['lnl'].size
    assert n_ph > 0 and table.shape == (12 * 16 + 64 + n_ph, 5)
    assert np.array_equal(table[:, 0], w / w.max()) and np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    back = N.read_stats(stats)
    assert back['phantom points'] == n_ph and isinstance(back['phantom points'], int)
    assert back['log(Z) boosted'] == run.boost_log_evidence()
    assert (back['log(Z)'], back['log(Z) error']) == run.log_evidence() and back['dead points'] == 12 * 16
    eq, eq_lnl = run.equal_weighted(np.random.default_rng(0))
    assert 0 < eq.shape[0] <= pts.shape[0] and eq_lnl.shape == (eq.shape[0],)
    # off: the files of a run built without the argument, byte for byte
    for sub, extra in (('zero', dict(boost_posterior=0.0)), ('absent', {})):
        (tmp_path / sub).mkdir()
        N.write_run(N.NestedRun(loglike, 3, **kw, **extra).run(), tmp_path / sub, 'run', names)
    for ext in ('txt', 'paramnames', 'stats'):
        assert (tmp_path / 'zero' / f'run.{ext}').read_bytes() == (tmp_path / 'absent' / f'run.{ext}').read_bytes()
    off = N.read_stats(tmp_path / 'zero' / 'run.stats')
    assert 'phantom points' not in off and 'log(Z) boosted' not in off and off['log(Z)'] == back['log(Z)']
    assert np.loadtxt(tmp_path / 'zero' / 'run.txt').shape == (12 * 16 + 64, 5)


def test_phantoms_struct_and_symbol():
    """vmx_struct_size(19) is the ctypes struct's; the library exports vmx_nested_run_phantoms."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(19) == C.sizeof(engine.NestedPhantoms) == 88
    assert 'vmx_nested_run_phantoms' in engine.EXPORTED_SYMBOLS
    assert hasattr(lib, 'vmx_nested_run_phantoms')
