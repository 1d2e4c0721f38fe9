"""boost_posterior in a set of nested-sampling runs, without a GPU: every run of ``python_iterations_many(boost=...)`` keeps the
phantom record ``python_iterations(boost=...)`` keeps on its stream, bit for bit, whole or cut into calls; the header's set rule
(vega_amd/csrc/vmx_nested.h "a set of runs": boost - the capacity and the place of a run's record), compiled with g++ under
AddressSanitizer / UBSan into tests/helpers/nested_set_boost_driver.cpp, against that restatement; ``merge_nested_boosted`` against
its definition in loops; the boosted merge of three replicas of a Gaussian; ``sample_mocks_nested`` with its table on the python
driver over a stand-in interface; what ``NestedSet`` and ``NestedRunSet`` refuse."""
import math
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vega_amd import nested as N
from vega_amd import replicas as rep

REPO = Path(__file__).resolve().parents[1]


def _correlated_gaussian(n, sigma=0.03):
    a = np.random.RandomState(1).randn(n, n)
    s = a @ a.T
    d = np.sqrt(np.diag(s))
    cov = s / np.outer(d, d) * sigma**2
    prec = np.linalg.inv(cov)

    def loglike(u, runs=None):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ri,ij,rj->r', d, prec, d)

    return loglike, cov, 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]


def _gauss(n, sigma=0.15, centre=0.5):
    def loglike(u, runs=None):
        d = (np.asarray(u) - centre) / sigma
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return -0.5 * acc
    return loglike


def _terraces(n):
    """lnL in whole steps: live points tie, and a trial on the contour's own terrace is not above L*."""
    smooth = _gauss(n)

    def loglike(u, runs=None):
        return np.floor(smooth(u))
    return loglike


def _same_record(a, b):
    for key in ('u', 'lnl', 'birth', 'tag'):
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
        assert np.array_equal(a[key], b[key]), key
    assert a['cluster'] is None and b['cluster'] is None


def _single(n, nlive, K, num_repeats, seed, stream, like, iterations, f, stop_after=None):
    """``python_iterations(boost=...)`` on ``stream`` from the draw: (live_u, live_lnl, dead, PhantomState)."""
    u = N.draw_live(nlive, n, seed, stream)
    lnl = like(u)
    state = N.PhantomState(f)
    stop = None if stop_after is None else (lambda it, dead_lnl, live_lnl: it >= stop_after)
    du, dl, dn, it, _ = N.python_iterations(u, lnl, 0, iterations, K, num_repeats, seed, stream, like, stop, boost=state)
    return u, lnl, (du, dl, dn), state


# ------------------------------------------------------------------ the set is its single runs, phantoms included
@pytest.mark.parametrize('f', [1.0, 0.3])
@pytest.mark.parametrize('n', [2, 6])
def test_every_run_keeps_the_phantoms_of_the_single_run(n, f):
    """E = 3 x (nlive 40, K 12), 4 repeats; run e stops after 2 + e iterations, so the runs leave the set one by one while the
    others go on recording."""
    like = _correlated_gaussian(n, sigma=0.1)[0]
    nlive, K, R, seed, streams = 40, 12, 4, 7, [4, 0, 2]
    u, lnl, it = np.zeros((3, nlive, n)), np.zeros((3, nlive)), np.zeros(3, dtype=np.int64)
    states = [N.PhantomState(f) for _ in streams]
    dead, status, done, st = N.python_iterations_many(u, lnl, it, 10, K, R, seed, streams, lambda rows, runs: like(rows),
                                                      lambda e, i, d, l: i >= 2 + e, draw=True, boost=states)
    assert list(done) == [2, 3, 4] and list(status) == [1, 1, 1]
    plain_u, plain_lnl, plain_it = np.zeros((3, nlive, n)), np.zeros((3, nlive)), np.zeros(3, dtype=np.int64)
    plain = N.python_iterations_many(plain_u, plain_lnl, plain_it, 10, K, R, seed, streams, lambda rows, runs: like(rows),
                                     lambda e, i, d, l: i >= 2 + e, draw=True)
    assert np.array_equal(plain_u, u) and np.array_equal(plain_lnl, lnl)             # (the set is the same set with or without)
    assert plain[3]['rows'] == st['rows'] and plain[3]['rounds'] == st['rounds'] and np.array_equal(plain[3]['per_run'], st['per_run'])
    kept = []
    for e, stream in enumerate(streams):
        su, sl, sdead, want = _single(n, nlive, K, R, seed, stream, like, 10, f, stop_after=2 + e)
        assert np.array_equal(u[e], su) and np.array_equal(lnl[e], sl)
        assert all(np.array_equal(a, b) for a, b in zip(dead[e], sdead)) and all(np.array_equal(a, b) for a, b in zip(plain[0][e], sdead))
        _same_record(states[e].record(n), want.record(n))
        got = states[e].record(n)
        kept.append(got['lnl'].size)
        assert np.all(got['lnl'] > got['birth']) and got['tag'][:, 0].max() == 1 + e and got['tag'][:, 2].max() <= R - 1
        assert len(states[e].calls) == 1
    assert all(k > 0 for k in kept)
    if f == 1.0:        # (every accepted inner point: at most K (R - 1) per iteration, fewer only where a slice step gave up)
        assert all(k <= (2 + e) * K * (R - 1) for e, k in enumerate(kept)) and kept[2] > 0.9 * 4 * K * (R - 1)


@pytest.mark.parametrize('f', [1.0, 0.3])
def test_a_boosted_set_cut_into_calls_is_the_same_set(f):
    n, nlive, K, R, seed, streams = 2, 40, 12, 4, 7, [4, 0, 2]
    like = _correlated_gaussian(n, sigma=0.1)[0]
    u, lnl, it = np.zeros((3, nlive, n)), np.zeros((3, nlive)), np.zeros(3, dtype=np.int64)
    states = [N.PhantomState(f) for _ in streams]
    for call in range(2):
        _, status, done, _ = N.python_iterations_many(u, lnl, it, 3, K, R, seed, streams, lambda rows, runs: like(rows),
                                                      draw=call == 0, boost=states)
        assert list(done) == [3, 3, 3] and list(status) == [0, 0, 0]
    for e, stream in enumerate(streams):
        su, sl, _, want = _single(n, nlive, K, R, seed, stream, like, 6, f)
        assert np.array_equal(u[e], su) and np.array_equal(lnl[e], sl) and len(states[e].calls) == 2
        _same_record(states[e].record(n), want.record(n))
    # the classes: run(3).run(3) is run(6), and every run is the NestedRun on its stream
    a = N.NestedRunSet(like, n, 3, num_live=nlive, threads=K, num_repeats=R, seed=seed, streams=streams, boost_posterior=f * R).run(3).run(3)
    b = N.NestedRunSet(like, n, 3, num_live=nlive, threads=K, num_repeats=R, seed=seed, streams=streams, boost_posterior=f * R).run(6)
    assert a.stats['calls'] == 2 and b.stats['calls'] == 1 and a.boost_posterior == f * R
    for e, stream in enumerate(streams):
        _same_record(a.phantoms(e), b.phantoms(e))
        _same_record(a.phantoms(e), states[e].record(n))
        one = N.NestedRun(lambda rows: like(rows), n, num_live=nlive, threads=K, num_repeats=R, seed=seed, stream=stream,
                          boost_posterior=f * R).run(6)
        _same_record(one.phantoms(), b.phantoms(e))
        for x, y in zip(one.samples(), b.samples()[e]):
            assert np.array_equal(x, y)
        for x, y in zip(one.samples(boost=False), b.samples(boost=False)[e]):
            assert np.array_equal(x, y)
        assert one.boost_log_evidence() == b.boost_log_evidence()[e] and np.array_equal(one.boost_index(), b.boost_index()[e])
        assert one.log_evidence() == (b.log_evidence()[0][e], b.log_evidence()[1][e])
    assert b.samples()[0][0].shape[0] == 6 * K + nlive + b.phantoms(0)['lnl'].size


def test_one_repeat_keeps_nothing():
    like = _gauss(2)
    u, lnl, it = np.zeros((2, 20, 2)), np.zeros((2, 20)), np.zeros(2, dtype=np.int64)
    states = [N.PhantomState(1.0), N.PhantomState(1.0)]
    N.python_iterations_many(u, lnl, it, 3, 6, 1, 7, [0, 1], lambda rows, runs: like(rows), draw=True, boost=states)
    for state in states:
        rec = state.record(2)
        assert rec['u'].shape == (0, 2) and rec['lnl'].shape == (0,) and rec['tag'].shape == (0, 3) and len(state.calls) == 1
    runs = N.NestedRunSet(like, 2, 2, num_live=20, threads=6, num_repeats=1, boost_posterior=1.0).run(2)
    assert runs.phantoms(1)['lnl'].size == 0 and runs.samples()[1][0].shape == (2 * 6 + 20, 2)
    with pytest.raises(ValueError, match='one PhantomState for each'):
        N.python_iterations_many(u, lnl, it, 1, 6, 1, 7, [0, 1], lambda rows, runs: like(rows), boost=states[:1])


# ------------------------------------------------------------------ header <-> NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('nested_set_boost') / 'nested_set_boost_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'nested_set_boost_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _hx(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0].to_bytes(8, 'big').hex()


def _hexes(a):
    return ' '.join(_hx(v) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _doubles(tokens):
    return np.array([struct.unpack('<d', struct.pack('<Q', int(t, 16)))[0] for t in tokens])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


HEADER_CASES = [(1, 12, 4, 3, 'plain'), (2, 16, 4, 3, 'ties'), (6, 20, 5, 4, 'plain'), (32, 40, 5, 3, 'plain')]


@pytest.mark.parametrize('n, nlive, K, num_repeats, case', HEADER_CASES)
def test_header_places_every_runs_phantoms_as_the_restatement(driver, n, nlive, K, num_repeats, case):
    """E = 3, f = 0.5, the stop rule ends the runs after 2, 4 and 3 iterations: run 0 is OUT while the others record.  The
    restatement's answers are replayed round by round through the header; per run every phantom point the header sees is one of
    the restatement's at f = 1 (point, lnL and tags bit for bit), its kept flag says whether the restatement at f = 0.5 has it,
    the kept ones lie in the run's own part of the record in the order they were accepted, and the record read back - points, lnL,
    birth, tags, counts - is the restatement's bit for bit."""
    E_, seed, f = 3, 11, 0.5
    streams, stop_at = [6, 0, 3], [2, 4, 3]
    like = _terraces(n) if case == 'ties' else _gauss(n)
    u0 = np.stack([N.draw_live(nlive, n, seed, s) for s in streams])
    lnl0 = np.stack([like(u) for u in u0])
    if case == 'ties':
        assert all(np.unique(l).size < l.size for l in lnl0)
    answers = []

    def watch(r, state):
        if state['total'] == 0:
            answers.append(np.empty(0))

    def evaluate(rows, runs):
        out = like(rows)
        answers.append(out)
        return out

    records = {}
    for frac in (f, 1.0):
        u, lnl, it = u0.copy(), lnl0.copy(), np.zeros(E_, dtype=np.int64)
        states = [N.PhantomState(frac) for _ in streams]
        answers.clear()
        dead, status, done, st = N.python_iterations_many(u, lnl, it, 10, K, num_repeats, seed, streams, evaluate,
                                                          stop=lambda e, i, d, l: i >= stop_at[e], watch=watch, boost=states)
        assert list(done) == stop_at and len(answers) == st['rounds']
        records[frac] = [s.record(n) for s in states]
    text = f'S {E_} {n} {nlive} {K} {num_repeats} 10 {seed:x} {_hx(f)} ' + ' '.join(f'{s:x}' for s in streams) + ' 0 0 0 '
    text += ' '.join(str(s) for s in stop_at) + f' {_hexes(u0)} {_hexes(lnl0)} '
    text += ' '.join(f'{len(a)} {_hexes(a)}' for a in answers)
    out = subprocess.run([str(driver)], input=text + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert not any(ln[0] == 'ERR' for ln in lines)
    capacity = 10 * K * (num_repeats - 1)
    seen = {e: [] for e in range(E_)}
    placed = {e: [] for e in range(E_)}
    for ln in (ln for ln in lines if ln[0] == 'P'):
        e, it_, k, r, kept, row = (int(v) for v in ln[1:7])
        seen[e].append(((it_, k, r), kept, _doubles(ln[7:])))
        if kept:
            placed[e].append(row)
        else:
            assert row == -1
    counts = [int(v) for v in next(ln for ln in lines if ln[0] == 'C')[2:]]
    back = {e: [] for e in range(E_)}
    for ln in (ln for ln in lines if ln[0] == 'U'):
        back[int(ln[1])].append((tuple(int(v) for v in ln[2:5]), _doubles(ln[5:])))
    for e in range(E_):
        full, want = records[1.0][e], records[f][e]
        # every phantom the header saw: the restatement's at f = 1, and the kept flag is the restatement's at f
        tags = sorted(t for t, _, _ in seen[e])
        assert tags == [tuple(int(v) for v in t) for t in full['tag']] and len(set(tags)) == len(tags)
        by_tag = {tuple(int(v) for v in t): i for i, t in enumerate(full['tag'])}
        kept_tags = {tuple(int(v) for v in t) for t in want['tag']}
        for tag, kept, vals in seen[e]:
            i = by_tag[tag]
            assert _same_bits(vals, np.concatenate([[full['lnl'][i]], full['u'][i]])) and bool(kept) == (tag in kept_tags), (e, tag)
        # the places: the run's own part of the record, one after the other in the order of acceptance
        assert placed[e] == list(range(e * capacity, e * capacity + counts[e])) and counts[e] == want['lnl'].size <= capacity
        # the record read back, put into the canonical order
        order = sorted(range(len(back[e])), key=lambda j: back[e][j][0])
        assert [back[e][j][0] for j in order] == [tuple(int(v) for v in t) for t in want['tag']]
        got = np.array([back[e][j][1] for j in order]).reshape(-1, n + 2)
        assert _same_bits(got[:, 0], want['lnl']) and _same_bits(got[:, 1], want['birth']) and _same_bits(got[:, 2:], want['u'])
        assert 0 < counts[e] < full['lnl'].size
    # run 0 left the set first and wrote nothing after its second iteration, while the others went on
    assert records[f][0]['tag'][:, 0].max() == 1 and records[f][1]['tag'][:, 0].max() == 3
    assert next(ln for ln in lines if ln[0] == 'Z') == ['Z', '3', '1', '1', '1']
    assert next(ln for ln in lines if ln[0] == 'D') == ['D', '3', '2', '4', '3']


# ------------------------------------------------------------------ the boosted merge
def _random_records(seed, with_phantoms=(True, False, True)):
    """Records of runs of different shapes with what the merge has to cope with: deaths of different replicas that tie, a
    phantom tied with a death, phantoms above every run's last death, a record without phantoms among records with them."""
    rng = np.random.default_rng(seed)
    shared = np.round(rng.normal(size=4), 3)                # levels that occur in several replicas
    out = []
    for r, has in enumerate(with_phantoms):
        nlive, K, iters = (10, 3, 6) if r != 1 else (7, 2, 5)
        dead = np.sort(np.round(rng.normal(size=iters * K) * 2.0, 3))
        dead[[2, 7]] = np.sort(shared[:2])[[0, 1]] if dead.size > 7 else dead[[2, 7]]
        dead = np.sort(dead)
        live = dead[-1] + np.round(rng.random(nlive) * 2.0 + 0.001, 3)
        live[1] = live[0]                                   # two final live points tie
        if r == 2 and out[0]['live_lnl'][2] > dead[-1]:
            live[3] = out[0]['live_lnl'][2]                 # ... and one ties with a live point of replica 0
        rec = dict(kind='nested', dead_lnl=dead, dead_nlive=np.tile(nlive - np.arange(K), iters), live_lnl=live,
                   points=rng.random((dead.size + nlive, 2)))
        if has:
            P = 25
            lstars = dead[K - 1::K]
            birth = lstars[rng.integers(0, iters, size=P)]
            lnl = birth + np.round(rng.random(P) * 5.0 + 0.001, 3)
            lnl[0] = 50.0 + r                               # above every run's last death
            lnl[1] = 50.0                                   # ... where phantoms of one replica and of different ones tie
            if dead[-1] > birth[2]:
                lnl[2] = dead[-1]                           # tied with a death of its own run
            if shared[0] > birth[3]:
                lnl[3] = shared[0]                          # tied with deaths of several runs
            rec.update(ph_lnl=lnl, ph_birth=birth, ph_u=rng.random((P, 2)), ph_points=rng.random((P, 2)))
        out.append(rec)
    return out


def _merge_by_definition(records):
    """``merge_nested_boosted`` as O(N^2) loops: (lnL, is-phantom, replica, index, live count m, log X, log w + lnL)."""
    seqs = [rep.death_sequence(r) for r in records]
    events = []
    for r, (l, c, idx) in enumerate(seqs):
        events += [(float(l[j]), 0, r, j, int(idx[j])) for j in range(l.size)]
    for r, rec in enumerate(records):
        if 'ph_lnl' in rec:
            events += [(float(v), 1, r, p, p) for p, v in enumerate(rec['ph_lnl'])]
    events.sort(key=lambda ev: ev[:4])
    rows, log_x = [], 0.0
    for level, is_ph, r, j, index in events:
        m = 0
        for q, (l, c, _) in enumerate(seqs):
            if q == r and not is_ph:
                m += int(c[j])
                continue
            for i in range(l.size):                         # the run's first event not below the level; none: it is exhausted
                if l[i] >= level:
                    m += int(c[i])
                    break
        for rec in records:
            if 'ph_lnl' in rec:
                for b, v in zip(rec['ph_birth'], rec['ph_lnl']):
                    m += 1 if b < level <= v else 0
        rows.append((level, is_ph, r, index, m, log_x - 1.0 / m, level + log_x + math.log1p(-math.exp(-1.0 / m))))
        log_x -= 1.0 / m
    return rows


@pytest.mark.parametrize('seed', range(5))
def test_the_boosted_merge_against_its_definition(seed):
    records = _random_records(seed)
    merged = rep.merge_nested_boosted(records)
    want = _merge_by_definition(records)
    N_ = len(want)
    assert merged['lnl'].shape == merged['weights'].shape == merged['phantom'].shape == (N_,) and merged['points'].shape == (N_, 2)
    assert np.array_equal(merged['lnl'], [w[0] for w in want]) and np.array_equal(merged['phantom'], [bool(w[1]) for w in want])
    assert np.array_equal(merged['replica'], [w[2] for w in want]) and np.array_equal(merged['index'], [w[3] for w in want])
    assert np.array_equal(merged['nlive'], [w[4] for w in want])
    assert np.all(np.abs(merged['log_x'] - np.array([w[5] for w in want])) <= 1e-13)
    lw = np.array([w[6] for w in want])
    log_z = N._logsumexp(lw)
    assert abs(merged['log_z_boost'] - log_z) <= 1e-13
    assert np.all(np.abs(merged['weights'] - np.exp(lw - log_z)) <= 1e-13) and abs(merged['weights'].sum() - 1.0) <= 1e-12
    # the cases the records were built for are there
    lnl, ph, who = merged['lnl'], merged['phantom'], merged['replica']
    tied = np.flatnonzero(lnl[1:] == lnl[:-1])
    assert np.any(~ph[tied] & ~ph[tied + 1] & (who[tied] != who[tied + 1]))           # deaths of different replicas
    assert np.any(~ph[tied] & ph[tied + 1]) and not np.any(ph[tied] & ~ph[tied + 1])  # a death before the phantom it ties with
    last_death = max(r['live_lnl'].max() for r in records)
    assert np.sum(lnl > last_death) >= 3 and np.all(ph[lnl > last_death])
    assert not np.any(ph & (who == 1)) and np.any(ph & (who == 0)) and np.any(ph & (who == 2))
    # the rows are the records' rows
    for j in range(N_):
        r, i = who[j], merged['index'][j]
        src = records[r]['ph_points'][i] if ph[j] else records[r]['points'][i]
        assert np.array_equal(merged['points'][j], src)
    # the evidence is the base merge's
    base = rep.merge_nested(records)
    assert (merged['log_z'], merged['err'], merged['info'], merged['num_live']) == (base['log_z'], base['err'], base['info'], base['num_live'])


def test_the_boosted_merge_without_phantoms_is_the_merge():
    records = _random_records(3, with_phantoms=(False, False, False))
    merged, base = rep.merge_nested_boosted(records), rep.merge_nested(records)
    assert np.array_equal(merged['lnl'], base['lnl']) and np.array_equal(merged['nlive'], base['nlive'])
    assert np.array_equal(merged['replica'], base['replica']) and np.array_equal(merged['index'], base['index'])
    assert np.all(np.abs(merged['weights'] - base['weights']) <= 1e-13) and not np.any(merged['phantom'])
    assert np.array_equal(merged['points'], base['points']) and abs(merged['log_z_boost'] - base['log_z']) <= 1e-13
    empty = [dict(r, ph_lnl=np.empty(0), ph_birth=np.empty(0), ph_u=np.empty((0, 2)), ph_points=np.empty((0, 2))) for r in records]
    assert np.array_equal(rep.merge_nested_boosted(empty)['weights'], merged['weights'])
    # merge_nested itself does not read the phantoms
    with_ph = _random_records(3)
    plain = [{k: v for k, v in r.items() if not k.startswith('ph_')} for r in with_ph]
    assert np.array_equal(rep.merge_nested(with_ph)['weights'], rep.merge_nested(plain)['weights'])
    bad = [dict(with_ph[0], ph_birth=with_ph[0]['ph_lnl'].copy())] + with_ph[1:]
    with pytest.raises(ValueError, match='above its birth contour'):
        rep.merge_nested_boosted(bad)


# ------------------------------------------------------------------ statistics
def test_the_boosted_merge_of_three_gaussian_replicas(tmp_path):
    """The sigma = 0.03 correlated Gaussian of tests/test_nested_host.py in n = 2, R = 3 replicas at (nlive 128, K 32), 10 repeats,
    every inner point kept (f = 1), each to its own termination, through their records.  Measured here: the Kish sample size of
    the boosted merge is 9.90 times the base merge's (13 373 against 1 350; phantoms 12 384 + 12 096 + 12 672).  Asserted: at least 3
    times (the bound tests/test_nested_boost_host.py holds one run to); the weighted mean within 5 sigma / sqrt(ESS) and every
    coordinate's weighted variance over the true one within 5 sqrt(2 / ESS) of 1, both with the base merge's ESS - the boosted
    chain must fit inside the base chain's own bars; |log Z_boost - true| <= 4 err; the evidence is the base merge's."""
    loglike, cov, log_z_true = _correlated_gaussian(2)
    runs = N.NestedRunSet(loglike, 2, 3, num_live=128, num_repeats=10, threads=32, seed=0, boost_posterior=10).run()
    assert np.all(runs.finished) and runs.runs[0].phantom_state.fraction == 1.0
    records = []
    for e, run in enumerate(runs.runs):
        rec = rep.nested_record(run)
        ph = run.phantoms()
        assert np.array_equal(rec['ph_u'], ph['u']) and np.array_equal(rec['ph_lnl'], ph['lnl']) and np.array_equal(rec['ph_birth'], ph['birth'])
        assert np.array_equal(rec['points'], run.samples(boost=False)[0]) and rec['points'].shape[0] == rec['dead_lnl'].size + 128
        records.append(rep.load_record(rep.save_record(tmp_path / f'r{e}.npz', rec)))
    plain = rep.nested_record(N.NestedRun(lambda u: loglike(u), 2, num_live=20, threads=6, num_repeats=3).run(2))
    assert not any(key.startswith('ph_') for key in plain)                          # (a run without phantoms: the keys of before)
    merged, base = rep.merge_nested_boosted(records), rep.merge_nested(records)
    w, pts = merged['weights'], merged['points']
    ess, ess_base = 1.0 / np.sum(w**2), 1.0 / np.sum(base['weights']**2)
    mean = w @ pts
    pull = (mean - 0.5) / (0.03 / np.sqrt(ess_base))
    ratio = (w @ (pts - mean)**2) / np.diag(cov)
    base_pull = (base['weights'] @ base['points'] - 0.5) / (0.03 / np.sqrt(ess_base))
    print(f'phantoms {[int(r["ph_lnl"].size) for r in records]}, sample size {ess:.0f} / base {ess_base:.0f} = {ess / ess_base:.2f}, '
          f'mean pulls {np.round(pull, 2)} (base {np.round(base_pull, 2)}), variance ratios {np.round(ratio, 3)} '
          f'(allowed +-{5 * math.sqrt(2 / ess_base):.3f}), log Z_boost - true {(merged["log_z_boost"] - log_z_true) / merged["err"]:+.2f} err, '
          f'log Z - true {(merged["log_z"] - log_z_true) / merged["err"]:+.2f} err')
    assert int(merged['phantom'].sum()) == sum(int(r['ph_lnl'].size) for r in records) > 0
    assert ess >= 3.0 * ess_base
    assert np.all(np.abs(pull) <= 5), pull
    assert np.all(np.abs(ratio - 1.0) <= 5 * math.sqrt(2 / ess_base)), ratio
    assert abs(merged['log_z_boost'] - log_z_true) <= 4 * merged['err']
    assert merged['log_z'] == base['log_z'] and merged['err'] == base['err'] and merged['num_live'] == 3 * 128
    # the merged files of the boosted merge
    files = rep.write_merged(tmp_path, 'merged', records, merged=merged)
    stats = rep.read_stats(files[2])
    assert stats['phantom points'] == int(merged['phantom'].sum()) and stats['log(Z) boosted'] == merged['log_z_boost']
    assert stats['log(Z)'] == base['log_z'] and np.loadtxt(files[0]).shape == (w.size, 2 + 2)
    assert 'phantom points' not in rep.read_stats(rep.write_merged(tmp_path, 'plain', records)[2])


# ------------------------------------------------------------------ sample_mocks_nested and its table, python driver
class _Engine:
    """What the ``python`` driver and ``sample_mocks_nested`` ask of an engine, with rows that live on the host."""
    max_batch = 16
    rows_device = 'cpu'

    def __init__(self):
        self.pools = {}

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1

    def set_mock_pool(self, name, pool):
        self.pools[name] = np.asarray(pool)


class _Item:
    cov_rescale = None
    cov = None


class _Problem:
    mc_config = None

    def __init__(self):
        self.items = {'c': _Item()}


class _Vega:
    """The surface of VegaInterface the set and ``MonteCarlo._sample_mocks`` use, over a Gaussian in (a, b) whose centre is the
    mock's two numbers."""
    param_names = ['a', 'fixed', 'b']
    max_batch = 16
    _use_global_cov = False

    def __init__(self):
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _Engine()
        self.problem = _Problem()
        self._icov = np.linalg.inv(0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]]))

    def freeze_metals(self, row=None):
        pass

    def _theta(self, _):
        return np.array([0.5, 2.0, 0.5])

    def _log_norm(self):
        return 1.25

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        theta = np.asarray(t.numpy(), dtype=np.float64)
        d = theta[:, [0, 2]] - self.engine.pools['c'][np.asarray(mock_rows.numpy())]
        return torch.from_numpy(np.einsum('ij,jk,ik->i', d, self._icov, d))


BASE_KEYS = ['sampler', 'names', 'mean', 'sd', 'covariance', 'log_z', 'log_z_err', 'info', 'iterations', 'status', 'num_live',
             'num_repeats', 'threads', 'precision', 'seed', 'driver', 'stats']
BASE_COLUMNS = ['a_mean', 'a_sd', 'b_mean', 'b_sd', 'log_z', 'log_z_err', 'info', 'iterations', 'status', 'covariance']


def test_sample_mocks_nested_with_boost_and_its_table(tmp_path):
    """Three mocks (the centres of the stand-in's Gaussian) at (nlive 64, K 16), 6 repeats, on the python driver: at b = 0 the
    dict and the table are key for key, column for column what they were; at b = 6 the runs and their evidences are the same
    runs, the summaries are the boosted chains', and the three columns and BOOST are there."""
    import sys
    sys.path.insert(0, str(REPO / 'tests'))
    from fits_standard import check_file
    from vega_amd import fitslite
    from vega_amd.montecarlo import MonteCarlo
    mocks = {'c': np.array([[0.5, 0.5], [0.52, 0.49], [0.47, 0.52]])}
    kw = dict(mocks=mocks, num_live=64, threads=16, num_repeats=6, seed=3, driver='python', max_iterations=20)
    got = {}
    for b in (0.0, 6.0):
        mc = MonteCarlo(_Vega())
        sampler = mc.sample_mocks_nested(**kw, **({} if b == 0.0 else dict(boost_posterior=b)))
        assert sampler.driver == 'python' and sampler.boost_posterior == b and list(sampler.iteration) == [20, 20, 20]
        path = mc.write_mock_posteriors(tmp_path / f'b{int(b)}')
        check_file(path)
        with fitslite.open(str(path)) as hdus:
            got[b] = (mc.mc_posteriors, sampler, list(hdus[1].columns.names), dict(hdus[1].header),
                      {name: np.array(hdus[1].data[name]) for name in hdus[1].columns.names})
    post0, s0, cols0, head0, _ = got[0.0]
    post, s, cols, head, data = got[6.0]
    assert list(post0) == BASE_KEYS and cols0 == BASE_COLUMNS and 'BOOST' not in head0
    assert list(post)[:len(BASE_KEYS)] == BASE_KEYS and set(post) - set(BASE_KEYS) == {'boost_posterior', 'phantoms', 'n_eff', 'log_z_boost'}
    assert cols == BASE_COLUMNS + ['phantoms', 'n_eff', 'log_z_boost'] and head['BOOST'] == 6.0
    # the base runs are the same runs
    assert np.array_equal(post['log_z'], post0['log_z']) and np.array_equal(post['log_z_err'], post0['log_z_err'])
    assert np.array_equal(post['info'], post0['info']) and s.stats['rows'] == s0.stats['rows']
    found = s.samples()
    for m in range(3):
        pts, _, w = found[m]
        assert post['phantoms'][m] == s.phantoms(m)['lnl'].size == pts.shape[0] - (20 * 16 + 64) > 0
        assert post['n_eff'][m] == 1.0 / np.sum(w * w) and post['log_z_boost'][m] == s.runs[m].boost_log_evidence()
        assert np.array_equal(post['mean'][m], w @ pts) and not np.array_equal(post['mean'][m], post0['mean'][m])
        base_w = s.samples(boost=False)[m][2]
        assert post['n_eff'][m] > 2.0 / np.sum(base_w * base_w)
    assert np.array_equal(data['phantoms'], post['phantoms']) and np.array_equal(data['n_eff'], post['n_eff'])
    assert np.array_equal(data['log_z_boost'], post['log_z_boost']) and np.array_equal(data['a_mean'], post['mean'][:, 0])
    # a member carries its run's phantoms and writes the boosted chain
    member = s.member(1)
    assert member.phantom_state is not s.runs[1].phantom_state and member.boost_posterior == 6.0
    for x, y in zip(member.samples(), found[1]):
        assert np.array_equal(x, y)
    txt, _, stats = member.write(tmp_path, 'member')
    assert np.loadtxt(txt).shape[0] == found[1][0].shape[0] and N.read_stats(stats)['phantom points'] == post['phantoms'][1]
    assert N.read_stats(stats)['log(Z)'] == post['log_z'][1]
    with pytest.raises(RuntimeError, match='read-only'):
        member.run()


# ------------------------------------------------------------------ refusals
def test_what_the_sets_refuse():
    like = _gauss(2)
    vega = _Vega()
    for bad in (-1.0, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='boost_posterior: a finite number, at least 0'):
            N.NestedRunSet(like, 2, 2, boost_posterior=bad)
        with pytest.raises(ValueError, match='boost_posterior: a finite number, at least 0'):
            N.NestedSet(vega, 2, driver='python', boost_posterior=bad)
    # a budget that leaves no iteration per call: 64 runs of 2000 threads and 160 repeats in 32 dimensions
    big = dict(num_live=4096, threads=2000, num_repeats=160)
    assert N.set_iterations_per_call(64, 2000, 160, 32, True) == 0 and N.set_iterations_per_call(64, 2000, 160, 32, False) == 32
    with pytest.raises(ValueError, match='more than the 200000000 bytes a call may hold'):
        N.NestedRunSet(lambda u, runs: np.zeros(len(u)), 32, 64, boost_posterior=1.0, **big)
    assert N.NestedRunSet(lambda u, runs: np.zeros(len(u)), 32, 64, **big).boost_posterior == 0.0      # (without boost it is a set)
    # the cap of a call: min(65536 // K, budget // (E K (R - 1) (8 n + 36)))
    ok = N.NestedRunSet(like, 2, 3, num_live=40, threads=12, num_repeats=4, boost_posterior=2.0)
    assert ok._per_call() == min(65536 // 12, N.PHANTOM_BUDGET // (3 * 12 * 3 * (8 * 2 + 36))) == 5461
    assert N.set_iterations_per_call(16, 32, 30, 6, True) == N.PHANTOM_BUDGET // (16 * 32 * 29 * 84) == 160
    assert N.NestedRunSet(like, 2, 3, num_live=40, threads=12, num_repeats=1, boost_posterior=2.0)._per_call() == 65536 // 12
    with pytest.raises(ValueError, match='keeps no phantom points'):
        N.NestedRunSet(like, 2, 2, num_live=20, threads=6, num_repeats=3).run(1).phantoms(0)


def test_the_struct_and_the_symbol():
    """vmx_struct_size(20) is the ctypes struct's; the library exports vmx_nested_run_many_phantoms."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(20) == C.sizeof(engine.NestedSetPhantoms) == 80
    assert 'vmx_nested_run_many_phantoms' in engine.EXPORTED_SYMBOLS and hasattr(lib, 'vmx_nested_run_many_phantoms')
    arrays = engine.PhantomArrays(3, 5, 2, 0.5)
    assert arrays.u.shape == (3, 5, 2) and arrays.count.dtype == np.int64 and arrays.struct().capacity == 5
