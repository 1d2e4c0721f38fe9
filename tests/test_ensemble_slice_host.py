"""Ensemble slice sampling without a GPU: the header the device kernels are built from (vega_amd/csrc/vmx_ensemble.h, the fifth
part), compiled with g++ under AddressSanitizer / UBSan into tests/helpers/ensemble_slice_driver.cpp, against the NumPy restatement
of vega_amd/ensemble.py bit for bit - every field of every walker, the counts, offsets, row order and scale after every round of
a set, the answers replayed; the cases that force a box answer on either side, a failed model, an answer equal to the slice
height, both caps, the null direction, a half of two and the word extremes; a set's member against the single run; a run cut into
calls; the restatement's stationarity on a correlated Gaussian and on half-normals pressed against the box; the settings, the
refusals and the new struct's layout."""
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

M64 = 2**64 - 1


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('ensemble_slice') / 'ensemble_slice_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_slice_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _ask(exe, lines):
    out = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    got = out.stdout.splitlines()
    assert 'ERR' not in got
    return got


def _bits(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


def _hx(v):
    return f'{_bits(v):016x}'


def _hxs(a):
    return ' '.join(f'{int(v):016x}' for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


# ------------------------------------------------------------------ the words
def test_block_uses_the_documented_counter(driver):
    """Counter (k, s, 2 j + h, 6) under the key (seed, stream): NumPy's Philox draws the same block, and the last word 6 keeps it
    apart from the blocks of the other parts (0 - 3)."""
    cases = [(0, 0, 0, 0, 0, 0), (5, 17, 1, 0, 9, 2), (5, 17, 0, 1, 9, 2), (1055, 2**40, 1, 16, M64, 7)]
    got = _ask(driver, [f'K {k} {s} {h} {j} {seed:x} {stream:x}' for k, s, h, j, seed, stream in cases])
    for line, (k, s, h, j, seed, stream) in zip(got, cases):
        c = k | (s << 64) | ((2 * j + h) << 128) | (6 << 192)
        ref = [int(v) for v in np.random.Philox(key=np.array([seed, stream], dtype=np.uint64), counter=c - 1).random_raw(4)]
        assert [int(t, 16) for t in line.split()] == ref == list(E.slice_block(k, s, h, j, seed, stream))
        for last in range(4):
            other = E.philox_block(k, s, 2 * j + h, last, seed, stream)
            assert list(other) != ref
    # (half 1 of block j and half 0 of block j + 1 are different counters: 2 j + 1 and 2 j + 2)
    assert E.slice_block(3, 4, 1, 0, 1, 1) != E.slice_block(3, 4, 0, 1, 1, 1)
    assert E.philox_block(3, 4, 5, 6, 7, 8) == tuple(int(v) for v in E.philox4x64_10(np.array([3, 4, 5, 6], dtype=np.uint64), (7, 8)))


def test_word_functions_at_the_extremes(driver):
    """The shrink draw, the slice height, the partners and the tuning rule: header = restatement on random words and on the words
    0 and 2**64 - 1.  A word of 0 gives the height -inf (everything finite lies in the slice) and t = L; the largest word stays
    below R."""
    rng = np.random.default_rng(2)
    words = [0, M64, 2**63, 2**11 - 1, 2**11] + [int(v) for v in rng.integers(0, 2**64, size=40, dtype=np.uint64)]
    lines, want = [], []
    for i, w in enumerate(words):
        L, R = (-0.25, 0.75) if i < 5 else (float(-rng.random() * 3), float(rng.random() * 3))
        lnl = -12.5 if i < 5 else float(-rng.random() * 100)
        lines += [f'S {_hx(L)} {_hx(R)} {w:x}', f'Y {_hx(lnl)} {w:x}']
        want += [E.slice_shrink(L, R, w), E.slice_height(lnl, w)]
        for H in (2, 3, 1056):
            w1 = words[(i * 7 + H) % len(words)]
            j1 = ((w >> 32) * H) >> 32
            j2 = ((w1 >> 32) * (H - 1)) >> 32
            j2 += j2 >= j1
            assert 0 <= j1 < H and 0 <= j2 < H and j1 != j2
            lines.append(f'P {H} {w:x} {w1:x}')
            want.append((j1, j2))
    for mu, ne, nc in [(1.0, 0, 0), (1.0, 5, 3), (0.7, 0, 900), (1e308, 10, 0), (1e-308, 1, 10**12), (3.0, 2**40, 2**41), (2.0**-1022, 1, 3)]:
        lines.append(f'T {_hx(mu)} {ne} {nc}')
        want.append(E.slice_tune(mu, ne, nc))
    for line, ref in zip(_ask(driver, lines), want):
        if isinstance(ref, tuple):
            assert tuple(int(t) for t in line.split()) == ref
        else:
            assert int(line.split()[0], 16) == _bits(ref), (line, ref)
    assert E.slice_height(-3.0, 0) == -math.inf and E.slice_shrink(-0.25, 0.75, 0) == -0.25 and E.slice_shrink(-0.25, 0.75, M64) < 0.75
    assert E.slice_tune(1.0, 0, 0) == 2.0 and E.slice_tune(1.0, 5, 3) == 1.25
    assert E.slice_tune(1e308, 10, 0) == 1e308 and E.slice_tune(1e-308, 1, 10**12) == 1e-308       # (overflow, a subnormal: mu stays)
    assert E.slice_tune(2.0**-1022, 1, 3) == 2.0**-1022


# ------------------------------------------------------------------ the header against the restatement, round by round
def _dump(run):
    """The state of a :class:`vega_amd.ensemble.SliceRounds` after a round, as the driver prints it."""
    total = sum(c for _, c, _ in run.listing)
    out = [f'ROUND {run.rounds - 1} {len(run.listing)} {total}']
    out += [f'LIST {e} {c} {o}' for e, c, o in run.listing]
    for e in range(run.E):
        out.append(f'ENS {e} {run.q[e]} {int(run.open[e])} {run.count_of[e]} {_hx(run.mu[e])} ' + ' '.join(str(int(v)) for v in run.counts[e])
                   + f' {int(run.step_counts[e, 0])} {int(run.step_counts[e, 1])}')
        if run.wk[e][0] is not None:
            for k in range(run.H):
                w = run.wk[e][k]
                f = w.fields()
                out.append(f'WK {e} {k} ' + ' '.join(_hx(v) for v in f[:5]) + ' ' + ' '.join(str(int(v)) for v in f[5:])
                           + f' {run.slot[e][k]} ' + _hxs(run.eta[e][k]))
        out += [f'X {e} ' + _hxs(run.x[e]), f'L {e} ' + _hxs(run.lnl[e]), f'A {e} ' + ' '.join(str(int(v)) for v in run.accepted[e])]
    return out


def _replay(driver, problem, policy):
    """Runs the restatement on ``problem`` with the answers ``policy(run, rows, ens, round)`` -> (chi2, status), then the driver
    on the same answers; asserts that the two agree line by line after every round and in the chain.  Returns the restatement."""
    x, lnl, acc, mu = (problem[key].copy() for key in ('x', 'lnl', 'accepted', 'mu'))
    E_, W, n = x.shape
    kw = {key: problem[key] for key in ('step0', 'n_steps', 'thin', 'seed', 'streams', 'lo', 'hi', 'log_norm', 'tune_steps',
                                        'max_expansions', 'max_contractions')}
    lines = [f"RUN {n} {W} {E_} {kw['step0']} {kw['n_steps']} {kw['thin']} {kw['tune_steps']} {kw['max_expansions']} "
             f"{kw['max_contractions']} {kw['seed']:x} {_hx(kw['log_norm'])}",
             ' '.join(f'{int(s):x}' for s in kw['streams']), _hxs(mu), _hxs(kw['lo']), _hxs(kw['hi']), _hxs(x), _hxs(lnl),
             ' '.join(str(int(v)) for v in acc.reshape(-1))]
    run = E.SliceRounds(x, lnl, acc, mu, **kw)
    want, chi2, status = [], None, None
    while run.active:
        rows, ens = run.round(chi2, status)
        want += _dump(run)
        want += [f'ROW {r} {int(ens[r])} ' + _hxs(rows[r]) for r in range(rows.shape[0])]
        if rows.shape[0]:
            chi2, status = policy(run, rows, ens, run.rounds - 1)
            lines += [f'{int(s)} {_hx(c)}' for c, s in zip(chi2, status)]
    want.append(f'END {run.rounds}')
    for e in range(E_):
        want += [f'MU {e} {_hx(mu[e])}', f'CHAIN {e} ' + _hxs(run.chain[e]), f'CHAINL {e} ' + _hxs(run.chain_lnl[e])]
    got = _ask(driver, lines)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.split() == b.split(), (i, a[:300], b[:300])
    assert len(got) == len(want)
    return run


def _problem(n, W, E_, n_steps, seed=3, lo=0.0, hi=1.0, centre=0.5, spread=0.02, **over):
    rng = np.random.default_rng([seed, n, W])
    x = centre + spread * rng.standard_normal((E_, W, n))
    p = dict(x=x, lnl=-0.5 * np.sum(((x - centre) / 0.05)**2, axis=2), accepted=np.zeros((E_, W), dtype=np.int64), mu=np.full(E_, 1.0),
             step0=0, n_steps=n_steps, thin=1, seed=seed, streams=[7 + 3 * e for e in range(E_)], lo=np.full(n, float(lo)),
             hi=np.full(n, float(hi)), log_norm=0.0, tune_steps=2, max_expansions=32, max_contractions=64)
    p.update(over)
    return p


def _gauss(centre=0.5, sigma=0.05, fail_every=0):
    def policy(run, rows, ens, rnd):
        chi2 = np.sum(((rows - centre) / sigma)**2, axis=1)
        status = np.zeros(rows.shape[0], dtype=np.int32)
        if fail_every:
            bad = (np.arange(rows.shape[0]) + rnd) % fail_every == 0
            status[bad[::2].nonzero()[0] * 2] = 1          # (a failed status ...)
            chi2[bad] = np.where(status[bad] == 1, chi2[bad], 1e100)       # (... or the engine's sentinel)
        return chi2, status
    return policy


@pytest.mark.parametrize('n', [1, 2, 6, 32, 64])
def test_header_equals_restatement_after_every_round(driver, n):
    """Three ensembles on streams of their own, a Gaussian likelihood whose answers fail now and then (a status, or the chi2
    sentinel), a mu that tunes for two of the three steps, thinning, a start past step 0: every field after every round."""
    W = max(2 * n, 4) + (2 if n < 32 else 0)
    run = _replay(driver, _problem(n, W, 3, 3, step0=5, thin=2, tune_steps=7, mu=np.array([1.0, 0.3, 2.5])), _gauss(fail_every=5))
    c = run.counts.sum(axis=0)
    assert c[E.SC_UPDATES] == 3 * 3 * W and c[E.SC_FAILED] > 0 and c[E.SC_EXPANSIONS] > 0 and c[E.SC_CONTRACTIONS] > 0
    assert c[E.SC_ROWS] == run.rows and run.chain.shape == (3, 2, W, n) and not np.array_equal(run.mu, [1.0, 0.3, 2.5])
    assert c[E.SC_MOVED] == run.accepted.sum()


def _walkers_of(run, ens):
    """The walker of every row of the round."""
    out = []
    for e, count, _ in run.listing:
        out += [run.wk[e][k] for k in run.row_walker[e][:count]]
    assert len(out) == len(ens)
    return out


def test_forced_box_answers_on_each_side(driver):
    """Walkers pressed against the lower face (ensemble 0) and the upper face (ensemble 1) with a long direction: the bracket's
    far end leaves the box, the machine answers itself and no row is spent; the trial points inside go on."""
    n, W = 2, 8
    p = _problem(n, W, 2, 3, mu=np.array([40.0, 40.0]), tune_steps=0)
    p['x'][0] = 0.001 + 0.0005 * np.random.default_rng(1).random((W, n))
    p['x'][1] = 0.999 - 0.0005 * np.random.default_rng(2).random((W, n))
    run = _replay(driver, p, _gauss(centre=0.0, sigma=0.5))
    assert np.all(run.counts[:, E.SC_BOX] > 0) and np.all(run.counts[:, E.SC_ROWS] > 0)
    assert np.all(run.x >= 0.0) and np.all(run.x <= 1.0)
    # an out-of-box left end and an out-of-box right end both occurred: a bracket that never expanded on that side and still shrank
    assert np.all(run.counts[:, E.SC_CONTRACTIONS] > 0)


def test_forced_answer_equal_to_the_height_is_outside_the_slice(driver):
    """Every stepping-out request is answered with exactly lnY: not in the slice (strictly greater is), so no expansion ever
    happens; the shrink requests get the Gaussian."""
    def policy(run, rows, ens, rnd):
        chi2, status = _gauss()(run, rows, ens, rnd)
        for r, w in enumerate(_walkers_of(run, ens)):
            if w.phase in (E.SLICE_LEFT, E.SLICE_RIGHT):
                chi2[r] = -2.0 * w.lnY          # (log_norm 0: 0 - 0.5 chi2 is lnY exactly)
                assert 0.0 - 0.5 * chi2[r] == w.lnY
        return chi2, status
    run = _replay(driver, _problem(3, 8, 2, 2), policy)
    assert run.counts[:, E.SC_EXPANSIONS].sum() == 0 and run.counts[:, E.SC_ROWS].sum() > 2 * 2 * 8 * 2


@pytest.mark.parametrize('max_e, max_c', [(32, 64), (3, 5), (1, 1)])
def test_forced_caps(driver, max_e, max_c):
    """Stepping out always answered 'in the slice' in a box that never ends: max_expansions per side, then - every shrink request
    answered 'outside' - max_contractions and the update ends where it began."""
    def policy(run, rows, ens, rnd):
        out = np.array([w.phase == E.SLICE_SHRINK for w in _walkers_of(run, ens)])
        return np.where(out, 1e50, -1e50), np.zeros(rows.shape[0], dtype=np.int32)
    p = _problem(2, 6, 2, 2, lo=-1e9, hi=1e9, max_expansions=max_e, max_contractions=max_c, tune_steps=1)
    start = p['x'].copy()
    run = _replay(driver, p, policy)
    updates = 2 * 2 * 6
    assert np.array_equal(run.counts.sum(axis=0), [updates, 0, updates * (2 * max_e + max_c), updates * 2 * max_e, updates * max_c, 0, 0,
                                                    updates])
    assert np.array_equal(run.x, start) and run.accepted.sum() == 0


def test_forced_null_direction_and_a_half_of_two(driver):
    """W = 4: the two partners are the whole other half.  Ensemble 0's half 1 sits on one point, so every update of its half 0 has
    the null direction: the walker stays, nothing is asked; ensemble 1 runs as ever."""
    p = _problem(2, 4, 2, 3)
    p['x'][0, 2:] = [0.4, 0.6]
    run = _replay(driver, p, _gauss())
    assert run.counts[0, E.SC_CAPPED_NULL] >= 2 and run.counts[1, E.SC_CAPPED_NULL] == 0
    assert run.counts[0, E.SC_MOVED] + run.counts[0, E.SC_CAPPED_NULL] == run.counts[0, E.SC_UPDATES] == 12
    # all four walkers on one point: every direction is null, no round has a row, and the run still ends
    p = _problem(2, 4, 1, 2)
    p['x'][:] = 0.5
    run = _replay(driver, p, _gauss())
    assert run.rows == 0 and run.rounds == 1 and np.array_equal(run.counts[0], [8, 0, 0, 0, 0, 0, 0, 8])


def test_a_finished_ensemble_leaves_and_the_others_keep_their_order(driver):
    """Ensemble 1 of three has the null direction throughout and is done in the first round: the list compacts, the offsets of
    the others follow, their chains do not change."""
    p = _problem(2, 6, 3, 2)
    p['x'][1] = 0.5
    run = _replay(driver, p, _gauss())
    alone = _problem(2, 6, 3, 2)
    for e in (0, 2):
        one = E.SliceRounds(alone['x'][e:e + 1].copy(), alone['lnl'][e:e + 1].copy(), np.zeros((1, 6), dtype=np.int64), np.ones(1), 0, 2,
                            1, 3, [alone['streams'][e]], alone['lo'], alone['hi'], 0.0, 2)
        chi2 = status = None
        while one.active:
            rows, ens = one.round(chi2, status)
            chi2, status = _gauss()(one, rows, ens, 0)
        assert np.array_equal(one.chain[0], run.chain[e])


# ------------------------------------------------------------------ the restatement as a sampler
def _analytic(centre, icov):
    def evaluate(rows, ens):
        d = rows - centre
        return np.einsum('ri,ij,rj->r', d, icov, d), np.zeros(rows.shape[0], dtype=np.int32)
    return evaluate


def _start(rng, E_, W, n, centre, spread, evaluate):
    x = centre + spread * rng.standard_normal((E_, W, n))
    lnl = np.stack([-0.5 * evaluate(x[e], None)[0] for e in range(E_)])
    return x, lnl, np.zeros((E_, W), dtype=np.int64), np.ones(E_)


def test_every_set_member_is_the_single_run_on_its_stream():
    n, W = 3, 8
    ev = _analytic(0.5, np.eye(n) / 0.05**2)
    x, lnl, acc, mu = _start(np.random.default_rng(0), 3, W, n, 0.5, 0.03, ev)
    x[2] = 0.5 + 0.4 * (x[2] - 0.5)         # (another ensemble altogether: narrower, and it tunes differently)
    lnl[2] = -0.5 * ev(x[2], None)[0]
    streams = [5, 0, 11]
    single = []
    for e in range(3):
        s = [a[e:e + 1].copy() for a in (x, lnl, acc, mu)]
        single.append((E.python_steps_slice_many(*s, 0, 12, 1, 9, streams[e:e + 1], np.zeros(n), np.ones(n), 0.0, ev, tune_steps=6), s))
    chain, chain_lnl, st = E.python_steps_slice_many(x, lnl, acc, mu, 0, 12, 1, 9, streams, np.zeros(n), np.ones(n), 0.0, ev, tune_steps=6)
    for e, ((c1, l1, st1), s) in enumerate(single):
        assert np.array_equal(chain[e], c1[0]) and np.array_equal(chain_lnl[e], l1[0]) and np.array_equal(st['slice_counts'][e], st1['slice_counts'][0])
        assert np.array_equal(x[e], s[0][0]) and np.array_equal(acc[e], s[2][0]) and mu[e] == s[3][0]
    assert len({float(m) for m in mu}) == 3 and st['proposals'] == 3 * 12 * W == st['slice_counts'][:, 0].sum()


@pytest.mark.parametrize('cut', [4, 10, 17])
def test_a_run_cut_into_calls_is_the_run(cut):
    """run(a) then run(b) equals run(a + b), mu included: a cut inside the tuning (4), at its end (10) and after it (17)."""
    n, W, steps = 2, 6, 24
    ev = _analytic(0.5, np.array([[1.0, 0.4], [0.4, 1.0]]) / 0.04**2)
    whole = _start(np.random.default_rng(1), 2, W, n, 0.5, 0.03, ev)
    parts = [a.copy() for a in whole]
    args = (3, 21, [0, 1], np.zeros(n), np.ones(n), 0.25, ev)
    chain, chain_lnl, st = E.python_steps_slice_many(*whole, 0, steps, *args, tune_steps=10)
    c1, l1, st1 = E.python_steps_slice_many(*parts, 0, cut, *args, tune_steps=10)
    c2, l2, st2 = E.python_steps_slice_many(*parts, cut, steps - cut, *args, tune_steps=10)
    assert np.array_equal(np.concatenate([c1, c2], axis=1), chain) and np.array_equal(np.concatenate([l1, l2], axis=1), chain_lnl)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    assert np.array_equal(st1['slice_counts'] + st2['slice_counts'], st['slice_counts']) and chain.shape == (2, steps // 3, W, n)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_stationary_on_a_correlated_gaussian(seed):
    """n = 10, rho = 0.5, sigma = 0.03, centred in the unit box; W = 40, 600 steps, the first 100 tune mu, 150 are discarded.
    Mean and covariance within 5 standard errors at n_eff = N / tau_max.  (A prototype of this rule gave tau 15 - 17, n_eff
    1050 - 1170, worst pulls 1.6 / 3.1, 4.92 rows per update and no capped update.)"""
    n, W, steps, sigma, rho = 10, 40, 600, 0.03, 0.5
    cov = sigma**2 * (np.full((n, n), rho) + (1.0 - rho) * np.eye(n))
    ev = _analytic(0.5, np.linalg.inv(cov))
    x, lnl, acc, mu = _start(np.random.default_rng(seed), 1, W, n, 0.5, 0.01, ev)
    chain, _, st = E.python_steps_slice_many(x, lnl, acc, mu, 0, steps, 1, seed, [0], np.zeros(n), np.ones(n), 0.0, ev, tune_steps=100)
    post = chain[0, 150:]
    tau = E.integrated_time(post)
    flat = post.reshape(-1, n)
    n_eff = flat.shape[0] / tau.max()
    counts = dict(zip(E.SLICE_COUNT_NAMES, (int(v) for v in st['slice_counts'][0])))
    pull_m = np.abs(flat.mean(axis=0) - 0.5) / (sigma / np.sqrt(n_eff))
    pull_c = np.abs(np.cov(flat.T) - cov) / (np.sqrt(2.0 / n_eff) * sigma**2)
    print('seed', seed, 'tau', tau.max(), 'n_eff', n_eff, 'pulls', pull_m.max(), pull_c.max(), 'rows per update',
          counts['rows'] / counts['updates'], 'mu', float(mu[0]), counts)
    assert n_eff > 300 and counts['capped'] == 0 and counts['moved'] == counts['updates'] == steps * W
    assert np.all(pull_m < 5.0) and np.all(pull_c < 5.0)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_half_normals_pressed_against_the_box(seed):
    """Independent Gaussians of sigma = 0.05 centred on the lower face of the unit box in each of n = 3 coordinates: W = 16, 800
    steps, 200 discarded.  Mean within 5 standard errors of sigma sqrt(2 / pi), variance within 25 % of sigma^2 (1 - 2 / pi), and
    at least a quarter of the trial points are box answers - answered without an engine row.  (The prototype: tau 8 - 10, worst
    pull 1.9, variance ratios 0.92 - 1.05, 1.9 - 2.1 box answers beside 3.1 - 3.4 rows per update.)"""
    n, W, steps, sigma = 3, 16, 800, 0.05
    ev = _analytic(0.0, np.eye(n) / sigma**2)
    rng = np.random.default_rng(seed)
    x = np.abs(sigma * rng.standard_normal((1, W, n)))
    lnl = -0.5 * ev(x[0], None)[0][None]
    acc, mu = np.zeros((1, W), dtype=np.int64), np.ones(1)
    chain, _, st = E.python_steps_slice_many(x, lnl, acc, mu, 0, steps, 1, seed, [0], np.zeros(n), np.ones(n), 0.0, ev, tune_steps=100)
    assert np.all(chain >= 0.0) and np.all(chain <= 1.0)
    post = chain[0, 200:]
    tau = E.integrated_time(post)
    flat = post.reshape(-1, n)
    n_eff = flat.shape[0] / tau.max()
    mean, var = sigma * np.sqrt(2.0 / np.pi), sigma**2 * (1.0 - 2.0 / np.pi)
    counts = dict(zip(E.SLICE_COUNT_NAMES, (int(v) for v in st['slice_counts'][0])))
    pull = np.abs(flat.mean(axis=0) - mean) / np.sqrt(var / n_eff)
    ratio = flat.var(axis=0) / var
    print('seed', seed, 'tau', tau.max(), 'pull', pull.max(), 'variance ratios', ratio, 'box', counts['box'] / counts['updates'], 'rows',
          counts['rows'] / counts['updates'])
    assert np.all(pull < 5.0) and np.all(np.abs(ratio - 1.0) < 0.25)
    assert counts['box'] >= 0.25 * (counts['box'] + counts['rows']) and counts['capped'] == 0


# ------------------------------------------------------------------ the arguments and the settings
def test_resolve_slice():
    assert E.resolve_slice('slice', 8) == dict(mu0=1.0, tune_steps=100)
    assert E.resolve_slice('slice', 4, mu=0.5, tune_steps=0) == dict(mu0=0.5, tune_steps=0)
    assert E.resolve_slice([('slice', 1.0)], 8) == dict(mu0=1.0, tune_steps=100)
    assert E.resolve_slice(None, 8) is None and E.resolve_slice('de', 8) is None and E.resolve_slice([('de', 0.8), ('snooker', 0.2)], 8) is None
    for bad in (dict(moves=[('slice', 0.5), ('de', 0.5)]), dict(moves=['slice', 'stretch']), dict(moves='slice', walkers=2),
                dict(moves='slice', mu=0.0), dict(moves='slice', mu=-1.0), dict(moves='slice', mu=np.inf), dict(moves='slice', mu=np.nan),
                dict(moves='slice', tune_steps=-1), dict(moves='slice', gamma0=0.5), dict(moves='slice', gamma_s=1.5),
                dict(moves='slice', sigma=1e-5), dict(moves='de', mu=1.0), dict(moves=None, tune_steps=5)):
        with pytest.raises(ValueError):
            E.resolve_slice(**dict(dict(walkers=8), **bad))
    for bad in (dict(H=1), dict(mu0=0.0), dict(mu0=np.nan), dict(tune_steps=-1), dict(max_e=0), dict(max_e=33), dict(max_c=0), dict(max_c=65),
                dict(flags=1)):
        assert not E.slice_ok(**dict(dict(H=2, mu0=1.0, tune_steps=0, max_e=32, max_c=64, flags=0), **bad))
    assert E.slice_ok(2, 1.0, 0, 1, 1) and E.slice_ok(1000, 1e-3, 10**6, 32, 64)
    with pytest.raises(ValueError, match='slice'):
        E.SliceRounds(np.zeros((1, 2, 1)), np.zeros((1, 2)), np.zeros((1, 2), dtype=np.int64), np.ones(1), 0, 1, 1, 0, [0], [0.0], [1.0], 0.0)


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'


def test_slice_settings_parse(tmp_path):
    base = f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\n'
    plain = E.sampler_settings(_config(base), SAMPLE)
    assert plain == dict(sampler='Ensemble', path=tmp_path, name='ensemble', walkers=8, steps=1000, seed=0, a=2.0, thin=1, init='ball',
                         init_scale=1.0, driver='device')            # (no slice key: exactly the dict of ever)
    got = E.sampler_settings(_config(base + 'moves = slice\n'), SAMPLE)
    assert got == dict(plain, moves='slice') and E.moves_arguments(got) == dict(moves='slice')
    got = E.sampler_settings(_config(base + 'moves = slice\nslice_mu = 0.5\nslice_tune_steps = 40\n'), SAMPLE)
    assert got == dict(plain, moves='slice', slice_mu=0.5, slice_tune_steps=40)
    assert E.moves_arguments(got) == dict(moves='slice', mu=0.5, tune_steps=40) and E.moves_arguments(plain) == {}


@pytest.mark.parametrize('text, match', [
    ('walkers = 8\nmoves = slice 0.5 de 0.5\n', 'not a member of a mixture'),
    ('walkers = 8\nmoves = de slice\n', 'not a member of a mixture'),
    ('walkers = 8\nmoves = slice 1\n', 'not a member of a mixture'),
    ('walkers = 8\nmoves = slice\nslice_mu = 0\n', 'positive and finite'),
    ('walkers = 8\nmoves = slice\nslice_mu = wide\n', 'slice_mu'),
    ('walkers = 8\nmoves = slice\nslice_tune_steps = -3\n', 'tune_steps'),
    ('walkers = 8\nmoves = slice\nslice_tune_steps = 1.5\n', 'slice_tune_steps'),
    ('walkers = 8\nmoves = slice\ngamma0 = 0.5\n', 'not of slice'),
    ('walkers = 8\nmoves = de\nslice_mu = 0.5\n', 'moves is not slice'),
    ('walkers = 8\nslice_tune_steps = 5\n', 'moves is not slice'),
    ('walkers = 8\nmoves = slice\nntemps = 4\n', 'ntemps'),
])
def test_slice_settings_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\n{text}'), SAMPLE)


class _StandInEngine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 6
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1


class _StandInVega:
    """The surface of VegaInterface the samplers use, over a correlated Gaussian in (a, b)."""
    param_names = ['a', 'fixed', 'b']
    mc_config = None

    def __init__(self, config=None):
        self.main_config = configparser.ConfigParser()
        self.main_config.optionxform = str
        if config is not None:
            self.main_config.read(config)
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _StandInEngine()
        self._icov = np.linalg.inv(0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]]))
        self.batches = []

    def compute_model(self, run_init=False):
        return None

    def freeze_metals(self, row):
        pass

    def _sync_monte_carlo(self):
        pass

    def _theta(self, _):
        return np.array([0.5, 2.0, 0.5])

    def _log_norm(self):
        return 1.25

    def chi2_batch(self, theta):
        d = np.asarray(theta, dtype=np.float64)[:, [0, 2]] - 0.5
        return np.einsum('ij,jk,ik->i', d, self._icov, d)

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        assert t.shape[0] <= self.engine.max_batch and mock_rows is None
        assert np.all(t.numpy()[:, 1] == 2.0)
        self.batches.append(t.shape[0])
        return torch.from_numpy(self.chi2_batch(t.numpy()))


def test_sampler_classes_run_slice():
    """``EnsembleSampler`` and ``EnsembleSet`` with ``moves='slice'`` through the python driver: the statistics, a member against
    the single run, the segments, the chunks of a round, and what is refused."""
    vega = _StandInVega()
    one = E.EnsembleSampler(vega, 8, seed=5, stream=2, driver='python', moves='slice', tune_steps=6).run(10)
    assert one.driver == 'python' and one.slice == dict(mu0=1.0, tune_steps=6) and one.moves is None
    st = one.stats
    assert st['steps'] == 10 and st['proposals'] == 80 == st['slice']['updates'] and st['accepted'] == st['slice']['moved'] == int(one.accepted.sum())
    assert st['moves'] == {'slice': dict(proposals=80, accepted=st['slice']['moved'])}
    assert st['mu'] == float(one.mu[0]) != 1.0 and st['slice']['rows_per_update'] == st['slice']['rows'] / 80
    assert set(E.SLICE_COUNT_NAMES) <= set(st['slice']) and st['slice']['per_ensemble'].shape == (1, 8)
    assert sum(vega.batches) == st['slice']['rows'] and st['engine_calls'] == len(vega.batches) and max(vega.batches) <= 6
    assert one.get_chain().shape == (10, 8, 2) and np.all(np.isfinite(one.get_autocorr_time()))
    assert np.array_equal(one.get_chain()[-1], one.x) and np.array_equal(one.get_log_lik()[-1], one.lnl)
    cut = E.EnsembleSampler(vega, 8, seed=5, stream=2, driver='python', moves='slice', tune_steps=6, segment=3).run(4).run(6)
    assert np.array_equal(cut.get_chain(), one.get_chain()) and cut.mu[0] == one.mu[0] and cut.stats['calls'] == 4
    assert np.array_equal(cut.slice_counts, one.slice_counts)
    both = E.EnsembleSet(vega, 3, 8, streams=[4, 2, 1], seed=5, driver='python', segment=4, moves='slice', tune_steps=6).run(10)
    member = both.member(1)
    assert np.array_equal(member.get_chain(), one.get_chain()) and np.array_equal(member.accepted, one.accepted)
    assert member.stats['slice']['updates'] == 80 and member.stats['mu'] == st['mu'] and member.stats['moves'] == st['moves']
    assert both.stats['mu'].shape == (3,) and both.stats['slice']['per_ensemble'].shape == (3, 8)
    assert both.stats['proposals'] == 240 and np.array_equal(both.per_ensemble[:, 0], both.slice_counts[:, E.SC_MOVED])
    other = E.EnsembleSampler(vega, 8, seed=5, stream=2, driver='python', moves='slice', mu=0.2, tune_steps=0).run(10)
    assert other.mu[0] == 0.2 and not np.array_equal(other.get_chain(), one.get_chain())
    with pytest.raises(ValueError, match='mixture'):
        E.EnsembleSampler(vega, 8, moves=[('slice', 0.5), ('de', 0.5)])
    with pytest.raises(ValueError, match='tempering'):
        E.TemperedEnsemble(vega, 8, ntemps=3, moves='slice')
    with pytest.raises(ValueError, match='tempering'):
        E.TemperedEnsemble(vega, 8, betas=[1.0, 0.5], moves=[('slice', 1.0)])
    with pytest.raises(ValueError, match="moves='slice'"):
        E.EnsembleSet(vega, 2, 8, mu=0.5)
    with pytest.raises(ValueError, match='mu'):
        E.EnsembleSampler(vega, 8, moves='slice', mu=-1.0)


def test_settings_reach_the_samplers(tmp_path):
    """``build_sampler``, the replicas one after the other and ``together = True`` run the configured slice sampler: through
    ``run_vega_sampler`` over the stand-in both paths write the same records, the chains of a sampler built by hand."""
    from vega_amd import replicas as rep
    folders = {}
    for tag, extra in (('seq', ''), ('tog', 'together = True\n')):
        out = tmp_path / tag
        out.mkdir()
        (out / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {out}\nname = run\ndriver = python\nwalkers = 8\nsteps = 30\nseed = 3\n'
                                      f'replicas = 2\nmoves = slice\nslice_mu = 0.8\nslice_tune_steps = 12\n{extra}')
        run = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                                 make_vega=lambda config, device: _StandInVega(config))
        assert run.replicas == 2 and all(s.slice == dict(mu0=0.8, tune_steps=12) for s in run.samplers)
        folders[tag] = out
    for r in range(2):
        seq, tog = (rep.load_record(rep.record_path(folders[tag], 'run', r)) for tag in ('seq', 'tog'))
        by_hand = E.EnsembleSampler(_StandInVega(), 8, seed=3, stream=r, driver='python', moves='slice', mu=0.8, tune_steps=12).run(30)
        assert np.array_equal(seq['chain'], by_hand.get_chain()) and np.array_equal(tog['chain'], by_hand.get_chain())
        assert seq['stats']['moves_slice_proposals'] == 240 == tog['stats']['moves_slice_proposals']
        assert seq['stats']['slice_rows'] == by_hand.stats['slice']['rows'] == tog['stats']['slice_rows']
        assert float(seq['stats']['mu']) == by_hand.stats['mu'] == float(tog['stats']['mu'])
    single = tmp_path / 'single'
    single.mkdir()
    (single / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {single}\nname = run\ndriver = python\nwalkers = 8\nsteps = 20\nmoves = slice\n')
    s = E.run_vega_sampler(str(single / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                           make_vega=lambda config, device: _StandInVega(config))
    assert s.slice == dict(mu0=1.0, tune_steps=100) and (single / 'run.txt').exists() and (single / 'run.paramnames').exists()
    assert np.loadtxt(single / 'run.txt').shape == (20 * 8, 4)


def test_slice_struct_matches_the_library():
    """The new struct's layout (vmx_struct_size index 25: the next free one) agrees with the ctypes binding, field by field, and the
    entry is bound."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    S = engine.EnsembleSlice
    assert lib.vmx_struct_size(25) == C.sizeof(S) == 24 and lib.vmx_struct_size(26) == -1 and lib.vmx_struct_size(22) == -1
    assert [(name, getattr(S, name).offset, getattr(S, name).size) for name, _ in S._fields_] == [
        ('mu0', 0, 8), ('tune_steps', 8, 4), ('max_expansions', 12, 4), ('max_contractions', 16, 4), ('flags', 20, 4)]
    assert len(lib.vmx_ensemble_run_slice.argtypes) == len(lib.vmx_ensemble_run_many.argtypes) + 2
    assert 'vmx_ensemble_run_slice' in engine.EXPORTED_SYMBOLS and hasattr(lib, 'vmx_ensemble_run_slice')
    assert engine.VMX_SLICE_COUNTS == len(engine.SLICE_COUNT_NAMES) == len(E.SLICE_COUNT_NAMES) == 8
    assert engine.SLICE_COUNT_NAMES == E.SLICE_COUNT_NAMES
