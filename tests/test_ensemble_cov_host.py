"""The ensemble sampler's covariance move without a GPU: the header the device kernel is built from (vega_amd/csrc/vmx_ensemble.h, the
sixth part), compiled with g++ under AddressSanitizer / UBSan into tests/helpers/ensemble_cov_driver.cpp, against the NumPy
restatement of vega_amd/ensemble.py bit for bit - the variate at the word extremes, the thresholds of four weights, the factor of a
half (which the driver also holds against the nested sampler's serial functions), the certain diagonal fallback, the proposals; the
restatement's sampling of the correlated 10-dimensional Gaussian in a box under the pure move; ``resolve_moves``, the ``[Ensemble]``
settings and the sampler classes with and without cov, and every refusal; the new struct's layout and the two new entries."""
import configparser
import ctypes as C
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
    exe = tmp_path_factory.mktemp('ensemble_cov') / 'ensemble_cov_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_cov_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _ask(exe, lines):
    out = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) and 'ERR' not in got
    return got


def _bits(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


def _hx(v):
    return f'{_bits(v):016x}'


def _half(rng, H, n):
    """A correlated half whose columns' standard deviations span three decades."""
    A = rng.normal(size=(n, n)) / np.sqrt(n) + np.eye(n)
    return (rng.normal(size=(H, n)) @ A.T) * 10.0 ** np.linspace(-1.5, 1.5, n) + rng.normal(size=n)


# ------------------------------------------------------------------ the header against the restatement
def test_variate_bitwise_and_at_the_word_extremes(driver):
    """0 and all ones give -+ 2 sqrt(3) to the last bit of the pinned product (-+131070 kappa); the variate is symmetric under
    the complement of the word, of unit variance, and the header equals the restatement on random words."""
    kappa = np.sqrt(np.float64(3.0) / np.float64(4294967295.0))
    rng = np.random.default_rng(2)
    words = [0, M64, 0xFFFF, 0xFFFF0000FFFF0000, 0x7FFF7FFF80008000, 1 << 63] + [int(v) for v in rng.integers(0, 2**64, size=300, dtype=np.uint64)]
    got = [int(t, 16) for t in _ask(driver, [f'Z {w:x}' for w in words])]
    ref = E.cov_z(np.array(words, dtype=np.uint64))
    assert got == [_bits(v) for v in ref]
    assert ref[0] == -131070.0 * kappa and ref[1] == 131070.0 * kappa
    assert abs(ref[1] - 2.0 * np.sqrt(3.0)) < 1e-4 and np.all(np.abs(ref) <= ref[1])
    assert ref[4] == 0.0            # (0x7fff + 0x7fff + 0x8000 + 0x8000 = 131070)
    flipped = E.cov_z(np.array(words, dtype=np.uint64) ^ np.uint64(M64))
    assert np.array_equal(flipped, -ref)
    z = E.cov_z(rng.integers(0, 2**64, size=400_000, dtype=np.uint64))
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / z.size)


WEIGHTS = [(0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 3.0), (0.0, 0.0, 0.3, 0.7), (0.25, 0.25, 0.25, 0.25), (0.3, 0.4, 0.3, 0.0),
           (0.0, 0.8, 0.2, 0.0), (1.0, 0.0, 0.0, 1e-300), (1e-300, 1e-300, 1e-300, 1e-300), (0.1, 0.0, 0.7, 2.0)]


def test_thresholds_and_choice_bitwise(driver):
    """The thresholds of four weights and the move they choose: the header equals the restatement; with a cov weight of 0 the
    first two thresholds are those of three weights and cov is never chosen; a pure cov run is chosen by every word."""
    got = _ask(driver, ['T ' + ' '.join(map(_hx, p)) for p in WEIGHTS])
    ts = []
    for line, p in zip(got, WEIGHTS):
        t = E.move_thresholds4(p)
        assert [int(v, 16) for v in line.split()] == [_bits(v) for v in t], p
        if p[3] == 0.0:
            assert t[:2] == E.move_thresholds(p[:3]) and t[2] == 1.0
        ts.append(t)
    rng = np.random.default_rng(3)
    words = np.concatenate([np.array([0, M64, 2**63, 2**63 - 1], dtype=np.uint64), rng.integers(0, 2**64, size=60, dtype=np.uint64)])
    seen = set()
    for t, p in zip(ts, WEIGHTS):
        ref = E.move_choice4(words, *t)
        got = [int(v) for v in _ask(driver, [f'M {_hx(t[0])} {_hx(t[1])} {_hx(t[2])} {int(w):x}' for w in words])]
        assert got == [int(v) for v in ref], p
        seen |= set(got)
        if p[:3] == (0.0, 0.0, 0.0):
            assert set(got) == {E.MOVE_COV}
        if p[3] == 0.0:
            assert E.MOVE_COV not in got and np.array_equal(ref, E.move_choice(words, t[0], t[1]))
    assert seen == {0, 1, 2, 3}


def test_variates_use_the_documented_counters(driver):
    """Column b of walker k takes word b % 4 of the block with counter (k, s, h, 2 + b // 4)."""
    cases = [(1, 0, 0, 0, 0, 0), (4, 5, 17, 1, 9, 2), (5, 1055, 2**40, 1, M64, 7), (18, 3, 2, 0, 1, 1), (64, 63, 9, 1, 5, 3)]
    got = _ask(driver, [f'V {n} {i} {s} {h} {seed:x} {stream:x}' for n, i, s, h, seed, stream in cases])
    for line, (n, i, s, h, seed, stream) in zip(got, cases):
        words = []
        for j in range((n + 3) // 4):
            c = i | (s << 64) | (h << 128) | ((2 + j) << 192)
            words += [int(v) for v in np.random.Philox(key=np.array([seed, stream], dtype=np.uint64), counter=c - 1).random_raw(4)]
        ref = E.cov_z(np.array(words[:n], dtype=np.uint64))
        assert [int(t, 16) for t in line.split()] == [_bits(v) for v in ref]
        assert np.array_equal(E.cov_variates([i], n, s, h, seed, stream)[0], ref)
        assert np.array_equal(E.cov_variates(np.arange(i + 1), n, s, h, seed, stream)[i], ref)


def _factor_line(c):
    H, n = c.shape
    return ' '.join(['F', str(n), str(H), *map(_hx, c.reshape(-1))])


def _check_factor(line, c):
    n = c.shape[1]
    tok = line.split()
    mean, Cf, good = E.half_factor(c)
    assert tok[0] == ('1' if good else '0')
    assert [int(t, 16) for t in tok[1:1 + n]] == [_bits(v) for v in mean]
    assert [int(t, 16) for t in tok[1 + n:]] == [_bits(v) for v in Cf.reshape(-1)]
    return mean, Cf, good


@pytest.mark.parametrize('n', [1, 2, 5, 32, 64])
def test_factor_bitwise(driver, n):
    """Mean and factor of a half at H = n + 1 (the fewest walkers with a factor) and H = 2 n: the header's entry-by-entry functions,
    the nested sampler's serial ones (compared inside the driver) and the restatement agree bit for bit; C C^T is the covariance."""
    rng = np.random.default_rng(300 + n)
    halves = [_half(rng, H, n) for H in (n + 1, 2 * n) if H >= 2]
    for line, c in zip(_ask(driver, [_factor_line(c) for c in halves]), halves):
        mean, Cf, good = _check_factor(line, c)
        assert good and np.all(np.triu(Cf, 1) == 0.0) and np.all(np.diag(Cf) > 0.0)
        cov = np.atleast_2d(np.cov(c.T))
        assert np.allclose(Cf @ Cf.T, cov, rtol=1e-6, atol=1e-9 * np.abs(cov).max())
        assert np.allclose(mean, c.mean(axis=0), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('n', [2, 5, 32])
def test_constant_column_gives_the_diagonal_fallback(driver, n):
    """A half with one column constant over its walkers: its mean is the constant exactly (k v / k is v), so its variance is
    exactly 0, the pivot exactly not positive, and the factor is the diagonal of standard deviations with a 0 in that column."""
    rng = np.random.default_rng(400 + n)
    c = _half(rng, 2 * n, n)
    col = n // 2
    c[:, col] = 0.375
    (line,) = _ask(driver, [_factor_line(c)])
    mean, Cf, good = _check_factor(line, c)
    assert not good and mean[col] == 0.375 and Cf[col, col] == 0.0
    assert np.all(Cf - np.diag(np.diag(Cf)) == 0.0)
    others = np.delete(np.arange(n), col)
    assert np.allclose(np.diag(Cf)[others], c[:, others].std(axis=0, ddof=1), rtol=1e-10)


def test_singular_half_agrees_whatever_the_last_pivot_rounds_to(driver):
    """H = n: the covariance has rank n - 1; both sides take the same branch."""
    rng = np.random.default_rng(7)
    halves = [_half(rng, n, n) for n in (2, 3, 8, 18)]
    for line, c in zip(_ask(driver, [_factor_line(c) for c in halves]), halves):
        _check_factor(line, c)


@pytest.mark.parametrize('n', [1, 2, 5, 32, 64])
def test_proposals_bitwise(driver, n):
    rng = np.random.default_rng(500 + n)
    cases, lines = [], []
    for k in range(40):
        _, Cf, _ = E.half_factor(_half(rng, n + 3, n))
        gamma = float(rng.choice([2.38 / np.sqrt(n), 1.0, rng.random() + 0.05]))
        s = rng.normal(size=n) * 10.0 ** np.linspace(-1.5, 1.5, n)
        words = rng.integers(0, 2**64, size=n, dtype=np.uint64) if k % 4 else rng.choice(np.array([0, M64], dtype=np.uint64), size=n)
        z = E.cov_z(words)
        cases.append((gamma, s, z, Cf))
        lines.append(' '.join(['P', str(n), _hx(gamma), *map(_hx, s), *map(_hx, z), *map(_hx, Cf.reshape(-1))]))
    for line, (gamma, s, z, Cf) in zip(_ask(driver, lines), cases):
        y = E.cov_propose(s[None], Cf, gamma, z[None])[0]
        assert [int(t, 16) for t in line.split()] == [_bits(v) for v in y]
        assert np.allclose(y, s + gamma * (Cf @ z), rtol=1e-9, atol=1e-12 * np.abs(s).max())


def test_half_step_with_cov_reads_the_other_half_alone():
    """The factor is that of the complementary half, whatever the active half holds; the proposals are s + gamma_c C z with the
    documented variates, and the factor of the decision is 0."""
    rng = np.random.default_rng(11)
    W, n = 12, 3
    x = rng.normal(size=(W, n))
    lo, hi = np.full(n, -50.0), np.full(n, 50.0)
    moves = E.resolve_moves('cov', n, W)
    assert moves['weights'] == (0.0, 0.0, 0.0, 1.0) and moves['cov_scale'] == 2.38 / np.sqrt(3.0)
    for h in (0, 1):
        y, inside, factor, _ = E.half_step_proposals(x, h, 4, 2.0, 1, 2, lo, hi, moves)
        other, own = x[(1 - h) * 6:(2 - h) * 6], x[h * 6:(h + 1) * 6]
        _, Cf, good = E.half_factor(other)
        assert good and inside.all() and np.all(factor == 0.0)
        assert np.array_equal(y, E.cov_propose(own, Cf, moves['cov_scale'], E.cov_variates(np.arange(6), n, 4, h, 1, 2)))
        moved = x.copy()
        moved[h * 6:(h + 1) * 6] += 1.0
        y2 = E.half_step_proposals(moved, h, 4, 2.0, 1, 2, lo, hi, moves)[0]
        assert np.array_equal(y2, E.cov_propose(moved[h * 6:(h + 1) * 6], Cf, moves['cov_scale'], E.cov_variates(np.arange(6), n, 4, h, 1, 2)))


# ------------------------------------------------------------------ the python driver on a Gaussian
def _gaussian_problem(n=10):
    """(the problem of tests/test_ensemble_moves_host.py)"""
    rng = np.random.default_rng(21)
    A = rng.normal(size=(n, n))
    cov = A @ A.T / n + 0.3 * np.eye(n)
    sd = np.sqrt(np.diag(cov))
    scale = np.linspace(0.5, 2.0, n)
    cov = cov / np.outer(sd, sd) * np.outer(scale, scale)
    mean = np.linspace(-1.0, 1.0, n)
    sd = np.sqrt(np.diag(cov))
    lo, hi = mean - 6 * sd, mean + 6 * sd
    lo[2] = mean[2] - 0.5 * sd[2]            # (the box clips one tail)
    return mean, cov, lo, hi


def _run_python(mean, cov, lo, hi, W, steps, moves, seed=3, thin=1, segments=None, a=2.0):
    icov = np.linalg.inv(cov)
    n = mean.size
    rng = np.random.default_rng(seed)
    x = np.clip(mean + 0.1 * np.sqrt(np.diag(cov)) * rng.standard_normal((W, n)), lo, hi)

    def chi2_of(rows):
        d = rows - mean
        return np.einsum('bi,ij,bj->b', d, icov, d)

    def evaluate(rows, h):
        return chi2_of(rows), np.zeros(rows.shape[0], dtype=np.int32)

    lnl = E.log_lik(-3.0, chi2_of(x))
    acc = np.zeros(W, dtype=np.int64)
    chains, lnls, stats = [], [], []
    step = 0
    for k in (segments or [steps]):
        ch, cl, st = E.python_steps(x, lnl, acc, step, k, thin, a, seed, 0, lo, hi, -3.0, evaluate, moves=E.resolve_moves(moves, n, W))
        chains.append(ch), lnls.append(cl), stats.append(st)
        step += k
    return np.concatenate(chains), np.concatenate(lnls), acc, stats


@pytest.mark.parametrize('moves', ['cov', [('cov', 0.7), ('snooker', 0.3)], [('stretch', 0.25), ('de', 0.25), ('snooker', 0.25), ('cov', 0.25)]], ids=str)
def test_the_chain_is_independent_of_the_cut(moves):
    mean, cov, lo, hi = _gaussian_problem()
    one = _run_python(mean, cov, lo, hi, 24, 60, moves, thin=3)
    two = _run_python(mean, cov, lo, hi, 24, 60, moves, thin=3, segments=[31, 29])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert one[0].shape == (20, 24, 10) and one[2].sum() > 0
    assert sum(int(st['cov_fallbacks'].sum()) for st in one[3]) == sum(int(st['cov_fallbacks'].sum()) for st in two[3]) == 0


def test_a_cov_weight_of_zero_is_the_run_of_three_moves():
    mean, cov, lo, hi = _gaussian_problem()
    mix = [('de', 0.8), ('snooker', 0.2)]
    one = _run_python(mean, cov, lo, hi, 24, 30, mix)
    two = _run_python(mean, cov, lo, hi, 24, 30, mix + [('cov', 0.0)])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2]) and 'cov_fallbacks' not in two[3][0]


def test_python_driver_samples_a_clipped_gaussian_under_pure_cov():
    """The correlated 10-D Gaussian in a box that clips one tail, under the pure covariance move: no sample outside the box; mean
    and covariance of the chain match the truncated Gaussian's within 5 Monte-Carlo standard errors at N / tau_max, tau measured
    on the chain; n_eff > 100 (a NumPy simulation of the rule gave tau about 33 at W = 64: 1500 steps after a third dropped
    leave n_eff about 1900)."""
    mean, cov, lo, hi = _gaussian_problem()
    draws = np.random.default_rng(5).multivariate_normal(mean, cov, size=3_000_000)
    draws = draws[np.all((draws >= lo) & (draws <= hi), axis=1)]
    m_ref, c_ref = draws.mean(axis=0), np.cov(draws.T)
    W, steps, burn = 64, 1500, 500
    chain, lnl, acc, stats = _run_python(mean, cov, lo, hi, W, steps, 'cov')
    assert np.all(chain >= lo) and np.all(chain <= hi)
    post = chain[burn:]
    tau = E.integrated_time(post)
    flat = post.reshape(-1, mean.size)
    n_eff = flat.shape[0] / tau.max()
    print('cov', 'tau', tau.max(), 'n_eff', n_eff, 'acceptance', acc.mean() / steps, 'fallbacks', stats[0]['cov_fallbacks'])
    assert n_eff > 100, tau
    sd = np.sqrt(np.diag(c_ref))
    assert np.all(np.abs(flat.mean(axis=0) - m_ref) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - m_ref) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - c_ref) < tol), ((np.cov(flat.T) - c_ref) / np.outer(sd, sd), n_eff)
    assert abs(m_ref[2] - mean[2]) > 0.1 * sd[2]         # (the clipped tail moved the mean: the box matters)
    assert 0.05 < acc.mean() / steps < 0.9
    assert int(stats[0]['cov_fallbacks'].sum()) == 0


# ------------------------------------------------------------------ the arguments and the settings
def test_resolve_moves_with_and_without_cov():
    d = E.resolve_moves('cov', 9, 32)
    assert d == dict(weights=(0.0, 0.0, 0.0, 1.0), gamma0=2.38 / np.sqrt(18.0), sigma=1e-5, gamma_s=1.7, cov_scale=2.38 / 3.0)
    d = E.resolve_moves([('cov', 0.7), ('snooker', 0.3)], 2, 6, cov_scale=0.5)
    assert d == dict(weights=(0.0, 0.0, 0.3, 0.7), gamma0=2.38 / 2.0, sigma=1e-5, gamma_s=1.7, cov_scale=0.5)
    assert E.resolve_moves(d, 2, 6) == d and E.has_cov(d)
    assert E.resolve_moves(dict(d, cov_scale=None), 2, 6, cov_scale=0.25)['cov_scale'] == 0.25
    # without a positive cov weight: exactly the dict of three weights
    three = dict(weights=(0.0, 0.8, 0.2), gamma0=2.38 / 2.0, sigma=1e-5, gamma_s=1.7)
    assert E.resolve_moves([('de', 0.8), ('snooker', 0.2)], 2, 6) == three
    assert E.resolve_moves([('de', 0.8), ('snooker', 0.2), ('cov', 0.0)], 2, 6) == three
    assert E.resolve_moves(dict(weights=(0.0, 0.8, 0.2, 0.0), gamma0=2.38 / 2.0), 2, 6) == three
    assert not E.has_cov(three) and not E.has_cov(None)
    assert E.names_cov('cov') and E.names_cov([('de', 1.0), ('cov', 0.1)]) and E.names_cov(d)
    assert not E.names_cov('de') and not E.names_cov([('cov', 0.0), 'de']) and not E.names_cov(None) and not E.names_cov(three)
    for bad in (dict(moves='cov', walkers=2), dict(moves='cov', cov_scale=0.0), dict(moves='cov', cov_scale=-1.0),
                dict(moves='cov', cov_scale=np.inf), dict(moves='cov', cov_scale=np.nan), dict(moves='de', cov_scale=1.0),
                dict(moves=None, cov_scale=1.0), dict(moves=[('cov', -1.0)]), dict(moves=[('cov', np.nan)]), dict(moves=[('cov', np.inf)]),
                dict(moves=[('cov', 0.0)]), dict(moves=[('cov', 0.0), ('de', 1.0)], cov_scale=1.0),
                dict(moves=dict(weights=(0.0, 0.0, 0.0, 0.0, 1.0))), dict(moves='walk'), dict(moves='kde')):
        args = dict(dict(n=1, walkers=8), **bad)
        with pytest.raises(ValueError):
            E.resolve_moves(**args)


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'


def test_cov_settings_parse(tmp_path):
    base = f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\n'
    plain = E.sampler_settings(_config(base), SAMPLE)
    assert 'moves' not in plain and 'cov_scale' not in plain
    for text, want in (('moves = cov\n', dict(moves=[('cov', 1.0)])),
                       ('moves = cov 0.7 snooker 0.3\n', dict(moves=[('cov', 0.7), ('snooker', 0.3)])),
                       ('moves = cov 0.7, snooker 0.3\ncov_scale = 1.2\n', dict(moves=[('cov', 0.7), ('snooker', 0.3)], cov_scale=1.2)),
                       ('moves = stretch de snooker cov\n', dict(moves=[('stretch', 1.0), ('de', 1.0), ('snooker', 1.0), ('cov', 1.0)]))):
        got = E.sampler_settings(_config(base + text), SAMPLE)
        assert got == dict(plain, **want), text
    cfg = E.sampler_settings(_config(base + 'moves = cov 0.7 snooker 0.3\ncov_scale = 1.2\n'), SAMPLE)
    assert E.moves_arguments(cfg) == dict(moves=[('cov', 0.7), ('snooker', 0.3)], cov_scale=1.2)
    # (a section without cov parses to what it did)
    got = E.sampler_settings(_config(base + 'moves = de 0.8 snooker 0.2\n'), SAMPLE)
    assert got == dict(plain, moves=[('de', 0.8), ('snooker', 0.2)])


@pytest.mark.parametrize('text, match', [
    ('walkers = 8\nmoves = cov\ncov_scale = 0\n', 'cov_scale'),
    ('walkers = 8\nmoves = cov\ncov_scale = -2\n', 'cov_scale'),
    ('walkers = 8\nmoves = cov\ncov_scale = much\n', 'cov_scale'),
    ('walkers = 8\nmoves = de\ncov_scale = 1\n', 'cov_scale'),
    ('walkers = 8\ncov_scale = 1\n', 'no moves'),
    ('walkers = 8\nmoves = cov -1\n', 'not negative'),
    ('walkers = 8\nmoves = cov 0\n', 'positive sum'),
    ('walkers = 8\nmoves = cov slice\n', 'slice'),
    ('walkers = 8\nmoves = slice\ncov_scale = 1\n', 'slice'),
    ('walkers = 8\nmoves = cov\nntemps = 3\n', 'ntemps'),
    ('walkers = 8\nmoves = cov 0.5 de 0.5\nntemps = 3\n', 'ntemps'),
    ('walkers = 8\nmoves = walk\n', 'unknown move'),
])
def test_cov_settings_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\n{text}'), SAMPLE)


# ------------------------------------------------------------------ the sampler classes and the launcher body over a stand-in
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
        return torch.from_numpy(self.chi2_batch(t.numpy()))


def test_sampler_classes_take_cov_and_count_it():
    """``EnsembleSampler`` and ``EnsembleSet`` with cov in the mixture through the python driver: the set's member e is the single
    run on its stream; ``stats['moves']`` has a cov entry exactly when the mixture has one, ``stats['cov']`` the scale and the
    fallbacks; the refusals of the classes."""
    vega = _StandInVega()
    mix = [('stretch', 0.25), ('de', 0.25), ('snooker', 0.25), ('cov', 0.25)]
    both = E.EnsembleSet(vega, 3, 8, streams=[4, 1, 2], seed=5, driver='python', segment=4, moves=mix, cov_scale=1.5).run(10)
    assert both.moves == E.resolve_moves(mix, 2, 8, cov_scale=1.5) and both.get_chain().shape == (3, 10, 8, 2)
    assert both.stats['cov'] == dict(scale=1.5, factor_fallbacks=0) and both.cov_fallbacks.shape == (3,)
    for e, stream in enumerate([4, 1, 2]):
        single = E.EnsembleSampler(vega, 8, seed=5, stream=stream, driver='python', moves=mix, cov_scale=1.5).run(10)
        member = both.member(e)
        assert np.array_equal(member.get_chain(), single.get_chain()) and np.array_equal(member.accepted, single.accepted)
        assert member.stats['moves'] == single.stats['moves'] and member.moves == single.moves
        assert member.stats['cov'] == single.stats['cov'] == dict(scale=1.5, factor_fallbacks=0)
        counts = single.stats['moves']
        assert list(counts) == ['stretch', 'de', 'snooker', 'cov'] and len(counts) == 4
        assert sum(c['proposals'] for c in counts.values()) == single.stats['proposals'] == 80
        assert sum(c['accepted'] for c in counts.values()) == single.stats['accepted'] == int(single.accepted.sum())
        assert counts['cov']['proposals'] > 0
    pure = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves='cov').run(10)
    assert pure.stats['moves']['cov'] == dict(proposals=80, accepted=pure.stats['accepted']) and pure.stats['accepted'] > 0
    assert pure.stats['cov'] == dict(scale=2.38 / np.sqrt(2.0), factor_fallbacks=0)
    cut = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves='cov', segment=3).run(10)
    assert np.array_equal(cut.get_chain(), pure.get_chain())
    # without cov: three names and no 'cov' key, as ever
    three = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves=[('de', 0.8), ('snooker', 0.2), ('cov', 0.0)]).run(4)
    old = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves=[('de', 0.8), ('snooker', 0.2)]).run(4)
    assert list(three.stats['moves']) == ['stretch', 'de', 'snooker'] and 'cov' not in three.stats and not hasattr(three, 'cov_fallbacks')
    assert np.array_equal(three.get_chain(), old.get_chain()) and three.moves == old.moves
    # walkers that all sit on one point: the covariance is exactly 0, every half-step falls back and proposes the walker's own point
    stuck = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves='cov').run(3, start=np.full((8, 2), 0.5))
    assert stuck.stats['cov']['factor_fallbacks'] == 6 and np.all(stuck.get_chain() == 0.5)
    for kw, match in ((dict(moves='cov', ntemps=3), 'tempering'), (dict(moves=[('cov', 0.5), ('de', 0.5)], betas=[1.0, 0.5]), 'tempering')):
        with pytest.raises(ValueError, match=match):
            E.TemperedEnsemble(vega, 8, **kw)
    with pytest.raises(ValueError, match='slice'):
        E.EnsembleSampler(vega, 8, moves=['cov', 'slice'])
    with pytest.raises(ValueError, match='slice'):
        E.EnsembleSampler(vega, 8, moves='slice', cov_scale=1.0)
    with pytest.raises(ValueError, match='cov_scale'):
        E.EnsembleSet(vega, 2, 8, moves='de', cov_scale=0.5)
    with pytest.raises(ValueError, match='cov_scale'):
        E.EnsembleSampler(vega, 8, cov_scale=0.5)
    with pytest.raises(ValueError, match='4 walkers'):
        E.EnsembleSampler(_OneParameter(), 2, moves='cov')


class _OneParameter(_StandInVega):
    def __init__(self):
        super().__init__()
        self.sample_params = {'limits': {'a': (0.0, 1.0)}, 'values': {'a': 0.5}, 'errors': {'a': 0.03}}


def test_cov_settings_reach_the_samplers(tmp_path):
    """``build_sampler``, the replicas one after the other and ``together = True`` run the configured mixture with cov: both paths
    write the same records, these are the chains of a sampler built by hand, and the records carry the cov counts beside the
    moves' counts."""
    from vega_amd import replicas as rep
    folders = {}
    for tag, extra in (('seq', ''), ('tog', 'together = True\n')):
        out = tmp_path / tag
        out.mkdir()
        (out / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {out}\nname = run\ndriver = python\nwalkers = 8\nsteps = 30\nseed = 3\n'
                                      f'replicas = 2\nmoves = cov 0.7 snooker 0.3\ncov_scale = 1.4\n{extra}')
        run = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                                 make_vega=lambda config, device: _StandInVega(config))
        assert run.replicas == 2
        assert all(s.moves == E.resolve_moves([('cov', 0.7), ('snooker', 0.3)], 2, 8, cov_scale=1.4) for s in run.samplers)
        folders[tag] = out
    for r in range(2):
        seq, tog = (rep.load_record(rep.record_path(folders[tag], 'run', r)) for tag in ('seq', 'tog'))
        by_hand = E.EnsembleSampler(_StandInVega(), 8, seed=3, stream=r, driver='python', moves=[('cov', 0.7), ('snooker', 0.3)],
                                    cov_scale=1.4).run(30)
        assert np.array_equal(seq['chain'], by_hand.get_chain()) and np.array_equal(tog['chain'], by_hand.get_chain())
        for rec in (seq, tog):
            assert rec['stats']['moves_cov_proposals'] == by_hand.stats['moves']['cov']['proposals'] > 0
            assert rec['stats']['moves_cov_accepted'] == by_hand.stats['moves']['cov']['accepted']
            assert rec['stats']['cov_scale'] == 1.4 and rec['stats']['cov_factor_fallbacks'] == 0


def test_cov_struct_and_entries_match_the_library():
    """The new struct's layout (vmx_struct_size index 27; 26 stays vacant) agrees with the ctypes binding, and the library exports
    the two new entries with the documented argument counts."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(27) == C.sizeof(engine.EnsembleCov) == 24
    assert lib.vmx_struct_size(26) == -1 and lib.vmx_struct_size(28) == -1
    assert {'vmx_ensemble_run_many_cov', 'vmx_ensemble_cov_factor'} <= set(engine.EXPORTED_SYMBOLS)
    assert hasattr(lib, 'vmx_ensemble_run_many_cov') and hasattr(lib, 'vmx_ensemble_cov_factor')
    assert len(lib.vmx_ensemble_run_many_cov.argtypes) == len(lib.vmx_ensemble_run_many_moves.argtypes) + 2
    assert len(lib.vmx_ensemble_cov_factor.argtypes) == 8
    assert len(lib.vmx_ensemble_run_many_moves.argtypes) == len(lib.vmx_ensemble_run_many.argtypes) + 1
