"""The ensemble sampler's differential-evolution and snooker moves and their mixtures without a GPU: the header the device kernel is
built from (vega_amd/csrc/vmx_ensemble.h, the second part), compiled with g++ under AddressSanitizer / UBSan into
tests/helpers/ensemble_moves_driver.cpp, against the NumPy restatement of vega_amd/ensemble.py bit for bit; the rule of the distinct
partners at the extremes of its words; the restatement's sampling of a correlated 10-dimensional Gaussian in a box under every pure
move and the 0.8 / 0.2 mixture; a chain that does not depend on the cut into segments; the ``[Ensemble] moves`` settings and their
way through ``build_sampler``, the replicas and ``together = True``; the new struct's layout."""
import configparser
import ctypes as C
import itertools
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vega_amd import ensemble as E

M64 = 2**64 - 1
MIXTURE = [('de', 0.8), ('snooker', 0.2)]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('ensemble_moves') / 'ensemble_moves_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_moves_driver.cpp')]
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


def _words(rng, k, size):
    """Random words; every fourth case takes each word from the extremes 0 and 2**64 - 1."""
    w = rng.integers(0, 2**64, size=size, dtype=np.uint64)
    if k % 4 == 0:
        w = rng.choice(np.array([0, M64], dtype=np.uint64), size=size)
    return w


# ------------------------------------------------------------------ the header against the restatement
def test_block_b_uses_the_documented_counter(driver):
    got = _ask(driver, [f'B {i} {s} {h} {seed:x} {stream:x}' for i, s, h, seed, stream in [(0, 0, 0, 0, 0), (5, 17, 1, 9, 2), (1055, 2**40, 1, M64, 7)]])
    for line, (i, s, h, seed, stream) in zip(got, [(0, 0, 0, 0, 0), (5, 17, 1, 9, 2), (1055, 2**40, 1, M64, 7)]):
        c = i | (s << 64) | (h << 128) | (1 << 192)
        ref = np.random.Philox(key=np.array([seed, stream], dtype=np.uint64), counter=c - 1).random_raw(4)
        assert [int(t, 16) for t in line.split()] == [int(v) for v in ref]
        assert np.array_equal(E.move_blocks(i + 1, s, h, seed, stream)[i], ref)
        assert not np.array_equal(E.step_blocks(i + 1, s, h, seed, stream)[i], ref)


WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.8, 0.2), (0.3, 0.4, 0.3), (0.0, 3.0, 0.0), (0.1, 0.0, 0.7),
           (0.4, 0.0, 0.0), (1e-300, 1e-300, 1e-300)]


def test_thresholds_choice_and_indices_bitwise(driver):
    """The thresholds of a set of weights, the move they choose from a word and the three partners: the header equals the
    restatement on random words and on the word extremes; a pure move is chosen by every word, the extremes included."""
    got = _ask(driver, ['T ' + ' '.join(map(_hx, p)) for p in WEIGHTS])
    ts = []
    for line, p in zip(got, WEIGHTS):
        t0, t1 = E.move_thresholds(p)
        assert [int(t, 16) for t in line.split()] == [_bits(t0), _bits(t1)], p
        ts.append((t0, t1))
    for k, p in enumerate(WEIGHTS[:3] + WEIGHTS[5:6] + WEIGHTS[7:8]):        # (pure moves of any weight)
        t0, t1 = E.move_thresholds(p)
        choice = E.move_choice(np.array([0, M64, 2**63, 12345], dtype=np.uint64), t0, t1)
        assert np.all(choice == int(np.argmax(p))), p
    rng = np.random.default_rng(1)
    cases, lines = [], []
    for k in range(600):
        t0, t1 = ts[k % len(ts)]
        H = int(rng.choice([1, 2, 3, 4, 5, 7, 32, 1056, int(rng.integers(3, 2**31))]))
        w = _words(rng, k, 4)
        cases.append((t0, t1, H, w))
        lines.append(f'M {_hx(t0)} {_hx(t1)} {H} ' + ' '.join(f'{int(v):x}' for v in w))
    seen = set()
    for line, (t0, t1, H, w) in zip(_ask(driver, lines), cases):
        move, j1, j2, j3 = (int(t) for t in line.split())
        assert move == int(E.move_choice(w[3:4], t0, t1)[0])
        seen.add(move)
        r1 = E.partner(w[0:1], H).astype(np.int64)
        assert j1 == int(r1[0]) and 0 <= j1 < H
        if H >= 2:
            r2 = E.partner2(w[1:2], H, r1)
            assert j2 == int(r2[0]) and 0 <= j2 < H and j2 != j1
        if H >= 3:
            r3 = E.partner3(w[2:3], H, r1, r2)
            assert j3 == int(r3[0]) and 0 <= j3 < H and len({j1, j2, j3}) == 3
    assert seen == {0, 1, 2}


@pytest.mark.parametrize('H', [3, 4, 5])
def test_three_indices_are_distinct_at_the_word_extremes(driver, H):
    combos = list(itertools.product((0, M64), repeat=3))
    got = _ask(driver, [f'M {_hx(0.0)} {_hx(0.0)} {H} {a:x} {b:x} {c:x} 0' for a, b, c in combos])
    for line, (a, b, c) in zip(got, combos):
        _, j1, j2, j3 = (int(t) for t in line.split())
        assert all(0 <= j < H for j in (j1, j2, j3)) and len({j1, j2, j3}) == 3, (a, b, c)
        r1 = E.partner(np.array([a], dtype=np.uint64), H).astype(np.int64)
        r2 = E.partner2(np.array([b], dtype=np.uint64), H, r1)
        r3 = E.partner3(np.array([c], dtype=np.uint64), H, r1, r2)
        assert (j1, j2, j3) == (int(r1[0]), int(r2[0]), int(r3[0]))
    if H == 3:      # (the three partners are the whole other half)
        assert all({int(t) for t in line.split()[1:]} == {0, 1, 2} for line in got)


def test_two_indices_are_distinct_in_a_half_of_two(driver):
    combos = list(itertools.product((0, M64, 2**63, 2**63 - 1), repeat=2))
    got = _ask(driver, [f'M {_hx(0.0)} {_hx(1.0)} 2 {a:x} {b:x} 0 0' for a, b in combos])
    for line, (a, b) in zip(got, combos):
        move, j1, j2, _ = (int(t) for t in line.split())
        assert move == E.MOVE_DE and {j1, j2} == {0, 1}
        r1 = E.partner(np.array([a], dtype=np.uint64), 2).astype(np.int64)
        assert (j1, j2) == (int(r1[0]), int(E.partner2(np.array([b], dtype=np.uint64), 2, r1)[0]))


def _rows(rng, n):
    scale = 10 ** rng.uniform(-3, 3)
    centre = rng.normal(size=n) * scale
    return [centre + rng.normal(size=n) * scale * 10 ** rng.uniform(-4, 0) for _ in range(4)]


@pytest.mark.parametrize('n', [1, 2, 5, 32, 64])
def test_de_proposals_bitwise(driver, n):
    rng = np.random.default_rng(100 + n)
    cases, lines = [], []
    for k in range(200):
        gamma0 = float(rng.choice([2.38 / np.sqrt(2 * n), 1.0, rng.random() + 0.1]))
        sigma = float(rng.choice([1e-5, 0.0, 0.3]))
        w = _words(rng, k, 2)
        s, c1, c2, _ = _rows(rng, n)
        cases.append((gamma0, sigma, w, s, c1, c2))
        lines.append(' '.join(['D', _hx(gamma0), _hx(sigma), f'{int(w[0]):x}', f'{int(w[1]):x}', str(n), *map(_hx, s), *map(_hx, c1),
                               *map(_hx, c2)]))
    for line, (gamma0, sigma, w, s, c1, c2) in zip(_ask(driver, lines), cases):
        tok = [int(t, 16) for t in line.split()]
        gamma = E.de_gamma(gamma0, sigma, w[0:1], w[1:2])
        assert tok[0] == _bits(gamma[0])
        assert gamma0 * (1 - sigma) <= gamma[0] <= gamma0 * (1 + sigma)
        assert tok[1:] == [_bits(v) for v in E.de_propose(s[None], c1[None], c2[None], gamma)[0]]


@pytest.mark.parametrize('n', [1, 2, 5, 32, 64])
def test_snooker_proposals_bitwise(driver, n):
    """Proposal, factor and whether it is one: random rows, rows whose walker sits on its partner (norm == 0: rejected, the
    walker's own position, nothing NaN), rows whose two projections are equal (the walker's own position, factor 0, a
    proposal) and rows whose proposal lands on the partner exactly (norm > 0, a factor that is not finite: rejected)."""
    rng = np.random.default_rng(200 + n)
    cases, lines = [], []
    for k in range(200):
        gamma_s = float(rng.choice([1.7, 1.0, 2.0 * rng.random() + 0.05]))
        s, z, z1, z2 = _rows(rng, n)
        if k % 10 == 3:
            z = s.copy()
        if k % 10 == 7:
            z1 = z2.copy()           # (p == 0: the proposal is the walker's own position, the factor 0)
        if k % 10 == 9:
            # y == z in exact arithmetic: d = (1, 0, ..), norm = 1, p = z1[0] - z2[0] = -1, gamma_s = 1, y = s - d = z
            gamma_s, z = 1.0, np.zeros(n)
            s, z1, z2 = np.eye(n)[0], rng.normal(size=n), rng.normal(size=n)
            z1[0], z2[0] = 0.0, 1.0
        cases.append((gamma_s, s, z, z1, z2))
        lines.append(' '.join(['S', _hx(gamma_s), str(n), *map(_hx, s), *map(_hx, z), *map(_hx, z1), *map(_hx, z2)]))
    n_ok = 0
    for k, (line, (gamma_s, s, z, z1, z2)) in enumerate(zip(_ask(driver, lines), cases)):
        tok = line.split()
        y, factor, ok = E.snooker_propose(s[None], z[None], z1[None], z2[None], gamma_s)
        assert (tok[0] == '1') == bool(ok[0]), k
        if ok[0]:
            assert int(tok[1], 16) == _bits(factor[0]), k
        else:
            assert not np.isfinite(struct.unpack('<d', struct.pack('<Q', int(tok[1], 16)))[0]) or int(tok[1], 16) == _bits(factor[0])
        assert [int(t, 16) for t in tok[2:]] == [_bits(v) for v in y[0]], k
        if k % 10 == 3:
            assert not ok[0] and np.array_equal(y[0], s) and factor[0] == 0.0
        if k % 10 == 7:
            assert ok[0] and np.array_equal(y[0], s) and factor[0] == 0.0
        if k % 10 == 9:
            assert not ok[0] and np.array_equal(y[0], z) and not np.isfinite(factor[0])
            assert not np.isfinite(struct.unpack('<d', struct.pack('<Q', int(tok[1], 16)))[0])
        n_ok += bool(ok[0])
    assert 150 <= n_ok <= 160


def test_snooker_with_a_walker_on_its_partner_is_rejected():
    """norm == 0 through the half-step: not inside, the proposal the walker's own position, and the decision a rejection."""
    x = np.tile(np.array([[0.1, 0.2, 0.3]]), (12, 1))
    moves = E.resolve_moves('snooker', 3, 12)
    y, inside, factor, b = E.half_step_proposals(x, 0, 0, 2.0, 1, 0, np.full(3, -1.0), np.full(3, 1.0), moves)
    assert not inside.any() and np.array_equal(y, x[:6]) and np.all(factor == 0.0) and np.all(np.isfinite(y))
    assert not E.accept(inside, np.ones(6, dtype=bool), factor, np.zeros(6), np.zeros(6), b[:, 2]).any()


# ------------------------------------------------------------------ the python driver
def _gaussian_problem(n=10):
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
    kw = {} if moves == 'default' else dict(moves=E.resolve_moves(moves, n, W))
    for k in (segments or [steps]):
        ch, cl, st = E.python_steps(x, lnl, acc, step, k, thin, a, seed, 0, lo, hi, -3.0, evaluate, **kw)
        chains.append(ch), lnls.append(cl), stats.append(st)
        step += k
    return np.concatenate(chains), np.concatenate(lnls), acc, stats


def test_the_pure_stretch_mixture_is_the_default_run():
    mean, cov, lo, hi = _gaussian_problem()
    one = _run_python(mean, cov, lo, hi, 24, 40, 'default')
    for moves in ('stretch', [('stretch', 0.4)], None):
        two = _run_python(mean, cov, lo, hi, 24, 40, moves)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert one[3][0]['accepted'] > 0


@pytest.mark.parametrize('moves', ['de', 'snooker', MIXTURE, [('stretch', 0.3), ('de', 0.4), ('snooker', 0.3)]], ids=str)
def test_the_chain_is_independent_of_the_cut(moves):
    mean, cov, lo, hi = _gaussian_problem()
    one = _run_python(mean, cov, lo, hi, 24, 60, moves, thin=3)
    two = _run_python(mean, cov, lo, hi, 24, 60, moves, thin=3, segments=[31, 29])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert one[0].shape == (20, 24, 10) and one[2].sum() > 0
    other = _run_python(mean, cov, lo, hi, 24, 60, 'default', thin=3)
    assert not np.array_equal(one[0], other[0])


@pytest.fixture(scope='module')
def truncated_moments():
    """Mean and covariance of the Gaussian in its box, by rejection sampling (3e6 draws: their own error is a few 1e-4 sd)."""
    mean, cov, lo, hi = _gaussian_problem()
    draws = np.random.default_rng(5).multivariate_normal(mean, cov, size=3_000_000)
    draws = draws[np.all((draws >= lo) & (draws <= hi), axis=1)]
    return draws.mean(axis=0), np.cov(draws.T)


@pytest.mark.parametrize('moves', ['stretch', 'de', 'snooker', MIXTURE], ids=str)
def test_python_driver_samples_a_clipped_gaussian(moves, truncated_moments):
    """A correlated 10-D Gaussian in a box that clips one tail, under every pure move and the 0.8 / 0.2 mixture: no sample outside
    the box; mean and covariance of the chain match the truncated Gaussian's within 5 Monte-Carlo standard errors at N / tau_max,
    tau measured on the chain.  (Seed and length were checked to give n_eff > 100 for every case: 1.1e3 at the least.)"""
    mean, cov, lo, hi = _gaussian_problem()
    W, steps, burn = 64, 2500, 500
    chain, lnl, acc, _ = _run_python(mean, cov, lo, hi, W, steps, moves)
    assert np.all(chain >= lo) and np.all(chain <= hi)
    post = chain[burn:]
    tau = E.integrated_time(post)
    m_ref, c_ref = truncated_moments
    flat = post.reshape(-1, mean.size)
    n_eff = flat.shape[0] / tau.max()
    print(moves, 'tau', tau.max(), 'n_eff', n_eff, 'acceptance', acc.mean() / steps)
    assert n_eff > 100, tau
    sd = np.sqrt(np.diag(c_ref))
    assert np.all(np.abs(flat.mean(axis=0) - m_ref) < 5 * sd / np.sqrt(n_eff)), ((flat.mean(axis=0) - m_ref) / sd, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - c_ref) < tol), ((np.cov(flat.T) - c_ref) / np.outer(sd, sd), n_eff)
    assert abs(m_ref[2] - mean[2]) > 0.1 * sd[2]         # (the clipped tail moved the mean: the box matters)
    assert 0.05 < acc.mean() / steps < 0.9


# ------------------------------------------------------------------ the arguments and the settings
def test_resolve_moves():
    d = E.resolve_moves('de', 8, 32)
    assert d == dict(weights=(0.0, 1.0, 0.0), gamma0=2.38 / np.sqrt(16.0), sigma=1e-5, gamma_s=1.7)
    d = E.resolve_moves(MIXTURE, 2, 6, gamma0=0.5, sigma=0.0, gamma_s=2.0)
    assert d == dict(weights=(0.0, 0.8, 0.2), gamma0=0.5, sigma=0.0, gamma_s=2.0)
    assert E.resolve_moves(d, 2, 6) == d
    assert E.resolve_moves(None, 2, 6) is None
    assert E.resolve_moves([('de', 1.0), ('de', 2.0), 'stretch'], 2, 4)['weights'] == (1.0, 3.0, 0.0)
    for bad in (dict(moves='walk'), dict(moves=[('de', -1.0)]), dict(moves=[('de', 0.0)]), dict(moves=[('de', np.nan)]),
                dict(moves=[('de', np.inf)]), dict(moves='snooker', walkers=4), dict(moves='de', walkers=2),
                dict(moves='de', gamma0=0.0), dict(moves='de', gamma0=np.inf), dict(moves='snooker', gamma_s=-1.0),
                dict(moves='de', sigma=-1e-3), dict(moves='de', sigma=np.nan), dict(moves=None, gamma0=1.0)):
        args = dict(dict(n=2, walkers=8), **bad)
        with pytest.raises(ValueError):
            E.resolve_moves(**args)


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'


def test_moves_settings_parse(tmp_path):
    base = f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\n'
    plain = E.sampler_settings(_config(base), SAMPLE)
    assert plain == dict(sampler='Ensemble', path=tmp_path, name='ensemble', walkers=8, steps=1000, seed=0, a=2.0, thin=1, init='ball',
                         init_scale=1.0, driver='device')            # (no moves: exactly the dict of ever)
    for text, want in (('moves = de 0.8 snooker 0.2\n', dict(moves=[('de', 0.8), ('snooker', 0.2)])),
                       ('moves = de\n', dict(moves=[('de', 1.0)])),
                       ('moves = snooker\n', dict(moves=[('snooker', 1.0)])),
                       ('moves = stretch\n', dict(moves=[('stretch', 1.0)])),
                       ('moves = stretch 0.3, de 0.4, snooker 0.3\n', dict(moves=[('stretch', 0.3), ('de', 0.4), ('snooker', 0.3)])),
                       ('moves = de snooker 0.25\n', dict(moves=[('de', 1.0), ('snooker', 0.25)])),
                       ('moves = de 0.8 snooker 0.2\ngamma0 = 0.7\nde_sigma = 1e-4\nsnooker_gamma = 1.5\n',
                        dict(moves=[('de', 0.8), ('snooker', 0.2)], gamma0=0.7, de_sigma=1e-4, snooker_gamma=1.5)),
                       ('moves = snooker\nsnooker_gamma = 2\n', dict(moves=[('snooker', 1.0)], snooker_gamma=2.0))):
        got = E.sampler_settings(_config(base + text), SAMPLE)
        assert got == dict(plain, **want), text
    cfg = E.sampler_settings(_config(base + 'moves = de 0.8 snooker 0.2\nde_sigma = 1e-4\n'), SAMPLE)
    assert E.moves_arguments(cfg) == dict(moves=[('de', 0.8), ('snooker', 0.2)], sigma=1e-4) and E.moves_arguments(plain) == {}


@pytest.mark.parametrize('text, match', [
    ('walkers = 8\nmoves = walk\n', 'unknown move'),
    ('walkers = 8\nmoves = de 0.8 kde 0.2\n', 'unknown move'),
    ('walkers = 8\nmoves = de -0.5 snooker 1\n', 'not negative'),
    ('walkers = 8\nmoves = de 0 snooker 0\n', 'positive sum'),
    ('walkers = 8\nmoves = 0.5 de\n', 'follows the name'),
    ('walkers = 8\nmoves = de 0.5 0.5\n', 'follows the name'),
    ('walkers = 8\nmoves =\n', 'at least one'),
    ('walkers = 4\nmoves = de 0.8 snooker 0.2\n', 'snooker'),
    ('walkers = 4\nmoves = snooker\n', 'at least 6 walkers'),
    ('walkers = 8\nmoves = de\ngamma0 = 0\n', 'gamma0'),
    ('walkers = 8\nmoves = de\nde_sigma = -1\n', 'sigma'),
    ('walkers = 8\nmoves = de\nsnooker_gamma = much\n', 'snooker_gamma'),
    ('walkers = 8\ngamma0 = 0.5\n', 'no moves'),
])
def test_moves_settings_refusals(tmp_path, text, match):
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


def test_sampler_classes_take_moves_and_count_them():
    """``EnsembleSampler`` and ``EnsembleSet`` with the mixture through the python driver: the set's member e is the single run
    on its stream, ``moves='stretch'`` is the run without moves, and ``stats['moves']`` counts every proposal under its move
    and - with a row for every step - every acceptance."""
    vega = _StandInVega()
    mix = [('stretch', 0.3), ('de', 0.4), ('snooker', 0.3)]
    both = E.EnsembleSet(vega, 3, 8, streams=[4, 1, 2], seed=5, driver='python', segment=4, moves=mix).run(10)
    assert both.moves == E.resolve_moves(mix, 2, 8) and both.get_chain().shape == (3, 10, 8, 2)
    for e, stream in enumerate([4, 1, 2]):
        single = E.EnsembleSampler(vega, 8, seed=5, stream=stream, driver='python', moves=mix).run(10)
        member = both.member(e)
        assert np.array_equal(member.get_chain(), single.get_chain()) and np.array_equal(member.accepted, single.accepted)
        assert member.stats['moves'] == single.stats['moves'] and member.moves == single.moves
        counts = single.stats['moves']
        assert set(counts) == {'stretch', 'de', 'snooker'}
        assert sum(c['proposals'] for c in counts.values()) == single.stats['proposals'] == 80
        assert sum(c['accepted'] for c in counts.values()) == single.stats['accepted'] == int(single.accepted.sum())
        assert all(0 <= c['accepted'] <= c['proposals'] for c in counts.values())
    total = both.stats['moves']
    assert sum(c['proposals'] for c in total.values()) == 240 and sum(c['accepted'] for c in total.values()) == both.stats['accepted']
    plain = E.EnsembleSampler(vega, 8, seed=5, driver='python').run(10)
    pure = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves='stretch').run(10)
    assert np.array_equal(plain.get_chain(), pure.get_chain()) and np.array_equal(plain.get_log_lik(), pure.get_log_lik())
    assert 'moves' not in plain.stats and plain.moves is None
    assert pure.stats['moves']['stretch'] == dict(proposals=80, accepted=plain.stats['accepted'])
    assert pure.stats['moves']['de'] == pure.stats['moves']['snooker'] == dict(proposals=0, accepted=0)
    # (the count reads the moves of a whole segment at once: the words of every half-step, walker h H + k under half h)
    resolved = E.resolve_moves(mix, 2, 8)
    drawn = E.steps_moves(4, 3, 7, 5, 2, resolved)
    assert drawn.shape == (7, 8) and set(drawn.reshape(-1)) == {0, 1, 2}
    for i, s in enumerate(range(3, 10)):
        assert np.array_equal(drawn[i], np.concatenate([E.half_step_moves(4, h, s, 5, 2, resolved) for h in (0, 1)]))
    thinned = E.EnsembleSampler(vega, 8, seed=5, thin=2, driver='python', moves='de').run(10)
    assert thinned.stats['moves']['de'] == dict(proposals=80, accepted=None)         # (not every step is recorded)
    assert thinned.stats['moves'].unseen is None
    # the counts are made when they are read, once per state of the run, and follow the run
    assert isinstance(pure.stats['moves'], E.MoveCounts) and pure.stats['moves'].unseen == 0 and both.stats['moves'].unseen == 0
    again = pure.stats['moves']['stretch']
    assert pure.stats['moves']['stretch'] is again
    pure.run(5)
    assert pure.stats['moves']['stretch'] == dict(proposals=120, accepted=pure.stats['accepted'])
    # DE between walkers that all sit on one point proposes the walker's own position: accepted, and credited to no move
    stuck = E.EnsembleSampler(vega, 8, seed=5, driver='python', moves='de').run(3, start=np.full((8, 2), 0.5))
    assert stuck.stats['accepted'] == 24 and stuck.stats['moves']['de'] == dict(proposals=24, accepted=0)
    assert stuck.stats['moves'].unseen == 24
    with pytest.raises(ValueError, match='snooker'):
        E.EnsembleSampler(vega, 4, moves='snooker')
    with pytest.raises(ValueError, match='moves'):
        E.EnsembleSet(vega, 2, 8, gamma0=0.5)


def test_settings_reach_the_samplers(tmp_path):
    """``build_sampler``, the replicas one after the other and ``together = True`` run the configured mixture: through
    ``run_vega_sampler`` over the stand-in both paths write the same records, and these are the chains of a sampler built with
    the same moves by hand; without ``moves`` the records are other chains."""
    from vega_amd import replicas as rep
    folders = {}
    for tag, extra in (('seq', ''), ('tog', 'together = True\n'), ('plain', None)):
        out = tmp_path / tag
        out.mkdir()
        moves = '' if extra is None else 'moves = de 0.8 snooker 0.2\nsnooker_gamma = 1.5\n' + extra
        (out / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {out}\nname = run\ndriver = python\nwalkers = 8\nsteps = 30\nseed = 3\n'
                                      f'replicas = 2\n{moves}')
        run = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                                 make_vega=lambda config, device: _StandInVega(config))
        assert run.replicas == 2
        assert all(s.moves == (None if extra is None else E.resolve_moves(MIXTURE, 2, 8, gamma_s=1.5)) for s in run.samplers)
        folders[tag] = out
    for r in range(2):
        seq, tog, plain = (rep.load_record(rep.record_path(folders[tag], 'run', r)) for tag in ('seq', 'tog', 'plain'))
        by_hand = E.EnsembleSampler(_StandInVega(), 8, seed=3, stream=r, driver='python', moves=MIXTURE, gamma_s=1.5).run(30)
        assert np.array_equal(seq['chain'], by_hand.get_chain()) and np.array_equal(tog['chain'], by_hand.get_chain())
        assert not np.array_equal(plain['chain'], by_hand.get_chain())
        assert seq['stats']['moves_de_proposals'] == by_hand.stats['moves']['de']['proposals'] == tog['stats']['moves_de_proposals']
        assert seq['stats']['moves_snooker_accepted'] == by_hand.stats['moves']['snooker']['accepted']
        assert not any(key.startswith('moves') for key in plain['stats'])


def test_moves_struct_matches_the_library():
    """The new struct's layout (vmx_struct_size index 23) agrees with the ctypes binding, and the entry is bound."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(23) == C.sizeof(engine.EnsembleMoves) == 56
    assert len(lib.vmx_ensemble_run_many_moves.argtypes) == len(lib.vmx_ensemble_run_many.argtypes) + 1
    assert 'vmx_ensemble_run_many_moves' in engine.EXPORTED_SYMBOLS and hasattr(lib, 'vmx_ensemble_run_many_moves')
