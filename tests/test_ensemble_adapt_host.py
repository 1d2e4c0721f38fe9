"""The adaptive temperature ladders of the ensemble sampler without a GPU: the rule the device kernel is built from
(vega_amd/csrc/vmx_ensemble.h, the fourth part), compiled with g++ under AddressSanitizer / UBSan into
tests/helpers/ensemble_adapt_driver.cpp, against the NumPy restatement of vega_amd/ensemble.py bit for bit; the restatement on a
narrow 4-D Gaussian whose default ladder does not reach its last rung; a chain and a ladder that do not depend on the cut into
calls; adaptation that never fires; the evidence of adaptive runs; the ``[Ensemble] adapt`` settings and their way through
``run_vega_sampler`` over a stand-in; the new entry's binding."""
import configparser
import math
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vega_amd import ensemble as E
from vega_amd import smc


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('ensemble_adapt') / 'ensemble_adapt_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_adapt_driver.cpp')]
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


# ------------------------------------------------------------------ the header against the restatement
def _random_ladder(rng, T, last):
    """1 > ... > last: the inner rungs geometric with random steps, or - every third - uniform."""
    if rng.integers(3) == 0:
        inner = np.sort(rng.uniform(last, 1.0, T - 2))[::-1]
    else:
        inner = np.exp(-np.cumsum(rng.uniform(0.05, 1.5, T - 2) * 8.0 / max(T, 8)))
        inner = last + (1.0 - last) * inner
    b = np.concatenate([[1.0], inner, [last]])
    assert E.ladder_ok(b)
    return b


def _adjust_cases():
    rng = np.random.default_rng(11)
    cases = []
    for T in (3, 4, 8, 64):
        for last in (0.0, float(rng.uniform(1e-4, 1e-2))):
            for W in (2, 16, 2112):
                counts = [np.zeros(T - 1, dtype=np.int64), np.full(T - 1, W), np.arange(T - 1) % 2 * W, (np.arange(T - 1) + 1) % 2 * W,
                          rng.integers(0, W + 1, T - 1), rng.integers(0, W + 1, T - 1)]
                for k, acc in enumerate(counts):
                    time = (0, 10**6)[k % 2] if W != 16 else (10**6, 0)[k % 2]
                    lag, tau = ((5.0, 2.0), (10000.0, 100.0))[(k // 2 + T) % 2]
                    cases.append((_random_ladder(rng, T, last), acc, W, time, lag, tau))
    return cases


def _ask_adjust(driver, cases):
    lines = [f'J {len(b)} {W} {time} {_hx(lag)} {_hx(tau)} ' + ' '.join(_hx(v) for v in b) + ' ' + ' '.join(str(int(a)) for a in acc)
             for b, acc, W, time, lag, tau in cases]
    out = []
    for line in _ask(driver, lines):
        tok = line.split()
        out.append((int(tok[0]), [int(v, 16) for v in tok[1:]]))
    return out


def test_ladder_adjust_bitwise(driver):
    """Random ladders of 3, 4, 8 and 64 rungs that end at 0 and above it, swap ratios all 0, all 1, alternating and random, at
    times 0 and 1e6 with (lag, time) (5, 2) and (10000, 100): the header and the restatement give the same ladder bit for bit;
    the first and the last beta never move; equal ratios move nothing by more than rounding; what comes out is a ladder."""
    cases = _adjust_cases()
    moved_by = []
    for (moved, got), (b, acc, W, time, lag, tau) in zip(_ask_adjust(driver, cases), cases):
        new, skipped = E.ladder_adjust(b, acc, W, time, lag, tau)
        assert moved == 1 - skipped
        assert got == [_bits(v) for v in new], (b, acc, W, time, lag, tau)
        assert new[0] == 1.0 and _bits(new[-1]) == _bits(b[-1]) and E.ladder_ok(new)
        if np.all(acc == acc[0]):           # (exp(0) = 1: the gaps stay, the sum is re-associated)
            np.testing.assert_allclose(new, b, rtol=1e-13)
        moved_by.append(np.max(np.abs(new[1:-1] / b[1:-1] - 1.0)))
    assert len(cases) == 4 * 2 * 3 * 6 and max(moved_by) > 0.3 and sum(m > 1e-3 for m in moved_by) > 40
    # a ratio above the next one widens the gap in 1 / beta (that pair swaps too easily: its rungs move apart)
    new, _ = E.ladder_adjust([1.0, 0.5, 0.25, 0.0], [16, 0, 0], 16, 0, 5.0, 2.0)
    assert new[1] < 0.5
    new, _ = E.ladder_adjust([1.0, 0.5, 0.25, 0.0], [0, 16, 16], 16, 0, 5.0, 2.0)
    assert new[1] > 0.5


def test_the_guard_keeps_a_ladder_that_would_cross_its_positive_last_rung(driver):
    """beta = (1, 0.5, 0.4), the first pair swapping always and the second never, kappa = 1 / 2: the new middle beta would be
    1 / (1 + e^0.5) = 0.378 < 0.4.  Header and restatement return the ladder unchanged and count one skipped sweep; with the last
    rung at 0 the same counts move the ladder."""
    b = np.array([1.0, 0.5, 0.4])
    assert 1.0 / (1.0 + math.exp(0.5)) < 0.4
    case = (b, np.array([16, 0]), 16, 0, 5.0, 2.0)
    (moved, got), = _ask_adjust(driver, [case])
    new, skipped = E.ladder_adjust(*case)
    assert moved == 0 and skipped == 1 and got == [_bits(v) for v in b] and np.array_equal(new, b)
    free = (np.array([1.0, 0.5, 0.0]),) + case[1:]
    (moved, got), = _ask_adjust(driver, [free])
    new, skipped = E.ladder_adjust(*free)
    assert moved == 1 and skipped == 0 and got == [_bits(v) for v in new] and abs(new[1] - 1.0 / (1.0 + math.exp(0.5))) < 1e-12
    # a tau so small that the exponential overflows: 1 / inf = 0 is not above the last rung either
    wild = (np.array([1.0, 0.5, 0.25, 0.0]), np.array([16, 0, 0]), 16, 0, 5.0, 1e-4)
    (moved, got), = _ask_adjust(driver, [wild])
    new, skipped = E.ladder_adjust(*wild)
    assert moved == 0 and skipped == 1 and np.array_equal(new, wild[0]) and got == [_bits(v) for v in wild[0]]


def test_the_small_decisions_bitwise(driver):
    xs = [0.0, -0.0, 0.5, -0.5, 1.0 / 3.0, 0.01, -0.01, 1e-300, 50.0, -50.0, 709.0, 709.5, -745.0, -746.0, float('nan')]
    for line, x in zip(_ask(driver, [f'E {_hx(x)}' for x in xs]), xs):
        assert int(line, 16) == _bits(smc.pexp(x)[0]), x
    oks = [(3, 1, 5.0, 2.0), (2, 1, 5.0, 2.0), (64, 7, 1e4, 100.0), (65, 1, 5.0, 2.0), (4, 0, 5.0, 2.0), (4, -1, 5.0, 2.0),
           (4, 1, 0.0, 2.0), (4, 1, 5.0, 0.0), (4, 1, -1.0, 2.0), (4, 1, float('inf'), 2.0), (4, 1, 5.0, float('nan'))]
    got = _ask(driver, [f'K {T} {every} {_hx(lag)} {_hx(tau)}' for T, every, lag, tau in oks])
    assert [int(v) for v in got] == [int(E.adapt_ok(*c)) for c in oks] == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    steps = [(s, every, until) for s in (0, 1, 2, 5, 6, 2**40 - 1) for every in (1, 3, 7) for until in (-1, 0, 3, 6, 2**40)]
    for line, (s, every, until) in zip(_ask(driver, [f'M {s} {every} {until}' for s, every, until in steps]), steps):
        time, due = (int(v) for v in line.split())
        assert time == E.sweep_time(s, every) == (s + 1) // every - 1
        assert due == int(E.adapt_due(s, until)) == int(until < 0 or s < until)


# ------------------------------------------------------------------ the python driver on a callable likelihood
SIGMA, N, W16 = 0.005, 4, 16
LOG_Z = 2.0 * math.log(2.0 * math.pi * SIGMA**2)          # a 4-D Gaussian of sigma 0.005 in the unit box, log_norm 0: -17.51752
UNIT = (np.zeros(N), np.ones(N))


def _gauss(rows, h=None):
    return np.sum((rows - 0.5)**2, axis=1) / SIGMA**2, np.zeros(rows.shape[0], dtype=np.int32)


def _start(shape, seed):
    return np.clip(0.5 + SIGMA * np.random.default_rng(seed).standard_normal(shape + (N,)), *UNIT)


def _run(betas, W, segments, seed=3, G=1, thin=1, swap_every=1, moves=None, adapt=None):
    """G ladders from ``betas`` [T] through python_steps_pt (``adapt`` None) or python_steps_pt_adapt (``adapt`` = (lag, time,
    adapt_until)) in the calls ``segments``: dict of the joined results."""
    T = len(betas)
    x = _start((G, T, W), seed)
    lnl = E.log_lik(0.0, _gauss(x.reshape(-1, N))[0]).reshape(G, T, W)
    acc = np.zeros((G, T, W), dtype=np.int64)
    streams = 64 * np.arange(G)[:, None] + np.arange(T)[None, :]
    ladders = np.tile(np.asarray(betas, dtype=np.float64), (G, 1))
    parts, step = [], 0
    for k in segments:
        if adapt is None:
            parts.append(E.python_steps_pt(x, lnl, acc, step, k, thin, swap_every, 2.0, seed, betas, streams, UNIT[0], UNIT[1], 0.0,
                                           _gauss, moves))
        else:
            parts.append(E.python_steps_pt_adapt(x, lnl, acc, step, k, thin, swap_every, 2.0, seed, ladders, streams, UNIT[0], UNIT[1],
                                                 0.0, _gauss, moves, adaptation_lag=adapt[0], adaptation_time=adapt[1],
                                                 adapt_until=adapt[2]))
            assert parts[-1][5] is ladders
        step += k
    out = dict(chain=np.concatenate([p[0] for p in parts], axis=2), lnl=np.concatenate([p[1] for p in parts], axis=2), acc=acc,
               per=sum(p[3] for p in parts), swaps=sum(p[4] for p in parts), part_swaps=[p[4] for p in parts], x=x, x_lnl=lnl,
               betas=ladders)
    if adapt is not None:
        out.update(hist=np.concatenate([p[6] for p in parts]), skipped=sum(p[7] for p in parts))
    return out


def _min_over_max(swaps):
    frac = swaps[0, :, 1] / swaps[0, :, 0]
    return float(frac.min() / frac.max()), frac


@pytest.fixture(scope='module')
def fixed_run():
    return _run(E.default_ladder(8), W16, [1500])


@pytest.fixture(scope='module')
def adapted_run():
    return _run(E.default_ladder(8), W16, [1500, 1500], adapt=(1000.0, 20.0, 1500))


def _evidence(run, first, betas):
    rows = run['lnl'].shape[2] - first
    return E.stepping_stone_evidence(betas, run['lnl'][0][:, first + rows // 4:])


def test_the_default_ladder_does_not_reach_its_last_rung(fixed_run):
    """T = 8, W = 16, seed 3, a sweep every step, 1500 steps on the ladder 1, 1/2, ..., 1/64, 0: the last pair hardly swaps, so
    min / max of the swap fractions is at most 0.05.  Measured: 0.51-0.53 and 0.0046 on the last pair, min / max 0.0087; log Z
    -17.84 +- 0.50."""
    ratio, frac = _min_over_max(fixed_run['swaps'])
    log_z, err = _evidence(fixed_run, 0, E.default_ladder(8))
    print('fixed ladder: swap fractions', frac, 'min / max', ratio, 'log Z', log_z, '+-', err, 'exact', LOG_Z)
    assert ratio <= 0.05


def test_the_adapted_ladder_swaps_evenly_and_gives_the_evidence(fixed_run, adapted_run):
    """The same run with 1500 adapting steps (lag 1000, time 20) and 1500 frozen ones: the frozen phase swaps at even rates
    (min / max >= 0.5); its stepping-stone evidence lies within 5 of its own err of the exact value, with err <= 0.15 and below
    the fixed ladder's.  Measured: the ladder 1, 0.30, 0.096, 0.030, 0.0089, 0.0026, 0.00068, 0; frozen fractions 0.23-0.29,
    min / max 0.80; log Z -17.457 +- 0.060, pull +1.0, against the fixed ladder's err of 0.50."""
    assert abs(LOG_Z - -17.51752) < 1e-5
    run = adapted_run
    ratio, frac = _min_over_max(run['part_swaps'][1])
    betas = run['betas'][0]
    log_z, err = _evidence(run, 1500, betas)
    _, fixed_err = _evidence(fixed_run, 0, E.default_ladder(8))
    print('adapted ladder', betas, 'frozen swap fractions', frac, 'min / max', ratio, 'log Z', log_z, '+-', err, 'pull',
          (log_z - LOG_Z) / err, 'fixed err', fixed_err, 'skipped', run['skipped'])
    assert ratio >= 0.5
    assert abs(log_z - LOG_Z) < 5 * err and err <= 0.15
    assert err < fixed_err
    # the record: a row per sweep, the ladder moving while it adapts and still afterwards, always a ladder
    hist = run['hist']
    assert hist.shape == (3000, 1, 8) and np.all(hist[:, :, 0] == 1.0) and np.all(hist[:, :, -1] == 0.0)
    assert all(E.ladder_ok(row[0]) for row in hist[::50])
    assert np.array_equal(hist[1499], hist[2999]) and np.array_equal(hist[2999, 0], betas) and not np.array_equal(hist[0], hist[1499])
    assert betas[-2] < 0.1 * E.default_ladder(8)[-2]          # (the ladder reaches down to the last rung)
    assert np.all(run['skipped'] == 0)


@pytest.mark.parametrize('swap_every', [1, 3])
def test_the_chain_and_the_ladder_do_not_depend_on_the_cut(swap_every):
    """60 steps in one call against 25 + 35: chain, lnL, swaps, betas and history bit for bit - the time of a sweep is a function
    of the global step.  The two ladders, on streams of their own, end different; adapt_until in the middle of a call stops the
    ladder there."""
    kw = dict(G=2, thin=2, swap_every=swap_every, adapt=(5.0, 2.0, -1), moves=E.resolve_moves([('stretch', 0.5), ('de', 0.5)], N, 8))
    one = _run(E.default_ladder(4), 8, [60], **kw)
    two = _run(E.default_ladder(4), 8, [25, 35], **kw)
    for key in ('chain', 'lnl', 'acc', 'per', 'swaps', 'x', 'x_lnl', 'betas', 'hist', 'skipped'):
        assert np.array_equal(one[key], two[key]), key
    assert one['hist'].shape == (60 // swap_every, 2, 4) and one['chain'].shape == (2, 4, 30, 8, N)
    assert not np.array_equal(one['betas'][0], one['betas'][1]) and np.array_equal(one['hist'][-1], one['betas'])
    assert np.max(np.abs(one['betas'][:, 1:3] / E.default_ladder(4)[1:3] - 1.0)) > 0.1
    until = _run(E.default_ladder(4), 8, [60], **dict(kw, adapt=(5.0, 2.0, 31)))
    last = 31 // swap_every - 1             # (the last sweep after a step below 31)
    assert np.array_equal(until['hist'][:last + 1], one['hist'][:last + 1]) and np.all(until['hist'][last:] == until['hist'][last])
    assert np.array_equal(until['chain'][:, :, :15], one['chain'][:, :, :15]) and not np.array_equal(until['chain'], one['chain'])


def test_the_driver_refuses_what_the_entry_refuses():
    for betas, every, lag, tau in (([1.0, 0.0], 1, 5.0, 2.0), ([1.0, 0.5, 0.0], 0, 5.0, 2.0), ([1.0, 0.5, 0.0], 1, 0.0, 2.0),
                                   ([1.0, 0.5, 0.0], 1, 5.0, float('inf')), ([1.0, 0.5, 0.5], 1, 5.0, 2.0)):
        T = len(betas)
        x = _start((1, T, 8), 3)
        with pytest.raises(ValueError):
            E.python_steps_pt_adapt(x, np.zeros((1, T, 8)), np.zeros((1, T, 8), dtype=np.int64), 0, 2, 1, every, 2.0, 3,
                                    np.array([betas]), np.arange(T)[None, :], UNIT[0], UNIT[1], 0.0, _gauss, adaptation_lag=lag,
                                    adaptation_time=tau)


# ------------------------------------------------------------------ the class and the launcher body over a stand-in
class _StandInEngine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 7
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1


class _StandInVega:
    """The surface of VegaInterface the samplers use, over a correlated Gaussian in (a, b) well inside its box."""
    param_names = ['a', 'fixed', 'b']
    mc_config = None
    COV = 0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]])

    def __init__(self, config=None):
        self.main_config = configparser.ConfigParser()
        self.main_config.optionxform = str
        if config is not None:
            self.main_config.read(config)
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _StandInEngine()
        self._icov = np.linalg.inv(self.COV)

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

    def derived_names(self):
        return []

    def chi2_batch(self, theta):
        d = np.asarray(theta, dtype=np.float64)[:, [0, 2]] - 0.5
        return np.einsum('ij,jk,ik->i', d, self._icov, d)

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        assert t.shape[0] <= self.engine.max_batch and mock_rows is None
        return torch.from_numpy(self.chi2_batch(t.numpy()))


EXACT = 1.25 + math.log(2.0 * math.pi * math.sqrt(np.linalg.det(_StandInVega.COV)))
ADAPT = dict(adapt=True, adaptation_lag=50, adaptation_time=5)


def test_adaptation_that_never_fires_is_the_fixed_run():
    vega = _StandInVega()
    fixed = E.TemperedEnsemble(vega, 8, ntemps=5, ladders=2, seed=3, driver='python').run(40)
    never = E.TemperedEnsemble(vega, 8, ntemps=5, ladders=2, seed=3, driver='python', adapt_steps=0, **ADAPT).run(40)
    assert np.array_equal(never.get_chain(rung=None), fixed.get_chain(rung=None))
    assert np.array_equal(never.get_log_lik(rung=None), fixed.get_log_lik(rung=None))
    assert np.array_equal(never.swaps, fixed.swaps) and np.array_equal(never.accepted, fixed.accepted)
    assert np.array_equal(never.current_betas, fixed.current_betas) and never.beta_history.shape == (0, 2, 5)
    assert np.array_equal(never.frozen_swap_fraction, never.swap_fraction)
    # the fixed run keeps what it had, and shows its ladder in the shapes of the adaptive one
    assert 'adapt_skipped' not in fixed.stats and np.array_equal(fixed.current_betas, np.tile(fixed.betas, (2, 1)))
    assert fixed.beta_history.shape == (0, 2, 5) and np.array_equal(fixed.frozen_swap_fraction, fixed.swap_fraction)
    assert never.log_evidence() == fixed.log_evidence()


def test_the_class_adapts_cuts_its_calls_and_reads_the_frozen_rows(tmp_path):
    vega = _StandInVega()
    kw = dict(ntemps=6, ladders=2, seed=3, thin=2, driver='python', adapt_steps=150, **ADAPT)
    s = E.TemperedEnsemble(vega, 8, **kw).run(400)
    assert s.stats['calls'] == 2 and s.step == 400 and s.recorded_rows == 200 and s.frozen_rows == (75, 125)
    assert s.beta_history.shape == (150, 2, 6) and np.array_equal(s.beta_history[-1], s.current_betas)
    assert not np.array_equal(s.current_betas[0], s.current_betas[1]) and not np.array_equal(s.current_betas[0], s.betas)
    assert np.all(s.current_betas[:, 0] == 1.0) and np.all(s.current_betas[:, -1] == 0.0)
    assert s.stats['adapt_skipped'].shape == (2,) and np.all(s.stats['adapt_skipped'] == 0)
    assert s.rung(2, ladder=1).beta == s.current_betas[1, 2] != s.betas[2]
    assert np.all(s.swaps[:, :, 0] == 400 * 8) and s.frozen_swap_fraction.shape == (2, 5)
    # however the run is cut, into calls of the user or segments of the class: the same chain and ladder
    cut = E.TemperedEnsemble(vega, 8, segment=37, **kw)
    cut.run(100).run(120).run(180)
    assert cut.stats['calls'] > 10
    for a, b in ((cut.get_chain(rung=None), s.get_chain(rung=None)), (cut.get_log_lik(rung=None), s.get_log_lik(rung=None)),
                 (cut.current_betas, s.current_betas), (cut.beta_history, s.beta_history), (cut.swaps, s.swaps),
                 (cut.frozen_swap_fraction, s.frozen_swap_fraction)):
        assert np.array_equal(a, b)
    # the frozen sweeps alone: the steps 150 .. 399 of a fixed run from the same state would count these
    frozen = cut._frozen_swaps
    assert np.all(frozen[:, :, 0] == 250 * 8) and np.all(frozen[:, :, 1] <= s.swaps[:, :, 1])
    # the evidence: only the frozen rows, with the final betas of the ladder asked for
    for g in range(2):
        lnl = s.get_log_lik(rung=None)[g]
        assert s.log_evidence(ladder=g) == E.stepping_stone_evidence(s.current_betas[g], lnl[:, 75 + 125 // 4:])
        assert s.log_evidence(ladder=g, discard=10) == E.stepping_stone_evidence(s.current_betas[g], lnl[:, 85:])
        assert s.log_evidence('ti', ladder=g) == E.thermodynamic_integration(s.current_betas[g], lnl[:, 75 + 125 // 4:].mean(axis=(1, 2)))
        log_z, err = s.log_evidence(ladder=g)
        print('ladder', g, s.current_betas[g], 'log Z', log_z, '+-', err, 'exact', EXACT)
        assert abs(log_z - EXACT) < 5 * err and err < 0.5
    # the stats file of an adaptive run, and back
    files = s.write(tmp_path, 'both')
    assert [[p.name for p in f] for f in files] == [[f'both_ladder{g}.txt', f'both_ladder{g}.paramnames', f'both_ladder{g}.stats']
                                                    for g in range(2)]
    stats = E.read_pt_stats(files[1][2])
    assert stats['log(Z)'] == s.log_evidence(ladder=1)[0] and stats['beta'] == list(s.current_betas[1]) and stats['steps'] == 400
    assert stats['swap fraction'] == list(s.swap_fraction[1]) and stats['frozen swap fraction'] == list(s.frozen_swap_fraction[1])
    assert stats['adapt_steps'] == 150 and stats['adaptation_lag'] == 50.0 and stats['adaptation_time'] == 5.0
    assert stats['adapt skipped'] == 0
    assert list(stats)[-5:] == ['adapt_steps', 'adaptation_lag', 'adaptation_time', 'adapt skipped', 'frozen swap fraction']


def test_the_evidence_of_a_ladder_that_still_moves_is_refused(tmp_path):
    vega = _StandInVega()
    s = E.TemperedEnsemble(vega, 8, ntemps=4, seed=3, driver='python', **ADAPT).run(30)
    assert s.beta_history.shape == (30, 1, 4) and s.frozen_rows == (30, 0) and np.all(np.isnan(s.frozen_swap_fraction))
    with pytest.raises(ValueError, match='adapt_steps'):
        s.log_evidence()
    with pytest.raises(ValueError, match='adapt_steps'):
        s.log_evidence('ti')
    said = []
    assert [p.name for p in s.write(tmp_path, 'moving', print_func=said.append)] == ['moving.txt', 'moving.paramnames']
    assert any('after the ladder froze' in line for line in said)
    late = E.TemperedEnsemble(vega, 8, ntemps=4, seed=3, driver='python', adapt_steps=29, **ADAPT).run(30)
    with pytest.raises(ValueError, match='adapt_steps'):
        late.log_evidence()
    late.run(1)
    assert late.frozen_rows == (29, 2) and late.log_evidence()[1] > 0.0
    for bad in (dict(ntemps=2), dict(ntemps=4, swap_every=0), dict(ntemps=4, adaptation_lag=0), dict(ntemps=4, adaptation_time=-1.0),
                dict(ntemps=4, adaptation_time=float('nan')), dict(ntemps=4, adapt_steps=-1)):
        with pytest.raises(ValueError):
            E.TemperedEnsemble(vega, 8, **dict(dict(adapt=True), **bad))


def test_a_fixed_run_writes_the_stats_file_it_wrote(tmp_path):
    s = E.TemperedEnsemble(_StandInVega(), 8, ntemps=4, seed=3, driver='python').run(20)
    text = s.write(tmp_path, 'fixed')[2].read_text().splitlines()
    assert [line.partition(' = ')[0] for line in text] == [
        'log(Z)', 'log(Z) error', 'log(Z) thermodynamic', 'log(Z) thermodynamic error', 'steps', 'walkers', 'swap_every', 'seed',
        'likelihood evaluations', 'beta', 'swap fraction']
    assert text[9] == 'beta = 1.0 0.5 0.25 0.0'


# ------------------------------------------------------------------ the settings
SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


def test_adapt_settings_parse(tmp_path):
    base = f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\nsteps = 100\n'
    plain = E.sampler_settings(_config(base + 'ntemps = 6\n'), SAMPLE)
    assert not {'adapt', 'adapt_steps', 'adaptation_lag', 'adaptation_time'} & set(plain)
    assert E.sampler_settings(_config(base + 'ntemps = 6\nadapt = True\n'), SAMPLE) == dict(plain, adapt=True, adapt_steps=50)
    got = E.sampler_settings(_config(base + 'ntemps = 3\nadapt = yes\nadapt_steps = 0\nadaptation_lag = 500\nadaptation_time = 7.5\n'),
                             SAMPLE)
    assert got == dict(plain, ntemps=3, adapt=True, adapt_steps=0, adaptation_lag=500.0, adaptation_time=7.5)
    assert E.sampler_settings(_config(base + 'ntemps = 6\nadapt = False\n'), SAMPLE) == dict(plain, adapt=False)
    assert E.sampler_settings(_config(base + 'ntemps = 6\nthin = 2\nadapt = True\nadapt_steps = 96\n'), SAMPLE)['adapt_steps'] == 96


@pytest.mark.parametrize('text, match', [
    ('adapt = True\n', 'no ntemps'), ('adapt_steps = 5\n', 'no ntemps'), ('adaptation_lag = 5\n', 'no ntemps'),
    ('adaptation_time = 5\n', 'no ntemps'),
    ('ntemps = 2\nadapt = True\n', 'ntemps >= 3'), ('ntemps = 4\nswap_every = 0\nadapt = True\n', 'swap_every >= 1'),
    ('ntemps = 4\nadapt = True\nadapt_steps = -1\n', 'adapt_steps'), ('ntemps = 4\nadapt = True\nadapt_steps = 101\n', 'adapt_steps'),
    ('ntemps = 4\nadapt = True\nadapt_steps = 99\n', 'two rows'), ('ntemps = 4\nthin = 2\nadapt = True\nadapt_steps = 98\n', 'two rows'),
    ('ntemps = 4\nadapt = True\nadapt_steps = some\n', 'whole number'), ('ntemps = 4\nadapt = perhaps\n', 'True or False'),
    ('ntemps = 4\nadapt = True\nadaptation_lag = 0\n', 'finite and positive'),
    ('ntemps = 4\nadapt = True\nadaptation_time = -2\n', 'finite and positive'),
    ('ntemps = 4\nadapt = True\nadaptation_time = inf\n', 'finite and positive'),
    ('ntemps = 4\nadapt_steps = 10\n', 'adapt is not True'), ('ntemps = 4\nadapt = False\nadaptation_lag = 10\n', 'adapt is not True'),
    ('ntemps = 4\nadapt = True\nreplicas = 2\n', 'replicas'), ('ntemps = 4\nadapt = True\ntogether = True\n', 'together'),
])
def test_adapt_settings_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\nsteps = 100\n{text}'), SAMPLE)


def test_run_vega_sampler_with_adapt_over_a_stand_in(tmp_path):
    (tmp_path / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {tmp_path}\nname = run\ndriver = python\nwalkers = 8\nsteps = 120\n'
                                       'seed = 3\nthin = 2\nntemps = 5\nbeta_min = 0.01\nadapt = True\nadaptation_lag = 50\n'
                                       'adaptation_time = 5\n')
    said = []
    run = E.run_vega_sampler(str(tmp_path / 'main.ini'), print_func=lambda *a: said.append(' '.join(map(str, a))), rank=0, world_size=1,
                             make_vega=lambda config, device: _StandInVega(config))
    assert isinstance(run, E.TemperedEnsemble) and run.adapt and run.adapt_steps == 60 and run.adaptation_lag == 50.0
    assert run.adaptation_time == 5.0 and run.beta_history.shape == (60, 1, 5) and run.frozen_rows == (30, 30)
    by_hand = E.TemperedEnsemble(_StandInVega(), 8, ntemps=5, beta_min=0.01, seed=3, thin=2, driver='python', adapt=True,
                                 adapt_steps=60, adaptation_lag=50, adaptation_time=5).run(120)
    assert np.array_equal(run.get_chain(rung=None), by_hand.get_chain(rung=None))
    assert np.array_equal(run.current_betas, by_hand.current_betas)
    log_z, err = run.log_evidence()
    assert f'log(Z) = {log_z} +- {err}' in said
    stats = E.read_pt_stats(tmp_path / 'run.stats')
    assert stats['log(Z)'] == log_z and stats['log(Z) error'] == err and stats['beta'] == list(run.current_betas[0])
    assert stats['beta'] != list(run.betas) and stats['adapt_steps'] == 60 and stats['adaptation_lag'] == 50.0
    assert stats['adaptation_time'] == 5.0 and stats['adapt skipped'] == int(run.stats['adapt_skipped'][0])
    assert stats['frozen swap fraction'] == list(run.frozen_swap_fraction[0]) and stats['swap fraction'] == list(run.swap_fraction[0])


def test_the_entry_is_bound():
    import ctypes as C

    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert 'vmx_ensemble_run_pt_adapt' in engine.EXPORTED_SYMBOLS and hasattr(lib, 'vmx_ensemble_run_pt_adapt')
    # the arguments of vmx_ensemble_run_pt, then the adaptation struct, the history and the guard's counts
    assert lib.vmx_ensemble_run_pt_adapt.argtypes[:-3] == lib.vmx_ensemble_run_pt.argtypes
    assert len(lib.vmx_ensemble_run_pt_adapt.argtypes) == len(lib.vmx_ensemble_run_pt.argtypes) + 3 == 25
    assert lib.vmx_struct_size(24) == C.sizeof(engine.EnsembleAdapt) == 32
    assert [name for name, _ in engine.EnsembleAdapt._fields_] == ['lag', 'time', 'adapt_until', 'flags', 'reserved']
    header = (REPO / 'include' / 'vegamx.h').read_text()
    assert 'int vmx_ensemble_run_pt_adapt(' in header and '} vmx_ensemble_adapt;' in header
    assert callable(engine.Engine.ensemble_run_pt_adapt)
