"""The ensemble sampler's parallel tempering without a GPU: the header the device kernels are built from
(vega_amd/csrc/vmx_ensemble.h, the third part), compiled with g++ under AddressSanitizer / UBSan into
tests/helpers/ensemble_pt_driver.cpp, against the NumPy restatement of vega_amd/ensemble.py bit for bit; the restatement on a
bimodal target a plain ensemble cannot cross; a chain that does not depend on the cut into calls; rungs without swaps that are the
plain ensembles; the stepping-stone and thermodynamic-integration evidences on exact draws of a 4-D Gaussian; the ``[Ensemble]
ntemps`` settings and their way through ``run_vega_sampler`` over a stand-in; the new entry's binding."""
import configparser
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
    exe = tmp_path_factory.mktemp('ensemble_pt') / 'ensemble_pt_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_pt_driver.cpp')]
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
BLOCKS = [(0, 0, 1, 0, 0), (5, 17, 3, 9, 2), (2111, 2**40, 63, M64, 7), (1, 2, 1, 3, 64)]


def test_the_two_blocks_use_the_documented_counters(driver):
    """Pair k of (rung t - 1, rung t) at step s: counter (k, s, t, 2); the rotation: counter (0, s, t, 3); both as NumPy's own
    Philox draws them, and apart from the blocks of the moves."""
    got = _ask(driver, [f'P {k} {s} {t} {seed:x} {stream:x}' for k, s, t, seed, stream in BLOCKS] +
               [f'R {s} {t} {seed:x} {stream:x}' for _, s, t, seed, stream in BLOCKS])
    for i, (k, s, t, seed, stream) in enumerate(BLOCKS):
        key = np.array([seed, stream], dtype=np.uint64)
        pair = np.random.Philox(key=key, counter=(k | (s << 64) | (t << 128) | (2 << 192)) - 1).random_raw(4)
        shift = np.random.Philox(key=key, counter=((s << 64) | (t << 128) | (3 << 192)) - 1).random_raw(4)
        assert [int(v, 16) for v in got[i].split()] == [int(v) for v in pair]
        assert [int(v, 16) for v in got[len(BLOCKS) + i].split()] == [int(v) for v in shift]
        assert np.array_equal(E.swap_blocks(k + 1, s, t, seed, stream)[k], pair)
        assert np.array_equal(E.shift_block(s, t, seed, stream), shift)
        assert not np.array_equal(E.step_blocks(k + 1, s, t % 2, seed, stream)[k], pair)
        assert not np.array_equal(E.move_blocks(k + 1, s, t % 2, seed, stream)[k], pair)


def _edge_lnl(rng, k):
    v = float(rng.normal(-2000.0, 900.0))
    return (v, 0.0, -0.0, -5e99, -1e-300, 1e3)[k % 11] if k % 11 < 6 else v


def test_tempered_decisions_bitwise(driver):
    """tempered(beta, lnL) and the decision built on it: the header equals the restatement bit for bit on random operands and at
    beta = 0 and 1; with beta = 1 the decision is the untempered one; with beta = 0 a proposal outside the box or with a failed
    model is still rejected, and one inside with a good model is decided by the factor alone."""
    rng = np.random.default_rng(3)
    betas = [1.0, 0.0, 0.5, 2.0**-5, 1.0 / 3.0, 0.9999999999999999, 5e-324]
    cases = [(betas[k % len(betas)], _edge_lnl(rng, k)) for k in range(300)]
    got = _ask(driver, [f'T {_hx(b)} {_hx(v)}' for b, v in cases])
    for line, (b, v) in zip(got, cases):
        assert int(line, 16) == _bits(E.tempered(b, np.float64(v))), (b, v)
        if b == 1.0:
            assert int(line, 16) == _bits(v)
    decisions, lines = [], []
    for k in range(600):
        beta = betas[k % len(betas)]
        inside, ok = int(k % 5 != 0), int(k % 4 != 0)
        factor = float(rng.normal(0.0, 2.0)) if k % 3 else 0.0
        old = _edge_lnl(rng, k)
        new = old if k % 13 == 0 else old + float(rng.normal(0.0, 3.0))        # (equal lnL among them)
        w2 = int(rng.integers(0, 2**64, dtype=np.uint64)) if k % 17 else (0, M64)[k % 2]
        decisions.append((inside, ok, factor, beta, new, old, w2))
        lines.append(f'A {inside} {ok} {_hx(factor)} {_hx(beta)} {_hx(new)} {_hx(old)} {w2:x}')
    seen = set()
    for line, (inside, ok, factor, beta, new, old, w2) in zip(_ask(driver, lines), decisions):
        hot, plain = (int(v) for v in line.split())
        word = np.array([w2], dtype=np.uint64)
        mine = bool(E.accept_tempered(np.array([inside]), np.array([ok]), np.array([factor]), beta, np.array([new]), np.array([old]),
                                      word)[0])
        assert hot == int(mine)
        assert plain == int(E.accept(np.array([inside]), np.array([ok]), np.array([factor]), np.array([new]), np.array([old]), word)[0])
        if beta == 1.0:
            assert hot == plain
        if not (inside and ok):
            assert hot == 0
        elif beta == 0.0:
            assert hot == int(factor > math.log(E.u01(word)[0]) if E.u01(word)[0] > 0 else True)
        seen.add((beta, hot))
    assert {(1.0, 0), (1.0, 1), (0.0, 0), (0.0, 1)} <= seen


def test_rotation_and_swap_rule_bitwise(driver):
    """The rotation of a word, the partner it gives every walker - r = 0, r = W - 1 and W = 2 among them - and the swap rule on
    random and equal lnL: the header equals the restatement; the partners of a rung are a permutation."""
    rng = np.random.default_rng(4)
    cases, lines = [], []
    for i in range(400):
        W = int(rng.choice([2, 2, 6, 8, 64, 2112, int(rng.integers(2, 2**31))]))
        w0 = (0, M64, 2**63)[i % 3] if i % 4 == 0 else int(rng.integers(0, 2**64, dtype=np.uint64))
        k = (0, W - 1)[i % 2] if i % 5 == 0 else int(rng.integers(0, W))
        cases.append((w0, W, k))
        lines.append(f'H {w0:x} {W} {k}')
    shifts = set()
    for line, (w0, W, k) in zip(_ask(driver, lines), cases):
        r, j = (int(v) for v in line.split())
        assert r == int(E.swap_shift(np.uint64(w0), W)) and 0 <= r < W
        assert j == int(E.swap_partner(k, r, W)) == (k + r) % W
        shifts.add('zero' if r == 0 else 'last' if r == W - 1 else 'other')
    assert shifts == {'zero', 'last', 'other'}
    for W in (2, 6, 2112):
        for r in (0, 1, W - 1):
            assert sorted(E.swap_partner(np.arange(W), r, W)) == list(range(W))
    ladder = [1.0, 0.5, 0.25, 2.0**-5, 0.0]
    cases, lines = [], []
    for i in range(600):
        t = 1 + i % (len(ladder) - 1)
        cold = _edge_lnl(rng, i)
        hot = cold if i % 9 == 0 else cold + float(rng.normal(0.0, 4.0 / max(ladder[t - 1] - ladder[t], 0.03)))
        word = int(rng.integers(0, 2**64, dtype=np.uint64)) if i % 17 else (0, M64)[i % 2]
        cases.append((ladder[t - 1], ladder[t], cold, hot, word))
        lines.append(f'S {_hx(ladder[t - 1])} {_hx(ladder[t])} {_hx(cold)} {_hx(hot)} {word:x}')
    took = []
    for line, (bc, bh, cold, hot, word) in zip(_ask(driver, lines), cases):
        mine = bool(E.swap_accept(bc, bh, np.array([cold]), np.array([hot]), np.array([word], dtype=np.uint64))[0])
        assert int(line) == int(mine)
        if hot >= cold:         # (a hotter walker that is no worse always comes down: u < 1, equal lnL included)
            assert mine
        took.append(mine)
    assert 0.2 < np.mean(took) < 0.95
    steps = [(s, every) for s in (0, 1, 2, 5, 6, 2**40 - 1) for every in (0, 1, 3, 7)]
    for line, (s, every) in zip(_ask(driver, [f'D {s} {every}' for s, every in steps]), steps):
        assert int(line) == int(E.swap_due(s, every)) == int(every > 0 and (s + 1) % every == 0)


LADDERS = [([1.0], True), ([1.0, 0.0], True), ([1.0, 0.5, 0.25, 0.0], True), ([1.0, 0.5, 0.25], True), ([0.5, 0.25], False),
           ([1.0, 1.0], False), ([1.0, 0.5, 0.5], False), ([1.0, 0.25, 0.5], False), ([1.0, -0.0, -0.1], False), ([1.0, -1e-300], False),
           ([1.0, float('nan')], False), ([1.0, float('inf')], False), ([float('inf')], False), ([], False),
           (list(np.linspace(1.0, 0.0, 64)), True), (list(np.linspace(1.0, 0.0, 65)), False)]


def test_ladders_bitwise(driver):
    got = _ask(driver, [f'L {len(b)} ' + ' '.join(_hx(v) for v in b) for b, _ in LADDERS])
    for line, (b, want) in zip(got, LADDERS):
        assert int(line) == int(E.ladder_ok(b)) == int(want), b


def test_default_ladder():
    assert np.array_equal(E.default_ladder(6), [1.0, 0.5, 0.25, 0.125, 0.0625, 0.0])
    assert np.array_equal(E.default_ladder(2), [1.0, 0.0]) and np.array_equal(E.default_ladder(3), [1.0, 0.5, 0.0])
    assert np.array_equal(E.default_ladder(64)[:-1], 2.0 ** -np.arange(63.0)) and E.ladder_ok(E.default_ladder(64))
    b = E.default_ladder(8, beta_min=0.01)
    assert b[0] == 1.0 and b[6] == 0.01 and b[7] == 0.0 and E.ladder_ok(b)
    np.testing.assert_allclose(b[1:7] / b[0:6], 0.01 ** (1 / 6), rtol=1e-12)
    for bad in (dict(ntemps=1), dict(ntemps=65), dict(ntemps=4, beta_min=0.0), dict(ntemps=4, beta_min=1.0), dict(ntemps=4, beta_min=-1)):
        with pytest.raises(ValueError):
            E.default_ladder(**bad)


# ------------------------------------------------------------------ the python driver on a callable likelihood
A_MODE, B_MODE = np.array([-10.0, 0.0]), np.array([10.0, 0.0])
BOX = (np.array([-20.0, -10.0]), np.array([20.0, 10.0]))
LADDER6 = np.array([1.0, 0.5, 0.25, 0.125, 0.0625, 0.0])
RUNS, STEPS, BURN, BATCH = 4, 1500, 300, 300


def _bimodal(rows, h=None):
    """chi2 = -2 lnL of the equal-weight mixture of two unit Gaussians 20 sigma apart (log_norm = 0)."""
    a = -0.5 * np.sum((rows - A_MODE)**2, axis=1)
    b = -0.5 * np.sum((rows - B_MODE)**2, axis=1)
    return -2.0 * (np.logaddexp(a, b) + math.log(0.5)), np.zeros(rows.shape[0], dtype=np.int32)


def _start_in_a(shape, seed):
    x = A_MODE + np.random.default_rng(seed).standard_normal(shape + (2,))
    return np.clip(x, *BOX)


def _run_pt(betas, W, steps, seed=5, G=1, thin=1, swap_every=1, segments=None, moves=None, target=_bimodal):
    T = len(betas)
    x = _start_in_a((G, T, W), seed)
    lnl = E.log_lik(0.0, target(x.reshape(-1, 2))[0]).reshape(G, T, W)
    acc = np.zeros((G, T, W), dtype=np.int64)
    streams = 64 * np.arange(G)[:, None] + np.arange(T)[None, :]
    parts, step = [], 0
    for k in (segments or [steps]):
        parts.append(E.python_steps_pt(x, lnl, acc, step, k, thin, swap_every, 2.0, seed, betas, streams, BOX[0], BOX[1], 0.0, target,
                                       moves))
        step += k
    chain = np.concatenate([p[0] for p in parts], axis=2)
    chain_lnl = np.concatenate([p[1] for p in parts], axis=2)
    return chain, chain_lnl, acc, sum(p[3] for p in parts), sum(p[4] for p in parts), x, lnl


@pytest.fixture(scope='module')
def bimodal_run():
    return _run_pt(LADDER6, 16, STEPS, G=RUNS)


def test_a_plain_ensemble_never_leaves_its_mode():
    x = _start_in_a((16,), 5)
    lnl = E.log_lik(0.0, _bimodal(x)[0])
    chain, _, st = E.python_steps(x, lnl, np.zeros(16, dtype=np.int64), 0, 700, 1, 2.0, 5, 0, BOX[0], BOX[1], 0.0, _bimodal)
    assert st['accepted'] > 0.2 * st['proposals'] and not np.any(chain[..., 0] > 0.0)


def _mode_fraction(chain):
    """The cold rungs' fraction in mode B past the burn-in with its standard error and the effective size that goes with it:
    (fraction, se, n_eff, tau = N / n_eff).  The ladders are independent runs and the series of a ladder is cut into batches of
    BATCH steps; the standard error is the larger of the scatter of the batch means and the scatter of the ladders' own means,
    each over the root of their number."""
    in_b = (chain[:, 0, BURN:, :, 0] > 0.0).astype(np.float64)           # [G, rows, W]
    G, rows, W = in_b.shape
    per_step = in_b.mean(axis=2)
    batches = per_step[:, :rows // BATCH * BATCH].reshape(G, -1, BATCH).mean(axis=2)
    se = max(batches.std(ddof=1) / math.sqrt(batches.size), per_step.mean(axis=1).std(ddof=1) / math.sqrt(G))
    n_eff = 0.25 / se**2
    return in_b.mean(), se, n_eff, in_b.size / n_eff


def test_the_cold_rung_visits_both_modes_in_equal_parts(bimodal_run):
    """Six rungs (1 ... 1/16, 0), W = 16, every walker of every rung started in mode A: the cold rung records points in mode B,
    and its fraction there lies within 5 binomial standard errors of 0.5 at an effective size N / tau; N / tau > 50, so that
    the bound cannot hide a chain that is stuck.

    tau is not taken from ``integrated_time`` of the indicator.  A slot of the cold rung changes its walker with every accepted
    swap (two steps out of three here), so a slot's indicator forgets within a few steps (tau about 2) whatever the ladder does,
    while the rung's fraction follows the share of the ladder's walkers on either side, which changes only as walkers cross on
    the hot rungs and come down.  The windowed estimator on the fraction's own series does not see that either in a run of this
    length: the slow part lies under the binomial noise of 16 walkers and the window closes early (7.5 on 900 rows of one
    ladder, where 2900 rows gave 40 and 154 on two seeds).  So the effective size comes from the fractions' own scatter, which
    needs no window: RUNS independent ladders, the series of each cut into batches of BATCH steps (:func:`_mode_fraction`);
    n_eff = 0.25 / se^2 is the size at which the binomial standard error is that scatter.  Measured over the seeds 5, 1, 2, 3:
    pulls -0.57, -0.67, +1.30, -1.26 at n_eff 1757, 626, 2324, 2650, that is tau = N / n_eff of 44, 123, 33, 29 steps."""
    chain, chain_lnl, acc, per, swaps, _, _ = bimodal_run
    assert chain.shape == (RUNS, 6, STEPS, 16, 2) and np.all(chain >= BOX[0]) and np.all(chain <= BOX[1])
    assert np.all(np.any(chain[:, 0, BURN:, :, 0] > 0.0, axis=(1, 2)))
    frac, se, n_eff, tau = _mode_fraction(chain)
    slot_tau = float(E.integrated_time((chain[0, 0, BURN:, :, 0] > 0.0).astype(np.float64))[0])
    print('fraction in B', frac, 'se', se, 'pull', (frac - 0.5) / se, 'n_eff', n_eff, 'tau', tau, "a slot's tau", slot_tau,
          'swap fractions', swaps[0, :, 1] / swaps[0, :, 0])
    assert n_eff > 50, (tau, n_eff)
    assert abs(frac - 0.5) < 5 * math.sqrt(0.25 / n_eff), (frac, n_eff)
    # the cold rung's points sit on the two modes; the last rung fills the box
    cold = chain[0, 0, BURN:].reshape(-1, 2)
    near = np.minimum(np.sum((cold - A_MODE)**2, axis=1), np.sum((cold - B_MODE)**2, axis=1))
    assert np.mean(near < 9.0) > 0.95
    hot = chain[0, 5, BURN:].reshape(-1, 2)
    assert np.all(np.abs(hot.mean(axis=0)) < 1.0) and abs(hot[:, 0].var() - 40.0**2 / 12.0) < 15.0
    assert np.all(swaps[:, :, 0] == STEPS * 16) and np.all(swaps[:, :, 1] > 0)
    np.testing.assert_array_equal(chain_lnl, E.log_lik(0.0, _bimodal(chain.reshape(-1, 2))[0]).reshape(chain_lnl.shape))


@pytest.mark.parametrize('moves', [None, [('stretch', 0.3), ('de', 0.4), ('snooker', 0.3)]], ids=str)
def test_the_chain_is_independent_of_the_cut(moves):
    mv = E.resolve_moves(moves, 2, 8)
    one = _run_pt(LADDER6[[0, 2, 5]], 8, 20, G=2, thin=2, swap_every=3, moves=mv)
    two = _run_pt(LADDER6[[0, 2, 5]], 8, 20, G=2, thin=2, swap_every=3, moves=mv, segments=[7, 13])
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    assert one[0].shape == (2, 3, 10, 8, 2) and np.all(one[4][:, :, 0] == 6 * 8) and one[4][:, :, 1].sum() > 0
    assert one[3].shape == (2, 3, 3) and np.array_equal(one[3][:, :, 0], one[2].sum(axis=2))
    other = _run_pt(LADDER6[[0, 2, 5]], 8, 20, G=2, thin=2, swap_every=4, moves=mv)
    assert not np.array_equal(one[0], other[0])
    assert not np.array_equal(one[0][0], one[0][1])          # (the ladders run on streams of their own)


def test_without_swaps_a_rung_at_beta_one_is_the_plain_ensemble():
    betas = LADDER6[[0, 1, 5]]
    chain, chain_lnl, acc, per, swaps, _, _ = _run_pt(betas, 8, 15, G=2, swap_every=0)
    assert np.all(swaps == 0)
    x = _start_in_a((2, 3, 8), 5)[:, 0].copy()
    lnl = E.log_lik(0.0, _bimodal(x.reshape(-1, 2))[0]).reshape(2, 8)
    acc1 = np.zeros((2, 8), dtype=np.int64)
    ref, ref_lnl, _, ref_per = E.python_steps_many(x, lnl, acc1, 0, 15, 1, 2.0, 5, [0, 64], BOX[0], BOX[1], 0.0, _bimodal)
    assert np.array_equal(chain[:, 0], ref) and np.array_equal(chain_lnl[:, 0], ref_lnl)
    assert np.array_equal(acc[:, 0], acc1) and np.array_equal(per[:, 0], ref_per)
    with_swaps = _run_pt(betas, 8, 15, G=2, swap_every=1)
    assert not np.array_equal(with_swaps[0][:, 0], ref) and with_swaps[4][:, :, 1].sum() > 0


# ------------------------------------------------------------------ the evidence: a 4-D unit Gaussian in a box of +-10 sigma
LOG_Z4 = 2.0 * math.log(2.0 * math.pi) - 4.0 * math.log(20.0)         # lnL = -|x|^2 / 2 over the uniform prior: -8.30717...
LADDER7 = np.array([1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.0])


def _exact_draws(betas, rows, seed):
    """lnL [T, rows, 1] of exact, independent draws of every rung: N(0, 1 / beta) per coordinate cut to [-10, 10], uniform at 0."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(betas), rows, 1))
    for t, beta in enumerate(betas):
        if beta == 0.0:
            x = rng.uniform(-10.0, 10.0, size=(rows, 4))
        else:
            x = rng.standard_normal((rows, 4)) / math.sqrt(beta)
            while np.any(np.abs(x) > 10.0):
                bad = np.abs(x) > 10.0
                x[bad] = rng.standard_normal(int(bad.sum())) / math.sqrt(beta)
        out[t, :, 0] = -0.5 * np.sum(x * x, axis=1)
    return out


def _exact_mean_lnl(betas):
    """<lnL>_beta of the same target: -2 E[x^2] of the cut Gaussian (100 / 3 at beta = 0)."""
    out = np.empty(len(betas))
    for t, beta in enumerate(betas):
        if beta == 0.0:
            out[t] = -2.0 * 100.0 / 3.0
            continue
        a = 10.0 * math.sqrt(beta)
        phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
        out[t] = -2.0 / beta * (1.0 - 2.0 * a * phi / math.erf(a / math.sqrt(2.0)))
    return out


def test_stepping_stones_on_exact_draws():
    assert abs(LOG_Z4 - -8.30717) < 1e-5
    log_z, err = E.stepping_stone_evidence(LADDER7, _exact_draws(LADDER7, 500, 1))
    print('stepping stones', log_z, '+-', err, 'pull', (log_z - LOG_Z4) / err)
    assert abs(log_z - LOG_Z4) < 5 * err and 0.0 < err <= 0.25
    with pytest.raises(ValueError, match='last beta is 0'):
        E.stepping_stone_evidence(LADDER7[:-1], _exact_draws(LADDER7[:-1], 50, 1))
    with pytest.raises(ValueError, match='last beta is 0'):
        E.thermodynamic_integration(LADDER7[:-1], np.zeros(6))


def test_thermodynamic_integration_on_the_exact_curve():
    fine = E.default_ladder(64, beta_min=1e-3)
    log_z, err = E.thermodynamic_integration(fine, _exact_mean_lnl(fine))
    print('ti, 64 rungs', log_z, '+-', err, 'off by', log_z - LOG_Z4)
    assert abs(log_z - LOG_Z4) <= err and err < 0.1
    coarse, coarse_err = E.thermodynamic_integration(LADDER7, _exact_mean_lnl(LADDER7))
    print('ti, 7 rungs', coarse, '+-', coarse_err, 'off by', coarse - LOG_Z4)
    assert coarse_err >= 0.5 * abs(coarse - LOG_Z4)
    assert -0.5 < coarse - LOG_Z4 < -0.4         # (the bias of the trapezoid rule on this ladder)


# ------------------------------------------------------------------ the settings
SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'
MC_HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\nrun_montecarlo = True\n[monte carlo]\nx = 1\n'


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


def test_tempering_settings_parse(tmp_path):
    base = f'{HEAD}[Ensemble]\npath = {tmp_path}\nwalkers = 8\n'
    plain = E.sampler_settings(_config(base), SAMPLE)
    assert not {'ntemps', 'beta_min', 'swap_every'} & set(plain)
    assert E.sampler_settings(_config(base + 'ntemps = 6\n'), SAMPLE) == dict(plain, ntemps=6, swap_every=1)
    got = E.sampler_settings(_config(base + 'ntemps = 8\nbeta_min = 0.01\nswap_every = 5\nmoves = de\n'), SAMPLE)
    assert got == dict(plain, ntemps=8, beta_min=0.01, swap_every=5, moves=[('de', 1.0)])
    assert E.sampler_settings(_config(base + 'ntemps = 3\nswap_every = 0\nreplicas = 1\n'), SAMPLE)['swap_every'] == 0


@pytest.mark.parametrize('head, text, match', [
    (HEAD, 'ntemps = 1\n', 'ntemps'), (HEAD, 'ntemps = 65\n', 'ntemps'), (HEAD, 'ntemps = many\n', 'whole numbers'),
    (HEAD, 'ntemps = 4\nbeta_min = 0\n', 'beta_min'), (HEAD, 'ntemps = 4\nbeta_min = 1.5\n', 'beta_min'),
    (HEAD, 'ntemps = 4\nswap_every = -1\n', 'swap_every'), (HEAD, 'beta_min = 0.1\n', 'no ntemps'), (HEAD, 'swap_every = 2\n', 'no ntemps'),
    (HEAD, 'ntemps = 4\nreplicas = 2\n', 'replicas'), (HEAD, 'ntemps = 4\ntogether = True\n', 'together'),
    (MC_HEAD, 'ntemps = 4\nmocks = 2\n', 'mocks'),
    (HEAD, 'ntemps = 4\nsteps = 3\nthin = 2\n', 'two recorded rows'),
])
def test_tempering_settings_refusals(tmp_path, head, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{head}[Ensemble]\npath = {tmp_path}\nwalkers = 8\n{text}'), SAMPLE)


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


def test_tempered_ensemble_over_a_stand_in(tmp_path):
    """``TemperedEnsemble`` through the python driver: the shapes of what it keeps, rungs as read-only members, the default
    streams 64 sigma + t, a run that does not depend on the segments, the cold rung without swaps equal to the single sampler,
    and the evidence of the Gaussian - log Z = log_norm + log(2 pi sqrt(det C)) over a unit box - within 5 err."""
    vega = _StandInVega()
    s = E.TemperedEnsemble(vega, 8, ntemps=7, beta_min=1e-3, ladders=2, seed=3, driver='python', moves=[('de', 0.8), ('snooker', 0.2)])
    assert np.array_equal(s.streams.reshape(2, 7), 64 * np.arange(2)[:, None] + np.arange(7)[None, :])
    s.run(300)
    assert s.driver == 'python' and 'moves' not in s.stats
    assert s.get_chain().shape == (300, 8, 2) and s.get_chain(rung=None).shape == (2, 7, 300, 8, 2)
    assert s.get_log_lik(rung=3, discard=100, ladder=1).shape == (200, 8) and s.get_chain(rung=6, flat=True).shape == (2400, 2)
    assert s.swap_fraction.shape == (2, 6) and np.all(s.swap_fraction > 0.05) and np.all(s.swaps[:, :, 0] == 300 * 8)
    assert s.stats['swaps_proposed'] == 2 * 6 * 300 * 8 and s.stats['swaps_accepted'] == s.swaps[:, :, 1].sum()
    assert s.stats['proposals'] == 14 * 8 * 300 and s.stats['accepted'] == s.accepted.sum()
    rung = s.rung(2, ladder=1)
    assert np.array_equal(rung.get_chain(), s.get_chain(rung=2, ladder=1)) and rung.beta == s.betas[2] and rung.stream == 64 + 2
    with pytest.raises(RuntimeError, match='read-only'):
        rung.run(1)
    with pytest.raises(IndexError):
        s.rung(7)
    exact = 1.25 + math.log(2.0 * math.pi * math.sqrt(np.linalg.det(vega.COV)))
    for g in range(2):
        log_z, err = s.log_evidence(ladder=g)
        ti, ti_err = s.log_evidence('ti', ladder=g)
        print('ladder', g, 'log Z', log_z, '+-', err, 'exact', exact, 'ti', ti, '+-', ti_err)
        assert abs(log_z - exact) < 5 * err and err < 0.5
    with pytest.raises(ValueError, match='method'):
        s.log_evidence('harmonic')
    cut = E.TemperedEnsemble(vega, 8, ntemps=7, beta_min=1e-3, ladders=2, seed=3, driver='python', segment=11,
                             moves=[('de', 0.8), ('snooker', 0.2)]).run(40)
    assert np.array_equal(cut.get_chain(rung=None), s.get_chain(rung=None)[:, :, :40]) and cut.stats['calls'] == 4
    free = E.TemperedEnsemble(vega, 8, betas=[1.0, 0.3], swap_every=0, streams=[[5, 9]], seed=3, driver='python').run(20)
    one = E.EnsembleSampler(vega, 8, seed=3, stream=5, driver='python').run(20)
    assert np.array_equal(free.get_chain(), one.get_chain()) and np.array_equal(free.rung(0).accepted, one.accepted)
    assert np.all(np.isnan(free.swap_fraction))
    with pytest.raises(ValueError, match='last beta is 0'):
        free.log_evidence()
    assert [p.name for p in free.write(tmp_path, 'free')] == ['free.txt', 'free.paramnames']
    short = E.TemperedEnsemble(vega, 8, ntemps=3, seed=3, driver='python').run(1)            # (one row: a chain, no evidence)
    assert short.recorded_rows == 1 and [p.name for p in short.write(tmp_path, 'short', print_func=lambda *_: None)] == ['short.txt', 'short.paramnames']
    with pytest.raises(ValueError, match='two rows'):
        short.log_evidence()
    with pytest.raises(TypeError):
        s.get_chain(0, 1, False, 2)         # (rung and ladder are keyword-only: the positional slots are EnsembleSet's)
    files = s.write(tmp_path, 'both')
    assert [[p.name for p in f] for f in files] == [[f'both_ladder{g}.txt', f'both_ladder{g}.paramnames', f'both_ladder{g}.stats']
                                                    for g in range(2)]
    stats = E.read_pt_stats(files[1][2])
    assert stats['log(Z)'] == s.log_evidence(ladder=1)[0] and stats['beta'] == list(s.betas) and stats['steps'] == 300
    assert stats['swap fraction'] == list(s.swap_fraction[1])
    for bad in (dict(), dict(ntemps=3, betas=[1.0, 0.0]), dict(betas=[0.9, 0.0]), dict(betas=[1.0, 0.5, 0.5]), dict(ntemps=3, swap_every=-1),
                dict(ntemps=3, ladders=0), dict(ntemps=3, streams=[1, 2]), dict(betas=[1.0, 0.0], beta_min=0.1)):
        with pytest.raises(ValueError):
            E.TemperedEnsemble(vega, 8, **bad)


def test_run_vega_sampler_with_ntemps_over_a_stand_in(tmp_path):
    (tmp_path / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {tmp_path}\nname = run\ndriver = python\nwalkers = 8\nsteps = 60\n'
                                       'seed = 3\nthin = 2\nntemps = 4\nbeta_min = 0.01\nswap_every = 2\n')
    said = []
    run = E.run_vega_sampler(str(tmp_path / 'main.ini'), print_func=lambda *a: said.append(' '.join(map(str, a))), rank=0, world_size=1,
                             make_vega=lambda config, device: _StandInVega(config))
    assert isinstance(run, E.TemperedEnsemble) and np.array_equal(run.betas, E.default_ladder(4, 0.01)) and run.swap_every == 2
    by_hand = E.TemperedEnsemble(_StandInVega(), 8, ntemps=4, beta_min=0.01, swap_every=2, seed=3, thin=2, driver='python').run(60)
    assert np.array_equal(run.get_chain(rung=None), by_hand.get_chain(rung=None))
    log_z, err = run.log_evidence()
    assert f'log(Z) = {log_z} +- {err}' in said
    table = np.loadtxt(tmp_path / 'run.txt')
    assert table.shape == (30 * 8, 4)
    np.testing.assert_array_equal(table[:, 2:], run.get_chain(flat=True))
    np.testing.assert_array_equal(table[:, 1], -run.get_log_lik(flat=True))
    assert (tmp_path / 'run.paramnames').read_text().splitlines() == ['a a', 'b b']
    stats = E.read_pt_stats(tmp_path / 'run.stats')
    assert stats['log(Z)'] == log_z and stats['log(Z) error'] == err and stats['beta'] == [1.0, 0.1, 0.01, 0.0]
    assert stats['swap_every'] == 2 and stats['walkers'] == 8 and stats['likelihood evaluations'] == 60 * 8 * 4


def test_the_entry_is_bound():
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert 'vmx_ensemble_run_pt' in engine.EXPORTED_SYMBOLS and hasattr(lib, 'vmx_ensemble_run_pt')
    assert len(lib.vmx_ensemble_run_pt.argtypes) == len(lib.vmx_ensemble_run_many_moves.argtypes) + 4
    header = (REPO / 'include' / 'vegamx.h').read_text()
    assert f'#define VMX_PT_MAXT {E.PT_MAXT}' in header
