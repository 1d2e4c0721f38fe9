"""Weighted sample sets without a GPU: vega_amd/csrc/vmx_chain_weighted.h, compiled with g++ under AddressSanitizer / UBSan
(tests/helpers/chain_weighted_driver.cpp, a stand-alone program run as a subprocess), against its NumPy restatement
(vega_amd/weighted.py) bit for bit; equal weights against the unweighted order statistics; the restatement against
``np.quantile(weights=, method='inverted_cdf')`` with the integer and with the float weights; the moments against the expressions
``MonteCarlo._sample_mocks`` writes; and mutations of the restatement, each of which a case here catches (docs/LAB_NOTES.md)."""
import math
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import chain_weighted_cases as wc
from vega_amd import ensemble as E
from vega_amd import weighted as W

REPO = Path(__file__).resolve().parents[1]
Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]


# ------------------------------------------------------------------ the header
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('weighted') / 'chain_weighted_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'chain_weighted_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _hex(a):
    return ' '.join(f'{v:016x}' for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64).tolist())


def _ask(exe, text):
    run = subprocess.run([str(exe)], input=text + '\n', capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout.splitlines()


def _doubles(line):
    return np.array([int(v, 16) for v in line.split()], dtype=np.uint64).view(np.float64)


def _shape(sets, capacity):
    x, lnl, w, counts = wc.store(sets, capacity)
    return x, lnl, w, f'{len(sets)} {capacity} {x.shape[2]} {" ".join(str(int(c)) for c in counts)}'


def header_all(exe, sets, capacity, targets):
    """Summary, order statistics at ``targets`` [E][R] and the best point of a store, from the header in one run."""
    x, lnl, w, shape = _shape(sets, capacity)
    Ens, n, R = len(sets), x.shape[2], len(targets[0])
    flat = ' '.join(str(int(t)) for row in targets for t in row)
    lines = _ask(exe, f'U {shape} {_hex(x)} {_hex(w)}\nO {shape} {R} {flat} {_hex(x)} {_hex(w)}\nB {shape} 1 {_hex(x)} {_hex(lnl)}')
    return dict(S=_doubles(lines[0]), n_eff=_doubles(lines[1]), mean=_doubles(lines[2]).reshape(Ens, n),
                covariance=_doubles(lines[3]).reshape(Ens, n, n), total=[int(v) for v in lines[4].split()], w_max=_doubles(lines[5]),
                values=_doubles(lines[6]).reshape(Ens, n, R), lnl_max=_doubles(lines[7]),
                index=np.array(lines[8].split(), dtype=np.int64), best=_doubles(lines[9]).reshape(Ens, n))


def restated_all(sets, targets):
    """The same from vega_amd/weighted.py."""
    summ = [W.weighted_summary(x, w) for x, _, w in sets]
    tops = [W.weighted_best(x, lnl) for x, lnl, _ in sets]
    out = {key: np.array([s[key] for s in summ]) for key in ('S', 'n_eff', 'mean', 'covariance', 'w_max')}
    out['total'] = [s['total'] for s in summ]
    out['values'] = np.array([W.weighted_order_statistics(x, w, t) for (x, _, w), t in zip(sets, targets)])
    out.update(lnl_max=np.array([t['lnl_max'] for t in tops]), index=np.array([t['index'] for t in tops], dtype=np.int64),
               best=np.array([t['best'] for t in tops]))
    return out


def same(a, b, where=None):
    assert set(a) == set(b)
    for key in a:
        if key == 'total':
            assert list(a[key]) == list(b[key]), (key, where)
        else:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (key, where)


@pytest.mark.parametrize('count, n', wc.SHAPES)
def test_the_header_equals_the_restatement(driver, count, n):
    """Bit for bit: three sets (0, 1 and ``count`` rows) in a store with room past the rows (filled with what would show), every
    kind of weight, every kind of column (NaN positions that carry weight and +-0 among them), equal positions under different
    weights, one target and sixteen (unsorted, with repeats, 1 and M, a cumulative sum and the one after it)."""
    variants = range(len(wc.cases.KIND_NAMES)) if 2 * n < len(wc.cases.KIND_NAMES) else [0]
    for kind in wc.WEIGHTS:
        for variant in variants:
            sets = wc.sets_of(count, n, kind, variant, seed=1)
            if kind == 'log-normal' and variant == 0:
                sets[2] = wc.sample_set(count, n, kind, variant, seed=1, equal_x=True)
            for R in (1, 16):
                targets = [wc.targets_of(s, R, seed=variant) for s in sets]
                ours = restated_all(sets, targets)
                same(header_all(driver, sets, count + 3, targets), ours, (kind, variant, R))
            assert np.isnan(ours['mean'][0]).all() and np.isnan(ours['covariance'][0]).all() and np.isnan(ours['n_eff'][0])
            assert ours['index'][0] == -1 and ours['total'][0] == 0 and np.isnan(ours['values'][0]).all()
            # one row carries all the weight: its own position, no covariance
            if sets[1][2][0] > 0.0:
                assert ours['n_eff'][1] == 1.0 and np.isnan(ours['covariance'][1]).all()
                assert np.array_equal(ours['mean'][1], sets[1][0][0], equal_nan=True)
            if kind == 'all zero':
                assert np.isnan(ours['n_eff'][1]) and np.isnan(ours['mean'][2]).all() and np.isnan(ours['values']).all()
                assert ours['total'] == [0, 0, 0]


def test_the_ragged_store(driver):
    """counts = (0, 1, 257) with room past the rows, and a store whose sets differ in kind."""
    for kind in wc.WEIGHTS:
        sets = wc.sets_of(257, 3, kind, 3, seed=4, counts=(0, 1, 257))
        targets = [wc.targets_of(s, 16, seed=2) for s in sets]
        same(header_all(driver, sets, 300, targets), restated_all(sets, targets), kind)
    sets = [wc.sample_set(c, 2, kind, v, seed=6) for v, (c, kind) in enumerate(zip((257, 0, 40, 256, 3, 255), wc.WEIGHTS))]
    targets = [wc.targets_of(s, 16, seed=3) for s in sets]
    same(header_all(driver, sets, 257, targets), restated_all(sets, targets))


def test_weights_that_may_be_stored(driver):
    w = np.array([0.0, -0.0, 1.0, 5e-324, 1.7976931348623157e308, -1e-300, -1.0, np.inf, -np.inf, np.nan])
    got = [int(v) for v in _ask(driver, f'W {w.size} {_hex(w)}')[0].split()]
    assert got == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    for k, ok in enumerate(got):
        if ok:
            W.check_weights(w[k:k + 1])
        else:
            with pytest.raises(ValueError):
                W.check_weights(w[k:k + 1])


# ------------------------------------------------------------------ what the definition implies
def test_equal_weights_give_the_unweighted_answer():
    """With equal weights every m is 2^32, so the target ceil(q M) falls into row ceil(q N) - 1 of the sorted column: the
    unweighted order statistic of vmx_chain_select.h, bit for bit."""
    qs = [0.0, 0.025, 0.16, 1.0 / 3.0, 0.5, 0.84, 0.975, 0.999, 1.0]
    for count, n in wc.SHAPES:
        for variant in (range(9) if n < 4 else [0]):
            x, _, w = wc.sample_set(count, n, 'all equal', variant, seed=3)
            m, M, _ = W.integer_weights(w)
            assert M == count << 32 and np.all(m == np.uint64(1 << 32))
            ranks = [max(math.ceil(Fraction(q) * count) - 1, 0) for q in qs]
            ref = E.chain_order_statistics(x.reshape(count, 1, n), ranks)
            assert W.weighted_quantiles(x, w, qs).tobytes() == ref.tobytes(), (count, n, variant)


def _gap_ok(x, m, M, qs):
    """From the integer cumulative sums alone: no C_i within 1e-9 M of q M."""
    C = np.array(wc.cumulative(x, m), dtype=object)
    return all(abs(Fraction(int(c)) - Fraction(q) * M) > Fraction(1, 10**9) * M for q in qs for c in C)


def _numpy_cases():
    """(x [N], w [N]) over N <= 700 and log-normal weights of width 0.1 / 3 / 30, a third of the weights zeroed in a fifth."""
    for trial in range(60):
        rng = np.random.default_rng([11, trial])
        N = int(rng.integers(2, 701))
        w = np.exp((0.1, 3.0, 30.0)[trial % 3] * rng.standard_normal(N))
        if trial % 5 == 0:
            w[rng.random(N) < 1.0 / 3.0] = 0.0
        yield trial, rng.standard_normal(N), w


def test_against_numpy_with_the_integer_weights():
    """``np.quantile(x, q, weights=m, method='inverted_cdf')`` compares a rounded cumsum / total with q; away from the ties of
    that comparison (asserted from the integer sums) it is the order statistic at ceil(q M), exactly."""
    qs = Q5 + [0.0, 0.25, 1.0 / 3.0, 0.999]
    checked = 0
    for trial, x, w in _numpy_cases():
        m, M, _ = W.integer_weights(w)
        assert _gap_ok(x, m, M, [q for q in qs if q > 0.0]), trial
        ours = W.weighted_order_statistics(x[:, None], w, W.weighted_targets(qs, M))[0]
        positive = m > 0        # (NumPy's q = 0 is the smallest sample, ours the smallest that carries weight)
        ref = np.quantile(x[positive], qs, weights=m[positive].astype(np.float64), method='inverted_cdf')
        assert ours.tobytes() == np.asarray(ref, dtype=np.float64).tobytes(), trial
        checked += len(qs)
    assert checked >= 500


def test_against_numpy_with_the_float_weights():
    """The truncation to 2^-32 w_max moves no quantile in {0.025, 0.16, 0.5, 0.84, 0.975} of these sets."""
    for trial, x, w in _numpy_cases():
        m, M, _ = W.integer_weights(w)
        assert _gap_ok(x, m, M, Q5), trial
        ours = W.weighted_quantiles(x[:, None], w, Q5)[0]
        ref = np.quantile(x, Q5, weights=w, method='inverted_cdf')
        assert ours.tobytes() == np.asarray(ref, dtype=np.float64).tobytes(), trial


def test_the_last_quantile_skips_truncated_weights():
    """q = 1 against the definition: the largest sample whose weight survives the truncation, not the largest sample."""
    x = np.array([0.5, 3.0, 1.0, 2.0, -1.0])
    w = np.array([1.0, 2.0**-33, 0.25, 2.0**-32, 0.0])
    m, M, w_max = W.integer_weights(w)
    assert m.tolist() == [1 << 32, 0, 1 << 30, 1, 0] and M == (1 << 32) + (1 << 30) + 1 and w_max == 1.0
    assert W.weighted_quantiles(x[:, None], w, [1.0])[0, 0] == 2.0
    assert W.weighted_quantiles(x[:, None], w, [0.0])[0, 0] == 0.5
    assert W.weighted_targets([0.0, 1.0, 0.5], 7) == [1, 7, 4] and W.weighted_targets([2.0**-40], 1 << 62) == [1 << 22]
    assert W.weighted_targets([0.1], 10**18) == [math.ceil(Fraction(0.1) * 10**18)]


# ------------------------------------------------------------------ the moments against the host loop of _sample_mocks
# the worst relative differences measured by test_moments_against_the_sample_mocks_expressions (printed there), and the bound:
# 100 x the worst, the margin the chain summary took - a BLAS dot and a pinned tree differ by rounding alone
WORST_MEAN, WORST_COV, WORST_NEFF = 1.504e-11, 3.301e-15, 4.788e-16
MOMENT_TOL = dict(mean=100 * WORST_MEAN, covariance=100 * WORST_COV, n_eff=100 * WORST_NEFF)


def moment_differences(pts, w, summ):
    """Relative differences between ``summ`` and the expressions of ``_sample_mocks`` on normalised weights: the mean against
    the sd, the covariance against sqrt(C_ii C_jj), n_eff against itself."""
    mean = w @ pts
    dev = pts - mean
    cov = (w[:, None] * dev).T @ dev / (1.0 - np.sum(w * w))
    sd = np.sqrt(np.diag(cov))
    n_eff = 1.0 / np.sum(w * w)
    return (float(np.max(np.abs(summ['mean'] - mean) / sd)), float(np.max(np.abs(summ['covariance'] - cov) / np.outer(sd, sd))),
            abs(summ['n_eff'] - n_eff) / n_eff)


def moment_sets():
    for trial in range(40):
        rng = np.random.default_rng([17, trial])
        count, n = int(rng.integers(50, 3000)), int(rng.integers(1, 7))
        w = np.exp((0.1, 1.0, 2.0)[trial % 3] * rng.standard_normal(count))
        if trial % 4 == 0:
            w[rng.random(count) < 1.0 / 3.0] = 0.0
        w /= w.sum()
        pts = rng.standard_normal((count, n)) * 10.0 ** rng.integers(-3, 4, n) + 10.0 ** rng.integers(-2, 3, n)
        yield pts, w


def test_moments_against_the_sample_mocks_expressions():
    worst = np.zeros(3)
    used = 0
    for pts, w in moment_sets():
        summ = W.weighted_summary(pts, w)
        if summ['n_eff'] < 10.0:
            continue
        used += 1
        worst = np.maximum(worst, moment_differences(pts, w, summ))
    print(f'weighted_summary against w @ pts: worst mean {worst[0]:.3e} sd, covariance {worst[1]:.3e} sqrt(C_ii C_jj), n_eff {worst[2]:.3e}')
    assert used >= 30
    assert worst[0] <= MOMENT_TOL['mean'] and worst[1] <= MOMENT_TOL['covariance'] and worst[2] <= MOMENT_TOL['n_eff']
    # weights that do not sum to 1 describe the set their normalisation does (a power of two scales exactly)
    pts, w = next(moment_sets())
    a, b = W.weighted_summary(pts, w), W.weighted_summary(pts, 8.0 * w)
    assert b['S'] == 8.0 * a['S'] and all(a[k].tobytes() == b[k].tobytes() for k in ('mean', 'covariance')) and a['n_eff'] == b['n_eff']


def test_arguments_of_the_restatements():
    x, lnl, w = wc.sample_set(20, 2, 'log-normal', 8)
    _, M, _ = W.integer_weights(w)
    for bad in ([], [0], [M + 1], list(range(1, 18))):
        with pytest.raises(ValueError):
            W.weighted_order_statistics(x, w, bad)
    assert W.weighted_order_statistics(x, w, [M] * 16).shape == (2, 16)
    for q in ([], [-0.1], [1.5], [np.nan], np.linspace(0, 1, 17)):
        with pytest.raises(ValueError, match='quantiles'):
            W.weighted_quantiles(x, w, q)
    with pytest.raises(ValueError):
        W.weighted_summary(x, w[:-1])
    with pytest.raises(ValueError):
        W.weighted_best(x, lnl[:-1])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='weights'):
            W.weighted_summary(x, np.where(np.arange(20) == 3, bad, w))
    both = W.summarise_sets([(x, lnl, w), (x[:0], lnl[:0], w[:0])], Q5)
    assert both['quantile_values'].shape == (2, 2, 5) and both['count'].tolist() == [20, 0] and np.isnan(both['best'][1]).all()


# ------------------------------------------------------------------ mutations of the restatement
MUTATIONS = ['> for >= in the walk', 'floor for ceil in the target', '2^31 for 2^32', 'reading past count', 'a tie to the higher row',
             'a sequential sum', 'the biased covariance', 'weights left out of the ranks']


def _restated(x, lnl, w, counts, n, q, mutate=None):
    """The definition over a store's buffers [E][capacity][...], with one line narrowed per mutation; ``mutate=None`` is the
    restatement.  Returns (mean, covariance, quantile values, best index) per set."""
    out = []
    for e, count in enumerate(counts.tolist()):
        c = min(count + 1, x.shape[1]) if mutate == 'reading past count' else count
        xe, le, we = x[e, :c], lnl[e, :c], w[e, :c]
        total = (lambda a: np.add.accumulate(a, axis=0)[-1]) if mutate == 'a sequential sum' else W.tree_sum
        mean, cov = np.full(n, np.nan), np.full((n, n), np.nan)
        scale = np.float64(2.0**31 if mutate == '2^31 for 2^32' else 2.0**32)
        m = ((we / we.max()) * scale).astype(np.uint64) if c and we.max() > 0.0 else np.zeros(c, dtype=np.uint64)
        if mutate == 'weights left out of the ranks':
            m = np.where(m > 0, np.uint64(1), m)
        M = sum(m.tolist())
        with np.errstate(all='ignore'):
            if c:
                S = np.float64(total(we))
                p = we / S
                s2 = np.float64(total(p * p))
                if S > 0.0:
                    mean = total(p[:, None] * xe)
                    if s2 < 1.0:
                        dx = xe - mean
                        for i in range(n):
                            cov[i] = total((p * dx[:, i])[:, None] * dx) / (1.0 if mutate == 'the biased covariance' else np.float64(1.0) - s2)
        values = np.full((n, len(q)), np.nan)
        if M > 0:
            t = [max(1, (Fraction(v) * M).__floor__() if mutate == 'floor for ceil in the target' else math.ceil(Fraction(v) * M)) for v in q]
            for d in range(n):
                keys = E.chain_keys(xe[:, d])
                order = np.argsort(keys, kind='stable')
                C = np.cumsum(m[order], dtype=np.uint64)
                at = np.searchsorted(C, np.array(t, dtype=np.uint64), side='right' if mutate == '> for >= in the walk' else 'left')
                values[d] = E.chain_unkeys(keys[order][np.minimum(at, c - 1)])
        real = ~np.isnan(le)
        index = -1
        if real.any():
            hits = np.flatnonzero(real & (le == le[real].max()))
            index = int(hits[-1] if mutate == 'a tie to the higher row' else hits[0])
        out.append((mean, cov, values, index))
    return out


def test_mutations_of_the_restatement_are_caught(driver):
    """Each narrowing of the definition changes an answer of a case above, so the cases can tell it from the header."""
    caught = {mu: False for mu in MUTATIONS}
    q = [0.0, 0.5, 1.0, 0.25, 0.84, 0.5 + 2.0**-40]
    # (two rows of equal weight: q M = 2^32 + 2^-7 lies between a cumulative sum and the target after it)
    for kind, variant, counts in [(k, v, (0, 1, 257)) for k in wc.WEIGHTS for v in (0, 4, 8)] + [('all equal', 8, (0, 1, 2))]:
        sets = wc.sets_of(257, 3, kind, variant, seed=1, counts=counts)
        x, lnl, w, counts = wc.store(sets, 260)
        # targets that sit on the cumulative sums of column 0 are quantiles q = C_i / M of it: a cumulative sum as a target
        m, M, _ = W.integer_weights(sets[2][2])
        qs = list(q)
        if M > 0:
            C = [c for c in wc.cumulative(sets[2][0][:, 0], m) if c > 0]
            on = Fraction(C[len(C) // 2], M)
            if on.denominator & (on.denominator - 1) == 0 and on.denominator <= 2**52:
                qs.append(float(on))
        targets = [W.weighted_targets(qs, s['total']) if s['total'] else [1] * len(qs) for s in (W.weighted_summary(a, c) for a, _, c in sets)]
        head = header_all(driver, sets, 260, targets)
        ours = _restated(x, lnl, w, counts, 3, qs)

        def differs(got):
            return any(not np.array_equal(g[0], head["mean"][e], equal_nan=True) or
                       not np.array_equal(np.tril(g[1]), np.tril(head["covariance"][e]), equal_nan=True) or
                       not np.array_equal(g[2], head['values'][e], equal_nan=True) or g[3] != head['index'][e]
                       for e, g in enumerate(got))
        assert not differs(ours), (kind, variant)
        for mu in MUTATIONS:
            caught[mu] = caught[mu] or differs(_restated(x, lnl, w, counts, 3, qs, mutate=mu))
    assert all(caught.values()), caught


# ------------------------------------------------------------------ the config key
def test_the_config_key():
    """``[Nested]`` / ``[SMC]`` ``weighted_quantiles``: parsed with ``mocks``; refused without, outside [0, 1], above 16 values."""
    import configparser
    for section in ('Nested', 'SMC'):
        def parse(text, mocks=True):
            cfg = configparser.ConfigParser()
            cfg[section] = {'weighted_quantiles': text} if text is not None else {}
            out = {'mocks': 3} if mocks else {}
            W.parse_weighted_quantiles(cfg[section], out, section)
            return out
        assert parse('0.025 0.16 0.5 0.84 0.975')['weighted_quantiles'] == Q5 and parse('0, 1')['weighted_quantiles'] == [0.0, 1.0]
        assert 'weighted_quantiles' not in parse(None) and 'weighted_quantiles' not in parse(None, mocks=False)
        for text in ('', '1.5', '-0.1 0.5', 'half', ' '.join(['0.5'] * 17)):
            with pytest.raises(ValueError, match=rf'\[{section}\] weighted_quantiles'):
                parse(text)
        with pytest.raises(ValueError, match=rf'\[{section}\] weighted_quantiles go with mocks'):
            parse('0.5', mocks=False)
