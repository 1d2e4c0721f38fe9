"""Order statistics and the best row of a recorded chain without a GPU: vega_amd/csrc/vmx_chain_select.h, compiled with g++ under
AddressSanitizer / UBSan (tests/helpers/chain_select_driver.cpp, a stand-alone program run as a subprocess), against its NumPy
restatements ``chain_order_statistics`` / ``chain_best`` bit for bit; the restatement against ``np.sort``; ``chain_quantiles``
against ``np.quantile(method='linear')`` under a bound derived below; and mutations of the restatement, each of which a case here
catches (docs/LAB_NOTES.md lists them)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import chain_select_cases as cases
from vega_amd import ensemble as E

REPO = Path(__file__).resolve().parents[1]

SHAPES = [(1, 2, 1), (85, 3, 1), (128, 2, 2), (86, 3, 3), (257, 6, 3), (300, 8, 64)]
ODD_FIRST = {1: 0, 85: 13, 128: 7, 86: 13, 257: 5, 300: 9}
SIGN = np.uint64(1 << 63)


# ------------------------------------------------------------------ the header
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('select') / 'chain_select_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'chain_select_driver.cpp')]
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


def _words(line):
    return np.array([int(v, 16) for v in line.split()], dtype=np.uint64)


def _store(chain, lnl, capacity, fill=0x7ff8dead0000beef):
    """The store's layout [E][capacity][...] around the rows, the slots past them filled with a word no column holds."""
    Ens, rows = chain.shape[:2]
    x = np.full((Ens, capacity) + chain.shape[2:], np.array([fill], dtype=np.uint64).view(np.float64)[0])
    x[:, :rows] = chain
    l = np.full((Ens, capacity) + chain.shape[2:3], 1e300)      # (a slot past the rows would win every best row)
    if lnl is not None:
        l[:, :rows] = lnl
    return x, l


def _header_stats(exe, chain, capacity, first, ranks):
    Ens, rows, W, n = chain.shape
    x, _ = _store(chain, None, capacity)
    line = _ask(exe, f'S {Ens} {capacity} {rows} {W} {n} {first} {len(ranks)} {" ".join(str(int(r)) for r in ranks)} {_hex(x)}')[0]
    return _words(line).view(np.float64).reshape(Ens, n, len(ranks))


def _header_best(exe, chain, lnl, capacity, first, position=True):
    Ens, rows, W, n = chain.shape
    x, l = _store(chain, lnl, capacity)
    lines = _ask(exe, f'B {Ens} {capacity} {rows} {W} {n} {first} {int(position)} {_hex(x)} {_hex(l)}')
    out = dict(lnl_max=_words(lines[0]).view(np.float64), best_row=np.array(lines[1].split(), dtype=np.int64),
               best_walker=np.array(lines[2].split(), dtype=np.int32))
    if position:
        out['best'] = _words(lines[3]).view(np.float64).reshape(Ens, n)
    return out


def _same_best(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.asarray(a[key]).dtype == np.asarray(b[key]).dtype, key
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def test_keys(driver):
    """key / unkey of the header and of the restatement on words of every class; the keys order them as the definition says."""
    words = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x3ff0000000000000,
                      0xbff0000000000000, 0x7fefffffffffffff, 0xffefffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                      0x7ff0000000000001, 0xfff0000000000001, 0x7ff8000000000000, 0xfff8000000000000, 0xffffffffffffffff,
                      0x7fffffffffffffff], dtype=np.uint64)
    lines = _ask(driver, f'K {words.size} ' + ' '.join(f'{w:016x}' for w in words.tolist()))
    keys, back = _words(lines[0]), _words(lines[1])
    ours = E.chain_keys(words.view(np.float64))
    assert np.array_equal(keys, ours) and np.array_equal(back, E.chain_unkeys(ours).view(np.uint64))
    nan = np.isnan(words.view(np.float64))
    assert np.all(keys[nan] == np.uint64(2**64 - 1)) and np.all(back[nan] == np.uint64(0x7ff8000000000000))
    assert np.array_equal(back[~nan], words[~nan]) and np.all(keys[~nan] < np.uint64(2**64 - 1))
    order = [0xfff0000000000000, 0xffefffffffffffff, 0xbff0000000000000, 0x8000000000000001, 0x8000000000000000, 0x0000000000000000,
             0x0000000000000001, 0x3ff0000000000000, 0x7fefffffffffffff, 0x7ff0000000000000, 0x7ff8000000000000]
    k = E.chain_keys(np.array(order, dtype=np.uint64).view(np.float64))
    assert np.all(k[1:] > k[:-1])


def test_the_count_limit(driver):
    """N = T W >= 2^31 is what vmx_chain_store_order_stats refuses by this function of the header (a store of that size takes
    tens of GiB to fill: the refusal is held here, not on the GPU)."""
    asked = [(1, 2), (2**21 - 1, 1024), (2**21, 1024), (2**31 - 1, 1), (2**31, 1), (2**40, 1024), (2097152, 1023), (2099203, 1023)]
    lines = _ask(driver, ' '.join(f'N {T} {W}' for T, W in asked))
    assert [int(v) for v in lines] == [int(T * W < 2**31) for T, W in asked] == [1, 1, 0, 1, 0, 0, 1, 0]


@pytest.mark.parametrize('T, W, n', SHAPES)
def test_the_header_equals_the_restatement(driver, T, W, n):
    """Bit for bit: two ensembles in a store with room past its rows, first row 0 and an odd one, R = 1 and R = 32 (unsorted, with
    repeats, 0 and N - 1 among them), every kind of column at every shape.  The restatement against ``np.sort``: equal as values
    where the kind has no NaN (a +0 / -0 pair compares equal, whichever of the two np.sort puts first), position for position with
    NaN == NaN where it has, and bit for bit where it has neither."""
    variants = range(len(cases.KIND_NAMES)) if 2 * n < len(cases.KIND_NAMES) else [0]
    for variant in variants:
        chain = cases.chain(2, T, W, n, variant, seed=1)
        for first in sorted({0, ODD_FIRST[T]}):
            N = (T - first) * W
            for R in (1, 32):
                ranks = cases.ranks_of(N, R, seed=variant)
                ours = E.chain_order_statistics(chain, ranks, first)
                assert ours.shape == (2, n, R)
                assert _header_stats(driver, chain, T + 3, first, ranks).tobytes() == ours.tobytes(), (variant, first, R)
                for e in range(2):
                    for d in range(n):
                        zeros, nans = cases.KINDS[cases.kind_of(2, n, variant, e, d)]
                        ref = np.sort(chain[e, first:, :, d].reshape(-1))[ranks]
                        if nans:
                            assert np.array_equal(ours[e, d], ref, equal_nan=True)
                            assert np.all(ours[e, d][np.isnan(ref)].view(np.uint64) == np.uint64(0x7ff8000000000000))
                        elif zeros:
                            assert np.array_equal(ours[e, d], ref)
                        else:
                            assert ours[e, d].tobytes() == ref.tobytes()
    # one ensemble of a stack is its own answer, whatever the other ranks asked, their order or their number
    one = E.chain_order_statistics(chain[1], ranks[:5][::-1], first)
    assert one.tobytes() == np.ascontiguousarray(ours[1][:, :5][:, ::-1]).tobytes()


def test_zeros_sort_by_sign(driver):
    """-0 before +0, in the header and the restatement alike (np.sort leaves it open)."""
    chain = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.0]).reshape(1, 3, 2, 1)
    ours = E.chain_order_statistics(chain, np.arange(6))
    assert list(np.signbit(ours[0, 0])) == [True, True, True, False, False, False] and ours[0, 0, 5] == 1.0
    assert _header_stats(driver, chain, 3, 0, np.arange(6)).tobytes() == ours.tobytes()


@pytest.mark.parametrize('T, W, n', SHAPES)
def test_the_best_row(driver, T, W, n):
    """Five ensembles, one per kind of lnL block: ties resolve to the lowest (row, walker), a NaN never wins, -inf may, a block
    that is all NaN gives -1; header and restatement bit for bit, with and without the position."""
    chain, lnl = cases.chain(5, T, W, n, 0, seed=2), cases.lnl_block(5, T, W, seed=2)
    for first in sorted({0, ODD_FIRST[T]}):
        ours = E.chain_best(chain, lnl, first)
        _same_best(_header_best(driver, chain, lnl, T + 2, first), ours)
        got = _header_best(driver, chain, lnl, T + 2, first, position=False)
        assert 'best' not in got and got['best_row'].tobytes() == ours['best_row'].tobytes()
        for e in range(5):
            flat = lnl[e, first:].reshape(-1)
            row, walker = int(ours['best_row'][e]), int(ours['best_walker'][e])
            if np.all(np.isnan(flat)):
                assert (row, walker) == (-1, -1) and np.isnan(ours['lnl_max'][e]) and np.all(np.isnan(ours['best'][e]))
                continue
            assert first <= row < T and 0 <= walker < W
            top = np.nanmax(flat)
            assert ours['lnl_max'][e] == top and not np.isnan(lnl[e, row, walker])
            assert (row - first) * W + walker == int(np.flatnonzero(flat == top)[0])
            assert ours['best'][e].tobytes() == chain[e, row, walker].tobytes()
        if T * W >= 6:
            assert ours['lnl_max'][3] == -np.inf and ours['best_row'][3] >= first
    single = E.chain_best(chain[1], lnl[1], 0)
    assert isinstance(single['lnl_max'], float) and single['best'].shape == (n,) and single['best_row'] == E.chain_best(chain, lnl)['best_row'][1]


# ------------------------------------------------------------------ quantiles against NumPy's
def test_quantiles_against_numpy():
    """``chain_quantiles`` against ``np.quantile(method='linear')`` over finite columns.

    The bound, with u = 2^-53, m = max(|x_lo|, |x_hi|) and d = x_hi - x_lo (|d| <= 2 m).  Either side evaluates a + t d (NumPy
    for t >= 0.5 the mirrored b - (1 - t) d) with a rounded difference, a rounded product, a rounded sum and, mirrored, a rounded
    1 - t: at most u (3 |d| + m) <= 7 u m away from the exact a + t d of its own t; both sides 14 u m.  The two fractional ranks:
    this code forms h = fl(q (N - 1)), off the exact q (N - 1) by at most u (N - 1); NumPy forms fl(fl(fl(N q) + fl(1 - q)) - 1),
    off by at most u N + u + u (N + 1) + u N; together less than u (4 N + 2).  The interpolant is continuous and piecewise linear
    in the fractional rank with the gaps between neighbouring order statistics as slopes, so that difference moves the value by
    at most u (4 N + 2) times the largest gap next to the rank (the ranks lo - 1 .. lo + 2).  Hence
        |ours - numpy| <= 14 u m + u (4 N + 2) gap.
    Measured here (printed): the worst difference is below 2 u m."""
    u = 2.0**-53
    q = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0, 1.0 / 3.0, 0.999])
    worst = 0.0
    for T, W, seed in ((1, 2, 0), (85, 3, 1), (128, 2, 2), (257, 6, 3), (625, 8, 4)):
        rng = np.random.default_rng(seed)
        cols = [cases.column(kind, T * W, rng) for kind in ('normal', 'two values', 'lowest byte', '56 leading bits', 'all equal')]
        cols.append(1e3 * rng.standard_normal(T * W))
        chain = np.stack(cols, axis=-1).reshape(T, W, len(cols))
        for first in (0, T // 3):
            ours = E.chain_quantiles(chain, q, first)
            flat = chain[first:].reshape(-1, len(cols))
            N = flat.shape[0]
            ref = np.quantile(flat, q, axis=0, method='linear').T
            srt = np.sort(flat, axis=0)
            lo = np.floor(q * (N - 1)).astype(int)
            for d in range(len(cols)):
                for k in range(q.size):
                    near = srt[max(lo[k] - 1, 0):lo[k] + 3, d]
                    gap = float(np.max(np.diff(near))) if near.size > 1 else 0.0
                    m = float(np.max(np.abs(near)))
                    bound = 14 * u * m + u * (4 * N + 2) * gap
                    diff = abs(ours[d, k] - ref[d, k])
                    worst = max(worst, diff / (u * m))
                    assert diff <= bound, (T, W, first, d, k, diff, bound)
    print(f'chain_quantiles against np.quantile: worst difference {worst:.2f} u max(|x_lo|, |x_hi|)')
    # the ends are order statistics themselves, and a stack is its members
    x = cases.chain(2, 86, 3, 3, 8, seed=5)
    both = E.chain_quantiles(x, [0.0, 1.0, 0.5], 13)
    assert both.shape == (2, 3, 3) and both[1].tobytes() == E.chain_quantiles(x[1], [0.0, 1.0, 0.5], 13).tobytes()
    N = 73 * 3
    assert np.array_equal(both[:, :, :2], E.chain_order_statistics(x, [0, N - 1], 13), equal_nan=True)


def test_arguments_of_the_restatements():
    x, lnl = cases.chain(2, 10, 3, 2, 8), cases.lnl_block(2, 10, 3)
    for bad in (dict(ranks=[]), dict(ranks=np.arange(33)), dict(ranks=[-1]), dict(ranks=[30]), dict(ranks=[0], first=10),
                dict(ranks=[0], first=-1), dict(ranks=[27], first=1)):
        with pytest.raises(ValueError):
            E.chain_order_statistics(x, **bad)
    assert E.chain_order_statistics(x, [26], first=1).shape == (2, 2, 1)
    for q in ([], [-0.1], [1.5], [np.nan], np.linspace(0, 1, 17)):
        with pytest.raises(ValueError, match='quantiles'):
            E.chain_quantiles(x, q)
    assert E.chain_quantiles(x, np.linspace(0, 1, 16)).shape == (2, 2, 16)
    with pytest.raises(ValueError):
        E.chain_best(x, lnl[:, :9])
    with pytest.raises(ValueError):
        E.chain_best(x, lnl, first=10)


# ------------------------------------------------------------------ mutations of the restatement
MUTATIONS = ['a key without the sign flip', 'a rank off by one', 'rows as the stride', 'first_row ignored', 'a tie to the highest index',
             'NaN as the largest lnL', 'NaN keys sorted first']


def _restated(x, l, Ens, capacity, rows, W, n, first, ranks, mutate=None):
    """The definition over a store's flat buffers, with one line narrowed per mutation; ``mutate=None`` is the restatement."""
    stride = rows if mutate == 'rows as the stride' else capacity
    chain = np.stack([x[e * stride * W * n:][:rows * W * n].reshape(rows, W, n) for e in range(Ens)])
    lnl = np.stack([l[e * stride * W:][:rows * W].reshape(rows, W) for e in range(Ens)])
    f = 0 if mutate == 'first_row ignored' else first
    N = (rows - f) * W
    flat = np.moveaxis(chain[:, f:], 3, 1).reshape(Ens, n, N)
    b = np.ascontiguousarray(flat).view(np.uint64)
    keys = np.where((b & SIGN) != 0, ~b, b if mutate == 'a key without the sign flip' else b | SIGN)
    keys = np.where(np.isnan(flat), np.uint64(0) if mutate == 'NaN keys sorted first' else np.uint64(2**64 - 1), keys)
    take = np.minimum(ranks + 1, N - 1) if mutate == 'a rank off by one' else ranks
    order = np.argsort(keys, axis=-1, kind='stable')
    stats = np.take_along_axis(flat, order, axis=-1)[:, :, take]
    stats = np.where(np.isnan(stats), np.float64(np.nan), stats)
    best = []
    for e in range(Ens):
        v = lnl[e, f:].reshape(-1)
        cand = np.where(np.isnan(v), np.inf if mutate == 'NaN as the largest lnL' else -np.inf, v)
        real = np.ones(v.size, dtype=bool) if mutate == 'NaN as the largest lnL' else ~np.isnan(v)
        if not real.any():
            best.append((-1, -1))
            continue
        hits = np.flatnonzero(real & (cand == cand[real].max()))
        at = int(hits[-1] if mutate == 'a tie to the highest index' else hits[0]) + f * W
        best.append((at // W, at % W))
    return stats, best


def test_mutations_of_the_restatement_are_caught(driver):
    """Each narrowing of the definition changes an answer of a case above, so the cases can tell it from the header."""
    Ens, T, W, n, capacity, first = 2, 86, 3, 3, 100, 13
    caught = {m: False for m in MUTATIONS}
    for variant in range(len(cases.KIND_NAMES)):
        chain, lnl = cases.chain(Ens, T, W, n, variant, seed=1), cases.lnl_block(5, T, W, seed=2)[[0, 1]]
        ranks = cases.ranks_of((T - first) * W, 32, seed=variant)
        x, l = _store(chain, lnl, capacity)
        stats = _header_stats(driver, chain, capacity, first, ranks)
        top = _header_best(driver, chain, lnl, capacity, first)
        where = list(zip(top['best_row'].tolist(), top['best_walker'].tolist()))
        ours, ours_best = _restated(x.reshape(-1), l.reshape(-1), Ens, capacity, T, W, n, first, ranks)
        assert ours.tobytes() == stats.tobytes() == E.chain_order_statistics(chain, ranks, first).tobytes() and ours_best == where
        for m in MUTATIONS:
            got, got_best = _restated(x.reshape(-1), l.reshape(-1), Ens, capacity, T, W, n, first, ranks, mutate=m)
            caught[m] = caught[m] or got.tobytes() != stats.tobytes() or got_best != where
    assert all(caught.values()), caught
