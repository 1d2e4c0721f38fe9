"""Inputs shared by tests/test_chain_select_host.py and tests/test_chain_quantiles_gpu.py: chains whose columns are built from bit
patterns that a radix select over 8-bit digits can get wrong, lnL blocks with ties and NaNs, and unsorted rank lists."""
import numpy as np

# kind -> (a +0 / -0 pair may occur, a NaN may occur): what a comparison with np.sort may assume (np.sort leaves the order of -0
# and +0 open, and NaN != NaN)
KINDS = {
    'all equal': (False, False),
    'two values': (False, False),
    'lowest byte': (False, False),
    'highest byte': (False, False),
    '56 leading bits': (False, False),
    'mixed': (True, False),
    'one nan': (False, True),
    'several nans': (True, True),
    'normal': (False, False),
}
KIND_NAMES = list(KINDS)


def _bits(words):
    return np.asarray(words, dtype=np.uint64).view(np.float64)


def column(kind, N, rng):
    """N doubles of the kind, in an order drawn by ``rng``."""
    if kind == 'all equal':
        return np.full(N, _bits([0x3fe51eb851eb851f])[0])
    if kind == 'two values':
        return _bits(np.where(rng.random(N) < 0.4, np.uint64(0x3ff0000000000001), np.uint64(0x3ff0000000000000)))
    if kind == 'lowest byte':
        return _bits(np.uint64(0x4008f5c28f5c2800) | rng.integers(0, 256, N).astype(np.uint64))
    if kind == 'highest byte':          # (the low 56 bits keep the exponent from being all ones: every value is finite)
        return _bits((rng.integers(0, 256, N).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789abcd))
    if kind == '56 leading bits':       # (negative: the key order runs against the bits)
        return _bits(np.uint64(0xbfd3c0ca4283de00) | rng.integers(0, 256, N).astype(np.uint64))
    if kind == 'mixed':
        pool = np.concatenate([[0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, -1e-310, 1.0, -1.0],
                               rng.standard_normal(6) * 1e3])
        return pool[rng.integers(0, pool.size, N)]
    if kind == 'one nan':
        x = rng.standard_normal(N)
        x[rng.integers(0, N)] = np.nan
        return x
    if kind == 'several nans':
        x = np.concatenate([rng.standard_normal(N), [0.0, -0.0]])[rng.integers(0, N + 2, N)]
        nans = _bits([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123, 0xfffc00000000beef, 0x7ff4000000000001])
        hit = rng.random(N) < 0.3
        hit[rng.integers(0, N)] = True
        x[hit] = nans[rng.integers(0, nans.size, int(hit.sum()))]
        return x
    return 1.0 + 0.05 * rng.standard_normal(N)


def kind_of(E, n, variant, e, d):
    return KIND_NAMES[(variant + e * n + d) % len(KIND_NAMES)]


def chain(E, rows, W, n, variant=0, seed=0):
    """[E, rows, W, n]: column d of ensemble e is of ``kind_of(E, n, variant, e, d)``."""
    rng = np.random.default_rng([seed, E, rows, W, n, variant])
    x = np.empty((E, rows, W, n))
    for e in range(E):
        for d in range(n):
            x[e, :, :, d] = column(kind_of(E, n, variant, e, d), rows * W, rng).reshape(rows, W)
    return x


def lnl_block(E, rows, W, seed=0):
    """[E, rows, W], ensemble e of kind e % 5: 0 - the maximum several times over (and +0 / -0 ties); 1 - NaNs around a maximum
    that is not first; 2 - all NaN; 3 - only NaN and -inf; 4 - plain."""
    rng = np.random.default_rng([seed, E, rows, W])
    out = np.empty((E, rows, W))
    for e in range(E):
        v = -np.abs(rng.standard_normal(rows * W)) - 1.0
        k = e % 5
        if k == 0:
            v[rng.integers(0, v.size, max(v.size // 3, 1))] = 0.0
            v[rng.integers(0, v.size, max(v.size // 3, 1))] = -0.0
        elif k == 1:
            v[rng.random(v.size) < 0.5] = np.nan
            v[rng.integers(0, v.size, 2)] = 3.5
        elif k == 2:
            v[:] = _bits([0xfff8000000000000])[0]
        elif k == 3:
            v[:] = np.nan
            v[rng.integers(0, v.size, max(v.size // 2, 1))] = -np.inf
        out[e] = v.reshape(rows, W)
    return out


def ranks_of(N, R, seed=0):
    """R ranks in [0, N), unsorted, with repeats; R >= 2 includes 0 and N - 1 (and a repeat of each when R >= 4)."""
    rng = np.random.default_rng([seed, N, R])
    if R == 1:
        return np.array([int(rng.integers(0, N))], dtype=np.int64)
    fixed = [N - 1, 0] + ([0, N - 1] if R >= 4 else [])
    ranks = np.concatenate([fixed, rng.integers(0, N, R - len(fixed))]).astype(np.int64)
    return ranks[rng.permutation(R)]
