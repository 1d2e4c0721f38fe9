"""Inputs shared by tests/test_chain_weighted_host.py and tests/test_sample_store_gpu.py: weighted, ragged sample sets whose columns
are the adversarial bit patterns of tests/chain_select_cases.py, weights of every kind the definition treats apart, and target
lists that sit on the cumulative sums."""
import numpy as np

import chain_select_cases as cases
from vega_amd import weighted as W
from vega_amd.ensemble import chain_keys

WEIGHTS = ['all equal', 'one dominant', 'a third zero', 'beyond 2^32', 'all zero', 'log-normal']
SHAPES = [(1, 1), (2, 1), (255, 2), (256, 1), (257, 3), (300, 64)]
FILL = 0x7ff8dead0000beef


def weights(kind, count, rng):
    """``count`` finite weights >= 0 of the kind (not normalised)."""
    if kind == 'all equal':
        return np.full(count, 0.7)
    if kind == 'all zero' or count == 0:
        return np.zeros(count)
    w = np.exp(rng.standard_normal(count))
    if kind == 'one dominant':
        w[rng.integers(0, count)] = 1e9
    elif kind == 'a third zero':
        w[rng.random(count) < 1.0 / 3.0] = 0.0
    elif kind == 'beyond 2^32':          # (ln 2^32 = 22.2: with a width of 30 many rows truncate to m = 0)
        w = np.exp(30.0 * rng.standard_normal(count))
    return w


def sample_set(count, n, kind, variant=0, seed=0, equal_x=False):
    """One set ``(x [count, n], lnl [count], w [count])``: the columns of ``chain_select_cases`` (NaNs that carry weight and +-0
    among them), the lnL blocks of its ``lnl_block`` (ties, NaNs), the weights of ``kind``; ``equal_x``: one value in every row."""
    rng = np.random.default_rng([seed, count, n, variant, WEIGHTS.index(kind)])
    x = cases.chain(1, count, 1, n, variant, seed=seed)[0, :, 0, :] if count else np.empty((0, n))
    if equal_x and count:
        x = np.broadcast_to(x[:1], x.shape).copy()
    lnl = cases.lnl_block(5, count, 1, seed=seed)[variant % 5, :, 0] if count else np.empty(0)
    return np.ascontiguousarray(x), np.ascontiguousarray(lnl), weights(kind, count, rng)


def sets_of(count, n, kind, variant=0, seed=0, counts=None):
    """The sets of a store: rows (0, 1, count) unless ``counts`` says otherwise."""
    counts = (0, 1, count) if counts is None else counts
    return [sample_set(c, n, kind, variant + k, seed) for k, c in enumerate(counts)]


def store(sets, capacity, fill=FILL):
    """The store's layout [E][capacity][...] around the sets, the slots past a set's rows filled with what would show: a word no
    column holds, an lnL that would win every best point, a weight that would dominate every sum."""
    E, n = len(sets), sets[0][0].shape[1]
    x = np.full((E, capacity, n), np.array([fill], dtype=np.uint64).view(np.float64)[0])
    lnl, w = np.full((E, capacity), 1e300), np.full((E, capacity), 1e30)
    for e, (xe, le, we) in enumerate(sets):
        x[e, :len(we)], lnl[e, :len(we)], w[e, :len(we)] = xe, le, we
    return x, lnl, w, np.array([len(s[2]) for s in sets], dtype=np.int64)


def cumulative(x_column, m):
    """The cumulative integer weights of a column in key order (Python integers)."""
    order = np.argsort(chain_keys(x_column), kind='stable')
    out, total = [], 0
    for v in m[order].tolist():
        total += v
        out.append(total)
    return out


def targets_of(one, R, seed=0):
    """R targets of a set in [1, M], unsorted: R = 1 a drawn one; R >= 6 holds 1 and M, a cumulative sum C_i of column 0 and
    C_i + 1, and repeats.  A set with M = 0 gets ones (they are ignored)."""
    x, _, w = one
    m, M, _ = W.integer_weights(w)
    if M == 0:
        return [1] * R
    rng = np.random.default_rng([seed, len(w), R])
    draw = lambda: int(rng.integers(1, min(M, 2**62), endpoint=True))
    if R == 1:
        return [draw()]
    C = [c for c in cumulative(x[:, 0], m) if c > 0]
    at = C[int(rng.integers(0, len(C)))]
    fixed = [1, M, at, min(at + 1, M), M, 1, at]
    out = (fixed + [draw() for _ in range(max(R - len(fixed), 0))])[:R]
    return [out[k] for k in rng.permutation(len(out))]
