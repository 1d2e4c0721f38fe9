"""Weighted, ragged sample sets: the summary, the order statistics and the best point of the posterior samples of a nested or an
SMC run - vega_amd/csrc/vmx_chain_weighted.h restated in NumPy, bit for bit.  A set is ``(x [count, n], lnl [count], w [count])``
with finite weights >= 0 that need not sum to 1; ``count = 0`` is a set.  What :class:`vega_amd.engine.SampleStore` computes on
the device, these functions compute on the host: the ``python`` driver, an engine group and ``where='host'`` use them."""
from fractions import Fraction

import numpy as np

from .ensemble import chain_keys, chain_unkeys, check_quantiles

SAMPLE_MAX_TARGETS = 16
SAMPLE_MAX_COUNT = 2**31 - 1
_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
QMETHOD = 'inverted_cdf'


def padded(count):
    """The terms of a tree: the least power of two >= max(count, 2)."""
    M = 2
    while M < count:
        M <<= 1
    return M


def tree_sum(a):
    """The stride-halving tree over the first axis of ``a``, padded with +0 to ``padded(count)`` terms (vmx_wchain::tree_sum)."""
    a = np.asarray(a, dtype=np.float64)
    M = padded(a.shape[0])
    a = np.concatenate([a, np.zeros((M - a.shape[0],) + a.shape[1:])])
    s = M // 2
    with np.errstate(invalid='ignore', over='ignore'):
        while s >= 1:
            a = a[:s] + a[s:2 * s]
            s //= 2
    return a[0]


def _canonical(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), _NAN, v)


def check_weights(w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or w.size > SAMPLE_MAX_COUNT:
        raise ValueError('weights: one per row')
    if not np.all((w >= 0.0) & np.isfinite(w)):
        raise ValueError('weights: finite and >= 0')
    return w


def integer_weights(w):
    """``(m, M, w_max)``: ``m_i = floor(w_i / w_max 2^32)`` as uint64 - one correctly rounded division, an exact scaling, a
    truncation - their sum ``M`` (a Python integer) and the largest weight (0 for an empty set, where every m is 0)."""
    w = check_weights(w)
    w_max = float(w.max()) if w.size else 0.0
    if not w_max > 0.0:
        return np.zeros(w.size, dtype=np.uint64), 0, w_max
    m = ((w / np.float64(w_max)) * np.float64(4294967296.0)).astype(np.uint64)
    return m, sum(m.tolist()), w_max


def weighted_summary(x, w):
    """``dict(count, S, n_eff, mean [n], sd [n], covariance [n, n], total, w_max)`` of one set: p = w / S, mean = sum p x,
    covariance = sum p dx dx^T / (1 - sum p^2) in two passes, n_eff = 1 / sum p^2, every sum the stride-halving tree.  NaN where
    the set cannot say: count = 0 or S = 0 (mean, covariance, n_eff), one row with all the weight (covariance)."""
    x, w = np.asarray(x, dtype=np.float64), check_weights(w)
    if x.ndim != 2 or x.shape[0] != w.size or x.shape[1] < 1:
        raise ValueError('x [count, n] with one weight per row')
    count, n = x.shape
    m, M, w_max = integer_weights(w)
    mean, cov, n_eff, S = np.full(n, _NAN), np.full((n, n), _NAN), _NAN, 0.0
    if count >= 1:
        S = np.float64(tree_sum(w))
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            p = w / S
            s2 = np.float64(tree_sum(p * p))
            if S > 0.0:
                n_eff = float(_canonical(np.float64(1.0) / s2))
                mean = _canonical(tree_sum(p[:, None] * x))
                if s2 < 1.0:
                    dx = x - mean
                    for i in range(n):
                        cov[i, :i + 1] = _canonical(tree_sum((p * dx[:, i])[:, None] * dx[:, :i + 1]) / (np.float64(1.0) - s2))
                        cov[:i + 1, i] = cov[i, :i + 1]
    with np.errstate(invalid='ignore'):
        sd = np.sqrt(np.diagonal(cov))
    return dict(count=count, S=float(S), n_eff=float(n_eff), mean=mean, sd=sd, covariance=cov, total=M, w_max=w_max)


def weighted_targets(q, M):
    """The targets of the quantiles ``q`` in a set of total integer weight ``M``: ``max(1, ceil(q M))``, exactly (``q`` is a
    dyadic rational, ``M`` an integer: no double product).  A list of Python integers."""
    q = check_quantiles(q)
    M = int(M)
    out = []
    for v in q.tolist():
        t = Fraction(v) * M
        out.append(max(1, -((-t.numerator) // t.denominator)))
    return out


def weighted_order_statistics(x, w, targets):
    """Weighted order statistics of every column of one set: entry r of column d is the smallest stored value v, in the total
    order of :func:`vega_amd.ensemble.chain_keys`, with ``sum_{x_i <= v} m_i >= targets[r]`` - that value's own bits, or the
    canonical NaN.  ``targets``: 1 .. 16 whole numbers in [1, M] in any order, repeats allowed; a set with M = 0 ignores them and
    answers NaN.  Returns [n, R]."""
    x = np.asarray(x, dtype=np.float64)
    m, M, _ = integer_weights(w)
    if x.ndim != 2 or x.shape[0] != m.size or x.shape[1] < 1:
        raise ValueError('x [count, n] with one weight per row')
    targets = [int(t) for t in np.atleast_1d(np.asarray(targets, dtype=object)).tolist()]
    if not 1 <= len(targets) <= SAMPLE_MAX_TARGETS:
        raise ValueError(f'targets: 1 .. {SAMPLE_MAX_TARGETS} of them')
    n = x.shape[1]
    if M == 0:
        return np.full((n, len(targets)), _NAN)
    if any(t < 1 or t > M for t in targets):
        raise ValueError(f'targets: 1 .. {M}')
    out = np.empty((n, len(targets)), dtype=np.uint64)
    t = np.array(targets, dtype=np.uint64)
    for d in range(n):
        keys = chain_keys(x[:, d])
        order = np.argsort(keys, kind='stable')
        cumulative = np.cumsum(m[order], dtype=np.uint64)
        out[d] = keys[order][np.searchsorted(cumulative, t, side='left')]
    return chain_unkeys(out)


def weighted_quantiles(x, w, q):
    """The inverted-CDF quantiles ``q`` of every column of one set, [n, Q]: the order statistics at :func:`weighted_targets`."""
    _, M, _ = integer_weights(w)
    return weighted_order_statistics(x, w, weighted_targets(q, M) if M > 0 else [1] * check_quantiles(q).size)


def weighted_best(x, lnl):
    """``dict(lnl_max, index, best [n])``: the row of the largest lnL - a NaN never wins, ties go to the lowest row; index -1 and
    NaNs where no row is a candidate.  Weights play no part."""
    x, lnl = np.asarray(x, dtype=np.float64), np.asarray(lnl, dtype=np.float64)
    if x.ndim != 2 or lnl.shape != x.shape[:1]:
        raise ValueError('x [count, n], lnl [count]')
    valid = ~np.isnan(lnl)
    if not np.any(valid):
        return dict(lnl_max=float(_NAN), index=-1, best=np.full(x.shape[1], _NAN))
    index = int(np.argmax(valid & (lnl == lnl[valid].max())))
    return dict(lnl_max=float(lnl[index]), index=index, best=x[index].copy())


def summarise_sets(sets, q=None):
    """The host summary of a list of sets ``(x, lnl, w)`` stacked per set, as :meth:`SampleStore` users get it from the device:
    ``dict(count [E], n_eff [E], mean [E, n], sd [E, n], covariance [E, n, n])`` and with ``q`` also ``weighted_quantiles [Q]``,
    ``quantile_values [E, n, Q]``, ``lnl_max [E]`` and ``best [E, n]``."""
    parts = [weighted_summary(x, w) for x, _, w in sets]
    out = {key: np.array([p[key] for p in parts]) for key in ('count', 'n_eff', 'mean', 'sd', 'covariance')}
    if q is not None:
        q = check_quantiles(q)
        tops = [weighted_best(x, lnl) for x, lnl, _ in sets]
        out.update(weighted_quantiles=q, quantile_values=np.array([weighted_quantiles(x, w, q) for x, _, w in sets]),
                   lnl_max=np.array([t['lnl_max'] for t in tops]), best=np.array([t['best'] for t in tops]))
    return out


def summarise_runs(sampler, found, q=None, where='device'):
    """What ``NestedSet.summary`` and ``SMCSet.summary`` share: ``found`` is a list over the runs of ``(points, lnL, weights)``
    (None: a run without samples, a set with count = 0).  ``where='device'`` on the ``device`` driver puts every run's samples
    into a :class:`vega_amd.engine.SampleStore` and reduces them there; ``'host'``, the ``python`` driver and an engine group use
    the restatements above.  Both give the same bits."""
    if where not in ('device', 'host'):
        raise ValueError("where: 'device' or 'host'")
    if q is not None:
        q = check_quantiles(q)
    n = sampler.n
    sets = [(np.empty((0, n)), np.empty(0), np.empty(0)) if part is None else
            tuple(np.ascontiguousarray(a, dtype=np.float64) for a in part) for part in found]
    if where == 'host' or getattr(sampler, 'driver', 'python') != 'device':   # (a set over a plain function has no engine)
        return summarise_sets(sets, q)
    store = sampler.vega.engine.sample_store(len(sets), n, max(1, max(len(s[2]) for s in sets)))
    try:
        for e, (x, lnl, w) in enumerate(sets):
            store.put(e, x, lnl, w)
        summ = store.summary()
        out = {key: summ[key] for key in ('count', 'n_eff', 'mean', 'sd', 'covariance')}
        if q is not None:
            top = store.best()
            out.update(weighted_quantiles=q, quantile_values=store.weighted_quantiles(q, total=summ['total']), lnl_max=top['lnl_max'],
                       best=top['best'])
    finally:
        store.close()
    return out


def parse_weighted_quantiles(sec, out, section):
    """``weighted_quantiles = q0 q1 ...`` of ``[Nested]`` / ``[SMC]`` (1 .. 16 values in [0, 1]) into ``out['weighted_quantiles']``:
    with ``mocks = M`` the table ``mock_posteriors.fits`` gains every parameter's inverted-CDF quantiles and best point.  Without
    the key nothing is added.  Refused without ``mocks`` (a single run writes its weighted chain for getdist)."""
    if 'weighted_quantiles' not in sec:
        return
    try:
        q = [float(v) for v in sec.get('weighted_quantiles').replace(',', ' ').split()]
    except ValueError:
        raise ValueError(f'[{section}] weighted_quantiles: numbers in [0, 1]') from None
    try:
        q = check_quantiles(q) if q else check_quantiles(np.empty(0))
    except ValueError as err:
        raise ValueError(f'[{section}] weighted_{err}') from None
    if 'mocks' not in out:
        raise ValueError(f'[{section}] weighted_quantiles go with mocks = M: a single run writes its chain for getdist')
    out['weighted_quantiles'] = [float(v) for v in q]
