"""Posterior sampling: the affine-invariant ensemble sampler (Goodman & Weare 2010, emcee's stretch move with
randomize_split=False; on request the differential-evolution, snooker and covariance moves and mixtures of them), run where the
walkers are.

The reference samples through PolyChord / pocoMC (bin/run_vega_mpi.py: ``[control] run_sampler = True``), which call
``log_lik`` one point at a time.  Here W walkers advance half an ensemble at a time: the ``device`` driver runs the whole walker
loop on the GPU (include/vegamx.h: vmx_ensemble_run - one small kernel per half-step, the engine's chain over the half's rows,
one host synchronisation per call); the ``python`` driver is the readable restatement of the same algorithm in NumPy over
``VegaInterface.chi2_batch_device``.  Both follow vega_amd/csrc/vmx_ensemble.h decision for decision, so that they produce the
same chain bit for bit.  The random stream is NumPy's Philox4x64-10 (one block per walker-in-half, step and half).
"""
import configparser
import math
import os
from collections.abc import Mapping
from pathlib import Path

import numpy as np

# ------------------------------------------------------------------ the algorithm (vmx_ensemble.h) in NumPy
_PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
_PHILOX_W = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B))
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """(high, low) 64-bit words of the 128-bit products a * b (uint64 arrays)."""
    a_lo, a_hi, b_lo, b_hi = a & _M32, a >> _S32, b & _M32, b >> _S32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32), a * b


def philox4x64_10(counter, key):
    """Random123 Philox4x64-10 of counters [..., 4] (word 0 least significant) under the key (k0, k1): blocks [..., 4] uint64.
    Equal to ``np.random.Philox(key=[k0, k1], counter=(c - 1) mod 2**256).random_raw(4)`` for the counter c."""
    c = np.array(counter, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    shape = c0.shape
    # (a key word may be an array that broadcasts against the counters' shape: the blocks of many streams in one pass)
    k0 = np.broadcast_to(np.asarray(key[0], dtype=np.uint64), shape).copy()
    k1 = np.broadcast_to(np.asarray(key[1], dtype=np.uint64), shape).copy()
    with np.errstate(over='ignore'):
        for r in range(10):
            if r > 0:
                k0 += _PHILOX_W[0]
                k1 += _PHILOX_W[1]
            hi0, lo0 = _mulhilo(np.full(shape, _PHILOX_M[0]), c0)
            hi1, lo1 = _mulhilo(np.full(shape, _PHILOX_M[1]), c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack([c0, c1, c2, c3], axis=-1)


def step_blocks(half, step, h, seed, stream=0):
    """The blocks of walkers-in-half 0 .. half-1 at global step ``step``, half ``h``: [half, 4] uint64."""
    ctr = np.zeros((half, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(half, dtype=np.uint64)
    ctr[:, 1] = np.uint64(step)
    ctr[:, 2] = np.uint64(h)
    return philox4x64_10(ctr, (int(seed), int(stream)))


def u01(x):
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0**-53


def partner(x0, half):
    return ((np.asarray(x0, dtype=np.uint64) >> _S32) * np.uint64(half)) >> _S32


def stretch_z(a, x1):
    t = (a - 1.0) * u01(x1)
    t = t + 1.0
    z = t * t
    return z / a


def propose(c, s, z):
    """Rows of the proposal: c the partners' positions [k, n], s the walkers' own [k, n], z [k]."""
    d = (c - s) * z[:, None]
    return c - d


def _log(v):
    # the C library's log, as the header compiled for the host calls it (np.log may take another implementation)
    return np.array([math.log(float(t)) if t > 0 else -math.inf for t in np.atleast_1d(v)])


def log_factor(n, z):
    return float(n - 1) * _log(z)


def log_lik(log_norm, chi2):
    return log_norm - 0.5 * np.asarray(chi2, dtype=np.float64)


def model_ok(status, chi2):
    return (np.asarray(status) == 0) & (np.asarray(chi2) < 1e99)


def accept(inside, ok, factor, lnl_new, lnl_old, x2):
    lhs = (factor + lnl_new) - lnl_old
    with np.errstate(invalid='ignore'):
        return np.asarray(inside, dtype=bool) & np.asarray(ok, dtype=bool) & (lhs > _log(u01(x2)))


# ---- the differential-evolution and snooker moves, and mixtures (vmx_ensemble.h, the second part)
MOVE_NAMES = ('stretch', 'de', 'snooker')
MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER = 0, 1, 2


def move_blocks(half, step, h, seed, stream=0):
    """Block B of walkers-in-half 0 .. half-1 at global step ``step``, half ``h`` (counter (k, step, h, 1)): [half, 4] uint64."""
    ctr = np.zeros((half, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(half, dtype=np.uint64)
    ctr[:, 1] = np.uint64(step)
    ctr[:, 2] = np.uint64(h)
    ctr[:, 3] = np.uint64(1)
    return philox4x64_10(ctr, (int(seed), int(stream)))


def move_thresholds(p):
    """(t0, t1) of the weights (p_stretch, p_de, p_snooker)."""
    p01 = float(p[0]) + float(p[1])
    total = p01 + float(p[2])
    return float(p[0]) / total, p01 / total


def move_choice(w0, t0, t1):
    u = u01(w0)
    return np.where(u < t0, MOVE_STRETCH, np.where(u < t1, MOVE_DE, MOVE_SNOOKER))


# ---- the covariance move (vmx_ensemble.h, the sixth part)
MOVE_COV = 3
COV_MOVE_NAMES = MOVE_NAMES + ('cov',)
_COV_KAPPA = float(np.sqrt(np.float64(3.0) / np.float64(4294967295.0)))


def move_thresholds4(p):
    """(t0, t1, t2) of the weights (p_stretch, p_de, p_snooker, p_cov)."""
    p01 = float(p[0]) + float(p[1])
    p012 = p01 + float(p[2])
    total = p012 + float(p[3])
    return float(p[0]) / total, p01 / total, p012 / total


def move_choice4(w0, t0, t1, t2):
    return np.where(u01(w0) >= t2, MOVE_COV, move_choice(w0, t0, t1))


def has_cov(moves):
    """The mixture ``moves`` (:func:`resolve_moves`) has the covariance move as its fourth member."""
    return moves is not None and len(moves['weights']) == 4


def choose_moves(w0, moves):
    """The move of every word ``w0`` (word 0 of block B) under the mixture ``moves``, of three weights or four."""
    if has_cov(moves):
        return move_choice4(w0, *move_thresholds4(moves['weights']))
    return move_choice(w0, *move_thresholds(moves['weights']))


def cov_z(words):
    """The variate of every 64-bit word: the centred sum of its four 16-bit fields times kappa = sqrt(3 / 4294967295) - symmetric,
    of unit variance, |z| <= 2 sqrt(3); not normal."""
    w = np.asarray(words, dtype=np.uint64)
    m = np.uint64(0xFFFF)
    total = (w & m) + ((w >> np.uint64(16)) & m) + ((w >> np.uint64(32)) & m) + (w >> np.uint64(48))
    d = total.astype(np.float64) - 131070.0
    return d * _COV_KAPPA


def cov_variates(walkers, n, step, h, seed, stream=0):
    """The variates z [len(walkers), n] of the walkers-in-half ``walkers`` at ``step``, half ``h``: column b from word b % 4 of
    the block with counter (k, step, h, 2 + b // 4)."""
    walkers = np.asarray(walkers, dtype=np.uint64)
    nb = (n + 3) // 4
    ctr = np.zeros((walkers.size, nb, 4), dtype=np.uint64)
    ctr[:, :, 0] = walkers[:, None]
    ctr[:, :, 1] = np.uint64(step)
    ctr[:, :, 2] = np.uint64(h)
    ctr[:, :, 3] = np.uint64(2) + np.arange(nb, dtype=np.uint64)[None, :]
    return cov_z(philox4x64_10(ctr, (int(seed), int(stream))).reshape(walkers.size, 4 * nb)[:, :n])


def half_factor(other):
    """The factor of the half ``other`` [H, n] (H >= 2): (mean [n], C [n, n] lower, good) - the mean and covariance in walker
    order, the Cholesky factor in the order of vmx_ns::cholesky, or with a pivot that is not positive (good False) the diagonal
    of standard deviations: :func:`vega_amd.nested.mean_cov` and :func:`vega_amd.nested.whiten`, whose order is the header's."""
    from .nested import mean_cov, whiten
    mean, cov = mean_cov(np.asarray(other, dtype=np.float64))
    C, good = whiten(cov)
    return mean, C, bool(good)


def cov_propose(s, C, gamma_c, z):
    """Rows of the covariance proposal: s the walkers' own positions [k, n], z their variates [k, n]: y_a = s_a + gamma_c (sum over
    b <= a of C_ab z_b), the sum in b order from 0.0."""
    y = np.empty_like(s)
    for a in range(s.shape[1]):
        acc = np.zeros(s.shape[0])
        for b in range(a + 1):
            acc = acc + C[a, b] * z[:, b]
        y[:, a] = s[:, a] + gamma_c * acc
    return y


def partner2(x1, half, j1):
    """The second partner, distinct from ``j1`` (half >= 2)."""
    j = partner(x1, half - 1).astype(np.int64)
    return j + (j >= j1)


def partner3(x3, half, j1, j2):
    """The third partner, distinct from ``j1`` and ``j2`` (half >= 3)."""
    j = partner(x3, half - 2).astype(np.int64)
    j = j + (j >= np.minimum(j1, j2))
    return j + (j >= np.maximum(j1, j2))


def de_gamma(gamma0, sigma, w1, w2):
    g = u01(w1) + u01(w2)
    g = g - 1.0
    t = sigma * g
    t = 1.0 + t
    return gamma0 * t


def de_propose(s, c1, c2, gamma):
    """Rows of the DE proposal: s the walkers' own positions [k, n], c1 and c2 the two partners' [k, n], gamma [k]."""
    d = c1 - c2
    t = gamma[:, None] * d
    return s + t


def _column_sum(terms):
    total = np.zeros(terms.shape[0])
    for d in range(terms.shape[1]):         # (in column order, as the header adds them)
        total = total + terms[:, d]
    return total


def snooker_propose(s, z, z1, z2, gamma_s):
    """Rows of the snooker proposal: s the walkers' own positions [k, n], z, z1, z2 the three partners' [k, n].  Returns
    (y [k, n], factor [k], ok [k]); not ok: no proposal (norm == 0 - then y is s and the factor 0 - or a factor not finite)."""
    n = s.shape[1]
    e = s - z
    norm = np.sqrt(_column_sum(e * e))
    some = norm > 0.0
    with np.errstate(all='ignore'):
        u = e / norm[:, None]
        p = _column_sum(u * z1) - _column_sum(u * z2)
        gp = gamma_s * p
        y = s + u * gp[:, None]
        r = y - z
        dl = _log(np.sqrt(_column_sum(r * r))) - _log(norm)
        factor = float(n - 1) * dl
    y = np.where(some[:, None], y, s)
    factor = np.where(some, factor, 0.0)
    return y, factor, some & np.isfinite(factor)


def resolve_moves(moves, n, walkers, gamma0=None, sigma=None, gamma_s=None, cov_scale=None):
    """The mixture a sampler of ``walkers`` walkers over ``n`` parameters runs with: None for ``moves`` None (the stretch move as
    ever), else dict(weights (stretch, DE, snooker), gamma0, sigma, gamma_s) - what vmx_ensemble_run_many_moves takes.
    ``moves``: ``'stretch'``, ``'de'`` or ``'snooker'``, a list of (name, weight), or such a dict.  Defaults: gamma0 =
    2.38 / sqrt(2 n), sigma = 1e-5, gamma_s = 1.7.  Refused as the library refuses them: an unknown name, a negative or
    non-finite weight, a zero sum, DE with fewer than 4 walkers, the snooker with fewer than 6, a scale that is not positive.
    ``'cov'`` - the covariance move (vmx_ensemble.h, the sixth part), alone or in the list; a dict may carry a fourth weight and
    ``cov_scale``: with a positive cov weight the result has four weights (stretch, DE, snooker, cov) and ``cov_scale`` (default
    2.38 / sqrt(n)) - what vmx_ensemble_run_many_cov takes; without one it is the dict of three weights.  Refused beside the above:
    ``cov_scale`` without a cov weight, cov with fewer than 4 walkers, a ``cov_scale`` that is not positive and finite."""
    if moves is None:
        if gamma0 is not None or sigma is not None or gamma_s is not None:
            raise ValueError('gamma0, sigma and gamma_s belong to moves: name the moves')
        if cov_scale is not None:
            raise ValueError("cov_scale belongs to the 'cov' move: name the moves")
        return None
    if isinstance(moves, dict):
        weights = [float(w) for w in moves['weights']]
        gamma0 = moves.get('gamma0') if gamma0 is None else gamma0
        sigma = moves.get('sigma') if sigma is None else sigma
        gamma_s = moves.get('gamma_s') if gamma_s is None else gamma_s
        cov_scale = moves.get('cov_scale') if cov_scale is None else cov_scale
        if len(weights) not in (3, 4):
            raise ValueError('moves: three weights (stretch, de, snooker), or four with cov')
        weights += [0.0] * (4 - len(weights))
    else:
        pairs = [(moves, 1.0)] if isinstance(moves, str) else list(moves)
        weights = [0.0, 0.0, 0.0, 0.0]
        for pair in pairs:
            name, w = (pair, 1.0) if isinstance(pair, str) else pair
            if name not in COV_MOVE_NAMES:
                raise ValueError(f"moves: unknown move {name!r}; one of 'stretch', 'de', 'snooker', 'cov'")
            weights[COV_MOVE_NAMES.index(name)] += float(w)
            if not float(w) >= 0.0:
                raise ValueError('moves: a weight must be finite and not negative')
    if not all(math.isfinite(w) and w >= 0.0 for w in weights):
        raise ValueError('moves: a weight must be finite and not negative')
    if not 0.0 < ((weights[0] + weights[1]) + weights[2]) + weights[3] < math.inf:
        raise ValueError('moves: the weights must have a positive sum')
    cov_weight = weights.pop()
    if not cov_weight > 0.0 and cov_scale is not None:
        raise ValueError("cov_scale belongs to the 'cov' move, which the moves do not name")
    if cov_weight > 0.0 and walkers < 4:
        raise ValueError("moves: 'cov' needs two walkers in the other half, at least 4 walkers")
    if weights[1] > 0.0 and walkers < 4:
        raise ValueError("moves: 'de' needs two partners in the other half, at least 4 walkers")
    if weights[2] > 0.0 and walkers < 6:
        raise ValueError("moves: 'snooker' needs three partners in the other half, at least 6 walkers")
    out = dict(weights=tuple(weights), gamma0=2.38 / math.sqrt(2.0 * n) if gamma0 is None else float(gamma0),
               sigma=1e-5 if sigma is None else float(sigma), gamma_s=1.7 if gamma_s is None else float(gamma_s))
    if not (math.isfinite(out['gamma0']) and out['gamma0'] > 0.0 and math.isfinite(out['gamma_s']) and out['gamma_s'] > 0.0):
        raise ValueError('moves: gamma0 and gamma_s must be positive and finite')
    if not (math.isfinite(out['sigma']) and out['sigma'] >= 0.0):
        raise ValueError('moves: sigma must be finite and not negative')
    if cov_weight > 0.0:
        out['weights'] = out['weights'] + (cov_weight,)
        out['cov_scale'] = 2.38 / math.sqrt(float(n)) if cov_scale is None else float(cov_scale)
        if not (math.isfinite(out['cov_scale']) and out['cov_scale'] > 0.0):
            raise ValueError('moves: cov_scale must be positive and finite')
    return out


def names_cov(moves):
    """``moves`` as a caller writes it names the covariance move with a positive weight."""
    if isinstance(moves, str):
        return moves == 'cov'
    if moves is None:
        return False
    if isinstance(moves, dict):
        return len(moves['weights']) == 4 and float(moves['weights'][3]) > 0.0
    return any(pair == 'cov' if isinstance(pair, str) else (pair[0] == 'cov' and float(pair[1]) > 0.0) for pair in moves)


def _names_slice(moves):
    if isinstance(moves, str):
        return moves == 'slice'
    if moves is None or isinstance(moves, dict):
        return False
    return any((pair if isinstance(pair, str) else pair[0]) == 'slice' for pair in moves)


def resolve_slice(moves, walkers, mu=None, tune_steps=None, gamma0=None, sigma=None, gamma_s=None):
    """``moves='slice'`` - ensemble slice sampling (vmx_ensemble.h, the fifth part) - as dict(mu0, tune_steps), defaults 1.0 and 100;
    None when ``moves`` does not name it.  Refused: ``'slice'`` inside a mixture, ``mu`` / ``tune_steps`` without it, the scales
    of the other moves with it, fewer than 4 walkers, a ``mu`` that is not positive and finite, negative ``tune_steps``."""
    if not _names_slice(moves):
        if mu is not None or tune_steps is not None:
            raise ValueError("mu and tune_steps belong to moves='slice'")
        return None
    if not isinstance(moves, str):
        pairs = [(pair, 1.0) if isinstance(pair, str) else tuple(pair) for pair in moves]
        if len(pairs) != 1 or not float(pairs[0][1]) > 0.0:
            raise ValueError("moves: 'slice' is a sampler of its own, not a member of a mixture: moves='slice'")
    if gamma0 is not None or sigma is not None or gamma_s is not None:
        raise ValueError("gamma0, sigma and gamma_s are scales of the stretch / DE / snooker moves, not of 'slice'")
    out = dict(mu0=1.0 if mu is None else float(mu), tune_steps=100 if tune_steps is None else int(tune_steps))
    if walkers < 4:
        raise ValueError("moves: 'slice' needs two partners in the other half, at least 4 walkers")
    if not (math.isfinite(out['mu0']) and out['mu0'] > 0.0):
        raise ValueError('mu: the scale of the slice directions must be positive and finite')
    if out['tune_steps'] < 0:
        raise ValueError('tune_steps: 0 or more steps')
    return out


def half_step_moves(H, h, step, seed, stream, moves):
    """The move of every walker of half ``h`` at ``step``: [H] of MOVE_STRETCH / MOVE_DE / MOVE_SNOOKER."""
    return choose_moves(move_blocks(H, step, h, seed, stream)[:, 0], moves)


def steps_moves(H, step0, n_steps, seed, stream, moves):
    """The move of every walker at the steps ``step0`` .. ``step0 + n_steps - 1``: [n_steps, 2 H] (walker h H + k: half h), the
    :func:`half_step_moves` of every half-step.  The walkers of a half-step are consecutive counters, so NumPy's own Philox
    draws their blocks B in one call (the generator :func:`philox4x64_10` restates; it increments before it encrypts)."""
    key = np.array([int(seed), int(stream)], dtype=np.uint64)
    words = np.empty((n_steps, 2, H), dtype=np.uint64)
    for i in range(n_steps):
        for h in (0, 1):
            counter = ((step0 + i) << 64) | (h << 128) | (1 << 192)
            words[i, h] = np.random.Philox(key=key, counter=counter - 1).random_raw(4 * H)[0::4]
    return choose_moves(words, moves).reshape(n_steps, 2 * H)


def half_step_blocks(H, step, h, seed, streams, last=0):
    """The blocks of the walkers-in-half 0 .. H-1 of every stream of ``streams`` [E] at ``step``, half ``h``, in one pass:
    [E, H, 4] uint64, entry e :func:`step_blocks` (``last`` 0) or :func:`move_blocks` (``last`` 1) of ``streams[e]``."""
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((streams.size, H, 4), dtype=np.uint64)
    ctr[:, :, 0] = np.arange(H, dtype=np.uint64)
    ctr[:, :, 1] = np.uint64(step)
    ctr[:, :, 2] = np.uint64(h)
    ctr[:, :, 3] = np.uint64(last)
    return philox4x64_10(ctr, (int(seed), streams[:, None]))


def half_step_proposals(x, h, step, a, seed, stream, lo, hi, moves=None, blocks=None, factor_of_half=None):
    """Proposals of half ``h`` at ``step`` for the walkers ``x`` [W, n]: (y [W/2, n], inside [W/2], factor [W/2], blocks).
    ``moves`` (:func:`resolve_moves`; None: the stretch move): every walker's move is drawn from the mixture.  ``blocks``
    (None: drawn here): the half's (:func:`step_blocks`, :func:`move_blocks` or None) when the caller has them already.
    ``factor_of_half`` (None: computed here when the mixture has the covariance move): :func:`half_factor` of the other half."""
    W, n = x.shape
    H = W // 2
    b = step_blocks(H, step, h, seed, stream) if blocks is None else blocks[0]
    j = partner(b[:, 0], H).astype(np.int64)
    other = x[(1 - h) * H:(2 - h) * H]
    c = other[j]
    s = x[h * H:(h + 1) * H]
    if moves is None:
        z = stretch_z(a, b[:, 1])
        y = propose(c, s, z)
        factor = log_factor(n, z)
        some = True
    else:
        m = move_blocks(H, step, h, seed, stream) if blocks is None else blocks[1]
        move = choose_moves(m[:, 0], moves)
        y, factor, some = np.empty((H, n)), np.zeros(H), np.ones(H, dtype=bool)
        k = np.flatnonzero(move == MOVE_COV)
        if k.size:
            _, C, _ = half_factor(other) if factor_of_half is None else factor_of_half
            y[k] = cov_propose(s[k], C, moves['cov_scale'], cov_variates(k, n, step, h, seed, stream))
        k = np.flatnonzero(move == MOVE_STRETCH)
        if k.size:
            z = stretch_z(a, b[k, 1])
            y[k], factor[k] = propose(c[k], s[k], z), log_factor(n, z)
        k = np.flatnonzero(move == MOVE_DE)
        if k.size:
            j2 = partner2(b[k, 1], H, j[k])
            y[k] = de_propose(s[k], c[k], other[j2], de_gamma(moves['gamma0'], moves['sigma'], m[k, 1], m[k, 2]))
        k = np.flatnonzero(move == MOVE_SNOOKER)
        if k.size:
            j2 = partner2(b[k, 1], H, j[k])
            j3 = partner3(b[k, 3], H, j[k], j2)
            y[k], factor[k], some[k] = snooker_propose(s[k], c[k], other[j2], other[j3], moves['gamma_s'])
    with np.errstate(invalid='ignore'):
        inside = some & np.all((y >= lo) & (y <= hi), axis=1)
    return y, inside, factor, b


# ---- parallel tempering: ladders and swaps (vmx_ensemble.h, the third part)
PT_MAXT = 64


def ladder_ok(betas):
    """A ladder the sampler takes: betas[0] == 1, finite, strictly decreasing, none negative, at most PT_MAXT rungs."""
    b = np.asarray(betas, dtype=np.float64)
    if b.ndim != 1 or not 1 <= b.size <= PT_MAXT or b[0] != 1.0:
        return False
    return bool(np.all(np.isfinite(b)) and np.all(b >= 0.0) and np.all(np.diff(b) < 0.0))


def default_ladder(ntemps, beta_min=None):
    """The ladder of ``ntemps`` = T >= 2 rungs: geometric from 1 to ``beta_min`` (default 2**-(T - 2)) over the first T - 1 rungs,
    then 0 - the rung that samples the box, which the stepping-stone evidence needs.  T = 2: (1, 0)."""
    T = int(ntemps)
    if not 2 <= T <= PT_MAXT:
        raise ValueError(f'ntemps: 2 .. {PT_MAXT} rungs')
    if T == 2:
        return np.array([1.0, 0.0])
    if beta_min is None:        # (the powers of two themselves, not their roots)
        return np.append(2.0 ** -np.arange(T - 1, dtype=np.float64), 0.0)
    beta_min = float(beta_min)
    if not 0.0 < beta_min < 1.0:
        raise ValueError('beta_min: between 0 and 1')
    betas = np.append(beta_min ** (np.arange(T - 1) / (T - 2.0)), 0.0)
    betas[0], betas[T - 2] = 1.0, beta_min
    if not ladder_ok(betas):
        raise ValueError('beta_min: the ladder must decrease strictly')
    return betas


def tempered(beta, lnl):
    """A rung's view of a log-likelihood: what its Metropolis decision compares."""
    return beta * np.asarray(lnl, dtype=np.float64)


def accept_tempered(inside, ok, factor, beta, lnl_new, lnl_old, x2):
    return accept(inside, ok, factor, tempered(beta, lnl_new), tempered(beta, lnl_old), x2)


def shift_block(step, t, seed, stream=0):
    """The block of the rotation of the pair (rung t - 1, rung t) at global step ``step`` (counter (0, step, t, 3)): [4] uint64."""
    ctr = np.array([0, step, t, 3], dtype=np.uint64)
    return philox4x64_10(ctr, (int(seed), int(stream)))


def swap_blocks(W, step, t, seed, stream=0):
    """The blocks of the pairs 0 .. W-1 of (rung t - 1, rung t) at global step ``step`` (counter (k, step, t, 2)): [W, 4] uint64."""
    ctr = np.zeros((W, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(W, dtype=np.uint64)
    ctr[:, 1] = np.uint64(step)
    ctr[:, 2] = np.uint64(t)
    ctr[:, 3] = np.uint64(2)
    return philox4x64_10(ctr, (int(seed), int(stream)))


def swap_shift(w0, W):
    """The rotation r in [0, W): walker k of the colder rung meets walker (k + r) mod W of the hotter one."""
    return partner(w0, W)


def swap_partner(k, r, W):
    j = np.asarray(k, dtype=np.int64) + int(r)
    return np.where(j >= W, j - W, j)


def swap_accept(beta_cold, beta_hot, lnl_cold, lnl_hot, word):
    db = beta_cold - beta_hot
    dl = np.asarray(lnl_hot, dtype=np.float64) - np.asarray(lnl_cold, dtype=np.float64)
    lhs = db * dl
    return lhs > _log(u01(word))


def swap_due(step, swap_every):
    return swap_every > 0 and (step + 1) % swap_every == 0


def swap_sweep(x, lnl, betas, step, seed, stream, swaps):
    """The swap sweep of one ladder after global step ``step``: ``x`` [T, W, n] and ``lnl`` [T, W] (updated in place), pairs of
    rungs from the hottest down, under the key (seed, ``stream``: the stream of rung 0); ``swaps`` [T - 1, 2] += (proposed,
    accepted)."""
    T, W = lnl.shape
    k = np.arange(W)
    # the blocks of all pairs of rungs in one pass: counters (k, step, t, 2) and (0, step, t, 3), t = 1 .. T - 1
    ctr = np.zeros((T - 1, W + 1, 4), dtype=np.uint64)
    ctr[:, :W, 0] = np.arange(W, dtype=np.uint64)
    ctr[:, :, 1] = np.uint64(step)
    ctr[:, :, 2] = np.arange(1, T, dtype=np.uint64)[:, None]
    ctr[:, :W, 3], ctr[:, W, 3] = np.uint64(2), np.uint64(3)
    words = philox4x64_10(ctr, (int(seed), int(stream)))[:, :, 0]
    for t in range(T - 1, 0, -1):
        r = int(swap_shift(words[t - 1, W], W))
        j = swap_partner(k, r, W)
        word = words[t - 1, :W]
        take = swap_accept(betas[t - 1], betas[t], lnl[t - 1], lnl[t, j], word)
        kk, jj = k[take], j[take]
        x[t - 1, kk], x[t, jj] = x[t, jj].copy(), x[t - 1, kk].copy()
        lnl[t - 1, kk], lnl[t, jj] = lnl[t, jj].copy(), lnl[t - 1, kk].copy()
        swaps[t - 1] += (W, int(take.sum()))


# ---- adaptive ladders (vmx_ensemble.h, the fourth part)
def adapt_ok(T, swap_every, lag, tau):
    """What the adaptive run takes beside a ladder: 3 <= T <= PT_MAXT rungs, sweeps, ``lag`` and ``tau`` finite and positive."""
    lag, tau = float(lag), float(tau)
    return bool(3 <= T <= PT_MAXT and swap_every > 0 and math.isfinite(lag) and lag > 0.0 and math.isfinite(tau) and tau > 0.0)


def sweep_time(step, swap_every):
    """The number of sweeps before the one after global step ``step``."""
    return (step + 1) // swap_every - 1


def adapt_due(step, adapt_until):
    return adapt_until < 0 or step < adapt_until


def ladder_adjust(betas, accepted, W, time, lag, tau):
    """vmx_ens::ladder_adjust, ptemcee's ``_get_ladder_adjustment`` with every operation rounded on its own: one ladder ``betas``
    [T] after one sweep whose pairs (t, t + 1) accepted ``accepted`` [T - 1] of ``W`` swaps, ``time`` sweeps before it.  Returns
    (the new ladder, 0) or, when the new ladder is not :func:`ladder_ok` (a positive last beta can be crossed), (the old one, 1).
    The first and the last beta never move."""
    from .smc import pexp
    old = np.array(betas, dtype=np.float64)
    T = old.size
    if T < 3:
        return old, 0
    with np.errstate(all='ignore'):
        ratio = np.asarray(accepted, dtype=np.int64).astype(np.float64) / np.float64(W)
        tl = np.float64(time) + np.float64(lag)
        decay = np.float64(lag) / tl
        kappa = decay / np.float64(tau)
        da = ratio[:-1] - ratio[1:]
        dS = kappa * da
        inv = 1.0 / old[:-1]
        dT = inv[1:] - inv[:-1]
        gap = dT * pexp(dS)
        new = old.copy()
        total = np.float64(1.0) / old[0]
        for i in range(T - 2):          # (in order: a cumulative sum that starts from 1 / beta[0])
            total = total + gap[i]
            new[i + 1] = np.float64(1.0) / total
    if not ladder_ok(new):
        return old, 1
    return new, 0


def _steps_pt(x, lnl, accepted, step0, n_steps, thin, swap_every, a, seed, betas, streams, lo, hi, log_norm, evaluate, moves, adapt):
    """The steps of :func:`python_steps_pt` over ladders of their own, ``betas`` [G, T] (updated in place when ``adapt`` - (lag,
    tau, adapt_until) - is given: :func:`ladder_adjust` after every sweep that is due to adapt).  Returns python_steps_pt's tuple
    and (the ladders after every sweep of the call [sweeps, G, T], the guard's counts [G])."""
    G, T, W, n = x.shape
    E = G * T
    xe, le, ae = x.reshape(E, W, n), lnl.reshape(E, W), accepted.reshape(E, W)
    flat_streams = np.asarray(streams, dtype=np.uint64).reshape(E)
    rows = (step0 + n_steps) // thin - step0 // thin
    chain, chain_lnl = np.empty((E, rows, W, n)), np.empty((E, rows, W))
    per = np.zeros((E, 3), dtype=np.int64)
    swaps = np.zeros((G, T - 1, 2), dtype=np.int64)
    hist, skipped = [], np.zeros(G, dtype=np.int64)
    s, end = step0, step0 + n_steps
    while s < end:
        # up to and with the next step a sweep follows (or the end); every step's row, of which the thinning picks
        stop = end if swap_every <= 0 or T < 2 else min(end, (s // swap_every + 1) * swap_every)
        part, part_lnl, _, p = python_steps_many(xe, le, ae, s, stop - s, 1, a, seed, flat_streams, lo, hi, log_norm, evaluate, moves,
                                                 betas=betas.reshape(E))
        per += p
        if T > 1 and swap_due(stop - 1, swap_every):
            for g in range(G):
                before = swaps[g, :, 1].copy()
                swap_sweep(x[g], lnl[g], betas[g], stop - 1, seed, int(flat_streams[g * T]), swaps[g])
                if adapt is not None and adapt_due(stop - 1, adapt[2]):
                    betas[g], skip = ladder_adjust(betas[g], swaps[g, :, 1] - before, W, sweep_time(stop - 1, swap_every), adapt[0],
                                                   adapt[1])
                    skipped[g] += skip
            hist.append(betas.copy())
            part[:, -1], part_lnl[:, -1] = xe, le
        for q in range(s, stop):
            if (q + 1) % thin == 0:
                r = (q + 1) // thin - step0 // thin - 1
                chain[:, r], chain_lnl[:, r] = part[:, q - s], part_lnl[:, q - s]
        s = stop
    st = dict(steps=n_steps, proposals=n_steps * W * E, accepted=int(per[:, 0].sum()), rejected_outside_box=int(per[:, 1].sum()),
              rejected_failed_model=int(per[:, 2].sum()), swaps_proposed=int(swaps[:, :, 0].sum()),
              swaps_accepted=int(swaps[:, :, 1].sum()))
    hist = np.array(hist).reshape(len(hist), G, T)
    return (chain.reshape(G, T, rows, W, n), chain_lnl.reshape(G, T, rows, W), st, per.reshape(G, T, 3), swaps), (hist, skipped)


def python_steps_pt(x, lnl, accepted, step0, n_steps, thin, swap_every, a, seed, betas, streams, lo, hi, log_norm, evaluate,
                    moves=None):
    """``n_steps`` steps of G temperature ladders of T rungs in NumPy - what vmx_ensemble_run_pt runs: the state ``x``
    [G, T, W, n], ``lnl`` [G, T, W] (untempered), ``accepted`` [G, T, W] (updated in place), ``betas`` [T], ``streams`` [G, T].
    The steps are :func:`python_steps_many`'s over the G T ensembles with the rung's beta in the decision, run up to every step
    after which a sweep is due (:func:`swap_due`: the global step counts); the sweep (:func:`swap_sweep`) comes before that step's
    chain row.  ``evaluate(rows, h)`` as there, for the G T W/2 rows of a half.  Returns (chain [G, T, rows, W, n], chain_lnl
    [G, T, rows, W], stats, per_ensemble [G, T, 3], swaps [G, T - 1, 2])."""
    ladders = np.tile(np.asarray(betas, dtype=np.float64), (x.shape[0], 1))
    return _steps_pt(x, lnl, accepted, step0, n_steps, thin, swap_every, a, seed, ladders, streams, lo, hi, log_norm, evaluate, moves,
                     None)[0]


def python_steps_pt_adapt(x, lnl, accepted, step0, n_steps, thin, swap_every, a, seed, betas, streams, lo, hi, log_norm, evaluate,
                          moves=None, adaptation_lag=10000.0, adaptation_time=100.0, adapt_until=-1):
    """:func:`python_steps_pt` over ladders of their own that adapt - what vmx_ensemble_run_pt_adapt runs: ``betas`` float64 [G, T]
    (updated in place); after every sweep that follows a global step s with ``adapt_until`` < 0 or s < ``adapt_until``, every
    ladder moves by :func:`ladder_adjust` with its own accepted swaps of that sweep and ``time`` = :func:`sweep_time` (the global
    step alone: a run cut into calls adapts identically); the row of step s and the next proposals see the new ladder.  Returns
    python_steps_pt's five, then ``betas``, the ladders after every sweep of the call [sweeps, G, T] and the sweeps whose new ladder
    the guard dropped, int64 [G]."""
    G, T = x.shape[:2]
    if not (isinstance(betas, np.ndarray) and betas.dtype == np.float64 and betas.shape == (G, T)):
        raise ValueError('betas: a float64 array [G, T] (updated in place)')
    if not adapt_ok(T, swap_every, adaptation_lag, adaptation_time):
        raise ValueError('adaptive ladders: T >= 3 rungs, swap_every >= 1, adaptation_lag and adaptation_time finite and positive')
    if not all(ladder_ok(b) for b in betas):
        raise ValueError(f'betas: every ladder from 1, strictly decreasing, none negative, at most {PT_MAXT}')
    out, (hist, skipped) = _steps_pt(x, lnl, accepted, step0, n_steps, thin, swap_every, a, seed, betas, streams, lo, hi, log_norm,
                                     evaluate, moves, (float(adaptation_lag), float(adaptation_time), int(adapt_until)))
    return out + (betas, hist, skipped)


def python_steps_many(x, lnl, accepted, step0, n_steps, thin, a, seed, streams, lo, hi, log_norm, evaluate, moves=None, betas=None):
    """``n_steps`` steps of E independent ensembles advanced together, in NumPy: the state ``x`` [E, W, n], ``lnl`` [E, W],
    ``accepted`` [E, W] (updated in place), ensemble e on the Philox stream ``streams[e]``.  Every half-step is decided ensemble by
    ensemble; only the likelihood is joined: ``evaluate(rows, h)`` -> (chi2 [E W/2], status [E W/2]) for the E W/2 rows
    [E W/2, n] of the half, ensemble e's at [e W/2, (e + 1) W/2) - the rows the device driver hands the engine (a proposal outside
    the box is replaced by the walker's own position).  Returns (chain [E, rows, W, n], chain_lnl [E, rows, W], stats,
    per_ensemble [E, 3]: accepted, rejected outside the box, rejected for a failed model).  ``moves`` (:func:`resolve_moves`; None:
    the stretch move): the mixture every walker's move is drawn from.  ``betas`` [E] (None: 1, the run of ever): ensemble e decides
    at the inverse temperature ``betas[e]`` (:func:`accept_tempered`; the stored lnl stays untempered).  With the covariance
    move in the mixture the factor of every half-step is computed once per ensemble, and ``stats['cov_fallbacks']`` int64 [E]
    counts the half-steps whose factor fell back to the diagonal."""
    E, W, n = x.shape
    H = W // 2
    rows = (step0 + n_steps) // thin - step0 // thin
    chain, chain_lnl = np.empty((E, rows, W, n)), np.empty((E, rows, W))
    per = np.zeros((E, 3), dtype=np.int64)
    cov = has_cov(moves)
    fallbacks = np.zeros(E, dtype=np.int64)
    for s in range(step0, step0 + n_steps):
        for h in (0, 1):
            mine = slice(h * H, (h + 1) * H)
            b_all = half_step_blocks(H, s, h, seed, streams)          # (the Philox blocks of all ensembles in one pass)
            m_all = None if moves is None else half_step_blocks(H, s, h, seed, streams, last=1)
            factors = [half_factor(x[e, (1 - h) * H:(2 - h) * H]) if cov else None for e in range(E)]
            if cov:
                fallbacks += [0 if f[2] else 1 for f in factors]
            props = [half_step_proposals(x[e], h, s, a, seed, streams[e], lo, hi, moves,
                                         blocks=(b_all[e], None if m_all is None else m_all[e]), factor_of_half=factors[e])
                     for e in range(E)]
            chi2, status = evaluate(np.concatenate([np.where(inside[:, None], y, x[e, mine])
                                                    for e, (y, inside, _, _) in enumerate(props)]), h)
            for e, (y, inside, factor, b) in enumerate(props):
                c2, st_e = chi2[e * H:(e + 1) * H], status[e * H:(e + 1) * H]
                ok = model_ok(st_e, c2)
                lnl_new = log_lik(log_norm, c2)
                if betas is None:
                    acc = accept(inside, ok, factor, lnl_new, lnl[e, mine], b[:, 2])
                else:
                    acc = accept_tempered(inside, ok, factor, float(betas[e]), lnl_new, lnl[e, mine], b[:, 2])
                x[e, mine][acc] = y[acc]
                lnl[e, mine][acc] = lnl_new[acc]
                accepted[e, mine] += acc
                per[e] += (int(acc.sum()), int((~inside).sum()), int((inside & ~ok).sum()))
        if (s + 1) % thin == 0:
            r = (s + 1) // thin - step0 // thin - 1
            chain[:, r], chain_lnl[:, r] = x, lnl
    st = dict(steps=n_steps, proposals=n_steps * W * E, accepted=int(per[:, 0].sum()), rejected_outside_box=int(per[:, 1].sum()),
              rejected_failed_model=int(per[:, 2].sum()))
    if cov:
        st['cov_fallbacks'] = fallbacks
    return chain, chain_lnl, st, per


# ---- ensemble slice sampling (vmx_ensemble.h, the fifth part): scalar functions over Python floats and integers, one per function
# of the header - a Python float is an IEEE double and every operation below is rounded on its own
SLICE_MAX_EXPANSIONS, SLICE_MAX_CONTRACTIONS = 32, 64
SLICE_LEFT, SLICE_RIGHT, SLICE_SHRINK, SLICE_DONE = 0, 1, 2, 3
END_NONE, END_MOVED, END_CAPPED, END_NULL = 0, 1, 2, 3
SLICE_COUNT_NAMES = ('updates', 'moved', 'rows', 'expansions', 'contractions', 'box', 'failed', 'capped')
SC_UPDATES, SC_MOVED, SC_ROWS, SC_EXPANSIONS, SC_CONTRACTIONS, SC_BOX, SC_FAILED, SC_CAPPED_NULL = range(8)
_M64 = (1 << 64) - 1
_INF = math.inf


def philox_block(c0, c1, c2, c3, k0, k1):
    """:func:`philox4x64_10` of one counter in Python integers: the four words."""
    m0, m1, w0, w1 = (int(v) for v in _PHILOX_M + _PHILOX_W)
    for r in range(10):
        if r > 0:
            k0, k1 = (k0 + w0) & _M64, (k1 + w1) & _M64
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & _M64, (p0 >> 64) ^ c3 ^ k1, p0 & _M64
    return c0, c1, c2, c3


def slice_block(k, s, h, j, seed, stream):
    return philox_block(int(k), int(s), 2 * int(j) + int(h), 6, int(seed) & _M64, int(stream) & _M64)


def _u01(word):
    return float(word >> 11) * 2.0**-53


def _log1(v):
    return math.log(v) if v > 0.0 else -_INF


class SliceWalker:
    """A walker's update (the header's struct of the same name)."""
    FIELDS = ('L', 'R', 't', 'lnY', 'lnl', 'phase', 'draw', 'left', 'right', 'contractions', 'rows', 'box', 'failed', 'end', 'asks')
    __slots__ = FIELDS

    def fields(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


def slice_word(w, k, s, h, seed, stream):
    i = w.draw
    w.draw = i + 1
    return slice_block(k, s, h, i // 4, seed, stream)[i % 4]


def slice_eta(mu, c1, c2):
    d = c1 - c2
    return mu * d


def slice_point(x, t, eta):
    p = t * eta
    return x + p


def slice_height(lnl, w2):
    return lnl + _log1(_u01(w2))


def slice_shrink(L, R, word):
    d = R - L
    m = d * _u01(word)
    return L + m


def slice_inside(x, t, eta, lo, hi):
    for xq, eq, l, h in zip(x, eta, lo, hi):
        y = slice_point(xq, t, eq)
        if not (l <= y <= h):
            return False
    return True


def slice_answer(w, log_norm, status, chi2):
    if status == 0 and chi2 < 1e99:
        return log_norm - 0.5 * chi2
    w.failed += 1
    return -_INF


def slice_take(w, answer, max_e, max_c, k, s, h, seed, stream):
    inside = answer > w.lnY
    if w.phase == SLICE_LEFT:
        if inside:
            w.L = w.L - 1.0
            w.left += 1
        if inside and w.left < max_e:
            w.t = w.L
            return
        w.phase, w.t = SLICE_RIGHT, w.R
        return
    if w.phase == SLICE_RIGHT:
        if inside:
            w.R = w.R + 1.0
            w.right += 1
        if inside and w.right < max_e:
            w.t = w.R
            return
        w.phase = SLICE_SHRINK
        w.t = slice_shrink(w.L, w.R, slice_word(w, k, s, h, seed, stream))
        return
    if w.phase != SLICE_SHRINK:
        return
    if inside:
        w.lnl, w.end, w.phase = answer, END_MOVED, SLICE_DONE
        return
    if w.t < 0.0:
        w.L = w.t
    else:
        w.R = w.t
    w.contractions += 1
    if w.contractions >= max_c:
        w.end, w.phase = END_CAPPED, SLICE_DONE
        return
    w.t = slice_shrink(w.L, w.R, slice_word(w, k, s, h, seed, stream))


def slice_settle(w, x, eta, lo, hi, max_e, max_c, k, s, h, seed, stream):
    w.asks = 0
    while w.phase != SLICE_DONE:
        if slice_inside(x, w.t, eta, lo, hi):
            w.asks = 1
            w.rows += 1
            return
        w.box += 1
        slice_take(w, -_INF, max_e, max_c, k, s, h, seed, stream)


def slice_open(x, lnl, other, mu, lo, hi, max_e, max_c, k, s, h, seed, stream):
    """The update of walker-in-half ``k`` at ``x`` (a list) opens against the other half ``other`` (a list of lists): (the walker,
    its direction)."""
    H = len(other)
    b = slice_block(k, s, h, 0, seed, stream)
    j1 = ((b[0] >> 32) * H) >> 32
    j2 = ((b[1] >> 32) * (H - 1)) >> 32
    j2 += j2 >= j1
    eta = [slice_eta(mu, c1, c2) for c1, c2 in zip(other[j1], other[j2])]
    null = all(v == 0.0 for v in eta)
    w = SliceWalker()
    w.lnY = slice_height(lnl, b[2])
    w.L = -_u01(b[3])
    w.R = w.L + 1.0
    w.t, w.lnl = w.L, lnl
    w.phase, w.end = (SLICE_DONE, END_NULL) if null else (SLICE_LEFT, END_NONE)
    w.draw = 4
    w.left = w.right = w.contractions = w.rows = w.box = w.failed = 0
    slice_settle(w, x, eta, lo, hi, max_e, max_c, k, s, h, seed, stream)
    return w, eta


def slice_advance(w, x, eta, lo, hi, log_norm, status, chi2, max_e, max_c, k, s, h, seed, stream):
    answer = slice_answer(w, log_norm, status, chi2)
    slice_take(w, answer, max_e, max_c, k, s, h, seed, stream)
    slice_settle(w, x, eta, lo, hi, max_e, max_c, k, s, h, seed, stream)


def slice_commit(w, x, eta, lnl, counts):
    """(the walker's position, its lnL, whether it moved) after the half; the update's counts are added to ``counts`` [8]."""
    moved = w.end == END_MOVED
    if moved:
        x, lnl = [slice_point(xq, w.t, eq) for xq, eq in zip(x, eta)], w.lnl
    counts += (1, int(moved), w.rows, w.left + w.right, w.contractions, w.box, w.failed, int(w.end in (END_CAPPED, END_NULL)))
    return x, lnl, moved


def slice_tune_due(s, tune_steps):
    return s < tune_steps


def slice_tune(mu, expansions, contractions):
    ne = max(1, int(expansions))
    num = 2.0 * float(ne)
    den = float(ne + int(contractions))
    f = num / den
    m = mu * f
    return m if 2.0**-1022 <= m <= 1.7976931348623157e308 else mu


def slice_ok(H, mu0, tune_steps, max_e, max_c, flags=0):
    return (H >= 2 and math.isfinite(mu0) and mu0 > 0.0 and tune_steps >= 0 and 1 <= max_e <= SLICE_MAX_EXPANSIONS
            and 1 <= max_c <= SLICE_MAX_CONTRACTIONS and flags == 0)


def slice_offsets(count):
    """(offsets, total) of the counts of the running ensembles, in list order."""
    offsets, total = [], 0
    for c in count:
        offsets.append(total)
        total += c
    return offsets, total


def slice_compact(active, count_of):
    return [e for e in active if count_of[e] > 0]


class SliceRounds:
    """The set round of ensemble slice sampling, round by round, as the device driver runs it: the state ``x`` [E, W, n], ``lnl``
    [E, W], ``accepted`` [E, W], ``mu`` [E] (all updated in place).  :meth:`round` takes the answers (chi2, status) of the rows the
    round before asked for and returns the next rows (rows [R, n], the ensemble of every row [R]) - in ascending (ensemble,
    walker) order - until the running list ``active`` is empty.  ``wk`` / ``eta`` / ``slot`` hold the machines, directions and
    engine rows of every ensemble's active half, ``q`` the half-steps done, ``counts`` [E, 8] the counts, ``count_of`` [E] the
    requests of the last round."""

    def __init__(self, x, lnl, accepted, mu, step0, n_steps, thin, seed, streams, lo, hi, log_norm, tune_steps=100,
                 max_expansions=SLICE_MAX_EXPANSIONS, max_contractions=SLICE_MAX_CONTRACTIONS):
        self.x, self.lnl, self.accepted, self.mu = x, lnl, accepted, mu
        self.E, self.W, self.n = x.shape
        self.H = self.W // 2
        if not all(slice_ok(self.H, float(m), tune_steps, max_expansions, max_contractions) for m in mu):
            raise ValueError('slice: W >= 4, mu positive and finite, tune_steps >= 0, 1 <= max_expansions <= 32, '
                             '1 <= max_contractions <= 64')
        self.step0, self.n_steps, self.thin, self.seed = int(step0), int(n_steps), int(thin), int(seed)
        self.streams = [int(v) for v in streams]
        self.lo, self.hi, self.log_norm = [float(v) for v in lo], [float(v) for v in hi], float(log_norm)
        self.tune_steps, self.max_e, self.max_c = int(tune_steps), int(max_expansions), int(max_contractions)
        E, H = self.E, self.H
        rows = (self.step0 + self.n_steps) // self.thin - self.step0 // self.thin
        self.chain, self.chain_lnl = np.empty((E, rows, self.W, self.n)), np.empty((E, rows, self.W))
        self.q, self.open = [0] * E, [False] * E
        self.wk, self.eta = [[None] * H for _ in range(E)], [[None] * H for _ in range(E)]
        self.slot, self.row_walker = [[-1] * H for _ in range(E)], [[] for _ in range(E)]
        self.counts, self.step_counts = np.zeros((E, 8), dtype=np.int64), np.zeros((E, 2), dtype=np.int64)
        self.count_of = [0] * E
        self.active = list(range(E)) if self.n_steps > 0 else []
        self.rounds = self.rows = 0

    def _half(self, e):
        return self.step0 + self.q[e] // 2, self.q[e] % 2

    def _pass(self, e, opening, chi2, status):
        s, h = self._half(e)
        H, stream = self.H, self.streams[e]
        mine = self.x[e, h * H:(h + 1) * H].tolist()
        tail = (self.max_e, self.max_c)
        if opening:
            other = self.x[e, (1 - h) * H:(2 - h) * H].tolist()
            mu = float(self.mu[e])
        self.row_walker[e] = order = []
        for k in range(H):
            if opening:
                self.wk[e][k], self.eta[e][k] = slice_open(mine[k], float(self.lnl[e, h * H + k]), other, mu, self.lo, self.hi, *tail,
                                                           k, s, h, self.seed, stream)
            elif self.wk[e][k].asks:
                row = self.slot[e][k]
                slice_advance(self.wk[e][k], mine[k], self.eta[e][k], self.lo, self.hi, self.log_norm, int(status[row]),
                              float(chi2[row]), *tail, k, s, h, self.seed, stream)
            if self.wk[e][k].asks:
                self.slot[e][k] = len(order)
                order.append(k)
        return len(order)

    def _commit(self, e):
        s, h = self._half(e)
        H = self.H
        took = np.zeros(8, dtype=np.int64)
        for k in range(H):
            w = h * H + k
            xk, lk, moved = slice_commit(self.wk[e][k], self.x[e, w].tolist(), self.eta[e][k], float(self.lnl[e, w]), took)
            if moved:
                self.x[e, w], self.lnl[e, w] = xk, lk
                self.accepted[e, w] += 1
        self.counts[e] += took
        self.step_counts[e] += (took[SC_EXPANSIONS], took[SC_CONTRACTIONS])
        if h == 1:
            if slice_tune_due(s, self.tune_steps):
                self.mu[e] = slice_tune(float(self.mu[e]), *self.step_counts[e])
            self.step_counts[e] = 0
            if (s + 1) % self.thin == 0:
                r = (s + 1) // self.thin - self.step0 // self.thin - 1
                self.chain[e, r], self.chain_lnl[e, r] = self.x[e], self.lnl[e]

    def round(self, chi2=None, status=None):
        counts = []
        for e in self.active:
            total = self._pass(e, False, chi2, status) if self.open[e] else 0
            while total == 0:
                if self.open[e]:
                    self._commit(e)
                    self.q[e] += 1
                    self.open[e] = False
                if self.q[e] >= 2 * self.n_steps:
                    break
                total = self._pass(e, True, None, None)
                self.open[e] = True
            counts.append(total)
        offsets, total = slice_offsets(counts)
        self.listing = list(zip(self.active, counts, offsets))         # (the round's list: ensemble, requests, offset)
        rows, ens = np.empty((total, self.n)), np.empty(total, dtype=np.int64)
        for a, e in enumerate(self.active):
            h = self.q[e] % 2
            for r, k in enumerate(self.row_walker[e][:counts[a]]):
                self.slot[e][k] = offsets[a] + r
                t = self.wk[e][k].t
                rows[offsets[a] + r] = [slice_point(xq, t, eq) for xq, eq in zip(self.x[e, h * self.H + k].tolist(), self.eta[e][k])]
                ens[offsets[a] + r] = e
            self.count_of[e] = counts[a]
        self.active = slice_compact(self.active, self.count_of)
        self.rounds += 1
        self.rows += total
        return rows, ens


def slice_stats(counts, mu):
    """``stats['slice']`` of the counts [E, 8] and scales [E] of a run: every count summed, ``per_ensemble`` [E, 8] in the order of
    ``SLICE_COUNT_NAMES``, ``rows_per_update`` and ``mu``."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    total = counts.sum(axis=0)
    out = {name: int(v) for name, v in zip(SLICE_COUNT_NAMES, total)}
    out.update(per_ensemble=counts.copy(), rows_per_update=float(total[SC_ROWS]) / max(int(total[SC_UPDATES]), 1),
               mu=np.array(mu, dtype=np.float64).copy())
    return out


def python_steps_slice_many(x, lnl, accepted, mu, step0, n_steps, thin, seed, streams, lo, hi, log_norm, evaluate, tune_steps=100,
                            max_expansions=SLICE_MAX_EXPANSIONS, max_contractions=SLICE_MAX_CONTRACTIONS):
    """``n_steps`` steps of ensemble slice sampling for E independent ensembles advanced together, in NumPy: the state ``x``
    [E, W, n], ``lnl`` [E, W], ``accepted`` [E, W] and the scales ``mu`` [E] (all updated in place), ensemble e on the Philox stream
    ``streams[e]``.  The rounds of :class:`SliceRounds` - the phases, the packing order and hence the chunks of the device driver;
    ``evaluate(rows [R, n], ens [R])`` -> (chi2 [R], status [R]) is the likelihood of a round's rows, ``ens`` the ensemble of every
    row.  Returns (chain [E, rows, W, n], chain_lnl [E, rows, W], stats with ``slice_counts`` [E, 8] and ``rounds``).  The rows of
    the steps below ``tune_steps`` are not a stationary chain: discard them."""
    run = SliceRounds(x, lnl, accepted, mu, step0, n_steps, thin, seed, streams, lo, hi, log_norm, tune_steps, max_expansions,
                      max_contractions)
    chi2 = status = None
    while run.active:
        rows, ens = run.round(chi2, status)
        if rows.shape[0]:
            chi2, status = evaluate(rows, ens)
    st = dict(steps=n_steps, proposals=int(run.counts[:, SC_UPDATES].sum()), accepted=int(run.counts[:, SC_MOVED].sum()),
              rejected_outside_box=0, rejected_failed_model=0, slice_counts=run.counts, rounds=run.rounds)
    if run.rows != int(run.counts[:, SC_ROWS].sum()):
        raise RuntimeError("slice: the engine's rows are not the walkers' requests")
    return run.chain, run.chain_lnl, st


def python_steps(x, lnl, accepted, step0, n_steps, thin, a, seed, stream, lo, hi, log_norm, evaluate, moves=None):
    """``n_steps`` steps of one ensemble in NumPy - :func:`python_steps_many` with E = 1 - from the state ``x`` [W, n], ``lnl`` [W],
    ``accepted`` [W] (updated in place); ``evaluate(rows, h)`` -> (chi2 [W/2], status [W/2]) for the half's rows [W/2, n].
    Returns (chain [rows, W, n], chain_lnl [rows, W], stats)."""
    chain, chain_lnl, st, _ = python_steps_many(x[None], lnl[None], accepted[None], step0, n_steps, thin, a, seed, [stream], lo, hi,
                                                log_norm, evaluate, moves)
    return chain[0], chain_lnl[0], st


def write_getdist(path, name, names, chain, chain_lnl, weights=None, derived=None, derived_names=None, derived_labels=None):
    """getdist's plain-text chain: ``name.txt`` (one row per sample: weight 1, -lnL, the parameters) and ``name.paramnames``
    (one ``name label`` line per parameter, label = name).  ``chain`` [..., n], ``chain_lnl`` [...]; ``weights`` [...]: a
    weighted chain (a nested sampler's), the first column then holds them.  ``derived`` [..., m] with ``derived_names`` [m]
    (``derived_labels`` [m], default the names): derived parameters, their columns after the sampled ones and their lines after
    the sampled parameters' (the layout of the reference's PolyChord chains)."""
    path = Path(path)
    table, lines = getdist_table(names, chain, chain_lnl, weights, derived, derived_names, derived_labels)
    np.savetxt(path / f'{name}.txt', table, fmt='%.17g')
    return path / f'{name}.txt', write_paramnames(path, name, lines)


def write_paramnames(path, name, lines):
    """``name.paramnames`` from (name, label) pairs."""
    with open(Path(path) / f'{name}.paramnames', 'w') as f:
        for nm, label in lines:
            f.write(f'{nm} {label}\n')
    return Path(path) / f'{name}.paramnames'


def getdist_table(names, chain, chain_lnl, weights=None, derived=None, derived_names=None, derived_labels=None):
    """(the rows of :func:`write_getdist`'s ``name.txt`` [samples, 2 + n (+ m)], the (name, label) pairs of its
    ``name.paramnames``)."""
    chain = np.asarray(chain, dtype=np.float64).reshape(-1, len(names))
    lnl = np.asarray(chain_lnl, dtype=np.float64).reshape(-1)
    first = np.ones(lnl.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    columns = [first, -lnl, chain]
    lines = [(nm, nm) for nm in names]
    if derived is not None:
        if derived_names is None:
            raise ValueError('derived columns need derived_names')
        derived_names = list(derived_names)
        labels = derived_names if derived_labels is None else list(derived_labels)
        block = np.asarray(derived, dtype=np.float64).reshape(-1, len(derived_names))
        if block.shape[0] != lnl.size or len(labels) != len(derived_names):
            raise ValueError('derived: one row per sample, one name and one label per column')
        columns.append(block)
        lines += list(zip(derived_names, labels))
    return np.column_stack(columns), lines


def marg_derived_labels(counts):
    """(names, labels) of the marginalisation coefficients as derived parameters for ``counts`` {correlation: coefficients}:
    ``<corr>_marg_<i>`` with the label ``M_{\\rm <corr>}^{<i>}`` (reference vega/samplers/sampler_interface.py:82-89), the
    correlations sorted by name (the stacking order of ``log_lik(..., return_marg_coeff=True)``, reference
    vega/vega_interface.py:371-383), a correlation's coefficients in template order."""
    names, labels = [], []
    for corr in sorted(counts):
        for i in range(int(counts[corr])):
            names.append(f'{corr}_marg_{i}')
            labels.append(f'M_{{\\rm {corr}}}^{{{i}}}')
    return names, labels


def parse_derived(section):
    """``derived = True | False`` of a sampler's section (absent: False); anything else is refused."""
    try:
        return section.getboolean('derived', False)
    except ValueError:
        raise ValueError(f"[{section.name}] derived: True or False") from None


def derived_rows(vega, cols, fixed_row, rows, chunk=0, lanes=0, const_hint=-1):
    """The derived block [R, len(vega.derived_names())] of recorded sampler rows ``rows`` [R, n] (physical values of the columns
    ``cols``; ``fixed_row`` supplies the others): one pass through ``marg_coeff_batch_device`` with the table level the run itself
    used.  Evaluation is deterministic, so this is what recording at evaluation time would have stored; rows that repeat (a
    walker that did not move) are evaluated once."""
    import torch
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(cols))
    m = len(vega.derived_names())
    if m == 0 or rows.shape[0] == 0:
        return np.empty((rows.shape[0], m))
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    theta = np.repeat(np.asarray(fixed_row, dtype=np.float64)[None, :], uniq.shape[0], axis=0)
    theta[:, cols] = uniq
    with EngineRows(vega, cols, chunk, lanes, const_hint) as er:
        block = vega.marg_coeff_batch_device(torch.from_numpy(np.ascontiguousarray(theta)).to(er.device)).cpu().numpy()
    return block[np.asarray(inverse).reshape(-1)]


def derived_for_write(sampler, derived, print_func=print):
    """The keyword arguments ``write_getdist`` takes for a sampler's ``write(..., derived=...)``: empty without the option, and
    with it when no correlation has marginalisation templates (said through ``print_func``)."""
    if not derived:
        return {}
    names = sampler.vega.derived_names()
    if not names:
        print_func('derived = True, but no correlation has marginalisation templates: writing the plain chain')
        return {}
    return dict(derived_names=names, derived_labels=sampler.vega.derived_labels())


def autocorr_func_1d(x):
    """Normalised autocorrelation function of a series by FFT (emcee.autocorr.function_1d)."""
    x = np.asarray(x, dtype=np.float64)
    n = 1
    while n < len(x):
        n <<= 1
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[:len(x)].real
    return acf / acf[0] if acf[0] != 0 else acf


def integrated_time(chain, c=5):
    """Integrated autocorrelation time per parameter of ``chain`` [steps, walkers, n] (or [steps] / [steps, walkers]): the
    walker-averaged autocorrelation function, summed up to Sokal's automatic window M >= c tau (emcee.autocorr.integrated_time)."""
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None, None]
    elif x.ndim == 2:
        x = x[:, :, None]
    tau = np.empty(x.shape[2])
    for d in range(x.shape[2]):
        f = np.mean([autocorr_func_1d(x[:, k, d]) for k in range(x.shape[1])], axis=0)
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(len(taus)) < c * taus
        window = int(np.argmin(m)) if np.any(m) else len(taus) - 1
        tau[d] = taus[window]
    return tau


# ------------------------------------------------------------------ the summary of a chain (vmx_chain.h, restated)
CHAIN_MAX_WALKERS = 1024
CHAIN_LAG_BLOCK = 32
SUMMARY_KEYS = ('count', 'mean', 'sd', 'covariance', 'tau', 'window', 'n_eff')


def _seq_sum(a):
    """The sum over the first axis in index order, one rounded addition per term (vmx_chain::seq_sum)."""
    return np.add.accumulate(a, axis=0)[-1]


def _chain_summary_one(x, c, lag_block, moments=True):
    T, W, n = x.shape
    count = T * W
    S = _seq_sum(x)                                                 # [W, n] the series sums
    m = S / float(T)                                                # the series' own means
    if moments:
        mean = _seq_sum(S) / float(count)
        y = x - mean
        cov = np.empty((n, n))
        for i in range(n):
            cov[i] = _seq_sum(_seq_sum(y[:, :, i, None] * y)) / np.float64(count - 1)
    tau, window = np.empty(n), np.empty(n, dtype=np.int64)
    cen = np.ascontiguousarray(np.moveaxis(x - m, 2, 0))            # [n, T, W] the centred series
    for d in range(n):
        s = cen[d]
        acov0 = _seq_sum(s * s)                                      # [W]
        flat = acov0 == 0.0
        cumulative, lag, closed = 0.0, 0, False
        while not closed:
            for l in range(lag, min(lag + lag_block, T)):
                acov = acov0 if l == 0 else _seq_sum(s[:T - l] * s[l:])
                with np.errstate(divide='ignore', invalid='ignore'):
                    rho = np.where(flat, acov, acov / acov0)
                f = _seq_sum(rho) / float(W)
                cumulative = f if l == 0 else cumulative + f
                taus = 2.0 * cumulative - 1.0
                if not (float(l) < c * taus) or l == T - 1:
                    tau[d], window[d], closed = taus, l, True
                    break
            lag += lag_block
    with np.errstate(divide='ignore', invalid='ignore'):
        n_eff = np.float64(count) / np.max(tau)
    if not moments:
        return dict(count=count, tau=tau, window=window, n_eff=n_eff)
    return dict(count=count, mean=mean, sd=np.sqrt(np.diagonal(cov)), covariance=cov, tau=tau, window=window, n_eff=n_eff)


def chain_summary(chain, first=0, c=5, lag_block=CHAIN_LAG_BLOCK, moments=True):
    """The summary of a recorded chain [rows, W, n] (or [E, rows, W, n]: every ensemble's, stacked) over the rows from ``first``
    on, as vmx_chain_store_summary computes it where the chain is recorded - vega_amd/csrc/vmx_chain.h restated, bit for bit:
    ``dict(count, mean [n], sd [n], covariance [n, n], tau [n], window [n], n_eff)``.  mean / covariance: two passes, ddof = 1
    over rows x walkers (``np.cov``); tau / window: emcee's estimator (:func:`integrated_time`) with direct lag sums up to Sokal's
    window M >= c tau, every sum sequential in its index; sd = sqrt(diag covariance), n_eff = count / max tau.  ``lag_block``
    (the lags computed at a time) changes no bit; without ``moments`` mean, sd and covariance are neither computed nor
    returned.  W >= 2 makes count - 1 >= 1 even for a single row (then tau = -1 and window = 0, as ``integrated_time`` gives)."""
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim not in (3, 4) or x.shape[-1] < 1 or x.shape[-2] < 2:
        raise ValueError('chain [rows, W, n] or [E, rows, W, n], W >= 2')
    first, c, lag_block = int(first), float(c), int(lag_block)
    rows = x.shape[-3]
    if not 0 <= first < rows:
        raise ValueError(f'first: a recorded row, 0 .. {rows - 1} (the summary needs at least one row)')
    if not (c > 0.0 and np.isfinite(c)) or lag_block < 1:
        raise ValueError('c positive and finite, lag_block >= 1')
    if x.ndim == 3:
        return _chain_summary_one(x[first:], c, lag_block, moments)
    parts = [_chain_summary_one(xe[first:], c, lag_block, moments) for xe in x]
    return {key: np.array([p[key] for p in parts]) for key in parts[0]}


# ------------------------------------------------------------------ order statistics and the best row (vmx_chain_select.h, restated)
CHAIN_MAX_RANKS = 32
CHAIN_MAX_QUANTILES = 16
SELECT_KEYS = ('q', 'quantiles', 'lnl_max', 'best', 'best_row', 'best_walker')
_SIGN, _NAN_KEY, _CANONICAL_NAN = np.uint64(1 << 63), np.uint64(2**64 - 1), np.uint64(0x7ff8000000000000)


def chain_keys(x):
    """The order-preserving 64-bit keys of doubles (vmx_select::key): all ones for every NaN of either sign, else ``~b`` if the
    sign bit of the bits ``b`` is set, else ``b | 1 << 63``.  Unsigned order of the keys: -inf < ... < -0 < +0 < ... < +inf < NaN."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    k = np.where((b & _SIGN) != 0, ~b, b | _SIGN)
    return np.where((b & ~_SIGN) > np.uint64(0x7ff0000000000000), _NAN_KEY, k)


def chain_unkeys(k):
    """The doubles of keys (vmx_select::unkey): a value's own bits, the canonical NaN for the NaN key."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k == _NAN_KEY, _CANONICAL_NAN, np.where((k & _SIGN) != 0, k ^ _SIGN, ~k)).view(np.float64)


def _select_rows(chain, first, min_walkers=1):
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim not in (3, 4) or x.shape[-1] < 1 or x.shape[-2] < min_walkers:
        raise ValueError('chain [rows, W, n] or [E, rows, W, n]')
    first = int(first)
    if not 0 <= first < x.shape[-3]:
        raise ValueError(f'first: a recorded row, 0 .. {x.shape[-3] - 1}')
    return (x[None] if x.ndim == 3 else x), first, x.ndim == 3


def chain_order_statistics(chain, ranks, first=0):
    """Exact order statistics of every column of a recorded chain [rows, W, n] (or [E, rows, W, n]) over the rows from ``first``
    on, as vmx_chain_store_order_stats computes them where the chain is recorded - vega_amd/csrc/vmx_chain_select.h restated, bit
    for bit: with N = (rows - first) W values per (ensemble, column), entry r is the ``ranks[r]``-th smallest (0 <= rank < N) in
    the total order of :func:`chain_keys` - NaNs last as in ``np.sort``, -0 before +0 - as that value's own bits, or the
    canonical NaN.  The keys are sorted, not the doubles.  ``ranks``: 1 .. 32 of them, in any order, repeats allowed.
    Returns [n, R] (or [E, n, R])."""
    x, first, single = _select_rows(chain, first)
    ranks = np.atleast_1d(np.asarray(ranks, dtype=np.int64))
    E, rows, W, n = x.shape
    N = (rows - first) * W
    if ranks.ndim != 1 or not 1 <= ranks.size <= CHAIN_MAX_RANKS:
        raise ValueError(f'ranks: 1 .. {CHAIN_MAX_RANKS} of them')
    if np.any(ranks < 0) or np.any(ranks >= N):
        raise ValueError(f'ranks: 0 .. {N - 1}')
    keys = np.moveaxis(chain_keys(x[:, first:]), 3, 1).reshape(E, n, N)
    out = chain_unkeys(np.sort(keys, axis=-1)[:, :, ranks])
    return out[0] if single else out


def chain_best(chain, chain_lnl, first=0):
    """The best recorded row of a chain [rows, W, n] with lnL [rows, W] (or [E, rows, W, n] and [E, rows, W]) over the rows from
    ``first`` on, as vmx_chain_store_best finds it (vega_amd/csrc/vmx_chain_select.h): ``dict(lnl_max, best [n], best_row,
    best_walker)``, per ensemble with a leading E.  A NaN lnL never wins, -inf may; among equal values the lowest (row, walker)
    wins; ``best_row`` counts from row 0 of the chain.  Without a candidate (all NaN): row -1, walker -1, lnL and position NaN."""
    x, first, single = _select_rows(chain, first)
    lnl = np.asarray(chain_lnl, dtype=np.float64)
    lnl = lnl[None] if single else lnl
    if lnl.shape != x.shape[:3]:
        raise ValueError('chain_lnl [rows, W] (or [E, rows, W]) of the chain')
    E, rows, W, n = x.shape
    top, at = np.full(E, np.nan), np.full((E, n), np.nan)
    row, walker = np.full(E, -1, dtype=np.int64), np.full(E, -1, dtype=np.int32)
    for e in range(E):
        flat = lnl[e, first:].reshape(-1)
        valid = ~np.isnan(flat)
        if not np.any(valid):
            continue
        index = int(np.argmax(valid & (flat == flat[valid].max()))) + first * W        # (the first of the equal ones)
        row[e], walker[e] = index // W, index % W
        top[e], at[e] = lnl[e, row[e], walker[e]], x[e, row[e], walker[e]]
    out = dict(lnl_max=top, best=at, best_row=row, best_walker=walker)
    return {key: (val[0].item() if val[0].ndim == 0 else val[0]) for key, val in out.items()} if single else out


def check_quantiles(q):
    """``q`` as a float array: 1 .. 16 values in [0, 1] (ValueError otherwise)."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= CHAIN_MAX_QUANTILES or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f'quantiles: 1 .. {CHAIN_MAX_QUANTILES} values in [0, 1]')
    return q


def quantile_ranks(q, N):
    """What the quantiles ``q`` of N values read: ``(ranks, lo, hi, g)`` with ``h = q (N - 1)`` in double, ``floor(h)`` and
    ``min(floor(h) + 1, N - 1)`` as places ``lo`` / ``hi`` in the sorted, distinct ``ranks`` (at most 2 Q <= 32 of them), and the
    fraction ``g = h - floor(h)``."""
    q = check_quantiles(q)
    h = q * np.float64(N - 1)
    low = np.floor(h)
    g = h - low
    low = low.astype(np.int64)
    high = np.minimum(low + 1, N - 1)
    ranks = np.unique(np.concatenate([low, high]))
    return ranks, np.searchsorted(ranks, low), np.searchsorted(ranks, high), g


def quantiles_of_order_statistics(stats, lo, hi, g):
    """``x_lo + g (x_hi - x_lo)`` over order statistics [..., R]: every operation a separately rounded IEEE one."""
    x_lo, x_hi = stats[..., lo], stats[..., hi]
    with np.errstate(invalid='ignore', over='ignore'):
        return x_lo + g * (x_hi - x_lo)


def chain_quantiles(chain, q, first=0):
    """The quantiles ``q`` (1 .. 16 values in [0, 1]) of every column of a recorded chain over the rows from ``first`` on,
    [n, Q] (or [E, n, Q]): host arithmetic over exact order statistics (:func:`chain_order_statistics`), so the device and the
    ``python`` driver give the same bits.  With N = (rows - first) W values: ``h = q (N - 1)`` in double, ``lo = floor(h)``,
    ``hi = min(lo + 1, N - 1)``, ``g = h - lo`` and the value ``x_lo + g (x_hi - x_lo)`` - ``np.quantile(method='linear')`` up
    to the rounding of the two fractional ranks."""
    x, first, single = _select_rows(chain, first)
    ranks, lo, hi, g = quantile_ranks(q, (x.shape[1] - first) * x.shape[2])
    out = quantiles_of_order_statistics(chain_order_statistics(x, ranks, first), lo, hi, g)
    return out[0] if single else out


# ------------------------------------------------------------------ what every sampler here sets up the same way
_NO_LIMITS = ('Sampler needs well defined prior limits. You passed a None. Please give numbers, or'
              ' just say par_name = True to use defaults.')


class SampledBox:
    """The sampled parameters of ``vega`` with their box: ``sample_params['limits']`` (the ``[sample]`` section, or the
    ``[monte carlo]`` one after ``initialize_monte_carlo``, as bin/run_vega_mpi.py picks them), checked as the reference checks
    them.  names, lo, hi, values, errors, n, cols (the engine's columns)."""

    def __init__(self, vega, sample_params=None):
        sp = vega.sample_params if sample_params is None else sample_params
        limits = dict(sp['limits'])
        for lims in limits.values():
            if lims is None or None in tuple(lims):
                raise ValueError(_NO_LIMITS)
        self.names = list(limits)
        if not self.names:
            raise ValueError('no sampled parameters')
        unknown = [nm for nm in self.names if nm not in vega.param_names]
        if unknown:
            raise KeyError(f'unknown parameters {unknown}')
        self.lo = np.array([float(limits[nm][0]) for nm in self.names])
        self.hi = np.array([float(limits[nm][1]) for nm in self.names])
        if not (np.all(np.isfinite(self.lo)) and np.all(np.isfinite(self.hi)) and np.all(self.lo < self.hi)):
            raise ValueError('Sampler needs well defined prior limits: finite, lower < upper')
        self.values = {nm: sp.get('values', {}).get(nm, vega.params.get(nm)) for nm in self.names}
        self.errors = {nm: sp.get('errors', {}).get(nm) for nm in self.names}
        self.n = len(self.names)
        self.cols = np.array([vega.param_names.index(nm) for nm in self.names], dtype=np.int32)


def freeze_and_pick_driver(vega, first_row, cols, driver_asked, device_method):
    """Before the first likelihood: ``freeze_metals`` on ``first_row`` (fast_metals: it plays the reference's first call; the
    engine may be replaced), the sampled columns must not be pinned by it, and the driver the engine allows - an engine group
    (one engine per transform setting, no single C handle, hence no ``device_method``) takes ``'python'``."""
    vega.freeze_metals(first_row)
    pinned = set(int(c) for c in getattr(vega, '_pinned_slots', ()))
    if pinned & set(int(c) for c in cols):
        raise ValueError('frozen metal terms: ' + ', '.join(vega._pinned_names) + ' must keep the values they had '
                         'when the terms were frozen (or be listed in [sample] beforehand)')
    return driver_asked if hasattr(vega.engine, device_method) else 'python'


class EngineRows:
    """The engine as a ``python`` driver's likelihood, set up as the device drivers set it up: inside the ``with`` block
    ``chi2(theta_rows)`` evaluates host rows [R, n_params] through ``chi2_batch_device`` in chunks of ``chunk`` (0: max_batch)
    with the table level the sampled columns ``cols`` allow (``const_hint`` -1) and two lanes; both are restored on exit.
    ``calls`` counts the engine calls."""

    def __init__(self, vega, cols, chunk=0, lanes=0, const_hint=-1):
        self.vega, self.eng = vega, vega.engine
        eng = self.eng
        self.single = hasattr(eng, 'ensemble_run')
        self.chunk = max(1, min(chunk if chunk > 0 else eng.max_batch, eng.max_batch))
        self.hint = const_hint
        if self.hint < 0:
            self.hint = eng.derived_const_hint(cols) if self.single else 0
        self.want_lanes = min(lanes if lanes > 0 else 2, 2)
        self.calls = 0

    def __enter__(self):
        import torch
        eng = self.eng
        self.saved_hint, self.saved_lanes = getattr(eng, 'nl_hint', 0), getattr(eng, 'lanes', 1)
        own = getattr(eng, 'rows_device', None)          # (a stand-in engine without a GPU names where its rows live)
        self.device = torch.device('cuda', getattr(eng, 'device', 0)) if own is None else torch.device(own)
        try:
            eng.set_constant_nl_hint(self.hint > 0, self.hint >= 2)
            if self.single and self.want_lanes > self.saved_lanes:
                eng.set_lanes(self.want_lanes)
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        eng = self.eng
        eng.set_constant_nl_hint(self.saved_hint > 0, self.saved_hint >= 2)
        if self.single and getattr(eng, 'lanes', 1) != self.saved_lanes:
            eng.set_lanes(self.saved_lanes)
        return False

    def chi2(self, theta_rows, mock_rows=None):
        """``mock_rows`` [R] (None: the installed data): per row the row of the mock pools it is compared with."""
        import torch
        t_dev = torch.from_numpy(np.ascontiguousarray(theta_rows)).to(self.device)
        R = theta_rows.shape[0]
        chi2 = np.empty(R)
        if mock_rows is None:
            for off in range(0, R, self.chunk):
                chi2[off:off + self.chunk] = self.vega.chi2_batch_device(t_dev[off:off + self.chunk].contiguous()).cpu().numpy()
                self.calls += 1
            return chi2
        m_dev = torch.from_numpy(np.ascontiguousarray(mock_rows, dtype=np.int32)).to(self.device)
        for off in range(0, R, self.chunk):
            chi2[off:off + self.chunk] = self.vega.chi2_batch_device(t_dev[off:off + self.chunk].contiguous(),
                                                                     mock_rows=m_dev[off:off + self.chunk].contiguous()).cpu().numpy()
            self.calls += 1
        return chi2


class EngineSampler:
    """What the samplers over ``vega`` hold and do alike (a mixin, set up by :meth:`_setup_engine`: the cube samplers' bases have
    constructors of their own): the interface, the sampled box (names, lo, hi, values, errors, cols), the driver asked for and the
    one picked when the first likelihood knows the engine, ``chunk`` / ``lanes`` / ``const_hint`` of the engine's calls."""

    def _setup_engine(self, vega, sample_params, driver, chunk, lanes, const_hint):
        """Returns the number of sampled parameters."""
        if driver not in ('device', 'python'):
            raise ValueError("driver: 'device' or 'python'")
        self.vega = vega
        box = SampledBox(vega, sample_params)
        self.names, self.lo, self.hi, self.values, self.errors, self.cols = box.names, box.lo, box.hi, box.values, box.errors, box.cols
        self.driver_asked, self.driver = driver, None
        self.chunk, self.lanes, self.const_hint = int(chunk), int(lanes), int(const_hint)
        self._rows = None
        return box.n

    def log_norm(self):
        return float(self.vega._log_norm())

    def _fixed_row(self):
        return np.asarray(self.vega._theta(None), dtype=np.float64).copy()

    def _pick_driver(self, first_row, device_method):
        self.driver = freeze_and_pick_driver(self.vega, first_row, self.cols, self.driver_asked, device_method)

    def _engine_rows(self):
        return EngineRows(self.vega, self.cols, self.chunk, self.lanes, self.const_hint)

    def _derived_of(self, rows):
        return derived_rows(self.vega, self.cols, self._fixed_row(), rows, self.chunk, self.lanes, self.const_hint)

    def _write_extra(self, derived, print_func, block):
        """The derived-parameter arguments of ``write_getdist`` for ``write(..., derived=...)``; ``block()`` computes the rows."""
        extra = derived_for_write(self, derived, print_func)
        if extra:
            extra['derived'] = block()
        return extra

    # ---- the samplers in the unit cube (a uniform prior over the box)
    def to_physical(self, u):
        from .nested import map_cube
        return map_cube(self.lo, self.hi, np.asarray(u, dtype=np.float64))

    def _evaluate(self, rows_u):
        from .nested import lnl_of
        rows_t = np.repeat(self._theta[None, :], rows_u.shape[0], axis=0)
        rows_t[:, self.cols] = self.to_physical(rows_u)
        # (chi2_batch_device reports a failed model by the 1e100 sentinel alone)
        return lnl_of(0, self._rows.chi2(rows_t), self.log_norm())

    def _begin_advance(self, first_u, device_method):
        """The fixed row of this call; on the first one the driver (``first_u``: the first point the run evaluates)."""
        self._theta = self._fixed_row()
        if self.driver is None:
            first = self._theta.copy()
            first[self.cols] = self.to_physical(first_u())
            self._pick_driver(first, device_method)

    def _advance_python(self, advance, count):
        """``advance(count)`` of the NumPy driver with the engine behind ``_evaluate``; its last result is the statistics."""
        with self._engine_rows() as self._rows:
            try:
                out = advance(count)
            finally:
                calls, self._rows = self._rows.calls, None
        out[-1]['engine_calls'] = out[-1]['host_waits'] = calls
        return out

    def derived(self):
        """The derived parameters (``vega.derived_names()``: the marginalisation coefficients) of the rows of ``samples()``,
        [N, m]: a pass over them after the run (:func:`derived_rows`), the same block whichever driver ran."""
        return self._derived_of(self.samples()[0])


# ------------------------------------------------------------------ the sampler
class MoveCounts(Mapping):
    """``stats['moves']`` of a sampler that runs a mixture of moves: {move: {proposals, accepted}} over the steps run so far,
    computed when it is read (:meth:`StretchSampler.move_counts`) and kept until the sampler advances; ``accepted`` is None
    with thin > 1.  ``unseen``: the accepted proposals no move could be credited with (None with thin > 1).  The moves are the
    three of ``MOVE_NAMES``, and ``cov`` when the mixture has it."""

    def __init__(self, sampler):
        self._sampler, self._step, self._counts, self._unseen = sampler, -1, None, None
        self._names = COV_MOVE_NAMES if has_cov(sampler.moves) else MOVE_NAMES

    def _read(self):
        s = self._sampler
        if self._step != s.step:
            total = s.move_counts().reshape(-1, len(self._names), 2).sum(axis=0)
            known = s.thin == 1
            self._counts = {name: dict(proposals=int(total[m, 0]), accepted=int(total[m, 1]) if known else None)
                            for m, name in enumerate(self._names)}
            self._unseen = int(np.sum(s.accepted)) - int(total[:, 1].sum()) if known else None
            self._step = s.step
        return self._counts

    @property
    def unseen(self):
        self._read()
        return self._unseen

    def __getitem__(self, name):
        return self._read()[name]

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)

    def __repr__(self):
        return repr(self._read())


class StretchSampler(EngineSampler):
    """What :class:`EnsembleSampler` and :class:`EnsembleSet` do alike: the settings of the stretch move, the statistics, the loop
    over segments and the python driver's engine.  ``_lead`` is the shape in front of the walkers: () or (E,).  A class supplies
    ``_prepare``, ``_segment_device`` and ``_python_steps``; a segment returns (chain, chain_lnl, stats) and, for a set, the
    per-ensemble counters."""
    _lead = ()

    def _setup_walkers(self, vega, walkers, a, seed, thin, driver, segment, sample_params, chunk, lanes, const_hint, moves=None,
                       gamma0=None, sigma=None, gamma_s=None, mu=None, tune_steps=None, cov_scale=None, chain='host'):
        self.n = self._setup_engine(vega, sample_params, driver, chunk, lanes, const_hint)
        if chain not in ('host', 'device'):
            raise ValueError("chain: 'host' or 'device'")
        self.chain_mode, self._store, self.convergence, self._fetched = chain, None, None, {}
        self.W = int(walkers)
        if chain == 'device' and self.W > CHAIN_MAX_WALKERS:
            raise ValueError(f"chain='device': at most {CHAIN_MAX_WALKERS} walkers")
        if self.W % 2 or self.W < 2 * self.n:
            raise ValueError(f'walkers: an even number, at least twice the {self.n} sampled parameters')
        self.a, self.seed = float(a), int(seed)
        if not self.a > 1.0:
            raise ValueError('a: the stretch scale must exceed 1')
        self.thin = int(thin)
        if self.thin < 1:
            raise ValueError('thin >= 1')
        self.segment = max(1, int(segment))
        # ensemble slice sampling (None: not asked for): mu0 and tune_steps; it is no member of a mixture
        self.slice = resolve_slice(moves, self.W, mu, tune_steps, gamma0, sigma, gamma_s)
        if self.slice is not None:
            if cov_scale is not None:
                raise ValueError("cov_scale is the scale of the 'cov' move, not of 'slice'")
            self.moves, self._moves_kw = None, dict(moves='slice', mu=self.slice['mu0'], tune_steps=self.slice['tune_steps'])
            return
        # the mixture of moves (None: the stretch move alone, the run of ever) and what asked for it, for a set's members
        self.moves = resolve_moves(moves, self.n, self.W, gamma0, sigma, gamma_s, cov_scale)
        self._moves_kw = {} if moves is None else dict(moves=moves, gamma0=gamma0, sigma=sigma, gamma_s=gamma_s)
        if cov_scale is not None:
            self._moves_kw['cov_scale'] = cov_scale

    def reset(self):
        self.x = self.lnl = None
        self.accepted = np.zeros(self._lead + (self.W,), dtype=np.int64)
        self.step = 0
        self._chain, self._chain_lnl = [], []
        self._drop_store()
        self.convergence = None
        self.stats = dict(steps=0, proposals=0, accepted=0, rejected_outside_box=0, rejected_failed_model=0, engine_calls=0,
                          seconds=0.0, seconds_enqueuing=0.0, host_synchronisations=0, calls=0)
        if self.moves is not None:
            self._start = None          # (the walkers ahead of the first step: what the first recorded row is compared with)
            self.stats['moves'] = MoveCounts(self)
        if has_cov(self.moves):
            # the half-steps whose factor fell back to the diagonal, per ensemble; stats['cov'] carries their sum
            self.cov_fallbacks = np.zeros(int(np.prod(self._lead, dtype=np.int64)), dtype=np.int64)
            self.stats['cov'] = dict(scale=self.moves['cov_scale'], factor_fallbacks=0)
        if self.slice is not None:
            lead = int(np.prod(self._lead, dtype=np.int64))
            self.mu = np.full(lead, self.slice['mu0'])
            self.slice_counts = np.zeros((lead, 8), dtype=np.int64)
            self.stats['rounds'] = 0
            self._slice_took()

    def _slice_took(self, st=None):
        """The counts of a segment join the run's: ``stats['slice']``, ``stats['mu']`` and ``stats['moves']`` as the drivers'
        counters have them."""
        if st is not None:
            self.slice_counts += st['slice_counts']
        self.stats['slice'] = slice_stats(self.slice_counts, self.mu)
        self.stats['mu'] = self.mu.copy() if self._lead else float(self.mu[0])
        self.stats['moves'] = {'slice': dict(proposals=self.stats['slice']['updates'], accepted=self.stats['slice']['moved'])}

    def _slice_arg(self):
        return dict(tune_steps=self.slice['tune_steps'], max_expansions=SLICE_MAX_EXPANSIONS, max_contractions=SLICE_MAX_CONTRACTIONS)

    def move_counts(self):
        """Per move the proposals and the accepted ones of the steps run so far, int64 [(E,) 3, 2] in the order of
        ``MOVE_NAMES`` ([(E,) 4, 2], ``COV_MOVE_NAMES``, when the mixture has the covariance move): counted on the host, and only when asked for (``stats['moves']`` reads it), from the words the drivers
        drew the moves from (block B of every walker) and the recorded rows - a run does not pay for it.  With a row for every
        step (thin = 1) a proposal counts as accepted when the walker's recorded position or lnL changed; an accepted proposal
        that lands on the walker's own position bit for bit (DE between two partners at one point, a snooker projection of
        exactly 0) is not seen: ``stats['moves'].unseen`` counts those.  With thin > 1 the accepted column is 0 and unknown."""
        H = self.W // 2
        lead = int(np.prod(self._lead, dtype=np.int64))
        streams = self.streams if self._lead else [self.stream]
        nm = 4 if has_cov(self.moves) else 3
        counts = np.zeros((lead, nm, 2), dtype=np.int64)
        if self.step > 0:
            axis = len(self._lead)
            rows = np.concatenate(self._recorded(), axis=axis).reshape(lead, -1, self.W, self.n)
            rows_lnl = np.concatenate(self._recorded(lnl=True), axis=axis).reshape(lead, -1, self.W)
            start, start_lnl = (a.reshape((lead, 1) + a.shape[axis:]) for a in self._start)
            for e in range(lead):
                move = steps_moves(H, 0, self.step, self.seed, int(streams[e]), self.moves)         # [steps, W]
                counts[e, :, 0] = np.bincount(move.reshape(-1), minlength=nm)
                if self.thin == 1:
                    moved = np.any(np.diff(np.concatenate([start[e], rows[e]]), axis=0) != 0.0, axis=2)
                    moved |= np.diff(np.concatenate([start_lnl[e], rows_lnl[e]]), axis=0) != 0.0
                    counts[e, :, 1] = np.bincount(move[moved], minlength=nm)
        return counts.reshape(self._lead + (nm, 2))

    def run(self, n_steps, start='ball', init_scale=1.0):
        """Advance by ``n_steps`` steps.  The first call draws the start, as the class's ``_start_positions`` says: ``'ball'``,
        ``'prior'`` or an array; later calls continue the chain."""
        theta = self._prepare(start, init_scale)
        try:
            self._open_store(int(n_steps))
            self._advance(theta, int(n_steps))
        finally:
            if self._store is not None:
                self.vega.engine.attach_chain_store(None)
        return self

    # ---- the recorded rows: a list of host blocks, or - chain='device' with the device driver - a store on the device
    def _rows_in_store(self):
        return self.chain_mode == 'device' and self.driver == 'device'

    def _open_store(self, n_steps):
        """Ahead of a run of ``n_steps`` steps with the rows on the device: the store, with room for the rows the run adds (sized from
        the first run's steps, grown by ``reserve`` on later calls), attached to the engine for the run."""
        if not self._rows_in_store():
            return
        eng = self.vega.engine
        need = (self.step + n_steps) // self.thin
        if self._store is not None and self._store.engine is not eng:
            raise RuntimeError("chain='device': the engine was replaced after rows were recorded on it")
        if self._store is None:
            self._store = eng.chain_store(int(np.prod(self._lead, dtype=np.int64)), self.W, self.n, need)
        else:
            self._store.reserve(need)
        self._fetched = {}
        eng.attach_chain_store(self._store)

    def _drop_store(self):
        store, self._store = getattr(self, '_store', None), None
        self._fetched = {}
        if store is not None:
            store.close()

    def close(self):
        """Release the chain store of ``chain='device'``: a sampler that has run owns its recorded rows on the device (with
        ``sample_mocks(summaries='device')`` the whole chain of every mock) until it is closed, reset or collected.  The rows are
        brought to the host first, so ``get_chain``, ``summary`` and the moves' counters keep answering - from the host rows,
        the same numbers; ``keep=False`` drops the rows instead (then those raise or return nothing)."""
        return self._close(True)

    def _close(self, keep):
        if self._store is not None:
            if keep and self._store.rows > 0:
                chain, chain_lnl = self._store.fetch()
                self._chain, self._chain_lnl = ([chain], [chain_lnl]) if self._lead else ([chain[0]], [chain_lnl[0]])
            self._drop_store()
        return self

    def discard_chain(self):
        """Release the chain store without bringing its rows to the host: the summaries already taken are all that is kept."""
        return self._close(False)

    def _recorded(self, lnl=False):
        """The recorded blocks, positions or lnL: the host list, or the store's rows fetched as one block."""
        if self._store is None or self._store.rows == 0:
            return self._chain_lnl if lnl else self._chain
        # (fetched once per state of the store: the members of a set slice one copy instead of fetching the whole store each)
        rows = self._store.rows
        held = self._fetched.get(lnl)
        if held is None or held[0] != rows:
            arr = self._store.fetch(lnl=True)[1] if lnl else self._store.fetch(lnl=False)[0]
            held = self._fetched[lnl] = (rows, arr if self._lead else arr[0])
        return [held[1]]

    def _recorded_count(self):
        """Rows recorded so far, per ensemble."""
        if self._store is not None:
            return self._store.rows
        return sum(part.shape[len(self._lead)] for part in self._chain_lnl)

    def summary(self, discard=0, c=5, quantiles=None):
        """``dict(count, mean, sd, covariance, tau, window, n_eff)`` of the recorded rows from ``discard`` on (per ensemble for a
        set: arrays with a leading E): mean and covariance (ddof 1) over rows x walkers, emcee's integrated autocorrelation time
        with its window, n_eff = count / max tau.  With the rows on the device (``chain='device'``, device driver) it is computed
        there (vmx_chain_store_summary) and a few numbers per ensemble cross to the host; otherwise it is
        :func:`chain_summary` over the host rows - the same numbers bit for bit.  ``quantiles=q`` adds the keys ``q``,
        ``quantiles`` [(E,) n, Q] (:meth:`quantiles`) and ``lnl_max``, ``best``, ``best_row``, ``best_walker`` (:meth:`best`);
        without it the dict is what it was."""
        if quantiles is not None:
            quantiles = check_quantiles(quantiles)
        if self._store is not None:
            out = self._store.summary(int(discard), c)
            out = out if self._lead else {key: (val[0].item() if val[0].ndim == 0 else val[0]) for key, val in out.items()}
        else:
            axis = len(self._lead)
            parts = self._chain
            if not parts:
                raise ValueError('summary: no recorded rows')
            out = chain_summary(np.concatenate(parts, axis=axis), int(discard), c)
            if not self._lead:
                out['n_eff'] = float(out['n_eff'])
        if quantiles is not None:
            out.update(q=quantiles, quantiles=self.quantiles(quantiles, discard), **self.best(discard))
        return out

    def _host_rows(self, what):
        """The recorded rows on the host as one block each, positions and lnL, for the restatements."""
        if not self._chain:
            raise ValueError(f'{what}: no recorded rows')
        axis = len(self._lead)
        return np.concatenate(self._chain, axis=axis), np.concatenate(self._chain_lnl, axis=axis)

    def quantiles(self, q, discard=0):
        """The quantiles ``q`` (1 .. 16 values in [0, 1]) of every sampled parameter over the recorded rows from ``discard`` on,
        [n, Q] (a set: [E, n, Q]), as :func:`chain_quantiles` defines them: linear interpolation between exact order statistics.
        With the rows on the device (``chain='device'``, device driver) the order statistics are found there
        (vmx_chain_store_order_stats) and at most 2 Q numbers per ensemble and parameter cross to the host; otherwise they come
        from the host rows - the same bits, since the interpolation is the same host arithmetic."""
        q, discard = check_quantiles(q), int(discard)
        if self._store is None:
            return chain_quantiles(self._host_rows('quantiles')[0], q, discard)
        rows = self._store.rows
        if not 0 <= discard < rows:
            raise ValueError(f'discard: a recorded row, 0 .. {rows - 1}')
        ranks, lo, hi, g = quantile_ranks(q, (rows - discard) * self.W)
        out = quantiles_of_order_statistics(self._store.order_statistics(ranks, discard), lo, hi, g)
        return out if self._lead else out[0]

    def best(self, discard=0):
        """``dict(lnl_max, best [n], best_row, best_walker)`` of the recorded rows from ``discard`` on (a set: arrays with a
        leading E): the largest recorded lnL and where it was - the lowest (row, walker) among equal ones, ``best_row`` counted
        from the first recorded row.  On the device with the rows there (vmx_chain_store_best), else :func:`chain_best`."""
        if self._store is None:
            return chain_best(*self._host_rows('best'), int(discard))
        out = self._store.best(int(discard))
        return out if self._lead else {key: (val[0].item() if val[0].ndim == 0 else val[0]) for key, val in out.items()}

    def _tau_now(self, discard, c):
        """tau [(E,) n] and the rows used of the check of :meth:`run_until`: E n doubles from the device."""
        if self._store is not None:
            tau = self._store.summary(int(discard), c, moments=False)['tau']
            return tau if self._lead else tau[0]
        axis = len(self._lead)         # (the rows behind the burn-in alone are stacked, and the moments are skipped)
        done, parts = 0, []
        for part in self._chain:
            rows = part.shape[axis]
            if done + rows > discard:
                parts.append(part[(slice(None),) * axis + (slice(max(discard - done, 0), None),)])
            done += rows
        return chain_summary(np.concatenate(parts, axis=axis), 0, c, moments=False)['tau']

    def run_until(self, max_steps, tau_factor=50, tau_rtol=0.01, check_every=100, burn=1.0 / 3.0, c=5, start='ball', init_scale=1.0):
        """Advance until the chain is long enough by its own integrated autocorrelation time (emcee's recipe), at most
        ``max_steps`` steps: after every ``check_every`` steps tau is estimated over the recorded rows behind the first
        floor(``burn`` rows); an ensemble is converged at a check when rows_used >= ``tau_factor`` max_d tau and max_d |tau -
        tau_previous| / tau <= ``tau_rtol``.  The run ends at the first check at which every ensemble is converged (all
        ensembles advance together until then), or at ``max_steps``.  ``convergence`` keeps ``dict(steps [checks], tau [checks,
        (E,) n], rows_used [checks], converged [(E,)], converged_at [(E,)]: the step of the first check at which the ensemble
        held, -1 if never)``.  The decision is host arithmetic over numbers both drivers produce bit for bit: both stop at the
        same step."""
        max_steps, check_every = int(max_steps), int(check_every)
        tau_factor, tau_rtol, burn = float(tau_factor), float(tau_rtol), float(burn)
        if max_steps < 1 or check_every < 1:
            raise ValueError('run_until: max_steps >= 1, check_every >= 1')
        if not (tau_factor > 0.0 and np.isfinite(tau_factor)) or not (tau_rtol >= 0.0 and np.isfinite(tau_rtol)):
            raise ValueError('run_until: tau_factor positive, tau_rtol not negative, both finite')
        if not 0.0 <= burn < 1.0:
            raise ValueError('run_until: burn in [0, 1)')
        lead = self._lead
        steps, taus, used = [], [], []
        converged, at = np.zeros(lead, dtype=bool), np.full(lead, -1, dtype=np.int64)
        previous, done = None, 0
        while done < max_steps:
            k = min(check_every, max_steps - done)
            self.run(k, start=start, init_scale=init_scale)
            done += k
            rows = self._recorded_count()
            if rows < 1:
                continue
            discard = int(np.floor(burn * rows))
            tau = np.asarray(self._tau_now(discard, c), dtype=np.float64)
            steps.append(self.step), taus.append(tau), used.append(rows - discard)
            with np.errstate(divide='ignore', invalid='ignore'):
                worst = np.max(tau, axis=-1)
                long_enough = (rows - discard) >= tau_factor * worst
                settled = np.max(np.abs(tau - previous) / tau, axis=-1) <= tau_rtol if previous is not None else np.zeros(lead, dtype=bool)
            converged = np.asarray(long_enough & settled & np.all(np.isfinite(tau) & (tau > 0.0), axis=-1))
            at = np.where((at < 0) & converged, self.step, at)
            previous = tau
            if np.all(converged):
                break
        self.convergence = dict(steps=np.array(steps, dtype=np.int64), tau=np.array(taus).reshape((len(taus),) + lead + (self.n,)),
                                rows_used=np.array(used, dtype=np.int64), converged=converged if lead else bool(converged),
                                converged_at=at if lead else int(at), max_steps=max_steps, tau_factor=tau_factor, tau_rtol=tau_rtol,
                                check_every=check_every, burn=burn)
        return self

    def _advance(self, theta, n_steps):
        done = 0
        on_device = self._store is not None
        while done < n_steps:
            k = min(self.segment, n_steps - done)
            segment = self._segment_device if self.driver == 'device' else self._segment_python
            if self.moves is not None and self._start is None:
                self._start = (self.x.copy(), self.lnl.copy())
            chain, chain_lnl, st, *per = segment(theta, k)
            if not on_device:
                self._chain.append(chain)
                self._chain_lnl.append(chain_lnl)
            if per:             # (a set's segment: the counters of every ensemble)
                self.per_ensemble += per[0]
            for key in st:
                if key in self.stats:
                    self.stats[key] += st[key]
            if self.slice is not None:
                self._slice_took(st)
            if has_cov(self.moves):
                self.cov_fallbacks += st['cov_fallbacks']
                self.stats['cov']['factor_fallbacks'] = int(self.cov_fallbacks.sum())
            self.stats['calls'] += 1
            self.step += k
            done += k

    def _keep_arg(self):
        # (with the rows in a store the library is asked for no host chain; otherwise the methods are called as ever)
        return dict(keep_chain=False) if self._store is not None else {}

    def _segment_python(self, theta, k):
        """The readable restatement: proposals and decisions in NumPy (``_python_steps``), chi2 of a half's rows through
        ``chi2_batch_device`` in the device driver's chunks, with its table level and lanes and, where given, every row's mock."""
        import time
        t0 = time.perf_counter()
        with self._engine_rows() as rows:
            def chi2(rows_x, mock_rows=None):
                rows_t = np.repeat(theta[None, :], rows_x.shape[0], axis=0)
                rows_t[:, self.cols] = rows_x
                # (chi2_batch_device reports a failed model by the 1e100 sentinel alone)
                return rows.chi2(rows_t, mock_rows=mock_rows), np.zeros(rows_x.shape[0], dtype=np.int32)

            out = self._python_steps(k, chi2)
        st = out[2]
        st['engine_calls'] = rows.calls
        st['host_synchronisations'] = rows.calls
        st['seconds'] = time.perf_counter() - t0
        return out

    def _moves_arg(self):
        # (without moves the engine's methods are called as ever: a stand-in engine need not know the argument)
        return {} if self.moves is None else dict(moves=self.moves)

    @property
    def acceptance_fraction(self):
        return self.accepted / max(self.step, 1)


class EnsembleSampler(StretchSampler):
    """W walkers over the sampled parameters of ``vega`` (``sample_params['limits']``: the ``[sample]`` section, or the
    ``[monte carlo]`` one after ``initialize_monte_carlo``, as bin/run_vega_mpi.py picks them; ``sample_params`` overrides).

    ``driver``: ``'device'`` (vmx_ensemble_run) or ``'python'`` (the NumPy restatement over ``chi2_batch_device``); an engine
    group (one engine per transform setting, no single C handle) takes ``'python'``.  The choice is made when ``run`` knows the
    engine - ``freeze_metals`` may replace it.  ``segment``: steps per call of the driver (the chain does not depend on it).

    ``moves`` (emcee's ``moves=``): None - the stretch move, the run of ever - or ``'stretch'``, ``'de'`` (emcee's DEMove),
    ``'snooker'`` (DESnookerMove) or a list of (name, weight), e.g. ``[('de', 0.8), ('snooker', 0.2)]``: every walker's move is
    drawn from the mixture at every step (vmx_ensemble_run_many_moves; the ``python`` driver runs the same rule).  ``gamma0``
    (default 2.38 / sqrt(2 n)) and ``sigma`` (1e-5) are the DE move's scale and jitter, ``gamma_s`` (1.7) the snooker's scale;
    DE needs 4 walkers, the snooker 6.  ``stats['moves']`` then counts per move the proposals and - with a row for every step
    (thin = 1) - the accepted ones, on the host from the words the moves were drawn from, when it is read
    ``moves='cov'``, or ``('cov', w)`` in the list: the covariance move (emcee's WalkMove over the whole other half, with the
    Roberts-Gelman-Gilks scale; vmx_ensemble_run_many_cov) - a Metropolis step whose increment has the covariance of the other half
    times ``cov_scale`` (default 2.38 / sqrt(n)), the factor computed on the device at every half-step.  It needs 4 walkers;
    ``stats['moves']`` then has a ``cov`` entry and ``stats['cov']`` is ``dict(scale, factor_fallbacks)`` - the half-steps whose
    covariance had no Cholesky factor and fell back to its diagonal.  It does not combine with tempering or ``'slice'`` yet.
    (:class:`MoveCounts`: the run itself does not pay for it).

    ``moves='slice'``: ensemble slice sampling (Karamanis & Beutler 2021, zeus's differential move; vmx_ensemble_run_slice, and
    :func:`python_steps_slice_many` the same run bit for bit) instead of a proposal and a decision - a sampler of its own, not a
    member of a mixture.  Every update moves its walker along the difference of two walkers of the other half, scaled by ``mu``
    (default 1.0), to a point drawn by a slice-sampling bracket; a trial point outside the box costs no likelihood row.  ``mu``
    tunes itself after every step with global index below ``tune_steps`` (default 100): discard those rows.  ``a`` is not read.
    ``stats['slice']`` holds the counts of ``SLICE_COUNT_NAMES`` (summed, and ``per_ensemble``) with ``rows_per_update``,
    ``stats['mu']`` the scale as it stands, ``stats['moves']`` is ``{'slice': {proposals: updates, accepted: moved}}``,
    ``stats['rounds']`` the rounds of the run, and ``accepted`` counts per walker the updates that moved it."""

    def __init__(self, vega, walkers, a=2.0, seed=0, thin=1, driver='device', segment=1000, sample_params=None, stream=0,
                 chunk=0, lanes=0, const_hint=-1, moves=None, gamma0=None, sigma=None, gamma_s=None, mu=None, tune_steps=None,
                 cov_scale=None, chain='host'):
        self._setup_walkers(vega, walkers, a, seed, thin, driver, segment, sample_params, chunk, lanes, const_hint, moves, gamma0,
                            sigma, gamma_s, mu, tune_steps, cov_scale, chain)
        self.stream = int(stream)
        self.reset()

    # ---- start
    def _start_positions(self, start, init_scale):
        """The start of ``run``'s first call: ``'ball'`` - the configured values plus init_scale x errors x N(0, 1), redrawn until
        inside the box - ``'prior'`` - uniform in the box - or an array [W, n]; both draws from ``np.random.default_rng(seed)``,
        with a non-zero ``stream`` from ``default_rng([seed, stream])``."""
        # (stream 0 draws what it always drew; another stream - a replica - starts from walkers of its own)
        rng = np.random.default_rng(self.seed if self.stream == 0 else [self.seed, self.stream])
        if isinstance(start, str) and start == 'prior':
            return self.lo + (self.hi - self.lo) * rng.random((self.W, self.n))
        if isinstance(start, str) and start == 'ball':
            centre = np.array([float(self.values[nm]) for nm in self.names])
            err = np.array([float(self.errors[nm]) if self.errors[nm] is not None else 0.01 * (h - l)
                            for nm, l, h in zip(self.names, self.lo, self.hi)])
            x = np.empty((self.W, self.n))
            for w in range(self.W):
                for _ in range(10000):
                    p = centre + init_scale * err * rng.standard_normal(self.n)
                    if np.all(p >= self.lo) and np.all(p <= self.hi):
                        break
                else:
                    raise ValueError('start ball: no draw inside the box (configured values outside the limits?)')
                x[w] = p
            return x
        x = np.array(start, dtype=np.float64)
        if x.shape != (self.W, self.n):
            raise ValueError(f'start: an array [{self.W}, {self.n}], "ball" or "prior"')
        if not (np.all(x >= self.lo) and np.all(x <= self.hi)):
            raise ValueError('start: every walker inside the box')
        return x

    def _prepare(self, start, init_scale):
        vega = self.vega
        theta = self._fixed_row()
        if self.x is None:
            x0 = self._start_positions(start, init_scale)
            theta_w = np.repeat(theta[None, :], self.W, axis=0)
            theta_w[:, self.cols] = x0
        else:
            x0 = None
            theta_w = theta[None, :]
        self._pick_driver(theta_w[0], 'ensemble_run')
        if self.x is None:
            chi2 = np.asarray(vega.chi2_batch(theta_w), dtype=np.float64)
            self.x, self.lnl = x0, log_lik(self.log_norm(), chi2)
            if not np.all(np.isfinite(self.lnl)):
                raise ValueError('a start walker has a non-finite log-likelihood')
        return theta

    # ---- run
    def _segment_device(self, theta, k):
        self.vega._sync_monte_carlo()
        if self.slice is not None:      # (the single run is the set of one)
            chain, chain_lnl, st = self.vega.engine.ensemble_run_slice(
                self.cols, self.lo, self.hi, theta, self.x[None], self.lnl[None], self.accepted[None], [self.stream], self.mu,
                self.step, k, thin=self.thin, log_norm=self.log_norm(), seed=self.seed, const_hint=self.const_hint,
                chunk=self.chunk, lanes=self.lanes, mu0=self.slice['mu0'], **self._slice_arg(), **self._keep_arg())
            return (None, None, st) if chain is None else (chain[0], chain_lnl[0], st)
        chain, chain_lnl, st = self.vega.engine.ensemble_run(
            self.cols, self.lo, self.hi, theta, self.x, self.lnl, self.accepted, self.step, k, thin=self.thin, a=self.a,
            log_norm=self.log_norm(), seed=self.seed, stream=self.stream, const_hint=self.const_hint, chunk=self.chunk,
            lanes=self.lanes, **self._moves_arg(), **self._keep_arg())
        return chain, chain_lnl, st

    def _python_steps(self, k, chi2):
        if self.slice is not None:
            chain, chain_lnl, st = python_steps_slice_many(
                self.x[None], self.lnl[None], self.accepted[None], self.mu, self.step, k, self.thin, self.seed, [self.stream],
                self.lo, self.hi, self.log_norm(), lambda rows_x, ens: chi2(rows_x), **self._slice_arg())
            return chain[0], chain_lnl[0], st
        return python_steps(self.x, self.lnl, self.accepted, self.step, k, self.thin, self.a, self.seed, self.stream, self.lo,
                            self.hi, self.log_norm(), lambda rows_x, h: chi2(rows_x), self.moves)

    # ---- results
    def _stack(self, parts, discard, thin, flat):
        lnl = parts is self._chain_lnl
        parts = self._recorded(lnl)
        if parts:
            arr = np.concatenate(parts)
        else:
            arr = np.empty((0, self.W) + (() if lnl else (self.n,)))
        arr = arr[int(discard)::int(thin)]
        return arr.reshape((-1,) + arr.shape[2:]) if flat else arr

    def get_chain(self, discard=0, thin=1, flat=False):
        """Recorded positions [rows, W, n] (rows = steps / thin of the sampler), ``discard`` / ``thin`` in recorded rows;
        ``flat``: [rows W, n].  With ``moves='slice'`` the rows of the steps below ``tune_steps`` - while the scale is tuned - are
        not a stationary chain: discard them."""
        return self._stack(self._chain, discard, thin, flat)

    def get_log_lik(self, discard=0, thin=1, flat=False):
        return self._stack(self._chain_lnl, discard, thin, flat)

    def get_autocorr_time(self, discard=0, thin=1, c=5):
        """Integrated autocorrelation time per parameter in recorded rows (emcee's estimator: :func:`integrated_time`)."""
        return integrated_time(self.get_chain(discard=discard, thin=thin), c=c)

    def get_derived(self, discard=0, thin=1, flat=False):
        """The derived parameters (``vega.derived_names()``: the marginalisation coefficients) of the recorded rows,
        [rows, W, m] like :meth:`get_chain` (``flat``: [rows W, m]) - a pass over the recorded rows after the run
        (:func:`derived_rows`), the same block whichever driver ran."""
        chain = self.get_chain(discard=discard, thin=thin)
        block = self._derived_of(chain.reshape(-1, self.n))
        return block if flat else block.reshape(chain.shape[:2] + (block.shape[1],))

    def write(self, path, name, derived=False, print_func=print):
        """getdist's plain-text chain of the recorded rows (:func:`write_getdist`): ``name.txt`` and ``name.paramnames``;
        ``derived``: with the derived parameters' columns and lines after the sampled ones."""
        extra = self._write_extra(derived, print_func, lambda: self.get_derived(flat=True))
        return write_getdist(path, name, self.names, self.get_chain(flat=True), self.get_log_lik(flat=True), **extra)


# ------------------------------------------------------------------ many ensembles in one run
class EnsembleSet(StretchSampler):
    """E independent ensembles of W walkers each over the sampled parameters of ``vega``, advanced together: the half-steps of all
    ensembles are decided at once and their E W/2 proposal rows go through the engine as one stream of chunks (``'device'``:
    vmx_ensemble_run_many, one work-group per ensemble; ``'python'``: :func:`python_steps_many` over ``chi2_batch_device``, cut
    into the same chunks).  Ensemble e runs on the Philox stream ``streams[e]`` (default ``range(E)``) from the walkers
    ``EnsembleSampler(..., seed=seed, stream=streams[e])`` draws, and is the chain that sampler makes - up to the last bits of lnL
    where the engine's batches are shaped differently.  ``mock_rows`` [E]: the row of the installed mock
    pools every ensemble is compared with - a posterior per Monte-Carlo mock (:meth:`vega_amd.montecarlo.MonteCarlo.sample_mocks`);
    None: every ensemble reads the data the interface has installed - replicas of one run.  An engine group takes ``'python'``.
    ``moves``, ``gamma0``, ``sigma``, ``gamma_s``, ``cov_scale``: the mixture of moves of every ensemble, as for
    :class:`EnsembleSampler` (with ``'cov'``, ``cov_fallbacks`` [E] counts every ensemble's factor fallbacks);
    ``moves='slice'`` with ``mu`` / ``tune_steps``: ensemble slice sampling, every ensemble with a scale of its own
    (vmx_ensemble_run_slice: the ensembles' requests of a round packed behind each other)."""

    def __init__(self, vega, ensembles, walkers, streams=None, mock_rows=None, a=2.0, seed=0, thin=1, driver='device', segment=1000,
                 sample_params=None, chunk=0, lanes=0, const_hint=-1, moves=None, gamma0=None, sigma=None, gamma_s=None, mu=None,
                 tune_steps=None, cov_scale=None, chain='host'):
        self._setup_walkers(vega, walkers, a, seed, thin, driver, segment, sample_params, chunk, lanes, const_hint, moves, gamma0,
                            sigma, gamma_s, mu, tune_steps, cov_scale, chain)
        self.E = int(ensembles)
        if self.E < 1:
            raise ValueError('ensembles: at least one')
        self._lead = (self.E,)
        self.streams = np.arange(self.E, dtype=np.uint64) if streams is None else np.array(streams, dtype=np.uint64)
        self.mock_rows = None if mock_rows is None else np.array(mock_rows, dtype=np.int32)
        if self.streams.shape != (self.E,) or (self.mock_rows is not None and self.mock_rows.shape != (self.E,)):
            raise ValueError(f'streams, mock_rows: one entry for each of the {self.E} ensembles')
        if self.mock_rows is not None and np.any(self.mock_rows < 0):
            raise ValueError('mock_rows: rows of the installed mock pools, none negative')
        self.reset()

    def reset(self):
        super().reset()
        self.per_ensemble = np.zeros((self.E, 3), dtype=np.int64)

    # ---- start
    def _member_settings(self, e):
        """An :class:`EnsembleSampler` with the settings of ensemble e (no state): what draws its start and reads its results."""
        return EnsembleSampler(self.vega, self.W, a=self.a, seed=self.seed, thin=self.thin, driver=self.driver_asked,
                               segment=self.segment, sample_params=dict(limits=dict(zip(self.names, zip(self.lo, self.hi))),
                                                                         values=self.values, errors=self.errors),
                               stream=int(self.streams[e]), chunk=self.chunk, lanes=self.lanes, const_hint=self.const_hint,
                               **self._moves_kw)

    def _start_positions(self, start, init_scale):
        """The starts of ``run``'s first call: ``'ball'``, ``'prior'`` - ensemble e as ``EnsembleSampler(seed, stream=streams[e])``
        draws them - or an array [E, W, n]."""
        if not isinstance(start, str):
            start = np.array(start, dtype=np.float64)
            if start.shape != (self.E, self.W, self.n):
                raise ValueError(f'start: an array [{self.E}, {self.W}, {self.n}], "ball" or "prior"')
        return np.stack([self._member_settings(e)._start_positions(start if isinstance(start, str) else start[e], init_scale)
                         for e in range(self.E)])

    def _start_chi2(self, theta_w):
        """chi2 of the start walkers [E, W, n_params]: ensemble by ensemble through the host entry, as a single sampler evaluates
        its start - against the ensemble's own mock when the set has mock rows."""
        vega, eng = self.vega, self.vega.engine
        if self.mock_rows is None:
            return np.stack([np.asarray(vega.chi2_batch(theta_w[e]), dtype=np.float64) for e in range(self.E)])
        try:
            out = []
            for e in range(self.E):
                vega._sync_monte_carlo()
                eng.set_mock_index(np.full(min(self.W, eng.max_batch), self.mock_rows[e], dtype=np.int32))
                out.append(np.asarray(vega.chi2_batch(theta_w[e]), dtype=np.float64))
        finally:
            eng.set_mock_index(None)
        return np.stack(out)

    def _prepare(self, start, init_scale):
        theta = self._fixed_row()
        if self.x is None:
            x0 = self._start_positions(start, init_scale)
            theta_w = np.tile(theta, (self.E, self.W, 1))
            theta_w[:, :, self.cols] = x0
            first = theta_w[0, 0]
        else:
            x0, first = None, theta
        self._pick_driver(first, 'ensemble_run_many')
        if self.x is None:
            self.x, self.lnl = x0, log_lik(self.log_norm(), self._start_chi2(theta_w))
            if not np.all(np.isfinite(self.lnl)):
                raise ValueError('a start walker has a non-finite log-likelihood')
        return theta

    # ---- run
    def _segment_device(self, theta, k):
        self.vega._sync_monte_carlo()
        if self.slice is not None:
            chain, chain_lnl, st = self.vega.engine.ensemble_run_slice(
                self.cols, self.lo, self.hi, theta, self.x, self.lnl, self.accepted, self.streams, self.mu, self.step, k,
                mock_rows=self.mock_rows, thin=self.thin, log_norm=self.log_norm(), seed=self.seed, const_hint=self.const_hint,
                chunk=self.chunk, lanes=self.lanes, mu0=self.slice['mu0'], **self._slice_arg(), **self._keep_arg())
            return chain, chain_lnl, st, self._slice_per(st)
        chain, chain_lnl, st = self.vega.engine.ensemble_run_many(
            self.cols, self.lo, self.hi, theta, self.x, self.lnl, self.accepted, self.streams, self.step, k,
            mock_rows=self.mock_rows, thin=self.thin, a=self.a, log_norm=self.log_norm(), seed=self.seed,
            const_hint=self.const_hint, chunk=self.chunk, lanes=self.lanes, **self._moves_arg(), **self._keep_arg())
        return chain, chain_lnl, st, st.pop('per_ensemble')

    @staticmethod
    def _slice_per(st):
        """``per_ensemble`` [E, 3] of a slice segment: moved; nothing is rejected."""
        per = np.zeros((st['slice_counts'].shape[0], 3), dtype=np.int64)
        per[:, 0] = st['slice_counts'][:, SC_MOVED]
        return per

    def _python_steps(self, k, chi2):
        if self.slice is not None:
            mocks = self.mock_rows
            chain, chain_lnl, st = python_steps_slice_many(
                self.x, self.lnl, self.accepted, self.mu, self.step, k, self.thin, self.seed, self.streams, self.lo, self.hi,
                self.log_norm(), lambda rows_x, ens: chi2(rows_x, None if mocks is None else mocks[ens]), **self._slice_arg())
            return chain, chain_lnl, st, self._slice_per(st)
        row_mock = None if self.mock_rows is None else np.repeat(self.mock_rows, self.W // 2)
        return python_steps_many(self.x, self.lnl, self.accepted, self.step, k, self.thin, self.a, self.seed, self.streams, self.lo,
                                 self.hi, self.log_norm(), lambda rows_x, h: chi2(rows_x, row_mock), self.moves)

    # ---- results
    def _stack(self, parts, tail, discard, thin, flat):
        parts = self._recorded(lnl=parts is self._chain_lnl)
        arr = np.concatenate(parts, axis=1) if parts else np.empty((self.E, 0, self.W) + tail)
        arr = arr[:, int(discard)::int(thin)]
        return arr.reshape((self.E, -1) + arr.shape[3:]) if flat else arr

    def get_chain(self, discard=0, thin=1, flat=False):
        """Recorded positions [E, rows, W, n] (rows = steps / thin of the set), ``discard`` / ``thin`` in recorded rows; ``flat``:
        [E, rows W, n].  With ``moves='slice'`` the rows of the steps below ``tune_steps`` - while the scale is tuned - are not a
        stationary chain: discard them."""
        return self._stack(self._chain, (self.n,), discard, thin, flat)

    def get_log_lik(self, discard=0, thin=1, flat=False):
        return self._stack(self._chain_lnl, (), discard, thin, flat)

    def get_autocorr_time(self, discard=0, thin=1, c=5):
        """Integrated autocorrelation time per ensemble and parameter in recorded rows, [E, n] (:func:`integrated_time`)."""
        chain = self.get_chain(discard=discard, thin=thin)
        return np.array([integrated_time(chain[e], c=c) for e in range(self.E)])

    def member(self, e):
        """Ensemble ``e`` as a sampler that has run: :class:`EnsembleSampler`'s result methods (``get_chain``, ``get_log_lik``,
        ``acceptance_fraction``, ``get_autocorr_time``, ``get_derived``, ``write``) over copies of its part of the set's state.
        Read-only: it cannot be advanced."""
        if not 0 <= int(e) < self.E:
            raise IndexError(f'member: 0 .. {self.E - 1}')
        e = int(e)
        m = self._member_settings(e)
        m.driver = self.driver
        m.run = m.reset = _read_only
        if self.x is not None:
            m.x, m.lnl = self.x[e].copy(), self.lnl[e].copy()
        m.accepted, m.step = self.accepted[e].copy(), self.step
        m._chain[:] = [part[e] for part in self._recorded()]
        m._chain_lnl[:] = [part[e] for part in self._recorded(lnl=True)]
        took, out, bad = (int(v) for v in self.per_ensemble[e])
        m.stats = dict(self.stats, proposals=self.step * self.W, accepted=took, rejected_outside_box=out, rejected_failed_model=bad)
        if self.moves is not None:
            m._start = None if self._start is None else (self._start[0][e].copy(), self._start[1][e].copy())
            m.stats['moves'] = MoveCounts(m)
        if has_cov(self.moves):
            m.cov_fallbacks = self.cov_fallbacks[e:e + 1].copy()
            m.stats['cov'] = dict(scale=self.moves['cov_scale'], factor_fallbacks=int(m.cov_fallbacks[0]))
        if self.slice is not None:
            m.mu, m.slice_counts = self.mu[e:e + 1].copy(), self.slice_counts[e:e + 1].copy()
            m.stats['proposals'] = int(m.slice_counts[0, SC_UPDATES])
            m._slice_took()
        return m


def _read_only(*args, **kwargs):
    raise RuntimeError('a member of an EnsembleSet is read-only: advance the set')


# ------------------------------------------------------------------ parallel tempering: ladders of ensembles, and the evidence
def _ends_at_zero(betas):
    if not (len(betas) >= 2 and betas[-1] == 0.0):
        raise ValueError('the evidence needs a ladder whose last beta is 0 (the rung that samples the box)')


def stepping_stone_evidence(betas, lnl):
    """The stepping-stone estimator (Xie et al. 2011) of log Z over a uniform prior on the box: log Z = sum over t >= 1 of
    log <exp((beta[t-1] - beta[t]) lnL)> over the rows of rung t, each mean with a max-shift.  ``lnl`` [T, rows, W]: the
    untempered lnL records of the rungs.  Returns (log Z, err): per rung the variance of the ratio over an effective sample size
    N / tau, tau the :func:`integrated_time` of the ratio's walker series (at least 1), the rungs added in quadrature.  Raises
    ValueError unless the last beta is 0."""
    betas = np.asarray(betas, dtype=np.float64)
    _ends_at_zero(betas)
    lnl = np.asarray(lnl, dtype=np.float64)
    if lnl.ndim != 3 or lnl.shape[0] != betas.size or lnl.shape[1] < 2:
        raise ValueError('lnl [T, rows, W] with at least two rows')
    log_z, var = 0.0, 0.0
    for t in range(1, betas.size):
        e = (betas[t - 1] - betas[t]) * lnl[t]
        top = e.max()
        ratio = np.exp(e - top)
        mean = ratio.mean()
        log_z += top + math.log(mean)
        tau = max(1.0, float(integrated_time(ratio)[0])) if np.ptp(ratio) > 0.0 else 1.0
        var += ratio.var(ddof=1) / mean**2 * tau / ratio.size
    return float(log_z), math.sqrt(var)


def _trapezoid(b, y):
    # (the ladder descends: the integral from beta = 0 up to 1)
    return float(-np.sum(np.diff(b) * 0.5 * (y[1:] + y[:-1])))


def thermodynamic_integration(betas, mean_lnl):
    """Thermodynamic integration: log Z = the integral of <lnL>_beta from 0 to 1 by the trapezoid rule over the ladder,
    ``mean_lnl`` [T] the rungs' means.  Returns (log Z, err) with ptemcee's error: the difference to the same rule on every
    second rung (rungs 0, 2, 4, ... and the last one) - the discretisation, not the sampling noise.  Raises ValueError unless the
    last beta is 0."""
    betas = np.asarray(betas, dtype=np.float64)
    _ends_at_zero(betas)
    y = np.asarray(mean_lnl, dtype=np.float64)
    if y.shape != betas.shape:
        raise ValueError('mean_lnl [T]')
    keep = np.unique(np.append(np.arange(0, betas.size, 2), betas.size - 1))
    log_z = _trapezoid(betas, y)
    return log_z, abs(log_z - _trapezoid(betas[keep], y[keep]))


class TemperedEnsemble(EnsembleSet):
    """Parallel tempering (ptemcee's answer to separated modes, and an evidence): ``ladders`` = G temperature ladders of T rungs
    each, a rung an ensemble of ``walkers`` walkers that decides at its beta (``betas`` [T]: 1 > ... >= 0, or ``ntemps`` = T with
    ``beta_min``: :func:`default_ladder`), with a swap sweep between adjacent rungs after every ``swap_every``-th step (0: none).
    An :class:`EnsembleSet` of G T ensembles - ladder g owns g T .. g T + T - 1, rung 0 the cold one - advanced in one device run
    (``'device'``: vmx_ensemble_run_pt; ``'python'``: :func:`python_steps_pt`, the same chain bit for bit).  ``streams`` [G]
    (default ``range(G)``): ladder stream sigma puts rung t on the Philox stream 64 sigma + t; [G, T]: every rung's own.
    ``mock_rows`` [G]: the mock every ladder is compared with.  The other arguments are :class:`EnsembleSet`'s.  With swaps a
    walker's recorded position also changes when it is exchanged, so ``stats['moves']`` is not kept.

    ``get_chain`` / ``get_log_lik`` read one rung (default the cold one, which ``write`` puts into the getdist chain);
    ``swap_fraction`` [G, T - 1] is the accepted fraction of the swaps between rungs t and t + 1; ``log_evidence`` is the
    stepping-stone or thermodynamic-integration evidence over the box, with the ``log_norm`` of the other samplers.

    ``adapt=True`` (ptemcee's adaptive ladder, Vousden et al. 2016; T >= 3 and swaps required): every ladder starts from ``betas``
    and moves its intermediate betas after every swap sweep so that all pairs of rungs come to swap at the same rate
    (:func:`ladder_adjust` with ptemcee's ``adaptation_lag`` and ``adaptation_time``, in sweeps), on the device
    (vmx_ensemble_run_pt_adapt) or in :func:`python_steps_pt_adapt`, the same chain bit for bit.  The sweeps after the global
    steps below ``adapt_steps`` adapt (None: all of them, as in ptemcee); ``run`` cuts its calls there, and the chain does not
    depend on any cut.  ``current_betas`` [G, T] are the ladders as they stand (a fixed run tiles its ladder), ``beta_history``
    [sweeps, G, T] the ladders after every adapting sweep, ``stats['adapt_skipped']`` [G] the sweeps whose new ladder was dropped
    because it was not in order, ``frozen_swap_fraction`` [G, T - 1] the swap fractions of the sweeps after the ladder froze.  The
    evidence of an adaptive run reads only the rows recorded after ``adapt_steps``, with the ladder's final betas."""

    def __init__(self, vega, walkers, ntemps=None, betas=None, swap_every=1, ladders=1, streams=None, mock_rows=None, beta_min=None,
                 a=2.0, seed=0, thin=1, driver='device', segment=1000, sample_params=None, chunk=0, lanes=0, const_hint=-1,
                 moves=None, gamma0=None, sigma=None, gamma_s=None, adapt=False, adapt_steps=None, adaptation_lag=10000,
                 adaptation_time=100, chain='host'):
        if chain != 'host':
            raise ValueError("chain: a temperature ladder keeps its rows on the host (chain='host'); the store is for the untempered runs")
        if _names_slice(moves):
            raise ValueError("moves: 'slice' does not combine with parallel tempering (ntemps / betas)")
        if names_cov(moves):
            raise ValueError("moves: 'cov' does not combine with parallel tempering (ntemps / betas) yet")
        if (ntemps is None) == (betas is None):
            raise ValueError('ntemps or betas: one of the two')
        if betas is None:
            self.betas = default_ladder(ntemps, beta_min)
        else:
            if beta_min is not None:
                raise ValueError('beta_min belongs to ntemps: betas are given')
            self.betas = np.array(betas, dtype=np.float64)
            if not ladder_ok(self.betas):
                raise ValueError(f'betas: from 1, strictly decreasing, none negative, at most {PT_MAXT}')
        self.T, self.G = int(self.betas.size), int(ladders)
        self.swap_every = int(swap_every)
        if self.G < 1 or self.swap_every < 0:
            raise ValueError('ladders: at least one; swap_every: 0 (no swaps) or more')
        self.adapt = bool(adapt)
        self.adapt_steps = None if adapt_steps is None else int(adapt_steps)
        self.adaptation_lag, self.adaptation_time = float(adaptation_lag), float(adaptation_time)
        if self.adapt and not adapt_ok(self.T, self.swap_every, self.adaptation_lag, self.adaptation_time):
            raise ValueError('adapt: at least 3 rungs, swap_every >= 1, adaptation_lag and adaptation_time finite and positive')
        if self.adapt and self.adapt_steps is not None and self.adapt_steps < 0:
            raise ValueError('adapt_steps: 0 or more steps, or None (adapt to the end)')
        if streams is None:
            streams = np.arange(self.G)
        streams = np.array(streams, dtype=np.uint64)
        if streams.shape == (self.G,):
            streams = np.uint64(64) * streams[:, None] + np.arange(self.T, dtype=np.uint64)[None, :]
        if streams.shape != (self.G, self.T):
            raise ValueError(f'streams: one for each of the {self.G} ladders, or [{self.G}, {self.T}]')
        self.ladder_mock_rows = None if mock_rows is None else np.array(mock_rows, dtype=np.int32)
        if self.ladder_mock_rows is not None and self.ladder_mock_rows.shape != (self.G,):
            raise ValueError(f'mock_rows: one entry for each of the {self.G} ladders')
        super().__init__(vega, self.G * self.T, walkers, streams=streams.reshape(-1),
                         mock_rows=None if mock_rows is None else np.repeat(self.ladder_mock_rows, self.T), a=a, seed=seed, thin=thin,
                         driver=driver, segment=segment, sample_params=sample_params, chunk=chunk, lanes=lanes, const_hint=const_hint,
                         moves=moves, gamma0=gamma0, sigma=sigma, gamma_s=gamma_s)

    def reset(self):
        super().reset()
        self.swaps = np.zeros((self.G, self.T - 1, 2), dtype=np.int64)
        self.stats.update(swaps_proposed=0, swaps_accepted=0)
        if self.swap_every > 0:
            self.stats.pop('moves', None)
        self.current_betas = np.tile(self.betas, (self.G, 1))
        self._frozen_swaps = np.zeros((self.G, self.T - 1, 2), dtype=np.int64)
        self._beta_hist = []
        if self.adapt:
            self.stats['adapt_skipped'] = np.zeros(self.G, dtype=np.int64)

    def _prepare(self, start, init_scale):
        theta = super()._prepare(start, init_scale)
        entry = 'ensemble_run_pt_adapt' if self.adapt else 'ensemble_run_pt'
        if self.driver == 'device' and not hasattr(self.vega.engine, entry):
            self.driver = 'python'
        return theta

    def run(self, n_steps, start='ball', init_scale=1.0):
        """:meth:`StretchSampler.run`; an adaptive run cuts its calls at ``adapt_steps``, so that every call is all adapting or all
        frozen."""
        if self.adapt and self.adapt_steps is not None and self.step < self.adapt_steps < self.step + n_steps:
            first = self.adapt_steps - self.step
            super().run(first, start=start, init_scale=init_scale)
            return super().run(n_steps - first)
        return super().run(n_steps, start=start, init_scale=init_scale)

    # ---- run
    def _shaped(self):
        lead = (self.G, self.T, self.W)
        return self.x.reshape(lead + (self.n,)), self.lnl.reshape(lead), self.accepted.reshape(lead)

    def _adapting(self):
        """Whether the call that starts at the current step adapts (``run`` cuts the calls at ``adapt_steps``)."""
        return self.adapt and (self.adapt_steps is None or self.step < self.adapt_steps)

    def _adapt_arg(self):
        return dict(adaptation_lag=self.adaptation_lag, adaptation_time=self.adaptation_time,
                    adapt_until=-1 if self.adapt_steps is None else self.adapt_steps)

    def _took(self, chain, chain_lnl, st, per, swaps, betas=None, hist=None, skipped=None):
        self.swaps += swaps
        if self._adapting():
            self._beta_hist.append(hist)
            self.stats['adapt_skipped'] += skipped
        else:
            self._frozen_swaps += swaps
        st = dict(st, swaps_proposed=int(swaps[:, :, 0].sum()), swaps_accepted=int(swaps[:, :, 1].sum()))
        return chain.reshape((self.E,) + chain.shape[2:]), chain_lnl.reshape((self.E,) + chain_lnl.shape[2:]), st, per.reshape(self.E, 3)

    def _segment_device(self, theta, k):
        self.vega._sync_monte_carlo()
        x, lnl, accepted = self._shaped()
        if self.adapt:
            chain, chain_lnl, st = self.vega.engine.ensemble_run_pt_adapt(
                self.cols, self.lo, self.hi, theta, x, lnl, accepted, self.current_betas, self.streams.reshape(self.G, self.T),
                self.step, k, swap_every=self.swap_every, mock_rows=self.ladder_mock_rows, thin=self.thin, a=self.a,
                log_norm=self.log_norm(), seed=self.seed, const_hint=self.const_hint, chunk=self.chunk, lanes=self.lanes,
                **self._adapt_arg(), **self._moves_arg())
            return self._took(chain, chain_lnl, st, st.pop('per_ensemble'), st.pop('swaps'), self.current_betas, st.pop('beta_hist'),
                              st.pop('adapt_skipped'))
        chain, chain_lnl, st = self.vega.engine.ensemble_run_pt(
            self.cols, self.lo, self.hi, theta, x, lnl, accepted, self.betas, self.streams.reshape(self.G, self.T), self.step, k,
            swap_every=self.swap_every, mock_rows=self.ladder_mock_rows, thin=self.thin, a=self.a, log_norm=self.log_norm(),
            seed=self.seed, const_hint=self.const_hint, chunk=self.chunk, lanes=self.lanes, **self._moves_arg())
        return self._took(chain, chain_lnl, st, st.pop('per_ensemble'), st.pop('swaps'))

    def _python_steps(self, k, chi2):
        row_mock = None if self.mock_rows is None else np.repeat(self.mock_rows, self.W // 2)
        x, lnl, accepted = self._shaped()
        if self.adapt:
            return self._took(*python_steps_pt_adapt(
                x, lnl, accepted, self.step, k, self.thin, self.swap_every, self.a, self.seed, self.current_betas,
                self.streams.reshape(self.G, self.T), self.lo, self.hi, self.log_norm(), lambda rows_x, h: chi2(rows_x, row_mock),
                self.moves, **self._adapt_arg()))
        return self._took(*python_steps_pt(x, lnl, accepted, self.step, k, self.thin, self.swap_every, self.a, self.seed, self.betas,
                                           self.streams.reshape(self.G, self.T), self.lo, self.hi, self.log_norm(),
                                           lambda rows_x, h: chi2(rows_x, row_mock), self.moves))

    # ---- results
    def _index(self, rung, ladder):
        if not (0 <= int(rung) < self.T and 0 <= int(ladder) < self.G):
            raise IndexError(f'rung 0 .. {self.T - 1} of ladder 0 .. {self.G - 1}')
        return int(ladder) * self.T + int(rung)

    def _rungs(self, arr, rung, ladder):
        if rung is None:
            arr = arr.reshape((self.G, self.T) + arr.shape[1:])
            return arr
        return arr[self._index(rung, ladder)]

    def get_chain(self, discard=0, thin=1, flat=False, *, rung=0, ladder=0):
        """Recorded positions of rung ``rung`` (0: the cold one) of ladder ``ladder``, [rows, W, n] (``flat``: [rows W, n]);
        ``rung=None``: of every rung, [G, T, rows, W, n]."""
        return self._rungs(super().get_chain(discard=discard, thin=thin, flat=flat), rung, ladder)

    def get_log_lik(self, discard=0, thin=1, flat=False, *, rung=0, ladder=0):
        """The untempered lnL of :meth:`get_chain`'s rows."""
        return self._rungs(super().get_log_lik(discard=discard, thin=thin, flat=flat), rung, ladder)

    def get_autocorr_time(self, discard=0, thin=1, c=5, *, rung=0, ladder=0):
        return integrated_time(self.get_chain(discard=discard, thin=thin, rung=rung, ladder=ladder), c=c)

    def rung(self, t, ladder=0):
        """Rung ``t`` of ladder ``ladder`` as a sampler that has run, read-only like :meth:`EnsembleSet.member`."""
        m = self.member(self._index(t, ladder))
        if self.swap_every > 0:
            m.stats.pop('moves', None)
        m.beta = float(self.current_betas[int(ladder), int(t)])
        return m

    @property
    def recorded_rows(self):
        return sum(part.shape[1] for part in self._chain_lnl)

    def run_until(self, *args, **kwargs):
        raise ValueError('run_until: the convergence stop is for the untempered runs; a temperature ladder runs its steps')

    def summary(self, *args, **kwargs):
        raise ValueError('summary: per rung, chain_summary(run.get_chain(rung=...))')

    def quantiles(self, *args, **kwargs):
        raise ValueError('quantiles: per rung, chain_quantiles(run.get_chain(rung=...), q)')

    def best(self, *args, **kwargs):
        raise ValueError('best: per rung, chain_best(run.get_chain(rung=...), run.get_log_lik(rung=...))')

    @property
    def swap_fraction(self):
        """The accepted fraction of the swaps proposed between the rungs t and t + 1, [G, T - 1] (nan before the first sweep)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.swaps[:, :, 1] / self.swaps[:, :, 0]

    @property
    def beta_history(self):
        """The ladders after every adapting sweep so far, [sweeps, G, T] (a fixed run: no row)."""
        return np.concatenate(self._beta_hist + [np.empty((0, self.G, self.T))])

    @property
    def frozen_swap_fraction(self):
        """:attr:`swap_fraction` over the sweeps after the ladder froze alone, [G, T - 1] (a fixed ladder: all sweeps; nan where
        there was none)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return self._frozen_swaps[:, :, 1] / self._frozen_swaps[:, :, 0]

    @property
    def frozen_rows(self):
        """(the first recorded row after the ladder last moved, the number of such rows): (0, all rows) for a fixed ladder; the
        rows of the steps from ``adapt_steps`` on for an adaptive one - none while it adapts."""
        rows = self.recorded_rows
        if not self.adapt:
            return 0, rows
        first = rows if self.adapt_steps is None else min(rows, self.adapt_steps // self.thin)
        return first, rows - first

    def log_evidence(self, method='ss', discard=None, ladder=0):
        """(log Z, err) over the uniform prior on the box, from the rungs' lnL records past the first ``discard`` recorded rows
        (None: a quarter of them): ``'ss'`` - :func:`stepping_stone_evidence` - or ``'ti'`` - :func:`thermodynamic_integration`.
        ValueError unless the ladder ends at beta = 0.  Both need one beta per rung: an adaptive run reads only the rows recorded
        after the ladder last moved (:attr:`frozen_rows`; ``discard`` counts from the first of them), with the ladder's final
        betas, and raises ValueError while fewer than two such rows exist - always with ``adapt_steps=None``."""
        _ends_at_zero(self.betas)
        first, rows = self.frozen_rows
        if self.adapt and rows < 2:
            raise ValueError('the evidence of an adaptive ladder needs at least two rows recorded after the ladder froze: set '
                             'adapt_steps below the number of steps' + (' (adapt_steps=None adapts to the end)'
                                                                        if self.adapt_steps is None else ''))
        betas = self.current_betas[int(ladder)]
        discard = rows // 4 if discard is None else int(discard)
        lnl = self.get_log_lik(discard=first + discard, rung=None)[int(ladder)]
        if method == 'ss':
            return stepping_stone_evidence(betas, lnl)
        if method == 'ti':
            return thermodynamic_integration(betas, lnl.mean(axis=(1, 2)))
        raise ValueError("method: 'ss' (stepping stones) or 'ti' (thermodynamic integration)")

    def write(self, path, name, derived=False, print_func=print):
        """getdist's plain-text chain of the cold rung - ``name.txt`` and ``name.paramnames`` (``name_ladder<g>`` with several
        ladders) - and, with a ladder that ends at beta = 0 and at least two recorded rows, ``name.stats`` with the evidence, as the
        nested and SMC runs write it."""
        out = []
        for g in range(self.G):
            nm = name if self.G == 1 else f'{name}_ladder{g}'
            files = tuple(self.rung(0, g).write(path, nm, derived=derived, print_func=print_func))
            if self.betas[-1] == 0.0 and self.T >= 2 and self.frozen_rows[1] >= 2:
                files += (write_pt_stats(self, path, nm, g),)
            elif self.betas[-1] == 0.0 and g == 0:
                print_func('fewer than two recorded rows' + (' after the ladder froze' if self.adapt else '') +
                           ': no evidence, no ' + f'{nm}.stats')
            out.append(files)
        return out[0] if self.G == 1 else out


def write_pt_stats(run, path, name, ladder=0):
    """``name.stats`` of a :class:`TemperedEnsemble`'s ladder: both evidences, the ladder and its swap fractions."""
    log_z, err = run.log_evidence('ss', ladder=ladder)
    ti, ti_err = run.log_evidence('ti', ladder=ladder)
    stats = Path(path) / f'{name}.stats'
    with open(stats, 'w') as f:
        f.write(f'log(Z) = {log_z!r}\nlog(Z) error = {err!r}\n')
        f.write(f'log(Z) thermodynamic = {ti!r}\nlog(Z) thermodynamic error = {ti_err!r}\n')
        f.write(f'steps = {run.step}\nwalkers = {run.W}\nswap_every = {run.swap_every}\nseed = {run.seed}\n')
        f.write(f'likelihood evaluations = {run.step * run.W * run.T}\n')
        f.write('beta = ' + ' '.join(repr(float(b)) for b in run.current_betas[ladder]) + '\n')
        f.write('swap fraction = ' + ' '.join(repr(float(v)) for v in run.swap_fraction[ladder]) + '\n')
        if run.adapt:       # (the final ladder above; a fixed run's file is what it was)
            f.write(f'adapt_steps = {run.adapt_steps}\nadaptation_lag = {run.adaptation_lag!r}\n')
            f.write(f'adaptation_time = {run.adaptation_time!r}\nadapt skipped = {int(run.stats["adapt_skipped"][ladder])}\n')
            f.write('frozen swap fraction = ' + ' '.join(repr(float(v)) for v in run.frozen_swap_fraction[ladder]) + '\n')
    return stats


def read_pt_stats(path):
    """``name.stats`` of :func:`write_pt_stats` back as a dict (floats for the evidence lines, lists of floats for ``beta`` and
    ``swap fraction``, ints for the counts; of an adaptive run also ``adapt_steps``, ``adaptation_lag``, ``adaptation_time``,
    ``adapt skipped`` and the list ``frozen swap fraction``, ``beta`` then being the final ladder)."""
    out = {}
    for line in Path(path).read_text().splitlines():
        key, _, val = line.partition(' = ')
        if key in ('beta', 'swap fraction', 'frozen swap fraction'):
            out[key] = [float(v) for v in val.split()]
        else:
            out[key] = float(val) if key.startswith('log(Z)') or key in ('adaptation_lag', 'adaptation_time') else int(val)
    return out


# ------------------------------------------------------------------ the config switch (bin/run_vega_mpi.py for one process)
_ENSEMBLE_DEFAULTS = dict(sampler='Ensemble', name='ensemble', walkers=None, steps=1000, seed=0, a=2.0, thin=1, init='ball', init_scale=1.0,
                          driver='device')


def section_settings(main_config, sample_params, section, **defaults):
    """What the settings of every sampler's section share: the section must be there, every sampled parameter must have limits,
    ``path`` is required, expanded and must exist; ``name`` and ``driver`` over ``defaults``, ``derived`` and ``replicas`` when
    stated.  Returns (the section, the limits, the settings so far: ``defaults`` with sampler, path, name, driver)."""
    if section not in main_config:
        raise RuntimeError('run_sampler called, but no sampler config found')
    sec = main_config[section]
    limits = sample_params['limits']
    for lims in limits.values():
        if lims is None or None in tuple(lims):
            raise ValueError(_NO_LIMITS)
    if 'path' not in sec:
        raise ValueError(f'[{section}] needs a path')
    path = Path(os.path.expandvars(sec.get('path')))
    assert path.exists(), ("The sampler 'path' does not correspond to an existing folder. Create the output folder before "
                           "running.")
    out = dict(defaults, sampler=section, path=path)
    out['name'] = sec.get('name', out['name'])
    out['driver'] = sec.get('driver', 'device')
    if 'derived' in sec:
        out['derived'] = parse_derived(sec)
    if 'replicas' in sec:
        from .replicas import parse_replicas
        out['replicas'] = parse_replicas(sec)
    if out['driver'] not in ('device', 'python'):
        raise ValueError(f"[{section}] driver: 'device' or 'python'")
    return sec, limits, out


def sampler_settings(main_config, sample_params):
    """The ``[Ensemble]`` settings of a main config that asks for the sampler, checked as the reference checks its samplers
    (vega_interface.py:186-195, samplers/sampler_interface.py:43-57).  A plain function of the parsed config and the sampled
    parameters: {sampler, path, name, walkers, steps, seed, a, thin, init, init_scale, driver} and, when the section states it,
    ``moves`` with ``gamma0`` / ``de_sigma`` / ``snooker_gamma`` / ``cov_scale`` (:func:`_parse_moves`: a mixture of the stretch,
    DE, snooker and cov moves; absent: the stretch move, and no such key), ``derived`` (True | False; absent means False: the chain files are what
    they were), ``replicas`` (R >= 1 independent copies on Philox streams 0 .. R - 1, merged afterwards:
    :mod:`vega_amd.replicas`) and ``ntemps`` with ``beta_min`` / ``swap_every`` and ``adapt`` with ``adapt_steps`` / ``adaptation_lag`` / ``adaptation_time``
    (:func:`_parse_tempering`: parallel tempering, and its adaptive ladder) and ``quantiles`` (:func:`_parse_quantiles`: with
    ``mocks``, every parameter's quantiles and best point per mock, found on the device);
    with ``sampler = Nested`` the ``[Nested]`` settings instead
    (:func:`vega_amd.nested.nested_settings`), with ``sampler = SMC`` the ``[SMC]`` ones (:func:`vega_amd.smc.smc_settings`)."""
    control = main_config['control'] if 'control' in main_config else {}
    run = control.getboolean('run_sampler', False) if hasattr(control, 'getboolean') else False
    if not run:
        raise ValueError('Warning: You called the sampler without asking for it. Add "run_sampler = True" to the "[control]" '
                         'section.')
    sampler = control.get('sampler', None)
    if sampler in ('Polychord', 'PocoMC'):
        raise NotImplementedError(f'sampler = {sampler}: that library is not available here; use sampler = Nested (evidence and a '
                                  'weighted posterior) or sampler = Ensemble')
    if sampler == 'Nested':
        from .nested import nested_settings
        return nested_settings(main_config, sample_params)
    if sampler == 'SMC':
        from .smc import smc_settings
        return smc_settings(main_config, sample_params)
    if sampler != 'Ensemble':
        raise ValueError('Sampler not recognized. Please use Nested or Ensemble.')
    sec, limits, out = section_settings(main_config, sample_params, 'Ensemble', **_ENSEMBLE_DEFAULTS)
    out['walkers'] = sec.getint('walkers', max(2 * len(limits), 32) + (max(2 * len(limits), 32) % 2))
    out['steps'] = sec.getint('steps', out['steps'])
    out['seed'] = sec.getint('seed', out['seed'])
    out['a'] = sec.getfloat('a', out['a'])
    out['thin'] = sec.getint('thin', out['thin'])
    out['init'] = sec.get('init', out['init'])
    out['init_scale'] = sec.getfloat('init_scale', out['init_scale'])
    if out['init'] not in ('ball', 'prior'):
        raise ValueError("[Ensemble] init: 'ball' or 'prior'")
    if out['walkers'] % 2 or out['walkers'] < 2 * len(limits):
        raise ValueError(f'[Ensemble] walkers: an even number, at least twice the {len(limits)} sampled parameters')
    if out['steps'] < 1 or out['thin'] < 1:
        raise ValueError('[Ensemble] steps and thin must be positive')
    if not out['a'] > 1.0:
        raise ValueError('[Ensemble] a: the stretch scale must exceed 1')
    _parse_moves(sec, out, len(limits))
    if 'mocks' in sec:
        out['mocks'] = _parse_mocks(sec, main_config)
    if 'together' in sec:
        try:
            out['together'] = sec.getboolean('together')
        except ValueError:
            raise ValueError('[Ensemble] together: True or False') from None
    _parse_tempering(sec, out)
    _parse_converge(sec, out)
    _parse_quantiles(sec, out)
    return out


def _parse_quantiles(sec, out):
    """``quantiles = q0 q1 ...`` of ``[Ensemble]`` (1 .. 16 values in [0, 1], e.g. ``0.025 0.16 0.5 0.84 0.975``) into
    ``out['quantiles']``: with ``mocks = M`` the run keeps its chains on the device (``summaries='device'``) and the table
    ``mock_posteriors.fits`` gains every parameter's quantiles and best point.  Without the key nothing is added.  Refused without
    ``mocks`` (a single run's chain file is there for getdist) and with ``ntemps``."""
    if 'quantiles' not in sec:
        return
    try:
        q = [float(v) for v in sec.get('quantiles').replace(',', ' ').split()]
    except ValueError:
        raise ValueError('[Ensemble] quantiles: numbers in [0, 1]') from None
    try:
        q = check_quantiles(q) if q else check_quantiles(np.empty(0))
    except ValueError as err:
        raise ValueError(f'[Ensemble] {err}') from None
    if 'ntemps' in out:
        raise ValueError('[Ensemble] quantiles and ntemps do not combine')
    if 'mocks' not in out:
        raise ValueError('[Ensemble] quantiles go with mocks = M: a single run writes its chain for getdist')
    out['quantiles'] = [float(v) for v in q]


_CONVERGE_KEYS = ('tau_factor', 'tau_rtol', 'check_every')


def _parse_converge(sec, out):
    """``converge = True`` of ``[Ensemble]``: the run stops by its own integrated autocorrelation times
    (:meth:`StretchSampler.run_until`, ``steps`` the maximum), with ``tau_factor``, ``tau_rtol`` and ``check_every`` when stated,
    into ``out['converge']`` - a dict of the stated ones.  Without ``converge`` nothing is added.  Not combined with ``ntemps``;
    ``replicas > 1`` need ``together = True`` (the set stops as one)."""
    stated = [key for key in _CONVERGE_KEYS if key in sec]
    if 'converge' not in sec:
        if stated:
            raise ValueError(f'[Ensemble] {", ".join(stated)}: settings of the convergence stop, but no converge')
        return
    try:
        on = sec.getboolean('converge')
    except ValueError:
        raise ValueError('[Ensemble] converge: True or False') from None
    if not on:
        if stated:
            raise ValueError(f'[Ensemble] {", ".join(stated)}: settings of the convergence stop, but converge is not True')
        return
    if 'ntemps' in sec:
        raise ValueError('[Ensemble] converge and ntemps do not combine yet')
    if out.get('replicas', 1) > 1 and not out.get('together', False):
        raise ValueError('[Ensemble] converge with replicas > 1 needs together = True: the set stops as one')
    conv = {}
    try:
        for key in ('tau_factor', 'tau_rtol'):
            if key in sec:
                conv[key] = sec.getfloat(key)
        if 'check_every' in sec:
            conv['check_every'] = sec.getint('check_every')
    except ValueError:
        raise ValueError('[Ensemble] tau_factor, tau_rtol: numbers; check_every: a whole number') from None
    for key, value in conv.items():
        if not (value > 0 and np.isfinite(value)):
            raise ValueError(f'[Ensemble] {key} must be positive')
    out['converge'] = conv


def write_convergence(sampler, path, name):
    """``name.convergence`` beside the chain files: one line per check of :meth:`StretchSampler.run_until` - the step, then tau
    per sampled parameter (a set: the worst member's) - and a last line ``converged = True|False``.  Returns the path."""
    conv = sampler.convergence
    lines = ['# step ' + ' '.join(sampler.names)]
    for step, tau in zip(conv['steps'], conv['tau']):
        worst = np.max(tau.reshape(-1, tau.shape[-1]), axis=0)
        lines.append(f'{int(step)} ' + ' '.join(f'{v:.17g}' for v in worst))
    lines.append(f'converged = {bool(np.all(conv["converged"]))}')
    out = Path(path) / f'{name}.convergence'
    out.write_text('\n'.join(lines) + '\n')
    return out


def _parse_tempering(sec, out):
    """``ntemps = T`` of ``[Ensemble]`` (T >= 2 rungs: parallel tempering, :class:`TemperedEnsemble` on
    :func:`default_ladder`), with ``beta_min`` and ``swap_every`` (default 1) when stated, into the keys of the same names.
    Without ``ntemps`` nothing is added.  Not combined with ``mocks``, ``together`` or ``replicas > 1``.  ``adapt = True``: the
    adaptive ladder of :class:`TemperedEnsemble` (``ntemps >= 3``, ``swap_every >= 1``), with ``adapt_steps`` (default
    ``steps // 2``, so that rows remain for the evidence) and, when stated, ``adaptation_lag`` and ``adaptation_time``; these keys
    too are added only when the section states ``adapt``."""
    if 'ntemps' in sec and out.get('moves') == 'slice':
        raise ValueError('[Ensemble] moves = slice does not combine with ntemps (parallel tempering)')
    if 'ntemps' in sec and out.get('moves') != 'slice' and names_cov(out.get('moves')):
        raise ValueError("[Ensemble] moves: 'cov' does not combine with ntemps (parallel tempering) yet")
    if 'ntemps' not in sec:
        stray = [key for key in ('beta_min', 'swap_every') + _ADAPT_KEYS if key in sec]
        if stray:
            raise ValueError(f'[Ensemble] {", ".join(stray)}: settings of a temperature ladder, but no ntemps')
        return
    try:
        out['ntemps'] = sec.getint('ntemps')
        if 'beta_min' in sec:
            out['beta_min'] = sec.getfloat('beta_min')
        out['swap_every'] = sec.getint('swap_every', 1)
    except ValueError:
        raise ValueError('[Ensemble] ntemps, swap_every: whole numbers; beta_min: a number') from None
    try:
        default_ladder(out['ntemps'], out.get('beta_min'))
    except ValueError as err:
        raise ValueError(f'[Ensemble] {err}') from None
    if out['swap_every'] < 0:
        raise ValueError('[Ensemble] swap_every: 0 (no swaps) or more')
    if out['steps'] // out['thin'] < 2:
        raise ValueError('[Ensemble] ntemps: the evidence needs at least two recorded rows, steps // thin >= 2')
    for key in ('mocks', 'together'):
        if key in out:
            raise ValueError(f'[Ensemble] ntemps and {key} do not combine yet')
    if out.get('replicas', 1) > 1:
        raise ValueError('[Ensemble] ntemps and replicas > 1 do not combine yet')
    _parse_adapt(sec, out)


_ADAPT_KEYS = ('adapt', 'adapt_steps', 'adaptation_lag', 'adaptation_time')


def _parse_adapt(sec, out):
    """The adaptive-ladder keys of a section that has ``ntemps`` (:func:`_parse_tempering`)."""
    stated = [key for key in _ADAPT_KEYS if key in sec]
    if not stated:
        return
    try:
        adapt = sec.getboolean('adapt', False)
    except ValueError:
        raise ValueError('[Ensemble] adapt: True or False') from None
    if not adapt:
        stray = [key for key in stated if key != 'adapt']
        if stray:
            raise ValueError(f'[Ensemble] {", ".join(stray)}: settings of an adaptive ladder, but adapt is not True')
        out['adapt'] = False
        return
    out['adapt'] = True
    try:
        out['adapt_steps'] = sec.getint('adapt_steps', out['steps'] // 2)
        for key in ('adaptation_lag', 'adaptation_time'):
            if key in sec:
                out[key] = sec.getfloat(key)
    except ValueError:
        raise ValueError('[Ensemble] adapt_steps: a whole number; adaptation_lag, adaptation_time: numbers') from None
    if out['ntemps'] < 3 or out['swap_every'] == 0:
        raise ValueError('[Ensemble] adapt: an adaptive ladder needs ntemps >= 3 and swap_every >= 1')
    if not adapt_ok(out['ntemps'], out['swap_every'], out.get('adaptation_lag', 1.0), out.get('adaptation_time', 1.0)):
        raise ValueError('[Ensemble] adaptation_lag, adaptation_time: finite and positive')
    if not 0 <= out['adapt_steps'] <= out['steps']:
        raise ValueError(f'[Ensemble] adapt_steps: 0 .. steps = {out["steps"]}')
    if out['steps'] // out['thin'] - out['adapt_steps'] // out['thin'] < 2:
        raise ValueError('[Ensemble] adapt_steps: the evidence needs at least two rows recorded after the ladder froze, '
                         'steps // thin - adapt_steps // thin >= 2')


_MOVE_KEYS = (('gamma0', 'gamma0'), ('de_sigma', 'sigma'), ('snooker_gamma', 'gamma_s'), ('cov_scale', 'cov_scale'))


def _parse_moves(sec, out, n):
    """``moves = de 0.8 snooker 0.2`` of ``[Ensemble]``: move names (stretch, de, snooker, cov), each with its weight after it - a
    bare name weighs 1, so that ``moves = de`` is the pure move - into ``out['moves']`` as a list of (name, weight); ``gamma0``,
    ``de_sigma``, ``snooker_gamma`` and ``cov_scale`` into the keys of the same names when stated.  Without ``moves`` nothing is added.  The
    mixture is checked against the walkers as :func:`resolve_moves` checks it."""
    scales = {}
    for key, _ in _MOVE_KEYS:
        if key in sec:
            try:
                scales[key] = sec.getfloat(key)
            except ValueError:
                raise ValueError(f'[Ensemble] {key}: a number') from None
    tokens = sec.get('moves', '').replace(',', ' ').split()
    slice_keys = [key for key, _ in _SLICE_KEYS if key in sec]
    if 'slice' in tokens:
        _parse_slice(sec, out, tokens, scales)
        return
    if slice_keys:
        raise ValueError(f'[Ensemble] {", ".join(slice_keys)}: settings of ensemble slice sampling, but moves is not slice')
    if 'moves' not in sec:
        if scales:
            raise ValueError(f'[Ensemble] {", ".join(scales)}: the scales of moves, but no moves are named')
        return
    pairs = []
    for tok in sec.get('moves').replace(',', ' ').split():
        try:
            w = float(tok)
        except ValueError:
            if tok not in COV_MOVE_NAMES:
                raise ValueError(f"[Ensemble] moves: unknown move {tok!r}; one of 'stretch', 'de', 'snooker', 'cov'") from None
            pairs.append([tok, None])
            continue
        if not pairs or pairs[-1][1] is not None:
            raise ValueError('[Ensemble] moves: a weight follows the name of its move')
        pairs[-1][1] = w
    if not pairs:
        raise ValueError('[Ensemble] moves: name at least one move')
    out['moves'] = [(name, 1.0 if w is None else w) for name, w in pairs]
    out.update(scales)
    try:
        resolve_moves(**moves_arguments(out), n=n, walkers=out['walkers'])
    except ValueError as err:
        raise ValueError(f'[Ensemble] {err}') from None


_SLICE_KEYS = (('slice_mu', 'mu'), ('slice_tune_steps', 'tune_steps'))


def _parse_slice(sec, out, tokens, scales):
    """``moves = slice`` of ``[Ensemble]``: ensemble slice sampling, ``out['moves'] = 'slice'``; ``slice_mu`` and
    ``slice_tune_steps`` into the keys of the same names when stated."""
    if tokens != ['slice']:
        raise ValueError("[Ensemble] moves: 'slice' is a sampler of its own, not a member of a mixture: moves = slice")
    if scales:
        raise ValueError(f'[Ensemble] {", ".join(scales)}: scales of the stretch / DE / snooker moves, not of slice')
    out['moves'] = 'slice'
    try:
        if 'slice_mu' in sec:
            out['slice_mu'] = sec.getfloat('slice_mu')
        if 'slice_tune_steps' in sec:
            out['slice_tune_steps'] = sec.getint('slice_tune_steps')
    except ValueError:
        raise ValueError('[Ensemble] slice_mu: a number; slice_tune_steps: a whole number') from None
    try:
        resolve_slice(**moves_arguments(out), walkers=out['walkers'])
    except ValueError as err:
        raise ValueError(f'[Ensemble] {err}') from None


def moves_arguments(cfg):
    """The ``moves`` / ``gamma0`` / ``sigma`` / ``gamma_s`` arguments of the sampler classes the settings ``cfg`` ask for (with
    ``moves = slice``: ``moves`` / ``mu`` / ``tune_steps``): empty without ``moves``, so that a run without them is constructed as
    ever."""
    if 'moves' not in cfg:
        return {}
    if cfg['moves'] == 'slice':
        return dict(moves='slice', **{arg: cfg[key] for key, arg in _SLICE_KEYS if key in cfg})
    return dict(moves=cfg['moves'], **{arg: cfg[key] for key, arg in _MOVE_KEYS if key in cfg})


def _parse_mocks(sec, main_config, section='Ensemble', own='an ensemble'):
    """``mocks = M`` of ``[Ensemble]`` (or ``[SMC]``): a posterior for each of M Monte-Carlo mocks in one run; it needs the
    Monte-Carlo mode."""
    try:
        M = sec.getint('mocks')
    except ValueError:
        raise ValueError(f'[{section}] mocks: a whole number, at least 1') from None
    if M < 1:
        raise ValueError(f'[{section}] mocks: a whole number, at least 1')
    control = main_config['control']
    if not control.getboolean('run_montecarlo', False):
        raise ValueError(f'[{section}] mocks needs "run_montecarlo = True" in the "[control]" section')
    if 'monte carlo' not in main_config:
        raise ValueError(f'[{section}] mocks needs a "[monte carlo]" section')
    if 'replicas' in sec and sec.getint('replicas') > 1:
        raise ValueError(f'[{section}] mocks and replicas > 1 do not combine: every mock has {own} of its own')
    return M


def chain_arguments(cfg):
    """``chain='device'`` for the settings that stop by convergence - the checks then read a few numbers per ensemble instead of
    the chain; empty otherwise, so that a run without ``converge`` is constructed as ever."""
    return dict(chain='device') if 'converge' in cfg else {}


def build_sampler(vega, cfg, sample_params, stream=0):
    """The sampler the settings ``cfg`` (:func:`sampler_settings`) ask for, on the Philox stream ``stream``."""
    if cfg['sampler'] == 'Nested':
        from .nested import NestedSampler
        return NestedSampler(vega, num_live=cfg['num_live'], num_repeats=cfg['num_repeats'], threads=cfg['threads'],
                             precision=cfg['precision'], seed=cfg['seed'], driver=cfg['driver'],
                             max_iterations=cfg['max_iterations'], sample_params=sample_params, stream=stream,
                             clustering=cfg.get('do_clustering', False), cluster_posteriors=cfg.get('cluster_posteriors', False),
                             boost_posterior=cfg.get('boost_posterior', 0.0))
    if cfg['sampler'] == 'SMC':
        from .smc import SMCSampler
        return SMCSampler(vega, particles=cfg['particles'], ess=cfg['ess'], sweeps=cfg['sweeps'], seed=cfg['seed'],
                          driver=cfg['driver'], max_stages=cfg['max_stages'], sample_params=sample_params, stream=stream,
                          **{key: cfg[key] for key in ('n_total', 'recycle') if key in cfg})
    if 'ntemps' in cfg:
        return TemperedEnsemble(vega, cfg['walkers'], ntemps=cfg['ntemps'], beta_min=cfg.get('beta_min'), swap_every=cfg['swap_every'],
                                streams=[stream], a=cfg['a'], seed=cfg['seed'], thin=cfg['thin'], driver=cfg['driver'],
                                sample_params=sample_params, **moves_arguments(cfg),
                                **{key: cfg[key] for key in _ADAPT_KEYS if key in cfg})
    return EnsembleSampler(vega, cfg['walkers'], a=cfg['a'], seed=cfg['seed'], thin=cfg['thin'], driver=cfg['driver'],
                           sample_params=sample_params, stream=stream, **moves_arguments(cfg), **chain_arguments(cfg))


def advance_sampler(sampler, cfg):
    """Run a sampler of :func:`build_sampler` as its settings say: the ensemble its steps, the others to their end."""
    if cfg['sampler'] in ('Nested', 'SMC'):
        return sampler.run()
    if 'converge' in cfg:
        return sampler.run_until(cfg['steps'], start=cfg['init'], init_scale=cfg['init_scale'], **cfg['converge'])
    return sampler.run(cfg['steps'], start=cfg['init'], init_scale=cfg['init_scale'])


def run_vega_sampler(config_path, search_dirs=(), print_func=print, rank=None, world_size=None, make_vega=None, **vega_kwargs):
    """bin/run_vega_mpi.py: initialise, compute the model once, switch to the Monte-Carlo mock when asked, require
    ``run_sampler = True`` and ``sampler = Ensemble``, ``Nested`` or ``SMC``, run the ``[Ensemble]`` / ``[Nested]`` / ``[SMC]``
    settings, write the getdist chain (a nested or SMC run also ``name.stats`` with the evidence; with ``derived = True`` in the
    sampler's section the marginalisation coefficients as derived columns).  Returns the sampler.

    One process per GPU: ``rank`` / ``world_size`` (default: ``RANK`` / ``WORLD_SIZE`` / ``LOCAL_RANK`` of the environment, as
    torchrun sets them; one process without them) share out the ``replicas = R`` of the sampler's section
    (:mod:`vega_amd.replicas`); the device is ``LOCAL_RANK % torch.cuda.device_count()``, chosen before anything touches the GPU.
    With R > 1 every rank returns a :class:`vega_amd.replicas.ReplicaRun` and rank 0 writes the merged files; without the key
    (or with R = 1) the files are those of one plain run, written by rank 0, and the other ranks return None.
    ``make_vega(config_path, device)`` may replace the interface (CPU tests of the body)."""
    from . import replicas
    rank, world, local_rank = replicas.ranks_from_environment(rank, world_size)
    if world > 1 or 'LOCAL_RANK' in os.environ:
        vega_kwargs.setdefault('device', replicas.device_of(local_rank))
    group = replicas.Group(rank, world)
    if rank > 0:
        print_func = _silent
    print_func('Initializing Vega')
    if make_vega is None:
        from .interface import VegaInterface
        vega = VegaInterface(config_path, search_dirs=search_dirs, **vega_kwargs)
    else:
        vega = make_vega(config_path, vega_kwargs.get('device', 0))
    sample_params = vega.sample_params
    _ = vega.compute_model(run_init=False)
    print_func('Finished initializing Vega')
    control = vega.main_config['control'] if 'control' in vega.main_config else configparser.ConfigParser()['DEFAULT']
    run_montecarlo = control.getboolean('run_montecarlo', False)
    if run_montecarlo and vega.mc_config is not None:
        vega.initialize_monte_carlo(print_func=print_func)
        sample_params = vega.mc_config['sample']
    elif run_montecarlo:
        raise ValueError('You asked to run over a Monte Carlo simulation, but no "[monte carlo]" section provided.')
    cfg = sampler_settings(vega.main_config, sample_params)
    kind = {'Nested': 'nested', 'SMC': 'SMC'}.get(cfg['sampler'], 'ensemble')
    if cfg.get('mocks'):
        sampler = None
        if rank == 0:
            print_func(f'Sampling the posteriors of {cfg["mocks"]} Monte-Carlo mocks in one run')
            sampler = _sample_config_mocks(vega, cfg, sample_params, control)
        group.barrier()
        print_func('Finished running sampler')
        return sampler
    if cfg.get('replicas', 1) > 1:
        print_func(f'Running {cfg["replicas"]} replicas of the {kind} sampler on {world} rank(s)')
        out = replicas.run_replicas(vega, cfg, sample_params, group, print_func)
        print_func(out.summary())
        print_func('Finished running sampler')
        return out
    sampler = None
    if rank == 0:           # (one run: the files of today, by the path of today)
        print_func(f'Running the {kind} sampler')
        sampler = advance_sampler(build_sampler(vega, cfg, sample_params), cfg)
        if hasattr(sampler, 'log_evidence'):
            log_z, err = sampler.log_evidence()
            print_func(f'log(Z) = {log_z} +- {err}')
        sampler.write(cfg['path'], cfg['name'], derived=cfg.get('derived', False), print_func=print_func)
        if 'converge' in cfg:
            write_convergence(sampler, cfg['path'], cfg['name'])
    group.barrier()
    print_func('Finished running sampler')
    return sampler


def _sample_config_mocks(vega, cfg, sample_params, control):
    """``[Ensemble] mocks = M``: M mocks around the Monte-Carlo fiducial with ``[control] mc_seed``, their posteriors as one
    :class:`EnsembleSet` (:meth:`vega_amd.montecarlo.MonteCarlo.sample_mocks`); writes the getdist chains ``<name>_mock<m>.txt``
    with one ``<name>.paramnames`` and the summary table ``mock_posteriors.fits``.  ``[SMC] mocks = M``: the same mocks as one
    :class:`vega_amd.smc.SMCSet`; every mock's three files ``<name>_mock<m>.txt`` / ``.paramnames`` / ``.stats`` (the evidence)
    and the table.  ``[Nested] mocks = M``: the same mocks as one :class:`vega_amd.nested.NestedSet`, with the same files per mock.
    Returns the set."""
    mc = vega.analysis
    scale = None
    if vega._use_global_cov and 'global_cov_rescale' in control:
        scale = control.getfloat('global_cov_rescale')
    mocks = mc.create_mocks(vega.mc_fiducial_model, cfg['mocks'], seed=control.getint('mc_seed', 0), scale=scale,
                            forecast=control.getboolean('forecast', False))
    if 'global' in mc.mc_mocks:
        mocks = mc.mc_mocks['global']
    if cfg['sampler'] == 'SMC':
        sampler = mc.sample_mocks(mocks=mocks, seed=cfg['seed'], scale=scale, sample_params=sample_params, driver=cfg['driver'],
                                  sampler='smc', particles=cfg['particles'], ess=cfg['ess'], sweeps=cfg['sweeps'],
                                  **{key: cfg[key] for key in ('n_total', 'recycle', 'weighted_quantiles') if key in cfg})
        for m in range(sampler.E):
            sampler.member(m).write(cfg['path'], f'{cfg["name"]}_mock{m}')
        mc.write_mock_posteriors(cfg['path'])
        return sampler
    if cfg['sampler'] == 'Nested':
        sampler = mc.sample_mocks_nested(mocks=mocks, seed=cfg['seed'], scale=scale, sample_params=sample_params,
                                         driver=cfg['driver'], num_live=cfg['num_live'], num_repeats=cfg['num_repeats'],
                                         threads=cfg['threads'], precision=cfg['precision'], max_iterations=cfg['max_iterations'],
                                         **{key: cfg[key] for key in ('weighted_quantiles',) if key in cfg})
        for m in range(sampler.E):
            if sampler.status[m] != 2:          # (a mock without a finite live lnL has nothing to write: its row of the table says so)
                sampler.member(m).write(cfg['path'], f'{cfg["name"]}_mock{m}')
        mc.write_mock_posteriors(cfg['path'])
        return sampler
    sampler = mc.sample_mocks(mocks=mocks, walkers=cfg['walkers'], steps=cfg['steps'], thin=cfg['thin'], seed=cfg['seed'],
                              scale=scale, sample_params=sample_params, driver=cfg['driver'], **moves_arguments(cfg),
                              **(dict(summaries='device') if 'converge' in cfg or 'quantiles' in cfg else {}),
                              **{key: cfg[key] for key in ('converge', 'quantiles') if key in cfg})
    if 'converge' in cfg:
        write_convergence(sampler, cfg['path'], cfg['name'])
    chain, lnl = sampler.get_chain(), sampler.get_log_lik()
    for m in range(sampler.E):
        table, lines = getdist_table(sampler.names, chain[m], lnl[m])
        np.savetxt(Path(cfg['path']) / f'{cfg["name"]}_mock{m}.txt', table, fmt='%.17g')
    write_paramnames(cfg['path'], cfg['name'], lines)
    mc.write_mock_posteriors(cfg['path'])
    return sampler


def _silent(*args, **kwargs):
    pass
