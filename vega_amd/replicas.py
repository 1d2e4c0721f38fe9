"""Replicas of the device samplers over the GPUs of a node, and their merges.

The reference's sampler entry is a parallel program (bin/run_vega_mpi.py spreads PolyChord or pocoMC over MPI ranks).  Here a
sampler step is a dependent chain of short batches with one small decision kernel between them, so one run cut across GPUs would
pay a collective and a host turn per round - more than the round - and would give up the property every sampler test rests on:
one pinned state machine, the same bits under either driver.  So ``replicas = R`` in ``[Ensemble]`` / ``[Nested]`` / ``[SMC]``
runs R independent copies of the configured sampler instead: replica r has the same ``seed`` and the Philox ``stream`` word r
(the second key word of every generator in vmx_ensemble.h, vmx_nested.h and vmx_smc.h), which is all that tells the copies apart.
Ranks take contiguous shares of ``range(R)`` (:func:`vega_amd.parallel.shard_bounds`) and run them one after the other on their
own engine; every replica leaves one record ``<name>.replica<r>.npz``; after a barrier rank 0 reads the R records back and merges:

* nested runs merge exactly into one run with the summed live count (:func:`merge_nested`; Skilling 2006, the rule nestcheck and
  dyPolyChord use); runs that kept phantom points (``boost_posterior``) carry them in their records and
  :func:`merge_nested_boosted` merges them into the weighted chain, the evidence staying the base merge's; replicas that cluster (``do_clustering``) number their clusters independently, so a record carries no
  cluster ids and the merged run has none (``cluster_posteriors`` with ``replicas > 1`` is refused when the settings are read),
* SMC evidences are unbiased, so they average (:func:`merge_smc`),
* independent ensembles are kept apart and supply what one ensemble cannot, a between-chain convergence figure
  (:func:`gelman_rubin`).

The merged files depend on the records alone, never on how many ranks made them.  There is no data-path collective: the process
group (gloo) carries barriers and one gather of small per-rank counts.  Everything in this module is NumPy on the host.
"""
import math
import os
import sys
import time
from pathlib import Path

import numpy as np

from . import ensemble as E
from . import nested as NS
from .parallel import shard_bounds

MAX_RANKS = 16          # rank processes of one node


# ------------------------------------------------------------------ settings
def parse_replicas(section):
    """``replicas = R`` of a sampler's section (an integer >= 1), or None when the section does not state it."""
    if 'replicas' not in section:
        return None
    try:
        R = section.getint('replicas')
    except ValueError:
        raise ValueError(f'[{section.name}] replicas: a whole number, at least 1') from None
    if R < 1:
        raise ValueError(f'[{section.name}] replicas: a whole number, at least 1')
    return R


# ------------------------------------------------------------------ records
_KINDS = ('ensemble', 'nested', 'smc')
_STAGE_KEYS = ('beta_prev', 'beta', 'ess', 'accepted', 'scale', 'cholesky', 'lnl', 'anc')


def _common(sampler, kind, points, derived):
    rec = dict(kind=kind, seed=int(sampler.seed), stream=int(sampler.stream), points=np.asarray(points, dtype=np.float64),
               names=np.array([str(nm) for nm in getattr(sampler, 'names', [f'p{i}' for i in range(sampler.n)])]),
               driver=str(getattr(sampler, 'driver', None) or 'python'))
    for key, val in sampler.stats.items():
        if key == 'moves':          # (the ensemble's per-move counts: one number per move and count; an unknown count is left out)
            rec.update({f'stats_moves_{move}_{what}': v for move, counts in val.items() for what, v in counts.items() if v is not None})
            continue
        if key == 'cov':            # (the covariance move: its scale and the factor fallbacks, one entry each)
            rec.update({f'stats_cov_{name}': v for name, v in val.items()})
            continue
        if key == 'slice':          # (ensemble slice sampling: its counts and scale, one entry each)
            rec.update({f'stats_slice_{name}': v for name, v in val.items()})
            continue
        rec[f'stats_{key}'] = val
    if derived:
        rec.update(derived=np.asarray(derived['derived'], dtype=np.float64), derived_names=np.array(list(derived['derived_names'])),
                   derived_labels=np.array(list(derived['derived_labels'])))
    return rec


def nested_record(run, derived=None):
    """The record of a finished :class:`vega_amd.nested.NestedRun`: the dead record, the final live points, the run's own
    evidence; ``points`` are the physical rows of the base run's samples (dead, then live).  A run that kept phantom points
    (``boost_posterior > 0``) also carries ``ph_u`` (in the cube), ``ph_lnl``, ``ph_birth`` and ``ph_points`` (physical) in the
    canonical order, and with ``derived`` (the block over its boosted ``samples()``) ``ph_derived``; a run without them writes
    the keys it always wrote."""
    du, dl, dn = run.dead()
    log_z, err = run.log_evidence()
    boosted = getattr(run, 'phantom_state', None) is not None
    extra = {}
    if boosted:
        ph = run.phantoms()
        extra = dict(ph_u=ph['u'], ph_lnl=ph['lnl'], ph_birth=ph['birth'], ph_points=np.asarray(run.to_physical(ph['u']), dtype=np.float64))
        if derived:         # (the block follows the boosted chain: back into the order dead, live, phantoms)
            block = np.asarray(derived['derived'], dtype=np.float64)
            rows = np.empty_like(block)
            rows[run.boost_index()] = block
            base = dl.size + run.live_lnl.size
            derived = dict(derived, derived=rows[:base])
            extra['ph_derived'] = rows[base:]
    rec = _common(run, 'nested', run.samples(boost=False)[0] if boosted else run.samples()[0], derived)
    rec.update(extra)
    rec.update(dead_u=du, dead_lnl=dl, dead_nlive=np.asarray(dn, dtype=np.int32), live_u=run.live_u.copy(),
               live_lnl=run.live_lnl.copy(), num_live=run.num_live, num_repeats=run.num_repeats, threads=run.threads,
               iteration=run.iteration, log_z=log_z, err=err, info=run.information())
    return rec


def smc_record(run, derived=None):
    """The record of an :class:`vega_amd.smc.SMCRun`: the final particles with their lnL, the stage record (one row per stage),
    the run's own evidence."""
    log_z, err = run.log_evidence()
    rec = _common(run, 'smc', run.samples()[0], derived)
    rec.update(u=run.u.copy(), lnl=run.lnl.copy(), particles=run.particles, sweeps=run.sweeps, ess_target=run.ess, stage=run.stage,
               log_z=log_z, err=err)
    for key in _STAGE_KEYS:
        rec[f'stage_{key}'] = np.array([r[key] for r in run.record])
    return rec


def ensemble_record(sampler, derived=None):
    """The record of an :class:`vega_amd.ensemble.EnsembleSampler`: chain and lnL as ``get_chain()`` / ``get_log_lik()`` return
    them, and ``accepted``."""
    chain = sampler.get_chain()
    rec = _common(sampler, 'ensemble', chain, derived)
    rec.update(chain=chain, chain_lnl=sampler.get_log_lik(), accepted=np.asarray(sampler.accepted, dtype=np.int64),
               steps=sampler.step, thin=sampler.thin, walkers=sampler.W)
    return rec


def record_of(sampler, derived=False, print_func=print):
    """The record of a finished sampler of any of the three kinds; ``derived``: with the derived block of its rows, computed
    here - by the rank that ran it - with the sampler's own ``derived()`` pass."""
    extra = E.derived_for_write(sampler, derived, print_func) if derived else {}
    if hasattr(sampler, 'get_chain'):
        if extra:
            extra['derived'] = sampler.get_derived()
        return ensemble_record(sampler, extra)
    if extra:
        extra['derived'] = sampler.derived()
    return smc_record(sampler, extra) if hasattr(sampler, 'particles') else nested_record(sampler, extra)


def record_path(path, name, r):
    return Path(path) / f'{name}.replica{r}.npz'


def save_record(path, record):
    """One ``.npz`` of arrays and scalars (nothing pickled)."""
    if record['kind'] not in _KINDS:
        raise ValueError(f'record kind: one of {_KINDS}')
    np.savez(path, **{key: np.asarray(val) for key, val in record.items()})
    return Path(path)


def load_record(path):
    """A record back: arrays as arrays, scalars as Python numbers and strings, ``stats`` gathered into a dict."""
    out, stats = {}, {}
    with np.load(path, allow_pickle=False) as f:
        for key in f.files:
            val = f[key]
            val = val.item() if val.ndim == 0 else val
            if key.startswith('stats_'):
                stats[key[6:]] = val
            else:
                out[key] = val
    out['stats'] = stats
    return out


def _stats_of(record):
    return record['stats'] if 'stats' in record else {k[6:]: v for k, v in record.items() if k.startswith('stats_')}


# ------------------------------------------------------------------ merges
def _same(records, key):
    vals = [r[key] for r in records]
    return all(np.array_equal(v, vals[0]) for v in vals[1:])


def _check(records, kind):
    records = list(records)
    if not records:
        raise ValueError('no records to merge')
    if any(r['kind'] != kind for r in records):
        raise ValueError(f'merge of {kind} records: every record must be one')
    if any(r['points'].shape[-1] != records[0]['points'].shape[-1] for r in records):
        raise ValueError('records of different parameter counts')
    if any(('derived' in r) != ('derived' in records[0]) for r in records):
        raise ValueError('records with and without derived columns')
    return records


def death_sequence(record):
    """A nested run as one sequence of deaths in ascending lnL: (lnL [m], live count [m], index [m] into the rows of the record's
    ``points``) - its dead record, then its final live points in ascending lnL (ties in index order) with the live counts
    nlive, nlive - 1, ..., 1."""
    dead_lnl, live_lnl = np.asarray(record['dead_lnl'], dtype=np.float64), np.asarray(record['live_lnl'], dtype=np.float64)
    order = np.argsort(live_lnl, kind='stable')
    nlive = live_lnl.size
    lnl = np.concatenate([dead_lnl, live_lnl[order]])
    count = np.concatenate([np.asarray(record['dead_nlive'], dtype=np.int64), nlive - np.arange(nlive, dtype=np.int64)])
    return lnl, count, np.concatenate([np.arange(dead_lnl.size), dead_lnl.size + order])


def merge_nested(records):
    """Independent nested runs as one run (Skilling 2006, section 'combining'): all deaths of all runs in ascending lnL (a stable
    sort of the runs' :func:`death_sequence` laid end to end, so that ties are broken by (replica, index)).  The live count at a
    merged death of level L is ``n = sum_r n_r(L)``: a run contributes the count recorded at its first event with lnL >= L - its
    own count at its own deaths - and 0 once it is exhausted.  Then the rule of :func:`vega_amd.nested.log_weights`:
    ``log X_i = log X_{i-1} - 1 / n_i``, ``w_i = X_{i-1} - X_i``, ``log Z = log sum_i L_i w_i``, ``H = sum_i p_i (lnL_i - log Z)``
    with ``p_i = L_i w_i / Z``, ``err = sqrt(H / sum_r nlive_r)``.  Every run ended by its own criterion; the final live points
    die one by one here (a single run's :func:`vega_amd.nested.evidence` gives them ``X_end / nlive`` each: the two agree to a
    few 1e-6 in log Z).

    Returns dict(log_z, err, info, points, lnl, weights (summing to 1), nlive (the merged counts), log_x, replica, index (which
    row of which record a merged row is), num_live (the summed live count) and ``derived`` when the records carry it)."""
    records = _check(records, 'nested')
    seqs = [death_sequence(r) for r in records]
    lnl = np.concatenate([s[0] for s in seqs])
    own = np.concatenate([s[1] for s in seqs])
    replica = np.concatenate([np.full(s[0].size, r, dtype=np.int64) for r, s in enumerate(seqs)])
    index = np.concatenate([s[2] for s in seqs])
    order = np.argsort(lnl, kind='stable')
    lnl, own, replica, index = lnl[order], own[order], replica[order], index[order]
    count = np.zeros(lnl.size, dtype=np.int64)
    for r, (l_r, n_r, _) in enumerate(seqs):
        first = np.searchsorted(l_r, lnl, side='left')
        there = first < l_r.size
        count += np.where(replica == r, own, np.where(there, n_r[np.minimum(first, l_r.size - 1)], 0))
    log_x = -np.cumsum(1.0 / count)
    log_w = np.concatenate([[0.0], log_x[:-1]]) + np.log1p(-np.exp(-1.0 / count))
    lw = lnl + log_w
    log_z = NS._logsumexp(lw)
    with np.errstate(invalid='ignore'):
        p = np.exp(lw - log_z) if np.isfinite(log_z) else np.zeros(lw.size)
    p = np.where(np.isfinite(p), p, 0.0)
    used = p > 0.0
    info = float(np.sum(p[used] * (lnl[used] - log_z))) if np.any(used) else 0.0
    num_live = int(sum(np.asarray(r['live_lnl']).size for r in records))
    out = dict(log_z=log_z, err=math.sqrt(max(info, 0.0) / num_live), info=info, lnl=lnl, weights=p / p.sum(), nlive=count,
               log_x=log_x, replica=replica, index=index, num_live=num_live,
               points=np.concatenate([np.asarray(r['points'])[s[2]] for r, s in zip(records, seqs)])[order])
    if 'derived' in records[0]:
        out['derived'] = np.concatenate([np.asarray(r['derived'])[s[2]] for r, s in zip(records, seqs)])[order]
    return out


def merge_nested_boosted(records):
    """:func:`merge_nested` with the records' phantom points (``ph_lnl``, ``ph_birth``, ``ph_points``; a record may have none)
    merged into the weighted chain, as :func:`vega_amd.nested.boosted_weights` does for one run.  The events are the runs'
    :func:`death_sequence` and all phantoms of all records, sorted by (lnL, deaths before phantoms, (replica, index)).  The
    live count of an event at level L is ``m = sum_r n_r(L) + a(L)``: ``n_r(L)`` by :func:`merge_nested`'s rule - a run's own count
    at its own deaths, the count at its first event with lnL >= L otherwise, 0 once it is exhausted - and
    ``a(L) = #{phantoms p of any record : birth_p < L <= lnL_p}``, a phantom being a point that is uniform in its birth contour
    until the level passes it.  Then ``log X_i = log X_{i-1} - 1 / m_i`` and ``w_i = X_{i-1} - X_i``.

    Returns :func:`merge_nested`'s dict with ``points``, ``lnl``, ``weights``, ``nlive`` (m), ``log_x``, ``replica`` and ``index``
    (a phantom's: its row of the record's phantoms) over the boosted events, ``phantom`` [rows] bool and ``log_z_boost`` (the
    log-sum of the boosted weights: a diagnostic); ``log_z``, ``err`` and ``info`` are :func:`merge_nested`'s, from the base
    records."""
    records = _check(records, 'nested')
    base = merge_nested(records)
    dims = np.asarray(records[0]['points']).shape[-1]
    seqs = [death_sequence(r) for r in records]
    ph_lnl = [np.asarray(r['ph_lnl'], dtype=np.float64) if 'ph_lnl' in r else np.empty(0) for r in records]
    ph_birth = [np.asarray(r['ph_birth'], dtype=np.float64) if 'ph_birth' in r else np.empty(0) for r in records]
    ph_pts = [np.asarray(r['ph_points'], dtype=np.float64).reshape(-1, dims) if 'ph_points' in r else np.empty((0, dims)) for r in records]
    if any(a.size != b.size or a.size != c.shape[0] for a, b, c in zip(ph_lnl, ph_birth, ph_pts)):
        raise ValueError('a record\'s ph_lnl, ph_birth and ph_points differ in length')
    if any(np.any(~(a > b)) for a, b in zip(ph_lnl, ph_birth)):
        raise ValueError('a phantom point must lie above its birth contour')
    lnl = np.concatenate([s[0] for s in seqs] + ph_lnl)
    own = np.concatenate([s[1] for s in seqs] + [np.zeros(a.size, dtype=np.int64) for a in ph_lnl])
    is_ph = np.concatenate([np.zeros(s[0].size, dtype=bool) for s in seqs] + [np.ones(a.size, dtype=bool) for a in ph_lnl])
    replica = np.concatenate([np.full(s[0].size, r, dtype=np.int64) for r, s in enumerate(seqs)] +
                             [np.full(a.size, r, dtype=np.int64) for r, a in enumerate(ph_lnl)])
    index = np.concatenate([s[2] for s in seqs] + [np.arange(a.size, dtype=np.int64) for a in ph_lnl])
    points = np.concatenate([np.asarray(r['points'])[s[2]] for r, s in zip(records, seqs)] + ph_pts)
    # (the events of every kind lie replica by replica, index by index: a stable sort leaves ties in that order)
    order = np.lexsort((is_ph, lnl))
    lnl, own, is_ph, replica, index = lnl[order], own[order], is_ph[order], replica[order], index[order]
    count = np.zeros(lnl.size, dtype=np.int64)
    for r, (l_r, n_r, _) in enumerate(seqs):
        first = np.searchsorted(l_r, lnl, side='left')
        there = first < l_r.size
        count += np.where((replica == r) & ~is_ph, own, np.where(there, n_r[np.minimum(first, l_r.size - 1)], 0))
    # a: lnL_p > birth_p, so #{birth_p < L <= lnL_p} = #{birth_p < L} - #{lnL_p < L}
    all_lnl, all_birth = np.sort(np.concatenate(ph_lnl)), np.sort(np.concatenate(ph_birth))
    count += np.searchsorted(all_birth, lnl, side='left') - np.searchsorted(all_lnl, lnl, side='left')
    log_x = -np.cumsum(1.0 / count)
    lw = lnl + np.concatenate([[0.0], log_x[:-1]]) + np.log1p(-np.exp(-1.0 / count))
    log_z_boost = NS._logsumexp(lw)
    with np.errstate(invalid='ignore'):
        p = np.exp(lw - log_z_boost) if np.isfinite(log_z_boost) else np.zeros(lw.size)
    p = np.where(np.isfinite(p), p, 0.0)
    out = dict(base, lnl=lnl, weights=p / p.sum(), nlive=count, log_x=log_x, replica=replica, index=index, points=points[order],
               phantom=is_ph, log_z_boost=log_z_boost)
    if 'derived' in records[0]:
        width = np.asarray(records[0]['derived']).shape[1:]
        if any(a.size and 'ph_derived' not in r for a, r in zip(ph_lnl, records)):
            raise ValueError('records with derived columns and phantom points need ph_derived')
        out['derived'] = np.concatenate([np.asarray(r['derived'])[s[2]] for r, s in zip(records, seqs)] +
                                        [np.asarray(r['ph_derived']) if 'ph_derived' in r else np.empty((0,) + width)
                                         for r in records])[order]
    return out


def merge_smc(records):
    """Independent SMC runs: every ``Z_r`` is an unbiased estimate of Z, so ``Z = mean_r Z_r``:
    ``log Z = logsumexp_r(log Z_r) - log R`` with ``err = sqrt(sum_r (Z_r err_r)^2) / sum_r Z_r`` (the runs' delta-method figures
    carried through the mean).  ``scatter = sd_r(log Z_r) / sqrt(R)`` stands beside it as a second witness, taken from the
    replicas themselves: the delta-method figure of one run was measured 1.0 - 1.2 times low (:func:`vega_amd.smc.evidence`).
    The samples are pooled; a sample of run r weighs ``Z_r / (N_r sum_s Z_s)`` (a run that found more mass speaks for more of it).

    Returns dict(log_z, err, scatter (NaN for one run), log_z_runs, err_runs, points, lnl, weights (summing to 1), replica, index
    and ``derived`` when the records carry it)."""
    records = _check(records, 'smc')
    R = len(records)
    lz = np.array([float(r['log_z']) for r in records])
    er = np.array([float(r['err']) for r in records])
    log_sum = NS._logsumexp(lz)
    share = np.exp(lz - log_sum)                         # Z_r / sum_s Z_s
    sizes = [np.asarray(r['lnl']).size for r in records]
    out = dict(log_z=log_sum - math.log(R), err=float(np.sqrt(np.sum((share * er)**2))),
               scatter=float(np.std(lz, ddof=1) / math.sqrt(R)) if R > 1 else math.nan, log_z_runs=lz, err_runs=er,
               points=np.concatenate([np.asarray(r['points']) for r in records]),
               lnl=np.concatenate([np.asarray(r['lnl'], dtype=np.float64) for r in records]),
               weights=np.concatenate([np.full(N, s / N) for s, N in zip(share, sizes)]),
               replica=np.concatenate([np.full(N, r, dtype=np.int64) for r, N in enumerate(sizes)]),
               index=np.concatenate([np.arange(N) for N in sizes]))
    if 'derived' in records[0]:
        out['derived'] = np.concatenate([np.asarray(r['derived']) for r in records])
    return out


def gelman_rubin(chains, discard=0):
    """The potential scale reduction R-hat (Gelman & Rubin 1992), split-free, per parameter over R >= 2 chains.  ``chains``: R
    arrays [rows, W, n] (ensembles: the walkers and steps of one ensemble are pooled into its within-variance) or [rows, n]; the
    first ``discard`` rows of each are dropped; every chain must keep the same number m >= 2 of draws.  With chain means
    ``mu_j`` and chain variances ``s_j^2`` (both over a chain's m draws, the variance with m - 1)::

        W = mean_j s_j^2        B / m = sum_j (mu_j - mean_j mu_j)^2 / (R - 1)
        var+ = (m - 1) / m  W + B / m        R-hat = sqrt(var+ / W)

    A parameter no chain moved in (W = 0) gives NaN."""
    flat = []
    for c in chains:
        c = np.asarray(c, dtype=np.float64)
        if c.ndim not in (2, 3):
            raise ValueError('gelman_rubin: chains [rows, walkers, n] or [rows, n]')
        c = c[int(discard):]
        flat.append(c.reshape(-1, c.shape[-1]))
    if len(flat) < 2:
        raise ValueError('gelman_rubin: at least two chains')
    m = flat[0].shape[0]
    if m < 2 or any(c.shape != flat[0].shape for c in flat):
        raise ValueError('gelman_rubin: chains of one shape with at least two draws after the discard')
    means = np.array([c.mean(axis=0) for c in flat])
    within = np.mean([c.var(axis=0, ddof=1) for c in flat], axis=0)
    between_over_m = means.var(axis=0, ddof=1)
    var_plus = (m - 1.0) / m * within + between_over_m
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt(var_plus / within)


def merge_ensemble(records, discard=None):
    """Independent ensembles stay apart - each is a chain of its own, which is what a between-chain figure needs.  Returns
    dict(chains [R][rows, W, n], lnl [R][rows, W], discard (default: the first half of the recorded rows), rhat [n] (NaN for one
    replica), acceptance [R] (mean acceptance fraction), tau [R, n] (integrated autocorrelation times in recorded rows), points
    and weights (the pooled rows, equal weights) and ``derived`` [R][rows, W, m] when the records carry it)."""
    records = _check(records, 'ensemble')
    chains = [np.asarray(r['chain']) for r in records]
    if any(c.shape != chains[0].shape for c in chains):
        raise ValueError('ensembles of different shapes')
    rows, _, n = chains[0].shape
    discard = rows // 2 if discard is None else int(discard)
    points = np.concatenate([c.reshape(-1, n) for c in chains])
    out = dict(chains=chains, lnl=[np.asarray(r['chain_lnl']) for r in records], discard=discard,
               rhat=gelman_rubin(chains, discard) if len(chains) > 1 else np.full(n, np.nan),
               acceptance=np.array([np.mean(np.asarray(r['accepted']) / max(int(r['steps']), 1)) for r in records]),
               tau=np.array([E.integrated_time(c) for c in chains]), points=points,
               weights=np.full(points.shape[0], 1.0 / max(points.shape[0], 1)))
    if 'derived' in records[0]:
        out['derived'] = [np.asarray(r['derived']) for r in records]
    return out


def merge(records):
    kind = records[0]['kind']
    return dict(ensemble=merge_ensemble, nested=merge_nested, smc=merge_smc)[kind](records)


# ------------------------------------------------------------------ the files of a merged run
def _derived_args(records, block):
    if 'derived' not in records[0]:
        return {}
    return dict(derived=block, derived_names=[str(s) for s in records[0]['derived_names']],
                derived_labels=[str(s) for s in records[0]['derived_labels']])


def _floats(values):
    return ' '.join(repr(float(v)) for v in values)


def write_merged(path, name, records, merged=None):
    """The final files of R > 1 replicas from their records.

    Nested / SMC: ``name.txt`` and ``name.paramnames`` - the merged weighted chain (weight / max weight, -lnL, the parameters,
    the derived columns) - and ``name.stats``: the merged figures under the keys of a single run's file (counts summed over the
    replicas), then ``replicas = R`` and one line ``replica <r> = log Z_r err_r`` per replica (SMC: also ``log(Z) scatter`` and
    each replica's ladder ``beta <r>``).  Ensemble: ``name_1.txt ... name_R.txt`` with one ``name.paramnames`` (getdist's
    multi-chain convention) and ``name.stats`` with ``Rhat <parameter>``, ``acceptance fraction <r>`` and ``autocorrelation
    time <r>``.  Nothing in them depends on clocks or on which rank ran what.  Returns the list of files."""
    path = Path(path)
    names = [str(s) for s in records[0]['names']]
    merged = merge(records) if merged is None else merged
    kind, R = records[0]['kind'], len(records)
    st = [_stats_of(r) for r in records]
    stats = path / f'{name}.stats'
    if kind == 'ensemble':
        files = []
        for k, (chain, lnl) in enumerate(zip(merged['chains'], merged['lnl'])):
            extra = _derived_args(records, merged['derived'][k] if 'derived' in merged else None)
            table, lines = E.getdist_table(names, chain, lnl, **extra)
            np.savetxt(path / f'{name}_{k + 1}.txt', table, fmt='%.17g')
            files.append(path / f'{name}_{k + 1}.txt')
        files.append(E.write_paramnames(path, name, lines))
        with open(stats, 'w') as f:
            f.write(f'replicas = {R}\nwalkers = {int(records[0]["walkers"])}\nsteps = {int(records[0]["steps"])}\n')
            f.write(f'thin = {int(records[0]["thin"])}\nseed = {int(records[0]["seed"])}\ndiscard = {merged["discard"]}\n')
            for nm, v in zip(names, merged['rhat']):
                f.write(f'Rhat {nm} = {float(v)!r}\n')
            for k in range(R):
                f.write(f'acceptance fraction {k} = {float(merged["acceptance"][k])!r}\n')
            for k in range(R):
                f.write(f'autocorrelation time {k} = {_floats(merged["tau"][k])}\n')
        return files + [stats]
    w = merged['weights']
    txt, pn = E.write_getdist(path, name, names, merged['points'], merged['lnl'], weights=w / w.max(),
                              **_derived_args(records, merged.get('derived')))
    rows = sum(int(s['rows']) for s in st)
    with open(stats, 'w') as f:
        if kind == 'nested':
            f.write(f'log(Z) = {merged["log_z"]!r}\nlog(Z) error = {merged["err"]!r}\nH = {merged["info"]!r}\n')
            f.write(f'dead points = {sum(np.asarray(r["dead_lnl"]).size for r in records)}\nlikelihood evaluations = {rows}\n')
            f.write(f'iterations = {sum(int(r["iteration"]) for r in records)}\nseed = {int(records[0]["seed"])}\n')
            f.write(f'num_live = {merged["num_live"]}\nnum_repeats = {int(records[0]["num_repeats"])}\n')
            f.write(f'threads = {int(records[0]["threads"])}\n')
            if 'log_z_boost' in merged:         # (a merge by merge_nested_boosted, passed in)
                f.write(f'phantom points = {int(np.sum(merged["phantom"]))}\nlog(Z) boosted = {merged["log_z_boost"]!r}\n')
        else:
            f.write(f'log(Z) = {merged["log_z"]!r}\nlog(Z) error = {merged["err"]!r}\n')
            f.write(f'stages = {sum(int(r["stage"]) for r in records)}\nsweeps = {int(records[0]["sweeps"])}\n')
            f.write(f'likelihood evaluations = {rows}\nseed = {int(records[0]["seed"])}\n')
            f.write(f'particles = {sum(int(r["particles"]) for r in records)}\ness = {float(records[0]["ess_target"])!r}\n')
        f.write(f'replicas = {R}\n')
        for k, r in enumerate(records):
            f.write(f'replica {k} = {float(r["log_z"])!r} {float(r["err"])!r}\n')
        if kind == 'smc':
            f.write(f'log(Z) scatter = {merged["scatter"]!r}\n')
            for k, r in enumerate(records):
                f.write(f'beta {k} = {_floats(r["stage_beta"])}\n')
    return [txt, pn, stats]


def read_stats(path):
    """``name.stats`` of a run with replicas back as a dict: whole numbers as ints, other single numbers as floats, several
    numbers on a line as a list of floats; ``replica <r>`` lines gathered as ``log(Z) replicas`` and ``log(Z) error replicas``,
    ``Rhat <parameter>`` lines as the dict ``Rhat``, the other numbered lines (``beta <r>``, ``acceptance fraction <r>``,
    ``autocorrelation time <r>``) as lists indexed by replica."""
    out, per = {}, {}
    for line in Path(path).read_text().splitlines():
        key, _, val = line.partition(' = ')
        parts = val.split()
        if key.startswith('Rhat '):
            out.setdefault('Rhat', {})[key[5:]] = float(val)
            continue
        head, _, tail = key.rpartition(' ')
        if head and tail.isdigit():
            vals = [float(v) for v in parts]
            per.setdefault(head, {})[int(tail)] = vals[0] if head == 'acceptance fraction' else vals
            continue
        if len(parts) != 1:
            out[key] = [float(v) for v in parts]
        else:
            try:
                out[key] = int(val)
            except ValueError:
                out[key] = float(val)
    for head, by_rank in per.items():
        vals = [by_rank[k] for k in sorted(by_rank)]
        if head == 'replica':
            out['log(Z) replicas'] = [v[0] for v in vals]
            out['log(Z) error replicas'] = [v[1] for v in vals]
        else:
            out[head] = vals
    return out


# ------------------------------------------------------------------ running replicas
def ranks_from_environment(rank=None, world_size=None):
    """(rank, world size, local rank): the arguments, else ``RANK`` / ``WORLD_SIZE`` / ``LOCAL_RANK`` as torchrun sets them, else
    one process."""
    rank = int(os.environ.get('RANK', '0')) if rank is None else int(rank)
    world = int(os.environ.get('WORLD_SIZE', '1')) if world_size is None else int(world_size)
    local = int(os.environ.get('LOCAL_RANK', str(rank)))
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f'rank {rank} of {world}')
    return rank, world, local


def device_of(local_rank):
    """``LOCAL_RANK % torch.cuda.device_count()`` - counting devices does not touch the GPU; the local rank where there is none."""
    import torch
    count = torch.cuda.device_count()
    return local_rank % count if count > 0 else local_rank


class Group:
    """The process group of the ranks: gloo, barriers and one object gather; nothing of it with one rank."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        if world > 1:
            import torch.distributed as dist
            if not dist.is_initialized():
                os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
                os.environ.setdefault('MASTER_PORT', '29556')
                dist.init_process_group('gloo', rank=rank, world_size=world)

    def barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()

    def gather(self, item):
        if self.world == 1:
            return [item]
        import torch.distributed as dist
        out = [None] * self.world
        dist.all_gather_object(out, item)
        return out


class ReplicaRun:
    """What :func:`run_replicas` returns on every rank: ``replicas`` R, ``block`` (lo, hi) of this rank, ``samplers`` and
    ``records`` of its own replicas, ``counts`` [(replicas, likelihood rows or proposals, seconds)] of all ranks, and on rank 0
    ``merged`` (:func:`merge`) and ``files``."""

    def __init__(self, **kw):
        self.merged = self.files = None
        self.__dict__.update(kw)

    def summary(self):
        work = sum(c[1] for c in self.counts)
        line = (f'{self.replicas} replicas on {len(self.counts)} rank(s): {work} likelihood evaluations, slowest rank '
                f'{max(c[2] for c in self.counts):.2f} s')
        if self.merged is not None and 'log_z' in self.merged:
            line = f'log(Z) = {self.merged["log_z"]:.4f} +- {self.merged["err"]:.4f}, ' + line
        elif self.merged is not None:
            line = 'R-hat - 1 at most ' + f'{np.nanmax(self.merged["rhat"]) - 1.0:.4f}, ' + line
        return line


def run_replicas(vega, cfg, sample_params, group, print_func=print):
    """Replicas ``shard_bounds(R, world, rank)`` of the configured sampler one after the other on ``vega`` (replica r: the
    settings ``cfg`` with ``stream = r``), one record file each; after a barrier rank 0 merges all R records - read back from
    their files, whoever wrote them - and writes the final files."""
    R = int(cfg.get('replicas', 1))
    lo, hi = shard_bounds(R, group.world, group.rank)
    t0 = time.perf_counter()
    samplers, records, work = [], [], 0
    ready = []
    if cfg.get('together', False) and cfg['sampler'] == 'Ensemble' and hi > lo:
        # the rank's replicas as one set: their half-steps decided together, their rows one stream of full batches for the engine
        both = E.EnsembleSet(vega, hi - lo, cfg['walkers'], streams=range(lo, hi), a=cfg['a'], seed=cfg['seed'], thin=cfg['thin'],
                             driver=cfg['driver'], sample_params=sample_params, **E.moves_arguments(cfg), **E.chain_arguments(cfg))
        E.advance_sampler(both, cfg)
        if 'converge' in cfg:       # (the rank's set stops as one: its record beside the chain files)
            E.write_convergence(both, cfg['path'], cfg['name'] if group.world == 1 else f'{cfg["name"]}_rank{group.rank}')
        ready = [both.member(k) for k in range(hi - lo)]
    if cfg.get('together', False) and cfg['sampler'] == 'SMC' and hi > lo:
        # the rank's replicas as one set: one host round per stage for all of them, their rows one stream of full batches
        from .smc import SMCSet
        both = SMCSet(vega, hi - lo, particles=cfg['particles'], streams=range(lo, hi), ess=cfg['ess'], sweeps=cfg['sweeps'],
                      seed=cfg['seed'], driver=cfg['driver'], max_stages=cfg['max_stages'], sample_params=sample_params)
        both.run()
        for k in range(hi - lo):        # (a single run that cannot go on raises: so does the set)
            if both.status[k] in (2, 3):
                raise ValueError(f'SMC: replica {lo + k} cannot go on (status {int(both.status[k])}): '
                                 + ('no particle has a finite log-likelihood' if both.status[k] == 2 else
                                    'the temperature ladder cannot advance: fewer than ess N particles carry weight'))
        ready = [both.member(k) for k in range(hi - lo)]
    if cfg.get('together', False) and cfg['sampler'] == 'Nested' and hi > lo:
        # the rank's replicas as one set: one host wait per set round for all of them, their requests packed into one stream of rows
        from .nested import NestedSet
        both = NestedSet(vega, hi - lo, num_live=cfg['num_live'], num_repeats=cfg['num_repeats'], threads=cfg['threads'],
                         precision=cfg['precision'], seed=cfg['seed'], streams=range(lo, hi), driver=cfg['driver'],
                         max_iterations=cfg['max_iterations'], sample_params=sample_params)
        both.run()
        for k in range(hi - lo):        # (a single run without a finite live lnL cannot be weighed: neither can the set's)
            if both.status[k] == 2:
                raise ValueError(f'Nested: replica {lo + k} cannot go on: no live point has a finite log-likelihood')
        ready = [both.member(k) for k in range(hi - lo)]
    for r in range(lo, hi):
        if ready:
            sampler = ready[r - lo]
        else:
            sampler = E.build_sampler(vega, cfg, sample_params, stream=r)
            E.advance_sampler(sampler, cfg)
        rec = record_of(sampler, cfg.get('derived', False), print_func)
        save_record(record_path(cfg['path'], cfg['name'], r), rec)
        samplers.append(sampler)
        records.append(rec)
        work += int(sampler.stats.get('rows', sampler.stats.get('proposals', 0)))
    seconds = time.perf_counter() - t0
    sys.stdout.flush()
    group.barrier()
    counts = group.gather((hi - lo, work, seconds))
    out = ReplicaRun(replicas=R, block=(lo, hi), samplers=samplers, records=records, counts=counts)
    if group.rank == 0:
        every = [load_record(record_path(cfg['path'], cfg['name'], r)) for r in range(R)]
        out.merged = merge(every)
        out.files = write_merged(cfg['path'], cfg['name'], every, out.merged)
    group.barrier()
    return out
