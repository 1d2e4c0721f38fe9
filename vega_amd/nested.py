"""Evidence and a weighted posterior: nested sampling (Skilling 2006) by slice sampling in the whitened unit cube, run where the
live points are.

The reference samples through PolyChord (bin/run_vega_mpi.py: ``[control] run_sampler = True``, ``sampler = Polychord``) and
takes away ``log Z +- err`` with a weighted posterior.  Here an iteration kills the K live points of lowest lnL, whitens with the
survivors' covariance, and lets K threads each walk ``num_repeats`` slice steps from a random survivor under the hard constraint
lnL > L*; the K end points replace the dead.  Every thread asks for one likelihood at a time, so a round is one batch of at most K
rows for the engine.  The ``device`` driver keeps live points, threads and bookkeeping on the GPU (include/vegamx.h:
vmx_nested_run); the ``python`` driver is the readable restatement in NumPy over ``VegaInterface.chi2_batch_device``.  Both follow
vega_amd/csrc/vmx_nested.h decision for decision, so that they produce the same dead record bit for bit.  Evidence, information
and termination are computed here, on the host, from the dead record - one code for both drivers.

``clustering`` (the reference's ``do_clustering``) splits the survivors of every iteration into clusters by mutual nearest
neighbours, whitens each on its own and keeps persistent ids, so that separated modes get factors that fit them, local evidences
(:meth:`NestedRun.clusters`) and chains of their own (``cluster_posteriors``).

``boost_posterior`` (the reference's key) keeps the accepted points inside the threads' walks - each a uniform draw from its
iteration's contour that the engine has already evaluated - as a phantom record beside the dead one and merges them into the
weighted chain (:func:`boosted_weights`); the evidence and its error stay those of the base run.  A set of runs
(:class:`NestedSet`, ``boost_posterior``) keeps one phantom record per run - on the device through vmx_nested_run_many_phantoms -
and replicas merge with their phantoms (:func:`vega_amd.replicas.merge_nested_boosted`); the ``[Nested]`` settings still refuse
``boost_posterior > 0`` with ``mocks``, ``together`` and ``replicas > 1``: sets and merges are boosted through Python.

What is not here: resume files; clustering in sets; ``boost_posterior`` for per-cluster chains.  The reference's other sampler, pocoMC, has its counterpart in vega_amd/smc.py.
"""
import math
import time
from pathlib import Path

import numpy as np

from . import ensemble as E

MAXN = 32
MAX_LIVE = 4096
MAX_STEP_OUT = 32
MAX_SHRINK = 64
WIDTH = 2.0
S_NEXT, S_LEFT, S_RIGHT, S_SHRINK, S_DONE = range(5)
KNN = 8
MAX_CLUSTERS = 8
# boost: the phantom record of one driver call is allocated at its capacity, on the host and on the device; this many bytes at the
# most (at n = 32 with the defaults - 384 threads, 160 repeats, 18 MB an iteration - 11 iterations a call)
PHANTOM_BUDGET = 200 * 1000 * 1000


def phantom_row_bytes(n):
    """u [n], lnL, birth; iteration (int64), thread, repeat, cluster (int32)."""
    return 8 * (n + 2) + 8 + 3 * 4


# ------------------------------------------------------------------ the algorithm (vmx_nested.h) in NumPy
def _blocks(k, t, j, last, seed, stream):
    """Philox blocks of the counters (k, t, j, last) (k, j arrays of one shape): [..., 4] uint64."""
    k = np.asarray(k, dtype=np.uint64)
    ctr = np.zeros(k.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = k
    ctr[..., 1] = np.uint64(t)
    ctr[..., 2] = np.asarray(j, dtype=np.uint64)
    ctr[..., 3] = np.uint64(last)
    return E.philox4x64_10(ctr, (int(seed), int(stream)))


def thread_blocks(k, t, j, seed, stream=0):
    return _blocks(k, t, j, 1, seed, stream)


def draw_live(nlive, n, seed, stream=0):
    """The initial live points [nlive, n] in the unit cube: coordinate c of point i from word c % 4 of block (i, 0, c / 4, 2)."""
    nb = (n + 3) // 4
    i = np.repeat(np.arange(nlive)[:, None], nb, axis=1)
    j = np.repeat(np.arange(nb)[None, :], nlive, axis=0)
    return E.u01(_blocks(i, 0, j, 2, seed, stream).reshape(nlive, nb * 4)[:, :n])


def map_cube(lo, hi, u):
    w = hi - lo
    p = w * u
    return lo + p


def lnl_of(status, chi2, log_norm):
    chi2 = np.asarray(chi2, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(E.model_ok(status, chi2), E.log_lik(log_norm, chi2), -np.inf)


def rank_live(lnl):
    """rank_i = #{j : lnL_j < lnL_i, or lnL_j == lnL_i and j < i}."""
    order = np.argsort(lnl, kind='stable')
    rank = np.empty(len(lnl), dtype=np.int32)
    rank[order] = np.arange(len(lnl), dtype=np.int32)
    return rank


def _sum_in_order(terms):
    """Sum over axis 0 with one accumulator per entry, in order, from 0.0 (np.sum would add pairwise)."""
    return np.add.accumulate(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms]), axis=0)[-1]


def mean_cov(u_surv):
    m = u_surv.shape[0]
    mean = _sum_in_order(u_surv) / float(m)
    dev = u_surv - mean
    cov = _sum_in_order(dev[:, :, None] * dev[:, None, :]) / float(m - 1)
    return mean, cov


def cholesky(cov):
    """The lower factor column by column as vmx_ns::cholesky computes it, or None when a pivot is not positive."""
    n = cov.shape[0]
    C = np.zeros((n, n))
    for j in range(n):
        s = cov[j, j]
        for k in range(j):
            s = s - C[j, k] * C[j, k]
        if not s > 0.0:
            return None
        piv = np.sqrt(s)
        C[j, j] = piv
        if j + 1 < n:
            t = cov[j + 1:, j].copy()
            for k in range(j):
                t = t - C[j + 1:, k] * C[j, k]
            C[j + 1:, j] = t / piv
    return C


def whiten(cov):
    """(the factor an iteration uses, whether it is the Cholesky factor)."""
    C = cholesky(cov)
    if C is not None:
        return C, True
    d = np.diag(cov)
    return np.diag(np.where(d > 0.0, np.sqrt(np.where(d > 0.0, d, 0.0)), 0.0)), False


# ---- clustering of the survivors (vmx_nested.h: "clustering")
def nearest_neighbours(u):
    """(nn [m, KNN] int32: every point's nearest others by (d2, position), -1 where m - 1 < KNN; d2 [m, m] with +inf on the
    diagonal), d2 accumulated coordinate by coordinate from 0.0."""
    m, n = u.shape
    d2 = np.zeros((m, m))
    for a in range(n):
        diff = u[:, None, a] - u[None, :, a]
        d2 = d2 + diff * diff
    d2[np.arange(m), np.arange(m)] = np.inf
    kk = min(KNN, m - 1)
    nn = np.full((m, KNN), -1, dtype=np.int32)
    nn[:, :kk] = np.argsort(d2, axis=1, kind='stable')[:, :kk]
    return nn, d2


def link_levels(nn):
    """[m, KNN]: the smallest k at which a point and its q-th neighbour are linked (each among the other's first k), KNN + 1: at
    none."""
    m = nn.shape[0]
    there = nn >= 0
    back = (nn[np.where(there, nn, 0)] == np.arange(m)[:, None, None]) & there[:, :, None]       # [m, q, r]: nn[nn[i, q], r] == i
    r = np.argmax(back, axis=2)
    return np.where(back.any(axis=2), np.maximum(np.arange(KNN)[None, :], r) + 1, KNN + 1)


def components(nn, levels, k, label=None):
    """The smallest position of every point's connected component under the links of level <= k (min-label propagation with
    pointer jumping to its fixed point, which no schedule changes)."""
    m = nn.shape[0]
    i, q = np.nonzero(levels <= k)
    j = nn[i, q]
    label = np.arange(m) if label is None else label.copy()
    while True:
        new = label.copy()
        np.minimum.at(new, i, label[j])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def cluster_points(u, prev_id, next_id):
    """The clusters of the points ``u`` [m, n] with previous ids ``prev_id`` [m] (0: none): dict(nn, k (the level used), label
    (raw), n_clusters, slot [m] (every point's cluster, by its place in the order), sizes, cluster_id [n_clusters], ids [m],
    next_id, mean [n_clusters, n], cov, C [n_clusters, n, n], cholesky [n_clusters])."""
    u = np.asarray(u, dtype=np.float64)
    prev_id = np.asarray(prev_id, dtype=np.int32)
    m, n = u.shape
    nn, d2 = nearest_neighbours(u)
    levels = link_levels(nn)
    label, before, k = None, 0, 2
    while True:
        label = components(nn, levels, k, label)
        count = int(np.sum(label == np.arange(m)))
        if (k >= 3 and count == before) or k == KNN:
            break
        before, k = count, k + 1
    roots, sizes = np.unique(label, return_counts=True)
    big = sizes >= 2 * n + 2
    roots, sizes = roots[big], sizes[big]
    order = np.lexsort((roots, -sizes))[:MAX_CLUSTERS]
    roots = roots[order]
    if roots.size == 0:
        slot = np.zeros(m, dtype=np.int32)
        nc = 1
    else:
        nc = roots.size
        slot = np.full(m, -1, dtype=np.int32)
        for c, r in enumerate(roots):
            slot[label == r] = c
        loose, held = np.flatnonzero(slot < 0), np.flatnonzero(slot >= 0)
        if loose.size:      # (argmin: the first of equal distances, the lowest position)
            slot[loose] = slot[held[np.argmin(d2[np.ix_(loose, held)], axis=1)]]
    cluster_id = np.zeros(nc, dtype=np.int32)
    for c in range(nc):
        had = prev_id[(slot == c) & (prev_id != 0)]
        pick = 0
        if had.size:
            ids, counts = np.unique(had, return_counts=True)
            pick = int(ids[np.argmax(counts)])
        if pick == 0 or pick in cluster_id[:c]:
            pick, next_id = next_id, next_id + 1
        cluster_id[c] = pick
    mean, cov, C, ok = np.zeros((nc, n)), np.zeros((nc, n, n)), np.zeros((nc, n, n)), np.zeros(nc, dtype=bool)
    for c in range(nc):
        mean[c], cov[c] = mean_cov(u[slot == c])
        C[c], ok[c] = whiten(cov[c])
    return dict(nn=nn, k=k, label=label, n_clusters=nc, slot=slot, sizes=np.bincount(slot, minlength=nc), cluster_id=cluster_id,
                ids=cluster_id[slot], next_id=int(next_id), mean=mean, cov=cov, C=C, cholesky=ok)


class ClusterState:
    """What clustering adds to a run's state: ``live_cluster`` [nlive] int32 (0: never labelled), ``next_id``, and the ids of the
    dead of every call (``dead``, one array per call)."""

    def __init__(self, nlive):
        self.live_cluster = np.zeros(nlive, dtype=np.int32)
        self.next_id = 1
        self.dead = []


def iteration_head(live_u, live_lnl, K, t, seed, stream=0, clusters=None):
    """Kill, whiten and choose the starts of iteration ``t``: dict(rank, killed [K] in order of death, lstar, surv (live indices
    of the survivors in order), mean, cov, C, cholesky, start [K] (live index each thread starts from)).  With ``clusters`` (a
    :class:`ClusterState`, whose survivors' ids and ``next_id`` move on): mean, cov, C, cholesky per cluster, ``cluster``
    (:func:`cluster_points` of the survivors), ``dead_cluster`` [K], ``start_slot`` [K] and ``C_thread`` [K, n, n]."""
    nlive = live_u.shape[0]
    rank = rank_live(live_lnl)
    killed = np.empty(K, dtype=np.int64)
    dying = np.flatnonzero(rank < K)
    killed[rank[dying]] = dying
    surv = np.flatnonzero(rank >= K)
    ks = np.arange(K)
    choice = E.partner(thread_blocks(ks, t, np.zeros(K, dtype=np.int64), seed, stream)[:, 0], nlive - K).astype(np.int64)
    if clusters is not None:
        cl = cluster_points(live_u[surv], clusters.live_cluster[surv], clusters.next_id)
        dead_cluster = clusters.live_cluster[killed].copy()
        clusters.live_cluster[surv] = cl['ids']
        clusters.next_id = cl['next_id']
        return dict(rank=rank, killed=killed, lstar=live_lnl[killed[K - 1]], surv=surv, mean=cl['mean'], cov=cl['cov'], C=cl['C'],
                    cholesky=cl['cholesky'], start=surv[choice], cluster=cl, dead_cluster=dead_cluster,
                    start_slot=cl['slot'][choice], C_thread=cl['C'][cl['slot'][choice]])
    mean, cov = mean_cov(live_u[surv])
    C, ok = whiten(cov)
    return dict(rank=rank, killed=killed, lstar=live_lnl[killed[K - 1]], surv=surv, mean=mean, cov=cov, C=C, cholesky=ok,
                start=surv[choice])


# ---- boost: the accepted points inside a walk (vmx_nested.h "boost")
def boost_fraction(boost_posterior, num_repeats):
    """f = min(1, b / num_repeats): one cannot boost by more than num_repeats."""
    return min(1.0, float(boost_posterior) / float(num_repeats))


def phantom_of(state_before, inside_before, answer, lstar, repeat_after, num_repeats):
    """vmx_ns::phantom_of on arrays: the index r of the phantom point the last advance produced, 0: none."""
    with np.errstate(invalid='ignore'):
        accepted = (state_before == S_SHRINK) & inside_before & (answer > lstar)
    return np.where(accepted & (repeat_after < num_repeats), repeat_after, 0).astype(np.int32)


def phantom_kept(k, t, r, f, seed, stream=0):
    """vmx_ns::phantom_kept: u01(word 0 of the Philox block (k, t, r, 3)) < f."""
    return E.u01(_blocks(k, t, r, 3, seed, stream)[..., 0]) < f


class PhantomState:
    """What boost adds to a run's state: the fraction f and the kept phantom points of every call (one dict per call, in the
    canonical order): ``u`` [N, n], ``lnl``, ``birth`` [N], ``tag`` [N, 3] int64 (iteration, thread, repeat), ``cluster`` [N]
    int32 (a run with clustering; else None)."""

    def __init__(self, fraction):
        self.fraction = float(fraction)
        if not 0.0 <= self.fraction <= 1.0:
            raise ValueError('the kept fraction of the phantom points: 0 .. 1')
        self.calls = []

    def append(self, u, lnl, birth, tag, cluster=None):
        """The points of one call, in any order: they are put into the canonical one first."""
        tag = np.asarray(tag, dtype=np.int64).reshape(-1, 3)
        order = np.lexsort((tag[:, 2], tag[:, 1], tag[:, 0]))
        self.calls.append(dict(u=np.asarray(u, dtype=np.float64)[order], lnl=np.asarray(lnl, dtype=np.float64)[order],
                               birth=np.asarray(birth, dtype=np.float64)[order], tag=tag[order],
                               cluster=None if cluster is None else np.asarray(cluster, dtype=np.int32)[order]))

    def record(self, n):
        if not self.calls:
            return dict(u=np.empty((0, n)), lnl=np.empty(0), birth=np.empty(0), tag=np.empty((0, 3), dtype=np.int64), cluster=None)
        out = {key: np.concatenate([c[key] for c in self.calls]) for key in ('u', 'lnl', 'birth', 'tag')}
        out['u'] = out['u'].reshape(-1, n)
        out['cluster'] = None if self.calls[0]['cluster'] is None else np.concatenate([c['cluster'] for c in self.calls])
        return out


class Threads:
    """The K state machines of an iteration (vmx_ns::Thread as arrays); ``C`` [n, n], or [K, n, n]: a factor per thread."""

    def __init__(self, u, lnl, C, lstar, t, num_repeats, seed, stream=0):
        K, n = u.shape
        self.K, self.n = K, n
        self.x, self.y, self.d = u.copy(), u.copy(), np.zeros((K, n))
        self.lnl = np.array(lnl, dtype=np.float64)
        self.L, self.R, self.t = np.zeros(K), np.zeros(K), np.zeros(K)
        self.draw = np.ones(K, dtype=np.int64)
        self.state = np.full(K, S_NEXT, dtype=np.int32)
        self.repeat, self.n_out, self.n_shrink = (np.zeros(K, dtype=np.int32) for _ in range(3))
        self.inside = np.ones(K, dtype=bool)
        self.C, self.lstar, self.iteration, self.num_repeats, self.seed, self.stream = C, lstar, t, num_repeats, seed, stream

    def _trial(self, ix):
        if ix.size == 0:
            return
        p = self.t[ix, None] * self.d[ix]
        v = self.x[ix] + p
        self.y[ix] = v
        self.inside[ix] = np.all((v >= 0.0) & (v <= 1.0), axis=1)

    def _new_direction(self, ix):
        n, nb = self.n, self.n // 4 + 1
        j = self.draw[ix][:, None] + np.arange(nb)[None, :]
        k = np.repeat(ix[:, None], nb, axis=1)
        u = E.u01(thread_blocks(k, self.iteration, j, self.seed, self.stream).reshape(ix.size, nb * 4)[:, :n + 1])
        self.draw[ix] += nb
        two = 2.0 * u[:, :n]
        g = two - 1.0
        r = u[:, n]
        s = np.zeros(ix.size)
        for i in range(n):
            s = s + g[:, i] * g[:, i]
        nrm = np.sqrt(s)
        bad = ~(nrm > 0.0)
        g[bad, 0] = 1.0
        nrm[bad] = 1.0
        g = g / nrm[:, None]
        d = np.zeros((ix.size, n))
        for jj in range(n):         # (d_i accumulates C_ij g_j in the order j = 0 .. i)
            col = self.C[jj:, jj][None, :] if self.C.ndim == 2 else self.C[ix][:, jj:, jj]
            d[:, jj:] = d[:, jj:] + col * g[:, jj][:, None]
        self.d[ix] = d
        rw = r * WIDTH
        self.L[ix] = -rw
        q1 = 1.0 - r
        self.R[ix] = q1 * WIDTH

    def _draw_trial(self, ix):
        if ix.size == 0:
            return
        u = E.u01(thread_blocks(ix, self.iteration, self.draw[ix], self.seed, self.stream)[:, 0])
        self.draw[ix] += 1
        wid = self.R[ix] - self.L[ix]
        p = wid * u
        self.t[ix] = self.L[ix] + p
        self._trial(ix)

    def advance(self, answer):
        """vmx_ns::advance of every thread with the lnL ``answer`` [K] of its last request: the mask of threads that ask again
        (their request: ``requests``)."""
        was = self.state.copy()
        with np.errstate(invalid='ignore'):
            ok = self.inside & (answer > self.lstar)
        more = ok & (self.n_out < MAX_STEP_OUT)
        a = np.flatnonzero((was == S_LEFT) & more)
        b = np.flatnonzero((was == S_LEFT) & ~more)
        self.L[a] = self.L[a] - WIDTH
        self.n_out[a] += 1
        self.t[a] = self.L[a]
        self.state[b] = S_RIGHT
        self.n_out[b] = 0
        self.t[b] = self.R[b]
        a2 = np.flatnonzero((was == S_RIGHT) & more)
        b2 = np.flatnonzero((was == S_RIGHT) & ~more)
        self.R[a2] = self.R[a2] + WIDTH
        self.n_out[a2] += 1
        self.t[a2] = self.R[a2]
        self._trial(np.concatenate([a, b, a2]))
        self.state[b2] = S_SHRINK
        self.n_shrink[b2] = 0
        acc = np.flatnonzero((was == S_SHRINK) & ok)
        self.x[acc] = self.y[acc]
        self.lnl[acc] = answer[acc]
        rej = (was == S_SHRINK) & ~ok
        neg = np.flatnonzero(rej & (self.t < 0.0))
        pos = np.flatnonzero(rej & ~(self.t < 0.0))
        self.L[neg] = self.t[neg]
        self.R[pos] = self.t[pos]
        self.n_shrink[rej] += 1
        again = np.flatnonzero(rej & (self.n_shrink < MAX_SHRINK))
        gave_up = np.flatnonzero(rej & ~(self.n_shrink < MAX_SHRINK))
        ended = np.concatenate([acc, gave_up])
        self.repeat[ended] += 1
        self.state[ended] = S_NEXT
        self._draw_trial(np.sort(np.concatenate([b2, again])))
        nxt = self.state == S_NEXT
        fin = np.flatnonzero(nxt & (self.repeat >= self.num_repeats))
        self.state[fin] = S_DONE
        self.inside[fin] = True
        go = np.flatnonzero(nxt & (self.repeat < self.num_repeats))
        if go.size:
            self._new_direction(go)
            self.state[go] = S_LEFT
            self.n_out[go] = 0
            self.t[go] = self.L[go]
            self._trial(go)
        return (was != S_DONE) & (self.state != S_DONE)

    def requests(self, asks):
        """Rows [R, n] in the cube the asking threads want evaluated (a thread whose point left the cube asks for its own
        position), and how many of them are such."""
        ks = np.flatnonzero(asks)
        return ks, np.where(self.inside[ks, None], self.y[ks], self.x[ks]), int((~self.inside[ks]).sum())


def python_iterations(live_u, live_lnl, iteration, n_iterations, K, num_repeats, seed, stream, evaluate, stop=None, clusters=None,
                      boost=None):
    """Up to ``n_iterations`` iterations in NumPy from the state ``live_u`` [nlive, n], ``live_lnl`` [nlive] (updated in place).
    ``evaluate(rows_u)`` -> lnL [R] of rows in the cube (-inf: a failed model).  ``stop(iterations, dead_lnl, live_lnl)`` as for
    the device driver.  ``clusters``: a :class:`ClusterState` turns clustering on (updated in place; the ids of this call's dead
    are appended to its ``dead``).  ``boost``: a :class:`PhantomState` records the kept phantom points of this call (appended to
    it; the run itself is the same run).  Returns (dead_u, dead_lnl, dead_nlive, iteration, stats)."""
    nlive, n = live_u.shape
    dead_u, dead_lnl, dead_n, dead_c = [], [], [], []
    if boost is not None and boost.fraction == 0.0:
        boost = None
    ph = dict(u=[], lnl=[], birth=[], tag=[], cluster=[])
    st = dict(iterations=0, rounds=0, rows=0, rows_own_position=0)
    for _ in range(n_iterations):
        head = iteration_head(live_u, live_lnl, K, iteration, seed, stream, clusters)
        killed = head['killed']
        dead_u.append(live_u[killed].copy())
        dead_lnl.append(live_lnl[killed].copy())
        dead_n.append(nlive - np.arange(K, dtype=np.int32))
        if clusters is not None:
            dead_c.append(head['dead_cluster'])
        T = Threads(live_u[head['start']], live_lnl[head['start']], head['C'] if clusters is None else head['C_thread'],
                    head['lstar'], iteration, num_repeats, seed, stream)
        answer = np.full(K, -np.inf)
        asks = T.advance(answer)
        while asks.any():
            ks, rows, own = T.requests(asks)
            answer = np.full(K, -np.inf)
            answer[ks] = evaluate(rows)
            st['rounds'] += 1
            st['rows'] += ks.size
            st['rows_own_position'] += own
            if boost is None:
                asks = T.advance(answer)
            else:
                was, inside = T.state.copy(), T.inside.copy()
                asks = T.advance(answer)
                r = phantom_of(was, inside, answer, T.lstar, T.repeat, num_repeats)
                kp = np.flatnonzero(r > 0)
                kp = kp[phantom_kept(kp, iteration, r[kp], boost.fraction, seed, stream)]
                if kp.size:
                    ph['u'].append(T.x[kp].copy())
                    ph['lnl'].append(T.lnl[kp].copy())
                    ph['birth'].append(np.full(kp.size, head['lstar'], dtype=np.float64))
                    ph['tag'].append(np.stack([np.full(kp.size, iteration, dtype=np.int64), kp.astype(np.int64),
                                               r[kp].astype(np.int64)], axis=1))
                    if clusters is not None:
                        ph['cluster'].append(head['cluster']['cluster_id'][head['start_slot'][kp]].astype(np.int32))
        live_u[killed] = T.x
        live_lnl[killed] = T.lnl
        if clusters is not None:
            clusters.live_cluster[killed] = head['cluster']['cluster_id'][head['start_slot']]
        iteration += 1
        st['iterations'] += 1
        if stop is not None and stop(iteration, dead_lnl[-1], live_lnl):
            break
    if clusters is not None:
        clusters.dead.append(np.concatenate(dead_c) if dead_c else np.empty(0, dtype=np.int32))
    if boost is not None:
        cat = {key: (np.concatenate(val) if val else None) for key, val in ph.items()}
        boost.append(cat['u'] if cat['u'] is not None else np.empty((0, n)), *(cat[key] if cat[key] is not None else np.empty(0)
                                                                                for key in ('lnl', 'birth')),
                     cat['tag'] if cat['tag'] is not None else np.empty((0, 3), dtype=np.int64),
                     None if clusters is None else (cat['cluster'] if cat['cluster'] is not None else np.empty(0, dtype=np.int32)))
    if not dead_u:
        return np.empty((0, n)), np.empty(0), np.empty(0, dtype=np.int32), iteration, st
    return np.concatenate(dead_u), np.concatenate(dead_lnl), np.concatenate(dead_n), iteration, st


# ------------------------------------------------------------------ a set of runs (vmx_nested.h: "a set of runs")
HEAD, WALK, OUT = 0, 1, 2
GOING, STOPPED, NO_FINITE = 0, 1, 2


def first_active(status, n_iterations):
    """vmx_ns::first_active: (the runs a call begins with, ascending; the phase of every run)."""
    phase = np.where((np.asarray(status) == GOING) & (n_iterations > 0), HEAD, OUT).astype(np.int32)
    return [int(e) for e in np.flatnonzero(phase != OUT)], phase


def heading_list(active, phase):
    """vmx_ns::heading_list: the active runs whose next iteration has to be headed, in the list's order."""
    return [e for e in active if phase[e] == HEAD]


def row_offsets(count):
    """vmx_ns::row_offsets: (the first engine row of every active run, the total) from the runs' request counts in list order."""
    offset, total = [], 0
    for c in count:
        offset.append(total)
        total += int(c)
    return offset, total


def after_iteration(stopped, done, n_iterations):
    """vmx_ns::after_iteration: (the phase, the status) of a run whose iteration has just ended."""
    if stopped:
        return OUT, STOPPED
    return (OUT if done >= n_iterations else HEAD), GOING


def compact_active(active, phase):
    """vmx_ns::compact_active: the runs not OUT keep their order and move up."""
    return [e for e in active if phase[e] != OUT]


def set_iterations_per_call(runs, K, num_repeats, n, boost):
    """Iterations per call of a set's driver: the dead record of a call is allocated up front (65536 // K), and with ``boost``
    the phantom records of all ``runs`` runs at their capacity K (num_repeats - 1) rows per run and iteration
    (vmx_ns::set_phantom_capacity) stay under PHANTOM_BUDGET bytes together; 0: not even one iteration fits."""
    per_call = max(1, 65536 // K)
    if boost and num_repeats > 1:
        per_call = min(per_call, PHANTOM_BUDGET // (runs * K * (num_repeats - 1) * phantom_row_bytes(n)))
    return per_call


def python_iterations_many(live_u, live_lnl, iteration, n_iterations, K, num_repeats, seed, streams, evaluate, stop=None, draw=False,
                           watch=None, boost=None):
    """Up to ``n_iterations`` iterations of each of E runs in NumPy (vmx_nested_run_many restated over :func:`iteration_head` and
    :class:`Threads`): ``live_u`` [E, nlive, n], ``live_lnl`` [E, nlive], ``iteration`` int64 [E] the runs' state, updated in place
    (a run without a finite live lnL keeps what it had at entry), ``streams`` [E].  A set round heads the runs in HEAD, advances
    every thread of every active run by the answer of the row it asked for, packs the requests in ascending (run, thread) order
    (:func:`row_offsets`), ends the iteration of the runs that ask for nothing and hands the rows to ``evaluate(rows_u [R, n], runs
    [R])`` -> lnL [R] (``runs``: the run of every row; not called when R = 0); a run whose iteration ended is asked
    ``stop(run, iterations, dead_lnl [K], live_lnl [nlive])`` and headed again in the next round.  ``draw``: the live points are
    drawn and evaluated first.  ``watch(round, state)`` sees every round before the host's turn.  Returns (dead: per run
    (dead_u, dead_lnl, dead_nlive) of the iterations done, status int32 [E]: 0 still going, 1 stopped, 2 no live point with a
    finite lnL; iterations_done int32 [E]; statistics with ``per_run`` int64 [E, 3]: rows evaluated, own-position rows, set
    rounds the run took part in).  ``boost``: a list of E :class:`PhantomState` - run e's kept phantom points of this call are
    appended to ``boost[e]`` as :func:`python_iterations` appends a run's (vmx_nested_run_many_phantoms; the phases, lists,
    packing order and rows are the same with or without it)."""
    E, nlive, n = live_u.shape
    if boost is not None:
        if len(boost) != E:
            raise ValueError(f'boost: one PhantomState for each of the {E} runs')
        if all(b.fraction == 0.0 for b in boost):
            boost = None
    ph = [dict(u=[], lnl=[], birth=[], tag=[]) for _ in range(E)]
    entry = (live_u.copy(), live_lnl.copy())
    per = np.zeros((E, 3), dtype=np.int64)
    status = np.zeros(E, dtype=np.int32)
    done = np.zeros(E, dtype=np.int32)
    dead = [([], [], []) for _ in range(E)]
    st = dict(iterations=0, rounds=0, rows=0, rows_own_position=0)
    if draw:
        for e in range(E):
            live_u[e] = draw_live(nlive, n, seed, int(streams[e]))
        first = np.asarray(evaluate(live_u.reshape(E * nlive, n), np.repeat(np.arange(E), nlive)), dtype=np.float64).reshape(E, nlive)
        per[:, 0] += nlive
        st['rows'] += E * nlive
        for e in range(E):
            live_lnl[e] = first[e]
            status[e] = GOING if np.any(first[e] > -np.inf) else NO_FINITE
    active, phase = first_active(status, n_iterations)
    heads, T, answer = {}, {}, {}
    while active:
        heading = heading_list(active, phase)
        for e in heading:
            it = int(iteration[e]) + int(done[e])
            head = heads[e] = iteration_head(live_u[e], live_lnl[e], K, it, seed, int(streams[e]))
            killed = head['killed']
            dead[e][0].append(live_u[e][killed].copy())
            dead[e][1].append(live_lnl[e][killed].copy())
            dead[e][2].append(nlive - np.arange(K, dtype=np.int32))
            T[e] = Threads(live_u[e][head['start']], live_lnl[e][head['start']], head['C'], head['lstar'], it, num_repeats, seed,
                           int(streams[e]))
            answer[e] = np.full(K, -np.inf)
            phase[e] = WALK
        requests, count = {}, []
        for e in active:
            if boost is None or boost[e].fraction == 0.0:
                requests[e] = T[e].requests(T[e].advance(answer[e]))
            else:
                t = T[e]
                was, inside = t.state.copy(), t.inside.copy()
                asks = t.advance(answer[e])
                r = phantom_of(was, inside, answer[e], t.lstar, t.repeat, num_repeats)
                kp = np.flatnonzero(r > 0)
                kp = kp[phantom_kept(kp, t.iteration, r[kp], boost[e].fraction, seed, int(streams[e]))]
                if kp.size:     # (before the end of the iteration, should it end in this round: T.x is the accepted point)
                    ph[e]['u'].append(t.x[kp].copy())
                    ph[e]['lnl'].append(t.lnl[kp].copy())
                    ph[e]['birth'].append(np.full(kp.size, t.lstar, dtype=np.float64))
                    ph[e]['tag'].append(np.stack([np.full(kp.size, t.iteration, dtype=np.int64), kp.astype(np.int64),
                                                  r[kp].astype(np.int64)], axis=1))
                requests[e] = t.requests(asks)
            count.append(requests[e][0].size)
        offset, total = row_offsets(count)
        for e, c in zip(active, count):
            per[e, 0] += c
            per[e, 1] += requests[e][2]
            per[e, 2] += 1
            if c == 0:
                killed = heads[e]['killed']
                live_u[e][killed] = T[e].x
                live_lnl[e][killed] = T[e].lnl
        st['rounds'] += 1
        st['rows'] += total
        if watch is not None:
            watch(st['rounds'] - 1, dict(active=list(active), heading=list(heading), count=list(count), offset=list(offset), total=total,
                                         threads=T, requests=requests, phase=phase.copy()))
        if total > 0:
            lnl = np.asarray(evaluate(np.concatenate([requests[e][1] for e in active], axis=0),
                                      np.repeat(np.array(active, dtype=np.int64), count)), dtype=np.float64)
        for e, c, o in zip(active, count, offset):
            if c > 0:
                answer[e] = np.full(K, -np.inf)
                answer[e][requests[e][0]] = lnl[o:o + c]
                continue
            done[e] += 1
            stopped = stop is not None and bool(stop(e, int(iteration[e]) + int(done[e]), dead[e][1][-1], live_lnl[e]))
            phase[e], status[e] = after_iteration(stopped, int(done[e]), n_iterations)
        active = compact_active(active, phase)
    out = []
    for e in range(E):
        if status[e] == NO_FINITE:
            live_u[e], live_lnl[e] = entry[0][e], entry[1][e]
        iteration[e] += int(done[e])
        if done[e] == 0:
            out.append((np.empty((0, n)), np.empty(0), np.empty(0, dtype=np.int32)))
        else:
            out.append(tuple(np.concatenate(part) for part in dead[e]))
    if boost is not None:
        for e in range(E):
            if boost[e].fraction == 0.0:
                continue
            got = ph[e]
            boost[e].append(np.concatenate(got['u']) if got['u'] else np.empty((0, n)),
                            np.concatenate(got['lnl']) if got['lnl'] else np.empty(0),
                            np.concatenate(got['birth']) if got['birth'] else np.empty(0),
                            np.concatenate(got['tag']) if got['tag'] else np.empty((0, 3), dtype=np.int64))
    st.update(iterations=int(done.sum()), rows_own_position=int(per[:, 1].sum()), per_run=per)
    return out, status, done, st


# ------------------------------------------------------------------ evidence (host, both drivers)
def _logsumexp(a):
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return -np.inf
    m = np.max(a)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(a - m))))


def log_weights(dead_lnl, dead_nlive, live_lnl):
    """log(L_i w_i) of the dead points followed by the live ones: log X_i = log X_{i-1} - 1 / n_i, w_i = X_{i-1} - X_i, the live
    points X_end / nlive each."""
    dead_nlive = np.asarray(dead_nlive, dtype=np.float64)
    log_x = -np.cumsum(1.0 / dead_nlive)
    log_x_before = np.concatenate([[0.0], log_x[:-1]])
    log_w = log_x_before + np.log1p(-np.exp(-1.0 / dead_nlive))
    log_x_end = log_x[-1] if log_x.size else 0.0
    log_w_live = np.full(len(live_lnl), log_x_end - math.log(len(live_lnl)))
    return np.concatenate([np.asarray(dead_lnl) + log_w, np.asarray(live_lnl) + log_w_live])


def boosted_weights(dead_lnl, dead_nlive, live_lnl, ph_lnl, ph_birth):
    """The base run and the kept phantom points (lnL ``ph_lnl`` > birth contour ``ph_birth``, canonical order) merged as runs are
    merged by birth contour.  L_D: the lnL of the last death.  The events are the deaths and the phantoms with lnL <= L_D, sorted
    by (lnL, deaths before phantoms, record order); the live count of event i is m_i = b_i + a_i, b_i the death's own recorded
    count (a phantom: that of the first death in record order with lnL >= its lnL) and a_i = #{phantoms p : birth_p < lnL_i <=
    lnL_p}; log X_i = log X_{i-1} - 1 / m_i, w_i = X_{i-1} - X_i (the expressions of :func:`log_weights`).  The final live points
    and the A phantoms above L_D are all uniform in the last contour: X_end / (nlive + A) each.

    Returns (log(L w) in the order events, live points, late phantoms; ``index`` - row j of that order is row index[j] of the
    deaths, the live points and the phantoms laid end to end; log Z_boost, the log-sum).  Without phantoms: :func:`log_weights`."""
    dead_lnl, live_lnl = np.asarray(dead_lnl, dtype=np.float64), np.asarray(live_lnl, dtype=np.float64)
    ph_lnl, ph_birth = np.asarray(ph_lnl, dtype=np.float64), np.asarray(ph_birth, dtype=np.float64)
    dead_nlive = np.asarray(dead_nlive, dtype=np.float64)
    D, nl, P = dead_lnl.size, live_lnl.size, ph_lnl.size
    early = ph_lnl <= dead_lnl[-1] if D else np.zeros(P, dtype=bool)
    ev_ph, late = np.flatnonzero(early), np.flatnonzero(~early)
    ev_lnl = np.concatenate([dead_lnl, ph_lnl[ev_ph]])
    is_ph = np.concatenate([np.zeros(D, dtype=np.int8), np.ones(ev_ph.size, dtype=np.int8)])
    src = np.concatenate([np.arange(D), ev_ph])
    order = np.lexsort((src, is_ph, ev_lnl))
    x = ev_lnl[order]
    # b: a phantom takes the count of the first death in record order whose lnL is not below its own
    first = np.searchsorted(np.maximum.accumulate(dead_lnl), ph_lnl[ev_ph], side='left') if D else np.empty(0, dtype=np.int64)
    b = np.concatenate([dead_nlive, dead_nlive[first]])[order]
    # a: lnL_p > birth_p, so #{birth_p < x <= lnL_p} = #{birth_p < x} - #{lnL_p < x}
    a = np.searchsorted(np.sort(ph_birth), x, side='left') - np.searchsorted(np.sort(ph_lnl), x, side='left')
    m = b + a
    log_x = -np.cumsum(1.0 / m)
    log_x_before = np.concatenate([[0.0], log_x[:-1]])
    log_w = log_x_before + np.log1p(-np.exp(-1.0 / m))
    log_x_end = log_x[-1] if log_x.size else 0.0
    tail = np.concatenate([live_lnl, ph_lnl[late]])
    lw = np.concatenate([x + log_w, tail + (log_x_end - math.log(nl + late.size))])
    index = np.concatenate([np.where(is_ph[order] == 1, D + nl + src[order], src[order]), D + np.arange(nl), D + nl + late])
    return lw, index.astype(np.int64), _logsumexp(lw)


def evidence(dead_lnl, dead_nlive, live_lnl):
    """(log Z, H, posterior weights p_i summing to 1) over the dead points followed by the live ones."""
    lw = log_weights(dead_lnl, dead_nlive, live_lnl)
    log_z = _logsumexp(lw)
    lnl = np.concatenate([np.asarray(dead_lnl, dtype=np.float64), np.asarray(live_lnl, dtype=np.float64)])
    with np.errstate(invalid='ignore'):
        p = np.exp(lw - log_z) if np.isfinite(log_z) else np.zeros(lw.size)
    p = np.where(np.isfinite(p), p, 0.0)
    used = p > 0.0
    info = float(np.sum(p[used] * (lnl[used] - log_z))) if np.any(used) else 0.0
    return log_z, info, p


class NestedRun:
    """A nested-sampling run over ``loglike(rows_u [R, n]) -> lnL [R]`` in the unit cube (-inf: a failed model), NumPy driver: the
    live points, the dead record, termination and the evidence.  :class:`NestedSampler` puts the engine behind it.
    ``clustering``: cluster the survivors of every iteration, whiten per cluster and keep ids (:meth:`clusters`).
    ``boost_posterior`` = b >= 0 (the reference's key; 0: off): keep the fraction min(1, b / num_repeats) of the accepted points
    inside the threads' walks (:meth:`phantoms`) and merge them into :meth:`samples`; the run, its evidence and its termination
    are those of b = 0."""

    def __init__(self, loglike, n, num_live=None, num_repeats=None, threads=None, precision=1e-3, seed=0, stream=0,
                 max_iterations=None, max_batch=None, clustering=False, boost_posterior=0.0):
        self.loglike = loglike
        self.boost_posterior = float(boost_posterior)
        if not (math.isfinite(self.boost_posterior) and self.boost_posterior >= 0.0):
            raise ValueError('boost_posterior: a finite number, at least 0')
        if not isinstance(clustering, (bool, np.bool_)):
            raise ValueError('clustering: True or False')
        self.clustering = bool(clustering)
        self.n = int(n)
        self.num_live = int(num_live) if num_live is not None else 25 * self.n
        self.num_repeats = int(num_repeats) if num_repeats is not None else 5 * self.n
        if threads is None:
            top = self.num_live // 2 if max_batch is None else min(self.num_live // 2, int(max_batch))
            threads = max(1, min(top // 64 * 64 if top >= 64 else 1, self.num_live - self.n - 1))
        self.threads = int(threads)
        self.precision = float(precision)
        self.seed, self.stream = int(seed), int(stream)
        self.max_iterations = None if max_iterations is None else int(max_iterations)
        if not 1 <= self.n <= MAXN:
            raise ValueError(f'1 .. {MAXN} sampled parameters')
        if not self.n + 2 <= self.num_live <= MAX_LIVE:
            raise ValueError(f'num_live: {self.n + 2} .. {MAX_LIVE} for {self.n} sampled parameters')
        if not 1 <= self.threads <= self.num_live - self.n - 1:
            raise ValueError(f'threads: 1 .. num_live - n - 1 = {self.num_live - self.n - 1}')
        if self.num_repeats < 1:
            raise ValueError('num_repeats >= 1')
        if not self.precision > 0.0:
            raise ValueError('precision > 0')
        if self.max_iterations is not None and self.max_iterations < 1:
            raise ValueError('max_iterations >= 1')
        self.reset()

    def reset(self):
        self.live_u = self.live_lnl = None
        self.iteration = 0
        self.terminated = False
        self._to_termination = True
        self._dead_u, self._dead_lnl, self._dead_n = [], [], []
        self._log_x, self._log_z_dead = 0.0, -np.inf
        self.cluster_state = ClusterState(self.num_live) if self.clustering else None
        self.phantom_state = PhantomState(boost_fraction(self.boost_posterior, self.num_repeats)) if self.boost_posterior > 0.0 else None
        self.stats = dict(iterations=0, rounds=0, rows=0, rows_own_position=0, engine_calls=0, host_waits=0, seconds=0.0,
                          seconds_enqueuing=0.0, calls=0)

    # ---- termination (PolyChord's precision_criterion), asked after every iteration by either driver
    def _stop(self, iterations, dead_lnl, live_lnl):
        nlive = self.num_live
        with np.errstate(invalid='ignore', divide='ignore'):
            for j, lnl in enumerate(np.asarray(dead_lnl, dtype=np.float64)):
                n_j = float(nlive - j)
                self._log_z_dead = float(np.logaddexp(self._log_z_dead, lnl + self._log_x + math.log1p(-math.exp(-1.0 / n_j))))
                self._log_x -= 1.0 / n_j
            log_z_live = self._log_x + _logsumexp(live_lnl) - math.log(nlive)
            done = bool(log_z_live - np.logaddexp(self._log_z_dead, log_z_live) < math.log(self.precision))
        if self.max_iterations is not None and iterations >= self.max_iterations:
            done = True
        self.terminated = done
        return done and self._to_termination      # (iterations asked for by number are all run)

    # ---- drivers
    def _draw(self):
        self.live_u = np.ascontiguousarray(draw_live(self.num_live, self.n, self.seed, self.stream))
        self.live_lnl = np.ascontiguousarray(self._evaluate(self.live_u), dtype=np.float64)
        self.stats['rows'] += self.num_live

    def _evaluate(self, rows_u):
        return np.asarray(self.loglike(rows_u), dtype=np.float64)

    def _advance(self, n_iterations):
        """One call of the driver: (dead_u, dead_lnl, dead_nlive, statistics)."""
        if self.live_u is None:
            self._draw()
        du, dl, dn, self.iteration, st = python_iterations(self.live_u, self.live_lnl, self.iteration, n_iterations, self.threads,
                                                           self.num_repeats, self.seed, self.stream, self._evaluate, self._stop,
                                                           clusters=self.cluster_state, boost=self.phantom_state)
        return du, dl, dn, st

    def _per_call(self):
        """Iterations per call of the driver: the dead record of a call is allocated up front, and with boost the phantom record
        at its capacity threads (num_repeats - 1) rows per iteration, which stays under PHANTOM_BUDGET bytes (at least one
        iteration)."""
        per_call = max(1, 65536 // self.threads)
        if self.phantom_state is not None and self.num_repeats > 1:
            rows = self.threads * (self.num_repeats - 1)
            per_call = min(per_call, max(1, PHANTOM_BUDGET // (rows * phantom_row_bytes(self.n))))
        return per_call

    def run(self, iterations=None):
        """To termination (``iterations`` None: the precision criterion or ``max_iterations``), or exactly ``iterations`` more
        iterations, whatever the criterion says (``terminated`` still reports it); the run does not depend on how it is cut."""
        t0 = time.perf_counter()
        self._to_termination = iterations is None
        per_call = self._per_call()
        if iterations is None:
            left = self.max_iterations - self.iteration if self.max_iterations is not None else per_call
            call = min(max(0, left), per_call) if not self.terminated else 0
        else:
            call = int(iterations)
        left_asked = call
        while call > 0:
            if iterations is not None:      # (one call, as ever; with boost cut to the phantom record's budget)
                call = min(left_asked, per_call) if self.phantom_state is not None else left_asked
            du, dl, dn, st = self._advance(call)
            left_asked -= call
            self._dead_u.append(du)
            self._dead_lnl.append(dl)
            self._dead_n.append(dn)
            for key, val in st.items():
                if key in self.stats and key != 'seconds':
                    self.stats[key] += val
            self.stats['calls'] += 1
            if iterations is not None:
                if left_asked <= 0 or st['iterations'] == 0:
                    break
                continue
            if self.terminated or st['iterations'] == 0:
                break
            if self.max_iterations is not None:
                call = min(per_call, self.max_iterations - self.iteration)
        self.stats['seconds'] += time.perf_counter() - t0
        return self

    # ---- results
    def dead(self):
        """The dead record: (u [N, n], lnL [N], live count [N])."""
        if not self._dead_u:
            return np.empty((0, self.n)), np.empty(0), np.empty(0, dtype=np.int32)
        return np.concatenate(self._dead_u), np.concatenate(self._dead_lnl), np.concatenate(self._dead_n)

    def _evidence(self):
        if self.live_u is None:
            raise ValueError('nothing has run yet')
        _, dl, dn = self.dead()
        return evidence(dl, dn, self.live_lnl)

    def log_evidence(self):
        """(log Z, its error sqrt(H / num_live))."""
        log_z, info, _ = self._evidence()
        return log_z, math.sqrt(max(info, 0.0) / self.num_live)

    def information(self):
        return self._evidence()[1]

    def to_physical(self, u):
        return u

    def phantoms(self):
        """The kept phantom points in the canonical order (ascending iteration, thread, repeat), a dict: ``u`` [N, n] in the cube,
        ``lnl`` [N], ``birth`` [N] (the L* they were accepted under), ``tag`` [N, 3] int64 (iteration, thread, repeat),
        ``cluster`` [N] int32 in a run with clustering (the id the thread's end point inherits), else None."""
        if self.phantom_state is None:
            raise ValueError('the run keeps no phantom points (boost_posterior > 0)')
        return self.phantom_state.record(self.n)

    def _boosted(self):
        """(log(L w), index, log Z_boost) of :func:`boosted_weights` over this run."""
        if self.live_u is None:
            raise ValueError('nothing has run yet')
        _, dl, dn = self.dead()
        ph = self.phantoms()
        return boosted_weights(dl, dn, self.live_lnl, ph['lnl'], ph['birth'])

    def boost_log_evidence(self):
        """log Z_boost, the log-sum of the boosted chain's weights: a consistency diagnostic, never the reported evidence (the
        phantoms of one walk are correlated: they sharpen the posterior, not the evidence error)."""
        return self._boosted()[2]

    def boost_index(self):
        """Row j of the boosted ``samples()`` is row ``boost_index()[j]`` of the dead points, the live points and
        :meth:`phantoms` laid end to end."""
        return self._boosted()[1]

    def samples(self, cluster=None, boost=None):
        """(points [N, n], lnL [N], weights [N] summing to 1): the dead points in order of death, then the live points;
        ``cluster``: those of one id of :meth:`clusters` only.  ``boost`` (None: on iff ``boost_posterior > 0``): the chain with
        the phantom points merged in - the events of :func:`boosted_weights` in their order, the live points, the phantoms above
        the last death."""
        boost = (self.phantom_state is not None and cluster is None) if boost is None else bool(boost)
        if boost and cluster is not None:
            raise ValueError('the chain of one cluster is not boosted: per-cluster chains are the base run\'s')
        du, dl, _ = self.dead()
        if boost:
            lw, index, log_z = self._boosted()
            ph = self.phantoms()
            with np.errstate(invalid='ignore'):
                p = np.exp(lw - log_z) if np.isfinite(log_z) else np.zeros(lw.size)
            p = np.where(np.isfinite(p), p, 0.0)
            pts = self.to_physical(np.concatenate([du, self.live_u, ph['u']])[index])
            return pts, np.concatenate([dl, self.live_lnl, ph['lnl']])[index], p / p.sum()
        p = self._evidence()[2]
        pts, lnl = self.to_physical(np.concatenate([du, self.live_u])), np.concatenate([dl, self.live_lnl])
        if cluster is not None:
            ids = self.cluster_ids()
            if int(cluster) not in ids:
                raise ValueError(f'no point carries the cluster id {cluster}')
            keep = ids == int(cluster)
            pts, lnl, p = pts[keep], lnl[keep], p[keep]
        return pts, lnl, p / p.sum()

    # ---- clusters
    def cluster_ids(self):
        """The id of every row of the unboosted :meth:`samples`: what a dead point held when it was killed (0: never labelled), then the live
        points' ids."""
        if self.cluster_state is None:
            raise ValueError('the run was not asked to cluster (clustering=True)')
        if self.live_u is None:
            raise ValueError('nothing has run yet')
        return np.concatenate(self.cluster_state.dead + [self.cluster_state.live_cluster]).astype(np.int32)

    def clusters(self):
        """Per id in order of decreasing posterior mass, a dict: ``id``, ``log_z`` (the log-sum of L_i w_i over the dead and final
        live points of that id, with the weights of :func:`log_weights`), ``mass`` (that local evidence over the whole),
        ``n_dead``, ``n_live``."""
        ids = self.cluster_ids()
        _, dl, dn = self.dead()
        lw = log_weights(dl, dn, self.live_lnl)
        log_z = _logsumexp(lw)
        out = []
        for j in np.unique(ids):
            lz = _logsumexp(lw[ids == j])
            with np.errstate(invalid='ignore'):
                mass = math.exp(lz - log_z) if np.isfinite(lz) and np.isfinite(log_z) else 0.0
            out.append(dict(id=int(j), log_z=lz, mass=mass, n_dead=int(np.sum(ids[:dl.size] == j)),
                            n_live=int(np.sum(ids[dl.size:] == j))))
        out.sort(key=lambda c: (-c['mass'], c['id']))
        return out

    def equal_weighted(self, rng=None):
        """Points of equal weight: each sample kept with probability weight / max weight.  (points [M, n], lnL [M])."""
        rng = np.random.default_rng(rng)
        pts, lnl, w = self.samples()
        keep = rng.random(w.size) < w / w.max()
        return pts[keep], lnl[keep]


# ------------------------------------------------------------------ the sampler over the engine
class NestedSampler(E.EngineSampler, NestedRun):
    """Nested sampling of ``vega`` over its sampled parameters (``sample_params['limits']`` as for
    :class:`vega_amd.ensemble.EnsembleSampler`), a uniform prior over the limits.

    Defaults as the reference's PolyChord interface: ``num_live`` 25 n, ``num_repeats`` 5 n; ``threads`` the largest multiple of 64
    not above min(num_live / 2, vega's max_batch), at least 1.  ``driver``: ``'device'`` (vmx_nested_run) or ``'python'`` (the NumPy
    restatement over ``chi2_batch_device``); an engine group takes ``'python'``."""

    def __init__(self, vega, num_live=None, num_repeats=None, threads=None, precision=1e-3, seed=0, driver='device',
                 sample_params=None, stream=0, chunk=0, lanes=0, const_hint=-1, max_iterations=None, clustering=False,
                 cluster_posteriors=False, boost_posterior=0.0):
        n = self._setup_engine(vega, sample_params, driver, chunk, lanes, const_hint)
        self.cluster_posteriors = bool(cluster_posteriors)
        NestedRun.__init__(self, None, n, num_live=num_live, num_repeats=num_repeats, threads=threads, precision=precision, seed=seed,
                           stream=stream, max_iterations=max_iterations, max_batch=getattr(vega, 'max_batch', None),
                           clustering=bool(clustering) or self.cluster_posteriors, boost_posterior=boost_posterior)

    def _advance(self, n_iterations):
        vega = self.vega
        self._begin_advance(lambda: draw_live(1, self.n, self.seed, self.stream)[0], 'nested_run')
        if self.driver == 'python':
            return self._advance_python(super()._advance, n_iterations)
        vega._sync_monte_carlo()
        draw = self.live_u is None
        if draw:
            self.live_u, self.live_lnl = np.zeros((self.num_live, self.n)), np.zeros(self.num_live)
        du, dl, dn, self.iteration, st = vega.engine.nested_run(
            self.cols, self.lo, self.hi, self._theta, self.live_u, self.live_lnl, self.iteration, n_iterations, self.threads,
            self.num_repeats, log_norm=self.log_norm(), seed=self.seed, stream=self.stream, const_hint=self.const_hint,
            chunk=self.chunk, lanes=self.lanes, draw_live=draw, stop=self._stop, clusters=self.cluster_state,
            **({} if self.phantom_state is None else dict(phantoms=self.phantom_state)))
        return du, dl, dn, st

    def write(self, path, name, derived=False, print_func=print):
        """getdist's weighted chain ``name.txt`` (weight / max weight, -lnL, the parameters: :func:`vega_amd.ensemble.write_getdist`),
        ``name.paramnames`` and ``name.stats``; ``derived``: with the derived parameters' columns and lines after the sampled
        ones.  With ``boost_posterior > 0`` the chain is the boosted one (PolyChord's posterior file) and ``name.stats`` also
        carries ``phantom points`` and ``log(Z) boosted``.  A sampler built with ``cluster_posteriors`` also writes ``name_cluster_<j>.txt``, j = 1 ... in the order of
        :meth:`clusters`, and their evidences and masses into ``name.stats``."""
        return write_run(self, path, name, self.names, cluster_posteriors=self.cluster_posteriors,
                         **self._write_extra(derived, print_func, self.derived))


class NestedRunSet:
    """E independent nested-sampling runs over ``loglike(rows_u [R, n], runs [R]) -> lnL [R]`` (``runs``: the run every row belongs
    to) advanced together by :func:`python_iterations_many`: run e is the :class:`NestedRun` on the Philox stream ``streams[e]``
    (default ``range(E)``), with its own dead record, termination test and evidence (``runs[e]``).  :class:`NestedSet` puts the
    engine behind it.  ``status`` [E]: 0 the run goes on, 1 its termination test ended it, 2 no drawn live point has a finite lnL
    (such a run is left out; the others are not affected).  ``boost_posterior`` = b >= 0 (0: off) as for :class:`NestedRun`:
    every run keeps its own phantom record (:meth:`phantoms`) and :meth:`samples` merges it in; the runs, their evidences and
    their termination are those of b = 0."""

    def __init__(self, loglike, n, runs, num_live=None, num_repeats=None, threads=None, precision=1e-3, seed=0, streams=None,
                 max_iterations=None, max_batch=None, clustering=False, boost_posterior=0.0):
        if clustering:
            raise ValueError('clustering is not part of a set of nested runs: run a NestedSampler(clustering=True) for each')
        self.loglike = loglike
        self.E = int(runs)
        if self.E < 1:
            raise ValueError('runs: at least one')
        self.streams = np.arange(self.E, dtype=np.uint64) if streams is None else np.array(streams, dtype=np.uint64)
        if self.streams.shape != (self.E,):
            raise ValueError(f'streams: one entry for each of the {self.E} runs')
        self.runs = [NestedRun(None, n, num_live=num_live, num_repeats=num_repeats, threads=threads, precision=precision, seed=seed,
                               stream=int(st), max_iterations=max_iterations, max_batch=max_batch, boost_posterior=boost_posterior)
                     for st in self.streams]
        probe = self.runs[0]
        self.n, self.num_live, self.num_repeats, self.threads = probe.n, probe.num_live, probe.num_repeats, probe.threads
        self.precision, self.seed, self.max_iterations = probe.precision, probe.seed, probe.max_iterations
        self.boost_posterior = probe.boost_posterior
        if self._per_call() < 1:
            raise ValueError(f'boost_posterior: one iteration of the {self.E} runs keeps up to {self.E} x {self.threads} x '
                             f'{self.num_repeats - 1} phantom points, more than the {PHANTOM_BUDGET} bytes a call may hold: fewer '
                             'runs in the set, fewer threads or fewer repeats')
        self.reset()

    def _per_call(self):
        """Iterations per call of the driver (:func:`set_iterations_per_call` over the whole set)."""
        return set_iterations_per_call(self.E, self.threads, self.num_repeats, self.n, self.boost_posterior > 0.0)

    def reset(self):
        for run in self.runs:
            run.reset()
        self.status = np.zeros(self.E, dtype=np.int32)
        self._drawn = False
        self.stats = dict(iterations=0, rounds=0, rows=0, rows_own_position=0, engine_calls=0, host_waits=0, seconds=0.0,
                          seconds_enqueuing=0.0, calls=0, per_run=np.zeros((self.E, 3), dtype=np.int64))

    @property
    def iteration(self):
        """[E]: the iterations every run has done."""
        return np.array([run.iteration for run in self.runs], dtype=np.int64)

    @property
    def finished(self):
        """[E]: the run's termination test (the precision criterion, or ``max_iterations``) is met."""
        return np.array([run.terminated for run in self.runs], dtype=bool)

    # ---- drivers
    def _evaluate(self, rows_u, runs):
        return np.asarray(self.loglike(rows_u, runs), dtype=np.float64)

    def _drive(self, idx, live_u, live_lnl, iteration, n_iterations, stop, draw, boost=None):
        """One call of the driver over the runs ``idx`` (their state stacked, updated in place; ``boost``: their
        :class:`PhantomState` objects, this call's kept points appended): what :func:`python_iterations_many` returns."""
        return python_iterations_many(live_u, live_lnl, iteration, n_iterations, self.threads, self.num_repeats, self.seed,
                                      self.streams[idx], lambda rows, runs: self._evaluate(rows, idx[runs]), stop, draw=draw,
                                      boost=boost)

    def _advance(self, idx, n_iterations):
        """Up to ``n_iterations`` iterations of each of the runs ``idx``, as a set of their own; returns the statistics."""
        draw = not self._drawn
        nlive, n = self.num_live, self.n
        if draw:
            live_u, live_lnl = np.zeros((idx.size, nlive, n)), np.zeros((idx.size, nlive))
        else:
            live_u = np.ascontiguousarray(np.stack([self.runs[e].live_u for e in idx]))
            live_lnl = np.ascontiguousarray(np.stack([self.runs[e].live_lnl for e in idx]))
        iteration = np.array([self.runs[e].iteration for e in idx], dtype=np.int64)

        def stop(a, iterations, dead_lnl, live):
            return self.runs[idx[a]]._stop(iterations, dead_lnl, live)

        boost = [self.runs[e].phantom_state for e in idx] if self.boost_posterior > 0.0 else None
        dead, status, done, st = self._drive(idx, live_u, live_lnl, iteration, n_iterations, stop, draw,
                                             **({} if boost is None else dict(boost=boost)))
        self._drawn = True
        per = np.zeros((self.E, 3), dtype=np.int64)
        per[idx] = st['per_run']
        for a, e in enumerate(idx):
            run = self.runs[e]
            self.status[e] = status[a]
            if status[a] == NO_FINITE:
                continue
            run.live_u, run.live_lnl, run.iteration = live_u[a].copy(), live_lnl[a].copy(), int(iteration[a])
            if done[a] > 0:
                run._dead_u.append(dead[a][0])
                run._dead_lnl.append(dead[a][1])
                run._dead_n.append(dead[a][2])
            run.stats['iterations'] += int(done[a])
            run.stats['rows'] += int(per[e, 0])
            run.stats['rows_own_position'] += int(per[e, 1])
            run.stats['rounds'] += int(per[e, 2])
            run.stats['calls'] += 1
        return dict(st, per_run=per)

    def run(self, iterations=None):
        """Every run to its own termination (``iterations`` None: the precision criterion or ``max_iterations``, run by run), or
        exactly ``iterations`` more iterations of every run, whatever the criterion says (``finished`` still reports it); the set
        does not depend on how it is cut."""
        t0 = time.perf_counter()
        for run in self.runs:
            run._to_termination = iterations is None
        per_call = self._per_call()         # (the dead record of a call is allocated up front, with boost the phantom records too)
        left = None if iterations is None else int(iterations)
        while True:
            going = self.status != NO_FINITE
            if iterations is None:
                going &= ~self.finished
                if self.max_iterations is not None:
                    going &= self.iteration < self.max_iterations
            idx = np.flatnonzero(going)
            if idx.size == 0:
                break
            if iterations is None:
                call = per_call if self.max_iterations is None else min(per_call, int(self.max_iterations - self.iteration[idx].min()))
            else:
                call = min(per_call, left)
                left -= call
            if call <= 0 and self._drawn:
                break
            st = self._advance(idx, max(call, 0))
            for key, val in st.items():
                if key in ('lanes', 'const_hint'):      # (what the engine ran with)
                    self.stats[key] = val
                elif key in self.stats and key != 'seconds':
                    self.stats[key] = self.stats[key] + val
            self.stats['calls'] += 1
            if iterations is not None and left <= 0:
                break
        self.stats['seconds'] += time.perf_counter() - t0
        return self

    # ---- results
    def _ran(self):
        if not self._drawn:
            raise ValueError('nothing has run yet')

    def log_evidence(self):
        """(log Z [E], its error sqrt(H / num_live) [E]); NaN for a run without a finite live lnL."""
        self._ran()
        out = np.full((2, self.E), np.nan)
        for e, run in enumerate(self.runs):
            if self.status[e] != NO_FINITE:
                out[:, e] = run.log_evidence()
        return out[0], out[1]

    def information(self):
        """H [E]; NaN for a run without a finite live lnL."""
        self._ran()
        return np.array([run.information() if self.status[e] != NO_FINITE else np.nan for e, run in enumerate(self.runs)])

    def dead(self, e):
        """The dead record of run ``e``: (u [N, n], lnL [N], live count [N])."""
        return self.runs[int(e)].dead()

    def to_physical(self, u):
        return u

    def samples(self, boost=None):
        """Per run (points [N_e, n], lnL [N_e], weights [N_e] summing to 1): its dead points in order of death, then its live
        points; None for a run without a finite live lnL.  ``boost`` (None: on iff ``boost_posterior > 0``): every run's chain
        with its phantom points merged in, as :meth:`NestedRun.samples` orders it."""
        self._ran()
        out = []
        for e, run in enumerate(self.runs):
            if self.status[e] == NO_FINITE:
                out.append(None)
                continue
            pts, lnl, w = run.samples(boost=boost)
            out.append((self.to_physical(pts), lnl, w))
        return out

    def phantoms(self, e):
        """The kept phantom points of run ``e`` in the canonical order: the dict of :meth:`NestedRun.phantoms`."""
        return self.runs[int(e)].phantoms()

    def summary(self, weighted_quantiles=None, boost=None, where='device'):
        """The weighted summary of every run's :meth:`samples` (``boost`` as there): ``dict(count [E], n_eff [E] (Kish), mean
        [E, n], sd [E, n], covariance [E, n, n])``, and with ``weighted_quantiles=q`` (1 .. 16 values in [0, 1]) also
        ``weighted_quantiles`` (the q), ``quantile_values`` [E, n, Q] (the inverted CDF), ``lnl_max`` [E] and ``best`` [E, n].
        ``where='device'`` reduces the samples in a sample store on the GPU (vega_amd/csrc/vmx_chain_weighted.h), ``'host'``, the
        ``python`` driver and an engine group with :mod:`vega_amd.weighted`: the same bits.  A run without a finite live lnL is a
        set without rows: count 0 and NaNs."""
        from .weighted import summarise_runs
        return summarise_runs(self, self.samples(boost=boost), weighted_quantiles, where)

    def boost_log_evidence(self):
        """log Z_boost [E] (:meth:`NestedRun.boost_log_evidence`: a diagnostic, never the reported evidence); NaN for a run
        without a finite live lnL."""
        self._ran()
        return np.array([run.boost_log_evidence() if self.status[e] != NO_FINITE else np.nan for e, run in enumerate(self.runs)])

    def boost_index(self):
        """Per run :meth:`NestedRun.boost_index` (row j of its boosted samples is row index[j] of its dead points, live points
        and phantoms laid end to end); None for a run without a finite live lnL."""
        self._ran()
        return [run.boost_index() if self.status[e] != NO_FINITE else None for e, run in enumerate(self.runs)]


class NestedSet(E.EngineSampler, NestedRunSet):
    """E independent nested-sampling runs of ``vega`` over its sampled parameters, advanced together: one host wait per set round
    for all of them, the requests of all runs packed into one stream of engine rows (``'device'``: vmx_nested_run_many, one
    work-group per run; ``'python'``: :func:`python_iterations_many` over ``chi2_batch_device``, cut into the same chunks).  Run e
    is on the Philox stream ``streams[e]`` (default ``range(E)``) and is the run ``NestedSampler(..., seed=seed,
    stream=streams[e])`` makes - up to the last bits of lnL where the engine's batches are shaped differently (DESIGN section
    6h).  ``mock_rows`` [E]: the row of the installed mock pools every run is compared with - log Z and a weighted posterior per
    Monte-Carlo mock (:meth:`vega_amd.montecarlo.MonteCarlo.sample_mocks_nested`); None: every run reads the data the interface has
    installed - replicas of one run (:func:`vega_amd.replicas.merge_nested`).  Every run ends on its own termination test.
    Clustering is not part of a set.  ``boost_posterior`` = b > 0: every run keeps the fraction min(1, b / num_repeats) of the
    accepted points inside its walks (``'device'``: vmx_nested_run_many_phantoms) and its samples, its member's files and
    ``sample_mocks_nested``'s summaries are the boosted chain's; the runs and their evidences are those of b = 0.  An engine group
    takes ``'python'``."""

    def __init__(self, vega, runs, num_live=None, num_repeats=None, threads=None, precision=1e-3, seed=0, streams=None, mock_rows=None,
                 driver='device', max_iterations=None, chunk=0, lanes=0, const_hint=-1, sample_params=None, clustering=False,
                 boost_posterior=0.0):
        if clustering:
            raise ValueError('clustering is not part of a set of nested runs: run a NestedSampler(clustering=True) for each')
        n = self._setup_engine(vega, sample_params, driver, chunk, lanes, const_hint)
        NestedRunSet.__init__(self, None, n, runs, num_live=num_live, num_repeats=num_repeats, threads=threads, precision=precision,
                              seed=seed, streams=streams, max_iterations=max_iterations, max_batch=getattr(vega, 'max_batch', None),
                              boost_posterior=boost_posterior)
        self.mock_rows = None if mock_rows is None else np.array(mock_rows, dtype=np.int32)
        if self.mock_rows is not None and self.mock_rows.shape != (self.E,):
            raise ValueError(f'mock_rows: one entry for each of the {self.E} runs')
        if self.mock_rows is not None and np.any(self.mock_rows < 0):
            raise ValueError('mock_rows: rows of the installed mock pools, none negative')

    def to_physical(self, u):
        return E.EngineSampler.to_physical(self, u)

    def _evaluate(self, rows_u, runs):
        rows_t = np.repeat(self._theta[None, :], rows_u.shape[0], axis=0)
        rows_t[:, self.cols] = self.to_physical(rows_u)
        return lnl_of(0, self._rows.chi2(rows_t, None if self.mock_rows is None else self.mock_rows[runs]), self.log_norm())

    def _drive(self, idx, live_u, live_lnl, iteration, n_iterations, stop, draw, boost=None):
        vega = self.vega
        self._begin_advance(lambda: draw_live(1, self.n, self.seed, int(self.streams[0]))[0], 'nested_run_many')
        if self.driver == 'python':
            with self._engine_rows() as self._rows:
                try:
                    dead, status, done, st = NestedRunSet._drive(self, idx, live_u, live_lnl, iteration, n_iterations, stop, draw,
                                                                 boost=boost)
                finally:
                    calls, self._rows = self._rows.calls, None
            return dead, status, done, dict(st, engine_calls=calls, host_waits=calls)
        vega._sync_monte_carlo()
        extra = {}
        if boost is not None:       # (with boost off the call is the one of before: vmx_nested_run_many)
            from .engine import PhantomArrays
            extra['phantoms'] = PhantomArrays(idx.size, max(0, int(n_iterations)) * self.threads * (self.num_repeats - 1), self.n,
                                              boost[0].fraction)
        out = vega.engine.nested_run_many(
            self.cols, self.lo, self.hi, self._theta, live_u, live_lnl, iteration, self.streams[idx], n_iterations, self.threads,
            self.num_repeats, mock_rows=None if self.mock_rows is None else self.mock_rows[idx], log_norm=self.log_norm(),
            seed=self.seed, const_hint=self.const_hint, chunk=self.chunk, lanes=self.lanes, draw_live=draw, stop=stop, **extra)
        if boost is not None:
            for a, state in enumerate(boost):
                state.append(*extra['phantoms'].run(a))
        return out

    def member(self, e):
        """Run ``e`` as a sampler that has run: :class:`NestedSampler`'s result methods (``log_evidence``, ``information``,
        ``samples``, ``dead``, ``derived``, ``write``) over copies of its part of the set's state; with ``boost_posterior > 0``
        it carries the run's phantom record, so that these give the boosted chain as a single boosted run does.  Read-only: it
        cannot be advanced."""
        if not 0 <= int(e) < self.E:
            raise IndexError(f'member: 0 .. {self.E - 1}')
        e = int(e)
        run = self.runs[e]
        m = NestedSampler(self.vega, num_live=self.num_live, num_repeats=self.num_repeats, threads=self.threads,
                          precision=self.precision, seed=self.seed, driver=self.driver_asked,
                          sample_params=dict(limits=dict(zip(self.names, zip(self.lo, self.hi))), values=self.values,
                                             errors=self.errors),
                          stream=int(self.streams[e]), chunk=self.chunk, lanes=self.lanes, const_hint=self.const_hint,
                          max_iterations=self.max_iterations, boost_posterior=self.boost_posterior)
        m.driver = self.driver
        m.run = m.reset = _read_only
        if run.live_u is not None:
            m.live_u, m.live_lnl = run.live_u.copy(), run.live_lnl.copy()
        m.iteration, m.terminated = run.iteration, run.terminated
        m._dead_u, m._dead_lnl, m._dead_n = list(run._dead_u), list(run._dead_lnl), list(run._dead_n)
        m._log_x, m._log_z_dead = run._log_x, run._log_z_dead
        m.stats = dict(run.stats)
        if run.phantom_state is not None:
            m.phantom_state.calls = list(run.phantom_state.calls)
        m.status = int(self.status[e])
        return m


def _read_only(*args, **kwargs):
    raise RuntimeError('a member of a NestedSet is read-only: advance the set')


def nested_settings(main_config, sample_params):
    """The ``[Nested]`` settings of a main config with ``sampler = Nested`` (called by
    :func:`vega_amd.ensemble.sampler_settings`, which has checked ``run_sampler``): {sampler, path, name, num_live, num_repeats,
    precision, seed, threads, driver, max_iterations}, and ``derived`` / ``replicas`` (:mod:`vega_amd.replicas`) when the section states them.``num_live``, ``num_repeats``, ``precision`` and ``seed`` mean what they
    mean in the reference's ``[Polychord]`` section, with its defaults; ``threads`` None: the sampler's own default.
    ``do_clustering`` / ``cluster_posteriors`` (the reference's keys, both False when absent and then not in the settings;
    ``cluster_posteriors`` implies ``do_clustering`` and is refused with ``replicas > 1``).  ``boost_posterior`` (the reference's
    key, a float >= 0, in the settings only when the section states it; > 0 is refused with ``mocks``, ``together`` and
    ``replicas > 1``).  ``mocks = M``: log Z and a weighted
    posterior for each of M Monte-Carlo mocks in one run (the conditions of ``[Ensemble] mocks``); ``together = True`` with
    ``replicas``: a rank's replicas advance as one :class:`NestedSet`; neither combines with ``do_clustering``."""
    sec, limits, out = E.section_settings(main_config, sample_params, 'Nested', name='nested')
    n = len(limits)
    out.update(num_live=sec.getint('num_live', 25 * n), num_repeats=sec.getint('num_repeats', 5 * n),
               precision=sec.getfloat('precision', 0.001), seed=sec.getint('seed', 0), threads=sec.getint('threads', None),
               max_iterations=sec.getint('max_iterations', None))
    for key in ('do_clustering', 'cluster_posteriors'):         # (the reference's [Polychord] keys; absent: the settings of before)
        if key in sec:
            out[key] = sec.getboolean(key)
    if out.get('cluster_posteriors'):
        out['do_clustering'] = True
        if out.get('replicas', 1) > 1:
            raise ValueError('[Nested] cluster_posteriors and replicas > 1 do not combine: the cluster ids of different replicas '
                             'are unrelated')
    if 'boost_posterior' in sec:                                # (the reference's key, 0.0 when absent and then not in the settings)
        try:
            out['boost_posterior'] = sec.getfloat('boost_posterior')
        except ValueError:
            raise ValueError('[Nested] boost_posterior: a number, at least 0') from None
        if not (math.isfinite(out['boost_posterior']) and out['boost_posterior'] >= 0.0):
            raise ValueError('[Nested] boost_posterior: a finite number, at least 0')
    if 'mocks' in sec:
        out['mocks'] = E._parse_mocks(sec, main_config, 'Nested', 'a nested run')
    from .weighted import parse_weighted_quantiles
    parse_weighted_quantiles(sec, out, 'Nested')
    if 'together' in sec:
        try:
            out['together'] = sec.getboolean('together')
        except ValueError:
            raise ValueError('[Nested] together: True or False') from None
    if out.get('do_clustering') and (out.get('mocks') or out.get('together')):
        raise ValueError('[Nested] do_clustering does not combine with mocks or together: clustering is not part of a set of runs')
    if out.get('boost_posterior', 0.0) > 0.0 and (out.get('mocks') or out.get('together') or out.get('replicas', 1) > 1):
        raise ValueError('[Nested] boost_posterior does not combine with mocks, together or replicas > 1: sets of runs and replica '
                         'merges keep no phantom points (out of scope)')
    if not n + 2 <= out['num_live'] <= MAX_LIVE:
        raise ValueError(f'[Nested] num_live: {n + 2} .. {MAX_LIVE} for {n} sampled parameters')
    if out['threads'] is not None and not 1 <= out['threads'] <= out['num_live'] - n - 1:
        raise ValueError(f'[Nested] threads: 1 .. num_live - n - 1 = {out["num_live"] - n - 1}')
    if out['num_repeats'] < 1:
        raise ValueError('[Nested] num_repeats must be positive')
    if not out['precision'] > 0.0:
        raise ValueError('[Nested] precision must be positive')
    if out['max_iterations'] is not None and out['max_iterations'] < 1:
        raise ValueError('[Nested] max_iterations must be positive')
    return out


def write_run(run, path, name, names, cluster_posteriors=False, **derived):
    """The three files of a finished :class:`NestedRun`: (txt, paramnames, stats); ``derived``: the derived-parameter arguments of
    :func:`vega_amd.ensemble.write_getdist`.  ``cluster_posteriors`` (a run with clustering): also ``name_cluster_<j>.txt`` for
    j = 1 ... in the order of ``run.clusters()``, the weighted chain of that id alone (with its own ``.paramnames``, so that
    getdist reads it as a chain of its own), and per cluster the lines
    ``log(Z_j)``, ``mass_j`` and ``id_j`` in ``name.stats``.  A run with ``boost_posterior > 0``: ``name.txt`` is the boosted
    chain, the per-cluster chains stay the base run's, and ``name.stats`` ends with ``phantom points`` and ``log(Z) boosted``."""
    pts, lnl, w = run.samples()
    txt, pn = E.write_getdist(path, name, names, pts, lnl, weights=w / w.max(), **derived)
    boosted = getattr(run, 'phantom_state', None) is not None
    found = run.clusters() if cluster_posteriors else []
    if found:
        ids = run.cluster_ids()
        block = derived.get('derived')
        if boosted:         # (the per-cluster chains are the base run's: its rows, and their derived rows out of the boosted block)
            pts, lnl, w = run.samples(boost=False)
            if block is not None:
                index = run.boost_index()
                base = np.empty((ids.size,) + np.asarray(block).shape[1:])
                base[index[index < ids.size]] = np.asarray(block)[index < ids.size]
                block = base
        for j, c in enumerate(found, start=1):
            keep = ids == c['id']
            extra = dict(derived, derived=np.asarray(block)[keep]) if block is not None else derived
            wj = w[keep]
            top = wj.max() if wj.size and wj.max() > 0.0 else 1.0
            E.write_getdist(path, f'{name}_cluster_{j}', names, pts[keep], lnl[keep], weights=wj / top, **extra)
    log_z, err = run.log_evidence()
    stats = Path(path) / f'{name}.stats'
    with open(stats, 'w') as f:
        f.write(f'log(Z) = {log_z!r}\nlog(Z) error = {err!r}\nH = {run.information()!r}\n')
        f.write(f'dead points = {sum(len(d) for d in run._dead_lnl)}\nlikelihood evaluations = {run.stats["rows"]}\n')
        f.write(f'iterations = {run.iteration}\nseed = {run.seed}\nnum_live = {run.num_live}\nnum_repeats = {run.num_repeats}\n')
        f.write(f'threads = {run.threads}\n')
        for j, c in enumerate(found, start=1):
            f.write(f'log(Z_{j}) = {c["log_z"]!r}\nmass_{j} = {c["mass"]!r}\nid_{j} = {c["id"]}\n')
        if boosted:
            f.write(f'phantom points = {run.phantoms()["lnl"].size}\nlog(Z) boosted = {run.boost_log_evidence()!r}\n')
    return txt, pn, stats


def read_stats(path):
    """``name.stats`` back as a dict (floats for the evidence lines, ints for the counts)."""
    out = {}
    for line in Path(path).read_text().splitlines():
        key, _, val = line.partition(' = ')
        real = key in ('log(Z)', 'log(Z) error', 'H', 'log(Z) boosted') or key.startswith('log(Z_') or key.startswith('mass_')
        out[key] = float(val) if real else int(val)
    return out
