"""Evidence and an equal-weight posterior by tempered sequential Monte Carlo (the scheme of pocoMC, without its normalising flow),
run where the particles are.

The reference's second sampler is pocoMC (bin/run_vega_mpi.py: ``[control] run_sampler = True``, ``sampler = PocoMC``).  Here N
particles start from the prior and walk a ladder of inverse temperatures 0 = beta_0 < beta_1 < ... = 1 chosen so that the effective
sample size of the importance weights stays at ``ess`` N; every stage reweights, resamples (systematic), whitens with the
particles' covariance and moves all particles by ``sweeps`` Metropolis sweeps under L^beta.  A sweep is one batch of N rows for the
engine.  The ``device`` driver keeps particles and bookkeeping on the GPU (include/vegamx.h: vmx_smc_run); the ``python`` driver is
the readable restatement in NumPy over ``VegaInterface.chi2_batch_device``.  Both follow vega_amd/csrc/vmx_smc.h decision for
decision - its own ``exp`` included - so that they produce the same particles and ancestors bit for bit.  The evidence is computed
here, on the host, from the stage record - one code for both drivers.

``log Z = sum_t log mean_i w_i(beta_t)`` with ``w_i = L_i^(beta_t - beta_{t-1})``; its error ``sqrt(sum_t (N / ESS_t - 1) / N)``
is the delta-method figure for independent particles: it ignores the correlation the moves leave behind (few sweeps make the
particles of a stage more alike than independent draws would be, and the seed-to-seed scatter then exceeds it; see
:func:`evidence`).

``n_total`` and ``recycle`` (pocoMC's ``posterior()``): with ``n_total`` the run goes on at beta = 1 with posterior rounds - whiten,
move, no reweighting, no resampling - until that many points are there; with ``recycle`` the particles of every stage are kept and
reweighted into one weighted chain (:func:`recycled_weights`), which costs no likelihood evaluation.

What is not here: pocoMC's flow-based preconditioning, ``dynamic`` particle counts, the trimming of the largest recycled weights,
state files.
"""
import math
import time
from pathlib import Path

import numpy as np

from . import ensemble as E
from . import nested as NS

MAXN = 32
MAX_PARTICLES = 4096
BISECTIONS = 60
LANES = 1024
DOMAIN_MOVE, DOMAIN_RESAMPLE, DOMAIN_START = 3, 4, 5

INV_LN2 = 1.44269504088896338700e+00
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
_EXP_COEF = (1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0,
             1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0)


# ------------------------------------------------------------------ the algorithm (vmx_smc.h) in NumPy
def _pow2(k):
    return ((np.asarray(k, dtype=np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)


def pexp(x):
    """vmx_smc::pexp: exp from separately rounded operations, the same bits as the header gives."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    nan, big, small = np.isnan(x), x > 709.0, x < -745.2
    xs = np.where(nan | big | small, 0.0, x)
    s = xs * INV_LN2
    kf = np.floor(s + 0.5)
    h = kf * LN2_HI
    r = xs - h
    low = kf * LN2_LO
    r = r - low
    p = np.full(x.shape, 1.0 / 6227020800.0)
    for c in _EXP_COEF:
        m = p * r
        p = m + c
    k = kf.astype(np.int64)
    deep = k < -1022
    q = p * _pow2(np.where(deep, k + 1000, k))
    out = np.where(deep, q * 2.0**-1000, q)
    out = np.where(small, 0.0, np.where(big, np.inf, out))
    return np.where(nan, x, out)


def _blocks(c0, c1, c2, c3, seed, stream):
    c0 = np.asarray(c0, dtype=np.uint64)
    ctr = np.zeros(c0.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = c0
    ctr[..., 1] = np.asarray(c1, dtype=np.uint64)
    ctr[..., 2] = np.asarray(c2, dtype=np.uint64)
    ctr[..., 3] = np.uint64(c3)
    return E.philox4x64_10(ctr, (int(seed), int(stream)))


def move_blocks(i, stage, sweep, j, seed, stream=0):
    """Blocks of particle ``i`` at (stage, sweep), block index ``j``: counter (i, stage 2^32 + sweep, j, 3)."""
    return _blocks(i, (int(stage) << 32) + int(sweep), j, DOMAIN_MOVE, seed, stream)


def resample_uniform(stage, seed, stream=0):
    return float(E.u01(_blocks(np.zeros(1), int(stage), 0, DOMAIN_RESAMPLE, seed, stream)[0, 0]))


def draw_start(N, n, seed, stream=0):
    """The start particles [N, n]: coordinate c of particle i from word c % 4 of block (i, 0, c / 4, 5)."""
    nb = (n + 3) // 4
    i = np.repeat(np.arange(N)[:, None], nb, axis=1)
    j = np.repeat(np.arange(nb)[None, :], N, axis=0)
    return E.u01(_blocks(i, 0, j, DOMAIN_START, seed, stream).reshape(N, nb * 4)[:, :n])


def start_scale(n):
    t = 3.0 / float(n)
    return 2.38 * math.sqrt(t)


def pad_pow2(N):
    M = 1
    while M < N:
        M <<= 1
    return M


def weights(dbeta, d):
    d = np.asarray(d, dtype=np.float64)
    dead = np.isneginf(d)
    return np.where(dead, 0.0, pexp(np.float64(dbeta) * np.where(dead, 0.0, d)))


def tree_sum(a):
    """The stride-halving tree over ``a`` padded with zeros to a power of two."""
    M = pad_pow2(a.size)
    a = np.concatenate([a, np.zeros(M - a.size)])
    s = M // 2
    while s >= 1:
        a = a[:s] + a[s:2 * s]
        s //= 2
    return float(a[0])


def weight_sums(dbeta, d):
    w = weights(dbeta, d)
    return tree_sum(w), tree_sum(w * w)


def ess_of(s1, s2):
    t = np.float64(s1) * np.float64(s1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(t / np.float64(s2))


def next_beta(beta_prev, d, target):
    """(beta_t, ESS(beta_t), S1(beta_t)) from beta_{t-1} and d_i = lnL_i - max lnL."""
    beta = 1.0
    s1, s2 = weight_sums(1.0 - beta_prev, d)
    if not ess_of(s1, s2) >= target:
        lo, hi = float(beta_prev), 1.0
        for _ in range(BISECTIONS):
            mid = 0.5 * (lo + hi)
            s1, s2 = weight_sums(mid - beta_prev, d)
            if ess_of(s1, s2) >= target:
                lo = mid
            else:
                hi = mid
        beta = lo
        s1, s2 = weight_sums(beta - beta_prev, d)
    return beta, ess_of(s1, s2), s1


def cumulative(w, s1):
    """The cumulative normalised weights: per-segment running sums plus the scanned segment totals; the last entry is 1."""
    N = w.size
    L = (N + LANES - 1) // LANES
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.concatenate([w / np.float64(s1), np.zeros(L * LANES - N)]).reshape(LANES, L)
    r = np.zeros((LANES, L))
    acc = np.zeros(LANES)
    for k in range(L):
        acc = acc + q[:, k]
        r[:, k] = acc
    t = acc.copy()
    step = 1
    while step < LANES:
        t = np.concatenate([t[:step], t[step:] + t[:-step]])
        step <<= 1
    pre = np.concatenate([[0.0], t[:-1]])
    c = (pre[:, None] + r).reshape(-1)[:N].copy()
    c[N - 1] = 1.0
    return c


def positions(v, N):
    s = np.float64(v) + np.arange(N, dtype=np.float64)
    return s / float(N)


def ancestors(c, p):
    N = c.size
    lo = np.zeros(p.size, dtype=np.int64)
    hi = np.full(p.size, N - 1, dtype=np.int64)
    while np.any(lo < hi):
        go = lo < hi
        mid = (lo + hi) // 2
        with np.errstate(invalid='ignore'):
            right = c[mid] > p
        hi = np.where(go & right, mid, hi)
        lo = np.where(go & ~right, mid + 1, lo)
    return lo.astype(np.int32)


def stage_head(u, lnl, beta_prev, ess, stage, seed, stream=0):
    """Reweight, resample and whiten for stage ``stage``: dict(beta, ess, s1, w, c, anc, u, lnl (resampled), mean, cov, C,
    cholesky).  ``beta`` NaN: no particle has a finite lnL."""
    N = u.shape[0]
    top = np.max(lnl)
    if top == -np.inf:
        return dict(beta=math.nan)
    with np.errstate(invalid='ignore'):
        d = lnl - top
    beta, ess_t, s1 = next_beta(beta_prev, d, np.float64(ess) * float(N))
    w = weights(beta - beta_prev, d)
    c = cumulative(w, s1)
    anc = ancestors(c, positions(resample_uniform(stage, seed, stream), N))
    u2, lnl2 = u[anc], lnl[anc]
    mean, cov = NS.mean_cov(u2)
    C, ok = NS.whiten(cov)
    return dict(beta=beta, ess=ess_t, s1=s1, w=w, c=c, anc=anc, u=u2, lnl=lnl2, mean=mean, cov=cov, C=C, cholesky=ok)


def propose(u, C, scale, stage, sweep, seed, stream=0):
    """Proposals of every particle at (stage, sweep): (y [N, n], inside [N], the deciding uniforms [N])."""
    N, n = u.shape
    nb = n // 4 + 1
    i = np.repeat(np.arange(N)[:, None], nb, axis=1)
    j = np.repeat(np.arange(nb)[None, :], N, axis=0)
    x = E.u01(move_blocks(i, stage, sweep, j, seed, stream).reshape(N, nb * 4)[:, :n + 1])
    two = 2.0 * x[:, :n]
    g = two - 1.0
    z = np.zeros((N, n))
    for jj in range(n):         # (z_a accumulates C_aj g_j in the order j = 0 .. a)
        z[:, jj:] = z[:, jj:] + C[jj:, jj][None, :] * g[:, jj][:, None]
    step = np.float64(scale) * z
    y = u + step
    return y, np.all((y >= 0.0) & (y <= 1.0), axis=1), x[:, n]


def accept(inside, ok, beta, lnl_new, lnl_old, ua):
    with np.errstate(invalid='ignore'):
        dl = lnl_new - lnl_old
        delta = np.float64(beta) * dl
        up = delta >= 0.0
        return inside & ok & (up | (ua < pexp(np.where(up | np.isnan(delta), 0.0, delta))))


def adapt(scale, accepted, N):
    a = float(accepted) / float(N)
    if a < 0.15:
        return scale * 0.8
    if a > 0.35:
        return scale * 1.25
    return scale


_REC_KEYS = ('beta_prev', 'beta', 'ess', 'accepted', 'scale', 'cholesky')


def posterior_round_head(u, lnl):
    """vmx_smc::posterior_round_head: the head of a posterior round, a stage entered with beta = 1.  No bisection, no weights, no
    resampling uniform; the particles stay as they are.  dict(beta = 1, ess = the particles with a finite lnL, anc the identity,
    u, lnl, mean, cov, C, cholesky) - the keys of :func:`stage_head` that the sweeps and the record read."""
    mean, cov = NS.mean_cov(u)
    C, ok = NS.whiten(cov)
    return dict(beta=1.0, ess=float(np.count_nonzero(lnl > -np.inf)), anc=np.arange(u.shape[0], dtype=np.int32), u=u, lnl=lnl,
                mean=mean, cov=cov, C=C, cholesky=ok)


def run_finished(beta, topups_left):
    """vmx_smc::run_finished: at beta = 1 with no posterior round owed."""
    return beta >= 1.0 and topups_left <= 0


# ------------------------------------------------------------------ a set of runs (vmx_smc.h: "a set of runs")
RUNNING, FINISHED, NO_FINITE, STUCK = 0, 1, 2, 3


def run_status(beta_before, beta_after):
    """vmx_smc::run_status: what a stage round made of a run."""
    if math.isnan(beta_after):
        return NO_FINITE
    if not beta_after > beta_before:
        return STUCK
    return FINISHED if beta_after >= 1.0 else RUNNING


def first_active(beta, draw):
    """vmx_smc::first_active: (the runs a call begins with, ascending; the status of every run)."""
    status = np.where(draw | (np.asarray(beta) < 1.0), RUNNING, FINISHED).astype(np.int32)
    return [int(e) for e in np.flatnonzero(status == RUNNING)], status


def compact_active(active, status):
    """vmx_smc::compact_active: the runs still going keep their order and move up."""
    return [e for e in active if status[e] == RUNNING]


def run_status_kept(beta_before, beta_after, topups_left):
    """vmx_smc::run_status_kept: (what a stage round made of a run that owed ``topups_left`` posterior rounds at its head, the
    rounds it owes now).  A posterior round (``beta_before`` = 1) pays one and cannot be stuck."""
    if math.isnan(beta_after):
        return NO_FINITE, topups_left
    if beta_before >= 1.0:
        topups_left -= 1
    elif not beta_after > beta_before:
        return STUCK, topups_left
    return (FINISHED if run_finished(beta_after, topups_left) else RUNNING), topups_left


def first_active_kept(beta, topups_left, draw):
    """vmx_smc::first_active_kept: a run at beta = 1 that owes posterior rounds begins the call."""
    going = np.array([draw or not run_finished(b, t) for b, t in zip(np.asarray(beta), np.asarray(topups_left))], dtype=bool)
    status = np.where(going, RUNNING, FINISHED).astype(np.int32)
    return [int(e) for e in np.flatnonzero(going)], status


def python_stages_many(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, streams, evaluate, draw=False, topups_left=None,
                       keep=None):
    """Up to ``n_stages`` stage rounds of E runs in NumPy (vmx_smc_run_many restated): ``u`` [E, N, n], ``lnl`` [E, N], ``stage``
    int64 [E], ``beta`` [E], ``scale`` [E] the runs' state, updated in place (a failed run's part is left as it was at entry),
    ``streams`` [E].  A round advances every run still going by one stage (:func:`stage_head`, then ``sweeps`` times
    :func:`propose` / :func:`accept` / :func:`adapt`, run by run); ``evaluate(rows_u [A N, n], runs [A])`` -> lnL [A N] takes the
    rows of the A runs still going (ascending, run ``runs[a]`` owns rows a N .. (a + 1) N - 1) at once.  ``draw``: the particles are
    drawn and evaluated first.  Returns (records: per run the list of stage dicts as :func:`python_stages` makes them, status
    int32 [E]: 0 still going, 1 at beta = 1, 2 no particle with a finite lnL, 3 the ladder cannot advance; stages_done int32 [E];
    statistics with ``per_run`` int64 [E, 4]: accepted, own-position rows, failed models, rows evaluated, and ``rounds``).

    ``topups_left`` int [E] (updated in place): the posterior rounds every run owes at beta = 1 (vmx_smc_run_many_kept restated) -
    such a run stays in the list and takes :func:`posterior_round_head` beside the others' :func:`stage_head`.  ``keep``: a list
    of E lists, run e's receives its particles at the entry of every stage it does.  With either, ``topups_left`` is returned
    after ``stages_done``."""
    E, N, n = u.shape
    new_form = keep is not None or topups_left is not None
    owed = np.zeros(E, dtype=np.int64) if topups_left is None else topups_left
    owed_entry = owed.copy()
    entry = (u.copy(), lnl.copy(), stage.copy(), beta.copy(), scale.copy())
    records = [[] for _ in range(E)]
    per = np.zeros((E, 4), dtype=np.int64)
    active, status = first_active_kept(beta, owed, bool(draw))
    rounds = 0

    def rows_of(parts):
        per[active, 3] += N
        return np.asarray(evaluate(np.concatenate(parts, axis=0), np.array(active, dtype=np.int64)), dtype=np.float64).reshape(len(active), N)

    if draw and active:
        for e in active:
            u[e] = draw_start(N, n, seed, int(streams[e]))
            beta[e], scale[e] = 0.0, start_scale(n)
        first = rows_of([u[e] for e in active])
        for a, e in enumerate(active):
            lnl[e] = first[a]
            status[e] = RUNNING if np.any(first[a] > -np.inf) else NO_FINITE
        active = compact_active(active, status)
    while rounds < n_stages and active:
        heads = {}
        for e in active:
            before = u[e].copy() if keep is not None else None
            if beta[e] >= 1.0:
                head = posterior_round_head(u[e], lnl[e])
            else:
                head = stage_head(u[e], lnl[e], float(beta[e]), ess, int(stage[e]), seed, int(streams[e]))
            heads[e] = head
            if keep is not None and not math.isnan(head['beta']):
                keep[e].append(before)
            if math.isnan(head['beta']):
                continue
            records[e].append(dict(beta_prev=float(beta[e]), beta=head['beta'], ess=head['ess'], lnl=lnl[e].copy(), anc=head['anc'],
                                   cholesky=head['cholesky'], accepted=0, scale=float(scale[e])))
            u[e], lnl[e] = head['u'], head['lnl']
        own, bad = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
        for s in range(sweeps):
            prop = {}
            for e in active:            # (a run without a finite lnL sends its rows as they are: the device does the same)
                if math.isnan(heads[e]['beta']):
                    prop[e] = None
                else:
                    prop[e] = propose(u[e], heads[e]['C'], float(scale[e]), int(stage[e]), s, seed, int(streams[e]))
            new = rows_of([u[e] if prop[e] is None else np.where(prop[e][1][:, None], prop[e][0], u[e]) for e in active])
            for a, e in enumerate(active):
                if prop[e] is None:
                    continue
                y, inside, ua = prop[e]
                ok = new[a] > -np.inf
                acc = accept(inside, ok, heads[e]['beta'], new[a], lnl[e], ua)
                u[e][acc] = y[acc]
                lnl[e][acc] = new[a][acc]
                k = int(acc.sum())
                scale[e] = adapt(float(scale[e]), k, N)
                records[e][-1]['accepted'] += k
                own[e] += int((~inside).sum())
                bad[e] += int((inside & ~ok).sum())
        for e in active:
            status[e], owed[e] = run_status_kept(float(beta[e]), heads[e]['beta'], int(owed[e]))
            if status[e] in (NO_FINITE, STUCK):
                continue
            records[e][-1]['scale'] = float(scale[e])
            beta[e] = heads[e]['beta']
            stage[e] += 1
            per[e, 0] += records[e][-1]['accepted']
            per[e, 1] += own[e]
            per[e, 2] += bad[e]
        active = compact_active(active, status)
        rounds += 1
    done = np.zeros(E, dtype=np.int32)
    for e in range(E):
        if status[e] in (NO_FINITE, STUCK):
            u[e], lnl[e], stage[e], beta[e], scale[e] = (arr[e] for arr in entry)
            owed[e] = owed_entry[e]
            records[e] = []
            if keep is not None:
                del keep[e][:]
            per[e, :3] = 0
        done[e] = len(records[e])
    st = dict(stages=int(done.sum()), sweeps=int(done.sum()) * sweeps, rows=int(per[:, 3].sum()), rows_own_position=int(per[:, 1].sum()),
              accepted=int(per[:, 0].sum()), rejected_failed_model=int(per[:, 2].sum()), rounds=rounds, per_run=per)
    if new_form:
        return records, status, done, owed, st
    return records, status, done, st


def python_stages(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, stream, evaluate, topups_left=0, keep=None):
    """Up to ``n_stages`` stages of one run in NumPy: the set of one of :func:`python_stages_many`, from the state ``u`` [N, n],
    ``lnl`` [N] (updated in place), stopping after the stage that reaches beta = 1.  ``evaluate(rows_u)`` -> lnL [N] of rows in the
    cube (-inf: a failed model).  Returns (record: a list of dicts per stage with beta_prev, beta, ess, lnl (before reweighting),
    anc, accepted, scale, cholesky; stage, beta, scale, stats).  A run that cannot go on raises ValueError and leaves ``u``,
    ``lnl`` and ``keep`` as they were at entry.  (There is no ``watch`` hook any more: nothing called it.)

    ``topups_left`` posterior rounds are owed at beta = 1 (vmx_smc.h: "kept populations and posterior rounds"): the run then goes
    on with stages headed by :func:`posterior_round_head`, one record row each (beta_prev = beta = 1), ``n_stages`` bounding both
    kinds together.  ``keep``, a list, receives the particles at the entry of every stage done.  With either, the rounds still
    owed are returned after ``scale``: (record, stage, beta, scale, topups_left, stats)."""
    new_form = keep is not None or bool(topups_left)
    stage, beta, scale = np.array([stage], dtype=np.int64), np.array([beta], dtype=np.float64), np.array([scale], dtype=np.float64)
    kept = [[]] if keep is not None else None
    records, status, _, owed, st = python_stages_many(
        u[None], lnl[None], stage, beta, scale, n_stages, ess, sweeps, seed, [stream], lambda rows_u, runs: evaluate(rows_u),
        topups_left=np.array([int(topups_left)], dtype=np.int64), keep=kept)
    if status[0] == NO_FINITE:
        raise ValueError('SMC: no particle has a finite log-likelihood')
    if status[0] == STUCK:
        raise ValueError('SMC: the temperature ladder cannot advance: fewer than ess N particles carry weight')
    if keep is not None:
        keep.extend(kept[0])
    st = {key: val for key, val in st.items() if key not in ('rounds', 'per_run')}
    if new_form:
        return records[0], int(stage[0]), float(beta[0]), float(scale[0]), int(owed[0]), st
    return records[0], int(stage[0]), float(beta[0]), float(scale[0]), st


# ------------------------------------------------------------------ evidence (host, both drivers)
def evidence(record, N):
    """(log Z, err) from the stage record: ``log Z = sum_t [log mean_i w_i(beta_t) + (beta_t - beta_{t-1}) max lnL]`` with
    ``w_i(beta_t) = exp((beta_t - beta_{t-1})(lnL_i - max lnL))``, through a log-sum-exp; ``err = sqrt(sum_t (N / ESS_t - 1) /
    N)``.  The error is the delta-method variance of a mean of N independent weights, stage by stage (relative variance of the
    mean weight = (N / ESS - 1) / N); resampling noise and the correlation between particles that share an ancestor and have
    not moved apart are not in it.  With the default 4 n sweeps the seed-to-seed scatter was measured at about 1.0 - 1.2 times
    this figure (tests/test_smc_host.py), with half as many sweeps about 1.5 times."""
    log_z, var = 0.0, 0.0
    for rec in record:
        db = rec['beta'] - rec['beta_prev']
        with np.errstate(invalid='ignore'):
            log_z += NS._logsumexp(db * np.asarray(rec['lnl'], dtype=np.float64)) - math.log(N)
        var += (N / rec['ess'] - 1.0) / N
    return log_z, math.sqrt(max(var, 0.0))


def running_evidence(record, N):
    """log Z at the entry of every stage of ``record`` and after the last one, [stages + 1], by :func:`evidence`'s own recursion:
    0 first, then the sums of its terms."""
    out = [0.0]
    for rec in record:
        db = rec['beta'] - rec['beta_prev']
        with np.errstate(invalid='ignore'):
            out.append(out[-1] + (NS._logsumexp(db * np.asarray(rec['lnl'], dtype=np.float64)) - math.log(N)))
    return np.array(out)


def recycled_weights(betas, log_z_running, lnl):
    """The particles of S populations of N points each as one weighted posterior sample, by the balance heuristic: population s
    was drawn from ``L^beta_s / Z_s`` over the prior (``betas`` [S]: 0 for the start, the ladder's values, 1 for every beta = 1
    population; ``log_z_running`` [S]: the running evidence at that stage, 0 for the start, the final value for every beta = 1
    population: :func:`running_evidence`), so that the S N points together are a sample of the mixture ``sum_s N L^beta_s /
    Z_s`` and a point with ``lnL = l`` has the posterior weight

        ``log w = l - logsumexp_s(log N + beta_s l - log Z_s)``.

    ``lnl`` [S, N].  A point with ``l = -inf`` gets weight 0 and takes no part.  Returns (the weights [S, N], normalised to sum
    1; ``log_z_recycled = logsumexp(log w)``: the sum of the unnormalised weights estimates Z).  float64 on the host, the same code
    for both drivers.  pocoMC trims the largest weights of its recycled chain afterwards; that is not done here."""
    betas = np.asarray(betas, dtype=np.float64).reshape(-1)
    log_z = np.asarray(log_z_running, dtype=np.float64).reshape(-1)
    lnl = np.asarray(lnl, dtype=np.float64)
    if lnl.ndim != 2 or betas.shape != (lnl.shape[0],) or log_z.shape != betas.shape:
        raise ValueError('recycled_weights: betas [S], log_z_running [S], lnl [S, N]')
    N = lnl.shape[1]
    live = lnl > -np.inf
    if not np.any(live):
        return np.zeros(lnl.shape), -math.inf
    l = lnl[live]
    terms = math.log(N) + betas[:, None] * l[None, :] - log_z[:, None]          # [S, points]
    top = terms.max(axis=0)
    log_w = l - (top + np.log(np.exp(terms - top[None, :]).sum(axis=0)))
    log_z_recycled = float(NS._logsumexp(log_w))
    w = np.zeros(lnl.shape)
    w[live] = np.exp(log_w - log_z_recycled)
    return w, log_z_recycled


KEEP_BUDGET = 1 << 30       # bytes of kept positions (stages + posterior rounds) N n 8 a run may hold
KEEP_STAGES = 64            # the ladder stages that figure assumes where max_stages is not given


def posterior_rounds_for(n_total, particles):
    """R = ceil(n_total / N) - 1 posterior rounds make (R + 1) N >= n_total points at beta = 1; None: 0."""
    if n_total is None:
        return 0
    if isinstance(n_total, bool) or int(n_total) != n_total or int(n_total) < particles:
        raise ValueError(f'n_total: a whole number, at least the {particles} particles')
    return -(-int(n_total) // particles) - 1


class SMCRun:
    """A tempered SMC run over ``loglike(rows_u [R, n]) -> lnL [R]`` in the unit cube (-inf: a failed model), NumPy driver: the
    particles, the stage record and the evidence.  :class:`SMCSampler` puts the engine behind it.

    ``n_total`` (a whole number >= ``particles``): after the ladder the run goes on with R = ceil(n_total / N) - 1 posterior rounds
    at beta = 1, and ``samples()`` returns the (R + 1) N points of the beta = 1 populations.  It counts points, not independent
    draws: successive rounds are ``sweeps`` sweeps apart, and a particle that no sweep moved appears again.  ``recycle``: the
    particles of every stage are kept and ``samples()`` returns all of them with :func:`recycled_weights`.  Either option keeps
    the positions of every population, (stages + R) N n 8 bytes; a run that would exceed ``KEEP_BUDGET`` with ``max_stages``
    (``KEEP_STAGES`` where it is None) ladder stages is refused here.  ``log_evidence()``, ``stages``, ``record`` and
    ``max_stages`` stay the ladder's: the rows of the posterior rounds are in ``posterior_rounds``."""

    def __init__(self, loglike, n, particles=1024, ess=0.5, sweeps=None, seed=0, stream=0, max_stages=None, n_total=None,
                 recycle=False):
        self.loglike = loglike
        self.n = int(n)
        self.particles = int(particles)
        self.ess = float(ess)
        self.sweeps = int(sweeps) if sweeps is not None else 4 * self.n
        self.seed, self.stream = int(seed), int(stream)
        self.max_stages = None if max_stages is None else int(max_stages)
        if not 1 <= self.n <= MAXN:
            raise ValueError(f'1 .. {MAXN} sampled parameters')
        if not max(2 * self.n + 2, 8) <= self.particles <= MAX_PARTICLES:
            raise ValueError(f'particles: {max(2 * self.n + 2, 8)} .. {MAX_PARTICLES} for {self.n} sampled parameters')
        if not 0.0 < self.ess < 1.0:
            raise ValueError('ess: between 0 and 1')
        if self.sweeps < 1:
            raise ValueError('sweeps >= 1')
        if self.max_stages is not None and self.max_stages < 1:
            raise ValueError('max_stages >= 1')
        self.rounds = posterior_rounds_for(n_total, self.particles)
        self.n_total = None if n_total is None else int(n_total)
        if not isinstance(recycle, (bool, np.bool_)):
            raise ValueError('recycle: True or False')
        self.recycle = bool(recycle)
        self.keeping = self.recycle or n_total is not None
        if self.keeping and ((self.max_stages or KEEP_STAGES) + self.rounds) * self.particles * self.n * 8 > KEEP_BUDGET:
            raise ValueError(f'n_total / recycle: the kept populations would exceed {KEEP_BUDGET} bytes')
        self.reset()

    def reset(self):
        self.u = self.lnl = None
        self.stage = 0
        self.beta = 0.0
        self.scale = start_scale(self.n)
        self.record = []
        self.topups_left = self.rounds
        self.posterior_rounds = []
        self.stats = dict(stages=0, sweeps=0, rows=0, rows_own_position=0, accepted=0, rejected_failed_model=0, engine_calls=0,
                          host_waits=0, seconds=0.0, seconds_enqueuing=0.0, calls=0)

    @property
    def finished(self):
        """At beta = 1 with no posterior round owed."""
        return run_finished(self.beta, self.topups_left)

    @property
    def stages(self):
        """The ladder so far, one entry per stage: dict of arrays beta_prev, beta, ess, acceptance (accepted / (N sweeps)),
        scale (after the stage)."""
        rec = self.record
        return dict(beta_prev=np.array([r['beta_prev'] for r in rec]), beta=np.array([r['beta'] for r in rec]),
                    ess=np.array([r['ess'] for r in rec]),
                    acceptance=np.array([r['accepted'] / (self.particles * self.sweeps) for r in rec]),
                    scale=np.array([r['scale'] for r in rec]))

    # ---- drivers
    def _evaluate(self, rows_u):
        return np.asarray(self.loglike(rows_u), dtype=np.float64)

    def _draw(self):
        self.u = np.ascontiguousarray(draw_start(self.particles, self.n, self.seed, self.stream))
        self.lnl = np.ascontiguousarray(self._evaluate(self.u), dtype=np.float64)
        self.stats['rows'] += self.particles
        if np.any(np.isnan(self.lnl)):
            raise ValueError('SMC: a start particle has a NaN log-likelihood')
        if not np.any(self.lnl > -np.inf):
            raise ValueError('SMC: no particle has a finite log-likelihood')

    def _advance(self, n_stages):
        """One call of the driver: (record, statistics)."""
        if self.u is None:
            self._draw()
        if not self.keeping:
            rec, self.stage, self.beta, self.scale, st = python_stages(
                self.u, self.lnl, self.stage, self.beta, self.scale, n_stages, self.ess, self.sweeps, self.seed, self.stream,
                self._evaluate)
            return rec, st
        keep = []
        rec, self.stage, self.beta, self.scale, self.topups_left, st = python_stages(
            self.u, self.lnl, self.stage, self.beta, self.scale, n_stages, self.ess, self.sweeps, self.seed, self.stream,
            self._evaluate, topups_left=self.topups_left, keep=keep)
        for r, before in zip(rec, keep):
            r['u'] = before
        return rec, st

    def run(self, stages=None):
        """To beta = 1 and through the posterior rounds owed (``stages`` None; ``max_stages`` bounds the ladder), or at most
        ``stages`` more stages, ladder stages and posterior rounds alike; the run does not depend on how it is cut."""
        t0 = time.perf_counter()
        budget = 1 << 20 if stages is None else int(stages)
        while budget > 0 and not self.finished:
            if self.beta >= 1.0:
                call = min(budget, self.topups_left)
            else:
                call = budget if self.max_stages is None else min(budget, max(0, self.max_stages - len(self.record)))
            if call <= 0:
                break
            at = self.stage
            rec, st = self._advance(call)
            for r in rec:           # (the rows of the posterior rounds stay out of the ladder's record)
                (self.posterior_rounds if r['beta_prev'] >= 1.0 else self.record).append(r)
            for key, val in st.items():
                if key in ('lanes', 'const_hint'):      # (what the engine ran with)
                    self.stats[key] = val
                elif key in self.stats and key != 'seconds':
                    self.stats[key] += val
            self.stats['calls'] += 1
            budget -= self.stage - at
            if self.stage == at:
                break
        self.stats['seconds'] += time.perf_counter() - t0
        return self

    # ---- results
    def log_evidence(self):
        """(log Z, its delta-method error: :func:`evidence`) of the stages run so far (the evidence when ``finished``)."""
        if self.u is None:
            raise ValueError('nothing has run yet')
        return evidence(self.record, self.particles)

    def to_physical(self, u):
        return u

    def populations(self):
        """The kept populations in the order they were made, the particles as they stand last: (u [S, N, n] in the unit cube, lnL
        [S, N], beta [S], the running log Z [S] of :func:`recycled_weights`).  Population s < stages is what ladder stage s
        reweighted; then the entries of the posterior rounds, then the particles."""
        if self.u is None:
            raise ValueError('nothing has run yet')
        if not self.keeping:
            raise ValueError('populations: the run keeps them with n_total or recycle')
        rows = self.record + self.posterior_rounds
        u = np.array([r['u'] for r in rows] + [self.u])
        lnl = np.array([r['lnl'] for r in rows] + [self.lnl])
        beta = np.array([r['beta_prev'] for r in rows] + [self.beta])
        log_z = running_evidence(self.record, self.particles)
        log_z = np.concatenate([log_z, np.full(len(self.posterior_rounds), log_z[-1])])
        return u, lnl, beta, log_z

    def _chain(self, recycle=None):
        """(u [points, n], lnL, weights, log_z_recycled or None) of the chain ``samples(recycle)`` returns."""
        if self.u is None:
            raise ValueError('nothing has run yet')
        recycle = self.recycle if recycle is None else bool(recycle)
        N = self.particles
        if not recycle and self.n_total is None:
            return self.u.copy(), self.lnl.copy(), np.full(N, 1.0 / N), None
        u, lnl, beta, log_z = self.populations()
        if not recycle:
            at_one = beta >= 1.0
            if not np.any(at_one):          # (the ladder is still going: the particles as they stand)
                at_one[-1] = True
            u, lnl = u[at_one], lnl[at_one]
            return u.reshape(-1, self.n), lnl.reshape(-1), np.full(lnl.size, 1.0 / lnl.size), None
        w, log_zr = recycled_weights(beta, log_z, lnl)
        return u.reshape(-1, self.n), lnl.reshape(-1), w.reshape(-1), log_zr

    def samples(self, recycle=None):
        """(points [N, n], lnL [N], weights [N] = 1 / N): the particles - the posterior sample once ``finished``.  ``recycle``
        (None: the constructor's setting) off with ``n_total``: the (R + 1) N points of the beta = 1 populations, equal weights; on:
        every kept population and the particles, [S N, n], with :func:`recycled_weights`."""
        u, lnl, w, _ = self._chain(recycle)
        return self.to_physical(u), lnl, w

    def n_eff(self, recycle=None):
        """Kish's sample size 1 / sum w^2 of the chain ``samples(recycle)`` returns.  It does not see the correlation between
        populations that are ``sweeps`` sweeps apart."""
        w = self._chain(recycle)[2]
        return float(1.0 / np.sum(w * w))

    def recycled_log_evidence(self):
        """``log_z_recycled`` of :func:`recycled_weights` over every kept population: the evidence from all stages' particles."""
        return self._chain(True)[3]


# ------------------------------------------------------------------ the sampler over the engine
_PER_CALL = 64          # stages per call of the device driver (its record is allocated up front)


class SMCSampler(E.EngineSampler, SMCRun):
    """Tempered SMC of ``vega`` over its sampled parameters (``sample_params['limits']`` as for
    :class:`vega_amd.ensemble.EnsembleSampler`), a uniform prior over the limits.  ``driver``: ``'device'`` (vmx_smc_run) or
    ``'python'`` (the NumPy restatement over ``chi2_batch_device``); an engine group takes ``'python'``."""

    def __init__(self, vega, particles=1024, ess=0.5, sweeps=None, seed=0, driver='device', chunk=0, sample_params=None, stream=0,
                 lanes=0, const_hint=-1, max_stages=None, n_total=None, recycle=False):
        n = self._setup_engine(vega, sample_params, driver, chunk, lanes, const_hint)
        SMCRun.__init__(self, None, n, particles=particles, ess=ess, sweeps=sweeps, seed=seed, stream=stream, max_stages=max_stages,
                        n_total=n_total, recycle=recycle)

    def _advance(self, n_stages):
        vega = self.vega
        self._begin_advance(lambda: draw_start(1, self.n, self.seed, self.stream)[0], 'smc_run')
        if self.driver == 'python':
            return self._advance_python(super()._advance, n_stages)
        vega._sync_monte_carlo()
        draw = self.u is None
        u = np.zeros((self.particles, self.n)) if draw else self.u
        lnl = np.zeros(self.particles) if draw else self.lnl
        record, total = [], None
        while n_stages > 0 and (draw or not self.finished):
            out = vega.engine.smc_run(
                self.cols, self.lo, self.hi, self._theta, u, lnl, self.stage, self.beta, self.scale, min(n_stages, _PER_CALL),
                self.ess, self.sweeps, log_norm=self.log_norm(), seed=self.seed, stream=self.stream, const_hint=self.const_hint,
                chunk=self.chunk, lanes=self.lanes, draw=draw, **(dict(keep=True, topups_left=self.topups_left) if self.keeping else {}))
            if self.keeping:
                rec, self.stage, self.beta, self.scale, self.topups_left, st = out
            else:
                rec, self.stage, self.beta, self.scale, st = out
            self.u, self.lnl = u, lnl
            draw = False
            n_stages -= min(n_stages, _PER_CALL)
            record.extend(rec)
            if total is None:
                total = dict(st)
            else:
                for key, val in st.items():
                    if key not in ('const_hint', 'lanes'):
                        total[key] += val
        return record, total or {}

    def write(self, path, name, derived=False, print_func=print):
        """getdist's chain ``name.txt`` (weight 1, -lnL, the parameters: :func:`vega_amd.ensemble.write_getdist`),
        ``name.paramnames`` and ``name.stats``; ``derived``: with the derived parameters' columns and lines after the sampled
        ones."""
        return write_run(self, path, name, self.names, **self._write_extra(derived, print_func, self.derived))


class SMCSet(E.EngineSampler):
    """E independent tempered SMC runs of N particles each over the sampled parameters of ``vega``, advanced together: one host
    round per stage for every run still going, the A N rows of a sweep through the engine as one stream of chunks (``'device'``:
    vmx_smc_run_many, one work-group per run; ``'python'``: :func:`python_stages_many` over ``chi2_batch_device``, cut into the
    same chunks).  Run e is on the Philox stream ``streams[e]`` (default ``range(E)``) and is the run
    ``SMCSampler(..., seed=seed, stream=streams[e])`` makes - up to the last bits of lnL where the engine's batches are shaped
    differently.  ``mock_rows`` [E]: the row of the installed mock pools every run is compared with - log Z
    and a posterior per Monte-Carlo mock (:meth:`vega_amd.montecarlo.MonteCarlo.sample_mocks`); None: every run reads the data
    the interface has installed - replicas of one run.  Every run ends on its own: at beta = 1 (``status`` 1), or because no
    particle has a finite lnL (2) or its ladder cannot advance (3); the last two do not stop the others.  An engine group takes
    ``'python'``.  ``n_total`` / ``recycle`` as for :class:`SMCRun`, the same for every run: a run that has reached beta = 1 stays
    in the set until it has paid its R posterior rounds (vmx_smc_run_many_kept), beside the runs still on the ladder."""

    def __init__(self, vega, runs, particles=1024, streams=None, mock_rows=None, ess=0.5, sweeps=None, seed=0, driver='device',
                 chunk=0, lanes=0, const_hint=-1, max_stages=None, sample_params=None, n_total=None, recycle=False):
        self.n = self._setup_engine(vega, sample_params, driver, chunk, lanes, const_hint)
        probe = SMCRun(None, self.n, particles=particles, ess=ess, sweeps=sweeps, seed=seed, max_stages=max_stages, n_total=n_total,
                       recycle=recycle)   # (its checks)
        self.particles, self.ess, self.sweeps, self.seed, self.max_stages = probe.particles, probe.ess, probe.sweeps, probe.seed, probe.max_stages
        self.n_total, self.rounds, self.recycle, self.keeping = probe.n_total, probe.rounds, probe.recycle, probe.keeping
        self.E = int(runs)
        if self.E < 1:
            raise ValueError('runs: at least one')
        self.streams = np.arange(self.E, dtype=np.uint64) if streams is None else np.array(streams, dtype=np.uint64)
        self.mock_rows = None if mock_rows is None else np.array(mock_rows, dtype=np.int32)
        if self.streams.shape != (self.E,) or (self.mock_rows is not None and self.mock_rows.shape != (self.E,)):
            raise ValueError(f'streams, mock_rows: one entry for each of the {self.E} runs')
        if self.mock_rows is not None and np.any(self.mock_rows < 0):
            raise ValueError('mock_rows: rows of the installed mock pools, none negative')
        self.reset()

    def reset(self):
        self.u = self.lnl = None
        self.stage = np.zeros(self.E, dtype=np.int64)
        self.beta = np.zeros(self.E)
        self.scale = np.full(self.E, start_scale(self.n))
        self.status = np.zeros(self.E, dtype=np.int32)
        self.record = [[] for _ in range(self.E)]
        self.topups_left = np.full(self.E, self.rounds, dtype=np.int32)
        self.posterior_rounds = [[] for _ in range(self.E)]
        self.stats = dict(stages=0, sweeps=0, rows=0, rows_own_position=0, accepted=0, rejected_failed_model=0, engine_calls=0,
                          host_waits=0, seconds=0.0, seconds_enqueuing=0.0, calls=0, rounds=0,
                          per_run=np.zeros((self.E, 4), dtype=np.int64))

    @property
    def finished(self):
        """[E]: the run has reached beta = 1 and owes no posterior round."""
        return (self.beta >= 1.0) & (self.topups_left <= 0)

    # ---- drivers
    def _advance(self, n_stages, rounds_only=False):
        """Up to ``n_stages`` rounds of the runs still going (``rounds_only``: of those at beta = 1 that owe posterior rounds), as
        a set of their own (the engine's rows are those of the runs still going either way); returns the statistics."""
        vega, N, n = self.vega, self.particles, self.n
        self._begin_advance(lambda: draw_start(1, n, self.seed, int(self.streams[0]))[0], 'smc_run_many')
        draw = self.u is None
        if draw:
            self.u, self.lnl = np.zeros((self.E, N, n)), np.zeros((self.E, N))
        idx = np.flatnonzero((self.status == RUNNING) & ((self.beta >= 1.0) if rounds_only else True))
        u, lnl = np.ascontiguousarray(self.u[idx]), np.ascontiguousarray(self.lnl[idx])
        stage, beta, scale = self.stage[idx].copy(), self.beta[idx].copy(), self.scale[idx].copy()
        owed = self.topups_left[idx].copy()
        kept = dict(keep=True, topups_left=owed) if self.keeping else {}
        streams = self.streams[idx]
        mocks = None if self.mock_rows is None else self.mock_rows[idx]
        records, total = [[] for _ in idx], None
        status = np.zeros(idx.size, dtype=np.int32)

        def add(st):
            nonlocal total
            if total is None:
                total = dict(st, per_run=st['per_run'].copy())
                return
            for key, val in st.items():
                if key not in ('const_hint', 'lanes'):
                    total[key] = total[key] + val

        if self.driver == 'python':
            log_norm = self.log_norm()

            def evaluate(rows_u, runs):
                rows_t = np.repeat(self._theta[None, :], rows_u.shape[0], axis=0)
                rows_t[:, self.cols] = self.to_physical(rows_u)
                return NS.lnl_of(0, self._rows.chi2(rows_t, None if mocks is None else np.repeat(mocks[runs], N)), log_norm)

            with self._engine_rows() as self._rows:
                try:
                    if self.keeping:
                        keep = [[] for _ in idx]
                        records, status, _, _, st = python_stages_many(u, lnl, stage, beta, scale, n_stages, self.ess, self.sweeps,
                                                                       self.seed, streams, evaluate, draw=draw, topups_left=owed,
                                                                       keep=keep)
                        for a in range(idx.size):
                            for r, before in zip(records[a], keep[a]):
                                r['u'] = before
                    else:
                        records, status, _, st = python_stages_many(u, lnl, stage, beta, scale, n_stages, self.ess, self.sweeps,
                                                                    self.seed, streams, evaluate, draw=draw)
                finally:
                    calls, self._rows = self._rows.calls, None
            add(dict(st, engine_calls=calls, host_waits=calls))
        else:
            vega._sync_monte_carlo()
            while True:
                k = min(n_stages, _PER_CALL)
                sub = np.flatnonzero(status == RUNNING)         # (a long run is cut into calls of _PER_CALL rounds)
                if sub.size == 0 or (k == 0 and not draw):
                    break
                su, sl, ss, sb, sc = (np.ascontiguousarray(arr[sub]) for arr in (u, lnl, stage, beta, scale))
                if self.keeping:
                    kept['topups_left'] = np.ascontiguousarray(owed[sub])
                rec, stat, _, st = vega.engine.smc_run_many(
                    self.cols, self.lo, self.hi, self._theta, su, sl, ss, sb, sc, streams[sub], k, self.ess, self.sweeps,
                    mock_rows=None if mocks is None else mocks[sub], log_norm=self.log_norm(), seed=self.seed,
                    const_hint=self.const_hint, chunk=self.chunk, lanes=self.lanes, draw=draw, **kept)
                u[sub], lnl[sub], stage[sub], beta[sub], scale[sub], status[sub] = su, sl, ss, sb, sc, stat
                if self.keeping:
                    owed[sub] = kept['topups_left']
                for a, e in enumerate(sub):
                    records[e].extend(rec[a])
                per = np.zeros((idx.size, 4), dtype=np.int64)
                per[sub] = st['per_run']
                add(dict(st, per_run=per, rounds=st['host_waits'] - 1 - (1 if draw else 0)))
                draw = False
                n_stages -= k
        self.u[idx], self.lnl[idx], self.stage[idx], self.beta[idx], self.scale[idx], self.status[idx] = u, lnl, stage, beta, scale, status
        self.topups_left[idx] = owed
        for a, e in enumerate(idx):
            for r in records[a]:        # (the rows of the posterior rounds stay out of the ladder's record)
                (self.posterior_rounds[e] if r['beta_prev'] >= 1.0 else self.record[e]).append(r)
        if total is not None:
            per = np.zeros((self.E, 4), dtype=np.int64)
            per[idx] = total['per_run']
            total['per_run'] = per
        return total or {}

    def run(self, stages=None):
        """Every run to its end (``stages`` None; ``max_stages`` bounds the runs), or at most ``stages`` more rounds (0 on a new
        set: the start particles alone); the set does not depend on how it is cut."""
        t0 = time.perf_counter()
        at = max(len(r) for r in self.record)       # (max_stages bounds the ladder: posterior rounds do not count)
        budget = 1 << 20 if stages is None else int(stages)
        call = budget if self.max_stages is None else min(budget, max(0, self.max_stages - at))

        def advance(count, rounds_only=False):
            before = self.stats['rounds']
            st = self._advance(count, rounds_only)
            for key, val in st.items():
                if key in ('lanes', 'const_hint'):      # (what the engine ran with)
                    self.stats[key] = val
                elif key in self.stats and key != 'seconds':
                    self.stats[key] = self.stats[key] + val
            self.stats['calls'] += 1
            return self.stats['rounds'] - before

        going = (self.status == RUNNING) & (True if self.u is None else ~self.finished)
        if (call > 0 or self.u is None) and np.any(going):        # (a first call of no stages draws and evaluates the start)
            budget -= advance(max(call, 0))
        # the runs at beta = 1 that owe posterior rounds go on where max_stages has stopped the ladder of the others
        owing = (self.status == RUNNING) & (self.beta >= 1.0) & (self.topups_left > 0)
        if budget > 0 and np.any(owing):
            advance(min(budget, int(self.topups_left[owing].max())), rounds_only=True)
        self.stats['seconds'] += time.perf_counter() - t0
        return self

    # ---- results
    def _ran(self):
        if self.u is None:
            raise ValueError('nothing has run yet')

    def log_evidence(self):
        """(log Z [E], its delta-method error [E]: :func:`evidence` of every run's record); NaN for a failed run."""
        self._ran()
        out = np.full((2, self.E), np.nan)
        for e in range(self.E):
            if self.status[e] not in (NO_FINITE, STUCK):
                out[:, e] = evidence(self.record[e], self.particles)
        return out[0], out[1]

    def samples(self, recycle=None):
        """(points [E, N, n], lnL [E, N], weights [E, N] = 1 / N): the particles of every run - its posterior sample once finished
        (a failed run's are what it started from).  With ``n_total`` or ``recycle`` (None: the constructor's setting) every
        entry is a list over the runs of what :meth:`SMCRun.samples` returns for that run: the ladders differ in length, and
        with them the recycled chains."""
        self._ran()
        recycle = self.recycle if recycle is None else bool(recycle)
        if not recycle and self.n_total is None:
            return self.to_physical(self.u.copy()), self.lnl.copy(), np.full((self.E, self.particles), 1.0 / self.particles)
        runs = [self._bare_member(e).samples(recycle) for e in range(self.E)]
        return [r[0] for r in runs], [r[1] for r in runs], [r[2] for r in runs]

    def summary(self, weighted_quantiles=None, recycle=None, where='device'):
        """The weighted summary of every run's :meth:`samples` (``recycle`` as there): ``dict(count [E], n_eff [E] (Kish), mean
        [E, n], sd [E, n], covariance [E, n, n])``, and with ``weighted_quantiles=q`` (1 .. 16 values in [0, 1]) also
        ``weighted_quantiles`` (the q), ``quantile_values`` [E, n, Q] (the inverted CDF), ``lnl_max`` [E] and ``best`` [E, n].
        ``where='device'`` reduces the samples in a sample store on the GPU (vega_amd/csrc/vmx_chain_weighted.h), ``'host'``, the
        ``python`` driver and an engine group with :mod:`vega_amd.weighted`: the same bits."""
        from .weighted import summarise_runs
        return summarise_runs(self, list(zip(*self.samples(recycle))), weighted_quantiles, where)

    def n_eff(self, recycle=None):
        """[E]: Kish's sample size of every run's chain (:meth:`SMCRun.n_eff`)."""
        self._ran()
        return np.array([self._bare_member(e).n_eff(recycle) for e in range(self.E)])

    def recycled_log_evidence(self):
        """[E]: :meth:`SMCRun.recycled_log_evidence` of every run; NaN for a failed run."""
        self._ran()
        return np.array([math.nan if self.status[e] in (NO_FINITE, STUCK) else self._bare_member(e).recycled_log_evidence()
                         for e in range(self.E)])

    def _bare_member(self, e):
        """Run ``e``'s state in an :class:`SMCRun` in the unit cube's own terms, for its result methods."""
        m = SMCRun(None, self.n, particles=self.particles, ess=self.ess, sweeps=self.sweeps, seed=self.seed, stream=int(self.streams[e]),
                   max_stages=self.max_stages, n_total=self.n_total, recycle=self.recycle)
        m.to_physical = self.to_physical
        m.u, m.lnl, m.stage, m.beta, m.scale = self.u[e], self.lnl[e], int(self.stage[e]), float(self.beta[e]), float(self.scale[e])
        m.record, m.posterior_rounds, m.topups_left = self.record[e], self.posterior_rounds[e], int(self.topups_left[e])
        return m

    def member(self, e):
        """Run ``e`` as a sampler that has run: :class:`SMCSampler`'s result methods (``log_evidence``, ``samples``, ``stages``,
        ``derived``, ``write``) over copies of its part of the set's state.  Read-only: it cannot be advanced."""
        if not 0 <= int(e) < self.E:
            raise IndexError(f'member: 0 .. {self.E - 1}')
        e = int(e)
        m = SMCSampler(self.vega, particles=self.particles, ess=self.ess, sweeps=self.sweeps, seed=self.seed, driver=self.driver_asked,
                       chunk=self.chunk, sample_params=dict(limits=dict(zip(self.names, zip(self.lo, self.hi))), values=self.values,
                                                            errors=self.errors),
                       stream=int(self.streams[e]), lanes=self.lanes, const_hint=self.const_hint, max_stages=self.max_stages,
                       n_total=self.n_total, recycle=self.recycle)
        m.driver = self.driver
        m.run = m.reset = _read_only
        if self.u is not None:
            m.u, m.lnl = self.u[e].copy(), self.lnl[e].copy()
        m.stage, m.beta, m.scale = int(self.stage[e]), float(self.beta[e]), float(self.scale[e])
        m.record = list(self.record[e])
        m.posterior_rounds, m.topups_left = list(self.posterior_rounds[e]), int(self.topups_left[e])
        took, own, bad, rows = (int(v) for v in self.stats['per_run'][e])
        done = len(m.record) + len(m.posterior_rounds)
        m.stats = dict({k: v for k, v in self.stats.items() if k not in ('per_run', 'rounds')}, stages=done,
                       sweeps=done * self.sweeps, rows=rows, rows_own_position=own, accepted=took, rejected_failed_model=bad)
        m.status = int(self.status[e])
        return m


def _read_only(*args, **kwargs):
    raise RuntimeError('a member of an SMCSet is read-only: advance the set')


def smc_settings(main_config, sample_params):
    """The ``[SMC]`` settings of a main config with ``sampler = SMC`` (called by :func:`vega_amd.ensemble.sampler_settings`, which
    has checked ``run_sampler``): {sampler, path, name, particles, ess, sweeps, seed, driver, max_stages}, and ``derived`` / ``replicas`` (:mod:`vega_amd.replicas`) when the section states them; ``sweeps``
    None: 4 n.  ``mocks = M``: log Z and a posterior for each of M Monte-Carlo mocks in one run (the conditions of ``[Ensemble]
    mocks``); ``together = True`` with ``replicas``: a rank's replicas advance as one :class:`SMCSet`.  ``n_total`` (a whole number
    >= ``particles``) and ``recycle`` (True | False) are in the settings only when the section states them (:class:`SMCRun`); both
    go with ``mocks`` and with ``together``, neither with ``replicas`` > 1: :func:`vega_amd.replicas.merge_smc` has no weighted
    chains yet."""
    sec, limits, out = E.section_settings(main_config, sample_params, 'SMC', name='smc')
    n = len(limits)
    out.update(particles=sec.getint('particles', 1024), ess=sec.getfloat('ess', 0.5), sweeps=sec.getint('sweeps', None),
               seed=sec.getint('seed', 0), max_stages=sec.getint('max_stages', None))
    if not 1 <= n <= MAXN:
        raise ValueError(f'[SMC] 1 .. {MAXN} sampled parameters')
    if not max(2 * n + 2, 8) <= out['particles'] <= MAX_PARTICLES:
        raise ValueError(f'[SMC] particles: {max(2 * n + 2, 8)} .. {MAX_PARTICLES} for {n} sampled parameters')
    if not 0.0 < out['ess'] < 1.0:
        raise ValueError('[SMC] ess: between 0 and 1')
    if out['sweeps'] is not None and out['sweeps'] < 1:
        raise ValueError('[SMC] sweeps must be positive')
    if out['max_stages'] is not None and out['max_stages'] < 1:
        raise ValueError('[SMC] max_stages must be positive')
    if 'mocks' in sec:
        out['mocks'] = E._parse_mocks(sec, main_config, 'SMC', 'an SMC run')
    from .weighted import parse_weighted_quantiles
    parse_weighted_quantiles(sec, out, 'SMC')
    if 'together' in sec:
        try:
            out['together'] = sec.getboolean('together')
        except ValueError:
            raise ValueError('[SMC] together: True or False') from None
    if 'n_total' in sec:
        try:
            out['n_total'] = sec.getint('n_total')
        except ValueError:
            raise ValueError('[SMC] n_total: a whole number, at least the particles') from None
        if out['n_total'] < out['particles']:
            raise ValueError('[SMC] n_total: a whole number, at least the particles')
    if 'recycle' in sec:
        try:
            out['recycle'] = sec.getboolean('recycle')
        except ValueError:
            raise ValueError('[SMC] recycle: True or False') from None
    if ('n_total' in out or 'recycle' in out) and out.get('replicas', 1) > 1:
        raise ValueError('[SMC] n_total / recycle and replicas > 1 do not combine yet: the replicas\' weighted chains cannot be merged')
    return out


def write_run(run, path, name, names, **derived):
    """The three files of an :class:`SMCRun`: (txt, paramnames, stats); ``derived``: the derived-parameter arguments of
    :func:`vega_amd.ensemble.write_getdist`."""
    pts, lnl, w = run.samples()
    keeping = getattr(run, 'keeping', False)
    if keeping:         # (getdist's weights: the largest is 1)
        derived = dict(derived, weights=w / w.max())
    txt, pn = E.write_getdist(path, name, names, pts, lnl, **derived)
    log_z, err = run.log_evidence()
    stats = Path(path) / f'{name}.stats'
    with open(stats, 'w') as f:
        f.write(f'log(Z) = {log_z!r}\nlog(Z) error = {err!r}\n')
        f.write(f'stages = {len(run.record) if keeping else run.stage}\nsweeps = {run.sweeps}\n')
        f.write(f'likelihood evaluations = {run.stats["rows"]}\n')
        f.write(f'seed = {run.seed}\nparticles = {run.particles}\ness = {run.ess!r}\n')
        f.write('beta = ' + ' '.join(repr(float(r['beta'])) for r in run.record) + '\n')
        if keeping:
            f.write(f'posterior rounds = {len(run.posterior_rounds)}\nposterior points = {lnl.size}\nn_eff = {run.n_eff()!r}\n')
            f.write(f'log(Z) recycled = {run.recycled_log_evidence()!r}\n')
    return txt, pn, stats


def read_stats(path):
    """``name.stats`` back as a dict (floats for the evidence lines and ``ess``, a list of floats for ``beta``, ints for the
    counts; ``n_eff`` and ``log(Z) recycled``, floats, where the run had ``n_total`` or ``recycle``)."""
    out = {}
    for line in Path(path).read_text().splitlines():
        key, _, val = line.partition(' = ')
        if key == 'beta':
            out[key] = [float(v) for v in val.split()]
        else:
            out[key] = float(val) if key in ('log(Z)', 'log(Z) error', 'ess', 'n_eff', 'log(Z) recycled') else int(val)
    return out
