"""Kept populations, posterior rounds and the recycled chain of the SMC sampler without a GPU: the header's section "kept
populations and posterior rounds" (vega_amd/csrc/vmx_smc.h), compiled with g++ under AddressSanitizer / UBSan into
tests/helpers/smc_keep_driver.cpp, against the NumPy restatement of vega_amd/smc.py bit for bit; nothing moves while the options
are off (tests/golden/smc_keep/before.npz: a run of the restatement as it was before the options existed); the ladder does not see
the rounds; cuts; ``recycled_weights`` against its definition in extended precision; the statistics of the recycled chain on
analytic likelihoods; the ``[SMC]`` keys; the writer; the struct."""
import configparser
import ctypes as C
import math
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vega_amd import ensemble as E
from vega_amd import smc as S


# ------------------------------------------------------------------ header <-> NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('smc_keep') / 'smc_keep_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'smc_keep_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _ask(exe, text):
    out = subprocess.run([str(exe)], input=text + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout.splitlines()


def _hx(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0].to_bytes(8, 'big').hex()


def _hexes(a):
    return ' '.join(_hx(v) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _doubles(tokens):
    return np.array([int(t, 16) for t in tokens], dtype=np.uint64).view(np.float64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _gauss_loglike(n, sigma=0.08):
    def loglike(u):
        return -0.5 * np.sum(((np.asarray(u) - 0.5) / sigma)**2, axis=1)
    return loglike


def _replay(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, stream, topups_left, loglike):
    """The restatement stage by stage, ladder stages and posterior rounds, recording what every step left behind and the answers
    the likelihood gave."""
    N = u.shape[0]
    u, lnl = u.copy(), lnl.copy()
    out, answers = [], []
    for _ in range(n_stages):
        if S.run_finished(beta, topups_left):
            break
        rec = dict(kept=u.copy(), kept_lnl=lnl.copy(), beta_prev=beta, round=beta >= 1.0, sweeps=[])
        head = S.posterior_round_head(u, lnl) if rec['round'] else S.stage_head(u, lnl, beta, ess, stage, seed, stream)
        rec['head'] = head
        assert not math.isnan(head['beta']) and (rec['round'] or head['beta'] > beta)
        u, lnl = head['u'].copy(), head['lnl'].copy()
        status, topups_left = S.run_status_kept(beta, head['beta'], topups_left)
        beta = head['beta']
        for s in range(sweeps):
            y, inside, ua = S.propose(u, head['C'], scale, stage, s, seed, stream)
            lnl_new = loglike(np.where(inside[:, None], y, u))
            answers.append(lnl_new)
            acc = S.accept(inside, lnl_new > -np.inf, beta, lnl_new, lnl, ua)
            u[acc] = y[acc]
            lnl[acc] = lnl_new[acc]
            scale = S.adapt(scale, int(acc.sum()), N)
            rec['sweeps'].append(dict(y=y, inside=inside, ua=ua, accepted=int(acc.sum()), scale=scale, u=u.copy(), lnl=lnl.copy()))
        stage += 1
        rec.update(stage=stage, topups_left=topups_left, status=status)
        out.append(rec)
    return out, answers, u, lnl, stage, beta, scale, topups_left


@pytest.mark.parametrize('n, N, case, beta0, topups, n_stages', [
    (1, 8, 'plain', 1.0, 2, 2), (2, 40, 'flat axis', 1.0, 2, 2), (6, 1100, 'minus inf', 1.0, 2, 2), (32, 40, 'plain', 1.0, 1, 1),
    (2, 40, 'ladder', 0.0, 2, 12), (6, 40, 'cut', 0.0, 3, 12), (2, 8, 'flat axis', 1.0, 1, 3)])
def test_header_equals_the_restatement_bitwise(driver, n, N, case, beta0, topups, n_stages):
    """Posterior rounds entered at beta = 1 (n = 1, 2, 6, 32; N = 8, 40, 1100; with a particle of lnL = -inf at entry, which the
    round's ESS does not count; with the diagonal fallback of a coordinate that is the same for every particle) and whole runs that
    walk the ladder and then pay their rounds ('cut': the call ends inside the rounds): the kept positions of every stage, the
    round's record row, identity ancestors, mean, covariance and factor, after every sweep the proposals, the deciding uniforms,
    the accepted count, the scale, every particle and its lnL, and after every stage the rounds still owed and the status - the
    header compiled by g++ and the NumPy restatement agree in every bit; ``python_stages`` is that same run."""
    seed, stream, sweeps, ess = 23 + n, 2, 2, 0.5
    u0 = S.draw_start(N, n, seed, stream)
    if case == 'flat axis':
        u0[:, n - 1] = 0.25
    loglike = _gauss_loglike(n, sigma=0.2 if n > 6 else 0.08)
    lnl0 = loglike(u0)
    if case == 'minus inf':
        lnl0[[3, N - 1]] = -np.inf
    stage0, scale0 = 5, S.start_scale(n)
    if case == 'cut':
        n_stages = len(_replay(u0, lnl0, stage0, 0.0, scale0, 64, ess, sweeps, seed, stream, topups, loglike)[0]) - 1
    steps, answers, u1, lnl1, stage1, beta1, scale1, left1 = _replay(u0, lnl0, stage0, beta0, scale0, n_stages, ess, sweeps, seed,
                                                                     stream, topups, loglike)
    n_rounds = sum(r['round'] for r in steps)
    assert n_rounds == (topups - 1 if case == 'cut' else topups) and left1 == topups - n_rounds
    assert beta0 == 1.0 or len(steps) - n_rounds >= 2
    text = (f'K {n} {N} {sweeps} {n_stages} {stage0} {_hx(beta0)} {_hx(scale0)} {_hx(ess)} {seed:x} {stream:x} {topups} {_hexes(u0)} '
            f'{_hexes(lnl0)} ' + ' '.join(_hexes(a) for a in answers))
    lines = iter(_ask(driver, text))

    def take(tag):
        parts = next(lines).split()
        assert parts[0] == tag, (parts[0], tag)
        return parts[1:]

    for rec in steps:
        head = rec['head']
        assert _same_bits(_doubles(take('U')), rec['kept'])
        if rec['round']:
            assert _same_bits(_doubles(take('G')), [1.0, 1.0, head['ess']]) and rec['beta_prev'] == head['beta'] == 1.0
            assert head['ess'] == float(np.count_nonzero(rec['kept_lnl'] > -np.inf))
            assert [int(t) for t in take('A')] == list(range(N)) == head['anc'].tolist()
            assert _same_bits(_doubles(take('M')), head['mean'])
            assert _same_bits(_doubles(take('V')), head['cov'])
            f = take('F')
            assert int(f[0]) == int(head['cholesky']) == (0 if case == 'flat axis' else 1)
            assert _same_bits(_doubles(f[1:]), head['C'])
        else:
            assert _same_bits(_doubles(take('H')), [rec['beta_prev'], head['beta'], head['ess']])
            assert [int(t) for t in take('A')] == head['anc'].tolist()
        for sw in rec['sweeps']:
            yl = take('Y')
            assert [int(t) for t in yl[:N]] == sw['inside'].astype(int).tolist()
            assert _same_bits(_doubles(yl[N:2 * N]), sw['ua']) and _same_bits(_doubles(yl[2 * N:]), sw['y'])
            xl = take('X')
            assert int(xl[0]) == sw['accepted']
            assert _same_bits(_doubles(xl[1:2]), [sw['scale']])
            assert _same_bits(_doubles(xl[2:2 + N * n]), sw['u']) and _same_bits(_doubles(xl[2 + N * n:]), sw['lnl'])
        assert [int(t) for t in take('T')] == [rec['stage'], rec['topups_left'], rec['status']]
    assert next(lines, None) is None
    if case == 'minus inf':
        assert steps[0]['head']['ess'] == N - 2
    last = steps[-1]
    assert last['status'] == (S.FINISHED if left1 == 0 else S.RUNNING) and (case == 'cut') == (left1 > 0)
    # python_stages is that run, its keep list the kept positions
    u, lnl, keep = u0.copy(), lnl0.copy(), []
    rec, stage, beta, scale, left, st = S.python_stages(u, lnl, stage0, beta0, scale0, n_stages, ess, sweeps, seed, stream, loglike,
                                                        topups_left=topups, keep=keep)
    assert _same_bits(u, u1) and _same_bits(lnl, lnl1) and (stage, beta, scale, left) == (stage1, beta1, scale1, left1)
    assert len(keep) == len(rec) == len(steps) and all(_same_bits(a, b['kept']) for a, b in zip(keep, steps))
    assert all(np.array_equal(a['anc'], b['head']['anc']) and a['ess'] == b['head']['ess'] for a, b in zip(rec, steps))
    assert [r['beta_prev'] >= 1.0 for r in rec] == [r['round'] for r in steps]
    assert st['rows'] == len(steps) * sweeps * N and st['stages'] == len(steps)


def test_set_statuses_with_rounds_owed(driver):
    """A set whose runs reach beta = 1 in different rounds and owe 2, 0 and 1 posterior rounds, a fourth whose ladder gets stuck
    and a fifth that enters at beta = 1 owing one round: ``first_active_kept``, ``run_status_kept`` and ``compact_active`` of the
    header against the restatement - a run that owes rounds stays RUNNING and in the list, and is FINISHED in the round that pays
    the last one."""
    beta = [0.0, 0.2, 0.0, 0.3, 1.0, 1.0]
    owed = [2, 0, 1, 1, 1, 0]
    after = {0: [0.4, 1.0, 1.0, 1.0], 1: [1.0], 2: [0.3, 0.6, 1.0, 1.0], 3: [0.5, 0.5], 4: [1.0]}
    # the restatement, round by round
    b, o = list(beta), list(owed)
    active, status = S.first_active_kept(b, o, False)
    assert active == [0, 1, 2, 3, 4] and status.tolist() == [0, 0, 0, 0, 0, 1]
    fed, expect = [], []
    k = {e: 0 for e in after}
    for _ in range(4):
        for e in active:
            a = after[e][k[e]]
            k[e] += 1
            fed.append(a)
            status[e], o[e] = S.run_status_kept(b[e], a, o[e])
            if status[e] in (S.RUNNING, S.FINISHED):
                b[e] = a
        active = S.compact_active(active, status)
        expect.append((status.tolist(), list(o), list(active)))
    assert [e[0] for e in expect] == [[0, 1, 0, 0, 1, 1], [0, 1, 0, 3, 1, 1], [0, 1, 0, 3, 1, 1], [1, 1, 1, 3, 1, 1]]
    assert expect[-1][1] == [0, 0, 0, 1, 0, 0] and [e[2] for e in expect] == [[0, 2, 3], [0, 2], [0, 2], []]
    lines = _ask(driver, f'S 6 0 {_hexes(beta)} {" ".join(map(str, owed))} 4 {_hexes(fed)}')
    assert lines[0].split()[1:] == ['0', '1', '2', '3', '4'] and lines[1].split()[1:] == ['0', '0', '0', '0', '0', '1']
    for r, (st, ow, act) in enumerate(expect):
        q, o_line, l_line = (lines[2 + 3 * r + j].split() for j in range(3))
        assert (q[0], o_line[0], l_line[0]) == ('Q', 'O', 'L')
        assert [int(t) for t in q[1:]] == st and [int(t) for t in o_line[1:]] == ow and [int(t) for t in l_line[1:]] == act
    # with draw every run begins; without rounds owed the forms are the old ones
    assert S.first_active_kept(beta, owed, True)[0] == list(range(6))
    assert S.first_active_kept(beta, [0] * 6, False)[0] == S.first_active(beta, False)[0]
    for bb, aa in ((0.2, 0.5), (0.2, 1.0), (0.2, 0.2), (0.2, math.nan)):
        assert S.run_status_kept(bb, aa, 0) == (S.run_status(bb, aa), 0)


# ------------------------------------------------------------------ nothing moves when it is off
def _set_evaluate(N, n, sig):
    def evaluate(rows, runs):
        rows = rows.reshape(len(runs), N, n)
        return np.concatenate([-0.5 * np.sum(((rows[a] - 0.5) / sig[r])**2, axis=1) for a, r in enumerate(runs)])
    return evaluate


def test_the_defaults_are_the_run_before():
    """``python_stages`` and ``python_stages_many`` at their defaults against the arrays a run of the restatement left before the
    options existed (tests/golden/smc_keep/before.npz): every particle, lnL, ancestor, beta and count, bit for bit, and the old
    return shapes."""
    g = np.load(REPO / 'tests' / 'golden' / 'smc_keep' / 'before.npz')
    n, N, sweeps, seed, stream = 2, 40, 3, 7, 1
    ll = _gauss_loglike(n)
    u = S.draw_start(N, n, seed, stream)
    lnl = ll(u)
    assert _same_bits(u, g['single_u0']) and _same_bits(lnl, g['single_lnl0'])
    out = S.python_stages(u, lnl, 0, 0.0, S.start_scale(n), 4, 0.5, sweeps, seed, stream, ll)
    assert len(out) == 5
    rec, stage, beta, scale, st = out
    assert _same_bits(u, g['single_u']) and _same_bits(lnl, g['single_lnl']) and _same_bits([stage, beta, scale], g['single_state'])
    assert _same_bits([r['beta'] for r in rec], g['single_beta']) and _same_bits([r['ess'] for r in rec], g['single_ess'])
    assert np.array_equal([r['anc'] for r in rec], g['single_anc']) and _same_bits([r['lnl'] for r in rec], g['single_rec_lnl'])
    assert [r['accepted'] for r in rec] == g['single_accepted'].tolist() and [st[k] for k in sorted(st)] == g['single_stats'].tolist()
    assert all('u' not in r for r in rec)
    E_, N = 3, 24
    u, lnl = np.zeros((E_, N, n)), np.zeros((E_, N))
    stage, beta, scale = np.zeros(E_, dtype=np.int64), np.zeros(E_), np.zeros(E_)
    out = S.python_stages_many(u, lnl, stage, beta, scale, 3, 0.5, sweeps, seed, np.array([0, 1, 1], dtype=np.uint64),
                               _set_evaluate(N, n, [0.08, 0.2, 0.05]), draw=True)
    assert len(out) == 4
    recs, status, done, st = out
    assert _same_bits(u, g['set_u']) and _same_bits(lnl, g['set_lnl']) and np.array_equal(stage, g['set_stage'])
    assert _same_bits(beta, g['set_beta']) and _same_bits(scale, g['set_scale'])
    assert np.array_equal(status, g['set_status']) and np.array_equal(done, g['set_done']) and status.tolist() == [1, 1, 0]
    assert np.array_equal(st['per_run'], g['set_per_run']) and st['rounds'] == int(g['set_rounds'])
    assert np.array_equal([r['anc'] for e in range(E_) for r in recs[e]], g['set_anc'])
    assert _same_bits([r['beta'] for e in range(E_) for r in recs[e]], g['set_rec_beta'])


def _correlated_gaussian(n, sigma=0.03, rho=0.5):
    """A normalised Gaussian at the centre of the unit cube: log Z = 0 (its mass outside the cube is below 1e-50)."""
    cov = sigma**2 * ((1 - rho) * np.eye(n) + rho * np.ones((n, n)))
    icov = np.linalg.inv(cov)
    log_det = np.linalg.slogdet(2 * np.pi * cov)[1]

    def loglike(u):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ij,jk,ik->i', d, icov, d) - 0.5 * log_det
    return loglike


KW = dict(particles=128, sweeps=4, seed=4, stream=1)


@pytest.fixture(scope='module')
def base_run():
    return S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, **KW).run()


@pytest.fixture(scope='module')
def topped_run():
    return S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=4 * 128, **KW).run()


def test_without_the_options_samples_are_the_particles(base_run):
    run = base_run
    pts, lnl, w = run.samples()
    assert np.array_equal(pts, run.u) and np.array_equal(lnl, run.lnl) and np.array_equal(w, np.full(128, 1.0 / 128))
    assert run.finished and not run.keeping and run.posterior_rounds == [] and run.topups_left == 0
    assert all('u' not in r for r in run.record) and run.n_eff() == pytest.approx(128.0, rel=1e-12)
    with pytest.raises(ValueError, match='n_total or recycle'):
        run.populations()


def test_the_ladder_does_not_see_the_rounds(base_run, topped_run):
    """``n_total = 4 N``: the ladder's record, ancestors and evidence are those of the run without it, bit for bit; the final
    ladder particles are the first beta = 1 population; three rounds follow, each N sweeps rows."""
    base, run = base_run, topped_run
    assert run.finished and run.rounds == 3 and len(run.posterior_rounds) == 3 and run.topups_left == 0
    assert len(run.record) == len(base.record) > 2 and run.stage == base.stage + 3
    for a, b in zip(run.record, base.record):
        assert (a['beta_prev'], a['beta'], a['ess'], a['accepted'], a['scale'], a['cholesky']) == \
            (b['beta_prev'], b['beta'], b['ess'], b['accepted'], b['scale'], b['cholesky'])
        assert np.array_equal(a['anc'], b['anc']) and _same_bits(a['lnl'], b['lnl'])
    assert run.log_evidence() == base.log_evidence() and np.array_equal(run.stages['beta'], base.stages['beta'])
    u, lnl, beta, log_z = run.populations()
    S_ = len(run.record)
    assert u.shape == (S_ + 4, 128, 3) and np.array_equal(beta[:S_], base.stages['beta_prev']) and np.all(beta[S_:] == 1.0)
    assert _same_bits(u[S_], base.u) and _same_bits(lnl[S_], base.lnl)
    assert log_z[0] == 0.0 and np.all(log_z[S_:] == run.log_evidence()[0])
    for r in run.posterior_rounds:
        assert r['beta_prev'] == r['beta'] == 1.0 and r['ess'] == 128.0 and np.array_equal(r['anc'], np.arange(128))
    assert run.stats['rows'] == base.stats['rows'] + 3 * 4 * 128
    pts, lnl_c, w = run.samples()
    assert pts.shape == (512, 3) and np.all(w == 1.0 / 512) and _same_bits(pts[:128], base.u) and _same_bits(pts[384:], run.u)
    assert run.n_eff() == pytest.approx(512.0, rel=1e-12)
    for bad in (127, 3.5, True):
        with pytest.raises(ValueError, match='n_total'):
            S.SMCRun(_correlated_gaussian(3), 3, n_total=bad, **KW)
    with pytest.raises(ValueError, match='recycle'):
        S.SMCRun(_correlated_gaussian(3), 3, recycle='yes', **KW)
    with pytest.raises(ValueError, match='bytes'):
        S.SMCRun(_correlated_gaussian(32, sigma=0.2), 32, particles=4096, n_total=4096 * 1100)
    assert S.posterior_rounds_for(None, 128) == 0 and S.posterior_rounds_for(128, 128) == 0 and S.posterior_rounds_for(129, 128) == 1


def test_the_run_does_not_depend_on_the_cut(topped_run):
    """``run(1)`` repeated - cut on the ladder, at beta = 1 and inside the rounds - is ``run()`` bit for bit in particles,
    populations and record; so is a run whose ladder ``max_stages`` would have cut one stage early, continued."""
    one = topped_run
    cut = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=4 * 128, **KW)
    seen = []
    while not cut.finished:
        cut.run(stages=1)
        seen.append((cut.beta, cut.topups_left))
    assert cut.stats['calls'] == one.stage and seen[-4:] == [(1.0, 3), (1.0, 2), (1.0, 1), (1.0, 0)] and one.stats['calls'] == 1
    two = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=4 * 128, **KW).run(stages=len(one.record) + 1).run()
    for other in (cut, two):
        assert _same_bits(one.u, other.u) and _same_bits(one.lnl, other.lnl) and one.scale == other.scale and one.stage == other.stage
        for a, b in zip(one.populations(), other.populations()):
            assert _same_bits(a, b)
        assert len(one.posterior_rounds) == len(other.posterior_rounds) and one.log_evidence() == other.log_evidence()
        for a, b in zip(one.record + one.posterior_rounds, other.record + other.posterior_rounds):
            assert (a['beta'], a['ess'], a['accepted'], a['scale']) == (b['beta'], b['ess'], b['accepted'], b['scale'])
    # max_stages bounds the ladder alone
    short = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=4 * 128, max_stages=len(one.record) - 1, **KW).run()
    assert not short.finished and short.beta < 1.0 and short.posterior_rounds == [] and short.topups_left == 3
    full = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=4 * 128, max_stages=len(one.record), **KW).run()
    assert full.finished and _same_bits(full.u, one.u) and len(full.posterior_rounds) == 3


def test_a_set_of_three_is_three_runs():
    """Three runs advanced together by ``python_stages_many`` with rounds owed (2, 0, 1), whole and cut round by round, each
    against ``python_stages`` on its stream: particles, kept positions, records and the rounds owed, bit for bit."""
    n, N, sweeps, seed = 2, 24, 3, 7
    streams, sig, owed0 = np.array([0, 1, 1], dtype=np.uint64), [0.08, 0.2, 0.05], [2, 0, 1]
    ev = _set_evaluate(N, n, sig)

    def new():
        return (np.zeros((3, N, n)), np.zeros((3, N)), np.zeros(3, dtype=np.int64), np.zeros(3), np.zeros(3),
                np.array(owed0, dtype=np.int32), [[] for _ in range(3)], [[] for _ in range(3)])

    u, lnl, stage, beta, scale, owed, keep, recs = new()
    r, status, done, left, st = S.python_stages_many(u, lnl, stage, beta, scale, 64, 0.5, sweeps, seed, streams, ev, draw=True,
                                                     topups_left=owed, keep=keep)
    assert left is owed and owed.tolist() == [0, 0, 0] and status.tolist() == [1, 1, 1] and np.all(beta == 1.0)
    cu, cl, cs, cb, csc, cowed, ckeep, crecs = new()
    first, history = True, []
    while True:
        r1, cstat, cdone, _, cst = S.python_stages_many(cu, cl, cs, cb, csc, 1, 0.5, sweeps, seed, streams, ev, draw=first,
                                                        topups_left=cowed, keep=ckeep)
        first = False
        for e in range(3):
            crecs[e].extend(r1[e])
        history.append(cstat.tolist())
        if np.all(cstat == S.FINISHED):
            break
    assert _same_bits(cu, u) and _same_bits(cl, lnl) and np.array_equal(cs, stage) and _same_bits(csc, scale)
    assert [len(k) for k in ckeep] == [len(k) for k in keep] == done.tolist() == [len(x) for x in crecs]
    ends = [min(k for k, h in enumerate(history) if h[e] == S.FINISHED) for e in range(3)]
    assert history[-1] == [1, 1, 1] and len(set(ends)) > 1 and len(history) == max(done)
    for e in range(3):
        ll = (lambda s: lambda rows: -0.5 * np.sum(((rows - 0.5) / s)**2, axis=1))(sig[e])
        su = S.draw_start(N, n, seed, int(streams[e]))
        sl = ll(su)
        k1 = []
        rec, s1, b1, sc1, left1, _ = S.python_stages(su, sl, 0, 0.0, S.start_scale(n), 64, 0.5, sweeps, seed, int(streams[e]), ll,
                                                     topups_left=owed0[e], keep=k1)
        assert _same_bits(su, u[e]) and _same_bits(sl, lnl[e]) and (s1, b1, sc1, left1) == (stage[e], 1.0, scale[e], 0)
        assert len(k1) == len(keep[e]) and all(_same_bits(a, b) and _same_bits(a, c) for a, b, c in zip(k1, keep[e], ckeep[e]))
        assert sum(x['beta_prev'] >= 1.0 for x in rec) == owed0[e] == sum(x['beta_prev'] >= 1.0 for x in r[e])
        assert all(np.array_equal(a['anc'], b['anc']) and _same_bits(a['lnl'], b['lnl']) for a, b in zip(rec, r[e]))
        assert st['per_run'][e, 3] == (len(rec) * sweeps + 1) * N


# ------------------------------------------------------------------ recycled_weights against its definition
def _definition(betas, log_z, lnl):
    """O(S N S) loops in long double: w = L / sum_s N L^beta_s / Z_s, normalised; log of the sum of the unnormalised ones."""
    ld = np.longdouble
    S_, N = lnl.shape
    raw = np.zeros((S_, N), dtype=ld)
    for s in range(S_):
        for i in range(N):
            l = ld(lnl[s, i])
            if lnl[s, i] == -np.inf:
                continue
            top = max(ld(betas[t]) * l - ld(log_z[t]) for t in range(S_))
            mix = ld(0)
            for t in range(S_):
                mix += ld(N) * np.exp(ld(betas[t]) * l - ld(log_z[t]) - top)
            raw[s, i] = np.exp(l - top) / mix
    total = raw.sum()
    return raw / total, np.log(total)


@pytest.mark.parametrize('case', ['ladder', 'minus inf', 'one stage', 'rounds'])
def test_recycled_weights_against_the_definition(case):
    """``recycled_weights`` at 1e-13 against loops over its definition in extended precision (the lnL are kept within a range
    whose exponentials long double holds): a ladder's populations; with a point of lnL = -inf (weight 0, no part in the sums); a
    one-stage ladder (the start and the final population: R = 0); with three beta = 1 populations."""
    rng = np.random.default_rng(3)
    N = 7
    if case == 'one stage':
        betas, log_z = np.array([0.0, 1.0]), np.array([0.0, -1.3])
    elif case == 'rounds':
        betas, log_z = np.array([0.0, 0.3, 1.0, 1.0, 1.0]), np.array([0.0, -2.0, -3.1, -3.1, -3.1])
    else:
        betas, log_z = np.array([0.0, 0.1, 0.45, 1.0]), np.array([0.0, -1.0, -2.2, -2.9])
    lnl = -rng.exponential(4.0, size=(betas.size, N)) * (1.0 + 3.0 * (1.0 - betas[:, None])) + 5.0
    if case == 'minus inf':
        lnl[0, 2] = lnl[2, 5] = -np.inf
    w, log_zr = S.recycled_weights(betas, log_z, lnl)
    ref, ref_z = _definition(betas, log_z, lnl)
    assert w.shape == lnl.shape and abs(w.sum() - 1.0) <= 1e-13
    assert np.max(np.abs(w - ref.astype(np.float64))) <= 1e-13 and abs(log_zr - float(ref_z)) <= 1e-13
    if case == 'minus inf':
        assert w[0, 2] == 0.0 and w[2, 5] == 0.0 and np.all(w[lnl > -np.inf] > 0.0)
    if case == 'one stage':     # (two populations: the weight is L / (N + N L / Z), by hand)
        by_hand = np.exp(lnl) / (N + N * np.exp(lnl - log_z[1]))
        assert np.allclose(w, by_hand / by_hand.sum(), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        S.recycled_weights(betas[:-1], log_z, lnl)


# ------------------------------------------------------------------ statistics on analytic likelihoods
def _pulls(pts, w, sigma, N):
    mean = np.sum(w[:, None] * pts, axis=0)
    sd = np.sqrt(np.sum(w[:, None] * (pts - mean)**2, axis=0))
    return (mean - 0.5) / (sigma / math.sqrt(N)), (sd - sigma) / (sigma / math.sqrt(2 * N))


@pytest.mark.parametrize('n, N, seed', [(2, 512, 3), (6, 1024, 3)])
def test_recycled_chain_of_a_gaussian(n, N, seed):
    """Correlated Gaussians (rho = 0.5, sigma = 0.03), ``recycle=True``: the weights sum to 1 within 1e-12; Kish's n_eff >= 1.5 N
    (0.77 of the lowest figure seen); |log_z_recycled - log Z| <= err; every coordinate's weighted mean within 5 sigma / sqrt(N)
    and every weighted sd within 5 sigma / sqrt(2 N) of sigma - the base chain's own bars, because the populations are
    correlated and Kish does not see it.  With ``n_total = 4 N`` on top: n_eff >= 4 N, the same bars.

    Seeds 0 .. 5 of this restatement, n = 2 / N = 512 and n = 6 / N = 1024: n_eff / N 2.48 - 2.74 and 1.95 - 2.05 (stages 5 and
    9), |log_z_recycled - log Z| at most 0.22 err, worst mean pull 1.39, worst sd pull 1.00; with n_total = 4 N: n_eff / N 5.64 -
    5.88 and 5.18 - 5.30, worst mean pull 0.81, worst sd pull 0.92, acceptance of the rounds 0.21 - 0.31."""
    sigma = 0.03
    run = S.SMCRun(_correlated_gaussian(n), n, particles=N, seed=seed, recycle=True).run()
    pts, lnl, w = run.samples()
    log_z, err = run.log_evidence()
    mean_pull, sd_pull = _pulls(pts, w, sigma, N)
    print(f'n = {n}: recycled n_eff / N {run.n_eff() / N:.3f}, {len(run.record)} stages, log Z {log_z:+.4f} +- {err:.4f}, recycled '
          f'{run.recycled_log_evidence():+.4f}, mean pulls {np.round(mean_pull, 2)}, sd pulls {np.round(sd_pull, 2)}')
    assert pts.shape == ((len(run.record) + 1) * N, n) and abs(w.sum() - 1.0) <= 1e-12
    assert run.n_eff() >= 1.5 * N
    assert abs(run.recycled_log_evidence() - log_z) <= err
    assert np.all(np.abs(mean_pull) <= 5) and np.all(np.abs(sd_pull) <= 5)
    assert run.samples(recycle=False)[0].shape == (N, n) and run.n_eff(recycle=False) == pytest.approx(N, rel=1e-12)
    more = S.SMCRun(_correlated_gaussian(n), n, particles=N, seed=seed, recycle=True, n_total=4 * N).run()
    pts, lnl, w = more.samples()
    mean_pull, sd_pull = _pulls(pts, w, sigma, N)
    acc = [r['accepted'] / (N * more.sweeps) for r in more.posterior_rounds]
    print(f'n = {n}: with n_total = 4 N n_eff / N {more.n_eff() / N:.3f}, acceptance of the rounds {np.round(acc, 3)}, mean pulls '
          f'{np.round(mean_pull, 2)}, sd pulls {np.round(sd_pull, 2)}')
    assert more.log_evidence() == run.log_evidence() and abs(w.sum() - 1.0) <= 1e-12
    assert more.n_eff() >= 4 * N
    assert np.all(np.abs(mean_pull) <= 5) and np.all(np.abs(sd_pull) <= 5)


def _two_modes(n=4, sigma=0.02):
    def loglike(u):
        u = np.asarray(u)
        a = -0.5 * np.sum(((u - 0.3) / sigma)**2, axis=1)
        b = -0.5 * np.sum(((u - 0.7) / sigma)**2, axis=1)
        return np.logaddexp(a, b) - math.log(2.0) - 0.5 * n * math.log(2 * math.pi * sigma * sigma)
    return loglike


def test_recycled_chain_keeps_the_masses_of_two_modes():
    """Two separated Gaussians (n = 4, N = 1024, seed 2): the recycled mass of the lower mode is within 8 err of 1/2 in log ratio
    (the bar of tests/test_smc_host.py) and differs from the final particles' mass by at most 0.02.  Measured: 0.517 against 0.518
    (seed 2) and 0.411 against 0.409; n_eff 2.7 - 2.9 N."""
    run = S.SMCRun(_two_modes(), 4, particles=1024, seed=2, recycle=True).run()
    err = run.log_evidence()[1]
    pts, _, w = run.samples()
    p_rec = float(w[pts.sum(axis=1) < 2.0].sum())
    p_last = float((run.samples(recycle=False)[0].sum(axis=1) < 2.0).mean())
    print(f'two modes: recycled mass of the lower mode {p_rec:.4f}, of the final particles {p_last:.4f}, n_eff / N {run.n_eff() / 1024:.2f}')
    assert abs(math.log(p_rec / (1.0 - p_rec))) <= 8 * err
    assert abs(p_rec - p_last) <= 0.02


# ------------------------------------------------------------------ the single run is the set of one
from vega_amd.smc import accept, adapt, posterior_round_head, propose, run_finished, stage_head  # noqa: E402  (the names the body below reads)


def _reference_python_stages(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, stream, evaluate, watch=None, topups_left=0, keep=None):
    """Up to ``n_stages`` stages in NumPy from the state ``u`` [N, n], ``lnl`` [N] (updated in place), stopping after the stage
    that reaches beta = 1.  ``evaluate(rows_u)`` -> lnL [N] of rows in the cube (-inf: a failed model).  ``watch(stage, sweep, u,
    lnl, scale, accepted)`` is called after every sweep.  Returns (record: a list of dicts per stage with beta_prev, beta, ess,
    lnl (before reweighting), anc, accepted, scale, cholesky; stage, beta, scale, stats).

    ``topups_left`` posterior rounds are owed at beta = 1 (vmx_smc.h: "kept populations and posterior rounds"): the run then goes
    on with stages headed by :func:`posterior_round_head`, one record row each (beta_prev = beta = 1), ``n_stages`` bounding both
    kinds together.  ``keep``, a list, receives the particles at the entry of every stage done.  With either, the rounds still
    owed are returned after ``scale``: (record, stage, beta, scale, topups_left, stats)."""
    N, n = u.shape
    record = []
    new_form = keep is not None or bool(topups_left)
    topups_left = int(topups_left)
    st = dict(stages=0, sweeps=0, rows=0, rows_own_position=0, accepted=0, rejected_failed_model=0)
    for _ in range(n_stages):
        if run_finished(beta, topups_left):
            break
        if keep is not None:
            keep.append(u.copy())
        if beta >= 1.0:
            head = posterior_round_head(u, lnl)
            topups_left -= 1
        else:
            head = stage_head(u, lnl, beta, ess, stage, seed, stream)
        if math.isnan(head['beta']):
            raise ValueError('SMC: no particle has a finite log-likelihood')
        if beta < 1.0 and not head['beta'] > beta:
            raise ValueError('SMC: the temperature ladder cannot advance: fewer than ess N particles carry weight')
        rec = dict(beta_prev=beta, beta=head['beta'], ess=head['ess'], lnl=lnl.copy(), anc=head['anc'], cholesky=head['cholesky'])
        u[:], lnl[:] = head['u'], head['lnl']
        beta = head['beta']
        acc_stage = 0
        for s in range(sweeps):
            y, inside, ua = propose(u, head['C'], scale, stage, s, seed, stream)
            lnl_new = np.asarray(evaluate(np.where(inside[:, None], y, u)), dtype=np.float64)
            ok = lnl_new > -np.inf
            acc = accept(inside, ok, beta, lnl_new, lnl, ua)
            u[acc] = y[acc]
            lnl[acc] = lnl_new[acc]
            k = int(acc.sum())
            scale = adapt(scale, k, N)
            acc_stage += k
            st['rows'] += N
            st['rows_own_position'] += int((~inside).sum())
            st['rejected_failed_model'] += int((inside & ~ok).sum())
            if watch is not None:
                watch(stage, s, u, lnl, scale, k)
        st['sweeps'] += sweeps
        st['accepted'] += acc_stage
        st['stages'] += 1
        rec.update(accepted=acc_stage, scale=scale)
        record.append(rec)
        stage += 1
    if new_form:
        return record, stage, beta, scale, topups_left, st
    return record, stage, beta, scale, st


def _both(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, stream, loglike, **kw):
    """``python_stages`` and the body it had before it became the set of one (above, verbatim), each on its own copy of the state:
    everything they hand back and leave behind is equal, bit for bit.  Returns what the reference returned, its u and lnl."""
    out = []
    for run in (_reference_python_stages, S.python_stages):
        own = dict(kw, keep=[]) if 'keep' in kw else dict(kw)
        uu, ll = u.copy(), lnl.copy()
        out.append((run(uu, ll, stage, beta, scale, n_stages, ess, sweeps, seed, stream, loglike, **own), uu, ll, own.get('keep')))
    (ref, ru, rl, rk), (got, gu, gl, gk) = out
    assert np.array_equal(ru, gu) and np.array_equal(rl, gl) and len(ref) == len(got) and len(ref[0]) == len(got[0])
    for a, b in zip(ref[0], got[0]):
        assert set(a) == set(b) == {'beta_prev', 'beta', 'ess', 'lnl', 'anc', 'accepted', 'scale', 'cholesky'}
        for key in a:
            assert np.array_equal(a[key], b[key]) and type(a[key]) is type(b[key]), key
    assert ref[1:-1] == got[1:-1] and [type(v) for v in ref[1:-1]] == [type(v) for v in got[1:-1]]     # stage, beta, scale(, topups_left)
    assert ref[-1] == got[-1] and list(ref[-1]) == list(got[-1])
    assert (rk is None) == (gk is None)
    if rk is not None:
        assert len(rk) == len(gk) == len(ref[0]) and all(np.array_equal(a, b) for a, b in zip(rk, gk))
    return ref, ru, rl


def _drawn(N, n, seed, stream, loglike):
    u = np.ascontiguousarray(S.draw_start(N, n, seed, stream))
    return u, loglike(u)


def test_one_run_from_a_fresh_draw_and_entered_on_the_ladder():
    """(a) from the start particles of stream 5; (b) entered at stage 3 with beta inside (0, 1), two more stages."""
    N, n, loglike = 64, 2, _gauss_loglike(2, sigma=0.01)
    u, lnl = _drawn(N, n, 9, 5, loglike)
    ref, u3, lnl3 = _both(u, lnl, 0, 0.0, S.start_scale(n), 3, 0.5, 4, 9, 5, loglike)
    rec, stage, beta, scale, st = ref
    assert stage == 3 and 0.0 < beta < 1.0 and st['stages'] == 3 and st['rows'] == 3 * 4 * N
    ref = _both(u3, lnl3, stage, beta, scale, 2, 0.5, 4, 9, 5, loglike)[0]
    assert ref[1] == 5 and ref[0][0]['beta_prev'] == beta and ref[-1]['stages'] == 2


def test_one_run_cut_inside_its_posterior_rounds():
    """(c) two rounds owed and a list for the kept populations; ``n_stages`` ends the call after the first round."""
    N, n, loglike = 64, 2, _gauss_loglike(2)
    u, lnl = _drawn(N, n, 4, 0, loglike)
    ladder = len(_reference_python_stages(u.copy(), lnl.copy(), 0, 0.0, S.start_scale(n), 64, 0.5, 4, 4, 0, loglike)[0])
    assert 3 <= ladder < 64
    ref, u1, lnl1 = _both(u, lnl, 0, 0.0, S.start_scale(n), ladder + 1, 0.5, 4, 4, 0, loglike, topups_left=2, keep=[])
    rec, stage, beta, scale, left, st = ref
    assert (stage, beta, left) == (ladder + 1, 1.0, 1) and rec[-1]['beta_prev'] == 1.0 and rec[-2]['beta_prev'] < 1.0
    ref = _both(u1, lnl1, stage, beta, scale, 5, 0.5, 4, 4, 0, loglike, topups_left=left, keep=[])[0]      # (entered at beta = 1)
    assert (ref[1], ref[4], len(ref[0])) == (ladder + 2, 0, 1)
    assert len(_both(u1, lnl1, ref[1], 1.0, ref[3], 5, 0.5, 4, 4, 0, loglike, topups_left=0, keep=[])[0][0]) == 0       # (nothing is left)


@pytest.mark.parametrize('N', [24, 1056])
def test_one_run_at_awkward_sizes(N):
    """(d) N = 24: not a power of two, fewer than a wavefront; N = 1056: beyond LANES, two particles per segment."""
    n, loglike = 2, _gauss_loglike(2)
    u, lnl = _drawn(N, n, 2, 1, loglike)
    assert N < 64 or (N > S.LANES and -(-N // S.LANES) == 2)
    ref = _both(u, lnl, 0, 0.0, S.start_scale(n), 2, 0.5, 3, 2, 1, loglike)[0]
    assert ref[1] == 2 and ref[-1]['rows'] == 2 * 3 * N
    _both(u, lnl, 0, 0.0, S.start_scale(n), 2, 0.5, 3, 2, 1, loglike, keep=[])


@pytest.mark.parametrize('case, match', [('none finite', 'no particle has a finite log-likelihood'), ('one finite', 'cannot advance')])
def test_one_run_that_cannot_go_on(case, match):
    """(e) no particle with a finite lnL at the head; (f) one among -inf: ESS = 1 at every beta, below ess N.  The exception has the
    reference's text, and ``u`` / ``lnl`` are left as the reference left them - it raised before it touched them, the set's
    body puts a failed run's entry state back.  (The reference had appended the entry particles to ``keep`` by then; the list is
    now left as it was.)"""
    N, n, loglike = 16, 2, _gauss_loglike(2)
    u = np.ascontiguousarray(S.draw_start(N, n, 1, 0))
    lnl = np.full(N, -np.inf)
    if case == 'one finite':
        lnl[-1] = 0.0
    left, texts = [], []
    for run in (_reference_python_stages, S.python_stages):
        uu, ll, keep = u.copy(), lnl.copy(), ['before']
        with pytest.raises(ValueError, match=match) as err:
            run(uu, ll, 0, 0.0, S.start_scale(n), 3, 0.5, 3, 1, 0, loglike, keep=keep)
        left.append((uu, ll, keep))
        texts.append(str(err.value))
    assert texts[0] == texts[1]
    assert np.array_equal(left[0][0], left[1][0]) and np.array_equal(left[0][1], left[1][1])
    assert np.array_equal(left[1][0], u) and np.array_equal(left[1][1], lnl)
    assert len(left[0][2]) == 2 and left[1][2] == ['before']


# ------------------------------------------------------------------ config, writer, struct
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = SMC\n'
MC = '[control]\nrun_sampler = True\nsampler = SMC\nrun_montecarlo = True\n[monte carlo]\nnum_mocks = 3\n'


def test_the_new_keys(tmp_path):
    s = E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\nparticles = 256\nn_total = 1000\nrecycle = True\n'), SAMPLE)
    assert s['n_total'] == 1000 and s['recycle'] is True and s['particles'] == 256
    assert E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\nrecycle = no\n'), SAMPLE)['recycle'] is False
    d = E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\n'), SAMPLE)
    assert 'n_total' not in d and 'recycle' not in d
    m = E.sampler_settings(_config(MC + f'[SMC]\npath = {tmp_path}\nmocks = 3\nn_total = 2048\nrecycle = True\n'), SAMPLE)
    assert (m['mocks'], m['n_total'], m['recycle']) == (3, 2048, True)
    t = E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\ntogether = True\nreplicas = 1\nn_total = 2048\n'), SAMPLE)
    assert (t['together'], t['n_total'], t['replicas']) == (True, 2048, 1)


@pytest.mark.parametrize('lines, match', [
    ('particles = 256\nn_total = 255\n', 'n_total'), ('n_total = many\n', 'n_total'), ('n_total = 1023\n', 'n_total'),
    ('recycle = perhaps\n', 'recycle'), ('replicas = 2\nn_total = 2048\n', 'replicas'), ('replicas = 2\nrecycle = True\n', 'replicas'),
    ('replicas = 2\ntogether = True\nrecycle = False\n', 'replicas')])
def test_the_new_keys_refusals(tmp_path, lines, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\n' + lines), SAMPLE)


def test_writer_round_trip(tmp_path, topped_run):
    """The chain written is the chain ``samples()`` gives, with getdist weights (the largest is 1); ``name.stats`` gains its four
    lines with an option and has none of them without."""
    run = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, n_total=300, recycle=True, **KW).run()
    names = ['a', 'b', 'c']
    txt, pn, stats = S.write_run(run, tmp_path, 'run', names)
    table = np.loadtxt(txt)
    pts, lnl, w = run.samples()
    assert table.shape == ((len(run.record) + 3) * 128, 5) and table[:, 0].max() == 1.0
    assert np.allclose(table[:, 0] / table[:, 0].sum(), w, rtol=1e-14, atol=0)
    assert np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    back = S.read_stats(stats)
    assert (back['log(Z)'], back['log(Z) error']) == run.log_evidence() and back['stages'] == len(run.record) == run.stage - 2
    assert back['posterior rounds'] == 2 and back['posterior points'] == lnl.size and back['n_eff'] == run.n_eff()
    assert back['log(Z) recycled'] == run.recycled_log_evidence() and back['beta'] == run.stages['beta'].tolist()
    assert back['likelihood evaluations'] == run.stats['rows'] == 128 * (1 + 4 * run.stage)
    # equal weights with n_total alone
    txt, _, stats = S.write_run(topped_run, tmp_path, 'top', names)
    table = np.loadtxt(txt)
    assert table.shape == (512, 5) and np.all(table[:, 0] == 1.0) and S.read_stats(stats)['n_eff'] == pytest.approx(512.0)
    plain = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, **KW).run()
    _, _, stats = S.write_run(plain, tmp_path, 'plain', names)
    assert set(S.read_stats(stats)) == {'log(Z)', 'log(Z) error', 'stages', 'sweeps', 'likelihood evaluations', 'seed', 'particles',
                                        'ess', 'beta'}


def test_keep_struct_and_exports_match_the_library():
    """vmx_smc_keep (vmx_struct_size index 21) agrees with the ctypes binding, and the two kept calls are exported and bound."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    assert lib.vmx_struct_size(21) == C.sizeof(engine.SmcKeep) == 24 and lib.vmx_struct_size(22) == -1
    for name in ('vmx_smc_run_kept', 'vmx_smc_run_many_kept'):
        assert name in engine.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(lib.vmx_smc_run_kept.argtypes) == len(lib.vmx_smc_run.argtypes) + 1
    assert len(lib.vmx_smc_run_many_kept.argtypes) == len(lib.vmx_smc_run_many.argtypes) + 1
