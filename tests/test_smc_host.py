"""The SMC sampler without a GPU: the header the device kernels are built from (vega_amd/csrc/vmx_smc.h), compiled with g++ under
AddressSanitizer / UBSan into tests/helpers/smc_driver.cpp, against the NumPy restatement of vega_amd/smc.py bit for bit - its
own exp, the Philox counters, the temperature ladder, the ancestors, whole stages and runs; the restatement's evidence on analytic
likelihoods (correlated Gaussians, two separated modes); independence of how a run is cut; failed models; the ``[SMC]`` config
checks; the writers; the structs."""
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
    exe = tmp_path_factory.mktemp('smc') / 'smc_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'smc_driver.cpp')]
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


def test_blocks_use_the_documented_counters(driver):
    """Particle i at (stage t, sweep s), block j: counter (i, t 2^32 + s, j, 3); resampling of stage t: (0, t, 0, 4); start
    particle i, block j: (i, 0, j, 5) - against NumPy's Philox (which increments before it encrypts) and against the header."""
    b = S.move_blocks(np.arange(5), 17, 6, np.array([0, 1, 2, 3, 8]), seed=9, stream=2)
    for i, j in zip(range(5), (0, 1, 2, 3, 8)):
        c = i | (((17 << 32) + 6) << 64) | (j << 128) | (3 << 192)
        assert np.array_equal(b[i], np.random.Philox(key=[9, 2], counter=c - 1).random_raw(4))
        got = _ask(driver, f'P {i} 17 6 {j} 9 2')[0].split()[1:]
        assert [int(t, 16) for t in got] == [int(x) for x in b[i]]
    v = S.resample_uniform(12, seed=4, stream=1)
    words = np.random.Philox(key=[4, 1], counter=((12 << 64) | (4 << 192)) - 1).random_raw(4)
    assert v == E.u01(words[0])
    assert _same_bits(_doubles(_ask(driver, 'V 12 4 1')[0].split()[1:]), [v])
    u = S.draw_start(7, 6, seed=3, stream=1)
    for i in range(7):
        words = np.concatenate([np.random.Philox(key=[3, 1], counter=(i | (j << 128) | (5 << 192)) - 1).random_raw(4)
                                for j in range(2)])
        assert np.array_equal(u[i], E.u01(words[:6]))
    assert _same_bits(_doubles(_ask(driver, 'D 7 6 3 1')[0].split()[1:]), u)
    assert np.all(u >= 0) and np.all(u < 1)


EXP_ULP = 2     # measured over the grid below: 1.0 ulp of math.exp at most (the polynomial's and the reduction's roundings)


def test_the_pinned_exp(driver):
    """pexp on a grid covering [-745, 0] and beyond, the points next to every reduction boundary (k + 1/2) ln 2, and the special
    values: the header and NumPy agree in every bit, both stay within EXP_ULP ulp of the C library's exp (measured: at most 1.0
    ulp over these 70 000 points, 0.5 ulp in the subnormals), never decrease, and give exp(0) = 1."""
    grid = np.linspace(-745.0, 0.0, 60001)
    edges = (np.arange(-1075, 1)[:, None] + 0.5) * math.log(2.0)
    edges = np.sort(np.concatenate([np.nextafter(edges, -np.inf), edges, np.nextafter(edges, np.inf)], axis=1).reshape(-1))
    rng = np.random.default_rng(1)
    x = np.sort(np.concatenate([grid, edges[(edges <= 0) & (edges > -746)], -rng.random(4000) * 745.0, -10.0**rng.uniform(-300, 0, 2000)]))
    special = np.array([0.0, -0.0, -745.13, -745.2, -745.3, -746.0, -1e308, -np.inf, np.nan, -5e-324, -1e-17, -708.4, -709.0])
    got = S.pexp(np.concatenate([x, special]))
    hdr = _doubles(_ask(driver, f'E {x.size + special.size} ' + _hexes(np.concatenate([x, special])))[0].split()[1:])
    assert _same_bits(got, hdr)
    y = got[:x.size]
    ref = np.array([math.exp(v) for v in x])
    ulp = np.abs(y - ref) / np.spacing(ref)
    print(f'pexp: {x.size} points, worst {ulp.max():.2f} ulp of math.exp at x = {x[np.argmax(ulp)]!r}')
    assert ulp.max() <= EXP_ULP
    assert np.all(np.diff(y) >= 0)
    sp = got[x.size:]
    assert sp[0] == 1.0 and sp[1] == 1.0 and sp[9] == 1.0 and sp[10] == 1.0
    assert np.all(sp[3:8] == 0.0) and math.isnan(sp[8]) and sp[2] > 0.0
    assert S.pexp(1.0)[0] == pytest.approx(math.e, rel=1e-15)


@pytest.mark.parametrize('N, case', [(8, 'plain'), (100, 'plain'), (513, 'failed'), (1024, 'plain'), (3000, 'ties'), (4096, 'failed')])
def test_next_beta_by_bisection(driver, N, case):
    """The ladder's next rung: the same bits from the header's serial tree and NumPy's, ESS(beta) = ess N to the bisection's
    resolution, and beta = 1 when the weights are flat enough."""
    rng = np.random.default_rng(N)
    lnl = -0.5 * rng.chisquare(4, N) * 40.0
    if case == 'failed':
        lnl[rng.random(N) < 0.2] = -np.inf
    if case == 'ties':
        lnl[::3] = lnl[0]
    for beta_prev, ess in ((0.0, 0.5), (0.25, 0.75), (0.5, 0.3)):       # (a fifth of the particles may carry no weight)
        d = lnl - lnl.max()
        beta, e, s1 = S.next_beta(beta_prev, d, np.float64(ess) * N)
        got = _doubles(_ask(driver, f'B {N} {_hx(beta_prev)} {_hx(ess)} {_hexes(lnl)}')[0].split()[1:])
        assert _same_bits(got, [beta, e, s1])
        assert beta_prev < beta < 1.0 and e >= ess * N and e - ess * N < 1e-6 * N
    flat = np.full(N, -3.0) + 1e-3 * rng.random(N)
    assert S.next_beta(0.1, flat - flat.max(), 0.5 * N)[0] == 1.0
    assert _doubles(_ask(driver, f'B {N} {_hx(0.1)} {_hx(0.5)} {_hexes(flat)}')[0].split()[1:])[0] == 1.0
    assert math.isnan(_doubles(_ask(driver, f'B {N} {_hx(0.0)} {_hx(0.5)} {_hexes(np.full(N, -np.inf))}')[0].split()[1:])[0])
    assert math.isnan(S.stage_head(np.zeros((N, 1)), np.full(N, -np.inf), 0.0, 0.5, 0, 1)['beta'])


def test_systematic_resampling_counts():
    """Ancestors are non-decreasing, no particle of weight 0 is one, and particle i is copied floor or ceil of N q_i times."""
    rng = np.random.default_rng(5)
    N = 1500
    w = rng.random(N) ** 4
    w[rng.random(N) < 0.3] = 0.0
    s1 = S.tree_sum(w)
    c = S.cumulative(w, s1)
    assert c[-1] == 1.0 and np.all(np.diff(c) >= -1e-15) and np.allclose(c, np.cumsum(w) / w.sum(), rtol=0, atol=1e-13)
    anc = S.ancestors(c, S.positions(0.37, N))
    assert np.all(np.diff(anc) >= 0) and np.all(w[anc] > 0)
    copies = np.bincount(anc, minlength=N)
    assert np.all(np.abs(copies - N * w / w.sum()) < 1.0 + 1e-9)


def _gauss_loglike(n, sigma=0.15, centre=0.5):
    def loglike(u):
        d = (np.asarray(u) - centre) / sigma
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return -0.5 * acc
    return loglike


def _replay(u, lnl, stage, beta, scale, n_stages, ess, sweeps, seed, stream, loglike):
    """The restatement stage by stage, recording what every step left behind and the answers the likelihood gave."""
    N = u.shape[0]
    u, lnl = u.copy(), lnl.copy()
    out, answers = [], []
    for _ in range(n_stages):
        if beta >= 1.0:
            break
        head = S.stage_head(u, lnl, beta, ess, stage, seed, stream)
        if math.isnan(head['beta']) or not head['beta'] > beta:
            out.append(dict(head=head, beta_prev=beta, sweeps=[]))
            break
        rec = dict(head=head, beta_prev=beta, sweeps=[])
        u, lnl, beta = head['u'].copy(), head['lnl'].copy(), head['beta']
        for s in range(sweeps):
            y, inside, ua = S.propose(u, head['C'], scale, stage, s, seed, stream)
            lnl_new = loglike(np.where(inside[:, None], y, u))
            answers.append(lnl_new)
            acc = S.accept(inside, lnl_new > -np.inf, beta, lnl_new, lnl, ua)
            u[acc] = y[acc]
            lnl[acc] = lnl_new[acc]
            scale = S.adapt(scale, int(acc.sum()), N)
            rec['sweeps'].append(dict(y=y, inside=inside, ua=ua, accepted=int(acc.sum()), scale=scale, u=u.copy(), lnl=lnl.copy()))
        out.append(rec)
        stage += 1
    return out, answers, u, lnl, stage, beta, scale


@pytest.mark.parametrize('n, N, case', [(1, 8, 'plain'), (2, 48, 'ties'), (6, 200, 'plain'), (32, 80, 'plain'), (2, 40, 'flat axis'),
                                        (6, 1100, 'failed'), (6, 48, 'flat axis')])
def test_header_equals_the_restatement_bitwise(driver, n, N, case):
    """Whole runs of up to three stages: weights, cumulative sums, ancestors (with ties and with particles of lnL = -inf), mean,
    covariance, factor (with the fallback of a pivot that is not positive: one coordinate the same for every particle), and after
    every sweep the proposals, the deciding uniforms, the accepted count, the scale, every particle and its lnL: the header
    compiled by g++ and the NumPy restatement agree in every bit; ``python_stages`` is that same run."""
    seed, stream, sweeps, ess = 11 + n, 3, 3, 0.5
    u0 = S.draw_start(N, n, seed, stream)
    if case == 'flat axis':
        u0[:, n - 1] = 0.25
    inner = _gauss_loglike(n, sigma=0.2 if n > 6 else 0.08)

    def loglike(u):
        out = inner(u)
        if case == 'failed':
            out = np.where(np.asarray(u)[:, 0] < 0.3, -np.inf, out)
        return out

    lnl0 = loglike(u0)
    if case == 'ties':
        order = np.argsort(lnl0)
        lnl0[order[-2]] = lnl0[order[-1]]
        lnl0[order[5]] = lnl0[order[9]]
        lnl0[order[0]] = -np.inf
    stage0, beta0, scale0 = 4, 0.0, S.start_scale(n)
    steps, answers, u1, lnl1, stage1, beta1, scale1 = _replay(u0, lnl0, stage0, beta0, scale0, 3, ess, sweeps, seed, stream, loglike)
    assert 2 <= len(steps) <= 3 and all(len(r['sweeps']) == sweeps for r in steps)   # (what is in effect one dimension ends early)
    assert len(steps) == 3 or n * (case == 'plain') == 1 or case == 'flat axis'
    text = (f'R {n} {N} {sweeps} 3 {stage0} {_hx(beta0)} {_hx(scale0)} {_hx(ess)} {seed:x} {stream:x} {_hexes(u0)} {_hexes(lnl0)} '
            + ' '.join(_hexes(a) for a in answers))
    lines = iter(_ask(driver, text))

    def take(tag):
        parts = next(lines).split()
        assert parts[0] == tag, (parts[0], tag)
        return parts[1:]

    for rec in steps:
        head = rec['head']
        assert _same_bits(_doubles(take('H')), [rec['beta_prev'], head['beta'], head['ess'], head['s1']])
        assert _same_bits(_doubles(take('W')), head['w'])
        assert _same_bits(_doubles(take('C')), head['c'])
        assert [int(t) for t in take('A')] == head['anc'].tolist()
        assert _same_bits(_doubles(take('M')), head['mean'])
        assert _same_bits(_doubles(take('V')), head['cov'])
        f = take('F')
        assert int(f[0]) == int(head['cholesky']) == (0 if case == 'flat axis' else 1)
        assert _same_bits(_doubles(f[1:]), head['C'])
        for sw in rec['sweeps']:
            yl = take('Y')
            assert [int(t) for t in yl[:N]] == sw['inside'].astype(int).tolist()
            assert _same_bits(_doubles(yl[N:2 * N]), sw['ua']) and _same_bits(_doubles(yl[2 * N:]), sw['y'])
            xl = take('X')
            assert int(xl[0]) == sw['accepted']
            assert _same_bits(_doubles(xl[1:2]), [sw['scale']])
            assert _same_bits(_doubles(xl[2:2 + N * n]), sw['u']) and _same_bits(_doubles(xl[2 + N * n:]), sw['lnl'])
    assert next(lines, None) is None
    if case == 'failed':
        assert np.all(steps[0]['head']['w'][np.isneginf(lnl0)] == 0.0) and np.all(np.isfinite(steps[0]['head']['lnl']))
    u, lnl = u0.copy(), lnl0.copy()
    rec, stage, beta, scale, st = S.python_stages(u, lnl, stage0, beta0, scale0, 3, ess, sweeps, seed, stream, loglike)
    assert _same_bits(u, u1) and _same_bits(lnl, lnl1) and (stage, beta, scale) == (stage1, beta1, scale1)
    assert [r['accepted'] for r in rec] == [sum(s['accepted'] for s in r['sweeps']) for r in steps]
    assert all(np.array_equal(a['anc'], b['head']['anc']) for a, b in zip(rec, steps))
    assert st['rows'] == len(steps) * sweeps * N and st['stages'] == len(steps)


# ------------------------------------------------------------------ evidence on analytic likelihoods
def _correlated_gaussian(n, sigma=0.03, rho=0.5):
    """A normalised Gaussian at the centre of the unit cube: log Z = 0 (its mass outside the cube is below 1e-50)."""
    cov = sigma**2 * ((1 - rho) * np.eye(n) + rho * np.ones((n, n)))
    icov = np.linalg.inv(cov)
    log_det = np.linalg.slogdet(2 * np.pi * cov)[1]

    def loglike(u):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ij,jk,ik->i', d, icov, d) - 0.5 * log_det
    return loglike


@pytest.mark.parametrize('n, N, seed', [(2, 512, 3), (4, 1024, 5), (6, 1024, 7)])
def test_gaussian_evidence_and_moments(n, N, seed):
    """Correlated Gaussians (rho = 0.5, sigma = 0.03), default 4 n sweeps, truth log Z = 0: |log Z| <= 5 err with err the
    delta-method figure of :func:`vega_amd.smc.evidence`; every coordinate's mean within 5 sigma / sqrt(N) and every marginal sd
    within 5 sigma / sqrt(2 N) of sigma, the bounds independent particles would give.

    Seeds 0 .. 31 of this restatement, per case n = 2 / 4 / 6: stages 5 / 7 / 9, likelihood evaluations 21.0k / 115.7k /
    222.2k, worst |log Z| / err 2.65 / 2.97 / 2.75, seed-to-seed sd of log Z over the mean err (0.089 / 0.081 / 0.092) 1.03 / 1.21 /
    1.15, worst coordinate mean 2.02 / 3.02 / 3.64 sigma / sqrt(N), worst marginal sd 2.32 / 2.27 / 2.81 sigma / sqrt(2 N)."""
    sigma = 0.03
    run = S.SMCRun(_correlated_gaussian(n), n, particles=N, seed=seed).run()
    assert run.finished and run.sweeps == 4 * n and run.stages['beta'][-1] == 1.0
    log_z, err = run.log_evidence()
    pts, lnl, w = run.samples()
    mean_pull = (pts.mean(axis=0) - 0.5) / (sigma / math.sqrt(N))
    sd_pull = (pts.std(axis=0, ddof=1) - sigma) / (sigma / math.sqrt(2 * N))
    print(f'n = {n}: log Z {log_z:+.4f} +- {err:.4f} (pull {log_z / err:+.2f}), {run.stage} stages, {run.stats["rows"]} evaluations, '
          f'mean pulls {np.round(mean_pull, 2)}, sd pulls {np.round(sd_pull, 2)}, acceptance {np.round(run.stages["acceptance"], 2)}')
    assert abs(log_z) <= 5 * err
    assert np.all(np.abs(mean_pull) <= 5) and np.all(np.abs(sd_pull) <= 5)
    assert np.all(w == 1.0 / N) and pts.shape == (N, n) and np.all(np.diff(run.stages['beta']) > 0)
    assert np.all(run.stages['ess'] >= 0.5 * N)


def _two_modes(n=4, sigma=0.02):
    def loglike(u):
        u = np.asarray(u)
        a = -0.5 * np.sum(((u - 0.3) / sigma)**2, axis=1)
        b = -0.5 * np.sum(((u - 0.7) / sigma)**2, axis=1)
        return np.logaddexp(a, b) - math.log(2.0) - 0.5 * n * math.log(2 * math.pi * sigma * sigma)
    return loglike


def test_two_separated_modes_keep_their_masses():
    """Two Gaussians of sigma = 0.02 at 0.3 1 and 0.7 1 in n = 4, N = 1024, the normalised mixture (log Z = 0): |log Z| <= 5 err,
    and |log(P_A / P_B)| <= 8 err.  After the first stages no move crosses between the modes, so each mode's mass is a local
    evidence carried by about N / 2 particles with error sqrt(2) err, independently; their log ratio has error 2 err, and the
    margin is 4 of those.  Seeds 0 .. 15 of this restatement: worst |log Z| / err 2.09, sd of log Z 1.08 err,
    err 0.083, masses of the lower mode 0.41 - 0.58, worst |log ratio| 0.37 = 4.4 err."""
    run = S.SMCRun(_two_modes(), 4, particles=1024, seed=2).run()
    log_z, err = run.log_evidence()
    pts = run.samples()[0]
    in_a = pts.sum(axis=1) < 2.0
    p_a = in_a.mean()
    print(f'two modes: log Z {log_z:+.4f} +- {err:.4f}, mass of the lower mode {p_a:.3f}, {run.stage} stages')
    assert run.finished and abs(log_z) <= 5 * err
    assert 0.0 < p_a < 1.0 and abs(math.log(p_a / (1.0 - p_a))) <= 8 * err
    for sel, centre in ((in_a, 0.3), (~in_a, 0.7)):
        assert np.all(np.abs(pts[sel].mean(axis=0) - centre) < 5 * 0.02 / math.sqrt(sel.sum()))


# ------------------------------------------------------------------ cuts, chunks, failed models
def test_the_run_does_not_depend_on_the_cut_or_the_chunks():
    loglike = _correlated_gaussian(3, sigma=0.05)
    kw = dict(particles=256, sweeps=5, seed=4, stream=1)
    one = S.SMCRun(loglike, 3, **kw).run()
    cut = S.SMCRun(loglike, 3, **kw)
    while not cut.finished:
        cut.run(stages=1)

    def chunked(u):
        return np.concatenate([loglike(u[k:k + 37]) for k in range(0, len(u), 37)])

    small = S.SMCRun(chunked, 3, **kw).run()
    assert one.finished and one.stats['calls'] == 1 and cut.stats['calls'] == one.stage > 2
    for other in (cut, small):
        assert _same_bits(one.u, other.u) and _same_bits(one.lnl, other.lnl)
        assert one.log_evidence() == other.log_evidence() and one.stage == other.stage and one.scale == other.scale
        assert all(np.array_equal(a['anc'], b['anc']) and _same_bits(a['lnl'], b['lnl']) for a, b in zip(one.record, other.record))
        assert one.stats['rows'] == other.stats['rows'] and one.stats['accepted'] == other.stats['accepted']
    before = one.stats['rows']
    assert one.run().stats['rows'] == before and one.run(stages=3).stage == cut.stage         # (nothing is left to do)
    capped = S.SMCRun(loglike, 3, max_stages=2, **kw).run()
    assert capped.stage == 2 and not capped.finished and capped.run().stage == 2
    assert all(np.array_equal(a['anc'], b['anc']) for a, b in zip(capped.record, one.record))


def test_a_likelihood_that_fails_on_part_of_the_cube():
    """The model fails for u_0 < 0.4 (lnL = -inf there): those particles get weight 0 at the first stage, no move enters the
    region, and the evidence is that of the Gaussian (whose mass there is negligible)."""
    inner = _correlated_gaussian(2, sigma=0.03)
    inner_shift = lambda u: inner(np.asarray(u) - np.array([0.1, 0.0]))     # noqa: E731  (centre (0.6, 0.5))

    def loglike(u):
        return np.where(np.asarray(u)[:, 0] < 0.4, -np.inf, inner_shift(u))

    run = S.SMCRun(loglike, 2, particles=512, seed=6).run()
    log_z, err = run.log_evidence()
    assert run.finished and np.all(run.samples()[0][:, 0] >= 0.4) and np.all(np.isfinite(run.lnl))
    assert np.isneginf(run.record[0]['lnl']).sum() > 150 and run.stats['rejected_failed_model'] >= 0
    assert abs(log_z) <= 5 * err, (log_z, err)
    # a wall 1.7 sigma from the centre: moves run into it (45 % of the start particles carry weight, hence ess = 0.3)
    wall = S.SMCRun(lambda u: np.where(np.asarray(u)[:, 0] < 0.55, -np.inf, inner_shift(u)), 2, particles=512, ess=0.3, seed=6).run()
    assert wall.finished and wall.stats['rejected_failed_model'] > 0 and np.all(wall.samples()[0][:, 0] >= 0.55)


def test_all_particles_failing_is_an_error():
    with pytest.raises(ValueError, match='finite log-likelihood'):
        S.SMCRun(lambda u: np.full(len(u), -np.inf), 2, particles=64).run()
    with pytest.raises(ValueError, match='NaN'):
        S.SMCRun(lambda u: np.full(len(u), np.nan), 2, particles=64).run()
    few = S.SMCRun(lambda u: np.where(np.asarray(u)[:, 0] < 0.9, -np.inf, 0.0), 2, particles=64, ess=0.5)
    with pytest.raises(ValueError, match='cannot advance'):       # (about 6 of 64 particles carry weight: ESS < ess N at any beta)
        few.run()


def test_arguments_are_checked():
    ll = _gauss_loglike(2)
    for kw in (dict(particles=7), dict(particles=4097), dict(ess=0.0), dict(ess=1.0), dict(sweeps=0), dict(max_stages=0)):
        with pytest.raises(ValueError):
            S.SMCRun(ll, 2, **kw)
    with pytest.raises(ValueError):
        S.SMCRun(ll, 33, particles=256)
    with pytest.raises(ValueError):
        S.SMCRun(ll, 6, particles=13)
    assert S.SMCRun(ll, 6, particles=14).sweeps == 24 and S.SMCRun(ll, 2, particles=8).scale == 2.38 * math.sqrt(1.5)
    with pytest.raises(ValueError, match='nothing has run'):
        S.SMCRun(ll, 2).log_evidence()


# ------------------------------------------------------------------ config
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = SMC\n'


def test_smc_sampler_settings(tmp_path):
    s = E.sampler_settings(_config(HEAD + f"""[SMC]
path = {tmp_path}
name = run_a
particles = 300
ess = 0.7
sweeps = 9
seed = 5
driver = python
max_stages = 40
"""), SAMPLE)
    assert s == dict(sampler='SMC', path=tmp_path, name='run_a', particles=300, ess=0.7, sweeps=9, seed=5, driver='python',
                     max_stages=40)
    d = E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\n'), SAMPLE)
    assert d == dict(sampler='SMC', path=tmp_path, name='smc', particles=1024, ess=0.5, sweeps=None, seed=0, driver='device',
                     max_stages=None)
    # a [PocoMC] section beside it is not read
    assert E.sampler_settings(_config(HEAD + f'[SMC]\npath = {tmp_path}\n[PocoMC]\nprecondition = True\nn_total = 4096\n'), SAMPLE) == d
    for other in ('Ensemble', 'Nested'):
        cfg = _config(f'[control]\nrun_sampler = True\nsampler = {other}\n[{other}]\npath = {tmp_path}\n')
        assert E.sampler_settings(cfg, SAMPLE)['sampler'] == other


@pytest.mark.parametrize('text, sample, error, match', [
    ('[control]\nsampler = SMC\n[SMC]\npath = {p}\n', SAMPLE, ValueError, 'run_sampler = True'),
    (HEAD, SAMPLE, RuntimeError, 'no sampler config'),
    (HEAD + '[SMC]\nname = a\n', SAMPLE, ValueError, 'path'),
    (HEAD + '[SMC]\npath = {p}/missing\n', SAMPLE, AssertionError, 'existing'),
    (HEAD + '[SMC]\npath = {p}\nparticles = 7\n', SAMPLE, ValueError, 'particles'),
    (HEAD + '[SMC]\npath = {p}\nparticles = 5000\n', SAMPLE, ValueError, 'particles'),
    (HEAD + '[SMC]\npath = {p}\ness = 0\n', SAMPLE, ValueError, 'ess'),
    (HEAD + '[SMC]\npath = {p}\ness = 1.0\n', SAMPLE, ValueError, 'ess'),
    (HEAD + '[SMC]\npath = {p}\nsweeps = 0\n', SAMPLE, ValueError, 'sweeps'),
    (HEAD + '[SMC]\npath = {p}\ndriver = cpu\n', SAMPLE, ValueError, 'driver'),
    (HEAD + '[SMC]\npath = {p}\nmax_stages = 0\n', SAMPLE, ValueError, 'max_stages'),
    (HEAD + '[SMC]\npath = {p}\n', {'limits': {'ap': (None, 1.2)}}, ValueError, 'well defined prior limits'),
    ('[control]\nrun_sampler = True\nsampler = PocoMC\n[PocoMC]\npath = {p}\n', SAMPLE, NotImplementedError, 'not available'),
    ('[control]\nrun_sampler = True\nsampler = Polychord\n[Polychord]\npath = {p}\n', SAMPLE, NotImplementedError, 'not available'),
    ('[control]\nrun_sampler = True\nsampler = Smc\n[SMC]\npath = {p}\n', SAMPLE, ValueError, 'not recognized'),
])
def test_smc_sampler_settings_refusals(tmp_path, text, sample, error, match):
    with pytest.raises(error, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), sample)


# ------------------------------------------------------------------ writers
def test_writer_round_trip(tmp_path):
    run = S.SMCRun(_correlated_gaussian(3, sigma=0.05), 3, particles=128, sweeps=4, seed=1).run()
    names = ['a', 'b', 'c']
    txt, pn, stats = S.write_run(run, tmp_path, 'run', names)
    table = np.loadtxt(txt)
    pts, lnl, w = run.samples()
    assert table.shape == (128, 5) and np.all(table[:, 0] == 1.0)
    assert np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    assert pn.read_text().splitlines() == [f'{nm} {nm}' for nm in names]
    back = S.read_stats(stats)
    assert (back['log(Z)'], back['log(Z) error']) == run.log_evidence()
    assert back['stages'] == run.stage and back['sweeps'] == 4 and back['seed'] == 1 and back['particles'] == 128
    assert back['ess'] == 0.5 and back['likelihood evaluations'] == run.stats['rows'] == 128 * (1 + 4 * run.stage)
    assert back['beta'] == run.stages['beta'].tolist() and back['beta'][-1] == 1.0


def test_smc_structs_match_the_library():
    """The SMC structs' layouts (vmx_struct_size indices 14 - 16) agree with the ctypes binding."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    for which, st in zip((14, 15, 16), (engine.SmcSpec, engine.SmcOptions, engine.SmcStats)):
        assert lib.vmx_struct_size(which) == C.sizeof(st), st.__name__
    assert 'vmx_smc_run' in engine.EXPORTED_SYMBOLS
    assert engine.VMX_NS_MAXN == S.MAXN and engine.VMX_SMC_MAX_PARTICLES == S.MAX_PARTICLES
    import vega_amd
    assert vega_amd.SMCSampler is S.SMCSampler and vega_amd.SMCRun is S.SMCRun
