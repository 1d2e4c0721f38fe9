"""The nested sampler without a GPU: the header the device kernels are built from (vega_amd/csrc/vmx_nested.h), compiled with g++
under AddressSanitizer / UBSan into tests/helpers/nested_driver.cpp, against the NumPy restatement of vega_amd/nested.py bit for
bit; the restatement's evidence on analytic likelihoods (correlated Gaussians, two separated modes, classic K = 1); independence
of how a run is cut; failed models; the ``[Nested]`` config checks; the writers; the structs."""
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
from vega_amd import nested as N


# ------------------------------------------------------------------ header <-> NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('nested') / 'nested_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'nested_driver.cpp')]
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
    return np.array([struct.unpack('<d', struct.pack('<Q', int(t, 16)))[0] for t in tokens])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_thread_and_live_blocks_use_the_documented_counters():
    """Thread k at iteration t, draw index j: counter (k, t, j, 1); live point i, block j: (i, 0, j, 2) - against NumPy's Philox
    (which increments before it encrypts)."""
    b = N.thread_blocks(np.arange(5), 17, np.array([0, 1, 2, 3, 40]), seed=9, stream=2)
    for k, j in zip(range(5), (0, 1, 2, 3, 40)):
        c = k | (17 << 64) | (j << 128) | (1 << 192)
        assert np.array_equal(b[k], np.random.Philox(key=[9, 2], counter=c - 1).random_raw(4))
    u = N.draw_live(7, 6, seed=3, stream=1)
    for i in range(7):
        words = np.concatenate([np.random.Philox(key=[3, 1], counter=(i | (j << 128) | (2 << 192)) - 1).random_raw(4)
                                for j in range(2)])
        assert np.array_equal(u[i], E.u01(words[:6]))
    assert np.all(u >= 0) and np.all(u < 1)


def _gauss_loglike(n, sigma=0.15, centre=0.5):
    def loglike(u):
        d = (np.asarray(u) - centre) / sigma
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return -0.5 * acc
    return loglike


def _replay(n, nlive, K, num_repeats, it, seed, stream, live_u, live_lnl, loglike):
    """One iteration of the restatement, recording what every call of advance left behind: (head, per thread the answers it was
    given, per thread the snapshots)."""
    head = N.iteration_head(live_u, live_lnl, K, it, seed, stream)
    T = N.Threads(live_u[head['start']], live_lnl[head['start']], head['C'], head['lstar'], it, num_repeats, seed, stream)
    answers = [[] for _ in range(K)]
    shots = [[] for _ in range(K)]

    def snap(ks, asks):
        for k in ks:
            shots[k].append((int(asks[k]), int(T.state[k]), int(T.repeat[k]), int(T.n_out[k]), int(T.n_shrink[k]),
                             int(T.inside[k]), int(T.draw[k]),
                             np.concatenate([[T.L[k], T.R[k], T.t[k], T.lnl[k]], T.x[k], T.y[k], T.d[k]])))

    asks = T.advance(np.full(K, -np.inf))
    snap(range(K), asks)
    while asks.any():
        ks, rows, _ = T.requests(asks)
        answer = np.full(K, -np.inf)
        answer[ks] = loglike(rows)
        for k in ks:
            answers[k].append(answer[k])
        asks = T.advance(answer)
        snap(ks, asks)
    return head, T, answers, shots


@pytest.mark.parametrize('n, nlive, K, case', [(1, 24, 8, 'plain'), (2, 48, 16, 'ties'), (6, 64, 24, 'plain'), (32, 80, 16, 'plain'),
                                               (2, 40, 8, 'flat axis'), (6, 48, 12, 'flat axis')])
def test_header_equals_the_restatement_bitwise(driver, n, nlive, K, case):
    """Live points, kill order (with ties), covariance, factor (with the fallback of a pivot that is not positive: one coordinate
    the same for every live point), starts, and every call of advance of every thread through a whole iteration: the header
    compiled by g++ and the NumPy restatement agree in every bit."""
    seed, stream, it, num_repeats = 11 + n, 3, 5, 3
    live_u = N.draw_live(nlive, n, seed, stream)
    got = _ask(driver, f'D {nlive} {n} {seed:x} {stream:x}')
    assert _same_bits(_doubles(got[0].split()[1:]), live_u)
    if case == 'flat axis':
        live_u[:, n - 1] = 0.25
    loglike = _gauss_loglike(n)
    live_lnl = loglike(live_u)
    order = np.argsort(live_lnl)
    if case == 'ties':
        live_lnl[order[3]] = live_lnl[order[1]]             # two equal among the killed
        live_lnl[order[K]] = live_lnl[order[K - 1]]         # the last killed equals the first survivor
        live_lnl[order[0]] = -np.inf
    head, T, answers, shots = _replay(n, nlive, K, num_repeats, it, seed, stream, live_u, live_lnl, loglike)
    assert head['cholesky'] == (case != 'flat axis')
    text = f'I {n} {nlive} {K} {num_repeats} {it} {seed:x} {stream:x} {_hexes(live_u)} {_hexes(live_lnl)} '
    text += ' '.join(f'{len(a)} {_hexes(a)}' for a in answers)
    lines = _ask(driver, text)
    assert [int(t) for t in lines[0].split()[1:]] == [int(r) for r in head['rank']]
    assert [int(t) for t in lines[1].split()[1:]] == [int(k) for k in head['killed']]
    assert _same_bits(_doubles(lines[2].split()[1:]), head['lstar'])
    assert _same_bits(_doubles(lines[3].split()[1:]), head['mean'])
    assert _same_bits(_doubles(lines[4].split()[1:]), head['cov'])
    assert int(lines[5].split()[1]) == int(head['cholesky'])
    assert _same_bits(_doubles(lines[5].split()[2:]), head['C'])
    assert [int(t) for t in lines[6].split()[1:]] == [int(s) for s in head['start']]
    if case == 'ties':      # equal lnL: the lower live index dies first, also across the boundary between killed and survivors
        assert head['rank'][order[0]] == 0
        for a, b in ((order[1], order[3]), (order[K - 1], order[K])):
            lo_i, hi_i = min(a, b), max(a, b)
            assert live_lnl[a] == live_lnl[b] and head['rank'][hi_i] == head['rank'][lo_i] + 1
        assert min(order[K - 1], order[K]) in head['killed'] and max(order[K - 1], order[K]) in head['surv']
    rows = [ln.split() for ln in lines[7:]]
    assert all(r[0] == 'T' for r in rows)
    per_thread = [[r for r in rows if int(r[1]) == k] for k in range(K)]
    n_calls = 0
    for k in range(K):
        assert len(per_thread[k]) == len(shots[k]) == len(answers[k]) + 1, k
        for r, s in zip(per_thread[k], shots[k]):
            assert [int(t) for t in r[2:9]] == list(s[:7]), (k, r[:9], s[:7])
            assert _same_bits(_doubles(r[9:]), s[7]), (k, r[:9])
            n_calls += 1
        assert shots[k][-1][0] == 0 and shots[k][-1][1] == N.S_DONE and shots[k][-1][2] == num_repeats
    assert n_calls >= K * (1 + 3 * num_repeats)
    # the end points satisfy the constraint they were walked under, inside the cube
    assert np.all(T.lnl[np.isfinite(T.lnl)] >= head['lstar']) and np.all((T.x >= 0) & (T.x <= 1))


def test_map_cube_and_lnl_bitwise(driver):
    rng = np.random.default_rng(5)
    lo, hi, u = rng.normal(size=40), rng.normal(size=40) + 3.0, rng.random(40)
    chi2 = np.concatenate([rng.random(10) * 1e4, [1e99, 1e100, np.nan, np.inf, 0.0]])
    status = [0] * 10 + [0, 0, 0, 0, 1]
    text = ' '.join(f'U {_hx(a)} {_hx(b)} {_hx(c)}' for a, b, c in zip(lo, hi, u))
    text += ' ' + ' '.join(f'X {s} {_hx(c)} {_hx(-1234.5678)}' for s, c in zip(status, chi2))
    got = _ask(driver, text)
    assert _same_bits(_doubles([g.split()[1] for g in got[:40]]), N.map_cube(lo, hi, u))
    want = N.lnl_of(np.array(status), chi2, -1234.5678)
    assert _same_bits(_doubles([g.split()[1] for g in got[40:]]), want)
    assert np.all(np.isneginf(want[10:]))


# ------------------------------------------------------------------ evidence on analytic likelihoods
def _correlated_gaussian(n, sigma=0.03):
    a = np.random.RandomState(1).randn(n, n)
    s = a @ a.T
    d = np.sqrt(np.diag(s))
    cov = s / np.outer(d, d) * sigma**2
    prec = np.linalg.inv(cov)

    def loglike(u):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ri,ij,rj->r', d, prec, d)

    return loglike, cov, 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]


GAUSS_CASES = [(2, 256, 64, s) for s in range(5)] + [(4, 512, 128, s) for s in range(5)] + [(6, 1024, 256, s) for s in range(2)]


@pytest.mark.parametrize('n, nlive, K, seed', GAUSS_CASES)
def test_evidence_of_a_correlated_gaussian(n, nlive, K, seed):
    """sigma = 0.03 per axis at the centre of the cube (truncation beyond 16 sigma: below 1e-50), a fixed correlation matrix:
    log Z = 1/2 log|2 pi Sigma|, H = -log Z - n / 2.  Every seed (n = 6 keeps seeds 0 - 1: 3.6 M evaluations a run):
    |log Z - true| <= 4 err, H within 10 %, err within 10 % of sqrt(H_true / nlive), the weighted mean within 5 sigma / sqrt(ESS)."""
    loglike, cov, log_z_true = _correlated_gaussian(n)
    h_true = -log_z_true - n / 2
    run = N.NestedRun(loglike, n, num_live=nlive, num_repeats=5 * n, threads=K, seed=seed).run()
    log_z, err = run.log_evidence()
    info = run.information()
    pts, lnl, w = run.samples()
    ess = 1.0 / np.sum(w**2)
    mean = w @ pts
    pull = (mean - 0.5) / (0.03 / np.sqrt(ess))
    print(f'n {n} seed {seed}: log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}), '
          f'H {info:.3f} (true {h_true:.3f}), ESS {ess:.0f}, mean pulls {np.round(pull, 2)}, iterations {run.iteration}, '
          f'evaluations {run.stats["rows"]}, per slice step {run.stats["rows"] / (run.iteration * K * 5 * n):.2f}')
    assert run.terminated
    assert abs(log_z - log_z_true) <= 4 * err
    assert abs(info - h_true) <= 0.1 * h_true
    assert abs(err - math.sqrt(h_true / nlive)) <= 0.1 * math.sqrt(h_true / nlive)
    assert np.all(np.abs(pull) <= 5), pull
    assert abs(w.sum() - 1) < 1e-12 and lnl.shape == w.shape == (pts.shape[0],)


@pytest.mark.parametrize('seed', range(5))
def test_two_separated_modes_and_the_chain_that_cannot_cross(seed):
    """Equal Gaussians of sigma = 0.02 at 0.3 * 1 and 0.7 * 1 in 4 dimensions: log Z = log 2 + (n / 2) log(2 pi sigma^2) within
    4 err, and the two modes' posterior masses agree within 4 sqrt(2 H / nlive) in the log (each mode's local evidence carries
    the error sqrt(H / nlive), independently).  A stretch-move ensemble started in a ball at mode A never visits mode B in 500
    steps - the reason this sampler exists."""
    n, sigma, nlive, K = 4, 0.02, 512, 128

    def loglike(u):
        u = np.asarray(u)
        a = -0.5 * np.sum((u - 0.3)**2, axis=1) / sigma**2
        b = -0.5 * np.sum((u - 0.7)**2, axis=1) / sigma**2
        return np.logaddexp(a, b)

    log_z_true = math.log(2) + 0.5 * n * math.log(2 * math.pi * sigma**2)
    run = N.NestedRun(loglike, n, num_live=nlive, num_repeats=5 * n, threads=K, seed=seed).run()
    log_z, err = run.log_evidence()
    pts, _, w = run.samples()
    in_a = np.sum((pts - 0.3)**2, axis=1) < np.sum((pts - 0.7)**2, axis=1)
    p_a, p_b = w[in_a].sum(), w[~in_a].sum()
    bound = 4 * math.sqrt(2 * run.information() / nlive)
    print(f'seed {seed}: log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}, pull {(log_z - log_z_true) / err:+.2f}), '
          f'P_A {p_a:.3f}, |log ratio| {abs(math.log(p_a / p_b)):.3f} (bound {bound:.3f})')
    assert abs(log_z - log_z_true) <= 4 * err
    assert p_a > 0 and p_b > 0 and abs(math.log(p_a / p_b)) <= bound
    if seed == 0:
        W = 32
        rng = np.random.default_rng(1)
        x = 0.3 + sigma * rng.standard_normal((W, n))
        lnl = loglike(x)
        chain, _, _ = E.python_steps(x, lnl, np.zeros(W, dtype=np.int64), 0, 500, 1, 2.0, 1, 0, np.zeros(n), np.ones(n), 0.0,
                                     lambda rows, h: (-2.0 * loglike(rows), np.zeros(len(rows), dtype=np.int32)))
        flat = chain.reshape(-1, n)
        assert np.all(np.sum((flat - 0.3)**2, axis=1) < np.sum((flat - 0.7)**2, axis=1))


def test_one_thread_is_classic_nested_sampling():
    loglike, cov, log_z_true = _correlated_gaussian(2)
    run = N.NestedRun(loglike, 2, num_live=64, num_repeats=10, threads=1, seed=0).run()
    _, _, counts = run.dead()
    assert np.all(counts == 64) and counts.size == run.iteration
    log_z, err = run.log_evidence()
    print(f'K = 1: log Z {log_z:.4f} (true {log_z_true:.4f}, err {err:.4f}), iterations {run.iteration}')
    assert abs(log_z - log_z_true) <= 4 * err
    _, lnl, _ = run.dead()
    assert np.all(np.diff(lnl) >= 0)


def test_the_run_does_not_depend_on_the_cut():
    loglike, _, _ = _correlated_gaussian(3)
    one = N.NestedRun(loglike, 3, num_live=96, num_repeats=6, threads=24, seed=4)
    one.run(iterations=21)
    cut = N.NestedRun(loglike, 3, num_live=96, num_repeats=6, threads=24, seed=4)
    for _ in range(3):
        cut.run(iterations=7)
    assert one.iteration == cut.iteration == 21 and cut.stats['calls'] == 3
    for a, b in zip(one.dead(), cut.dead()):
        assert a.shape == b.shape and _same_bits(a, b)
    assert _same_bits(one.live_u, cut.live_u) and _same_bits(one.live_lnl, cut.live_lnl)
    assert one.log_evidence() == cut.log_evidence()
    assert one.stats['rows'] == cut.stats['rows'] and one.stats['rounds'] == cut.stats['rounds']
    # ... and to termination from there
    one.run()
    cut.run()
    assert one.terminated and one.iteration == cut.iteration and one.log_evidence() == cut.log_evidence()


def test_failed_models_die_first_and_weigh_nothing():
    """A likelihood that reports failed models (lnL = -inf) where u_0 < 0.3: once the kills have removed them no live point lies
    there again, and their dead points carry no weight."""
    base, _, _ = _correlated_gaussian(2, sigma=0.05)

    def loglike(u):
        u = np.asarray(u)
        return np.where(u[:, 0] < 0.3, -np.inf, base(u))

    n_failed = int((N.draw_live(128, 2, 3)[:, 0] < 0.3).sum())
    assert n_failed == 40                           # (of the 128 initial points: more than one iteration's 32 deaths)
    run = N.NestedRun(loglike, 2, num_live=128, num_repeats=10, threads=32, seed=3)
    run.run(iterations=1)
    assert np.isneginf(run.dead()[1]).all()
    run.run()
    du, dl, _ = run.dead()
    failed = np.isneginf(dl)
    last = np.flatnonzero(failed).max()
    # (a thread of the first iteration may start from a failed survivor and stay there: L* was -inf)
    assert n_failed <= failed.sum() < 64 and last < 64
    assert np.all(du[failed, 0] < 0.3) and np.all(du[last + 1:, 0] >= 0.3)
    assert np.all(run.live_u[:, 0] >= 0.3) and np.all(np.isfinite(run.live_lnl))
    pts, lnl, w = run.samples()
    assert np.all(w[np.isneginf(lnl)] == 0.0) and np.isfinite(run.log_evidence()[0])
    # half of the prior mass is cut away beyond 4 sigma of the centre: the evidence is that of the whole Gaussian
    log_z, err = run.log_evidence()
    assert abs(log_z - _correlated_gaussian(2, sigma=0.05)[2]) <= 4 * err


def test_constructor_defaults_and_refusals():
    f = _gauss_loglike(3)
    run = N.NestedRun(f, 3)
    assert run.num_live == 75 and run.num_repeats == 15 and run.threads == 1
    assert N.NestedRun(f, 6, num_live=1024).threads == 512 and N.NestedRun(f, 6, num_live=1024, max_batch=256).threads == 256
    assert N.NestedRun(f, 6, num_live=300).threads == 128
    for kw in (dict(num_live=4), dict(num_live=5000), dict(num_live=64, threads=61), dict(threads=0), dict(num_repeats=0),
               dict(precision=0.0), dict(max_iterations=0)):
        with pytest.raises(ValueError):
            N.NestedRun(f, 3, **kw)
    with pytest.raises(ValueError):
        N.NestedRun(f, 33, num_live=1000)


# ------------------------------------------------------------------ config
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Nested\n'


def test_nested_sampler_settings(tmp_path):
    s = E.sampler_settings(_config(HEAD + f"""[Nested]
path = {tmp_path}
name = run_a
num_live = 300
num_repeats = 7
precision = 0.01
seed = 5
threads = 64
driver = python
max_iterations = 40
"""), SAMPLE)
    assert s == dict(sampler='Nested', path=tmp_path, name='run_a', num_live=300, num_repeats=7, precision=0.01, seed=5,
                     threads=64, driver='python', max_iterations=40)
    d = E.sampler_settings(_config(HEAD + f'[Nested]\npath = {tmp_path}\n'), SAMPLE)
    assert d == dict(sampler='Nested', path=tmp_path, name='nested', num_live=50, num_repeats=10, precision=0.001, seed=0,
                     threads=None, driver='device', max_iterations=None)
    assert E.sampler_settings(_config(f'[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {tmp_path}\n'),
                              SAMPLE)['sampler'] == 'Ensemble'


@pytest.mark.parametrize('text, sample, error, match', [
    ('[control]\nsampler = Nested\n[Nested]\npath = {p}\n', SAMPLE, ValueError, 'run_sampler = True'),
    (HEAD, SAMPLE, RuntimeError, 'no sampler config'),
    (HEAD + '[Nested]\nname = a\n', SAMPLE, ValueError, 'path'),
    (HEAD + '[Nested]\npath = {p}/missing\n', SAMPLE, AssertionError, 'existing'),
    (HEAD + '[Nested]\npath = {p}\nnum_live = 3\n', SAMPLE, ValueError, 'num_live'),
    (HEAD + '[Nested]\npath = {p}\nnum_live = 5000\n', SAMPLE, ValueError, 'num_live'),
    (HEAD + '[Nested]\npath = {p}\nnum_live = 64\nthreads = 62\n', SAMPLE, ValueError, 'threads'),
    (HEAD + '[Nested]\npath = {p}\nthreads = 0\n', SAMPLE, ValueError, 'threads'),
    (HEAD + '[Nested]\npath = {p}\nnum_repeats = 0\n', SAMPLE, ValueError, 'num_repeats'),
    (HEAD + '[Nested]\npath = {p}\nprecision = 0\n', SAMPLE, ValueError, 'precision'),
    (HEAD + '[Nested]\npath = {p}\nprecision = -0.1\n', SAMPLE, ValueError, 'precision'),
    (HEAD + '[Nested]\npath = {p}\ndriver = cpu\n', SAMPLE, ValueError, 'driver'),
    (HEAD + '[Nested]\npath = {p}\nmax_iterations = 0\n', SAMPLE, ValueError, 'max_iterations'),
    (HEAD + '[Nested]\npath = {p}\n', {'limits': {'ap': (None, 1.2)}}, ValueError, 'well defined prior limits'),
    ('[control]\nrun_sampler = True\nsampler = Polychord\n[Polychord]\npath = {p}\n', SAMPLE, NotImplementedError, 'Nested'),
])
def test_nested_sampler_settings_refusals(tmp_path, text, sample, error, match):
    with pytest.raises(error, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), sample)


# ------------------------------------------------------------------ writers
def test_writer_round_trip(tmp_path):
    loglike, _, _ = _correlated_gaussian(3)
    run = N.NestedRun(loglike, 3, num_live=64, num_repeats=6, threads=16, seed=1, max_iterations=12).run()
    assert run.terminated and run.iteration == 12
    names = ['a', 'b', 'c']
    txt, pn, stats = N.write_run(run, tmp_path, 'run', names)
    table = np.loadtxt(txt)
    pts, lnl, w = run.samples()
    assert table.shape == (12 * 16 + 64, 5)
    assert np.array_equal(table[:, 0], w / w.max()) and table[:, 0].max() == 1.0
    np.testing.assert_allclose(table[:, 0] / table[:, 0].sum(), w, rtol=1e-14, atol=0)
    assert np.array_equal(table[:, 1], -lnl) and np.array_equal(table[:, 2:], pts)
    assert pn.read_text().splitlines() == [f'{nm} {nm}' for nm in names]
    back = N.read_stats(stats)
    assert (back['log(Z)'], back['log(Z) error']) == run.log_evidence() and back['H'] == run.information()
    assert back['dead points'] == 12 * 16 and back['iterations'] == 12 and back['seed'] == 1 and back['num_live'] == 64
    assert back['num_repeats'] == 6 and back['threads'] == 16 and back['likelihood evaluations'] == run.stats['rows']
    eq, eq_lnl = run.equal_weighted(np.random.default_rng(0))
    assert 0 < eq.shape[0] <= pts.shape[0] and eq.shape[1] == 3 and eq_lnl.shape == (eq.shape[0],)


def test_write_getdist_without_weights_is_unchanged(tmp_path):
    rng = np.random.default_rng(3)
    chain, lnl = rng.normal(size=(5, 4, 2)), rng.normal(size=(5, 4))
    txt, _ = E.write_getdist(tmp_path, 'plain', ['x', 'y'], chain, lnl)
    want = ''.join(' '.join('%.17g' % v for v in [1.0, -l, *row]) + '\n' for row, l in zip(chain.reshape(-1, 2), lnl.reshape(-1)))
    assert txt.read_text() == want
    txt_w, _ = E.write_getdist(tmp_path, 'weighted', ['x', 'y'], chain, lnl, weights=np.full((5, 4), 0.5))
    assert np.all(np.loadtxt(txt_w)[:, 0] == 0.5) and np.array_equal(np.loadtxt(txt_w)[:, 1:], np.loadtxt(txt)[:, 1:])


def test_nested_structs_match_the_library():
    """The nested structs' layouts (vmx_struct_size indices 11 - 13) agree with the ctypes binding."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    for which, st in zip((11, 12, 13), (engine.NestedSpec, engine.NestedOptions, engine.NestedStats)):
        assert lib.vmx_struct_size(which) == C.sizeof(st), st.__name__
    assert 'vmx_nested_run' in engine.EXPORTED_SYMBOLS
    assert engine.VMX_NS_MAXN == N.MAXN and engine.VMX_NS_MAX_LIVE == N.MAX_LIVE
    import vega_amd
    assert vega_amd.NestedSampler is N.NestedSampler
