"""The ensemble sampler without a GPU: the header the device kernels are built from (vega_amd/csrc/vmx_ensemble.h), compiled with
g++ under AddressSanitizer / UBSan into tests/helpers/ensemble_driver.cpp, against NumPy's Philox and the NumPy restatement of
vega_amd/ensemble.py bit for bit; the restatement's sampling on analytic posteriors; emcee's autocorrelation estimator on AR(1)
series; the ``[Ensemble]`` config checks and the getdist writer."""
import configparser
import ctypes as C
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vega_amd import ensemble as E


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('ensemble') / 'ensemble_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'ensemble_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _ask(exe, lines):
    out = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, out.stderr[-4000:]
    return out.stdout.splitlines()


def _hx(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0].to_bytes(8, 'big').hex()


def _bits(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


M64 = 2**64 - 1
COUNTERS = [0, 1, 2, 5, 2**64 - 1, 2**64, 2**64 + 3, 2**128 - 1, 2**128, 2**192 - 1, 2**192 + 2**64 - 1, 2**256 - 1,
            (3 << 192) | (7 << 128) | (11 << 64) | 13]
KEYS = [(0, 0), (1, 0), (123456789, 0), (2**64 - 1, 2**64 - 1), (42, 7)]


def test_philox_blocks_equal_numpy(driver):
    """Counters with carries across every word, and c = 0 (the Random123 known-answer vector): the header's block, NumPy's
    Philox one step before, and the NumPy restatement are the same four words."""
    lines, want, words = [], [], []
    for c in COUNTERS:
        w = [(c >> (64 * i)) & M64 for i in range(4)]
        for key in KEYS:
            lines.append('P ' + ' '.join(f'{v:x}' for v in w + list(key)))
            want.append(np.random.Philox(key=list(key), counter=(c - 1) % 2**256).random_raw(4))
            words.append((w, key))
    got = _ask(driver, lines)
    for line, ref, (w, key) in zip(got, want, words):
        assert [int(t, 16) for t in line.split()] == [int(v) for v in ref], (w, key)
        assert np.array_equal(E.philox4x64_10(np.array(w, dtype=np.uint64), key), ref), (w, key)
    assert got[0] == '16554d9eca36314c db20fe9d672d0fdc d7e772cee186176b 7e68b68aec7ba23b'


def test_step_blocks_use_the_documented_counter():
    b = E.step_blocks(5, 17, 1, seed=9, stream=2)
    for i in range(5):
        c = i | (17 << 64) | (1 << 128)
        assert np.array_equal(b[i], np.random.Philox(key=[9, 2], counter=c - 1).random_raw(4))


@pytest.mark.parametrize('n', [1, 3, 7])
def test_proposal_and_decision_bitwise(driver, n):
    """Random positions, boxes and blocks: partner, z, proposal, factor, lnL and decision of the header equal the restatement."""
    rng = np.random.default_rng(n)
    cases, lines = [], []
    for k in range(400):
        a = float(rng.choice([2.0, 1.5, 3.7, 1.0 + rng.random()]))
        H = int(rng.integers(1, 5000))
        x = rng.integers(0, 2**64, size=3, dtype=np.uint64)
        c, s = rng.normal(size=n) * 10 ** rng.uniform(-3, 3), rng.normal(size=n) * 10 ** rng.uniform(-3, 3)
        lo, hi = np.minimum(c, s) - rng.random(n), np.maximum(c, s) + rng.random(n)
        if k % 3 == 0:
            hi = hi - rng.random(n) * (hi - lo)      # (boxes that cut some proposals)
        status = int(rng.choice([0, 0, 0, 1]))
        chi2 = float(rng.choice([rng.random() * 1e4, 1e100, rng.random() * 30]))
        log_norm, lnl_old = float(rng.normal() * 100), float(rng.normal() * 100 - 20)
        cases.append((a, H, x, c, s, lo, hi, status, chi2, log_norm, lnl_old))
        lines.append(' '.join(['C', _hx(a), str(n), str(H), *(f'{int(v):x}' for v in x), str(status), _hx(chi2), _hx(log_norm),
                               _hx(lnl_old), *map(_hx, c), *map(_hx, s), *map(_hx, lo), *map(_hx, hi)]))
    got = _ask(driver, lines)
    n_acc = n_in = 0
    for line, (a, H, x, c, s, lo, hi, status, chi2, log_norm, lnl_old) in zip(got, cases):
        tok = line.split()
        j = int(E.partner(np.array([x[0]]), H)[0])
        z = E.stretch_z(a, np.array([x[1]]))
        y = E.propose(c[None, :], s[None, :], z)[0]
        inside = bool(np.all((y >= lo) & (y <= hi)))
        factor = E.log_factor(n, z)[0]
        lnl_new = E.log_lik(log_norm, np.array([chi2]))[0]
        acc = bool(E.accept(np.array([inside]), E.model_ok(np.array([status]), np.array([chi2])), np.array([factor]),
                            np.array([lnl_new]), np.array([lnl_old]), np.array([x[2]]))[0])
        assert int(tok[0]) == j and 0 <= j < H
        assert int(tok[1], 16) == _bits(z[0])
        assert int(tok[2], 16) == _bits(factor)
        assert int(tok[3], 16) == _bits(lnl_new)
        assert (tok[4] == '1') == inside and (tok[5] == '1') == acc
        assert [int(t, 16) for t in tok[6:]] == [_bits(v) for v in y]
        n_acc += acc
        n_in += inside
    assert 0 < n_acc < len(cases) and 0 < n_in < len(cases)      # (both branches of every decision were taken)


def test_stretch_z_lies_in_its_range():
    x = np.random.default_rng(0).integers(0, 2**64, size=100000, dtype=np.uint64)
    for a in (2.0, 1.3, 5.0):
        z = E.stretch_z(a, x)
        assert z.min() >= 1 / a and z.max() <= a
    assert E.partner(np.array([2**64 - 1], dtype=np.uint64), 7)[0] == 6


def _gaussian_problem():
    rng = np.random.default_rng(11)
    n = 5
    A = rng.normal(size=(n, n))
    cov = A @ A.T / n + 0.3 * np.eye(n)
    sd = np.sqrt(np.diag(cov))
    cov = cov / np.outer(sd, sd) * np.outer(np.linspace(0.5, 2.0, n), np.linspace(0.5, 2.0, n))
    mean = np.linspace(-1.0, 1.0, n)
    sd = np.sqrt(np.diag(cov))
    lo, hi = mean - 6 * sd, mean + 6 * sd
    lo[2] = mean[2] - 0.5 * sd[2]            # (the box clips one tail)
    return mean, cov, lo, hi


def _run_python(mean, cov, lo, hi, W, steps, seed=3, thin=1, x0=None, segments=None, fail=None):
    icov = np.linalg.inv(cov)
    n = mean.size
    rng = np.random.default_rng(seed)
    x = x0.copy() if x0 is not None else mean + 0.1 * np.sqrt(np.diag(cov)) * rng.standard_normal((W, n))
    x = np.clip(x, lo, hi)

    def chi2_of(rows):
        d = rows - mean
        return np.einsum('bi,ij,bj->b', d, icov, d)

    def evaluate(rows, h):
        chi2 = chi2_of(rows)
        status = np.zeros(rows.shape[0], dtype=np.int32)
        if fail is not None:
            bad = fail(rows)
            chi2[bad], status[bad] = 1e100, 1
        return chi2, status

    lnl = E.log_lik(-3.0, chi2_of(x))
    acc = np.zeros(W, dtype=np.int64)
    chains, lnls, stats = [], [], []
    step = 0
    for k in (segments or [steps]):
        ch, cl, st = E.python_steps(x, lnl, acc, step, k, thin, 2.0, seed, 0, lo, hi, -3.0, evaluate)
        chains.append(ch), lnls.append(cl), stats.append(st)
        step += k
    return np.concatenate(chains), np.concatenate(lnls), acc, stats


def test_python_driver_samples_a_clipped_gaussian():
    """A correlated 5-D Gaussian in a box that clips one tail: no sample outside the box; mean and covariance of the chain match
    the truncated Gaussian's (rejection sampling of 4e6 draws) within 5 Monte-Carlo standard errors from the measured
    autocorrelation time."""
    mean, cov, lo, hi = _gaussian_problem()
    W, steps, burn = 64, 3000, 500
    chain, lnl, acc, _ = _run_python(mean, cov, lo, hi, W, steps)
    assert np.all(chain >= lo) and np.all(chain <= hi)
    post = chain[burn:]
    tau = E.integrated_time(post)
    assert np.all(tau > 1) and np.all(tau < 200), tau
    rng = np.random.default_rng(5)
    draws = rng.multivariate_normal(mean, cov, size=4_000_000)
    draws = draws[np.all((draws >= lo) & (draws <= hi), axis=1)]
    m_ref, c_ref = draws.mean(axis=0), np.cov(draws.T)
    flat = post.reshape(-1, mean.size)
    n_eff = flat.shape[0] / tau.max()
    sd = np.sqrt(np.diag(c_ref))
    assert np.all(np.abs(flat.mean(axis=0) - m_ref) < 5 * sd / np.sqrt(n_eff)), (flat.mean(axis=0), m_ref, n_eff)
    tol = 5 * np.sqrt(2.0 / n_eff) * np.outer(sd, sd)
    assert np.all(np.abs(np.cov(flat.T) - c_ref) < tol), (np.cov(flat.T) - c_ref, tol)
    assert abs(m_ref[2] - mean[2]) > 0.1 * sd[2]         # (the clipped tail moved the mean: the box matters)
    assert 0.2 < acc.mean() / steps < 0.8


def test_python_driver_is_cut_independent_and_rejects_failures():
    mean, cov, lo, hi = _gaussian_problem()
    one = _run_python(mean, cov, lo, hi, 16, 60, thin=3)
    two = _run_python(mean, cov, lo, hi, 16, 60, thin=3, segments=[31, 29])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert one[0].shape == (20, 16, 5)
    # models that fail above a plane (the walkers start below it) are never accepted, and are counted as such
    plane = mean[0] + 0.5 * np.sqrt(cov[0, 0])
    chain, _, _, stats = _run_python(mean, cov, lo, hi, 16, 200, fail=lambda rows: rows[:, 0] > plane)
    assert np.all(chain[:, :, 0] <= plane)
    assert stats[0]['rejected_failed_model'] > 0
    assert stats[0]['proposals'] == stats[0]['steps'] * 16


@pytest.mark.parametrize('phi', [0.5, 0.8, 0.9])
def test_autocorr_time_on_ar1(phi):
    rng = np.random.default_rng(int(phi * 10))
    steps, walkers = 40000, 16
    e = rng.standard_normal((steps, walkers))
    x = np.empty_like(e)
    x[0] = e[0] / np.sqrt(1 - phi**2)
    for t in range(1, steps):
        x[t] = phi * x[t - 1] + e[t]
    tau = E.integrated_time(x[:, :, None])[0]
    want = (1 + phi) / (1 - phi)
    assert abs(tau - want) < 0.1 * want, (tau, want)


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}, 'values': {}, 'errors': {}}


def test_sampler_settings(tmp_path):
    cfg = _config(f"""[control]
run_sampler = True
sampler = Ensemble
[Ensemble]
path = {tmp_path}
name = chain_a
walkers = 40
steps = 300
seed = 5
a = 2.5
thin = 3
init = prior
init_scale = 0.5
driver = python
""")
    s = E.sampler_settings(cfg, SAMPLE)
    assert s['path'] == tmp_path and s['name'] == 'chain_a' and s['walkers'] == 40 and s['steps'] == 300
    assert s['seed'] == 5 and s['a'] == 2.5 and s['thin'] == 3 and s['init'] == 'prior' and s['init_scale'] == 0.5
    assert s['driver'] == 'python'
    d = E.sampler_settings(_config(f'[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {tmp_path}\n'), SAMPLE)
    assert d['walkers'] % 2 == 0 and d['walkers'] >= 4 and d['a'] == 2.0 and d['thin'] == 1 and d['driver'] == 'device'


@pytest.mark.parametrize('text, sample, error, match', [
    ('[control]\nsampler = Ensemble\n[Ensemble]\npath = {p}\n', SAMPLE, ValueError, 'run_sampler = True'),
    ('[control]\nrun_sampler = False\nsampler = Ensemble\n[Ensemble]\npath = {p}\n', SAMPLE, ValueError, 'run_sampler = True'),
    ('[control]\nrun_sampler = True\nsampler = Polychord\n[Polychord]\npath = {p}\n', SAMPLE, NotImplementedError, 'Ensemble'),
    ('[control]\nrun_sampler = True\nsampler = PocoMC\n[PocoMC]\npath = {p}\n', SAMPLE, NotImplementedError, 'Ensemble'),
    ('[control]\nrun_sampler = True\nsampler = Emcee\n', SAMPLE, ValueError, 'not recognized'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n', SAMPLE, RuntimeError, 'no sampler config'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\n',
     {'limits': {'ap': (None, 1.2)}}, ValueError, 'well defined prior limits'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}/missing\n', SAMPLE, AssertionError, 'existing'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\nwalkers = 3\n', SAMPLE, ValueError, 'walkers'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\nwalkers = 2\n', SAMPLE, ValueError, 'walkers'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\na = 1\n', SAMPLE, ValueError, 'stretch'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\nthin = 0\n', SAMPLE, ValueError, 'thin'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\ninit = uniform\n', SAMPLE, ValueError, 'init'),
    ('[control]\nrun_sampler = True\nsampler = Ensemble\n[Ensemble]\npath = {p}\ndriver = cpu\n', SAMPLE, ValueError, 'driver'),
])
def test_sampler_settings_refusals(tmp_path, text, sample, error, match):
    with pytest.raises(error, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), sample)


def test_writer_round_trip(tmp_path):
    mean, cov, lo, hi = _gaussian_problem()
    W, steps, thin = 16, 30, 3
    chain, lnl, _, _ = _run_python(mean, cov, lo, hi, W, steps, thin=thin)
    names = [f'p{i}' for i in range(mean.size)]
    txt, pn = E.write_getdist(tmp_path, 'run', names, chain, lnl)
    table = np.loadtxt(txt)
    assert table.shape == (steps // thin * W, 2 + mean.size)
    assert np.all(table[:, 0] == 1.0)
    assert np.array_equal(table[:, 1], -lnl.reshape(-1))
    assert np.array_equal(table[:, 2:], chain.reshape(-1, mean.size))
    assert pn.read_text().splitlines() == [f'{nm} {nm}' for nm in names]


def test_ensemble_structs_match_the_library():
    """The ensemble structs' layouts (vmx_struct_size indices 8 - 10) agree with the ctypes binding."""
    import __graft_entry__ as g
    g.build()
    from vega_amd import engine
    lib = engine.load_library()
    for which, st in zip((8, 9, 10), (engine.EnsembleSpec, engine.EnsembleOptions, engine.EnsembleStats)):
        assert lib.vmx_struct_size(which) == C.sizeof(st), st.__name__
    assert 'vmx_ensemble_run' in engine.EXPORTED_SYMBOLS and 'vmx_derived_const_hint' in engine.EXPORTED_SYMBOLS
