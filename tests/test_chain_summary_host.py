"""The summary of a recorded chain without a GPU: vega_amd/csrc/vmx_chain.h, compiled with g++ under AddressSanitizer / UBSan
(tests/helpers/chain_driver.cpp), against its NumPy restatement ``chain_summary`` bit for bit; the restatement against the
project's own FFT estimator ``integrated_time`` and ``np.mean`` / ``np.cov``; the refusals of ``chain='device'``, ``run_until``
and the ``[Ensemble] converge`` settings; ``run_until`` on the ``python`` driver over a stand-in likelihood.

Tolerance of the comparison with the FFT estimator and NumPy's moments.  Measured here over the shapes of ``SHAPES`` (first row 0
and odd; the test prints every figure): tau differed from ``integrated_time`` by at most 3.5e-15 relative, the mean from
``np.mean`` by 3.4e-15 relative, the covariance from ``np.cov`` by 1.3e-15 of sqrt(C_ii C_jj) (the independent columns'
covariances are noise around zero: an entry is held to the scale of its two variances).  RTOL is 100 x the worst of these,
3.5e-13 - and so tighter than the 1e-10 it must never exceed."""
import configparser
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vega_amd import ensemble as E

REPO = Path(__file__).resolve().parents[1]

RTOL = 3.5e-13
MARGIN = 0.05
SHAPES = [(2, 2, 1), (64, 4, 1), (65, 6, 3), (130, 2, 2), (257, 6, 3), (600, 8, 3), (300, 8, 64)]
ODD_FIRST = {2: 1, 64: 7, 65: 3, 130: 11, 257: 5, 600: 13, 300: 9}


# ------------------------------------------------------------------ inputs
def _host_windows(x, c=5.0):
    """Per parameter (window, min_M |M - c taus[M]| for M <= window) of the host FFT estimator alone."""
    out = []
    for d in range(x.shape[2]):
        f = np.mean([E.autocorr_func_1d(x[:, k, d]) for k in range(x.shape[1])], axis=0)
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(len(taus)) < c * taus
        window = int(np.argmin(m)) if np.any(m) else len(taus) - 1
        out.append((window, float(np.min(np.abs(np.arange(window + 1) - c * taus[:window + 1])))))
    return out


def _ar1(T, W, phi, rng):
    z = np.empty((T, W))
    e = rng.standard_normal((T, W))
    z[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        z[t] = phi * z[t - 1] + e[t]
    return 1.0 + 0.05 * z


_CACHE = {}


def _chain(T, W, n):
    """AR(1) series 1 + 0.05 z, phi spread over 0.3 .. 0.9 across the parameters (the offset makes the mean subtraction matter).
    A parameter's series is redrawn - judged by the host FFT estimator alone - until no lag up to its window comes within MARGIN
    of the window's bound, for first row 0 and the odd one: a rounding difference then cannot move a window.

    This is a selection of inputs by the guarded quantity, and not the fixed seeds 1 - 5 the issue quotes a smallest margin of
    0.077 for: that figure is not reproduced here.  With plain seeds this generator's smallest margin over the listed shapes
    was 0.0012, and with 64 independent parameters (the (300, 8, 64) shape) no seed of the first 60 cleared 0.05 for all of them
    at once - some lag of some parameter nearly always lands within 0.05 of its bound.  So each parameter's series is drawn
    until it clears the bound; the code under test takes no part in the choice, and the test below still asserts the margin
    from the host estimator before it compares a window."""
    if (T, W, n) not in _CACHE:
        x = np.empty((T, W, n))
        for d, phi in enumerate(np.linspace(0.3, 0.9, n) if n > 1 else [0.6]):
            for attempt in range(400):
                x[:, :, d] = _ar1(T, W, phi, np.random.default_rng([T, W, n, d, attempt]))
                if all(_host_windows(x[first:, :, d:d + 1])[0][1] > MARGIN for first in (0, ODD_FIRST[T])):
                    break
            else:
                raise AssertionError('no series with a clear window')
        x.setflags(write=False)
        _CACHE[(T, W, n)] = x
    return _CACHE[(T, W, n)]


# ------------------------------------------------------------------ the header
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('chain') / 'chain_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'chain_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _header_summary(exe, x, first, c=5.0, lag_block=32):
    rows, W, n = x.shape
    words = ' '.join(f'{v:016x}' for v in np.ascontiguousarray(x).reshape(-1).view(np.uint64).tolist())
    text = f'Y {rows} {W} {n} {first} {int(np.float64(c).view(np.uint64)):016x} {lag_block} {words}\n'
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()

    def doubles(line):
        return np.array([int(v, 16) for v in line.split()], dtype=np.uint64).view(np.float64)
    return dict(count=int(lines[0]), mean=doubles(lines[1]), covariance=doubles(lines[2]).reshape(n, n), tau=doubles(lines[3]),
                window=np.array(lines[4].split(), dtype=np.int64))


def _same_bits(a, b):
    assert a['count'] == b['count']
    for key in ('mean', 'covariance', 'tau'):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    assert np.array_equal(a['window'], b['window'])


@pytest.mark.parametrize('T, W, n', SHAPES)
def test_the_header_equals_the_restatement(driver, T, W, n):
    """Bit for bit, first row 0 and an odd one; neither side's lag block (32 and 5 in the header, 32 and 7 in NumPy) changes a bit."""
    x = _chain(T, W, n)
    for first in (0, ODD_FIRST[T]):
        ours = E.chain_summary(x, first)
        _same_bits(_header_summary(driver, x, first), ours)
        _same_bits(_header_summary(driver, x, first, lag_block=5), E.chain_summary(x, first, lag_block=7))
        assert ours['count'] == (T - first) * W and ours['sd'].tobytes() == np.sqrt(np.diagonal(ours['covariance'])).tobytes()
        with np.errstate(divide='ignore'):
            assert ours['n_eff'] == ours['count'] / ours['tau'].max()


def _special(kind):
    T, W = 97, 4
    x = _chain(257, 6, 3)[:T, :W, :2].copy()
    if kind == 'constant':              # acov[0] = 0 for every walker of column 0 (0.5 T is exact: the series' mean is 0.5)
        x[:, :, 0] = 0.5
    elif kind == 'one walker constant':
        x[:, 2, 0] = 0.25
    else:                               # a ramp, read with c = 2000: so correlated that the window never closes - the T - 1 branch
        x[:, :, 0] = np.arange(T)[:, None] * 0.01 + np.arange(W)[None, :]     # (the sum of all lags of a centred series is 0: taus
        # falls back to 0 at the last lag, so with emcee's c = 5 every window closes before it unless T is tiny - (2, 2, 1) above)
    return x


@pytest.mark.parametrize('kind', ['constant', 'one walker constant', 'window never closes'])
def test_special_series(driver, kind):
    x = _special(kind)
    c = 2000.0 if kind == 'window never closes' else 5.0
    for first in (0, 5):
        ours = E.chain_summary(x, first, c=c)
        _same_bits(_header_summary(driver, x, first, c=c), ours)
        _same_bits(_header_summary(driver, x, first, c=c, lag_block=3), ours)
        T = x.shape[0] - first
        if kind == 'constant':          # rho = acov = 0 at every lag: taus = -1, and the window closes at once
            assert ours['tau'][0] == -1.0 and ours['window'][0] == 0 and ours['covariance'][0, 0] == 0.0 and ours['mean'][0] == 0.5
        elif kind == 'window never closes':
            assert ours['window'][0] == T - 1 and abs(ours['tau'][0]) < 1e-9           # (all lags of a centred series sum to 0)
        else:
            assert np.isfinite(ours['tau'][0]) and 0 < ours['window'][0] < T - 1
        assert ours['window'][1] == E.chain_summary(_chain(257, 6, 3)[:97, :4, :2], first, c=c)['window'][1]     # (column 1 is untouched)


def test_a_single_row(driver):
    """first = rows - 1, T = 1: every centred series is 0, so tau = -1 and the window 0 as ``integrated_time`` gives them; the
    moments are those of the W points of the row (count - 1 = W - 1 >= 1), and nothing warns."""
    import warnings
    x = _chain(65, 6, 3)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ours = E.chain_summary(x, 64)
    _same_bits(_header_summary(driver, x, 64), ours)
    assert ours['count'] == 6 and np.all(ours['tau'] == -1.0) and np.all(ours['window'] == 0) and ours['n_eff'] == -6.0
    assert np.array_equal(ours['tau'], E.integrated_time(x[64:]))
    np.testing.assert_allclose(ours['mean'], x[64].mean(axis=0), rtol=RTOL)
    np.testing.assert_allclose(ours['covariance'], np.cov(x[64].T), rtol=1e-12, atol=0.0)
    only = E.chain_summary(x, 3, moments=False)
    assert set(only) == {'count', 'tau', 'window', 'n_eff'} and only['tau'].tobytes() == E.chain_summary(x, 3)['tau'].tobytes()


def test_a_stack_of_ensembles_is_its_members():
    x = np.stack([_chain(65, 6, 3), _chain(65, 6, 3)[::-1], _chain(257, 6, 3)[100:165]])
    both = E.chain_summary(x, first=3)
    assert both['mean'].shape == (3, 3) and both['covariance'].shape == (3, 3, 3) and both['window'].shape == (3, 3)
    assert both['count'].shape == (3,) and both['n_eff'].shape == (3,)
    for e in range(3):
        one = E.chain_summary(x[e], first=3)
        for key in E.SUMMARY_KEYS:
            assert np.asarray(both[key][e]).tobytes() == np.asarray(one[key]).tobytes(), key


# ------------------------------------------------------------------ the restatement against the estimators of ever
def _rel(ours, ref, scale):
    """The largest |ours - ref| / scale; an entry whose scale is 0 (T = 2: tau is exactly 0) is held to equality."""
    diff = np.abs(np.asarray(ours) - ref)
    return float(np.max(np.where(scale > 0.0, diff / np.where(scale > 0.0, scale, 1.0), np.where(diff == 0.0, 0.0, np.inf))))


@pytest.mark.parametrize('T, W, n', SHAPES)
def test_the_restatement_against_fft_and_numpy(T, W, n):
    x = _chain(T, W, n)
    for first in (0, ODD_FIRST[T]):
        rows = x[first:]
        host = _host_windows(rows)
        # from the host estimator alone: no lag up to the window is within MARGIN of its bound, so no rounding moves a window
        assert min(m for _, m in host) > MARGIN
        ours = E.chain_summary(x, first)
        assert list(ours['window']) == [w for w, _ in host]
        tau = E.integrated_time(rows)
        flat = rows.reshape(-1, n)
        mean, cov = flat.mean(axis=0), np.atleast_2d(np.cov(flat.T))
        scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
        err = dict(tau=_rel(ours['tau'], tau, np.abs(tau)), mean=_rel(ours['mean'], mean, np.abs(mean)), cov=_rel(ours['covariance'], cov, scale))
        print(f'T {T} W {W} n {n} first {first}: tau {err["tau"]:.2e} mean {err["mean"]:.2e} covariance {err["cov"]:.2e}')
        assert err['tau'] <= RTOL and err['mean'] <= RTOL and err['cov'] <= RTOL
        assert np.allclose(ours['sd'], flat.std(axis=0, ddof=1), rtol=RTOL, atol=0.0)


def test_arguments_of_the_restatement():
    x = _chain(64, 4, 1)
    for bad in (dict(first=64), dict(first=-1), dict(c=0.0), dict(c=np.inf), dict(lag_block=0)):
        with pytest.raises(ValueError):
            E.chain_summary(x, **bad)
    with pytest.raises(ValueError):
        E.chain_summary(x[:, :, 0])
    with pytest.raises(ValueError):
        E.chain_summary(x[:, :1])


# ------------------------------------------------------------------ the samplers over a stand-in likelihood
class _StandInEngine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 16
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1

    def set_mock_index(self, index=None):
        pass


class _StandInVega:
    """The surface of VegaInterface the samplers use, over an n = 2 Gaussian in (a, b)."""
    param_names = ['a', 'fixed', 'b']
    mc_config = None

    def __init__(self, config=None):
        self.main_config = configparser.ConfigParser()
        self.main_config.optionxform = str
        if config is not None:
            self.main_config.read(config)
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _StandInEngine()
        self._icov = np.linalg.inv(0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]]))

    def compute_model(self, run_init=False):
        return None

    def freeze_metals(self, row):
        pass

    def _sync_monte_carlo(self):
        pass

    def _theta(self, _):
        return np.array([0.5, 2.0, 0.5])

    def _log_norm(self):
        return 1.25

    def chi2_batch(self, theta):
        d = np.asarray(theta, dtype=np.float64)[:, [0, 2]] - 0.5
        return np.einsum('ij,jk,ik->i', d, self._icov, d)

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        return torch.from_numpy(self.chi2_batch(t.numpy()))


def test_chain_device_on_the_python_driver_keeps_the_rows_on_the_host():
    """``chain='device'`` with the ``python`` driver: the chain of ``chain='host'`` bit for bit, and ``summary`` is the restatement."""
    vega = _StandInVega()
    host = E.EnsembleSet(vega, 2, 8, seed=3, driver='python', segment=7).run(40)
    dev = E.EnsembleSet(vega, 2, 8, seed=3, driver='python', segment=7, chain='device').run(40)
    assert dev._store is None and np.array_equal(dev.get_chain(), host.get_chain()) and np.array_equal(dev.get_log_lik(), host.get_log_lik())
    summ, ref = dev.summary(discard=5), E.chain_summary(host.get_chain(), 5)
    assert set(summ) == set(E.SUMMARY_KEYS)
    for key in E.SUMMARY_KEYS:
        assert np.asarray(summ[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
    one = E.EnsembleSampler(vega, 8, seed=3, driver='python', chain='device').run(40)
    assert np.array_equal(one.get_chain(), host.get_chain()[0])
    s1 = one.summary(discard=5)
    assert s1['mean'].shape == (2,) and s1['count'] == 35 * 8 and s1['tau'].tobytes() == ref['tau'][0].tobytes()
    assert isinstance(s1['n_eff'], float) and s1['n_eff'] == ref['n_eff'][0]


def test_run_until_converges_with_loose_settings():
    vega = _StandInVega()
    run = E.EnsembleSet(vega, 2, 8, seed=1, driver='python', chain='device')
    run.run_until(600, tau_factor=4, tau_rtol=0.5, check_every=50)
    conv = run.convergence
    assert np.all(conv['converged']) and run.step < 600 and run.step == conv['steps'][-1] and run.step % 50 == 0
    assert conv['tau'].shape == (len(conv['steps']), 2, 2) and conv['converged_at'].shape == (2,)
    assert np.all(conv['converged_at'] > 0) and np.all(conv['converged_at'] <= run.step) and conv['converged_at'].max() == run.step
    # the last check restated: rows behind the burn-in against tau_factor tau, tau against the check before
    rows = run.get_chain().shape[1]
    discard = int(np.floor(rows / 3.0))
    tau = E.chain_summary(run.get_chain(), discard)['tau']
    assert tau.tobytes() == conv['tau'][-1].tobytes() and conv['rows_used'][-1] == rows - discard
    assert np.all(rows - discard >= 4 * tau.max(axis=1))
    assert np.all(np.max(np.abs(tau - conv['tau'][-2]) / tau, axis=1) <= 0.5)
    # the single sampler is the set of one
    one = E.EnsembleSampler(vega, 8, seed=1, driver='python').run_until(600, tau_factor=4, tau_rtol=0.5, check_every=50)
    assert one.convergence['converged'] is True and one.convergence['converged_at'] == one.step and one.convergence['tau'].shape[1:] == (2,)


def test_run_until_says_when_the_steps_ran_out():
    vega = _StandInVega()
    run = E.EnsembleSet(vega, 2, 8, seed=1, driver='python').run_until(60, tau_factor=50, tau_rtol=0.01, check_every=25)
    conv = run.convergence
    assert run.step == 60 and list(conv['steps']) == [25, 50, 60] and not np.any(conv['converged'])
    assert list(conv['converged_at']) == [-1, -1]


@pytest.mark.parametrize('kw', [dict(max_steps=0), dict(check_every=0), dict(tau_factor=0), dict(tau_factor=np.inf), dict(tau_rtol=-0.1),
                                dict(burn=1.0), dict(burn=-0.1)])
def test_run_until_refusals(kw):
    run = E.EnsembleSampler(_StandInVega(), 8, driver='python')
    with pytest.raises(ValueError, match='run_until'):
        run.run_until(**dict(dict(max_steps=10), **kw))
    assert run.step == 0


def test_chain_argument_refusals():
    vega = _StandInVega()
    with pytest.raises(ValueError, match="chain: 'host' or 'device'"):
        E.EnsembleSampler(vega, 8, chain='gpu')
    with pytest.raises(ValueError, match="chain: 'host' or 'device'"):
        E.EnsembleSet(vega, 2, 8, chain='both')
    with pytest.raises(ValueError, match='at most 1024 walkers'):
        E.EnsembleSampler(vega, 1026, chain='device')
    with pytest.raises(ValueError, match='temperature ladder'):
        E.TemperedEnsemble(vega, 8, ntemps=3, chain='device')
    ladder = E.TemperedEnsemble(vega, 8, ntemps=3)
    with pytest.raises(ValueError, match='run_until'):
        ladder.run_until(10)
    with pytest.raises(ValueError, match='no recorded rows'):
        E.EnsembleSampler(vega, 8, driver='python').summary()


# ------------------------------------------------------------------ the settings
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'


def test_converge_parses(tmp_path):
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nconverge = True\n'), SAMPLE)
    assert s['converge'] == {}
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nconverge = True\ntau_factor = 20\ntau_rtol = 0.05\ncheck_every = 40\n'), SAMPLE)
    assert s['converge'] == dict(tau_factor=20.0, tau_rtol=0.05, check_every=40) and E.chain_arguments(s) == dict(chain='device')
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nconverge = False\n'), SAMPLE)
    assert 'converge' not in s and E.chain_arguments(s) == {}
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nreplicas = 2\ntogether = True\nconverge = True\n'), SAMPLE)
    assert s['converge'] == {} and s['together'] is True


@pytest.mark.parametrize('body, match', [
    ('tau_factor = 20\n', 'tau_factor: settings of the convergence stop, but no converge'),
    ('tau_rtol = 0.1\ncheck_every = 5\n', 'tau_rtol, check_every: settings of the convergence stop, but no converge'),
    ('converge = False\ncheck_every = 5\n', 'but converge is not True'),
    ('converge = perhaps\n', 'converge: True or False'),
    ('converge = True\nntemps = 3\n', 'converge and ntemps do not combine'),
    ('converge = True\ntau_factor = 0\n', 'tau_factor must be positive'),
    ('converge = True\ntau_rtol = -0.5\n', 'tau_rtol must be positive'),
    ('converge = True\ntau_rtol = 0\n', 'tau_rtol must be positive'),
    ('converge = True\ncheck_every = 0\n', 'check_every must be positive'),
    ('converge = True\ncheck_every = soon\n', 'check_every: a whole number'),
    ('converge = True\ntau_factor = many\n', 'tau_factor, tau_rtol: numbers'),
    ('converge = True\nreplicas = 2\n', 'needs together = True'),
])
def test_converge_refusals(tmp_path, body, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\n{body}'), SAMPLE)


def test_the_launcher_writes_the_convergence_file(tmp_path):
    """``[Ensemble] converge = True`` through ``run_vega_sampler`` over the stand-in: the run stops early, and ``run.convergence``
    holds a line per check and the verdict; a set (``together``) writes its worst member's tau."""
    (tmp_path / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {tmp_path}\nname = run\ndriver = python\nwalkers = 8\nsteps = 600\nseed = 1\n'
                                       'converge = True\ntau_factor = 4\ntau_rtol = 0.5\ncheck_every = 50\n')
    run = E.run_vega_sampler(str(tmp_path / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                             make_vega=lambda config, device: _StandInVega(config))
    assert run.step < 600 and run.convergence['converged'] is True
    lines = (tmp_path / 'run.convergence').read_text().splitlines()
    assert lines[0] == '# step a b' and lines[-1] == 'converged = True' and len(lines) == 2 + len(run.convergence['steps'])
    last = lines[-2].split()
    assert int(last[0]) == run.step and [float(v) for v in last[1:]] == list(run.convergence['tau'][-1])
    assert (tmp_path / 'run.txt').exists()
    out = tmp_path / 'set'
    out.mkdir()
    (out / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {out}\nname = run\ndriver = python\nwalkers = 8\nsteps = 40\nseed = 1\n'
                                  'replicas = 2\ntogether = True\nconverge = True\ncheck_every = 20\n')
    both = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                              make_vega=lambda config, device: _StandInVega(config))
    lines = (out / 'run.convergence').read_text().splitlines()
    assert lines[-1] == 'converged = False' and [int(l.split()[0]) for l in lines[1:-1]] == [20, 40]
    assert all(s.step == 40 for s in both.samplers)
