"""Many ensembles advanced together (vega_amd/ensemble.py: EnsembleSet, python_steps_many) on the CPU, without an engine: the set's
NumPy restatement makes, for every ensemble, exactly the chain a single-ensemble loop kept here (`_reference_python_steps`) makes on
that ensemble's Philox stream and data - whole or cut into segments -, `python_steps` (the set of one) makes that chain too, every
member starts from the walkers the single sampler draws, the config keys
``[Ensemble] mocks`` / ``together`` parse and refuse as documented, and over a stand-in interface the ``python`` driver gives every
ensemble its mock and ``together = True`` writes the records and merged files of the sequential path."""
import configparser
from types import SimpleNamespace

import numpy as np
import pytest

from vega_amd import ensemble as E

STREAMS = (0, 5, 2)
W, N, STEPS, THIN, SEED, A, LOG_NORM = 8, 4, 25, 2, 9, 2.0, -1.5


def _problem():
    """A correlated Gaussian in 4 dimensions with another mean per "mock"."""
    rng = np.random.default_rng(4)
    B = rng.normal(size=(N, N))
    cov = B @ B.T / N + 0.5 * np.eye(N)
    means = np.array([[0.0, 0.5, -0.5, 1.0], [1.5, -1.0, 0.25, 0.0], [-2.0, 0.75, 1.0, -0.5]])
    sd = np.sqrt(np.diag(cov))
    lo, hi = means.min(axis=0) - 4 * sd, means.max(axis=0) + 4 * sd
    return means, np.linalg.inv(cov), lo, hi, sd


def _chi2(rows, mean, icov):
    d = rows - mean
    return np.einsum('bi,ij,bj->b', d, icov, d)


def _starts(means, sd, lo, hi):
    rng = np.random.default_rng(1)
    return np.clip(means[:, None, :] + 0.3 * sd * rng.standard_normal((len(STREAMS), W, N)), lo, hi)


def _reference_python_steps(x, lnl, accepted, step0, n_steps, thin, a, seed, stream, lo, hi, log_norm, evaluate):
    """The single-ensemble loop as `python_steps` was written before it became the E = 1 case of `python_steps_many`: the
    reference both are held to.  Same arguments, same returned triple."""
    W, n = x.shape
    H = W // 2
    rows = (step0 + n_steps) // thin - step0 // thin
    chain, chain_lnl = np.empty((rows, W, n)), np.empty((rows, W))
    st = dict(steps=n_steps, proposals=n_steps * W, accepted=0, rejected_outside_box=0, rejected_failed_model=0)
    for s in range(step0, step0 + n_steps):
        for h in (0, 1):
            y, inside, factor, b = E.half_step_proposals(x, h, s, a, seed, stream, lo, hi)
            mine = slice(h * H, (h + 1) * H)
            chi2, status = evaluate(np.where(inside[:, None], y, x[mine]), h)
            ok = E.model_ok(status, chi2)
            lnl_new = E.log_lik(log_norm, chi2)
            acc = E.accept(inside, ok, factor, lnl_new, lnl[mine], b[:, 2])
            x[mine][acc] = y[acc]
            lnl[mine][acc] = lnl_new[acc]
            accepted[mine] += acc
            st['accepted'] += int(acc.sum())
            st['rejected_outside_box'] += int((~inside).sum())
            st['rejected_failed_model'] += int((inside & ~ok).sum())
        if (s + 1) % thin == 0:
            r = (s + 1) // thin - step0 // thin - 1
            chain[r], chain_lnl[r] = x, lnl
    return chain, chain_lnl, st


@pytest.fixture(scope='module')
def separate():
    """Three separate `_reference_python_steps` runs: the reference, computed once."""
    means, icov, lo, hi, sd = _problem()
    x0 = _starts(means, sd, lo, hi)
    out = []
    for e, stream in enumerate(STREAMS):
        x = x0[e].copy()
        lnl = E.log_lik(LOG_NORM, _chi2(x, means[e], icov))
        acc = np.zeros(W, dtype=np.int64)
        chain, chain_lnl, st = _reference_python_steps(
            x, lnl, acc, 0, STEPS, THIN, A, SEED, stream, lo, hi, LOG_NORM,
            lambda rows, h, e=e: (_chi2(rows, means[e], icov), np.zeros(len(rows), dtype=np.int32)))
        out.append((chain, chain_lnl, acc, x, lnl, st))
    return out


def _run_set(segments):
    means, icov, lo, hi, sd = _problem()
    H = W // 2
    x = _starts(means, sd, lo, hi)
    lnl = np.stack([E.log_lik(LOG_NORM, _chi2(x[e], means[e], icov)) for e in range(len(STREAMS))])
    acc = np.zeros((len(STREAMS), W), dtype=np.int64)

    def evaluate(rows, h):
        assert rows.shape == (len(STREAMS) * H, N)
        chi2 = np.concatenate([_chi2(rows[e * H:(e + 1) * H], means[e], icov) for e in range(len(STREAMS))])
        return chi2, np.zeros(rows.shape[0], dtype=np.int32)

    chains, lnls, per, step = [], [], np.zeros((len(STREAMS), 3), dtype=np.int64), 0
    for k in segments:
        ch, cl, st, p = E.python_steps_many(x, lnl, acc, step, k, THIN, A, SEED, np.array(STREAMS, dtype=np.uint64), lo, hi, LOG_NORM,
                                            evaluate)
        assert st['proposals'] == k * W * len(STREAMS) and st['accepted'] == p[:, 0].sum()
        chains.append(ch), lnls.append(cl)
        per += p
        step += k
    return np.concatenate(chains, axis=1), np.concatenate(lnls, axis=1), acc, x, lnl, per


@pytest.mark.parametrize('segments', [[STEPS], [7, 7, 7, 4]])
def test_the_set_restates_separate_runs(separate, segments):
    chain, chain_lnl, acc, x, lnl, per = _run_set(segments)
    assert chain.shape == (3, STEPS // THIN, W, N) and chain_lnl.shape == (3, STEPS // THIN, W)
    for e, (ch, cl, a, x_e, lnl_e, st) in enumerate(separate):
        assert np.array_equal(chain[e], ch) and np.array_equal(chain_lnl[e], cl)
        assert np.array_equal(acc[e], a) and np.array_equal(x[e], x_e) and np.array_equal(lnl[e], lnl_e)
        assert tuple(per[e]) == (st['accepted'], st['rejected_outside_box'], st['rejected_failed_model'])
    assert 0 < per[:, 0].sum() < STEPS * W * 3
    # (the ensembles are different chains: another stream, another mean)
    assert not np.array_equal(chain[0], chain[1]) and not np.array_equal(chain[1], chain[2])


def test_python_steps_is_the_set_of_one():
    """`python_steps` against the reference loop from a step0 that is no multiple of thin, on a non-zero stream: chain, lnL, the
    state updated in place, the counters and the statistics, bit for bit; the rows `evaluate` sees are one half's."""
    means, icov, lo, hi, sd = _problem()
    step0, n_steps, thin, stream = 3, STEPS, 2, 5
    start = _starts(means, sd, lo, hi)[1]
    seen = []

    def evaluate(rows, h):
        seen.append((rows.shape, h))
        return _chi2(rows, means[1], icov), np.zeros(len(rows), dtype=np.int32)

    runs = []
    for steps in (_reference_python_steps, E.python_steps):
        x = start.copy()
        lnl = E.log_lik(LOG_NORM, _chi2(x, means[1], icov))
        acc = np.arange(W, dtype=np.int64)
        chain, chain_lnl, st = steps(x, lnl, acc, step0, n_steps, thin, A, SEED, stream, lo, hi, LOG_NORM, evaluate)
        runs.append((chain, chain_lnl, x, lnl, acc, st))
    ref, new = runs
    rows = (step0 + n_steps) // thin - step0 // thin
    assert new[0].shape == (rows, W, N) and new[1].shape == (rows, W)
    for got, want in zip(new[:5], ref[:5]):
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    assert new[5] == ref[5] and list(new[5]) == list(ref[5])
    assert 0 < ref[5]['accepted'] < n_steps * W and not np.array_equal(new[2], start)
    assert seen[:2 * n_steps] == seen[2 * n_steps:] and set(shape for shape, _ in seen) == {(W // 2, N)}


def _stand_in():
    names = ['a', 'b', 'c']
    sp = {'limits': {'a': (-1.0, 1.0), 'b': (0.0, 4.0), 'c': (-3.0, -1.0)}, 'values': {'a': 0.1, 'b': 2.0, 'c': -2.0},
          'errors': {'a': 0.05, 'b': None, 'c': 0.2}}
    return SimpleNamespace(param_names=['z', 'c', 'a', 'b'], params={'a': 0.1, 'b': 2.0, 'c': -2.0, 'z': 1.0}, sample_params=sp), names


@pytest.mark.parametrize('start', ['ball', 'prior'])
def test_members_start_where_the_single_sampler_starts(start):
    vega, names = _stand_in()
    both = E.EnsembleSet(vega, 3, 8, streams=STREAMS, seed=6)
    assert both.names == names and both.streams.tolist() == list(STREAMS)
    x0 = both._start_positions(start, 0.7)
    assert x0.shape == (3, 8, 3)
    for e, stream in enumerate(STREAMS):
        single = E.EnsembleSampler(vega, 8, seed=6, stream=stream)
        assert np.array_equal(x0[e], single._start_positions(start, 0.7))
    assert not np.array_equal(x0[0], x0[1])
    assert E.EnsembleSet(vega, 4, 8).streams.tolist() == [0, 1, 2, 3]       # (the default: range(E))
    given = np.clip(x0 + 0.01, both.lo, both.hi)
    assert np.array_equal(both._start_positions(given, 1.0), given)
    with pytest.raises(ValueError, match='start'):
        both._start_positions(given[:2], 1.0)


def test_set_arguments_are_checked():
    vega, _ = _stand_in()
    for kw, match in ((dict(ensembles=0, walkers=8), 'ensembles'), (dict(ensembles=2, walkers=7), 'walkers'),
                      (dict(ensembles=2, walkers=4), 'walkers'), (dict(ensembles=2, walkers=8, streams=[1]), 'streams'),
                      (dict(ensembles=2, walkers=8, mock_rows=[0, 1, 2]), 'mock_rows'),
                      (dict(ensembles=2, walkers=8, mock_rows=[0, -1]), 'mock_rows'), (dict(ensembles=2, walkers=8, a=1.0), 'stretch'),
                      (dict(ensembles=2, walkers=8, thin=0), 'thin'), (dict(ensembles=2, walkers=8, driver='cpu'), 'driver')):
        with pytest.raises(ValueError, match=match):
            E.EnsembleSet(vega, **kw)
    both = E.EnsembleSet(vega, 2, 8)
    member = both.member(1)
    assert member.stream == 1 and member.get_chain().shape == (0, 8, 3) and member.get_log_lik().shape == (0, 8)
    with pytest.raises(RuntimeError, match='read-only'):
        member.run(3)
    with pytest.raises(IndexError):
        both.member(2)


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'ap': (0.5, 1.5), 'at': (0.5, 1.5)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'
MC = '[monte carlo]\nap = 0.5 1.5 1.05 0.01\nat = 0.5 1.5 0.95 0.01\n'


def test_mocks_and_together_parse(tmp_path):
    s = E.sampler_settings(_config(f'{HEAD}run_montecarlo = True\n{MC}[Ensemble]\npath = {tmp_path}\nmocks = 5\nwalkers = 8\n'), SAMPLE)
    assert s['mocks'] == 5 and 'together' not in s and 'replicas' not in s
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nreplicas = 3\ntogether = True\n'), SAMPLE)
    assert s['together'] is True and s['replicas'] == 3 and 'mocks' not in s
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nreplicas = 3\ntogether = False\n'), SAMPLE)
    assert s['together'] is False
    s = E.sampler_settings(_config(f'{HEAD}[Ensemble]\npath = {tmp_path}\nreplicas = 3\n'), SAMPLE)
    assert 'together' not in s and 'mocks' not in s             # (absent: the sequential path of today)


@pytest.mark.parametrize('text, match', [
    (HEAD + MC + '[Ensemble]\npath = {p}\nmocks = 3\n', 'run_montecarlo'),
    (HEAD + 'run_montecarlo = False\n' + MC + '[Ensemble]\npath = {p}\nmocks = 3\n', 'run_montecarlo'),
    (HEAD + 'run_montecarlo = True\n[Ensemble]\npath = {p}\nmocks = 3\n', r'\[monte carlo\]'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Ensemble]\npath = {p}\nmocks = 0\n', 'mocks'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Ensemble]\npath = {p}\nmocks = many\n', 'mocks'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Ensemble]\npath = {p}\nmocks = 3\nreplicas = 2\n', 'replicas'),
    (HEAD + '[Ensemble]\npath = {p}\ntogether = perhaps\n', 'together'),
])
def test_mocks_and_together_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), SAMPLE)


# ------------------------------------------------------------------ the python driver and the launcher body over a stand-in
class _StandInEngine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 6
    rows_device = 'cpu'
    mock_index = None

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1

    def set_mock_index(self, index=None):
        self.mock_index = None if index is None else np.asarray(index)


class _StandInVega:
    """The surface of VegaInterface the set uses, over a Gaussian in (a, b) whose mean moves with the "mock" row."""
    param_names = ['a', 'fixed', 'b']
    mc_config = None
    SHIFT = np.array([[0.0, 0.0], [0.02, -0.01], [-0.03, 0.02]])

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

    def _chi2(self, theta, rows):
        theta = np.asarray(theta, dtype=np.float64)
        assert np.all(theta[:, 1] == 2.0)
        d = theta[:, [0, 2]] - 0.5 - (0.0 if rows is None else self.SHIFT[np.asarray(rows)])
        return np.einsum('ij,jk,ik->i', d, self._icov, d)

    def chi2_batch(self, theta):
        idx = self.engine.mock_index
        assert idx is None or len(theta) <= len(idx) or len(set(idx.tolist())) == 1
        return self._chi2(theta, None if idx is None else np.resize(idx, len(theta)))

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        assert t.shape[0] <= self.engine.max_batch
        return torch.from_numpy(self._chi2(t.numpy(), None if mock_rows is None else mock_rows.numpy()))


def test_the_python_driver_gives_every_ensemble_its_mock():
    """E = 3 on the mock rows (2, 0, 2) in chunks that cut through ensembles: every member is the single sampler's chain on its
    stream with its mock's likelihood."""
    vega = _StandInVega()
    both = E.EnsembleSet(vega, 3, 8, streams=[4, 1, 2], mock_rows=[2, 0, 2], seed=5, thin=2, driver='python', segment=4).run(10)
    assert both.driver == 'python' and both.get_chain().shape == (3, 5, 8, 2) and both.stats['calls'] == 3
    assert both.stats['engine_calls'] == 10 * 2 * 2 and vega.engine.mock_index is None
    for e, (stream, row) in enumerate(zip([4, 1, 2], [2, 0, 2])):
        single = E.EnsembleSampler(vega, 8, seed=5, stream=stream)
        x = single._start_positions('ball', 1.0)
        lnl = E.log_lik(1.25, vega._chi2(np.insert(x, 1, 2.0, axis=1), np.full(8, row)))
        acc = np.zeros(8, dtype=np.int64)
        chain, chain_lnl, st = E.python_steps(
            x, lnl, acc, 0, 10, 2, 2.0, 5, stream, single.lo, single.hi, 1.25,
            lambda rows, h, row=row: (vega._chi2(np.insert(rows, 1, 2.0, axis=1), np.full(len(rows), row)), np.zeros(len(rows), dtype=np.int32)))
        member = both.member(e)
        assert np.array_equal(member.get_chain(), chain) and np.array_equal(member.get_log_lik(), chain_lnl)
        assert np.array_equal(member.accepted, acc) and member.stats['accepted'] == st['accepted'] and member.step == 10
        assert np.array_equal(both.get_autocorr_time()[e], member.get_autocorr_time())
    assert not np.array_equal(both.get_chain()[0], both.get_chain()[2])


def test_replicas_together_write_the_records_of_the_sequential_path(tmp_path):
    """``together = True`` through ``run_vega_sampler`` over the stand-in (whose chi2 does not depend on the batch): the same records,
    key for key and bit for bit in the chains, and the same merged files as the sequential path."""
    from vega_amd import replicas as rep
    folders = {}
    for tag, extra in (('seq', ''), ('tog', 'together = True\n')):
        out = tmp_path / tag
        out.mkdir()
        (out / 'main.ini').write_text(f'{HEAD}[Ensemble]\npath = {out}\nname = run\ndriver = python\nwalkers = 8\nsteps = 30\nseed = 3\n'
                                      f'thin = 2\nreplicas = 3\n{extra}')
        run = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                                 make_vega=lambda config, device: _StandInVega(config))
        assert run.replicas == 3 and len(run.samplers) == 3 and [s.stream for s in run.samplers] == [0, 1, 2]
        folders[tag] = out
    for r in range(3):
        seq, tog = (rep.load_record(rep.record_path(folders[tag], 'run', r)) for tag in ('seq', 'tog'))
        assert set(seq) == set(tog) and set(seq['stats']) == set(tog['stats'])
        for key in ('chain', 'chain_lnl', 'accepted', 'points', 'names', 'steps', 'thin', 'walkers', 'seed', 'stream', 'kind', 'driver'):
            assert np.array_equal(seq[key], tog[key]), key
        for key in ('steps', 'proposals', 'accepted', 'rejected_outside_box', 'rejected_failed_model'):
            assert seq['stats'][key] == tog['stats'][key], key
    for name in ('run_1.txt', 'run_2.txt', 'run_3.txt', 'run.paramnames', 'run.stats'):
        assert (folders['seq'] / name).read_bytes() == (folders['tog'] / name).read_bytes(), name
