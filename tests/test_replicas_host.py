"""Replicas of the samplers and their merges (vega_amd/replicas.py) without a GPU: the nested merge on two runs small enough to
write out by hand and against the single-run evidence, merged evidences of nested and SMC replicas on a Gaussian of known
evidence, R-hat against an independent restatement, the ``replicas`` setting, and the body of the launcher over a stand-in
interface - in one process and in two (gloo) - whose final files must not depend on the number of ranks."""
import configparser
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import REPO

from vega_amd import ensemble as E
from vega_amd import nested as N
from vega_amd import smc as S


def _replicas():
    from vega_amd import replicas
    return replicas


# ------------------------------------------------------------------ the nested merge by hand
def _hand_record(dead_lnl, dead_nlive, live_lnl, stream):
    dead_lnl, live_lnl = np.array(dead_lnl, dtype=float), np.array(live_lnl, dtype=float)
    lnl = np.concatenate([dead_lnl, live_lnl])
    return dict(kind='nested', seed=0, stream=stream, dead_lnl=dead_lnl, dead_nlive=np.array(dead_nlive), live_lnl=live_lnl,
                dead_u=np.zeros((dead_lnl.size, 1)), live_u=np.zeros((live_lnl.size, 1)),
                points=(100.0 * stream + np.arange(lnl.size, dtype=float))[:, None], names=np.array(['x']))


def test_nested_merge_of_two_runs_written_out_by_hand():
    """Run A (nlive 2): deaths at lnL -5, -3, live -1, -2.  Run B (nlive 3): deaths at -4, -3, live -0.5, -2.5, -1.5.

    =====  =======  =====  ==========================  ===
    lnL    of       own n  other run's first >= lnL    n
    =====  =======  =====  ==========================  ===
    -5     A dead   2      B -4 (3)                    5
    -4     B dead   3      A -3 (2)                    5
    -3     A dead   2      B -3 (3)                    5    (the tie: A before B)
    -3     B dead   3      A -3 (2)                    5
    -2.5   B live   3      A -2 (2)                    5
    -2     A live   2      B -1.5 (2)                  4
    -1.5   B live   2      A -1 (1)                    3
    -1     A live   1      B -0.5 (1)                  2
    -0.5   B live   1      A exhausted (0)             1
    =====  =======  =====  ==========================  ===
    """
    rep = _replicas()
    a = _hand_record([-5.0, -3.0], [2, 2], [-1.0, -2.0], 0)
    b = _hand_record([-4.0, -3.0], [3, 3], [-0.5, -2.5, -1.5], 1)
    m = rep.merge_nested([a, b])
    want_n = np.array([5, 5, 5, 5, 5, 4, 3, 2, 1])
    want_lnl = np.array([-5.0, -4.0, -3.0, -3.0, -2.5, -2.0, -1.5, -1.0, -0.5])
    assert np.array_equal(m['nlive'], want_n) and np.array_equal(m['lnl'], want_lnl)
    assert np.array_equal(m['replica'], [0, 1, 0, 1, 1, 0, 1, 0, 1])
    # rows of each record's points: dead in order, then live as stored (A: -1, -2; B: -0.5, -2.5, -1.5)
    assert np.array_equal(m['points'][:, 0], [0.0, 100.0, 1.0, 101.0, 103.0, 3.0, 104.0, 2.0, 102.0])
    want_log_x = -np.array([1 / 5, 2 / 5, 3 / 5, 4 / 5, 1.0, 1.0 + 1 / 4, 1.0 + 1 / 4 + 1 / 3, 1.0 + 1 / 4 + 1 / 3 + 1 / 2,
                            2.0 + 1 / 4 + 1 / 3 + 1 / 2])
    np.testing.assert_allclose(m['log_x'], want_log_x, rtol=1e-15)
    x = np.concatenate([[1.0], np.exp(want_log_x)])
    w = x[:-1] - x[1:]
    z = np.sum(np.exp(want_lnl) * w)
    p = np.exp(want_lnl) * w / z
    assert m['log_z'] == pytest.approx(math.log(z), abs=1e-14)
    np.testing.assert_allclose(m['weights'], p, rtol=1e-13)
    assert abs(m['weights'].sum() - 1.0) < 1e-15
    info = np.sum(p * (want_lnl - math.log(z)))
    assert m['info'] == pytest.approx(info, abs=1e-13) and m['num_live'] == 5
    assert m['err'] == pytest.approx(math.sqrt(info / 5), abs=1e-13)
    # the order of the records decides the tie and nothing else
    m2 = rep.merge_nested([b, a])
    assert np.array_equal(m2['nlive'], want_n) and m2['log_z'] == pytest.approx(m['log_z'], abs=1e-15)
    assert np.array_equal(m2['replica'], [1, 0, 0, 1, 0, 1, 0, 1, 0])


# ------------------------------------------------------------------ evidence on the Gaussian of tests/test_smc_host.py
def _correlated_gaussian(n, sigma=0.03, rho=0.5):
    """A normalised Gaussian at the centre of the unit cube: log Z = 0 (its mass outside the cube is below 1e-50)."""
    cov = sigma**2 * ((1 - rho) * np.eye(n) + rho * np.ones((n, n)))
    icov = np.linalg.inv(cov)
    log_det = np.linalg.slogdet(2 * np.pi * cov)[1]

    def loglike(u):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ij,jk,ik->i', d, icov, d) - 0.5 * log_det
    return loglike


_NESTED = {}


def _nested_run(seed, stream):
    if (seed, stream) not in _NESTED:
        _NESTED[seed, stream] = N.NestedRun(_correlated_gaussian(2), 2, num_live=256, num_repeats=10, threads=64, seed=seed,
                                            stream=stream).run()
    return _NESTED[seed, stream]


def test_one_nested_run_merges_into_its_own_evidence():
    """R = 1: the merge differs from :func:`vega_amd.nested.evidence` only in how the final live points die (one by one instead
    of X_end / nlive each): |delta log Z| <= 1e-5 (2.2e-6 where the rule was settled)."""
    rep = _replicas()
    run = _nested_run(0, 0)
    rec = rep.nested_record(run)
    m = rep.merge_nested([rec])
    log_z, err = run.log_evidence()
    print(f'log Z {log_z!r} merged {m["log_z"]!r} (delta {m["log_z"] - log_z:.2e}), err {err!r} merged {m["err"]!r}')
    assert abs(m['log_z'] - log_z) <= 1e-5
    assert m['num_live'] == 256 and abs(m['err'] - err) <= 1e-4 * err
    du, dl, dn = run.dead()
    assert np.array_equal(m['nlive'][:dl.size], dn) and np.array_equal(m['nlive'][dl.size:], 256 - np.arange(256))
    assert np.array_equal(m['lnl'][:dl.size], dl) and np.array_equal(m['points'][:dl.size], du)
    assert abs(m['weights'].sum() - 1.0) < 1e-12


@pytest.mark.parametrize('seed', [0, 1])
def test_merged_nested_evidence_of_a_gaussian(seed):
    """n = 2, nlive 256, K 64, R = 4 (streams 0 - 3 of one seed), truth log Z = 0: |log Z| <= 5 err, and the merged err within
    10 % of the single runs' mean err / sqrt(R) (the law is exact up to the estimate of H)."""
    rep = _replicas()
    runs = [_nested_run(seed, r) for r in range(4)]
    assert all(run.terminated for run in runs)
    recs = [rep.nested_record(run) for run in runs]
    assert [rec['stream'] for rec in recs] == [0, 1, 2, 3]
    m = rep.merge_nested(recs)
    single = np.array([run.log_evidence() for run in runs])
    print(f'seed {seed}: merged log Z {m["log_z"]:+.4f} +- {m["err"]:.4f} (pull {m["log_z"] / m["err"]:+.2f}), H {m["info"]:.3f}, '
          f'single {np.round(single[:, 0], 4)} +- {np.round(single[:, 1], 4)}, mean err / 2 = {single[:, 1].mean() / 2:.4f}')
    assert len({tuple(run.live_u[0]) for run in runs}) == 4          # (four different runs)
    assert abs(m['log_z']) <= 5 * m['err']
    assert abs(m['err'] - single[:, 1].mean() / 2) <= 0.1 * single[:, 1].mean() / 2
    assert m['num_live'] == 1024 and np.all(np.diff(m['lnl']) >= 0) and abs(m['weights'].sum() - 1.0) < 1e-12
    assert m['nlive'].max() == 1024 and m['nlive'][-1] == 1 and m['points'].shape == (m['lnl'].size, 2)
    ess = 1.0 / np.sum(m['weights']**2)
    pull = (m['weights'] @ m['points'] - 0.5) / (0.03 / np.sqrt(ess))
    assert np.all(np.abs(pull) <= 5), pull


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_merged_smc_evidence_of_a_gaussian(seed):
    """N = 512, R = 4, truth log Z = 0: |log Z| <= 5 err; the weights sum to 1 and a run's total weight is Z_r / sum Z."""
    rep = _replicas()
    runs = [S.SMCRun(_correlated_gaussian(2), 2, particles=512, seed=seed, stream=r).run() for r in range(4)]
    assert all(run.finished for run in runs)
    recs = [rep.smc_record(run) for run in runs]
    m = rep.merge_smc(recs)
    lz = np.array([run.log_evidence()[0] for run in runs])
    er = np.array([run.log_evidence()[1] for run in runs])
    print(f'seed {seed}: merged log Z {m["log_z"]:+.4f} +- {m["err"]:.4f} (pull {m["log_z"] / m["err"]:+.2f}), scatter '
          f'{m["scatter"]:.4f}, single {np.round(lz, 4)} +- {np.round(er, 4)}')
    assert len(set(lz)) == 4
    assert abs(m['log_z']) <= 5 * m['err']
    assert m['log_z'] == pytest.approx(math.log(np.mean(np.exp(lz))), abs=1e-12)
    assert m['err'] == pytest.approx(math.sqrt(np.sum((np.exp(lz) * er)**2)) / np.sum(np.exp(lz)), rel=1e-12)
    assert m['scatter'] == pytest.approx(np.std(lz, ddof=1) / 2, rel=1e-12)
    assert abs(m['weights'].sum() - 1.0) < 1e-12 and m['points'].shape == (4 * 512, 2)
    for r in range(4):
        assert m['weights'][m['replica'] == r].sum() == pytest.approx(np.exp(lz[r]) / np.exp(lz).sum(), rel=1e-12)
        assert np.array_equal(m['points'][m['replica'] == r], runs[r].samples()[0])


# ------------------------------------------------------------------ R-hat
def _rhat_restated(chains):
    """Gelman & Rubin (1992) from the textbook: B = m var(chain means), W = mean of chain variances,
    R-hat^2 = (m - 1) / m + B / (m W)."""
    out = []
    for d in range(chains[0].shape[-1]):
        series = [np.asarray(c)[..., d].ravel() for c in chains]
        m = len(series[0])
        mus = [sum(s) / m for s in series]
        grand = sum(mus) / len(mus)
        B = m * sum((mu - grand)**2 for mu in mus) / (len(mus) - 1)
        W = sum(sum((s - mu)**2) / (m - 1) for s, mu in zip(series, mus)) / len(series)
        out.append(math.sqrt((m - 1) / m + B / (m * W)))
    return np.array(out)


def test_gelman_rubin():
    rep = _replicas()
    rng = np.random.default_rng(8)
    chains = [rng.normal(size=(50, 6, 3)) * [1.0, 2.0, 0.5] + [0.1 * k, 0.0, -0.2 * k] for k in range(3)]
    np.testing.assert_allclose(rep.gelman_rubin(chains), _rhat_restated(chains), rtol=1e-12)
    np.testing.assert_allclose(rep.gelman_rubin(chains, discard=20), _rhat_restated([c[20:] for c in chains]), rtol=1e-12)
    iid = [rng.normal(size=(10000, 2)) for _ in range(4)]
    assert np.all(rep.gelman_rubin(iid) < 1.01)
    shifted = [c.copy() for c in iid]
    shifted[2][:, 0] += 1.0
    rhat = rep.gelman_rubin(shifted)
    assert rhat[0] > 1.1 and rhat[1] < 1.01
    with pytest.raises(ValueError):
        rep.gelman_rubin(iid[:1])
    with pytest.raises(ValueError):
        rep.gelman_rubin([iid[0], iid[1][:50]])


# ------------------------------------------------------------------ settings
SAMPLE = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}


def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


@pytest.mark.parametrize('sampler', ['Ensemble', 'Nested', 'SMC'])
def test_the_replicas_setting(tmp_path, sampler):
    head = f'[control]\nrun_sampler = True\nsampler = {sampler}\n[{sampler}]\npath = {tmp_path}\n'
    plain = E.sampler_settings(_config(head), SAMPLE)
    assert 'replicas' not in plain
    with_r = E.sampler_settings(_config(head + 'replicas = 3\n'), SAMPLE)
    assert with_r == dict(plain, replicas=3)
    assert E.sampler_settings(_config(head + 'replicas = 1\n'), SAMPLE) == dict(plain, replicas=1)
    for bad in ('0', '-2', 'two', '1.5'):
        with pytest.raises(ValueError, match='replicas'):
            E.sampler_settings(_config(head + f'replicas = {bad}\n'), SAMPLE)


# ------------------------------------------------------------------ the launcher body, one rank and two
class _StandInEngine:
    """What the ``python`` drivers ask of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 64
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1


class _StandInVega:
    """The surface of VegaInterface the samplers and ``run_vega_sampler`` use, over the normalised Gaussian above in (a, b); a
    third parameter stays fixed."""
    param_names = ['a', 'fixed', 'b']
    max_batch = 64
    mc_config = None

    def __init__(self, config):
        self.main_config = configparser.ConfigParser()
        self.main_config.optionxform = str
        self.main_config.read(config)
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = SAMPLE
        self.engine = _StandInEngine()
        cov = 0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]])
        self._icov, self._log_det = np.linalg.inv(cov), np.linalg.slogdet(2 * np.pi * cov)[1]

    def compute_model(self, run_init=False):
        return None

    def freeze_metals(self, row):
        pass

    def _theta(self, _):
        return np.array([0.5, 2.0, 0.5])

    def _log_norm(self):
        return -0.5 * self._log_det

    def chi2_batch(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        assert np.all(theta[:, 1] == 2.0)
        d = theta[:, [0, 2]] - 0.5
        return np.einsum('ij,jk,ik->i', d, self._icov, d)

    def chi2_batch_device(self, t):
        import torch
        return torch.from_numpy(self.chi2_batch(t.numpy()))


def _make_vega(config, device):
    return _StandInVega(config)


_SETTINGS = {'Ensemble': 'walkers = 8\nsteps = 30\nseed = 3\n',
             'Nested': 'num_live = 48\nnum_repeats = 4\nthreads = 8\nseed = 3\nmax_iterations = 25\n',
             'SMC': 'particles = 64\nsweeps = 4\nseed = 3\n'}


def _write_config(folder, sampler, replicas=4):
    out = Path(folder) / sampler
    out.mkdir(parents=True)
    text = (f'[control]\nrun_sampler = True\nsampler = {sampler}\n[{sampler}]\npath = {out}\nname = run\ndriver = python\n'
            + _SETTINGS[sampler] + (f'replicas = {replicas}\n' if replicas is not None else ''))
    (out / 'main.ini').write_text(text)
    return out / 'main.ini'


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, folder):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, str(REPO / 'tests'))
    import torch.distributed as dist
    from vega_amd import run_vega_sampler
    for sampler in _SETTINGS:
        out = run_vega_sampler(str(Path(folder) / sampler / 'main.ini'), make_vega=_make_vega, print_func=lambda *_: None)
        assert out.block == ((0, 2) if rank == 0 else (2, 4)) and len(out.records) == 2
        assert [c[0] for c in out.counts] == [2, 2]
        assert (out.merged is not None) == (rank == 0)
    dist.destroy_process_group()


def _final_files(folder):
    return {p.name: p.read_bytes() for p in Path(folder).iterdir() if p.suffix in ('.txt', '.paramnames', '.stats')}


def test_the_final_files_do_not_depend_on_the_world_size(tmp_path):
    """R = 4 replicas of each sampler (``python`` driver over the stand-in): once in this process, once shared by two ranks."""
    import torch.multiprocessing as mp
    from vega_amd import run_vega_sampler
    rep = _replicas()
    for sampler in _SETTINGS:
        _write_config(tmp_path / 'one', sampler)
        _write_config(tmp_path / 'two', sampler)
    lines = []
    for sampler in _SETTINGS:
        out = run_vega_sampler(str(tmp_path / 'one' / sampler / 'main.ini'), make_vega=_make_vega, rank=0, world_size=1,
                               print_func=lines.append)
        assert out.replicas == 4 and out.block == (0, 4) and len(out.records) == 4 and out.merged is not None
        assert [rec['stream'] for rec in out.records] == [0, 1, 2, 3] and all(rec['seed'] == 3 for rec in out.records)
    assert any('4 replicas on 1 rank(s)' in line for line in lines)
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path / 'two')), nprocs=2, join=True)
    want = {'Ensemble': {'run_1.txt', 'run_2.txt', 'run_3.txt', 'run_4.txt', 'run.paramnames', 'run.stats'},
            'Nested': {'run.txt', 'run.paramnames', 'run.stats'}, 'SMC': {'run.txt', 'run.paramnames', 'run.stats'}}
    for sampler in _SETTINGS:
        one, two = _final_files(tmp_path / 'one' / sampler), _final_files(tmp_path / 'two' / sampler)
        assert set(one) == want[sampler] == set(two)
        for name in one:
            assert one[name] == two[name], (sampler, name)
        for r in range(4):
            a = rep.load_record(rep.record_path(tmp_path / 'one' / sampler, 'run', r))
            b = rep.load_record(rep.record_path(tmp_path / 'two' / sampler, 'run', r))
            assert a['stream'] == b['stream'] == r and np.array_equal(a['points'], b['points'])


def test_the_merged_files_hold_what_the_merges_return(tmp_path):
    from vega_amd import run_vega_sampler
    rep = _replicas()
    quiet = dict(make_vega=_make_vega, rank=0, world_size=1, print_func=lambda *_: None)
    # nested
    out = run_vega_sampler(str(_write_config(tmp_path, 'Nested')), **quiet)
    folder = tmp_path / 'Nested'
    m = out.merged
    table = np.loadtxt(folder / 'run.txt')
    assert np.array_equal(table[:, 0], m['weights'] / m['weights'].max()) and np.array_equal(table[:, 1], -m['lnl'])
    assert np.array_equal(table[:, 2:], m['points']) and (folder / 'run.paramnames').read_text() == 'a a\nb b\n'
    st = rep.read_stats(folder / 'run.stats')
    assert (st['log(Z)'], st['log(Z) error'], st['H']) == (m['log_z'], m['err'], m['info'])
    assert st['replicas'] == 4 and st['num_live'] == 4 * 48 and st['iterations'] == 100 and st['dead points'] == 4 * 25 * 8
    assert st['likelihood evaluations'] == sum(s.stats['rows'] for s in out.samplers) and st['seed'] == 3
    assert st['log(Z) replicas'] == [s.log_evidence()[0] for s in out.samplers]
    assert st['log(Z) error replicas'] == [s.log_evidence()[1] for s in out.samplers]
    assert list(st)[:10] == list(N.read_stats(_plain_stats(tmp_path, 'Nested')))
    # SMC
    out = run_vega_sampler(str(_write_config(tmp_path, 'SMC')), **quiet)
    folder = tmp_path / 'SMC'
    m = out.merged
    table = np.loadtxt(folder / 'run.txt')
    assert table.shape == (4 * 64, 4) and np.array_equal(table[:, 0], m['weights'] / m['weights'].max())
    st = rep.read_stats(folder / 'run.stats')
    assert (st['log(Z)'], st['log(Z) error'], st['log(Z) scatter']) == (m['log_z'], m['err'], m['scatter'])
    assert st['replicas'] == 4 and st['particles'] == 4 * 64 and st['ess'] == 0.5 and st['sweeps'] == 4
    assert st['log(Z) replicas'] == [s.log_evidence()[0] for s in out.samplers]
    assert st['beta'] == [[float(r['beta']) for r in s.record] for s in out.samplers]
    # ensemble
    out = run_vega_sampler(str(_write_config(tmp_path, 'Ensemble')), **quiet)
    folder = tmp_path / 'Ensemble'
    for k, s in enumerate(out.samplers):
        table = np.loadtxt(folder / f'run_{k + 1}.txt')
        assert np.array_equal(table[:, 2:], s.get_chain(flat=True)) and np.all(table[:, 0] == 1.0)
    assert not np.array_equal(out.samplers[0].get_chain()[0], out.samplers[1].get_chain()[0])
    st = rep.read_stats(folder / 'run.stats')
    assert st['replicas'] == 4 and st['walkers'] == 8 and st['steps'] == 30 and st['discard'] == 15
    np.testing.assert_array_equal([st['Rhat'][nm] for nm in ('a', 'b')],
                                  rep.gelman_rubin([s.get_chain() for s in out.samplers], discard=15))
    assert st['acceptance fraction'] == [float(s.acceptance_fraction.mean()) for s in out.samplers]
    assert np.array_equal(st['autocorrelation time'], [s.get_autocorr_time() for s in out.samplers])


def _plain_stats(tmp_path, sampler):
    from vega_amd import run_vega_sampler
    cfg = _write_config(tmp_path / 'plain', sampler, replicas=None)
    run_vega_sampler(str(cfg), make_vega=_make_vega, rank=0, world_size=1, print_func=lambda *_: None)
    return tmp_path / 'plain' / sampler / 'run.stats'


@pytest.mark.parametrize('sampler', ['Ensemble', 'Nested', 'SMC'])
def test_one_replica_writes_the_files_of_a_plain_run(tmp_path, sampler):
    from vega_amd import run_vega_sampler
    quiet = dict(make_vega=_make_vega, rank=0, world_size=1, print_func=lambda *_: None)
    a = run_vega_sampler(str(_write_config(tmp_path / 'absent', sampler, replicas=None)), **quiet)
    b = run_vega_sampler(str(_write_config(tmp_path / 'one', sampler, replicas=1)), **quiet)
    assert type(a) is type(b) and a.stream == b.stream == 0 and not hasattr(a, 'merged')
    one, absent = _final_files(tmp_path / 'one' / sampler), _final_files(tmp_path / 'absent' / sampler)
    assert set(one) == set(absent) == {'run.txt', 'run.paramnames'} | ({'run.stats'} if sampler != 'Ensemble' else set())
    assert one == absent
    assert not list((tmp_path / 'one' / sampler).glob('*.npz'))


def test_records_round_trip(tmp_path):
    rep = _replicas()
    run = S.SMCRun(_correlated_gaussian(2), 2, particles=64, sweeps=4, seed=1, stream=2).run()
    rec = rep.smc_record(run)
    back = rep.load_record(rep.save_record(tmp_path / 'r.npz', rec))
    assert back['kind'] == 'smc' and back['seed'] == 1 and back['stream'] == 2 and back['stats']['rows'] == run.stats['rows']
    assert (back['log_z'], back['err']) == run.log_evidence()
    assert np.array_equal(back['u'], run.u) and np.array_equal(back['lnl'], run.lnl) and np.array_equal(back['points'], run.u)
    assert np.array_equal(back['stage_beta'], run.stages['beta']) and back['stage_lnl'].shape == (run.stage, 64)
    with np.load(tmp_path / 'r.npz', allow_pickle=False) as f:          # arrays and scalars only
        assert all(f[k].dtype.kind in 'biufU' for k in f.files)


# ------------------------------------------------------------------ the script starts its own ranks
def _script():
    sys.path.insert(0, str(REPO / 'scripts'))
    import run_vega_sampler
    return run_vega_sampler


def test_the_script_bounds_its_ranks(capsys):
    script = _script()
    for ranks in ('0', '17'):
        with pytest.raises(SystemExit) as exc:
            script.main(['main.ini', '--ranks', ranks])
        assert exc.value.code == 2
    assert '--ranks: 1 .. 16' in capsys.readouterr().err


def test_a_failing_rank_ends_the_run(tmp_path):
    """Two ranks on a config that does not exist: the first failure ends the run with a non-zero status; nothing is retried."""
    script = _script()
    assert script.main([str(tmp_path / 'missing.ini'), '--ranks', '2', '--timeout', '300']) != 0
