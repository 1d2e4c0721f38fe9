"""A set of SMC runs without a GPU: the NumPy restatement ``python_stages_many`` against ``python_stages`` run by run and bit for
bit over analytic likelihoods (nothing depends on the shape of a batch): runs that end at different stages, a run that fails,
cuts; the decisions the set adds to vega_amd/csrc/vmx_smc.h, compiled with g++ under AddressSanitizer / UBSan
(tests/helpers/smc_set_driver.cpp), against their restatement; ``SMCSet`` over a stand-in interface; the ``[SMC] mocks`` /
``together`` settings; the FITS table of the SMC mock posteriors."""
import configparser
import math
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from vega_amd import ensemble as E
from vega_amd import smc as S

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'tests'))

SEED, ESS, SWEEPS, N = 7, 0.5, 3, 72


def _loglike(n, shift=0.0):
    """A correlated Gaussian well inside the cube, sd 0.05."""
    cov = 0.05**2 * (0.6 * np.eye(n) + 0.4)
    icov = np.linalg.inv(cov)

    def f(rows_u):
        d = np.asarray(rows_u) - 0.5 - shift
        return -0.5 * np.einsum('ij,jk,ik->i', d, icov, d)
    return f


def _start(n, streams, like):
    u = np.stack([S.draw_start(N, n, SEED, int(s)) for s in streams])
    return u, np.stack([like(ue) for ue in u])


def _single(u, lnl, stage, beta, scale, n_stages, stream, like):
    u, lnl = u.copy(), lnl.copy()
    rec, stage, beta, scale, st = S.python_stages(u, lnl, stage, beta, scale, n_stages, ESS, SWEEPS, SEED, stream, like)
    return dict(u=u, lnl=lnl, rec=rec, stage=stage, beta=beta, scale=scale, st=st)


def _many(u, lnl, stage, beta, scale, n_stages, streams, evaluate, draw=False):
    u, lnl = u.copy(), lnl.copy()
    stage, beta, scale = np.array(stage, dtype=np.int64), np.array(beta, dtype=np.float64), np.array(scale, dtype=np.float64)
    rec, status, done, st = S.python_stages_many(u, lnl, stage, beta, scale, n_stages, ESS, SWEEPS, SEED, np.array(streams, dtype=np.uint64),
                                                 evaluate, draw=draw)
    return dict(u=u, lnl=lnl, rec=rec, stage=stage, beta=beta, scale=scale, status=status, done=done, st=st)


def _same_record(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for key in ra:
            assert np.array_equal(ra[key], rb[key]), key


def _same_run(many, e, single):
    assert np.array_equal(many['u'][e], single['u']) and np.array_equal(many['lnl'][e], single['lnl'])
    assert many['stage'][e] == single['stage'] and many['beta'][e] == single['beta'] and many['scale'][e] == single['scale']
    _same_record(many['rec'][e], single['rec'])
    assert many['done'][e] == len(single['rec'])
    st = single['st']
    assert list(many['st']['per_run'][e]) == [st['accepted'], st['rows_own_position'], st['rejected_failed_model'], st['rows']]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('n', [2, 6])
def test_the_set_is_its_single_runs(n):
    """E = 4 runs, N = 72 (no multiple of 64, no power of two): every run of the set is ``python_stages`` on its stream, bit for
    bit in u, lnL, ancestors, beta, scale and the record; runs on equal streams are equal."""
    streams, like = [3, 0, 3, 9], _loglike(n)
    u, lnl = _start(n, streams, like)
    zeros, scale = [0, 0, 0, 0], [S.start_scale(n)] * 4
    many = _many(u, lnl, zeros, [0.0] * 4, scale, 64, streams, lambda rows, runs: like(rows))
    assert list(many['status']) == [S.FINISHED] * 4 and np.all(many['beta'] == 1.0)
    for e, stream in enumerate(streams):
        single = _single(u[e], lnl[e], 0, 0.0, S.start_scale(n), 64, stream, like)
        assert len(single['rec']) >= 3
        _same_run(many, e, single)
    assert np.array_equal(many['u'][0], many['u'][2]) and not np.array_equal(many['u'][0], many['u'][1])
    assert many['st']['rounds'] == max(many['done']) and many['st']['stages'] == int(many['done'].sum())
    # drawn by the set itself: the same runs, with the N start rows counted
    drawn = _many(np.zeros_like(u), np.zeros_like(lnl), zeros, [0.0] * 4, scale, 64, streams, lambda rows, runs: like(rows), draw=True)
    assert np.array_equal(drawn['u'], many['u']) and np.array_equal(drawn['lnl'], many['lnl'])
    assert np.array_equal(drawn['st']['per_run'][:, 3], many['st']['per_run'][:, 3] + N)


def test_runs_end_at_different_stages():
    """Run 0 enters in the state a single run has after 3 stages, run 1 at the start: run 0 leaves early, the rows of the later
    rounds are run 1's alone, and run 1 is what it is without run 0."""
    n, like = 2, _loglike(2)
    u, lnl = _start(n, [5, 6], like)
    early = _single(u[0], lnl[0], 0, 0.0, S.start_scale(n), 3, 5, like)
    assert early['beta'] < 1.0
    rows_seen = []

    def evaluate(rows, runs):
        rows_seen.append((len(rows), list(runs)))
        return like(rows)

    many = _many(np.stack([early['u'], u[1]]), np.stack([early['lnl'], lnl[1]]), [3, 0], [early['beta'], 0.0],
                 [early['scale'], S.start_scale(n)], 64, [5, 6], evaluate)
    assert many['done'][0] < many['done'][1] and list(many['status']) == [S.FINISHED, S.FINISHED]
    _same_run(many, 0, _single(early['u'], early['lnl'], 3, early['beta'], early['scale'], 64, 5, like))
    _same_run(many, 1, _single(u[1], lnl[1], 0, 0.0, S.start_scale(n), 64, 6, like))
    assert many['stage'][0] == 3 + many['done'][0]
    both = many['done'][0] * SWEEPS
    assert all(seen == (2 * N, [0, 1]) for seen in rows_seen[:both]) and all(seen == (N, [1]) for seen in rows_seen[both:])
    assert len(rows_seen) == many['done'][1] * SWEEPS
    alone = _many(u[1:], lnl[1:], [0], [0.0], [S.start_scale(n)], 64, [6], lambda rows, runs: like(rows))
    assert np.array_equal(alone['u'][0], many['u'][1]) and np.array_equal(alone['lnl'][0], many['lnl'][1])


def test_a_failing_run_leaves_the_others_alone():
    """Run 1's likelihood is -inf everywhere: status 2, its state as it was entered, no stage done; runs 0 and 2 are the single
    runs; the call succeeds."""
    n, like = 2, _loglike(2)
    streams = [1, 2, 4]

    def evaluate(rows, runs):
        out = like(rows).reshape(len(runs), N)
        out[np.asarray(runs) == 1] = -np.inf
        return out.reshape(-1)

    u0, lnl0 = np.full((3, N, n), 0.125), np.full((3, N), -3.0)
    many = _many(u0, lnl0, [0, 0, 0], [0.0] * 3, [0.7] * 3, 64, streams, evaluate, draw=True)
    assert list(many['status']) == [S.FINISHED, S.NO_FINITE, S.FINISHED] and list(many['done'] > 0) == [True, False, True]
    assert np.array_equal(many['u'][1], u0[1]) and np.array_equal(many['lnl'][1], lnl0[1])
    assert many['stage'][1] == 0 and many['beta'][1] == 0.0 and many['scale'][1] == 0.7 and many['rec'][1] == []
    assert list(many['st']['per_run'][1]) == [0, 0, 0, N]
    u, lnl = _start(n, streams, like)
    for e in (0, 2):
        single = _single(u[e], lnl[e], 0, 0.0, S.start_scale(n), 64, streams[e], like)
        assert np.array_equal(many['u'][e], single['u']) and np.array_equal(many['lnl'][e], single['lnl'])
        _same_record(many['rec'][e], single['rec'])


def test_a_run_whose_ladder_is_stuck_gets_status_3():
    """One particle alone carries weight and ess N = 36 are asked for: beta cannot advance; the other run goes on."""
    n, like = 2, _loglike(2)
    u, lnl = _start(n, [1, 2], like)
    lnl[0, 1:] = -np.inf
    many = _many(u, lnl, [0, 0], [0.0, 0.0], [0.5, 0.5], 64, [1, 2], lambda rows, runs: like(rows))
    assert list(many['status']) == [S.STUCK, S.FINISHED] and many['done'][0] == 0
    assert np.array_equal(many['u'][0], u[0]) and np.array_equal(many['lnl'][0], lnl[0]) and many['beta'][0] == 0.0
    _same_run(many, 1, _single(u[1], lnl[1], 0, 0.0, 0.5, 64, 2, like))


def test_the_set_cut_into_calls_is_the_same_set():
    n, like = 6, _loglike(6)
    streams = [0, 1, 2]
    u, lnl = _start(n, streams, like)
    whole = _many(u, lnl, [0] * 3, [0.0] * 3, [S.start_scale(n)] * 3, 64, streams, lambda rows, runs: like(rows))
    cut = dict(u=u, lnl=lnl, stage=[0] * 3, beta=[0.0] * 3, scale=[S.start_scale(n)] * 3)
    records, calls = [[] for _ in streams], 0
    while True:
        cut = _many(cut['u'], cut['lnl'], cut['stage'], cut['beta'], cut['scale'], 1, streams, lambda rows, runs: like(rows))
        for e in range(3):
            records[e].extend(cut['rec'][e])
        calls += 1
        if np.all(cut['status'] == S.FINISHED):
            break
        assert calls < 64
    assert calls == max(whole['done']) and calls > 2
    for key in ('u', 'lnl', 'stage', 'beta', 'scale'):
        assert np.array_equal(cut[key], whole[key]), key
    for e in range(3):
        _same_record(records[e], whole['rec'][e])


# ------------------------------------------------------------------ the header's decisions
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('smc_set') / 'smc_set_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'smc_set_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _hex(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0].item().to_bytes(8, 'big').hex()


def _ask(exe, text):
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return [[int(v) for v in line.split()] for line in run.stdout.splitlines()]


def test_header_decisions_equal_the_restatement(driver):
    """run_status, start_status, first_active and compact_active of the header against smc.py, and the host loop over made-up
    words: runs that finish, stall and lose their particles in different rounds; the list stays ascending, the statuses and the
    stages done are those of the restatement's loop."""
    betas = [0.0, 0.25, 1.0, math.nan, math.inf, -0.0, 0.9999999999999999]
    pairs = [(a, b) for a in betas[:3] + betas[6:] for b in betas]
    answers = _ask(driver, ''.join(f'S {_hex(a)} {_hex(b)}\n' for a, b in pairs))
    assert [a[0] for a in answers] == [S.run_status(a, b) for a, b in pairs]
    assert _ask(driver, f'T {_hex(0.0)}\nT {_hex(1.0)}\nT {_hex(72.0)}\n') == [[S.NO_FINITE], [S.RUNNING], [S.RUNNING]]
    rng = np.random.default_rng(3)
    for E_ in (1, 2, 5, 9):
        for draw in (0, 1):
            beta = rng.choice([0.0, 0.3, 1.0], size=E_)
            out = _ask(driver, f'F {E_} {draw} ' + ' '.join(_hex(b) for b in beta) + '\n')[0]
            active, status = S.first_active(beta, bool(draw))
            assert out == [len(active)] + active + list(status)
            stat = rng.integers(0, 4, size=E_)
            keep = _ask(driver, f'C {len(active)} ' + ' '.join(map(str, active)) + f' {E_} ' + ' '.join(map(str, stat)) + '\n')[0]
            mine = S.compact_active(active, stat)
            assert keep == [len(mine)] + mine and mine == sorted(mine)
    # the loop: words per round for the active runs, in the list's order
    E_, rounds = 6, 5
    beta0 = np.array([0.0, 0.5, 1.0, 0.0, 0.2, 0.0])
    script = {0: [0.3, 1.0], 1: [0.75, 0.75], 3: [math.nan], 4: [0.4, 0.6, 0.8, 0.9, 0.95], 5: [0.5, 0.9, 1.0]}
    active, status = S.first_active(beta0, False)
    beta, done, at, words, lists = beta0.copy(), np.zeros(E_, dtype=int), {e: 0 for e in script}, [], []
    for _ in range(rounds):
        if not active:
            break
        lists.append([len(active)] + list(active))
        for e in active:
            after = script[e][at[e]]
            at[e] += 1
            words.append(after)
            status[e] = S.run_status(beta[e], after)
            if status[e] in (S.NO_FINITE, S.STUCK):
                continue
            beta[e], done[e] = after, done[e] + 1
        active = S.compact_active(active, status)
    done[(status == S.NO_FINITE) | (status == S.STUCK)] = 0
    out = _ask(driver, f'L {E_} 0 ' + ' '.join(_hex(b) for b in beta0) + f' {rounds} ' + ' '.join(_hex(w) for w in words) + '\n')
    assert out[:-2] == lists and lists[0] == [5, 0, 1, 3, 4, 5] and lists[-1] == [1, 4]
    assert out[-2] == [E_] + list(status) and list(status) == [1, 3, 1, 2, 0, 1]
    assert out[-1] == [E_] + list(done) and list(done) == [2, 0, 0, 0, 5, 3]


# ------------------------------------------------------------------ SMCSet over a stand-in interface
class _Engine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 50
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1

    def set_mock_pool(self, name, pool):
        pass

    def set_mock_index(self, index=None):
        pass


class _Vega:
    """The surface of VegaInterface the set uses, over a Gaussian in (a, b) whose mean moves with the mock row."""
    param_names = ['a', 'fixed', 'b']
    mc_config = None
    _use_global_cov = False
    SHIFT = np.array([[0.0, 0.0], [0.02, -0.01], [-0.03, 0.02]])

    def __init__(self, config=None):
        self.main_config = configparser.ConfigParser()
        self.main_config.optionxform = str
        if config is not None:
            self.main_config.read(config)
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _Engine()
        self.problem = None
        self._icov = np.linalg.inv(0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]]))

    def compute_model(self, run_init=False):
        return None

    def freeze_metals(self, row=None):
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

    def chi2_batch_device(self, t, mock_rows=None):
        import torch
        assert t.shape[0] <= self.engine.max_batch
        return torch.from_numpy(self._chi2(t.numpy(), None if mock_rows is None else mock_rows.numpy()))


def test_the_python_driver_gives_every_run_its_mock_and_its_evidence():
    """E = 3 on the mock rows (2, 0, 2) in chunks of 50 that cut through runs of 72: every member is the single run on its stream
    with its mock's likelihood, cut or not; log Z is the Gaussian's integral over the unit box."""
    vega = _Vega()
    streams, rows = [4, 1, 4], [2, 0, 2]
    both = S.SMCSet(vega, 3, particles=N, streams=streams, mock_rows=rows, seed=5, driver='python').run()
    cut = S.SMCSet(vega, 3, particles=N, streams=streams, mock_rows=rows, seed=5, driver='python')
    while not np.all(cut.finished):
        cut.run(1)
    assert both.driver == 'python' and np.all(both.finished) and list(both.status) == [1, 1, 1]
    assert np.array_equal(cut.u, both.u) and np.array_equal(cut.stage, both.stage) and cut.stats['calls'] == both.stats['rounds'] > 1
    for e, (stream, row) in enumerate(zip(streams, rows)):
        single = S.SMCRun(lambda u, row=row: 1.25 - 0.5 * vega._chi2(np.insert(u, 1, 2.0, axis=1), np.full(len(u), row)), 2,
                          particles=N, seed=5, stream=stream).run()
        member = both.member(e)
        assert np.array_equal(member.u, single.u) and np.array_equal(member.lnl, single.lnl) and member.stage == single.stage
        _same_record(member.record, single.record)
        assert member.log_evidence() == single.log_evidence() and member.stream == stream
        for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model'):
            assert member.stats[key] == single.stats[key], key
        with pytest.raises(RuntimeError, match='read-only'):
            member.run()
    assert np.array_equal(both.u[0], both.u[2]) and not np.array_equal(both.u[0], both.u[1])
    log_z, err = both.log_evidence()
    exact = 1.25 + math.log(2.0 * math.pi * math.sqrt(np.linalg.det(np.linalg.inv(vega._icov))))
    assert np.all(np.abs(log_z - exact) <= 5.0 * err) and np.all(err > 0.0)
    pts, lnl, w = both.samples()
    assert pts.shape == (3, N, 2) and lnl.shape == (3, N) and np.allclose(w.sum(axis=1), 1.0)
    with pytest.raises(IndexError):
        both.member(3)


def test_set_arguments_are_checked():
    vega = _Vega()
    for kw, match in ((dict(runs=0), 'at least one'), (dict(runs=2, streams=[1]), 'one entry'), (dict(runs=2, mock_rows=[0, -1]), 'negative'),
                      (dict(runs=2, particles=4), 'particles'), (dict(runs=2, ess=1.0), 'ess'), (dict(runs=2, driver='host'), 'driver')):
        with pytest.raises(ValueError, match=match):
            S.SMCSet(vega, **kw)
    with pytest.raises(ValueError, match='nothing has run'):
        S.SMCSet(vega, 2).log_evidence()


# ------------------------------------------------------------------ settings
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'ap': (0.5, 1.5), 'at': (0.5, 1.5)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = SMC\n'
MC = '[monte carlo]\nap = 0.5 1.5 1.05 0.01\nat = 0.5 1.5 0.95 0.01\n'


def test_mocks_and_together_parse(tmp_path):
    s = E.sampler_settings(_config(f'{HEAD}run_montecarlo = True\n{MC}[SMC]\npath = {tmp_path}\nmocks = 5\nparticles = 64\n'), SAMPLE)
    assert s['mocks'] == 5 and s['sampler'] == 'SMC' and s['particles'] == 64 and 'together' not in s and 'replicas' not in s
    s = E.sampler_settings(_config(f'{HEAD}[SMC]\npath = {tmp_path}\nreplicas = 3\ntogether = True\n'), SAMPLE)
    assert s['together'] is True and s['replicas'] == 3 and 'mocks' not in s
    s = E.sampler_settings(_config(f'{HEAD}[SMC]\npath = {tmp_path}\nreplicas = 3\ntogether = False\n'), SAMPLE)
    assert s['together'] is False
    s = E.sampler_settings(_config(f'{HEAD}[SMC]\npath = {tmp_path}\nreplicas = 3\n'), SAMPLE)
    assert 'together' not in s and 'mocks' not in s             # (absent: the sequential path of today)


@pytest.mark.parametrize('text, match', [
    (HEAD + MC + '[SMC]\npath = {p}\nmocks = 3\n', r'\[SMC\] mocks needs "run_montecarlo = True"'),
    (HEAD + 'run_montecarlo = False\n' + MC + '[SMC]\npath = {p}\nmocks = 3\n', 'run_montecarlo'),
    (HEAD + 'run_montecarlo = True\n[SMC]\npath = {p}\nmocks = 3\n', r'\[SMC\] mocks needs a "\[monte carlo\]" section'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[SMC]\npath = {p}\nmocks = 0\n', r'\[SMC\] mocks: a whole number'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[SMC]\npath = {p}\nmocks = many\n', r'\[SMC\] mocks: a whole number'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[SMC]\npath = {p}\nmocks = 3\nreplicas = 2\n', 'every mock has an SMC run of its own'),
    (HEAD + '[SMC]\npath = {p}\ntogether = perhaps\n', r'\[SMC\] together: True or False'),
])
def test_mocks_and_together_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), SAMPLE)


def test_the_ensemble_messages_are_what_they_were(tmp_path):
    head = HEAD.replace('SMC', 'Ensemble')
    with pytest.raises(ValueError) as err:
        E.sampler_settings(_config(f'{head}run_montecarlo = True\n{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\nreplicas = 2\n'), SAMPLE)
    assert str(err.value) == '[Ensemble] mocks and replicas > 1 do not combine: every mock has an ensemble of its own'
    with pytest.raises(ValueError) as err:
        E.sampler_settings(_config(f'{head}{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\n'), SAMPLE)
    assert str(err.value) == '[Ensemble] mocks needs "run_montecarlo = True" in the "[control]" section'


# ------------------------------------------------------------------ the replicas of a rank as one set
def test_replicas_together_write_the_records_of_the_sequential_path(tmp_path):
    """``[SMC] together = True`` through ``run_vega_sampler`` over the stand-in (whose chi2 does not depend on the batch): the same
    records, key for key and bit for bit, and the same merged files as the sequential path."""
    from vega_amd import replicas as rep
    folders = {}
    for tag, extra in (('seq', ''), ('tog', 'together = True\n')):
        out = tmp_path / tag
        out.mkdir()
        (out / 'main.ini').write_text(f'{HEAD}[SMC]\npath = {out}\nname = run\ndriver = python\nparticles = {N}\nseed = 3\nreplicas = 3\n{extra}')
        run = E.run_vega_sampler(str(out / 'main.ini'), print_func=lambda *_: None, rank=0, world_size=1,
                                 make_vega=lambda config, device: _Vega(config))
        assert run.replicas == 3 and [s.stream for s in run.samplers] == [0, 1, 2]
        folders[tag] = out
    for r in range(3):
        seq, tog = (rep.load_record(rep.record_path(folders[tag], 'run', r)) for tag in ('seq', 'tog'))
        assert set(seq) == set(tog) and set(seq['stats']) == set(tog['stats'])
        for key in seq:
            if key != 'stats':
                assert np.array_equal(seq[key], tog[key]), key
        for key in ('stages', 'sweeps', 'rows', 'rows_own_position', 'accepted', 'rejected_failed_model'):
            assert seq['stats'][key] == tog['stats'][key], key
    names = sorted(p.name for p in folders['seq'].iterdir() if p.name != 'main.ini')
    assert names == sorted(p.name for p in folders['tog'].iterdir() if p.name != 'main.ini') and 'run.stats' in names
    for name in names:
        if not name.endswith('.npz'):
            assert (folders['seq'] / name).read_text() == (folders['tog'] / name).read_text(), name


# ------------------------------------------------------------------ the table of the mock posteriors
def test_the_smc_posteriors_table_is_standard_fits(tmp_path):
    """``sample_mocks(sampler='smc')`` over the stand-in, then ``write_mock_posteriors``: a standard FITS file with the SMC columns
    and header; the ensemble table's columns are what they were."""
    from fits_standard import check_file
    from vega_amd.montecarlo import MonteCarlo
    vega = _Vega()
    mc = MonteCarlo.__new__(MonteCarlo)
    mc.vega = vega
    vega.problem = type('P', (), dict(mc_config=None, items={}))()
    import vega_amd.montecarlo as M
    saved = M.item_scales
    M.item_scales = lambda prob, scale: {'x': 1.0}
    try:
        run = mc.sample_mocks(mocks={'x': np.zeros((3, 4))}, seed=2, driver='python', sampler='smc', particles=N, sweeps=4)
    finally:
        M.item_scales = saved
    post = mc.mc_posteriors
    assert post['sampler'] == 'smc' and post['mean'].shape == (3, 2) and post['covariance'].shape == (3, 2, 2)
    assert np.all(np.isfinite(post['log_z'])) and np.all(post['log_z_err'] > 0) and list(post['status']) == [1, 1, 1]
    assert np.array_equal(post['stages'], run.stage) and mc.mc_chains.shape == (3, N, 2) and mc.mc_chain_lnl.shape == (3, N)
    assert np.all((post['acceptance'] > 0.0) & (post['acceptance'] < 1.0))
    path = mc.write_mock_posteriors(tmp_path)
    check_file(str(path))
    raw = Path(path).read_bytes()
    for word in (b'a_mean', b'b_sd', b'log_z', b'log_z_err', b'stages', b'status', b'covariance', b'SAMPLER', b'PARTICLE', b'ESS',
                 b'SWEEPS', b'SEED'):
        assert word in raw, word
    assert b'_tau' not in raw and b'WALKERS' not in raw
    with pytest.raises(ValueError, match="'ensemble' or 'smc'"):
        mc.sample_mocks(mocks={'x': np.zeros((3, 4))}, sampler='nested')
