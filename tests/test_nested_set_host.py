"""A set of nested-sampling runs without a GPU: what vega_amd/csrc/vmx_nested.h adds for a set ("a set of runs": phases, the active
and the heading list, the row offsets and the row order), compiled with g++ under AddressSanitizer / UBSan into
tests/helpers/nested_set_driver.cpp, against the NumPy restatement ``python_iterations_many`` field for field after every round;
every run of the restatement against ``python_iterations`` on its stream bit for bit; a set cut into calls; a run without a finite
live lnL; the evidence of correlated Gaussians; what ``NestedSet`` and the ``[Nested]`` settings refuse."""
import configparser
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vega_amd import ensemble as E
from vega_amd import nested as N

REPO = Path(__file__).resolve().parents[1]


def _gauss(n, sigma=0.15, centre=0.5):
    def loglike(u, runs=None):
        d = (np.asarray(u) - centre) / sigma
        acc = np.zeros(d.shape[0])
        for i in range(n):
            acc = acc + d[:, i] * d[:, i]
        return -0.5 * acc
    return loglike


def _single(n, nlive, K, num_repeats, seed, stream, like, iterations, it0=0, stop=None):
    """The single run on ``stream``: drawn, taken to iteration ``it0``, then ``iterations`` more; (state at it0, result)."""
    u = N.draw_live(nlive, n, seed, stream)
    lnl = like(u)
    if it0:
        N.python_iterations(u, lnl, 0, it0, K, num_repeats, seed, stream, like)
    at = (u.copy(), lnl.copy())
    du, dl, dn, it, st = N.python_iterations(u, lnl, it0, iterations, K, num_repeats, seed, stream, like, stop)
    return at, (u, lnl, du, dl, dn, it, st)


def _same_as_single(u, lnl, dead, single):
    su, sl, du, dl, dn, _, _ = single
    assert np.array_equal(u, su) and np.array_equal(lnl, sl)
    assert np.array_equal(dead[0], du) and np.array_equal(dead[1], dl) and np.array_equal(dead[2], dn)


# ------------------------------------------------------------------ the set is its single runs
SHAPE = dict(n=2, nlive=20, K=6, num_repeats=3, seed=7)


def _set_of(streams, like, n_iterations, stop_at=None, it0=None, **shape):
    s = dict(SHAPE, **shape)
    E_ = len(streams)
    u, lnl = np.zeros((E_, s['nlive'], s['n'])), np.zeros((E_, s['nlive']))
    it = np.zeros(E_, dtype=np.int64)
    draw = it0 is None
    if not draw:
        for e, stream in enumerate(streams):
            (u[e], lnl[e]), _ = _single(s['n'], s['nlive'], s['K'], s['num_repeats'], s['seed'], stream, like, 0, it0=it0[e])
            it[e] = it0[e]
    stop = None if stop_at is None else (lambda e, iterations, dead_lnl, live_lnl: iterations >= stop_at[e])
    out = N.python_iterations_many(u, lnl, it, n_iterations, s['K'], s['num_repeats'], s['seed'], streams,
                                   lambda rows, runs: like(rows), stop, draw=draw)
    return (u, lnl, it) + out


@pytest.mark.parametrize('streams, stop_at, it0', [
    ([0, 1, 2], None, None),                    # the plain set
    ([5, 1, 9, 1], None, None),                 # other streams, another E, a stream twice
    ([3], None, None),                          # the set of one
    ([0, 1, 2], [2, 5, 3], None),               # runs that stop earlier
    ([0, 1, 2], None, [0, 3, 1]),               # a run entered three iterations later
])
def test_every_run_of_the_set_is_the_single_run_on_its_stream(streams, stop_at, it0):
    like = _gauss(2)
    u, lnl, it, dead, status, done, st = _set_of(streams, like, 5, stop_at, it0)
    for e, stream in enumerate(streams):
        want = 5 if stop_at is None else min(5, stop_at[e])
        first = 0 if it0 is None else it0[e]
        _, single = _single(2, 20, 6, 3, 7, stream, like, want, it0=first)
        _same_as_single(u[e], lnl[e], dead[e], single)
        assert done[e] == want and it[e] == first + want and status[e] == (N.STOPPED if stop_at is not None and stop_at[e] <= 5 else N.GOING)
        rows = single[6]['rows'] + (20 if it0 is None else 0)
        assert st['per_run'][e, 0] == rows and st['per_run'][e, 1] == single[6]['rows_own_position']
        assert st['per_run'][e, 2] == single[6]['rounds'] + want         # (every iteration ends in a round of its own)
    assert st['iterations'] == done.sum() and st['rows'] == st['per_run'][:, 0].sum()
    assert st['rounds'] == st['per_run'][:, 2].max()                    # (no run ever waits for another)
    if streams == [5, 1, 9, 1]:
        assert np.array_equal(u[1], u[3]) and not np.array_equal(u[0], u[1])


def test_a_set_cut_into_calls_is_the_same_set():
    like = _gauss(2)
    streams = [4, 0, 2]
    whole = _set_of(streams, like, 6)
    u, lnl = np.zeros((3, 20, 2)), np.zeros((3, 20))
    it = np.zeros(3, dtype=np.int64)
    parts = [[] for _ in streams]
    for k, cut in enumerate((0, 1, 3, 2)):
        dead, status, done, _ = N.python_iterations_many(u, lnl, it, cut, 6, 3, 7, streams, lambda rows, runs: like(rows), draw=k == 0)
        assert list(done) == [cut] * 3 and list(status) == [0, 0, 0]
        for e in range(3):
            parts[e].append(dead[e])
    assert np.array_equal(u, whole[0]) and np.array_equal(lnl, whole[1]) and list(it) == [6, 6, 6]
    for e in range(3):
        for j in range(3):
            assert np.array_equal(np.concatenate([p[j] for p in parts[e]]), whole[3][e][j])


def test_a_run_without_a_finite_live_lnl_gets_status_2():
    """Run 1 sees -inf everywhere: status 2, its arrays as they were, no iteration, and the others are what they are without it."""
    like = _gauss(2)

    def evaluate(rows, runs):
        return np.where(runs == 1, -np.inf, like(rows))

    u, lnl = np.full((3, 20, 2), 0.25), np.full((3, 20), -3.0)
    it = np.zeros(3, dtype=np.int64)
    dead, status, done, st = N.python_iterations_many(u, lnl, it, 3, 6, 3, 7, [0, 1, 2], evaluate, draw=True)
    assert list(status) == [0, 2, 0] and list(done) == [3, 0, 3] and list(it) == [3, 0, 3]
    assert np.all(u[1] == 0.25) and np.all(lnl[1] == -3.0) and dead[1][0].shape == (0, 2)
    assert list(st['per_run'][1]) == [20, 0, 0]
    for e in (0, 2):
        _, single = _single(2, 20, 6, 3, 7, e, like, 3)
        _same_as_single(u[e], lnl[e], dead[e], single)
    # without the draw the status is never 2, and n_iterations = 0 does nothing
    dead, status, done, _ = N.python_iterations_many(u, lnl, it, 0, 6, 3, 7, [0, 1, 2], evaluate)
    assert list(status) == [0, 0, 0] and list(done) == [0, 0, 0]


# ------------------------------------------------------------------ header <-> NumPy
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ is not installed')
    exe = tmp_path_factory.mktemp('nested_set') / 'nested_set_driver'
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
           '-o', str(exe), str(REPO / 'tests' / 'helpers' / 'nested_set_driver.cpp')]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    assert 'warning' not in built.stderr, built.stderr[-4000:]
    return exe


def _hx(v):
    return struct.unpack('<Q', struct.pack('<d', float(v)))[0].to_bytes(8, 'big').hex()


def _hexes(a):
    return ' '.join(_hx(v) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _doubles(tokens):
    return np.array([struct.unpack('<d', struct.pack('<Q', int(t, 16)))[0] for t in tokens])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_header_equals_the_restatement_after_every_round(driver):
    """E = 3, n = 2, nlive 16, K 4, num_repeats 3; the stop rule ends the runs after 2, 4 and 3 iterations, so that the heading
    and the active list change.  The restatement records every round (lists, counts, offsets, row order, every field of every
    thread, phases) and the answers it was given; the header replays the answers and must print the same."""
    E_, n, nlive, K, num_repeats, seed = 3, 2, 16, 4, 3, 11
    streams, stop_at = [6, 0, 3], [2, 4, 3]
    like = _gauss(n)
    u0 = np.stack([N.draw_live(nlive, n, seed, s) for s in streams])
    lnl0 = np.stack([like(u) for u in u0])
    rounds, answers = [], []

    def watch(r, state):
        T = state['threads']
        shot = {}
        for e in state['active']:
            t = T[e]
            asks = np.zeros(K, dtype=int)
            asks[state['requests'][e][0]] = 1
            shot[e] = [((int(asks[k]), int(t.state[k]), int(t.repeat[k]), int(t.n_out[k]), int(t.n_shrink[k]), int(t.inside[k]),
                         int(t.draw[k])), np.concatenate([[t.L[k], t.R[k], t.t[k], t.lnl[k]], t.x[k], t.y[k], t.d[k]]))
                       for k in range(K)]
        order = [(e, int(k)) for e in state['active'] for k in state['requests'][e][0]]
        rounds.append(dict(state, shot=shot, order=order))
        if state['total'] == 0:
            answers.append(np.empty(0))

    def evaluate(rows, runs):
        out = like(rows)
        answers.append(out)
        return out

    heads = []
    real_head = N.iteration_head

    def spy_head(live_u, live_lnl, K_, t, seed_, stream=0, clusters=None):
        head = real_head(live_u, live_lnl, K_, t, seed_, stream, clusters)
        heads.append((int(stream), int(t), head))
        return head

    u, lnl, it = u0.copy(), lnl0.copy(), np.zeros(E_, dtype=np.int64)
    N.iteration_head = spy_head
    try:
        dead, status, done, st = N.python_iterations_many(u, lnl, it, 10, K, num_repeats, seed, streams, evaluate,
                                                          stop=lambda e, i, d, l: i >= stop_at[e], watch=watch)
    finally:
        N.iteration_head = real_head
    assert list(done) == stop_at and list(status) == [1, 1, 1] and len(rounds) == len(answers) == st['rounds']
    text = f'S {E_} {n} {nlive} {K} {num_repeats} 10 {seed:x} ' + ' '.join(f'{s:x}' for s in streams) + ' 0 0 0 '
    text += ' '.join(str(s) for s in stop_at) + f' {_hexes(u0)} {_hexes(lnl0)} '
    text += ' '.join(f'{len(a)} {_hexes(a)}' for a in answers)
    out = subprocess.run([str(driver)], input=text + '\n', capture_output=True, text=True, timeout=600,
                         env={'ASAN_OPTIONS': 'detect_leaks=1', 'UBSAN_OPTIONS': 'print_stacktrace=1'})
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln.split() for ln in out.stdout.splitlines()]
    pos, heads_seen = 0, 0
    sizes = set()
    for r, want in enumerate(rounds):
        assert lines[pos] == ['N', str(r)]
        assert [int(t) for t in lines[pos + 1][2:]] == want['active'] and int(lines[pos + 1][1]) == len(want['active'])
        assert [int(t) for t in lines[pos + 2][2:]] == want['heading']
        sizes.add((len(want['active']), len(want['heading'])))
        pos += 3
        for e in want['heading']:
            stream, t, head = heads[heads_seen]
            heads_seen += 1
            assert lines[pos] == ['H', str(e), str(t)] and stream == streams[e]
            assert [int(v) for v in lines[pos + 1][1:]] == [int(v) for v in head['rank']]
            assert [int(v) for v in lines[pos + 2][1:]] == [int(v) for v in head['killed']]
            assert _same_bits(_doubles(lines[pos + 3][1:]), head['lstar'])
            assert _same_bits(_doubles(lines[pos + 4][1:]), head['mean'])
            assert _same_bits(_doubles(lines[pos + 5][1:]), head['cov'])
            assert int(lines[pos + 6][1]) == int(head['cholesky']) and _same_bits(_doubles(lines[pos + 6][2:]), head['C'])
            assert [int(v) for v in lines[pos + 7][1:]] == [int(v) for v in head['start']]
            pos += 8
        for e in want['active']:
            for k in range(K):
                row = lines[pos]
                ints, reals = want['shot'][e][k]
                assert row[0] == 'T' and int(row[1]) == e and int(row[2]) == k, (r, e, k, row[:3])
                assert tuple(int(v) for v in row[3:10]) == ints, (r, e, k, row[:10], ints)
                assert _same_bits(_doubles(row[10:]), reals), (r, e, k)
                pos += 1
        for a, e in enumerate(want['active']):
            assert lines[pos] == ['O', str(e), str(want['count'][a]), str(want['offset'][a])]
            pos += 1
        assert int(lines[pos][1]) == want['total']
        got = [int(v) for v in lines[pos][2:]]
        assert list(zip(got[0::2], got[1::2])) == want['order']             # ascending (run, thread)
        assert want['order'] == sorted(want['order'])
        assert [int(v) for v in lines[pos + 1][2:]] == [int(p) for p in want['phase']]
        pos += 2
    assert lines[pos] == ['Z', '3', '1', '1', '1'] and lines[pos + 1] == ['D', '3', '2', '4', '3']
    final = _doubles(lines[pos + 2][1:]).reshape(E_, nlive * (n + 1))
    for e in range(E_):
        assert _same_bits(final[e, :nlive * n], u[e]) and _same_bits(final[e, nlive * n:], lnl[e])
    assert heads_seen == len(heads) == sum(stop_at) and len(lines) == pos + 3
    # the lists did change: all three heading together, one alone, fewer runs than at the start
    assert (3, 3) in sizes and any(a == 3 and h == 1 for a, h in sizes) and any(a < 3 for a, _ in sizes)


# ------------------------------------------------------------------ evidence
def _correlated_gaussian(n, sigma=0.03):
    a = np.random.RandomState(1).randn(n, n)
    s = a @ a.T
    d = np.sqrt(np.diag(s))
    cov = s / np.outer(d, d) * sigma**2
    prec = np.linalg.inv(cov)

    def loglike(u, runs=None):
        d = np.asarray(u) - 0.5
        return -0.5 * np.einsum('ri,ij,rj->r', d, prec, d)

    return loglike, cov, 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]


def test_evidence_of_four_correlated_gaussians():
    """E = 4 runs at (nlive 128, K 32) on the correlated Gaussian of tests/test_nested_host.py (n = 2, sigma 0.03), streams 0 .. 3,
    each to its own termination: |log Z - true| <= 4 err, the bound of that file's analytic cases; run 2 is the NestedRun on
    stream 2 bit for bit."""
    loglike, cov, log_z_true = _correlated_gaussian(2)
    runs = N.NestedRunSet(loglike, 2, 4, num_live=128, num_repeats=10, threads=32, seed=0).run()
    log_z, err = runs.log_evidence()
    print('log Z', log_z, 'err', err, 'pulls', (log_z - log_z_true) / err, 'iterations', runs.iteration, 'rounds', runs.stats['rounds'])
    assert np.all(runs.finished) and list(runs.status) == [1, 1, 1, 1]
    assert np.all(np.abs(log_z - log_z_true) <= 4 * err)
    assert len(set(runs.iteration)) > 1                     # (the runs ended at iterations of their own)
    one = N.NestedRun(lambda u: loglike(u), 2, num_live=128, num_repeats=10, threads=32, seed=0, stream=2).run()
    assert one.log_evidence() == (log_z[2], err[2]) and one.iteration == runs.iteration[2] and one.information() == runs.information()[2]
    assert one.stats['rows'] == runs.runs[2].stats['rows'] == runs.stats['per_run'][2, 0]
    pts, lnl, w = runs.samples()[2]
    assert np.array_equal(pts, one.samples()[0]) and abs(w.sum() - 1) < 1e-12
    # run(3) then run(3) is run(6)
    a = N.NestedRunSet(loglike, 2, 3, num_live=40, threads=12, num_repeats=4, seed=1).run(3).run(3)
    b = N.NestedRunSet(loglike, 2, 3, num_live=40, threads=12, num_repeats=4, seed=1).run(6)
    for e in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(a.dead(e), b.dead(e))) and np.array_equal(a.runs[e].live_u, b.runs[e].live_u)
    assert list(a.iteration) == [6, 6, 6] and a.stats['calls'] == 2 and b.stats['calls'] == 1


# ------------------------------------------------------------------ NestedSet over a stand-in interface
class _Engine:
    """What the ``python`` driver asks of an engine (vega_amd.ensemble.EngineRows), with rows that live on the host."""
    max_batch = 16
    rows_device = 'cpu'

    def set_constant_nl_hint(self, on=True, gaussian=False):
        self.nl_hint = 0 if not on else 2 if gaussian else 1


class _Vega:
    """The surface of VegaInterface the set uses, over a Gaussian in (a, b) whose mean moves with the mock row."""
    param_names = ['a', 'fixed', 'b']
    max_batch = 16
    SHIFT = np.array([[0.0, 0.0], [0.02, -0.01], [-0.03, 0.02]])

    def __init__(self):
        self.params = {'a': 0.5, 'fixed': 2.0, 'b': 0.5}
        self.sample_params = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {'a': 0.5, 'b': 0.5}, 'errors': {'a': 0.03, 'b': 0.03}}
        self.engine = _Engine()
        self._icov = np.linalg.inv(0.03**2 * np.array([[1.0, 0.5], [0.5, 1.0]]))
        self.batches = []

    def freeze_metals(self, row=None):
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
        self.batches.append(t.shape[0])
        return torch.from_numpy(self._chi2(t.numpy(), None if mock_rows is None else mock_rows.numpy()))


def test_the_python_driver_gives_every_run_its_mock():
    """E = 3 on the mock rows (2, 0, 2), streams (4, 1, 4), chunks of 16 that cut through the runs' rows: every member is the single
    run on its stream with its mock's likelihood; members are read-only and write."""
    vega = _Vega()
    streams, rows = [4, 1, 4], [2, 0, 2]
    both = N.NestedSet(vega, 3, num_live=40, threads=12, num_repeats=4, streams=streams, mock_rows=rows, seed=5, driver='python').run(4)
    assert both.driver == 'python' and list(both.iteration) == [4, 4, 4] and max(vega.batches) == 16 and min(vega.batches) < 16
    for e, (stream, row) in enumerate(zip(streams, rows)):
        single = N.NestedRun(lambda u, row=row: 1.25 - 0.5 * vega._chi2(np.insert(u, 1, 2.0, axis=1), np.full(len(u), row)), 2,
                             num_live=40, threads=12, num_repeats=4, seed=5, stream=stream).run(4)
        member = both.member(e)
        assert np.array_equal(member.live_u, single.live_u) and np.array_equal(member.live_lnl, single.live_lnl)
        assert all(np.array_equal(x, y) for x, y in zip(member.dead(), single.dead())) and member.stream == stream
        assert member.log_evidence() == single.log_evidence() and member.stats['rows'] == single.stats['rows']
        with pytest.raises(RuntimeError, match='read-only'):
            member.run()
    assert np.array_equal(both.runs[0].live_u, both.runs[2].live_u) and not np.array_equal(both.runs[0].live_u, both.runs[1].live_u)
    with pytest.raises(IndexError):
        both.member(3)


def test_set_arguments_are_checked():
    vega = _Vega()
    for kw, match in ((dict(runs=2, clustering=True), 'clustering is not part of a set'), (dict(runs=0), 'at least one'),
                      (dict(runs=2, streams=[1]), 'one entry'), (dict(runs=2, mock_rows=[0]), 'one entry'),
                      (dict(runs=2, mock_rows=[0, -1]), 'negative'), (dict(runs=2, num_live=3), 'num_live'),
                      (dict(runs=2, num_live=20, threads=18), 'threads'), (dict(runs=2, driver='host'), 'driver')):
        with pytest.raises(ValueError, match=match):
            N.NestedSet(vega, **kw)
    with pytest.raises(ValueError, match='clustering is not part of a set'):
        N.NestedRunSet(None, 2, 2, clustering=True)
    with pytest.raises(ValueError, match='nothing has run'):
        N.NestedSet(vega, 2).log_evidence()


# ------------------------------------------------------------------ settings
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'ap': (0.5, 1.5), 'at': (0.5, 1.5)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Nested\n'
MC = '[monte carlo]\nap = 0.5 1.5 1.05 0.01\nat = 0.5 1.5 0.95 0.01\n'


def test_mocks_and_together_parse(tmp_path):
    s = E.sampler_settings(_config(f'{HEAD}run_montecarlo = True\n{MC}[Nested]\npath = {tmp_path}\nmocks = 5\nnum_live = 64\n'), SAMPLE)
    assert s['mocks'] == 5 and s['sampler'] == 'Nested' and s['num_live'] == 64 and 'together' not in s and 'replicas' not in s
    s = E.sampler_settings(_config(f'{HEAD}[Nested]\npath = {tmp_path}\nreplicas = 3\ntogether = True\n'), SAMPLE)
    assert s['together'] is True and s['replicas'] == 3 and 'mocks' not in s
    s = E.sampler_settings(_config(f'{HEAD}[Nested]\npath = {tmp_path}\nreplicas = 3\n'), SAMPLE)
    assert 'together' not in s and 'mocks' not in s             # (absent: the sequential path of today)


@pytest.mark.parametrize('text, match', [
    (HEAD + MC + '[Nested]\npath = {p}\nmocks = 3\n', r'\[Nested\] mocks needs "run_montecarlo = True"'),
    (HEAD + 'run_montecarlo = True\n[Nested]\npath = {p}\nmocks = 3\n', r'\[Nested\] mocks needs a "\[monte carlo\]" section'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Nested]\npath = {p}\nmocks = 0\n', r'\[Nested\] mocks: a whole number'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Nested]\npath = {p}\nmocks = 3\nreplicas = 2\n', 'every mock has a nested run of its own'),
    (HEAD + 'run_montecarlo = True\n' + MC + '[Nested]\npath = {p}\nmocks = 3\ndo_clustering = True\n', 'do_clustering'),
    (HEAD + '[Nested]\npath = {p}\nreplicas = 2\ntogether = True\ndo_clustering = True\n', 'do_clustering'),
    (HEAD + '[Nested]\npath = {p}\ntogether = perhaps\n', r'\[Nested\] together: True or False'),
])
def test_mocks_and_together_refusals(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(text.format(p=tmp_path)), SAMPLE)
