"""The host-only pieces of the chain quantiles: the ``[Ensemble] quantiles`` setting, the table ``write_mock_posteriors`` writes
from a hand-made ``mc_posteriors``, and the samplers' ``quantiles`` / ``best`` / ``summary(quantiles=...)`` on the ``python``
driver over a stand-in likelihood (the rows on the host: the restatements of vega_amd/csrc/vmx_chain_select.h)."""
import configparser

import numpy as np
import pytest

from fits_standard import check_file
from test_chain_summary_host import _StandInVega
from vega_amd import ensemble as E
from vega_amd import fitslite

Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]


# ------------------------------------------------------------------ the samplers on the python driver
def test_the_samplers_answer_from_the_host_rows():
    vega = _StandInVega()
    run = E.EnsembleSet(vega, 2, 8, seed=3, driver='python', segment=7, chain='device').run(40)
    chain, lnl = run.get_chain(), run.get_log_lik()
    assert run._store is None
    q = run.quantiles(Q5, 5)
    assert q.shape == (2, 2, 5) and q.tobytes() == E.chain_quantiles(chain, Q5, 5).tobytes()
    assert np.all(np.diff(q, axis=2) >= 0.0)
    top, ref = run.best(5), E.chain_best(chain, lnl, 5)
    assert set(top) == {'lnl_max', 'best', 'best_row', 'best_walker'}
    for key in ref:
        assert np.asarray(top[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
    for e in range(2):
        flat = lnl[e, 5:].reshape(-1)
        assert top['lnl_max'][e] == flat.max() and (top['best_row'][e] - 5) * 8 + top['best_walker'][e] == int(np.argmax(flat))
    plain, full = run.summary(discard=5), run.summary(discard=5, quantiles=Q5)
    assert set(plain) == set(E.SUMMARY_KEYS) and set(full) == set(E.SUMMARY_KEYS) | set(E.SELECT_KEYS)
    assert full['quantiles'].tobytes() == q.tobytes() and list(full['q']) == Q5 and full['best'].tobytes() == top['best'].tobytes()
    for key in E.SUMMARY_KEYS:
        assert np.asarray(full[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    # the single sampler is the set of one, and a member answers like its set
    one = E.EnsembleSampler(vega, 8, seed=3, driver='python').run(40)
    assert np.array_equal(one.get_chain(), chain[0])
    assert one.quantiles(Q5, 5).tobytes() == q[0].tobytes() and one.quantiles(0.5).shape == (2, 1)
    a = one.best(5)
    assert isinstance(a['lnl_max'], float) and a['lnl_max'] == top['lnl_max'][0] and a['best'].tobytes() == top['best'][0].tobytes()
    assert a['best_row'] == top['best_row'][0] and a['best_walker'] == top['best_walker'][0]
    s1 = one.summary(discard=5, quantiles=Q5)
    assert set(s1) == set(full) and s1['quantiles'].shape == (2, 5) and set(one.summary(discard=5)) == set(E.SUMMARY_KEYS)
    member = run.member(1)
    assert member.quantiles(Q5, 5).tobytes() == q[1].tobytes() and member.best(5)['best_row'] == top['best_row'][1]
    for bad in (dict(q=[]), dict(q=[1.5]), dict(q=np.linspace(0, 1, 17)), dict(q=[0.5], discard=40), dict(q=[0.5], discard=-1)):
        with pytest.raises(ValueError):
            run.quantiles(**bad)
    with pytest.raises(ValueError):
        run.best(40)
    with pytest.raises(ValueError, match='no recorded rows'):
        E.EnsembleSampler(vega, 8, driver='python').best()
    ladder = E.TemperedEnsemble(vega, 8, ntemps=3)
    for call in (lambda: ladder.quantiles(Q5), lambda: ladder.best(), lambda: ladder.summary(quantiles=Q5)):
        with pytest.raises(ValueError, match='per rung'):
            call()


# ------------------------------------------------------------------ the settings
def _config(text):
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read_string(text)
    return cfg


SAMPLE = {'limits': {'a': (0.0, 1.0), 'b': (0.0, 1.0)}, 'values': {}, 'errors': {}}
HEAD = '[control]\nrun_sampler = True\nsampler = Ensemble\n'
MC = 'run_montecarlo = True\n[monte carlo]\nnum_mocks = 4\n'


def test_quantiles_parse(tmp_path):
    s = E.sampler_settings(_config(f'{HEAD}{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\nquantiles = 0.025 0.16 0.5 0.84 0.975\n'), SAMPLE)
    assert s['quantiles'] == Q5 and s['mocks'] == 3
    s = E.sampler_settings(_config(f'{HEAD}{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\nquantiles = 0, 1\n'), SAMPLE)
    assert s['quantiles'] == [0.0, 1.0]
    s = E.sampler_settings(_config(f'{HEAD}{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\n'), SAMPLE)
    assert 'quantiles' not in s
    s = E.sampler_settings(_config(f'{HEAD}{MC}[Ensemble]\npath = {tmp_path}\nmocks = 3\nquantiles = ' + ' '.join(['0.5'] * 16) + '\n'), SAMPLE)
    assert len(s['quantiles']) == 16


@pytest.mark.parametrize('head, body, match', [
    (HEAD, 'quantiles = 0.5\n', 'quantiles go with mocks'),
    (HEAD, 'quantiles = 0.5\nntemps = 3\n', 'quantiles and ntemps do not combine'),
    (HEAD + MC, 'mocks = 3\nquantiles = 0.5 1.5\n', r'quantiles: 1 .. 16 values in \[0, 1\]'),
    (HEAD + MC, 'mocks = 3\nquantiles = -0.1\n', r'quantiles: 1 .. 16 values in \[0, 1\]'),
    (HEAD + MC, 'mocks = 3\nquantiles = nan\n', r'quantiles: 1 .. 16 values in \[0, 1\]'),
    (HEAD + MC, 'mocks = 3\nquantiles =\n', r'quantiles: 1 .. 16 values in \[0, 1\]'),
    (HEAD + MC, 'mocks = 3\nquantiles = ' + ' '.join(['0.5'] * 17) + '\n', r'quantiles: 1 .. 16 values in \[0, 1\]'),
    (HEAD + MC, 'mocks = 3\nquantiles = median\n', r'quantiles: numbers in \[0, 1\]'),
])
def test_quantiles_refusals(tmp_path, head, body, match):
    with pytest.raises(ValueError, match=match):
        E.sampler_settings(_config(f'{head}[Ensemble]\npath = {tmp_path}\n{body}'), SAMPLE)


# ------------------------------------------------------------------ the table
def _posteriors(M=3, n=2, q=None):
    rng = np.random.default_rng(11)
    cov = np.einsum('mij,mkj->mik', *(2 * [rng.standard_normal((M, n, n))]))
    post = dict(names=['ap', 'bias_eta_LYA'][:n], mean=rng.standard_normal((M, n)), sd=np.sqrt(np.diagonal(cov, axis1=1, axis2=2)),
                covariance=cov, tau=1.0 + rng.random((M, n)), acceptance=rng.random(M), n_eff=100.0 * rng.random(M), steps=30, burn=10,
                thin=1, walkers=8, seed=5, driver='device', stats={})
    if q is not None:
        post.update(quantiles=np.asarray(q, dtype=np.float64), quantile_values=np.sort(rng.standard_normal((M, n, len(q))), axis=2),
                    lnl_max=-rng.random(M), best=rng.standard_normal((M, n)))
    return post


def test_the_table_gains_the_columns_only_when_asked(tmp_path):
    from vega_amd.montecarlo import MonteCarlo
    mc = MonteCarlo.__new__(MonteCarlo)
    mc.mc_posteriors = plain = _posteriors()
    path = mc.write_mock_posteriors(tmp_path / 'plain')
    check_file(path)
    hdu = fitslite.open(path)[1]
    old_names = list(hdu.columns.names)
    assert old_names == ['ap_mean', 'ap_sd', 'ap_tau', 'bias_eta_LYA_mean', 'bias_eta_LYA_sd', 'bias_eta_LYA_tau', 'acceptance', 'n_eff',
                         'covariance']
    assert 'NQUANT' not in hdu.header and not [k for k in hdu.header if k.startswith('QUANT')]
    mc.mc_posteriors = post = _posteriors(q=Q5)
    path = mc.write_mock_posteriors(tmp_path / 'with')
    check_file(path)
    hdu = fitslite.open(path)[1]
    new = [f'{nm}_{tail}' for nm in post['names'] for tail in ['q0', 'q1', 'q2', 'q3', 'q4', 'best']] + ['lnl_max']
    assert list(hdu.columns.names) == old_names + new
    assert hdu.header['NQUANT'] == 5 and [hdu.header[f'QUANT{k}'] for k in range(5)] == Q5 and hdu.header['STEPS'] == 30
    for j, nm in enumerate(post['names']):
        for k in range(5):
            assert np.array_equal(hdu.data[f'{nm}_q{k}'], post['quantile_values'][:, j, k])
        assert np.array_equal(hdu.data[f'{nm}_best'], post['best'][:, j]) and np.array_equal(hdu.data[f'{nm}_mean'], post['mean'][:, j])
    assert np.array_equal(hdu.data['lnl_max'], post['lnl_max']) and np.array_equal(hdu.data['n_eff'], post['n_eff'])
    for key in ('mean', 'sd', 'tau'):       # (the columns of ever hold what they held)
        assert np.array_equal(plain[key], post[key])
    # one parameter and sixteen quantiles: the widest table still validates
    mc.mc_posteriors = _posteriors(M=2, n=1, q=np.linspace(0, 1, 16))
    path = mc.write_mock_posteriors(tmp_path / 'wide')
    check_file(path)
    assert fitslite.open(path)[1].header['QUANT15'] == 1.0
