"""The weighted sample store attached to the nested and SMC sets on real engines: ``NestedSet.summary`` / ``SMCSet.summary`` on the
device equal the host restatement bit for bit, with and without ``boost_posterior`` / ``recycle``;
``sample_mocks_nested(summaries='device', weighted_quantiles=...)`` and its SMC counterpart against the default call on a twin
engine, down to the FITS table; one config end to end."""
import configparser

import numpy as np
import pytest

from conftest import GOLDEN
from test_chain_weighted_host import MOMENT_TOL

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]
NEW_KEYS = {'weighted_quantiles', 'quantile_values', 'lnl_max', 'best'}


def _sample_params(vega, names):
    defaults = {'bias_eta_LYA': ((-0.5, 0.0), 0.01), 'beta_LYA': ((0.5, 3.0), 0.05), 'ap': ((0.5, 1.5), 0.01), 'at': ((0.5, 1.5), 0.01)}
    return {'limits': {n: defaults[n][0] for n in names}, 'values': {n: vega.params[n] for n in names},
            'errors': {n: defaults[n][1] for n in names}}


def _fresh_mock_vega():
    """The auto problem with the synthetic covariance (mocks are drawn from one), on an engine of its own."""
    from vega_amd import VegaInterface, synthetic
    from vega_amd.setup import build_problem
    prob = build_problem('configs/auto/main.ini', search_dirs=[GOLDEN])
    for item in prob.items.values():
        item.set_covariance(synthetic.covariance(item.data_grid.rp, item.data_grid.rt))
    vega = VegaInterface(None, problem=prob, max_batch=256)
    vega.freeze_metals()
    return vega


@pytest.fixture
def mock_vegas():
    """Two engines built alike and used by nothing else, so that twin runs make the same sequence of engine calls."""
    pair = [_fresh_mock_vega(), _fresh_mock_vega()]
    yield pair
    for vega in pair:
        vega.close()


@pytest.fixture(scope='module')
def pool_vega():
    """One engine with a pool of 4 mocks installed."""
    from vega_amd.montecarlo import MonteCarlo
    vega = _fresh_mock_vega()
    for name, pool in MonteCarlo(vega).create_mocks(vega.compute_model(), 4, seed=1).items():
        vega.engine.set_mock_pool(name, pool)
    yield vega
    vega.close()


def _same(dev, host, with_q):
    keys = {'count', 'n_eff', 'mean', 'sd', 'covariance'} | (NEW_KEYS if with_q else set())
    assert set(dev) == set(host) == keys
    for key in keys:
        assert np.asarray(dev[key]).shape == np.asarray(host[key]).shape and np.asarray(dev[key]).dtype == np.asarray(host[key]).dtype, key
        assert np.asarray(dev[key]).tobytes() == np.asarray(host[key]).tobytes(), key


def _sensible(summ, found, n):
    """Quantile values are non-decreasing in q and stored samples; the best point is the argmax of the chain."""
    for e, part in enumerate(found):
        if part is None:
            assert summ['count'][e] == 0 and np.isnan(summ['quantile_values'][e]).all() and np.isnan(summ['lnl_max'][e])
            continue
        pts, lnl, w = part
        assert summ['count'][e] == lnl.size and np.all(np.diff(summ['quantile_values'][e], axis=1) >= 0.0)
        for d in range(n):
            assert np.all(np.isin(summ['quantile_values'][e, d], pts[:, d]))
        at = int(np.argmax(lnl))
        assert summ['lnl_max'][e] == lnl[at] and summ['best'][e].tobytes() == np.ascontiguousarray(pts[at]).tobytes()


# ------------------------------------------------------------------ the sets' own summaries
@pytest.mark.parametrize('boost', [0.0, 2.0])
def test_nested_set_summary(pool_vega, boost):
    from vega_amd import NestedSet
    sp = _sample_params(pool_vega, AUTO_SAMPLED)
    kw = dict(num_live=48, threads=12, num_repeats=3, seed=4, max_iterations=6, sample_params=sp, mock_rows=[2, 0, 3])
    run = NestedSet(pool_vega, 3, **kw, **({'boost_posterior': boost} if boost else {})).run()
    assert run.driver == 'device'
    found = run.samples()
    _same(run.summary(), run.summary(where='host'), False)
    dev = run.summary(weighted_quantiles=Q5)
    _same(dev, run.summary(weighted_quantiles=Q5, where='host'), True)
    _sensible(dev, found, 4)
    if boost:
        assert dev['count'].tolist() == [part[1].size for part in found] and np.all(dev['count'] > 6 * 12 + 48)
        _same(run.summary(boost=False), run.summary(boost=False, where='host'), False)
        assert run.summary(boost=False)['count'].tolist() == [6 * 12 + 48] * 3
    py = NestedSet(pool_vega, 3, driver='python', **kw, **({'boost_posterior': boost} if boost else {})).run()
    assert set(py.summary(weighted_quantiles=Q5)) == set(dev)
    for bad in (dict(where='gpu'), dict(weighted_quantiles=[1.5]), dict(weighted_quantiles=[])):
        with pytest.raises(ValueError):
            run.summary(**bad)
    _same(run.summary(), run.summary(where='host'), False)


@pytest.mark.parametrize('recycle', [False, True])
def test_smc_set_summary(pool_vega, recycle):
    from vega_amd.smc import SMCSet
    sp = _sample_params(pool_vega, AUTO_SAMPLED)
    kw = dict(particles=64, sweeps=4, seed=5, sample_params=sp, mock_rows=[1, 3, 0])
    run = SMCSet(pool_vega, 3, **kw, **(dict(n_total=200, recycle=True) if recycle else {})).run()
    assert run.driver == 'device'
    found = list(zip(*run.samples()))
    _same(run.summary(), run.summary(where='host'), False)
    dev = run.summary(weighted_quantiles=Q5)
    _same(dev, run.summary(weighted_quantiles=Q5, where='host'), True)
    _sensible(dev, found, 4)
    assert dev['count'].tolist() == [part[1].size for part in found]
    if recycle:
        assert np.all(dev['count'] > 64) and np.allclose(dev['n_eff'], run.n_eff(), rtol=100 * MOMENT_TOL['n_eff'] + 1e-12, atol=0)
        _same(run.summary(recycle=False), run.summary(recycle=False, where='host'), False)
    else:
        assert np.all(dev['n_eff'] == 64.0)          # (equal weights 1 / 64: every sum is exact)


# ------------------------------------------------------------------ a posterior per mock
def _moments_close(post, twin, chains):
    """The device moments against the default call's within the tolerances measured in tests/test_chain_weighted_host.py, plus
    the reference's own error: the host expressions (``w @ pts``, ``... / (1 - sum w^2)``) take sum w = 1, the samplers' weights
    sum to S = 1 within 1e-12 only (tests/test_smc_keep_gpu.py asserts that much), and the store normalises by S.  With w = S p
    the host mean is S x the mean and the host covariance S (1 - s2) / (1 - S^2 s2) x the covariance, s2 = sum p^2: to first
    order in S - 1 a relative (S - 1) and (S - 1) (1 + s2) / (1 - s2); the second order is below 1e-24.  S and s2 are taken
    from the kept chain with ``math.fsum``, not from the store.  Beside it, without any allowance: the device moments against
    the same host expressions on the weights normalised first, ``w / fsum(w)``, at the plain measured tolerance."""
    import math
    sd = twin['sd']
    off = np.array([abs(math.fsum(w) - 1.0) for _, _, w in chains])
    s2 = np.array([math.fsum(w * w) / math.fsum(w) ** 2 for _, _, w in chains])
    for m in range(len(chains)):
        print(f'mock {m}: |S - 1| {off[m]:.2e}, mean {np.max(np.abs(post["mean"][m] - twin["mean"][m]) / sd[m]):.2e} sd, covariance '
              f'{np.max(np.abs(post["covariance"][m] - twin["covariance"][m]) / np.outer(sd[m], sd[m])):.2e} sqrt(C_ii C_jj)')
    for m, (pts, _, w) in enumerate(chains):
        p = w / math.fsum(w)
        mean = p @ pts
        dev = pts - mean
        cov = (p[:, None] * dev).T @ dev / (1.0 - np.sum(p * p))
        root = np.sqrt(np.diag(cov))
        assert np.all(np.abs(post['mean'][m] - mean) <= MOMENT_TOL['mean'] * root), m
        assert np.all(np.abs(post['covariance'][m] - cov) <= MOMENT_TOL['covariance'] * np.outer(root, root)), m
    assert np.all(off <= 1e-12)
    grow = off * (1.0 + s2) / (1.0 - s2)
    assert np.all(np.abs(post['mean'] - twin['mean']) <= MOMENT_TOL['mean'] * sd + off[:, None] * np.abs(twin['mean']))
    assert np.all(np.abs(post['covariance'] - twin['covariance']) <=
                  MOMENT_TOL['covariance'] * sd[:, :, None] * sd[:, None, :] + grow[:, None, None] * np.abs(twin['covariance']))
    assert np.all(np.abs(post['sd'] - twin['sd']) <= (MOMENT_TOL['covariance'] + grow[:, None]) * sd)


def _table(path, post, names, asked):
    from fits_standard import check_file
    from vega_amd import fitslite
    check_file(path)
    hdu = fitslite.open(str(path))[1]
    cols = hdu.columns.names
    if not asked:
        assert 'lnl_max' not in cols and not [c for c in cols if c.endswith('_best') or '_q' in c] and 'QMETHOD' not in hdu.header
        return
    assert hdu.header['NQUANT'] == 5 and [hdu.header[f'QUANT{k}'] for k in range(5)] == Q5 and hdu.header['QMETHOD'] == 'inverted_cdf'
    for j, name in enumerate(names):
        for k in range(5):
            assert np.array_equal(hdu.data[f'{name}_q{k}'], post['quantile_values'][:, j, k])
        assert np.array_equal(hdu.data[f'{name}_best'], post['best'][:, j]) and np.array_equal(hdu.data[f'{name}_mean'], post['mean'][:, j])
    assert np.array_equal(hdu.data['lnl_max'], post['lnl_max'])


def test_sample_mocks_nested_on_the_device(mock_vegas, tmp_path):
    from vega_amd.montecarlo import MonteCarlo
    vega, twin_vega = mock_vegas
    sp = _sample_params(vega, AUTO_SAMPLED)
    mc, twin_mc = MonteCarlo(vega), MonteCarlo(twin_vega)
    kw = dict(num_mocks=3, seed=5, sample_params=sp, num_live=48, threads=12, num_repeats=3, max_iterations=6, boost_posterior=2.0)
    run = mc.sample_mocks_nested(summaries='device', weighted_quantiles=Q5, **kw)
    post = dict(mc.mc_posteriors)
    twin_mc.sample_mocks_nested(**kw)
    twin = twin_mc.mc_posteriors
    assert set(post) == set(twin) | NEW_KEYS and 'n_eff' in twin
    for a, b in zip(mc.mc_chains, twin_mc.mc_chains):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    _moments_close(post, twin, mc.mc_chains)
    assert np.all(np.abs(post['n_eff'] - twin['n_eff']) <= MOMENT_TOL['n_eff'] * twin['n_eff'])
    assert list(post['weighted_quantiles']) == Q5 and post['quantile_values'].shape == (3, 4, 5)
    _sensible(dict(post, count=np.array([c[1].size for c in mc.mc_chains])), mc.mc_chains, 4)
    _table(mc.write_mock_posteriors(tmp_path / 'asked'), post, AUTO_SAMPLED, True)
    _table(twin_mc.write_mock_posteriors(tmp_path / 'plain'), twin, AUTO_SAMPLED, False)
    host = run.summary(weighted_quantiles=Q5, where='host')
    for key in NEW_KEYS | {'mean', 'covariance'}:
        assert np.asarray(post[key]).tobytes() == np.asarray(host[key]).tobytes(), key
    with pytest.raises(ValueError, match='summaries'):
        mc.sample_mocks_nested(summaries='gpu', **kw)
    with pytest.raises(ValueError, match='quantiles'):
        mc.sample_mocks_nested(weighted_quantiles=[2.0], **kw)


def test_sample_mocks_smc_on_the_device(mock_vegas, tmp_path):
    from vega_amd.montecarlo import MonteCarlo
    vega, twin_vega = mock_vegas
    sp = _sample_params(vega, AUTO_SAMPLED)
    mc, twin_mc = MonteCarlo(vega), MonteCarlo(twin_vega)
    kw = dict(num_mocks=3, seed=5, sample_params=sp, sampler='smc', particles=64, sweeps=4, n_total=200, recycle=True)
    mc.sample_mocks(weighted_summaries='device', weighted_quantiles=Q5, **kw)
    post = dict(mc.mc_posteriors)
    twin_mc.sample_mocks(**kw)
    twin = twin_mc.mc_posteriors
    assert set(post) == set(twin) | NEW_KEYS
    for a, b in zip(mc.mc_chains, twin_mc.mc_chains):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    _moments_close(post, twin, mc.mc_chains)
    assert np.array_equal(post['n_eff'], twin['n_eff'])         # (the SMC set's n_eff stays its own)
    _sensible(dict(post, count=np.array([c[1].size for c in mc.mc_chains])), mc.mc_chains, 4)
    _table(mc.write_mock_posteriors(tmp_path / 'asked'), post, AUTO_SAMPLED, True)
    _table(twin_mc.write_mock_posteriors(tmp_path / 'plain'), twin, AUTO_SAMPLED, False)
    # with quantiles alone the moments keep the host's bits
    mc.sample_mocks(weighted_quantiles=Q5, **kw)
    assert mc.mc_posteriors['quantile_values'].shape == (3, 4, 5)
    with pytest.raises(ValueError, match='quantiles'):
        mc.sample_mocks(weighted_quantiles=Q5, num_mocks=3, sample_params=sp)           # (sampler='ensemble')
    with pytest.raises(ValueError, match="quantiles go with sampler='ensemble'"):
        mc.sample_mocks(quantiles=Q5, **kw)
    with pytest.raises(ValueError, match='weighted_summaries'):
        mc.sample_mocks(weighted_summaries='gpu', **kw)


# ------------------------------------------------------------------ one config end to end
def test_a_nested_config_with_weighted_quantiles_end_to_end(tmp_path):
    from conftest import mc_launcher_config
    from vega_amd import run_vega_sampler
    from vega_amd.nested import NestedSet
    config = mc_launcher_config(tmp_path)
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / config)
    cfg['control'].update(run_sampler='True', sampler='Nested')
    out = tmp_path / 'chains_mocks'
    out.mkdir()
    cfg['Nested'] = dict(path=str(out), name='run', mocks='3', num_live='48', threads='12', num_repeats='3', seed='4', max_iterations='6',
                         weighted_quantiles='0.025 0.16 0.5 0.84 0.975')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert isinstance(sampler, NestedSet) and sampler.E == 3
        post = sampler.vega.analysis.mc_posteriors
        assert list(post['weighted_quantiles']) == Q5 and post['quantile_values'].shape == (3, len(sampler.names), 5)
        assert post['quantile_values'].tobytes() == sampler.summary(weighted_quantiles=Q5)['quantile_values'].tobytes()
        _table(out / 'mock_posteriors.fits', post, list(sampler.names), True)
    finally:
        sampler.vega.close()
