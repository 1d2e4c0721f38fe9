"""Order statistics, quantiles and the best row of a chain store on a real engine (include/vegamx.h: vmx_chain_store_order_stats,
vmx_chain_store_best; vega_amd/csrc/vmx_chain_select.h): a store alone gives the restatement's bits on columns built to break a
radix select, through uneven cuts, a ``reserve`` and a capacity above its rows; poisoned scratch changes nothing; attached to runs
the device answers are those of the sorted host chain, for both drivers; ``sample_mocks(quantiles=...)`` gives the same bits with
and without a chain on the host, down to the FITS table; every refusal leaves the store as it was."""
import configparser

import numpy as np
import pytest

import chain_select_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AUTO_SAMPLED = ['bias_eta_LYA', 'beta_LYA', 'ap', 'at']
Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]


def _sample_params(vega, names):
    defaults = {'bias_eta_LYA': ((-0.5, 0.0), 0.01), 'beta_LYA': ((0.5, 3.0), 0.05), 'ap': ((0.5, 1.5), 0.01), 'at': ((0.5, 1.5), 0.01)}
    return {'limits': {n: defaults[n][0] for n in names}, 'values': {n: vega.params[n] for n in names},
            'errors': {n: defaults[n][1] for n in names}}


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


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
    """Two engines built alike and used by nothing else: the last bits of a chi2 depend on the calls an engine has taken before
    (docs/LAB_NOTES.md: a twin engine is bitwise equal only on the same sequence of calls), so twin runs that are to be compared
    bit for bit each take a fresh one."""
    pair = [_fresh_mock_vega(), _fresh_mock_vega()]
    yield pair
    for vega in pair:
        vega.close()


def _same_best(got, ref):
    assert set(got) == set(ref) == {'lnl_max', 'best', 'best_row', 'best_walker'}
    for key in ref:
        assert np.asarray(got[key]).shape == np.asarray(ref[key]).shape, key
        assert np.asarray(got[key]).tobytes() == np.asarray(ref[key]).astype(np.asarray(got[key]).dtype).tobytes(), key


def _filled(eng, chain, lnl, slack=5):
    """A store with room past its rows, filled in uneven cuts with a ``reserve`` half-way."""
    Ens, T, W, n = chain.shape
    store = eng.chain_store(Ens, W, n, max(T // 2, 1))
    cuts = [c for c in (1, T // 3, T // 2) if 0 < c] if T > 3 else [T]
    done = 0
    for k, cut in enumerate(cuts + [T]):
        cut = min(cut, T - done)
        if cut <= 0:
            continue
        if done + cut > store.capacity:
            store.reserve(T + slack)
        store.append(chain[:, done:done + cut], lnl[:, done:done + cut])
        done += cut
    assert store.rows == T and (store.capacity > T or T == 1)
    return store


# ------------------------------------------------------------------ the store alone
@pytest.mark.parametrize('Ens, T, W, n', [(3, 85, 3, 3), (3, 128, 2, 3), (3, 86, 3, 3), (1, 1, 2, 1), (2, 257, 6, 64)])
def test_the_store_gives_the_restatements_bits(auto_vega, Ens, T, W, n):
    """N = T W one below, at and just above a 256-lane stride (255, 256, 258), the smallest store, and n at VMX_ENS_MAXN; E = 3 so
    that a wrong ensemble offset shows; every kind of adversarial column (E n = 9 kinds at the first three shapes); first rows 0,
    13 and rows - 1; R = 1 and R = 32 unsorted with repeats."""
    from vega_amd.ensemble import chain_best, chain_order_statistics
    variants = range(len(cases.KIND_NAMES)) if Ens * n == 1 else [0]
    for variant in variants:
        chain, lnl = cases.chain(Ens, T, W, n, variant, seed=3), cases.lnl_block(Ens, T, W, seed=3 + variant)
        store = _filled(auto_vega.engine, chain, lnl)
        try:
            for first in sorted({0, min(13, T - 1), T - 1}):
                N = (T - first) * W
                for R in (1, 32):
                    ranks = cases.ranks_of(N, R, seed=variant)
                    got = store.order_statistics(ranks, first)
                    assert got.shape == (Ens, n, R)
                    assert got.tobytes() == chain_order_statistics(chain, ranks, first).tobytes(), (variant, first, R)
                # the answer to a rank does not depend on the ranks asked with it, their order or their number
                alone = store.order_statistics(np.sort(np.unique(ranks))[:3], first)
                assert alone.tobytes() == chain_order_statistics(chain, np.sort(np.unique(ranks))[:3], first).tobytes()
                _same_best(store.best(first), chain_best(chain, lnl, first))
                assert set(store.best(first, position=False)) == {'lnl_max', 'best_row', 'best_walker'}
        finally:
            store.close()


def test_best_row_kinds(auto_vega):
    """Five ensembles, one per kind of lnL block (ties, NaNs around the maximum, all NaN, NaN and -inf only, plain)."""
    from vega_amd.ensemble import chain_best
    chain, lnl = cases.chain(5, 86, 3, 2, 8, seed=4), cases.lnl_block(5, 86, 3, seed=4)
    store = _filled(auto_vega.engine, chain, lnl)
    try:
        for first in (0, 13, 85):
            got = store.best(first)
            _same_best(got, chain_best(chain, lnl, first))
            assert got['best_row'][2] == -1 and got['best_walker'][2] == -1 and np.isnan(got['lnl_max'][2]) and np.all(np.isnan(got['best'][2]))
        assert store.best(0)['lnl_max'][3] == -np.inf and store.best(0)['best_row'][3] >= 0
    finally:
        store.close()


def test_poisoned_scratch_changes_nothing():
    """Three fresh engines - the switch off, off and on: the same calls on a larger and then a smaller range of a store (its
    scratch kept from the larger call) and on a second, smaller store give the same bits on all three."""
    from vega_amd import VegaInterface
    from vega_amd.engine import poison_scratch
    from vega_amd.ensemble import chain_best, chain_order_statistics
    big, big_lnl = cases.chain(3, 86, 3, 3, 0, seed=6), cases.lnl_block(3, 86, 3, seed=6)
    small, small_lnl = cases.chain(2, 20, 4, 2, 4, seed=7), cases.lnl_block(2, 20, 4, seed=7)
    calls = [(big, big_lnl, 0), (big, big_lnl, 60), (small, small_lnl, 0), (small, small_lnl, 19)]

    def sequence(vega):
        out = []
        stores = {}
        try:
            for chain, lnl, first in calls:
                if id(chain) not in stores:
                    stores[id(chain)] = _filled(vega.engine, chain, lnl)
                store = stores[id(chain)]
                ranks = cases.ranks_of((chain.shape[1] - first) * chain.shape[2], 32, seed=first)
                top = store.best(first)
                out.append((store.order_statistics(ranks, first), top['lnl_max'], top['best'], top['best_row'], top['best_walker']))
        finally:
            for store in stores.values():
                store.close()
        return out

    outs = []
    for k in range(3):
        vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=16)
        try:
            with poison_scratch(k == 2):
                outs.append(sequence(vega))
        finally:
            vega.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for (chain, lnl, first), got in zip(calls, outs[2]):
        ranks = cases.ranks_of((chain.shape[1] - first) * chain.shape[2], 32, seed=first)
        assert got[0].tobytes() == chain_order_statistics(chain, ranks, first).tobytes()
        assert got[1].tobytes() == chain_best(chain, lnl, first)['lnl_max'].tobytes()


# ------------------------------------------------------------------ attached to runs
MOVES = {'stretch': {}, 'mixture': dict(moves=[('de', 0.5), ('snooker', 0.3), ('cov', 0.2)])}


@pytest.mark.parametrize('thin', [1, 3])
@pytest.mark.parametrize('kind', list(MOVES))
def test_attached_to_runs(auto_vega, kind, thin):
    """EnsembleSet(E = 3, W = 8), 40 steps: the device order statistics are the sorted ``get_chain()``, quantiles and the best row
    agree between the device and the ``python`` driver bit for bit, ``summary(quantiles=...)`` adds exactly the new keys and
    ``summary()`` keeps exactly ``SUMMARY_KEYS``; a member and a closed set answer from the host rows with the same bits."""
    from vega_amd import EnsembleSet
    from vega_amd.ensemble import SELECT_KEYS, SUMMARY_KEYS, chain_best, chain_order_statistics, chain_quantiles
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    kw = dict(seed=7, thin=thin, segment=7, sample_params=sp, **MOVES[kind])
    dev = EnsembleSet(auto_vega, 3, 8, chain='device', **kw).run(40)
    assert dev._store is not None and dev._chain == []
    chain, lnl = dev.get_chain(), dev.get_log_lik()
    rows = 40 // thin
    for discard in (0, 3):
        N = (rows - discard) * 8
        ranks = cases.ranks_of(N, 32, seed=thin)
        got = dev._store.order_statistics(ranks, discard)
        assert got.tobytes() == chain_order_statistics(chain, ranks, discard).tobytes()
        ref = np.sort(np.moveaxis(chain[:, discard:], 3, 1).reshape(3, 4, N), axis=-1)[:, :, ranks]
        assert np.array_equal(got, ref)             # (sampled positions: finite, and no -0)
        assert dev.quantiles(Q5, discard).tobytes() == chain_quantiles(chain, Q5, discard).tobytes()
        _same_best(dev.best(discard), chain_best(chain, lnl, discard))
        top = dev.best(discard)
        for e in range(3):
            flat = lnl[e, discard:].reshape(-1)
            assert top['lnl_max'][e] == flat.max() and (top['best_row'][e] - discard) * 8 + top['best_walker'][e] == int(np.argmax(flat))
    py = EnsembleSet(auto_vega, 3, 8, chain='device', driver='python', **kw).run(40)
    assert py._store is None and np.array_equal(py.get_chain(), chain)
    assert py.quantiles(Q5, 3).tobytes() == dev.quantiles(Q5, 3).tobytes()
    _same_best(py.best(3), dev.best(3))
    plain, full = dev.summary(discard=3), dev.summary(discard=3, quantiles=Q5)
    assert set(plain) == set(SUMMARY_KEYS) and set(full) == set(SUMMARY_KEYS) | set(SELECT_KEYS)
    assert full['quantiles'].shape == (3, 4, 5) and list(full['q']) == Q5 and full['best'].shape == (3, 4)
    theirs = py.summary(discard=3, quantiles=Q5)
    assert set(theirs) == set(full) and set(py.summary(discard=3)) == set(SUMMARY_KEYS)
    for key in full:
        assert np.asarray(full[key]).tobytes() == np.asarray(theirs[key]).astype(np.asarray(full[key]).dtype).tobytes(), key
    for key in SUMMARY_KEYS:
        assert np.asarray(full[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    member = dev.member(1)
    assert member.quantiles(Q5, 3).tobytes() == full['quantiles'][1].tobytes()
    assert member.best(3)['best'].tobytes() == full['best'][1].tobytes() and member.best(3)['best_row'] == full['best_row'][1]
    assert set(member.summary(discard=3, quantiles=Q5)) == set(full)
    dev.close()
    assert dev._store is None and dev.quantiles(Q5, 3).tobytes() == full['quantiles'].tobytes()
    _same_best(dev.best(3), {key: full[key] for key in ('lnl_max', 'best', 'best_row', 'best_walker')})


def test_the_single_sampler_is_the_set_of_one(auto_vega):
    from vega_amd import EnsembleSampler, EnsembleSet
    from vega_amd.ensemble import SELECT_KEYS, SUMMARY_KEYS, chain_quantiles
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    one = EnsembleSampler(auto_vega, 8, seed=7, stream=2, segment=7, sample_params=sp, chain='device').run(40)
    both = EnsembleSet(auto_vega, 1, 8, streams=[2], seed=7, segment=7, sample_params=sp, chain='device').run(40)
    assert one._store is not None and one._store.E == 1
    q = one.quantiles(Q5, 5)
    assert q.shape == (4, 5) and q.tobytes() == both.quantiles(Q5, 5)[0].tobytes() == chain_quantiles(one.get_chain(), Q5, 5).tobytes()
    a, b = one.best(5), both.best(5)
    assert isinstance(a['lnl_max'], float) and a['best'].shape == (4,) and a['lnl_max'] == b['lnl_max'][0]
    assert a['best'].tobytes() == b['best'][0].tobytes() and a['best_row'] == b['best_row'][0] and a['best_walker'] == b['best_walker'][0]
    full = one.summary(discard=5, quantiles=Q5)
    assert set(full) == set(SUMMARY_KEYS) | set(SELECT_KEYS) and set(one.summary(discard=5)) == set(SUMMARY_KEYS)
    assert full['quantiles'].tobytes() == q.tobytes()
    host = EnsembleSampler(auto_vega, 8, seed=7, stream=2, segment=7, sample_params=sp).run(40)
    assert host.quantiles(Q5, 5).tobytes() == q.tobytes() and host.best(5)['best'].tobytes() == a['best'].tobytes()


# ------------------------------------------------------------------ a posterior per mock: quantiles without a chain on the host
def test_sample_mocks_with_quantiles(mock_vegas, tmp_path):
    """``summaries='device', keep_chains=False, quantiles=...`` on one engine and the twin ``summaries='host', keep_chains=True`` on
    another built alike, the same seed: the runs make the same engine calls, so the chains are equal bit for bit (asserted) and
    with them ``quantile_values``, ``lnl_max`` and ``best``."""
    from fits_standard import check_file
    from vega_amd import fitslite
    from vega_amd.ensemble import chain_best, chain_quantiles
    from vega_amd.montecarlo import MonteCarlo
    vega, twin_vega = mock_vegas
    sp = _sample_params(vega, AUTO_SAMPLED)
    mc, twin_mc = MonteCarlo(vega), MonteCarlo(twin_vega)
    kw = dict(num_mocks=4, walkers=8, steps=30, seed=5, sample_params=sp)
    lean = mc.sample_mocks(summaries='device', keep_chains=False, quantiles=Q5, **kw)
    assert mc.mc_chains is None and mc.mc_chain_lnl is None and lean._chain == [] and lean._fetched == {} and lean._store.rows == 30
    post = dict(mc.mc_posteriors)
    assert list(post['quantiles']) == Q5 and post['quantile_values'].shape == (4, 4, 5) and post['lnl_max'].shape == (4,) and post['best'].shape == (4, 4)
    path = mc.write_mock_posteriors(tmp_path / 'lean')
    # the rows the store holds, fetched only now: the device answers are the restatements' over them
    held, held_lnl = lean.get_chain(), lean.get_log_lik()
    assert post['quantile_values'].tobytes() == chain_quantiles(held, Q5, 10).tobytes()
    top = chain_best(held, held_lnl, 10)
    assert post['lnl_max'].tobytes() == top['lnl_max'].tobytes() and post['best'].tobytes() == top['best'].tobytes()
    lean.discard_chain()
    twin_mc.sample_mocks(summaries='host', keep_chains=True, quantiles=Q5, **kw)
    twin = twin_mc.mc_posteriors
    assert twin_mc.mc_chains.tobytes() == held.tobytes() and twin_mc.mc_chain_lnl.tobytes() == held_lnl.tobytes()
    for key in ('quantile_values', 'lnl_max', 'best'):
        assert post[key].tobytes() == twin[key].tobytes(), key
    mc.mc_chains, mc.mc_chain_lnl = twin_mc.mc_chains, twin_mc.mc_chain_lnl
    # the best point is the argmax of the kept chain behind the burn-in (a third of the steps), the quantiles those of its rows
    for m in range(4):
        flat = mc.mc_chain_lnl[m, 10:].reshape(-1)
        at = int(np.argmax(flat))
        assert post['lnl_max'][m] == flat[at] and post['best'][m].tobytes() == mc.mc_chains[m, 10 + at // 8, at % 8].tobytes()
    # (against NumPy's own quantiles: N = 160 values per column, so the bound of tests/test_chain_select_host.py, 14 u m + u (4 N +
    # 2) gap with gap <= 2 m, stays below 1300 u m = 1.5e-13 m; held to that here)
    ref = np.quantile(mc.mc_chains[:, 10:].reshape(4, -1, 4), Q5, axis=1, method='linear')
    np.testing.assert_allclose(post['quantile_values'], np.moveaxis(ref, 0, 2), rtol=1.5e-13, atol=0.0)
    assert np.all(np.diff(post['quantile_values'], axis=2) >= 0.0)
    # the table validates and carries the new columns only when asked
    check_file(path)
    hdu = fitslite.open(path)[1]
    assert hdu.header['NQUANT'] == 5 and [hdu.header[f'QUANT{k}'] for k in range(5)] == Q5
    for j, name in enumerate(AUTO_SAMPLED):
        for k in range(5):
            assert np.array_equal(hdu.data[f'{name}_q{k}'], post['quantile_values'][:, j, k])
        assert np.array_equal(hdu.data[f'{name}_best'], post['best'][:, j]) and np.array_equal(hdu.data[f'{name}_mean'], post['mean'][:, j])
    assert np.array_equal(hdu.data['lnl_max'], post['lnl_max'])
    mc.sample_mocks(summaries='device', keep_chains=False, **kw).discard_chain()
    plain = mc.mc_posteriors
    assert not {'quantiles', 'quantile_values', 'lnl_max', 'best'} & set(plain)
    for key in ('mean', 'covariance', 'tau'):
        assert plain[key].tobytes() == post[key].tobytes(), key
    names = fitslite.open(mc.write_mock_posteriors(tmp_path / 'plain'))[1].columns.names
    assert 'lnl_max' not in names and not [c for c in names if c.endswith('_best') or '_q' in c]
    with pytest.raises(ValueError, match="quantiles go with sampler='ensemble'"):
        mc.sample_mocks(sampler='smc', quantiles=Q5, **kw)
    with pytest.raises(ValueError, match='quantiles'):
        mc.sample_mocks(quantiles=[1.5], **kw)


def test_a_config_with_mocks_and_quantiles_end_to_end(tmp_path):
    from conftest import mc_launcher_config
    from fits_standard import check_file
    from vega_amd import EnsembleSet, fitslite, run_vega_sampler
    config = mc_launcher_config(tmp_path)
    cfg = configparser.ConfigParser()
    cfg.optionxform = str
    cfg.read(tmp_path / config)
    cfg['control'].update(run_sampler='True', sampler='Ensemble')
    out = tmp_path / 'chains_mocks'
    out.mkdir()
    cfg['Ensemble'] = dict(path=str(out), name='run', mocks='3', walkers='8', steps='30', seed='4', quantiles='0.025 0.16 0.5 0.84 0.975')
    with open(tmp_path / config, 'w') as f:
        cfg.write(f)
    sampler = run_vega_sampler(config, search_dirs=[tmp_path, GOLDEN], print_func=lambda *_: None)
    try:
        assert isinstance(sampler, EnsembleSet) and sampler.E == 3 and sampler.chain_mode == 'device' and sampler._store is not None
        post = sampler.vega.analysis.mc_posteriors
        assert list(post['quantiles']) == Q5 and post['quantile_values'].shape == (3, len(sampler.names), 5)
        assert post['quantile_values'].tobytes() == sampler.quantiles(Q5, discard=10).tobytes()
        check_file(out / 'mock_posteriors.fits')
        hdu = fitslite.open(str(out / 'mock_posteriors.fits'))[1]
        assert hdu.header['NQUANT'] == 5 and np.array_equal(hdu.data['lnl_max'], post['lnl_max'])
        for j, name in enumerate(sampler.names):
            assert np.array_equal(hdu.data[f'{name}_q2'], post['quantile_values'][:, j, 2])
            assert np.array_equal(hdu.data[f'{name}_best'], post['best'][:, j])
        assert (out / 'run_mock2.txt').exists()
    finally:
        sampler.vega.close()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_store_as_it_was(auto_vega):
    import ctypes as C
    from vega_amd import EnsembleSampler, EnsembleSet
    from vega_amd.engine import EngineError
    from vega_amd.ensemble import chain_summary
    eng = auto_vega.engine
    chain, lnl = cases.chain(2, 10, 4, 2, 8, seed=9), cases.lnl_block(5, 10, 4, seed=9)[[4, 0]]
    store = _filled(eng, chain, lnl)
    dptr, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    try:
        before = store.summary(1)

        def untouched():
            after = store.summary(1)
            assert all(np.asarray(after[key]).tobytes() == np.asarray(before[key]).tobytes() for key in before)
            assert store.rows == 10 and store.fetch()[0].tobytes() == chain.tobytes()
        N = 40
        for ranks, first in (([], 0), (np.arange(33), 0), ([-1], 0), ([N], 0), ([0, N - 4], 1), ([0], 10), ([0], -1)):
            with pytest.raises(EngineError, match='invalid argument'):
                store.order_statistics(ranks, first)
            untouched()
        for first in (10, -1):
            with pytest.raises(EngineError, match='invalid argument'):
                store.best(first)
            untouched()
        # NULL store and NULL outputs, at the C entries themselves
        lib, h = eng.lib, store._handle()
        ranks, values = np.zeros(1, dtype=np.int64), np.zeros((2, 2, 1))
        top, row, walker = np.zeros(2), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
        rp, vp, tp = ranks.ctypes.data_as(i64p), values.ctypes.data_as(dptr), top.ctypes.data_as(dptr)
        wp, op = walker.ctypes.data_as(C.POINTER(C.c_int32)), row.ctypes.data_as(i64p)
        assert lib.vmx_chain_store_order_stats(None, 0, 1, rp, vp) == -1 and b'invalid argument' in lib.vmx_last_error()
        assert lib.vmx_chain_store_order_stats(h, 0, 1, None, vp) == -1 and lib.vmx_chain_store_order_stats(h, 0, 1, rp, None) == -1
        assert lib.vmx_chain_store_best(None, 0, tp, op, wp, None) == -1 and lib.vmx_chain_store_best(h, 0, None, op, wp, None) == -1
        assert lib.vmx_chain_store_best(h, 0, tp, None, wp, None) == -1 and lib.vmx_chain_store_best(h, 0, tp, op, None, None) == -1
        untouched()
        assert lib.vmx_chain_store_best(h, 0, tp, op, wp, None) == 0 and lib.vmx_chain_store_order_stats(h, 0, 1, rp, vp) == 0
        untouched()
        assert store.order_statistics([N - 5], 1).shape == (2, 2, 1)
    finally:
        store.close()
    # (N >= 2^31 needs a store of tens of GiB filled row by row: that refusal is one function of the header, held to its
    # definition in tests/test_chain_select_host.py::test_the_count_limit)
    sp = _sample_params(auto_vega, AUTO_SAMPLED)
    run = EnsembleSet(auto_vega, 2, 8, seed=1, sample_params=sp, chain='device').run(6)
    ref = run.summary()
    for bad in (dict(q=[]), dict(q=[-0.5]), dict(q=[0.5, 1.01]), dict(q=np.linspace(0, 1, 17)), dict(q=[0.5], discard=6), dict(q=[0.5], discard=-1)):
        with pytest.raises(ValueError):
            run.quantiles(**bad)
    with pytest.raises(ValueError, match='quantiles'):
        run.summary(quantiles=[2.0])
    with pytest.raises(EngineError, match='invalid argument'):
        run.best(6)
    assert all(np.asarray(run.summary()[key]).tobytes() == np.asarray(ref[key]).tobytes() for key in ref)
    run.close()
    with pytest.raises(ValueError, match='no recorded rows'):
        EnsembleSampler(auto_vega, 8, sample_params=sp, driver='python').quantiles([0.5])
