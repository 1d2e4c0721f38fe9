"""The weighted sample store on a real engine (include/vegamx.h: vmx_sample_store_*; vega_amd/csrc/vmx_chain_weighted.h): a store
alone gives the restatement's bits (vega_amd/weighted.py) for ragged sets, every kind of weight and column and targets that sit on
the cumulative sums; a ``put`` replaces a longer set by a shorter one; poisoned scratch changes nothing; every refusal leaves the
store and the engine usable."""
import numpy as np
import pytest

import chain_weighted_cases as wc
from conftest import GOLDEN
from vega_amd import weighted as W

pytestmark = pytest.mark.gpu

Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]
COUNTS = (0, 1, 255, 256, 257)


@pytest.fixture(scope='module')
def auto_vega():
    from vega_amd import VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    yield vega
    vega.close()


def _filled(eng, sets, slack=4):
    n = sets[0][0].shape[1]
    store = eng.sample_store(len(sets), n, max(len(s[2]) for s in sets) + slack)
    for e, (x, lnl, w) in enumerate(sets):
        store.put(e, x, lnl, w)
    return store


def _check(store, sets, targets, where=None):
    """Summary, order statistics and best point of the store against the restatement of every set, bit for bit."""
    summ, top, values = store.summary(), store.best(), store.order_statistics(targets)
    assert store.counts().tolist() == [len(s[2]) for s in sets]
    for e, (x, lnl, w) in enumerate(sets):
        ref, best = W.weighted_summary(x, w), W.weighted_best(x, lnl)
        for key in ('S', 'n_eff', 'mean', 'sd', 'covariance', 'w_max'):
            assert np.asarray(summ[key][e]).tobytes() == np.asarray(ref[key], dtype=np.float64).tobytes(), (key, e, where)
        assert summ['total'][e] == ref['total'] and summ['count'][e] == ref['count'], (e, where)
        assert values[e].tobytes() == W.weighted_order_statistics(x, w, targets[e]).tobytes(), (e, where)
        assert top['index'][e] == best['index'] and top['best'][e].tobytes() == best['best'].tobytes(), (e, where)
        assert np.float64(top['lnl_max'][e]).tobytes() == np.float64(best['lnl_max']).tobytes(), (e, where)
    return summ, top, values


# ------------------------------------------------------------------ the store alone
@pytest.mark.parametrize('n', [1, 3])
def test_the_store_gives_the_restatements_bits(auto_vega, n):
    """Five sets of 0, 1, 255, 256 and 257 rows (one below, at and above a 256-lane stride) in a store with room past the rows,
    every kind of weight, columns with NaNs that carry weight and +-0, equal positions under different weights; one target and
    sixteen (unsorted, with repeats, 1 and M, a cumulative sum and the one after it); then E = 1."""
    for k, kind in enumerate(wc.WEIGHTS):
        sets = wc.sets_of(257, n, kind, variant=k, seed=2, counts=COUNTS)
        if kind == 'log-normal':
            sets[3] = wc.sample_set(256, n, kind, k, seed=2, equal_x=True)
        store = _filled(auto_vega.engine, sets)
        try:
            for R in (1, 16):
                _check(store, sets, [wc.targets_of(s, R, seed=k) for s in sets], (kind, R))
            assert set(store.best(position=False)) == {'lnl_max', 'index'}
            q = store.weighted_quantiles(Q5)
            assert q.shape == (5, n, 5)
            for e, (x, _, w) in enumerate(sets):
                assert q[e].tobytes() == W.weighted_quantiles(x, w, Q5).tobytes()
            x, lnl, w = store.fetch(4)
            assert x.tobytes() == sets[4][0].tobytes() and lnl.tobytes() == sets[4][1].tobytes() and w.tobytes() == sets[4][2].tobytes()
        finally:
            store.close()
        one = _filled(auto_vega.engine, sets[4:])
        try:
            _check(one, sets[4:], [wc.targets_of(sets[4], 16, seed=k)], (kind, 'E = 1'))
        finally:
            one.close()


def test_sixty_four_columns(auto_vega):
    sets = wc.sets_of(40, 64, 'log-normal', variant=0, seed=5, counts=(40, 0, 7))
    store = _filled(auto_vega.engine, sets)
    try:
        _check(store, sets, [wc.targets_of(s, 16, seed=1) for s in sets])
    finally:
        store.close()


def test_a_tree_longer_than_the_lds(auto_vega):
    """8193 rows: the first count whose tree (8192 terms after the first level) leaves the work-group's LDS; beside a short set."""
    sets = [wc.sample_set(8193, 2, 'log-normal', 8, seed=8), wc.sample_set(300, 2, 'a third zero', 8, seed=8)]
    store = _filled(auto_vega.engine, sets)
    try:
        _check(store, sets, [wc.targets_of(s, 16, seed=4) for s in sets])
    finally:
        store.close()


def test_put_replaces_a_longer_set_by_a_shorter_one(auto_vega):
    sets = wc.sets_of(257, 3, 'log-normal', variant=3, seed=3, counts=(257, 256, 40))
    store = _filled(auto_vega.engine, sets)
    try:
        _check(store, sets, [wc.targets_of(s, 16) for s in sets])
        sets[0] = wc.sample_set(19, 3, 'one dominant', 5, seed=9)
        store.put(0, *sets[0])
        _check(store, sets, [wc.targets_of(s, 16) for s in sets], 'shorter')
        sets[1] = wc.sample_set(0, 3, 'all equal', 0)
        store.put(1, *sets[1])
        summ, top, values = _check(store, sets, [wc.targets_of(s, 16) for s in sets], 'emptied')
        assert np.isnan(summ['mean'][1]).all() and top['index'][1] == -1 and np.isnan(values[1]).all() and store.fetch(1)[0].shape == (0, 3)
    finally:
        store.close()


def test_poisoned_scratch_changes_nothing():
    """Three fresh engines - the switch off, off and on: a store, a shorter set put into it (the scratch kept from the longer one)
    and a second, smaller store give the same bits on all three, and the restatement's."""
    from vega_amd import VegaInterface
    from vega_amd.engine import poison_scratch
    big = wc.sets_of(257, 3, 'a third zero', variant=1, seed=6, counts=COUNTS)
    small = wc.sets_of(40, 2, 'beyond 2^32', variant=2, seed=7, counts=(40, 3))
    shorter = wc.sample_set(30, 3, 'log-normal', 4, seed=6)

    def sequence(vega):
        out = []
        a = _filled(vega.engine, big)
        try:
            out.append(_check(a, big, [wc.targets_of(s, 16) for s in big]))
            now = big[:4] + [shorter]
            a.put(4, *shorter)
            out.append(_check(a, now, [wc.targets_of(s, 16) for s in now]))
            b = _filled(vega.engine, small)
            try:
                out.append(_check(b, small, [wc.targets_of(s, 16) for s in small]))
            finally:
                b.close()
        finally:
            a.close()
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
        for (s0, t0, v0), (s1, t1, v1) in zip(outs[0], other):
            assert v0.tobytes() == v1.tobytes() and s0['total'] == s1['total']
            assert all(np.asarray(s0[key]).tobytes() == np.asarray(s1[key]).tobytes() for key in s0 if key != 'total')
            assert all(t0[key].tobytes() == t1[key].tobytes() for key in t0)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_store_and_the_engine_usable(auto_vega):
    import ctypes as C
    from vega_amd.engine import EngineError
    eng = auto_vega.engine
    sets = wc.sets_of(40, 2, 'log-normal', variant=8, seed=9, counts=(40, 0, 12))
    store = _filled(eng, sets, slack=4)
    targets = [wc.targets_of(s, 16) for s in sets]
    try:
        before = _check(store, sets, targets)

        def untouched():
            after = _check(store, sets, targets)
            assert after[2].tobytes() == before[2].tobytes() and after[0]['mean'].tobytes() == before[0]['mean'].tobytes()
        x, lnl, w = sets[2]
        for e in (-1, 3):
            with pytest.raises(EngineError, match='invalid argument'):
                store.put(e, x, lnl, w)
            untouched()
        big = wc.sample_set(45, 2, 'log-normal', 0)
        with pytest.raises(EngineError, match='invalid argument'):
            store.put(0, *big)
        untouched()
        for bad in (-1e-300, np.nan, np.inf, -np.inf):
            with pytest.raises(EngineError, match='invalid argument'):
                store.put(2, x, lnl, np.where(np.arange(12) == 5, bad, w))
            untouched()
        M = before[0]['total']
        for t in ([[]] * 3, [list(range(1, 18))] * 3, [[0], [1], [1]], [[1], [1], [M[2] + 1]], [[M[0] + 1], [1], [1]]):
            with pytest.raises(EngineError, match='invalid argument'):
                store.order_statistics(t)
            untouched()
        assert np.isnan(store.order_statistics([[1], [2**63], [M[2]]])[1]).all()       # (a set with M = 0 ignores its targets)
        for q in ([], [-0.1], [1.5], np.linspace(0, 1, 17)):
            with pytest.raises(ValueError, match='quantiles'):
                store.weighted_quantiles(q)
        with pytest.raises(ValueError):
            store.put(0, x[:, :1], lnl, w)
        # NULL arguments and sizes, at the C entries themselves
        lib, h = eng.lib, store._handle()
        dptr, u64p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        d = np.zeros(64)
        dp, up, ip = d.ctypes.data_as(dptr), np.ones(3, dtype=np.uint64).ctypes.data_as(u64p), np.zeros(3, dtype=np.int64).ctypes.data_as(i64p)
        out = C.c_void_p()
        for E, n, cap in ((0, 2, 4), (1, 0, 4), (1, 65, 4), (1, 2, -1), (1, 2, 2**31)):
            assert lib.vmx_sample_store_create(eng._h, E, n, cap, C.byref(out)) == -1 and b'invalid argument' in lib.vmx_last_error()
        assert lib.vmx_sample_store_create(None, 1, 1, 1, C.byref(out)) == -1 and lib.vmx_sample_store_create(eng._h, 1, 1, 1, None) == -1
        assert lib.vmx_sample_store_put(None, 0, 1, dp, dp, dp) == -1 and lib.vmx_sample_store_put(h, 0, 1, None, dp, dp) == -1
        assert lib.vmx_sample_store_put(h, 0, 1, dp, None, dp) == -1 and lib.vmx_sample_store_put(h, 0, 1, dp, dp, None) == -1
        assert lib.vmx_sample_store_put(h, 0, -1, dp, dp, dp) == -1
        assert lib.vmx_sample_store_counts(None, ip) == -1 and lib.vmx_sample_store_counts(h, None) == -1
        assert lib.vmx_sample_store_fetch(None, 0, dp, dp, dp) == -1 and lib.vmx_sample_store_fetch(h, 3, dp, dp, dp) == -1
        assert lib.vmx_sample_store_summary(None, dp, dp, dp, dp, up, dp) == -1 and lib.vmx_sample_store_summary(h, dp, dp, dp, dp, None, dp) == -1
        assert lib.vmx_sample_store_summary(h, None, dp, dp, dp, up, dp) == -1 and lib.vmx_sample_store_summary(h, dp, dp, dp, None, up, dp) == -1
        assert lib.vmx_sample_store_order_stats(None, 1, up, dp) == -1 and lib.vmx_sample_store_order_stats(h, 1, None, dp) == -1
        assert lib.vmx_sample_store_order_stats(h, 1, up, None) == -1 and lib.vmx_sample_store_order_stats(h, 0, up, dp) == -1
        assert lib.vmx_sample_store_best(None, dp, ip, None) == -1 and lib.vmx_sample_store_best(h, None, ip, None) == -1
        assert lib.vmx_sample_store_best(h, dp, None, None) == -1 and lib.vmx_sample_store_destroy(None) == -1
        untouched()
        assert lib.vmx_sample_store_best(h, dp, ip, None) == 0 and lib.vmx_sample_store_order_stats(h, 1, up, dp) == 0
        untouched()
    finally:
        store.close()
    with pytest.raises(EngineError, match='closed'):
        store.summary()
    assert np.isfinite(auto_vega.chi2())            # (the engine goes on)


def test_quantiles_of_an_smc_run_are_still_refused(auto_vega):
    """``sample_mocks(sampler='smc', quantiles=...)``: the linear-interpolated quantiles stay the ensemble sampler's."""
    from vega_amd.montecarlo import MonteCarlo
    with pytest.raises(ValueError, match="quantiles go with sampler='ensemble'"):
        MonteCarlo(auto_vega).sample_mocks(sampler='smc', quantiles=Q5, num_mocks=2)
