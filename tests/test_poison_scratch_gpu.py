"""Every device-resident driver under poisoned scratch (include/vegamx.h: vmx_debug_poison_scratch; vega_amd/engine.py:
poison_scratch).  With the switch on, device scratch of plain doubles that a call takes without clearing it - DevBuf::alloc(count,
false) and every ensure(), whether or not it reallocates - reads as NaN, so a kernel that reads what no writer of the call covered
shows it in the call's outputs.  On a fresh process such memory usually reads as zeros, and the rest of the suite cannot see it.

The problem is `a63` of tests/helpers/small_grids.py (one auto-correlation, n_masked = 59: 27 of the 64 padded columns are
padding), two sampled parameters.  The scheme of every case: three fresh engines take the identical sequence of calls; engines 1
and 2 run with the switch off and must agree bit for bit in every output (the control: a walker's path depends on what the
engine's tables hold from earlier calls, so only identical histories compare), engine 3 runs with the switch on and must agree
bit for bit with engine 1, every output that is finite there finite here.  Every sequence holds a larger run followed by a
smaller one on the same engine - more fits, walkers, live points, particles first - so that the smaller run is served from
buffers ensure() did not reallocate: under poison they then stand for the stale contents of the larger run.

The counts are the smallest at which every kernel of a driver launches and the second run's extents are smaller than the first's;
they are named below.  The quadratic form's per-mock terms are also held to r^T C^-1 r in np.longdouble at the bar
tests/test_grid_shapes_gpu.py uses for a mock.
"""
import copy

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import small_grids as sg
from test_grid_shapes_gpu import QUAD_MOCK_BAR

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAMES = ['bias_eta_LYA', 'beta_LYA']
LIMITS = {'bias_eta_LYA': (-0.5, 0.0), 'beta_LYA': (0.5, 3.0)}
ERRORS = {'bias_eta_LYA': 0.01, 'beta_LYA': 0.05}
MAX_BATCH = 64
# fits: on the data (starts spread about the configured values), on pool rows the walkers bring, on streamed mocks
DATA_FITS = (5, 2)
ROW_FITS = (12, 5)                  # (12 mocks through the host matvec entry: more than 8 vectors, the split-K slabs of mv_part)
STREAMED = ((20, 8), (6, 4))        # (mocks, wave): three waves of 8, 8, 4, then two of 4, 2 in buffers sized for waves of 8
FACTORED = ((8, 8), (3, 4))         # r5184, the factored form
# samplers
W, W_SMALL = 8, 6                   # walkers (the snooker move needs three partners in the other half: W >= 6)
E, E_SMALL = 3, 2                   # ensembles / runs of a set
STEPS = 20
TEMPS = 3                           # rungs of a ladder (the adaptive ladder needs three)
LIVE, LIVE_SMALL, THREADS, REPEATS, ITERATIONS = 24, 16, 4, 3, 4
PARTICLES, PARTICLES_SMALL, SWEEPS, STAGES = 48, 32, 3, 4
MIXTURE = [('stretch', 0.4), ('de', 0.3), ('snooker', 0.3)]
COV_MIXTURE = [('stretch', 0.3), ('de', 0.2), ('snooker', 0.2), ('cov', 0.3)]


@pytest.fixture(scope='module')
def a63(tmp_path_factory):
    sg.check_claims()
    prob = sg.build_case(tmp_path_factory.mktemp('a63'), 'a63', GOLDEN)
    sg.check_facts('a63', prob)
    assert [it.data_size % 32 for it in prob.items.values()] == [27]
    return prob


def _sample_params(prob):
    return {'limits': dict(LIMITS), 'values': {n: prob.params[n] for n in NAMES}, 'errors': dict(ERRORS),
            'fix': {n: False for n in NAMES}}


def _three(prob, sequence, max_batch=MAX_BATCH):
    """The outputs of `sequence(vega)` on three fresh engines: switch off, off, on."""
    from vega_amd import VegaInterface
    from vega_amd.engine import poison_scratch
    outs = []
    for k in range(3):
        vega = VegaInterface(None, problem=prob, max_batch=max_batch)
        try:
            with poison_scratch(k == 2):
                outs.append(sequence(vega))
        finally:
            vega.close()
    return outs


def _leaves(obj, path=''):
    """(path, array) of everything numeric in a nest of dicts, lists, tuples, arrays and numbers; host timings left out."""
    if obj is None:
        return
    if isinstance(obj, dict):
        for key in sorted(obj, key=str):
            if 'seconds' in str(key):
                continue
            yield from _leaves(obj[key], f'{path}/{key}')
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _leaves(v, f'{path}[{i}]')
    elif isinstance(obj, str):
        yield path, np.frombuffer(obj.encode(), dtype=np.uint8)
    else:
        yield path, np.ascontiguousarray(obj)


def _assert_same(a, b, what):
    la, lb = list(_leaves(a)), list(_leaves(b))
    assert [p for p, _ in la] == [p for p, _ in lb], what
    assert la, what
    for (path, x), (_, y) in zip(la, lb):
        assert x.shape == y.shape and x.dtype == y.dtype, f'{what}: {path}'
        if x.dtype.kind == 'f':
            lost = np.isfinite(x) & ~np.isfinite(y)
            assert not lost.any(), f'{what}: {path} has {int(lost.sum())} of {x.size} finite entries not finite'
        assert x.tobytes() == y.tobytes(), f'{what}: {path} differs in {int(np.sum(x != y))} of {x.size} entries'


def _check(outs):
    _assert_same(outs[0], outs[1], 'control (engines 1 and 2, both unpoisoned)')
    _assert_same(outs[0], outs[2], 'poisoned scratch (engine 3 against engine 1)')


def _fit_out(res):
    out = {k: getattr(res, k) for k in ('values', 'errors', 'covariance', 'fval', 'edm', 'is_valid', 'hesse_failed', 'nfcn', 'n_iter')}
    assert np.isfinite(out['fval']).all()           # (on engine 1: what engine 3 must keep)
    return out


def _monte_carlo(vega):
    from vega_amd.montecarlo import MonteCarlo
    vega.freeze_metals()
    mc = MonteCarlo(vega)
    mc.driver, mc.stream_mocks = 'device', True
    vega.analysis = mc
    return mc


def _streamed(mc, fid, sp, runs, seed=3):
    out = []
    for k, (n, wave) in enumerate(runs):
        res = mc._fit_streamed_mocks(fid, n, seed=seed + k, sample_params=sp, wave=wave)
        st = mc.driver_stats
        assert st['fits_unfinished'] == 0 and st['evaluations'] == int(res.nfcn.sum())
        out.append(dict(fit=_fit_out(res), mocks=dict(mc.mc_mocks)))
    return out


# ---------------------------------------------------------------------------------------------------------- vmx_fit_migrad
def test_fits_on_the_data_and_on_rows_the_walkers_bring(a63):
    """W.theta / W.chi2 / the result arrays of FitWorkspace, and - through `create_mocks` with 12 mocks - mv_part, the split-K
    slabs of the host matvec entry (vmx_matmul_host with more than 8 vectors)."""
    sp = _sample_params(a63)

    def sequence(vega):
        mc = _monte_carlo(vega)
        fitter = mc.minimizer(sp)
        start0 = np.array([sp['values'][n] for n in NAMES])
        out = {}
        for F in DATA_FITS:
            start = start0[None, :] * (1 + 0.03 * np.arange(F))[:, None]
            out[f'data {F}'] = _fit_out(fitter.minimize(n_fits=F, start=start, fixed=mc._fixed))
        fid = vega.compute_model()
        for k, n in enumerate(ROW_FITS):
            mocks = mc.create_mocks(fid, n, seed=5 + k)
            out[f'rows {n}'] = dict(mocks=dict(mocks), fit=_fit_out(mc._fit_mocks(mocks, n, sample_params=sp)))
        # the entry itself: 12 and then 9 vectors through the slabs, against the host product
        item = next(iter(a63.items.values()))
        A = np.linalg.cholesky(item.cov[:, item.data_mask][item.data_mask, :])
        for B in (12, 9):
            X = np.random.RandomState(B).randn(B, A.shape[1])
            Y = vega.engine.matmul_host(A, X)
            np.testing.assert_allclose(Y, X @ A.T, rtol=0, atol=1e-13 * np.abs(A).sum(axis=1).max() * np.abs(X).max())
            out[f'matmul {B}'] = Y
        return out

    _check(_three(a63, sequence))


@pytest.mark.parametrize('chain', ['q', 'full'])
def test_streamed_mocks_with_an_inverse_covariance(a63, chain, monkeypatch):
    """The mock stream of vmx_fit_migrad (mc_z, mc_noise, mc_r0, mc_t; waves that do not divide the mocks) with the item's C^-1:
    the Q' form - q_lin by the W product, q_c0 by the C^-1 product and k_rowdot, all over n_masked_pad columns of mc_r0 - and
    the full chain (VMX_NO_QUAD, the knob of tests/test_knobs_gpu.py: k_mock_rows alone, the pools)."""
    if chain == 'full':
        monkeypatch.setenv('VMX_NO_QUAD', '1')
    sp = _sample_params(a63)

    def sequence(vega):
        mc = _monte_carlo(vega)
        eng = vega.engine
        if chain == 'q':
            eng.set_quadratic_form_kind('q')
        out = _streamed(mc, vega.compute_model(), sp, STREAMED)
        eng.eval(np.tile(eng.low.theta0, (2, 1)))
        assert eng.last_form() == chain
        return out

    _check(_three(a63, sequence))


@pytest.mark.parametrize('chain', ['q', 'full'])
def test_streamed_mocks_without_an_inverse_covariance(a63, chain, monkeypatch):
    """The third branch: an item without a covariance has the identity for C^-1, and the constants of its mocks are
    k_rowdot(mc_r0, mc_r0).  The interface draws no mocks without a covariance, so the factor (that of the case's covariance),
    the draws and the stream go to the engine as MonteCarlo._fit_streamed_mocks sends them."""
    if chain == 'full':
        monkeypatch.setenv('VMX_NO_QUAD', '1')
    sp = _sample_params(a63)
    (name, item), = a63.items.items()
    factor = np.linalg.cholesky(item.cov[:, item.data_mask][item.data_mask, :])
    plain = copy.copy(a63)
    plain.items = {name: copy.copy(item)}
    plain.items[name].set_covariance(None)

    def sequence(vega):
        from vega_amd.montecarlo import _fiducial_on_data_grid
        mc = _monte_carlo(vega)
        eng = vega.engine
        if chain == 'q':
            eng.set_quadratic_form_kind('q')
        fid = _fiducial_on_data_grid(item, vega.compute_model()[name])[item.data_mask]
        eng.set_mock_factor(name, factor, fid)
        out = []
        for k, (n, wave) in enumerate(STREAMED):
            draws = eng.pinned_empty((n, item.data_size))
            draws[:] = np.random.RandomState(7 + k).randn(n, item.data_size)
            fitter = mc.minimizer(sp)
            mc._mock_rows = np.arange(n, dtype=np.int32)
            mc._mock_stream = dict(draws=draws, counter=np.array([n], dtype=np.int32), wave=wave, timeout=300.)
            try:
                res = fitter.minimize(n_fits=n, fixed=mc._fixed)
            finally:
                mc._mock_rows = mc._mock_stream = None
            assert mc.driver_stats['fits_unfinished'] == 0
            pool = eng.get_mock_pool(name, n)
            scale = np.abs(fid).max() + np.abs(factor).sum(axis=1).max() * np.abs(draws).max()
            np.testing.assert_allclose(pool, fid[None, :] + draws @ factor.T, rtol=0, atol=1e-13 * scale)
            keep = {k2: getattr(res, k2) for k2 in ('values', 'errors', 'covariance', 'fval', 'edm', 'is_valid', 'hesse_failed', 'nfcn', 'n_iter')}
            assert np.isfinite(keep['fval']).all()
            out.append(dict(fit=keep, pool=pool))
        eng.eval(np.tile(eng.low.theta0, (2, 1)))
        assert eng.last_form() == chain
        return out

    _check(_three(plain, sequence))


def test_streamed_mocks_with_the_factored_form(tmp_path_factory):
    """The first branch: `r5184` (n_masked = 1256, 1256 % 32 = 8: 24 padded columns), the factored form: u0 = U r0 over
    n_masked_pad columns of mc_r0.  8 mocks, then 3 in waves of 4."""
    prob = sg.build_case(tmp_path_factory.mktemp('r5184'), 'r5184', GOLDEN)
    sg.check_facts('r5184', prob)
    assert [it.data_size % 32 for it in prob.items.values()] == [8]
    sp = _sample_params(prob)

    def sequence(vega):
        mc = _monte_carlo(vega)
        eng = vega.engine
        eng.set_quadratic_form_kind('factored')
        out = _streamed(mc, vega.compute_model(), sp, FACTORED)
        eng.eval(np.tile(eng.low.theta0, (2, 1)))
        assert eng.last_form() == 'factored'
        return out

    _check(_three(prob, sequence))


def test_per_mock_terms_of_the_quadratic_form_against_extended_precision(a63):
    """After a streamed run the linear terms and constants of every mock were made on the device from mc_r0.  chi2 of the
    quadratic form with those rows (chi2_batch_device, the mocks' rows) at every mock's best fit and at the fiducial row against
    (mock - S m)^T C^-1 (mock - S m) in np.longdouble, mock the pool row as the device holds it and m the engine's own full-chain
    model of the same row (held to its own oracles by tests/test_grid_shapes_gpu.py): |chi2 - ref| <= QUAD_MOCK_BAR S, S = |r|^T
    |C^-1| |r| - the bar of test_quadratic_forms_against_extended_precision for a mock.  Under poison, where a read of the pad
    columns cannot hide."""
    if np.finfo(LD).nmant < 63:
        pytest.skip('np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference')
    import torch
    from vega_amd import VegaInterface
    from vega_amd.engine import poison_scratch
    sp = _sample_params(a63)
    (name, item), = a63.items.items()
    cinv = np.asarray(item.chi2_matrix, dtype=LD)
    vega = VegaInterface(None, problem=a63, max_batch=MAX_BATCH)
    try:
        with poison_scratch():
            mc = _monte_carlo(vega)
            eng = vega.engine
            eng.set_quadratic_form_kind('q')
            n, wave = STREAMED[0]
            res = mc._fit_streamed_mocks(vega.compute_model(), n, seed=3, sample_params=sp, wave=wave)
            pool = eng.get_mock_pool(name, n)
            cols = [eng.low.slot[p] for p in NAMES]
            theta = np.tile(eng.low.theta0, (2 * n, 1))
            theta[:n, cols] = res.values                  # every mock's best fit; rows n .. 2 n - 1: the fiducial row
            rows = np.tile(np.arange(n, dtype=np.int32), 2)
            dev = torch.device('cuda', 0)
            got = vega.chi2_batch_device(torch.from_numpy(theta).to(dev), mock_rows=torch.from_numpy(rows).to(dev)).cpu().numpy()
            assert eng.last_form() == 'q'
            model = eng.eval(theta, want_model=True)[2][:, eng.model_slices[name]][:, item.model_mask]
        worst = 0.0
        for b in range(2 * n):
            r = pool[rows[b]].astype(LD) - model[b].astype(LD)
            ref, s = r @ (cinv @ r), np.abs(r) @ (np.abs(cinv) @ np.abs(r))
            err = abs(LD(got[b]) - ref)
            print(f'POISON_QUAD row {b} mock {rows[b]} chi2 {got[b]!r} err/S {float(err / s):.3e}')
            assert np.isfinite(got[b]) and err <= QUAD_MOCK_BAR * s, (b, got[b], float(ref), float(err / s))
            worst = max(worst, float(err / s))
        assert worst < QUAD_MOCK_BAR
    finally:
        vega.close()


def test_a_new_covariance_reaches_the_streamed_mocks(a63):
    """set_covariance drops the cached Cholesky factors: after a covariance scaled by 4 the streamed driver sends the new factor
    (the engine's copy is keyed on the cache's entry) and its mocks are fiducial + cholesky(4 C) . draws, stated here without
    the cache, at the bar of tests/test_fit_device_gpu.py::test_mocks_made_while_their_fits_run - the same sequence as the host
    test of tests/test_round2_host.py."""
    from vega_amd import VegaInterface
    from vega_amd.montecarlo import _fiducial_on_data_grid
    sp = _sample_params(a63)
    prob = copy.copy(a63)
    (name, item), = a63.items.items()
    prob.items = {name: copy.copy(item)}
    mine = prob.items[name]
    mine.__dict__.pop('_cholesky', None)
    masked = item.cov[:, item.data_mask][item.data_mask, :]
    vega = VegaInterface(None, problem=prob, max_batch=MAX_BATCH)
    try:
        mc = _monte_carlo(vega)
        fid = vega.compute_model()
        fid_masked = _fiducial_on_data_grid(item, fid[name])[item.data_mask]
        n, wave = STREAMED[1]
        got = []
        for factor in (1.0, 4.0):
            if factor != 1.0:
                mine.set_covariance(factor * item.cov)
            mc._fit_streamed_mocks(fid, n, seed=9, sample_params=sp, wave=wave)
            got.append(mc.mc_mocks[name].copy())
            np.random.seed(9)
            draws = np.random.randn(n * item.data_size).reshape(n, item.data_size)
            want = fid_masked[None, :] + draws @ np.linalg.cholesky(factor * masked).T
            np.testing.assert_allclose(got[-1], want, rtol=0, atol=1e-13 * np.abs(want).max(), err_msg=f'covariance x {factor}')
        noise = [g - fid_masked[None, :] for g in got]
        np.testing.assert_allclose(noise[1], 2.0 * noise[0], rtol=0, atol=4e-13 * np.abs(got[0]).max())
        assert np.abs(noise[0]).max() > 1e3 * 4e-13 * np.abs(got[0]).max()          # (the factor of two is far above the bar)
    finally:
        vega.close()


# ---------------------------------------------------------------------------------------------------------- the samplers
def _box(prob):
    sp = _sample_params(prob)
    sp.pop('fix')
    return sp


def _with_pool(vega, n=6):
    from vega_amd.montecarlo import MonteCarlo
    vega.freeze_metals()
    mocks = MonteCarlo(vega).create_mocks(vega.compute_model(), n, seed=1)
    for name, pool in mocks.items():
        vega.engine.set_mock_pool(name, pool)


def _ensemble_out(s):
    out = dict(chain=s.get_chain(), lnl=s.get_log_lik(), accepted=s.accepted, x=s.x, last_lnl=s.lnl, stats={k: v for k, v in s.stats.items()
                                                                                                                  if isinstance(v, (int, float, np.ndarray))})
    for key in ('per_ensemble', 'swaps', 'current_betas', 'cov_fallbacks', 'mu', 'slice_counts'):
        if getattr(s, key, None) is not None:
            out[key] = getattr(s, key)
    if getattr(s, 'adapt', False):
        out['beta_history'] = s.beta_history
    assert np.isfinite(out['chain']).all() and np.isfinite(out['lnl']).all()
    return out


ENSEMBLE_KINDS = ['stretch', 'mixture', 'tempered', 'adaptive', 'cov', 'slice', 'mock rows', 'chain store']


@pytest.mark.parametrize('kind', ENSEMBLE_KINDS)
def test_ensembles(a63, kind):
    """vmx_ensemble_run(_many, _many_moves, _pt, _pt_adapt, _many_cov, _slice), the stand-alone factor stage
    (vmx_ensemble_cov_factor: alloc(.., false)), and a run with an attached chain store and its device summary (chain_alloc)."""
    box = _box(a63)

    def sequence(vega):
        from vega_amd import EnsembleSampler, EnsembleSet, TemperedEnsemble
        out = []
        for big in (True, False):
            w, e = (W, E) if big else (W_SMALL, E_SMALL)
            kw = dict(seed=7, sample_params=box, driver='device')
            if kind == 'stretch':
                s = EnsembleSampler(vega, w, **kw).run(STEPS)
            elif kind == 'mixture':
                s = EnsembleSet(vega, e, w, moves=MIXTURE, **kw).run(STEPS)
            elif kind == 'tempered':
                s = TemperedEnsemble(vega, w, ntemps=TEMPS, ladders=e - 1, swap_every=2, moves=MIXTURE, **kw).run(STEPS)
            elif kind == 'adaptive':
                s = TemperedEnsemble(vega, w, ntemps=TEMPS, ladders=e - 1, swap_every=1, adapt=True, adaptation_lag=5, adaptation_time=3,
                                     **kw).run(STEPS, start='prior')
            elif kind == 'cov':
                s = EnsembleSet(vega, e, w, moves=COV_MIXTURE, cov_scale=1.5, **kw).run(STEPS)
                half = np.random.RandomState(2).rand(e, w // 2, 2)
                out.append(dict(zip(('mean', 'factor', 'flag'), vega.engine.ensemble_cov_factor(half))))
            elif kind == 'slice':
                s = EnsembleSet(vega, e, w, moves='slice', tune_steps=6, **kw).run(STEPS)
            elif kind == 'mock rows':
                if big:
                    _with_pool(vega)
                s = EnsembleSet(vega, e, w, mock_rows=list(range(e)), **kw).run(STEPS)
            else:
                s = EnsembleSet(vega, e, w, chain='device', thin=2, **kw).run(STEPS)
                assert s.driver == 'device'
                out.append(s.summary(discard=2))
                s.run(STEPS // 2)
                out.append(s.summary(discard=4))
            assert s.driver == 'device'
            out.append(_ensemble_out(s))
            s.close()
        return out

    _check(_three(a63, sequence))


def _nested_out(s):
    out = dict(dead=s.dead(), live_u=s.live_u, live_lnl=s.live_lnl, iteration=s.iteration, log_z=s.log_evidence())
    if s.phantom_state is not None:
        out['phantoms'] = s.phantoms()
    if s.cluster_state is not None:
        out['cluster_ids'] = s.cluster_ids()
    return out


@pytest.mark.parametrize('kind', ['plain', 'clustered', 'phantoms', 'clustered phantoms', 'set', 'set phantoms'])
def test_nested_runs(a63, kind):
    """vmx_nested_run, _clustered (with the stand-alone clustering's workspace: vmx_nested_cluster_points), _phantoms,
    vmx_nested_run_many and _many_phantoms (with mock rows)."""
    box = _box(a63)

    def sequence(vega):
        from vega_amd import NestedSampler, NestedSet
        from vega_amd.engine import cluster_points
        out = []
        for big in (True, False):
            live, e = (LIVE, E) if big else (LIVE_SMALL, E_SMALL)
            kw = dict(num_live=live, threads=THREADS, num_repeats=REPEATS, seed=5, sample_params=box, driver='device')
            if kind.startswith('set'):
                if big:
                    _with_pool(vega)
                s = NestedSet(vega, e, mock_rows=list(range(e)), **(dict(boost_posterior=2) if 'phantoms' in kind else {}), **kw)
                s.run(ITERATIONS)
                assert s.driver == 'device'
                out.append([_nested_out(run) for run in s.runs] + [s.status])
                continue
            extra = {}
            if 'clustered' in kind:
                extra['clustering'] = True
            if 'phantoms' in kind:
                extra['boost_posterior'] = 2
            s = NestedSampler(vega, **extra, **kw).run(iterations=ITERATIONS)
            assert s.driver == 'device'
            out.append(_nested_out(s))
            if kind == 'clustered':
                pts = np.random.RandomState(live).rand(live, 2)
                out.append(cluster_points(pts, np.zeros(live, dtype=np.int32), 1))
        return out

    _check(_three(a63, sequence))


def _smc_out(s):
    return dict(u=s.u, lnl=s.lnl, stage=s.stage, beta=s.beta, scale=s.scale, record=s.record, rounds=s.posterior_rounds,
                status=getattr(s, 'status', None), log_z=s.log_evidence())


@pytest.mark.parametrize('kind', ['single', 'set', 'kept', 'kept set'])
def test_smc_runs(a63, kind):
    """vmx_smc_run, _many (with mock rows), _kept and _many_kept (the kept stages: rec_u, posterior rounds)."""
    box = _box(a63)

    def sequence(vega):
        from vega_amd import SMCSampler, SMCSet
        out = []
        for big in (True, False):
            N, e = (PARTICLES, E) if big else (PARTICLES_SMALL, E_SMALL)
            kw = dict(particles=N, sweeps=SWEEPS, seed=5, sample_params=box, driver='device')
            if 'kept' in kind:
                kw.update(n_total=2 * N, recycle=True)
            if 'set' in kind:
                if big:
                    _with_pool(vega)
                s = SMCSet(vega, e, mock_rows=list(range(e)), **kw)
            else:
                s = SMCSampler(vega, **kw)
            s.run() if 'kept' in kind else s.run(stages=STAGES)
            assert s.driver == 'device'
            out.append(_smc_out(s))
            if 'kept' in kind:
                out.append(s.samples())
        return out

    _check(_three(a63, sequence))
