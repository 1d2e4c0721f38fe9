"""The chi2 chain on small, awkward grids (tests/helpers/small_grids.py: 63 to 5184 model bins) against the reference's
fixture and against extended precision.

The products after xi - distortion product, C^-1 product or covariance tape, the Q' tape with its contraction epilogue, the
factored form, the streaming and CSR kernels - tile by problem size; the rest of the suite runs them at 2500, 5000 and 10000
bins only.  Here every case is built from files in the reference's layout on its own grid and run at B = 1 (three times:
level-2 tables, host-side sum), 5 (streaming kernels), 9 (one ragged walker tile) and 70 (two walker tiles, the second ragged),
the walkers being the fixture's four, tiled:

  (a) chi2 (1e-6) and models (1e-8 of scale, rtol 1e-8 on the masked bins) of the unmodified reference
      (tests/golden/expected_small_grids.npz), dense and CSR engine, chi2-only and with a model;
  (b) the distortion product against y = DM . xi in np.longdouble, xi being the model of a twin engine with identity
      distortion matrices (shown bitwise equal to the engine's own xi first, on the stage taps of vmx_debug_read): |model - y| <= (K + 16) u |DM| |xi| for EVERY
      element, u = 2^-53, K = n_model - the a-priori bound of an fp64 sum of K products in any order plus 16 roundings for
      the post stage.  A dropped or doubled K stage, row or tile edge moves a result by ~1/K of |DM| |xi|: ten orders above;
  (c) chi2 of the full chain against r^T C^-1 r in longdouble with the engine's own model: |chi2 - ref| <=
      (2 max n_masked + 8) u S, S = sum |r|^T |C^-1| |r| - as is (covariance tape above 8 walkers, C^-1 products + k_chi2
      below) and with VMX_NO_CINV_TAPE (the triangular k_gemm_nt at B = 9 and 70);
  (d) both quadratic forms ('q', 'factored') against chi2 in longdouble from the twin's xi, with the case's data vector
      (1e-11 S) and with a mock at the fiducial model (chi2 ~ n_masked; 1e-10 S) - the bars of tests/test_quadratic_form_gpu.py,
      taken relative to S so that a small chi2 on a 63-bin grid does not turn rounding into a failure;
  (e) one answer however the walkers are batched (chi2 1e-10, models 1e-11 of scale), repeated calls bitwise equal.

Each case's claimed facts (sizes, remainders, tape_row0, tile counts) are asserted before anything runs on the device.
The largest error / bound per case and check is printed (`SMALLGRID_RATIOS` lines, one per set-up of a case; -s shows them).
"""
import copy
import json

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import small_grids as sg

pytestmark = pytest.mark.gpu

CHI2_RTOL = 1e-6
BATCHES = (1, 5, 9, 70)
U = 2.0**-53
QUAD_DATA_BAR, QUAD_MOCK_BAR = 1e-11, 1e-10         # (d): of S, with the case's data vector and with a mock
LD = np.longdouble
ALL_CASES = list(sg.CASES)
NO_BROADBAND = [c for c in ALL_CASES if not any(item['broadband'] for item in sg.CASES[c][0])]


def _assert_xi(got, ref, mask, what):       # (tests/test_csr_gpu.py)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-8 * scale, what
    np.testing.assert_allclose(got[mask], ref[mask], rtol=1e-8, atol=1e-12 * scale, err_msg=what)


def _twin_problem(prob):
    """The same problem with identity distortion matrices and no broadband: its model is the pre-distortion vector xi (an
    identity product and an empty post stage are exact).  With COEFMOD 2 the model then lives on the model grid; chi2 of the
    twin means nothing and is not looked at."""
    twin = copy.copy(prob)
    twin.items = {}
    for name, item in prob.items.items():
        t = copy.copy(item)
        n = item.model_grid.size
        t.distortion = np.eye(n)
        t.broadband = []
        if item.dist_grid.size != n:
            t.dist_grid = item.model_grid
            t.model_mask = np.arange(n) < item.data_size
        twin.items[name] = t
    return twin


class _Run:
    """One case: the problem (facts checked), the fixture's walkers, engines made on demand, results kept per (engine, B)."""

    def __init__(self, case, tmp):
        self.case = case
        sg.check_claims()
        self.prob = sg.build_case(tmp, case, GOLDEN)
        sg.check_facts(case, self.prob)                 # before anything touches the device
        with np.load(GOLDEN / 'expected_small_grids.npz') as z:
            self.exp = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + '/')}
        self.vegas, self.results, self.ratios, self._yhat = {}, {}, {}, {}
        self.n_masked_max = max(item.data_size for item in self.prob.items.values())
        self.cinv = {n: np.asarray(it.chi2_matrix, dtype=LD) for n, it in self.prob.items.items()}
        self.cinv_abs = {n: np.abs(c) for n, c in self.cinv.items()}

    def vega(self, kind):
        from vega_amd import VegaInterface
        if kind not in self.vegas:
            prob = _twin_problem(self.prob) if kind == 'twin' else self.prob
            threshold = 1.1 if kind == 'csr' else 0.0
            v = self.vegas[kind] = VegaInterface(None, problem=prob, max_batch=max(BATCHES), csr_threshold=threshold)
            assert v.engine.csr_items == (list(prob.items) if kind == 'csr' else [])
        return self.vegas[kind]

    def batch(self, eng, B):
        names = [str(n) for n in self.exp['param_names']]
        base = np.stack([eng.theta_from_params(dict(zip(names, row))) for row in self.exp['theta']])
        which = (np.arange(B) + 1) % base.shape[0]          # (B = 1 is a walker away from the form's expansion point)
        return base[which], which

    def evaluate(self, kind, B, vega=None, key=None):
        key = (key or kind, B)
        if key in self.results:
            return self.results[key]
        eng = (vega or self.vega(kind)).engine
        theta, which = self.batch(eng, B)
        res = {'which': which}
        # (the twin takes the same sequence of calls: a single walker's P(k,mu) stage moves to its level-2 tables with them)
        res['quad'] = [eng.eval(theta)[0] for _ in range(3 if B == 1 else 2)]
        res['full'], res['status'], res['model'] = eng.eval(theta, want_model=True)
        res['taps'] = self.taps(eng, B)
        res['full_again'], _, res['model_again'] = eng.eval(theta, want_model=True)
        self.results[key] = res
        return res

    def taps(self, eng, B):
        """xi of the last model request as the engine holds it: the per-pipeline bins (what = 1; batches above 8 walkers sum
        them on the way and keep none) and the assembled vector the distortion product read (what = 5; a single walker's
        fused product keeps none).  {tap: array}: at least one of the two exists for every batch size."""
        from vega_amd.engine import EngineError
        sizes = [it.model_grid.size for it in self.prob.items.values()]
        cap = B * max((n + 31) // 32 * 32 for n in sizes)
        out = {}
        if B <= 8:
            for p in range(eng.n_pipelines):
                out[f'pipeline {p}'] = eng.debug_read(1, p, cap).copy()
        for q, n in enumerate(sizes):
            try:
                out[f'item {q}'] = eng.debug_read(5, q, cap).reshape(B, -1)[:, :n].copy()
            except EngineError:
                assert B == 1
        assert out
        return out

    def dense_matrix(self, name):
        dm = self.prob.items[name].distortion
        return np.asarray(dm.toarray() if hasattr(dm, 'toarray') else dm, dtype=float)

    def yhat(self, name, xi_row):
        """(DM xi, |DM| |xi|) in longdouble for one fp64 vector xi, kept per vector (a batch repeats four walkers)."""
        key = (name, xi_row.tobytes())
        if key not in self._yhat:
            if name not in self._yhat:
                dm = self.dense_matrix(name).astype(LD)
                self._yhat[name] = (dm, np.abs(dm))
            dm, dm_abs = self._yhat[name]
            x = xi_row.astype(LD)
            self._yhat[key] = (dm @ x, dm_abs @ np.abs(x))
        return self._yhat[key]

    def chi2_ld(self, residuals):
        """(sum_items r^T C^-1 r, sum_items |r|^T |C^-1| |r|) in longdouble; residuals: {item: r}."""
        chi2, s = LD(0), LD(0)
        for name, r in residuals.items():
            key = ('chi2', name, r.view(np.uint8).reshape(r.size, -1)[:, :10].tobytes())       # (the 80 bits that count)
            if key not in self._yhat:
                self._yhat[key] = (r @ (self.cinv[name] @ r), np.abs(r) @ (self.cinv_abs[name] @ np.abs(r)))
            chi2, s = chi2 + self._yhat[key][0], s + self._yhat[key][1]
        return chi2, s

    def note(self, what, ratio):
        self.ratios[what] = max(self.ratios.get(what, 0.0), float(ratio))

    def close(self):
        print('\nSMALLGRID_RATIOS', json.dumps({'case': self.case, **{k: float(f'{v:.3g}') for k, v in sorted(self.ratios.items())}}))
        for v in self.vegas.values():
            v.close()
        self.vegas = {}


@pytest.fixture(scope='module')
def run(request, tmp_path_factory):
    r = _Run(request.param, tmp_path_factory.mktemp(request.param))
    yield r
    r.close()


def _need_extended_precision():
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference')


def _classes(eng, theta, want_model):
    eng.set_profiling(True)
    eng.timings(reset=True)
    eng.eval(theta, want_model=want_model)
    t = eng.timings(reset=True)
    eng.set_profiling(False)
    return {k: v[1] for k, v in t.items()}


@pytest.mark.parametrize('kind', ['dense', 'csr'])
@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_chi2_and_models_of_the_reference(run, kind):
    """(a)"""
    eng = run.vega(kind).engine
    assert eng.quadratic_form
    for B in BATCHES:
        res = run.evaluate(kind, B)
        which = res['which']
        assert not res['status'].any()
        ref = run.exp['chi2'][which]
        for i, quad in enumerate(res['quad']):
            np.testing.assert_allclose(quad, ref, rtol=CHI2_RTOL, err_msg=f'{run.case} {kind} B={B} chi2-only call {i}')
        np.testing.assert_allclose(res['full'], ref, rtol=CHI2_RTOL, err_msg=f'{run.case} {kind} B={B} full chain')
        run.note(f'a/{kind}/chi2_rel', max(np.abs(res['full'] / ref - 1).max(), max(np.abs(q / ref - 1).max() for q in res['quad'])))
        for b in range(B):
            for name, sl in eng.model_slices.items():
                _assert_xi(res['model'][b, sl], run.exp[f'model/{name}'][which[b]], run.prob.items[name].model_mask,
                           f'{run.case} {kind} B={B} walker {b} {name}')
        # which kernel classes ran: chi2-only is the quadratic form alone, a model request the full chain
        theta, _ = run.batch(eng, B)
        n = _classes(eng, theta, False)
        assert n['quadratic_form_product'] > 0 and n['distortion_product'] == 0 and n['invcov_product'] == 0, (run.case, kind, B, n)
        n = _classes(eng, theta, True)
        assert n['quadratic_form_product'] == 0 and n['distortion_product'] > 0 and n['invcov_product'] > 0, (run.case, kind, B, n)


@pytest.mark.parametrize('kind', ['dense', 'csr'])
@pytest.mark.parametrize('run', NO_BROADBAND, indirect=True)
def test_distortion_product_against_extended_precision(run, kind):
    """(b)"""
    _need_extended_precision()
    eng, twin = run.vega(kind).engine, run.vega('twin').engine
    assert eng.n_pipelines == twin.n_pipelines
    for B in BATCHES:
        res, tw = run.evaluate(kind, B), run.evaluate('twin', B)
        assert not tw['status'].any()
        shared = sorted(set(res['taps']) & set(tw['taps']))
        assert shared and (B > 8 or len(shared) >= eng.n_pipelines), (B, sorted(res['taps']), sorted(tw['taps']))
        for tap in shared:
            np.testing.assert_array_equal(res['taps'][tap], tw['taps'][tap], err_msg=f'{run.case} {kind} B={B}: xi of {tap} differs from the twin')
        for name, item in run.prob.items.items():
            k = item.model_grid.size
            xi, model = tw['model'][:, twin.model_slices[name]], res['model'][:, eng.model_slices[name]]
            assert xi.shape == (B, k) and model.shape == (B, item.dist_grid.size)
            for b in range(B):
                y, y_abs = run.yhat(name, xi[b])
                err, bound = np.abs(model[b].astype(LD) - y), (k + 16) * U * y_abs
                worst = int(np.argmax(err - bound))
                assert np.all(err <= bound), (f'{run.case} {kind} B={B} walker {b} {name}: bin {worst} off by {float(err[worst]):.3e}, '
                                              f'bound {float(bound[worst]):.3e}')
                run.note(f'b/{kind}', (err / bound).max())


@pytest.mark.parametrize('tape', [True, False], ids=['as is', 'VMX_NO_CINV_TAPE'])
@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_full_chain_chi2_against_extended_precision(run, tape, monkeypatch):
    """(c)"""
    _need_extended_precision()
    vega = None
    if not tape:
        from vega_amd import VegaInterface
        monkeypatch.setenv('VMX_NO_CINV_TAPE', '1')
        vega = VegaInterface(None, problem=run.prob, max_batch=max(BATCHES), csr_threshold=0.0)
    try:
        for B in BATCHES:
            res = run.evaluate('dense', B, vega=vega, key='dense' if tape else 'dense_products')
            assert not res['status'].any()
            eng = (vega or run.vega('dense')).engine
            rows, inverse = np.unique(res['model'], axis=0, return_inverse=True)
            ref = []
            for m in rows:
                ref.append(run.chi2_ld({name: item.masked_data_vec.astype(LD) - m[eng.model_slices[name]][item.model_mask].astype(LD)
                                        for name, item in run.prob.items.items()}))
            for b in range(B):
                chi2, s = ref[int(np.ravel(inverse)[b])]
                bound = (2 * run.n_masked_max + 8) * U * s
                err = abs(LD(res['full'][b]) - chi2)
                assert err <= bound, f'{run.case} B={B} walker {b}: chi2 off by {float(err):.3e}, bound {float(bound):.3e}'
                run.note('c/tape' if tape else 'c/products', err / bound)
    finally:
        if vega is not None:
            vega.close()


@pytest.mark.parametrize('form', ['q', 'factored'])
@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_quadratic_forms_against_extended_precision(run, form):
    """(d)  With the post-distortion broadband (a1287_bb) the twin has no broadband to add: there the distorted model of
    the reference residual is the engine's own full-chain model, which (a) and (c) hold."""
    _need_extended_precision()
    from vega_amd.montecarlo import create_mocks
    vega = run.vega('dense')
    eng = vega.engine
    with_bb = run.case not in NO_BROADBAND
    fid = run.evaluate('dense', 5)
    w0 = int(np.flatnonzero(fid['which'] == 0)[0])
    mocks = create_mocks(run.prob, {n: fid['model'][w0, sl] for n, sl in eng.model_slices.items()}, 1, seed=3)
    eng.set_quadratic_form_kind(form)
    try:
        for name, pool in mocks.items():
            eng.set_mock_pool(name, pool)
        for B in BATCHES:
            theta, which = run.batch(eng, B)
            res = run.evaluate('dense', B)
            if not with_bb:
                tw = run.evaluate('twin', B)
                twin = run.vega('twin').engine
            for data, tol in ((None, QUAD_DATA_BAR), (mocks, QUAD_MOCK_BAR)):
                eng.set_mock_index(None if data is None else np.zeros(B, dtype=np.int32))
                got = eng.eval(theta)[0]
                assert eng.last_form() == form
                n = _classes(eng, theta, False)
                assert n['quadratic_form_product'] > 0 and n['distortion_product'] == 0 and n['invcov_product'] == 0, (run.case, form, B, n)
                np.testing.assert_array_equal(eng.eval(theta)[0], got)
                for b in range(B):
                    resid = {}
                    for name, item in run.prob.items.items():
                        if with_bb:
                            y = res['model'][b, eng.model_slices[name]].astype(LD)
                        else:
                            y = run.yhat(name, tw['model'][b, twin.model_slices[name]])[0]
                        d = item.masked_data_vec if data is None else data[name][0]
                        resid[name] = d.astype(LD) - y[item.model_mask]
                    chi2, s = run.chi2_ld(resid)
                    err = abs(LD(got[b]) - chi2)
                    what = 'data' if data is None else 'mock'
                    assert err <= tol * s, (f'{run.case} {form} {what} B={B} walker {b}: chi2 {got[b]!r} off by {float(err):.3e} = '
                                            f'{float(err / s):.2e} S (bar {tol:g} S)')
                    run.note(f'd/{form}/{what}/err_over_S', err / s)
                    if data is not None and which[b] == 0:
                        # the minimiser's regime: a mock at its own model has chi2 ~ n_masked (ten standard deviations of room)
                        n_data = sum(it.data_size for it in run.prob.items.values())
                        assert got[b] < n_data + 10 * np.sqrt(2 * n_data)
    finally:
        eng.set_mock_index(None)
        eng.set_quadratic_form_kind('auto')


@pytest.mark.parametrize('kind', ['dense', 'csr'])
@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_one_answer_regardless_of_batching(run, kind):
    """(e)"""
    big = run.evaluate(kind, max(BATCHES))
    scale = np.abs(big['model']).max()
    first = {w: int(np.flatnonzero(big['which'] == w)[0]) for w in range(4)}
    for B in BATCHES:
        res = run.evaluate(kind, B)
        at = np.array([first[w] for w in res['which']])
        np.testing.assert_allclose(res['full'], big['full'][at], rtol=1e-10, err_msg=f'{run.case} {kind} B={B} full chain')
        np.testing.assert_allclose(res['quad'][-1], big['quad'][-1][at], rtol=1e-10, err_msg=f'{run.case} {kind} B={B} chi2-only')
        assert np.abs(res['model'] - big['model'][at]).max() <= 1e-11 * scale, (run.case, kind, B)
        np.testing.assert_array_equal(res['quad'][-1], res['quad'][-2])
        np.testing.assert_array_equal(res['full_again'], res['full'])
        np.testing.assert_array_equal(res['model_again'], res['model'])
        run.note(f'e/{kind}/chi2_rel', np.abs(res['full'] / big['full'][at] - 1).max())
        run.note(f'e/{kind}/model_of_scale', np.abs(res['model'] - big['model'][at]).max() / scale)
