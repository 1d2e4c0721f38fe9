"""The Q' form's quadratic term over the trapezoidal root of Q' (|| L dx ||^2, L = Qt^T U S DM' by Householder reflectors on the
GPU; the tape stores partial tiles, k_chi2_root squares and adds them) on the small, awkward grids of
tests/helpers/small_grids.py.  (n_masked, nq) per item, k_off = nq - n_masked:

  a65          (65, 65)       k_off = 0; n_masked mod 64 = 1; nq mod 64 odd
  a65_cut      (44, 65)       fewer than 64 rows; k_off = 21, no multiple of 32
  a1296        (959, 1296)    n_masked mod 64 = 63; nq mod 64 = 16, even; k_off = 337
  a1287_bb     (1243, 1299)   additive broadband columns; nq mod 64 = 19; k_off = 56
  j_small_big  (59, 63) + (1312, 1320)   two items on one tape; the second counts its row tiles from a ragged first one (32 rows)

For B in {9, 64, 65, 256}, with the case's data and with a mock pool, an engine made with VMX_QUAD_ROOT=force (the root
whatever the tapes' prices: these grids are too small for it to pay) is held against
  - a fresh engine with VMX_NO_QUAD_ROOT=1 (the half-triangle contraction): 1e-11 S, S = sum |r|^T |C^-1| |r| of run.chi2_ld;
  - chi2 in np.longdouble, with the bars of test_grid_shapes_gpu.py::test_quadratic_forms_against_extended_precision
    (1e-11 S data, 1e-10 S mocks);
  - itself: repeated calls and lanes 1 and 2 bitwise equal; after a rescaled covariance and the original one set again (two
    rebuilds of Q' and L), bitwise equal to what the fresh engine gave.
The factor itself, on the largest of the shapes: || L v ||^2 against v^T Q' v in longdouble for 8 random v, relative error <= 1e-13.
The worst figures are printed (`QUADROOT_RATIOS`; -s shows them)."""
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

import test_grid_shapes_gpu as gs
from helpers import small_grids as sg

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = ['a65', 'a65_cut', 'a1296', 'a1287_bb', 'j_small_big']
BATCHES = (9, 64, 65, 256)
ENV = {'root': ('VMX_QUAD_ROOT', 'force'), 'triangle': ('VMX_NO_QUAD_ROOT', '1')}


@contextmanager
def _env(pair):
    old = {k: os.environ.pop(k, None) for k in ('VMX_QUAD_ROOT', 'VMX_NO_QUAD_ROOT')}
    if pair:
        os.environ[pair[0]] = pair[1]
    try:
        yield
    finally:
        for k in ('VMX_QUAD_ROOT', 'VMX_NO_QUAD_ROOT'):
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class _RootRun(gs._Run):
    """The case with engines 'root' / 'triangle' (kind 'q', 256 walkers) beside the twin; chi2 per (engine, B, data) kept."""

    def vega(self, kind):
        from vega_amd import VegaInterface
        if kind not in self.vegas:
            prob = gs._twin_problem(self.prob) if kind == 'twin' else self.prob
            with _env(ENV.get(kind)):
                v = self.vegas[kind] = VegaInterface(None, problem=prob, max_batch=max(BATCHES), csr_threshold=0.0)
                if kind in ENV:
                    v.engine.set_quadratic_form_kind('q')
                    for name, pool in self.mocks().items():
                        v.engine.set_mock_pool(name, pool)
                    v.engine.eval(self.batch(v.engine, 9)[0])          # (the form is built here, under the engine's own switches)
        return self.vegas[kind]

    def reference_models(self):
        """The four fixture walkers' distorted models in longdouble {item: [4, n_dist]} (row = index into the fixture's theta)."""
        if not hasattr(self, '_models'):
            with_bb = self.case not in gs.NO_BROADBAND
            kind = 'dense' if with_bb else 'twin'
            res = self.evaluate(kind, 4)
            eng = self.vega(kind).engine
            order = np.argsort(res['which'])
            self._models = {}
            for name in self.prob.items:
                rows = res['model'][order][:, eng.model_slices[name]]
                self._models[name] = rows.astype(LD) if with_bb else np.stack([self.yhat(name, r)[0] for r in rows])
        return self._models

    def mocks(self):
        if not hasattr(self, '_mocks'):
            from vega_amd.montecarlo import create_mocks
            ref = self.evaluate('dense', 4)
            eng = gs._Run.vega(self, 'dense').engine
            w0 = int(np.flatnonzero(ref['which'] == 0)[0])
            self._mocks = create_mocks(self.prob, {n: ref['model'][w0, sl] for n, sl in eng.model_slices.items()}, 1, seed=3)
        return self._mocks

    def reference(self, what):
        """(chi2, S) in longdouble per fixture walker, for the data vector or the mock."""
        key = ('ref', what)
        if key not in self.results:
            models, out = self.reference_models(), []
            for w in range(4):
                resid = {}
                for name, item in self.prob.items.items():
                    d = item.masked_data_vec if what == 'data' else self.mocks()[name][0]
                    resid[name] = d.astype(LD) - models[name][w][item.model_mask]
                out.append(self.chi2_ld(resid))
            self.results[key] = out
        return self.results[key]

    def chi2(self, kind, B, what):
        """chi2 [B] of a chi2-only call on engine `kind` ('root' / 'triangle'), the repeat checked bitwise; kept."""
        key = (kind, B, what)
        if key not in self.results:
            eng = self.vega(kind).engine
            theta, _ = self.batch(eng, B)
            eng.set_mock_index(None if what == 'data' else np.zeros(B, dtype=np.int32))
            try:
                got = eng.eval(theta)[0]
                assert eng.last_form() == 'q'
                assert int(eng.debug_read(4, 0, 12)[11]) == (1 if kind == 'root' else 0), (self.case, kind, B)
                np.testing.assert_array_equal(eng.eval(theta)[0], got, err_msg=f'{self.case} {kind} B={B} {what}: a repeated call')
            finally:
                eng.set_mock_index(None)
            self.results[key] = got
        return self.results[key]

    def close(self):
        print('\nQUADROOT_RATIOS', json.dumps({'case': self.case, **{k: float(f'{v:.3g}') for k, v in sorted(self.ratios.items())}}))
        for v in self.vegas.values():
            v.close()
        self.vegas = {}


@pytest.fixture(scope='module')
def run(request, tmp_path_factory):
    r = _RootRun(request.param, tmp_path_factory.mktemp('root_' + request.param))
    yield r
    r.close()


def test_the_cases_cover_the_shapes_the_root_tiles_by():
    facts = {c: [(f['n_masked'], f['nq']) for f in sg.CASES[c][1]] for c in CASES}
    assert facts == {'a65': [(65, 65)], 'a65_cut': [(44, 65)], 'a1296': [(959, 1296)], 'a1287_bb': [(1243, 1299)],
                     'j_small_big': [(59, 63), (1312, 1320)]}
    shapes = [s for c in CASES for s in facts[c]]
    assert any(q == m for m, q in shapes) and any((q - m) % 32 for m, q in shapes) and any(m < 64 for m, q in shapes)
    assert {1, 63} <= {m % 64 for m, q in shapes} and {0, 1} == {q % 64 % 2 for m, q in shapes}
    assert any(sg.tape_row0(m) > 0 for m, q in shapes) and any(item['broadband'] for c in CASES for item in sg.CASES[c][0])


@pytest.mark.parametrize('run', CASES, indirect=True)
def test_root_against_the_triangle_and_extended_precision(run):
    gs._need_extended_precision()
    for what, tol in (('data', 1e-11), ('mock', 1e-10)):
        ref = run.reference(what)
        for B in BATCHES:
            which = run.batch(run.vega('root').engine, B)[1]
            root, tri = run.chi2('root', B, what), run.chi2('triangle', B, what)
            for b in range(B):
                chi2, s = ref[which[b]]
                d_tri, d_ref = abs(LD(root[b]) - LD(tri[b])), abs(LD(root[b]) - chi2)
                run.note(f'{what}/root_minus_triangle_over_S', d_tri / s)
                run.note(f'{what}/root_minus_longdouble_over_S', d_ref / s)
                run.note(f'{what}/triangle_minus_longdouble_over_S', abs(LD(tri[b]) - chi2) / s)
                assert d_tri <= 1e-11 * s, (f'{run.case} {what} B={B} walker {b}: root {root[b]!r}, triangle {tri[b]!r}: '
                                            f'{float(d_tri / s):.2e} S (bar 1e-11 S)')
                assert d_ref <= tol * s, (f'{run.case} {what} B={B} walker {b}: root {root[b]!r} off by {float(d_ref / s):.2e} S '
                                          f'(bar {tol:g} S)')


@pytest.mark.parametrize('run', CASES, indirect=True)
def test_lanes_one_and_two_bitwise_equal(run):
    import torch
    eng = run.vega('root').engine
    for B in BATCHES:
        theta = run.batch(eng, B)[0]
        d_theta = torch.from_numpy(np.ascontiguousarray(theta)).cuda()
        outs = {}
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            try:
                outs[lanes] = [torch.zeros(B, dtype=torch.float64, device='cuda') for _ in range(4)]
                for out in outs[lanes]:
                    eng.eval_device(d_theta.data_ptr(), B, out.data_ptr())
                eng.sync()
            finally:
                eng.set_lanes(1)
        for out in outs[1] + outs[2]:
            assert torch.equal(out, outs[1][0]), (run.case, B)
        np.testing.assert_array_equal(outs[2][1].cpu().numpy(), run.chi2('root', B, 'data'), err_msg=f'{run.case} B={B}: device call against host call')


@pytest.mark.parametrize('run', CASES, indirect=True)
def test_a_rebuild_gives_the_fresh_engine_bit_for_bit(run):
    fresh = {(B, what): run.chi2('root', B, what).copy() for B in BATCHES for what in ('data', 'mock')}
    eng = run.vega('root').engine
    try:
        for name, item in run.prob.items.items():
            eng.set_invcov(name, item.chi2_matrix / 4.0)
        theta = run.batch(eng, 65)[0]
        scaled = eng.eval(theta)[0]
        assert int(eng.debug_read(4, 0, 12)[11]) == 1
        np.testing.assert_allclose(scaled, eng.eval(theta, want_model=True)[0], rtol=1e-9)
        assert not np.array_equal(scaled, fresh[(65, 'data')])
    finally:
        for name, item in run.prob.items.items():
            eng.set_invcov(name, item.chi2_matrix)
    for key in list(run.results):
        if key[0] == 'root':
            del run.results[key]
    for (B, what), want in fresh.items():
        np.testing.assert_array_equal(run.chi2('root', B, what), want, err_msg=f'{run.case} B={B} {what}: after two rebuilds')


@pytest.mark.parametrize('run', ['a1287_bb'], indirect=True)
def test_the_factor_reproduces_the_quadratic_form(run):
    gs._need_extended_precision()
    eng = run.vega('root').engine
    eng.eval(run.batch(eng, 9)[0])
    (nm, nq), = [(f['n_masked'], f['nq']) for f in sg.CASES[run.case][1]]
    ld = (nq + 31) // 32 * 32
    L = eng.debug_read(20, 0, nm * ld).reshape(nm, ld)[:, :nq]
    H = eng.debug_read(21, 0, nq * ld).reshape(nq, ld)[:, :nq]
    # the trapezoid: L[i][j] = 0 for j > i + (nq - nm), exactly
    assert not np.triu(L, nq - nm + 1).any() and not np.triu(H, 1).any()
    Ll, Hl = L.astype(LD), H.astype(LD)
    rng = np.random.default_rng(11)
    for _ in range(8):
        v = rng.standard_normal(nq).astype(LD)
        y = Ll @ v
        quad, root = 2 * (v @ (Hl @ v)), y @ y            # (half form: L' below the diagonal, half the diagonal on it)
        rel = abs(root - quad) / quad
        run.note('factor/rel', rel)
        assert rel <= 1e-13, f'|| L v ||^2 = {float(root)!r}, v^T Q\' v = {float(quad)!r}: relative {float(rel):.2e}'
