"""The metal terms on small, awkward grids (tests/helpers/small_grids.py: METAL_CASES, 63 to 1320 model bins) against the
reference's fixture and against extended precision.

`new_metals = True` gives every metal pair a real matrix on any grid, as a Kronecker product A [n_rp^2] (x) B [n_rt^2] (or A
alone with `rp_only_metal_mats`); the rest of the suite applies such matrices at 2500 and 5000 bins only, where n_rp and n_rt
are multiples of the five outputs a thread of k_metal_kron owns, and plans the sums on the way (xi_sum_plan) for one layout in
which no pair has a matrix.  Here every case runs at B = 1 (three calls), 5, 9 and 70 - the fixture's four parameter rows,
tiled - on three engines: 'kron' (the default), 'dense' (kron_metals = False: the same matrices uploaded whole) and 'nosums'
('kron' built under VMX_NO_XI_SUMS: every pipeline keeps its own array):

  (a) chi2 (1e-6) and models (1e-8 of scale, rtol 1e-8 on the fitted bins) of the unmodified reference
      (tests/golden/expected_small_metals.npz), chi2-only and with a model, every engine, every B;
  (b) every metal-matrix product (vmx_debug_read 3) against M . xi in np.longdouble, xi being the pair's own bins
      (vmx_debug_read 1) of the SAME evaluation, for EVERY element, u = 2^-53:
          dense      |err| <= (K + 2) u |M| |xi|, K = n_model - an fp64 sum of K products in any order, + the result's rounding;
          Kronecker  |err| <= (n_rt + n_rp + 4) u |A| (|Xi| |B|^T) - two chains of n_rt and n_rp fused multiply-adds, + one rounding
                     of every entry of M = A (x) B, which the reference product uses;
          rp-only    |err| <= (n_rp + 2) u |A| |Xi|;
      an element whose bound is 0 is an exact 0 (a pair whose lines fall off a short grid has an all-zero matrix), and at
      most half of all (pair, element) entries have a zero bound.  Kronecker and dense products differ by at most the sum
      of their bounds.  Up to 8 walkers the engines as built keep the per-pipeline bins ('kron', 'dense' serve B = 1, 5);
      above, the production engines sum plain pipelines on the way and vmx_debug_read 1 refuses, so B = 9 and 70 are taken
      from the engines built under VMX_NO_XI_SUMS ('nosums', 'dense_nosums'): k_metal_kron and the grouped products are the
      same kernels there (mx1320 alone has nothing to sum - its core pipelines are not lean - and is served as built at every B);
  (c) the sums on the way against arrays kept: the assembled vector (vmx_debug_read 5; at B = 1 the model of an identity-
      distortion twin) of 'kron' against 'nosums', per element |diff| <= (2 T + 8) u sum_t |term_t|, T = the item's terms
      (smooth, peak, every pair), the magnitudes from the CPU oracle's saved components - each engine adds T terms in its
      own order, T roundings of the products and T of the sums each at the most.  A dropped, doubled or mis-factored
      member moves an element by a whole term;
  (d) chi2 of the quadratic form (vmx_debug_read 4 [8] says it ran) and of the full chain against r^T C^-1 r in longdouble
      with the engine's own model: 1e-11 S with the case's data, 1e-10 S with a mock at the fiducial model,
      S = sum |r|^T |C^-1| |r| (the bars of tests/test_grid_shapes_gpu.py (d));
  (e) one answer however the walkers are batched (chi2 1e-10, models 1e-11 of scale), repeated calls bitwise equal.

Two Problem-level variants of m63 run (a) against the CPU oracle (held to the reference on m63 in
tests/test_small_grids_host.py), then (c) and (e): m63_mixed (two main x metal pairs without matrix: plain, groupable pairs
next to matrix pairs in one item) and m63_fast (fast_metals = True, chi2 at the fiducial point first: static vectors, shared
pipelines, static groups).

Each case's claimed facts are asserted before anything runs on the device.  The largest error / bound per case and check is
printed (`METALGRID_RATIOS` lines, one per case; -s shows them).
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
LD = np.longdouble
BASE_CASES = list(sg.METAL_CASES)
ALL_CASES = BASE_CASES + list(sg.METAL_VARIANTS)
ENGINES = ('kron', 'dense', 'nosums')


def _assert_xi(got, ref, mask, what):       # (tests/test_csr_gpu.py)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-8 * scale, what
    np.testing.assert_allclose(got[mask], ref[mask], rtol=1e-8, atol=1e-12 * scale, err_msg=what)


def _twin_problem(prob):
    """The same problem with identity distortion matrices (no case here has a broadband): its model is the assembled
    pre-distortion vector - an identity product is exact."""
    twin = copy.copy(prob)
    twin.items = {}
    for name, item in prob.items.items():
        t = copy.copy(item)
        assert not item.broadband and item.dist_grid.size == item.model_grid.size
        t.distortion = np.eye(item.model_grid.size)
        twin.items[name] = t
    return twin


def _csr_dot_ld(csr, x):
    """(M x, |M| |x|) in longdouble for a scipy CSR matrix (a dense longdouble copy of fifteen 1296^2 matrices is 400 MB)."""
    csr = csr.tocsr()
    rows = np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))
    prod = csr.data.astype(LD) * x.astype(LD)[csr.indices]
    y, y_abs = np.zeros(csr.shape[0], dtype=LD), np.zeros(csr.shape[0], dtype=LD)
    np.add.at(y, rows, prod)
    np.add.at(y_abs, rows, np.abs(prod))
    return y, y_abs


class _Run:
    """One case or variant: the problem (facts checked), the reference rows, engines made on demand, results per (engine, B)."""

    def __init__(self, case, tmp):
        from oracle import vega_cpu as oc
        self.case = case
        self.variant = case in sg.METAL_VARIANTS
        base = sg.METAL_VARIANTS.get(case, case)
        sg.check_claims()
        self.base_prob = sg.build_case(tmp, base, GOLDEN)
        sg.check_facts(base, self.base_prob)                # before anything touches the device
        self.facts = sg.METAL_CASES[base][1]
        self.prob = sg.metal_variant(self.base_prob, case) if self.variant else self.base_prob
        with np.load(GOLDEN / 'expected_small_metals.npz') as z:
            self.exp = {k[len(base) + 1:]: z[k] for k in z.files if k.startswith(base + '/')}
        self.names = [str(n) for n in self.exp['param_names']]
        if case == 'm63_fast':
            # main x metal pairs with equal betas share one pipeline from the first evaluation on (the reference's per-call
            # cache): the unsampled metal betas keep their configured values in every row
            theta = self.exp['theta'].copy()
            main = {t for item in self.prob.items.values() for t in (item.tracer1.name, item.tracer2.name)}
            for j, n in enumerate(self.names):
                if n.startswith('beta_') and n[5:] not in main and n != 'beta_hcd':
                    theta[:, j] = theta[0, j]
            self.exp['theta'] = theta
        # the oracle: the variants' reference, and the magnitudes of the terms for (c)
        oc.reset_metal_cache(self.prob)
        if case == 'm63_fast':
            oc.chi2(self.prob)                              # the reference's first evaluation freezes the metal x metal terms
        self.term_abs = {name: [] for name in self.prob.items}
        self.n_terms = {name: 2 + len(item.metals) for name, item in self.prob.items.items()}
        chi2, models = [], {name: [] for name in self.prob.items}
        for row in self.exp['theta']:
            pars = dict(zip(self.names, row))
            taps = {}
            model = oc.compute_model(self.prob, pars, taps=taps)
            lp = oc.local_params(self.prob, pars)
            for name, item in self.prob.items.items():
                models[name].append(np.asarray(model[name]))
                self.term_abs[name].append(self._term_magnitudes(oc, item, lp, taps[name]))
            if self.variant:
                chi2.append(oc.chi2(self.prob, pars))
        if self.variant:
            self.exp['chi2'] = np.array(chi2)
            for name in self.prob.items:
                self.exp[f'model/{name}'] = np.array(models[name])
        self.vegas, self.results, self.ratios, self._cache = {}, {}, {}, {}
        self.served = {}
        self.cinv = {n: np.asarray(it.chi2_matrix, dtype=LD) for n, it in self.prob.items.items()}
        self.cinv_abs = {n: np.abs(c) for n, c in self.cinv.items()}

    def _term_magnitudes(self, oc, item, lp, taps):
        """sum_t |term_t| per bin: |bao_amp xi_peak| + |xi_smooth| + sum over pairs |bias product x xi_pair| (fp64 is ample)."""
        total = np.abs(lp['bao_amp'] * taps['peak']['xi_core']) + np.abs(taps['smooth']['xi_core'])
        local = dict(lp)
        if item.metal_opts['fast_metals'] and 'growth_rate' in local and self.prob.growth_rate is not None:
            local['growth_rate'] = self.prob.growth_rate
        assert list(taps['xi_metal']) == [p.names for p in item.metals] and not item.metal_opts['single_metal_beta']
        for pair in item.metals:
            b1, _, b2, _ = oc.bias_beta(local, *pair.names)
            xi = taps['xi_metal'][pair.names]
            total = total + np.abs(b1 * b2 * xi if item.metal_opts['fast_metal_bias'] else xi)
        return total

    def vega(self, kind):
        """'kron' | 'dense' | 'nosums' | 'dense_nosums' | 'twin' | 'twin_nosums'."""
        from vega_amd import VegaInterface
        if kind not in self.vegas:
            prob = _twin_problem(self.prob) if kind.startswith('twin') else self.prob
            mp = pytest.MonkeyPatch()
            if kind.endswith('nosums'):
                mp.setenv('VMX_NO_XI_SUMS', '1')
            try:
                v = VegaInterface(None, problem=prob, max_batch=max(BATCHES), kron_metals=not kind.startswith('dense'), csr_threshold=0.0)
                if self.case == 'm63_fast':
                    n_before = v.engine.n_pipelines
                    v.chi2()                                # chi2 at the fiducial point first: the engine is rebuilt with the frozen terms
                    assert v.engine.n_pipelines < n_before
            finally:
                mp.undo()
            assert v.engine.csr_items == []
            self.vegas[kind] = v
        return self.vegas[kind]

    def batch(self, eng, B):
        base = np.stack([eng.theta_from_params(dict(zip(self.names, row))) for row in self.exp['theta']])
        which = (np.arange(B) + 1) % base.shape[0]          # (B = 1 is a walker away from the form's expansion point)
        return base[which], which

    def evaluate(self, kind, B):
        key = (kind, B)
        if key in self.results:
            return self.results[key]
        vega = self.vega(kind)
        eng = vega.engine
        theta, which = self.batch(eng, B)
        vega._check_pinned(theta)
        res = {'which': which}
        res['quad'] = [eng.eval(theta)[0] for _ in range(3 if B == 1 else 2)]
        res['form'] = eng.last_form()
        res['full'], res['status'], res['model'] = eng.eval(theta, want_model=True)
        res['form_full'] = eng.last_form()
        res.update(self.taps(eng, B))
        res['full_again'], _, res['model_again'] = eng.eval(theta, want_model=True)
        self.results[key] = res
        return res

    def taps(self, eng, B):
        """Of the last model request: 'vec' {item: [B, n]} the assembled vector (vmx_debug_read 5; None for a single walker,
        whose fused distortion product keeps none), and for the cases 'xi' / 'xim' {(item, pair): [B, n]} - the bins of every
        pair with a matrix (1) and its product (3); 'xi' is None where the engine summed its plain pipelines on the way."""
        from vega_amd.engine import EngineError
        sizes = {name: it.model_grid.size for name, it in self.prob.items.items()}
        cap = B * max((n + 31) // 32 * 32 for n in sizes.values())
        vec = {}
        for q, (name, n) in enumerate(sizes.items()):
            try:
                vec[name] = eng.debug_read(5, q, cap).reshape(B, -1)[:, :n].copy()
            except EngineError:
                assert B == 1
                vec = None
                break
        out = {'vec': vec}
        if self.variant:
            return out
        xi, xim = {}, {}
        for (name, mi), (g, pid, has_matrix) in eng.metal_source.items():
            assert has_matrix and pid >= 0                  # the facts: every pair of every case has a matrix
            n = sizes[name]
            xim[(name, mi)] = eng.debug_read(3, g, cap).reshape(B, -1)[:, :n].copy()
            if xi is not None:
                try:
                    xi[(name, mi)] = eng.debug_read(1, pid, cap).reshape(B, -1)[:, :n].copy()
                except EngineError:
                    assert B > 8 and not xi
                    xi = None
        assert len(xim) == sum(f['n_pairs'] for f in self.facts)
        out.update(xi=xi, xim=xim)
        return out

    def product_ld(self, name, mi, x):
        """(M x, |M| |x| from M, the engine-form magnitude) in longdouble for pair ``mi`` of item ``name``; the last is
        |A| (|Xi| |B|^T) or |A| |Xi| from the Kronecker factors.  Kept per vector (a batch repeats four walkers)."""
        key = (name, mi, x.tobytes())
        if key not in self._cache:
            pair = self.prob.items[name].metals[mi]
            y, y_abs = _csr_dot_ld(pair.matrix, x)
            a, b = pair.kron
            xi2 = np.abs(x.astype(LD)).reshape(a.shape[0], -1)
            t = xi2 if b is None else xi2 @ np.abs(b.astype(LD)).T
            self._cache[key] = (y, y_abs, (np.abs(a.astype(LD)) @ t).ravel())
        return self._cache[key]

    def chi2_ld(self, residuals):
        """(sum_items r^T C^-1 r, sum_items |r|^T |C^-1| |r|) in longdouble; residuals: {item: r}."""
        chi2, s = LD(0), LD(0)
        for name, r in residuals.items():
            key = ('chi2', name, r.view(np.uint8).reshape(r.size, -1)[:, :10].tobytes())       # (the 80 bits that count)
            if key not in self._cache:
                self._cache[key] = (r @ (self.cinv[name] @ r), np.abs(r) @ (self.cinv_abs[name] @ np.abs(r)))
            chi2, s = chi2 + self._cache[key][0], s + self._cache[key][1]
        return chi2, s

    def note(self, what, ratio):
        self.ratios[what] = max(self.ratios.get(what, 0.0), float(ratio))

    def close(self):
        print('\nMETALGRID_RATIOS', json.dumps({'case': self.case, **{k: float(f'{v:.3g}') for k, v in sorted(self.ratios.items())},
                                               'b_served_by': {str(k): v for k, v in sorted(self.served.items())}}))
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


@pytest.mark.parametrize('kind', ENGINES)
@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_chi2_and_models_of_the_reference(run, kind):
    """(a)  The cases against the unmodified reference's fixture, the two variants against the CPU oracle."""
    eng = run.vega(kind).engine
    assert eng.quadratic_form
    for B in BATCHES:
        res = run.evaluate(kind, B)
        which = res['which']
        assert not res['status'].any()
        assert res['form'] in ('q', 'factored') and res['form_full'] == 'full', (run.case, kind, B, res['form'], res['form_full'])
        ref = run.exp['chi2'][which]
        for i, quad in enumerate(res['quad']):
            np.testing.assert_allclose(quad, ref, rtol=CHI2_RTOL, err_msg=f'{run.case} {kind} B={B} chi2-only call {i}')
        np.testing.assert_allclose(res['full'], ref, rtol=CHI2_RTOL, err_msg=f'{run.case} {kind} B={B} full chain')
        run.note(f'a/{kind}/chi2_rel', max(np.abs(res['full'] / ref - 1).max(), max(np.abs(q / ref - 1).max() for q in res['quad'])))
        for name, sl in eng.model_slices.items():
            ref_m = run.exp[f'model/{name}']
            for b in range(B):
                _assert_xi(res['model'][b, sl], ref_m[which[b]], run.prob.items[name].model_mask,
                           f'{run.case} {kind} B={B} walker {b} {name}')
            run.note(f'a/{kind}/model_of_scale', np.abs(res['model'][:, sl] - ref_m[which]).max() / np.abs(ref_m).max())


@pytest.mark.parametrize('run', BASE_CASES, indirect=True)
def test_metal_products_against_extended_precision(run):
    """(b)  B = 1 and 5 from 'kron' and 'dense' as built, B = 9 and 70 from 'nosums' and 'dense_nosums' (see the module text);
    which engine served which B is asserted here and printed with the ratios."""
    _need_extended_precision()
    for B in BATCHES:
        kron, dense = run.evaluate('kron', B), run.evaluate('dense', B)
        served = ('kron', 'dense')
        if kron['xi'] is None:
            assert dense['xi'] is None and B > 8
            served = ('nosums', 'dense_nosums')
            for b in BATCHES[:BATCHES.index(B)]:            # (the same sequence of calls on both engines)
                run.evaluate('dense_nosums', b)
            kron, dense = run.evaluate('nosums', B), run.evaluate('dense_nosums', B)
            assert not dense['status'].any() and not kron['status'].any()
        assert B > 8 or served == ('kron', 'dense')        # (an item whose core pipelines are not lean has nothing to sum on the way)
        run.served[B] = '+'.join(served)
        assert kron['xi'] is not None and dense['xi'] is not None and sorted(kron['xi']) == sorted(kron['xim']) == sorted(dense['xim'])
        n_entries = n_zero = 0
        for (name, mi), xi in sorted(kron['xi'].items()):
            item = run.prob.items[name]
            a, b = item.metals[mi].kron
            n_rp, n_rt, k = a.shape[0], item.model_grid.size // a.shape[0], item.model_grid.size
            np.testing.assert_array_equal(dense['xi'][(name, mi)], xi, err_msg=f'{run.case} B={B} {name} pair {mi}: the two engines disagree on xi')
            for w in range(B):
                y, m_abs, kron_abs = run.product_ld(name, mi, xi[w])
                bounds = {'dense': (k + 2) * U * m_abs,
                          'kron': ((n_rp + 2) if b is None else (n_rt + n_rp + 4)) * U * kron_abs}
                got = {'dense': dense['xim'][(name, mi)][w], 'kron': kron['xim'][(name, mi)][w]}
                for form in ('dense', 'kron'):
                    err, bound = np.abs(got[form].astype(LD) - y), bounds[form]
                    worst = int(np.argmax(err - bound))
                    assert np.all(err <= bound), (f'{run.case} {form} B={B} walker {w} {name} pair {mi} {item.metals[mi].names}: bin {worst} '
                                                  f'off by {float(err[worst]):.3e}, bound {float(bound[worst]):.3e}')
                    zero = bound == 0
                    assert np.all(got[form][zero] == 0.0), f'{run.case} {form} B={B} walker {w} {name} pair {mi}: a zero row gave a non-zero'
                    if np.any(~zero):
                        run.note(f'b/{form}', (err[~zero] / bound[~zero]).max())
                    if form == 'kron':
                        n_entries += k
                        n_zero += int(zero.sum())
                both = bounds['dense'] + bounds['kron']
                diff = np.abs(got['dense'].astype(LD) - got['kron'].astype(LD))
                assert np.all(diff <= both), f'{run.case} B={B} walker {w} {name} pair {mi}: Kronecker and dense products differ by {float(diff.max()):.3e}'
                if np.any(both > 0):
                    run.note('b/kron_vs_dense', (diff[both > 0] / both[both > 0]).max())
        assert 2 * n_zero <= n_entries, (run.case, B, n_zero, n_entries)
        run.note('b/zero_bound_fraction', n_zero / n_entries)


@pytest.mark.parametrize('run', ALL_CASES, indirect=True)
def test_sums_on_the_way_against_arrays_kept(run):
    """(c)  Measured on one MI355X (largest |diff| / bound): 0 at B = 1 and 5 everywhere (nothing is summed on the way up to 8
    walkers), for mx1320 at every B (its core pipelines are not lean, so nothing is summed there) and for the cross item of mj
    (none of its pipelines is summed); 0.047 to 0.249 at B = 9 and 70 for every auto item and both variants.  This check found
    a dependence on layout: beside an item that sums, a lean pipeline that keeps its array used to run through
    k_xi_bins_group as a group of one, which rounds apart from k_xi_bins_lean; the last bits then passed through the metal
    matrices and mj's cross item missed the bound (ratio 1.18).  Such pipelines now take k_xi_bins_lean (xi_sum_plan:
    lean_single)."""
    _need_extended_precision()
    for B in BATCHES:
        prod, kept = run.evaluate('kron', B), run.evaluate('nosums', B)
        if prod['vec'] is None:
            assert B == 1 and kept['vec'] is None
            tw = {kind: run.evaluate(kind, B) for kind in ('twin', 'twin_nosums')}
            assert not tw['twin']['status'].any() and not tw['twin_nosums']['status'].any()
            vec = {kind: {name: r['model'][:, run.vega(kind).engine.model_slices[name]] for name in run.prob.items} for kind, r in tw.items()}
            prod_vec, kept_vec = vec['twin'], vec['twin_nosums']
        else:
            prod_vec, kept_vec = prod['vec'], kept['vec']
        for name in run.prob.items:
            t = run.n_terms[name]
            for w in range(B):
                bound = (2 * t + 8) * U * run.term_abs[name][prod['which'][w]].astype(LD)
                diff = np.abs(prod_vec[name][w].astype(LD) - kept_vec[name][w].astype(LD))
                worst = int(np.argmax(diff - bound))
                assert np.all(bound > 0)
                run.note('c', (diff / bound).max())
                run.note(f'c/{name}/B{B}', (diff / bound).max())
                assert np.all(diff <= bound), (f'{run.case} B={B} walker {w} {name}: bin {worst} differs by {float(diff[worst]):.3e}, '
                                               f'bound {float(bound[worst]):.3e}')


@pytest.mark.parametrize('run', BASE_CASES, indirect=True)
def test_chi2_against_extended_precision(run):
    """(d)"""
    _need_extended_precision()
    from vega_amd.montecarlo import create_mocks
    eng = run.vega('kron').engine
    fid = run.evaluate('kron', 5)
    w0 = int(np.flatnonzero(fid['which'] == 0)[0])
    mocks = create_mocks(run.prob, {n: fid['model'][w0, sl] for n, sl in eng.model_slices.items()}, 1, seed=3)
    n_data = sum(it.data_size for it in run.prob.items.values())
    try:
        for name, pool in mocks.items():
            eng.set_mock_pool(name, pool)
        for B in BATCHES:
            theta, which = run.batch(eng, B)
            for data, tol in ((None, 1e-11), (mocks, 1e-10)):
                what = 'data' if data is None else 'mock'
                eng.set_mock_index(None if data is None else np.zeros(B, dtype=np.int32))
                quad = eng.eval(theta)[0]
                assert eng.last_form() in ('q', 'factored'), (run.case, B, eng.last_form())
                np.testing.assert_array_equal(eng.eval(theta)[0], quad)
                full, status, model = eng.eval(theta, want_model=True)
                assert eng.last_form() == 'full' and not status.any()
                for b in range(B):
                    resid = {}
                    for name, item in run.prob.items.items():
                        d = item.masked_data_vec if data is None else data[name][0]
                        resid[name] = d.astype(LD) - model[b, eng.model_slices[name]][item.model_mask].astype(LD)
                    chi2, s = run.chi2_ld(resid)
                    for form, got in (('quad', quad[b]), ('full', full[b])):
                        err = abs(LD(got) - chi2)
                        assert err <= tol * s, (f'{run.case} {form} {what} B={B} walker {b}: chi2 {got!r} off by {float(err):.3e} = '
                                                f'{float(err / s):.2e} S (bar {tol:g} S)')
                        run.note(f'd/{form}/{what}/err_over_S', err / s)
                    if data is not None and which[b] == 0:
                        # the minimiser's regime: a mock at its own model has chi2 ~ n_masked (ten standard deviations of room)
                        assert quad[b] < n_data + 10 * np.sqrt(2 * n_data)
    finally:
        eng.set_mock_index(None)


@pytest.mark.parametrize('kind', ENGINES)
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
