"""The spline-bins kernels against the extended-precision oracle of tests/helpers/xi_bins_oracle.py, bin by bin, under its
a-priori bound (no bin excluded), on the small, awkward grids of tests/helpers/small_grids.py: a63 (less than one 256-thread
block), a1287 (five blocks + 7), j_small_big (63 and 1320 bins in one launch sized by the larger; the cross-correlation
carries delta_rp and the radiation term), and option cases on them (xi_bins_oracle.CASES: radiation on rescaled coordinates,
Croom + power evolution, split evolution, UV shot noise 1 and 2, relativistic + asymmetry odd multipoles, single_ell,
n_ell 2, 3, 4, fht_lowring = False, an additive template with pre- and post-distortion broadband), and the static-basis forms on
the metal cases.

Walkers: the fiducial point and three seeded ones that move ap, at and delta_rp, tiled to B = 1, 5, 9 and 70 (odd counts for
the two-walker kernels).  Every form is reached as run_chain chooses it, and the route mask (vmx_debug_read 4 [9]) is asserted
against what the planner's rules give for the case - on the first, second and third call, the replayed graph included:

  model request, B <= 8                          k_xi_bins<false>                      engine 'default'
  model request, B > 8                           k_xi_bins_group (both components lean), k_xi_bins_lean (a lean pipeline that keeps its
                                                 array), k_xi_bins<false> (the rest)   engine 'default'
  model request, B > 8, VMX_NO_XI_SUMS           k_xi_bins_lean (+ k_xi_bins<false>)    engine 'nosums'
  model request, B > 8, VMX_NO_XI_LEAN           k_xi_bins<false>                      engine 'nolean'
  chi2-only, B <= 8                              k_xi_assemble_quad (both branches)    engine 'default'
  chi2-only, B > 8                               k_xi_quad_plain, or k_xi_assemble_quad where an item is no lean pair or carries an
                                                 additive template or a pre-distortion broadband (a63_bb: all three, and twelve
                                                 post-distortion broadband coefficients behind the model bins)

Per case and form: (a) the route; (b) every bin of every pipeline (vmx_debug_read 1), every entry of x' - x0' (10) and every
group sum (14) within the oracle's bound, the oracle fed the same evaluation's coefficients (2), scalars (6) and static arrays
(8); r = 0 bins and padding exactly 0; (c) the scalars against the parameters; (d) a walker's row bit for bit the same at every
position of the batch (the tiling puts every walker into both slots of a two-walker thread) and at B = 9 and B = 11, where
the coefficient product hands the bins the same bits (asserted: at least one row per form is compared bit for bit; on one MI355X
all are); at B = 9 and B = 70 the product tiles differently and its coefficients differ in the window the bins read, so a row is
compared bit for bit where its operands are equal and otherwise held to the two bounds plus the oracle's own difference; (e) different forms within the sum of their bounds; (f) status 0, and
VMX_STATUS_BOUNDS for exactly the one walker whose alphas carry r' below the first knot, from every form.

The static-basis forms (test_static_basis_forms): k_poly_bins at set-up (vmx_debug_read 12 against the spline and Legendre sums of
the basis coefficients, 15), k_xi_bins_static (B <= 8), k_xi_bins_static_nw<4> (B > 8 under VMX_NO_XI_SUMS: B mod 4 = 1 and 2),
k_xi_bins<true> (VMX_NO_STATIC_BINS) and the sums of k_xi_bins_static_group<2> (19; factor kind 2 from vmx_debug_read 17).

They run on the metal cases m63, m63_mixed, m63_fast and mj (xi_bins_oracle.STATIC_CASES), whose per-walker pipelines and lean
groups are held to the oracle in the same evaluations; these forms read no per-walker coefficient, so their rows are asserted
equal at every batch size.

The largest error / bound per case and form is printed (`XIBINS_RATIOS` lines; -s shows them).
"""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import xi_bins_oracle as xo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = xo.U
BATCHES = (1, 5, 9, 70)
ENV = {'default': None, 'nosums': 'VMX_NO_XI_SUMS', 'nolean': 'VMX_NO_XI_LEAN'}
STATUS_BOUNDS = 1


def _lean(d):
    """vmx_finalize's rule for k_xi_bins_lean."""
    return d.evol == (0, 0) and not d.additive and d.single_ell < 0 and (not d.radiation or not d.is_peak)


def expected_route(descs, B, mode, same_grid, kind, pre_terms=()):
    """The bins kernels run_chain launches for items [(peak Desc, smooth Desc)] without metal terms; pre_terms: per item, whether
    it carries an additive template or a pre-distortion broadband (xi_plain_args: such an item stays with k_xi_assemble_quad)."""
    bits = {'same_grid'} if same_grid else set()
    if mode == 'quad':
        std = [all(d.evol == (0, 0) and not d.additive for d in pair) for pair in descs]
        lean_pair = [s and all(d.single_ell < 0 for d in pair) for s, pair in zip(std, descs)]
        plain = [s and not any(d.radiation for d in pair) for s, pair in zip(std, descs)]
        if B > 8 and all(lean_pair) and not any(pre_terms):
            return bits | {'quad_plain'}
        return bits | {'assemble_quad'} | (set() if all(plain) else {'assemble_quad_general'})
    if B <= 8 or kind == 'nolean':
        return bits | {'general'}
    for pair in descs:
        lean = [d for d in pair if _lean(d)]
        if len(lean) < len(pair):
            bits.add('general')
        if len(lean) == 2 and kind == 'default':
            bits.add('group')
        elif lean:
            bits.add('lean')
    return bits


class _Run:
    def __init__(self, case, tmp, build=xo.build_case, env=ENV, **vega_options):
        self.case, self.env, self.vega_options = case, env, vega_options
        self.prob = build(tmp, case, GOLDEN)                        # (claims checked before anything touches the device)
        self.rows = xo.walker_params(self.prob)
        self.vegas, self.results, self.ratios, self.ulps, self._oracle = {}, {}, {}, {}, {}

    def vega(self, kind):
        from vega_amd import VegaInterface
        if kind not in self.vegas:
            mp = pytest.MonkeyPatch()
            for name in (self.env[kind] or '').split():
                mp.setenv(name, '1')
            try:
                v = VegaInterface(None, problem=self.prob, max_batch=max(BATCHES), **self.vega_options)
                if self.case == 'm63_fast':
                    v.chi2()                    # chi2 at the fiducial point first: the engine is rebuilt with the frozen terms
            finally:
                mp.undo()
            self.vegas[kind] = v
        return self.vegas[kind]

    def static(self, kind):
        """Per pipeline of an engine: Desc, static arrays, grid (set-up taps, read once)."""
        key = ('static', kind)
        if key not in self._oracle:
            eng = self.vega(kind).engine
            eng.eval(eng.low.theta0[None, :])                       # (the taps want an evaluation behind them)
            self._oracle[key] = {pid: (xo.Desc.from_engine(eng, pid), eng.bins_static(pid), eng.bins_grid(pid))
                                 for pid in range(eng.n_pipelines)}
        return self._oracle[key]

    def items(self, kind):
        eng = self.vega(kind).engine
        return [(name, eng.pipe_index[(name, 'peak')], eng.pipe_index[(name, 'smooth')]) for name in self.prob.items]

    def evaluate(self, kind, B, mode, extra_row=None):
        key = (kind, B, mode, None if extra_row is None else tuple(sorted(extra_row.items())))
        if key in self.results:
            return self.results[key]
        eng = self.vega(kind).engine
        st = self.static(kind)
        base = np.stack([eng.theta_from_params(row) for row in self.rows])
        which = (np.arange(B) + 1 + np.arange(B) // 4) % base.shape[0]       # (every walker in both slots of a two-walker thread)
        theta = base[which]
        if extra_row is not None:
            theta[min(2, B - 1)] = eng.theta_from_params(extra_row)
            which = which.copy()
            which[min(2, B - 1)] = -1
        res = dict(which=which, theta=theta, routes=[], status=[])
        for _ in range(3):
            chi2, status, model = eng.eval(theta, want_model=mode == 'model')
            res['routes'].append(eng.bins_route() - {'poly_bins'})
            res['status'].append(status.copy())
        res['scal'] = eng.bins_scalars(B)
        res['coef'] = eng.bins_coefficients(B)
        res['xi'], res['q'], res['groups'], res['static_groups'] = {}, {}, [], []
        route = res['routes'][-1]
        if mode == 'quad':
            for name, _, _ in self.items(kind):
                res['q'][name] = eng.quad_vector(name, B)
        if 'group' in route:
            res['groups'] = [(g, eng.lean_group_sum(i, B)) for i, g in enumerate(eng.lean_groups())]
        if 'static_group' in route:
            res['static_groups'] = [(g, eng.lean_group_sum(i, B, static=True)) for i, g in enumerate(eng.lean_groups(static=True))]
        if 'group' in route or 'static_group' in route:
            res['factors'] = eng.metal_factors(B) if eng.metal_source else None
        elif mode == 'model' or B <= 8:
            res['xi'] = {pid: eng.bins_xi(pid, B) for pid in st}
        self.results[key] = res
        return res

    def oracle(self, kind, res, b, pid):
        """(xi, bound, oob) of walker b of an evaluation, from its own taps; kept per distinct operands."""
        desc, st, grid = self.static(kind)[pid]
        sc, coef = res['scal'][b, pid], res['coef'][:, grid['column'], b, :]
        eng = self.vega(kind).engine
        key = (kind, pid, sc.tobytes(), coef.tobytes())
        if key not in self._oracle:
            terms = xo.engine_terms(eng, pid, res['theta'][b]) if desc.additive else None       # (of parameters no walker here moves)
            xi, bound, oob, parts = xo.xi_bins(desc, st, grid, sc, eng.bins_scalar_index(), coef, terms=terms)
            self._oracle[key] = (xi, bound, oob, parts['window'])
        return self._oracle[key][:3]

    def same_operands(self, kind, a, ia, b, ib, pid):
        """Whether walker ia of evaluation a and walker ib of b hand the bins of a pipeline the same bits: the scalars, and the
        coefficient rows inside the window the bins read (outside it the product leaves what an earlier evaluation wrote)."""
        col = self.static(kind)[pid][2]['column']
        self.oracle(kind, a, ia, pid)
        desc, st, grid = self.static(kind)[pid]
        lo, hi = self._oracle[(kind, pid, a['scal'][ia, pid].tobytes(), a['coef'][:, col, ia, :].tobytes())][3]
        return np.array_equal(a['scal'][ia, pid], b['scal'][ib, pid]) and \
            np.array_equal(a['coef'][:desc.n_ell, col, ia, lo:hi], b['coef'][:desc.n_ell, col, ib, lo:hi])

    def note(self, what, ratio):
        self.ratios[what] = max(self.ratios.get(what, 0.0), float(ratio))

    def close(self):
        print('\nXIBINS_RATIOS', json.dumps({'case': self.case, **{k: float(f'{v:.3g}') for k, v in sorted(self.ratios.items())},
                                            'ulps': {k: float(f'{v:.3g}') for k, v in sorted(self.ulps.items())}}))
        for v in self.vegas.values():
            v.close()
        self.vegas = {}


@pytest.fixture(scope='module')
def run(request, tmp_path_factory):
    assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'
    r = _Run(request.param, tmp_path_factory.mktemp(request.param))
    yield r
    r.close()


def _within(got, exact, bound, what):
    err = np.abs(got.astype(LD) - exact)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f'{what}: bin {worst} off by {float(err[worst]):.3e}, bound {float(bound[worst]):.3e}'
    assert np.all(got[bound == 0] == 0), f'{what}: a bin with a zero bound is not an exact 0'
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _same_row(run, kind, a, ia, b, ib, pid, row_a, row_b, what):
    """(d) across two evaluations: where the operands the bins read are the same bits (the walker's scalars, its coefficient
    rows), the rows are the same bits; where the coefficient product rounded apart (it tiles by batch size), the rows differ by no
    more than their bounds and what the oracle itself makes of the two sets of operands.  Returns whether the comparison was bitwise."""
    xa, da, _ = run.oracle(kind, a, ia, pid)
    xb, db, _ = run.oracle(kind, b, ib, pid)
    if run.same_operands(kind, a, ia, b, ib, pid):
        np.testing.assert_array_equal(row_a, row_b, err_msg=what)
        return True
    n = xa.size
    diff = np.abs(row_a[:n].astype(LD) - row_b[:n].astype(LD))
    assert np.all(diff <= da + db + np.abs(xa - xb)), (what, float(diff.max()))
    return False


def _ulps(run, what, diff, values):
    """The largest difference in ulps of the bin's own value (large where xi crosses zero) and in ulps of the vector's largest."""
    mag = np.abs(values)
    if not mag.any():
        return
    own = (diff[mag > 0] / np.spacing(mag[mag > 0])).max()
    run.ulps[what + '/ulp_of_bin'] = max(run.ulps.get(what + '/ulp_of_bin', 0.0), float(own))
    run.ulps[what + '/ulp_of_scale'] = max(run.ulps.get(what + '/ulp_of_scale', 0.0), float(diff.max() / np.spacing(mag.max())))


def _first(which):
    return {int(w): int(np.flatnonzero(which == w)[0]) for w in np.unique(which)}


def _check_bins(run, kind, B, mode, form):
    """(a), (b) for the per-pipeline bins, (d) within the batch, (f) status."""
    res = run.evaluate(kind, B, mode)
    st = run.static(kind)
    descs = [(st[p][0], st[s][0]) for _, p, s in run.items(kind)]
    extras = run.vega(kind).engine.item_extras
    pre = [extras[name]['template'] is not None or any(t[0] in (0, 1) for t in extras[name]['broadband']) for name, _, _ in run.items(kind)]
    want = expected_route(descs, B, mode, st[0][2]['same_grid'], kind, pre)
    for call, route in enumerate(res['routes']):
        assert route == want, (run.case, kind, B, mode, call, sorted(route), sorted(want))
    for status in res['status']:
        assert not status.any(), (run.case, kind, B, mode, status)
    first = _first(res['which'])
    for pid, xi in res['xi'].items():
        desc, stat, grid = st[pid]
        n = grid['n']
        assert np.all(xi[:, n:] == 0), f'{run.case} {form} B={B} pipeline {pid}: padding written'
        for b in range(B):
            at = first[int(res['which'][b])]
            if at != b:
                np.testing.assert_array_equal(xi[b], xi[at], err_msg=f'{run.case} {form} B={B} pipeline {pid}: walker {b} differs from its copy at {at}')
                continue
            exact, bound, oob = run.oracle(kind, res, b, pid)
            assert not oob.any()
            assert np.all(xi[b, :n][stat['r'] == 0] == 0)
            run.note(f'b/{form}', _within(xi[b, :n], exact, bound, f'{run.case} {form} B={B} walker {b} pipeline {pid}'))
    return res


@pytest.mark.parametrize('run', list(xo.CASES), indirect=True)
def test_model_request_bins(run):
    """k_xi_bins<false> (B <= 8; B > 8 under VMX_NO_XI_LEAN) and k_xi_bins_lean (B > 8 under VMX_NO_XI_SUMS) bin by bin; (d)
    across B = 9 and 70; (e) the two forms against each other."""
    got = {}
    for kind, batches in (('default', (1, 5)), ('nosums', (9, 11, 70)), ('nolean', (9, 11, 70))):
        for B in batches:
            got[(kind, B)] = _check_bins(run, kind, B, 'model', {'default': 'general', 'nosums': 'lean+rest', 'nolean': 'general'}[kind])
    for kind in ('nosums', 'nolean'):
        for other in (70, 11):
            small, big = got[(kind, 9)], got[(kind, other)]
            fs, fb = _first(small['which']), _first(big['which'])
            for pid in small['xi']:
                for w in fs:
                    bitwise = _same_row(run, kind, small, fs[w], big, fb[w], pid, small['xi'][pid][fs[w]], big['xi'][pid][fb[w]],
                                        f'{run.case} {kind} pipeline {pid} walker {w}: B = 9 and B = {other} differ')
                    run.ulps[f'd/{kind}/bitwise_9_{other}'] = run.ulps.get(f'd/{kind}/bitwise_9_{other}', 0) + int(bitwise)
        # (B = 9 and 11 share the coefficient product's tiling: the bins kernels are compared bit for bit on equal operands)
        assert run.ulps[f'd/{kind}/bitwise_9_11'] > 0, (run.case, kind)
    # (e) lean + rest against the general kernel, walker by walker
    a, b = got[('nosums', 9)], got[('nolean', 9)]
    fa = _first(a['which'])
    for pid in a['xi']:
        n = run.static('nosums')[pid][2]['n']
        for w, at in fa.items():
            _, ba, _ = run.oracle('nosums', a, at, pid)
            _, bb, _ = run.oracle('nolean', b, at, pid)
            diff = np.abs(a['xi'][pid][at, :n].astype(LD) - b['xi'][pid][at, :n].astype(LD))
            assert np.all(diff <= ba + bb), (run.case, pid, w, float(diff.max()))
            _ulps(run, 'e/lean_vs_general', diff, a['xi'][pid][at, :n])


@pytest.mark.parametrize('run', list(xo.CASES), indirect=True)
def test_group_sums(run):
    """k_xi_bins_group: sum of factor x xi over a group's members, against the oracle's sum under the members' bounds plus,
    per member, the product (1) and the running sum (1)."""
    eng = run.vega('default').engine
    groups = eng.lean_groups()
    st = run.static('default')
    n_lean_pairs = sum(_lean(st[p][0]) and _lean(st[s][0]) for _, p, s in run.items('default'))
    assert len(groups) == n_lean_pairs
    if not groups:
        return
    gkept = {}
    for B in (9, 11, 70):
        res = _check_bins(run, 'default', B, 'model', 'group')
        assert 'group' in res['routes'][-1] and len(res['groups']) == len(groups)
        first = _first(res['which'])
        for g, array in res['groups']:
            assert g['presum'] and np.all(array[:, g['n']:] == 0)
            for b in range(B):
                at = first[int(res['which'][b])]
                if at != b:
                    np.testing.assert_array_equal(array[b], array[at])
                    continue
                acc, bound = np.zeros(g['n'], LD), np.zeros(g['n'], LD)
                for pid, fkind, findex in g['members']:
                    assert fkind in (0, 1)
                    f = LD(1) if fkind == 0 else LD(res['theta'][b, findex])
                    xi, dxi, _ = run.oracle('default', res, b, pid)
                    prod = f * xi
                    acc = acc + prod
                    bound = bound + abs(f) * dxi + U * np.abs(prod) + U * np.abs(acc)
                run.note('b/group', _within(array[b, :g['n']], acc, bound, f'{run.case} group B={B} walker {b} members {g["members"]}'))
                gkept[(B, tuple(g['members']), int(res['which'][b]))] = (array[b, :g['n']].copy(), acc, bound)
    small = run.evaluate('default', 9, 'model')
    fs = _first(small['which'])
    for other in (70, 11):
        big = run.evaluate('default', other, 'model')
        fb = _first(big['which'])
        run.ulps[f'd/group/bitwise_9_{other}'] = 0
        for (B, members, w), (row, acc, bound) in gkept.items():
            if B != 9:
                continue
            row2, acc2, bound2 = gkept[(other, members, w)]
            if all(run.same_operands('default', small, fs[w], big, fb[w], pid) for pid, _, _ in members):
                np.testing.assert_array_equal(row, row2, err_msg=f'{run.case} group {members} walker {w}: B = 9 and B = {other} differ')
                run.ulps[f'd/group/bitwise_9_{other}'] += 1
            else:
                assert np.all(np.abs(row.astype(LD) - row2.astype(LD)) <= bound + bound2 + np.abs(acc - acc2)), (run.case, members, w, other)
    assert run.ulps['d/group/bitwise_9_11'] > 0, run.case


@pytest.mark.parametrize('run', list(xo.CASES), indirect=True)
def test_chi2_only_entries(run):
    """k_xi_assemble_quad (B <= 8: its bins are stored and checked too) and k_xi_quad_plain (B > 8): every entry of x' - x0'
    against fma(bao, xi_peak, xi_smooth) - x0' of the oracle; (e) the two forms against each other."""
    eng = run.vega('default').engine
    assert eng.quadratic_form
    bao = eng.low.slot['bao_amp']
    kept = {}
    for B in BATCHES + (11,):
        res = _check_bins(run, 'default', B, 'quad', 'assemble_quad' if B <= 8 else 'quad')
        form = 'quad_plain' if 'quad_plain' in res['routes'][-1] else 'assemble_quad'
        first = _first(res['which'])
        for name, p, s in run.items('default'):
            q, x0 = res['q'][name]
            n = run.static('default')[p][2]['n']
            extras = eng.item_extras[name]
            n_tail = sum(t[2].size for t in extras['broadband'] if t[0] == 3)
            assert q.shape[1] == x0.size and np.all(q[:, n + n_tail:] == 0) and np.all(x0[n + n_tail:] == 0)
            assert n_tail == xo.CASES[run.case][2].get(name, {}).get('n_post_coef', 0)
            for b in range(B):
                at = first[int(res['which'][b])]
                if at != b:
                    np.testing.assert_array_equal(q[b], q[at])
                    continue
                xp, dxp, _ = run.oracle('default', res, b, p)
                xs, dxs, _ = run.oracle('default', res, b, s)
                v, bound = xo.quad_entry(res['theta'][b, bao], xp, dxp, xs, dxs, x0[:n], extras, res['theta'][b])
                run.note(f'b/{form}', _within(q[b, :n], v, bound, f'{run.case} {form} B={B} walker {b} {name}'))
                if n_tail:
                    tail, dtail = xo.quad_tail(res['theta'][b, bao], extras, res['theta'][b], x0, n)
                    run.note(f'b/{form}/tail', _within(q[b, n:n + n_tail], tail, dtail, f'{run.case} {form} B={B} walker {b} {name}: broadband coefficients'))
                kept[(B, name, int(res['which'][b]))] = (q[b, :n].copy(), bound, x0[:n].copy(), v)
    r9 = run.evaluate('default', 9, 'quad')
    f9 = _first(r9['which'])
    for other in (70, 11):
        ro = run.evaluate('default', other, 'quad')
        fo = _first(ro['which'])
        run.ulps[f'd/quad/bitwise_9_{other}'] = 0
        for name, p, s in run.items('default'):
            for w in f9:
                q9, b9, _, v9 = kept[(9, name, w)]
                qo, bo, _, vo = kept[(other, name, w)]
                if all(run.same_operands('default', r9, f9[w], ro, fo[w], pid) for pid in (p, s)):
                    np.testing.assert_array_equal(q9, qo, err_msg=f'{run.case} {name} walker {w}: B = 9 and B = {other} differ')
                    run.ulps[f'd/quad/bitwise_9_{other}'] += 1
                else:
                    assert np.all(np.abs(q9.astype(LD) - qo.astype(LD)) <= b9 + bo + np.abs(v9 - vo)), (run.case, name, w, other)
    assert run.ulps['d/quad/bitwise_9_11'] > 0, run.case
    for (B, name, w), (q9, b9, x0, _) in kept.items():
        if B == 9:
            q5, b5, _, _ = kept[(5, name, w)]
            diff = np.abs(q9.astype(LD) - q5.astype(LD))
            assert np.all(diff <= b9 + b5), (run.case, name, w, float(diff.max()))
            _ulps(run, 'e/quad_forms', diff, q9 + x0)          # (in ulps of x': x' - x0' itself is ~0 at the expansion point)


@pytest.mark.parametrize('run', list(xo.CASES), indirect=True)
def test_scalars_against_the_parameters(run):
    """(c)  ap, at, delta_rp, the evolution exponents and the radiation parameters are copies of the parameters (exact); the
    reciprocals of the radiation lengths are one correctly rounded division (u)."""
    eng = run.vega('default').engine
    res = run.evaluate('default', 5, 'model')
    ix = eng.bins_scalar_index()
    names = eng.names
    for pid, (desc, _, _) in run.static('default').items():
        d = eng.pipe_descs[pid]
        for b in range(5):
            sc, t = res['scal'][b, pid], dict(zip(names, res['theta'][b]))
            assert d.scale_mode in (0, 1)                           # (unit - the smooth component here - or ap, at themselves)
            want_scale = (res['theta'][b, d.scale_slot[0]], res['theta'][b, d.scale_slot[1]]) if d.scale_mode == 1 else (1.0, 1.0)
            assert (sc[ix['AP']], sc[ix['AT']]) == want_scale
            assert sc[ix['DRP']] == (res['theta'][b, d.drp_slot] if d.drp_slot >= 0 else 0.0)
            evol = sorted([(sc[ix['EV1A']], sc[ix['EV1B']]), (sc[ix['EV2A']], sc[ix['EV2B']])])
            want = sorted((t['croom_par0'], t['croom_par1']) if d.tracer[q].evol_kind == 1 else (res['theta'][b, d.tracer[q].alpha_slot], 0.0)
                          for q in range(2))
            assert evol == want, (run.case, pid, evol, want)
            if desc.radiation:
                for key, name in (('RAD_S', 'strength'), ('RAD_A', 'asymmetry'), ('RAD_L', 'lifetime'), ('RAD_D', 'decrease')):
                    assert sc[ix[key]] == t['qso_rad_' + name]
                for key, src in (('RAD_IL', 'RAD_L'), ('RAD_ID', 'RAD_D')):
                    exact = 1 / LD(sc[ix[src]])
                    assert abs(LD(sc[ix[key]]) - exact) <= U * exact
        grid = run.static('default')[pid][2]
        for e in range(desc.n_ell):
            assert abs(LD(grid['inv_h'][e]) - 1 / LD(grid['h'][e])) <= U / LD(grid['h'][e])      # (the stored 1 / h: one rounding, as the bound counts)


@pytest.mark.parametrize('run', ['a63', 'j_small_big'], indirect=True)
def test_out_of_range_walker_is_flagged_alone(run):
    """(f)  ap = at = 1e-6 carries every r' (at most ~2e-4) below the first knot (x0 ~ -7.07, r ~ 8.5e-4): VMX_STATUS_BOUNDS
    for that walker and no other, from every form."""
    far = {'ap': 1e-6, 'at': 1e-6}
    for kind, B, mode in (('default', 5, 'model'), ('nosums', 9, 'model'), ('default', 9, 'model'), ('nolean', 9, 'model'),
                          ('default', 5, 'quad'), ('default', 9, 'quad')):
        res = run.evaluate(kind, B, mode, extra_row=far)
        for status in res['status']:
            flagged = (status & STATUS_BOUNDS) != 0
            assert flagged[2] and flagged.sum() == 1 and not status[~flagged].any(), (run.case, kind, B, mode, status)


# ---------------------------------------------------------------------------------------------------------------------
# the static-basis forms: k_poly_bins (set-up), k_xi_bins_static, k_xi_bins_static_nw<4>, k_xi_bins_static_group<2>, k_xi_bins<true>
# ---------------------------------------------------------------------------------------------------------------------
STATIC_ENV = dict(ENV, notaps='VMX_NO_STATIC_BINS VMX_NO_XI_SUMS')
STATIC_BATCHES = {'default': (1, 5, 9, 11, 70), 'nosums': (9, 11, 70), 'notaps': (1, 5, 9, 11)}


@pytest.fixture(scope='module')
def static_run(request, tmp_path_factory):
    assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'
    r = _Run(request.param, tmp_path_factory.mktemp(request.param), build=xo.build_static_case, env=STATIC_ENV, csr_threshold=0.0)
    yield r
    r.close()


def _planned_route(eng, st, kind, B):
    """run_chain's choice from the planner's own lists (the groups of vmx_debug_read 13 and 18) and the pipelines' descriptors."""
    per_walker = [p for p, (_, _, g) in st.items() if g['column'] >= 0]
    lean = [p for p in per_walker if _lean(st[p][0])]
    on_bins = [p for p, (_, _, g) in st.items() if g['static_basis'] >= 0 and g['static_bins']]
    on_taps = [p for p, (_, _, g) in st.items() if g['static_basis'] >= 0 and not g['static_bins']]
    groups, static_groups = eng.lean_groups(), eng.lean_groups(static=True)
    grouped = {pid for g in groups + static_groups for pid, _, _ in g['members']}
    sums_on = B > 8 and bool(groups or static_groups)
    bits = {'static_taps'} if on_taps else set()
    if B <= 8 or not lean:
        bits.add('general')
    else:
        bits |= ({'group'} if sums_on and groups else set()) | ({'lean'} if set(lean) - grouped or not (sums_on and groups) else set())
        bits |= {'general'} if len(lean) < len(per_walker) else set()
    if on_bins:
        bits.add('poly_bins')
        if sums_on:
            bits |= ({'static_group'} if static_groups else set()) | ({'static'} if set(on_bins) - grouped else set())
        else:
            bits.add('static_nw' if B > 8 else 'static')
    return bits


def _static_oracle(run, kind, res, b, pid, y, basis):
    """(xi, bound) of a static-basis pipeline: from the basis on its bins, or - tap form - from the basis coefficients."""
    desc, stat, grid = run.static(kind)[pid]
    ix = run.vega(kind).engine.bins_scalar_index()
    if grid['static_bins']:
        return xo.static_bins(desc, stat, res['scal'][b, pid], ix, y[pid][:, :grid['n']])
    exact, bound, oob, _ = xo.xi_bins(desc, stat, grid, res['scal'][b, pid], ix, None, basis=basis[:, grid['static_basis']])
    assert not oob.any()
    return exact, bound


@pytest.mark.parametrize('static_run', list(xo.STATIC_CASES), indirect=True)
def test_static_basis_forms(static_run):
    run = static_run
    claims = xo.STATIC_CASES[run.case]['routes']
    rows, seen = {}, set()
    for kind, batches in STATIC_BATCHES.items():
        eng = run.vega(kind).engine
        st = run.static(kind)
        static_pids = [pid for pid, (_, _, g) in st.items() if g['static_basis'] >= 0]
        assert static_pids and all(st[p][2]['column'] < 0 for p in static_pids)
        for pid in static_pids:
            d = eng.pipe_descs[pid]
            assert not d.uv_shotnoise and not d.radiation and st[pid][0].evol == (0, 0) and st[pid][2]['odd_ncoef'] == 0
        assert (kind == 'notaps') == (not any(st[p][2]['static_bins'] for p in static_pids))
        # set-up: k_poly_bins against the spline and Legendre sums of the basis coefficients
        basis, y = eng.poly_coefficients(), {}
        for pid in static_pids:
            desc, stat, grid = st[pid]
            if not grid['static_bins']:
                continue
            y[pid] = eng.poly_bins(pid)
            n = grid['n']
            exact, bound, oob = xo.poly_bins(desc, stat, grid, basis[:, grid['static_basis']])
            assert not oob.any() and np.all(y[pid][:, n:] == 0)
            for i in range(3):
                run.note('b/poly_bins', _within(y[pid][i, :n], exact[i], bound[i], f'{run.case} {kind} k_poly_bins pipeline {pid} basis vector {i}'))
        for B in batches:
            res = run.evaluate(kind, B, 'model')
            want = _planned_route(eng, st, kind, B)
            literal = claims.get((kind, 'small' if B <= 8 else 'big'))
            assert literal is None or literal == want, (run.case, kind, B, sorted(literal), sorted(want))
            for call, route in enumerate(res['routes']):
                route = (route | (eng.bins_route() & {'poly_bins'})) - {'same_grid'}
                assert route == want, (run.case, kind, B, call, sorted(route), sorted(want))
                seen |= route
            assert not any(status.any() for status in res['status'])
            first = _first(res['which'])
            for pid in static_pids if res['xi'] else ():
                grid = st[pid][2]
                form = ('static_nw' if B > 8 else 'static') if grid['static_bins'] else 'static_taps'
                xi, n = res['xi'][pid], grid['n']
                assert np.all(xi[:, n:] == 0)
                for b in range(B):
                    w, at = int(res['which'][b]), first[int(res['which'][b])]
                    if at != b:
                        np.testing.assert_array_equal(xi[b], xi[at], err_msg=f'{run.case} {form} B={B} pipeline {pid} walker {b}')
                        continue
                    exact, bound = _static_oracle(run, kind, res, b, pid, y, basis)
                    run.note(f'b/{form}', _within(xi[b, :n], exact, bound, f'{run.case} {kind} {form} B={B} walker {b} pipeline {pid}'))
                    # (d) these forms read the walker's scalars and static arrays only: one row for one walker at every B > 8 (and <= 8)
                    key = (kind, form, pid, w)
                    if key in rows:
                        np.testing.assert_array_equal(xi[b], rows[key], err_msg=f'{run.case} {kind} {form} pipeline {pid} walker {w}: B = {B} differs')
                    rows[key] = xi[b].copy()
            # the per-walker pipelines beside them (core pairs; mj: the cross item's metal pipelines, lean singles)
            for pid in (p for p, (_, _, g) in st.items() if g['column'] >= 0) if res['xi'] else ():
                n = st[pid][2]['n']
                for b in sorted(set(first.values())):
                    exact, bound, oob = run.oracle(kind, res, b, pid)
                    assert not oob.any()
                    run.note('b/per_walker', _within(res['xi'][pid][b, :n], exact, bound, f'{run.case} {kind} B={B} walker {b} pipeline {pid}'))
            # the sums on the way: k_xi_bins_group and k_xi_bins_static_group, every factor kind
            for what, groups in (('group', res['groups']), ('static_group', res['static_groups'])):
                for g, array in groups:
                    assert g['presum'] and len(g['members']) > 1 and np.all(array[:, g['n']:] == 0)
                    for b in range(B):
                        w, at = int(res['which'][b]), first[int(res['which'][b])]
                        if at != b:
                            np.testing.assert_array_equal(array[b], array[at])
                            continue
                        acc, bound = np.zeros(g['n'], LD), np.zeros(g['n'], LD)
                        for pid, fkind, findex in g['members']:
                            f = LD(1) if fkind == 0 else LD(res['theta'][b, findex]) if fkind == 1 else LD(res['factors'][b, 0, findex])
                            xi, dxi = run.oracle(kind, res, b, pid)[:2] if what == 'group' else _static_oracle(run, kind, res, b, pid, y, basis)
                            prod = f * xi
                            acc = acc + prod
                            bound = bound + abs(f) * dxi + U * np.abs(prod) + U * np.abs(acc)
                        run.note(f'b/{what}', _within(array[b, :g['n']], acc, bound, f'{run.case} {what} B={B} walker {b} members {g["members"]}'))
                        key = (kind, what, tuple(g['members']), w)
                        if what == 'static_group' and key in rows:
                            np.testing.assert_array_equal(array[b], rows[key], err_msg=f'{run.case} static group walker {w}: B = {B} differs')
                        rows[key] = array[b].copy()
    # every static form the case claims was reached, under an asserted route
    for literal in claims.values():
        assert literal <= seen | {'general', 'lean', 'group'}, (run.case, sorted(literal), sorted(seen))
    assert {'poly_bins', 'static', 'static_nw', 'static_taps'} <= seen, (run.case, sorted(seen))
