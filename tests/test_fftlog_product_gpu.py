"""The engine's FFTLog o spline product  coef_ell = OP_ell P_ell  (run_chain -> launch_product(KC_FFTLOG)) against np.longdouble,
element by element under the a-priori bound (K + 2) u (|OP| |P|) of tests/helpers/fftlog_product.py, in every form the host
chooses for it - as the chain runs it: with the device row window k_prologue writes, the device column limit the P(k,mu)
kernels leave, the four multipoles as its batch, and stale rows of earlier evaluations around the window.

Engines (module-scoped, at most two alive): a63 (two coefficient columns), mj (the most columns of the suite), a63_ell2
(n_ell = 2: two multipoles no bin reads), j_odd (odd multipoles: the window fully open) and the fht_extrap problem of
tests/test_variants_gpu.py (K = 2048: 64 K stages, power-law pads, no column limit).

Every batch is evaluated as: walkers A with the weakest smoothing the mu rule's box allows (large live limit) and another
dilation (another window), then walkers B with the strongest (small live limit) twice.  The form (vmx_debug_read 4 [10]) is
asserted against helpers.fftlog_product.expected_form on all three calls (the second and third replay the captured graph), and the
checks run on B's taps (0: P_ell, 2: coefficients, 4: live limit and window, 6: scalars):

  (a) every multipole, column and walker, every coefficient row of the device's window: |coef - ref| <= bound; an exact 0 where
      the bound is 0.  (The P(k,mu) kernels form all four multipoles for every pipeline - EngineDev::n_ell is VMX_MAX_ELL - so a
      pipeline with n_ell < 4 hands the product real rows for the multipoles its bins never read: a63_ell2 holds them to the
      bound like any other.)
  (b) a row outside the window keeps the bits A left, or satisfies (a) (the MFMA kernels finish the window's last 64-row tile);
      rows [n_coef, ncp) are never non-zero;
  (c) the window covers the rows every walker's bins read (helpers.fftlog_product.bins_window), with the walker whose alphas
      put r' below the first knot and one with NaN in ap (the window then opens fully, and the other walkers' rows inside their
      own windows are bit for bit those of the batch with the fiducial point in the NaN walker's place);
  (d) every P_ell sample from the live limit on is an exact 0.0, every sample finite, the limit a multiple of the k tile the
      batch size guarantees (or nk);
  (e) the fht_extrap pads against f_0 ratio^-t and f_n ratio^t in longdouble at (E_POW + 1) u;
  (f) one walker in batches of different forms: inside the rows its bins read the coefficients differ by no more than the two
      bounds (plus the difference of the two references where the P(k,mu) stage handed the batches different bits), and are the
      same bits where form and operand are the same.

`FFTLOG_RATIOS` lines (-s shows them) carry the largest err / bound per case and form, the reference's seconds, and the
table level / live limit of the P(k,mu) stage per batch.  No size reaches the four-buffer ring (tests/test_fftlog_product_host.py:
its interval lies inside the 64 x 32 one, which is tested first); every evaluation here asserts that none reports it.
"""
import json
import time

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import fftlog_product as fp
from helpers import xi_bins_oracle as xo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = fp.U
STATUS_BOUNDS = 1
MAX_BATCH = {'a63': 769, 'mj': 70, 'a63_ell2': 40, 'j_odd': 84, 'j_small_big': 16, 'extrap': 161}
N_COLUMNS = {'a63': 2, 'mj': 8, 'a63_ell2': 2, 'j_odd': 4, 'j_small_big': 4, 'extrap': 2}


class _Case:
    def __init__(self, name, tmp):
        from vega_amd import VegaInterface
        assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'
        self.name = name
        base = None
        if name == 'extrap':
            from test_variants_gpu import _extrap_problem
            self.prob = _extrap_problem()
        elif name == 'mj':
            self.prob = xo.build_static_case(tmp, name, GOLDEN)
        else:
            self.prob = xo.build_case(tmp, name, GOLDEN)
        self.vega = VegaInterface(None, problem=self.prob, max_batch=MAX_BATCH[name])
        eng = self.eng = self.vega.engine
        if name == 'extrap':
            # (the golden walkers of this problem carry sigmaNL = 0: spectra with non-zero end samples)
            exp = np.load(GOLDEN / 'expected_fht_extrap.npz')
            base = eng.theta_from_params(dict(zip([str(n) for n in exp['param_names']], map(float, exp['theta'][0]))))
        self.theta0 = eng.low.theta0.copy() if base is None else base
        self.slot = eng.low.slot
        _, status, _ = eng.eval(self.theta0[None, :], want_model=True)          # (the taps want an evaluation behind them)
        assert not status.any()
        grid = eng.bins_grid(0)
        self.n_coef, self.ncp, self.n_columns = grid['n_coef'], grid['ncp'], grid['n_columns']
        assert self.n_columns == N_COLUMNS[name], (name, self.n_columns)
        self.nk, self.pads = int(np.asarray(self.prob.k).size), sum(eng.fftlog_pads)
        self.nkp = fp.pad32(self.nk + self.pads)
        assert (self.n_coef, self.ncp) == (self.nk + 2, fp.pad32(self.nk + 2))
        pipes = [p for it in self.prob.items.values() for p in [it.core] + [m.pipeline for m in it.metals]]
        lowring = {p.xi.fht_lowring for p in pipes}
        assert len(lowring) == 1
        self.ops = fp.operators(self.prob.k, lowring=lowring.pop(), extrap=eng.fht_extrap)
        assert all(op.shape == (self.n_coef, self.nk + self.pads) for op in self.ops)
        self.ix = eng.bins_scalar_index()
        self.static = {pid: (xo.Desc.from_engine(eng, pid), eng.bins_static(pid), eng.bins_grid(pid)) for pid in range(eng.n_pipelines)}
        self.column = {pid: st[2]['column'] for pid, st in self.static.items() if st[2]['column'] >= 0}
        assert sorted(self.column.values()) == list(range(self.n_columns))
        self.fully_open = any(st[2]['odd_ncoef'] > 0 for st in self.static.values())
        self.ratios, self.seconds, self.pk, self.repeats = {}, {}, {}, {True: 0, False: 0}

    # ---- evaluations
    def batch_for(self, ncols):
        """The smallest batch with at least ncols columns."""
        return -(-ncols // self.n_columns)

    def walkers(self, B, spread, seed, smoothing=None, scale=1.0):
        base = self.theta0.copy()
        base[self.slot['ap']] *= scale
        base[self.slot['at']] *= scale
        return fp.walkers(base, self.slot, B, spread, seed, smoothing)

    def run(self, theta, mode, lanes=1):
        """One evaluation and its taps; the form against the host rule restated."""
        eng, B = self.eng, theta.shape[0]
        chi2, status, _ = eng.eval(theta, want_model=mode == 'model')
        facts = eng.debug_read(4, 0, 11)
        form = eng.fftlog_form()
        want = fp.expected_form(self.n_coef, B * self.n_columns, lanes, self.pads)
        assert form == want, (self.name, B, lanes, sorted(form), sorted(want))
        assert 'ring' not in form
        return dict(B=B, theta=theta, status=status.copy(), chi2=chi2.copy(), form=form, live=int(facts[0]), level=int(facts[4]),
                    win=(int(facts[5]), int(facts[6])))

    def taps(self, res):
        eng, n = self.eng, res['B'] * self.n_columns
        res['P'] = eng.debug_read(0, 0, 4 * n * self.nkp).reshape(4, n, self.nkp).copy()
        res['coef'] = eng.debug_read(2, 0, 4 * n * self.ncp).reshape(4, n, self.ncp).copy()
        res['scal'] = eng.bins_scalars(res['B'])
        return res

    def sequence(self, B, mode='model', lanes=1, spread='narrow', seed=0, smoothing=(fp.WEAK, fp.STRONG), first_spread=None):
        """A (weak smoothing, dilated by 6 %: another window, a larger live limit), then B twice; returns (A, B) with their taps."""
        if lanes != 1:
            self.eng.set_lanes(lanes)
        try:
            a = self.taps(self.run(self.walkers(B, first_spread or spread, 1000 + seed, smoothing[0], scale=1.06), mode, lanes))
            theta = self.walkers(B, spread, 2000 + seed, smoothing[1])
            b = self.taps(self.run(theta, mode, lanes))
            again = self.taps(self.run(theta, mode, lanes))
        finally:
            if lanes != 1:
                self.eng.set_lanes(1)
        # the repeat: the same window; and where the P(k,mu) stage handed over the same bits (it may take another route for
        # parameters it has just seen: its tables are kept across evaluations), the same coefficients bit for bit
        np.testing.assert_array_equal(again['scal'], b['scal'])
        assert again['win'] == b['win']
        self.check_limit(again)
        self.repeats[np.array_equal(again['P'], b['P'])] += 1
        if np.array_equal(again['P'], b['P']):
            np.testing.assert_array_equal(again['coef'], b['coef'], err_msg=f'{self.name} B={B}: coefficients of a repeated evaluation')
        return a, b

    # ---- checks
    def check_limit(self, res):
        """(d)"""
        P, live, nk, what = res['P'], res['live'], self.nk, f'{self.name} B={res["B"]}'
        assert np.all(np.isfinite(P)), f'{what}: a P_ell sample is not finite'
        assert not P[:, :, self.nk + self.pads:].any(), f'{what}: padding columns of P_ell written'
        if self.pads:
            assert live == nk, (what, live)             # (no smoothing: every wavenumber is live, and no limit is passed)
            return
        assert 0 < live <= nk and (live % fp.pk_tile(res['B']) == 0 or live == nk), (what, live)
        assert np.all(P[:, :, live:] == 0.0), f'{what}: a P_ell sample at or behind the live limit {live} is not an exact 0'
        last = np.flatnonzero(np.any(P != 0, axis=(0, 1)))
        assert last.size and last[-1] < live, (what, live)

    def check_product(self, res, before, tag):
        """(a), (b) on the taps of `res`; before: the coefficient tap of the evaluation before it (same batch size).  Returns the
        rows checked, and the bound and the reference of every element of them (for (f))."""
        P, coef, (lo, hi), n_coef = res['P'], res['coef'], res['win'], self.n_coef
        what = f'{self.name} B={res["B"]} {tag}'
        self.check_limit(res)
        assert np.all(np.isfinite(coef)), f'{what}: a coefficient is not finite'
        assert not coef[:, :, n_coef:].any(), f'{what}: rows [n_coef, ncp) written'
        lo, hi = max(lo, 0), min(hi, n_coef - 1)
        assert lo <= hi, (what, res['win'])
        if self.fully_open:
            assert (lo, hi) == (0, n_coef - 1), (what, res['win'])
        inside = np.zeros(n_coef, bool)
        inside[lo:hi + 1] = True
        changed = coef[:, :, :n_coef] != before[:, :, :n_coef]
        rows = np.flatnonzero(inside | changed.any(axis=(0, 1)))
        # (rows rewritten outside the window: the rest of the window's last 64-row tile at the most)
        assert rows.size <= inside.sum() + fp.GEMM_BM and rows[0] >= lo, (what, res['win'], int(rows[0]), int(rows[-1]), rows.size)
        last = np.flatnonzero(np.any(P != 0, axis=(0, 1)))
        cols = self.nk + self.pads if self.pads else min(self.nk, fp.pad32(max(res['live'], int(last[-1]) + 1)))
        k_terms = self.nk + self.pads
        form = '+'.join(sorted(res['form']))
        bounds = np.zeros((4, coef.shape[1], rows.size))
        refs = np.zeros((4, coef.shape[1], rows.size), LD)
        t0 = time.perf_counter()
        for e in range(4):
            ref, bound = fp.reference(self.ops[e], P[e], rows, cols, k_terms)
            got = coef[e][:, rows]
            must = inside[rows][None, :] | changed[e][:, rows]           # (an unchanged element outside the window keeps its bits)
            err = np.abs(got.astype(LD) - ref)
            bad = must & (err > bound)
            if bad.any():
                c, r = np.unravel_index(int(np.argmax(np.where(must, err - bound, -1))), err.shape)
                raise AssertionError(f'{what} ell={2 * e} column {c} row {rows[r]} (window {res["win"]}, live {res["live"]}): off by '
                                     f'{float(err[c, r]):.3e}, bound {bound[c, r]:.3e}; {int(bad.sum())} elements over their bound')
            assert np.all(got[must & (bound == 0)] == 0), f'{what} ell={2 * e}: an element with a zero bound is not an exact 0'
            live = must & (bound > 0)
            if live.any():
                self.ratios[form] = max(self.ratios.get(form, 0.0), float((err[live] / bound[live]).max()))
            bounds[e], refs[e] = bound, ref
        self.seconds[f'{tag} B={res["B"]}'] = round(time.perf_counter() - t0, 2)
        self.pk[f'{tag} B={res["B"]}'] = (res['level'], res['live'], hi - lo + 1)
        # every used multipole of every column was really there (a check of zeros against zeros would hold nothing)
        for pid, col in self.column.items():
            n_ell = self.static[pid][0].n_ell
            sl = slice(col * res['B'], (col + 1) * res['B'])
            assert np.all(np.any(bounds[:n_ell, sl] > 0, axis=2)), f'{what}: a used multipole of pipeline {pid} has a zero operand'
        return rows, bounds, refs

    def windows(self, res, walkers):
        """{(walker, pipeline): [lo, hi)} the bins read, for the pipelines with a coefficient column."""
        return {(b, pid): fp.bins_window(self.static[pid], res['scal'][b, pid], self.ix) for b in walkers for pid in self.column}

    def close(self):
        print('\nFFTLOG_RATIOS', json.dumps({'case': self.name, 'ratios': {k: float(f'{v:.3g}') for k, v in sorted(self.ratios.items())},
                                            'reference_seconds': self.seconds, 'level_live_window': self.pk,
                                            'repeats_with_equal_P': self.repeats[True], 'repeats_with_other_P': self.repeats[False]}))
        self.vega.close()


_CASES = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    """name -> _Case, built on first use; at most two engines alive: a63, which most tests use, and one other."""
    def get(name):
        if name not in _CASES:
            while len(_CASES) >= 2:
                _CASES.pop(next(n for n in _CASES if n != 'a63')).close()
            _CASES[name] = _Case(name, tmp_path_factory.mktemp(name))
        return _CASES[name]
    yield get
    while _CASES:
        _CASES.pop(next(iter(_CASES))).close()


def _sizes(case):
    """label -> (ncols wanted, kernel of the form, lanes) from the host rule's own edges."""
    below, first32, last32, above = fp.form_edges(case.n_coef)
    return {'gemv_2': (2, 'nb2', 1), 'gemv_4': (4, 'nb4', 1), 'gemv_6': (6, 'nb8', 1), 'gemv_8': (8, 'nb8', 1),
            'mfma64_10': (10, 'mfma64', 1), 'mfma64_64': (64, 'mfma64', 1), 'mfma64_65': (65, 'mfma64', 1),
            'mfma64_last': (below - case.n_columns + 1, 'mfma64', 1), 'mfma32_first': (first32, 'mfma32', 1),
            'mfma32_x32': (first32 // 32 * 32 + 32, 'mfma32', 1), 'mfma32_tail': (first32 // 32 * 32 + 65, 'mfma32', 1),
            'mfma32_last': (last32 - case.n_columns + 1, 'mfma32', 1), 'mfma64_next': (above, 'mfma64', 1),
            'lanes2_mfma64': (69, 'mfma64', 2), 'lanes2_mfma32': (first32 // 32 * 32 + 33, 'mfma32', 2)}


A63_LABELS = ('gemv_2', 'gemv_4', 'gemv_6', 'gemv_8', 'mfma64_10', 'mfma64_64', 'mfma64_65', 'mfma64_last', 'mfma32_first',
              'mfma32_x32', 'mfma32_tail', 'mfma32_last', 'mfma64_next', 'lanes2_mfma64', 'lanes2_mfma32')
SWEEP = [('a63', label) for label in A63_LABELS] + \
        [('mj', 'gemv_8'), ('mj', 'mfma64_10'), ('mj', 'mfma32_first'),
         ('a63_ell2', 'gemv_2'), ('a63_ell2', 'gemv_8'), ('a63_ell2', 'mfma64_10'), ('a63_ell2', 'mfma64_65'),
         ('j_odd', 'gemv_4'), ('j_odd', 'gemv_8'), ('j_odd', 'mfma64_10'), ('j_odd', 'mfma64_65'), ('j_odd', 'mfma32_first'),
         ('extrap', 'gemv_2'), ('extrap', 'mfma64_10'), ('extrap', 'mfma32_first')]


@pytest.mark.parametrize('name,label', SWEEP)
def test_product_in_every_form(cases, name, label):
    """(a), (b), (d) at the sizes of the host rule's edges; the batch sizes follow from expected_form."""
    case = cases(name)
    ncols, kernel, lanes = _sizes(case)[label]
    B = case.batch_for(ncols)
    n = B * case.n_columns
    assert kernel in fp.expected_form(case.n_coef, n, lanes, case.pads), (name, label, n)
    if label == 'mfma64_last':
        assert 'mfma32' in fp.expected_form(case.n_coef, n + case.n_columns, lanes, case.pads)
    if label == 'mfma32_first':
        assert 'mfma64' in fp.expected_form(case.n_coef, n - case.n_columns, lanes, case.pads)
    if label == 'mfma32_x32':
        assert n % 32 == 0 and n % 64 != 0
    if label == 'mfma32_tail':
        assert 0 < n % 32 < 4
    if label == 'mfma32_last':
        assert 'mfma64' in fp.expected_form(case.n_coef, n + case.n_columns, lanes, case.pads)
    if label == 'mfma64_65':
        assert 64 < n <= 64 + case.n_columns                    # (one or two columns into the second walker tile: B n_columns steps)
    # chi2-only and model requests alternate: k_chi2 or the bins / assemble kernels end the chain and reset the window
    mode = 'chi2' if sum(map(ord, label)) % 2 else 'model'
    a, b = case.sequence(B, mode=mode, lanes=lanes, seed=len(label) + n)
    assert not b['status'].any(), (name, label, b['status'])
    assert ('batch_y' in b['form']) == (lanes == 2 and n > 8)
    if not case.fully_open:
        assert b['win'] != a['win']                             # (A's dilation moved the window: stale rows lie around B's)
    if not case.pads and name != 'mj':
        assert b['live'] < a['live'], (a['live'], b['live'])    # (narrow after wide: samples A left alive must be zeros now)
    case.check_product(b, a['coef'], label)


@pytest.mark.parametrize('name', ['a63', 'j_small_big'])
def test_window_covers_what_the_bins_read(cases, name):
    """(c), with the wide spread: both extremes of [0.55, 1.45] in the batch, delta_rp over +- 25 where the case has it."""
    case = cases(name)
    eng, slot, B = case.eng, case.slot, 6
    theta = case.walkers(B, 'wide', 77)
    theta[4, slot['ap']] = theta[4, slot['at']] = 1e-6          # r' below the first knot: VMX_STATUS_BOUNDS
    with_nan = theta.copy()
    theta[5] = case.theta0                                      # the fiducial point in the NaN walker's place
    with_nan[5, slot['ap']] = np.nan
    first = case.taps(case.run(case.walkers(B, 'narrow', 78, scale=1.06), 'model'))
    plain = case.taps(case.run(theta, 'model'))
    assert (plain['status'][4] & STATUS_BOUNDS) and not plain['status'][[0, 1, 2, 3, 5]].any(), plain['status']
    case.check_product(plain, first['coef'], 'wide')
    lo, hi = plain['win']
    assert 0 <= lo <= hi <= case.n_coef - 1
    windows = case.windows(plain, range(B))
    for (b, pid), (wlo, whi) in windows.items():
        assert lo <= wlo and whi - 1 <= hi, (name, b, pid, (wlo, whi), plain['win'])
    assert min(w[0] for w in windows.values()) == 0             # (the walker below the first knot reads the first cell)
    spans = {b: (min(w[0] for (bb, _), w in windows.items() if bb == b), max(w[1] for (bb, _), w in windows.items() if bb == b)) for b in range(B)}
    assert spans[0] != spans[1]                                 # (the extremes do read different rows)
    # the lower edge: the same walkers without the one below the first knot (it pins the window's first row to 0)
    inner_theta = theta.copy()
    inner_theta[4] = case.theta0
    inner = case.taps(case.run(inner_theta, 'model'))
    assert not inner['status'].any() and 0 < inner['win'][0] <= inner['win'][1] <= case.n_coef - 1, (inner['status'], inner['win'])
    for (b, pid), (wlo, whi) in case.windows(inner, range(B)).items():
        assert inner['win'][0] <= wlo and whi - 1 <= inner['win'][1], (name, b, pid, (wlo, whi), inner['win'])
    case.check_product(inner, plain['coef'], 'wide_inner')
    opened = case.taps(case.run(with_nan, 'model'))
    assert opened['win'] == (0, case.n_coef - 1), opened['win']
    assert opened['status'][5] != 0 and (opened['status'][4] & STATUS_BOUNDS) and not opened['status'][:4].any(), opened['status']
    case.check_limit(opened)
    for (b, pid), (wlo, whi) in windows.items():
        if b == 5:
            continue
        col = case.column[pid] * B + b
        np.testing.assert_array_equal(opened['P'][:, col], plain['P'][:, col], err_msg=f'{name} walker {b}: P_ell beside a NaN walker')
        np.testing.assert_array_equal(opened['coef'][:, col, wlo:whi], plain['coef'][:, col, wlo:whi],
                                      err_msg=f'{name} walker {b} pipeline {pid}: rows {wlo}..{whi} beside a NaN walker')


PK_SHAPES = {'a63': (1, 5, 9, 30, 70), 'mj': (1, 3, 30, 70)}


@pytest.mark.parametrize('name', list(PK_SHAPES))
def test_column_limit_of_every_pk_shape(cases, name):
    """(d) and (a) at the batch sizes of run_chain's P(k,mu) launch shapes - 8-, 16- and 64-wide k_pk_multipoles (every walker its
    own smoothing lengths), k_pk_tab2 <16, 16, 1>, <64, 4, 1> and <64, 4, 2> (the batch shares them: table level 2), k_pk_w <1> and
    <2> on mj's shared-W groups - narrow after wide: the smoothing lengths move the live limit by dozens of samples."""
    case = cases(name)
    levels = set()
    for B in PK_SHAPES[name]:
        for kind, smoothing in (('shared', (fp.WEAK, fp.STRONG)), ('own', ((fp.WEAK, 2 * fp.WEAK), (0.6 * fp.STRONG, fp.STRONG)))):
            a, b = case.sequence(B, mode='model', seed=500 + B, smoothing=smoothing)
            assert not b['status'].any()
            if name == 'mj':
                assert a['live'] == b['live'] == case.nk            # (its metal pipelines carry no damping factor: every wavenumber is live)
            else:
                assert a['live'] - b['live'] >= 64, (name, B, kind, a['live'], b['live'])       # (across multiples of 32)
            case.check_limit(a)
            case.check_product(b, a['coef'], f'pk_{kind}')
            levels.add((kind, b['level']))
    assert ('shared', 2) in levels and any(level < 2 for kind, level in levels if kind == 'own'), sorted(levels)


def test_fht_extrap_pads(cases):
    """(e)  k_pk_extrap: left pad t = f_0 (f_1 / f_0)^-t, right pad t = f_n (f_n / f_m)^t; ratio one IEEE division as in the kernel
    (the same bits), pow and the product in longdouble; the bar (E_POW + 1) u relative: pow's documented error and one rounding of
    the product."""
    case = cases('extrap')
    B = 3
    a, b = case.sequence(B, mode='model', seed=9)
    assert not b['status'].any() and 'k_limit' not in b['form']
    nk, (lo, hi) = case.nk, case.eng.fftlog_pads
    assert (lo, hi) == (617, 617)
    P = b['P']
    worst, n_zero_ends = 0.0, 0
    bar = (fp.E_POW + 1) * LD(U)
    for pid, col in case.column.items():
        n_ell = case.static[pid][0].n_ell
        for e in range(4):
            for w in range(B):
                row = P[e, col * B + w]
                if e >= n_ell:
                    assert not row[nk:].any()                       # (pads of unused multipoles are exact zeros)
                    continue
                f0, f1, fm, fn = row[0], row[1], row[nk - 2], row[nk - 1]
                # (the peak component's template ends in exact zeros - full and smooth spectrum agree there: ratio 0, pads 0)
                assert f0 != 0 and fm != 0
                left = LD(f0) * np.power(LD(f1 / f0), -np.arange(1, lo + 1).astype(LD))
                right = LD(fn) * np.power(LD(fn / fm), np.arange(1, hi + 1).astype(LD))
                want = np.concatenate([left, right])
                assert np.all(np.isfinite(want))
                n_zero_ends += int(fn == 0)
                got = row[nk:nk + lo + hi].astype(LD)
                normal = np.abs(want) > LD(np.finfo(np.float64).tiny) / LD(U)      # (relative bars hold above the subnormals)
                assert normal.any()
                err = np.abs(got - want)[normal] / np.abs(want)[normal]
                worst = max(worst, float(err.max() / LD(U)))
                assert np.all(err <= bar), (pid, e, w, float(err.max() / LD(U)))
                assert np.all(np.abs(got - want)[~normal] <= LD(np.finfo(np.float64).tiny))
    case.ratios['pads: largest error in u'] = worst
    case.ratios['pads: rows whose last sample is 0'] = n_zero_ends


def test_one_answer_however_it_is_tiled(cases):
    """(f)  Three walkers at the head of batches of every form; inside the rows a walker's bins read, its coefficients differ
    between two forms by no more than the two bounds - and are the same bits where the form is the same (B = 5 and 6: 64 x 64
    tiles, the walker in the same tile)."""
    case = cases('a63')
    first32 = fp.form_edges(case.n_coef)[1]
    head = case.walkers(3, 'narrow', 4242, fp.STRONG)
    got = {}
    for B in (4, 5, 6, case.batch_for(first32)):
        theta = case.walkers(B, 'narrow', 4300 + B, fp.STRONG)
        theta[:3] = head
        before = case.taps(case.run(case.walkers(B, 'narrow', 4400 + B, fp.WEAK, scale=1.06), 'model'))
        res = case.taps(case.run(theta, 'model'))
        rows, bounds, refs = case.check_product(res, before['coef'], 'tiled')
        got[B] = (res, rows, bounds, refs, case.windows(res, range(3)))
    kernels = [next(k for k in ('gemv', 'mfma64', 'mfma32') if k in got[B][0]['form']) for B in got]
    assert kernels == ['gemv', 'mfma64', 'mfma64', 'mfma32']
    bitwise = 0
    batches = list(got)
    for i, Ba in enumerate(batches):
        for Bb in batches[i + 1:]:
            (ra, rows_a, bound_a, ref_a, win_a), (rb, rows_b, bound_b, ref_b, win_b) = got[Ba], got[Bb]
            for (w, pid), (wlo, whi) in win_a.items():
                assert win_b[(w, pid)] == (wlo, whi)                # (the same scalars: the same rows)
                ca, cb = case.column[pid] * Ba + w, case.column[pid] * Bb + w
                xa, xb = ra['coef'][:, ca, wlo:whi], rb['coef'][:, cb, wlo:whi]
                ia, ib = np.searchsorted(rows_a, np.arange(wlo, whi)), np.searchsorted(rows_b, np.arange(wlo, whi))
                for rows_x, ix, res in ((rows_a, ia, ra), (rows_b, ib, rb)):
                    assert ix.max() < rows_x.size and np.array_equal(rows_x[ix], np.arange(wlo, whi)), \
                        f'walker {w} pipeline {pid}: its bins read rows {wlo}..{whi - 1}, the product of B = {res["B"]} computed {res["win"]}'
                # (the P(k,mu) stage chooses its kernel by batch size as well, and its mu rules differ at the 1e-9 level: where the
                # operands differ, what the reference itself makes of the two is allowed on top of the two bounds)
                same_operand = np.array_equal(ra['P'][:, ca], rb['P'][:, cb])
                moved = np.abs(ref_a[:, ca][:, ia] - ref_b[:, cb][:, ib])
                diff = np.abs(xa.astype(LD) - xb.astype(LD))
                assert np.all(diff <= bound_a[:, ca][:, ia] + bound_b[:, cb][:, ib] + moved), (Ba, Bb, w, pid, float(diff.max()))
                if ra['form'] == rb['form'] and same_operand:
                    np.testing.assert_array_equal(xa, xb, err_msg=f'walker {w} pipeline {pid}: B = {Ba} and {Bb} in the same form')
                    bitwise += 1
    assert bitwise > 0
    case.ratios['tiled: rows compared bit for bit'] = bitwise
