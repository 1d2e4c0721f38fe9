"""tests/helpers/fftlog_product.py without a device: the host's choice of the FFTLog product's kernel restated (expected_form)
at the edges of its intervals, the oracle's bound against fp64 sums in other orders (and that it bites), the walkers, and the
bins' window.

With nk = 814 (every golden template): n_coef = 816, 13 row tiles, est = 16 ceil(ncols / 64) - streaming kernels up to 8
columns, 64 x 64 tiles for 9 ... 320 and from 1537, 64 x 32 tiles for 321 ... 1536.  The four-buffer ring's interval [160, 320]
lies inside the 64 x 32 interval [96, 384], which launch_gemm_group tests first, and K is never split for this call (it hands
plan_gemm no slab rows): no column count reaches the ring.
"""
import time

import numpy as np
import pytest

from conftest import GOLDEN, load_problem
from helpers import fftlog_product as fp

LD = np.longdouble
N_COEF = 816


def test_expected_form_at_the_interval_edges():
    x, y = {'batch_x', 'k_limit'}, {'batch_y', 'k_limit'}
    assert fp.estimate(N_COEF, 64) == 16 and fp.estimate(N_COEF, 65) == 32
    assert fp.form_edges(N_COEF) == (320, 321, 1536, 1537)
    want = {1: {'gemv1'}, 2: {'gemv', 'nb2'}, 3: {'gemv', 'nb4'}, 4: {'gemv', 'nb4'}, 5: {'gemv', 'nb8'}, 6: {'gemv', 'nb8'},
            8: {'gemv', 'nb8'}, 9: x | {'mfma64'}, 10: x | {'mfma64'}, 64: x | {'mfma64'}, 65: x | {'mfma64'},
            320: x | {'mfma64'}, 321: x | {'mfma32'}, 352: x | {'mfma32'}, 386: x | {'mfma32'}, 1536: x | {'mfma32'},
            1537: x | {'mfma64'}, 4096: x | {'mfma64'}}
    for ncols, form in want.items():
        assert fp.expected_form(N_COEF, ncols) == form, ncols
        if ncols > 8:
            assert fp.expected_form(N_COEF, ncols, lanes=2) == (form - x) | y, ncols
        else:
            assert fp.expected_form(N_COEF, ncols, lanes=2) == form, ncols
    # fht_extrap: 1234 pad samples, K = 2048 - no column limit, the same intervals (they count row and walker tiles only)
    assert fp.pad32(814 + 1234) == 2048
    assert fp.expected_form(N_COEF, 2, pads=1234) == {'gemv', 'nb2'}
    assert fp.expected_form(N_COEF, 10, pads=1234) == {'batch_x', 'mfma64'}
    assert fp.expected_form(N_COEF, 322, pads=1234) == {'batch_x', 'mfma32'}
    # a single column leaves k_gemv1 for k_gemv<1> above 5120 operand columns
    assert fp.expected_form(5200, 1) == {'gemv', 'nb1'} and fp.expected_form(5100, 1) == {'gemv1'}


def test_form_bits_are_the_headers():
    """Engine.FFTLOG_FORM_BITS against the VMX_FFT_* enum of include/vegamx.h (vmx_debug_read 4 [10])."""
    import re
    from conftest import REPO
    from vega_amd.engine import Engine
    header = (REPO / 'include' / 'vegamx.h').read_text()
    enum = {name.lower(): int(value) for name, value in re.findall(r'VMX_FFT_([A-Z0-9_]+) = (\d+)', header)}
    assert enum.pop('nb_shift') == 8
    assert enum == Engine.FFTLOG_FORM_BITS and all(bit < 1 << 8 for bit in enum.values())


def test_no_size_reaches_the_ring():
    """launch_gemm_group asks for 64 x 32 tiles (est in [96, 384]) before it asks for the ring (est in [160, 320])."""
    for n_coef in (64, 65, 200, 816, 817, 2050, 4098, 9000):
        for lanes in (1, 2):
            forms = [fp.expected_form(n_coef, ncols, lanes) for ncols in range(1, 6000)]
            assert not any('ring' in f for f in forms), n_coef
            assert any('mfma32' in f for f in forms) or fp.estimate(n_coef, 1) > 384, n_coef


@pytest.fixture(scope='module')
def operands():
    """A real operator set and the CPU reference's own P_ell of the golden auto-correlation (peak and smooth), with the
    model's smoothing: the samples die out well before the last wavenumber."""
    assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'
    from oracle import vega_cpu as oc
    prob = load_problem('auto')
    taps = {}
    oc.compute_model(prob, {}, taps=taps)
    ops = fp.operators(prob.k)
    rows = np.stack([np.asarray(taps['lyalya_lyalya'][c]['pk_ell'][ell], dtype=np.float64) for c in ('peak', 'smooth') for ell in (0, 2, 4, 6)])
    return np.asarray(prob.k).size, ops, rows.reshape(2, 4, -1)


def test_fp64_sums_in_other_orders_stay_inside_the_bound(operands):
    nk, ops, p = operands
    assert ops[0].shape == (nk + 2, nk) and p.shape == (2, 4, nk)
    rng = np.random.default_rng(5)
    rows = np.arange(nk + 2)
    worst = 0.0
    for e in range(4):
        t0 = time.perf_counter()
        ref, bound = fp.reference(ops[e], p[:, e], rows, nk, nk)
        seconds = time.perf_counter() - t0
        assert ref.dtype == LD and ref.shape == bound.shape == (2, nk + 2) and np.all(bound > 0)
        print(f'\nFFTLOG_REFERENCE_RATE ell={2 * e} {2 * rows.size * nk / seconds:.3g} multiply-adds / s')
        for c in range(2):
            terms = ops[e] * p[c, e][None, :]                       # the fp64 products, one rounding each
            order = rng.permutation(nk)
            shuffled = np.zeros(nk + 2)
            for j in order:                                         # one running sum in a shuffled order
                shuffled = shuffled + terms[:, j]
            lanes = [np.zeros(nk + 2) for _ in range(4)]
            for j in range(nk):                                     # four interleaved partial sums, added at the end
                lanes[j % 4] = lanes[j % 4] + terms[:, j]
            four = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])
            blas = ops[e] @ p[c, e]
            for what, got in (('shuffled', shuffled), ('four', four), ('blas', blas)):
                err = np.abs(got.astype(LD) - ref[c])
                assert np.all(err <= bound[c]), (what, e, c, float((err / bound[c]).max()))
                worst = max(worst, float((err / bound[c]).max()))
    print(f'FFTLOG_HOST_RATIO {worst:.3g}')
    assert worst < 0.2                  # (a bound of K u against random rounding of ~ sqrt(K) u: the margin a real kernel has)


def test_the_bound_bites(operands):
    """What the device checks must see: a dropped K stage (the column limit rounded down), a row taken from its neighbour (a
    window or tile off by one), and another walker's operand."""
    nk, ops, p = operands
    rows = np.arange(nk + 2)
    last = int(np.flatnonzero(p[0, 0])[-1]) + 1
    assert 64 < last < nk                                           # (the smoothing leaves exact zeros behind the live samples)
    ref, bound = fp.reference(ops[0], p[0, 0], rows, nk, nk)
    good = ops[0] @ p[0, 0]
    stage = int(np.argmax(np.abs(p[0, 0]))) // 32 * 32
    keep = np.ones(nk, bool)
    keep[stage:stage + 32] = False
    dropped = ops[0][:, keep] @ p[0, 0][keep]
    for what, got in (('dropped stage', dropped), ('shifted rows', np.roll(good, 1)), ('other operand', ops[0] @ p[1, 0])):
        err = np.abs(got.astype(LD) - ref[0])
        assert np.any(err > bound[0]), what
    # ... and what they cannot see: the samples just below the live limit are the underflowing tail of the smoothing's
    # Gaussian (|P| < 1e-30 of the row's largest), so the LAST K stage carries less than the bound - the column limit is held by
    # the test of the zeros behind it and of its rounding, not by the product
    tail = ops[0][:, :last // 32 * 32 - 32] @ p[0, 0][:last // 32 * 32 - 32]
    assert np.all(np.abs(tail.astype(LD) - ref[0]) <= bound[0])
    assert np.abs(p[0, 0][last // 32 * 32 - 32:]).max() < 1e-30 * np.abs(p[0, 0]).max()
    # columns past the last live sample are exact zeros: a product cut there is the same product
    cut, cut_bound = fp.reference(ops[0], p[0, 0], rows, fp.pad32(last), nk)
    assert np.array_equal(cut, ref) and np.array_equal(cut_bound, bound)
    # an unused multipole's row of zeros: reference and bound are exact zeros
    zero, zero_bound = fp.reference(ops[0], np.zeros((3, nk)), rows[:5], nk, nk)
    assert not zero.any() and not zero_bound.any() and zero.shape == (3, 5)


def test_walkers_are_distinct_and_inside_the_box():
    from vega_amd.mu_quadrature import rule_box
    prob = load_problem('joint')
    names = sorted(prob.params)
    slot = {n: i for i, n in enumerate(names)}
    theta0 = np.array([prob.params[n] for n in names])
    box = rule_box(names)
    assert set(fp.SMOOTHING) <= set(box) and all(box[n][0] <= fp.WEAK < fp.STRONG <= box[n][1] for n in fp.SMOOTHING)
    for spread, smoothing in (('narrow', fp.WEAK), ('narrow', (6.0, fp.STRONG)), ('wide', None), ('wide', fp.STRONG)):
        theta = fp.walkers(theta0, slot, 70, spread, seed=3, smoothing=smoothing)
        assert np.unique(theta, axis=0).shape[0] == 70
        for name, (lo, hi) in box.items():
            assert np.all((theta[:, slot[name]] >= lo) & (theta[:, slot[name]] <= hi)), name
        ap, at = theta[:, slot['ap']], theta[:, slot['at']]
        if spread == 'wide':
            assert ap.min() == at.min() == 0.55 and ap.max() == at.max() == 1.45 and np.abs(theta[:, slot['drp_QSO']]).max() > 20
        else:
            assert np.all(np.abs(ap / theta0[slot['ap']] - 1) <= 0.02) and np.all(np.abs(at / theta0[slot['at']] - 1) <= 0.02)
        assert np.unique(theta[:, slot['beta_LYA']]).size == 70
    assert np.array_equal(fp.walkers(theta0, slot, 9, 'wide', seed=4), fp.walkers(theta0, slot, 9, 'wide', seed=4))
    assert [fp.pk_tile(b) for b in (1, 3, 4, 23, 24, 64)] == [8, 8, 16, 16, 64, 64]


def test_bins_window_is_the_oracles(tmp_path):
    """bins_window against the window of a full oracle evaluation, and the dilation moves it."""
    from helpers import xi_bins_oracle as xo
    prob = xo.build_case(tmp_path, 'a63', GOLDEN)
    got = {}
    for alpha in (0.55, 1.0, 1.45):
        o = xo.host_operands(prob, {'ap': alpha, 'at': alpha})[('lyalya_lyalya', 'peak')]       # (the smooth component is not rescaled here)
        full = xo.xi_bins(o['desc'], o['st'], o['grid'], o['sc'], o['ix'], o['coef'], terms=o['terms'])[3]['window']
        got[alpha] = fp.bins_window((o['desc'], o['st'], o['grid']), o['sc'], o['ix'])
        assert got[alpha] == full and 0 <= full[0] < full[1] <= o['grid']['n_coef']
    assert got[0.55][0] < got[1.0][0] < got[1.45][0] and got[0.55][1] < got[1.0][1] < got[1.45][1]
