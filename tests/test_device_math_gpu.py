"""The hand-written device math functions of the kernels (vega_amd/csrc/vmx_device.h: vmx_log, vmx_exp, vmx_rsqrt) against
np.longdouble, elementwise through vmx_debug_math, about 2 10^5 points per function.  The bars are derived from the
algorithms (below), asserted here, and are what tests/helpers/xi_bins_oracle.py takes as E_LOG, E_EXP and E_RSQRT.
u = 2^-53; "ulp" is the spacing of float64 at the exact value.

vmx_log   the code's own claim: error < 1 ulp of the exact value (the classic s = f / (2 + f) formulation with fdlibm's
          minimax coefficients; an ulp is at most 2 u of the value, which is the oracle's E_LOG).

vmx_exp   n = rint(x log2 e), r = x - n ln2_hi - n ln2_lo, degree-12 Taylor polynomial by Horner, ldexp.  Relative to exp(x),
          worst at r = -ln 2 / 2 (the result's scale is exp(r) >= 0.7071 there):
            reduction    n ln2_hi is exact (ln2_hi has 32 significant bits, |n| < 2^11) and so is x - n ln2_hi (both are
                         multiples of the ulp of x and the difference is below 1/2); the second fma rounds once, u |r| <= 0.35 u;
                         ln2_hi + ln2_lo misses ln 2 by < 2^-86, times |n| <= 1075: 1e-7 u.  rint of the rounded product can pass
                         the half-way point by |x| u: |r| <= (ln 2 / 2)(1 + 1e-13).                                    0.35 u
            truncation   sum_{k >= 13} |r|^k / k! <= (ln 2 / 2)^13 / 13! / (1 - |r| / 14) = 1.671e-16 / 0.9752 for r > 0
                         (relative to exp(r) = 1.414: 1.1 u); for r < 0 the series alternates, the first term bounds it:
                         1.671e-16 / 0.7071 = 2.363e-16                                                               2.13 u
            Horner       the roundings of the inner steps reach the result through the remaining factors of r: the step
                         that forms q1 = (e^r - 1) / r contributes |r| u |q1| = 0.293 u, the one before |r|^2 u |q2| = 0.054 u,
                         the rest 0.007 u: 0.354 u absolute, over 0.7071                                               0.50 u
            coefficients 1/3! ... 1/12! rounded to float64: u (e^|r| - 1 - |r| - r^2 / 2) / 0.7071                      0.02 u
            last fma     one rounding of the result                                                                    1.00 u
          sum 4.00 u = 4.44e-16 (EXP_BAR).  A subnormal result is rounded once more by ldexp: + 2^-1075 absolute.  The header
          comment said "~2e-16", which is the truncation term alone.  Arguments <= -746 give exactly 0 (p 2^n < 2^-1075 rounds
          to zero) down to -1e12, the most negative argument tried (at ~ -1e300 the reduction itself overflows; no kernel passes
          such an argument: the evolution and radiation exponents are sums of a few terms of order 1 to 100).

vmx_rsqrt y = v_rsq_f64(x), documented to 2^29 ulp: y = (1 + e0) / sqrt(x), |e0| <= 2^-23.  e = 1 - (x y) y computed with one
          rounding of x y (u) and one of the fma (2^-22 u): e = e_exact + eta, |eta| <= 1.0000005 u.  The result
          y (1 + e / 2 + 3 e^2 / 8) against y (1 - e_exact)^(-1/2) = y (1 + e/2 + 3 e^2/8 + 5 e^3/16 + ...):
            third-order remainder 5/16 |e|^3 (1 + 2^-20) <= 5/16 2^-66                                                3.8e-5 u
            eta / 2                                                                                                   0.50 u
            roundings of y e and of the inner fma, scaled by |e| <= 2^-22                                              1e-6 u
            last fma                                                                                                   1.00 u
          sum < 1.501 u (RSQRT_BAR), for every normal x whose x y^2 neither overflows nor underflows: nothing in the derivation
          needs x >= 1, and the radiation term's arguments below 1 are served as well as those above (the header comment said
          "for x >= 1").  x = 0 gives NaN (0 times infinity): the radiation term would pass it for a bin with r_par + drp = 0 and
          r_perp = 0, which no grid of bin centres has.
"""
import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2) ** -53
EXP_BAR = 4 * U
RSQRT_BAR = LD(1.501) * U
SEED = 20260803 + 31


@pytest.fixture(scope='module')
def engine():
    from vega_amd import VegaInterface
    assert np.finfo(LD).eps == LD(2) ** -63, 'np.longdouble must carry a 64-bit mantissa (eps 1.08e-19)'
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=1)
    yield vega.engine
    vega.close()


def _ulp(v):
    """The spacing of float64 at |v| (normal range)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(LD(1), e - 53)


def _neighbours(points, steps=4):
    out = [points]
    lo = hi = points
    for _ in range(steps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def test_log(engine):
    rng = np.random.default_rng(SEED)
    centres = 2.0 + 4.0 * np.arange(50)
    grid_r2 = (centres[:, None]**2 + centres[None, :]**2).ravel()
    k = np.arange(-20, 28)
    x = np.concatenate([
        np.concatenate([a * a * grid_r2 for a in (0.9, 0.97, 1.0, 1.03, 1.1)]),           # r'^2 of 4 Mpc/h bins out to 200
        np.exp(rng.uniform(np.log(1e-6), np.log(1e8), 150000)),
        1.0 + rng.uniform(-1, 1, 20000) * 2.0**-30, _neighbours(np.array([1.0]), 64),
        _neighbours(np.sqrt(0.5) * 2.0**k, 8),                                             # both sides of every switch point
        2.0**np.arange(-1022, 1024), _neighbours(2.0**k, 2)])
    x = x[(x > 0) & np.isfinite(x)]
    got = engine.debug_math('log', x)
    exact = np.log(x.astype(LD))
    one = x == 1.0
    assert one.any() and np.all(got[one] == 0.0)
    err = np.abs(got.astype(LD) - exact)[~one] / _ulp(exact[~one])
    worst = int(np.argmax(err))
    print(f'\nDEVICE_MATH log: {x.size} points, largest error {float(err.max()):.4f} ulp at x = {x[~one][worst]!r}')
    assert np.all(err < 1), (x[~one][worst], float(err.max()))


def test_exp(engine):
    rng = np.random.default_rng(SEED + 1)
    odd = np.arange(-2149, 2047, 2)                                                        # odd multiples of ln 2 / 2
    assert np.all(odd % 2 == 1)
    half = (odd.astype(LD) * np.log(LD(2)) / 2).astype(np.float64)
    x = np.concatenate([
        rng.uniform(-745, 709, 120000), _neighbours(half[(half > -745) & (half < 709)], 4),
        rng.uniform(-1, 1, 30000), rng.uniform(-60, 0, 30000),                             # evolution, radiation
        np.array([0.0, -0.0, 1e-300, -1e-300, 709.0, -708.0, -708.5, -740.0, -745.0])])
    got = engine.debug_math('exp', x)
    exact = np.exp(x.astype(LD))
    bar = EXP_BAR * exact + np.where(exact < LD(2) ** -1022, LD(2) ** -1075, 0)
    err = np.abs(got.astype(LD) - exact)
    normal = exact >= LD(2) ** -1022
    worst = int(np.argmax(np.where(normal, err / exact, 0)))
    print(f'\nDEVICE_MATH exp: {x.size} points, largest relative error {float((err / exact)[normal].max() / U):.4f} u '
          f'at x = {x[worst]!r} (bar {float(EXP_BAR / U):.2f} u); subnormal results: largest error '
          f'{float((err[~normal] / LD(2) ** -1074).max()) if (~normal).any() else 0:.3f} of the smallest subnormal')
    bad = int(np.argmax(err - bar))
    assert np.all(err <= bar), (x[bad], got[bad], float(err[bad] / exact[bad] / U))
    zero = np.array([-746.0, -750.0, -800.0, -1e3, -1e4, -1e6, -1e9, -1e12])
    assert np.all(engine.debug_math('exp', zero) == 0.0)
    assert engine.debug_math('exp', np.array([0.0]))[0] == 1.0


def test_rsqrt(engine):
    rng = np.random.default_rng(SEED + 2)
    x = np.concatenate([
        np.exp(rng.uniform(np.log(1e-6), np.log(1e10), 180000)),
        np.exp(rng.uniform(np.log(1e-6), np.log(1.0), 20000)),                             # below 1: the radiation term's r_shift^2
        4.0**np.arange(-10, 17), _neighbours(np.array([1.0, 0.25, 4.0]), 32), 1.0 + rng.uniform(-1, 1, 5000) * 2.0**-30])
    got = engine.debug_math('rsqrt', x)
    exact = 1 / np.sqrt(x.astype(LD))
    rel = np.abs(got.astype(LD) - exact) / exact
    worst = int(np.argmax(rel))
    below = x < 1
    print(f'\nDEVICE_MATH rsqrt: {x.size} points, largest relative error {float(rel.max() / U):.4f} u at x = {x[worst]!r}; '
          f'below 1: {float(rel[below].max() / U):.4f} u, from 1: {float(rel[~below].max() / U):.4f} u (bar {float(RSQRT_BAR / U):.3f} u)')
    assert np.all(rel <= RSQRT_BAR), (x[worst], float(rel.max() / U))
