"""The FFTLog o spline product  coef_ell = OP_ell P_ell  (run_chain -> launch_product(KC_FFTLOG), vega_amd/csrc/vegamx.hip) for
tests/test_fftlog_product_host.py and tests/test_fftlog_product_gpu.py: the host's choice of kernel restated, an
extended-precision reference with its a-priori bound, the coefficient rows a walker's bins read, and seeded walkers.

Shapes: the engine holds four operators OP_ell [n_coef][nkp] (n_coef = nk + 2 rows; nkp = the nk samples - with `fht_extrap`
the nk + pads samples - padded to a multiple of 32 with zero columns), the P(k,mu) stage leaves P [4][ncols][nkp] with
ncols = B n_columns (column-major: index = column B + walker), and the product writes coef [4][ncols][ncp], ncp = n_coef padded
to 32.  Only the rows inside a device window (what the batch's bins can read) are computed; with no pads the MFMA kernels stop
at a device column limit (the live wavenumbers, rounded up to 32).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GEMM_BM = GEMM_BN = 64
VMX_MAX_ELL = 4
E_POW = 16          # ulp of fp64 pow: the ROCm installation states no bound for its device library, so the OpenCL C
                    # specification's (7.4, relative error as ULPs: pow <= 16 ulp) stands in


def pad32(n):
    return (n + 31) // 32 * 32


def gemv1_applies(n, k):
    """vegamx.hip: the single-column streaming kernel keeps x in LDS."""
    return n == 1 and k <= 5120 and k * 8 <= 48 * 1024


def estimate(n_coef, ncols):
    """launch_gemm_group's estimate of the live 64 x 64 tiles: a third of the operator's row tiles, for every walker tile and
    multipole."""
    tm, tn = -(-n_coef // GEMM_BM), -(-ncols // GEMM_BN)
    return tn * VMX_MAX_ELL * ((tm * 3 + 9) // 10)


def expected_form(n_coef, ncols, lanes=1, pads=0):
    """The form launch_product / launch_gemm_group give the FFTLog product of an engine with n_coef coefficient rows (nk =
    n_coef - 2 samples, `pads` power-law pad samples behind them), ncols = B n_columns columns and `lanes` batches in flight: the
    set Engine.fftlog_form() reports.  In the order of the host code: the single-column kernel, the streaming kernels up to
    eight columns (they read whole rows: no column limit), then the MFMA kernels - 64 x 32 tiles where the estimate lies in
    [96, 384], else the four-buffer ring where it lies in [160, 320] and one batch is in flight, else 64 x 64 tiles.  (K is never
    split: the call hands plan_gemm no slab rows.)"""
    k = pad32(n_coef - 2 + pads)
    if gemv1_applies(ncols, k):
        return {'gemv1'}
    if ncols <= 8:
        return {'gemv', 'nb%d' % (1 if ncols == 1 else 2 if ncols == 2 else 4 if ncols <= 4 else 8)}
    ring_allowed = lanes == 1
    form = {'batch_x' if ring_allowed else 'batch_y'} | (set() if pads else {'k_limit'})
    est = estimate(n_coef, ncols)
    if 96 <= est <= 384:
        return form | {'mfma32'}
    if ring_allowed and 160 <= est <= 320:
        return form | {'ring'}
    return form | {'mfma64'}


def form_edges(n_coef):
    """The column counts at which the MFMA form changes: (largest ncols with est < 96, smallest with est >= 96, largest with
    est <= 384, smallest above)."""
    per_tile = estimate(n_coef, 1)
    tn_lo = -(-96 // per_tile)                  # the first walker-tile count inside [96, 384]
    tn_hi = 384 // per_tile                     # ... and the last
    assert tn_lo <= tn_hi, 'no 64 x 32 interval for this operator'
    return (tn_lo - 1) * GEMM_BN, (tn_lo - 1) * GEMM_BN + 1, tn_hi * GEMM_BN, tn_hi * GEMM_BN + 1


def operators(k, lowring=True, extrap=False):
    """The four operators as vega_amd/engine.py makes and uploads them (same calls, same machine: the same bits)."""
    from vega_amd import fftlog_op
    from vega_amd.engine import _f64
    return [_f64(fftlog_op.xi_operator(_f64(k), ell, lowring=lowring, extrap=extrap)[0]) for ell in (0, 2, 4, 6)]


def reference(op, p_rows, rows, cols, k_terms):
    """op [n_coef][>= cols] of one multipole, p_rows [n][>= cols] (or one row [>= cols]) fp64 -> (ref [n][len(rows)] in
    np.longdouble, bound [n][len(rows)]) of  op[rows, :cols] @ P[:cols]:  the a-priori bound of an fp64 sum of k_terms products
    in any order and with any fusing, (k_terms + 2) u (|op| |P|), u = 2^-53 - the sum of absolute products formed in fp64 and
    lowered by its own worst-case rounding (1 - 2 k_terms u), so that the bound used is never above the stated one.  k_terms:
    the operand columns that are not padding (nk, or nk + pads).  Distinct operand rows are multiplied once."""
    p_rows = np.atleast_2d(np.asarray(p_rows, dtype=np.float64))
    rows = np.asarray(rows, dtype=np.int64)
    uniq, inverse = np.unique(p_rows[:, :cols], axis=0, return_inverse=True)
    a = np.ascontiguousarray(op[rows][:, :cols])
    live = np.flatnonzero(np.any(uniq != 0, axis=1))
    ref = np.zeros((uniq.shape[0], rows.size), LD)
    bound = np.zeros((uniq.shape[0], rows.size))
    if live.size and rows.size:
        ref[live] = uniq[live].astype(LD) @ a.astype(LD).T
        bound[live] = ((k_terms + 2) * U * (1 - 2 * k_terms * U)) * (np.abs(uniq[live]) @ np.abs(a).T)
    inverse = np.ravel(inverse)
    return ref[inverse], bound[inverse]


def bins_window(static, scalars, index):
    """The half-open range [lo, hi) of coefficient rows the bins of one walker and pipeline read, from what
    tests/helpers/xi_bins_oracle.py computes on the way (xi_bins: parts['window'], the cells of the bins' ln r' and the four taps
    of each) - not from the prologue's formula.  static: (Desc, static arrays, grid) of the pipeline as the engine's taps give
    them; scalars: the walker's row of Engine.bins_scalars; index: Engine.bins_scalar_index()."""
    from helpers import xi_bins_oracle as xo
    desc, st, grid = static
    zeros = np.zeros((4, grid['n_coef']))
    return xo.xi_bins(desc, st, grid, scalars, index, zeros, raw=True)[3]['window']


# ---------------------------------------------------------------------------------------------------------------------
# walkers: every one of a batch distinct (a swapped walker tile must show), seeded, inside the mu rule's box
# ---------------------------------------------------------------------------------------------------------------------
SMOOTHING = ('par_sigma_smooth', 'per_sigma_smooth')
WEAK, STRONG = 0.3, 10.0        # smoothing lengths: the box of the mu rule is [0, 10] (vega_amd/mu_quadrature.py: RULE_BOX);
                                # 0.3 keeps exp(-(k sigma)^2 / 2) alive ~ 33 times further in k than 10 does


def walkers(theta0, slot, batch, spread, seed, smoothing=None):
    """theta [batch][n_params]: every walker its own ap, at (narrow: within 2 % of the base; wide: over [0.55, 1.45] with
    both extremes in the batch - walkers 0 and 1 - and delta_rp over +- 25 where the problem has one) and its own Kaiser
    parameters (bias_eta_LYA, beta_LYA within 5 %: every P_ell row of the batch differs).  smoothing: None (as the base), a
    number (both lengths, shared by the batch: the tabulated P(k,mu) kernels where the engine has them) or (lo, hi) (per
    walker, uniform: the kernels that exponentiate per walker)."""
    rng = np.random.default_rng(seed)
    theta = np.tile(np.asarray(theta0, dtype=np.float64), (batch, 1))
    if spread == 'narrow':
        theta[:, slot['ap']] *= 1 + rng.uniform(-0.02, 0.02, batch)
        theta[:, slot['at']] *= 1 + rng.uniform(-0.02, 0.02, batch)
        if 'drp_QSO' in slot:
            theta[:, slot['drp_QSO']] += rng.uniform(-0.5, 0.5, batch)
    else:
        assert spread == 'wide'
        theta[:, slot['ap']] = rng.uniform(0.55, 1.45, batch)
        theta[:, slot['at']] = rng.uniform(0.55, 1.45, batch)
        theta[0, slot['ap']] = theta[0, slot['at']] = 0.55
        if batch > 1:
            theta[1, slot['ap']] = theta[1, slot['at']] = 1.45
        if 'drp_QSO' in slot:
            theta[:, slot['drp_QSO']] = rng.uniform(-25.0, 25.0, batch)
    for name in ('bias_eta_LYA', 'beta_LYA'):
        if name in slot:
            theta[:, slot[name]] *= 1 + rng.uniform(-0.05, 0.05, batch)
    if smoothing is not None:
        for name in SMOOTHING:
            if name in slot:
                theta[:, slot[name]] = smoothing if np.isscalar(smoothing) else rng.uniform(smoothing[0], smoothing[1], batch)
    return theta


def pk_tile(batch):
    """What every P(k,mu) launch shape of run_chain guarantees of its k tile from the batch size alone (an engine has at
    least one group of each kind it launches): B x groups >= 24 takes the 64-wide shapes of k_pk_multipoles, k_pk_tab2 and
    k_pk_w; >= 4 the 16-wide ones (or wider); below, 8-wide tiles can run.  The live limit is a multiple of the value returned, or
    nk."""
    return 64 if batch >= 24 else 16 if batch >= 4 else 8
