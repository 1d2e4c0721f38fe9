"""The spline-bins stage restated in np.longdouble from the kernels' own operands, with an a-priori error bound per bin,
and a float64 twin of the kernel arithmetic with named mutations (tests/test_xi_bins_host.py, tests/test_xi_bins_gpu.py).

What a bin's value is (vega_amd/csrc/vmx_device.h: xi_bin_value, xi_plain_spline; the same arithmetic is copied into
k_xi_bins<false>, k_xi_bins_lean, k_xi_bins_group, k_xi_assemble_quad and k_xi_quad_plain):

    r_par' = ap (r_par + drp),  r_perp' = at r_perp,  r'^2 = r_par'^2 + r_perp'^2,  x = ln(r'^2) / 2,  mu' = r_par' / r'
    per multipole:  u = (x - x0) / h,  j = clamp(floor u, 0, n_coef - 4),  t = u - j,
                    s = (c[j] (1 - t)^3 + c[j+1] (3 t^3 - 6 t^2 + 4) + c[j+2] (-3 t^3 + 3 t^2 + 3 t + 1) + c[j+3] t^3) / 6
    xi = sum_ell s_ell L_ell(mu')      (single_ell: xi = s of that multipole, no Legendre factor)
    xi *= evolution x growth;  + radiation (smooth component only)

The operands are what the engine's taps return (Engine.bins_static, bins_scalars, bins_grid, bins_coefficients): every one of
them is a float64 the kernel reads, so the restatement is exact up to longdouble rounding (eps 1.08e-19) and the only
error left to bound is the kernel's own.  The oracle divides by h; the kernels multiply by the stored 1 / h.

THE BOUND, term by term, u = 2^-53 (one rounding is a relative error of at most u).  Every operation is counted as a
rounding of its own, a fused multiply-add as two (product, sum): the kernels' fma calls and the compiler's contractions
only remove roundings, and the float64 twin below, which has no fused operation, is covered by the same count.

  coordinates   r_par' : r_par + drp (1), times ap (1)                      -> 2 u relative
                r_perp': at r_perp (1)                                      -> 1 u
                r'^2   : squares double the inputs, each square (1), sum (1) -> max(2 * 2 + 1, 2 * 1 + 1) + 1 = 6 u
  x             d ln = relative error of r'^2, halved, + the logarithm      -> dx = 3 u + E_LOG |ln r'^2| / 2
  mu'           r_par' (2 u), rsqrt of r'^2 (3 u + E_RSQRT), product (1)    -> dmu = (6 u + E_RSQRT) |mu'|
  knot          x - x0 (1), the stored 1 / h (1), product (1); t = u - floor(u) is exact
                                                                            -> du = (dx + u |x - x0|) / h + 2 u |u|
  spline        a cubic B-spline's derivative is a convex combination of coefficient differences, so an error du of the knot
                coordinate - an index that flips at a cell edge included - moves s by at most
                max |c[q+1] - c[q]| du, q over the six coefficients around the cell (outside [0, 1], polynomial extension of
                the end cells under `extrapolate`, by sum |c_q| |w_q'(t)| / 6 du instead)
  weights       t2 = t t (1), t3 = t2 t (2), 1 - t (1):
                w0 = (1 - t)^3                       3 u from 1 - t, two products   -> 5 u |w0|
                w1 = 3 t3 - 6 t2 + 4                 3 u |3 t3| + 2 u |6 t2| + u |3 t3 - 6 t2| + u |w1|
                w2 = -3 t3 + 3 t2 + 3 t + 1          3 u |3 t3| + 2 u |3 t2| + u |3 t2 - 3 t3| + u |3 t| + u |3 t2 - 3 t3 + 3 t| + u |w2|
                w3 = t3                              2 u |w3|
  spline sum    four products (1 each), three additions (<= 3 on a term), the constant 1/6 (1) and its product (1)
                                                                            -> (sum |c_q| dw_q + 6 u sum |c_q w_q|) / 6
  Legendre      |L'(mu')| dmu, + the rounding of the polynomial in mu'^2 by a running error bound of the kernel's
                Horner steps (a product and an addition per step, mu'^2 itself rounded once)
  Legendre sum  one product per multipole, at most n_ell - 1 additions      -> n_ell u sum |s_ell L_ell|
  evolution     standard: arg = (a1 + a2) ln z: (2) -> 2 u |arg|; split: a1 ln z1 (1) + a2 ln z2 (1), sum (1) -> 2 u (|a1 ln z1| + |a2 ln z2|);
                relative (E_EXP + darg); Croom and pow: see _evolution
  tail          xi ev (1), times growth (1)  [the lean forms: ev growth (1), xi times it (1)]  -> 2 u
  radiation     see _radiation; its sum with xi (1)

E_LOG, E_EXP and E_RSQRT are the bars of tests/test_device_math_gpu.py (derived there, asserted on the device).
"""
import numpy as np

LD = np.longdouble
U = LD(2) ** -53
E_LOG = 2 * U                   # vmx_log: error < 1 ulp of the exact value; an ulp is at most 2 u of the value
E_EXP = 4 * U                   # vmx_exp: tests/test_device_math_gpu.py, EXP_BAR
E_RSQRT = LD(1.501) * U         # vmx_rsqrt: tests/test_device_math_gpu.py, RSQRT_BAR

MUTATIONS = ('knot_plus_one', 'w1_digit', 'w2_digit', 'l4_34', 'l6_230', 'mu_unrescaled', 'lnrelz_swapped',
             'surplus_walker', 'radiation_on_peak')


class Desc:
    """What the bins kernels read of a pipeline's descriptor."""

    def __init__(self, n_ell, single_ell=-1, split_evol=False, evol=(0, 0), z_eff=0.0, radiation=0, is_peak=False, same_tracer=False, additive=False):
        self.same_tracer, self.additive = bool(same_tracer), bool(additive)      # additive: UV shot noise or odd multipoles
        self.n_ell, self.single_ell, self.split_evol = int(n_ell), int(single_ell), bool(split_evol)
        self.evol, self.z_eff, self.radiation, self.is_peak = tuple(int(e) for e in evol), float(z_eff), int(radiation), bool(is_peak)

    @classmethod
    def from_engine(cls, eng, pid):
        d = eng.pipe_descs[pid]
        return cls(d.n_ell, d.single_ell, eng.bins_grid(pid)['split_evol'], (d.tracer[0].evol_kind, d.tracer[1].evol_kind),
                   d.z_eff, d.radiation, bool(d.is_peak), bool(d.same_tracer), bool(d.uv_shotnoise) or eng.bins_grid(pid)['odd_ncoef'] > 0)

    @classmethod
    def from_pipe(cls, prob, pipe, component):
        xi = pipe.xi
        evol = tuple(int(xi.evol_model.get(t.name, 'standard') == 'croom') for t in (pipe.tracer1, pipe.tracer2))
        return cls(xi.ell_max // 2 + 1, xi.single_multipole // 2 if xi.single_multipole >= 0 else -1,
                   getattr(pipe, 'rel_z_evol_1', None) is not None, evol, prob.z_eff,
                   int(xi.radiation) * (2 if xi.rescale_coords_systematics else 1), component == 'peak',
                   additive=bool(xi.uv_shotnoise or xi.relativistic or xi.asymmetry))


def _scalar_names():
    from vega_amd.engine import Engine
    return Engine.BINS_SCALAR_NAMES


HOST_INDEX = dict({n: i for i, n in enumerate(_scalar_names())}, NS=len(_scalar_names()))


def host_static(pipe):
    """The per-bin static arrays from a Problem's pipeline (host tests: the engine's taps return what it uploaded)."""
    r, mu = np.asarray(pipe.r, float), np.asarray(pipe.mu, float)
    relz = np.asarray(pipe.rel_z_evol, float) * np.ones_like(r)
    relz1 = getattr(pipe, 'rel_z_evol_1', None)
    relz2 = getattr(pipe, 'rel_z_evol_2', None)
    out = dict(r=r, rp=r * mu, rt=r * np.sqrt(1 - mu**2), z=np.asarray(pipe.z, float) * np.ones_like(r), relz=relz,
               lnrelz=np.log(relz if relz1 is None else np.asarray(relz1, float)),
               growth=np.asarray(pipe.xi_growth, float) * np.ones_like(r))
    out['lnrelz2'] = out['lnrelz'] if relz2 is None else np.log(np.asarray(relz2, float))
    return out


def host_scalars(prob, pipe, params, component):
    """A walker's scalars for the bins, as k_prologue forms them from the parameters (float64, HOST_INDEX order)."""
    from oracle import vega_cpu as oc
    pars = dict(params, peak=component == 'peak')
    ap, at = oc.get_ap_at(prob.scale, pars, corr_name=pipe.corr_name, metal_corr=pipe.metal_corr)
    s = np.zeros(HOST_INDEX['NS'])
    s[HOST_INDEX['AP']], s[HOST_INDEX['AT']] = ap, at
    s[HOST_INDEX['DRP']] = pars.get(pipe.delta_rp_name, 0.0) if pipe.delta_rp_name is not None else 0.0
    for q, tr in enumerate((pipe.tracer1, pipe.tracer2)):
        if pipe.xi.evol_model.get(tr.name, 'standard') == 'croom':
            s[HOST_INDEX[f'EV{q + 1}A']], s[HOST_INDEX[f'EV{q + 1}B']] = pars['croom_par0'], pars['croom_par1']
        else:
            s[HOST_INDEX[f'EV{q + 1}A']] = pars[f'alpha_{tr.name}']
    if pipe.xi.radiation:
        for key, name in (('RAD_S', 'strength'), ('RAD_A', 'asymmetry'), ('RAD_L', 'lifetime'), ('RAD_D', 'decrease')):
            s[HOST_INDEX[key]] = pars['qso_rad_' + name]
        s[HOST_INDEX['RAD_IL']], s[HOST_INDEX['RAD_ID']] = 1.0 / s[HOST_INDEX['RAD_L']], 1.0 / s[HOST_INDEX['RAD_D']]
    return s


# ---------------------------------------------------------------------------------------------------------------------
# extended precision, with the bound
# ---------------------------------------------------------------------------------------------------------------------
LEGENDRE = {0: [1.0], 1: [-0.5, 1.5], 2: [0.375, -3.75, 4.375], 3: [-0.3125, 6.5625, -19.6875, 14.4375]}   # in y = mu^2, ascending


def _legendre(e, mu, dmu):
    """(L_2e(mu), bound on the kernel's error of it): |L'| dmu + the rounding of the kernel's Horner form in y = mu^2,
    scale (((a3 y + a2) y + a1) y + a0) with integer a and a power-of-two scale (exact): per step a product (1) and an
    addition (1), y rounded once."""
    if e == 0:
        return np.ones_like(mu), np.zeros_like(mu)
    kernel = {1: (0.5, [3.0, -1.0]), 2: (0.125, [35.0, -30.0, 3.0]), 3: (0.0625, [231.0, -315.0, 105.0, -5.0])}[e]
    scale, a = LD(kernel[0]), [LD(c) for c in kernel[1]]
    y = mu * mu
    p, err, dp = a[0] * np.ones_like(y), np.zeros_like(y), np.zeros_like(y)      # value, rounding bound, d/dy
    dy = U * y
    for c in a[1:]:
        dp = dp * y + p
        prod = p * y
        err = err * y + np.abs(p) * dy + U * np.abs(prod)       # the step's inherited error, y's rounding, the product
        p = prod + c
        err = err + U * np.abs(p)                                # the addition
    value, slope = scale * p, scale * dp * 2 * mu                # dL/dmu = dL/dy 2 mu
    return value, np.abs(slope) * dmu + scale * err


def _spline(c, x, dx, x0, h, n_coef, dc=None):
    """(s, bound, u) of one multipole: c [n_coef] (dc: the kernel's error of each coefficient it forms itself), x [n] longdouble."""
    cl = c.astype(LD)
    u = (x - LD(x0)) / LD(h)
    j = np.clip(np.floor(u).astype(np.int64), 0, n_coef - 4)
    t = u - j
    du = (dx + U * np.abs(x - LD(x0))) / LD(h) + 2 * U * np.abs(u)
    t2, t3, omt = t * t, t * t * t, 1 - t
    w = [omt**3, 3 * t3 - 6 * t2 + 4, -3 * t3 + 3 * t2 + 3 * t + 1, t3]
    dw = [5 * U * np.abs(w[0]),
          U * (3 * np.abs(3 * t3) + 2 * np.abs(6 * t2) + np.abs(3 * t3 - 6 * t2) + np.abs(w[1])),
          U * (3 * np.abs(3 * t3) + 2 * np.abs(3 * t2) + np.abs(3 * t2 - 3 * t3) + np.abs(3 * t) + np.abs(3 * t2 - 3 * t3 + 3 * t) + np.abs(w[2])),
          2 * U * np.abs(w[3])]
    taps = [cl[j + q] for q in range(4)]
    s = sum(taps[q] * w[q] for q in range(4)) / 6
    mag = sum(np.abs(taps[q] * w[q]) for q in range(4))
    rounding = (sum(np.abs(taps[q]) * dw[q] for q in range(4)) + 6 * U * mag) / 6
    if dc is not None:
        rounding = rounding + sum(np.abs(w[q]) * dc[j + q] for q in range(4)) / 6
    # the knot coordinate: the six coefficients around the cell
    diffs = np.abs(np.diff(cl))
    lo, hi = np.clip(j - 1, 0, n_coef - 2), np.clip(j + 3, 0, n_coef - 2)       # differences q = j - 1 ... j + 3
    slope = np.zeros_like(u)
    for q in range(5):
        slope = np.maximum(slope, diffs[np.clip(lo + q, lo, hi)])
    outside = (t < 0) | (t > 1)
    if np.any(outside):
        wp = [-3 * omt**2, 9 * t2 - 12 * t, -9 * t2 + 6 * t + 3, 3 * t2]
        ext = sum(np.abs(taps[q] * wp[q]) for q in range(4)) / 6
        slope = np.where(outside, np.maximum(slope, ext), slope)
    return s, rounding + slope * du, u


def _evolution(desc, st, sc, ix):
    """(evolution x growth, relative bound of the kernel's product xi -> xi ev growth, tail roundings included)."""
    lnz, lnz2, growth = st['lnrelz'].astype(LD), st['lnrelz2'].astype(LD), st['growth'].astype(LD)
    a1, a2 = LD(sc[ix['EV1A']]), LD(sc[ix['EV2A']])
    if desc.evol == (0, 0):
        if desc.split_evol:
            arg, darg = a1 * lnz + a2 * lnz2, 2 * U * (np.abs(a1 * lnz) + np.abs(a2 * lnz2))
        else:
            arg = (a1 + a2) * lnz
            darg = 2 * U * np.abs(arg)
        return np.exp(arg) * growth, E_EXP + darg + 2 * U
    # the general kernel's loop over the tracers: Croom (a + c (1 + z)^2) / (a + c (1 + z_eff)^2), or pow(rel z, a)
    ev, rel = np.ones_like(lnz), np.zeros_like(lnz)
    z1, ze = 1 + st['z'].astype(LD), 1 + LD(desc.z_eff)
    for q in range(2):
        a, c = LD(sc[ix[f'EV{q + 1}A']]), LD(sc[ix[f'EV{q + 1}B']])
        if desc.evol[q] == 1:
            # 1 + z (1), its square (1), times c (1): 3 u on the second term; the sum (1); the same below; the quotient (1)
            num, den = a + c * z1 * z1, a + c * ze * ze
            rel = rel + (3 * U * np.abs(c * z1 * z1) + U * np.abs(num)) / np.abs(num) + (3 * U * abs(c * ze * ze) + U * abs(den)) / abs(den) + U
            ev = ev * num / den
        else:
            # pow of the device library: 1 ulp (2 u) of a value whose exponent a ln(rel z) the oracle takes from rel z itself
            ev = ev * np.exp(a * np.log(st['relz'].astype(LD)))
            rel = rel + 2 * U
        rel = rel + U                                            # ev *= ...
    return ev * growth, rel + 2 * U


def _radiation(desc, st, sc, ix):
    """(xi_rad, bound): the QSO radiation term as every form writes it.
      rp = r_par + drp (1)   [rescaled: ap (r_par + drp) + drp: 2 u |ap (r_par + drp)| + u |rp|];  rt = r_perp [rescaled: at r_perp (1)]
      rs2 = rp rp + rt rt: 2 |rp| d(rp) + u rp^2 + (2 rel(rt) + 1) u rt^2 + u rs2;  irs = rsqrt(rs2): rel(rs2) / 2 + E_RSQRT
      rs = rs2 irs (1);  ms = rp irs (1);  amplitude S irs^2 (1 - A (1 - ms^2)): irs^2 (1), ms^2 (1), 1 - (1), A x (1), 1 - (1), S x (1), x (1)
      exponent -rs ((1 + ms) IL + ID): 1 + ms (1), product (1), sum (1), x (1);  exp: E_EXP + the exponent's error;  amplitude x exp (1)"""
    rp0, rt0 = st['rp'].astype(LD), st['rt'].astype(LD)
    ap, at, drp = LD(sc[ix['AP']]), LD(sc[ix['AT']]), LD(sc[ix['DRP']])
    S, A, IL, ID = (LD(sc[ix[k]]) for k in ('RAD_S', 'RAD_A', 'RAD_IL', 'RAD_ID'))
    if desc.radiation == 2:
        inner = ap * (rp0 + drp)
        rp, d_rp = inner + drp, 2 * U * np.abs(inner) + U * np.abs(inner + drp)
        rt, rel_rt = at * rt0, U
    else:
        rp, rt, rel_rt = rp0 + drp, rt0, LD(0)
        d_rp = U * np.abs(rp)
    rs2 = rp * rp + rt * rt
    d_rs2 = 2 * np.abs(rp) * d_rp + U * rp * rp + (2 * rel_rt + U) * rt * rt + U * rs2
    irs = 1 / np.sqrt(rs2)
    rel_irs = d_rs2 / rs2 / 2 + E_RSQRT
    rs, rel_rs = rs2 * irs, d_rs2 / rs2 + rel_irs + U
    ms = rp * irs
    d_ms = irs * d_rp + np.abs(ms) * (rel_irs + U)
    one = 1 - ms * ms
    d_one = 2 * np.abs(ms) * d_ms + U * ms * ms + U * np.abs(one)
    brk = 1 - A * one
    d_brk = np.abs(A) * d_one + U * np.abs(A * one) + U * np.abs(brk)
    amp = S * irs * irs * brk
    d_amp = np.abs(S * irs * irs) * d_brk + np.abs(amp) * (2 * rel_irs + 3 * U)
    opm = 1 + ms
    d_opm = d_ms + U * np.abs(opm)
    f = opm * IL + ID
    d_f = np.abs(IL) * d_opm + U * np.abs(opm * IL) + U * np.abs(f)
    arg = -rs * f
    d_arg = np.abs(rs) * d_f + np.abs(arg) * (rel_rs + U)
    ex = np.exp(arg)
    xr = amp * ex
    return xr, ex * d_amp + np.abs(xr) * (E_EXP + d_arg + U)


def kaiser(desc, sc, ix):
    """(a [3], da [3]): the Kaiser coefficients of a static-basis pipeline as kaiser_coefficients forms them, with the kernel's
    error: a0 = c01 c02 (1), a1 = c01 c12 + c11 c02 (product, product, sum), a2 = c11 c12 (1)."""
    c01, c11 = LD(sc[ix['BIAS1']]), LD(sc[ix['BB1']])
    c02, c12 = (c01, c11) if desc.same_tracer else (LD(sc[ix['BIAS2']]), LD(sc[ix['BB2']]))
    a = [c01 * c02, c01 * c12 + c11 * c02, c11 * c12]
    return a, [U * abs(a[0]), U * (abs(c01 * c12) + abs(c11 * c02)) + U * abs(a[1]), U * abs(a[2])]


def kaiser_combination(a, da, y):
    """a2 y2 + (a1 y1 + a0 y0) as the kernels write it (fma(a2, y2, fma(a1, y1, a0 y0))), y [3][...] exact operands: per step the
    coefficient's error, the product (1) and the sum (1)."""
    y = [np.asarray(v).astype(LD) for v in y]
    t0 = a[0] * y[0]
    s1 = a[1] * y[1] + t0
    s2 = a[2] * y[2] + s1
    bound = (np.abs(y[0]) * da[0] + U * np.abs(t0)) + (np.abs(y[1]) * da[1] + U * np.abs(a[1] * y[1]) + U * np.abs(s1)) + \
            (np.abs(y[2]) * da[2] + U * np.abs(a[2] * y[2]) + U * np.abs(s2))
    return s2, bound


def static_bins(desc, st, sc, ix, y):
    """k_xi_bins_static, _static_nw and a member of _static_group: the Kaiser combination of the basis on the bins y [3, n]
    (vmx_debug_read 12), times evolution and growth: (xi, bound)."""
    a, da = kaiser(desc, sc, ix)
    v, dv = kaiser_combination(a, da, y)
    ev, rel = _evolution(desc, st, sc, ix)
    return v * ev, dv * np.abs(ev) + np.abs(v * ev) * rel


def poly_bins(desc, st, grid, basis):
    """k_poly_bins: the spline and Legendre sums of the three basis vectors (basis [4, 3, >= n_coef], vmx_debug_read 15) at the
    bins' own (r, mu) - unit scales, no delta_rp, the library logarithm (1 ulp, as E_LOG): (Y [3, n], bound [3, n], out of range)."""
    unit = {'AP': 0, 'AT': 1, 'DRP': 2}
    out = [xi_bins(desc, st, grid, np.array([1.0, 1.0, 0.0]), unit, basis[:, i], raw=True) for i in range(3)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), out[0][2] | out[1][2] | out[2][2]


def _shot_noise(terms, r, rr2, d_rr2_rel, mu, dmu):
    """(term, bound): bg^2 amp lam / r_sn A(r_sn / lam), A linear in its table.  mode 1: r_sn = r (an operand); mode 2:
    r_sn = sqrt(r'^2 + mu'^2): the square of mu' (1), the sum (1), the root (1).  tau = r_sn / lam (1); pos = (tau - tau0) / dtau: (1),
    (1); A is piecewise linear and continuous, so an error of pos - a cell that flips included - moves it by the largest slope of
    the cells around; its own arithmetic A[j] + f (A[j+1] - A[j]): difference (1), product (1), sum (1); the amplitude
    bg bg amp lam / r_sn A: five operations."""
    mode, amp, lam, bg, tau0, dtau, table = terms
    amp, lam, bg, table = LD(amp), LD(lam), LD(bg), np.asarray(table).astype(LD)
    if mode == 2:
        s2 = rr2 + mu * mu
        rsn = np.sqrt(s2)
        rel = (rr2 * d_rr2_rel + 2 * np.abs(mu) * dmu + U * mu * mu + U * s2) / s2 / 2 + U
    else:
        rsn, rel = r.astype(LD), LD(0)
    tau = rsn / lam
    pos = (tau - LD(tau0)) / LD(dtau)
    dpos = (np.abs(tau) * (rel + U) + U * np.abs(tau - LD(tau0))) / LD(dtau) + U * np.abs(pos)
    n = table.size
    j = np.clip(np.floor(pos).astype(np.int64), 0, n - 2)
    f = pos - j
    a = np.where(pos <= 0, table[0], np.where(pos > n - 1, 0, table[j] + f * (table[j + 1] - table[j])))
    slopes = np.abs(np.diff(table))
    slope = np.maximum(np.maximum(slopes[np.clip(j - 1, 0, n - 2)], slopes[j]), slopes[np.clip(j + 1, 0, n - 2)])
    da = slope * dpos + 2 * U * np.abs(f * (table[j + 1] - table[j])) + U * np.abs(a)
    assert np.all(pos < n - 2), 'the bound assumes bins below the table\'s last knot (A jumps to 0 behind it; it is continuous at the first)'
    value = bg * bg * amp * lam / rsn * a
    return value, np.abs(bg * bg * amp * lam / rsn) * da + np.abs(value) * (5 * U + rel)


def _odd_terms(terms, rr2, d_rr2_rel, mu, dmu):
    """(term, bound): the relativistic and asymmetry terms on the rescaled coordinates.  r' = sqrt(r'^2) (1), x = log r' (library,
    E_LOG), u = (x - x0) / h; four cubic B-spline sums (the bound of _spline); l1 = mu', l3 = (5 mu'^2 - 3) mu' / 2: square (1),
    product (1), difference (1), product (1); every term a chain of at most four products, every sum (1)."""
    rel_on, asy_on, coef, x0, h, amps = terms
    rr = np.sqrt(rr2)
    rel_rr = d_rr2_rel / 2 + U
    x = np.log(rr)
    dx = rel_rr + E_LOG * np.abs(x)
    n_coef = coef.shape[1]
    sp = [_spline(coef[q], x, dx, x0, h, n_coef)[:2] for q in range(4)]
    t = [LD(v) for v in amps]
    l1, l3 = mu, (5 * mu * mu - 3) * mu / 2
    dl1 = dmu
    dl3 = np.abs((15 * mu * mu - 3) / 2) * dmu + U * (2 * np.abs(5 * mu * mu * mu / 2) + 2 * np.abs(l3) + np.abs(l3))
    total, bound = np.zeros_like(mu), np.zeros_like(mu)

    def add(value, dvalue):
        nonlocal total, bound
        total = total + value
        bound = bound + dvalue + U * np.abs(total)

    def prod(factors):
        """product of (value, absolute error) pairs: first-order propagation + one rounding per multiplication"""
        value = np.ones_like(mu)
        for v, _ in factors:
            value = value * v
        err = sum(np.abs(value) * np.where(v != 0, dv / np.where(v != 0, np.abs(v), 1), 0) for v, dv in factors)
        return value, err + (len(factors) - 1) * U * np.abs(value)

    zero = np.zeros_like(mu)
    if rel_on:
        a = prod([(t[0] * np.ones_like(mu), zero), sp[0], (l1, dl1)])
        b = prod([(t[1] * np.ones_like(mu), zero), sp[1], (l3, dl3)])
        add(a[0] + b[0], a[1] + b[1] + U * np.abs(a[0] + b[0]))
    if asy_on:
        inner = t[2] * sp[2][0] - t[3] * sp[3][0]
        dinner = abs(t[2]) * sp[2][1] + abs(t[3]) * sp[3][1] + U * (np.abs(t[2] * sp[2][0]) + np.abs(t[3] * sp[3][0]) + np.abs(inner))
        a = prod([(inner, dinner), (rr, rr * rel_rr), (l1, dl1)])
        b = prod([(t[4] * np.ones_like(mu), zero), sp[3], (rr, rr * rel_rr), (l3, dl3)])
        add(a[0] + b[0], a[1] + b[1] + U * np.abs(a[0] + b[0]))
    return total, bound


def xi_bins(desc, st, grid, sc, ix, coef, basis=None, raw=False, terms=None):
    """One walker's bins of one pipeline: (xi [n] longdouble, bound [n], out of range [n] bool, parts).
    st: the static arrays; grid: x0, h, xlast [4], n_coef, extrapolate; sc: the walker's scalars, ix: their indices;
    terms: {'uv': (mode, amp, lambda, bias_gamma, tau0, dtau, A table), 'odd': (relativistic, asymmetry, coefficient rows [4, n],
    x0, h, the five amplitudes)} - the additive terms only the general kernel knows.
    coef [4, >= n_coef]: the walker's spline coefficients of this pipeline's column - or, for a static-basis pipeline on
    rescaled coordinates (k_xi_bins<true>), basis [4, 3, >= n_coef]: the kernel forms every tap as the Kaiser combination of the
    three basis coefficients.  raw: the spline and Legendre sums alone (k_poly_bins)."""
    r, rp0, rt0 = st['r'], st['rp'].astype(LD), st['rt'].astype(LD)
    ap, at, drp = LD(sc[ix['AP']]), LD(sc[ix['AT']]), LD(sc[ix['DRP']])
    n_coef = grid['n_coef']
    dcoef = [None] * 4
    if basis is not None:
        a, da = kaiser(desc, sc, ix)
        combined = [kaiser_combination(a, da, [basis[e, i] for i in range(3)]) for e in range(4)]
        coef, dcoef = [c[0] for c in combined], [c[1] for c in combined]
    rrp, rrt = ap * (rp0 + drp), at * rt0
    rr2 = rrp * rrp + rrt * rrt
    live = (r != 0) & (rr2 != 0)
    safe = np.where(live, rr2, LD(1))
    x = np.log(safe) / 2
    dx = 3 * U + E_LOG * np.abs(np.log(safe)) / 2
    mu = rrp / np.sqrt(safe)
    dmu = (6 * U + E_RSQRT) * np.abs(mu)
    xi, bound, mag = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    oob = np.zeros(x.shape, bool)
    window = (n_coef, 0)                    # the coefficient rows [lo, hi) the bins read
    for e in range(desc.n_ell):
        inside = np.ones(x.shape, bool) if grid['extrapolate'] else ~((x < LD(grid['x0'][e])) | (x > LD(grid['xlast'][e])))
        oob |= live & ~inside
        s, ds, u = _spline(coef[e], x, dx, grid['x0'][e], grid['h'][e], n_coef, dcoef[e])
        if live.any():
            cells = np.clip(np.floor(u[live]).astype(np.int64), 0, n_coef - 4)
            window = (min(window[0], int(cells.min())), max(window[1], int(cells.max()) + 4))
        if desc.single_ell >= 0:
            if e == desc.single_ell:
                xi, bound = np.where(inside, s, xi), np.where(inside, ds, bound)
            continue
        leg, dleg = _legendre(e, mu, dmu)
        term = s * leg
        xi = xi + np.where(inside, term, 0)
        bound = bound + np.where(inside, ds * np.abs(leg) + np.abs(s) * dleg, 0)
        mag = mag + np.where(inside, np.abs(term), 0)
    bound = bound + desc.n_ell * U * mag
    xi, bound = np.where(live, xi, 0), np.where(live, bound, 0)
    if raw:
        return xi, bound, oob, {'window': window}
    ev, rel = _evolution(desc, st, sc, ix)
    spline_part = xi * ev
    bound = bound * np.abs(ev) + np.abs(spline_part) * rel
    total = spline_part
    parts = {'spline': spline_part, 'window': window}
    if desc.radiation and not desc.is_peak:
        xr, dxr = _radiation(desc, st, sc, ix)
        total = total + xr
        bound = bound + dxr + U * np.abs(total)
        parts['radiation'] = xr
    for key, fn in (('uv', _shot_noise), ('odd', _odd_terms)):
        if terms and key in terms:
            args = (terms[key], r, rr2, 6 * U, mu, dmu) if key == 'uv' else (terms[key], np.where(live, rr2, LD(1)), 6 * U, mu, dmu)
            value, dvalue = fn(*args)
            total = total + value
            bound = bound + dvalue + U * np.abs(total)
            parts[key] = value
    return total, bound, oob, parts


def _broadband_total(terms, pos, theta, n):
    """bb_total: (total [n], bound) of the polynomial terms at one position (0 pre-mul, 1 pre-add).  Per term
    corr = sum_c theta_c basis_c as a chain of fused multiply-adds: per step the product (1) and the sum (1); multiplicative:
    1 + corr (1), total times it (1); additive: total + corr (1)."""
    mul = pos == 0
    total, bound = (np.ones(n, LD) if mul else np.zeros(n, LD)), np.zeros(n, LD)
    for p, func, slots, basis in terms:
        if p != pos:
            continue
        assert func == 0, 'polynomial terms only'
        corr, dcorr = np.zeros(n, LD), np.zeros(n, LD)
        for c, slot in enumerate(slots):
            prod = LD(theta[slot]) * basis[c].astype(LD)
            corr = corr + prod
            dcorr = dcorr + U * np.abs(prod) + U * np.abs(corr)
        if mul:
            factor = 1 + corr
            dfactor = dcorr + U * np.abs(factor)
            bound = bound * np.abs(factor) + np.abs(total) * dfactor
            total = total * factor
            bound = bound + U * np.abs(total)
        else:
            total = total + corr
            bound = bound + dcorr + U * np.abs(total)
    return total, bound


def quad_entry(bao, xp, dxp, xs, dxs, x0, extras=None, theta=None):
    """The entries of x' - x0' that k_xi_assemble_quad and k_xi_quad_plain store for the model bins:
    v = fma(bao, xi_peak, xi_smooth): the product (1), the sum (1);
    + amplitude x additive template: product (1), sum (1)                       [k_xi_assemble_quad, extras['template']]
    x the pre-distortion multiplicative broadband: (1)                          [extras['broadband'], position 0]
    + (1 + bao) x the pre-distortion additive broadband: 1 + bao (1), product (1), sum (1)          [position 1]
    - x0': (1).  Returns (v [n], bound [n])."""
    n = xp.size
    bao = LD(bao)
    v = bao * xp + xs
    dv = abs(bao) * dxp + dxs + U * np.abs(bao * xp) + U * np.abs(v)
    if extras and extras['template'] is not None:
        vec, slot, default = extras['template']
        amp = LD(theta[slot] if slot >= 0 else default)
        prod = amp * vec[:n].astype(LD)
        v = v + prod
        dv = dv + U * np.abs(prod) + U * np.abs(v)
    if extras and any(t[0] == 0 for t in extras['broadband']):
        total, dtotal = _broadband_total(extras['broadband'], 0, theta, n)
        dv = dv * np.abs(total) + np.abs(v) * dtotal
        v = v * total
        dv = dv + U * np.abs(v)
    if extras and any(t[0] == 1 for t in extras['broadband']):
        total, dtotal = _broadband_total(extras['broadband'], 1, theta, n)
        opb = 1 + bao
        prod = opb * total
        v = v + prod
        dv = dv + abs(opb) * dtotal + 2 * U * np.abs(prod) + U * np.abs(v)
    out = v - x0[:n].astype(LD)
    return out, dv + U * np.abs(out)


def quad_tail(bao, extras, theta, x0, n):
    """The entries behind the model bins: (1 + bao) c_j - x0' for the coefficients c_j of the additive post-distortion broadband
    terms, in the order of the terms: 1 + bao (1), the product (1), the difference (1).  Returns (v [n_coef], bound)."""
    slots = [slot for p, func, sl, _ in (extras['broadband'] if extras else []) if p == 3 for slot in sl]
    coefs = np.array([theta[slot] for slot in slots], dtype=LD)
    prod = (1 + LD(bao)) * coefs
    v = prod - x0[n:n + len(slots)].astype(LD)
    return v, 2 * U * np.abs(prod) + U * np.abs(v)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 twin of the kernel arithmetic (the bound must hold for it; a mutation must break it)
# ---------------------------------------------------------------------------------------------------------------------
def twin_bins(desc, st, grid, sc, ix, coef, mutation=None, terms=None):
    """xi [n] float64 of one walker, with the kernels' operations in the kernels' order (libm's log and exp and 1 / sqrt in
    place of the device functions: each within the bars the bound assumes)."""
    assert mutation is None or mutation in MUTATIONS
    r, rp0, rt0 = st['r'], st['rp'], st['rt']
    ap, at, drp = sc[ix['AP']], sc[ix['AT']], sc[ix['DRP']]
    n_coef = grid['n_coef']
    rrp, rrt = ap * (rp0 + drp), at * rt0
    rr2 = rrp * rrp + rrt * rrt
    live = (r != 0) & (rr2 != 0)
    safe = np.where(live, rr2, 1.0)
    x = 0.5 * np.log(safe)
    mu = rrp * (1.0 / np.sqrt(safe))
    if mutation == 'mu_unrescaled':
        raw = (rp0 + drp) * (rp0 + drp) + rt0 * rt0
        mu = (rp0 + drp) * (1.0 / np.sqrt(np.where(live, raw, 1.0)))
    x2 = mu * mu
    legs = [np.ones_like(x2), 0.5 * (3.0 * x2 - 1.0),
            0.125 * (((34.0 if mutation == 'l4_34' else 35.0) * x2 - 30.0) * x2 + 3.0),
            0.0625 * ((((230.0 if mutation == 'l6_230' else 231.0) * x2 - 315.0) * x2 + 105.0) * x2 - 5.0)]
    xi = np.zeros_like(x)
    for e in range(desc.n_ell):
        inside = np.ones(x.shape, bool) if grid['extrapolate'] else ~((x < grid['x0'][e]) | (x > grid['xlast'][e]))
        u = (x - grid['x0'][e]) * (1.0 / grid['h'][e])
        j = np.clip(np.floor(u).astype(np.int64), 0, n_coef - 4)
        t = u - j
        if mutation == 'knot_plus_one':
            j = np.minimum(j + 1, n_coef - 4)
        t2 = t * t
        t3 = t2 * t
        omt = 1.0 - t
        w0 = omt * omt * omt
        w1 = 3.0 * t3 - (6.000000000001 if mutation == 'w1_digit' else 6.0) * t2 + 4.0
        w2 = -3.0 * t3 + 3.0 * t2 + (3.000000000001 if mutation == 'w2_digit' else 3.0) * t + 1.0
        c = coef[e]
        s = (c[j] * w0 + c[j + 1] * w1 + c[j + 2] * w2 + c[j + 3] * t3) * (1.0 / 6.0)
        if desc.single_ell >= 0:
            if e == desc.single_ell:
                xi = np.where(inside, s, xi)
        else:
            xi = xi + np.where(inside, s * legs[e], 0.0)
    xi = np.where(live, xi, 0.0)
    lnz, lnz2 = st['lnrelz'], (st['lnrelz'] if mutation == 'lnrelz_swapped' else st['lnrelz2'])
    if desc.evol == (0, 0):
        a1, a2 = sc[ix['EV1A']], sc[ix['EV2A']]
        ev = np.exp(a1 * lnz + a2 * lnz2) if desc.split_evol else np.exp((a1 + a2) * lnz)
    else:
        ev = np.ones_like(x)
        for q in range(2):
            a, c = sc[ix[f'EV{q + 1}A']], sc[ix[f'EV{q + 1}B']]
            if desc.evol[q] == 1:
                z1, ze = 1.0 + st['z'], 1.0 + desc.z_eff
                ev = ev * ((a + c * z1 * z1) / (a + c * ze * ze))
            else:
                ev = ev * np.power(st['relz'], a)
    xi = xi * ev
    xi = xi * st['growth']
    if desc.radiation and (not desc.is_peak or mutation == 'radiation_on_peak'):
        resc = desc.radiation == 2
        rp = ap * (rp0 + drp) + drp if resc else rp0 + drp
        rtr = at * rt0 if resc else rt0
        rs2 = rp * rp + rtr * rtr
        irs = 1.0 / np.sqrt(rs2)
        rs, ms = rs2 * irs, rp * irs
        xr = sc[ix['RAD_S']] * (irs * irs) * (1.0 - sc[ix['RAD_A']] * (1.0 - ms * ms))
        xr = xr * np.exp(-rs * ((1.0 + ms) * sc[ix['RAD_IL']] + sc[ix['RAD_ID']]))
        xi = xi + xr
    if terms and 'uv' in terms:
        mode, amp, lam, bg, tau0, dtau, table = terms['uv']
        rsn = np.sqrt(rr2 + mu * mu) if mode == 2 else r
        pos = (rsn / lam - tau0) / dtau
        j = np.clip(pos.astype(np.int64), 0, table.size - 2)
        f = pos - j
        a = np.where(pos <= 0, table[0], np.where(pos >= table.size - 1, 0.0, table[j] + f * (table[j + 1] - table[j])))
        xi = xi + bg * bg * amp * lam / rsn * a
    if terms and 'odd' in terms:
        rel_on, asy_on, oc, ox0, oh, t = terms['odd']
        rr = np.sqrt(safe)
        u = (np.log(rr) - ox0) / oh
        j = np.clip(np.floor(u).astype(np.int64), 0, oc.shape[1] - 4)
        tt = u - j
        t2 = tt * tt
        t3 = t2 * tt
        omt = 1.0 - tt
        w0, w1, w2 = omt * omt * omt, 3.0 * t3 - 6.0 * t2 + 4.0, -3.0 * t3 + 3.0 * t2 + 3.0 * tt + 1.0
        sp = [(oc[q][j] * w0 + oc[q][j + 1] * w1 + oc[q][j + 2] * w2 + oc[q][j + 3] * t3) * (1.0 / 6.0) for q in range(4)]
        l1, l3 = mu, 0.5 * (5.0 * mu * mu - 3.0) * mu
        if rel_on:
            xi = xi + (t[0] * sp[0] * l1 + t[1] * sp[1] * l3)
        if asy_on:
            xi = xi + ((t[2] * sp[2] - t[3] * sp[3]) * rr * l1 + t[4] * sp[3] * rr * l3)
    return xi


def twin_batch(desc, st, grid, scal, ix, coefs, nw=2, mutation=None, terms=None):
    """A batch through a kernel that gives a thread nw walkers: slot w of block b0 serves walker min(b0 + w, B - 1) and a
    surplus slot stores nothing.  scal [B, NS], coefs [B, 4, n_coef] -> [B, n]."""
    B = scal.shape[0]
    out = np.zeros((B, st['r'].size))
    for b0 in range(0, B, nw):
        for w in range(nw):
            b = min(b0 + w, B - 2 if mutation == 'surplus_walker' and B > 1 else B - 1)
            if b0 + w < B:
                inner = None if mutation == 'surplus_walker' else mutation
                out[b0 + w] = twin_bins(desc, st, grid, scal[b], ix, coefs[b], inner, terms=terms)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_xi_bins_gpu.py (and, without a device, of tests/test_xi_bins_host.py)
# ---------------------------------------------------------------------------------------------------------------------
WALKER_SEED = 20260803 + 37
N_WALKERS = 3                   # + the fiducial point


def _cross(prob):
    return prob.items['lyalya_qso'].core


def _auto(prob):
    return prob.items['lyalya_lyalya'].core


def _rad2(prob):
    _cross(prob).xi.rescale_coords_systematics = True
    prob.params.update(qso_rad_asymmetry=0.3, qso_rad_lifetime=25.0)


def _croom(prob):
    _cross(prob).xi.evol_model['QSO'] = 'croom'
    prob.params.update(croom_par0=0.53, croom_par1=0.289)


def _uv(prob, rescaled=False):
    for item in prob.items.values():
        item.core.xi.uv_shotnoise = True
        item.core.xi.rescale_coords_systematics = rescaled
    prob.params.update(uv_shotnoise_amp=0.5, lambda_uv=300.0)
    prob.params.setdefault('bias_gamma', 0.13)


def _uv2(prob):
    _uv(prob, rescaled=True)


def _odd(prob):
    _cross(prob).xi.relativistic = _cross(prob).xi.asymmetry = True
    prob.params.update({'Arel1': -13.5, 'Arel3': 1.0, 'Aasy0': 1.0, 'Aasy2': 1.0, 'Aasy3': 1.0})


def _bb(prob):
    """The additive template (instrumental systematics), a multiplicative and an additive pre-distortion broadband, and an
    additive post-distortion one (entries behind the model bins) on the auto-correlation."""
    from vega_amd.setup import BroadbandTerm
    item = prob.items['lyalya_lyalya']
    name = item.name
    rt = np.asarray(item.core.r) * np.sqrt(1 - np.asarray(item.core.mu)**2)
    grid = np.linspace(0.0, rt.max() + 4.0, 12)
    item.inst_sys_table = np.column_stack([grid, 1.0 + 0.5 * np.cos(grid / 7.0)])
    item.broadband = [BroadbandTerm(f'BB-{name}-0 mul pre rp,rt', 'broadband', 'mul', 'pre', 'rp,rt', (0, 1, 1), (0, 2, 2)),
                      BroadbandTerm(f'BB-{name}-1 add pre r,mu', 'broadband', 'add', 'pre', 'r,mu', (-2, 0, 1), (0, 2, 2)),
                      BroadbandTerm(f'BB-{name}-2 add post r,mu', 'broadband', 'add', 'post', 'r,mu', (0, 2, 1), (0, 6, 2))]
    rng = np.random.default_rng(WALKER_SEED + 1)
    for term in item.broadband:
        for i in range(term.r1[0], term.r1[1] + 1, term.r1[2]):
            for j in range(term.r2[0], term.r2[1] + 1, term.r2[2]):
                prob.params[f'{term.name} ({i},{j})'] = 1e-3 * rng.standard_normal()


def _split(prob):
    core = _cross(prob)
    rel = np.asarray(core.rel_z_evol, float) * np.ones_like(np.asarray(core.r, float))
    core.rel_z_evol_1, core.rel_z_evol_2 = rel, 1.01 * rel**1.1


def _set(**kw):
    def apply(prob):
        for core in (item.core for item in prob.items.values()):
            for key, value in kw.items():
                assert hasattr(core.xi, key) or key == 'fht_lowring', key
                setattr(core.xi, key, value)
    return apply


# name -> (grid case of tests/helpers/small_grids.py, change of the Problem, claims {item: dict})
CASES = {
    # (fht_lowring, the default, gives every multipole its own ln r grid: the SAME = false instantiations)
    'a63': ('a63', None, {'lyalya_lyalya': dict(n=63, n_ell=4, radiation=0, same_grid=False)}),
    'a1287': ('a1287', None, {'lyalya_lyalya': dict(n=1287, n_ell=4, radiation=0)}),
    # 63 and 1320 bins in one launch sized by the larger; the cross-correlation carries delta_rp and the radiation term
    'j_small_big': ('j_small_big', None, {'lyalya_lyalya': dict(n=63, n_ell=4, radiation=0), 'lyalya_qso': dict(n=1320, n_ell=4, radiation=1)}),
    'j_rad2': ('j_small_big', _rad2, {'lyalya_qso': dict(n=1320, radiation=2)}),
    'j_croom': ('j_small_big', _croom, {'lyalya_qso': dict(n=1320, evol=(0, 1))}),
    'j_split': ('j_small_big', _split, {'lyalya_qso': dict(n=1320, split_evol=True)}),
    # UV shot noise on the bins' own r and (`rescale-coords-systematics`) on sqrt(r'^2 + mu'^2); the odd multipoles of the cross
    'a63_uv': ('a63', _uv, {'lyalya_lyalya': dict(n=63, uv=1)}),
    'j_uv2': ('j_small_big', _uv2, {'lyalya_lyalya': dict(n=63, uv=2), 'lyalya_qso': dict(n=1320, uv=2, radiation=2)}),
    'j_odd': ('j_small_big', _odd, {'lyalya_qso': dict(n=1320, odd=True)}),
    # the additive template and the pre-distortion broadband lines of k_xi_assemble_quad, twelve entries behind the model bins
    'a63_bb': ('a63', _bb, {'lyalya_lyalya': dict(n=63, template=True, n_pre=2, n_post_coef=12)}),
    'a63_single2': ('a63', _set(single_multipole=2), {'lyalya_lyalya': dict(n=63, single_ell=1)}),
    'a63_ell2': ('a63', _set(ell_max=2), {'lyalya_lyalya': dict(n=63, n_ell=2)}),
    'a63_ell4': ('a63', _set(ell_max=4), {'lyalya_lyalya': dict(n=63, n_ell=3)}),
    'a1287_ell4': ('a1287', _set(ell_max=4), {'lyalya_lyalya': dict(n=1287, n_ell=3)}),
    # one ln r grid for every multipole: the SAME = true instantiations
    'a63_nolowring': ('a63', _set(fht_lowring=False), {'lyalya_lyalya': dict(n=63, n_ell=4, same_grid=True)}),
    'a1287_nolowring': ('a1287', _set(fht_lowring=False), {'lyalya_lyalya': dict(n=1287, n_ell=4, same_grid=True)}),
}


# the static-basis forms, on the metal cases of tests/helpers/small_grids.py: m63 (auto 7 x 9, fifteen pairs, every one with a
# matrix: each keeps its own array), m63_mixed (two pairs without matrix: a static group of two), m63_fast (fast_metals, chi2 at
# the fiducial point first: frozen metal x metal terms, shared pipelines) and mj (m63's item beside a cross-correlation of 1320
# bins whose metal pipelines carry the quasar's velocity dispersion - no Kaiser polynomial, so they form their multipoles per
# walker and, a matrix reading each, run as lean singles: group, lean single, general and static forms beside a 1320-bin item).  routes: the literal claim per (engine, B <= 8 or above), where one is made.
STATIC_CASES = {
    'm63': dict(base='m63', n=[63], n_pairs=[15], no_matrix=0, routes={
        ('default', 'small'): {'general', 'static', 'poly_bins'}, ('nosums', 'big'): {'lean', 'static_nw', 'poly_bins'},
        ('default', 'big'): {'group', 'static', 'poly_bins'}, ('notaps', 'small'): {'general', 'static_taps'},
        ('notaps', 'big'): {'lean', 'static_taps'}}),
    'm63_mixed': dict(base='m63', n=[63], n_pairs=[15], no_matrix=2, routes={
        ('default', 'small'): {'general', 'static', 'poly_bins'}, ('nosums', 'big'): {'lean', 'static_nw', 'poly_bins'},
        ('default', 'big'): {'group', 'static', 'static_group', 'poly_bins'}, ('notaps', 'small'): {'general', 'static_taps'},
        ('notaps', 'big'): {'lean', 'static_taps'}}),
    'm63_fast': dict(base='m63', n=[63], n_pairs=[15], no_matrix=0, routes={}),
    'mj': dict(base='mj', n=[63, 1320], n_pairs=[15, 4], no_matrix=0, routes={
        ('default', 'small'): {'general', 'static', 'poly_bins'},
        ('nosums', 'big'): {'lean', 'general', 'static_nw', 'poly_bins'},
        ('default', 'big'): {'group', 'lean', 'general', 'static', 'poly_bins'},
        ('notaps', 'small'): {'general', 'static_taps'}, ('notaps', 'big'): {'lean', 'general', 'static_taps'}}),
}


def build_static_case(tmp_path, case, golden):
    from helpers import small_grids as sg
    claim = STATIC_CASES[case]
    prob = sg.build_case(tmp_path, claim['base'], golden)
    sg.check_facts(claim['base'], prob)
    if case != claim['base']:
        prob = sg.metal_variant(prob, case)
    items = list(prob.items.values())
    assert [np.asarray(it.core.r).size for it in items] == claim['n'] and [len(it.metals) for it in items] == claim['n_pairs']
    assert sum(p.matrix is None for it in items for p in it.metals) == claim['no_matrix']
    assert all(it.metal_opts['fast_metals'] == (case == 'm63_fast') for it in items)
    return prob


def build_case(tmp_path, case, golden):
    """The Problem of a case, its claims checked (before any device is touched)."""
    import copy
    from helpers import small_grids as sg
    grid, change, claims = CASES[case]
    prob = copy.deepcopy(sg.build_case(tmp_path, grid, golden))
    sg.check_facts(grid, prob)
    if change is not None:
        change(prob)
    check_claims(case, prob)
    return prob


def check_claims(case, prob):
    from vega_amd import fftlog_op
    _, _, claims = CASES[case]
    for name, claim in claims.items():
        core = prob.items[name].core
        for component in ('peak', 'smooth'):
            d = Desc.from_pipe(prob, core, component)
            assert np.asarray(core.r).size == claim['n'], (case, name)
            if 'uv' in claim:
                assert int(core.xi.uv_shotnoise) * (2 if core.xi.rescale_coords_systematics else 1) == claim['uv']
            if 'template' in claim:
                item = prob.items[name]
                assert item.inst_sys_table is not None and np.any((np.asarray(core.r) * np.asarray(core.mu) > 0) & (np.asarray(core.r) * np.asarray(core.mu) < item.rp_binsize))
                assert sum(t.pos == 'pre' for t in item.broadband) == claim['n_pre'] and {t.kind for t in item.broadband if t.pos == 'pre'} == {'mul', 'add'}
                n_post = sum(len(range(t.r1[0], t.r1[1] + 1, t.r1[2])) * len(range(t.r2[0], t.r2[1] + 1, t.r2[2])) for t in item.broadband if t.pos == 'post')
                assert n_post == claim['n_post_coef']
            if 'odd' in claim:
                assert core.xi.relativistic and core.xi.asymmetry
            for key in ('n_ell', 'single_ell', 'split_evol', 'evol', 'radiation'):
                if key in claim:
                    assert getattr(d, key) == claim[key], (case, name, key, getattr(d, key))
        if 'same_grid' in claim:
            x0 = [fftlog_op.xi_operator(prob.k, ell, lowring=getattr(core.xi, 'fht_lowring', True))[1] for ell in (0, 2)]
            assert (x0[0] == x0[1]) == claim['same_grid'], (case, x0)
    for item in prob.items.values():
        if item.core.xi.radiation:
            # the radiation term takes rsqrt of (r_par' + drp)^2 + r_perp'^2 without a guard: no bin may have r_perp = 0, or a
            # walker's delta_rp could cancel a bin centre and hand it 0 (NaN)
            st = host_static(item.core)
            assert np.all(st['rt'] > 0), case
    sizes = sorted(np.asarray(item.core.r).size for item in prob.items.values())
    assert sizes[0] < 256 or sizes[0] % 256, case            # less than a block, or a ragged last block


def walker_params(prob, n=N_WALKERS, seed=WALKER_SEED):
    """The fiducial point and n seeded walkers that move ap, at and - where the problem has one - the cross-correlation's
    delta_rp: a list of parameter overrides."""
    rng = np.random.default_rng(seed)
    rows = [{}]
    for _ in range(n):
        row = {'ap': prob.params['ap'] * (1 + 0.03 * rng.standard_normal()), 'at': prob.params['at'] * (1 + 0.03 * rng.standard_normal())}
        if 'drp_QSO' in prob.params:
            row['drp_QSO'] = prob.params['drp_QSO'] + 0.5 * rng.standard_normal()
        rows.append(row)
    return rows


def host_grid(prob, core):
    """The spline grid and the operators OP_ell of a pipeline's options: ({x0, h, xlast, n_coef, extrapolate}, [OP_ell])."""
    from vega_amd import fftlog_op
    assert not core.xi.old_fftlog and not getattr(core.xi, 'fht_extrap', False)
    ops = [fftlog_op.xi_operator(prob.k, ell, lowring=getattr(core.xi, 'fht_lowring', True)) for ell in (0, 2, 4, 6)]
    x0, h, n = np.array([o[1] for o in ops]), np.array([o[2] for o in ops]), ops[0][3]
    return dict(x0=x0, h=h, xlast=x0 + (n - 1) * h, n_coef=n + 2, extrapolate=False, same_grid=bool(np.all(x0 == x0[0]))), [o[0] for o in ops]


def host_terms(prob, core, pars, pk_lin):
    """The additive terms of a pipeline from a Problem (as Engine._add_pipeline and the lowering hand them to the engine)."""
    from vega_amd import fftlog_op, static_terms
    terms = {}
    if core.xi.uv_shotnoise:
        tau, a = static_terms.shotnoise_a()
        bg = pars['bias_gamma'] if 'bias_gamma' in pars else pars['bias_gamma_e']
        terms['uv'] = (2 if core.xi.rescale_coords_systematics else 1, pars['uv_shotnoise_amp'], pars['lambda_uv'], bg,
                       float(tau[0]), float(tau[1] - tau[0]), np.asarray(a, float))
    if core.xi.relativistic or core.xi.asymmetry:
        rows = [fftlog_op.hamilton_spline(prob.k, pk_lin, ell, kind) for kind, ell in (('rel', 1), ('rel', 3), ('asy', 0), ('asy', 2))]
        terms['odd'] = (bool(core.xi.relativistic), bool(core.xi.asymmetry), np.stack([row[0] for row in rows]), rows[0][1], rows[0][2],
                        [pars.get(n, 0.0) for n in ('Arel1', 'Arel3', 'Aasy0', 'Aasy2', 'Aasy3')])
    return terms or None


def engine_terms(eng, pid, theta_row):
    """The same from an engine's taps and a walker's parameters."""
    from vega_amd import static_terms
    d, g = eng.pipe_descs[pid], eng.bins_grid(pid)
    terms = {}
    if d.uv_shotnoise:
        tau, a = static_terms.shotnoise_a()
        terms['uv'] = (int(d.uv_shotnoise), *(theta_row[d.uvsn_slot[i]] for i in range(3)), float(tau[0]), float(tau[1] - tau[0]), np.asarray(a, float))
    if g['odd_ncoef'] > 0:
        names = ('Arel1', 'Arel3', 'Aasy0', 'Aasy2', 'Aasy3')
        amps = [theta_row[eng.low.slot[n]] if n in eng.low.slot else 0.0 for n in names]
        terms['odd'] = ('Arel1' in eng.low.slot, 'Aasy0' in eng.low.slot, eng.odd_coefficients(pid), g['odd_x0'], g['odd_h'], amps)
    return terms or None


def host_operands(prob, overrides):
    """Per (item, component) of a Problem at one parameter point, everything xi_bins takes, from the CPU reference's own
    multipoles: coefficients OP_ell P_ell (vega_amd/fftlog_op.py) of oracle.vega_cpu's P_ell; and the reference's xi."""
    from oracle import vega_cpu as oc
    pars = oc.local_params(prob, overrides)
    taps = {}
    oc.compute_model(prob, overrides, taps=taps)
    out = {}
    for name, item in prob.items.items():
        core = item.core
        grid, ops = host_grid(prob, core)
        # (coefficient i multiplies the B-spline centred on knot i - 1: a bin in cell j = floor((x - x0) / h) reads c[j .. j + 3])
        for component in ('peak', 'smooth'):
            desc = Desc.from_pipe(prob, core, component)
            sub = taps[name][component]
            coef = np.zeros((4, grid['n_coef']))
            ells = [2 * e for e in range(desc.n_ell)] if desc.single_ell < 0 else [2 * desc.single_ell]
            for ell in ells:
                coef[ell // 2] = ops[ell // 2] @ sub['pk_ell'][ell]
            pk_lin = prob.pk_full - prob.pk_smooth if component == 'peak' else prob.pk_smooth
            out[(name, component)] = dict(desc=desc, st=host_static(core), grid=grid, sc=host_scalars(prob, core, pars, component),
                                          ix=HOST_INDEX, coef=coef, ref=sub['xi_core'], terms=host_terms(prob, core, pars, pk_lin))
    return out
