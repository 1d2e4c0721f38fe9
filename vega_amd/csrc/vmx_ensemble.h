// The affine-invariant ensemble sampler (Goodman & Weare 2010, the "stretch move" of emcee), pinned decision for decision.
//
// The walker loop runs where the walkers are (vmx_ensemble_run, vegamx.hip: one small kernel per half-step decides the half that
// was just evaluated and proposes the next one); vega_amd/ensemble.py restates every expression below in NumPy (the `python`
// driver) and tests/helpers/ensemble_driver.cpp compiles this header with g++ so that tests/test_ensemble_host.py can hold the two
// against each other bit for bit.  No HIP type, no heap.
//
//   random numbers   Random123 Philox4x64-10 (NumPy's np.random.Philox): one block per (walker-in-half i, global step s, half h),
//                    counter (i, s, h, 0) (word 0 least significant), key (seed, stream).  The block equals
//                    np.random.Philox(key=[seed, stream], counter=(c - 1) mod 2**256).random_raw(4) (NumPy increments before it
//                    encrypts).  A uniform double from a word x: (x >> 11) 2**-53.
//   halves           walkers [0, W/2) and [W/2, W); step s updates half 0 against half 1, then half 1 against the updated half 0
//                    (emcee with randomize_split=False).
//   proposal         walker k of the active half, block words x0, x1, x2: partner j = ((x0 >> 32) (W/2)) >> 32 of the other
//                    half; t = (a - 1) u(x1); t = t + 1; z = t t; z = z / a; per sampled column y = c - (c - s) z (c the partner's
//                    position, s the walker's own); factor = (n - 1) log(z).
//   decision         accept iff every y lies in [lo, hi], the engine's status is 0 and chi2 < 1e99, and
//                    (factor + lnL_new) - lnL_old > log(u(x2)), with lnL = log_norm - 0.5 chi2.
//
// Every expression is the separately rounded IEEE operations written above: device code contracts a * b + c into an FMA by
// default, so the functions below switch contraction off (clang) - g++ has no FMA in the baseline x86-64 ISA and is left alone.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef VMX_HD
#if defined(__HIPCC__)
#define VMX_HD __host__ __device__
#else
#define VMX_HD
#endif
#endif

#if defined(__clang__)
#define VMX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VMX_NO_CONTRACT
#endif

#include "vmx_pexp.h"

namespace vmx_ens {

struct Block { uint64_t w[4]; };

VMX_HD inline void mulhilo(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// Philox4x64 with 10 rounds (Random123 philox4x64_R(10, ctr, key))
VMX_HD inline Block philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1)
{
    constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += W0; k1 += W1; }
        uint64_t hi0, lo0, hi1, lo1;
        mulhilo(M0, c0, hi0, lo0);
        mulhilo(M1, c2, hi1, lo1);
        const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    return Block{{c0, c1, c2, c3}};
}

// the block of walker-in-half i at global step s, half h
VMX_HD inline Block step_block(int64_t i, int64_t s, int h, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)i, (uint64_t)s, (uint64_t)h, 0, seed, stream);
}

VMX_HD inline double u01(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

// partner index in the complementary half of `half` walkers
VMX_HD inline int64_t partner(uint64_t x0, int64_t half) { return (int64_t)(((x0 >> 32) * (uint64_t)half) >> 32); }

VMX_HD inline double stretch_z(double a, uint64_t x1)
{
    VMX_NO_CONTRACT
    double t = (a - 1.0) * u01(x1);
    t = t + 1.0;
    double z = t * t;
    z = z / a;
    return z;
}

// one sampled column of the proposal: c the partner's position, s the walker's own
VMX_HD inline double propose(double c, double s, double z)
{
    VMX_NO_CONTRACT
    const double d = (c - s) * z;
    return c - d;
}

VMX_HD inline double log_factor(int n, double z)
{
    VMX_NO_CONTRACT
    return (double)(n - 1) * log(z);
}

VMX_HD inline double log_lik(double log_norm, double chi2)
{
    VMX_NO_CONTRACT
    const double h = 0.5 * chi2;
    return log_norm - h;
}

VMX_HD inline bool model_ok(int32_t status, double chi2) { return status == 0 && chi2 < 1e99; }

// the Metropolis decision of a proposal (inside: every column in its box; ok: model_ok)
VMX_HD inline bool accept(bool inside, bool ok, double factor, double lnl_new, double lnl_old, uint64_t x2)
{
    VMX_NO_CONTRACT
    if (!inside || !ok) return false;
    const double lhs = (factor + lnl_new) - lnl_old;
    return lhs > log(u01(x2));
}

// ---- the differential-evolution and snooker moves, and mixtures of the three (vmx_ensemble_run_many_moves: k_ens_half_moves)
//
// Both are red-blue moves like the stretch move: a walker of the active half is moved using only walkers of the other half, so
// the half-step and the decision above stay what they are.  Only + - x / sqrt log, each rounded on its own; no Box-Muller and
// no trigonometric function (they would end the bit-for-bit agreement of the two drivers).
//
//   random numbers   walker-in-half k, step s, half h has two blocks: A, counter (k, s, h, 0), the block above - w0 the first
//                    index, w1 the second index (in the stretch move its uniform, as ever), w2 the acceptance word, w3 the third
//                    index - and B, counter (k, s, h, 1): w0 the move choice, w1 and w2 the jitter, w3 unused.
//   partners         distinct walkers of the other half of H: j1 = partner(A.w0, H); j2 = partner(A.w1, H - 1), plus 1 if
//                    j2 >= j1 (H >= 2); j3 = partner(A.w3, H - 2), raised by 1 if it is at or above the smaller of j1, j2 and
//                    the raised value by 1 again if it is at or above the larger (H >= 3).
//   mixture          weights (p_stretch, p_de, p_snooker) >= 0 of positive sum S reach the device as the thresholds t0 = p0 / S,
//                    t1 = (p0 + p1) / S: stretch if u(B.w0) < t0, DE if u(B.w0) < t1, else snooker.  A pure move has its weight
//                    equal to S (x / x = 1 exactly, and u < 1) and draws from the same words.
//   DE               ter Braak 2006, emcee's DEMove: g = (u(B.w1) + u(B.w2)) - 1; gamma = gamma0 (1 + sigma g); per column
//                    y = s + gamma (c[j1] - c[j2]); factor = 0.  The jitter g is triangular on (-1, 1) where emcee's is normal:
//                    it is symmetric about 0 and independent of the state, so the proposal density stays symmetric and the
//                    move reversible.  gamma0 comes from the host as a double (default 2.38 / sqrt(2 n)); sigma defaults to 1e-5.
//   snooker          ter Braak & Vrugt 2008, emcee's DESnookerMove: z = c[j1], z1 = c[j2], z2 = c[j3]; d = s - z;
//                    norm = sqrt(sum d^2); u = d / norm; p = sum u z1 - sum u z2; y = s + u (gamma_s p);
//                    factor = (n - 1) (log(sqrt(sum (y - z)^2)) - log(norm)); every sum in column order.  norm == 0 (not
//                    greater than 0) or a factor that is not finite marks the proposal as not inside: it is rejected and counted
//                    with the box rejections; with norm == 0 the proposal is the walker's own position and the factor 0.
//                    gamma_s defaults to 1.7.
//   box, decision    unchanged: a proposal outside the box evaluates the walker's own position; accept(...) above.
enum Move { MOVE_STRETCH = 0, MOVE_DE = 1, MOVE_SNOOKER = 2 };

// block B of walker-in-half i at global step s, half h
VMX_HD inline Block move_block(int64_t i, int64_t s, int h, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)i, (uint64_t)s, (uint64_t)h, 1, seed, stream);
}

// the thresholds of the weights (p_stretch, p_de, p_snooker)
VMX_HD inline void move_thresholds(const double* p, double& t0, double& t1)
{
    VMX_NO_CONTRACT
    const double p01 = p[0] + p[1];
    const double sum = p01 + p[2];
    t0 = p[0] / sum;
    t1 = p01 / sum;
}

VMX_HD inline int move_choice(uint64_t w0, double t0, double t1)
{
    const double u = u01(w0);
    return u < t0 ? MOVE_STRETCH : (u < t1 ? MOVE_DE : MOVE_SNOOKER);
}

// the second partner, distinct from j1 (half >= 2)
VMX_HD inline int64_t partner2(uint64_t x1, int64_t half, int64_t j1)
{
    const int64_t j = partner(x1, half - 1);
    return j >= j1 ? j + 1 : j;
}

// the third partner, distinct from j1 and j2 (half >= 3)
VMX_HD inline int64_t partner3(uint64_t x3, int64_t half, int64_t j1, int64_t j2)
{
    const int64_t small = j1 < j2 ? j1 : j2, large = j1 < j2 ? j2 : j1;
    int64_t j = partner(x3, half - 2);
    if (j >= small) j += 1;
    if (j >= large) j += 1;
    return j;
}

VMX_HD inline double de_gamma(double gamma0, double sigma, uint64_t w1, uint64_t w2)
{
    VMX_NO_CONTRACT
    double g = u01(w1) + u01(w2);
    g = g - 1.0;
    double t = sigma * g;
    t = 1.0 + t;
    return gamma0 * t;
}

// one sampled column of the DE proposal: s the walker's own position, c1 and c2 the two partners'
VMX_HD inline double de_propose(double s, double c1, double c2, double gamma)
{
    VMX_NO_CONTRACT
    const double d = c1 - c2;
    const double t = gamma * d;
    return s + t;
}

VMX_HD inline bool is_finite(double v) { return v - v == 0.0; }

// the snooker proposal y[n] of the walker at s[n] along its line through z[n], with the projections of z1[n] and z2[n] on that
// line; false: not a proposal (norm == 0, or a factor that is not finite).  y must not overlap the inputs.
VMX_HD inline bool snooker_propose(int n, const double* s, const double* z, const double* z1, const double* z2, double gamma_s,
                                   double* y, double& factor)
{
    VMX_NO_CONTRACT
    double ss = 0.0;
    for (int d = 0; d < n; ++d) {
        const double e = s[d] - z[d];
        const double q = e * e;
        ss = ss + q;
    }
    const double norm = sqrt(ss);
    if (!(norm > 0.0)) {
        for (int d = 0; d < n; ++d) y[d] = s[d];
        factor = 0.0;
        return false;
    }
    double p1 = 0.0, p2 = 0.0;
    for (int d = 0; d < n; ++d) {
        const double e = s[d] - z[d];
        const double u = e / norm;
        const double q1 = u * z1[d];
        p1 = p1 + q1;
        const double q2 = u * z2[d];
        p2 = p2 + q2;
    }
    const double p = p1 - p2;
    const double gp = gamma_s * p;
    double tt = 0.0;
    for (int d = 0; d < n; ++d) {
        const double e = s[d] - z[d];
        const double u = e / norm;
        const double m = u * gp;
        const double v = s[d] + m;
        y[d] = v;
        const double r = v - z[d];
        const double q = r * r;
        tt = tt + q;
    }
    const double l_new = log(sqrt(tt));
    const double l_old = log(norm);
    const double dl = l_new - l_old;
    factor = (double)(n - 1) * dl;
    return is_finite(factor);
}

// ---- parallel tempering: ladders of ensembles and the swaps between their rungs (vmx_ensemble_run_pt: k_ens_half_pt, k_ens_swap)
//
//   ladder           beta[0] = 1 > beta[1] > ... > beta[T - 1] >= 0, T <= PT_MAXT.  A run holds G ladders; ladder g owns the
//                    ensembles g T .. g T + T - 1, rung 0 the cold one.  Every rung is an ensemble as above, on its own stream.
//   decision         rung t accepts iff inside, model ok and (factor + beta lnL_new) - beta lnL_old > log(u(w2)): the products
//                    a = beta lnL_new and b = beta lnL_old first, each rounded, then accept(inside, ok, factor, a, b, w2).  With
//                    beta = 1 the products are exact and the decision is the one above bit for bit; with beta = 0 a proposal
//                    outside the box or with a failed model is still rejected.  The stored lnL is untempered, always.
//   swap sweep       after step s when swap_every > 0 and (s + 1) % swap_every == 0 (s the global step: a run cut into calls swaps
//                    at the same steps), once half 1 of step s is decided and before the chain row of step s is recorded.  Pairs
//                    of rungs from the hottest down, one after the other: t = T - 1, ..., 1, rung t - 1 against rung t, so that a
//                    walker may travel several rungs in one sweep.
//   pairing          a random rotation: r = swap_shift(w0, W) = partner(w0, W), w0 the first word of the block with counter
//                    (0, s, t, 3); walker k of rung t - 1 is paired with walker (k + r) mod W of rung t - disjoint pairs, chosen
//                    independently of the state.
//   swap rule        pair k draws word 0 of the block with counter (k, s, t, 2); db = beta[t - 1] - beta[t];
//                    dl = lnL_hot - lnL_cold; lhs = db dl; swap iff lhs > log(u(word)).  A swap exchanges the n positions and the
//                    lnL; the accepted / box / failed counters stay with the slot.
//   key              both blocks: (seed, the stream of the ladder's rung 0).  The last counter words 2 and 3 keep them apart from
//                    the blocks of the moves (0 and 1).
constexpr int PT_MAXT = 64;

// a ladder the sampler takes: beta[0] == 1, finite, strictly decreasing, none negative
VMX_HD inline bool ladder_ok(const double* beta, int T)
{
    if (T < 1 || T > PT_MAXT || !(beta[0] == 1.0)) return false;
    for (int t = 0; t < T; ++t) {
        if (!is_finite(beta[t]) || !(beta[t] >= 0.0)) return false;
        if (t > 0 && !(beta[t] < beta[t - 1])) return false;
    }
    return true;
}

// a rung's view of a log-likelihood: what its Metropolis decision compares
VMX_HD inline double tempered(double beta, double lnl)
{
    VMX_NO_CONTRACT
    return beta * lnl;
}

// the decision of a proposal on the rung of beta
VMX_HD inline bool accept_tempered(bool inside, bool ok, double factor, double beta, double lnl_new, double lnl_old, uint64_t x2)
{
    const double a = tempered(beta, lnl_new), b = tempered(beta, lnl_old);
    return accept(inside, ok, factor, a, b, x2);
}

// the block of the rotation of the pair (rung t - 1, rung t) at global step s
VMX_HD inline Block shift_block(int64_t s, int t, uint64_t seed, uint64_t stream)
{
    return philox4x64_10(0, (uint64_t)s, (uint64_t)t, 3, seed, stream);
}

// the block of pair k of (rung t - 1, rung t) at global step s: w0 the acceptance word
VMX_HD inline Block swap_block(int64_t k, int64_t s, int t, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)k, (uint64_t)s, (uint64_t)t, 2, seed, stream);
}

// the rotation r in [0, W): walker k of the colder rung meets walker (k + r) mod W of the hotter one
VMX_HD inline int64_t swap_shift(uint64_t w0, int64_t W) { return partner(w0, W); }

VMX_HD inline int64_t swap_partner(int64_t k, int64_t r, int64_t W)
{
    const int64_t j = k + r;
    return j >= W ? j - W : j;
}

VMX_HD inline bool swap_accept(double beta_cold, double beta_hot, double lnl_cold, double lnl_hot, uint64_t word)
{
    VMX_NO_CONTRACT
    const double db = beta_cold - beta_hot;
    const double dl = lnl_hot - lnl_cold;
    const double lhs = db * dl;
    return lhs > log(u01(word));
}

// a sweep is due after global step s
VMX_HD inline bool swap_due(int64_t s, int32_t swap_every) { return swap_every > 0 && (s + 1) % swap_every == 0; }

}  // namespace vmx_ens

// ---- adaptive ladders (vmx_ensemble_run_pt_adapt: k_ens_swap_adapt), the fourth part
//
// Vousden, Farr & Mandel 2016, ptemcee's _get_ladder_adjustment: after a whole swap sweep the intermediate betas of a ladder move
// so that all adjacent pairs of rungs come to swap at the same rate; the adjustment decays, so that the chain becomes a proper one.
//
//   ratios           A_t = (double)accepted_t / (double)W for the pair (rung t, rung t + 1), t = 0 .. T - 2: the accepted swaps of
//                    this sweep alone, every pair of which was decided with the old ladder.
//   time             the number of sweeps before this one: (s + 1) / swap_every - 1 for the sweep after global step s, a function
//                    of the global step only (a run cut into calls adapts identically).
//   strength         decay = lag / (time + lag); kappa = decay / tau (ptemcee's adaptation_lag and adaptation_time, in sweeps).
//   rule             sum = 1 / beta[0]; for i = 0 .. T - 3 in order: dS = kappa (A_i - A_{i+1});
//                    gap = (1 / beta[i + 1] - 1 / beta[i]) pexp(dS); sum = sum + gap; beta'[i + 1] = 1 / sum - every operation
//                    rounded on its own, the betas on the right the old ones, pexp the pinned exponential of vmx_smc.h.
//                    beta[0] = 1 and beta[T - 1] (0 or positive) never move.
//   guard            a new ladder that is not ladder_ok (finite, strictly decreasing, the fixed last rung included - a positive
//                    last beta can be crossed) is dropped: the old one stays for this sweep and the ladder's adapt_skipped count
//                    goes up by one.
//   when             the sweep after global step s adapts iff adapt_until < 0 or s < adapt_until.
namespace vmx_ens {

// what the adaptive run takes beside a ladder: T >= 3 rungs, sweeps, lag and tau finite and positive
VMX_HD inline bool adapt_ok(int T, int32_t swap_every, double lag, double tau)
{
    return T >= 3 && T <= PT_MAXT && swap_every > 0 && is_finite(lag) && lag > 0.0 && is_finite(tau) && tau > 0.0;
}

// the number of sweeps before the one after global step s
VMX_HD inline int64_t sweep_time(int64_t s, int32_t swap_every) { return (s + 1) / swap_every - 1; }

VMX_HD inline bool adapt_due(int64_t s, int64_t adapt_until) { return adapt_until < 0 || s < adapt_until; }

// one ladder after one sweep: beta[T] in and out, accepted[T - 1] the sweep's accepted swaps per pair of rungs (any integer type);
// false: the guard held and beta is what it was
template <class Count>
VMX_HD inline bool ladder_adjust(double* beta, const Count* accepted, int T, int64_t W, int64_t time, double lag, double tau)
{
    VMX_NO_CONTRACT
    if (T < 3 || T > PT_MAXT) return true;          // (nothing between the two fixed rungs)
    const double tl = (double)time + lag;
    const double decay = lag / tl;
    const double kappa = decay / tau;
    double fresh[PT_MAXT];
    fresh[0] = beta[0];
    fresh[T - 1] = beta[T - 1];
    double sum = 1.0 / beta[0];
    for (int i = 0; i + 2 < T; ++i) {
        const double a0 = (double)accepted[i] / (double)W;
        const double a1 = (double)accepted[i + 1] / (double)W;
        const double da = a0 - a1;
        const double dS = kappa * da;
        const double inv_hot = 1.0 / beta[i + 1];
        const double inv_cold = 1.0 / beta[i];
        const double dT = inv_hot - inv_cold;
        const double gap = dT * vmx_smc::pexp(dS);
        sum = sum + gap;
        fresh[i + 1] = 1.0 / sum;
    }
    if (!ladder_ok(fresh, T)) return false;
    for (int t = 1; t + 1 < T; ++t) beta[t] = fresh[t];
    return true;
}

}  // namespace vmx_ens
