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

// ---- ensemble slice sampling (vmx_ensemble_run_slice: k_ens_slice_advance, k_ens_slice_emit), the fifth part
//
// Karamanis & Beutler 2021 (zeus's differential move): the direction of a walker's update comes from two walkers of the other
// half, so the move is affine-invariant like the ones above; the step along it is a slice-sampling bracket (Neal 2003: stepping
// out, then shrinkage), so no update is rejected; the length scale mu tunes itself from the counts of expansions and
// contractions.  One step is two halves, as ever: in half h of global step s walker-in-half k of the active half (H = W / 2)
// makes one update against the other half c, which is fixed for the whole half-step.  Only + - x / log, each rounded on its own.
//
//   random numbers   walker k reads the blocks with counter (k, s, 2 j + h, 6) under the key (seed, stream), j = 0, 1, ... its own
//                    block index within this update (the parts above use the last words 0 - 3, the nested and SMC samplers 1 - 5
//                    under their own rules: 6 is free).  Block 0: w0 -> j1 = partner(w0, H); w1 -> j2 = partner2(w1, H, j1);
//                    w2 -> the slice height lnY = lnL_k + log(u01(w2)); w3 -> the bracket, r = u01(w3), L = -r, R = L + 1.
//                    Every shrink draw takes the next unused word (w0 of block 1, w1 of block 1, ...: word index `draw` of the
//                    walker, block draw / 4, word draw % 4); stepping out draws nothing.  A walker's stream depends on (k, s, h)
//                    and its own history alone: the run is the same however rows are cut into chunks, lanes or calls.
//   direction        eta_q = mu (c[j1]_q - c[j2]_q) per column, the difference first.  Every eta_q exactly 0: no update, the
//                    walker stays (END_NULL).  A trial point is y_q = x_q + t eta_q, the product first.
//   answer           of the trial point at t: outside the box in any column -inf, given by the machine itself without an engine
//                    row (counted as box); inside, a request goes to the engine and the answer is log_lik(log_norm, chi2), or
//                    -inf when model_ok fails (counted as failed).  In the slice iff answer > lnY, strictly.
//   machine          LEFT: the trial is t = L; in the slice: L = L - 1, one expansion, and LEFT again unless that was the
//                    max_expansions-th of this side; else RIGHT.  RIGHT: likewise with t = R, R = R + 1; then SHRINK with
//                    t = L + (R - L) u01(next word) (the difference, the product, the sum).  SHRINK: in the slice: the walker
//                    moves to t and takes that lnL (END_MOVED); else L = t if t < 0, else R = t, one contraction, and after
//                    max_contractions of them the update ends where it began (END_CAPPED); else the next t.  The machine keeps
//                    answering itself (slice_settle) until it holds a request inside the box or is done: a round carries real
//                    evaluations only, and no row is ever a walker's own position.
//   scale            after both halves of a step with global index s < tune_steps: Ne = max(1, expansions), Nc = contractions of
//                    the step over all W walkers; mu <- mu (2 Ne / (Ne + Nc)) (zeus's rule; the sums in integers, one division,
//                    one product); a product that is not a positive normal number leaves mu as it was.  The rule reads the
//                    global step alone: a run cut into calls tunes identically.
//   the set round    every ensemble still running gives each of its walkers the answer of the row it asked for, advances the
//                    machines and counts its requests; at 0 the half is over: it is committed (slice_commit), at a step's end mu
//                    is tuned, the counters are added and the chain row written when due, and unless its steps are done the next
//                    half opens - so it has requests again (or the next half is over at once, and so on).  Ensembles do not wait
//                    for each other.  Rows are packed in ascending (ensemble, walker) order: a walker's place among its
//                    ensemble's requests is the number of requesting walkers before it, the ensemble's offset the sum of the
//                    counts of the running ensembles before it (slice_offsets).  No atomic decides a row.
constexpr int SLICE_MAX_EXPANSIONS = 32, SLICE_MAX_CONTRACTIONS = 64;
enum SlicePhase { SLICE_LEFT = 0, SLICE_RIGHT = 1, SLICE_SHRINK = 2, SLICE_DONE = 3 };
enum SliceEnd { END_NONE = 0, END_MOVED = 1, END_CAPPED = 2, END_NULL = 3 };
// the counts of a run, per ensemble: [SLICE_COUNTS]
enum SliceCount { SC_UPDATES = 0, SC_MOVED, SC_ROWS, SC_EXPANSIONS, SC_CONTRACTIONS, SC_BOX, SC_FAILED, SC_CAPPED_NULL, SLICE_COUNTS };

// a walker's update: the bracket, the trial, the height, the lnL it moved to; where the machine is, the next unused word, and
// the update's own counts (left, right: the expansions of either side); asks: a request is out, its answer is due
struct SliceWalker {
    double L, R, t, lnY, lnl;
    int32_t phase, draw, left, right, contractions, rows, box, failed, end, asks;
};

VMX_HD inline Block slice_block(int64_t k, int64_t s, int h, int64_t j, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)k, (uint64_t)s, 2 * (uint64_t)j + (uint64_t)h, 6, seed, stream);
}

// the walker's next unused word
VMX_HD inline uint64_t slice_word(SliceWalker& w, int64_t k, int64_t s, int h, uint64_t seed, uint64_t stream)
{
    const int32_t i = w.draw;
    w.draw = i + 1;
    const Block b = slice_block(k, s, h, i / 4, seed, stream);
    const int r = i % 4;        // (selected, not indexed: a lane's array indexed at run time would live in scratch memory)
    return r == 0 ? b.w[0] : (r == 1 ? b.w[1] : (r == 2 ? b.w[2] : b.w[3]));
}

VMX_HD inline double slice_eta(double mu, double c1, double c2)
{
    VMX_NO_CONTRACT
    const double d = c1 - c2;
    return mu * d;
}

// one column of the trial point at t
VMX_HD inline double slice_point(double x, double t, double eta)
{
    VMX_NO_CONTRACT
    const double p = t * eta;
    return x + p;
}

VMX_HD inline double slice_height(double lnl, uint64_t w2)
{
    VMX_NO_CONTRACT
    return lnl + log(u01(w2));
}

VMX_HD inline double slice_shrink(double L, double R, uint64_t word)
{
    VMX_NO_CONTRACT
    const double d = R - L;
    const double m = d * u01(word);
    return L + m;
}

// the trial point at t lies in the box (a NaN lies outside)
VMX_HD inline bool slice_inside(int n, const double* x, double t, const double* eta, const double* lo, const double* hi)
{
    bool in = true;
    for (int q = 0; q < n; ++q) {
        const double y = slice_point(x[q], t, eta[q]);
        in = in && y >= lo[q] && y <= hi[q];
    }
    return in;
}

// the engine's answer of a request; *failed goes up when the model failed
VMX_HD inline double slice_answer(double log_norm, int32_t status, double chi2, int32_t* failed)
{
    if (model_ok(status, chi2)) return log_lik(log_norm, chi2);
    *failed += 1;
    return -INFINITY;
}

// the machine takes the answer of its trial
VMX_HD inline void slice_take(SliceWalker& w, double answer, int max_e, int max_c, int64_t k, int64_t s, int h, uint64_t seed,
                              uint64_t stream)
{
    VMX_NO_CONTRACT
    const bool in = answer > w.lnY;
    if (w.phase == SLICE_LEFT) {
        if (in) { w.L = w.L - 1.0; w.left += 1; }
        if (in && w.left < max_e) { w.t = w.L; return; }
        w.phase = SLICE_RIGHT;
        w.t = w.R;
        return;
    }
    if (w.phase == SLICE_RIGHT) {
        if (in) { w.R = w.R + 1.0; w.right += 1; }
        if (in && w.right < max_e) { w.t = w.R; return; }
        w.phase = SLICE_SHRINK;
        w.t = slice_shrink(w.L, w.R, slice_word(w, k, s, h, seed, stream));
        return;
    }
    if (w.phase != SLICE_SHRINK) return;
    if (in) { w.lnl = answer; w.end = END_MOVED; w.phase = SLICE_DONE; return; }
    if (w.t < 0.0) w.L = w.t; else w.R = w.t;
    w.contractions += 1;
    if (w.contractions >= max_c) { w.end = END_CAPPED; w.phase = SLICE_DONE; return; }
    w.t = slice_shrink(w.L, w.R, slice_word(w, k, s, h, seed, stream));
}

// the machine answers itself until it holds a request inside the box (asks = 1) or is done
VMX_HD inline void slice_settle(SliceWalker& w, int n, const double* x, const double* eta, const double* lo, const double* hi, int max_e,
                                int max_c, int64_t k, int64_t s, int h, uint64_t seed, uint64_t stream)
{
    w.asks = 0;
    while (w.phase != SLICE_DONE) {
        if (slice_inside(n, x, w.t, eta, lo, hi)) { w.asks = 1; w.rows += 1; return; }
        w.box += 1;
        slice_take(w, -INFINITY, max_e, max_c, k, s, h, seed, stream);
    }
}

// a walker's update opens: block 0, the direction eta[n] from the other half `other` [H][n], the height and the bracket; then the
// machine settles on its first request
VMX_HD inline void slice_open(SliceWalker& w, double* eta, int n, const double* x, double lnl, const double* other, int64_t H, double mu,
                              const double* lo, const double* hi, int max_e, int max_c, int64_t k, int64_t s, int h, uint64_t seed,
                              uint64_t stream)
{
    VMX_NO_CONTRACT
    const Block b = slice_block(k, s, h, 0, seed, stream);
    const int64_t j1 = partner(b.w[0], H), j2 = partner2(b.w[1], H, j1);
    bool null = true;
    for (int q = 0; q < n; ++q) {
        eta[q] = slice_eta(mu, other[j1 * n + q], other[j2 * n + q]);
        null = null && eta[q] == 0.0;
    }
    w.lnY = slice_height(lnl, b.w[2]);
    const double r = u01(b.w[3]);
    w.L = -r;
    w.R = w.L + 1.0;
    w.t = w.L;
    w.lnl = lnl;
    w.phase = null ? SLICE_DONE : SLICE_LEFT;
    w.end = null ? END_NULL : END_NONE;
    w.draw = 4;
    w.left = w.right = w.contractions = w.rows = w.box = w.failed = 0;
    slice_settle(w, n, x, eta, lo, hi, max_e, max_c, k, s, h, seed, stream);
}

// the answer of the walker's request has come: (status, chi2) of its engine row
VMX_HD inline void slice_advance(SliceWalker& w, int n, const double* x, const double* eta, const double* lo, const double* hi,
                                 double log_norm, int32_t status, double chi2, int max_e, int max_c, int64_t k, int64_t s, int h,
                                 uint64_t seed, uint64_t stream)
{
    const double answer = slice_answer(log_norm, status, chi2, &w.failed);
    slice_take(w, answer, max_e, max_c, k, s, h, seed, stream);
    slice_settle(w, n, x, eta, lo, hi, max_e, max_c, k, s, h, seed, stream);
}

// the half is over: a walker that moved goes to its trial point - the row the engine evaluated, bit for bit - and takes its lnL;
// the update's counts go to counts[SLICE_COUNTS] (any integer type).  Returns 1 if the walker moved.
template <class Count>
VMX_HD inline int slice_commit(const SliceWalker& w, int n, double* x, const double* eta, double* lnl, Count* counts)
{
    const int moved = w.end == END_MOVED ? 1 : 0;
    if (moved) {
        for (int q = 0; q < n; ++q) x[q] = slice_point(x[q], w.t, eta[q]);
        *lnl = w.lnl;
    }
    counts[SC_UPDATES] += 1;
    counts[SC_MOVED] += moved;
    counts[SC_ROWS] += w.rows;
    counts[SC_EXPANSIONS] += w.left + w.right;
    counts[SC_CONTRACTIONS] += w.contractions;
    counts[SC_BOX] += w.box;
    counts[SC_FAILED] += w.failed;
    counts[SC_CAPPED_NULL] += w.end == END_CAPPED || w.end == END_NULL ? 1 : 0;
    return moved;
}

// a step with global index s tunes the scale
VMX_HD inline bool slice_tune_due(int64_t s, int32_t tune_steps) { return s < (int64_t)tune_steps; }

// zeus's rule from the step's expansions and contractions over all walkers
VMX_HD inline double slice_tune(double mu, int64_t expansions, int64_t contractions)
{
    VMX_NO_CONTRACT
    const int64_t ne = expansions < 1 ? 1 : expansions;
    const double num = 2.0 * (double)ne;
    const double den = (double)(ne + contractions);
    const double f = num / den;
    const double m = mu * f;
    return m >= 0x1.0p-1022 && m <= 0x1.fffffffffffffp+1023 ? m : mu;
}

// what the run takes beside what vmx_ensemble_run_many takes
VMX_HD inline bool slice_ok(int64_t H, double mu0, int32_t tune_steps, int32_t max_e, int32_t max_c, int32_t flags)
{
    return H >= 2 && is_finite(mu0) && mu0 > 0.0 && tune_steps >= 0 && max_e >= 1 && max_e <= SLICE_MAX_EXPANSIONS && max_c >= 1 &&
           max_c <= SLICE_MAX_CONTRACTIONS && flags == 0;
}

// the half-step q of a call that starts at global step step0: its step and half
VMX_HD inline int64_t slice_step(int64_t step0, int64_t q) { return step0 + q / 2; }VMX_HD inline int slice_half(int64_t q) { return (int)(q % 2); }

// the packing of a round: offset[a] of the a-th running ensemble is the sum of the counts before it in list order; the total
VMX_HD inline int32_t slice_offsets(const int32_t* count, int A, int32_t* offset)
{
    int32_t total = 0;
    for (int a = 0; a < A; ++a) { if (offset) offset[a] = total; total += count[a]; }
    return total;
}

// the running list after a round: an ensemble that asked for nothing has done its steps and leaves, the order stays
VMX_HD inline int slice_compact(int32_t* active, int A, const int32_t* count_of)
{
    int B = 0;
    for (int a = 0; a < A; ++a)
        if (count_of[active[a]] > 0) active[B++] = active[a];
    return B;
}

}  // namespace vmx_ens

// ---- the covariance move (vmx_ensemble_run_many_cov: k_ens_half_cov), the sixth part
//
// A Metropolis step whose increment has the covariance of the complementary half: emcee's WalkMove taken over the whole other
// half, with the Roberts-Gelman-Gilks scale.  A red-blue move like the others: the factor below depends on the other half alone,
// which is fixed for the whole half-step, so the move is reversible by the same argument.  Only + - x / sqrt, each rounded on its
// own.  (tests/helpers/ensemble_cov_driver.cpp compiles this part for tests/test_ensemble_cov_host.py.)
//
//   the factor       for the half-step that proposes half h the other half c[H][n] is fixed: mean_a = (sum_i c_ia) / H and
//                    cov_ab = (sum_i (c_ia - mean_a)(c_ib - mean_b)) / (H - 1), both summed in walker order with one accumulator
//                    from 0.0 (half_mean_entry, half_cov_entry: the order of vmx_ns::mean_entry and cov_entry).  C is the lower
//                    Cholesky factor in the operation order of vmx_ns::cholesky - column by column, the inner sums in k order
//                    (chol_pivot, chol_entry; in place: the lower triangle of cov goes in, C comes out).  A pivot that is not
//                    positive: C = diag(sqrt(cov_aa)), 0 where cov_aa is not positive (vmx_ns::whiten's fallback), and the
//                    half-step counts as a fallback.  Every entry is a function of its inputs alone: a work-group that gives
//                    every entry to one thread computes the factor of half_factor bit for bit.
//   the variate      one 64-bit word w gives z = ((double)(a0 + a1 + a2 + a3) - 131070) kappa, a0 .. a3 the four 16-bit fields
//                    of w, kappa = sqrt(3 / 4294967295): symmetric about 0, of unit variance, |z| <= 2 sqrt(3), exact in integers
//                    up to the last product.  It is not normal (the sum of four uniforms): like the triangular DE jitter it is
//                    symmetric and independent of the state, which is all reversibility needs.
//   the words        column b of walker-in-half k at step s, half h takes word b % 4 of the block with counter
//                    (k, s, h, 2 + b / 4); blocks 0 and 1 stay what they are (the move is refused with tempering and with
//                    slice sampling, whose blocks carry the last words 2, 3 and 6).
//   the proposal     y_a = s_a + gamma_c (sum_{b <= a} C_ab z_b): the sum in b order from 0.0, the product by gamma_c a rounding
//                    of its own; factor = 0.  gamma_c comes from the host as a double (default 2.38 / sqrt(n)).
//   the mixture      weights (p_stretch, p_de, p_snooker, p_cov): t0 and t1 as above but over the sum of all four,
//                    t2 = (p0 + p1 + p2) / sum; the move is cov when u(B.w0) >= t2, else move_choice.  With p_cov = 0 the sum,
//                    t0 and t1 are those of three weights.  A pure cov run draws from the same words.
//   box, decision    unchanged.
namespace vmx_ens {

constexpr int MOVE_COV = 3;

// the thresholds of the weights (p_stretch, p_de, p_snooker, p_cov)
VMX_HD inline void move_thresholds4(const double* p, double& t0, double& t1, double& t2)
{
    VMX_NO_CONTRACT
    const double p01 = p[0] + p[1];
    const double p012 = p01 + p[2];
    const double sum = p012 + p[3];
    t0 = p[0] / sum;
    t1 = p01 / sum;
    t2 = p012 / sum;
}

VMX_HD inline int move_choice4(uint64_t w0, double t0, double t1, double t2)
{
    return u01(w0) >= t2 ? MOVE_COV : move_choice(w0, t0, t1);
}

// what the run takes beside what the moves entry takes
VMX_HD inline bool cov_ok(double weight, double scale, uint32_t flags, uint32_t reserved)
{
    return is_finite(weight) && weight >= 0.0 && is_finite(scale) && scale > 0.0 && flags == 0 && reserved == 0;
}

// the mean of column a over the half c[H][n].  (The rows are read HALF_BATCH at a time ahead of the sum, so that a device thread
// has that many loads in flight instead of one per addition; the additions are the same ones in the same order.)
constexpr int HALF_BATCH = 8;
VMX_HD inline double half_mean_entry(int a, const double* c, int64_t H, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    int64_t i = 0;
    for (; i + HALF_BATCH <= H; i += HALF_BATCH) {
        double v[HALF_BATCH];
        for (int u = 0; u < HALF_BATCH; ++u) v[u] = c[(size_t)(i + u) * n + a];
        for (int u = 0; u < HALF_BATCH; ++u) acc = acc + v[u];
    }
    for (; i < H; ++i) acc = acc + c[(size_t)i * n + a];
    return acc / (double)H;
}

VMX_HD inline double half_cov_entry(int a, int b, const double* c, const double* mean, int64_t H, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    const double ma = mean[a], mb = mean[b];
    int64_t i = 0;
    for (; i + HALF_BATCH <= H; i += HALF_BATCH) {
        double va[HALF_BATCH], vb[HALF_BATCH];
        for (int u = 0; u < HALF_BATCH; ++u) { va[u] = c[(size_t)(i + u) * n + a]; vb[u] = c[(size_t)(i + u) * n + b]; }
        for (int u = 0; u < HALF_BATCH; ++u) {
            const double da = va[u] - ma;
            const double db = vb[u] - mb;
            const double p = da * db;
            acc = acc + p;
        }
    }
    for (; i < H; ++i) {
        const double da = c[(size_t)i * n + a] - ma;
        const double db = c[(size_t)i * n + b] - mb;
        const double p = da * db;
        acc = acc + p;
    }
    return acc / (double)(H - 1);
}

// entry q = a (a + 1) / 2 + b of the lower triangle, b <= a
VMX_HD inline void tri_entry(int q, int& a, int& b)
{
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= q) ++a;
    b = q - a * (a + 1) / 2;
}

// The factor in place, C[n][ld] (ld >= n the row stride): columns k < j hold the factor, column j the covariance.
// What is under the root of pivot j; the pivot is its sqrt when it is positive
VMX_HD inline double chol_pivot(int j, const double* C, int ld)
{
    VMX_NO_CONTRACT
    double s = C[j * ld + j];
    for (int k = 0; k < j; ++k) {
        const double p = C[j * ld + k] * C[j * ld + k];
        s = s - p;
    }
    return s;
}

// entry (i, j), i > j, of the factor, given pivot j
VMX_HD inline double chol_entry(int i, int j, const double* C, int ld, double piv)
{
    VMX_NO_CONTRACT
    double t = C[i * ld + j];
    for (int k = 0; k < j; ++k) {
        const double p = C[i * ld + k] * C[j * ld + k];
        t = t - p;
    }
    return t / piv;
}

VMX_HD inline double fallback_entry(double cov_aa) { return cov_aa > 0.0 ? sqrt(cov_aa) : 0.0; }

// The factor of the half c[H][n] (H >= 2), one entry after the other: mean[n], C[n][ld] (the strict upper triangle 0), diag[n] the
// covariance's diagonal.  true: the Cholesky factor; false: the diagonal fallback
VMX_HD inline bool half_factor(int n, int64_t H, const double* c, double* mean, double* C, int ld, double* diag)
{
    for (int a = 0; a < n; ++a) mean[a] = half_mean_entry(a, c, H, n);
    for (int a = 0; a < n; ++a) {
        for (int b = 0; b <= a; ++b) C[a * ld + b] = half_cov_entry(a, b, c, mean, H, n);
        for (int b = a + 1; b < n; ++b) C[a * ld + b] = 0.0;
        diag[a] = C[a * ld + a];
    }
    bool good = true;
    for (int j = 0; j < n && good; ++j) {
        const double s = chol_pivot(j, C, ld);
        if (!(s > 0.0)) { good = false; break; }
        const double piv = sqrt(s);
        C[j * ld + j] = piv;
        for (int i = j + 1; i < n; ++i) C[i * ld + j] = chol_entry(i, j, C, ld, piv);
    }
    if (good) return true;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) C[a * ld + b] = a == b ? fallback_entry(diag[a]) : 0.0;
    return false;
}

VMX_HD inline double cov_z(uint64_t w)
{
    VMX_NO_CONTRACT
    const double kappa = sqrt(3.0 / 4294967295.0);
    const uint64_t a = (w & 0xFFFFull) + ((w >> 16) & 0xFFFFull) + ((w >> 32) & 0xFFFFull) + (w >> 48);
    const double d = (double)a - 131070.0;
    return d * kappa;
}

// block j of the variates of walker-in-half i at global step s, half h: the columns 4 j .. 4 j + 3
VMX_HD inline Block cov_block(int64_t i, int64_t s, int h, int j, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)i, (uint64_t)s, (uint64_t)h, 2 + (uint64_t)j, seed, stream);
}

// the variates z[n] of walker-in-half i
VMX_HD inline void cov_variates(int n, int64_t i, int64_t s, int h, uint64_t seed, uint64_t stream, double* z)
{
    for (int b = 0; b < n; b += 4) {
        const Block blk = cov_block(i, s, h, b / 4, seed, stream);
        z[b] = cov_z(blk.w[0]);
        if (b + 1 < n) z[b + 1] = cov_z(blk.w[1]);
        if (b + 2 < n) z[b + 2] = cov_z(blk.w[2]);
        if (b + 3 < n) z[b + 3] = cov_z(blk.w[3]);
    }
}

// The proposal of the walker at s[n], in place: y[n] holds the variates and takes the proposal (from the last column down: y_a
// reads the variates b <= a alone).  y must not overlap s.
VMX_HD inline void cov_propose(int n, const double* s, const double* C, int ld, double gamma_c, double* y)
{
    VMX_NO_CONTRACT
    for (int a = n - 1; a >= 0; --a) {
        double acc = 0.0;
        for (int b = 0; b <= a; ++b) {
            const double p = C[a * ld + b] * y[b];
            acc = acc + p;
        }
        const double t = gamma_c * acc;
        y[a] = s[a] + t;
    }
}

}  // namespace vmx_ens
