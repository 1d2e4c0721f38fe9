// Tempered sequential Monte Carlo (the scheme of pocoMC without its normalising flow), pinned decision for decision.
//
// N particles walk from the prior (beta = 0) to the posterior (beta = 1) along a ladder of inverse temperatures chosen by the
// effective sample size; every stage reweights, resamples, whitens and moves all particles by `sweeps` Metropolis sweeps under
// L^beta.  The loop runs where the particles are (vmx_smc_run, vegamx.hip: k_smc_stage once per stage, k_smc_move once per
// sweep, one work-group per run); vega_amd/smc.py restates every expression below in NumPy (the `python` driver) and tests/helpers/smc_driver.cpp compiles
// this header with g++ so that tests/test_smc_host.py can hold the two against each other bit for bit.  No HIP type, no heap.
//
//   cube             particles live in u in [0, 1]^n (vmx_ns::map_cube: a uniform prior over the limits); lnL = log_norm - 0.5 chi2,
//                    -inf for a failed model (vmx_ns::lnl_of).  Target of stage t: L^beta_t inside the cube.
//   random numbers   vmx_ens::philox4x64_10 keyed (seed, stream), a uniform double from a word by vmx_ens::u01.  Counters (word 0
//                    first):  start particle i      (i, 0, j, 5)                    coordinate c: word c % 4 of block j = c / 4
//                             resampling of stage t (0, t, 0, 4)                    word 0 is v
//                             particle i, stage t, sweep s  (i, t 2^32 + s, j, 3)   words q = 0 .. n from blocks j = q / 4, word q % 4:
//                                                                                   g_q = 2 u - 1 for q < n, word n decides
//                    A particle's stream depends on nothing but (i, t, s).  Stages count from 0 over the whole run.
//   exp              pexp below: range reduction by k = floor(x / ln 2 + 1/2) with a two-word ln 2, a degree-13 Horner polynomial
//                    in the remainder, a power of two - separately rounded operations only, so that NumPy restates it bit for
//                    bit.  Nothing that decides calls the C library.
//   a stage t        given beta_{t-1} and lnL_i:
//     weights        d_i = lnL_i - max_j lnL_j;  w_i(beta) = pexp((beta - beta_{t-1}) d_i), 0 where lnL_i = -inf.
//     sums           S1 = sum w_i and S2 = sum w_i^2 by the stride-halving tree over the array padded with zeros to M, the power
//                    of two >= N: for s = M/2, M/4 .. 1: a_i = a_i + a_{i+s} (i < s); the sum is a_0.  ESS = S1 S1 / S2.
//     next beta      1 if ESS(1) >= ess N; otherwise [lo, hi] = [beta_{t-1}, 1] halved BISECTIONS times at mid = 0.5 (lo + hi),
//                    lo = mid where ESS(mid) >= ess N, hi = mid elsewhere; beta_t = lo.  No finite lnL at all, or beta_t =
//                    beta_{t-1} (fewer than ess N particles carry weight): the run ends with an error.
//     cumulative     q_i = w_i(beta_t) / S1.  Segments of L = ceil(N / LANES) consecutive particles, LANES of them (the last ones
//                    empty): r_i the running sum inside the segment from 0.0, T_j its total; the T_j scanned inclusively in
//                    log2 LANES rounds (step = 1, 2, 4 ..: T_j = T_j + T_{j-step} for j >= step, from the values of the round
//                    before); c_i = P_j + r_i with P_j the scanned total of segment j - 1 (0.0 for j = 0); c_{N-1} = 1.
//     resample       position p_i = (v + i) / N; ancestor a_i by the bisection  lo = 0, hi = N - 1; while lo < hi: mid =
//                    (lo + hi) / 2; c_mid > p_i ? hi = mid : lo = mid + 1.  Particle i becomes a copy of particle a_i.
//     precondition   mean, covariance and factor C of the resampled particles: vmx_ns::mean_entry / cov_entry over all of them
//                    (K = 0), vmx_ns::whiten with its diagonal fallback.
//     sweeps         s = 0 .. sweeps - 1: z_a = sum_{j <= a} C_aj g_j (in that order), y_a = u_a + scale z_a.  Outside the cube:
//                    rejected without an evaluation (the engine's row is the particle's own position).  Inside: accepted iff the
//                    model is ok and (D = beta_t (lnL_y - lnL_u) >= 0 or u01(word n) < pexp(D)).  After the sweep, with a =
//                    accepted / N: scale = 0.8 scale if a < 0.15, 1.25 scale if a > 0.35.
//   start            beta = 0, scale = 2.38 sqrt(3 / n); the scale carries over from stage to stage.  After the sweeps of the stage
//                    with beta_t = 1 the particles are the posterior sample, weight 1 / N each.
//
//   a set of runs   vmx_smc_run_many advances E such runs a stage per host round, one work-group per run (vmx_smc_run is the set
//                    of one, by the same host body and kernels); the status of a run and the list of the runs still going are
//                    decided at the end of this header (tests/helpers/smc_set_driver.cpp).
//
// Every expression is the separately rounded IEEE operations written below (contraction off, as in vmx_ensemble.h); sqrt and / are
// correctly rounded.  The evidence is computed from the stage record by host Python (vega_amd/smc.py: evidence).
#pragma once
#include <cstring>

#include "vmx_nested.h"

namespace vmx_smc {

constexpr int MAXN = vmx_ns::MAXN;
constexpr int MAX_PARTICLES = 4096;
constexpr int BISECTIONS = 60;
constexpr int LANES = 1024;                 // segments of the cumulative sum: the lanes of the work-group that computes it
constexpr uint64_t DOMAIN_MOVE = 3, DOMAIN_RESAMPLE = 4, DOMAIN_START = 5;

// ---- exp: pexp and its constants live in vmx_pexp.h (namespace vmx_smc, as ever), which vmx_ensemble.h includes

// ---- random numbers
VMX_HD inline vmx_ens::Block move_block(int64_t i, int64_t stage, int64_t sweep, int64_t j, uint64_t seed, uint64_t stream)
{
    return vmx_ens::philox4x64_10((uint64_t)i, ((uint64_t)stage << 32) + (uint64_t)sweep, (uint64_t)j, DOMAIN_MOVE, seed, stream);
}

VMX_HD inline double resample_uniform(int64_t stage, uint64_t seed, uint64_t stream)
{
    return vmx_ens::u01(vmx_ens::philox4x64_10(0, (uint64_t)stage, 0, DOMAIN_RESAMPLE, seed, stream).w[0]);
}

// start particle i: u[n]
VMX_HD inline void draw_start(int64_t i, int n, uint64_t seed, uint64_t stream, double* u)
{
    for (int c = 0; c < n; c += 4) {
        const vmx_ens::Block b = vmx_ens::philox4x64_10((uint64_t)i, 0, (uint64_t)(c / 4), DOMAIN_START, seed, stream);
        for (int q = 0; q < 4 && c + q < n; ++q) u[c + q] = vmx_ens::u01(b.w[q]);
    }
}

VMX_HD inline double start_scale(int n)
{
    VMX_NO_CONTRACT
    const double t = 3.0 / (double)n;
    return 2.38 * sqrt(t);
}

// ---- weights and their sums
VMX_HD inline int pad_pow2(int N) { int M = 1; while (M < N) M <<= 1; return M; }

VMX_HD inline double weight(double dbeta, double d)
{
    VMX_NO_CONTRACT
    if (d == -INFINITY) return 0.0;
    return pexp(dbeta * d);
}

VMX_HD inline double square(double w) { VMX_NO_CONTRACT return w * w; }

VMX_HD inline double ess_of(double s1, double s2)
{
    VMX_NO_CONTRACT
    const double t = s1 * s1;
    return t / s2;
}

VMX_HD inline double midpoint(double lo, double hi)
{
    VMX_NO_CONTRACT
    const double s = lo + hi;
    return 0.5 * s;
}

// the stride-halving tree over a[M] (destroyed), M a power of two
inline double tree_sum(double* a, int M)
{
    VMX_NO_CONTRACT
    for (int s = M / 2; s >= 1; s /= 2)
        for (int i = 0; i < s; ++i) a[i] = a[i] + a[i + s];
    return a[0];
}

// S1, S2 of the weights at beta_prev + dbeta; d[N], scratch[2 M]
inline void weight_sums(double dbeta, const double* d, int N, double* scratch, double& s1, double& s2)
{
    const int M = pad_pow2(N);
    double* a = scratch;
    double* b = scratch + M;
    for (int i = 0; i < M; ++i) {
        const double w = i < N ? weight(dbeta, d[i]) : 0.0;
        a[i] = w;
        b[i] = square(w);
    }
    s1 = tree_sum(a, M);
    s2 = tree_sum(b, M);
}

// beta_t from beta_{t-1}; ess_out = ESS(beta_t), s1_out = S1(beta_t).  NaN: no particle has a finite lnL (d is then unusable).
inline double next_beta(double beta_prev, const double* d, int N, double target, double* scratch, double& ess_out, double& s1_out)
{
    VMX_NO_CONTRACT
    double s1, s2;
    double beta = 1.0;
    weight_sums(1.0 - beta_prev, d, N, scratch, s1, s2);
    if (!(ess_of(s1, s2) >= target)) {
        double lo = beta_prev, hi = 1.0;
        for (int it = 0; it < BISECTIONS; ++it) {
            const double mid = midpoint(lo, hi);
            weight_sums(mid - beta_prev, d, N, scratch, s1, s2);
            if (ess_of(s1, s2) >= target) lo = mid; else hi = mid;
        }
        beta = lo;
        weight_sums(beta - beta_prev, d, N, scratch, s1, s2);
    }
    ess_out = ess_of(s1, s2);
    s1_out = s1;
    return beta;
}

// ---- cumulative weights and ancestors
VMX_HD inline int segment_length(int N) { return (N + LANES - 1) / LANES; }

// running sum of segment j: c[i] = r_i for its particles, returns the total
VMX_HD inline double segment_sums(int j, const double* w, double s1, int N, double* c)
{
    VMX_NO_CONTRACT
    const int L = segment_length(N);
    double r = 0.0;
    for (int i = j * L; i < (j + 1) * L && i < N; ++i) {
        const double q = w[i] / s1;
        r = r + q;
        c[i] = r;
    }
    return r;
}

// c[N] from w[N]; totals[2 LANES] scratch
inline void cumulative(const double* w, double s1, int N, double* totals, double* c)
{
    VMX_NO_CONTRACT
    double* t = totals;
    double* t2 = totals + LANES;
    for (int j = 0; j < LANES; ++j) t[j] = segment_sums(j, w, s1, N, c);
    for (int step = 1; step < LANES; step <<= 1) {
        for (int j = 0; j < LANES; ++j) t2[j] = j >= step ? t[j] + t[j - step] : t[j];
        for (int j = 0; j < LANES; ++j) t[j] = t2[j];
    }
    const int L = segment_length(N);
    for (int i = 0; i < N; ++i) {
        const int j = i / L;
        const double pre = j > 0 ? t[j - 1] : 0.0;
        c[i] = pre + c[i];
    }
    c[N - 1] = 1.0;
}

VMX_HD inline double position(double v, int i, int N)
{
    VMX_NO_CONTRACT
    const double s = v + (double)i;
    return s / (double)N;
}

VMX_HD inline int ancestor(const double* c, int N, double p)
{
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (c[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- a sweep
// the proposal of particle i at (stage, sweep) from u[n] into y[n] (no overlap); ua: the uniform that decides.  true: y in the cube
VMX_HD inline bool propose(int64_t i, int64_t stage, int64_t sweep, int n, const double* C, double scale, const double* u,
                           uint64_t seed, uint64_t stream, double* y, double& ua)
{
    VMX_NO_CONTRACT
    for (int q = 0; q <= n; q += 4) {       // (y holds g first)
        const vmx_ens::Block b = move_block(i, stage, sweep, q / 4, seed, stream);
        for (int w = 0; w < 4 && q + w <= n; ++w) {
            const double x = vmx_ens::u01(b.w[w]);
            if (q + w < n) { const double two = 2.0 * x; y[q + w] = two - 1.0; }
            else ua = x;
        }
    }
    bool in = true;
    for (int a = n - 1; a >= 0; --a) {      // (z_a reads g_0 .. g_a: from the last row up, each slot is free when it is written)
        double acc = 0.0;
        for (int j = 0; j <= a; ++j) { const double p = C[a * n + j] * y[j]; acc = acc + p; }
        const double step = scale * acc;
        const double v = u[a] + step;
        y[a] = v;
        in = in && v >= 0.0 && v <= 1.0;
    }
    return in;
}

VMX_HD inline bool accept(bool inside, bool ok, double beta, double lnl_new, double lnl_old, double ua)
{
    VMX_NO_CONTRACT
    if (!inside || !ok) return false;
    const double dl = lnl_new - lnl_old;
    const double delta = beta * dl;
    if (delta >= 0.0) return true;
    return ua < pexp(delta);
}

VMX_HD inline double adapt(double scale, int64_t accepted, int N)
{
    VMX_NO_CONTRACT
    const double a = (double)accepted / (double)N;
    if (a < 0.15) return scale * 0.8;
    if (a > 0.35) return scale * 1.25;
    return scale;
}

// ---- a set of runs (vmx_smc_run_many): E independent runs advanced a stage per host round; nothing below crosses runs
// A run's status: RUNNING while beta < 1 (also the status of a run whose call ran out of stages), FINISHED at beta = 1, NO_FINITE
// when no particle has a finite lnL (the stage head reports beta = NaN), STUCK when the ladder cannot advance (beta_t =
// beta_{t-1}).  The last two end the run without ending the set.
constexpr int RUNNING = 0, FINISHED = 1, NO_FINITE = 2, STUCK = 3;

// after a stage round: beta_before the run's beta at the head of the stage, beta_after the word its kernels handed back
VMX_HD inline int run_status(double beta_before, double beta_after)
{
    if (beta_after != beta_after) return NO_FINITE;
    if (!(beta_after > beta_before)) return STUCK;
    return beta_after >= 1.0 ? FINISHED : RUNNING;
}

// after the start: `finite` of the N drawn particles have a finite lnL
VMX_HD inline int start_status(double finite) { return finite > 0.0 ? RUNNING : NO_FINITE; }

// the runs a call begins with, in ascending order: every run with draw, the runs with beta < 1 otherwise.  Returns their number;
// status[e] = FINISHED for the others.
VMX_HD inline int first_active(const double* beta, int E, bool draw, int32_t* active, int32_t* status)
{
    int A = 0;
    for (int e = 0; e < E; ++e) {
        status[e] = draw || beta[e] < 1.0 ? RUNNING : FINISHED;
        if (status[e] == RUNNING) active[A++] = e;
    }
    return A;
}

// drop the runs that are no longer RUNNING; the rest keep their (ascending) order and move up: run active[a] owns the engine rows
// a N .. (a + 1) N - 1 of the next round.  Returns the new number.
VMX_HD inline int compact_active(int32_t* active, int A, const int32_t* status)
{
    int B = 0;
    for (int a = 0; a < A; ++a)
        if (status[active[a]] == RUNNING) active[B++] = active[a];
    return B;
}

// ---- kept populations and posterior rounds (vmx_smc_run_kept, vmx_smc_run_many_kept)
// A weighted posterior from every population the run walked through (vega_amd/smc.py: recycled_weights) needs their positions,
// and more points at beta = 1 need more moves there.
//   kept population  the population a stage reweights is the particles at its entry: their lnL is the stage's rec_lnl row, their
//                    positions go to the row of the same index of rec_u [stages][N][n].  The final particles are the last
//                    population.
//   posterior round  a stage entered with beta_prev = 1.  No bisection, no weights, no resampling uniform (the block (0, t, 0, 4)
//                    of that stage is not read); the ancestors are the identity.  Record row: beta_prev = beta = 1, ESS = the
//                    number of particles with a finite lnL; rec_lnl and rec_u the particles at entry.  Mean, covariance and
//                    factor of the particles as they stand (mean_entry / cov_entry / whiten, fallback included), then the
//                    stage's sweeps through the unchanged propose / accept / adapt at beta = 1.  The Philox stage index is the
//                    run's global stage index, which keeps counting: a run is the same however it is cut, also inside the rounds.
//   rounds owed      topups_left is state beside stage, beta and scale.  beta >= 1 and topups_left = 0: the run is finished;
//                    beta >= 1 and topups_left > 0: the next stage is a posterior round, which pays one.  n_stages of a call bounds
//                    ladder stages and posterior rounds together, one record row each.
//   a set            a run at beta = 1 that owes rounds stays RUNNING and in the active list; it is FINISHED in the round that
//                    pays the last one.  compact_active reads nothing but the statuses and serves both forms.
VMX_HD inline bool posterior_round(double beta_prev) { return beta_prev >= 1.0; }

// nothing is left to do
VMX_HD inline bool run_finished(double beta, int32_t topups_left) { return beta >= 1.0 && topups_left <= 0; }

// ESS of a posterior round's record row: the particles with a finite lnL
VMX_HD inline double round_ess(const double* lnl, int N)
{
    int c = 0;
    for (int i = 0; i < N; ++i) c += lnl[i] > -INFINITY ? 1 : 0;
    return (double)c;
}

// the head of a posterior round over u[N][n], lnl[N] (both left as they are): row[0 .. 2] = 1, 1, ESS; anc the identity; mean[n],
// cov[n][n], C[n][n]; zero[N] zeros.  Returns whiten's flag (row[5] of the record).
inline bool posterior_round_head(const double* u, const double* lnl, int N, int n, const int32_t* zero, double* row, int32_t* anc,
                                 double* mean, double* cov, double* C)
{
    row[0] = 1.0; row[1] = 1.0; row[2] = round_ess(lnl, N);
    for (int i = 0; i < N; ++i) anc[i] = i;
    for (int a = 0; a < n; ++a) mean[a] = vmx_ns::mean_entry(a, u, zero, N, 0, n);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) cov[a * n + b] = cov[b * n + a] = vmx_ns::cov_entry(a, b, u, zero, mean, N, 0, n);
    return vmx_ns::whiten(n, cov, C);
}

// run_status with rounds owed: topups_left is the count at the head of the stage and is paid here.  A posterior round (beta_before
// >= 1) cannot be STUCK; beta_after NaN: no particle has a finite lnL (the count is then left as it was).
VMX_HD inline int run_status_kept(double beta_before, double beta_after, int32_t& topups_left)
{
    if (beta_after != beta_after) return NO_FINITE;
    if (posterior_round(beta_before)) topups_left -= 1;
    else if (!(beta_after > beta_before)) return STUCK;
    return run_finished(beta_after, topups_left) ? FINISHED : RUNNING;
}

// first_active with rounds owed (topups_left NULL: none): a run at beta = 1 that owes rounds begins the call
VMX_HD inline int first_active_kept(const double* beta, const int32_t* topups_left, int E, bool draw, int32_t* active, int32_t* status)
{
    int A = 0;
    for (int e = 0; e < E; ++e) {
        status[e] = draw || !run_finished(beta[e], topups_left ? topups_left[e] : 0) ? RUNNING : FINISHED;
        if (status[e] == RUNNING) active[A++] = e;
    }
    return A;
}

}  // namespace vmx_smc
