// The summary of a recorded ensemble chain, pinned sum for sum: what the host needs of a chain without the chain.
//
// A chain store (vmx_chain_store_*, vegamx.hip) keeps the recorded rows of E ensembles where the half-step kernels write them,
// positions [E][capacity][W][n] and lnL [E][capacity][W]; vmx_chain_store_summary reduces the rows [first_row, rows) of every
// ensemble there (k_chain_moments, k_chain_centre, k_chain_acf) and hands back O(E n^2) numbers.  vega_amd/ensemble.py restates
// every expression below in NumPy (chain_summary) and tests/helpers/chain_driver.cpp compiles this header with g++ so that
// tests/test_chain_summary_host.py can hold the two against each other bit for bit.  No HIP type, no heap.
//
// With T = rows - first_row >= 1 rows x[t][w][d] (t < T, w < W, d < n) of one ensemble:
//
//   every sum        is sequential: it starts from its first term and adds the others in index order, one rounded addition each
//                    (seq_sum and its kin below; np.add.accumulate along an axis is the same sum).  The order of every sum is a
//                    function of (T, W) alone: no sum is split by a tile, a lag block, a launch shape or E.
//   count            T W.
//   series sums      S[w][d] = sum_t x[t][w][d];  the series' own mean  m[w][d] = S[w][d] / T.
//   mean             mean[d] = (sum_w S[w][d]) / count           (walker by walker: the series sums, then the walkers).
//   covariance       P[w][i][j] = sum_t (x[t][w][i] - mean[i]) (x[t][w][j] - mean[j]);  covariance[i][j] = (sum_w P[w][i][j]) /
//                    (count - 1): two passes, ddof = 1 over the flattened rows x walkers (np.cov of the rows).
//   centred series   c[t][w] = x[t][w][d] - m[w][d], per parameter d.
//   autocovariance   acov[w][l] = sum_{t < T - l} c[t][w] c[t + l][w]: one lane per (walker, lag), sequential in t - the order chosen
//                    of the two the design allows (the other, the stride-halving tree of vmx_smc.h, would need a scratch per lane).
//   rho              rho[w][l] = acov[w][l] / acov[w][0]; acov[w][l] itself where acov[w][0] == 0 (a constant series).
//   f                f[l] = (sum_w rho[w][l]) / W.
//   taus             C[M] = sum_{l <= M} f[l] (sequential in l);  taus[M] = 2 C[M] - 1.
//   window           the first M in [0, T) with not (M < c taus[M]); T - 1 if there is none.  tau = taus[window].
//
// This is emcee's estimator as vega_amd.ensemble.integrated_time states it, with direct sums in place of the FFT.  The lags are
// computed in blocks (any size: no lag's value depends on its block) until the window closes, so the cost is T W (window + one
// block) per parameter, not T^2.  Every expression is the separately rounded IEEE operations written below (contraction off, as
// in vmx_ensemble.h); / is correctly rounded.
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

#ifndef VMX_NO_CONTRACT
#if defined(__clang__)
#define VMX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VMX_NO_CONTRACT
#endif
#endif

namespace vmx_chain {

constexpr int MAXW = 1024;          // walkers of a store: acov[w][0] of a parameter stays in the work-group's LDS
constexpr int TILE = 4096;          // doubles of the work-group's staging area: W x lags of a block, W x pairs of a chunk
constexpr int LAG_BLOCK = 32;       // lags of a block at most (the summary does not depend on it)

// lags of a block, pairs of a chunk: as many as W of them fit the staging area
VMX_HD inline int per_tile(int W, int most) { const int k = TILE / W; return k < 1 ? 1 : (k < most ? k : most); }

// ---- the sums: p[0] + p[stride] + ... in index order, `count` >= 1 terms
VMX_HD inline double seq_sum(const double* p, int64_t count, int64_t stride)
{
    VMX_NO_CONTRACT
    double s = p[0];
    for (int64_t t = 1; t < count; ++t) s = s + p[t * stride];
    return s;
}

VMX_HD inline double quotient(double total, int64_t by)
{
    VMX_NO_CONTRACT
    return total / (double)by;
}

VMX_HD inline double centred(double x, double m) { VMX_NO_CONTRACT return x - m; }

// sum_t (xi[t] - mi) (xj[t] - mj) over `count` >= 1 terms `stride` apart
VMX_HD inline double product_sum(const double* xi, const double* xj, double mi, double mj, int64_t count, int64_t stride)
{
    VMX_NO_CONTRACT
    double s = centred(xi[0], mi) * centred(xj[0], mj);
    for (int64_t t = 1; t < count; ++t) {
        const double a = centred(xi[t * stride], mi), b = centred(xj[t * stride], mj);
        const double p = a * b;
        s = s + p;
    }
    return s;
}

// acov[l] of the centred series c[0], c[stride] ... c[(T - 1) stride], 0 <= l < T
VMX_HD inline double lag_sum(const double* c, int64_t T, int64_t l, int64_t stride)
{
    VMX_NO_CONTRACT
    const double* d = c + l * stride;
    double s = c[0] * d[0];
    for (int64_t t = 1; t < T - l; ++t) {
        const double p = c[t * stride] * d[t * stride];
        s = s + p;
    }
    return s;
}

VMX_HD inline double rho(double acov_l, double acov_0)
{
    VMX_NO_CONTRACT
    return acov_0 == 0.0 ? acov_l : acov_l / acov_0;
}

VMX_HD inline double taus_of(double cumulative)
{
    VMX_NO_CONTRACT
    const double t = 2.0 * cumulative;
    return t - 1.0;
}

// Sokal's window closes at M: not (M < c taus) - a NaN closes it, as the comparison of integrated_time does
VMX_HD inline bool window_closes(int64_t M, double c, double taus)
{
    VMX_NO_CONTRACT
    const double bound = c * taus;
    return !((double)M < bound);
}

// The state of the walk over the lags of one parameter: the lags come in index order, whoever computed them
struct Window {
    double cumulative = 0.0, tau = 0.0;
    int64_t next = 0, window = -1;          // the lag awaited; the window once it has closed
};

// f[l] of lag l = W.next joins; true when the window has closed (or l = T - 1 was the last lag)
VMX_HD inline bool window_take(Window& S, double f, int64_t T, double c)
{
    VMX_NO_CONTRACT
    S.cumulative = S.next == 0 ? f : S.cumulative + f;
    const double taus = taus_of(S.cumulative);
    const int64_t M = S.next;
    S.next = M + 1;
    if (window_closes(M, c, taus) || M == T - 1) {
        S.window = M;
        S.tau = taus;
        return true;
    }
    return false;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the whole summary of one ensemble on the host, the loops of the kernels in plain order: x [T][W][n] (the rows from
// first_row on), scratch [T W + 2 W n + W + TILE]; lag_block: the lags of a block (any value >= 1 gives the same bits)
inline void summary(const double* x, int64_t T, int W, int n, double c, int lag_block, double* scratch, int64_t& count, double* mean,
                    double* covariance, double* tau, int64_t* window)
{
    const int64_t Wn = (int64_t)W * n;
    double* S = scratch;                // [W][n] series sums
    double* m = S + Wn;                 // [W][n] series means
    double* cen = m + Wn;               // [T][W] centred series of one parameter
    double* acov0 = cen + T * W;        // [W] acov[w][0] of that parameter
    double* tile = acov0 + W;           // [TILE]
    count = T * W;
    for (int64_t q = 0; q < Wn; ++q) {
        S[q] = seq_sum(x + q, T, Wn);
        m[q] = quotient(S[q], T);
    }
    for (int d = 0; d < n; ++d) mean[d] = quotient(seq_sum(S + d, W, n), count);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            for (int w = 0; w < W; ++w) tile[w] = product_sum(x + (int64_t)w * n + i, x + (int64_t)w * n + j, mean[i], mean[j], T, Wn);
            covariance[i * n + j] = covariance[j * n + i] = quotient(seq_sum(tile, W, 1), count - 1);
        }
    for (int d = 0; d < n; ++d) {
        for (int64_t t = 0; t < T; ++t)
            for (int w = 0; w < W; ++w) cen[t * W + w] = centred(x[t * Wn + (int64_t)w * n + d], m[(int64_t)w * n + d]);
        Window win;
        const int LB = per_tile(W, lag_block < 1 ? 1 : lag_block);
        bool closed = false;
        for (int64_t l0 = 0; l0 < T && !closed; l0 += LB) {
            const int64_t lags = T - l0 < LB ? T - l0 : LB;
            for (int64_t k = 0; k < lags; ++k)
                for (int w = 0; w < W; ++w) {
                    const double a = lag_sum(cen + w, T, l0 + k, W);
                    if (l0 + k == 0) acov0[w] = a;
                    tile[k * W + w] = rho(a, acov0[w]);
                }
            for (int64_t k = 0; k < lags && !closed; ++k) closed = window_take(win, quotient(seq_sum(tile + k * W, W, 1), W), T, c);
        }
        tau[d] = win.tau;
        window[d] = win.window;
    }
}
#endif

}  // namespace vmx_chain
