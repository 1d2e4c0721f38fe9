// The summary, the order statistics and the best point of weighted, ragged sample sets, pinned: what the posterior of a nested or
// an SMC run is quoted by, without the samples.
//
// A sample store (vmx_sample_store_*, vegamx.hip) keeps E sets on the device, positions x [E][capacity][n], lnL [E][capacity] and
// weights w [E][capacity]; set e has count[e] >= 0 rows, the rows [0, count[e]), and nothing behind them is ever read.  Every
// weight is finite and >= 0 (vmx_sample_store_put refuses others); a set may carry zeros.  vmx_sample_store_summary,
// _order_stats and _best reduce every set there (k_wchain_scale, k_wchain_moments, k_wchain_keys, k_wchain_select,
// k_wchain_best).  vega_amd/weighted.py restates every expression below in NumPy and tests/helpers/chain_weighted_driver.cpp
// compiles this header with g++ so that tests/test_chain_weighted_host.py can hold the two against each other bit for bit.  No
// HIP type, no heap.  key / unkey / leading / digit / find_group / regroup / take are those of vmx_chain_select.h, unchanged.
//
//   every sum        of doubles is the stride-halving tree of vmx_smc.h (tree_sum): the count terms, padded with +0 to
//                    M = padded(count) - the least power of two that is >= max(count, 2) - are added a[i] = a[i] + a[i + s] for
//                    i < s, s = M / 2, M / 4 ... 1.  Chosen over the sequential order of vmx_chain.h because a boosted nested
//                    run has 10^5 rows in one set: the tree is log2 M levels of independent additions that a work-group shares,
//                    the sequential sum is 10^5 dependent additions on one lane.  The order is a function of count alone: not of
//                    E, of a launch shape or of a tile.
//   w_max, S         the largest weight (a maximum is exact in any order; 0 for an empty set) and S = sum w.
//   p                p_i = w_i / S, one correctly rounded division.
//   s2, n_eff        s2 = sum p_i p_i;  n_eff = 1 / s2 (Kish).
//   mean             mean_d = sum (p_i x_id).
//   covariance       cov_ij = (sum ((p_i (x_ii - mean_i)) (x_ij - mean_j))) / (1 - s2), i >= j and mirrored: two passes, the
//                    reliability-weights estimate.
//   degenerate sets  count = 0 or S = 0: mean, covariance and n_eff NaN.  s2 >= 1 (one row carries all the weight): covariance
//                    NaN.  No error.  Every NaN handed out is the canonical one (a NaN position that carries weight makes its
//                    mean and covariances NaN; the payload a sum would carry is nobody's business).
//   integer weights  m_i = (uint64) floor(w_i / w_max 2^32): one correctly rounded division, an exact scaling, a truncation
//                    (0 <= m_i <= 2^32; 0 for every row when w_max = 0).  A weight below 2^-32 w_max counts as 0: it moves a
//                    cumulative weight by at most count 2^-32 of the largest weight.  M = sum m_i, an integer sum: any order
//                    gives the same value, and count <= 2^31 - 1 keeps M < 2^63.
//   order statistic  for a target t, 1 <= t <= M: the smallest key k with C(k) = sum_{key_i <= k} m_i >= t, unkeyed - a stored
//                    value's own bits (the canonical NaN for a NaN) in the key order of vmx_chain_select.h (-0 before +0, NaN
//                    last).  A row with m_i = 0 is never the answer.  Found by the radix select of vmx_chain_select.h with sums
//                    of m in the histograms: eight passes of 8-bit digits; the digit of a pass is the first bin whose cumulative
//                    sum reaches the target left, which then loses what lay below (walk).  Up to MAX_TARGETS targets go together,
//                    taken in non-decreasing order (repeats share a histogram; the caller's order is put back afterwards).  No
//                    floating-point operation takes part once the m_i are made.  A set with M = 0 answers the canonical NaN.
//   quantile         host arithmetic on every driver: t = max(1, ceil(q M)) computed exactly (q is a dyadic rational, M an
//                    integer); the quantile is the order statistic at t - the inverted CDF, not the linear interpolation of
//                    the ensemble chains' quantiles.
//   best point       the largest lnL over the rows [0, count): a NaN never wins, ties go to the lowest row (vmx_select::take);
//                    no candidate: index -1, lnL and position the canonical NaN.  Weights play no part.
//
// Every expression is the separately rounded IEEE operations written below (contraction off); / is correctly rounded.
#pragma once
#include <cstdint>

#include "vmx_chain_select.h"

namespace vmx_wchain {

using vmx_select::BINS;
using vmx_select::PASSES;
using vmx_select::CANONICAL_NAN;

constexpr int MAX_TARGETS = 16;                         // targets of a call (VMX_SAMPLE_MAX_TARGETS)
constexpr int64_t MAX_COUNT = (int64_t(1) << 31) - 1;   // rows of a set: M stays below 2^63

VMX_HD inline double canonical_nan() { return vmx_select::double_of(CANONICAL_NAN); }
VMX_HD inline double canonical(double v) { VMX_NO_CONTRACT return v != v ? canonical_nan() : v; }

// terms of a tree: the least power of two >= max(count, 2)
VMX_HD inline int64_t padded(int64_t count)
{
    int64_t M = 2;
    while (M < count) M <<= 1;
    return M;
}

VMX_HD inline double add(double a, double b) { VMX_NO_CONTRACT return a + b; }
VMX_HD inline double larger(double a, double b) { VMX_NO_CONTRACT return b > a ? b : a; }
VMX_HD inline double share(double w, double S) { VMX_NO_CONTRACT return w / S; }
VMX_HD inline double square_term(double w, double S) { VMX_NO_CONTRACT const double p = w / S; return p * p; }
VMX_HD inline double mean_term(double w, double S, double x) { VMX_NO_CONTRACT const double p = w / S; return p * x; }
VMX_HD inline double cov_term(double w, double S, double xi, double mi, double xj, double mj)
{
    VMX_NO_CONTRACT
    const double p = w / S, a = xi - mi, b = xj - mj;
    const double t = p * a;
    return t * b;
}
VMX_HD inline double n_eff_of(double S, double s2)
{
    VMX_NO_CONTRACT
    if (!(S > 0.0)) return canonical_nan();
    return canonical(1.0 / s2);
}
VMX_HD inline double mean_of(double S, double sum) { VMX_NO_CONTRACT return S > 0.0 ? canonical(sum) : canonical_nan(); }
VMX_HD inline double covariance_of(double S, double s2, double sum)
{
    VMX_NO_CONTRACT
    if (!(S > 0.0) || !(s2 < 1.0)) return canonical_nan();
    const double d = 1.0 - s2;
    return canonical(sum / d);
}

VMX_HD inline uint64_t integer_weight(double w, double w_max)
{
    VMX_NO_CONTRACT
    if (!(w_max > 0.0)) return 0;
    const double r = w / w_max;
    const double s = r * 4294967296.0;
    return (uint64_t)s;
}

// whether a weight may be stored: finite and >= 0
VMX_HD inline bool weight_ok(double w) { VMX_NO_CONTRACT return w >= 0.0 && w <= 1.7976931348623157e308; }

// the next digit of a target: the first bin whose cumulative sum reaches `left` (>= 1); `left` becomes the target within that bin
// (the bins hold at least `left` in all: the target is no larger than the sum of its prefix)
VMX_HD inline int walk(const uint64_t* hist, uint64_t& left)
{
    uint64_t below = 0;
    int d = 0;
    for (; d < BINS - 1; ++d) {
        const uint64_t h = hist[d];
        if (below + h >= left) break;
        below += h;
    }
    left -= below;
    return d;
}

// `targets` [R] in non-decreasing order into `sorted` [R]; place[r]: where targets[r] went (insertion sort, stable)
VMX_HD inline void sort_targets(const uint64_t* targets, int R, uint64_t* sorted, int* place)
{
    int order[MAX_TARGETS];
    for (int r = 0; r < R; ++r) {
        int at = r;
        while (at > 0 && sorted[at - 1] > targets[r]) { sorted[at] = sorted[at - 1]; order[at] = order[at - 1]; --at; }
        sorted[at] = targets[r];
        order[at] = r;
    }
    for (int k = 0; k < R; ++k) place[order[k]] = k;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the whole of it on the host, the loops of the kernels in plain order.
// the stride-halving tree over a[M] (destroyed), M a power of two >= 2
inline double tree_sum(double* a, int64_t M)
{
    for (int64_t s = M / 2; s >= 1; s /= 2)
        for (int64_t i = 0; i < s; ++i) a[i] = add(a[i], a[i + s]);
    return a[0];
}

struct Scale {
    double w_max, S, s2;
    uint64_t M;
};

// w [count] -> w_max, S, s2, m [count] and M; scratch [padded(count)]
inline Scale scale(const double* w, int64_t count, uint64_t* m, double* scratch)
{
    Scale r;
    r.w_max = 0.0; r.S = 0.0; r.s2 = canonical_nan(); r.M = 0;
    if (count < 1) return r;
    const int64_t P = padded(count);
    for (int64_t i = 0; i < count; ++i) r.w_max = larger(r.w_max, w[i]);
    for (int64_t i = 0; i < P; ++i) scratch[i] = i < count ? w[i] : 0.0;
    r.S = tree_sum(scratch, P);
    for (int64_t i = 0; i < P; ++i) scratch[i] = i < count ? square_term(w[i], r.S) : 0.0;
    r.s2 = tree_sum(scratch, P);
    for (int64_t i = 0; i < count; ++i) { m[i] = integer_weight(w[i], r.w_max); r.M += m[i]; }
    return r;
}

// The summary of a store: x [E][capacity][n], w [E][capacity], counts [E]; S, n_eff, w_max [E], total [E] (M), mean [E][n],
// covariance [E][n][n]; m: scratch [max count], scratch [padded(max count)]
inline void summary(const double* x, const double* w, const int64_t* counts, int E, int64_t capacity, int n, uint64_t* m, double* scratch,
                    double* S, double* n_eff, double* mean, double* covariance, uint64_t* total, double* w_max)
{
    for (int e = 0; e < E; ++e) {
        const int64_t count = counts[e], P = padded(count);
        const double* xe = x + (int64_t)e * capacity * n;
        const double* we = w + (int64_t)e * capacity;
        const Scale sc = scale(we, count, m, scratch);
        S[e] = sc.S; w_max[e] = sc.w_max; total[e] = sc.M;
        const bool live = count >= 1;
        n_eff[e] = live ? n_eff_of(sc.S, sc.s2) : canonical_nan();
        double* me = mean + (int64_t)e * n;
        double* ce = covariance + (int64_t)e * n * n;
        for (int d = 0; d < n; ++d) {
            if (!live) { me[d] = canonical_nan(); continue; }
            for (int64_t i = 0; i < P; ++i) scratch[i] = i < count ? mean_term(we[i], sc.S, xe[i * n + d]) : 0.0;
            me[d] = mean_of(sc.S, tree_sum(scratch, P));
        }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) {
                double v = canonical_nan();
                if (live) {
                    for (int64_t k = 0; k < P; ++k)
                        scratch[k] = k < count ? cov_term(we[k], sc.S, xe[k * n + i], me[i], xe[k * n + j], me[j]) : 0.0;
                    v = covariance_of(sc.S, sc.s2, tree_sum(scratch, P));
                }
                ce[i * n + j] = ce[j * n + i] = v;
            }
    }
}

// u non-decreasing targets (each in [1, M]) over the N keys of a column with their integer weights -> u keys;
// hist [MAX_TARGETS][BINS]
inline void select_column(const uint64_t* keys, const uint64_t* m, int64_t N, int u, const uint64_t* targets, uint64_t* hist, uint64_t* out)
{
    uint64_t prefix[MAX_TARGETS], group_prefix[MAX_TARGETS], left[MAX_TARGETS];
    int group[MAX_TARGETS];
    for (int r = 0; r < u; ++r) { prefix[r] = 0; left[r] = targets[r]; }
    int g = vmx_select::regroup(prefix, u, group, group_prefix);
    for (int p = 0; p < PASSES; ++p) {
        for (int q = 0; q < g * BINS; ++q) hist[q] = 0;
        for (int64_t i = 0; i < N; ++i) {
            const int at = vmx_select::find_group(group_prefix, g, vmx_select::leading(keys[i], p));
            if (at >= 0) hist[at * BINS + vmx_select::digit(keys[i], p)] += m[i];
        }
        for (int r = 0; r < u; ++r) prefix[r] = (prefix[r] << 8) | (uint64_t)walk(hist + group[r] * BINS, left[r]);
        g = vmx_select::regroup(prefix, u, group, group_prefix);
    }
    for (int r = 0; r < u; ++r) out[r] = prefix[r];
}

// Order statistics of a store: targets [E][R] in any order, repeats allowed, each in [1, M_e] (ignored where M_e = 0);
// values [E][n][R] as bits; keys, m: scratch [max count] each
inline void order_stats(const double* x, const double* w, const int64_t* counts, int E, int64_t capacity, int n, int R, const uint64_t* targets,
                        uint64_t* keys, uint64_t* m, uint64_t* values)
{
    uint64_t hist[MAX_TARGETS * BINS], sorted[MAX_TARGETS], found[MAX_TARGETS];
    int place[MAX_TARGETS];
    for (int e = 0; e < E; ++e) {
        const int64_t count = counts[e];
        const double* xe = x + (int64_t)e * capacity * n;
        const double* we = w + (int64_t)e * capacity;
        double w_max = 0.0;
        uint64_t M = 0;
        for (int64_t i = 0; i < count; ++i) w_max = larger(w_max, we[i]);
        for (int64_t i = 0; i < count; ++i) { m[i] = integer_weight(we[i], w_max); M += m[i]; }
        sort_targets(targets + (int64_t)e * R, R, sorted, place);
        for (int d = 0; d < n; ++d) {
            if (M > 0) {
                for (int64_t i = 0; i < count; ++i) keys[i] = vmx_select::key(xe[i * n + d]);
                select_column(keys, m, count, R, sorted, hist, found);
            }
            for (int r = 0; r < R; ++r) values[((int64_t)e * n + d) * R + r] = M > 0 ? vmx_select::unkey(found[place[r]]) : CANONICAL_NAN;
        }
    }
}

// The best point of every set: lnl [E][capacity]; lnl_max [E] (bits), index [E], position [E][n] (bits; may be null)
inline void best(const double* x, const double* lnl, const int64_t* counts, int E, int64_t capacity, int n, uint64_t* lnl_max, int64_t* index,
                 uint64_t* position)
{
    for (int e = 0; e < E; ++e) {
        vmx_select::Best b = vmx_select::candidate(0.0, -1);
        for (int64_t q = 0; q < counts[e]; ++q) b = vmx_select::take(b, vmx_select::candidate(lnl[(int64_t)e * capacity + q], q));
        index[e] = b.index < 0 ? -1 : b.index;
        lnl_max[e] = b.index < 0 ? CANONICAL_NAN : vmx_select::bits_of(b.value);
        if (position)
            for (int d = 0; d < n; ++d)
                position[(int64_t)e * n + d] = b.index < 0 ? CANONICAL_NAN : vmx_select::bits_of(x[((int64_t)e * capacity + b.index) * n + d]);
    }
}
#endif

}  // namespace vmx_wchain
