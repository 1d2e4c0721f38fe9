// Order statistics and the best row of a recorded ensemble chain, pinned: what a posterior is quoted by, without the chain.
//
// A chain store (vmx_chain_store_*, vegamx.hip; vmx_chain.h) keeps positions x [E][capacity][W][n] and lnL [E][capacity][W] on the
// device.  vmx_chain_store_order_stats hands back exact order statistics of every (ensemble, column) over the rows [first_row,
// rows), vmx_chain_store_best the best row of every ensemble (k_chain_keys, k_chain_select, k_chain_best).  vega_amd/ensemble.py
// restates both in NumPy (chain_order_statistics, chain_best) and tests/helpers/chain_select_driver.cpp compiles this header with
// g++ so that tests/test_chain_select_host.py can hold the two against each other bit for bit.  No HIP type, no heap.
//
//   key              of a double with bits b: all ones for every NaN of either sign; else ~b if the sign bit is set, else b | 1 << 63.
//                    Unsigned order of the keys is the order used everywhere: -inf < ... < -0 < +0 < ... < +inf < NaN (np.sort's
//                    order, with -0 before +0 on top of it).  unkey gives the value's own bits back, the canonical NaN
//                    0x7ff8000000000000 for the NaN key.
//   order statistic  with T = rows - first_row and N = T W values of column d of ensemble e, rank k (0 <= k < N) is the k-th
//                    smallest key, unkeyed: a stored value's bits or the canonical NaN.  It is found by a most-significant-digit
//                    radix select: eight passes of 8-bit digits; in pass p the keys that share the 8 p leading bits chosen so far
//                    are counted per next digit (integer counts: any order of counting gives the same histogram), and the digit
//                    is the first one whose cumulative count exceeds the rank left (walk).  Several ranks go together: they are
//                    taken sorted and distinct (the caller's order and repeats are put back afterwards), so the prefixes of
//                    consecutive ranks are non-decreasing and the ranks that still share a prefix share a histogram (regroup,
//                    find_group).  No floating-point operation takes part: the answer depends on the N keys and k alone, not on a
//                    launch shape, E, the other ranks or a tile.
//   best row         the largest lnL over rows [first_row, rows) x walkers.  A NaN is no candidate; -inf is.  Among equal values
//                    (+0 == -0) the lowest index row W + walker wins.  "Greater, or equal and lower index" (take) is associative
//                    and commutative, so every reduction tree gives the same answer.  No candidate: index -1 (row -1, walker -1,
//                    lnL and position the canonical NaN).
//
// No double is computed here (keys are integer functions of bits, the best row is chosen by comparisons); the contraction guard of
// vmx_chain.h is kept on the comparisons all the same.  Quantiles are host arithmetic over order statistics (ensemble.py).
#pragma once
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

namespace vmx_select {

constexpr int MAX_RANKS = 32;           // ranks of a call (VMX_CHAIN_MAX_RANKS)
constexpr int BINS = 256, PASSES = 8;   // 8-bit digits of a 64-bit key, most significant first
constexpr uint64_t NAN_KEY = ~0ull, CANONICAL_NAN = 0x7ff8000000000000ull, SIGN = 1ull << 63;

VMX_HD inline uint64_t bits_of(double v) { uint64_t b; __builtin_memcpy(&b, &v, 8); return b; }
VMX_HD inline double double_of(uint64_t b) { double v; __builtin_memcpy(&v, &b, 8); return v; }

VMX_HD inline uint64_t key_of_bits(uint64_t b)
{
    if ((b & ~SIGN) > 0x7ff0000000000000ull) return NAN_KEY;
    return (b & SIGN) ? ~b : (b | SIGN);
}
VMX_HD inline uint64_t key(double v) { return key_of_bits(bits_of(v)); }
VMX_HD inline uint64_t unkey(uint64_t k) { return k == NAN_KEY ? CANONICAL_NAN : ((k & SIGN) ? (k ^ SIGN) : ~k); }

// what a call may ask: N = T W values per column below 2^31 (the counts of a pass are 32-bit)
VMX_HD inline bool count_fits(int64_t T, int64_t W) { return T >= 1 && W >= 1 && T <= ((int64_t(1) << 31) - 1) / W; }

// the 8 p leading bits of a key (0 in pass 0), and its digit of pass p
VMX_HD inline uint64_t leading(uint64_t k, int p) { return p == 0 ? 0ull : k >> (64 - 8 * p); }
VMX_HD inline int digit(uint64_t k, int p) { return (int)((k >> (56 - 8 * p)) & 0xffu); }

// the group whose prefix is `top` among the g ascending, distinct prefixes, or -1
VMX_HD inline int find_group(const uint64_t* prefix, int g, uint64_t top)
{
    int lo = 0, hi = g;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (prefix[mid] < top) lo = mid + 1; else hi = mid;
    }
    return lo < g && prefix[lo] == top ? lo : -1;
}

// the next digit of a rank: the first bin whose cumulative count exceeds `left`; `left` becomes the rank within that bin
// (the bins hold more than `left` keys in all: the rank is below the count of its prefix)
VMX_HD inline int walk(const uint32_t* hist, uint32_t& left)
{
    uint32_t below = 0;
    int d = 0;
    for (; d < BINS - 1; ++d) {
        const uint32_t h = hist[d];
        if (left < below + h) break;
        below += h;
    }
    left -= below;
    return d;
}

// after a pass: the u ranks' prefixes (ascending, since the ranks are) into groups of equal prefix; returns their number
VMX_HD inline int regroup(const uint64_t* prefix, int u, int* group, uint64_t* group_prefix)
{
    int g = 0;
    for (int r = 0; r < u; ++r) {
        if (r == 0 || prefix[r] != prefix[r - 1]) group_prefix[g++] = prefix[r];
        group[r] = g - 1;
    }
    return g;
}

// ---- the best row: a candidate is (value, index), index < 0 for none
struct Best {
    double value;
    int64_t index;
};

VMX_HD inline Best candidate(double v, int64_t index)
{
    VMX_NO_CONTRACT
    Best b;
    b.value = v;
    b.index = v != v ? -1 : index;
    return b;
}

// whether candidate b wins over candidate a: the greater value, or the lower index of equal ones; none (index < 0) never wins
VMX_HD inline bool wins(double b_value, int64_t b_index, double a_value, int64_t a_index)
{
    VMX_NO_CONTRACT
    if (b_index < 0) return false;
    if (a_index < 0) return true;
    return b_value > a_value || (b_value == a_value && b_index < a_index);
}

// of two candidates the one that wins
VMX_HD inline Best take(Best a, Best b) { return wins(b.value, b.index, a.value, a.index) ? b : a; }

// sorted, distinct ranks of `ranks` [R] into `sorted` [R]; returns their number
VMX_HD inline int distinct_ranks(const int64_t* ranks, int R, int64_t* sorted)
{
    int u = 0;
    for (int r = 0; r < R; ++r) {
        int at = 0;
        while (at < u && sorted[at] < ranks[r]) ++at;
        if (at < u && sorted[at] == ranks[r]) continue;
        for (int k = u; k > at; --k) sorted[k] = sorted[k - 1];
        sorted[at] = ranks[r];
        ++u;
    }
    return u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the whole of it on the host, the loops of the kernels in plain order.
// u ascending distinct ranks of the N keys of a column -> u keys; hist [MAX_RANKS][BINS]
inline void select_column(const uint64_t* keys, int64_t N, int u, const int64_t* ranks, uint32_t* hist, uint64_t* out)
{
    uint64_t prefix[MAX_RANKS], group_prefix[MAX_RANKS];
    uint32_t left[MAX_RANKS];
    int group[MAX_RANKS];
    for (int r = 0; r < u; ++r) { prefix[r] = 0; left[r] = (uint32_t)ranks[r]; }
    int g = regroup(prefix, u, group, group_prefix);
    for (int p = 0; p < PASSES; ++p) {
        for (int q = 0; q < g * BINS; ++q) hist[q] = 0;
        for (int64_t i = 0; i < N; ++i) {
            const int at = find_group(group_prefix, g, leading(keys[i], p));
            if (at >= 0) hist[at * BINS + digit(keys[i], p)] += 1;
        }
        for (int r = 0; r < u; ++r) prefix[r] = (prefix[r] << 8) | (uint64_t)walk(hist + group[r] * BINS, left[r]);
        g = regroup(prefix, u, group, group_prefix);
    }
    for (int r = 0; r < u; ++r) out[r] = prefix[r];
}

// order statistics of a store: x [E][capacity][W][n], the rows [first, rows); ranks [R] in any order, repeats allowed, each in
// [0, (rows - first) W); values [E][n][R] as bits; keys: scratch [(rows - first) W]
inline void order_stats(const double* x, int E, int64_t capacity, int64_t rows, int W, int n, int64_t first, int R, const int64_t* ranks,
                        uint64_t* keys, uint64_t* values)
{
    uint32_t hist[MAX_RANKS * BINS];
    int64_t sorted[MAX_RANKS];
    uint64_t found[MAX_RANKS];
    const int u = distinct_ranks(ranks, R, sorted);
    const int64_t T = rows - first, N = T * W;
    for (int e = 0; e < E; ++e)
        for (int d = 0; d < n; ++d) {
            for (int64_t t = 0; t < T; ++t)
                for (int w = 0; w < W; ++w) keys[t * W + w] = key(x[(((int64_t)e * capacity + first + t) * W + w) * n + d]);
            select_column(keys, N, u, sorted, hist, found);
            for (int r = 0; r < R; ++r) {
                int at = 0;
                while (sorted[at] != ranks[r]) ++at;
                values[((int64_t)e * n + d) * R + r] = unkey(found[at]);
            }
        }
}

// the best row of every ensemble: lnl [E][capacity][W]; lnl_max [E] (bits), row [E] (from row 0 of the store), walker [E],
// position [E][n] (bits; may be null)
inline void best(const double* x, const double* lnl, int E, int64_t capacity, int64_t rows, int W, int n, int64_t first, uint64_t* lnl_max,
                 int64_t* row, int32_t* walker, uint64_t* position)
{
    for (int e = 0; e < E; ++e) {
        Best b = candidate(0.0, -1);
        for (int64_t q = first * W; q < rows * W; ++q) b = take(b, candidate(lnl[(int64_t)e * capacity * W + q], q));
        row[e] = b.index < 0 ? -1 : b.index / W;
        walker[e] = b.index < 0 ? -1 : (int32_t)(b.index % W);
        lnl_max[e] = b.index < 0 ? CANONICAL_NAN : bits_of(b.value);
        if (position)
            for (int d = 0; d < n; ++d)
                position[(int64_t)e * n + d] = b.index < 0 ? CANONICAL_NAN : bits_of(x[((int64_t)e * capacity * W + b.index) * n + d]);
    }
}
#endif

}  // namespace vmx_select
