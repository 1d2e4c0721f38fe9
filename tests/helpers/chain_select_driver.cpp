// CPU driver of the order statistics and the best row of vega_amd/csrc/vmx_chain_select.h, built by
// tests/test_chain_select_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.  A store is given whole, with its
// capacity: x [E][capacity][W][n], lnl [E][capacity][W].
//   K count bits[count]                                   -> two lines: key of every word; unkey of every key
//   N T W                                                 -> 1 when T W values per column may be selected from (below 2^31), else 0
//   S E capacity rows W n first R ranks[R] x[...]         -> vmx_select::order_stats: one line, values [E][n][R]
//   B E capacity rows W n first position x[...] lnl[...]  -> vmx_select::best: lnl_max [E]; row [E]; walker [E]; with position != 0
//                                                            a fourth line, position [E][n]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_chain_select.h"

static std::string need()
{
    char buf[64];
    if (std::scanf("%63s", buf) != 1) { std::printf("ERR\n"); std::exit(2); }
    return buf;
}
static int64_t integer() { return std::atoll(need().c_str()); }
static uint64_t word() { return std::strtoull(need().c_str(), nullptr, 16); }
static double dbl() { const uint64_t b = word(); double d; std::memcpy(&d, &b, 8); return d; }

static void put(const std::vector<uint64_t>& v)
{
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %016" PRIx64 : "%016" PRIx64, v[i]);
    std::printf("\n");
}

struct Shape {
    int E, W, n;
    int64_t capacity, rows, first;
    bool read()
    {
        E = (int)integer(); capacity = integer(); rows = integer(); W = (int)integer(); n = (int)integer(); first = integer();
        return E >= 1 && W >= 1 && n >= 1 && rows >= 1 && capacity >= rows && first >= 0 && first < rows;
    }
};

int main()
{
    char buf[64];
    while (std::scanf("%63s", buf) == 1) {
        const std::string tok = buf;
        if (tok == "K") {
            const int64_t count = integer();
            std::vector<uint64_t> k((size_t)count), back((size_t)count);
            for (int64_t i = 0; i < count; ++i) {
                const double v = dbl();
                k[i] = vmx_select::key(v);
                back[i] = vmx_select::unkey(k[i]);
            }
            put(k);
            put(back);
        } else if (tok == "N") {
            const int64_t T = integer(), W = integer();
            std::printf("%d\n", vmx_select::count_fits(T, W) ? 1 : 0);
        } else if (tok == "S") {
            Shape s;
            if (!s.read()) { std::printf("ERR\n"); return 2; }
            const int R = (int)integer();
            if (R < 1 || R > vmx_select::MAX_RANKS) { std::printf("ERR\n"); return 2; }
            std::vector<int64_t> ranks((size_t)R);
            const int64_t N = (s.rows - s.first) * s.W;
            for (int64_t& r : ranks) { r = integer(); if (r < 0 || r >= N) { std::printf("ERR\n"); return 2; } }
            std::vector<double> x((size_t)s.E * s.capacity * s.W * s.n);
            for (double& v : x) v = dbl();
            // (exactly what the header asks for: a write past it is an ASan report)
            std::vector<uint64_t> keys((size_t)N), values((size_t)s.E * s.n * R);
            vmx_select::order_stats(x.data(), s.E, s.capacity, s.rows, s.W, s.n, s.first, R, ranks.data(), keys.data(), values.data());
            put(values);
        } else if (tok == "B") {
            Shape s;
            if (!s.read()) { std::printf("ERR\n"); return 2; }
            const bool position = integer() != 0;
            std::vector<double> x((size_t)s.E * s.capacity * s.W * s.n), lnl((size_t)s.E * s.capacity * s.W);
            for (double& v : x) v = dbl();
            for (double& v : lnl) v = dbl();
            std::vector<uint64_t> top((size_t)s.E), at((size_t)s.E * s.n);
            std::vector<int64_t> row((size_t)s.E);
            std::vector<int32_t> walker((size_t)s.E);
            vmx_select::best(x.data(), lnl.data(), s.E, s.capacity, s.rows, s.W, s.n, s.first, top.data(), row.data(), walker.data(),
                             position ? at.data() : nullptr);
            put(top);
            for (int e = 0; e < s.E; ++e) std::printf(e ? " %" PRId64 : "%" PRId64, row[e]);
            std::printf("\n");
            for (int e = 0; e < s.E; ++e) std::printf(e ? " %d" : "%d", (int)walker[e]);
            std::printf("\n");
            if (position) put(at);
        } else {
            std::printf("ERR\n");
            return 2;
        }
    }
    return 0;
}
