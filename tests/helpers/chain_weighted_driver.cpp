// CPU driver of the weighted summary, order statistics and best point of vega_amd/csrc/vmx_chain_weighted.h, built by
// tests/test_chain_weighted_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.  A store is given whole, with its
// capacity: x [E][capacity][n], lnl [E][capacity], w [E][capacity], and the rows of every set counts [E].
//   U E capacity n counts[E] x[...] w[...]                    -> vmx_wchain::summary: six lines, S [E]; n_eff [E]; mean [E][n];
//                                                                covariance [E][n][n]; total [E] (decimal); w_max [E]
//   O E capacity n counts[E] R targets[E][R] x[...] w[...]    -> vmx_wchain::order_stats: one line, values [E][n][R]
//   B E capacity n counts[E] position x[...] lnl[...]         -> vmx_wchain::best: lnl_max [E]; index [E]; with position != 0 a
//                                                                third line, position [E][n]
//   W count w[count]                                          -> 1 / 0 per weight: whether it may be stored
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_chain_weighted.h"

static std::string need()
{
    char buf[64];
    if (std::scanf("%63s", buf) != 1) { std::printf("ERR\n"); std::exit(2); }
    return buf;
}
static int64_t integer() { return std::atoll(need().c_str()); }
static uint64_t word() { return std::strtoull(need().c_str(), nullptr, 16); }
static uint64_t natural() { return std::strtoull(need().c_str(), nullptr, 10); }
static double dbl() { const uint64_t b = word(); double d; std::memcpy(&d, &b, 8); return d; }

static void put(const std::vector<uint64_t>& v)
{
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %016" PRIx64 : "%016" PRIx64, v[i]);
    std::printf("\n");
}
static void put(const std::vector<double>& v)
{
    std::vector<uint64_t> b(v.size());
    if (!v.empty()) std::memcpy(b.data(), v.data(), v.size() * 8);
    put(b);
}

struct Shape {
    int E, n;
    int64_t capacity, most;
    std::vector<int64_t> counts;
    bool read()
    {
        E = (int)integer(); capacity = integer(); n = (int)integer();
        if (E < 1 || n < 1 || capacity < 0) return false;
        counts.resize((size_t)E);
        most = 0;
        for (int64_t& c : counts) {
            c = integer();
            if (c < 0 || c > capacity) return false;
            most = std::max(most, c);
        }
        return true;
    }
};

int main()
{
    char buf[64];
    while (std::scanf("%63s", buf) == 1) {
        const std::string tok = buf;
        if (tok == "U") {
            Shape s;
            if (!s.read()) { std::printf("ERR\n"); return 2; }
            std::vector<double> x((size_t)s.E * s.capacity * s.n), w((size_t)s.E * s.capacity);
            for (double& v : x) v = dbl();
            for (double& v : w) v = dbl();
            // (exactly what the header asks for: a write past it is an ASan report)
            std::vector<uint64_t> m((size_t)s.most), total((size_t)s.E);
            std::vector<double> scratch((size_t)vmx_wchain::padded(s.most)), S((size_t)s.E), n_eff((size_t)s.E), w_max((size_t)s.E),
                mean((size_t)s.E * s.n), cov((size_t)s.E * s.n * s.n);
            vmx_wchain::summary(x.data(), w.data(), s.counts.data(), s.E, s.capacity, s.n, m.data(), scratch.data(), S.data(), n_eff.data(),
                                mean.data(), cov.data(), total.data(), w_max.data());
            put(S); put(n_eff); put(mean); put(cov);
            for (int e = 0; e < s.E; ++e) std::printf(e ? " %" PRIu64 : "%" PRIu64, total[e]);
            std::printf("\n");
            put(w_max);
        } else if (tok == "O") {
            Shape s;
            if (!s.read()) { std::printf("ERR\n"); return 2; }
            const int R = (int)integer();
            if (R < 1 || R > vmx_wchain::MAX_TARGETS) { std::printf("ERR\n"); return 2; }
            std::vector<uint64_t> targets((size_t)s.E * R);
            for (uint64_t& t : targets) t = natural();
            std::vector<double> x((size_t)s.E * s.capacity * s.n), w((size_t)s.E * s.capacity);
            for (double& v : x) v = dbl();
            for (double& v : w) v = dbl();
            std::vector<uint64_t> keys((size_t)s.most), m((size_t)s.most), values((size_t)s.E * s.n * R);
            vmx_wchain::order_stats(x.data(), w.data(), s.counts.data(), s.E, s.capacity, s.n, R, targets.data(), keys.data(), m.data(),
                                    values.data());
            put(values);
        } else if (tok == "B") {
            Shape s;
            if (!s.read()) { std::printf("ERR\n"); return 2; }
            const bool position = integer() != 0;
            std::vector<double> x((size_t)s.E * s.capacity * s.n), lnl((size_t)s.E * s.capacity);
            for (double& v : x) v = dbl();
            for (double& v : lnl) v = dbl();
            std::vector<uint64_t> top((size_t)s.E), at((size_t)s.E * s.n);
            std::vector<int64_t> index((size_t)s.E);
            vmx_wchain::best(x.data(), lnl.data(), s.counts.data(), s.E, s.capacity, s.n, top.data(), index.data(), position ? at.data() : nullptr);
            put(top);
            for (int e = 0; e < s.E; ++e) std::printf(e ? " %" PRId64 : "%" PRId64, index[e]);
            std::printf("\n");
            if (position) put(at);
        } else if (tok == "W") {
            const int64_t count = integer();
            for (int64_t i = 0; i < count; ++i) std::printf(i ? " %d" : "%d", vmx_wchain::weight_ok(dbl()) ? 1 : 0);
            std::printf("\n");
        } else {
            std::printf("ERR\n");
            return 2;
        }
    }
    return 0;
}
