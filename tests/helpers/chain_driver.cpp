// CPU driver of the chain summary of vega_amd/csrc/vmx_chain.h, built by tests/test_chain_summary_host.py with g++ under
// AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers on stdout; doubles travel as the hex of their
// bits so that nothing is rounded on the way.
//   Y rows W n first c lag_block x[rows W n]    -> vmx_chain::summary over the rows from `first` on: five lines - count; mean [n];
//                                                  covariance [n n]; tau [n]; window [n]
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_chain.h"

static std::string need()
{
    char buf[64];
    if (std::scanf("%63s", buf) != 1) { std::printf("ERR\n"); std::exit(2); }
    return buf;
}
static int64_t integer() { return std::atoll(need().c_str()); }
static double dbl() { const uint64_t b = std::strtoull(need().c_str(), nullptr, 16); double d; std::memcpy(&d, &b, 8); return d; }

static void put(const std::vector<double>& v)
{
    for (size_t i = 0; i < v.size(); ++i) {
        uint64_t b;
        std::memcpy(&b, &v[i], 8);
        std::printf(i ? " %016" PRIx64 : "%016" PRIx64, b);
    }
    std::printf("\n");
}

int main()
{
    char buf[64];
    while (std::scanf("%63s", buf) == 1) {
        const std::string tok = buf;
        if (tok == "Y") {
            const int64_t rows = integer();
            const int W = (int)integer(), n = (int)integer();
            const int64_t first = integer();
            const double c = dbl();
            const int lag_block = (int)integer();
            if (rows < 1 || W < 1 || W > vmx_chain::MAXW || n < 1 || first < 0 || first >= rows) { std::printf("ERR\n"); return 2; }
            std::vector<double> x((size_t)rows * W * n);
            for (double& v : x) v = dbl();
            const int64_t T = rows - first;
            // (exactly what the header asks for: a write past it is an ASan report)
            std::vector<double> scratch((size_t)T * W + 2 * (size_t)W * n + W + vmx_chain::TILE);
            std::vector<double> mean(n), cov((size_t)n * n), tau(n);
            std::vector<int64_t> window(n);
            int64_t count = 0;
            vmx_chain::summary(x.data() + (size_t)first * W * n, T, W, n, c, lag_block, scratch.data(), count, mean.data(), cov.data(),
                               tau.data(), window.data());
            std::printf("%" PRId64 "\n", count);
            put(mean);
            put(cov);
            put(tau);
            for (int d = 0; d < n; ++d) std::printf(d ? " %" PRId64 : "%" PRId64, window[d]);
            std::printf("\n");
        } else {
            std::printf("ERR\n");
            return 2;
        }
    }
    return 0;
}
