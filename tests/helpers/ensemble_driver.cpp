// CPU driver of the ensemble sampler's header (vega_amd/csrc/vmx_ensemble.h), built by tests/test_ensemble_host.py with g++ under
// AddressSanitizer / UBSan.  Reads one request per line on stdin, answers one line on stdout; doubles travel as the hex of their
// bits so that nothing is rounded on the way.
//   P c0 c1 c2 c3 k0 k1                      -> the Philox4x64-10 block (4 hex words)
//   C a n H x0 x1 x2 status chi2 log_norm lnl_old c[n] s[n] lo[n] hi[n]   (words and doubles in hex)
//                                            -> partner, z, factor, lnL_new, inside, accept, y[n]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_ensemble.h"

static uint64_t word(const char* s) { return std::strtoull(s, nullptr, 16); }
static double dbl(const char* s) { const uint64_t b = word(s); double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

int main()
{
    char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "P" && tok.size() == 7) {
            const vmx_ens::Block b = vmx_ens::philox4x64_10(word(tok[1].c_str()), word(tok[2].c_str()), word(tok[3].c_str()),
                                                            word(tok[4].c_str()), word(tok[5].c_str()), word(tok[6].c_str()));
            std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b.w[0], b.w[1], b.w[2], b.w[3]);
        } else if (tok[0] == "C" && tok.size() >= 11) {
            const double a = dbl(tok[1].c_str());
            const int n = std::atoi(tok[2].c_str());
            const int64_t H = std::atoll(tok[3].c_str());
            if (n < 1 || tok.size() != (size_t)11 + 4 * n) { std::printf("ERR\n"); continue; }
            const uint64_t x0 = word(tok[4].c_str()), x1 = word(tok[5].c_str()), x2 = word(tok[6].c_str());
            const int32_t status = std::atoi(tok[7].c_str());
            const double chi2 = dbl(tok[8].c_str()), log_norm = dbl(tok[9].c_str()), lnl_old = dbl(tok[10].c_str());
            const int64_t j = vmx_ens::partner(x0, H);
            const double z = vmx_ens::stretch_z(a, x1);
            std::vector<double> y(n);
            bool inside = true;
            for (int d = 0; d < n; ++d) {
                const double c = dbl(tok[11 + d].c_str()), s = dbl(tok[11 + n + d].c_str());
                const double lo = dbl(tok[11 + 2 * n + d].c_str()), hi = dbl(tok[11 + 3 * n + d].c_str());
                y[d] = vmx_ens::propose(c, s, z);
                inside = inside && y[d] >= lo && y[d] <= hi;
            }
            const double factor = vmx_ens::log_factor(n, z);
            const double lnl_new = vmx_ens::log_lik(log_norm, chi2);
            const bool acc = vmx_ens::accept(inside, vmx_ens::model_ok(status, chi2), factor, lnl_new, lnl_old, x2);
            std::printf("%" PRId64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d", j, bits(z), bits(factor), bits(lnl_new),
                        inside ? 1 : 0, acc ? 1 : 0);
            for (int d = 0; d < n; ++d) std::printf(" %016" PRIx64, bits(y[d]));
            std::printf("\n");
        } else {
            std::printf("ERR\n");
        }
        std::fflush(stdout);
    }
    return 0;
}
