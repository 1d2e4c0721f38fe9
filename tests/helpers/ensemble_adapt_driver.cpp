// CPU driver of the ensemble sampler's adaptive ladders (vega_amd/csrc/vmx_ensemble.h, the fourth part), built by
// tests/test_ensemble_adapt_host.py with g++ under AddressSanitizer / UBSan.  Reads one request per line on stdin, answers one line
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   J T W time lag tau beta[T] accepted[T - 1]       -> adjusted (1, or 0: the guard held), the ladder after ladder_adjust (T hex)
//   K T swap_every lag tau                           -> adapt_ok
//   M s swap_every adapt_until                       -> sweep_time, adapt_due
//   E x                                              -> pexp(x)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_ensemble.h"

static uint64_t word(const std::string& s) { return std::strtoull(s.c_str(), nullptr, 16); }
static double dbl(const std::string& s) { const uint64_t b = word(s); double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

int main()
{
    static char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "J" && tok.size() >= 6) {
            const int T = std::atoi(tok[1].c_str());
            if (T < 3 || T > vmx_ens::PT_MAXT || tok.size() != (size_t)6 + T + (T - 1)) { std::printf("ERR\n"); continue; }
            const int64_t W = std::atoll(tok[2].c_str()), time = std::atoll(tok[3].c_str());
            const double lag = dbl(tok[4]), tau = dbl(tok[5]);
            std::vector<double> beta(T);
            std::vector<int64_t> accepted(T - 1);
            for (int t = 0; t < T; ++t) beta[t] = dbl(tok[6 + t]);
            for (int t = 0; t + 1 < T; ++t) accepted[t] = std::atoll(tok[6 + T + t].c_str());
            const bool moved = vmx_ens::ladder_adjust(beta.data(), accepted.data(), T, W, time, lag, tau);
            std::printf("%d", moved ? 1 : 0);
            for (int t = 0; t < T; ++t) std::printf(" %016" PRIx64, bits(beta[t]));
            std::printf("\n");
        } else if (tok[0] == "K" && tok.size() == 5) {
            std::printf("%d\n", vmx_ens::adapt_ok(std::atoi(tok[1].c_str()), std::atoi(tok[2].c_str()), dbl(tok[3]), dbl(tok[4])) ? 1 : 0);
        } else if (tok[0] == "M" && tok.size() == 4) {
            const int64_t s = std::atoll(tok[1].c_str());
            const int every = std::atoi(tok[2].c_str());
            if (every < 1) { std::printf("ERR\n"); continue; }
            std::printf("%" PRId64 " %d\n", vmx_ens::sweep_time(s, every), vmx_ens::adapt_due(s, std::atoll(tok[3].c_str())) ? 1 : 0);
        } else if (tok[0] == "E" && tok.size() == 2) {
            std::printf("%016" PRIx64 "\n", bits(vmx_smc::pexp(dbl(tok[1]))));
        } else {
            std::printf("ERR\n");
        }
        std::fflush(stdout);
    }
    return 0;
}
