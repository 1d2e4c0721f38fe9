// CPU driver of the decisions a set of SMC runs adds to vega_amd/csrc/vmx_smc.h ("a set of runs"), built by
// tests/test_smc_set_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers on
// stdout, one line each; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   S beta_before beta_after        -> vmx_smc::run_status
//   T finite                        -> vmx_smc::start_status
//   F E draw beta[E]                -> vmx_smc::first_active: A, the A active runs, then the E statuses
//   C A active[A] E status[E]       -> vmx_smc::compact_active: B, the B runs that stay
//   L E draw beta[E] rounds then per round the words (beta_after per active run, in the list's order)
//                                   -> the host loop of vmx_smc_run_many over those words: per round a line with the active list the
//                                      round ran with, last a line with the E statuses and a line with the stages done
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_smc.h"

static std::string need()
{
    char buf[64];
    if (std::scanf("%63s", buf) != 1) { std::printf("ERR\n"); std::exit(2); }
    return buf;
}
static int64_t integer() { return std::atoll(need().c_str()); }
static double dbl() { const uint64_t b = std::strtoull(need().c_str(), nullptr, 16); double d; std::memcpy(&d, &b, 8); return d; }

static void put_list(const int32_t* v, int count)
{
    std::printf("%d", count);
    for (int i = 0; i < count; ++i) std::printf(" %d", (int)v[i]);
}

int main()
{
    char buf[64];
    while (std::scanf("%63s", buf) == 1) {
        const std::string tok = buf;
        if (tok == "S") {
            const double before = dbl(), after = dbl();
            std::printf("%d\n", vmx_smc::run_status(before, after));
        } else if (tok == "T") {
            std::printf("%d\n", vmx_smc::start_status(dbl()));
        } else if (tok == "F") {
            const int E = (int)integer();
            const bool draw = integer() != 0;
            std::vector<double> beta(E);
            for (double& b : beta) b = dbl();
            std::vector<int32_t> active(E), status(E);        // (exactly E: a write past the list is an ASan report)
            const int A = vmx_smc::first_active(beta.data(), E, draw, active.data(), status.data());
            put_list(active.data(), A);
            for (int e = 0; e < E; ++e) std::printf(" %d", (int)status[e]);
            std::printf("\n");
        } else if (tok == "C") {
            const int A = (int)integer();
            std::vector<int32_t> active(A);
            for (int32_t& a : active) a = (int32_t)integer();
            const int E = (int)integer();
            std::vector<int32_t> status(E);
            for (int32_t& s : status) s = (int32_t)integer();
            const int B = vmx_smc::compact_active(active.data(), A, status.data());
            put_list(active.data(), B);
            std::printf("\n");
        } else if (tok == "L") {
            const int E = (int)integer();
            const bool draw = integer() != 0;
            std::vector<double> beta(E);
            for (double& b : beta) b = dbl();
            const int rounds = (int)integer();
            std::vector<int32_t> active(E), status(E), done(E, 0);
            int A = vmx_smc::first_active(beta.data(), E, draw, active.data(), status.data());
            if (draw) for (double& b : beta) b = 0.0;
            for (int r = 0; r < rounds && A > 0; ++r) {
                put_list(active.data(), A);
                std::printf("\n");
                for (int a = 0; a < A; ++a) {
                    const int q = active[a];
                    const double after = dbl();
                    status[q] = vmx_smc::run_status(beta[q], after);
                    if (status[q] == vmx_smc::NO_FINITE || status[q] == vmx_smc::STUCK) continue;
                    beta[q] = after;
                    done[q] += 1;
                }
                A = vmx_smc::compact_active(active.data(), A, status.data());
            }
            put_list(status.data(), E);
            std::printf("\n");
            for (int q = 0; q < E; ++q)
                if (status[q] == vmx_smc::NO_FINITE || status[q] == vmx_smc::STUCK) done[q] = 0;
            put_list(done.data(), E);
            std::printf("\n");
        } else {
            std::printf("ERR\n");
            return 2;
        }
    }
    return 0;
}
