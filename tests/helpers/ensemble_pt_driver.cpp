// CPU driver of the ensemble sampler's parallel tempering (vega_amd/csrc/vmx_ensemble.h, the third part), built by
// tests/test_ensemble_pt_host.py with g++ under AddressSanitizer / UBSan.  Reads one request per line on stdin, answers one line on
// stdout; words travel in hex and doubles as the hex of their bits so that nothing is rounded on the way.
//   P k s t seed stream                              -> the block of pair k (4 hex words)
//   R s t seed stream                                -> the block of the rotation (4 hex words)
//   T beta lnl                                       -> tempered(beta, lnl)
//   A inside ok factor beta lnl_new lnl_old w2       -> accept_tempered, accept (the untempered decision on the same operands)
//   H w0 W k                                         -> r = swap_shift(w0, W), swap_partner(k, r, W)
//   S beta_cold beta_hot lnl_cold lnl_hot word       -> swap_accept
//   D s swap_every                                   -> swap_due
//   L T beta[T]                                      -> ladder_ok
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
static void print_block(const vmx_ens::Block& b)
{
    std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b.w[0], b.w[1], b.w[2], b.w[3]);
}

int main()
{
    static char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "P" && tok.size() == 6) {
            print_block(vmx_ens::swap_block(std::atoll(tok[1].c_str()), std::atoll(tok[2].c_str()), std::atoi(tok[3].c_str()),
                                            word(tok[4]), word(tok[5])));
        } else if (tok[0] == "R" && tok.size() == 5) {
            print_block(vmx_ens::shift_block(std::atoll(tok[1].c_str()), std::atoi(tok[2].c_str()), word(tok[3]), word(tok[4])));
        } else if (tok[0] == "T" && tok.size() == 3) {
            std::printf("%016" PRIx64 "\n", bits(vmx_ens::tempered(dbl(tok[1]), dbl(tok[2]))));
        } else if (tok[0] == "A" && tok.size() == 8) {
            const bool inside = std::atoi(tok[1].c_str()) != 0, ok = std::atoi(tok[2].c_str()) != 0;
            const double factor = dbl(tok[3]), beta = dbl(tok[4]), lnl_new = dbl(tok[5]), lnl_old = dbl(tok[6]);
            std::printf("%d %d\n", vmx_ens::accept_tempered(inside, ok, factor, beta, lnl_new, lnl_old, word(tok[7])) ? 1 : 0,
                        vmx_ens::accept(inside, ok, factor, lnl_new, lnl_old, word(tok[7])) ? 1 : 0);
        } else if (tok[0] == "H" && tok.size() == 4) {
            const int64_t W = std::atoll(tok[2].c_str()), k = std::atoll(tok[3].c_str());
            if (W < 1 || k < 0 || k >= W) { std::printf("ERR\n"); continue; }
            const int64_t r = vmx_ens::swap_shift(word(tok[1]), W);
            std::printf("%" PRId64 " %" PRId64 "\n", r, vmx_ens::swap_partner(k, r, W));
        } else if (tok[0] == "S" && tok.size() == 6) {
            std::printf("%d\n", vmx_ens::swap_accept(dbl(tok[1]), dbl(tok[2]), dbl(tok[3]), dbl(tok[4]), word(tok[5])) ? 1 : 0);
        } else if (tok[0] == "D" && tok.size() == 3) {
            std::printf("%d\n", vmx_ens::swap_due(std::atoll(tok[1].c_str()), std::atoi(tok[2].c_str())) ? 1 : 0);
        } else if (tok[0] == "L" && tok.size() >= 2) {
            const int T = std::atoi(tok[1].c_str());
            if (T < 0 || tok.size() != (size_t)2 + T) { std::printf("ERR\n"); continue; }
            std::vector<double> beta(T > 0 ? T : 1, 0.0);
            for (int t = 0; t < T; ++t) beta[t] = dbl(tok[2 + t]);
            std::printf("%d\n", vmx_ens::ladder_ok(beta.data(), T) ? 1 : 0);
        } else {
            std::printf("ERR\n");
        }
        std::fflush(stdout);
    }
    return 0;
}
