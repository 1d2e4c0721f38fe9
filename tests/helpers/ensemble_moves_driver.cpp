// CPU driver of the ensemble sampler's differential-evolution and snooker moves (vega_amd/csrc/vmx_ensemble.h, the second part),
// built by tests/test_ensemble_moves_host.py with g++ under AddressSanitizer / UBSan.  Reads one request per line on stdin, answers
// one line on stdout; words travel in hex and doubles as the hex of their bits so that nothing is rounded on the way.
//   B i s h seed stream                      -> block B of the walker (4 hex words)
//   T p0 p1 p2                               -> the thresholds t0, t1
//   M t0 t1 H a0 a1 a3 b0                    -> move, j1, j2, j3 (j2 = -1 with H < 2, j3 = -1 with H < 3: not defined there)
//   D gamma0 sigma b1 b2 n s[n] c1[n] c2[n]  -> gamma, y[n]
//   S gamma_s n s[n] z[n] z1[n] z2[n]        -> ok, factor, y[n]
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

static std::vector<double> row(const std::vector<std::string>& tok, size_t at, int n)
{
    std::vector<double> v(n);
    for (int d = 0; d < n; ++d) v[d] = dbl(tok[at + d]);
    return v;
}

int main()
{
    static char line[1 << 18];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "B" && tok.size() == 6) {
            const vmx_ens::Block b = vmx_ens::move_block(std::atoll(tok[1].c_str()), std::atoll(tok[2].c_str()), std::atoi(tok[3].c_str()),
                                                         word(tok[4]), word(tok[5]));
            std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b.w[0], b.w[1], b.w[2], b.w[3]);
        } else if (tok[0] == "T" && tok.size() == 4) {
            const double p[3] = {dbl(tok[1]), dbl(tok[2]), dbl(tok[3])};
            double t0, t1;
            vmx_ens::move_thresholds(p, t0, t1);
            std::printf("%016" PRIx64 " %016" PRIx64 "\n", bits(t0), bits(t1));
        } else if (tok[0] == "M" && tok.size() == 8) {
            const double t0 = dbl(tok[1]), t1 = dbl(tok[2]);
            const int64_t H = std::atoll(tok[3].c_str());
            const int move = vmx_ens::move_choice(word(tok[7]), t0, t1);
            const int64_t j1 = vmx_ens::partner(word(tok[4]), H);
            const int64_t j2 = H >= 2 ? vmx_ens::partner2(word(tok[5]), H, j1) : -1;
            const int64_t j3 = H >= 3 ? vmx_ens::partner3(word(tok[6]), H, j1, j2) : -1;
            std::printf("%d %" PRId64 " %" PRId64 " %" PRId64 "\n", move, j1, j2, j3);
        } else if (tok[0] == "D" && tok.size() >= 6) {
            const int n = std::atoi(tok[5].c_str());
            if (n < 1 || tok.size() != (size_t)6 + 3 * n) { std::printf("ERR\n"); continue; }
            const double gamma = vmx_ens::de_gamma(dbl(tok[1]), dbl(tok[2]), word(tok[3]), word(tok[4]));
            const std::vector<double> s = row(tok, 6, n), c1 = row(tok, 6 + n, n), c2 = row(tok, 6 + 2 * n, n);
            std::printf("%016" PRIx64, bits(gamma));
            for (int d = 0; d < n; ++d) std::printf(" %016" PRIx64, bits(vmx_ens::de_propose(s[d], c1[d], c2[d], gamma)));
            std::printf("\n");
        } else if (tok[0] == "S" && tok.size() >= 3) {
            const int n = std::atoi(tok[2].c_str());
            if (n < 1 || tok.size() != (size_t)3 + 4 * n) { std::printf("ERR\n"); continue; }
            const std::vector<double> s = row(tok, 3, n), z = row(tok, 3 + n, n), z1 = row(tok, 3 + 2 * n, n), z2 = row(tok, 3 + 3 * n, n);
            std::vector<double> y(n);
            double factor = 0.0;
            const bool ok = vmx_ens::snooker_propose(n, s.data(), z.data(), z1.data(), z2.data(), dbl(tok[1]), y.data(), factor);
            std::printf("%d %016" PRIx64, ok ? 1 : 0, bits(factor));
            for (int d = 0; d < n; ++d) std::printf(" %016" PRIx64, bits(y[d]));
            std::printf("\n");
        } else {
            std::printf("ERR\n");
        }
        std::fflush(stdout);
    }
    return 0;
}
