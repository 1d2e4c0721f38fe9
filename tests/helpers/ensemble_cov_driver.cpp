// CPU driver of the ensemble sampler's covariance move (vega_amd/csrc/vmx_ensemble.h, the sixth part), built by
// tests/test_ensemble_cov_host.py with g++ under AddressSanitizer / UBSan.  Reads one request per line on stdin, answers one line
// on stdout; words travel in hex and doubles as the hex of their bits so that nothing is rounded on the way.
//   Z w                                      -> the variate of the word
//   T p0 p1 p2 p3                            -> the thresholds t0, t1, t2
//   M t0 t1 t2 w0                            -> the move
//   V n i s h seed stream                    -> the variates z[n] of the walker
//   F n H c[H n]                             -> good, mean[n], C[n n] of half_factor (row stride n | 1, as the kernel's), after
//                                               checking that vmx_ns::mean_entry / cov_entry / whiten over the same rows give the
//                                               same bits (ERR otherwise)
//   P n gamma s[n] z[n] C[n n]               -> y[n]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_nested.h"

static uint64_t word(const std::string& s) { return std::strtoull(s.c_str(), nullptr, 16); }
static double dbl(const std::string& s) { const uint64_t b = word(s); double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

static std::vector<double> row(const std::vector<std::string>& tok, size_t at, size_t n)
{
    std::vector<double> v(n);
    for (size_t d = 0; d < n; ++d) v[d] = dbl(tok[at + d]);
    return v;
}

int main()
{
    static char line[1 << 18];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "Z" && tok.size() == 2) {
            std::printf("%016" PRIx64 "\n", bits(vmx_ens::cov_z(word(tok[1]))));
        } else if (tok[0] == "T" && tok.size() == 5) {
            const double p[4] = {dbl(tok[1]), dbl(tok[2]), dbl(tok[3]), dbl(tok[4])};
            double t0, t1, t2;
            vmx_ens::move_thresholds4(p, t0, t1, t2);
            std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(t0), bits(t1), bits(t2));
        } else if (tok[0] == "M" && tok.size() == 5) {
            std::printf("%d\n", vmx_ens::move_choice4(word(tok[4]), dbl(tok[1]), dbl(tok[2]), dbl(tok[3])));
        } else if (tok[0] == "V" && tok.size() == 7) {
            const int n = std::atoi(tok[1].c_str());
            if (n < 1 || n > 64) { std::printf("ERR\n"); continue; }
            std::vector<double> z(n);
            vmx_ens::cov_variates(n, std::atoll(tok[2].c_str()), std::atoll(tok[3].c_str()), std::atoi(tok[4].c_str()), word(tok[5]),
                                  word(tok[6]), z.data());
            for (int d = 0; d < n; ++d) std::printf("%s%016" PRIx64, d ? " " : "", bits(z[d]));
            std::printf("\n");
        } else if (tok[0] == "F" && tok.size() >= 3) {
            const int n = std::atoi(tok[1].c_str()), H = std::atoi(tok[2].c_str());
            if (n < 1 || n > 64 || H < 2 || tok.size() != (size_t)3 + (size_t)H * n) { std::printf("ERR\n"); continue; }
            const std::vector<double> c = row(tok, 3, (size_t)H * n);
            const int ld = n | 1;
            std::vector<double> mean(n), C((size_t)n * ld), diag(n);
            const bool good = vmx_ens::half_factor(n, H, c.data(), mean.data(), C.data(), ld, diag.data());
            // the nested sampler's serial functions over the same rows: every row a survivor
            std::vector<int32_t> rank(H, 0);
            std::vector<double> m2(n), cov((size_t)n * n, 0.0), C2((size_t)n * n);
            for (int a = 0; a < n; ++a) m2[a] = vmx_ns::mean_entry(a, c.data(), rank.data(), H, 0, n);
            for (int a = 0; a < n; ++a)
                for (int b = 0; b <= a; ++b) cov[(size_t)a * n + b] = vmx_ns::cov_entry(a, b, c.data(), rank.data(), m2.data(), H, 0, n);
            const bool good2 = vmx_ns::whiten(n, cov.data(), C2.data());
            bool same = good == good2;
            for (int a = 0; a < n; ++a) {
                same = same && bits(mean[a]) == bits(m2[a]) && bits(diag[a]) == bits(cov[(size_t)a * n + a]);
                for (int b = 0; b < n; ++b) same = same && bits(C[(size_t)a * ld + b]) == bits(C2[(size_t)a * n + b]);
            }
            if (!same) { std::printf("ERR\n"); continue; }
            std::printf("%d", good ? 1 : 0);
            for (int a = 0; a < n; ++a) std::printf(" %016" PRIx64, bits(mean[a]));
            for (int a = 0; a < n; ++a)
                for (int b = 0; b < n; ++b) std::printf(" %016" PRIx64, bits(C[(size_t)a * ld + b]));
            std::printf("\n");
        } else if (tok[0] == "P" && tok.size() >= 3) {
            const int n = std::atoi(tok[1].c_str());
            if (n < 1 || n > 64 || tok.size() != (size_t)3 + 2 * (size_t)n + (size_t)n * n) { std::printf("ERR\n"); continue; }
            const std::vector<double> s = row(tok, 3, n), C = row(tok, 3 + 2 * (size_t)n, (size_t)n * n);
            std::vector<double> y = row(tok, 3 + (size_t)n, n);
            vmx_ens::cov_propose(n, s.data(), C.data(), n, dbl(tok[2]), y.data());
            for (int d = 0; d < n; ++d) std::printf("%s%016" PRIx64, d ? " " : "", bits(y[d]));
            std::printf("\n");
        } else {
            std::printf("ERR\n");
        }
        std::fflush(stdout);
    }
    return 0;
}
