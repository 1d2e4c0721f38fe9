// CPU driver of the SMC sampler's header (vega_amd/csrc/vmx_smc.h), built by tests/test_smc_host.py with g++ under
// AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers on stdout; doubles travel as the hex of their
// bits so that nothing is rounded on the way.
//   E count x[count]                         -> one line: pexp of each
//   P i stage sweep j seed stream            -> the four words of the move block
//   V stage seed stream                      -> the resampling uniform
//   D N n seed stream                        -> one line: the start particles u [N][n]
//   B N beta_prev ess lnl[N]                 -> next beta alone: beta, ESS, S1 (beta NaN: no finite lnL)
//   R n N sweeps n_stages stage beta scale ess seed stream  u[N][n]  lnl[N]  then per stage and sweep the N answers (lnL of the
//     rows asked for; -inf: a failed model)  -> per stage the lines H (beta_prev beta ESS S1), W (weights), C (cumulative), A
//                                               (ancestors), M (mean), V (cov), F (1: Cholesky factor, 0: fallback; the factor),
//                                               then per sweep Y (inside flags, the deciding uniforms, the proposals) and X (accepted,
//                                               scale, u, lnl); a stage that cannot run ends the answer with a line Z
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_smc.h"

static bool next(std::string& tok)
{
    char buf[64];
    if (std::scanf("%63s", buf) != 1) return false;
    tok = buf;
    return true;
}
static std::string need() { std::string t; if (!next(t)) { std::printf("ERR\n"); std::exit(2); } return t; }
static uint64_t word() { return std::strtoull(need().c_str(), nullptr, 16); }
static int64_t integer() { return std::atoll(need().c_str()); }
static double dbl() { const uint64_t b = word(); double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static void put(double d) { std::printf(" %016" PRIx64, bits(d)); }
static void line(const char* tag, const std::vector<double>& v)
{
    std::printf("%s", tag);
    for (double x : v) put(x);
    std::printf("\n");
}

// d_i = lnL_i - max lnL; false: no finite lnL
static bool offsets(const std::vector<double>& lnl, std::vector<double>& d)
{
    double top = -INFINITY;
    for (double v : lnl) top = v > top ? v : top;
    if (top == -INFINITY) return false;
    d.resize(lnl.size());
    for (size_t i = 0; i < lnl.size(); ++i) d[i] = lnl[i] - top;
    return true;
}

int main()
{
    std::string cmd;
    while (next(cmd)) {
        if (cmd == "E") {
            const int64_t count = integer();
            std::printf("E");
            for (int64_t i = 0; i < count; ++i) put(vmx_smc::pexp(dbl()));
            std::printf("\n");
        } else if (cmd == "P") {
            const int64_t i = integer(), stage = integer(), sweep = integer(), j = integer();
            const uint64_t seed = word(), stream = word();
            const vmx_ens::Block b = vmx_smc::move_block(i, stage, sweep, j, seed, stream);
            std::printf("P %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b.w[0], b.w[1], b.w[2], b.w[3]);
        } else if (cmd == "V") {
            const int64_t stage = integer();
            const uint64_t seed = word(), stream = word();
            std::printf("V"); put(vmx_smc::resample_uniform(stage, seed, stream)); std::printf("\n");
        } else if (cmd == "D") {
            const int N = (int)integer(), n = (int)integer();
            const uint64_t seed = word(), stream = word();
            if (n < 1 || n > vmx_smc::MAXN || N < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u(n);
            std::printf("D");
            for (int i = 0; i < N; ++i) {
                vmx_smc::draw_start(i, n, seed, stream, u.data());
                for (int c = 0; c < n; ++c) put(u[c]);
            }
            std::printf("\n");
        } else if (cmd == "B") {
            const int N = (int)integer();
            const double beta_prev = dbl(), ess = dbl();
            if (N < 1 || N > vmx_smc::MAX_PARTICLES) { std::printf("ERR\n"); return 2; }
            std::vector<double> lnl(N), d, scratch(2 * (size_t)vmx_smc::pad_pow2(N));
            for (auto& v : lnl) v = dbl();
            double e = NAN, s1 = NAN, beta = NAN;
            if (offsets(lnl, d)) beta = vmx_smc::next_beta(beta_prev, d.data(), N, ess * (double)N, scratch.data(), e, s1);
            std::printf("B"); put(beta); put(e); put(s1); std::printf("\n");
        } else if (cmd == "R") {
            const int n = (int)integer(), N = (int)integer(), sweeps = (int)integer(), n_stages = (int)integer();
            int64_t stage = integer();
            double beta = dbl(), scale = dbl();
            const double ess = dbl();
            const uint64_t seed = word(), stream = word();
            if (n < 1 || n > vmx_smc::MAXN || N < 2 || N > vmx_smc::MAX_PARTICLES || sweeps < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u((size_t)N * n), lnl(N), u2((size_t)N * n), lnl2(N), d, w(N), c(N), y((size_t)N * n), ua(N);
            std::vector<double> scratch(2 * (size_t)vmx_smc::pad_pow2(N)), totals(2 * vmx_smc::LANES);
            std::vector<double> mean(n), cov((size_t)n * n), C((size_t)n * n);
            std::vector<int32_t> zero(N, 0), anc(N), inside(N);
            for (auto& v : u) v = dbl();
            for (auto& v : lnl) v = dbl();
            for (int t = 0; t < n_stages && beta < 1.0; ++t, ++stage) {
                double e = 0.0, s1 = 0.0;
                if (!offsets(lnl, d)) { std::printf("Z\n"); break; }
                const double beta_prev = beta;
                beta = vmx_smc::next_beta(beta_prev, d.data(), N, ess * (double)N, scratch.data(), e, s1);
                std::printf("H"); put(beta_prev); put(beta); put(e); put(s1); std::printf("\n");
                if (!(beta > beta_prev)) { std::printf("Z\n"); break; }
                for (int i = 0; i < N; ++i) w[i] = vmx_smc::weight(beta - beta_prev, d[i]);
                vmx_smc::cumulative(w.data(), s1, N, totals.data(), c.data());
                line("W", w);
                line("C", c);
                const double v = vmx_smc::resample_uniform(stage, seed, stream);
                std::printf("A");
                for (int i = 0; i < N; ++i) {
                    anc[i] = vmx_smc::ancestor(c.data(), N, vmx_smc::position(v, i, N));
                    std::printf(" %d", anc[i]);
                    for (int q = 0; q < n; ++q) u2[(size_t)i * n + q] = u[(size_t)anc[i] * n + q];
                    lnl2[i] = lnl[anc[i]];
                }
                std::printf("\n");
                u = u2;
                lnl = lnl2;
                for (int a = 0; a < n; ++a) mean[a] = vmx_ns::mean_entry(a, u.data(), zero.data(), N, 0, n);
                for (int a = 0; a < n; ++a)
                    for (int b = 0; b <= a; ++b)
                        cov[a * n + b] = cov[b * n + a] = vmx_ns::cov_entry(a, b, u.data(), zero.data(), mean.data(), N, 0, n);
                const bool chol = vmx_ns::whiten(n, cov.data(), C.data());
                line("M", mean);
                line("V", cov);
                std::printf("F %d", chol ? 1 : 0); for (double x : C) put(x); std::printf("\n");
                for (int s = 0; s < sweeps; ++s) {
                    std::printf("Y");
                    for (int i = 0; i < N; ++i) {
                        inside[i] = vmx_smc::propose(i, stage, s, n, C.data(), scale, u.data() + (size_t)i * n, seed, stream,
                                                     y.data() + (size_t)i * n, ua[i]) ? 1 : 0;
                        std::printf(" %d", inside[i]);
                    }
                    for (double x : ua) put(x);
                    for (double x : y) put(x);
                    std::printf("\n");
                    int64_t accepted = 0;
                    for (int i = 0; i < N; ++i) {
                        const double answer = dbl();
                        const bool ok = answer > -INFINITY;
                        if (vmx_smc::accept(inside[i] != 0, ok, beta, answer, lnl[i], ua[i])) {
                            for (int q = 0; q < n; ++q) u[(size_t)i * n + q] = y[(size_t)i * n + q];
                            lnl[i] = answer;
                            accepted += 1;
                        }
                    }
                    scale = vmx_smc::adapt(scale, accepted, N);
                    std::printf("X %" PRId64, accepted); put(scale);
                    for (double x : u) put(x);
                    for (double x : lnl) put(x);
                    std::printf("\n");
                }
            }
        } else {
            std::printf("ERR\n");
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
