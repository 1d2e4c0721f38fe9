// CPU driver of the nested sampler's header (vega_amd/csrc/vmx_nested.h), built by tests/test_nested_host.py with g++ under
// AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers on stdout; doubles travel as the hex of their
// bits so that nothing is rounded on the way.
//   D nlive n seed stream                    -> one line: the initial live points u [nlive][n]
//   U lo hi u                                -> map_cube
//   X status chi2 log_norm                   -> lnl_of
//   I n nlive K num_repeats iteration seed stream  u[nlive][n]  lnl[nlive]  then per thread: count, that many answers
//                                            -> lines R (ranks), K (killed in order), L (L*), M (mean), V (cov), C (1: Cholesky
//                                               factor, 0: the diagonal fallback; the factor), S (live index each thread starts
//                                               from), then per thread one line T per call of advance (the first without an
//                                               answer, then one per recorded answer while the thread asks): k asks state repeat
//                                               n_out n_shrink inside draw  L R t lnl  x[n] y[n] d[n]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_nested.h"

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

static void show(int64_t k, bool asks, const vmx_ns::Thread& T, int n)
{
    std::printf("T %" PRId64 " %d %d %d %d %d %d %" PRId64, k, asks ? 1 : 0, T.state, T.repeat, T.n_out, T.n_shrink, T.inside, T.draw);
    put(T.L); put(T.R); put(T.t); put(T.lnl);
    for (int i = 0; i < n; ++i) put(T.x[i]);
    for (int i = 0; i < n; ++i) put(T.y[i]);
    for (int i = 0; i < n; ++i) put(T.d[i]);
    std::printf("\n");
}

int main()
{
    std::string cmd;
    while (next(cmd)) {
        if (cmd == "D") {
            const int nlive = (int)integer(), n = (int)integer();
            const uint64_t seed = word(), stream = word();
            if (n < 1 || n > vmx_ns::MAXN || nlive < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u(n);
            std::printf("D");
            for (int i = 0; i < nlive; ++i) {
                vmx_ns::draw_live(i, n, seed, stream, u.data());
                for (int c = 0; c < n; ++c) put(u[c]);
            }
            std::printf("\n");
        } else if (cmd == "U") {
            const double lo = dbl(), hi = dbl(), u = dbl();
            std::printf("U"); put(vmx_ns::map_cube(lo, hi, u)); std::printf("\n");
        } else if (cmd == "X") {
            const int32_t status = (int32_t)integer();
            const double chi2 = dbl(), log_norm = dbl();
            std::printf("X"); put(vmx_ns::lnl_of(status, chi2, log_norm)); std::printf("\n");
        } else if (cmd == "I") {
            const int n = (int)integer(), nlive = (int)integer(), K = (int)integer(), num_repeats = (int)integer();
            const int64_t it = integer();
            const uint64_t seed = word(), stream = word();
            if (n < 1 || n > vmx_ns::MAXN || nlive > vmx_ns::MAX_LIVE || K < 1 || nlive - K < n + 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u((size_t)nlive * n), lnl(nlive);
            for (auto& v : u) v = dbl();
            for (auto& v : lnl) v = dbl();
            std::vector<int32_t> rank(nlive), killed(K), surv;
            for (int i = 0; i < nlive; ++i) {
                rank[i] = vmx_ns::rank_of(i, lnl.data(), nlive);
                if (rank[i] < K) killed[rank[i]] = i; else surv.push_back(i);
            }
            std::printf("R"); for (int i = 0; i < nlive; ++i) std::printf(" %d", rank[i]); std::printf("\n");
            std::printf("K"); for (int k = 0; k < K; ++k) std::printf(" %d", killed[k]); std::printf("\n");
            const double lstar = lnl[killed[K - 1]];
            std::printf("L"); put(lstar); std::printf("\n");
            std::vector<double> mean(n), cov((size_t)n * n), C((size_t)n * n);
            for (int a = 0; a < n; ++a) mean[a] = vmx_ns::mean_entry(a, u.data(), rank.data(), nlive, K, n);
            for (int a = 0; a < n; ++a)
                for (int b = 0; b <= a; ++b)
                    cov[a * n + b] = cov[b * n + a] = vmx_ns::cov_entry(a, b, u.data(), rank.data(), mean.data(), nlive, K, n);
            const bool chol = vmx_ns::whiten(n, cov.data(), C.data());
            std::printf("M"); for (double v : mean) put(v); std::printf("\n");
            std::printf("V"); for (double v : cov) put(v); std::printf("\n");
            std::printf("C %d", chol ? 1 : 0); for (double v : C) put(v); std::printf("\n");
            std::vector<int32_t> start(K);
            std::printf("S");
            for (int k = 0; k < K; ++k) {
                start[k] = surv[(size_t)vmx_ns::start_choice(k, it, nlive - K, seed, stream)];
                std::printf(" %d", start[k]);
            }
            std::printf("\n");
            const vmx_ns::Iteration I{C.data(), lstar, it, seed, stream, n, num_repeats};
            for (int k = 0; k < K; ++k) {
                vmx_ns::Thread T;
                vmx_ns::start(T, n, u.data() + (size_t)start[k] * n, lnl[start[k]]);
                bool asks = vmx_ns::advance(T, I, k, -INFINITY);
                show(k, asks, T, n);
                const int64_t count = integer();
                for (int64_t a = 0; a < count; ++a) {
                    const double answer = dbl();
                    if (!asks) continue;
                    asks = vmx_ns::advance(T, I, k, answer);
                    show(k, asks, T, n);
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
