// CPU driver of the boost part of the nested sampler's header (vega_amd/csrc/vmx_nested.h "boost"), built by
// tests/test_nested_boost_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   Q k t r f seed stream                    -> phantom_kept: one line "Q 0|1"
//   B n nlive K num_repeats iteration seed stream f  u[nlive][n]  lnl[nlive]  then per round: count, that many answers (the
//                                               answers of the asking threads in ascending thread order; the rounds go on while a
//                                               thread asks)
//                                            -> one whole iteration as the drivers make it: lines K (killed in order), L (L*),
//                                               D (the dead lnL), then in the order they happen P k r kept lnl x[n] (a phantom
//                                               point, kept: phantom_kept at f) and G k r (slice step r of thread k gave up after
//                                               MAX_SHRINK), then per thread E k lnl x[n] (its end point), and N rounds rows
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

int main()
{
    std::string cmd;
    while (next(cmd)) {
        if (cmd == "Q") {
            const int64_t k = integer(), t = integer(), r = integer();
            const double f = dbl();
            const uint64_t seed = word(), stream = word();
            std::printf("Q %d\n", vmx_ns::phantom_kept(k, t, (int32_t)r, f, seed, stream) ? 1 : 0);
        } else if (cmd == "B") {
            const int n = (int)integer(), nlive = (int)integer(), K = (int)integer(), num_repeats = (int)integer();
            const int64_t it = integer();
            const uint64_t seed = word(), stream = word();
            const double f = dbl();
            if (n < 1 || n > vmx_ns::MAXN || nlive > vmx_ns::MAX_LIVE || K < 1 || nlive - K < n + 1 || num_repeats < 1) {
                std::printf("ERR\n");
                return 2;
            }
            std::vector<double> u((size_t)nlive * n), lnl(nlive);
            for (auto& v : u) v = dbl();
            for (auto& v : lnl) v = dbl();
            std::vector<int32_t> rank(nlive), killed(K), surv;
            for (int i = 0; i < nlive; ++i) {
                rank[i] = vmx_ns::rank_of(i, lnl.data(), nlive);
                if (rank[i] < K) killed[rank[i]] = i; else surv.push_back(i);
            }
            std::printf("K"); for (int k = 0; k < K; ++k) std::printf(" %d", killed[k]); std::printf("\n");
            const double lstar = lnl[killed[K - 1]];
            std::printf("L"); put(lstar); std::printf("\n");
            std::printf("D"); for (int k = 0; k < K; ++k) put(lnl[killed[k]]); std::printf("\n");
            std::vector<double> mean(n), cov((size_t)n * n), C((size_t)n * n);
            for (int a = 0; a < n; ++a) mean[a] = vmx_ns::mean_entry(a, u.data(), rank.data(), nlive, K, n);
            for (int a = 0; a < n; ++a)
                for (int b = 0; b <= a; ++b)
                    cov[a * n + b] = cov[b * n + a] = vmx_ns::cov_entry(a, b, u.data(), rank.data(), mean.data(), nlive, K, n);
            (void)vmx_ns::whiten(n, cov.data(), C.data());
            const vmx_ns::Iteration I{C.data(), lstar, it, seed, stream, n, num_repeats};
            std::vector<vmx_ns::Thread> T(K);
            std::vector<char> asks(K);
            int asking = 0;
            for (int k = 0; k < K; ++k) {
                const int s = surv[(size_t)vmx_ns::start_choice(k, it, nlive - K, seed, stream)];
                vmx_ns::start(T[k], n, u.data() + (size_t)s * n, lnl[s]);
                asks[k] = vmx_ns::advance(T[k], I, k, -INFINITY) ? 1 : 0;
                asking += asks[k];
            }
            int64_t rounds = 0, rows = 0;
            while (asking > 0) {
                const int64_t count = integer();
                if (count != asking) { std::printf("ERR\n"); return 2; }
                rounds += 1;
                rows += count;
                asking = 0;
                for (int k = 0; k < K; ++k) {
                    if (!asks[k]) continue;
                    const double answer = dbl();
                    const int32_t state_before = T[k].state, inside_before = T[k].inside, repeat_before = T[k].repeat;
                    asks[k] = vmx_ns::advance(T[k], I, k, answer) ? 1 : 0;
                    asking += asks[k];
                    const int32_t r = vmx_ns::phantom_of(state_before, inside_before, answer, lstar, T[k], num_repeats);
                    const bool accepted = state_before == vmx_ns::S_SHRINK && inside_before != 0 && answer > lstar;
                    if (r > 0) {
                        std::printf("P %d %d %d", k, r, vmx_ns::phantom_kept(k, it, r, f, seed, stream) ? 1 : 0);
                        put(T[k].lnl);
                        for (int i = 0; i < n; ++i) put(T[k].x[i]);
                        std::printf("\n");
                    }
                    if (state_before == vmx_ns::S_SHRINK && T[k].repeat != repeat_before && !accepted)
                        std::printf("G %d %d\n", k, T[k].repeat);
                }
            }
            for (int k = 0; k < K; ++k) {
                std::printf("E %d", k);
                put(T[k].lnl);
                for (int i = 0; i < n; ++i) put(T[k].x[i]);
                std::printf("\n");
            }
            std::printf("N %" PRId64 " %" PRId64 "\n", rounds, rows);
        } else {
            std::printf("ERR\n");
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
