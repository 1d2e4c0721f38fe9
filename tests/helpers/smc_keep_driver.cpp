// CPU driver of the SMC header's section "kept populations and posterior rounds" (vega_amd/csrc/vmx_smc.h), built by
// tests/test_smc_keep_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers on
// stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   K n N sweeps n_stages stage beta scale ess seed stream topups_left  u[N][n]  lnl[N]  then per stage and sweep the N answers (lnL
//     of the rows asked for; -inf: a failed model)
//       -> per stage U (the kept positions: the particles at entry), then for a ladder stage H (beta_prev beta ESS) and A
//          (ancestors), for a posterior round G (the record row: beta_prev beta ESS), A (ancestors), M (mean), V (cov), F (1:
//          Cholesky factor, 0: fallback; the factor); per sweep Y (inside flags, the deciding uniforms, the proposals) and X
//          (accepted, scale, u, lnl); after the stage T (stage index, topups_left).  A stage that cannot run ends the answer with Z.
//   S E draw beta[E] topups_left[E] rounds  then per round one beta_after per active run, in the order of the list
//       -> L (the active list) and Q (the statuses) of first_active_kept, then per round Q (statuses), O (rounds owed), L (the
//          list compact_active leaves)
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
static void ints(const char* tag, const int32_t* v, int count)
{
    std::printf("%s", tag);
    for (int i = 0; i < count; ++i) std::printf(" %d", v[i]);
    std::printf("\n");
}

int main()
{
    std::string cmd;
    while (next(cmd)) {
        if (cmd == "K") {
            const int n = (int)integer(), N = (int)integer(), sweeps = (int)integer(), n_stages = (int)integer();
            int64_t stage = integer();
            double beta = dbl(), scale = dbl();
            const double ess = dbl();
            const uint64_t seed = word(), stream = word();
            int32_t topups_left = (int32_t)integer();
            if (n < 1 || n > vmx_smc::MAXN || N < 2 || N > vmx_smc::MAX_PARTICLES || sweeps < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u((size_t)N * n), lnl(N), u2((size_t)N * n), lnl2(N), d(N), w(N), c(N), y((size_t)N * n), ua(N);
            std::vector<double> scratch(2 * (size_t)vmx_smc::pad_pow2(N)), totals(2 * vmx_smc::LANES);
            std::vector<double> mean(n), cov((size_t)n * n), C((size_t)n * n), row(3);
            std::vector<int32_t> zero(N, 0), anc(N), inside(N);
            for (auto& v : u) v = dbl();
            for (auto& v : lnl) v = dbl();
            for (int t = 0; t < n_stages && !vmx_smc::run_finished(beta, topups_left); ++t, ++stage) {
                line("U", u);
                const double beta_prev = beta;
                if (vmx_smc::posterior_round(beta_prev)) {
                    const bool chol = vmx_smc::posterior_round_head(u.data(), lnl.data(), N, n, zero.data(), row.data(), anc.data(),
                                                                    mean.data(), cov.data(), C.data());
                    line("G", row);
                    ints("A", anc.data(), N);
                    line("M", mean);
                    line("V", cov);
                    std::printf("F %d", chol ? 1 : 0); for (double x : C) put(x); std::printf("\n");
                    beta = row[1];
                } else {
                    double top = -INFINITY, e = 0.0, s1 = 0.0;
                    for (double v : lnl) top = v > top ? v : top;
                    if (top == -INFINITY) { std::printf("Z\n"); break; }
                    for (int i = 0; i < N; ++i) d[i] = lnl[i] - top;
                    beta = vmx_smc::next_beta(beta_prev, d.data(), N, ess * (double)N, scratch.data(), e, s1);
                    std::printf("H"); put(beta_prev); put(beta); put(e); std::printf("\n");
                    if (!(beta > beta_prev)) { std::printf("Z\n"); break; }
                    for (int i = 0; i < N; ++i) w[i] = vmx_smc::weight(beta - beta_prev, d[i]);
                    vmx_smc::cumulative(w.data(), s1, N, totals.data(), c.data());
                    const double v = vmx_smc::resample_uniform(stage, seed, stream);
                    for (int i = 0; i < N; ++i) {
                        anc[i] = vmx_smc::ancestor(c.data(), N, vmx_smc::position(v, i, N));
                        for (int q = 0; q < n; ++q) u2[(size_t)i * n + q] = u[(size_t)anc[i] * n + q];
                        lnl2[i] = lnl[anc[i]];
                    }
                    ints("A", anc.data(), N);
                    u = u2;
                    lnl = lnl2;
                    for (int a = 0; a < n; ++a) mean[a] = vmx_ns::mean_entry(a, u.data(), zero.data(), N, 0, n);
                    for (int a = 0; a < n; ++a)
                        for (int b = 0; b <= a; ++b)
                            cov[a * n + b] = cov[b * n + a] = vmx_ns::cov_entry(a, b, u.data(), zero.data(), mean.data(), N, 0, n);
                    vmx_ns::whiten(n, cov.data(), C.data());
                }
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
                const int status = vmx_smc::run_status_kept(beta_prev, beta, topups_left);
                std::printf("T %" PRId64 " %d %d\n", stage + 1, (int)topups_left, status);
            }
        } else if (cmd == "S") {
            const int E = (int)integer();
            const bool draw = integer() != 0;
            if (E < 1 || E > 4096) { std::printf("ERR\n"); return 2; }
            std::vector<double> beta(E);
            std::vector<int32_t> owed(E), active(E), status(E);
            for (auto& v : beta) v = dbl();
            for (auto& v : owed) v = (int32_t)integer();
            const int rounds = (int)integer();
            int A = vmx_smc::first_active_kept(beta.data(), owed.data(), E, draw, active.data(), status.data());
            ints("L", active.data(), A);
            ints("Q", status.data(), E);
            for (int r = 0; r < rounds; ++r) {
                for (int a = 0; a < A; ++a) {
                    const int q = active[a];
                    const double after = dbl();
                    status[q] = vmx_smc::run_status_kept(beta[q], after, owed[q]);
                    if (status[q] == vmx_smc::RUNNING || status[q] == vmx_smc::FINISHED) beta[q] = after;
                }
                A = vmx_smc::compact_active(active.data(), A, status.data());
                ints("Q", status.data(), E);
                ints("O", owed.data(), E);
                ints("L", active.data(), A);
            }
        } else {
            std::printf("ERR\n");
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
