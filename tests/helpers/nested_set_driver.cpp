// CPU driver of what a set of nested-sampling runs adds to vega_amd/csrc/vmx_nested.h ("a set of runs"), built by
// tests/test_nested_set_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated tokens on stdin, answers on
// stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   S E n nlive K num_repeats n_iterations seed  stream[E]  iteration[E]  stop_at[E]  u[E][nlive][n]  lnl[E][nlive]
//     then per set round: total, that many answers (the lnL of the engine's rows 0 .. total - 1 of that round)
//   replays the host loop of vmx_nested_run_many over the recorded answers; run e's stop callback says yes once its iterations
//   reach stop_at[e] (-1: never).  Per round the lines
//     N round | A the active list | G the heading list
//     per headed run: H run iteration, then R, K, L, M, V, C, S as tests/helpers/nested_driver.cpp prints them
//     per active run and thread: T run, then what nested_driver.cpp prints per call of advance
//     O per active run: run count offset | Q total, then per engine row: run thread | P the E phases after the launches
//   and at the end: Z the E statuses | D the E iterations done | F every run's live points and their lnL.
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
static std::string need() { std::string t; if (!next(t)) { std::printf("ERR input\n"); std::exit(2); } return t; }
static uint64_t word() { return std::strtoull(need().c_str(), nullptr, 16); }
static int64_t integer() { return std::atoll(need().c_str()); }
static double dbl() { const uint64_t b = word(); double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static void put(double d) { std::printf(" %016" PRIx64, bits(d)); }
static void put_list(const char* tag, const int32_t* v, int count)
{
    std::printf("%s %d", tag, count);
    for (int i = 0; i < count; ++i) std::printf(" %d", (int)v[i]);
    std::printf("\n");
}

static void show(int run, int64_t k, bool asks, const vmx_ns::Thread& T, int n)
{
    std::printf("T %d %" PRId64 " %d %d %d %d %d %d %" PRId64, run, k, asks ? 1 : 0, T.state, T.repeat, T.n_out, T.n_shrink, T.inside, T.draw);
    put(T.L); put(T.R); put(T.t); put(T.lnl);
    for (int i = 0; i < n; ++i) put(T.x[i]);
    for (int i = 0; i < n; ++i) put(T.y[i]);
    for (int i = 0; i < n; ++i) put(T.d[i]);
    std::printf("\n");
}

struct Run {
    std::vector<double> u, lnl, mean, cov, C;
    std::vector<int32_t> rank, killed, surv, slot;
    std::vector<vmx_ns::Thread> th;
    std::vector<char> asks;
    double lstar = 0.0;
};

int main()
{
    std::string cmd;
    while (next(cmd)) {
        if (cmd != "S") { std::printf("ERR command\n"); return 2; }
        const int E = (int)integer(), n = (int)integer(), nlive = (int)integer(), K = (int)integer(), num_repeats = (int)integer();
        const int64_t n_iterations = integer();
        const uint64_t seed = word();
        if (E < 1 || n < 1 || n > vmx_ns::MAXN || nlive > vmx_ns::MAX_LIVE || K < 1 || nlive - K < n + 1) { std::printf("ERR shape\n"); return 2; }
        std::vector<uint64_t> stream(E);
        std::vector<int64_t> it0(E), stop_at(E);
        for (auto& v : stream) v = word();
        for (auto& v : it0) v = integer();
        for (auto& v : stop_at) v = integer();
        std::vector<Run> runs(E);
        for (Run& r : runs) {
            r.u.resize((size_t)nlive * n); r.lnl.resize(nlive); r.mean.resize(n); r.cov.resize((size_t)n * n); r.C.resize((size_t)n * n);
            r.rank.resize(nlive); r.killed.resize(K); r.slot.assign(K, -1); r.th.resize(K); r.asks.assign(K, 0);
            for (auto& v : r.u) v = dbl();
        }
        for (Run& r : runs)
            for (auto& v : r.lnl) v = dbl();
        // (exactly E entries each: a write past a list is an ASan report)
        std::vector<int32_t> status(E, vmx_ns::GOING), phase(E), active(E), heading(E), done(E, 0), count(E);
        std::vector<int64_t> offset(E);
        std::vector<double> answers;
        int A = vmx_ns::first_active(status.data(), E, n_iterations, active.data(), phase.data());
        for (int round = 0; A > 0; ++round) {
            const int H = vmx_ns::heading_list(active.data(), A, phase.data(), heading.data());
            std::printf("N %d\n", round);
            put_list("A", active.data(), A);
            put_list("G", heading.data(), H);
            // the head launch
            for (int h = 0; h < H; ++h) {
                const int q = heading[h];
                Run& r = runs[q];
                const int64_t it = it0[q] + done[q];
                std::printf("H %d %" PRId64 "\n", q, it);
                r.surv.clear();
                for (int i = 0; i < nlive; ++i) {
                    r.rank[i] = vmx_ns::rank_of(i, r.lnl.data(), nlive);
                    if (r.rank[i] < K) r.killed[r.rank[i]] = i; else r.surv.push_back(i);
                }
                std::printf("R"); for (int i = 0; i < nlive; ++i) std::printf(" %d", r.rank[i]); std::printf("\n");
                std::printf("K"); for (int k = 0; k < K; ++k) std::printf(" %d", r.killed[k]); std::printf("\n");
                r.lstar = r.lnl[r.killed[K - 1]];
                std::printf("L"); put(r.lstar); std::printf("\n");
                for (int a = 0; a < n; ++a) r.mean[a] = vmx_ns::mean_entry(a, r.u.data(), r.rank.data(), nlive, K, n);
                for (int a = 0; a < n; ++a)
                    for (int b = 0; b <= a; ++b)
                        r.cov[a * n + b] = r.cov[b * n + a] = vmx_ns::cov_entry(a, b, r.u.data(), r.rank.data(), r.mean.data(), nlive, K, n);
                const bool chol = vmx_ns::whiten(n, r.cov.data(), r.C.data());
                std::printf("M"); for (double v : r.mean) put(v); std::printf("\n");
                std::printf("V"); for (double v : r.cov) put(v); std::printf("\n");
                std::printf("C %d", chol ? 1 : 0); for (double v : r.C) put(v); std::printf("\n");
                std::printf("S");
                for (int k = 0; k < K; ++k) {
                    const int i = r.surv[(size_t)vmx_ns::start_choice(k, it, nlive - K, seed, stream[q])];
                    std::printf(" %d", i);
                    vmx_ns::start(r.th[k], n, r.u.data() + (size_t)i * n, r.lnl[i]);
                    r.slot[k] = -1;
                }
                std::printf("\n");
                phase[q] = vmx_ns::WALK;
            }
            // the advance: every thread takes the answer of the row it asked for; the run counts its requests
            for (int a = 0; a < A; ++a) {
                const int q = active[a];
                Run& r = runs[q];
                const vmx_ns::Iteration I{r.C.data(), r.lstar, it0[q] + done[q], seed, stream[q], n, num_repeats};
                count[a] = 0;
                for (int k = 0; k < K; ++k) {
                    vmx_ns::Thread& T = r.th[k];
                    r.asks[k] = 0;
                    if (T.state != vmx_ns::S_DONE) {
                        const double answer = r.slot[k] >= 0 ? answers.at((size_t)r.slot[k]) : -INFINITY;
                        r.asks[k] = vmx_ns::advance(T, I, k, answer) ? 1 : 0;
                    }
                    count[a] += r.asks[k];
                    show(q, k, r.asks[k] != 0, T, n);
                }
            }
            // the packing, in ascending (run, thread) order
            const int64_t total = vmx_ns::row_offsets(count.data(), A, offset.data());
            std::vector<int32_t> row_run((size_t)total), row_thread((size_t)total);
            for (int a = 0; a < A; ++a) {
                const int q = active[a];
                Run& r = runs[q];
                std::printf("O %d %d %" PRId64 "\n", q, count[a], offset[a]);
                int64_t row = offset[a];
                for (int k = 0; k < K; ++k) {
                    r.slot[k] = r.asks[k] ? (int32_t)row : -1;
                    if (!r.asks[k]) continue;
                    row_run.at((size_t)row) = q;
                    row_thread.at((size_t)row) = k;
                    row += 1;
                }
                if (vmx_ns::iteration_ended(count[a]))          // the end points take the killed points' slots
                    for (int k = 0; k < K; ++k) {
                        const int i = r.killed[k];
                        for (int d = 0; d < n; ++d) r.u[(size_t)i * n + d] = r.th[k].x[d];
                        r.lnl[i] = r.th[k].lnl;
                    }
            }
            std::printf("Q %" PRId64, total);
            for (int64_t row = 0; row < total; ++row) std::printf(" %d %d", row_run[(size_t)row], row_thread[(size_t)row]);
            std::printf("\n");
            put_list("P", phase.data(), E);
            // the host's turn
            if (integer() != total) { std::printf("ERR total\n"); return 2; }
            answers.resize((size_t)total);
            for (auto& v : answers) v = dbl();
            for (int a = 0; a < A; ++a) {
                const int q = active[a];
                if (!vmx_ns::iteration_ended(count[a])) { phase[q] = vmx_ns::WALK; continue; }
                done[q] += 1;
                const bool stopped = stop_at[q] >= 0 && it0[q] + done[q] >= stop_at[q];
                phase[q] = vmx_ns::after_iteration(stopped, done[q], n_iterations, &status[q]);
            }
            A = vmx_ns::compact_active(active.data(), A, phase.data());
        }
        put_list("Z", status.data(), E);
        put_list("D", done.data(), E);
        std::printf("F");
        for (const Run& r : runs) { for (double v : r.u) put(v); for (double v : r.lnl) put(v); }
        std::printf("\n");
        std::fflush(stdout);
    }
    return 0;
}
