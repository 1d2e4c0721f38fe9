// CPU driver of what boost adds to a set of nested-sampling runs in vega_amd/csrc/vmx_nested.h ("a set of runs": boost), built by
// tests/test_nested_set_boost_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated tokens on stdin, answers
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   S E n nlive K num_repeats n_iterations seed f  stream[E]  iteration[E]  stop_at[E]  u[E][nlive][n]  lnl[E][nlive]
//     then per set round: total, that many answers (the lnL of the engine's rows 0 .. total - 1 of that round)
//   replays the host loop of vmx_nested_run_many_phantoms over the recorded answers as tests/helpers/nested_set_driver.cpp replays
//   vmx_nested_run_many; every run keeps its phantom points in its own part of one record [E][capacity], capacity =
//   set_phantom_capacity, a round's kept points in thread order at the rows set_phantom_row gives behind the run's own count.
//     per round, active run and phantom point: P run iteration thread r kept row (-1: not kept) lnl x[n]
//     at the end: C the E counts | per run and row of its record: U run iteration thread repeat lnl birth u[n] |
//                 Z the E statuses | D the E iterations done
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
        const double f = dbl();
        if (E < 1 || n < 1 || n > vmx_ns::MAXN || nlive > vmx_ns::MAX_LIVE || K < 1 || nlive - K < n + 1 || num_repeats < 1) {
            std::printf("ERR shape\n");
            return 2;
        }
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
        // the record [E][capacity], exactly as large as the rule says a call needs: a write past it is an ASan report
        const int64_t capacity = vmx_ns::set_phantom_capacity(n_iterations, K, num_repeats);
        const size_t rows = (size_t)E * (size_t)capacity;
        std::vector<double> ph_u(rows * n), ph_lnl(rows), ph_birth(rows);
        std::vector<int64_t> ph_it(rows), ph_count(E, 0);
        std::vector<int32_t> ph_thread(rows), ph_repeat(rows);
        std::vector<int32_t> status(E, vmx_ns::GOING), phase(E), active(E), heading(E), done(E, 0), count(E);
        std::vector<int64_t> offset(E);
        std::vector<double> answers;
        int A = vmx_ns::first_active(status.data(), E, n_iterations, active.data(), phase.data());
        while (A > 0) {
            const int H = vmx_ns::heading_list(active.data(), A, phase.data(), heading.data());
            for (int h = 0; h < H; ++h) {
                const int q = heading[h];
                Run& r = runs[q];
                const int64_t it = it0[q] + done[q];
                r.surv.clear();
                for (int i = 0; i < nlive; ++i) {
                    r.rank[i] = vmx_ns::rank_of(i, r.lnl.data(), nlive);
                    if (r.rank[i] < K) r.killed[r.rank[i]] = i; else r.surv.push_back(i);
                }
                r.lstar = r.lnl[r.killed[K - 1]];
                for (int a = 0; a < n; ++a) r.mean[a] = vmx_ns::mean_entry(a, r.u.data(), r.rank.data(), nlive, K, n);
                for (int a = 0; a < n; ++a)
                    for (int b = 0; b <= a; ++b)
                        r.cov[a * n + b] = r.cov[b * n + a] = vmx_ns::cov_entry(a, b, r.u.data(), r.rank.data(), r.mean.data(), nlive, K, n);
                (void)vmx_ns::whiten(n, r.cov.data(), r.C.data());
                for (int k = 0; k < K; ++k) {
                    const int i = r.surv[(size_t)vmx_ns::start_choice(k, it, nlive - K, seed, stream[q])];
                    vmx_ns::start(r.th[k], n, r.u.data() + (size_t)i * n, r.lnl[i]);
                    r.slot[k] = -1;
                }
                phase[q] = vmx_ns::WALK;
            }
            // the advance with the phantom step: a run OUT is not in the list and writes nothing
            for (int a = 0; a < A; ++a) {
                const int q = active[a];
                Run& r = runs[q];
                const int64_t it = it0[q] + done[q];
                const vmx_ns::Iteration I{r.C.data(), r.lstar, it, seed, stream[q], n, num_repeats};
                count[a] = 0;
                int64_t p = 0;          // the round's kept points of this run so far, in thread order
                for (int k = 0; k < K; ++k) {
                    vmx_ns::Thread& T = r.th[k];
                    r.asks[k] = 0;
                    if (T.state == vmx_ns::S_DONE) continue;
                    const double answer = r.slot[k] >= 0 ? answers.at((size_t)r.slot[k]) : -INFINITY;
                    const int32_t state_before = T.state, inside_before = T.inside;
                    r.asks[k] = vmx_ns::advance(T, I, k, answer) ? 1 : 0;
                    count[a] += r.asks[k];
                    const int32_t rr = vmx_ns::phantom_of(state_before, inside_before, answer, r.lstar, T, num_repeats);
                    if (rr <= 0) continue;
                    const bool kept = vmx_ns::phantom_kept(k, it, rr, f, seed, stream[q]);
                    int64_t row = -1;
                    if (kept) {
                        row = vmx_ns::set_phantom_row(q, capacity, ph_count[q], p);
                        p += 1;
                        if (row < (int64_t)q * capacity || row >= (int64_t)(q + 1) * capacity) { std::printf("ERR row\n"); return 2; }
                        for (int d = 0; d < n; ++d) ph_u.at((size_t)row * n + d) = T.x[d];
                        ph_lnl.at((size_t)row) = T.lnl; ph_birth.at((size_t)row) = r.lstar;
                        ph_it.at((size_t)row) = it; ph_thread.at((size_t)row) = k; ph_repeat.at((size_t)row) = T.repeat;
                    }
                    std::printf("P %d %" PRId64 " %d %d %d %" PRId64, q, it, k, (int)rr, kept ? 1 : 0, row);
                    put(T.lnl);
                    for (int d = 0; d < n; ++d) put(T.x[d]);
                    std::printf("\n");
                }
                ph_count[q] += p;       // (before the end of the iteration, should it end in this round)
            }
            const int64_t total = vmx_ns::row_offsets(count.data(), A, offset.data());
            for (int a = 0; a < A; ++a) {
                const int q = active[a];
                Run& r = runs[q];
                int64_t row = offset[a];
                for (int k = 0; k < K; ++k) {
                    r.slot[k] = r.asks[k] ? (int32_t)row : -1;
                    row += r.asks[k];
                }
                if (vmx_ns::iteration_ended(count[a]))
                    for (int k = 0; k < K; ++k) {
                        const int i = r.killed[k];
                        for (int d = 0; d < n; ++d) r.u[(size_t)i * n + d] = r.th[k].x[d];
                        r.lnl[i] = r.th[k].lnl;
                    }
            }
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
        std::printf("C %d", E);
        for (int q = 0; q < E; ++q) std::printf(" %" PRId64, ph_count[q]);
        std::printf("\n");
        for (int q = 0; q < E; ++q)
            for (int64_t i = 0; i < ph_count[q]; ++i) {
                const size_t row = (size_t)vmx_ns::set_phantom_row(q, capacity, 0, i);
                std::printf("U %d %" PRId64 " %d %d", q, ph_it.at(row), (int)ph_thread.at(row), (int)ph_repeat.at(row));
                put(ph_lnl.at(row)); put(ph_birth.at(row));
                for (int d = 0; d < n; ++d) put(ph_u.at(row * n + d));
                std::printf("\n");
            }
        put_list("Z", status.data(), E);
        put_list("D", done.data(), E);
        std::fflush(stdout);
    }
    return 0;
}
