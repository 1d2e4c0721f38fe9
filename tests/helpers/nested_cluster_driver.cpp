// CPU driver of the nested sampler's clustering (vega_amd/csrc/vmx_nested.h, "clustering"), built by
// tests/test_nested_cluster_host.py with g++ under AddressSanitizer / UBSan.  Reads whitespace-separated requests on stdin, answers
// on stdout; doubles travel as the hex of their bits so that nothing is rounded on the way.
//   C m n next_id  u[m][n]  prev_id[m]       -> lines N (the neighbour lists [m][8]), K (level used, cluster count, next_id), S (the
//                                               cluster of every point), I (the new ids), Z (cluster ids, then sizes), M (means),
//                                               F (per cluster 1: Cholesky factor, 0: the diagonal fallback), W (the factors)
//   I n nlive K num_repeats iteration seed stream next_id  u[nlive][n]  lnl[nlive]  live_cluster[nlive]  then per thread: count,
//     that many answers                      -> lines D (the ids of the dead), then N K S I Z M F W of the survivors, B (live index
//                                               each thread starts from), G (the cluster of each start), per thread one line T per
//                                               call of advance (as tests/helpers/nested_driver.cpp), and E (live_cluster after
//                                               the iteration, next_id)
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

struct Clusters {
    std::vector<int32_t> slot, id, size;
    std::vector<double> mean, cov, C;
    int k = 0, nc = 0;
};

// the clustering of the m points (rows surv[p] of u and prev, surv empty: the rows themselves), printed; ids are written into prev
static Clusters cluster(const std::vector<double>& u, const std::vector<int32_t>& surv, int m, int n, std::vector<int32_t>& prev,
                        int32_t& next_id)
{
    using namespace vmx_ns;
    const int32_t* sv = surv.empty() ? nullptr : surv.data();
    std::vector<int32_t> nn((size_t)m * KNN), label(m), size(m), slot0(m);
    Clusters R;
    R.slot.assign(m, 0); R.id.assign(MAX_CLUSTERS, 0); R.size.assign(MAX_CLUSTERS, 0);
    int32_t k = 0, nc = 0;
    cluster_points(u.data(), sv, m, n, prev.data(), &next_id, nn.data(), label.data(), size.data(), slot0.data(), R.slot.data(),
                   R.id.data(), R.size.data(), &k, &nc);
    R.k = k; R.nc = nc;
    R.mean.assign((size_t)nc * n, 0.0); R.cov.assign((size_t)nc * n * n, 0.0); R.C.assign((size_t)nc * n * n, 0.0);
    std::vector<int> chol(nc);
    for (int c = 0; c < nc; ++c) {
        double* mean = R.mean.data() + (size_t)c * n;
        double* cov = R.cov.data() + (size_t)c * n * n;
        for (int a = 0; a < n; ++a) mean[a] = cluster_mean_entry(a, u.data(), sv, R.slot.data(), m, c, R.size[c], n);
        for (int a = 0; a < n; ++a)
            for (int b = 0; b <= a; ++b)
                cov[a * n + b] = cov[b * n + a] = cluster_cov_entry(a, b, u.data(), sv, R.slot.data(), mean, m, c, R.size[c], n);
        chol[c] = whiten(n, cov, R.C.data() + (size_t)c * n * n) ? 1 : 0;
    }
    for (int p = 0; p < m; ++p) prev[row_of(sv, p)] = R.id[R.slot[p]];
    std::printf("N"); for (int32_t v : nn) std::printf(" %d", v); std::printf("\n");
    std::printf("K %d %d %d\n", k, nc, next_id);
    std::printf("S"); for (int32_t v : R.slot) std::printf(" %d", v); std::printf("\n");
    std::printf("I"); for (int p = 0; p < m; ++p) std::printf(" %d", prev[row_of(sv, p)]); std::printf("\n");
    std::printf("Z"); for (int c = 0; c < nc; ++c) std::printf(" %d", R.id[c]); for (int c = 0; c < nc; ++c) std::printf(" %d", R.size[c]);
    std::printf("\n");
    std::printf("M"); for (double v : R.mean) put(v); std::printf("\n");
    std::printf("F"); for (int c = 0; c < nc; ++c) std::printf(" %d", chol[c]); std::printf("\n");
    std::printf("W"); for (double v : R.C) put(v); std::printf("\n");
    return R;
}

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
        if (cmd == "C") {
            const int m = (int)integer(), n = (int)integer();
            int32_t next_id = (int32_t)integer();
            if (n < 1 || n > vmx_ns::MAXN || m < 2 || m > vmx_ns::MAX_LIVE || next_id < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u((size_t)m * n);
            std::vector<int32_t> prev(m);
            for (auto& v : u) v = dbl();
            for (auto& v : prev) v = (int32_t)integer();
            (void)cluster(u, {}, m, n, prev, next_id);
        } else if (cmd == "I") {
            const int n = (int)integer(), nlive = (int)integer(), K = (int)integer(), num_repeats = (int)integer();
            const int64_t it = integer();
            const uint64_t seed = word(), stream = word();
            int32_t next_id = (int32_t)integer();
            if (n < 1 || n > vmx_ns::MAXN || nlive > vmx_ns::MAX_LIVE || K < 1 || nlive - K < n + 1 || next_id < 1) { std::printf("ERR\n"); return 2; }
            std::vector<double> u((size_t)nlive * n), lnl(nlive);
            std::vector<int32_t> live_cluster(nlive);
            for (auto& v : u) v = dbl();
            for (auto& v : lnl) v = dbl();
            for (auto& v : live_cluster) v = (int32_t)integer();
            std::vector<int32_t> rank(nlive), killed(K), surv;
            for (int i = 0; i < nlive; ++i) {
                rank[i] = vmx_ns::rank_of(i, lnl.data(), nlive);
                if (rank[i] < K) killed[rank[i]] = i; else surv.push_back(i);
            }
            const int m = nlive - K;
            const double lstar = lnl[killed[K - 1]];
            std::printf("D"); for (int k = 0; k < K; ++k) std::printf(" %d", live_cluster[killed[k]]); std::printf("\n");
            const Clusters R = cluster(u, surv, m, n, live_cluster, next_id);
            std::vector<int32_t> start(K), start_slot(K);
            for (int k = 0; k < K; ++k) {
                const int64_t choice = vmx_ns::start_choice(k, it, m, seed, stream);
                start[k] = surv[(size_t)choice];
                start_slot[k] = R.slot[(size_t)choice];
            }
            std::printf("B"); for (int k = 0; k < K; ++k) std::printf(" %d", start[k]); std::printf("\n");
            std::printf("G"); for (int k = 0; k < K; ++k) std::printf(" %d", start_slot[k]); std::printf("\n");
            for (int k = 0; k < K; ++k) {
                const vmx_ns::Iteration I{R.C.data() + (size_t)start_slot[k] * n * n, lstar, it, seed, stream, n, num_repeats};
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
                live_cluster[killed[k]] = R.id[start_slot[k]];
            }
            std::printf("E"); for (int32_t v : live_cluster) std::printf(" %d", v); std::printf(" %d\n", next_id);
        } else {
            std::printf("ERR\n");
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
