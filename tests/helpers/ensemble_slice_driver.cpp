// Ensemble slice sampling without a GPU: vega_amd/csrc/vmx_ensemble.h (the fifth part) compiled for the host, for
// tests/test_ensemble_slice_host.py.  One command per line on stdin; doubles travel as the 16 hex digits of their bits, words as hex.
//   S L R word                 -> slice_shrink
//   Y lnl word                 -> slice_height
//   P H w0 w1                  -> partner, partner2
//   T mu expansions contractions -> slice_tune
//   K k s h j seed stream      -> slice_block, four words
//   RUN n W E step0 n_steps thin tune_steps max_e max_c seed log_norm   then, each on a line of its own: streams [E], mu [E], lo [n],
//       hi [n], x [E W n], lnl [E W], accepted [E W]; then the set's rounds: after every round the whole state is printed, and the
//       answers of the round's rows are read - `status chi2` per row, in row order.  The loop is the device driver's: a pass over
//       every running ensemble (answers, machines, and while it asks for nothing commit / tune / record / open), the packing, the
//       compaction.  Ends with the chain.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../vega_amd/csrc/vmx_ensemble.h"

using namespace vmx_ens;

static double from_hex(const std::string& s)
{
    const uint64_t b = std::stoull(s, nullptr, 16);
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

static void put(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    std::printf(" %016" PRIx64, b);
}

static bool read_words(std::vector<uint64_t>& out, size_t count)
{
    std::string line, tok;
    if (!std::getline(std::cin, line)) return false;
    std::istringstream in(line);
    out.clear();
    while (in >> tok) out.push_back(std::stoull(tok, nullptr, 16));
    return out.size() == count;
}

static bool read_doubles(std::vector<double>& out, size_t count)
{
    std::vector<uint64_t> words;
    if (!read_words(words, count)) return false;
    out.resize(count);
    if (count) std::memcpy(out.data(), words.data(), count * sizeof(double));
    return true;
}

struct Run {
    int n, W, E, H, n_steps, thin, tune_steps, max_e, max_c;
    int64_t step0, rows;
    uint64_t seed;
    double log_norm;
    std::vector<uint64_t> streams;
    std::vector<double> mu, lo, hi, x, lnl, eta, chain, chain_lnl;
    std::vector<int64_t> accepted, counts, step_counts, q;
    std::vector<SliceWalker> wk;
    std::vector<int32_t> slot, row_walker, open, opened, active, count_of;
    std::vector<int32_t> status;
    std::vector<double> chi2;

    int pass(int e, bool opening)
    {
        const int64_t s = slice_step(step0, q[e]);
        const int h = slice_half(q[e]);
        const double* xe = x.data() + (size_t)e * W * n;
        int total = 0;
        for (int k = 0; k < H; ++k) {
            SliceWalker& w = wk[(size_t)e * H + k];
            double* et = eta.data() + ((size_t)e * H + k) * n;
            const double* xk = xe + ((size_t)h * H + k) * n;
            if (opening) {
                slice_open(w, et, n, xk, lnl[(size_t)e * W + (size_t)h * H + k], xe + (size_t)(1 - h) * H * n, H, mu[e], lo.data(), hi.data(),
                           max_e, max_c, k, s, h, seed, streams[e]);
            } else if (w.asks) {
                const int row = slot[(size_t)e * H + k];
                slice_advance(w, n, xk, et, lo.data(), hi.data(), log_norm, status[row], chi2[row], max_e, max_c, k, s, h, seed, streams[e]);
            }
            if (w.asks) {
                slot[(size_t)e * H + k] = total;
                row_walker[(size_t)e * H + total] = k;
                total += 1;
            }
        }
        return total;
    }

    void commit(int e)
    {
        const int64_t s = slice_step(step0, q[e]);
        const int h = slice_half(q[e]);
        int64_t took[SLICE_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < H; ++k) {
            const size_t w = (size_t)e * W + (size_t)h * H + k;
            accepted[w] += slice_commit(wk[(size_t)e * H + k], n, x.data() + w * n, eta.data() + ((size_t)e * H + k) * n, &lnl[w], took);
        }
        for (int i = 0; i < SLICE_COUNTS; ++i) counts[(size_t)e * SLICE_COUNTS + i] += took[i];
        step_counts[2 * e] += took[SC_EXPANSIONS];
        step_counts[2 * e + 1] += took[SC_CONTRACTIONS];
        if (h != 1) return;
        if (slice_tune_due(s, tune_steps)) mu[e] = slice_tune(mu[e], step_counts[2 * e], step_counts[2 * e + 1]);
        step_counts[2 * e] = step_counts[2 * e + 1] = 0;
        if ((s + 1) % thin == 0) {
            const size_t r = (size_t)e * rows + (size_t)((s + 1) / thin - step0 / thin - 1);
            std::memcpy(chain.data() + r * W * n, x.data() + (size_t)e * W * n, (size_t)W * n * sizeof(double));
            std::memcpy(chain_lnl.data() + r * W, lnl.data() + (size_t)e * W, (size_t)W * sizeof(double));
        }
    }

    void dump(int round, int A, const std::vector<int32_t>& count, const std::vector<int32_t>& offset, int total) const
    {
        std::printf("ROUND %d %d %d\n", round, A, total);
        for (int a = 0; a < A; ++a) std::printf("LIST %d %d %d\n", (int)active[a], (int)count[a], (int)offset[a]);
        for (int e = 0; e < E; ++e) {
            std::printf("ENS %d %" PRId64 " %d %d", e, q[e], (int)open[e], (int)count_of[e]);
            put(mu[e]);
            for (int i = 0; i < SLICE_COUNTS; ++i) std::printf(" %" PRId64, counts[(size_t)e * SLICE_COUNTS + i]);
            std::printf(" %" PRId64 " %" PRId64 "\n", step_counts[2 * e], step_counts[2 * e + 1]);
            if (opened[e])
                for (int k = 0; k < H; ++k) {
                    const SliceWalker& w = wk[(size_t)e * H + k];
                    std::printf("WK %d %d", e, k);
                    put(w.L); put(w.R); put(w.t); put(w.lnY); put(w.lnl);
                    std::printf(" %d %d %d %d %d %d %d %d %d %d %d", w.phase, w.draw, w.left, w.right, w.contractions, w.rows, w.box, w.failed,
                                w.end, w.asks, (int)slot[(size_t)e * H + k]);
                    for (int d = 0; d < n; ++d) put(eta[((size_t)e * H + k) * n + d]);
                    std::printf("\n");
                }
            std::printf("X %d", e);
            for (size_t i = 0; i < (size_t)W * n; ++i) put(x[(size_t)e * W * n + i]);
            std::printf("\nL %d", e);
            for (int i = 0; i < W; ++i) put(lnl[(size_t)e * W + i]);
            std::printf("\nA %d", e);
            for (int i = 0; i < W; ++i) std::printf(" %" PRId64, accepted[(size_t)e * W + i]);
            std::printf("\n");
        }
    }

    int go()
    {
        int A = n_steps > 0 ? E : 0, round = 0;
        for (int e = 0; e < E; ++e) active[e] = e;
        std::vector<int32_t> count(E), offset(E);
        while (A > 0) {
            for (int a = 0; a < A; ++a) {
                const int e = active[a];
                int total = open[e] ? pass(e, false) : 0;
                while (total == 0) {
                    if (open[e]) { commit(e); q[e] += 1; open[e] = 0; }
                    if (q[e] >= 2 * (int64_t)n_steps) break;
                    total = pass(e, true);
                    open[e] = opened[e] = 1;
                }
                count[a] = total;
            }
            const int total = slice_offsets(count.data(), A, offset.data());
            for (int a = 0; a < A; ++a) {
                const int e = active[a];
                for (int r = 0; r < count[a]; ++r) slot[(size_t)e * H + row_walker[(size_t)e * H + r]] = offset[a] + r;
                count_of[e] = count[a];
            }
            dump(round, A, count, offset, total);
            for (int a = 0; a < A; ++a) {
                const int e = active[a], h = slice_half(q[e]);
                for (int r = 0; r < count[a]; ++r) {
                    const int k = row_walker[(size_t)e * H + r];
                    const SliceWalker& w = wk[(size_t)e * H + k];
                    std::printf("ROW %d %d", offset[a] + r, e);
                    for (int d = 0; d < n; ++d)
                        put(slice_point(x[((size_t)e * W + (size_t)h * H + k) * n + d], w.t, eta[((size_t)e * H + k) * n + d]));
                    std::printf("\n");
                }
            }
            status.assign(total, 0);
            chi2.assign(total, 0.0);
            for (int r = 0; r < total; ++r) {
                std::string line, tok;
                if (!std::getline(std::cin, line)) return 1;
                std::istringstream in(line);
                if (!(in >> status[r] >> tok)) return 1;
                chi2[r] = from_hex(tok);
            }
            A = slice_compact(active.data(), A, count_of.data());
            round += 1;
        }
        std::printf("END %d\n", round);
        for (int e = 0; e < E; ++e) {
            std::printf("MU %d", e);
            put(mu[e]);
            std::printf("\nCHAIN %d", e);
            for (size_t i = 0; i < (size_t)rows * W * n; ++i) put(chain[(size_t)e * rows * W * n + i]);
            std::printf("\nCHAINL %d", e);
            for (size_t i = 0; i < (size_t)rows * W; ++i) put(chain_lnl[(size_t)e * rows * W + i]);
            std::printf("\n");
        }
        return 0;
    }
};

static int run(std::istringstream& in)
{
    Run R;
    std::string tok, seed;
    if (!(in >> R.n >> R.W >> R.E >> R.step0 >> R.n_steps >> R.thin >> R.tune_steps >> R.max_e >> R.max_c >> seed >> tok)) return 1;
    R.seed = std::stoull(seed, nullptr, 16);
    R.log_norm = from_hex(tok);
    R.H = R.W / 2;
    if (R.n < 1 || R.E < 1 || R.W % 2 || R.thin < 1 || R.n_steps < 0 || R.step0 < 0) return 1;
    std::string line;
    if (!read_words(R.streams, R.E)) return 1;
    if (!read_doubles(R.mu, R.E) || !read_doubles(R.lo, R.n) || !read_doubles(R.hi, R.n)) return 1;
    const size_t EW = (size_t)R.E * R.W, EH = (size_t)R.E * R.H;
    if (!read_doubles(R.x, EW * R.n) || !read_doubles(R.lnl, EW)) return 1;
    if (!std::getline(std::cin, line)) return 1;
    std::istringstream acc(line);
    R.accepted.resize(EW);
    for (size_t i = 0; i < EW; ++i)
        if (!(acc >> R.accepted[i])) return 1;
    if (!slice_ok(R.H, 1.0, R.tune_steps, R.max_e, R.max_c, 0)) return 1;
    R.rows = (R.step0 + R.n_steps) / R.thin - R.step0 / R.thin;
    R.chain.assign((size_t)R.rows * EW * R.n, 0.0);
    R.chain_lnl.assign((size_t)R.rows * EW, 0.0);
    R.eta.assign(EH * R.n, 0.0);
    R.wk.assign(EH, SliceWalker{});
    R.slot.assign(EH, -1);
    R.row_walker.assign(EH, -1);
    R.counts.assign((size_t)R.E * SLICE_COUNTS, 0);
    R.step_counts.assign((size_t)R.E * 2, 0);
    R.q.assign(R.E, 0);
    R.open.assign(R.E, 0);
    R.opened.assign(R.E, 0);
    R.active.assign(R.E, 0);
    R.count_of.assign(R.E, 0);
    return R.go();
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, a, b, c;
        in >> cmd;
        if (cmd == "S" && in >> a >> b >> c) {
            put(slice_shrink(from_hex(a), from_hex(b), std::stoull(c, nullptr, 16)));
        } else if (cmd == "Y" && in >> a >> b) {
            put(slice_height(from_hex(a), std::stoull(b, nullptr, 16)));
        } else if (cmd == "P" && in >> a >> b >> c) {
            const int64_t H = std::stoll(a), j1 = partner(std::stoull(b, nullptr, 16), H);
            std::printf(" %" PRId64 " %" PRId64, j1, partner2(std::stoull(c, nullptr, 16), H, j1));
        } else if (cmd == "T" && in >> a >> b >> c) {
            put(slice_tune(from_hex(a), std::stoll(b), std::stoll(c)));
        } else if (cmd == "K") {
            int64_t k, s, j;
            int h;
            std::string seed, stream;
            if (!(in >> k >> s >> h >> j >> seed >> stream)) { std::printf("ERR\n"); continue; }
            const Block blk = slice_block(k, s, h, j, std::stoull(seed, nullptr, 16), std::stoull(stream, nullptr, 16));
            for (int i = 0; i < 4; ++i) std::printf(" %" PRIx64, blk.w[i]);
        } else if (cmd == "RUN") {
            if (run(in)) { std::printf("ERR\n"); return 1; }
            continue;
        } else {
            std::printf("ERR");
        }
        std::printf("\n");
    }
    return 0;
}
