// CPU driver of the trapezoidal ("root") tapes of vmx_plan::plan_quad_tape (vega_amd/csrc/vmx_plan.h), built by
// tests/test_planner_root_host.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// and run without a GPU: prints one line per case, "FAIL ..." and a non-zero exit code when an invariant breaks.
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>

#include "../../vega_amd/csrc/vmx_plan.h"

using namespace vmx_plan;

static int failures = 0;
static void expect(bool ok, const char* what)
{
    if (!ok) { std::printf("FAIL %s\n", what); ++failures; }
}

static int pad32(int n) { return (n + 31) / 32 * 32; }

struct Shape { int rows, cols; };      // (n_masked, nq) of an item

// every K range covered once by its segments, indices 0, 1, .. in K order, as many as seg_count says and no more than max_segs
// (what the partial buffer holds): counted here on its own, beside check_quad_tape
static void segments(const Tape& T, const std::vector<TapeProblem>& probs, int tn, const char* label)
{
    std::map<std::tuple<int, int, int>, std::vector<std::tuple<int, int, int>>> ranges;
    for (auto& w : T.work) ranges[{w.prob, w.mt, w.nt}].push_back({w.kbeg, w.kend, w.slab});
    size_t want_ranges = 0;
    for (size_t q = 0; q < probs.size(); ++q) want_ranges += (size_t)((probs[q].nq + 63) / 64) * tn;
    bool ok = ranges.size() == want_ranges;
    int most = 0;
    for (auto& kv : ranges) {
        auto v = kv.second;
        std::sort(v.begin(), v.end());
        const int prob = std::get<0>(kv.first), mt = std::get<1>(kv.first), nt = std::get<2>(kv.first);
        int at = 0;
        for (size_t j = 0; j < v.size(); ++j) {
            ok = ok && std::get<0>(v[j]) == at && std::get<1>(v[j]) > at && std::get<2>(v[j]) == (int)j;
            at = std::get<1>(v[j]);
        }
        // row tile mt reads k < k_off + (one past its last row), rounded up to a stage, within the padded row
        const int want = std::min((probs[prob].k_off + tape_tile_hi(probs[prob].nq, mt, 64) + 31) / 32, probs[prob].nq_pad / 32) * 32;
        ok = ok && at == want;
        ok = ok && T.seg_count[(size_t)(T.tile_off[prob] + mt) * tn + nt] == (int32_t)v.size();
        most = std::max(most, (int)v.size());
    }
    ok = ok && most == T.max_segs;
    expect(ok, (std::string("segments of ") + label).c_str());
}

int main()
{
    // (n_masked, nq): the small awkward grids of tests/test_quad_root_gpu.py - k_off = 0, k_off no multiple of 32, fewer than 64
    // rows, n_masked mod 64 = 1 and 63, nq mod 64 odd and even, a joint problem - and the bench's joint fit
    const std::vector<std::vector<Shape>> shapes = {
        {{65, 65}}, {{44, 65}}, {{959, 1296}}, {{1243, 1299}}, {{59, 63}, {1312, 1320}}, {{1256, 5184}},
        {{1590, 2512}, {3180, 5000}},
    };
    const int batches[] = {9, 64, 65, 129, 256};
    const int block_counts[] = {512, 608, 200, 8};
    const double entry = 2.5, skew = 0.12;
    int cases = 0;
    for (auto& sh : shapes)
        for (int B : batches)
            for (int blocks : block_counts) {
                std::vector<TapeProblem> probs;
                for (auto& s : sh) probs.push_back({s.rows, pad32(s.cols), s.cols - s.rows});
                const int tn = (B + 63) / 64;
                for (bool bands : {false, true}) {
                    const Tape T = plan_quad_tape(probs, tn, blocks, entry, skew, 64, 32, bands, true);
                    const std::string why = check_quad_tape(T, probs, tn, entry, skew);
                    char label[200];
                    std::snprintf(label, sizeof label, "root tape rows0=%d cols0=%d items=%zu B=%d blocks=%d bands=%d: %s", sh[0].rows, sh[0].cols,
                                  sh.size(), B, blocks, (int)bands, why.c_str());
                    expect(why.empty(), label);
                    segments(T, probs, tn, label);
                    const Tape again = plan_quad_tape(probs, tn, blocks, entry, skew, 64, 32, bands, true);
                    expect(T.work.size() == again.work.size() && T.queue == again.queue && T.seg_count == again.seg_count &&
                           (T.work.empty() || std::memcmp(T.work.data(), again.work.data(), T.work.size() * sizeof(GemmWork)) == 0),
                           "identical inputs give identical root tapes");
                    if (!bands) {
                        std::printf("ok root tape rows0=%d cols0=%d items=%zu B=%d blocks=%d: %zu entries, at most %d segments a range, cap %.1f\n",
                                    sh[0].rows, sh[0].cols, sh.size(), B, blocks, T.work.size(), T.max_segs, T.capacity);
                        ++cases;
                    }
                }
            }
    // the bench's shapes at B = 256 on 512 blocks: the stage counts the trapezoid was proposed with, and its advantage
    {
        const std::vector<TapeProblem> root = {{1590, 2528, 2512 - 1590}, {3180, 5024, 5000 - 3180}}, tri = {{2512, 2528}, {5000, 5024}};
        int64_t sr = 0, st = 0;
        for (auto& p : root) for (int mt = 0; mt < (p.nq + 63) / 64; ++mt) sr += tape_tile_stages(p, mt, 64, 32);
        for (auto& p : tri) for (int mt = 0; mt < (p.nq + 63) / 64; ++mt) st += tape_tile_stages(p, mt, 64, 32);
        std::printf("bench stages per group of walker tiles: root %lld, triangle %lld\n", (long long)sr, (long long)st);
        expect(st == 7841 && sr < st && sr * 100 < st * 88, "the bench's root tape has at least 12 % fewer K stages than its triangle");
        const Tape R = plan_quad_tape(root, 4, 512, entry, skew, 64, 32, true, true);
        expect(R.max_segs >= 1 && R.max_segs <= 8, "the bench's ranges are cut into a handful of segments at most");
    }
    // k_off = 0 with rows = nq: today's tape, entry for entry - with or without the segment bookkeeping (which numbers the slabs only)
    for (auto& sh : std::vector<std::vector<int>>{{2512, 5000}, {2512}, {70}, {64}, {65, 1}, {3180, 1590, 2500, 5000}})
        for (int B : batches)
            for (int blocks : block_counts) {
                std::vector<TapeProblem> plain, zero;
                for (int n : sh) { plain.push_back({n, pad32(n)}); zero.push_back({n, pad32(n), 0}); }
                const int tn = (B + 63) / 64;
                const Tape a = plan_quad_tape(plain, tn, blocks, 4.0, skew, 64, 32, true);
                const Tape b = plan_quad_tape(zero, tn, blocks, 4.0, skew, 64, 32, true, false);
                Tape c = plan_quad_tape(zero, tn, blocks, 4.0, skew, 64, 32, true, true);
                expect(a.work.size() == b.work.size() && a.queue == b.queue && a.nt_off == b.nt_off && a.piece_at == b.piece_at &&
                       (a.work.empty() || std::memcmp(a.work.data(), b.work.data(), a.work.size() * sizeof(GemmWork)) == 0),
                       "k_off = 0 reproduces the triangle's tape byte for byte");
                expect(check_quad_tape(c, zero, tn, 4.0, skew).empty(), "k_off = 0 with segments passes the tape's invariants");
                for (auto& w : c.work) w.slab = 0;
                expect(a.work.size() == c.work.size() && a.queue == c.queue && a.nt_off == c.nt_off &&
                       (a.work.empty() || std::memcmp(a.work.data(), c.work.data(), a.work.size() * sizeof(GemmWork)) == 0),
                       "the segment bookkeeping changes the slab indices only");
            }
    std::printf("root cases %d\n", cases);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all root planner checks passed\n");
    return 0;
}
