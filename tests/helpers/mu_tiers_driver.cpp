// CPU driver of the mu node rules' host code (vega_amd/csrc/vmx_plan.h: mu_rule_extra, build_mu_tiers, mu_tier_of,
// plan_mu_tiles, mu_mean_nodes), built by tests/test_mu_tiers.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// and run without a GPU: "FAIL ..." lines and a non-zero exit code when an invariant breaks; the node lists and the tile
// plans are printed for the test to compare with vega_amd/mu_quadrature.py.
#include <cstdio>
#include <cstring>

#include "../../vega_amd/csrc/vmx_plan.h"

using namespace vmx_plan;

static int failures = 0;
static void expect(bool ok, const char* what)
{
    if (!ok) { std::printf("FAIL %s\n", what); ++failures; }
}

// the logarithmic grid of the test (tests/test_mu_tiers.py generates the same one)
static std::vector<double> log_grid(int nk, double k0, double dlnk)
{
    std::vector<double> k(nk);
    for (int i = 0; i < nk; ++i) k[i] = k0 * std::exp(dlnk * i);
    return k;
}

static void check_plan(const std::vector<double>& k, int kt, double k_node_max, int n_tiers, const char* tag)
{
    const int nk = (int)k.size(), n_tiles = (nk + kt - 1) / kt;
    const std::vector<uint16_t> z = plan_mu_tiles(k.data(), nk, kt, k_node_max, n_tiers, 256);
    char what[160];
    std::snprintf(what, sizeof what, "%s kt=%d tiers=%d", tag, kt, n_tiers);
    expect((int)z.size() == n_tiles, what);
    if ((int)z.size() != n_tiles) return;
    std::vector<int> seen(n_tiles, 0);
    int last_class = -1, last_tile = -1;
    std::printf("plan %s:", what);
    for (int i = 0; i < n_tiles; ++i) {
        const int tile = z[i] & 0xfff, tier = z[i] >> 12;
        expect(tile < n_tiles && tier < n_tiers, "zmap entry in range");
        if (tile >= n_tiles) return;
        ++seen[tile];
        const double k_end = k[std::min((tile + 1) * kt, nk) - 1];
        expect(tier == mu_tier_of(k_end, n_tiers), "tier of the tile");
        expect(tier == 0 || k_end <= mu_tier_rules()[tier].k_max, "tier within its k_max");
        const int cls = k[tile * kt] > k_node_max ? MU_TIERS : tier;
        expect(cls > last_class || (cls == last_class && tile > last_tile), "classes in order, ascending k within");
        last_class = cls; last_tile = tile;
        std::printf(" %d/%d", tile, tier);
    }
    std::printf("\n");
    for (int t = 0; t < n_tiles; ++t) expect(seen[t] == 1, "every tile once");
}

int main()
{
    // the node lists: the main rule alone and with the tiers behind it
    std::vector<double> mu1, w1, mu3, w3;
    MuTierDesc d1[MU_TIERS], d3[MU_TIERS];
    build_mu_tiers(1000, 1, mu1, w1, d1);
    build_mu_tiers(1000, MU_TIERS, mu3, w3, d3);
    expect(mu1.size() == 82 && w1.size() == 82 && mu3.size() == 82 + 50 + 34 && w3.size() == mu3.size(), "node counts");
    expect(std::memcmp(mu1.data(), mu3.data(), 82 * sizeof(double)) == 0 && std::memcmp(w1.data(), w3.data(), 82 * sizeof(double)) == 0,
           "the main rule is unchanged by the tiers");
    const int want[MU_TIERS][4] = {{48, 48, 0, 82}, {16, 16, 82, 50}, {4, 4, 132, 34}};
    for (int t = 0; t < MU_TIERS; ++t) {
        expect(d3[t].lo == want[t][0] && d3[t].hi == want[t][1] && d3[t].x_off == want[t][2] && d3[t].x_cnt == want[t][3], "tier descriptor");
        expect(d1[t].lo == 48 && d1[t].hi == 48 && d1[t].x_off == 0 && d1[t].x_cnt == 82, "descriptors without tiers: the main rule");
        expect(d3[t].x_off + d3[t].x_cnt <= (int)mu3.size(), "tier nodes inside the list");
        // the weights reproduce the 1000-point midpoint sums of mu^p
        const int powers[4] = {0, 2, 8, 14};
        for (int p : powers) {
            long double ref = 0.0L, got = 0.0L;
            for (int j = 0; j < 1000; ++j) {
                const long double m = (j + 0.5L) / 1000.0L, v = std::pow(m, (long double)p);
                ref += v;
                if (j < d3[t].lo || j >= 1000 - d3[t].hi) got += v;
            }
            for (int j = 0; j < d3[t].x_cnt; ++j) got += (long double)w3[d3[t].x_off + j] * std::pow((long double)mu3[d3[t].x_off + j], (long double)p);
            const double rel = (double)std::fabs((got - ref) / ref);
            std::printf("moment tier %d p %d rel %.3g\n", t, p, rel);
            expect(rel <= 2e-14, "midpoint sum of mu^p");
        }
        for (int j = 0; j < d3[t].x_cnt; ++j) {
            const double m = mu3[d3[t].x_off + j];
            expect(m > 0.0 && m <= 1.0, "node in (0, 1]");
            std::printf("node %d %d %.17g %.17g\n", t, j, m, w3[d3[t].x_off + j]);
        }
    }
    // tiers of a tile
    expect(mu_tier_of(1e-4, MU_TIERS) == 2 && mu_tier_of(0.0058, MU_TIERS) == 2 && mu_tier_of(0.0059, MU_TIERS) == 1, "42-node tier up to its k_max");
    expect(mu_tier_of(0.11, MU_TIERS) == 1 && mu_tier_of(0.111, MU_TIERS) == 0 && mu_tier_of(50.0, MU_TIERS) == 0, "82-node tier up to its k_max");
    expect(mu_tier_of(1e-4, 1) == 0 && mu_tier_of(1e-4, 2) == 1, "fewer tiers");
    // launch plans: the joint fit's grid shape (814 wavenumbers), short and ragged grids, one tile
    const std::vector<double> grid = log_grid(814, 1e-4, 0.02);
    for (int kt : {64, 16}) {
        for (int n_tiers = 1; n_tiers <= MU_TIERS; ++n_tiers) check_plan(grid, kt, 6.0, n_tiers, "grid814");
        check_plan(grid, kt, 0.0, MU_TIERS, "rule-off");
        check_plan(log_grid(65, 1e-3, 0.1), kt, 6.0, MU_TIERS, "grid65");
        check_plan(log_grid(9, 1e-3, 0.5), kt, 6.0, MU_TIERS, "grid9");
    }
    {
        const std::vector<uint16_t> z = plan_mu_tiles(grid.data(), 814, 64, 0.0, MU_TIERS, 256);
        bool identity = z.size() == 13;
        for (size_t i = 0; i < z.size(); ++i) identity = identity && (z[i] & 0xfff) == (int)i;
        expect(identity, "rule off: plain order");
        expect(plan_mu_tiles(grid.data(), 814, 16, 6.0, MU_TIERS, 50).empty(), "more tiles than entries: no plan");
        expect(plan_mu_tiles(grid.data(), 814, 16, 6.0, MU_TIERS, 51).size() == 51, "exactly as many tiles as entries");
        const std::vector<double> big = log_grid(5000, 1e-4, 0.003);
        expect(plan_mu_tiles(big.data(), 5000, 1, 6.0, MU_TIERS, 100000).empty(), "more tiles than 12 bits: no plan");
    }
    // the statistic: mean nodes per wavenumber on the rule
    expect(mu_mean_nodes(grid.data(), 814, 64, 0, MU_TIERS, d3) == 178.0, "nothing on the rule: the main rule's count");
    expect(mu_mean_nodes(grid.data(), 814, 64, 576, 1, d1) == 178.0, "without tiers: exactly the main rule's count");
    expect(mu_mean_nodes(grid.data(), 814, 0, 576, MU_TIERS, d3) == 178.0, "no tile width: the main rule's count");
    {
        double sum = 0.0;
        for (int i = 0; i < 576; ++i) { const MuTierDesc& d = d3[mu_tier_of(grid[std::min((i / 64 + 1) * 64, 814) - 1], MU_TIERS)]; sum += d.lo + d.hi + d.x_cnt; }
        const double mean = mu_mean_nodes(grid.data(), 814, 64, 576, MU_TIERS, d3);
        std::printf("mean nodes %.6f\n", mean);
        expect(mean == sum / 576 && mean < 178.0 && mean > 42.0, "mean nodes with tiers");
        expect(mu_mean_nodes(grid.data(), 814, 16, 100000, MU_TIERS, d3) < 178.0, "k_on_rule clipped to the grid");
    }
    if (failures == 0) std::printf("all mu tier checks passed\n");
    return failures ? 1 : 0;
}
