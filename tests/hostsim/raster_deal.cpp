// Host build of the deal of k_raster's runs (drt_amd/csrc/drt_raster.h: raster_deal_boundary, raster_deal_end, raster_deal_slice), for
// tests/test_raster_deal_host.py.  g++ -O2 -std=c++17 -fPIC -shared; with -DRASTER_DEAL_MAIN a program of its own that runs a fixed set of
// cases (the sanitizer build of the test).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../drt_amd/csrc/drt_raster.h"

using namespace drt;

extern "C" {

// B[0 .. V] as (run, item) pairs from the costs, by the definition: inclusive prefix sums, then one bisection per boundary.
void rd_boundaries(const uint32_t* cost, uint32_t n_runs, uint32_t n_waves, uint32_t c_fixed, uint32_t* out) {
    std::vector<uint64_t> prefix(n_runs);
    uint64_t acc = 0;
    for (uint32_t r = 0; r < n_runs; ++r) { acc += raster_deal_weight(cost[r], c_fixed); prefix[r] = acc; }
    for (uint32_t v = 0; v <= n_waves; ++v) {
        const DealPos b = raster_deal_boundary(prefix.data(), n_runs, n_waves, v, c_fixed);
        out[2 * v] = b.run; out[2 * v + 1] = b.item;
    }
}

// The same table the way k_raster_deal writes it: every run places the boundaries that fall into it.  Entries no run claims keep 0xFFFFFFFF.
void rd_boundaries_by_run(const uint32_t* cost, uint32_t n_runs, uint32_t n_waves, uint32_t c_fixed, uint32_t* out) {
    for (uint32_t k = 0; k < 2 * (n_waves + 1); ++k) out[k] = 0xFFFFFFFFu;
    uint64_t total = 0, before = 0;
    for (uint32_t r = 0; r < n_runs; ++r) total += raster_deal_weight(cost[r], c_fixed);
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint64_t with = before + raster_deal_weight(cost[r], c_fixed);
        raster_deal_place(reinterpret_cast<DealPos*>(out), r, before, with, total, n_waves, c_fixed);      // (the call k_raster_deal's thread of run r makes)
        before = with;
    }
    out[2 * n_waves] = n_runs; out[2 * n_waves + 1] = 0;
    if (n_runs == 0) for (uint32_t k = 0; k < 2 * n_waves; ++k) out[k] = 0;
}

// Every wave's loop as k_raster<true> runs it, against the ACTUAL totals of the runs: owners[r] counts the waves that own run r;
// next[r] ends as the item up to which run r was worked, every non-empty slice having started where the one before it ended (the
// return value counts those that did not: gaps and overlaps); wave_cost[v] = sum over the runs the wave visits of c_fixed + its items.
int64_t rd_replay(const uint32_t* B, uint32_t n_runs, uint32_t n_waves, const uint32_t* actual, uint32_t c_fixed, int32_t* owners, uint32_t* next, uint64_t* wave_cost) {
    int64_t bad = 0;
    for (uint32_t r = 0; r < n_runs; ++r) { owners[r] = 0; next[r] = 0; }
    for (uint32_t v = 0; v < n_waves; ++v) {
        const DealPos b0 = v == 0 ? DealPos{0, 0} : raster_deal_clamp(DealPos{B[2 * v], B[2 * v + 1]}, n_runs);
        const DealPos b1 = v + 1 >= n_waves ? DealPos{n_runs, 0} : raster_deal_clamp(DealPos{B[2 * v + 2], B[2 * v + 3]}, n_runs);
        DealRange g = raster_deal_range(b0, b1);
        if (g.end > n_runs) g.end = n_runs;
        uint64_t c = 0;
        for (; g.run < g.end; raster_deal_next(g)) {
            const uint32_t r = g.run;
            const DealSlice sl = raster_deal_slice(g), by_rule = raster_deal_slice(b0, b1, r);
            if (sl.lo != by_rule.lo || sl.hi != by_rule.hi || sl.owner != by_rule.owner) ++bad;      // the walk gives the rule's slices
            owners[r] += sl.owner ? 1 : 0;
            const uint32_t total = actual[r], stop = total < sl.hi ? total : sl.hi;
            c += c_fixed;
            if (sl.lo >= stop) continue;
            if (sl.lo != next[r]) ++bad;
            next[r] = stop;
            c += stop - sl.lo;
        }
        wave_cost[v] = c;
    }
    return bad;
}

}  // extern "C"

#ifdef RASTER_DEAL_MAIN
static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static int one(const std::vector<uint32_t>& cost, uint32_t V, uint32_t c_fixed, uint64_t& seed) {
    const uint32_t n = (uint32_t)cost.size();
    std::vector<uint32_t> B(2 * (V + 1)), next(n), actual(cost);
    std::vector<int32_t> owners(n);
    std::vector<uint64_t> wc(V);
    rd_boundaries(cost.data(), n, V, c_fixed, B.data());
    std::vector<uint32_t> B2(B.size());
    rd_boundaries_by_run(cost.data(), n, V, c_fixed, B2.data());
    int fails = B != B2;
    for (int variant = 0; variant < 3; ++variant) {
        if (variant == 1) for (auto& a : actual) a = a / 2;
        if (variant == 2) for (auto& a : actual) a = rnd(seed) % 4 == 0 ? 0 : rnd(seed) % 5000;
        fails += rd_replay(B.data(), n, V, actual.data(), c_fixed, owners.data(), next.data(), wc.data()) != 0;
        for (uint32_t r = 0; r < n; ++r) fails += owners[r] != 1 || next[r] != actual[r];
    }
    return fails;
}

int main() {
    uint64_t seed = 12345;
    int fails = 0;
    for (uint32_t V : {1u, 7u, 64u, 8192u})
        for (uint32_t n : {0u, 1u, V - 1, V, V + 1, 4 * V}) {
            std::vector<uint32_t> random(n), zeros(n, 0u), giant(n, 0u), huge(n);
            for (auto& c : random) c = rnd(seed) % 2 ? 0 : rnd(seed) % 3073;
            if (n) giant[n / 3] = 3072;
            for (auto& c : huge) c = (uint32_t)((0xFFFFFFFFull / (n ? n : 1)) - rnd(seed) % 3);
            for (const auto* c : {&random, &zeros, &giant, &huge}) fails += one(*c, V, kRasterDealFixed, seed);
        }
    std::printf("raster_deal: %d failures\n", fails);
    return fails ? 1 : 0;
}
#endif
