// check_adaptive_plan: the round bookkeeping of an adaptive render
// (csrc/adaptive_plan.h) on the CPU.  Sweeps base counts, sample factors, round
// sizes, rectangles, active-tile counts and path budgets and checks that
//   (a) the rounds of a render cover samples [0, cap) once, in order, round 0
//       covering min(N, cap), and that no round follows the cap,
//   (b) the batches of a round cover every (listed tile, sample of the round)
//       pair once, tile-major then sample-major, so a tile's batches follow
//       each other in sample order (the splat walks a pixel's samples in order),
//   (c) a simulated render, in which every pixel stops at a count of its own,
//       ends with no active tile, every pixel's samples taken exactly up to its
//       count's round, and the compaction keeping the key order,
//   (d) the pre-pass strip's sample ids lie past the film's and fit an int row,
// then a few literal cases.  `make` builds it with ASan + UBSan;
// tests/test_adaptive_scene.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../my-mitsuba_amd/csrc/adaptive_plan.h"

namespace {

long g_rounds = 0, g_plans = 0, g_renders = 0;

[[noreturn]] void fail(const char *what, uint32_t N, int factor, uint32_t later, int w, int h, uint32_t mp) {
    fprintf(stderr, "check_adaptive_plan: FAILED %s at N %u factor %d later %u rect %dx%d maxPaths %u\n", what, N, factor, later, w, h, mp);
    exit(1);
}
#define CHECK(cond) do { if (!(cond)) fail(#cond, N, factor, later, w, h, mp); } while (0)

// (a)
void check_rounds(uint32_t N, int factor, uint32_t later) {
    const int w = 0, h = 0;
    const uint32_t mp = 0;
    const uint32_t cap = adaptive_cap(factor, N);
    CHECK(cap >= 1 && (factor <= 0 ? cap == 1 : cap == (uint32_t)factor * N));
    uint32_t next = 0, s0, ns, r = 0;
    for (; adaptive_round(N, cap, later, r, s0, ns); ++r) {
        CHECK(s0 == next && ns >= 1 && s0 + ns <= cap);
        if (r == 0) CHECK(ns == std::min(N, cap));
        else CHECK(ns <= (later ? later : N));
        next = s0 + ns;
        ++g_rounds;
        CHECK(r < (1u << 25));
    }
    CHECK(next == cap && r >= 1);
    CHECK(!adaptive_round(N, cap, later, r + 1, s0, ns));
}

// (b), (c)
void check_render(uint32_t N, int factor, uint32_t later, int w, int h, uint32_t mp, uint32_t seed) {
    const uint32_t cap = adaptive_cap(factor, N);
    const RenderPlan all = plan_render(w, h, 1u, 1, 0, 0, PLAN_TILE_SLOTS, 1u, true);
    std::vector<int32_t> keys(all.ntiles);
    for (uint32_t v = 0; v < all.ntiles; ++v) keys[v] = (int32_t)v;
    // every tile's pixels stop at counts of their own in [min(N, cap), cap]; the
    // tile stays active until its last one has
    std::vector<uint32_t> stopAt(all.allTiles), taken(all.allTiles, 0u), active(all.allTiles, 0u);
    uint32_t x = seed * 2654435761u + 12345u;
    const uint32_t first = std::min(N, cap);
    for (uint32_t &v : stopAt) {
        x = x * 1664525u + 1013904223u;
        v = first + (cap > first ? (x >> 8) % (cap - first + 1) : 0u);
    }
    std::vector<int32_t> finished;
    uint32_t s0, ns;
    for (uint32_t r = 0; !keys.empty(); ++r) {
        CHECK(adaptive_round(N, cap, later, r, s0, ns));
        const RenderPlan R = adaptive_round_plan(w, h, (uint32_t)keys.size(), s0, ns, mp);
        ++g_plans;
        CHECK(R.lanes == 1 && R.ntiles == keys.size());
        std::vector<uint32_t> next(keys.size(), s0);
        for (size_t i = 0; i < R.batches.size(); ++i) {
            const PlanBatch &B = R.batches[i];
            CHECK(B.ntiles >= 1 && B.ns >= 1 && (uint64_t)B.tile0 + B.ntiles <= keys.size());
            CHECK(B.s0 >= s0 && B.s0 + B.ns <= s0 + ns);
            CHECK((uint64_t)B.nslots == (uint64_t)B.ntiles * B.ns * 256 && B.nslots <= std::max<uint32_t>(256u, mp));
            for (uint32_t t = B.tile0; t < B.tile0 + B.ntiles; ++t) {
                CHECK(next[t] == B.s0);   // the tile's batches in sample order, none skipped
                next[t] = B.s0 + B.ns;
                const uint32_t key = (uint32_t)keys[t];
                // a tile that stopped in an earlier batch of this round is still
                // listed until the round ends: its pixels are dead there
                if (taken[key] == stopAt[key] && B.s0 > s0) continue;
                CHECK(taken[key] == B.s0);
                taken[key] = std::min(stopAt[key], B.s0 + B.ns);   // the samples after the stop are dropped
                active[key] = taken[key] < stopAt[key] ? 1u : 0u;
            }
        }
        for (uint32_t v : next) CHECK(v == s0 + ns);
        const std::vector<int32_t> before = keys;
        const uint32_t kept = adaptive_compact(keys, active, finished);
        CHECK(kept == keys.size() && kept + finished.size() == before.size());
        size_t a = 0, f = 0;
        for (int32_t k : before) {   // the order is kept on both sides
            if (active[(size_t)k]) CHECK(a < keys.size() && keys[a++] == k);
            else CHECK(f < finished.size() && finished[f++] == k);
        }
    }
    for (uint32_t k = 0; k < all.allTiles; ++k) CHECK(taken[k] == stopAt[k] && !active[k]);
    ++g_renders;
}

// (d)
void check_prepass(uint64_t filmPixels, uint32_t cap, bool expect) {
    const uint32_t N = 0, later = 0, mp = 0;
    const int factor = 0, w = (int)filmPixels, h = (int)cap;
    int32_t row0 = -1, rows = -1;
    const bool ok = adaptive_prepass_rows(filmPixels, cap, row0, rows);
    CHECK(ok == expect);
    if (!ok) return;
    CHECK(rows == 625 && (uint64_t)rows * 16 >= ADAPTIVE_PREPASS_SAMPLES);
    CHECK((uint64_t)row0 * 16 >= filmPixels * cap && (uint64_t)(row0 - 1) * 16 < filmPixels * cap + 16);
    CHECK((uint64_t)row0 + rows + 16 <= (uint64_t)INT32_MAX);
}

}  // namespace

int main() {
    for (uint32_t N : {8u, 9u, 16u, 64u, 100u})
        for (int factor : {0, 1, 2, 3, 32, 1000})
            for (uint32_t later : {0u, 1u, 3u, 8u, 64u, 1000u, 65536u, 100000u}) check_rounds(N, factor, later);
    const int rects[][2] = {{1, 1}, {16, 16}, {17, 16}, {40, 24}, {100, 40}};
    uint32_t seed = 1;
    for (uint32_t N : {8u, 13u})
        for (int factor : {0, 1, 2, 5})
            for (uint32_t later : {0u, 1u, 5u, 64u})
                for (auto &r : rects)
                    for (uint32_t mp : {256u, 1000u, 4096u, 1u << 20, 3u << 28}) check_render(N, factor, later, r[0], r[1], mp, seed++);
    check_prepass(40 * 24, 32, true);
    check_prepass(1280ull * 720, 2048, true);
    check_prepass(1ull << 28, 1u << 24, false);   // 2^52 ids: no int row holds them
    {   // the literal case of the GPU tests: N 8, factor 4, default rounds
        uint32_t s0, ns;
        if (!(adaptive_cap(4, 8) == 32 && adaptive_round(8, 32, 0, 3, s0, ns) && s0 == 24 && ns == 8 && !adaptive_round(8, 32, 0, 4, s0, ns) &&
              adaptive_round(8, 32, 5, 5, s0, ns) && s0 == 28 && ns == 4)) {
            fprintf(stderr, "check_adaptive_plan: FAILED literal rounds\n");
            return 1;
        }
    }
    printf("check_adaptive_plan: %ld rounds, %ld round plans, %ld simulated renders ok\n", g_rounds, g_plans, g_renders);
    return 0;
}
