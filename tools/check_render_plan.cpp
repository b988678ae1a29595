// check_render_plan: the batch plan of a render call (csrc/render_plan.h) on
// the CPU.  Sweeps rectangles, sample counts, tile deals, key lists, lane
// counts and path budgets and checks for every plan that
//   (a) every (virtual tile, sample) pair lies in exactly one batch,
//   (b) a batch never exceeds a lane's share of the path budget,
//   (c) the planned tile groups are a multiple of the lane count, or one per tile,
//   (d) the single-lane modes and calls of fewer than two tiles take one lane,
//   (e) a batch's fan (direct / ao: `fan` rays per path slot) is nslots * fan
//       and stays within PLAN_MAX_RAYS, whatever the path budget,
// then a few literal plans worked out by hand from the formulas (README's "C5
// in three batches" among them).  `make` builds it with ASan + UBSan;
// tests/test_render_plan.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../my-mitsuba_amd/csrc/render_plan.h"

namespace {

long g_plans = 0, g_fewer = 0;

struct Case {
    int w, h;
    uint32_t spp;
    int stride, offset;
    uint32_t keys, maxPaths, lanes;
    bool single;
    uint32_t fan = 1;
};

[[noreturn]] void fail(const Case &c, const char *what) {
    fprintf(stderr, "check_render_plan: FAILED %s at %dx%d spp %u stride %d offset %d keys %u maxPaths %u lanes %u single %d fan %u\n", what,
            c.w, c.h, c.spp, c.stride, c.offset, c.keys, c.maxPaths, c.lanes, (int)c.single, c.fan);
    exit(1);
}
#define CHECK(c, cond) do { if (!(cond)) fail(c, #cond); } while (0)

RenderPlan plan_of(const Case &c) {
    return plan_render(c.w, c.h, c.spp, c.stride, c.offset, c.keys, c.maxPaths, c.lanes, c.single, c.fan);
}

// the invariants (a)-(d) of one plan
RenderPlan check(const Case &c) {
    const RenderPlan R = plan_of(c);
    ++g_plans;
    // the header of the plan against the definitions
    const uint32_t tx = ((uint32_t)c.w + 15) / 16, ty = ((uint32_t)c.h + 15) / 16;
    CHECK(c, R.tilesX == tx && R.allTiles == tx * ty);
    CHECK(c, R.tstride == (c.stride > 1 ? (uint32_t)c.stride : 1u) && R.toffset == (c.stride > 1 ? (uint32_t)c.offset : 0u));
    uint32_t dealt = 0;
    for (uint32_t k = R.toffset; k < R.allTiles; k += R.tstride) ++dealt;
    CHECK(c, R.ntiles == (c.keys ? c.keys : dealt));
    // (d)
    CHECK(c, R.lanes == ((c.single || R.ntiles < 2) ? 1u : c.lanes));
    // (b)
    const uint64_t lanePaths = std::max<uint64_t>(256, std::min<uint64_t>(c.maxPaths / R.lanes, (1ull << 31) / c.fan));
    CHECK(c, R.fan == c.fan);
    CHECK(c, R.sppPerBatch >= 1 && R.tilesPerBatch >= 1);
    CHECK(c, (uint64_t)R.tilesPerBatch * R.sppPerBatch * 256 <= lanePaths);
    // (a), and the order: tile-major, then sample-major
    std::vector<unsigned char> seen((size_t)R.ntiles * c.spp, 0);
    uint32_t groups = 0;
    for (size_t i = 0; i < R.batches.size(); ++i) {
        const PlanBatch &B = R.batches[i];
        CHECK(c, B.ntiles >= 1 && B.ns >= 1 && (uint64_t)B.tile0 + B.ntiles <= R.ntiles && (uint64_t)B.s0 + B.ns <= c.spp);
        CHECK(c, B.ntiles <= R.tilesPerBatch && B.ns <= R.sppPerBatch);
        CHECK(c, (uint64_t)B.nslots == (uint64_t)B.ntiles * B.ns * 256 && B.nslots <= lanePaths);
        // (e)
        CHECK(c, (uint64_t)B.nrays == (uint64_t)B.nslots * c.fan && (uint64_t)B.nslots * c.fan <= (1ull << 31));
        if (B.s0 == 0) ++groups;
        if (i) {
            const PlanBatch &A = R.batches[i - 1];
            CHECK(c, B.tile0 > A.tile0 || (B.tile0 == A.tile0 && B.s0 > A.s0));
        }
        for (uint32_t t = B.tile0; t < B.tile0 + B.ntiles; ++t)
            for (uint32_t s = B.s0; s < B.s0 + B.ns; ++s) CHECK(c, seen[(size_t)t * c.spp + s]++ == 0);
    }
    for (unsigned char v : seen) CHECK(c, v == 1);
    // (c): the planned groups; rounding tilesPerBatch up can leave fewer in the list
    CHECK(c, R.tileGroups % R.lanes == 0 || R.tileGroups == R.ntiles);
    CHECK(c, groups <= R.tileGroups && groups == (R.ntiles + R.tilesPerBatch - 1) / R.tilesPerBatch);
    if (groups < R.tileGroups) ++g_fewer;
    return R;
}

void sweep() {
    const int rects[][2] = {{1, 1}, {15, 9}, {16, 16}, {17, 16}, {32, 16}, {33, 31}, {64, 48}, {100, 40}, {199, 113}, {200, 120}};
    const uint32_t spps[] = {1, 2, 7, 64, 100, 256, 300};
    const uint32_t paths[] = {256, 300, 1000, 4096, 65536, 1u << 20, 771000000u, 3u << 28};
    for (auto &r : rects)
        for (uint32_t spp : spps)
            for (uint32_t mp : paths)
                for (uint32_t lanes = 1; lanes <= 4; ++lanes)
                    for (int single = 0; single < 2; ++single) {
                        for (int stride = 0; stride <= 5; ++stride)
                            for (int offset = 0; offset < std::max(1, stride); ++offset)
                                check(Case{r[0], r[1], spp, stride, offset, 0, mp, lanes, single != 0});
                        for (uint32_t keys : {1u, 2u, 7u}) check(Case{r[0], r[1], spp, 0, 0, keys, mp, lanes, single != 0});
                    }
    // the fan of direct / ao renders (one lane): 2 = (1,1), 8 = (4,4), an odd
    // one, one that caps the default budget, and the largest
    for (auto &r : rects)
        for (uint32_t spp : spps)
            for (uint32_t mp : paths)
                for (uint32_t fan : {2u, 8u, 13u, 1000u, PLAN_MAX_FAN}) {
                    for (int stride = 0; stride <= 3; ++stride)
                        for (int offset = 0; offset < std::max(1, stride); ++offset)
                            check(Case{r[0], r[1], spp, stride, offset, 0, mp, 1, true, fan});
                    check(Case{r[0], r[1], spp, 0, 0, 7, mp, 1, true, fan});
                }
}

void literals() {
    const uint32_t dflt = 3u << 28;
    {   // 1280x720, 256 spp: one batch
        const Case c{1280, 720, 256, 0, 0, 0, dflt, 1, false};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 3600 && R.batches.size() == 1 && R.batches[0].nslots == 235929600u);
    }
    {   // 1920x1080, 1024 spp in 3/4 of 288 GB: "C5 in three batches"
        const Case c{1920, 1080, 1024, 0, 0, 0, 771000000u, 1, false};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 8160 && R.batches.size() == 3);
        for (const PlanBatch &B : R.batches) CHECK(c, B.ntiles == 2720 && B.ns == 1024 && B.nslots == 713031680u);
    }
    {   // three lanes over a small budget: the sample batches alternate 5 and 3
        const Case c{64, 48, 8, 0, 0, 0, 4096, 3, false};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 12 && R.lanes == 3 && R.sppPerBatch == 5 && R.tilesPerBatch == 1 && R.batches.size() == 24);
        for (size_t i = 0; i < R.batches.size(); ++i) CHECK(c, R.batches[i].nslots == ((i & 1) ? 768u : 1280u));
    }
    {   // one tile: one lane, whatever was asked for
        const Case c{16, 16, 100, 0, 0, 0, 2048, 4, false};
        const RenderPlan R = check(c);
        CHECK(c, R.lanes == 1 && R.sppPerBatch == 8 && R.batches.size() == 13 && R.batches.back().ns == 4);
    }
    {   // a third of the deal
        const Case c{100, 40, 4, 3, 1, 0, dflt, 1, false};
        const RenderPlan R = check(c);
        CHECK(c, R.tilesX == 7 && R.allTiles == 21 && R.ntiles == 7 && R.batches.size() == 1 && R.batches[0].nslots == 7168);
    }
    {   // direct (4,4) at 1280x720, 64 spp: 8 rays per slot cap a batch at 2^28 slots, so one batch still
        const Case c{1280, 720, 64, 0, 0, 0, dflt, 1, true, 8};
        const RenderPlan R = check(c);
        CHECK(c, R.batches.size() == 1 && R.batches[0].nslots == 58982400u && R.batches[0].nrays == 471859200u);
    }
    {   // a fan of 1000 over 200x120, 64 spp: 2^31 / 1000 = 2147483 slots per batch hold 131 tiles of 64 samples
        const Case c{200, 120, 64, 0, 0, 0, dflt, 1, true, 1000};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 104 && R.sppPerBatch == 64 && R.tilesPerBatch == 104 && R.batches.size() == 1);
    }
    {   // the same at 640x480: 1200 tiles in ten groups of 120
        const Case c{640, 480, 64, 0, 0, 0, dflt, 1, true, 1000};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 1200 && R.tilesPerBatch == 120 && R.batches.size() == 10 && R.batches[0].nrays == 1966080000u);
    }
    {   // two tiles keep the lanes asked for; the groups stop at one per tile
        const Case c{32, 16, 1, 0, 0, 0, dflt, 4, false};
        const RenderPlan R = check(c);
        CHECK(c, R.ntiles == 2 && R.lanes == 4 && R.batches.size() == 2 && R.batches[0].ntiles == 1 && R.batches[1].ntiles == 1);
    }
}

}  // namespace

int main() {
    sweep();
    literals();
    printf("check_render_plan: %ld plans ok (%ld list fewer tile groups than planned)\n", g_plans, g_fewer);
    return 0;
}
