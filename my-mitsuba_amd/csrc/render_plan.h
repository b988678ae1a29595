// render_plan.h -- how a render call is cut into batches: pure integer
// arithmetic on the host (no HIP include; tools/check_render_plan.cpp compiles
// it with g++ and checks it over a sweep of shapes).
//
// A call renders the virtual tiles [0, ntiles) of its rectangle, spp samples
// each; a batch is tiles [tile0, tile0 + ntiles) x samples [s0, s0 + ns) and
// holds one path slot per tile pixel and sample.  mtsg.hip fits maxPaths to
// the free HBM (fit_paths), fills its DevBatch records from the plan and runs
// `lanes` batches at a time.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

constexpr int PLAN_TILE = 16;                                     // tile edge (kernels.h TILE)
constexpr uint32_t PLAN_TILE_SLOTS = PLAN_TILE * PLAN_TILE;       // path slots per tile and sample
// row rotation of the tile deal (include/mtsg.h): fixed at 1, as the
// oracle, mtsg_tile_windows and mtsg.put_tile_windows assume (the round-3
// measurement override is gone: a rank with another rotation would put
// its tiles in the wrong places without an error)
constexpr int PLAN_DEAL_SKEW = 1;
// direct / ao renders send a fan of `fan` rays per path slot (shadow + BSDF
// rays; `path`: 1).  A batch's fan is indexed with 31 bits (bit 31 of a shadow
// ray's target marks a final slot, kernels.h shadow_unoccluded), so a batch
// holds at most PLAN_MAX_RAYS / fan slots, and one tile of one sample fits
// whatever the fan is up to PLAN_MAX_FAN.
constexpr uint32_t PLAN_MAX_RAYS = 1u << 31;
constexpr uint32_t PLAN_MAX_FAN = PLAN_MAX_RAYS / PLAN_TILE_SLOTS / 128;   // 65536

struct PlanBatch {
    uint32_t tile0, ntiles;   // virtual tile range
    uint32_t s0, ns;          // sample range
    uint32_t nslots;          // ntiles * ns * PLAN_TILE_SLOTS
    uint32_t nrays;           // nslots * fan: the batch's fan entries (<= PLAN_MAX_RAYS)
};

struct RenderPlan {
    uint32_t tilesX, allTiles;         // tile grid of the rectangle
    uint32_t ntiles;                   // virtual tiles of this call (its share of the deal, or the listed keys)
    uint32_t tstride, toffset;         // deal key of virtual tile v = toffset + v * tstride (unless listed)
    uint32_t lanes;                    // batches in flight
    uint32_t sppPerBatch, tilesPerBatch;
    uint32_t tileGroups;               // planned tile ranges: a multiple of lanes, or one per tile
    uint32_t fan;                      // rays per path slot
    std::vector<PlanBatch> batches;    // tile-major, then sample-major
};

// tile_w x tile_h: the rectangle; listedKeys: the number of deal keys of
// mtsg_set_tile_list (0: none, the call takes tile_stride / tile_offset);
// maxPaths: the path slots in flight over all lanes, after the memory fit;
// singleLane: the debug, counting, multichannel and direct / ao modes;
// fan: 1 .. PLAN_MAX_FAN (maxPaths already counts the fan's bytes per slot)
inline RenderPlan plan_render(int tile_w, int tile_h, uint32_t spp, int tile_stride, int tile_offset, uint32_t listedKeys,
                              uint32_t maxPaths, uint32_t lanes, bool singleLane, uint32_t fan = 1) {
    RenderPlan R;
    R.fan = std::max(1u, std::min(fan, PLAN_MAX_FAN));
    const uint32_t tilesY = (uint32_t)(tile_h + PLAN_TILE - 1) / PLAN_TILE;
    R.tilesX = (uint32_t)(tile_w + PLAN_TILE - 1) / PLAN_TILE;
    R.allTiles = R.tilesX * tilesY;
    R.tstride = tile_stride > 1 ? (uint32_t)tile_stride : 1u;
    R.toffset = tile_stride > 1 ? (uint32_t)tile_offset : 0u;
    R.ntiles = listedKeys ? listedKeys : R.toffset < R.allTiles ? (R.allTiles - R.toffset + R.tstride - 1) / R.tstride : 0u;
    // Lanes: independent batches on their own streams, issued bounce by bounce
    // in lock step, so one lane's launch tail (its slowest rays) overlaps the
    // other lane's launch.
    R.lanes = (singleLane || R.ntiles < 2) ? 1u : lanes;
    const uint32_t lanePaths = std::max<uint32_t>(PLAN_TILE_SLOTS, std::min(maxPaths / R.lanes, PLAN_MAX_RAYS / R.fan));
    R.sppPerBatch = std::max(1u, std::min(spp, lanePaths / PLAN_TILE_SLOTS));
    // equal-sized batches, a multiple of the lane count: a nearly empty last
    // batch costs a full set of bounce launches (and their tails) for a
    // sliver of the work
    const uint32_t tilesMax = std::max(1u, lanePaths / (PLAN_TILE_SLOTS * R.sppPerBatch));
    const uint32_t fit = std::max(1u, (R.ntiles + tilesMax - 1) / tilesMax);
    R.tileGroups = std::min(R.ntiles ? R.ntiles : 1u, (fit + R.lanes - 1) / R.lanes * R.lanes);
    R.tilesPerBatch = std::max(1u, (R.ntiles + R.tileGroups - 1) / R.tileGroups);
    for (uint32_t t0 = 0; t0 < R.ntiles; t0 += R.tilesPerBatch)
        for (uint32_t s0 = 0; s0 < spp; s0 += R.sppPerBatch) {
            PlanBatch B;
            B.tile0 = t0;
            B.ntiles = std::min(R.tilesPerBatch, R.ntiles - t0);
            B.s0 = s0;
            B.ns = std::min(R.sppPerBatch, spp - s0);
            B.nslots = B.ntiles * B.ns * PLAN_TILE_SLOTS;
            B.nrays = B.nslots * R.fan;
            R.batches.push_back(B);
        }
    return R;
}
