// adaptive_plan.h -- the round bookkeeping of an adaptive render
// (src/integrators/misc/adaptive.cpp:197-284 on a wavefront): pure integer
// arithmetic on the host, beside render_plan.h (no HIP include;
// tools/check_adaptive_plan.cpp compiles it with g++ and sweeps it).
//
// A pixel takes samples 0, 1, ... until it stops, at the latest at the cap.
// Round 0 renders samples [0, min(N, cap)) of every tile of the call, round
// r >= 1 the next `later` samples of the tiles that still hold an active
// pixel; a round is cut into batches by plan_render over the listed tiles,
// its sample range shifted to the round's.  The pre-pass (adaptive.cpp:125-159)
// runs as a strip of 16 pixel columns below every sample id the film uses.
#pragma once

#include "render_plan.h"

constexpr uint32_t ADAPTIVE_PREPASS_SAMPLES = 10000;   // nSamples (adaptive.cpp:128)
constexpr uint32_t ADAPTIVE_MAX_ROUND = 65536;         // MTSG_OPT_ADAPTIVE_ROUND's range

// the most samples a pixel takes: count >= maxSampleFactor * N stops it, after
// at least one sample (adaptive.cpp:241-251)
inline uint32_t adaptive_cap(int32_t maxSampleFactor, uint32_t N) {
    const uint64_t c = (uint64_t)(maxSampleFactor > 0 ? maxSampleFactor : 0) * N;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c, 1u << 24));
}

// samples [s0, s0 + ns) of round r; false: no such round (the cap is covered)
inline bool adaptive_round(uint32_t N, uint32_t cap, uint32_t later, uint32_t r, uint32_t &s0, uint32_t &ns) {
    const uint32_t first = std::min(N, cap);
    later = std::max(1u, std::min(later ? later : N, ADAPTIVE_MAX_ROUND));
    if (r == 0) { s0 = 0; ns = first; return true; }
    const uint64_t b = (uint64_t)first + (uint64_t)(r - 1) * later;
    if (b >= cap) return false;
    s0 = (uint32_t)b;
    ns = std::min(later, cap - s0);
    return true;
}

// the batches of a round over nActive listed tiles (nActive >= 1)
inline RenderPlan adaptive_round_plan(int tile_w, int tile_h, uint32_t nActive, uint32_t s0, uint32_t ns, uint32_t maxPaths) {
    RenderPlan R = plan_render(tile_w, tile_h, ns, 1, 0, nActive, maxPaths, 1u, true);
    for (PlanBatch &b : R.batches) b.s0 += s0;
    return R;
}

// keeps the keys whose tile still holds an active pixel (active[key] != 0), in
// order; the others go to `finished`.  Returns the number kept.
inline uint32_t adaptive_compact(std::vector<int32_t> &keys, const std::vector<uint32_t> &active, std::vector<int32_t> &finished) {
    uint32_t n = 0;
    finished.clear();
    for (size_t v = 0; v < keys.size(); ++v) {
        const int32_t k = keys[v];
        if ((size_t)k < active.size() && active[(size_t)k]) keys[n++] = k;
        else finished.push_back(k);
    }
    keys.resize(n);
    return n;
}

// The pre-pass strip: sample i is "pixel" (i % 16, row0 + i / 16) of a film 16
// wide with one sample per pixel, so its sample id is row0 * 16 + i; row0 is
// the first row whose ids lie past the film's own (film pixels x cap).
// false: the strip's rows do not fit an int.
inline bool adaptive_prepass_rows(uint64_t filmPixels, uint32_t cap, int32_t &row0, int32_t &rows) {
    const uint64_t r0 = (filmPixels * cap + PLAN_TILE - 1) / PLAN_TILE;
    rows = (int32_t)((ADAPTIVE_PREPASS_SAMPLES + PLAN_TILE - 1) / PLAN_TILE);
    if (r0 + (uint64_t)rows + PLAN_TILE > (uint64_t)INT32_MAX) return false;
    row0 = (int32_t)r0;
    return true;
}
