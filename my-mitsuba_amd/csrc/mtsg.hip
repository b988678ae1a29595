// mtsg.hip -- MI355X (gfx950, CDNA4) wavefront unidirectional path tracer
// behind the C-ABI in include/mtsg.h.
//
// Replaces, for the `path` plugin, the reference's per-sample CPU loop
//   SamplingIntegrator::renderBlock   src/librender/integrator.cpp:144-197
//   MIPathTracer::Li                  src/integrators/path/path.cpp:119-294
//   ShapeKDTree::rayIntersect         src/librender/skdtree.cpp:112-226
//   SAHKDTree3D::rayIntersectHavran   include/mitsuba/render/sahkdtree3.h:178-308
//   TriAccel::rayIntersect            include/mitsuba/render/triaccel.h:96-158
//   diffuse / roughconductor / dielectric sample, eval, pdf
//   AreaLight + Scene::sampleEmitterDirect / pdfEmitterDirect
//   ImageBlock::put                   include/mitsuba/render/imageblock.h:124-204
// with a wavefront of SoA path states in HBM:
//   k_camera -> [ k_trace_closest -> k_shade -> k_trace_shadow ] x bounces -> k_splat
// Active paths are compacted into queues with wave-aggregated atomics
// (__ballot / __popcll / mbcnt on 64-lane waves); the kd-tree traversal
// keeps a short stack in LDS (kd-restart on overflow); the film is splatted
// per 16x16 tile into LDS and flushed with one float atomic per texel.
// No MFMA: the path has no dense contraction.  See DESIGN.md.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include <chrono>
#include <functional>

#include "../../include/mtsg.h"
#include "device_math.h"
#include "envmap.h"
#include "sampler.h"

#include "kernels.h"
#include "render_plan.h"
#include "adaptive_plan.h"
#include "kd_layout.h"

// the default of MTSG_OPT_RAY_PRESETUP.  0: measured on C3, the producers' tests
// and the 16 B per ray cost more than the refill saves (shade +4.4 ms, camera
// +0.8, trace -3.7 of 129; profiles/ray_presetup_ab.txt).  1: a build for A/B
// runs of a benchmark that sets no options.
#ifndef MTSG_RAY_PRESETUP
#define MTSG_RAY_PRESETUP 0
#endif
// the default of MTSG_OPT_LEAF_FILTER (0: a build for A/B runs of a benchmark
// that sets no options)
#ifndef MTSG_LEAF_FILTER
#define MTSG_LEAF_FILTER 1
#endif

static_assert(PLAN_TILE == TILE, "render_plan.h plans in tiles of kernels.h's edge");

namespace {

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
thread_local std::string g_err;

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            g_err = std::string(#expr) + ": " + hipGetErrorString(_e);                 \
            return _e == hipErrorOutOfMemory ? MTSG_ERR_OOM : MTSG_ERR_DEVICE;         \
        }                                                                              \
    } while (0)

template <class T>
int upload(const T *src, size_t n, T **dst) {
    *dst = nullptr;
    if (n == 0) return MTSG_OK;
    HIP_TRY(hipMalloc((void **)dst, n * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return MTSG_OK;
}

// The scratch buffers of the query entries: n T on the device, freed with the
// scope.  Every step keeps its failure in the caller's `e` and is skipped once
// `e` is set, so an entry checks `e` once after its last step.  (The scene's
// long-lived buffers state their lifetimes themselves: allocs, free_batch,
// free_aov.)
template <class T>
struct DevBuf {
    hipError_t &e;
    const size_t n;
    T *p = nullptr;
    // n == 0: no buffer (p stays null); src: n T to upload
    DevBuf(hipError_t &err, size_t count, const T *src = nullptr) : e(err), n(count) {
        if (e == hipSuccess && n) e = hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess && n && src) e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    ~DevBuf() { hipFree(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    void zero() { if (e == hipSuccess && n) e = hipMemset(p, 0, n * sizeof(T)); }
    void download(T *dst) { if (e == hipSuccess && n) e = hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost); }
};

}  // namespace

struct mtsg_scene {
    int device = 0;
    mtsg_tile_fn tileFn = nullptr;   // tile completion (mtsg_set_tile_callback)
    void *tileUser = nullptr;
    hipStream_t stream = nullptr;
    DevScene ds{};
    DevCamera cam{};
    std::vector<void *> allocs;
    // batch buffers
    uint32_t capacity = 0;         // paths per batch (per lane)
    uint32_t requestedBatch = 0;   // paths in flight over all lanes
    int lanes = MTSG_LANES;        // concurrent batches (streams) of a render
    int stagger = 0;               // bounces between the starts of consecutive lanes
    int lanesAlloc = 0;            // lanes with path state allocated
    hipStream_t lstream[MTSG_MAX_LANES] = {};   // lstream[0] == stream
    // mtsg_set_tile_list: the deal keys a render call takes (empty: tile_stride / tile_offset)
    std::vector<int32_t> tileKeys;
    int32_t *tileKeysDev = nullptr;
    size_t tileKeysCap = 0;
    DevPaths LP[MTSG_MAX_LANES]{};
    std::vector<void *> batchAllocs;
    uint32_t *hostCnt = nullptr;   // pinned copy of the queue counters (2 per lane)
    int cuCount = 0;
    int traceGrid = 0, shadeGrid = 0, traceGridInst = 0, finishGrid = 0, finishGridMats = 0;
    // tail mode: once a bounce starts with fewer than finishPaths paths, k_finish
    // carries them through their remaining bounces in one launch (0: off)
    uint32_t finishPaths = 0;
    // a tail-kernel wave shades once 16 of its busy lanes wait to (or none traces):
    // r06, with the 4-wave material kernels, C5 tail 18.3 -> 13.4 ms, C3 0.66 ->
    // 0.58, two-level 1.16 -> 0.99 against 1 (profiles/r06_finish_threshold.txt)
    uint32_t finishShadeMin = 16;
    uint32_t flags = 0;
    int samplerType = MTSG_SAMPLER_INDEPENDENT, samplerDim = 4;
    int qmcInv[2][3] = {{0, 0, 0}, {0, 0, 0}};
    int traceMode = 0;            // 0: refill at 16 idle lanes (measured best), 1: at 32
    // camera ray differentials (DevScene::cam_diffs / cam_env_diffs): stored
    // in the path state for filtered textures (or MTSG_OPT_CAMERA_DIFFS 1),
    // else recomputed at bounce 0 for environment misses
    bool texDiffs = false, hasEnvmap = false, storeCamDiffs = false;
    int rayOrder = 0;             // MTSG_OPT_RAY_ORDER: 1 = bounce rays sorted per window by direction (k_sortwin;
                                  // measured r06: C3 trace +6.7 ms, profiles/r06_ray_order.txt)
    float *dumpL = nullptr;
    std::atomic<int> cancel{0};
    bool knobs = false;   // traversal test overrides set (mtsg_set_test_knobs): KNOBS kernels, no tail mode
    // flat scenes: k_trace_s tests the rectangles once per ray at its setup
    // (kernels.h spec_init<true>) when the option is on (MTSG_OPT_RECT_SETUP)
    // and the scene can take it (at most RECT_SETUP_CAP rectangles, keyed
    // n_triangles + index); else the kernels that test them in the leaves
    bool rectSetupOpt = true, rectSetupOk = false;
    // ... and in that mode, on request, the kernels that make the path
    // integrator's rays (k_camera, k_shade) run those tests and leave each ray's
    // pre-record for the refill (MTSG_OPT_RAY_PRESETUP; DevPaths::pre)
    bool rayPresetupOpt = MTSG_RAY_PRESETUP != 0;
    // ... and in that mode the timed kernels walk the filtered leaf addressing
    // (kd_layout.h blocksRS: no rectangle records in the leaves; null when no
    // leaf references a rectangle) unless MTSG_OPT_LEAF_FILTER is 0.  Both
    // layouts stay resident, so the option switches per launch.
    bool leafFilterOpt = MTSG_LEAF_FILTER != 0;
    const uint4 *blocksRS = nullptr;
    uint2 root2RS{};
    mtsg_stats stats{};
    std::vector<hipEvent_t> evPool;
    size_t evUsed = 0;
    std::vector<std::pair<int, size_t>> timed;   // (kind, event index)
    std::vector<unsigned long long> stragglers;  // MTSG_FLAG_COUNT: slow-ray records
    unsigned long long *waveTimes = nullptr;     // MTSG_FLAG_WAVETIME: [launch][wave][WT_WORDS]
    uint32_t wtLaunches = 0;
    bool extBsdfs = false;   // conductor / plastic / twosided records or textures present (k_shade<..., true>)
    bool ext2 = false;       // a record of a type above roughplastic: the EM_ALL kernels at EXT level 2 (emitterSet is EM_ALL then)
    int mats = MATS_ALL;     // material classes of the scene's records (k_shade<..., MATS>)
    bool shadeGeneric = false;   // MTSG_OPT_SHADE_GENERIC: the all-materials kernel (A/B tests)
    // the scene's emitter kinds next to its material classes: EM_ALL with a
    // point / spot / directional / constant emitter (the kernels that hold
    // every kind), else EM_ENV / EM_AREA (the kernels those scenes always ran)
    int emitterSet = EM_AREA;
    uint32_t nTextures = 0;
    const uint32_t *sobolM = nullptr;        // sobol sampler tables (device)
    const uint64_t *sobolVdc = nullptr, *sobolVdcInv = nullptr;
    uint64_t sobolScramble = 0;
    // multichannel / field integrators (mtsg_scene_set_aov; fields.hip): the
    // active child set, its device tables, and the SoA field planes, which are
    // allocated only while a set with fields is active
    bool aovOn = false;
    DevAov aov{};
    std::vector<void *> aovAllocs;
    float *fieldPlanes = nullptr;
    size_t fieldCap = 0;
    int fieldCount = 0;               // fields the planes were sized for
    uint32_t nShapes = 0;
    std::vector<int32_t> bsdfTexture; // mtsg_bsdf::texture of every record (host copy)
    float *dumpMulti = nullptr;       // mtsg_render_samples_multi
    // direct / ao integrators (mtsg_scene_set_direct; direct.hip): the
    // descriptor and the fan buffers of a batch, allocated by the first such
    // render (one lane) and freed with the path state
    bool directOn = false;
    mtsg_direct_desc direct{};
    DevDirect fan{};
    std::vector<void *> fanAllocs;
    size_t fanClosest = 0, fanShadow = 0;   // BSDF / shadow rays the buffers hold
    // adaptive integrator (mtsg_scene_set_adaptive; adaptive.hip): the
    // descriptor, the size of the rounds after the first (MTSG_OPT_ADAPTIVE_ROUND,
    // 0: the base count), and what the last such render leaves for mtsg_adaptive_info
    bool adaptiveOn = false;
    mtsg_adaptive_desc adaptive{};
    uint32_t adaptiveRound = 0;
    bool adaptiveHave = false;
    mtsg_adaptive_result adaptiveResult{};
    std::vector<uint32_t> adaptiveCounts;
};

namespace {

int set_device(mtsg_scene *s) {
    HIP_TRY(hipSetDevice(s->device));
    return MTSG_OK;
}

// bytes of a sample's fan: per BSDF ray origin, direction, hit, tie entry,
// instance, bsdfVal + pdf, flag; per shadow ray origin, direction,
// contribution and its cell
constexpr size_t FAN_CLOSEST_BYTES = 32 + 16 + 4 + 4 + 16 + 4, FAN_SHADOW_BYTES = 48 + 16;
size_t fan_bytes(uint32_t ne, uint32_t nb) { return nb * FAN_CLOSEST_BYTES + ne * FAN_SHADOW_BYTES; }

void free_fan(mtsg_scene *s) {
    for (void *p : s->fanAllocs) hipFree(p);
    s->fanAllocs.clear();
    s->fan = DevDirect{};
    s->fanClosest = s->fanShadow = 0;
}

void free_batch(mtsg_scene *s) {
    free_fan(s);
    for (void *p : s->batchAllocs) hipFree(p);
    s->batchAllocs.clear();
    if (s->fieldPlanes) hipFree(s->fieldPlanes);
    s->fieldPlanes = nullptr;
    s->fieldCap = 0;
    s->fieldCount = 0;
    s->capacity = 0;
    s->lanesAlloc = 0;
}

int ensure_batch(mtsg_scene *s, uint32_t paths, int lanes) {
    // the order buffer (k_sortwin) and the pre-records only once
    // MTSG_OPT_RAY_ORDER 1 / MTSG_OPT_RAY_PRESETUP 1 ask for them
    const bool order = s->rayOrder == 1 || s->LP[0].orderBuf, pre = s->rayPresetupOpt || s->LP[0].preBuf;
    if (s->capacity >= paths && s->lanesAlloc >= lanes && (!order || s->LP[0].orderBuf) && (!pre || s->LP[0].preBuf)) return MTSG_OK;
    paths = std::max(paths, s->capacity);
    lanes = std::max(lanes, s->lanesAlloc);
    free_batch(s);
    auto alloc = [&](size_t bytes, void **p) -> int {
        HIP_TRY(hipMalloc(p, bytes));
        s->batchAllocs.push_back(*p);
        return MTSG_OK;
    };
    size_t n = paths;
    int rc = MTSG_OK;
    for (int l = 0; l < lanes; ++l) {
    DevPaths &P = s->LP[l];
#define A(field, T) if ((rc = alloc(n * sizeof(T), (void **)&P.field)) != MTSG_OK) return rc
    A(ray_o, float4); A(ray_d, float4); A(T, float4); A(aux, float4); A(Lp, float4); A(meta, uint4);
    A(n_ray_o, float4); A(n_ray_d, float4); A(n_T, float4); A(n_aux, float4); A(n_Lp, float4); A(n_meta, uint4);
    A(hit, float4); A(L, float4); A(sh_o, float4); A(sh_d, float4); A(sh_c, float4);
    if (s->ds.inst) { A(hitInst, uint32_t); } else P.hitInst = nullptr;
    A(tie, uint32_t);
    if (pre) { A(preBuf, float4); } else P.preBuf = nullptr;
    P.pre = nullptr;
    if (order) { A(orderBuf, uint32_t); } else P.orderBuf = nullptr;
    P.order = nullptr;
#undef A
    if ((rc = alloc(CNT_WORDS * sizeof(uint32_t), (void **)&P.cnt)) != MTSG_OK) return rc;
    if ((rc = alloc(CTR_WORDS * sizeof(unsigned long long), (void **)&P.ctr)) != MTSG_OK) return rc;
    HIP_TRY(hipMemset(P.ctr, 0, CTR_WORDS * sizeof(unsigned long long)));
    }
    s->capacity = paths;
    s->lanesAlloc = lanes;
    return MTSG_OK;
}

// the fan buffers of a direct / ao batch of `slots` samples (lane 0's)
int ensure_fan(mtsg_scene *s, size_t slots, uint32_t ne, uint32_t nb) {
    const size_t nC = slots * nb, nS = slots * ne;
    if (s->fanClosest >= nC && s->fanShadow >= nS) return MTSG_OK;
    free_fan(s);
    auto alloc = [&](size_t bytes, void **p) -> int {
        *p = nullptr;
        if (!bytes) return MTSG_OK;
        HIP_TRY(hipMalloc(p, bytes));
        s->fanAllocs.push_back(*p);
        return MTSG_OK;
    };
    DevDirect &D = s->fan;
    DevPaths &F = D.F;
    int rc;
#define A(ptr, n, T) if ((rc = alloc((n) * sizeof(T), (void **)&ptr)) != MTSG_OK) return rc
    A(F.ray_o, nC, float4); A(F.ray_d, nC, float4); A(F.hit, nC, float4); A(F.tie, nC, uint32_t);
    if (s->ds.inst) { A(F.hitInst, nC, uint32_t); }
    A(D.val, nC, float4); A(D.flag, nC, uint32_t);
    A(F.sh_o, nS, float4); A(F.sh_d, nS, float4); A(F.sh_c, nS, float4); A(F.Lp, nS, float4);
#undef A
    s->fanClosest = nC;
    s->fanShadow = nS;
    return MTSG_OK;
}

enum { K_CAMERA = 0, K_CLOSEST, K_SHADOW, K_SHADE, K_SPLAT, K_FINISH, K_SORT };

// the survivors k_shade compacted into n_* are the next bounce's paths
void swap_bounce(DevPaths &P) {
    std::swap(P.ray_o, P.n_ray_o);
    std::swap(P.ray_d, P.n_ray_d);
    std::swap(P.T, P.n_T);
    std::swap(P.aux, P.n_aux);
    std::swap(P.Lp, P.n_Lp);
    std::swap(P.meta, P.n_meta);
}

hipEvent_t next_event(mtsg_scene *s) {
    if (s->evUsed == s->evPool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        s->evPool.push_back(e);
    }
    return s->evPool[s->evUsed++];
}

// bracket a launch with events when timing is enabled
template <class F>
void timed_launch(mtsg_scene *s, int kind, hipStream_t st, F f) {
    if (!(s->flags & MTSG_FLAG_TIMING)) { f(); return; }
    size_t i0 = s->evUsed;
    hipEventRecord(next_event(s), st);
    f();
    hipEventRecord(next_event(s), st);
    s->timed.emplace_back(kind, i0);
}

// One traversal launch over a work list (see k_trace_s): closest rays cIn,
// shadow rays sIn.  traceMode 1 refills lanes at 32 idle lanes instead of 16
// (MTSG_TRACE_MODE, for measurement).
template <bool COUNT>
void launch_trace_c(mtsg_scene *s, const DevPaths &P, int cIn, int sIn, uint32_t n, hipStream_t st, bool pre) {
    dim3 g(s->traceGrid), blk(TRACE_BLOCK);
    unsigned long long *wt = nullptr;
    if ((s->flags & MTSG_FLAG_WAVETIME) && s->waveTimes && s->wtLaunches < WT_MAX_LAUNCHES && !s->ds.inst)
        wt = s->waveTimes + (size_t)WT_WORDS * s->traceGrid * s->wtLaunches++;
    // the KNOBS instantiations read the stack caps and restart limits the
    // scene was created with (test overrides); the COUNT pass ignores them
    // closest rays that met an exact tie: traced again with the mailbox
    // (a grid a quarter of the trace grid's; two-level: the exact Havran).
    // The flat traversal retraces them inside its own launch (TIE_INLINE).
    const dim3 tg(std::max<unsigned>(1u, (unsigned)s->traceGrid / 4u));
    if (!s->ds.inst) {   // the flat kernels: trace_flat.hip
        FlatTraceLaunch a{g, tg, st, &s->ds, &P, cIn, sIn, n, wt, COUNT, s->knobs, s->traceMode == 1,
                          MTSG_MAILBOX && cIn != -2 && !TIE_INLINE, s->rectSetupOpt && s->rectSetupOk, pre};
        a.leafFilter = s->leafFilterOpt && s->blocksRS != nullptr;
        a.blocksRS = s->blocksRS;
        a.root2RS = s->root2RS;
        launch_trace_flat(a);
        return;
    }
    if (s->knobs && !COUNT)
        hipLaunchKernelGGL((k_trace_s<false, MTSG_INST_MIN_IDLE, true, true>), dim3(s->traceGridInst), blk, 0, st, s->ds, P, cIn, sIn, n, wt);
    else hipLaunchKernelGGL((k_trace_s<COUNT, MTSG_INST_MIN_IDLE, true>), dim3(s->traceGridInst), blk, 0, st, s->ds, P, cIn, sIn, n, wt);
    if (MTSG_MAILBOX && cIn != -2) hipLaunchKernelGGL(k_tie_i, tg, blk, 0, st, s->ds, P);
}
// pre: the rays carry pre-records (P.pre; FlatTraceLaunch::pre)
void launch_trace(mtsg_scene *s, bool count, const DevPaths &P, int cIn, int sIn, uint32_t n, hipStream_t st, bool pre = false) {
    if (count) launch_trace_c<true>(s, P, cIn, sIn, n, st, pre);
    else launch_trace_c<false>(s, P, cIn, sIn, n, st, pre);
}
// whether a handle's flat traversal launches can take pre-records at all: the
// setup mode is on and applies, and the test knobs' kernel is not in use
bool presetup_applies(const mtsg_scene *s) {
    return s->rayPresetupOpt && s->rectSetupOpt && s->rectSetupOk && !s->ds.inst && !s->knobs;
}

// k_shade / k_finish are instantiated per sampler in smp_kernels.hip
ShadeLaunch shade_args(mtsg_scene *s, const DevIntegrator &I, const DevBatch &B, const DevPaths &P, int b, int qin, hipStream_t st,
                       dim3 grid, dim3 block) {
    ShadeLaunch a;
    a.grid = grid;
    a.block = block;
    a.stream = st;
    a.S = &s->ds;
    a.I = &I;
    a.B = &B;
    a.P = &P;
    a.bounce = b;
    a.qin = qin;
    a.nIdentity = B.nslots;
    a.hasAlpha = s->cam.has_alpha || s->aovOn;   // multichannel: alpha is always a channel of the block
    a.shadeMin = s->finishShadeMin;
    a.env = (s->ds.has_env & 1) != 0;
    a.ext = s->extBsdfs;
    a.inst = s->ds.inst != nullptr;
    a.emx = s->emitterSet == EM_ALL;
    a.ext2 = s->ext2;
    a.mats = (s->shadeGeneric || a.emx) ? (int)MATS_ALL : s->mats;
    return a;
}
// where bounce 0 finds the camera rays' differentials (mtsg_scene::storeCamDiffs)
void camera_diff_mode(mtsg_scene *s) {
    // (a thinlens ray's differentials depend on its aperture sample: always carried)
    s->ds.cam_diffs = (s->texDiffs || (s->hasEnvmap && (s->storeCamDiffs || s->cam.lens))) ? 1 : 0;
    s->ds.cam_env_diffs = (s->hasEnvmap && !s->ds.cam_diffs) ? 1 : 0;
    s->cam.diffs = s->ds.cam_diffs;
}
void launch_shade(mtsg_scene *s, const DevIntegrator &I, const DevBatch &B, const DevPaths &P, int b, int qin, hipStream_t st) {
    const ShadeLaunch a = shade_args(s, I, B, P, b, qin, st, dim3(s->shadeGrid), dim3(SHADE_BLOCK));
    switch (I.smp.type) {
        case MTSG_SAMPLER_HALTON: launch_shade_smp<MTSG_SAMPLER_HALTON>(a); break;
        case MTSG_SAMPLER_HAMMERSLEY: launch_shade_smp<MTSG_SAMPLER_HAMMERSLEY>(a); break;
        case MTSG_SAMPLER_LDSAMPLER: launch_shade_smp<MTSG_SAMPLER_LDSAMPLER>(a); break;
        case MTSG_SAMPLER_SOBOL: launch_shade_smp<MTSG_SAMPLER_SOBOL>(a); break;
        default: launch_shade_smp<MTSG_SAMPLER_INDEPENDENT>(a);
    }
}
void launch_finish(mtsg_scene *s, const DevIntegrator &I, const DevBatch &B, const DevPaths &P, int qin, hipStream_t st) {
    const bool mats = finish_uses_mats(I.smp.type, s->extBsdfs, s->ds.inst != nullptr,
                                       (s->shadeGeneric || s->emitterSet == EM_ALL) ? (int)MATS_ALL : s->mats);
    const ShadeLaunch a = shade_args(s, I, B, P, 1, qin, st, dim3(mats ? s->finishGridMats : s->finishGrid), dim3(TRACE_BLOCK));
    switch (I.smp.type) {
        case MTSG_SAMPLER_HALTON: launch_finish_smp<MTSG_SAMPLER_HALTON>(a); break;
        case MTSG_SAMPLER_HAMMERSLEY: launch_finish_smp<MTSG_SAMPLER_HAMMERSLEY>(a); break;
        case MTSG_SAMPLER_LDSAMPLER: launch_finish_smp<MTSG_SAMPLER_LDSAMPLER>(a); break;
        case MTSG_SAMPLER_SOBOL: launch_finish_smp<MTSG_SAMPLER_SOBOL>(a); break;
        default: launch_finish_smp<MTSG_SAMPLER_INDEPENDENT>(a);
    }
}
// k_splat<K, C>: the reconstruction filter's footprint of K x K texels (5, up
// to 3, or up to 9) and C floats per texel (5 with the film's alpha channel)
void launch_splat(mtsg_scene *s, const DevIntegrator &I, const DevBatch &B, const DevPaths &P, float *film, int blockW, int blockH,
                  int win, hipStream_t st) {
    const dim3 g(B.ntiles, (B.ns + SPLAT_CHUNK - 1) / SPLAT_CHUNK);
    const int K = 2 * s->cam.border + 1;
#define SPLAT(W, C) hipLaunchKernelGGL((k_splat<W, C>), g, dim3(BLOCK), 0, st, s->cam, I, B, P, film, blockW, blockH, win)
    if (K == 5 && !s->cam.has_alpha) SPLAT(5, 4);
    else if (K == 5) SPLAT(5, 5);
    else if (K <= 3 && !s->cam.has_alpha) SPLAT(3, 4);
    else if (K <= 3) SPLAT(3, 5);
    else if (!s->cam.has_alpha) SPLAT(9, 4);
    else SPLAT(9, 5);
#undef SPLAT
}

// Sampler constants of a render (setFilmResolution with blocked = true over
// the film's crop size: halton.cpp:240-271, hammersley.cpp:181-200)
DevSampler make_sampler(const mtsg_scene *s, uint32_t spp) {
    DevSampler S{};
    S.type = s->samplerType;
    S.ldDim = s->samplerDim;
    while ((1u << S.ldBits) < spp) ++S.ldBits;
    S.stride = 1;
    S.primes = s->ds.qmcPrimes;
    S.off = s->ds.qmcOff;
    S.perm = s->ds.qmcPerm;
    S.sobolM = s->sobolM;
    S.vdc = s->sobolVdc;
    S.vdcInv = s->sobolVdcInv;
    S.sobolScramble = s->sobolScramble;
    S.logRes = 0;
    S.sobolRes = 1.0f;
    if (S.type == MTSG_SAMPLER_SOBOL) {
        // setFilmResolution(crop size, bucketed = true) (sobol.cpp:147-158)
        uint32_t r = 1;
        while (r < (uint32_t)std::max(s->cam.crop_w, s->cam.crop_h)) r <<= 1;
        S.sobolRes = (float)r;
        while ((1u << (S.logRes + 1)) <= r) ++S.logRes;
    }
    for (int b = 0; b < 2; ++b)
        for (int j = 0; j < 3; ++j) S.inv[b][j] = (uint16_t)s->qmcInv[b][j];
    const int crop[2] = {s->cam.crop_w, s->cam.crop_h};
    if (S.type == MTSG_SAMPLER_HALTON) {
        const uint32_t primes[2] = {2, 3};
        for (int i = 0; i < 2; ++i) {
            uint32_t value = 1, e = 0;
            while ((int)value < std::min(crop[i], 128)) { value *= primes[i]; ++e; }
            S.primePow[i] = value;
            S.primeExp[i] = e;
            S.stride *= value;
        }
        // multiplicativeInverse (halton.cpp:211-234)
        auto inv = [](int64_t a, int64_t n) {
            int64_t t = 0, nt = 1, r = n, nr = a % n;
            while (nr) { int64_t q = r / nr; std::swap(t, nt); nt -= q * t; std::swap(r, nr); nr -= q * r; }
            return (uint32_t)(t < 0 ? t + n : t);
        };
        S.multInv[0] = S.primePow[0] > 1 ? inv(S.primePow[1], S.primePow[0]) : 0;
        S.multInv[1] = S.primePow[1] > 1 ? inv(S.primePow[0], S.primePow[1]) : 0;
    } else if (S.type == MTSG_SAMPLER_HAMMERSLEY) {
        for (int i = 0; i < 2; ++i) {
            uint32_t r = 1;
            while (r < (uint32_t)crop[i]) r <<= 1;
            S.res[i] = std::min<uint32_t>(128, r);
        }
        S.logH = 0;
        while ((1u << (S.logH + 1)) <= S.res[1]) ++S.logH;
        S.factor = 1.0f / (float)((size_t)spp * S.res[0] * S.res[1]);
        S.stride = S.res[1];
    }
    return S;
}

// the SoA field planes of the active child set, one float per path slot and
// channel; plain renders allocate none (PATH_STATE_BYTES is unchanged)
int ensure_fields(mtsg_scene *s) {
    const int nf = s->aov.nf;
    if (s->fieldPlanes && s->fieldCap >= s->capacity && s->fieldCount >= nf) return MTSG_OK;
    if (s->fieldPlanes) hipFree(s->fieldPlanes);
    s->fieldPlanes = nullptr;
    s->fieldCap = 0;
    s->fieldCount = 0;
    if (nf == 0) return MTSG_OK;
    HIP_TRY(hipMalloc((void **)&s->fieldPlanes, (size_t)s->capacity * nf * 3 * sizeof(float)));
    s->fieldCap = s->capacity;
    s->fieldCount = nf;
    return MTSG_OK;
}
void free_aov(mtsg_scene *s) {
    for (void *p : s->aovAllocs) hipFree(p);
    s->aovAllocs.clear();
    if (s->fieldPlanes) hipFree(s->fieldPlanes);
    s->fieldPlanes = nullptr;
    s->fieldCap = 0;
    s->fieldCount = 0;
    s->aovOn = false;
    s->aov = DevAov{};
}

const char *const traversal_error =
    "kd-tree traversal: a ray reached the restart limit without making progress (kernels.h kd_restart)";
// Mitsuba's Log(EError) of Halton/Hammersley (halton.cpp:343-386) and sobol (sobol.cpp:223-239)
const char *dim_error(int sampler) {
    return sampler == MTSG_SAMPLER_SOBOL
               ? "Lookup dimension exceeds the direction number table size! You may have to reduce the 'maxDepth' parameter of your integrator."
               : "Lookup dimension exceeds the prime number table size! You may have to reduce the 'maxDepth' parameter of your integrator.";
}

// Mitsuba's Log(EError) of HammersleySampler::request2DArray (hammersley.cpp:297-301)
constexpr uint64_t MAX_ARRAY_ENTRIES = 1ull << 31;   // spp x array size (sampler.h smp_array2D)
const char *const hammersley_array_error =
    "request2DArray(): Not supported for the Hammersley QMC sequence! If you used this sampler together with the 'direct' or 'ao' "
    "integrators, you will have to set the 'shadingSamples' parameter to 1 to use this sampler.";

// the fan of a direct / ao render: shadow and BSDF rays per camera sample
void fan_counts(const mtsg_scene *s, const mtsg_render_params *p, uint32_t &ne, uint32_t &nb) {
    ne = nb = 0;
    if (p->integrator == MTSG_INTEGRATOR_DIRECT) { ne = s->direct.emitter_samples; nb = s->direct.bsdf_samples; }
    else if (p->integrator == MTSG_INTEGRATOR_AO) ne = s->direct.ao_samples;
}
// the 2D array requests of its configureSampler (direct.cpp:138-144, ao.cpp:65-70)
DevArrays fan_arrays(uint32_t ne, uint32_t nb) {
    DevArrays A{};
    if (ne > 1) A.n[A.count++] = ne;
    if (nb > 1) A.n[A.count++] = nb;
    return A;
}

int validate(const mtsg_render_params *p, const mtsg_scene *s) {
    if (!p) { g_err = "null params"; return MTSG_ERR_INVALID; }
    if (p->spp == 0) { g_err = "spp must be > 0"; return MTSG_ERR_INVALID; }
    if (s->samplerType == MTSG_SAMPLER_LDSAMPLER && (p->spp & (p->spp - 1))) {
        g_err = "ldsampler: the sample count must be a power of two";
        return MTSG_ERR_INVALID;
    }
    if (p->rr_depth <= 0) { g_err = "'rrDepth' must be set to a value greater than zero!"; return MTSG_ERR_INVALID; }
    if (p->max_depth <= 0 && p->max_depth != -1) { g_err = "'maxDepth' must be set to -1 (infinite) or a value greater than zero!"; return MTSG_ERR_INVALID; }
    if (p->tile_w <= 0 || p->tile_h <= 0 || p->tile_x < 0 || p->tile_y < 0 ||
        p->tile_x + p->tile_w > s->cam.film_w || p->tile_y + p->tile_h > s->cam.film_h) {
        g_err = "tile rectangle outside the film";
        return MTSG_ERR_INVALID;
    }
    if (p->tile_stride < 0 || (p->tile_stride > 1 && (p->tile_offset < 0 || p->tile_offset >= p->tile_stride))) {
        g_err = "invalid tile_stride / tile_offset";
        return MTSG_ERR_INVALID;
    }
    if (p->integrator < MTSG_INTEGRATOR_PATH || p->integrator > MTSG_INTEGRATOR_AO) { g_err = "unknown integrator"; return MTSG_ERR_INVALID; }
    if (p->integrator == MTSG_INTEGRATOR_DIRECT || p->integrator == MTSG_INTEGRATOR_AO) {
        const bool ao = p->integrator == MTSG_INTEGRATOR_AO;
        if (!s->directOn) {
            g_err = std::string(ao ? "ao" : "direct") + ": the handle has no mtsg_direct_desc (mtsg_scene_set_direct)";
            return MTSG_ERR_INVALID;
        }
        const mtsg_direct_desc &d = s->direct;
        if (!ao && d.emitter_samples + d.bsdf_samples == 0) { g_err = "direct: emitterSamples + bsdfSamples must be greater than zero"; return MTSG_ERR_INVALID; }
        if (ao && (d.ao_samples == 0 || !(d.ao_ray_length > 0))) { g_err = "ao: shadingSamples and rayLength must be greater than zero"; return MTSG_ERR_INVALID; }
        const bool arrays = ao ? d.ao_samples > 1 : (d.emitter_samples > 1 || d.bsdf_samples > 1);
        if (arrays && s->samplerType == MTSG_SAMPLER_HAMMERSLEY) {
            g_err = hammersley_array_error;
            return MTSG_ERR_INVALID;
        }
        // one array's entry s n + k indexes 32-bit sequences, and the ldsampler's
        // shuffle walks a power of two that holds spp n
        const uint64_t most = ao ? d.ao_samples : std::max(d.emitter_samples, d.bsdf_samples);
        if (most * p->spp > MAX_ARRAY_ENTRIES) { g_err = "sample arrays: spp x array size exceeds 2^31"; return MTSG_ERR_INVALID; }
    }
    if (p->integrator == MTSG_INTEGRATOR_PATH2_OM) {
        if (!s->ds.om) { g_err = "myPath2_OM: the scene has no occupancy maps"; return MTSG_ERR_INVALID; }
        if (s->samplerType != MTSG_SAMPLER_INDEPENDENT) { g_err = "myPath2_OM: only the independent sampler is supported"; return MTSG_ERR_INVALID; }
        if (p->max_depth < 1) { g_err = "myPath2_OM: 'maxDepthEye' must be at least 1"; return MTSG_ERR_INVALID; }
        if (p->om_strategy < MTSG_OM_STRATEGY_BSDF || p->om_strategy > MTSG_OM_STRATEGY_MIS || p->om_mis < MTSG_OM_MIS_UNIFORM ||
            p->om_mis > MTSG_OM_MIS_POWER) {
            g_err = "myPath2_OM: unknown strategy or MIS mode";
            return MTSG_ERR_INVALID;
        }
    }
    return MTSG_OK;
}

// The paths a render keeps in flight over all lanes: the requested batch, or
// the default fitted to the free HBM (stateBytes per path)
uint32_t fit_paths(const mtsg_scene *s, size_t stateBytes) {
    if (s->requestedBatch) return s->requestedBatch;
    uint32_t maxPaths = DEFAULT_BATCH_PATHS;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
        const size_t held = (size_t)s->capacity * s->lanesAlloc * (PATH_STATE_BYTES + (s->LP[0].orderBuf ? PATH_ORDER_BYTES : 0) + (s->LP[0].preBuf ? PATH_PRE_BYTES : 0)) + (size_t)s->fieldCap * s->fieldCount * 3 * sizeof(float) +
                            s->fanClosest * FAN_CLOSEST_BYTES + s->fanShadow * FAN_SHADOW_BYTES;
        // 3/4 of the free HBM (288 GB on an MI355X: 768M paths, C5's three
        // batches of 713M); the rest stays for the scene and other users
        const size_t fit = (size_t)((freeB + held) * 0.75 / stateBytes);
        maxPaths = (uint32_t)std::max<size_t>(TILE * TILE, std::min<size_t>(maxPaths, fit));
    }
    return maxPaths;
}

// One render call: the batches of its plan (render_plan.h), plan.lanes at a
// time, each on its lane's stream and issued bounce by bounce in lock step.
// Bounce b of a lane: one trace launch over this bounce's closest rays (work
// list qin(b), identity for b = 0) and bounce b-1's shadow rays (S((b-1) & 1)),
// then k_shade appends the next bounce's paths to qout(b) = (b & 1) ^ 1 and
// its shadow rays to S(b & 1).
// win = 0: film is the ImageBlock of the whole rectangle + border; win > 0:
// film holds one win x win window per tile of this call (mtsg_render_device_tiles)
struct RenderRun {
    mtsg_scene *s;
    const mtsg_render_params *p;
    DevIntegrator I;
    RenderPlan plan;
    float *film;
    int win;
    bool multi;
    std::chrono::steady_clock::time_point t0;
    bool count = false;
    bool fieldsOnly = false;   // multichannel without a `path` child
    bool useFinish = false;    // tail mode (k_finish)
    bool direct = false;       // direct / ao: camera rays, the fan, resolve (direct.hip)
    // the `path` integrator on a flat scene in the setup mode: k_camera and
    // k_shade write each ray's pre-record and the trace launches read it.  Not
    // the multichannel, direct / ao and myPath2_OM routes: their rays carry none.
    bool pre = false;
    // adaptive (adaptive.hip): its camera in place of k_camera, its splat in
    // place of k_splat (none in the pre-pass), rounds in place of the plan
    bool adaptive = false;
    DevAdaptive adv{};
    int blockW = 0, blockH = 0, maxBounces = 0;
    struct Lane {
        DevBatch B;
        int last = -1;
        int start = 0;
        bool open = false;
        bool finished = false;   // the tail kernel took over the batch's remaining bounces
        hipEvent_t cntEv[2] = {nullptr, nullptr};
    } lane[MTSG_MAX_LANES];
    hipEvent_t startEv = nullptr;

    // the deal key of virtual tile v, on the host
    int hostKey(int v) const { return s->tileKeys.empty() ? (int)plan.toffset + v * (int)plan.tstride : s->tileKeys[v]; }
    uint32_t *hostCnt(uint32_t l, int bb) const { return s->hostCnt + HOSTCNT_STRIDE * (2 * l + (bb & 1)); }
    // books bounce bb of lane l from its counters' copy; returns the paths it left for bounce bb + 1
    uint32_t account(uint32_t l, int bb) {
        const uint32_t *hc = hostCnt(l, bb);
        const uint32_t consumed = bb == 0 ? lane[l].B.nslots : hc[(bb & 1) ? CNT_Q1 : CNT_Q0];
        s->stats.rays_closest += consumed;
        s->stats.rays_shadow += hc[cnt_s(bb & 1)];
        s->stats.launches_trace_closest++;
        return hc[((bb & 1) ^ 1) ? CNT_Q1 : CNT_Q0];
    }
    DevBatch dev_batch(const PlanBatch &b) const {   // (in DevBatch's field order)
        return DevBatch{p->tile_x, p->tile_y, p->tile_w, p->tile_h, (int)plan.tilesX, (int)b.tile0, (int)b.ntiles,
                        (int)plan.tstride, (int)plan.toffset, PLAN_DEAL_SKEW, b.s0, b.ns, b.nslots,
                        s->tileKeys.empty() ? nullptr : s->tileKeysDev, s->cam.lens ? 1u : 0u};
    }
    DirectLaunch direct_args(uint32_t l) const {
        return DirectLaunch{s->lstream[l], &s->ds, &I, &lane[l].B, &s->LP[l], &s->fan, s->cam.has_alpha, (s->ds.has_env & 1) != 0, s->extBsdfs,
                            s->shadeGeneric ? (int)MATS_ALL : s->mats, s->emitterSet == EM_ALL, s->ext2};
    }
    AdaptiveLaunch adaptive_args(uint32_t l) const {
        return AdaptiveLaunch{s->lstream[l], &s->ds, &s->cam, &I, &lane[l].B, &s->LP[l], &adv, film, blockW, blockH};
    }
    FieldsLaunch fields(uint32_t l) const {
        return FieldsLaunch{s->lstream[l], &s->ds, &s->cam, &I, &lane[l].B, &s->LP[l], &s->aov, film, blockW, blockH, win};
    }
    // the rectangle's part of tile v: origin and size
    void tile_rect(int key, const DevBatch &B, int &x, int &y, int &w, int &h) const {
        int tx, ty;
        tile_of_key(key, B.tiles_x, tx, ty, B.skew);
        x = tx * TILE;
        y = ty * TILE;
        w = std::min(TILE, p->tile_w - x);
        h = std::min(TILE, p->tile_h - y);
    }

    // the per-render events; work the caller queued on s->stream (the film
    // memset of mtsg_render) precedes every lane's first kernel
    int open_lanes() {
        for (uint32_t l = 0; l < plan.lanes; ++l)
            for (int k = 0; k < 2; ++k)
                if (hipEventCreateWithFlags(&lane[l].cntEv[k], hipEventDisableTiming) != hipSuccess) { g_err = "event"; return MTSG_ERR_DEVICE; }
        if (plan.lanes > 1) {
            if (hipEventCreateWithFlags(&startEv, hipEventDisableTiming) != hipSuccess || hipEventRecord(startEv, s->stream) != hipSuccess) {
                g_err = "event";
                return MTSG_ERR_DEVICE;
            }
            for (uint32_t l = 1; l < plan.lanes; ++l)
                if (hipStreamWaitEvent(s->lstream[l], startEv, 0) != hipSuccess) { g_err = "stream wait"; return MTSG_ERR_DEVICE; }
        }
        return MTSG_OK;
    }

    // the copy of a bounce's queue counters that account() and the error check read
    int copy_counters(uint32_t l, int b) {
        HIP_TRY(hipMemcpyAsync(hostCnt(l, b), s->LP[l].cnt, (CNT_S1 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->lstream[l]));
        HIP_TRY(hipEventRecord(lane[l].cntEv[b & 1], s->lstream[l]));
        lane[l].last = b;
        return MTSG_OK;
    }
    // the batch needs no further bounce launches
    int end_lane(uint32_t l, int b) {
        lane[l].open = false;
        lane[l].finished = true;
        return copy_counters(l, b);
    }

    // issue bounce b of lane l: camera, reset, optional sort, trace, fields,
    // then the tail kernel or shade, then the counters' copy
    int issue_bounce(uint32_t l, int b) {
        Lane &L = lane[l];
        DevPaths &P = s->LP[l];
        hipStream_t st = s->lstream[l];
        if (b == 0) {
            HIP_TRY(hipMemsetAsync(P.cnt, 0, CNT_WORDS * sizeof(uint32_t), st));
            P.pre = pre ? P.preBuf : nullptr;
            timed_launch(s, K_CAMERA, st, [&]() {
                const dim3 g((L.B.nslots + BLOCK - 1) / BLOCK);
                if (adaptive) launch_adaptive_camera(adaptive_args(l));
                else if (s->cam.lens && pre) hipLaunchKernelGGL(k_camera_lens<true>, g, dim3(BLOCK), 0, st, s->ds, s->cam, I, L.B, P);
                else if (s->cam.lens) hipLaunchKernelGGL(k_camera_lens<false>, g, dim3(BLOCK), 0, st, s->ds, s->cam, I, L.B, P);
                else if (pre) hipLaunchKernelGGL(k_camera<true>, g, dim3(BLOCK), 0, st, s->ds, s->cam, I, L.B, P);
                else hipLaunchKernelGGL(k_camera<false>, g, dim3(BLOCK), 0, st, s->ds, s->cam, I, L.B, P);
            });
        }
        const int qin = b == 0 ? -1 : (b & 1);
        const int qout = (b & 1) ^ 1;
        hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, st, P.cnt, qout, b & 1);
        // bounce rays in direction-sorted windows (k_sortwin); the
        // camera rays keep their tile order
        DevPaths PT = P;
        PT.camEnc = (b == 0 && s->ds.camCompact) ? 1u : 0u;   // bounce 0: camera rays as k_camera stores them
        if (b >= 1 && s->rayOrder == 1) {
            timed_launch(s, K_SORT, st, [&]() {
                hipLaunchKernelGGL(k_sortwin, dim3(s->cuCount * 2), dim3(SORT_BLOCK), 0, st, P, qin);
            });
            PT.order = P.orderBuf;
        }
        timed_launch(s, K_CLOSEST, st, [&]() { launch_trace(s, count, PT, qin, b == 0 ? -1 : ((b - 1) & 1), L.B.nslots, st, pre); });
        if (multi && b == 0) {
            // the bounce-0 hits are final (the tie retrace is part of the trace
            // launch) and the work list is the identity: the field children
            if (s->aov.nf || fieldsOnly) launch_fields(fields(l));
            // no `path` child: no shading, no further bounce; the counters'
            // copy carries the traversal's error word
            if (fieldsOnly) return end_lane(l, 0);
        }
        if (direct) {
            // the fan of the camera samples (work list: the identity), one
            // trace launch over its BSDF rays (identity over slot * nb + j) and
            // its shadow rays (S0), then the sum per sample.  The shadow rays'
            // cells start at zero; the fan shares the lane's counters.
            const DevDirect &D = s->fan;
            if (D.ne) HIP_TRY(hipMemsetAsync(D.F.Lp, 0, (size_t)L.B.nslots * D.ne * sizeof(float4), st));
            timed_launch(s, K_SHADE, st, [&]() { launch_direct_shade(direct_args(l)); });
            hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, st, P.cnt, -1, -1);
            timed_launch(s, K_CLOSEST, st, [&]() { launch_trace(s, count, D.F, D.nb ? -1 : -2, 0, L.B.nslots * D.nb, st); });
            timed_launch(s, K_SHADE, st, [&]() { launch_direct_resolve(direct_args(l)); });
            return end_lane(l, 0);
        }
        if (useFinish && b >= 1) {
            // the count of this bounce's paths is known once bounce b-1 is
            // done (the GPU meanwhile runs this bounce's trace): few left ->
            // k_finish carries them to their ends in one launch
            HIP_TRY(hipEventSynchronize(L.cntEv[(b - 1) & 1]));
            const uint32_t left = account(l, b - 1);
            if (left < s->finishPaths) {
                hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, st, P.cnt, -1, -1);
                timed_launch(s, K_FINISH, st, [&]() { launch_finish(s, I, L.B, P, qin, st); });
                s->stats.launches_finish++;
                s->stats.paths_finish += left;
                return end_lane(l, b);
            }
        }
        timed_launch(s, K_SHADE, st, [&]() { launch_shade(s, I, L.B, P, b, qin, st); });
        swap_bounce(P);
        if (b + 1 >= maxBounces) L.open = false;
        return copy_counters(l, b);
    }

    // lagged check: if bounce b-1 produced nothing, bounce b was empty
    // (also for a lane that launched its last bounce b just now, so
    // every bounce is booked once: b-1 here, the last one in collect_batch)
    int check_empty(uint32_t l, int b) {
        Lane &L = lane[l];
        if (b >= 1 && L.last == b && !useFinish) {
            HIP_TRY(hipEventSynchronize(L.cntEv[(b - 1) & 1]));
            if (account(l, b - 1) == 0) L.open = false;
        }
        return MTSG_OK;
    }

    // close lane l's batch: the last bounce's shadow rays, then the splat
    int close_batch(uint32_t l) {
        Lane &L = lane[l];
        DevPaths &P = s->LP[l];
        hipStream_t st = s->lstream[l];
        if (L.last >= 0 && !L.finished) {
            hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, st, P.cnt, -1, -1);
            timed_launch(s, K_SHADOW, st, [&]() { launch_trace(s, count, P, -2, L.last & 1, 0u, st, pre); });
            s->stats.launches_trace_shadow++;
            // the error word again, after this launch: a traversal error of
            // the last bounce's shadow rays fails the render too (the copy
            // of bounce L.last's counters was taken before this launch)
            HIP_TRY(hipMemcpyAsync(hostCnt(l, L.last) + CNT_ERR, P.cnt + CNT_ERR, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(L.cntEv[L.last & 1], st));
        }
        timed_launch(s, K_SPLAT, st, [&]() {
            if (adaptive) { if (!adv.prepass) launch_adaptive_splat(adaptive_args(l)); }
            else if (multi) launch_splat_multi(fields(l));
            else launch_splat(s, I, L.B, P, film, blockW, blockH, win, st);
        });
        if (!adaptive) s->stats.samples += (uint64_t)L.B.nslots;
        return MTSG_OK;
    }

    // collect the nb batches in flight: the last bounce's accounting and the
    // error word, then the tile callbacks and the debug dumps
    int collect_batches(uint32_t nb) {
        for (uint32_t l = 0; l < nb; ++l) {
            Lane &L = lane[l];
            if (L.last < 0) continue;
            HIP_TRY(hipEventSynchronize(L.cntEv[L.last & 1]));
            if (fieldsOnly || direct) {
                // one closest launch per batch, one camera ray per sample inside the rectangle
                s->stats.launches_trace_closest++;
                for (int tl = 0; tl < L.B.ntiles; ++tl) {
                    int x, y, w, h;
                    tile_rect(hostKey(L.B.tile0 + tl), L.B, x, y, w, h);
                    s->stats.rays_closest += (uint64_t)w * h * L.B.ns;
                }
                if (direct) {
                    // the fan's launch: the BSDF rays k_direct_shade sent (its
                    // count in Q1) and the shadow rays it appended (S0)
                    s->stats.launches_trace_closest++;
                    s->stats.rays_closest += hostCnt(l, 0)[CNT_Q1];
                    s->stats.rays_shadow += hostCnt(l, 0)[CNT_S0];
                }
            } else {
                account(l, L.last);
            }
            // the error word is sticky within the batch: the last copy holds it
            const uint32_t err = hostCnt(l, L.last)[CNT_ERR];
            if (err & CNT_ERR_TRAVERSAL) {
                g_err = traversal_error;
                return MTSG_ERR_TRAVERSAL;
            }
            if (err) {
                g_err = dim_error(s->samplerType);
                return MTSG_ERR_INVALID;
            }
        }
        if (s->tileFn && !adaptive) {   // (adaptive: a tile is complete when its last pixel stops, run_adaptive)
            // the tiles whose last samples this batch splatted are complete
            for (uint32_t l = 0; l < nb; ++l) {
                HIP_TRY(hipStreamSynchronize(s->lstream[l]));
                const DevBatch &B = lane[l].B;
                if (B.s0 + B.ns < p->spp) continue;
                for (int tl = 0; tl < B.ntiles; ++tl) {
                    const int key = hostKey(B.tile0 + tl);
                    int x, y, w, h;
                    tile_rect(key, B, x, y, w, h);
                    s->tileFn(s->tileUser, key, p->tile_x + x, p->tile_y + y, w, h);
                }
            }
        }
        int rc = MTSG_OK;
        if (s->dumpMulti) rc = dump_multi();
        if (rc == MTSG_OK && s->dumpL) rc = dump_radiance();
        return rc;
    }

    // debug dumps (single batch, one lane): f(slot, i) for every slot of the
    // batch inside the rectangle, i the index of its sample in [tile_h][tile_w][spp]
    template <class F>
    void for_each_sample(F f) const {
        const DevBatch &B = lane[0].B;
        for (uint32_t slot = 0; slot < B.nslots; ++slot) {
            const uint32_t pix = slot & (TILE * TILE - 1), rest = slot >> 8;
            const uint32_t sl = rest % B.ns, tl = rest / B.ns;
            int tx, ty;
            tile_of_key(hostKey(B.tile0 + (int)tl), B.tiles_x, tx, ty, B.skew);
            int lx, ly;
            tile_pix(pix, lx, ly);
            const int x = tx * TILE + lx, y = ty * TILE + ly;
            if (x >= p->tile_w || y >= p->tile_h) continue;
            f(slot, ((size_t)y * p->tile_w + x) * p->spp + B.s0 + sl);
        }
    }
    // the batch's per-slot children: the `path` child and alpha from L, the
    // fields from their planes
    int dump_multi() const {
        const uint32_t n = lane[0].B.nslots;
        const DevAov &A = s->aov;
        std::vector<float4> L(n);
        std::vector<float> F((size_t)3 * A.nf * n);
        HIP_TRY(hipMemcpyAsync(L.data(), s->LP[0].L, n * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
        for (int k = 0; k < 3 * A.nf; ++k)
            HIP_TRY(hipMemcpyAsync(F.data() + (size_t)k * n, A.planes + (size_t)k * A.cap, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        const size_t per = (size_t)3 * A.m + 1;
        for_each_sample([&](uint32_t slot, size_t i) {
            float *o = s->dumpMulti + i * per;
            if (A.pathChild >= 0) { o[3 * A.pathChild] = L[slot].x; o[3 * A.pathChild + 1] = L[slot].y; o[3 * A.pathChild + 2] = L[slot].z; }
            for (int f = 0; f < A.nf; ++f)
                for (int c = 0; c < 3; ++c) o[3 * A.child[f] + c] = F[(size_t)(3 * f + c) * n + slot];
            o[3 * A.m] = L[slot].w;
        });
        return MTSG_OK;
    }
    // the batch's per-slot radiance
    int dump_radiance() const {
        const uint32_t n = lane[0].B.nslots;
        std::vector<float4> L(n);
        HIP_TRY(hipMemcpyAsync(L.data(), s->LP[0].L, n * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for_each_sample([&](uint32_t slot, size_t i) {
            float *o = s->dumpL + i * 4;
            o[0] = L[slot].x; o[1] = L[slot].y; o[2] = L[slot].z; o[3] = L[slot].w;
        });
        return MTSG_OK;
    }

    // every error in here returns at once; finish() then drains the lanes
    // and destroys the per-render events, whatever happened
    int run_batches() {
        const uint32_t nl = plan.lanes;
        for (size_t k0 = 0; k0 < plan.batches.size(); k0 += nl) {
            if (s->cancel.load()) { g_err = "cancelled"; return MTSG_ERR_CANCELLED; }
            const uint32_t nb = (uint32_t)std::min<size_t>(nl, plan.batches.size() - k0);
            for (uint32_t l = 0; l < nb; ++l) {
                Lane &L = lane[l];
                L.B = dev_batch(plan.batches[k0 + l]);
                L.last = -1;
                L.open = true;
                L.finished = false;
                // staggered lanes: lane l starts `stagger` bounces after lane
                // l-1, so its early, full launches overlap the other lanes'
                // late, tail-bound ones
                L.start = (int)l * s->stagger;
            }
            int rc;
            if ((rc = run_bounces(nb)) != MTSG_OK) return rc;
        }
        return MTSG_OK;
    }

    // the nb batches in lane[0..nb) from their camera rays to their splat
    int run_bounces(uint32_t nb) {
        int rc;
        for (int gb = 0;; ++gb) {
            // cancel() between bounces (the whole frame is usually one batch)
            if (s->cancel.load()) { g_err = "cancelled"; return MTSG_ERR_CANCELLED; }
            for (uint32_t l = 0; l < nb; ++l)
                if (lane[l].open && gb >= lane[l].start && (rc = issue_bounce(l, gb - lane[l].start)) != MTSG_OK) return rc;
            bool any = false;
            for (uint32_t l = 0; l < nb; ++l) {
                if ((rc = check_empty(l, gb - lane[l].start)) != MTSG_OK) return rc;
                any |= lane[l].open;
            }
            if (!any) break;
        }
        for (uint32_t l = 0; l < nb; ++l)
            if ((rc = close_batch(l)) != MTSG_OK) return rc;
        return collect_batches(nb);
    }

    // one batch on lane 0
    int run_single(const DevBatch &B) {
        Lane &L = lane[0];
        L.B = B;
        L.last = -1;
        L.open = true;
        L.finished = false;
        L.start = 0;
        return run_bounces(1);
    }

    // An adaptive render (adaptive.hip, adaptive_plan.h): the pre-pass, then
    // rounds over the tiles that still hold an active pixel.  keys: the call's
    // deal keys; keysDev: room for them on the device; maxPaths: the memory fit;
    // Ipre / preB: the integrator constants and the batch of the pre-pass strip.
    int run_adaptive(std::vector<int32_t> keys, int32_t *keysDev, uint32_t maxPaths, const DevIntegrator &Ipre, const DevBatch &preB,
                     uint32_t later) {
        int rc;
        mtsg_adaptive_result &res = s->adaptiveResult;
        const DevIntegrator Irounds = I;
        // pre-pass (adaptive.cpp:125-159): the strip's luminances, summed in
        // float in sample order on the host, so every GPU of a split render
        // holds the same value
        {
            I = Ipre;
            adv.prepass = 1;
            rc = run_single(preB);
            I = Irounds;
            adv.prepass = 0;
            if (rc != MTSG_OK) return rc;
            std::vector<float4> L(preB.nslots);
            HIP_TRY(hipMemcpyAsync(L.data(), s->LP[0].L, L.size() * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            std::vector<float> lum(ADAPTIVE_PREPASS_SAMPLES, 0.0f);
            for (uint32_t slot = 0; slot < preB.nslots; ++slot) {
                int lx, ly;
                tile_pix(slot & (TILE * TILE - 1), lx, ly);
                const uint32_t i = (((slot >> 8) * TILE) + (uint32_t)ly) * TILE + (uint32_t)lx;
                if (i < ADAPTIVE_PREPASS_SAMPLES) lum[i] = L[slot].x * 0.212671f + L[slot].y * 0.715160f + L[slot].z * 0.072169f;
            }
            float sum = 0.0f;
            for (float v : lum) sum += v;
            adv.avgLum = sum / (float)ADAPTIVE_PREPASS_SAMPLES;
            res.average_luminance = adv.avgLum;
            double m = 0, q = 0;
            for (float v : lum) m += v;
            m /= ADAPTIVE_PREPASS_SAMPLES;
            for (float v : lum) q += (v - m) * (v - m);
            res.luminance_variance = (float)(q / (ADAPTIVE_PREPASS_SAMPLES - 1));
        }
        std::vector<uint32_t> active(plan.allTiles, 0u);
        std::vector<int32_t> finished;
        const uint32_t N = adv.baseCount, cap = I.spp;
        for (uint32_t r = 0; !keys.empty(); ++r) {
            uint32_t s0, ns;
            if (!adaptive_round(N, cap, later, r, s0, ns)) { g_err = "adaptive: pixels left active past the cap"; return MTSG_ERR_DEVICE; }
            // cancel() between rounds, as between batches
            if (s->cancel.load()) { g_err = "cancelled"; return MTSG_ERR_CANCELLED; }
            HIP_TRY(hipMemcpyAsync(keysDev, keys.data(), keys.size() * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
            const RenderPlan rp = adaptive_round_plan(p->tile_w, p->tile_h, (uint32_t)keys.size(), s0, ns, maxPaths);
            for (const PlanBatch &b : rp.batches) {
                if (s->cancel.load()) { g_err = "cancelled"; return MTSG_ERR_CANCELLED; }
                DevBatch B = dev_batch(b);
                B.tstride = 1;
                B.toffset = 0;
                B.keys = keysDev;
                if (B.nslots > s->capacity) { g_err = "adaptive: a round's batch exceeds the path state"; return MTSG_ERR_DEVICE; }
                if ((rc = run_single(B)) != MTSG_OK) return rc;
            }
            // the tiles whose last pixel stopped leave the list
            HIP_TRY(hipMemcpyAsync(active.data(), adv.tileActive, active.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            adaptive_compact(keys, active, finished);
            res.rounds = r + 1;
            if (s->tileFn)
                for (int32_t key : finished) {
                    int x, y, w, h;
                    tile_rect(key, lane[0].B, x, y, w, h);
                    s->tileFn(s->tileUser, key, p->tile_x + x, p->tile_y + y, w, h);
                }
        }
        // the per-pixel counts of the rectangle, row-major
        std::vector<uint32_t> status((size_t)plan.allTiles * TILE * TILE);
        HIP_TRY(hipMemcpy(status.data(), adv.status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        s->adaptiveCounts.assign((size_t)p->tile_w * p->tile_h, 0u);
        uint64_t total = 0;
        for (uint32_t key = 0; key < plan.allTiles; ++key) {
            int tx, ty;
            tile_of_key((int)key, (int)plan.tilesX, tx, ty, PLAN_DEAL_SKEW);
            for (uint32_t pix = 0; pix < (uint32_t)(TILE * TILE); ++pix) {
                int lx, ly;
                tile_pix(pix, lx, ly);
                const int x = tx * TILE + lx, y = ty * TILE + ly;
                if (x >= p->tile_w || y >= p->tile_h) continue;
                const uint32_t c = status[(size_t)key * TILE * TILE + pix] & ~ADAPTIVE_DONE;
                s->adaptiveCounts[(size_t)y * p->tile_w + x] = c;
                total += c;
            }
        }
        res.total_samples = total;
        s->stats.samples = total;
        return MTSG_OK;
    }

    // drain every lane (also after an error or a cancel: the caller may free
    // the film as soon as this returns), release the per-render events and
    // consume the cancel flag; then the timings and counters of a good render
    int finish(int result) {
        hipError_t e = hipSuccess;
        for (uint32_t l = 0; l < plan.lanes; ++l) {
            const hipError_t el = hipStreamSynchronize(s->lstream[l]);
            if (e == hipSuccess) e = el;
            for (int k = 0; k < 2; ++k)
                if (lane[l].cntEv[k]) hipEventDestroy(lane[l].cntEv[k]);
        }
        if (startEv) hipEventDestroy(startEv);
        // the cancel flag is consumed (cleared) when a render returns, so a
        // cancel that races with the start of a render is not lost
        s->cancel.store(0);
        if (e != hipSuccess) { g_err = std::string("render: ") + hipGetErrorString(e); return MTSG_ERR_DEVICE; }
        e = hipGetLastError();
        if (e != hipSuccess) { g_err = std::string("kernel launch: ") + hipGetErrorString(e); return MTSG_ERR_DEVICE; }
        if (result != MTSG_OK) return result;
        mtsg_stats &st = s->stats;
        // samples actually inside the rectangle (all tiles of this call)
        if (plan.tstride == 1 && s->tileKeys.empty() && !adaptive) st.samples = (uint64_t)p->tile_w * p->tile_h * p->spp;
        if (s->flags & MTSG_FLAG_TIMING) {
            // in the order of K_CAMERA .. K_SORT
            double *const sums[] = {&st.ms_camera, &st.ms_trace_closest, &st.ms_trace_shadow, &st.ms_shade, &st.ms_splat, &st.ms_finish, &st.ms_sort};
            for (auto &te : s->timed) {
                float ms = 0;
                hipEventElapsedTime(&ms, s->evPool[te.second], s->evPool[te.second + 1]);
                *sums[te.first] += ms;
            }
        }
        if (count) {
            // the traversal counters, by the names of kernels.h (CTR_*)
            unsigned long long c[CTR_WORDS];
            HIP_TRY(hipMemcpy(c, s->LP[0].ctr, sizeof(c), hipMemcpyDeviceToHost));
            const unsigned long long *sh = c + CTR_SHADOW;
            st.nodes_visited = c[CTR_NODES];                     st.shadow_nodes_visited = sh[CTR_NODES];
            st.leaf_refs = c[CTR_REFS];                          st.shadow_leaf_refs = sh[CTR_REFS];
            st.tri_tests = c[CTR_TESTS];                         st.shadow_tri_tests = sh[CTR_TESTS];
            st.wave_node_iters = c[CTR_WAVE_NODE_ITERS];         st.shadow_wave_node_iters = sh[CTR_WAVE_NODE_ITERS];
            st.wave_test_iters = c[CTR_WAVE_TEST_ITERS];         st.shadow_wave_test_iters = sh[CTR_WAVE_TEST_ITERS];
            st.wave_steps = c[CTR_WAVE_STEPS];                   st.shadow_wave_steps = sh[CTR_WAVE_STEPS];
            st.wave_active_lanes = c[CTR_WAVE_ACTIVE];           st.shadow_wave_active_lanes = sh[CTR_WAVE_ACTIVE];
            st.iter_max_closest = c[CTR_ITER_MAX];               st.iter_max_shadow = sh[CTR_ITER_MAX];
            for (int k = 0; k < CTR_HIST_BINS; ++k) {
                st.iter_hist_closest[k] = c[CTR_HIST_CLOSEST + k];
                st.iter_hist_shadow[k] = c[CTR_HIST_SHADOW + k];
            }
            const unsigned long long *rec = c + CTR_STRAGGLER_RECORDS;
            s->stragglers.assign(rec, rec + CTR_STRAGGLER_WORDS * std::min<unsigned long long>(c[CTR_STRAGGLERS], STRAGGLER_MAX));
            st.instance_visits = c[CTR_INST_VISITS];             st.shadow_instance_visits = c[CTR_INST_VISITS + 1];
            st.instance_rejects = c[CTR_INST_REJECTS];
            st.instance_prefiltered = c[CTR_INST_PREFILTERED];
            st.tie_retraces = c[CTR_TIE_RETRACES];
            st.guard_rays_closest = c[CTR_GUARD_RAYS];           st.guard_rays_shadow = c[CTR_GUARD_RAYS + 1];
            st.guard_steps_closest = c[CTR_GUARD_STEPS];         st.guard_steps_shadow = c[CTR_GUARD_STEPS + 1];
            st.restarts_closest = c[CTR_RESTARTS];               st.restarts_shadow = c[CTR_RESTARTS + 1];
        }
        st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return MTSG_OK;
    }
};

// A render call on a handle with an adaptive descriptor (mtsg.h
// mtsg_scene_set_adaptive): its checks, the per-pixel state, then
// RenderRun::run_adaptive.  The state is allocated before the memory fit, so
// the fit sees what is left, and freed when the call returns.
int render_adaptive(mtsg_scene *s, const mtsg_render_params *p, float *film, int win, bool multi) {
    const mtsg_adaptive_desc &d = s->adaptive;
    if (p->integrator != MTSG_INTEGRATOR_PATH) { g_err = "adaptive: the child integrator must be `path`"; return MTSG_ERR_INVALID; }
    if (multi || s->aovOn) { g_err = "adaptive: not inside or around `multichannel`"; return MTSG_ERR_INVALID; }
    if (s->dumpL) { g_err = "adaptive: mtsg_render_samples has no fixed shape under a per-pixel sample count"; return MTSG_ERR_INVALID; }
    if (win) { g_err = "adaptive: the tile-window entries are not offered (use mtsg_render / mtsg_render_device)"; return MTSG_ERR_INVALID; }
    if (s->samplerType != MTSG_SAMPLER_INDEPENDENT) {
        g_err = "The error-controlling integrator should only be used in conjunction with the independent sampler";
        return MTSG_ERR_INVALID;
    }
    if (p->spp != d.base_count) { g_err = "adaptive: params.spp must equal the descriptor's base_count"; return MTSG_ERR_INVALID; }
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t N = d.base_count, cap = adaptive_cap(d.max_sample_factor, N);
    int32_t row0, rows;
    if (!adaptive_prepass_rows((uint64_t)s->cam.film_w * s->cam.film_h, cap, row0, rows)) {
        g_err = "adaptive: film size x sample cap leaves no sample ids for the pre-pass";
        return MTSG_ERR_INVALID;
    }
    // the call's tiles: its share of the deal, or the listed keys
    RenderPlan plan = plan_render(p->tile_w, p->tile_h, 1u, p->tile_stride, p->tile_offset, (uint32_t)s->tileKeys.size(), PLAN_TILE_SLOTS, 1u, true);
    for (int32_t k : s->tileKeys)
        if ((uint32_t)k >= plan.allTiles) { g_err = "tile list: a deal key lies outside the rectangle's tiles"; return MTSG_ERR_INVALID; }
    std::vector<int32_t> keys(plan.ntiles);
    for (uint32_t v = 0; v < plan.ntiles; ++v) keys[v] = s->tileKeys.empty() ? (int32_t)(plan.toffset + v * plan.tstride) : s->tileKeys[v];
    // per-pixel state: status, mean, meanSqr and the parked K x K x CH window
    const int K = 2 * s->cam.border + 1, KT = K == 5 ? 5 : K <= 3 ? 3 : 9, CH = s->cam.has_alpha ? 5 : 4;
    const size_t stride = (size_t)plan.allTiles * TILE * TILE;
    std::vector<void *> allocs;
    struct Free {
        std::vector<void *> &a;
        ~Free() { for (void *q : a) hipFree(q); }
    } freeAll{allocs};
    auto alloc = [&](size_t bytes, void **q) -> int {
        HIP_TRY(hipMalloc(q, bytes));
        allocs.push_back(*q);
        return MTSG_OK;
    };
    DevAdaptive A{};
    int32_t *keysDev = nullptr;
    if ((rc = alloc(stride * sizeof(uint32_t), (void **)&A.status)) != MTSG_OK) return rc;
    if ((rc = alloc(stride * sizeof(float), (void **)&A.mean)) != MTSG_OK) return rc;
    if ((rc = alloc(stride * sizeof(float), (void **)&A.meanSqr)) != MTSG_OK) return rc;
    if ((rc = alloc(stride * sizeof(float) * KT * KT * CH, (void **)&A.win)) != MTSG_OK) return rc;
    if ((rc = alloc(plan.allTiles * sizeof(uint32_t), (void **)&A.tileActive)) != MTSG_OK) return rc;
    if ((rc = alloc(plan.allTiles * sizeof(int32_t), (void **)&keysDev)) != MTSG_OK) return rc;
    HIP_TRY(hipMemsetAsync(A.status, 0, stride * sizeof(uint32_t), s->stream));
    HIP_TRY(hipMemsetAsync(A.tileActive, 0, plan.allTiles * sizeof(uint32_t), s->stream));
    A.stride = stride;
    A.maxError = d.max_error;
    A.quantile = d.quantile;
    A.baseCount = N;
    A.limit = (uint32_t)std::min<uint64_t>((uint64_t)std::max(d.max_sample_factor, 0) * N, cap);
    const uint32_t maxPaths = fit_paths(s, PATH_STATE_BYTES + (s->LP[0].orderBuf ? PATH_ORDER_BYTES : 0) + (s->LP[0].preBuf ? PATH_PRE_BYTES : 0));
    // the pre-pass strip: 16 columns, one sample per "pixel", ids past the film's
    const uint32_t preTiles = ((uint32_t)rows + TILE - 1) / TILE;
    const DevBatch preB{0, row0, TILE, rows, 1, 0, (int)preTiles, 1, 0, PLAN_DEAL_SKEW, 0u, 1u, preTiles * (uint32_t)(TILE * TILE), nullptr,
                        s->cam.lens ? 1u : 0u};
    // the largest round batch, for the path state
    // (a later round lists fewer tiles and may cut them into larger groups than
    // the first: what bounds every batch is the lane's budget and the round itself)
    uint32_t s0, ns, need = preB.nslots;
    const uint64_t lanePaths = std::max<uint64_t>(PLAN_TILE_SLOTS, std::min<uint64_t>(maxPaths, PLAN_MAX_RAYS));
    for (uint32_t r = 0; r < 2 && adaptive_round(N, cap, s->adaptiveRound, r, s0, ns); ++r)
        need = std::max<uint32_t>(need, (uint32_t)std::min<uint64_t>(lanePaths, (uint64_t)plan.ntiles * ns * PLAN_TILE_SLOTS));
    if ((rc = ensure_batch(s, need, 1)) != MTSG_OK) return rc;
    // the sample id's stride is the cap: sample s of a pixel is sample s of
    // the plain `path` render with spp = cap
    DevIntegrator I{p->max_depth, p->rr_depth, p->strict_normals, p->hide_emitters, cap, p->seed, (uint32_t)s->cam.film_w, make_sampler(s, cap)};
    DevIntegrator Ipre = I;
    Ipre.spp = 1;
    Ipre.film_w = TILE;
    memset(&s->stats, 0, sizeof(s->stats));
    s->wtLaunches = 0;
    if ((s->flags & MTSG_FLAG_WAVETIME) && !s->waveTimes)
        HIP_TRY(hipMalloc((void **)&s->waveTimes, (size_t)WT_WORDS * s->traceGrid * WT_MAX_LAUNCHES * sizeof(unsigned long long)));
    s->evUsed = 0;
    s->timed.clear();
    const bool count = (s->flags & MTSG_FLAG_COUNT) != 0;
    if (count) HIP_TRY(hipMemsetAsync(s->LP[0].ctr, 0, CTR_WORDS * sizeof(unsigned long long), s->stream));
    // the differentials are always carried: bounce 0 would recompute them with
    // the sample-id stride, which is not their scale here
    // (for this call only: the guard puts the handle's mode back on every way out)
    struct KeepDiffs {
        mtsg_scene *s;
        int diffs, envDiffs, camDiffs;
        explicit KeepDiffs(mtsg_scene *sc) : s(sc), diffs(sc->ds.cam_diffs), envDiffs(sc->ds.cam_env_diffs), camDiffs(sc->cam.diffs) {}
        ~KeepDiffs() {
            s->ds.cam_diffs = diffs;
            s->ds.cam_env_diffs = envDiffs;
            s->cam.diffs = camDiffs;
        }
    } keepDiffs(s);
    if (s->hasEnvmap) {
        s->ds.cam_diffs = 1;
        s->ds.cam_env_diffs = 0;
        s->cam.diffs = 1;
    }
    s->adaptiveHave = false;
    s->adaptiveResult = mtsg_adaptive_result{};
    s->adaptiveResult.quantile = d.quantile;
    s->adaptiveResult.width = p->tile_w;
    s->adaptiveResult.height = p->tile_h;
    plan.lanes = 1;
    RenderRun R{s, p, I, std::move(plan), film, 0, false, t0};
    R.count = count;
    R.blockW = p->tile_w + 2 * s->cam.border;
    R.blockH = p->tile_h + 2 * s->cam.border;
    R.maxBounces = p->max_depth > 0 ? p->max_depth : 1 << 30;
    R.useFinish = s->finishPaths > 0 && !count && !s->knobs;
    R.adaptive = true;
    R.adv = A;
    rc = R.open_lanes();
    if (rc == MTSG_OK) rc = R.run_adaptive(std::move(keys), keysDev, maxPaths, Ipre, preB, s->adaptiveRound);
    rc = R.finish(rc);
    s->adaptiveHave = rc == MTSG_OK;
    return rc;
}

// the checks and sizing of a render call, then its RenderRun
int render_impl(mtsg_scene *s, const mtsg_render_params *p, float *film, int win = 0, bool multi = false) {
    int rc;
    if ((rc = validate(p, s)) != MTSG_OK) return rc;
    if (s->adaptiveOn) return render_adaptive(s, p, film, win, multi);
    // a handle with a multichannel child set renders through the *_multi
    // entries only (3m + 2 floats per texel), a plain handle through the others
    if (s->aovOn && !multi) {
        g_err = "the scene's integrator is multichannel: use the _multi render entries (channels are not dropped)";
        return MTSG_ERR_INVALID;
    }
    if (multi && !s->aovOn) { g_err = "no multichannel child set is active (mtsg_scene_set_aov)"; return MTSG_ERR_INVALID; }
    if (multi && p->integrator != MTSG_INTEGRATOR_PATH) { g_err = "multichannel: only `path` and `field` children"; return MTSG_ERR_INVALID; }
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const bool count = (s->flags & MTSG_FLAG_COUNT) != 0;
    // direct / ao: the fan of ne shadow and nb BSDF rays per camera sample
    const bool direct = p->integrator == MTSG_INTEGRATOR_DIRECT || p->integrator == MTSG_INTEGRATOR_AO;
    uint32_t ne, nb;
    fan_counts(s, p, ne, nb);
    // bytes of state per path: the field planes join it while fields are
    // active, the fan's rays and cells in a direct / ao render
    const uint32_t maxPaths = fit_paths(s, PATH_STATE_BYTES + (s->rayOrder == 1 || s->LP[0].orderBuf ? PATH_ORDER_BYTES : 0) +
                                               (s->rayPresetupOpt || s->LP[0].preBuf ? PATH_PRE_BYTES : 0) + (multi ? (size_t)s->aov.nf * 3 * sizeof(float) : 0) + fan_bytes(ne, nb));
    if ((s->dumpL || s->dumpMulti) && (uint64_t)p->tile_w * p->tile_h * p->spp > maxPaths) { g_err = "render_samples: tile does not fit one batch"; return MTSG_ERR_INVALID; }
    // The debug and counting modes use one lane (multichannel too: one set of
    // field planes; direct / ao: one set of fan buffers)
    RenderPlan plan = plan_render(p->tile_w, p->tile_h, p->spp, p->tile_stride, p->tile_offset, (uint32_t)s->tileKeys.size(), maxPaths,
                                  (uint32_t)s->lanes, s->dumpL || s->dumpMulti || count || multi || direct, direct ? ne + nb : 1u);
    for (int32_t k : s->tileKeys)
        if ((uint32_t)k >= plan.allTiles) { g_err = "tile list: a deal key lies outside the rectangle's tiles"; return MTSG_ERR_INVALID; }
    if (direct && s->dumpL && plan.batches.size() > 1) { g_err = "render_samples: tile does not fit one batch"; return MTSG_ERR_INVALID; }
    if ((rc = ensure_batch(s, plan.tilesPerBatch * plan.sppPerBatch * TILE * TILE, (int)plan.lanes)) != MTSG_OK) return rc;
    if (direct) {
        if ((rc = ensure_fan(s, (size_t)plan.tilesPerBatch * plan.sppPerBatch * TILE * TILE, ne, nb)) != MTSG_OK) return rc;
        DevDirect &D = s->fan;
        D.ao = p->integrator == MTSG_INTEGRATOR_AO ? 1 : 0;
        D.ne = ne;
        D.nb = nb;
        D.rayLength = s->direct.ao_ray_length;
        // MIDirectIntegrator::configure (direct.cpp:128-136)
        D.weightBSDF = 1 / (float)nb;
        D.weightLum = 1 / (float)ne;
        D.fracBSDF = nb / (float)(ne + nb);
        D.fracLum = ne / (float)(ne + nb);
        D.arrays = fan_arrays(ne, nb);
        D.F.cnt = s->LP[0].cnt;
        D.F.ctr = s->LP[0].ctr;
    }
    if (multi) {
        if ((rc = ensure_fields(s)) != MTSG_OK) return rc;
        s->aov.planes = s->fieldPlanes;
        s->aov.cap = s->fieldCap;
    }
    DevIntegrator I{p->max_depth, p->rr_depth, p->strict_normals, p->hide_emitters, p->spp, p->seed, (uint32_t)s->cam.film_w,
                    make_sampler(s, p->spp)};
    I.om = p->integrator == MTSG_INTEGRATOR_PATH2_OM ? 1 : 0;
    I.om_strategy = p->om_strategy;
    I.om_mis = p->om_mis;
    I.om_jitter = p->om_jitter;
    memset(&s->stats, 0, sizeof(s->stats));
    s->wtLaunches = 0;
    if ((s->flags & MTSG_FLAG_WAVETIME) && !s->waveTimes)
        HIP_TRY(hipMalloc((void **)&s->waveTimes, (size_t)WT_WORDS * s->traceGrid * WT_MAX_LAUNCHES * sizeof(unsigned long long)));
    s->evUsed = 0;
    s->timed.clear();
    if (count) HIP_TRY(hipMemsetAsync(s->LP[0].ctr, 0, CTR_WORDS * sizeof(unsigned long long), s->stream));
    RenderRun R{s, p, I, std::move(plan), film, win, multi, t0};
    R.count = count;
    R.fieldsOnly = multi && s->aov.pathChild < 0;
    R.blockW = p->tile_w + 2 * s->cam.border;
    R.blockH = p->tile_h + 2 * s->cam.border;
    // myPath2_OM shades depths 1..maxDepthEye and one more launch books the
    // emitters its last BSDF rays found
    R.maxBounces = I.om ? p->max_depth + 1 : (p->max_depth > 0 ? p->max_depth : 1 << 30);
    // tail mode (k_finish): one lane, not in the instrumented or myPath2_OM modes
    R.useFinish = s->finishPaths > 0 && R.plan.lanes == 1 && !count && !I.om && !s->knobs && !direct;
    R.direct = direct;
    R.pre = presetup_applies(s) && !multi && !direct && !I.om;
    if (direct) R.maxBounces = 1;
    rc = R.open_lanes();
    if (rc == MTSG_OK) rc = R.run_batches();
    return R.finish(rc);
}

// floats of the ImageBlock of a call's rectangle + border: rgb, alpha, weight,
// or the 3m + 2 channels of the multichannel child set
size_t block_floats(const mtsg_scene *s, const mtsg_render_params *p, bool multi) {
    return (size_t)(p->tile_w + 2 * s->cam.border) * (p->tile_h + 2 * s->cam.border) * (multi ? 3 * (size_t)s->aov.m + 2 : 5);
}
// mtsg_render / mtsg_render_multi: a device block, cleared, rendered, copied to `out`
int render_to_host(mtsg_scene *s, const mtsg_render_params *p, float *out, bool multi) {
    int rc;
    if ((rc = validate(p, s)) != MTSG_OK) return rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const size_t bytes = block_floats(s, p, multi) * sizeof(float);
    float *film = nullptr;
    HIP_TRY(hipMalloc((void **)&film, bytes));
    hipError_t e = hipMemsetAsync(film, 0, bytes, s->stream);
    if (e != hipSuccess) { hipFree(film); g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    rc = render_impl(s, p, film, 0, multi);
    if (rc == MTSG_OK) {
        e = hipMemcpy(out, film, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { g_err = hipGetErrorString(e); rc = MTSG_ERR_DEVICE; }
    }
    hipFree(film);
    return rc;
}
// mtsg_render_samples / mtsg_render_samples_multi: the render above into a
// block that is dropped, with the per-sample dump (RenderRun::dump_*) into `out`
int render_samples(mtsg_scene *s, const mtsg_render_params *p, float *out, bool multi) {
    int rc;
    if ((rc = validate(p, s)) != MTSG_OK) return rc;
    float *&dump = multi ? s->dumpMulti : s->dumpL;
    std::vector<float> block(block_floats(s, p, multi));
    dump = out;
    rc = render_to_host(s, p, block.data(), multi);
    dump = nullptr;
    return rc;
}

}  // namespace

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

int mtsg_device_pci_id(int device, char *buf, int len) {
    if (!buf || len < 13) { g_err = "mtsg_device_pci_id: buffer too small"; return MTSG_ERR_INVALID; }
    if (hipDeviceGetPCIBusId(buf, len, device) != hipSuccess) { g_err = "hipDeviceGetPCIBusId failed"; return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

int mtsg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int gfx950 = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++gfx950;
    }
    return gfx950;
}

int mtsg_scene_create(const mtsg_scene_desc *d, int device, mtsg_scene **out) {
    if (!d || !out) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    *out = nullptr;
    if (d->abi_version != MTSG_ABI_VERSION) { g_err = "ABI version mismatch"; return MTSG_ERR_INVALID; }
    if (d->n_prims != d->n_triangles + d->n_rects + d->n_instances || d->n_nodes == 0 || d->n_emitters == 0) {
        g_err = "inconsistent scene description";
        return MTSG_ERR_INVALID;
    }
    if (d->camera.border > MAX_BORDER) { g_err = "reconstruction filter radius too large (border > 4)"; return MTSG_ERR_INVALID; }
    if (d->camera.sensor_type != MTSG_SENSOR_PERSPECTIVE && d->camera.sensor_type != MTSG_SENSOR_THINLENS) {
        g_err = "unknown sensor type";
        return MTSG_ERR_INVALID;
    }
    if (d->camera.sensor_type == MTSG_SENSOR_THINLENS) {
        if (!(d->camera.aperture_radius > 0) || !(d->camera.focus_distance > 0)) {
            g_err = "thinlens sensor: aperture_radius and focus_distance must be > 0";
            return MTSG_ERR_INVALID;
        }
        if (d->om) { g_err = "myPath2_OM scenes take the perspective sensor only"; return MTSG_ERR_INVALID; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_err = "no such HIP device";
        return MTSG_ERR_NODEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_err = std::string("device is not gfx950: ") + prop.gcnArchName;
        return MTSG_ERR_NODEVICE;
    }
    auto *s = new mtsg_scene();
    s->device = device;
    auto fail = [&](int rc) { mtsg_scene_destroy(s); return rc; };
    if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; delete s; return MTSG_ERR_DEVICE; }
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { g_err = "stream"; delete s; return MTSG_ERR_DEVICE; }
    s->cuCount = prop.multiProcessorCount;
    // ---- convert + upload (host-side SoA -> device layout)
    std::vector<float4> vpos(d->n_vertices), vnrm(d->n_vertices);
    for (uint32_t i = 0; i < d->n_vertices; ++i) {
        vpos[i] = make_float4(d->vtx_pos[3 * i], d->vtx_pos[3 * i + 1], d->vtx_pos[3 * i + 2], 0.f);
        vnrm[i] = make_float4(d->vtx_nrm[3 * i], d->vtx_nrm[3 * i + 1], d->vtx_nrm[3 * i + 2], 0.f);
    }
    std::vector<uint4> tidx(d->n_triangles);
    for (uint32_t t = 0; t < d->n_triangles; ++t)
        tidx[t] = make_uint4(d->tri_idx[3 * t], d->tri_idx[3 * t + 1], d->tri_idx[3 * t + 2], 0);
    for (uint32_t sh = 0; sh < d->n_shapes; ++sh)
        if (d->shapes[sh].type == MTSG_SHAPE_MESH)
            for (uint32_t t = 0; t < d->shapes[sh].tri_count; ++t) tidx[d->shapes[sh].tri_begin + t].w = sh;
    std::vector<float4> shrec((size_t)d->n_triangles * 6);
    for (uint32_t t = 0; t < d->n_triangles; ++t) {
        const uint4 ti = tidx[t];
        if (ti.x >= d->n_vertices || ti.y >= d->n_vertices || ti.z >= d->n_vertices || ti.w >= d->n_shapes) {
            g_err = "triangle index out of range";
            return fail(MTSG_ERR_INVALID);
        }
        const float *P = d->vtx_pos, *N = d->vtx_nrm;
        float f[24];
        for (int k = 0; k < 3; ++k) {
            f[k] = P[3 * ti.x + k]; f[3 + k] = P[3 * ti.y + k]; f[6 + k] = P[3 * ti.z + k];
            f[9 + k] = N[3 * ti.x + k]; f[12 + k] = N[3 * ti.y + k]; f[15 + k] = N[3 * ti.z + k];
            f[18 + k] = d->tri_dpdu[3 * t + k];
        }
        const mtsg_shape &sh = d->shapes[ti.w];
        uint32_t u[3] = {ti.w, (uint32_t)sh.bsdf | (sh.face_normals ? 0x80000000u : 0u), (uint32_t)sh.emitter};
        memcpy(f + 21, u, sizeof(u));
        memcpy(&shrec[6 * (size_t)t], f, sizeof(f));
    }
    int rc;
    DevScene &ds = s->ds;
    auto up = [&](auto *src, size_t n, auto **dst) {
        int r = upload(src, n, dst);
        if (r == MTSG_OK && *dst) s->allocs.push_back((void *)*dst);
        return r;
    };
    // the setup mode names rectangle r by the tie key n_triangles + r, its
    // TriAccel index in the leaf records: hold the description to that
    s->rectSetupOk = MTSG_RECT_SETUP && d->n_rects <= RECT_SETUP_CAP;
    for (uint32_t r = 0; r < d->n_rects && s->rectSetupOk; ++r) {
        if (!d->triaccel || (uint64_t)d->n_triangles + r >= d->n_prims) { s->rectSetupOk = false; break; }
        const mtsg_triaccel &ta = d->triaccel[d->n_triangles + r];
        s->rectSetupOk = ta.k == MTSG_TRIACCEL_SHAPE && ta.prim_index == r && ta.shape_index < d->n_shapes &&
                         d->shapes[ta.shape_index].type == MTSG_SHAPE_RECT;
    }
    // ---- device kd-tree layout from Mitsuba's KDNode array (kd_layout.h: host
    // only).  A flat scene that takes the setup mode gets the filtered leaf
    // addressing next to it (blocksRS; MTSG_OPT_LEAF_FILTER): this is the one
    // place a handle's layout is made, so both arrays always come from the
    // same tree (a replaced or refitted tree reaches the device as a new handle).
    KdLayout lay;
    if (const char *what = kd_layout(d, s->rectSetupOk && d->n_rects > 0 && d->n_instances == 0, lay)) {
        g_err = what;
        return fail(MTSG_ERR_INVALID);
    }
    static_assert(sizeof(KdU4) == sizeof(uint4) && sizeof(KdF4) == sizeof(float4), "kd_layout.h arrays upload as uint4 / float4");
    const std::vector<KdU2> &groupRoots = lay.groupRoots;
    const uint2 root2 = make_uint2(lay.root2.x, lay.root2.y);
    uint4 *dblocks, *dblocksRS; float4 *dtriL; float4 *dvpos, *dvnrm, *dshrec; uint4 *dtidx;
    mtsg_rect *rects; mtsg_shape *shapes; mtsg_bsdf *bsdfs; mtsg_emitter *emitters; float *ecdf, *etcdf;
    if ((rc = up(reinterpret_cast<const float4 *>(lay.triL.data()), lay.triL.size(), &dtriL)) ||
        (rc = up(reinterpret_cast<const uint4 *>(lay.blocks.data()), lay.blocks.size(), &dblocks)) ||
        (rc = up(reinterpret_cast<const uint4 *>(lay.blocksRS.data()), lay.blocksRS.size(), &dblocksRS)) ||
        (rc = up(vpos.data(), vpos.size(), &dvpos)) || (rc = up(vnrm.data(), vnrm.size(), &dvnrm)) ||
        (rc = up(tidx.data(), tidx.size(), &dtidx)) ||
        (rc = up(shrec.data(), shrec.size(), &dshrec)) ||
        (rc = up(d->rects, d->n_rects, &rects)) || (rc = up(d->shapes, d->n_shapes, &shapes)) ||
        (rc = up(d->bsdfs, d->n_bsdfs, &bsdfs)) || (rc = up(d->emitters, d->n_emitters, &emitters)) ||
        (rc = up(d->emitter_cdf, d->n_emitters + 1, &ecdf)) ||
        (rc = up(d->emitter_tri_cdf, d->n_emitter_tri_cdf, &etcdf)))
        return fail(rc);
    ds.blocks = dblocks; ds.root2 = root2;
    s->blocksRS = dblocksRS;   // null: no leaf references a rectangle, or the scene does not take the setup mode
    s->root2RS = make_uint2(lay.root2RS.x, lay.root2RS.y);
    ds.triL = dtriL; ds.vpos = dvpos; ds.vnrm = dvnrm;
    int constantEmitter = -1;   // index of the scene's constant environment emitter
    {
        // to_object rows of every rectangle, 48 B each (DevScene::rectM)
        std::vector<float4> rm((size_t)3 * std::max<uint32_t>(d->n_rects, 1u), make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < d->n_rects; ++i)
            for (int k = 0; k < 3; ++k) {
                const float *m = d->rects[i].to_object + 4 * k;
                rm[3 * i + k] = make_float4(m[0], m[1], m[2], m[3]);
            }
        // per rectangle its shading data, per emitter its rectangle's rows
        // (DevScene::rectSh / emitRect)
        if (d->n_bsdfs >= 0xFFFFu || d->n_emitters >= 0xFFFEu) { g_err = "too many BSDFs or emitters"; return fail(MTSG_ERR_INVALID); }
        std::vector<float4> rs((size_t)2 * std::max<uint32_t>(d->n_rects, 1u), make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < d->n_rects; ++i) {
            const mtsg_rect &R = d->rects[i];
            if (R.shape_index >= d->n_shapes) { g_err = "rectangle with an invalid shape index"; return fail(MTSG_ERR_INVALID); }
            const mtsg_shape &sh = d->shapes[R.shape_index];
            uint32_t be = ((uint32_t)sh.bsdf & 0xFFFFu) | (uint32_t)(sh.emitter + 1) << 16, si = R.shape_index;
            float bef, sif;
            memcpy(&bef, &be, 4);
            memcpy(&sif, &si, 4);
            rs[2 * i] = make_float4(R.frame_n[0], R.frame_n[1], R.frame_n[2], sif);
            rs[2 * i + 1] = make_float4(R.dpdu[0], R.dpdu[1], R.dpdu[2], bef);
        }
        std::vector<float4> er((size_t)4 * std::max<uint32_t>(d->n_emitters, 1u), make_float4(0, 0, 0, 0));
        int nEnvironment = 0;
        for (uint32_t e = 0; e < d->n_emitters; ++e) {
            const mtsg_emitter &em = d->emitters[e];
            const int32_t sidx = em.shape;
            uint32_t type = (uint32_t)MTSG_SHAPE_MESH + 100u;   // not a shape emitter (environment)
            // every kind is checked here: an unknown type must not fall
            // through into the area sampling
            if (em.type == MTSG_EMITTER_AREA) {
            } else if (em.type == MTSG_EMITTER_ENVMAP) {
                ++nEnvironment;
                if (!d->has_envmap || d->envmap.emitter != (int32_t)e) {
                    g_err = "emitter " + std::to_string(e) + ": envmap emitter without the scene's environment record";
                    return fail(MTSG_ERR_INVALID);
                }
            } else if (em.type >= MTSG_EMITTER_POINT && em.type <= MTSG_EMITTER_CONSTANT) {
                if (!d->emitter_ext) {
                    g_err = "emitter " + std::to_string(e) + ": point / spot / directional / constant emitter without emitter_ext";
                    return fail(MTSG_ERR_INVALID);
                }
                if (d->om) { g_err = "myPath2_OM scenes take area and envmap emitters only"; return fail(MTSG_ERR_INVALID); }
                const mtsg_emitter_ext &x = d->emitter_ext[e];
                s->emitterSet = EM_ALL;
                // the rows emitter_sample_ext reads (kernels.h)
                if (em.type == MTSG_EMITTER_POINT) {
                    er[4 * e] = make_float4(x.position[0], x.position[1], x.position[2], 0.f);
                } else if (em.type == MTSG_EMITTER_SPOT) {
                    if (!(x.cos_cutoff_angle <= x.cos_beam_width) || !std::isfinite(x.inv_transition_width)) {
                        g_err = "emitter " + std::to_string(e) + ": spot with inconsistent beam constants";
                        return fail(MTSG_ERR_INVALID);
                    }
                    er[4 * e] = make_float4(x.position[0], x.position[1], x.position[2], x.cos_beam_width);
                    er[4 * e + 1] = make_float4(x.to_local[6], x.to_local[7], x.to_local[8], x.cos_cutoff_angle);
                    er[4 * e + 2] = make_float4(x.cutoff_angle, x.inv_transition_width, 0.f, 0.f);
                } else if (em.type == MTSG_EMITTER_DIRECTIONAL) {
                    er[4 * e] = make_float4(x.direction[0], x.direction[1], x.direction[2], x.bsphere_radius);
                    er[4 * e + 1] = make_float4(x.bsphere_center[0], x.bsphere_center[1], x.bsphere_center[2], 0.f);
                } else {
                    ++nEnvironment;
                    if (!(x.bsphere_radius > 0)) {
                        g_err = "emitter " + std::to_string(e) + ": constant emitter without a bounding sphere";
                        return fail(MTSG_ERR_INVALID);
                    }
                    er[4 * e] = make_float4(x.bsphere_center[0], x.bsphere_center[1], x.bsphere_center[2], x.bsphere_radius);
                    constantEmitter = (int)e;
                }
            } else {
                g_err = "emitter " + std::to_string(e) + ": unknown emitter type " + std::to_string(em.type);
                return fail(MTSG_ERR_INVALID);
            }
            if (nEnvironment > 1) { g_err = "only one environment emitter (envmap or constant) is supported"; return fail(MTSG_ERR_INVALID); }
            if (sidx >= 0 && (uint32_t)sidx < d->n_shapes) {
                const mtsg_shape &sh = d->shapes[sidx];
                type = (uint32_t)sh.type;
                if (sh.type == MTSG_SHAPE_RECT && sh.rect < d->n_rects) {
                    const mtsg_rect &R = d->rects[sh.rect];
                    for (int k = 0; k < 3; ++k)
                        er[4 * e + k] = make_float4(R.to_world[4 * k], R.to_world[4 * k + 1], R.to_world[4 * k + 2], R.to_world[4 * k + 3]);
                    er[4 * e + 3] = make_float4(R.frame_n[0], R.frame_n[1], R.frame_n[2], 0.f);
                }
            }
            memcpy(&er[4 * e + 3].w, &type, 4);
        }
        float4 *drm, *drs, *der;
        if ((rc = up(rm.data(), rm.size(), &drm)) || (rc = up(rs.data(), rs.size(), &drs)) || (rc = up(er.data(), er.size(), &der)))
            return fail(rc);
        ds.rectM = drm;
        ds.rectSh = drs;
        ds.emitRect = der;
    }
    ds.tidx = dtidx; ds.shrec = dshrec; ds.rects = rects; ds.shapes = shapes; ds.bsdfs = bsdfs;
    ds.emitters = emitters; ds.emitter_cdf = ecdf; ds.emitter_tri_cdf = etcdf;
    ds.inst = nullptr;
    if (d->n_instances) {
        std::vector<float4> in((size_t)8 * d->n_instances);
        for (uint32_t i = 0; i < d->n_instances; ++i) {
            const mtsg_instance &I = d->instances[i];
            const mtsg_group &G = d->groups[I.group];
            const float *L = I.to_local, *W = I.to_world;
            float4 *o = &in[8 * (size_t)i];
            for (int r = 0; r < 3; ++r) {
                o[r] = make_float4(L[4 * r], L[4 * r + 1], L[4 * r + 2], L[4 * r + 3]);
                o[3 + r] = make_float4(W[4 * r], W[4 * r + 1], W[4 * r + 2], W[4 * r + 3]);
            }
            const KdU2 gr = groupRoots[I.group];
            float r0, r1;
            memcpy(&r0, &gr.x, 4);
            memcpy(&r1, &gr.y, 4);
            o[6] = make_float4(G.aabb_min[0], G.aabb_min[1], G.aabb_min[2], r0);
            o[7] = make_float4(G.aabb_max[0], G.aabb_max[1], G.aabb_max[2], r1);
        }
        float4 *dinst;
        if ((rc = up(in.data(), in.size(), &dinst))) return fail(rc);
        ds.inst = dinst;
    }
    // traversal stacks and the kd-restart guard (kernels.h kd_restart): the
    // compile-time defaults; only mtsg_set_test_knobs (tests) changes them
    ds.capFlat = SHORT_STACK;
    ds.capGrp = INNER_STACK;
    ds.capTop = OUTER_STACK;
    ds.rstGuard = RST_GUARD;
    ds.rstMax = RST_MAX;
    ds.rstMaxC = RST_MAX;
    ds.instPrefilter = 1;
    s->knobs = false;
    // two-level tie keys (kernels.h spec_iter_i): the TriAccel key count as
    // the per-instance stride, so keys of different (primitive, instance)
    // pairs never coincide; scenes too large for 32-bit keys fall back to an
    // odd multiplier (a bijection per instance; pairs across instances can
    // then collide, which only hides a tie of two such primitives)
    ds.instKeyStride = (uint64_t)d->n_prims * ((uint64_t)d->n_instances + 1) <= 0xFFFFFFFFull ? d->n_prims : 0x9E3779B1u;
    // environment emitter tables (envmap.h)
    // (a constant environment: 2 * (index + 1), read by the EM_ALL kernels alone)
    ds.has_env = d->has_envmap ? 1 : constantEmitter >= 0 ? 2 * (constantEmitter + 1) : 0;
    if (s->emitterSet != EM_ALL) s->emitterSet = d->has_envmap ? EM_ENV : EM_AREA;
    s->mats = 0;
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) {
        const mtsg_bsdf &b = d->bsdfs[i];
        if (b.type == MTSG_BSDF_CONDUCTOR || b.type == MTSG_BSDF_PLASTIC || b.type == MTSG_BSDF_ROUGHDIELECTRIC ||
            b.type == MTSG_BSDF_ROUGHPLASTIC || b.twosided)
            s->extBsdfs = true;
        if (b.type > MTSG_BSDF_ROUGHPLASTIC && d->om) {
            g_err = "myPath2_OM scenes take the BSDF types up to roughplastic only";
            return fail(MTSG_ERR_INVALID);
        }
        // phong, ward, roughdiffuse, difftrans, thindielectric: only the
        // all-kinds kernels at EXT level 2 hold them, so every other scene
        // keeps the kernels it ran before
        if (b.type > MTSG_BSDF_ROUGHPLASTIC) {
            s->ext2 = s->extBsdfs = true;
            s->emitterSet = EM_ALL;
        }
        // the material classes the non-extended shading kernel must hold
        if (b.type == MTSG_BSDF_DIFFUSE) s->mats |= MAT_DIFFUSE;
        else if (b.type == MTSG_BSDF_ROUGHCONDUCTOR) s->mats |= b.distribution == MTSG_MF_GGX ? MAT_RC_GGX : MAT_RC_OTHER;
        else if (b.type == MTSG_BSDF_DIELECTRIC) s->mats |= MAT_DIELECTRIC;
        else s->mats |= MATS_ALL;
        if (b.twosided && (b.back < 0 || (uint32_t)b.back >= d->n_bsdfs)) {
            g_err = "bsdf " + std::to_string(i) + ": twosided back record out of range";
            return fail(MTSG_ERR_INVALID);
        }
    }
    ds.env = DevEnv{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (d->has_envmap) {
        const mtsg_envmap &E = d->envmap;
        const mtsg_mipmap &EM = E.mip;
        if (EM.levels <= 0 || EM.levels > MTSG_ENVMAP_MAX_LEVELS || !d->env_texels || !d->env_cdf_rows || !d->env_cdf_cols ||
            !d->env_row_weights || E.emitter < 0 || (uint32_t)E.emitter >= d->n_emitters) {
            g_err = "inconsistent environment map description";
            return fail(MTSG_ERR_INVALID);
        }
        size_t need = 0;
        for (int l = 0; l < EM.levels; ++l)
            need = std::max(need, (size_t)EM.level_offset[l] + 3 * (size_t)EM.level_w[l] * EM.level_h[l]);
        if (need > d->n_env_texels) { g_err = "environment map texel array too small"; return fail(MTSG_ERR_INVALID); }
        mtsg_envmap *dE; float *dt, *dr, *dc, *dw;
        uint32_t *dgr, *dgc;
        const int W = EM.level_w[0], H = EM.level_h[0];
        // guide tables of the CDF searches (envmap.h env_sample_reuse_guided):
        // entry g = std::lower_bound of g / ENV_GUIDE over the size + 1 entries
        auto guides = [](const float *cdf, uint32_t size, uint32_t *out) {
            for (uint32_t g = 0; g <= ENV_GUIDE; ++g)
                out[g] = (uint32_t)(std::lower_bound(cdf, cdf + size + 1, (float)g / (float)ENV_GUIDE) - cdf);
        };
        std::vector<uint32_t> gr(ENV_GUIDE + 1), gc((size_t)(ENV_GUIDE + 1) * H);
        guides(d->env_cdf_rows, (uint32_t)H, gr.data());
        for (int y = 0; y < H; ++y) guides(d->env_cdf_cols + (size_t)y * (W + 1), (uint32_t)W, gc.data() + (size_t)y * (ENV_GUIDE + 1));
        if ((rc = up(&E, 1, &dE)) || (rc = up(d->env_texels, d->n_env_texels, &dt)) ||
            (rc = up(d->env_cdf_rows, (size_t)H + 1, &dr)) || (rc = up(d->env_cdf_cols, (size_t)(W + 1) * H, &dc)) ||
            (rc = up(d->env_row_weights, (size_t)H, &dw)) || (rc = up(gr.data(), gr.size(), &dgr)) ||
            (rc = up(gc.data(), gc.size(), &dgc)))
            return fail(rc);
        ds.env = DevEnv{dE, dt, dr, dc, dw, dgr, dgc};
    }
    // bitmap textures (mipmap.h) and the per-triangle records of their lookups
    ds.textures = nullptr; ds.tex_texels = nullptr; ds.ttex = nullptr;
    bool texDiffs = false;
    for (uint32_t i = 0; i < d->n_bsdfs; ++i)
        if (d->bsdfs[i].texture < 0 || (uint32_t)d->bsdfs[i].texture > d->n_textures) {
            g_err = "bsdf " + std::to_string(i) + ": texture index out of range";
            return fail(MTSG_ERR_INVALID);
        }
    if (d->n_textures) {
        if (!d->textures || !d->tex_texels || (d->n_triangles && (!d->tri_uv || !d->tri_dpdv))) {
            g_err = "inconsistent texture description";
            return fail(MTSG_ERR_INVALID);
        }
        for (uint32_t i = 0; i < d->n_textures; ++i) {
            const mtsg_mipmap &M = d->textures[i].mip;
            bool ok = M.levels > 0 && M.levels <= MTSG_MIPMAP_MAX_LEVELS && M.filter >= MTSG_MIP_NEAREST && M.filter <= MTSG_MIP_EWA &&
                      M.wrap_u >= MTSG_WRAP_CLAMP && M.wrap_u <= MTSG_WRAP_ONE && M.wrap_v >= MTSG_WRAP_CLAMP && M.wrap_v <= MTSG_WRAP_ONE;
            for (int l = 0; ok && l < M.levels; ++l)
                ok = M.level_w[l] > 0 && M.level_h[l] > 0 &&
                     (size_t)M.level_offset[l] + 3 * (size_t)M.level_w[l] * M.level_h[l] <= d->n_tex_texels;
            if (!ok) { g_err = "texture " + std::to_string(i) + ": malformed MIP map"; return fail(MTSG_ERR_INVALID); }
            texDiffs |= M.filter == MTSG_MIP_TRILINEAR || M.filter == MTSG_MIP_EWA;
        }
        mtsg_texture *dtex; float *dtt;
        if ((rc = up(d->textures, d->n_textures, &dtex)) || (rc = up(d->tex_texels, d->n_tex_texels, &dtt)))
            return fail(rc);
        ds.textures = dtex; ds.tex_texels = dtt;
        s->nTextures = d->n_textures;
        s->extBsdfs = true;   // texture lookups live in the extended shade kernel
    }
    // the per-triangle texture records: with textures, or for the `uv` field of
    // a multichannel scene without any (the builder fills tri_uv for it)
    if (d->tri_uv && d->tri_dpdv) {
        std::vector<float4> tt((size_t)3 * std::max(1u, d->n_triangles), make_float4(0, 0, 0, 0));
        for (uint32_t t = 0; t < d->n_triangles; ++t) {
            const float *uv = d->tri_uv + 6 * (size_t)t, *dv = d->tri_dpdv + 3 * (size_t)t;
            tt[3 * t] = make_float4(uv[0], uv[1], uv[2], uv[3]);
            tt[3 * t + 1] = make_float4(uv[4], uv[5], dv[0], dv[1]);
            tt[3 * t + 2] = make_float4(dv[2], 0.f, 0.f, 0.f);
        }
        float4 *dttex;
        if ((rc = up(tt.data(), tt.size(), &dttex))) return fail(rc);
        ds.ttex = dttex;
    }
    s->nShapes = d->n_shapes;
    s->bsdfTexture.resize(d->n_bsdfs);
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) s->bsdfTexture[i] = d->bsdfs[i].texture;
    s->texDiffs = texDiffs;
    s->hasEnvmap = d->has_envmap != 0;
    // myPath2_OM occupancy maps (om.cpp)
    ds.om = nullptr; ds.om_bits = nullptr;
    if (d->om) {
        if (!d->om_bits) { g_err = "occupancy maps without their bits"; return fail(MTSG_ERR_INVALID); }
        mtsg_om *dom; uint32_t *dbits;
        if ((rc = up(d->om, 1, &dom)) ||
            (rc = up(d->om_bits, (size_t)MTSG_OM_COUNT * MTSG_OM_SIZE * MTSG_OM_SIZE * (MTSG_OM_SIZE / 32), &dbits)))
            return fail(rc);
        ds.om = dom; ds.om_bits = dbits;
    }
    ds.n_emitters = d->n_emitters;
    ds.n_tri = d->n_triangles;
    ds.n_rect = d->n_rects;
    ds.n_bsdfs = d->n_bsdfs;
    for (int k = 0; k < 3; ++k) { ds.bmin[k] = d->aabb_min[k]; ds.bmax[k] = d->aabb_max[k]; }
    DevCamera &c = s->cam;
    const mtsg_camera &hc = d->camera;
    memcpy(c.s2c, hc.sample_to_camera, sizeof(c.s2c));
    memcpy(c.c2w, hc.camera_to_world, sizeof(c.c2w));
    c.near_clip = hc.near_clip; c.far_clip = hc.far_clip; c.inv_res_x = hc.inv_res_x; c.inv_res_y = hc.inv_res_y;
    c.film_w = hc.film_w; c.film_h = hc.film_h;
    c.filter_radius = hc.filter_radius; c.filter_scale = hc.filter_scale; c.border = hc.border;
    c.has_alpha = hc.has_alpha;
    memcpy(c.filter_values, hc.filter_values, sizeof(c.filter_values));
    memcpy(c.dx, hc.dx, sizeof(c.dx));
    memcpy(c.dy, hc.dy, sizeof(c.dy));
    c.crop_w = hc.crop_w; c.crop_h = hc.crop_h;
    c.lens = hc.sensor_type == MTSG_SENSOR_THINLENS ? 1 : 0;
    c.aperture_radius = hc.aperture_radius; c.focus_distance = hc.focus_distance;
    ds.camO[0] = c.c2w[3]; ds.camO[1] = c.c2w[7]; ds.camO[2] = c.c2w[11];
    ds.camNear = c.near_clip; ds.camFar = c.far_clip;
    ds.camCompact = (ds.inst || c.lens) ? 0 : 1;   // (a thinlens ray starts on the aperture: k_camera_lens)
    c.compact = ds.camCompact;
    camera_diff_mode(s);
    // the camera on the device too: bounce 0 recomputes a missing camera ray's
    // differentials from it (DevScene::cam_env_diffs)
    {
        DevCamera *dc;
        if ((rc = up(&s->cam, 1, &dc))) return fail(rc);
        ds.camDev = dc;
    }
    // sampler and its quasi-Monte Carlo tables
    s->samplerType = d->sampler.type;
    s->samplerDim = d->sampler.dimension;
    if (s->samplerType < MTSG_SAMPLER_INDEPENDENT || s->samplerType > MTSG_SAMPLER_SOBOL) {
        g_err = "unknown sampler type";
        return fail(MTSG_ERR_INVALID);
    }
    if (s->samplerType == MTSG_SAMPLER_HALTON || s->samplerType == MTSG_SAMPLER_HAMMERSLEY) {
        if (!d->qmc_primes || !d->qmc_perm_offset) { g_err = "sampler: missing QMC tables"; return fail(MTSG_ERR_INVALID); }
        uint32_t *dp, *doff;
        if ((rc = up(d->qmc_primes, MTSG_QMC_PRIMES, &dp)) || (rc = up(d->qmc_perm_offset, MTSG_QMC_PRIMES, &doff)))
            return fail(rc);
        s->ds.qmcPrimes = dp;
        s->ds.qmcOff = doff;
        if (d->qmc_perm) {
            const size_t n = (size_t)d->qmc_perm_offset[MTSG_QMC_PRIMES - 1] + d->qmc_primes[MTSG_QMC_PRIMES - 1];
            uint16_t *dperm;
            if ((rc = up(d->qmc_perm, n, &dperm))) return fail(rc);
            s->ds.qmcPerm = dperm;
            // inverse permutations of the first two bases (faure.cpp:74-78)
            for (int b = 0; b < 2; ++b)
                for (uint32_t j = 0; j < d->qmc_primes[b]; ++j) s->qmcInv[b][d->qmc_perm[d->qmc_perm_offset[b] + j]] = (int)j;
        }
    }
    if (s->samplerType == MTSG_SAMPLER_SOBOL) {
        if (!d->sobol_matrices || !d->sobol_vdc || !d->sobol_vdc_inv) { g_err = "sampler: missing sobol tables"; return fail(MTSG_ERR_INVALID); }
        uint32_t r = 1, m = 0;
        while (r < (uint32_t)std::max(d->camera.crop_w, d->camera.crop_h)) r <<= 1;
        while ((1u << (m + 1)) <= r) ++m;
        if (m > 1 && (m > d->sobol_vdc_inv_rows || m > d->sobol_vdc_rows + 1)) { g_err = "sobol: film too large for the look_up tables"; return fail(MTSG_ERR_INVALID); }
        uint32_t *dm;
        uint64_t *dv, *dvi;
        if ((rc = up(d->sobol_matrices, (size_t)MTSG_SOBOL_DIMS * MTSG_SOBOL_COLUMNS, &dm)) ||
            (rc = up(d->sobol_vdc, (size_t)d->sobol_vdc_rows * MTSG_SOBOL_COLUMNS + MTSG_SOBOL_COLUMNS, &dv)) ||
            (rc = up(d->sobol_vdc_inv, (size_t)d->sobol_vdc_inv_rows * MTSG_SOBOL_COLUMNS, &dvi)))
            return fail(rc);
        s->sobolM = dm;
        s->sobolVdc = dv;
        s->sobolVdcInv = dvi;
        s->sobolScramble = d->sobol_scramble;
    }
    // persistent grids from the occupancy query
    int perCU = 0;
    if ((perCU = trace_flat_blocks_per_cu()) <= 0) perCU = 8;
    s->traceGrid = s->cuCount * perCU;
    perCU = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, (const void *)k_trace_s<false, MTSG_INST_MIN_IDLE, true>, TRACE_BLOCK, 0) != hipSuccess ||
        perCU <= 0)
        perCU = 4;
    s->traceGridInst = s->cuCount * perCU;
#ifndef MTSG_SHADE_WG_PER_CU
#define MTSG_SHADE_WG_PER_CU 64   // k_shade workgroups of 256 per CU, 4 resident (r05_shade_launch.txt: 8 -> 64, C3 shade -5%)
#endif
    s->shadeGrid = s->cuCount * MTSG_SHADE_WG_PER_CU * 256 / SHADE_BLOCK;
    perCU = 0;
    if ((perCU = finish_blocks_per_cu(false)) <= 0) perCU = 3;
    s->finishGrid = s->cuCount * perCU;
    if ((perCU = finish_blocks_per_cu(true)) <= 0) perCU = 3;
    s->finishGridMats = s->cuCount * perCU;
    // two-level traversal: the per-lane save slots of its grid (kernels.h save_vec)
    s->ds.instSave = nullptr;
    if (s->ds.inst && !MTSG_INST_REGSAVE) {
        uint4 *save = nullptr;
        // slots for the larger of the two grids that switch levels (k_trace_s, k_finish)
        const size_t lanes = (size_t)std::max(s->traceGridInst, s->finishGrid) * TRACE_BLOCK;
        if (hipMalloc((void **)&save, (size_t)SAVE_VECS * lanes * sizeof(uint4)) != hipSuccess) {
            g_err = "out of device memory (instance save slots)";
            return fail(MTSG_ERR_OOM);
        }
        s->allocs.push_back(save);
        s->ds.instSave = save;
    }
    s->finishPaths = MTSG_DEFAULT_FINISH_PATHS;
    s->lstream[0] = s->stream;
    for (int l = 1; l < MTSG_MAX_LANES; ++l)
        if (hipStreamCreateWithFlags(&s->lstream[l], hipStreamNonBlocking) != hipSuccess) { g_err = "stream"; return fail(MTSG_ERR_DEVICE); }
    if (hipHostMalloc((void **)&s->hostCnt, 2 * MTSG_MAX_LANES * HOSTCNT_STRIDE * sizeof(uint32_t)) != hipSuccess) { g_err = "pinned alloc"; return fail(MTSG_ERR_OOM); }
    *out = s;
    return MTSG_OK;
}

int mtsg_set_batch_paths(mtsg_scene *s, uint32_t paths) {
    if (!s || paths < TILE * TILE) { g_err = "batch must hold at least 256 paths"; return MTSG_ERR_INVALID; }
    s->requestedBatch = paths;
    return MTSG_OK;
}

int mtsg_set_test_knobs(mtsg_scene *s, const mtsg_test_knobs *k) {
    if (!s) return MTSG_ERR_INVALID;
    DevScene &ds = s->ds;
    ds.capFlat = SHORT_STACK;
    ds.capGrp = INNER_STACK;
    ds.capTop = OUTER_STACK;
    ds.rstGuard = RST_GUARD;
    ds.rstMax = RST_MAX;
    if (k) {
        if (k->stack_cap > 0) {
            const uint32_t cap = (uint32_t)k->stack_cap;
            ds.capFlat = std::min(ds.capFlat, cap);
            ds.capGrp = std::min(ds.capGrp, cap);
            ds.capTop = std::min(ds.capTop, cap);
        }
        if (k->restart_guard >= 0) ds.rstGuard = (uint32_t)k->restart_guard;
        if (k->restart_limit >= 0) ds.rstMax = std::min<uint32_t>(RST_MAX, (uint32_t)k->restart_limit);
    }
    ds.rstMaxC = (k && k->limit_shadow_only) ? RST_MAX : ds.rstMax;
    ds.instPrefilter = (k && k->no_instance_prefilter) ? 0u : 1u;
    // any change selects the KNOBS kernel instantiations (the production
    // kernels keep their compile-time constants) and turns the tail kernel off
    s->knobs = ds.capFlat != (uint32_t)SHORT_STACK || ds.capGrp != (uint32_t)INNER_STACK || ds.capTop != (uint32_t)OUTER_STACK ||
               ds.rstGuard != RST_GUARD || ds.rstMax != RST_MAX || ds.rstMaxC != RST_MAX || !ds.instPrefilter;
    return MTSG_OK;
}

int mtsg_set_finish_paths(mtsg_scene *s, uint32_t paths) {
    if (!s) return MTSG_ERR_INVALID;
    s->finishPaths = paths;
    return MTSG_OK;
}

int mtsg_scene_kernel_sets(mtsg_scene *s, int32_t *material_set, int32_t *emitter_set) {
    if (!s || !material_set || !emitter_set) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    // what shade_args hands the independent sampler's launchers
    const bool emx = s->emitterSet == EM_ALL;
    *material_set = mats_kernel_set((s->shadeGeneric || emx) ? (int)MATS_ALL : s->mats) + ((s->extBsdfs || emx) ? 16 : 0) + (s->ext2 ? 32 : 0);
    *emitter_set = emx ? MTSG_EMITTER_SET_ALL : (s->ds.has_env & 1) ? MTSG_EMITTER_SET_ENVMAP : MTSG_EMITTER_SET_AREA;
    return MTSG_OK;
}

int mtsg_set_option(mtsg_scene *s, int32_t key, int64_t value) {
    if (!s) { g_err = "null scene"; return MTSG_ERR_INVALID; }
    switch (key) {
        case MTSG_OPT_TRACE_REFILL:
            if (value != 16 && value != 32) { g_err = "MTSG_OPT_TRACE_REFILL: 16 or 32 idle lanes"; return MTSG_ERR_INVALID; }
            s->traceMode = value == 32 ? 1 : 0;
            return MTSG_OK;
        case MTSG_OPT_FINISH_SHADE_MIN:
            if (value < 1 || value > 64) { g_err = "MTSG_OPT_FINISH_SHADE_MIN: 1..64 lanes"; return MTSG_ERR_INVALID; }
            s->finishShadeMin = (uint32_t)value;
            return MTSG_OK;
        case MTSG_OPT_LANES:
            if (value < 1 || value > MTSG_MAX_LANES) { g_err = "MTSG_OPT_LANES: 1..4 concurrent batches"; return MTSG_ERR_INVALID; }
            s->lanes = (int)value;
            return MTSG_OK;
        case MTSG_OPT_STAGGER:
            if (value < 0 || value > 16) { g_err = "MTSG_OPT_STAGGER: 0..16 bounces"; return MTSG_ERR_INVALID; }
            s->stagger = (int)value;
            return MTSG_OK;
        case MTSG_OPT_SHADE_GENERIC:
            s->shadeGeneric = value != 0;
            return MTSG_OK;
        case MTSG_OPT_RAY_ORDER:
            if (value < 0 || value > 1) { g_err = "MTSG_OPT_RAY_ORDER: 0 (append order) or 1 (direction-sorted windows)"; return MTSG_ERR_INVALID; }
            s->rayOrder = (int)value;
            return MTSG_OK;
        case MTSG_OPT_CAMERA_DIFFS:
            if (value < 0 || value > 1) { g_err = "MTSG_OPT_CAMERA_DIFFS: 0 (recomputed on a miss) or 1 (stored)"; return MTSG_ERR_INVALID; }
            s->storeCamDiffs = value != 0;
            camera_diff_mode(s);
            return MTSG_OK;
        case MTSG_OPT_RECT_SETUP:
            if (value < 0 || value > 1) { g_err = "MTSG_OPT_RECT_SETUP: 0 (rectangles tested in the leaves) or 1 (at ray setup)"; return MTSG_ERR_INVALID; }
            s->rectSetupOpt = value != 0;
            return MTSG_OK;
        case MTSG_OPT_RAY_PRESETUP:
            if (value < 0 || value > 1) { g_err = "MTSG_OPT_RAY_PRESETUP: 0 (rectangles tested in the traversal's refill) or 1 (where the rays are made)"; return MTSG_ERR_INVALID; }
            s->rayPresetupOpt = value != 0;
            return MTSG_OK;
        case MTSG_OPT_LEAF_FILTER:
            if (value < 0 || value > 1) { g_err = "MTSG_OPT_LEAF_FILTER: 0 (the setup mode steps over rectangle records) or 1 (its leaves hold none)"; return MTSG_ERR_INVALID; }
            s->leafFilterOpt = value != 0;
            return MTSG_OK;
        case MTSG_OPT_ADAPTIVE_ROUND:
            if (value < 0 || value > (int64_t)ADAPTIVE_MAX_ROUND) { g_err = "MTSG_OPT_ADAPTIVE_ROUND: 0 (the base count) or 1..65536 samples per later round"; return MTSG_ERR_INVALID; }
            s->adaptiveRound = (uint32_t)value;
            return MTSG_OK;
        default:
            g_err = "unknown option key " + std::to_string(key);
            return MTSG_ERR_INVALID;
    }
}

int mtsg_set_flags(mtsg_scene *s, uint32_t flags) {
    if (!s) return MTSG_ERR_INVALID;
    s->flags = flags;
    return MTSG_OK;
}

int mtsg_get_stats(mtsg_scene *s, mtsg_stats *out) {
    if (!s || !out) return MTSG_ERR_INVALID;
    *out = s->stats;
    return MTSG_OK;
}

int mtsg_debug_wavetimes(mtsg_scene *s, uint64_t *out, uint32_t max_launches, uint32_t *waves) {
    if (!s || !waves || (!out && max_launches)) return MTSG_ERR_INVALID;
    *waves = (uint32_t)s->traceGrid;
    const uint32_t n = std::min(max_launches, s->wtLaunches);
    if (n && s->waveTimes &&
        hipMemcpy(out, s->waveTimes, (size_t)WT_WORDS * s->traceGrid * n * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return MTSG_ERR_DEVICE;
    return (int)s->wtLaunches;
}

int mtsg_debug_stragglers(mtsg_scene *s, float *out, uint32_t max_rays) {
    if (!s || (!out && max_rays)) return MTSG_ERR_INVALID;
    const uint32_t n = (uint32_t)(s->stragglers.size() / 8);
    for (uint32_t k = 0; k < std::min(n, max_rays); ++k) {
        const unsigned long long *w = &s->stragglers[8 * k];
        float *o = out + 12 * k;
        for (int j = 0; j < 6; ++j) {
            const uint32_t bits = (uint32_t)w[j];
            memcpy(&o[j], &bits, 4);
        }
        const uint32_t w6 = (uint32_t)w[6], w7 = (uint32_t)w[7];
        o[6] = (float)(w6 & 0x7FFFFFFFu);
        o[7] = (float)(w6 >> 31);
        o[8] = (float)(w7 & 4095u);
        o[9] = (float)((w7 >> 12) & 4095u);
        o[10] = (float)(w7 >> 24);
        o[11] = 0.0f;
    }
    return (int)n;
}

int mtsg_set_tile_callback(mtsg_scene *s, mtsg_tile_fn fn, void *user) {
    if (!s) return MTSG_ERR_INVALID;
    s->tileFn = fn;
    s->tileUser = user;
    return MTSG_OK;
}

void mtsg_cancel_clear(mtsg_scene *s) {
    if (s) s->cancel.store(0);
}

void mtsg_cancel(mtsg_scene *s) {
    if (s) s->cancel.store(1);
}

int mtsg_device_alloc(mtsg_scene *s, size_t bytes, void **out) {
    if (!s || !out) return MTSG_ERR_INVALID;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    HIP_TRY(hipMalloc(out, bytes));
    return MTSG_OK;
}
int mtsg_device_free(mtsg_scene *s, void *ptr) {
    if (!s) return MTSG_ERR_INVALID;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    HIP_TRY(hipFree(ptr));
    return MTSG_OK;
}
int mtsg_device_memset(mtsg_scene *s, void *ptr, size_t bytes) {
    if (!s) return MTSG_ERR_INVALID;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    HIP_TRY(hipMemsetAsync(ptr, 0, bytes, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MTSG_OK;
}
int mtsg_device_to_host(mtsg_scene *s, void *dst, const void *src, size_t bytes) {
    if (!s) return MTSG_ERR_INVALID;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MTSG_OK;
}

int mtsg_scene_set_aov(mtsg_scene *s, const mtsg_aov_desc *d) {
    if (!s) { g_err = "null scene"; return MTSG_ERR_INVALID; }
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    if (!d) { free_aov(s); return MTSG_OK; }
    if (d->n_children < 1 || d->n_children > MTSG_MAX_SUBINTEGRATORS) {
        g_err = "multichannel: 1 to " + std::to_string(MTSG_MAX_SUBINTEGRATORS) + " child integrators";
        return MTSG_ERR_INVALID;
    }
    if (d->n_bsdfs != s->ds.n_bsdfs || d->n_shapes != s->nShapes || (d->n_bsdfs && !d->bsdfs) || (d->n_shapes && !d->shapes) ||
        (d->n_elems && !d->elem_starts)) {
        g_err = "multichannel: the descriptor's BSDF / shape tables do not match the scene";
        return MTSG_ERR_INVALID;
    }
    DevAov A{};
    A.m = (int)d->n_children;
    A.pathChild = -1;
    bool needUv = false;
    for (int k = 0; k < A.m; ++k) {
        const mtsg_aov_child &c = d->children[k];
        if (c.kind == MTSG_AOV_PATH) {
            if (A.pathChild >= 0) { g_err = "multichannel: at most one `path` child"; return MTSG_ERR_INVALID; }
            A.pathChild = k;
            continue;
        }
        if (c.kind < MTSG_FIELD_POSITION || c.kind > MTSG_FIELD_PRIM_INDEX) { g_err = "multichannel: unknown child kind"; return MTSG_ERR_INVALID; }
        A.kind[A.nf] = c.kind;
        A.child[A.nf] = k;
        for (int j = 0; j < 3; ++j) A.undef[A.nf][j] = c.undefined[j];
        needUv |= c.kind == MTSG_FIELD_UV;
        ++A.nf;
    }
    for (uint32_t i = 0; i < d->n_bsdfs; ++i)
        if (d->bsdfs[i].textured) {
            if (!s->bsdfTexture[i]) { g_err = "multichannel: a textured albedo record on a BSDF without a texture"; return MTSG_ERR_INVALID; }
            needUv = true;
        }
    if (needUv && s->ds.n_tri && !s->ds.ttex) {
        g_err = "multichannel: the `uv` field and textured albedos need the scene's tri_uv / tri_dpdv";
        return MTSG_ERR_INVALID;
    }
    for (uint32_t i = 0; i < d->n_shapes; ++i) {
        const mtsg_aov_shape &sh = d->shapes[i];
        if (sh.elem_count < 1 || (uint64_t)sh.elem_offset + sh.elem_count > d->n_elems) {
            g_err = "multichannel: shape " + std::to_string(i) + " has an invalid element range";
            return MTSG_ERR_INVALID;
        }
    }
    memcpy(A.w2c, d->world_to_camera, sizeof(A.w2c));
    free_aov(s);
    mtsg_aov_bsdf *db = nullptr;
    mtsg_aov_shape *dsh = nullptr;
    uint32_t *de = nullptr;
    auto up = [&](auto *src, size_t n, auto **dst) {
        int r = upload(src, n, dst);
        if (*dst) s->aovAllocs.push_back((void *)*dst);
        return r;
    };
    if ((rc = up(d->bsdfs, d->n_bsdfs, &db)) || (rc = up(d->shapes, d->n_shapes, &dsh)) || (rc = up(d->elem_starts, d->n_elems, &de))) {
        free_aov(s);
        return rc;
    }
    A.bsdfs = db;
    A.shapes = dsh;
    A.elems = de;
    s->aov = A;
    s->aovOn = true;
    return MTSG_OK;
}

int mtsg_scene_set_direct(mtsg_scene *s, const mtsg_direct_desc *d) {
    if (!s) { g_err = "null scene"; return MTSG_ERR_INVALID; }
    if (!d) { s->directOn = false; s->direct = mtsg_direct_desc{}; return MTSG_OK; }
    // one sample's fan must leave room for a tile of samples in a batch (render_plan.h)
    if ((uint64_t)d->emitter_samples + d->bsdf_samples > PLAN_MAX_FAN || d->ao_samples > PLAN_MAX_FAN) {
        g_err = "direct / ao: more than " + std::to_string(PLAN_MAX_FAN) + " shading samples per camera sample";
        return MTSG_ERR_INVALID;
    }
    if (d->ao_samples && !(d->ao_ray_length > 0)) { g_err = "ao: rayLength must be greater than zero (mtsh_scene_direct resolves the default)"; return MTSG_ERR_INVALID; }
    s->direct = *d;
    s->directOn = true;
    return MTSG_OK;
}

int mtsg_scene_set_adaptive(mtsg_scene *s, const mtsg_adaptive_desc *d) {
    if (!s) { g_err = "null scene"; return MTSG_ERR_INVALID; }
    if (!d) { s->adaptiveOn = false; s->adaptive = mtsg_adaptive_desc{}; return MTSG_OK; }
    // adaptive.cpp:176-178, and this project's own refusal of the unbounded mode
    if (d->base_count < 8) { g_err = "Starting the adaptive integrator with less than 8 samples per pixel does not make much sense -- giving up."; return MTSG_ERR_INVALID; }
    if (d->max_sample_factor < 0) { g_err = "adaptive: max_sample_factor must not be negative: a bound on the samples per pixel is required"; return MTSG_ERR_INVALID; }
    if ((uint64_t)d->max_sample_factor * d->base_count > (1u << 24)) { g_err = "adaptive: max_sample_factor x base_count exceeds 2^24 samples per pixel"; return MTSG_ERR_INVALID; }
    if (!(d->max_error >= 0.0f) || !(d->quantile >= 0.0f)) { g_err = "adaptive: max_error and quantile must not be negative"; return MTSG_ERR_INVALID; }
    s->adaptive = *d;
    s->adaptiveOn = true;
    return MTSG_OK;
}

int mtsg_adaptive_info(mtsg_scene *s, mtsg_adaptive_result *out, uint32_t *counts, size_t capacity) {
    if (!s || !out) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    if (!s->adaptiveHave) { g_err = "mtsg_adaptive_info: the handle has rendered no adaptive scene"; return MTSG_ERR_INVALID; }
    *out = s->adaptiveResult;
    if (counts) {
        if (capacity < s->adaptiveCounts.size()) { g_err = "mtsg_adaptive_info: counts holds fewer than tile_w x tile_h entries"; return MTSG_ERR_INVALID; }
        memcpy(counts, s->adaptiveCounts.data(), s->adaptiveCounts.size() * sizeof(uint32_t));
    }
    return MTSG_OK;
}

int mtsg_render_device_multi(mtsg_scene *s, const mtsg_render_params *p, float *film) {
    if (!s || !film) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_impl(s, p, film, 0, true);
}

int mtsg_render_device_tiles_multi(mtsg_scene *s, const mtsg_render_params *p, float *windows) {
    if (!s || !windows) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_impl(s, p, windows, TILE + 2 * s->cam.border, true);
}

int mtsg_render_multi(mtsg_scene *s, const mtsg_render_params *p, float *out) {
    if (!s || !out) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    if (!s->aovOn) { g_err = "no multichannel child set is active (mtsg_scene_set_aov)"; return MTSG_ERR_INVALID; }
    return render_to_host(s, p, out, true);
}

int mtsg_render_samples_multi(mtsg_scene *s, const mtsg_render_params *p, float *out) {
    if (!s || !out || !p) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    if (!s->aovOn) { g_err = "no multichannel child set is active (mtsg_scene_set_aov)"; return MTSG_ERR_INVALID; }
    return render_samples(s, p, out, true);
}

int mtsg_render_device(mtsg_scene *s, const mtsg_render_params *p, float *film) {
    if (!s || !film) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_impl(s, p, film);
}

int mtsg_tile_windows(mtsg_scene *s, const mtsg_render_params *p, uint32_t *ntiles, int32_t *window) {
    if (!s || !ntiles || !window) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    int rc;
    if ((rc = validate(p, s)) != MTSG_OK) return rc;
    *ntiles = plan_render(p->tile_w, p->tile_h, p->spp, p->tile_stride, p->tile_offset, (uint32_t)s->tileKeys.size(), DEFAULT_BATCH_PATHS, 1, true).ntiles;
    *window = TILE + 2 * s->cam.border;
    return MTSG_OK;
}

int mtsg_set_tile_list(mtsg_scene *s, const int32_t *keys, uint32_t n) {
    if (!s || (n && !keys)) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    std::vector<int32_t> k(keys, keys + n), sorted(k);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t i = 0; i < n; ++i)
        if (sorted[i] < 0 || (i && sorted[i] == sorted[i - 1])) {
            g_err = "tile list: deal keys must be distinct and non-negative";
            return MTSG_ERR_INVALID;
        }
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    if (n > s->tileKeysCap) {
        if (s->tileKeysDev) hipFree(s->tileKeysDev);
        s->tileKeysDev = nullptr;
        s->tileKeysCap = 0;
        HIP_TRY(hipMalloc((void **)&s->tileKeysDev, n * sizeof(int32_t)));
        s->tileKeysCap = n;
    }
    if (n) HIP_TRY(hipMemcpy(s->tileKeysDev, k.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    s->tileKeys.swap(k);
    return MTSG_OK;
}

int mtsg_render_device_tiles(mtsg_scene *s, const mtsg_render_params *p, float *windows) {
    if (!s || !windows) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_impl(s, p, windows, TILE + 2 * s->cam.border);
}

int mtsg_render(mtsg_scene *s, const mtsg_render_params *p, float *rgbaw_out) {
    if (!s || !rgbaw_out) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_to_host(s, p, rgbaw_out, false);
}

int mtsg_render_samples(mtsg_scene *s, const mtsg_render_params *p, float *L_out) {
    if (!s || !L_out) { g_err = "null argument"; return MTSG_ERR_INVALID; }
    return render_samples(s, p, L_out, false);
}

// The producer's part of a ray query in the pre-record mode, what k_camera and
// k_shade do for the rays they make: a closest ray's pre-record into P.pre; a
// shadow ray of list Q is appended to P's list (CNT_S0) unless a rectangle
// occludes it (its cell then keeps "occluded": no contribution arrives).
static __global__ void k_query_pre(DevScene S, DevPaths P, DevPaths Q, uint32_t n, int shadow) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!shadow) {
        stS(&P.pre[i], ray_prerecord(S, ldS(P.ray_o + i), ldS(P.ray_d + i), false));
        return;
    }
    const float4 so = ldS(Q.sh_o + i), sd = ldS(Q.sh_d + i);   // sh_o.w = maxt, sh_d.w = mint
    const float4 rec = ray_prerecord(S, make_float4(so.x, so.y, so.z, sd.w), make_float4(sd.x, sd.y, sd.z, so.w), true);
    if (__float_as_uint(rec.w) != 0xFFFFFFFFu) return;
    const uint32_t j = atomicAdd(&P.cnt[CNT_S0], 1u);
    stS(&P.sh_o[j], so);
    stS(&P.sh_d[j], sd);
    stS(&P.sh_c[j], ldS(Q.sh_c + i));
}

// Ray queries run the production traversal kernel (the one the integrator
// launches, selected by traceMode) over a work list of n rays; with
// MTSG_OPT_RAY_PRESETUP 1, where it applies, as the path integrator runs it:
// over rays with pre-records (k_query_pre).
static int trace_rays(mtsg_scene *s, uint32_t n, const float *rays, float *t, float *u, float *v, uint32_t *prim,
                      uint8_t *occ, bool shadow) {
    if (!s || (!rays && n)) return MTSG_ERR_INVALID;
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    std::vector<float4> a(n), b(n), c(shadow ? n : 0);
    for (uint32_t i = 0; i < n; ++i) {
        const float *r = rays + 8 * (size_t)i;   // o.xyz, d.xyz, mint, maxt
        if (shadow) {
            a[i] = make_float4(r[0], r[1], r[2], r[7]);
            b[i] = make_float4(r[3], r[4], r[5], r[6]);
            uint32_t tgt = 0x80000000u | i;
            float ft;
            memcpy(&ft, &tgt, 4);
            c[i] = make_float4(1.f, 0.f, 0.f, ft);   // unoccluded -> L[i].x = 1
        } else {
            a[i] = make_float4(r[0], r[1], r[2], r[6]);
            b[i] = make_float4(r[3], r[4], r[5], r[7]);
        }
    }
    std::vector<float4> out(n, make_float4(INFINITY, 0.f, 0.f, 0.f));
    if (!shadow) {
        const uint32_t miss = 0xFFFFFFFFu;
        for (auto &o : out) memcpy(&o.w, &miss, 4);
    } else {
        for (auto &o : out) o = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    hipError_t e = hipSuccess;
    DevBuf<float4> da(e, n, a.data()), db(e, n, b.data()), dout(e, n, out.data()), dc(e, c.size(), c.data());
    DevBuf<uint32_t> hitInst(e, s->ds.inst ? n : 0), tie(e, shadow ? 0 : n), cnt(e, CNT_WORDS);
    DevBuf<unsigned long long> ctr(e, CTR_WORDS);
    hitInst.zero();
    tie.zero();
    cnt.zero();
    ctr.zero();
    DevPaths D{};
    (shadow ? D.sh_o : D.ray_o) = da.p;
    (shadow ? D.sh_d : D.ray_d) = db.p;
    (shadow ? D.L : D.hit) = dout.p;
    D.sh_c = dc.p;
    D.hitInst = hitInst.p;
    D.tie = tie.p;
    D.cnt = cnt.p;
    D.ctr = ctr.p;
    const bool pre = presetup_applies(s);
    DevBuf<float4> dpre(e, pre && !shadow ? n : 0), da2(e, pre && shadow ? n : 0), db2(e, pre && shadow ? n : 0), dc2(e, pre && shadow ? n : 0);
    if (e == hipSuccess && shadow && !pre) e = hipMemcpy(D.cnt + CNT_S0, &n, sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    if (pre) {
        const DevPaths Q = D;
        if (shadow) { D.sh_o = da2.p; D.sh_d = db2.p; D.sh_c = dc2.p; }
        else D.pre = dpre.p;
        hipLaunchKernelGGL(k_query_pre, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, D, Q, n, shadow ? 1 : 0);
    }
    if (shadow) launch_trace(s, false, D, -2, 0, 0u, s->stream, pre);
    else launch_trace(s, false, D, -1, -1, n, s->stream, pre);
    e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipGetLastError();
    dout.download(out.data());
    uint32_t err = 0;
    if (e == hipSuccess) e = hipMemcpy(&err, D.cnt + CNT_ERR, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    if (err & CNT_ERR_TRAVERSAL) { g_err = traversal_error; return MTSG_ERR_TRAVERSAL; }
    for (uint32_t i = 0; i < n; ++i) {
        if (shadow) {
            occ[i] = out[i].x == 0.f ? 1 : 0;
        } else {
            uint32_t pb2;
            memcpy(&pb2, &out[i].w, 4);
            prim[i] = pb2;   // triangle index, 0x80000000 | rectangle index, or ~0 (miss)
            t[i] = out[i].x; u[i] = out[i].y; v[i] = out[i].z;
        }
    }
    return MTSG_OK;
}

int mtsg_env_eval(mtsg_scene *s, uint32_t n, const float *dirs, const float *rx, const float *ry, float *out) {
    if (!s || (!dirs && n) || (!out && n) || ((rx == nullptr) != (ry == nullptr))) { g_err = "invalid arguments"; return MTSG_ERR_INVALID; }
    if (!(s->ds.has_env & 1)) { g_err = "scene has no environment emitter"; return MTSG_ERR_INVALID; }
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const size_t n3 = (size_t)n * 3;
    hipError_t e = hipSuccess;
    DevBuf<float> dd(e, n3, dirs), dout(e, n3), dx(e, rx ? n3 : 0, rx), dy(e, ry ? n3 : 0, ry);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_env_eval, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, dd.p, dx.p, dy.p, n, dout.p);
        e = hipStreamSynchronize(s->stream);
    }
    dout.download(out);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

int mtsg_tex_eval(mtsg_scene *s, int tex, uint32_t n, const float *uv, const float *duv, float *out) {
    if (!s || (!uv && n) || (!out && n)) { g_err = "invalid arguments"; return MTSG_ERR_INVALID; }
    if (tex < 0 || (uint32_t)tex >= s->nTextures) { g_err = "texture index out of range"; return MTSG_ERR_INVALID; }
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    hipError_t e = hipSuccess;
    DevBuf<float> dd(e, (size_t)n * 2, uv), dout(e, (size_t)n * 3), duv_d(e, duv ? (size_t)n * 4 : 0, duv);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tex_eval, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, tex, dd.p, duv_d.p, n, dout.p);
        e = hipStreamSynchronize(s->stream);
    }
    dout.download(out);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

int mtsg_om_query(mtsg_scene *s, uint32_t n, const float *dirs, const float *o1, const float *o2, int32_t *ids, int32_t *vis) {
    if (!s || (n && (!dirs || !o1 || !o2 || !ids || !vis))) { g_err = "invalid arguments"; return MTSG_ERR_INVALID; }
    if (!s->ds.om) { g_err = "scene has no occupancy maps"; return MTSG_ERR_INVALID; }
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const size_t n3 = (size_t)n * 3;
    hipError_t e = hipSuccess;
    DevBuf<float> dd(e, n3, dirs), d1(e, n3, o1), d2(e, n3, o2);
    DevBuf<int32_t> di(e, n), dv(e, n);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_om_query, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, dd.p, d1.p, d2.p, n, di.p, dv.p);
        e = hipStreamSynchronize(s->stream);
    }
    di.download(ids);
    dv.download(vis);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

}  // extern "C"

namespace {
// mtsg_bsdf_query: bsdf_sample / bsdf_eval as the shading kernels call them,
// at the widest EXT level, one thread per query; alb is the caller's, or the
// constant of the record that answers: the back record of a twosided front
// record where bsdf_eval (wi.z <= 0) or bsdf_sample (wi.z < 0) hands over to it
__global__ void k_bsdf_query(DevScene S, int bsdf, int mode, uint32_t n, const float *in, const float *albIn, float *out,
                             uint32_t *flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *q = in + 6 * (size_t)i;
    const mtsg_bsdf &b = S.bsdfs[bsdf];
    const float3 wi = mk3(q[0], q[1], q[2]);
    const bool back = b.twosided && (mode == MTSG_BSDF_QUERY_EVAL ? !(wi.z > 0) : wi.z < 0);
    const mtsg_bsdf &eff = back ? S.bsdfs[b.back] : b;
    const float3 alb = albIn ? ld3(albIn + 3 * (size_t)i) : ld3(eff.reflectance);
    if (mode == MTSG_BSDF_QUERY_EVAL) {
        float pdf;
        const float3 v = bsdf_eval<2>(S.bsdfs, b, alb, wi, mk3(q[3], q[4], q[5]), pdf);
        float *o = out + 4 * (size_t)i;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = pdf;
        if (flags) flags[i] = MTSG_BSDF_QUERY_OK;
        return;
    }
    BsdfSample r;
    r.wo = r.weight = mk3(0, 0, 0);
    r.pdf = 0.0f;
    const float u = q[5];
    const bool ok = bsdf_sample<2>(S.bsdfs, b, alb, wi, q[3], q[4], r, [&]() { return u; });
    float *o = out + 8 * (size_t)i;
    if (ok) {
        o[0] = r.wo.x; o[1] = r.wo.y; o[2] = r.wo.z;
        o[3] = r.weight.x; o[4] = r.weight.y; o[5] = r.weight.z;
        o[6] = r.pdf; o[7] = r.eta;
        flags[i] = MTSG_BSDF_QUERY_OK | ((r.delta & 1u) ? MTSG_BSDF_QUERY_DELTA : 0u) | ((r.delta & 2u) ? MTSG_BSDF_QUERY_NULL : 0u);
    } else {
        for (int k = 0; k < 8; ++k) o[k] = 0.0f;
        flags[i] = 0u;
    }
}
}  // namespace

extern "C" int mtsg_bsdf_query(mtsg_scene *s, int32_t bsdf, int32_t mode, uint32_t n, const float *in, const float *alb, float *out,
                               uint32_t *flags) {
    if (!s || (n && (!in || !out)) || (mode != MTSG_BSDF_QUERY_SAMPLE && mode != MTSG_BSDF_QUERY_EVAL) ||
        (mode == MTSG_BSDF_QUERY_SAMPLE && n && !flags)) {
        g_err = "invalid arguments";
        return MTSG_ERR_INVALID;
    }
    if (bsdf < 0 || (uint32_t)bsdf >= s->ds.n_bsdfs) { g_err = "BSDF index out of range"; return MTSG_ERR_INVALID; }
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    const size_t no = mode == MTSG_BSDF_QUERY_EVAL ? 4 : 8;
    hipError_t e = hipSuccess;
    DevBuf<float> din(e, (size_t)n * 6, in), dalb(e, alb ? (size_t)n * 3 : 0, alb), dout(e, (size_t)n * no);
    DevBuf<uint32_t> df(e, flags ? n : 0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bsdf_query, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, (int)bsdf, (int)mode, n, din.p, dalb.p, dout.p, df.p);
        e = hipStreamSynchronize(s->stream);
    }
    dout.download(out);
    if (flags) df.download(flags);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

namespace mtsg {
void set_last_error(const std::string &e) { g_err = e; }   // kdbuild.hip
}

namespace {
// A: the handle's sample array requests; a negative kind reads the next one
__global__ void k_sampler_draws(DevIntegrator I, DevArrays A, int x, int y, uint32_t s, uint32_t n, const int32_t *kinds, float *out,
                                int *err) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PathSampler p = path_sampler(I, x, y, s, 0, 0);
    uint32_t req = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int t = I.smp.type;
        if (kinds[i] < 0) {   // next2DArray(-kinds[i])
            const uint32_t r = req++, m = (uint32_t)(-kinds[i]);
            const uint64_t pix = pixel_index(I, p);
            for (uint32_t k = 0; k < m; ++k) {
                float a, b;
                if (t == MTSG_SAMPLER_HALTON) smp_array2D<MTSG_SAMPLER_HALTON>(I.smp, p, I.seed, pix, I.spp, r, m, k, a, b);
                else if (t == MTSG_SAMPLER_LDSAMPLER) smp_array2D<MTSG_SAMPLER_LDSAMPLER>(I.smp, p, I.seed, pix, I.spp, r, m, k, a, b);
                else if (t == MTSG_SAMPLER_SOBOL) smp_array2D<MTSG_SAMPLER_SOBOL>(I.smp, p, I.seed, pix, I.spp, r, m, k, a, b);
                else smp_array2D<MTSG_SAMPLER_INDEPENDENT>(I.smp, p, I.seed, pix, I.spp, r, m, k, a, b);
                *out++ = a;
                *out++ = b;
            }
            continue;
        }
        if (t == MTSG_SAMPLER_HALTON) smp_skip_arrays<MTSG_SAMPLER_HALTON>(p, A.count, kinds[i] == 2 ? 2 : 1);
        else if (t == MTSG_SAMPLER_SOBOL) smp_skip_arrays<MTSG_SAMPLER_SOBOL>(p, A.count, kinds[i] == 2 ? 2 : 1);
        if (kinds[i] == 2) {
            float a, b;
            if (t == MTSG_SAMPLER_HALTON) next2D<MTSG_SAMPLER_HALTON>(I, p, a, b);
            else if (t == MTSG_SAMPLER_HAMMERSLEY) next2D<MTSG_SAMPLER_HAMMERSLEY>(I, p, a, b);
            else if (t == MTSG_SAMPLER_LDSAMPLER) next2D<MTSG_SAMPLER_LDSAMPLER>(I, p, a, b);
            else if (t == MTSG_SAMPLER_SOBOL) next2D<MTSG_SAMPLER_SOBOL>(I, p, a, b);
            else next2D<MTSG_SAMPLER_INDEPENDENT>(I, p, a, b);
            *out++ = a;
            *out++ = b;
        } else {
            float a;
            if (t == MTSG_SAMPLER_HALTON) a = next1D<MTSG_SAMPLER_HALTON>(I, p);
            else if (t == MTSG_SAMPLER_HAMMERSLEY) a = next1D<MTSG_SAMPLER_HAMMERSLEY>(I, p);
            else if (t == MTSG_SAMPLER_LDSAMPLER) a = next1D<MTSG_SAMPLER_LDSAMPLER>(I, p);
            else if (t == MTSG_SAMPLER_SOBOL) a = next1D<MTSG_SAMPLER_SOBOL>(I, p);
            else a = next1D<MTSG_SAMPLER_INDEPENDENT>(I, p);
            *out++ = a;
        }
    }
    *err = p.dimError ? 1 : 0;
}

// mtsg_camera_rays: the camera rays of the listed slots as bounce 0 reads
// them (load_closest_ray), and the differentials k_camera parked in T / aux
__global__ void k_camera_rays_read(DevScene S, DevPaths P, const uint32_t *slots, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = slots[i];
    float4 ro, rd;
    load_closest_ray(S, P, slot, P.camEnc != 0, ro, rd);
    const float4 rx = ldS(&P.T[slot]), ry = ldS(&P.aux[slot]);
    float *o = out + (size_t)14 * i;
    o[0] = ro.x; o[1] = ro.y; o[2] = ro.z;
    o[3] = rd.x; o[4] = rd.y; o[5] = rd.z;
    o[6] = ro.w; o[7] = rd.w;
    o[8] = rx.x; o[9] = rx.y; o[10] = rx.z;
    o[11] = ry.x; o[12] = ry.y; o[13] = ry.z;
}
}  // namespace

extern "C" {

int mtsg_sampler_draws(mtsg_scene *s, const mtsg_render_params *p, int x, int y, uint32_t si, uint32_t n,
                       const int32_t *kinds, float *out) {
    if (!s || !p || (n && (!kinds || !out)) || p->spp == 0) { g_err = "invalid arguments"; return MTSG_ERR_INVALID; }
    if (n == 0) return MTSG_OK;
    int rc;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    // the array requests of the handle's descriptor (`direct`'s when it has
    // any, else `ao`'s); kinds[i] = -n reads them in order
    DevArrays A{};
    if (s->directOn) {
        A = fan_arrays(s->direct.emitter_samples, s->direct.bsdf_samples);
        if (!A.count) A = fan_arrays(s->direct.ao_samples, 0);
    }
    uint32_t nOut = 0, req = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (kinds[i] < 0) {
            if (s->samplerType == MTSG_SAMPLER_HAMMERSLEY) { g_err = hammersley_array_error; return MTSG_ERR_INVALID; }
            if (kinds[i] > -2 || req >= A.count || A.n[req] != (uint32_t)(-kinds[i]) || (uint64_t)A.n[req] * p->spp > MAX_ARRAY_ENTRIES) {
                g_err = "mtsg_sampler_draws: kinds[i] = -n must name the next sample array of the handle's mtsg_direct_desc";
                return MTSG_ERR_INVALID;
            }
            ++req;
            nOut += 2 * (uint32_t)(-kinds[i]);
        } else {
            nOut += kinds[i] == 2 ? 2 : 1;
        }
    }
    DevIntegrator I{p->max_depth, p->rr_depth, p->strict_normals, p->hide_emitters, p->spp, p->seed,
                    (uint32_t)s->cam.film_w, make_sampler(s, p->spp)};
    hipError_t e = hipSuccess;
    DevBuf<int32_t> dk(e, n, kinds);
    DevBuf<float> dout(e, nOut);
    DevBuf<int> derr(e, 1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sampler_draws, dim3(1), dim3(64), 0, s->stream, I, A, x, y, si, n, dk.p, dout.p, derr.p);
        e = hipStreamSynchronize(s->stream);
    }
    int err = 0;
    dout.download(out);
    derr.download(&err);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    if (err) {
        g_err = dim_error(s->samplerType);
        return MTSG_ERR_INVALID;
    }
    return MTSG_OK;
}

int mtsg_camera_rays(mtsg_scene *s, const mtsg_render_params *p, uint32_t n, const int32_t *xys, float *out) {
    if (!s || (n && (!xys || !out))) { g_err = "invalid arguments"; return MTSG_ERR_INVALID; }
    int rc;
    if ((rc = validate(p, s)) != MTSG_OK) return rc;
    if (n == 0) return MTSG_OK;
    if ((rc = set_device(s)) != MTSG_OK) return rc;
    // one batch over the whole rectangle and every sample: k_camera's own launch
    const uint32_t tilesX = (uint32_t)(p->tile_w + TILE - 1) / TILE, tilesY = (uint32_t)(p->tile_h + TILE - 1) / TILE;
    const uint64_t nslots64 = (uint64_t)tilesX * tilesY * TILE * TILE * p->spp;
    if (nslots64 > (1u << 22)) { g_err = "camera_rays: rectangle x spp exceeds 2^22 sample slots"; return MTSG_ERR_INVALID; }
    const uint32_t nslots = (uint32_t)nslots64;
    const DevBatch B{p->tile_x, p->tile_y, p->tile_w, p->tile_h, (int)tilesX, 0, (int)(tilesX * tilesY), 1, 0, PLAN_DEAL_SKEW,
                     0u, p->spp, nslots, nullptr, s->cam.lens ? 1u : 0u};
    // the slot of each (x, y, s): the inverse of slot_pixel
    std::vector<uint32_t> tileOf((size_t)tilesX * tilesY), pixOf(TILE * TILE), slots(n);
    for (uint32_t v = 0; v < tilesX * tilesY; ++v) {
        int tx, ty;
        tile_of_key((int)v, (int)tilesX, tx, ty, PLAN_DEAL_SKEW);
        tileOf[(size_t)ty * tilesX + tx] = v;
    }
    for (uint32_t pix = 0; pix < TILE * TILE; ++pix) {
        int lx, ly;
        tile_pix(pix, lx, ly);
        pixOf[ly * TILE + lx] = pix;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const int x = xys[3 * i] - p->tile_x, y = xys[3 * i + 1] - p->tile_y, si = xys[3 * i + 2];
        if (x < 0 || y < 0 || x >= p->tile_w || y >= p->tile_h || si < 0 || (uint32_t)si >= p->spp) {
            g_err = "camera_rays: a sample lies outside the rectangle or the sample count";
            return MTSG_ERR_INVALID;
        }
        const uint32_t v = tileOf[(size_t)(y / TILE) * tilesX + x / TILE];
        slots[i] = ((v * p->spp + (uint32_t)si) * (TILE * TILE)) + pixOf[(y % TILE) * TILE + x % TILE];
    }
    DevIntegrator I{p->max_depth, p->rr_depth, p->strict_normals, p->hide_emitters, p->spp, p->seed, (uint32_t)s->cam.film_w,
                    make_sampler(s, p->spp)};
    I.om = p->integrator == MTSG_INTEGRATOR_PATH2_OM ? 1 : 0;
    I.om_strategy = p->om_strategy;
    I.om_mis = p->om_mis;
    I.om_jitter = p->om_jitter;
    DevCamera cam = s->cam;
    cam.diffs = 1;   // the differentials too (myPath2_OM has none: zeros)
    hipError_t e = hipSuccess;
    DevBuf<float4> ro(e, nslots), rd(e, nslots), T(e, nslots), aux(e, nslots), L(e, nslots);
    DevBuf<uint4> meta(e, nslots);
    DevBuf<uint32_t> dslots(e, n, slots.data());
    DevBuf<float> dout(e, (size_t)14 * n);
    if (e == hipSuccess) e = hipMemsetAsync(T.p, 0, nslots * sizeof(float4), s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(aux.p, 0, nslots * sizeof(float4), s->stream);
    if (e == hipSuccess) {
        DevPaths P{};
        P.ray_o = ro.p; P.ray_d = rd.p; P.T = T.p; P.aux = aux.p; P.L = L.p; P.meta = meta.p;
        P.camEnc = s->ds.camCompact ? 1u : 0u;
        const dim3 g((nslots + BLOCK - 1) / BLOCK);
        if (cam.lens) hipLaunchKernelGGL(k_camera_lens<false>, g, dim3(BLOCK), 0, s->stream, s->ds, cam, I, B, P);
        else hipLaunchKernelGGL(k_camera<false>, g, dim3(BLOCK), 0, s->stream, s->ds, cam, I, B, P);
        hipLaunchKernelGGL(k_camera_rays_read, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->ds, P, dslots.p, n, dout.p);
        e = hipStreamSynchronize(s->stream);
    }
    dout.download(out);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return MTSG_ERR_DEVICE; }
    return MTSG_OK;
}

int mtsg_trace_closest(mtsg_scene *s, uint32_t n, const float *rays, float *t, float *u, float *v, uint32_t *prim) {
    return trace_rays(s, n, rays, t, u, v, prim, nullptr, false);
}

int mtsg_trace_shadow(mtsg_scene *s, uint32_t n, const float *rays, uint8_t *occluded) {
    return trace_rays(s, n, rays, nullptr, nullptr, nullptr, nullptr, occluded, true);
}

void mtsg_scene_destroy(mtsg_scene *s) {
    if (!s) return;
    hipSetDevice(s->device);
    if (s->stream) hipStreamSynchronize(s->stream);
    free_batch(s);
    for (void *p : s->allocs) hipFree(p);
    for (hipEvent_t e : s->evPool) hipEventDestroy(e);
    if (s->hostCnt) hipHostFree(s->hostCnt);
    if (s->waveTimes) hipFree(s->waveTimes);
    for (int l = 1; l < MTSG_MAX_LANES; ++l)
        if (s->lstream[l]) hipStreamDestroy(s->lstream[l]);
    if (s->stream) hipStreamDestroy(s->stream);
    if (s->tileKeysDev) hipFree(s->tileKeysDev);
    free_aov(s);
    delete s;
}

void mtsg_last_error(char *buf, size_t size) {
    if (!buf || !size) return;
    strncpy(buf, g_err.c_str(), size - 1);
    buf[size - 1] = 0;
}

}  // extern "C"
