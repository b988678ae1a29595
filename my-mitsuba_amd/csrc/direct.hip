// direct.hip -- the `direct` and `ao` integrators
// (src/integrators/direct/direct.cpp:146-309, ao.cpp:84-125).
//
// Both shoot a fan of rays from the camera ray's hit: `direct` emitterSamples
// shadow rays and bsdfSamples BSDF rays, `ao` shadingSamples occlusion rays.
// A batch is
//   k_camera -> trace (camera rays) -> k_direct_shade -> trace (BSDF rays +
//   shadow rays, one launch) -> k_direct_resolve -> k_splat
// with the unchanged traversal kernels.  The fan lives in its own DevPaths
// (DevDirect::F), which shares the batch's counters:
//   BSDF ray j of sample slot    closest ray slot * nb + j (identity work list);
//                                a sample that sends none stores a dead ray
//                                (maxt < 0, as the camera's dead slots)
//   shadow rays                  appended to the shadow list (workgroup-
//                                aggregated, as k_shade appends); ray i of a
//                                sample accumulates into its private cell
//                                F.Lp[slot * ne + i] (zeroed per batch), so
//                                shadow_unoccluded's read-modify-write has one
//                                writer per target
// k_direct_resolve sums a sample's cells and then its BSDF rays' emitter hits
// in index order, so a render is reproducible whatever order the rays finish in.
// Random numbers: a technique with one sample draws the sampler's next 2D
// number, one with more reads its sample array (sampler.h smp_array2D).
#pragma clang diagnostic ignored "-Wunused-function"
#include "kernels.h"

namespace {

// regular draws next to sample arrays: halton / sobol skip the reserved dimensions
template <int SMP>
DEV void reg2D(const DevIntegrator &I, const DevArrays &A, PathSampler &p, float &a, float &b) {
    smp_skip_arrays<SMP>(p, A.count, 2);
    next2D<SMP>(I, p, a, b);
}
template <int SMP>
DEV float reg1D(const DevIntegrator &I, const DevArrays &A, PathSampler &p) {
    smp_skip_arrays<SMP>(p, A.count, 1);
    return next1D<SMP>(I, p);
}
template <int SMP>
DEV void array2D(const DevIntegrator &I, const PathSampler &p, uint32_t r, uint32_t n, uint32_t k, float &a, float &b) {
    smp_array2D<SMP>(I.smp, p, I.seed, pixel_index(I, p), I.spp, r, n, k, a, b);
}

// workgroup-aggregated append to one list (block_append2 with one list);
// every thread of the workgroup calls it
DEV uint32_t block_append1(BlockAppend &ba, uint32_t *gcnt, bool p) {
    if (threadIdx.x == 0) ba.cnt[0] = 0;
    __syncthreads();
    const unsigned long long m = __ballot(p);
    const unsigned long long below = (1ull << lane_id()) - 1ull;
    uint32_t w = 0;
    if (lane_id() == 0 && m) w = atomicAdd(&ba.cnt[0], (uint32_t)__popcll(m));
    w = __shfl(w, 0);
    __syncthreads();
    if (threadIdx.x == 0) ba.base[0] = ba.cnt[0] ? atomicAdd(gcnt, ba.cnt[0]) : 0u;
    __syncthreads();
    return ba.base[0] + w + (uint32_t)__popcll(m & below);
}

// One thread per camera sample, after the camera rays' trace launch.
// direct.cpp:156-306 in order; ao.cpp:91-120.  Writes the sample's emitted
// radiance (ao: the value of a miss) and alpha to P.L, its refN to P.aux, and
// the fan to D.F.
// MATS: the material classes compiled in, as k_shade's (kernels.h MAT_*).
template <int ENV, int SMP, int EXT, int MATS = MATS_ALL>
__global__ void __launch_bounds__(BLOCK) k_direct_shade(DevScene S, DevIntegrator I, DevBatch B, DevPaths P, DevDirect D, int hasAlpha) {
    __shared__ BlockAppend ba;
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    const bool inBatch = slot < B.nslots;
    const bool alive = inBatch && camera_meta(B, slot).x != 0u;
    const DevPaths &F = D.F;
    bool sampleOn = false;   // the sample reached the sampling loops
    Its its;
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    float3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1), wi = mk3(0, 0, 1), alb = mk3(0, 0, 0), refN = mk3(0, 0, 0);
    uint32_t inst = 0xFFFFFFFFu;
    int bsdfIdx = 0;
    PathSampler smp{};
    if (alive) {
        h = ldS(&P.hit[slot]);
        float4 ro4, rd4;
        load_closest_ray(S, P, slot, S.camCompact != 0, ro4, rd4);
        ro = xyz(ro4);
        rd = xyz(rd4);
        int x, y;
        uint32_t sIdx;
        slot_pixel(B, slot, x, y, sIdx);
        // after the camera's pixel jitter and a thinlens sensor's aperture sample (camera_meta)
        smp = path_sampler(I, x, y, sIdx, 2u + 2u * B.sensorDraws, 1u + B.sensorDraws);
        const bool valid = __float_as_uint(h.w) != 0xFFFFFFFFu;
        float3 L = mk3(0, 0, 0);
        // RadianceQueryRecord::rayIntersect (records.inl:117-143)
        const float alpha = hasAlpha ? (valid ? 1.0f : 0.0f) : 1.0f;
        // the camera ray's scaled differentials, parked in T / aux (k_camera)
        float3 rxd = mk3(0, 0, 0), ryd = mk3(0, 0, 0);
        if (S.cam_diffs) {
            rxd = xyz(ldS(&P.T[slot]));
            ryd = xyz(ldS(&P.aux[slot]));
        }
        if (!valid) {
            if (D.ao) {
                L = mk3(1.f, 1.f, 1.f);   // ao.cpp:91-95
            } else if (ENV == EM_ALL && !(S.has_env & 1)) {   // a constant environment, or none
                if (constant_emitter(S) >= 0 && !I.hide_emitters) L = L + ld3(S.emitters[constant_emitter(S)].radiance);
            } else if (ENV && !I.hide_emitters) {   // Scene::evalEnvironment of the differential camera ray
                if (!S.cam_diffs) camera_ray_differentials<SMP>(*S.camDev, I, x, y, sIdx, rxd, ryd);
                L = L + env_eval(S.env, rd, true, rxd, ryd);
            }
        } else {
            inst = S.inst ? P.hitInst[slot] : 0xFFFFFFFFu;
            fill_its(S, ro, rd, h, inst, its);
            if (D.ao) {
                sampleOn = true;
            } else {
                const mtsg_bsdf &bsdf = S.bsdfs[its.bsdf];
                bsdfIdx = its.bsdf;
                wi = its.sh.toLocal(-rd);
                if (EXT) {
                    const mtsg_bsdf &eff = (bsdf.twosided && !(wi.z > 0)) ? S.bsdfs[bsdf.back] : bsdf;
                    alb = eff.texture ? texture_eval(S, eff.texture - 1, h, inst, its, ro, S.cam_diffs != 0, rxd, ryd)
                                      : ld3(eff.reflectance);
                } else {
                    alb = ld3(bsdf.reflectance);
                }
                if (its.emitter >= 0 && !I.hide_emitters && dot(its.sh.n, -rd) > 0) L = L + ld3(S.emitters[its.emitter].radiance);
                sampleOn = !(I.strict_normals && dot(rd, its.geoN) * wi.z >= 0);   // direct.cpp:175-187
                refN = bsdf.ref_n_zero ? mk3(0, 0, 0) : its.sh.n;
            }
        }
        stS(&P.L[slot], make_float4(L.x, L.y, L.z, alpha));
        if (sampleOn && !D.ao) stS(&P.aux[slot], make_float4(refN.x, refN.y, refN.z, 0.f));
    }

    // ---- emitter sampling (direct.cpp:210-245) / occlusion rays (ao.cpp:113-120)
    // the draw is taken whatever the BSDF and the count are (direct.cpp:210-214)
    float ex = 0.f, ey = 0.f;
    if (sampleOn && D.ne <= 1) reg2D<SMP>(I, D.arrays, smp, ex, ey);
    for (uint32_t i = 0; i < D.ne; ++i) {
        bool emit = false;
        float4 so = make_float4(0.f, 0.f, 0.f, 0.f), sd = so;
        float3 c = mk3(0, 0, 0);
        if (sampleOn) {
            float sx = ex, sy = ey;
            if (D.ne > 1) array2D<SMP>(I, smp, 0u, D.ne, i, sx, sy);
            if (D.ao) {
                const float3 d = its.sh.toWorld(cosine_hemisphere(sx, sy));
                so = make_float4(its.p.x, its.p.y, its.p.z, D.rayLength);
                sd = make_float4(d.x, d.y, d.z, kEpsilon);
                c = mk3(1.f, 1.f, 1.f);
                emit = true;
            } else if (S.bsdfs[bsdfIdx].smooth) {
                const mtsg_bsdf &bsdf = S.bsdfs[bsdfIdx];
                // Scene::sampleEmitterDirect, as shade_path (kernels.h) takes it
                float emPdf;
                const uint32_t ei = pmf_sample_reuse(S.emitter_cdf, S.n_emitters, sx, emPdf);
                const mtsg_emitter &E = S.emitters[ei];
                float3 dd, value;
                float dist, pdf;
                bool accepted, delta = false;
                if (ENV && E.type == MTSG_EMITTER_ENVMAP) {
                    accepted = env_sample_direct(S.env, its.p, sx, sy, dd, dist, value, pdf);
                } else if (ENV == EM_ALL && E.type >= MTSG_EMITTER_POINT) {
                    accepted = emitter_sample_ext(S, E, ei, its.p, refN, sx, sy, dd, dist, value, pdf, delta);
                } else {
                    float3 ep, en;
                    emitter_sample_position(S, E, ei, sx, sy, ep, en);
                    dd = ep - its.p;
                    const float distSquared = dot(dd, dd);
                    dist = sqrtf(distSquared);
                    dd = dd / dist;
                    const float dp = fabsf(dot(dd, en));
                    pdf = E.inv_area * (dp != 0 ? (distSquared / dp) : 0.0f);
                    accepted = dot(dd, refN) >= 0 && dot(dd, en) < 0 && pdf != 0;
                    if (accepted) value = ld3(E.radiance) / pdf;
                }
                if (accepted) {
                    pdf *= emPdf;
                    value = value / emPdf;
                    const float3 wo = its.sh.toLocal(dd);
                    float bpdf;
                    const float3 bval = bsdf_eval<EXT, MATS>(S.bsdfs, bsdf, alb, wi, wo, bpdf);
                    if (!isZero(bval) && (!I.strict_normals || dot(its.geoN, dd) * wo.z > 0)) {
                        // direct.cpp:235-239: the BSDF pdf enters only for emitters on a surface sampled in solid angle
                        const float weight = mis(pdf * D.fracLum, (ENV == EM_ALL && delta) ? 0.0f : bpdf * D.fracBSDF) * D.weightLum;
                        c = value * bval * weight;
                        if (!isZero(c)) {
                            emit = true;
                            so = make_float4(its.p.x, its.p.y, its.p.z, dist * (1 - kShadowEpsilon));
                            sd = make_float4(dd.x, dd.y, dd.z, kEpsilon);
                        }
                    }
                }
            }
        }
        const uint32_t pos = block_append1(ba, &P.cnt[CNT_S0], emit);
        if (emit) {
            stS(&F.sh_o[pos], so);
            stS(&F.sh_d[pos], sd);
            stS(&F.sh_c[pos], make_float4(c.x, c.y, c.z, __uint_as_float(slot * D.ne + i)));   // its cell in F.Lp
        }
    }

    // ---- BSDF sampling (direct.cpp:251-306, up to the ray)
    float bx = 0.f, by = 0.f;
    if (sampleOn && D.nb == 1) reg2D<SMP>(I, D.arrays, smp, bx, by);
    uint32_t live = 0;
    for (uint32_t j = 0; j < D.nb; ++j) {
        bool emit = false;
        BsdfSample bs;
        float3 wo = mk3(0, 0, 1);
        if (sampleOn) {
            float sx = bx, sy = by;
            if (D.nb > 1) array2D<SMP>(I, smp, D.ne > 1 ? 1u : 0u, D.nb, j, sx, sy);
            if (bsdf_sample<EXT, MATS>(S.bsdfs, S.bsdfs[bsdfIdx], alb, wi, sx, sy, bs, [&]() { return reg1D<SMP>(I, D.arrays, smp); })) {
                wo = its.sh.toWorld(bs.wo);
                emit = !(I.strict_normals && dot(its.geoN, wo) * bs.wo.z <= 0);
            }
        }
        if (inBatch) {
            const size_t pos = (size_t)slot * D.nb + j;
            if (emit) {
                stS(&F.ray_o[pos], make_float4(its.p.x, its.p.y, its.p.z, kEpsilon));
                stS(&F.ray_d[pos], make_float4(wo.x, wo.y, wo.z, INFINITY));
                stS(&D.val[pos], make_float4(bs.weight.x, bs.weight.y, bs.weight.z, bs.pdf));
                D.flag[pos] = EXT >= 2 ? bs.delta : (bs.delta ? 1u : 0u);
                ++live;
            } else {   // no ray: the traversal skips it and writes no hit
                stS(&F.ray_o[pos], make_float4(0.f, 0.f, 0.f, 0.f));
                stS(&F.ray_d[pos], make_float4(0.f, 0.f, 1.f, -1.0f));
            }
        }
    }
    if (D.nb) {   // the BSDF rays actually sent (mtsg_stats::rays_closest)
        // one global atomic per workgroup: a contended word takes ~11 ns per
        // atomic, and a wave-level add here cost as much as the rest of the kernel
        for (int o = 32; o > 0; o >>= 1) live += __shfl_down(live, o);
        if (threadIdx.x == 0) ba.cnt[1] = 0;
        __syncthreads();
        if (lane_id() == 0 && live) atomicAdd(&ba.cnt[1], live);
        __syncthreads();
        if (threadIdx.x == 0 && ba.cnt[1]) atomicAdd(&P.cnt[CNT_Q1], ba.cnt[1]);
    }
    if ((SMP == MTSG_SAMPLER_HALTON || SMP == MTSG_SAMPLER_SOBOL || SMP == MTSG_SAMPLER_HAMMERSLEY) && smp.dimError)
        atomicOr(&P.cnt[CNT_ERR], CNT_ERR_QMC_DIM);
}

// One thread per camera sample, after the fan's trace launch: Li = Le + the
// shadow rays' cells in index order, then the BSDF rays' emitter or
// environment hits in index order (direct.cpp:276-305); ao: the mean of the
// cells (ao.cpp:118-122).
// NULLEV: the scene's BSDFs can sample a null event (EXT level 2)
template <int ENV, bool NULLEV = false>
__global__ void __launch_bounds__(BLOCK) k_direct_resolve(DevScene S, DevIntegrator I, DevBatch B, DevPaths P, DevDirect D) {
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= B.nslots || camera_meta(B, slot).x == 0u) return;
    const DevPaths &F = D.F;
    const float4 L4 = ldS(&P.L[slot]);
    float3 L = xyz(L4);
    const bool valid = __float_as_uint(ldS(&P.hit[slot]).w) != 0xFFFFFFFFu;
    if (!valid) return;   // P.L is final: the environment, 0, or ao's 1
    if (D.ao) L = mk3(0, 0, 0);
    for (uint32_t i = 0; i < D.ne; ++i) L = L + xyz(ldS(&F.Lp[(size_t)slot * D.ne + i]));
    if (D.ao) {
        const float recip = 1.0f / (float)D.ne;   // Spectrum::operator/= (spectrum.h:447-456)
        L = L * recip;
    }
    if (D.nb) {
        const float3 refN = xyz(ldS(&P.aux[slot]));
        for (uint32_t j = 0; j < D.nb; ++j) {
            const size_t pos = (size_t)slot * D.nb + j;
            const float4 rd4 = ldS(&F.ray_d[pos]);
            if (rd4.w < 0.0f) continue;   // no ray
            const float3 ro = xyz(ldS(&F.ray_o[pos])), rd = xyz(rd4);
            const float4 h = ldS(&F.hit[pos]);
            const float4 bv = ldS(&D.val[pos]);
            const bool delta = D.flag[pos] != 0u;
            float3 value;
            float lumPdf = 0.0f;
            if (__float_as_uint(h.w) == 0xFFFFFFFFu) {
                // the environment, if any (direct.cpp:285-294): hideEmitters
                // hides it from a null event (thindielectric's transmission)
                if (!ENV) continue;
                if (NULLEV && I.hide_emitters && (D.flag[pos] & 2u)) continue;
                if (ENV == EM_ALL && !(S.has_env & 1)) {   // a constant environment, or none
                    const int ce = constant_emitter(S);
                    float pdfSA;
                    if (ce < 0 || !constant_miss(S, (uint32_t)ce, ro, rd, refN, pdfSA)) continue;
                    const float lp = delta ? 0.0f : pdfSA * S.emitters[ce].pdf_discrete;
                    const float w = mis(bv.w * D.fracBSDF, lp * D.fracLum) * D.weightBSDF;
                    L = L + ld3(S.emitters[ce].radiance) * xyz(bv) * w;
                    continue;
                }
                const float3 v = env_rot(S.env.E->to_local, rd);
                float ux, uy;
                env_uv(v, ux, uy);
                value = env_eval_uv(S.env, v, ux, uy, false, rd, rd);
                float nearT, farT;
                if (!(env_sphere(S.env, ro, rd, nearT, farT) && !(nearT > 0) && !(farT < 0))) continue;   // fillDirectSamplingRecord
                if (!delta) lumPdf = env_internal_pdf_uv(S.env, v, ux, uy) * S.emitters[S.env.E->emitter].pdf_discrete;
            } else {
                Its its;
                fill_its(S, ro, rd, h, S.inst ? F.hitInst[pos] : 0xFFFFFFFFu, its);
                if (its.emitter < 0) continue;
                const mtsg_emitter &E = S.emitters[its.emitter];
                value = dot(its.sh.n, -rd) > 0 ? ld3(E.radiance) : mk3(0, 0, 0);
                if (!delta) {   // Scene::pdfEmitterDirect with dRec.setQuery(ray, its), as shade_path
                    if (dot(rd, refN) >= 0 && dot(rd, its.sh.n) < 0) lumPdf = E.inv_area * (h.x * h.x) / fabsf(dot(rd, its.sh.n));
                    lumPdf *= E.pdf_discrete;
                }
            }
            const float weight = mis(bv.w * D.fracBSDF, lumPdf * D.fracLum) * D.weightBSDF;   // direct.cpp:302
            L = L + value * xyz(bv) * weight;
        }
    }
    stS(&P.L[slot], make_float4(L.x, L.y, L.z, L4.w));
}

#ifndef MTSG_TU_EXT2
template <int SMP>
void shade_smp(const DirectLaunch &a) {
    const dim3 g((a.B->nslots + BLOCK - 1) / BLOCK), b(BLOCK);
    const bool ext = a.ext && !a.D->ao;   // ao reads no BSDF
#define SHADE(ENV, EXT, MATS) hipLaunchKernelGGL((k_direct_shade<ENV, SMP, EXT, MATS>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D, a.hasAlpha)
    // a point, spot, directional or constant emitter: the kernel that holds
    // every emitter kind (as launch_shade_smp; ao samples no emitter)
    if (a.emx && !a.D->ao) { SHADE(EM_ALL, true, MATS_ALL); return; }
    // the smallest compiled material set that holds the scene's, for the
    // independent sampler (as launch_shade_smp picks k_shade's, smp_kernels.hip)
    if constexpr (SMP == MTSG_SAMPLER_INDEPENDENT) {
        if (!ext && !a.D->ao) {
            switch (mats_kernel_set(a.mats)) {
                case MAT_DIFFUSE:
                    if (a.env) SHADE(true, false, MAT_DIFFUSE); else SHADE(false, false, MAT_DIFFUSE);
                    return;
                case MAT_DIFFUSE | MAT_RC_GGX:
                    if (a.env) SHADE(true, false, MAT_DIFFUSE | MAT_RC_GGX); else SHADE(false, false, MAT_DIFFUSE | MAT_RC_GGX);
                    return;
                case MAT_DIFFUSE | MAT_RC_GGX | MAT_DIELECTRIC:
                    if (a.env) SHADE(true, false, MAT_DIFFUSE | MAT_RC_GGX | MAT_DIELECTRIC);
                    else SHADE(false, false, MAT_DIFFUSE | MAT_RC_GGX | MAT_DIELECTRIC);
                    return;
                default: break;
            }
        }
    }
    if (a.env) { if (ext) SHADE(true, true, MATS_ALL); else SHADE(true, false, MATS_ALL); }
    else { if (ext) SHADE(false, true, MATS_ALL); else SHADE(false, false, MATS_ALL); }
#undef SHADE
}
#endif

}  // namespace

namespace mtsg {

#ifdef MTSG_TU_EXT2
// the kernels of DirectLaunch::ext2 scenes (a BSDF type above roughplastic), in
// a translation unit of their own: every emitter kind and every BSDF
template <int SMP>
static void shade_ext2(const DirectLaunch &a) {
    const dim3 g((a.B->nslots + BLOCK - 1) / BLOCK), b(BLOCK);
    hipLaunchKernelGGL((k_direct_shade<EM_ALL, SMP, 2, MATS_ALL>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D, a.hasAlpha);
}
void launch_direct_shade_ext2(const DirectLaunch &a) {
    switch (a.I->smp.type) {
        case MTSG_SAMPLER_HALTON: shade_ext2<MTSG_SAMPLER_HALTON>(a); break;
        case MTSG_SAMPLER_HAMMERSLEY: shade_ext2<MTSG_SAMPLER_HAMMERSLEY>(a); break;
        case MTSG_SAMPLER_LDSAMPLER: shade_ext2<MTSG_SAMPLER_LDSAMPLER>(a); break;
        case MTSG_SAMPLER_SOBOL: shade_ext2<MTSG_SAMPLER_SOBOL>(a); break;
        default: shade_ext2<MTSG_SAMPLER_INDEPENDENT>(a);
    }
}
void launch_direct_resolve_ext2(const DirectLaunch &a) {
    const dim3 g((a.B->nslots + BLOCK - 1) / BLOCK), b(BLOCK);
    hipLaunchKernelGGL((k_direct_resolve<EM_ALL, true>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D);
}
#else

void launch_direct_shade(const DirectLaunch &a) {
    if (a.ext2 && !a.D->ao) { launch_direct_shade_ext2(a); return; }   // (ao reads no BSDF)
    switch (a.I->smp.type) {
        case MTSG_SAMPLER_HALTON: shade_smp<MTSG_SAMPLER_HALTON>(a); break;
        case MTSG_SAMPLER_HAMMERSLEY: shade_smp<MTSG_SAMPLER_HAMMERSLEY>(a); break;
        case MTSG_SAMPLER_LDSAMPLER: shade_smp<MTSG_SAMPLER_LDSAMPLER>(a); break;
        case MTSG_SAMPLER_SOBOL: shade_smp<MTSG_SAMPLER_SOBOL>(a); break;
        default: shade_smp<MTSG_SAMPLER_INDEPENDENT>(a);
    }
}

void launch_direct_resolve(const DirectLaunch &a) {
    const dim3 g((a.B->nslots + BLOCK - 1) / BLOCK), b(BLOCK);
    if (a.ext2 && !a.D->ao) launch_direct_resolve_ext2(a);
    else if (a.emx) hipLaunchKernelGGL((k_direct_resolve<EM_ALL>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D);
    else if (a.env) hipLaunchKernelGGL((k_direct_resolve<true>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D);
    else hipLaunchKernelGGL((k_direct_resolve<false>), g, b, 0, a.stream, *a.S, *a.I, *a.B, *a.P, *a.D);
}
#endif   // MTSG_TU_EXT2

}  // namespace mtsg
