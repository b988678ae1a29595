// fields.hip -- the `multichannel` integrator's `field` children
// (src/integrators/misc/multichannel.cpp:87-243, field.cpp:55-187) and the
// splat of its 3m + 2 float ImageBlock.
//
// multichannel intersects the camera ray once and hands the same record to
// every child (multichannel.cpp:205-214); a field is a function of that
// record and draws no random number.  So k_fields runs once per batch, on the
// batch's stream between the bounce-0 trace launch (its tie retrace included:
// the hits are final) and the bounce-0 shading, where the work list is still
// the identity (position == sample slot).  It turns the hit into the
// intersection record with the code the path's shading uses (fill_its,
// tri_uv / rect_uv, texture_eval: kernels.h) and writes each requested field
// as three SoA planes of one float per sample slot.
//
// The film: k_splat's register window cannot hold 3m + 2 channels, so the
// block is splatted in passes that share splat_tile (kernels.h) -- jitter,
// Mitsuba block origin, LDS filter table, shifted-phase LDS reduction: the
// `path` child's spectrum with alpha and weight (k_splat_mc), then one field
// per grid slice (k_splat_field), each adding into its floats of the texel.
// No pass rejects a sample: multichannel's blocks are created with
// warn = false (multichannel.cpp:143-145, imageblock.h:147-151).
#pragma clang diagnostic ignored "-Wunused-function"
#include "kernels.h"

namespace {

// its.primIndex and the Scene::m_shapes position of its.shape (field.cpp:
// 159-172): triangle p of shape `shape` lies in the element e of its mesh
// with the last start <= its local index (mtsg_aov_shape)
DEV void shape_prim_index(const DevScene &S, const DevAov &A, uint32_t p, int shape, float &shapeIdx, float &primIdx) {
    const mtsg_aov_shape sh = A.shapes[shape];
    if (p & 0x80000000u) {   // rectangle: one primitive
        shapeIdx = (float)sh.scene_index;
        primIdx = 0.0f;
        return;
    }
    const uint32_t local = p - S.shapes[shape].tri_begin;
    uint32_t e = 0;
    while (e + 1 < sh.elem_count && A.elems[sh.elem_offset + e + 1] <= local) ++e;
    shapeIdx = sh.scene_index < 0 ? -1.0f : (float)(sh.scene_index + (int)e);
    primIdx = (float)(local - A.elems[sh.elem_offset + e]);
}

__global__ void __launch_bounds__(BLOCK) k_fields(DevScene S, DevBatch B, DevPaths P, DevAov A) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= B.nslots) return;
    if (camera_meta(B, slot).x == 0u) return;   // a slot outside the rectangle: never splatted
    const float4 h = ldS(&P.hit[slot]);
    const bool valid = __float_as_uint(h.w) != 0xFFFFFFFFu;
    // fields only: the colour pass splats alpha and weight from L
    if (A.pathChild < 0) stS(&P.L[slot], make_float4(0.f, 0.f, 0.f, valid ? 1.0f : 0.0f));
    float *out = A.planes + slot;
    if (!valid) {
        for (int f = 0; f < A.nf; ++f)
            for (int c = 0; c < 3; ++c) out[(size_t)(3 * f + c) * A.cap] = A.undef[f][c];
        return;
    }
    // the camera ray as the traversal and the shading read it (load_path)
    float4 ro4, rd4;
    load_closest_ray(S, P, slot, S.camCompact != 0, ro4, rd4);
    const float3 ro = xyz(ro4), rd = xyz(rd4);
    const uint32_t inst = S.inst ? P.hitInst[slot] : 0xFFFFFFFFu;
    Its its;
    fill_its(S, ro, rd, h, inst, its);
    const uint32_t p = __float_as_uint(h.w);
    for (int f = 0; f < A.nf; ++f) {
        float3 v = mk3(0.f, 0.f, 0.f);
        switch (A.kind[f]) {
            case MTSG_FIELD_POSITION: v = its.p; break;
            case MTSG_FIELD_REL_POSITION: {
                // Transform::operator()(Point) (transform.h:131-146)
#pragma clang fp contract(off)
                const float *m = A.w2c;
                const float x = m[0] * its.p.x + m[1] * its.p.y + m[2] * its.p.z + m[3];
                const float y = m[4] * its.p.x + m[5] * its.p.y + m[6] * its.p.z + m[7];
                const float z = m[8] * its.p.x + m[9] * its.p.y + m[10] * its.p.z + m[11];
                const float w = m[12] * its.p.x + m[13] * its.p.y + m[14] * its.p.z + m[15];
                v = w == 1.0f ? mk3(x, y, z) : mk3(x, y, z) / w;
                break;
            }
            case MTSG_FIELD_DISTANCE: v = mk3(h.x, h.x, h.x); break;
            case MTSG_FIELD_GEO_NORMAL: v = its.geoN; break;
            case MTSG_FIELD_SH_NORMAL: v = its.sh.n; break;
            case MTSG_FIELD_UV: {
                float2 uv;
                if (p & 0x80000000u) {
                    uv = rect_uv(h);
                } else {
                    const float4 *t = S.ttex + 3 * (size_t)p;
                    uv = tri_uv(t[0], t[1], h);
                }
                v = mk3(uv.x, uv.y, 0.f);
                break;
            }
            case MTSG_FIELD_ALBEDO: {
                // twosided picks the side by its.wi.z > 0 (twosided.cpp:198-203)
                const float3 wi = its.sh.toLocal(-rd);
                const mtsg_bsdf &b = S.bsdfs[its.bsdf];
                const int eff = (b.twosided && !(wi.z > 0)) ? b.back : its.bsdf;
                const mtsg_aov_bsdf ab = A.bsdfs[eff];
                v = ld3(ab.factor);
                if (ab.textured)
                    v = texture_eval(S, S.bsdfs[eff].texture - 1, h, inst, its, ro, false, mk3(0, 0, 0), mk3(0, 0, 0)) * v;
                break;
            }
            case MTSG_FIELD_SHAPE_INDEX:
            case MTSG_FIELD_PRIM_INDEX: {
                float si, pi;
                shape_prim_index(S, A, p, its.shape, si, pi);
                const float x = A.kind[f] == MTSG_FIELD_SHAPE_INDEX ? si : pi;
                v = mk3(x, x, x);
                break;
            }
        }
        out[(size_t)(3 * f) * A.cap] = v.x;
        out[(size_t)(3 * f + 1) * A.cap] = v.y;
        out[(size_t)(3 * f + 2) * A.cap] = v.z;
    }
}

// the `path` child's spectrum (coff >= 0) with alpha and weight: P.L
template <int K>
__global__ void __launch_bounds__(BLOCK) k_splat_mc(DevCamera C, DevIntegrator I, DevBatch B, DevPaths P, float *film, int blockW,
                                                    int blockH, int winSz, int stride, int coff) {
    splat_tile<K, 5, false, true>(C, I, B, P, film, blockW, blockH, winSz, SplatMulti{nullptr, 0, stride, coff});
}
// field child blockIdx.z: its three planes into the texel's floats 3 * child ..
template <int K>
__global__ void __launch_bounds__(BLOCK) k_splat_field(DevCamera C, DevIntegrator I, DevBatch B, DevPaths P, DevAov A, float *film,
                                                       int blockW, int blockH, int winSz) {
    const int f = blockIdx.z;
    splat_tile<K, 3, false, true>(C, I, B, P, film, blockW, blockH, winSz,
                                  SplatMulti{A.planes + (size_t)(3 * f) * A.cap, A.cap, 3 * A.m + 2, 3 * A.child[f]});
}

template <int K>
void splat_multi(const FieldsLaunch &a) {
    const DevBatch &B = *a.B;
    const DevAov &A = *a.A;
    const unsigned chunks = (B.ns + SPLAT_CHUNK - 1) / SPLAT_CHUNK;
    hipLaunchKernelGGL((k_splat_mc<K>), dim3(B.ntiles, chunks), dim3(BLOCK), 0, a.stream, *a.C, *a.I, B, *a.P, a.film, a.blockW,
                       a.blockH, a.win, 3 * A.m + 2, A.pathChild < 0 ? -1 : 3 * A.pathChild);
    if (A.nf)
        hipLaunchKernelGGL((k_splat_field<K>), dim3(B.ntiles, chunks, A.nf), dim3(BLOCK), 0, a.stream, *a.C, *a.I, B, *a.P, A, a.film,
                           a.blockW, a.blockH, a.win);
}

}  // namespace

namespace mtsg {

void launch_fields(const FieldsLaunch &a) {
    const DevBatch &B = *a.B;
    hipLaunchKernelGGL(k_fields, dim3((B.nslots + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, a.stream, *a.S, B, *a.P, *a.A);
}

void launch_splat_multi(const FieldsLaunch &a) {
    const int K = 2 * a.C->border + 1;
    if (K == 5) splat_multi<5>(a);
    else if (K <= 3) splat_multi<3>(a);
    else splat_multi<9>(a);
}

}  // namespace mtsg
