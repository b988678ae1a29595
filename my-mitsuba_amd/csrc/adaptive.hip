// adaptive.hip -- the `adaptive` meta-integrator around `path`
// (src/integrators/misc/adaptive.cpp:68-285) on the wavefront.
//
// The reference samples one pixel at a time until its Z-test is satisfied
// (renderBlock, :197-284).  Here a render runs in rounds: round r traces
// samples [s0, s0 + ns) of the tiles that still hold an active pixel with the
// `path` kernels as they are, and two kernels of this unit frame them:
//
//   k_camera_adaptive  k_camera / k_camera_lens with two differences: a pixel
//                      that has stopped gets the dead ray of a slot outside
//                      the rectangle, and the ray differentials are scaled by
//                      1 / sqrt(N) of the base count N, which is no longer the
//                      sample-id stride (that is the cap).  In the pre-pass
//                      (:125-159) the first 2D draw is a position on the full
//                      film and the differentials are left out.
//   k_adaptive_splat   one thread per pixel, as splat_tile: it walks the
//                      pixel's samples of the batch in order, updates Knuth's
//                      (count, mean, meanSqr), finds the first sample at which
//                      the pixel stops and drops the ones after it.  A pixel
//                      that stops scales its K x K x CH window by 1 / count
//                      (:273-283) and adds it to the film through the LDS tile;
//                      one that goes on parks window and statistics in HBM.
//
// The statistics are plain float operations in the reference's order, one
// rounding each (this unit is built without contraction, and says so again at
// the spot), so a float32 restatement on the host reproduces every stop.
#pragma clang diagnostic ignored "-Wunused-function"
#include "kernels.h"

namespace {

// state index of pixel `pix` of the tile with deal key `key`
DEV size_t ad_index(int key, uint32_t pix) { return (size_t)key * (TILE * TILE) + pix; }

template <bool LENS>
__global__ void __launch_bounds__(BLOCK) k_camera_adaptive(DevScene S, DevCamera C, DevIntegrator I, DevBatch B, DevPaths P, DevAdaptive A) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= B.nslots) return;
    int x, y;
    uint32_t s;
    slot_pixel(B, slot, x, y, s);
    bool alive = x < B.rect_x + B.rect_w && y < B.rect_y + B.rect_h;
    if (alive && !A.prepass) {
        const uint32_t tl = (slot >> 8) / B.ns;
        alive = !(A.status[ad_index(batch_key(B, B.tile0 + (int)tl), slot & (TILE * TILE - 1))] & ADAPTIVE_DONE);
    }
    if (!alive) {
        // dead slot, as k_camera's: a negative maxt.  A stopped pixel lies
        // inside the rectangle, so bounce 0 shades it as a miss and may read
        // the differentials: they are the ray's own direction
        if (!C.compact) stS(&P.ray_o[slot], make_float4(0.f, 0.f, 0.f, 0.f));
        stS(&P.ray_d[slot], make_float4(0.f, 0.f, 1.f, -1.0f));
        if (C.diffs) {
            stS(&P.T[slot], make_float4(0.f, 0.f, 1.f, 1.f));
            stS(&P.aux[slot], make_float4(0.f, 0.f, 1.f, 0.f));
        }
        stS(&P.L[slot], make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    // the differentials' scale is 1 / sqrt(N) (adaptive.cpp:183-184,230):
    // camera_differentials and lens_ray take it from the sample count they are given
    DevIntegrator IN = I;
    IN.spp = A.baseCount;
    PathSampler p = path_sampler(I, x, y, s, 0, 0);
    float a, b, u = 0.5f, v = 0.5f;
    next2D<MTSG_SAMPLER_INDEPENDENT>(I, p, a, b);
    if (LENS) next2D<MTSG_SAMPLER_INDEPENDENT>(I, p, u, v);
    int cx = x, cy = y;
    if (A.prepass) {
        // samplePos = nextSample2D() * filmSize (adaptive.cpp:142-144)
        a *= (float)C.film_w;
        b *= (float)C.film_h;
        cx = cy = 0;
    }
    float4 ro, rd;
    float3 rxs, rys;
    if (LENS) {
        if (C.diffs && !A.prepass) lens_ray<true>(C, IN, cx, cy, a, b, u, v, ro, rd, rxs, rys);
        else lens_ray<false>(C, IN, cx, cy, a, b, u, v, ro, rd, rxs, rys);
        if (A.prepass) rxs = rys = xyz(rd);
        stS(&P.ray_o[slot], ro);
        stS(&P.ray_d[slot], rd);
    } else {
        const float3 nearP = camera_near(C, cx, cy, a, b);
        const float3 d = normalize(nearP);
        const float invZ = 1.0f / d.z;
        const float3 wd = camera_to_world_dir(C, d);
        if (C.compact) {
            stS(&P.ray_d[slot], make_float4(wd.x, wd.y, wd.z, invZ));
        } else {
            stS(&P.ray_o[slot], make_float4(C.c2w[3], C.c2w[7], C.c2w[11], C.near_clip * invZ));
            stS(&P.ray_d[slot], make_float4(wd.x, wd.y, wd.z, C.far_clip * invZ));
        }
        if (A.prepass) rxs = rys = wd;
        else if (C.diffs) camera_differentials(C, IN, nearP, wd, rxs, rys);
    }
    if (C.diffs) {   // parked in T and aux until bounce 0 is shaded, as k_camera's
        stS(&P.T[slot], make_float4(rxs.x, rxs.y, rxs.z, 1.f));
        stS(&P.aux[slot], make_float4(rys.x, rys.y, rys.z, 0.f));
    }
}

// One workgroup = one 16x16 tile of the batch, every sample of the batch: a
// pixel's samples depend on each other through its statistics, so they are
// walked by one thread (k_splat cuts them into chunks over blockIdx.y).
template <int K, int CH>
__global__ void __launch_bounds__(BLOCK) k_adaptive_splat(DevCamera C, DevIntegrator I, DevBatch B, DevPaths P, DevAdaptive A, float *film,
                                                          int blockW, int blockH) {
    __shared__ float acc[CH][LT * LT];
    __shared__ float flt[32];
    constexpr int R = K / 2;
    for (int k = threadIdx.x; k < CH * LT * LT; k += BLOCK) (&acc[0][0])[k] = 0.0f;
    if (threadIdx.x < 32) flt[threadIdx.x] = C.filter_values[threadIdx.x];
    __syncthreads();
    const int tl = blockIdx.x;
    const int key = batch_key(B, B.tile0 + tl);
    int tx, ty;
    tile_of_key(key, B.tiles_x, tx, ty, B.skew);
    const int x0 = B.rect_x + tx * TILE, y0 = B.rect_y + ty * TILE;
    const int bord = C.border;
    const int pix = threadIdx.x;
    int lx, ly;
    tile_pix((uint32_t)pix, lx, ly);
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < B.rect_x + B.rect_w && y < B.rect_y + B.rect_h;
    // window and block geometry: splat_tile's (the same Mitsuba block origin,
    // so the weights are bit-identical to the plain film's)
    const int bx0 = (B.rect_x - bord) - (x - R), by0 = (B.rect_y - bord) - (y - R);
    const int mbx = B.rect_x + ((x - B.rect_x) & ~31) - bord, mby = B.rect_y + ((y - B.rect_y) & ~31) - bord;
    const int wxo = (x - R) - mbx, wyo = (y - R) - mby;
    const size_t idx = ad_index(key, (uint32_t)pix);
    const uint32_t st0 = inside ? A.status[idx] : ADAPTIVE_DONE;
    const bool active = !(st0 & ADAPTIVE_DONE);
    uint32_t count = st0 & ~ADAPTIVE_DONE;
    float mean = 0.0f, meanSqr = 0.0f;
    float win[K][K][CH];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c)
#pragma unroll
            for (int h = 0; h < CH; ++h) win[r][c][h] = 0.0f;
    bool stopped = false;
    if (active) {
        if (count) {   // what an earlier batch parked
            mean = A.mean[idx];
            meanSqr = A.meanSqr[idx];
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int h = 0; h < CH; ++h) win[r][c][h] = A.win[(size_t)((r * K + c) * CH + h) * A.stride + idx];
        }
        // the batches of a tile follow each other in sample order: B.s0 == count
        for (uint32_t sl = 0; sl < B.ns && !stopped; ++sl) {
            const uint32_t slot = ((uint32_t)tl * B.ns + sl) * (TILE * TILE) + pix;
            const float4 L = ldS(&P.L[slot]);
            float sampleLuminance = 0.0f;
            // ImageBlock::put rejects invalid samples (imageblock.h:147-151);
            // they count with luminance 0 (adaptive.cpp:235-240)
            if (isfinite(L.x) && isfinite(L.y) && isfinite(L.z) && L.x >= 0 && L.y >= 0 && L.z >= 0) {
                float ja, jb;
                camera_jitter(I, x, y, B.s0 + sl, ja, jb);
                const float px = ((float)x + ja) - 0.5f - (float)mbx;
                const float py = ((float)y + jb) - 0.5f - (float)mby;
                float wx[K], wy[K];
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const bool okx = c >= bx0 && c < bx0 + blockW;
                    const bool oky = c >= by0 && c < by0 + blockH;
                    wx[c] = okx ? flt[min((int)fabsf(((float)(wxo + c) - px) * C.filter_scale), 31)] : 0.0f;
                    wy[c] = oky ? flt[min((int)fabsf(((float)(wyo + c) - py) * C.filter_scale), 31)] : 0.0f;
                }
                const float v[5] = {L.x, L.y, L.z, L.w, 1.0f};
                {
                    // one FMA per term, as splat_tile's window update
#pragma clang fp contract(fast)
#pragma unroll
                    for (int r = 0; r < K; ++r)
#pragma unroll
                        for (int c = 0; c < K; ++c) {
                            const float w = wx[c] * wy[r];
#pragma unroll
                            for (int h = 0; h < CH; ++h) win[r][c][h] += w * v[CH == 4 ? (h == 3 ? 4 : h) : h];
                        }
                }
                {
#pragma clang fp contract(off)
                    // Spectrum::getLuminance of linear RGB (spectrum.h)
                    sampleLuminance = L.x * 0.212671f + L.y * 0.715160f + L.z * 0.072169f;
                }
            }
            ++count;
            {
                // adaptive.cpp:246-270, one rounding per operation
#pragma clang fp contract(off)
                const float delta = sampleLuminance - mean;
                mean += delta / (float)count;
                meanSqr += delta * (sampleLuminance - mean);
                if (count >= A.limit) {
                    stopped = true;
                } else if (count >= A.baseCount) {
                    const float variance = meanSqr / (float)(count - 1);
                    const float stdError = sqrtf(variance / (float)count);
                    const float ciWidth = stdError * A.quantile;
                    const float base = fmaxf(mean, A.avgLum * 0.01f);
                    if (ciWidth <= A.maxError * base) stopped = true;
                }
            }
        }
        if (stopped) {
            A.status[idx] = count | ADAPTIVE_DONE;
            const float factor = 1.0f / (float)count;   // adaptive.cpp:275
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int h = 0; h < CH; ++h) win[r][c][h] *= factor;
        } else {
            A.status[idx] = count;
            A.mean[idx] = mean;
            A.meanSqr[idx] = meanSqr;
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int c = 0; c < K; ++c)
#pragma unroll
                    for (int h = 0; h < CH; ++h) A.win[(size_t)((r * K + c) * CH + h) * A.stride + idx] = win[r][c][h];
        }
    }
    // the tile stays in the next round's list while a pixel of it goes on
    const int more = __syncthreads_or(active && !stopped);
    if (threadIdx.x == 0) A.tileActive[key] = more ? 1u : 0u;
    // the windows of the pixels that stopped, in K*K shifted phases (splat_tile)
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const int o = (ly + r + MAX_BORDER - R) * LT + (lx + c + MAX_BORDER - R);
            if (stopped) {
#pragma unroll
                for (int h = 0; h < CH; ++h) acc[h][o] += win[r][c][h];
            }
            __syncthreads();
        }
    for (int j = threadIdx.x; j < LT * LT * 5; j += BLOCK) {
        const int k = j / 5, h = j - 5 * k;
        const int ty2 = k / LT, tx2 = k % LT;
        const int fx = x0 - MAX_BORDER + tx2 - (B.rect_x - bord), fy = y0 - MAX_BORDER + ty2 - (B.rect_y - bord);
        if (fx < 0 || fy < 0 || fx >= blockW || fy >= blockH) continue;
        const float w = acc[CH - 1][k];
        if (w == 0.0f) continue;
        // no alpha channel (CH == 4): alpha == 1 per sample, so its sum is the weight
        const float val = h < 3 ? acc[h][k] : (h == 3 && CH == 5 ? acc[CH == 5 ? 3 : 0][k] : w);
        unsafeAtomicAdd(film + ((size_t)fy * blockW + fx) * 5 + h, val);
    }
}

}  // namespace

namespace mtsg {

void launch_adaptive_camera(const AdaptiveLaunch &a) {
    const DevBatch &B = *a.B;
    const dim3 g((B.nslots + BLOCK - 1) / BLOCK);
    if (a.C->lens) hipLaunchKernelGGL(k_camera_adaptive<true>, g, dim3(BLOCK), 0, a.stream, *a.S, *a.C, *a.I, B, *a.P, *a.A);
    else hipLaunchKernelGGL(k_camera_adaptive<false>, g, dim3(BLOCK), 0, a.stream, *a.S, *a.C, *a.I, B, *a.P, *a.A);
}

void launch_adaptive_splat(const AdaptiveLaunch &a) {
    const DevBatch &B = *a.B;
    const dim3 g(B.ntiles);
    const int K = 2 * a.C->border + 1;
#define SPLAT(KW, NCH) \
    hipLaunchKernelGGL((k_adaptive_splat<KW, NCH>), g, dim3(BLOCK), 0, a.stream, *a.C, *a.I, B, *a.P, *a.A, a.film, a.blockW, a.blockH)
    if (K == 5 && !a.C->has_alpha) SPLAT(5, 4);
    else if (K == 5) SPLAT(5, 5);
    else if (K <= 3 && !a.C->has_alpha) SPLAT(3, 4);
    else if (K <= 3) SPLAT(3, 5);
    else if (!a.C->has_alpha) SPLAT(9, 4);
    else SPLAT(9, 5);
#undef SPLAT
}

}  // namespace mtsg
