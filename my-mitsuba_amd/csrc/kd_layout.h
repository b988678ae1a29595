// kd_layout.h -- the device layout of a scene's kd-trees, made on the host from
// Mitsuba's KDNode array (same splits and leaves, re-laid out): sibling pairs
// (host only, the input of the two-level blocks), the blocks, and leaf-ordered
// TriAccel copies.  The top-level tree and every shape group's tree (two-level
// instancing) share both arrays.  No HIP include: tools/check_kd_layout.cpp
// compiles it with g++ and checks it on the CPU; mtsg.hip uploads its arrays
// (KdU4 / KdF4 have the layout of uint4 / float4).
//
// Node words (8 B) are described at DevScene::blocks (kernels.h).
//
// The filtered leaf addressing (`blocksRS`, on request): the flat traversal's
// setup mode tests every rectangle once per ray at its setup, so a rectangle
// record in a leaf is only stepped over there.  blocksRS has the block indices
// and the inner words of `blocks`; a leaf that references a rectangle points
// at a copy of its other records, in their order, appended behind triL's
// existing records (an empty range if nothing is left), every other leaf keeps
// its range.  triL is shared: the kernels that visit primitives in Mitsuba's
// order read `blocks` and never see the appended copies.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <unordered_map>
#include <vector>

#include "../../include/mtsg.h"

namespace mtsg {

struct KdU2 { uint32_t x, y; };
struct KdU4 { uint32_t x, y, z, w; };
struct KdF4 { float x, y, z, w; };
static_assert(sizeof(KdU4) == 16 && sizeof(KdF4) == 16 && sizeof(mtsg_triaccel) == 48, "uploaded as uint4 / float4 / 3 float4");

constexpr uint32_t KD_KINST = 4u;   // leaf-ordered TriAccel copy of an instance primitive: k = 4 (kernels.h KINST)

struct KdLayout {
    std::vector<KdU4> blocks;
    std::vector<KdF4> triL;          // 3 per record
    KdU2 root2{};
    std::vector<KdU2> groupRoots;    // per shape group its tree's root word
    // the filtered addressing: empty unless asked for and some leaf references
    // a rectangle; then triL holds the appended copies behind record triBase
    std::vector<KdU4> blocksRS;
    KdU2 root2RS{};
    size_t triBase = 0;              // records of the unfiltered layout
    size_t leavesFiltered = 0, leavesEmptied = 0;
};

// The layout of `d`.  filter: also the filtered addressing (flat scenes that
// take the setup mode; a scene with shape groups gets none).  Returns nullptr,
// or what is wrong with the tree.
inline const char *kd_layout(const mtsg_scene_desc *d, bool filter, KdLayout &out) {
    auto u2 = [](uint32_t x, uint32_t y) { return KdU2{x, y}; };
    auto u4 = [](uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return KdU4{x, y, z, w}; };
    std::vector<KdU4> pairs;
    std::vector<KdF4> &triL = out.triL;
    triL.clear();
    pairs.reserve(d->n_nodes / 2 + 1);
    triL.reserve((size_t)d->n_indices * 3);
    bool layoutOk = true;
    const mtsg_kdnode *tNodes = d->nodes;
    const uint32_t *tIdx = d->indices;
    uint32_t tNodeCount = d->n_nodes, tIdxCount = d->n_indices;
    filter = filter && d->n_groups == 0 && d->n_instances == 0;
    std::vector<KdU2> rectLeaves;   // leaf words of the leaves that reference a rectangle
    std::function<KdU2(uint32_t, int)> convert = [&](uint32_t ni, int depth) -> KdU2 {
        if (depth > 64 || ni >= tNodeCount) { layoutOk = false; return u2(0x80000000u, 0u); }
        const mtsg_kdnode &N = tNodes[ni];
        if (N.combined & 0x80000000u) {
            const uint32_t start = (uint32_t)(triL.size() / 3);
            bool hasRect = false;
            for (uint32_t e = N.combined & 0x7FFFFFFFu; e < N.data; ++e) {
                const uint32_t p = e < tIdxCount ? tIdx[e] : 0xFFFFFFFFu;
                if (p >= d->n_prims) { layoutOk = false; break; }
                mtsg_triaccel ta = d->triaccel[p];
                if (ta.k == MTSG_TRIACCEL_SHAPE && ta.shape_index < d->n_shapes &&
                    d->shapes[ta.shape_index].type == MTSG_SHAPE_INSTANCE) {
                    if (ta.prim_index >= d->n_instances) { layoutOk = false; break; }
                    ta.k = KD_KINST;
                    // the instance's world box in the record's free words
                    // (n_u n_v n_d = min, a_u a_v b_nu = max): the group box's
                    // corners through to_world in double, widened by 1e-4 of
                    // its size and position and rounded outward, so the
                    // traversal's prefilter (kernels.h inst_box) never drops an
                    // entry the exact group-space clip would take
                    const mtsg_instance &I = d->instances[ta.prim_index];
                    if (I.group >= d->n_groups) { layoutOk = false; break; }
                    const mtsg_group &G = d->groups[I.group];
                    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                    for (int c = 0; c < 8; ++c) {
                        const double q[3] = {(c & 1) ? G.aabb_max[0] : G.aabb_min[0], (c & 2) ? G.aabb_max[1] : G.aabb_min[1],
                                             (c & 4) ? G.aabb_max[2] : G.aabb_min[2]};
                        for (int a = 0; a < 3; ++a) {
                            const float *W = I.to_world + 4 * a;
                            const double w = (double)W[0] * q[0] + (double)W[1] * q[1] + (double)W[2] * q[2] + (double)W[3];
                            lo[a] = std::min(lo[a], w);
                            hi[a] = std::max(hi[a], w);
                        }
                    }
                    double ext = 0, mag = 0;
                    for (int a = 0; a < 3; ++a) {
                        ext = std::max(ext, hi[a] - lo[a]);
                        mag = std::max(mag, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
                    }
                    const double m = 1e-4 * (ext + mag) + 1e-30;
                    float bmin[3], bmax[3];
                    for (int a = 0; a < 3; ++a) {
                        bmin[a] = std::nextafter((float)(lo[a] - m), -INFINITY);
                        bmax[a] = std::nextafter((float)(hi[a] + m), INFINITY);
                    }
                    if (!std::isfinite(bmin[0] + bmin[1] + bmin[2] + bmax[0] + bmax[1] + bmax[2])) {
                        // a degenerate or unbounded transform: a box that takes every ray
                        for (int a = 0; a < 3; ++a) { bmin[a] = -INFINITY; bmax[a] = INFINITY; }
                    }
                    ta.n_u = bmin[0]; ta.n_v = bmin[1]; ta.n_d = bmin[2];
                    ta.a_u = bmax[0]; ta.a_v = bmax[1]; ta.b_nu = bmax[2];
                }
                hasRect |= ta.k == MTSG_TRIACCEL_SHAPE;
                // the TriAccel index (Mitsuba's mailbox key, kernels.h
                // mailbox_step) in place of the shape index
                ta.shape_index = p;
                KdF4 t[3];
                memcpy(t, &ta, sizeof(t));
                triL.push_back(t[0]); triL.push_back(t[1]); triL.push_back(t[2]);
            }
            const KdU2 w = u2(0x80000000u | start, (uint32_t)(triL.size() / 3));
            if (filter && hasRect) rectLeaves.push_back(w);
            return w;
        }
        const uint32_t left = ni + ((N.combined & ~(3u | 0x40000000u)) >> 2);
        const uint32_t pi = (uint32_t)pairs.size();
        pairs.push_back(u4(0, 0, 0, 0));
        const KdU2 L = convert(left, depth + 1);
        const KdU2 R = convert(left + 1, depth + 1);
        pairs[pi] = u4(L.x, L.y, R.x, R.y);
        return u2((N.combined & 3u) | (pi << 2), N.data);
    };
    const KdU2 root = convert(0, 0);
    std::vector<KdU2> &groupRoots = out.groupRoots;
    groupRoots.assign(d->n_groups, u2(0, 0));
    if (d->n_instances && (!d->instances || !d->groups || !d->group_nodes || !d->group_indices)) layoutOk = false;
    for (uint32_t g = 0; g < d->n_groups && layoutOk; ++g) {
        const mtsg_group &G = d->groups[g];
        if ((uint64_t)G.node_offset + G.n_nodes > d->n_group_nodes || (uint64_t)G.index_offset + G.n_indices > d->n_group_indices ||
            G.n_nodes == 0) { layoutOk = false; break; }
        tNodes = d->group_nodes + G.node_offset;
        tIdx = d->group_indices + G.index_offset;
        tNodeCount = G.n_nodes;
        tIdxCount = G.n_indices;
        groupRoots[g] = convert(0, 0);
    }
    for (uint32_t i = 0; i < d->n_instances && layoutOk; ++i)
        if (d->instances[i].group >= d->n_groups) layoutOk = false;
    if (!layoutOk || pairs.size() >= (1u << 29) || triL.size() / 3 >= (1u << 30)) return "malformed or oversized kd-tree";
    // ---- two-level blocks from the binary pair layout
    std::vector<KdU4> &blocks = out.blocks;
    blocks.clear();
    blocks.reserve(pairs.size() * 2 + 8);
    // the scene root's block and the blocks of its (up to four) grandchildren
    // come first, blocks 0-4: the top four levels of the tree in 320 B (the
    // MTSG_LDS_TOP variant stages them in LDS)
    std::unordered_map<uint32_t, uint32_t> preBlock;
    auto reserveBlock = [&](uint32_t pair) {
        preBlock[pair] = (uint32_t)(blocks.size() / 4);
        blocks.resize(blocks.size() + 4, u4(0, 0, 0, 0));
    };
    if (!(root.x & 0x80000000u)) {
        reserveBlock(root.x >> 2);
        const KdU4 pr = pairs[root.x >> 2];
        for (const KdU2 c : {u2(pr.x, pr.y), u2(pr.z, pr.w)}) {
            if (c.x & 0x80000000u) continue;
            const KdU4 gp = pairs[c.x >> 2];
            for (const KdU2 g : {u2(gp.x, gp.y), u2(gp.z, gp.w)})
                if (!(g.x & 0x80000000u)) reserveBlock(g.x >> 2);
        }
    }
    // where conv2 wrote a leaf word: half h (0: x y, 1: z w) of blocks[i] as 2 * i + h
    std::vector<uint64_t> leafSlots;
    auto noteLeaves = [&](size_t slot, KdU2 l, KdU2 r) {
        if (!filter) return;
        if (l.x & 0x80000000u) leafSlots.push_back(2 * (uint64_t)slot);
        if (r.x & 0x80000000u) leafSlots.push_back(2 * (uint64_t)slot + 1);
    };
    std::function<KdU2(KdU2, bool, uint32_t)> conv2 = [&](KdU2 w, bool isRoot, uint32_t slot) -> KdU2 {
        if (w.x & 0x80000000u) return w;                       // leaf: unchanged
        const KdU4 pr = pairs[w.x >> 2];
        const KdU2 L = u2(pr.x, pr.y), R = u2(pr.z, pr.w);
        if (isRoot) {
            uint32_t b;
            const auto pre = preBlock.find(w.x >> 2);
            if (pre != preBlock.end()) {
                b = pre->second;
            } else {
                b = (uint32_t)(blocks.size() / 4);
                blocks.resize(blocks.size() + 4, u4(0, 0, 0, 0));
            }
            const KdU2 nL = conv2(L, false, 4 * b + 1);
            const KdU2 nR = conv2(R, false, 4 * b + 2);
            blocks[4 * b] = u4(nL.x, nL.y, nR.x, nR.y);
            noteLeaves(4 * (size_t)b, nL, nR);
            return u2((w.x & 3u) | (b << 3), w.y);
        }
        // pair-only node: its children are block roots (or leaves)
        const KdU2 nL = conv2(L, true, 0), nR = conv2(R, true, 0);
        blocks[slot] = u4(nL.x, nL.y, nR.x, nR.y);
        noteLeaves(slot, nL, nR);
        return u2((w.x & 3u) | 4u | (slot << 3), w.y);
    };
    out.root2 = conv2(root, true, 0);
    for (auto &gr : groupRoots) gr = conv2(gr, true, 0);
    blocks.resize(blocks.size() + 4, u4(0, 0, 0, 0));   // slack for the 3-slot fetch of the last slot
    if (blocks.size() < 20) blocks.resize(20, u4(0, 0, 0, 0));   // blocks 0-4 are always readable
    if (blocks.size() >= (1u << 29)) return "kd-tree too large for the two-level layout";
    out.triBase = triL.size() / 3;
    // ---- the filtered addressing
    out.blocksRS.clear();
    out.root2RS = out.root2;
    out.leavesFiltered = out.leavesEmptied = 0;
    if (!rectLeaves.empty()) {
        // a leaf that holds a record is the only one with its start
        std::unordered_map<uint32_t, KdU2> moved;
        moved.reserve(rectLeaves.size() * 2);
        for (const KdU2 w : rectLeaves) {
            const uint32_t st = (uint32_t)(triL.size() / 3);
            for (uint32_t e = w.x & 0x7FFFFFFFu; e < w.y; ++e) {
                uint32_t k;
                memcpy(&k, &triL[3 * (size_t)e].x, 4);
                if (k == MTSG_TRIACCEL_SHAPE) continue;
                for (int j = 0; j < 3; ++j) { const KdF4 f = triL[3 * (size_t)e + j]; triL.push_back(f); }
            }
            const uint32_t en = (uint32_t)(triL.size() / 3);
            // nothing left: an empty leaf at the leaf's own start
            moved[w.x] = st < en ? u2(0x80000000u | st, en) : u2(w.x, w.x & 0x7FFFFFFFu);
            ++out.leavesFiltered;
            out.leavesEmptied += st == en;
        }
        // the grown array under the checks of the unfiltered one: record
        // indices below 2^30, so that 3 * index < 2^32 (kernels.h spec_iter)
        if (triL.size() / 3 >= (1u << 30)) return "kd-tree too large for the filtered leaf records";
        auto remap = [&](KdU2 w) {
            if (!(w.x & 0x80000000u) || (w.x & 0x7FFFFFFFu) >= w.y) return w;   // inner or empty
            const auto it = moved.find(w.x);
            return it == moved.end() ? w : it->second;
        };
        out.blocksRS = blocks;
        for (const uint64_t s : leafSlots) {
            KdU4 &b = out.blocksRS[(size_t)(s >> 1)];
            if (s & 1) { const KdU2 n = remap(u2(b.z, b.w)); b.z = n.x; b.w = n.y; }
            else { const KdU2 n = remap(u2(b.x, b.y)); b.x = n.x; b.y = n.y; }
        }
        out.root2RS = remap(out.root2);   // the root itself a leaf: its own root word
    }
    if (triL.empty()) triL.resize(3, KdF4{0, 0, 0, 0});
    return nullptr;
}

}  // namespace mtsg
