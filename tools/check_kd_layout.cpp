// check_kd_layout: the device kd-tree layout (my-mitsuba_amd/csrc/kd_layout.h)
// and its filtered leaf addressing, on the CPU.  Three inputs:
//   (1) scenes/cbox.xml (6 rectangles): the unfiltered arrays are the bytes
//       the library uploaded before the layout moved into the header (FNV-1a 64
//       digests recorded from that commit, tests/golden/kd_layout_cbox_digests.txt),
//       with and without the filtered addressing asked for;
//   (2) a builder scene of 2 rectangles and 12 triangles under a hand-made,
//       geometrically valid tree (tests/golden/leaf_filter_scene.txt; the GPU
//       test renders the same scene): leaves of rectangle records only, with a
//       rectangle record first, in the middle (two in a row) and last, and a
//       leaf without one;
//   (3) that scene under a one-leaf tree: the kd root is itself a leaf.
// For every layout with a filtered addressing it checks that
//   (a) blocks and blocksRS have the same size and the same inner words,
//   (b) every filtered leaf range equals the original range minus the
//       MTSG_TRIACCEL_SHAPE records, in order, byte for byte,
//   (c) a leaf without a rectangle record keeps its range,
//   (d) every range of either addressing lies inside triL, the original
//       ranges below the first appended record,
//   (e) asking for the filter leaves blocks, root2 and the first triBase
//       records of triL what they are without it.
//   tools/check_kd_layout <repository root>
// `make` builds it with ASan + UBSan; tests/test_kd_layout.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mtsh.h"
#include "../my-mitsuba_amd/csrc/kd_layout.h"

using namespace mtsg;

namespace {

[[noreturn]] void die(const std::string &what) {
    fprintf(stderr, "check_kd_layout: FAILED %s\n", what.c_str());
    exit(1);
}
#define CHECK(name, cond) do { if (!(cond)) die(std::string(name) + ": " #cond); } while (0)

uint64_t fnv(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

struct LeafStats { size_t leaves = 0, filtered = 0, emptied = 0, kept = 0, first = 0, middle = 0, last = 0; };

uint32_t rec_k(const KdLayout &L, size_t e) {
    uint32_t k;
    memcpy(&k, &L.triL[3 * e].x, 4);
    return k;
}

// (b) (c) (d) for one leaf word and its filtered counterpart
void check_leaf(const char *name, const KdLayout &L, KdU2 w, KdU2 f, LeafStats &st) {
    const size_t nrec = L.triL.size() / 3;
    const uint32_t s0 = w.x & 0x7FFFFFFFu, e0 = w.y, s1 = f.x & 0x7FFFFFFFu, e1 = f.y;
    CHECK(name, (f.x & 0x80000000u) != 0);
    CHECK(name, s0 <= e0 && e0 <= L.triBase);
    CHECK(name, s1 <= e1 && e1 <= nrec);
    ++st.leaves;
    std::vector<uint32_t> keep;
    for (uint32_t e = s0; e < e0; ++e)
        if (rec_k(L, e) != MTSG_TRIACCEL_SHAPE) keep.push_back(e);
    if (keep.size() == e0 - s0) {   // (c)
        CHECK(name, w.x == f.x && w.y == f.y);
        ++st.kept;
        return;
    }
    ++st.filtered;
    st.emptied += keep.empty();
    st.first += rec_k(L, s0) == MTSG_TRIACCEL_SHAPE && !keep.empty();
    st.last += rec_k(L, e0 - 1) == MTSG_TRIACCEL_SHAPE && !keep.empty();
    for (uint32_t e = s0 + 1; e + 1 < e0; ++e)
        st.middle += rec_k(L, e) == MTSG_TRIACCEL_SHAPE && rec_k(L, s0) != MTSG_TRIACCEL_SHAPE && rec_k(L, e0 - 1) != MTSG_TRIACCEL_SHAPE;
    CHECK(name, e1 - s1 == keep.size());
    if (keep.empty()) return;
    CHECK(name, s1 >= L.triBase);   // a copy behind the unfiltered records
    for (size_t i = 0; i < keep.size(); ++i) {
        CHECK(name, memcmp(&L.triL[3 * (size_t)keep[i]], &L.triL[3 * ((size_t)s1 + i)], 48) == 0);
        CHECK(name, rec_k(L, s1 + i) != MTSG_TRIACCEL_SHAPE);
    }
}

// walks both addressings from their roots side by side: (a) - (d)
void walk(const char *name, const KdLayout &L, KdU2 a, KdU2 b, LeafStats &st, int depth) {
    CHECK(name, depth < 80);
    if (a.x & 0x80000000u) { check_leaf(name, L, a, b, st); return; }
    CHECK(name, a.x == b.x && a.y == b.y);   // inner words are equal
    const bool pairOnly = (a.x & 4u) != 0;
    const size_t slot = pairOnly ? (a.x >> 3) : (size_t)(a.x >> 3) * 4;
    CHECK(name, slot < L.blocks.size());
    const KdU4 p = L.blocks[slot], q = L.blocksRS[slot];
    walk(name, L, KdU2{p.x, p.y}, KdU2{q.x, q.y}, st, depth + 1);
    walk(name, L, KdU2{p.z, p.w}, KdU2{q.z, q.w}, st, depth + 1);
}

LeafStats check_filtered(const char *name, const mtsg_scene_desc *d, const KdLayout &plain, const KdLayout &L) {
    // (e)
    CHECK(name, plain.blocksRS.empty() && plain.triBase == L.triBase);
    CHECK(name, plain.blocks.size() == L.blocks.size() && memcmp(plain.blocks.data(), L.blocks.data(), 16 * L.blocks.size()) == 0);
    CHECK(name, plain.root2.x == L.root2.x && plain.root2.y == L.root2.y);
    CHECK(name, memcmp(plain.triL.data(), L.triL.data(), 48 * L.triBase) == 0);
    CHECK(name, L.triBase > 0 && plain.triL.size() == 3 * L.triBase);
    // (a): same size, and every word pair that is no leaf in one is the same in the other
    CHECK(name, L.blocksRS.size() == L.blocks.size());
    for (size_t i = 0; i < L.blocks.size(); ++i) {
        const KdU4 p = L.blocks[i], q = L.blocksRS[i];
        CHECK(name, (p.x >> 31) == (q.x >> 31) && (p.z >> 31) == (q.z >> 31));
        if (!(p.x >> 31)) CHECK(name, p.x == q.x && p.y == q.y);
        if (!(p.z >> 31)) CHECK(name, p.z == q.z && p.w == q.w);
    }
    LeafStats st;
    walk(name, L, L.root2, L.root2RS, st, 0);
    CHECK(name, st.filtered == L.leavesFiltered && st.emptied == L.leavesEmptied && st.filtered > 0);
    // the leaves of the description, counted on its own nodes
    size_t leaves = 0;
    for (uint32_t i = 0; i < d->n_nodes; ++i) leaves += d->nodes[i].combined >> 31;
    CHECK(name, st.leaves == leaves);
    printf("%s: %zu blocks words, %zu + %zu records, %zu leaves: %zu filtered (%zu emptied; rectangle first %zu, middle %zu, last %zu), %zu kept\n",
           name, L.blocks.size(), L.triBase, L.triL.size() / 3 - L.triBase, st.leaves, st.filtered, st.emptied, st.first, st.middle,
           st.last, st.kept);
    return st;
}

void layouts(const char *name, const mtsg_scene_desc *d, KdLayout &plain, KdLayout &filt) {
    const char *e = kd_layout(d, false, plain);
    if (e) die(std::string(name) + ": " + e);
    e = kd_layout(d, true, filt);
    if (e) die(std::string(name) + ": " + e);
}

mtsh_prop prop_xf(const char *name, const float (&m)[16]) {
    mtsh_prop p{};
    p.name = name;
    p.type = MTSH_PROP_TRANSFORM;
    memcpy(p.m, m, sizeof(p.m));
    return p;
}
mtsh_prop prop_i(const char *name, int64_t v) { mtsh_prop p{}; p.name = name; p.type = MTSH_PROP_INTEGER; p.i = v; return p; }
mtsh_prop prop_f(const char *name, float v) { mtsh_prop p{}; p.name = name; p.type = MTSH_PROP_FLOAT; p.f = v; return p; }
mtsh_prop prop_rgb(const char *name, float r, float g, float b) {
    mtsh_prop p{};
    p.name = name;
    p.type = MTSH_PROP_SPECTRUM;
    p.v[0] = r; p.v[1] = g; p.v[2] = b;
    return p;
}
mtsh_prop prop_s(const char *name, const char *s) { mtsh_prop p{}; p.name = name; p.type = MTSH_PROP_STRING; p.s = s; return p; }

struct Fixture {
    std::vector<float> pos;
    std::vector<uint32_t> tri, nodes, idx;
    float lo[3], hi[3];
    uint32_t maxDepth = 0;
};

Fixture read_fixture(const std::string &path) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("cannot open " + path);
    Fixture F;
    char key[32];
    unsigned n;
    auto expect = [&](const char *k) { if (fscanf(f, "%31s %u", key, &n) != 2 || strcmp(key, k)) die(path + ": expected " + k); };
    expect("vertices");
    F.pos.resize(3 * (size_t)n);
    for (float &v : F.pos) if (fscanf(f, "%f", &v) != 1) die(path + ": vertices");
    expect("triangles");
    F.tri.resize(3 * (size_t)n);
    for (uint32_t &v : F.tri) if (fscanf(f, "%u", &v) != 1) die(path + ": triangles");
    expect("nodes");
    F.nodes.resize(2 * (size_t)n);
    for (uint32_t &v : F.nodes) if (fscanf(f, "%u", &v) != 1) die(path + ": nodes");
    expect("indices");
    F.idx.resize(n);
    for (uint32_t &v : F.idx) if (fscanf(f, "%u", &v) != 1) die(path + ": indices");
    if (fscanf(f, "%31s %f %f %f %f %f %f", key, F.lo, F.lo + 1, F.lo + 2, F.hi, F.hi + 1, F.hi + 2) != 7 || strcmp(key, "aabb")) die(path + ": aabb");
    if (fscanf(f, "%31s %u", key, &F.maxDepth) != 2 || strcmp(key, "max_depth")) die(path + ": max_depth");
    fclose(f);
    return F;
}

// the builder scene of tests/test_gpu_leaf_filter.py: a floor (y = 0) and a
// wall that is the light (x = 1), twelve small triangles between them
mtsh_scene *builder_scene(const Fixture &F, const std::string &root) {
    mtsh_builder *b = mtsh_scene_begin((root + "/scenes").c_str());
    if (!b) die("mtsh_scene_begin");
    auto ok = [&](int32_t rc, const char *what) {
        if (rc < 0) { char e[512]; mtsh_last_error(e, sizeof(e)); die(std::string(what) + ": " + e); }
        return rc;
    };
    const mtsh_prop ip[] = {prop_i("maxDepth", 4)};
    ok(mtsh_scene_set_integrator(b, "path", ip, 1), "integrator");
    const float cam[16] = {1, 0, 0, 0, 0, 0, -1, 1.9f, 0, 1, 0, 0, 0, 0, 0, 1};   // above, looking down
    const mtsh_prop sp[] = {prop_f("fov", 70.0f), prop_xf("toWorld", cam)};
    ok(mtsh_scene_set_sensor(b, "perspective", sp, 2), "sensor");
    const mtsh_prop fp[] = {prop_i("width", 32), prop_i("height", 32), prop_s("pixelFormat", "rgba")};
    ok(mtsh_scene_set_film(b, "hdrfilm", fp, 3, "gaussian", nullptr, 0), "film");
    const mtsh_prop smp[] = {prop_i("sampleCount", 4)};
    ok(mtsh_scene_set_sampler(b, "independent", smp, 1), "sampler");
    const mtsh_prop gp[] = {prop_rgb("reflectance", 0.6f, 0.6f, 0.6f)};
    const int32_t grey = ok(mtsh_scene_add_bsdf(b, "diffuse", gp, 1, nullptr, 0), "bsdf");
    const mtsh_prop lp[] = {prop_rgb("radiance", 6.0f, 6.0f, 6.0f)};
    const int32_t light = ok(mtsh_scene_add_emitter(b, "area", lp, 1), "emitter");
    const float floorM[16] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1};
    const float wallM[16] = {0, 0, -1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1};
    const mtsh_prop r0[] = {prop_xf("toWorld", floorM)}, r1[] = {prop_xf("toWorld", wallM)};
    ok(mtsh_scene_add_shape(b, "rectangle", r0, 1, grey, -1, -1), "floor");
    ok(mtsh_scene_add_shape(b, "rectangle", r1, 1, grey, light, -1), "wall");
    mtsh_mesh m{};
    m.name = "chips";
    m.n_vertices = (uint32_t)(F.pos.size() / 3);
    m.n_triangles = (uint32_t)(F.tri.size() / 3);
    m.positions = F.pos.data();
    m.indices = F.tri.data();
    m.face_normals = 1;
    ok(mtsh_scene_add_mesh(b, &m, grey, -1, -1), "mesh");
    mtsh_scene *s = mtsh_scene_finish(b, nullptr);
    if (!s) { char e[512]; mtsh_last_error(e, sizeof(e)); die(std::string("mtsh_scene_finish: ") + e); }
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <repository root>\n", argv[0]); return 2; }
    const std::string root = argv[1];
    // ---- (1) the Cornell box
    {
        const char *defs[] = {"width=16", "height=16", "spp=1"};
        mtsh_scene *sc = mtsh_scene_load((root + "/scenes/cbox.xml").c_str(), defs, 3);
        if (!sc) { char e[512]; mtsh_last_error(e, sizeof(e)); die(e); }
        const mtsg_scene_desc *d = mtsh_scene_desc(sc);
        KdLayout plain, filt;
        layouts("cbox", d, plain, filt);
        const std::string gp = root + "/tests/golden/kd_layout_cbox_digests.txt";
        FILE *g = fopen(gp.c_str(), "r");
        if (!g) die("cannot open " + gp);
        unsigned long long nb = 0, hb = 0, nt = 0, ht = 0, rx = 0, ry = 0;
        if (fscanf(g, "blocks %llu %llx triL %llu %llx root2 %llx %llx", &nb, &hb, &nt, &ht, &rx, &ry) != 6) die(gp + ": malformed");
        fclose(g);
        printf("cbox: blocks %zu %016llx triL %zu %016llx root2 %x %x\n", 16 * plain.blocks.size(),
               (unsigned long long)fnv(plain.blocks.data(), 16 * plain.blocks.size()), 16 * plain.triL.size(),
               (unsigned long long)fnv(plain.triL.data(), 16 * plain.triL.size()), plain.root2.x, plain.root2.y);
        CHECK("cbox", 16 * plain.blocks.size() == nb && fnv(plain.blocks.data(), 16 * plain.blocks.size()) == hb);
        CHECK("cbox", 16 * plain.triL.size() == nt && fnv(plain.triL.data(), 16 * plain.triL.size()) == ht);
        CHECK("cbox", plain.root2.x == rx && plain.root2.y == ry);
        CHECK("cbox", d->n_rects == 6);
        check_filtered("cbox", d, plain, filt);
        mtsh_scene_free(sc);
    }
    // ---- (2) the builder scene under its hand-made tree
    const Fixture F = read_fixture(root + "/tests/golden/leaf_filter_scene.txt");
    {
        mtsh_scene *sc = builder_scene(F, root);
        if (mtsh_scene_set_kdtree(sc, (const mtsg_kdnode *)F.nodes.data(), (uint32_t)(F.nodes.size() / 2), F.idx.data(), (uint32_t)F.idx.size(),
                                  F.lo, F.hi, F.maxDepth) != 0) { char e[512]; mtsh_last_error(e, sizeof(e)); die(e); }
        const mtsg_scene_desc *d = mtsh_scene_desc(sc);
        CHECK("builder", d->n_rects == 2 && d->n_triangles == 12 && d->n_nodes == 13);
        KdLayout plain, filt;
        layouts("builder", d, plain, filt);
        const LeafStats st = check_filtered("builder", d, plain, filt);
        CHECK("builder", st.leaves == 7 && st.filtered == 6 && st.emptied == 2 && st.kept == 1);
        CHECK("builder", st.first >= 1 && st.middle >= 1 && st.last >= 1);
        // 20 references, 8 of them rectangles; 4 filtered leaves keep 2 + 2 + 2 + 3 records
        CHECK("builder", filt.triBase == 20 && filt.triL.size() / 3 == 29);
        mtsh_scene_free(sc);
    }
    // ---- (3) ... and under a one-leaf tree: the root word itself is remapped
    {
        mtsh_scene *sc = builder_scene(F, root);
        std::vector<uint32_t> all(14);
        for (uint32_t i = 0; i < 14; ++i) all[i] = (i * 5u) % 14u;   // every primitive once, rectangles (12, 13) inside
        const mtsg_kdnode leaf = {0x80000000u, 14u};
        if (mtsh_scene_set_kdtree(sc, &leaf, 1, all.data(), 14, F.lo, F.hi, 0) != 0) { char e[512]; mtsh_last_error(e, sizeof(e)); die(e); }
        const mtsg_scene_desc *d = mtsh_scene_desc(sc);
        KdLayout plain, filt;
        layouts("root-leaf", d, plain, filt);
        CHECK("root-leaf", (filt.root2.x >> 31) && filt.root2.x == 0x80000000u && filt.root2.y == 14);
        CHECK("root-leaf", filt.root2RS.x == (0x80000000u | 14u) && filt.root2RS.y == 26);
        const LeafStats st = check_filtered("root-leaf", d, plain, filt);
        CHECK("root-leaf", st.leaves == 1 && st.filtered == 1 && st.emptied == 0);
        // rectangles only: the root leaf becomes empty
        const uint32_t rects[2] = {13, 12};
        const mtsg_kdnode leaf2 = {0x80000000u, 2u};
        if (mtsh_scene_set_kdtree(sc, &leaf2, 1, rects, 2, F.lo, F.hi, 0) != 0) { char e[512]; mtsh_last_error(e, sizeof(e)); die(e); }
        d = mtsh_scene_desc(sc);
        KdLayout plain2, filt2;
        layouts("root-leaf of rectangles", d, plain2, filt2);
        CHECK("root-leaf of rectangles", (filt2.root2RS.x >> 31) && (filt2.root2RS.x & 0x7FFFFFFFu) == filt2.root2RS.y);
        check_filtered("root-leaf of rectangles", d, plain2, filt2);
        // no rectangle in the tree: nothing extra is built
        const uint32_t tris[3] = {0, 5, 7};
        const mtsg_kdnode leaf3 = {0x80000000u, 3u};
        if (mtsh_scene_set_kdtree(sc, &leaf3, 1, tris, 3, F.lo, F.hi, 0) != 0) { char e[512]; mtsh_last_error(e, sizeof(e)); die(e); }
        d = mtsh_scene_desc(sc);
        KdLayout plain3, filt3;
        layouts("no rectangle reference", d, plain3, filt3);
        CHECK("no rectangle reference", filt3.blocksRS.empty() && filt3.triL.size() == plain3.triL.size());
        mtsh_scene_free(sc);
    }
    printf("check_kd_layout: ok\n");
    return 0;
}
