// check_multichannel_host: the host side of a multichannel scene, end to end,
// as a stand-alone program that the Makefile builds together with the host
// sources under -fsanitize=address,undefined (CPU only):
//   check_multichannel_host scene.xml out.exr
// loads the XML (multichannel integrator, multi-entry hdrfilm), checks the
// descriptor handed to the device (mtsh_scene_aov) against the scene's own
// tables, develops a synthetic block of 3m + 2 floats per texel -- negative
// values, an infinity and zero-weight texels included -- and writes the EXR.
// Exit status 0 = every check held (and the sanitizers saw nothing).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mtsh.h"

static int fail(const char *what) {
    char buf[1024];
    mtsh_last_error(buf, sizeof(buf));
    fprintf(stderr, "check_multichannel_host: %s (%s)\n", what, buf);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s scene.xml out.exr\n", argv[0]); return 2; }
    mtsh_set_kd_threads(2);
    mtsh_scene *s = mtsh_scene_load(argv[1], nullptr, 0);
    if (!s) return fail("load");
    const mtsg_aov_desc *a = mtsh_scene_aov(s);
    if (!a) return fail("the scene's integrator is not multichannel");
    const mtsg_scene_desc *d = mtsh_scene_desc(s);
    if (a->n_children < 1 || a->n_children > MTSG_MAX_SUBINTEGRATORS || a->n_bsdfs != d->n_bsdfs || a->n_shapes != d->n_shapes)
        return fail("descriptor sizes");
    // every table entry is readable and consistent
    double sum = 0;
    for (uint32_t i = 0; i < a->n_bsdfs; ++i) sum += a->bsdfs[i].factor[0] + a->bsdfs[i].factor[1] + a->bsdfs[i].factor[2] + a->bsdfs[i].textured;
    for (uint32_t i = 0; i < a->n_shapes; ++i) {
        const mtsg_aov_shape &sh = a->shapes[i];
        if (sh.elem_count < 1 || sh.elem_offset + sh.elem_count > a->n_elems) return fail("element range");
        for (uint32_t e = 0; e < sh.elem_count; ++e) sum += a->elem_starts[sh.elem_offset + e];
        if (d->shapes[i].type == MTSG_SHAPE_MESH && a->elem_starts[sh.elem_offset + sh.elem_count - 1] >= d->shapes[i].tri_count)
            return fail("element start beyond the mesh");
    }
    if (!std::isfinite(sum)) return fail("table values");
    int32_t formats[MTSG_MAX_SUBINTEGRATORS];
    const int nf = mtsh_scene_film_formats(s, formats, MTSG_MAX_SUBINTEGRATORS);
    if (nf != (int)a->n_children) return fail("one pixel format per child");
    std::vector<char> names(4096);
    const int nc = mtsh_scene_film_channels(s, names.data(), names.size());
    if (nc <= 0) return fail("channel names");
    if (mtsh_scene_film_channels(s, names.data(), 3) != -2) return fail("short name buffer not refused");
    std::vector<const char *> np;
    for (const char *q = names.data(); (int)np.size() < nc; q += strlen(q) + 1) np.push_back(q);

    mtsg_render_params p;
    mtsh_scene_render_params(s, &p);
    const int w = p.tile_w, h = p.tile_h;
    const size_t ch = 3 * (size_t)nf + 2;
    std::vector<float> block((size_t)w * h * ch);
    for (size_t k = 0; k < (size_t)w * h; ++k) {
        float *t = &block[k * ch];
        for (size_t c = 0; c + 2 < ch; ++c) t[c] = (float)((int)((k * 7 + c * 13) % 41) - 20) * 0.25f;
        t[ch - 1] = (float)(k % 5);             // every fifth texel has weight 0
        t[ch - 2] = t[ch - 1] * 0.5f;
    }
    block[ch + 1] = INFINITY;
    std::vector<float> img((size_t)w * h * nc);
    if (mtsh_develop_multi(block.data(), w, h, formats, nf, img.data()) != nc) return fail("develop");
    for (int c = 0; c < nc; ++c)
        if (img[c] != 0.0f) return fail("a zero-weight texel did not develop to 0");
    if (mtsh_develop_multi(block.data(), w, h, formats, 0, img.data()) != -1) return fail("zero formats not refused");
    if (mtsh_write_exr(argv[2], w, h, nc, np.data(), img.data()) != 0) return fail("write_exr");
    int rw = 0, rh = 0;
    if (mtsh_read_image(argv[2], &rw, &rh, nullptr, 0) != 0 || rw != w || rh != h) return fail("the written file does not read back");
    printf("check_multichannel_host: %d children, %d channels, %dx%d ok\n", nf, nc, w, h);
    mtsh_scene_free(s);
    return 0;
}
