// scene_digest — TEST INFRASTRUCTURE ONLY (tests/test_scene_digest.py). The device records that
// librtg's prepare_scene (rtg_scene.hip) builds from a loaded scene, as one FNV-1a digest per
// HostScene array plus the scalars, one "name value" pair per line. No GPU call. Built by build.py
// build_scene_digest; run: scene_digest <scene dir> | scene_digest synth <n triangles> <seed> <dir>
#include "../../include/rth.h"
#include "../../raytracingrenderer_amd/csrc/device/rtg_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T>
static void digest(const char* name, const std::vector<T>& v) {
    unsigned long long h = 1469598103934665603ull;  // FNV-1a, 64 bits, over the array's bytes
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    std::printf("%s %016llx\nn_%s %zu\n", name, h, name, v.size());
}
static void bits(const char* name, const float* f, int n) {
    std::printf("%s", name);
    for (int k = 0; k < n; ++k) {
        unsigned u;
        std::memcpy(&u, f + k, 4);
        std::printf("%c%08x", k ? ',' : ' ', u);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 && !(argc == 5 && !std::strcmp(argv[1], "synth"))) {
        std::fprintf(stderr, "usage: scene_digest <scene dir> | scene_digest synth <n triangles> <seed> <dir>\n");
        return 2;
    }
    const char* dir = argv[argc - 1];
    if (argc == 5 && rth_write_synthetic(dir, (uint32_t)std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), 1024, 1024)) {
        std::printf("synthetic scene failed: %s\n", rth_last_error());
        return 2;
    }
    rth_load_options o{};
    o.skip_missing = 1;
    rth_scene* s = nullptr;
    if (rth_load_scene(dir, &o, &s)) { std::printf("load failed: %s\n", rth_last_error()); return 2; }
    HostScene hs;
    if (int rc = prepare_scene(rth_scene_desc(s), hs)) { std::printf("prepare_scene failed: %d %s\n", rc, g_err.c_str()); return 1; }
    digest("nodes", hs.nodes);
    digest("nodesq", hs.nodesq);
    digest("leafbox", hs.leafbox);
    digest("img", hs.img);
    digest("tris48", hs.tris48);
    digest("shade", hs.shade);
    digest("mats", hs.mats);
    digest("lights", hs.lights);
    digest("texinfo", hs.texinfo);
    digest("texels", hs.texels);
    std::printf("root_word %d\nroot_wordw %d\nusew %d\nrebuilt %d\nbvh_depth %u\nwide_depth %u\nimg_tri %d\n", hs.root_word,
                hs.root_wordw, (int)hs.usew, (int)hs.rebuilt, hs.bvh_depth, hs.wide_depth, hs.img_tri);
    std::printf("light_count %d\nenv_tex %d\nenv_off %d\nenv_w %d\nenv_h %d\nenv_uniform %d\n", hs.n_lights, hs.env_tex,
                hs.env_off, hs.env_w, hs.env_h, (int)hs.env_uniform);
    bits("env_one", hs.env_one, 3);
    bits("cull_scale", &hs.cull_scale, 1);
    bits("root_box", hs.root_box, 6);
    rth_free_scene(s);
    return 0;
}
