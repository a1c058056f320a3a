// rtg_light_pick.hip — rtg_set_light_sampling (include/rtg.h): power-weighted selection of the light an
// NEE sample goes to. The host weighs the light list (area lights from their device records, the
// environment light from rtg_env.hip's cell weights), mixes in the uniform share, runs Vose's algorithm
// (rtg_env_alias.h, the builder of the environment table) and uploads one 16-byte entry per light;
// k_shade_pick is the shading kernel with light_pick() (rtg_dev.h) at its three pick sites. Built with
// rtg_shade.hip's flags (raytracingrenderer_amd/build.py: DEVICE_FLAGS).
#include "rtg_internal.h"
#include "rtg_env_alias.h"

#include <chrono>
#include <cmath>

// k_shade / k_shade_env (rtg_shade.hip) with the light picked through the alias table: kernels of their
// own name, taking the table as an argument only they have, so SceneView, ChunkArgs and the eight
// k_shade / k_shade_env instantiations stay as they were. ENV as k_shade_env's (et is unused without).
// ALT = false: pathTrace alone, at 7 waves per SIMD; ALT = true: RTG_SHADE_ENV_ALT_WAVES, as their
// k_shade_env counterparts (DESIGN.md §8d has the register table).
template <bool ALT, bool TAB, bool ENVT>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_shade_pick(
    SceneView s, ChunkArgs a, PathBufs p, int b, EnvTable et, LightPick lpk) {
    constexpr bool ENV = ENVT;
    constexpr bool PICK = true;
#include "rtg_shade_body.h"
}
// rtg_probe_light_pick: light_pick on given draws
__global__ void k_probe_light_pick(LightPick lpk, unsigned nl, const unsigned* r0, const float* d1, unsigned n, int* li,
                                   float* pmf) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pm;
    li[i] = light_pick(lpk.table, nl, r0[i], d1[i], pm);
    pmf[i] = pm;
}

// k_shade_pick drawing from the Owen-scrambled Sobol sampler (rtg_set_sampler; rtg_sampler.h), as rtg_shade.hip's
// k_sobol_shade: the waves per SIMD are k_shade_pick's
#define RTG_SHADE_SOBOL
template <bool ALT, bool TAB, bool ENVT>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_sobol_shade_pick(
    SceneView s, ChunkArgs a, PathBufs p, int b, EnvTable et, LightPick lpk) {
    constexpr bool ENV = ENVT;
    constexpr bool PICK = true;
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_SOBOL

int launch_shade_pick(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                      const PathBufs& p, int b) {
    const int sel = (m.alt ? 4 : 0) | (m.tab ? 2 : 0) | (m.env.table ? 1 : 0);
    void (*const kern[8])(SceneView, ChunkArgs, PathBufs, int, EnvTable, LightPick) = {
        k_shade_pick<false, false, false>, k_shade_pick<false, false, true>, k_shade_pick<false, true, false>,
        k_shade_pick<false, true, true>,   k_shade_pick<true, false, false>, k_shade_pick<true, false, true>,
        k_shade_pick<true, true, false>,   k_shade_pick<true, true, true>};
    void (*const kern_sobol[8])(SceneView, ChunkArgs, PathBufs, int, EnvTable, LightPick) = {
        k_sobol_shade_pick<false, false, false>, k_sobol_shade_pick<false, false, true>,
        k_sobol_shade_pick<false, true, false>,  k_sobol_shade_pick<false, true, true>,
        k_sobol_shade_pick<true, false, false>,  k_sobol_shade_pick<true, false, true>,
        k_sobol_shade_pick<true, true, false>,   k_sobol_shade_pick<true, true, true>};
    hipLaunchKernelGGL(m.sobol ? kern_sobol[sel] : kern[sel], dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b, m.env, m.pick);
    LAUNCH_OK("k_shade_pick");
    return RTG_OK;
}

static bool pick_active(const rtg_handle* h) {
    return h->light_sampling.mode == RTG_LIGHTS_POWER && h->mt.light.p != nullptr;
}

static bool finite_d(double x) { return x == x && x <= 1.7976931348623157e308 && x >= -1.7976931348623157e308; }

// pmf, Vose and the entries from n weights (include/rtg.h): false when there is nothing to build from
// (a negative or non-finite weight, or a sum that is 0 or not finite)
static bool build_pick(const double* w, uint32_t n, double lambda, std::vector<double>& pmf, rtg_env::Alias& al,
                       uint32_t* entries) {
    double sum = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(w[i] >= 0.0) || !finite_d(w[i])) return false;
        sum += w[i];
    }
    if (!(sum > 0.0) || !finite_d(sum)) return false;
    pmf.resize(n);
    for (uint32_t i = 0; i < n; ++i) pmf[i] = ((1.0 - lambda) * w[i]) / sum + lambda / (double)n;
    std::vector<double> p(n);
    for (uint32_t i = 0; i < n; ++i) p[i] = pmf[i] * (double)n;
    rtg_env::vose(p, pmf.data(), n, al);  // the environment table's builder, on p_k = pmf_k * n
    for (uint32_t i = 0; i < n; ++i) {
        const float pf = (float)al.prob[i], ps = (float)pmf[i], pa = (float)pmf[al.alias[i]];
        uint32_t* e = entries + 4 * (size_t)i;
        std::memcpy(e + 0, &pf, 4);
        e[1] = al.alias[i];
        std::memcpy(e + 2, &ps, 4);
        std::memcpy(e + 3, &pa, 4);
    }
    return true;
}

static bool share_ok(double s) { return s >= 0.0 && s <= 1.0; }  // (false for NaN)

// The handle's table for uniform_share `share`: weights from the uploaded light records (and the
// environment map's cell weights), Vose on the host, entries uploaded. A fallback of include/rtg.h leaves
// no table (the pick stays uniform).
static int build_light_table(rtg_handle* h, float share) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)h->sv.n_lights;
    std::vector<DevLight> rec(n);
    std::vector<double> wts(n, 0.0), pmf;
    std::vector<uint32_t> entries((size_t)n * 4);
    DevBuf<uint4> d_tab;
    if (int rc = h->scene.lights.download(rec.data(), n)) return rc;
    bool ok = n > 1;
    for (uint32_t i = 0; i < n && ok; ++i) {
        const DevLight& L = rec[i];
        int type;
        std::memcpy(&type, &L.v1t.w, 4);
        if (type == 0) {
            const float l = ((0.2126f * L.em.x) + (0.7152f * L.em.y)) + (0.0722f * L.em.z);  // Colour::Lum
            const float c = (l > 0.0f && l <= RTG_FLT_MAX) ? l : 0.0f;
            wts[i] = (double)c * (double)L.v0a.w;
        } else {
            const float* rb = h->sv.root_box;
            const double dx = (double)rb[3] - (double)rb[0], dy = (double)rb[4] - (double)rb[1],
                         dz = (double)rb[5] - (double)rb[2];
            const double R = 0.5 * std::sqrt((dx * dx + dy * dy) + dz * dz);
            if (!(R > 0.0) || !finite_d(R) || h->sv.env_tex < 0) { ok = false; break; }
            std::vector<double> own;  // (the §8c weights: the environment table's when it was built)
            if (!h->env_built)
                if (int rc = env_cell_weights(h, own)) return rc;
            const std::vector<double>& cw = h->env_built ? h->env_weights : own;
            double S = 0.0;
            for (double x : cw) S += x;
            const double pi = 3.14159265358979323846;
            wts[i] = (2.0 * pi * pi) * R * R * (S / (double)cw.size());
        }
    }
    rtg_env::Alias al;
    if (ok && build_pick(wts.data(), n, (double)share, pmf, al, entries.data()))
        if (int rc = d_tab.upload((const uint4*)entries.data(), n)) return rc;
    h->mt.light = std::move(d_tab);
    h->light_built = true;
    h->light_built_share = share;
    h->light_entries.swap(entries);
    h->light_weights.swap(wts);
    h->light_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RTG_OK;
}

int light_sampling_check(const char* who, const rtg_light_sampling* p) {
    if (!p) { g_err = std::string(who) + ": null argument"; return RTG_ERR_ARG; }
    if (p->mode != RTG_LIGHTS_UNIFORM && p->mode != RTG_LIGHTS_POWER) {
        g_err = std::string(who) + ": unknown mode";
        return RTG_ERR_ARG;
    }
    if (!share_ok((double)p->uniform_share)) {
        g_err = std::string(who) + ": uniform_share outside [0, 1]";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

extern "C" {

int rtg_light_sampling_defaults(rtg_light_sampling* p) {
    if (!p) { g_err = "rtg_light_sampling_defaults: null argument"; return RTG_ERR_ARG; }
    p->mode = RTG_LIGHTS_UNIFORM;
    p->uniform_share = 0.125f;
    return RTG_OK;
}

int rtg_set_light_sampling(rtg_handle* h, const rtg_light_sampling* p) {
    if (!h) { g_err = "rtg_set_light_sampling: null handle"; return RTG_ERR_ARG; }
    if (int rc = light_sampling_check("rtg_set_light_sampling", p)) return rc;
    if (int rc = settle(h)) return rc;
    if (p->mode == RTG_LIGHTS_POWER && (!h->light_built || h->light_built_share != p->uniform_share))
        if (int rc = build_light_table(h, p->uniform_share)) return rc;
    h->light_sampling = *p;
    return light_grid_sync(h);  // rtg_set_light_grid's tables follow the mode and uniform_share
}

int rtg_get_light_sampling(rtg_handle* h, rtg_light_sampling* p) {
    if (!h || !p) { g_err = "rtg_get_light_sampling: null argument"; return RTG_ERR_ARG; }
    *p = h->light_sampling;
    return RTG_OK;
}

int rtg_light_weights(rtg_handle* h, double* weights) {
    if (!h || !weights) { g_err = "rtg_light_weights: null argument"; return RTG_ERR_ARG; }
    if (!pick_active(h)) { g_err = "rtg_light_weights: no table is active"; return RTG_ERR_ARG; }
    std::memcpy(weights, h->light_weights.data(), h->light_weights.size() * sizeof(double));
    return RTG_OK;
}

int rtg_light_table(rtg_handle* h, uint32_t* n, float* entries, double* build_ms) {
    if (!h || !n) { g_err = "rtg_light_table: null argument"; return RTG_ERR_ARG; }
    *n = 0;
    if (build_ms) *build_ms = h->light_build_ms;
    if (!pick_active(h)) return RTG_OK;
    *n = (uint32_t)h->sv.n_lights;
    if (entries) std::memcpy(entries, h->light_entries.data(), h->light_entries.size() * sizeof(uint32_t));
    return RTG_OK;
}

int rtg_light_records(rtg_handle* h, float* out) {
    if (!h || !out) { g_err = "rtg_light_records: null argument"; return RTG_ERR_ARG; }
    static_assert(sizeof(DevLight) == 20 * sizeof(float), "rtg_light_records: 20 floats per light");
    HIPOK(hipSetDevice(h->device));
    return h->scene.lights.download((DevLight*)out, (size_t)h->sv.n_lights);
}

int rtg_probe_light_pick(rtg_handle* h, const uint32_t* r0, const float* d1, uint32_t n, int32_t* li, float* pmf) {
    if (!h || !r0 || !d1 || !li || !pmf) { g_err = "rtg_probe_light_pick: null argument"; return RTG_ERR_ARG; }
    if (!pick_active(h)) { g_err = "rtg_probe_light_pick: no table is active"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 4u) { g_err = "rtg_probe_light_pick: too many cases"; return RTG_ERR_ARG; }
    if (n == 0) return RTG_OK;
    HIPOK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n * 4;  // (every buffer holds n 4-byte values)
    return probe_run({{r0, bytes}, {d1, bytes}}, {{li, bytes}, {pmf, bytes}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_light_pick, dim3((n + 255) / 256), dim3(256), 0, nullptr, LightPick{h->mt.light.p},
                           (unsigned)h->sv.n_lights, (const unsigned*)d[0], (const float*)d[1], (unsigned)n, (int*)d[2],
                           (float*)d[3]);
    });
}

int rtg_light_pick_build(const double* weights, uint32_t n, double uniform_share, double* pmf, double* prob,
                         uint32_t* alias, float* entries) {
    if (!weights || !pmf || !prob || !alias || !entries || n == 0 || n > RTG_ENV_MAX_CELLS || !share_ok(uniform_share)) {
        g_err = "rtg_light_pick_build: bad argument";
        return RTG_ERR_ARG;
    }
    std::vector<double> pm;
    rtg_env::Alias al;
    if (!build_pick(weights, n, uniform_share, pm, al, reinterpret_cast<uint32_t*>(entries))) {
        g_err = "rtg_light_pick_build: a negative or non-finite weight, or the weights sum to 0";
        return RTG_ERR_ARG;
    }
    for (uint32_t i = 0; i < n; ++i) {
        pmf[i] = pm[i];
        prob[i] = al.prob[i];
        alias[i] = al.alias[i];
    }
    return RTG_OK;
}

}  // extern "C"
