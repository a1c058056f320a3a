// rtg_light_grid.hip — rtg_set_light_grid (include/rtg.h): RTG_LIGHTS_POWER's pick made to depend on the
// shading point. The host lays a grid over the reference root box, weighs every light for every cell
// (§8d's weight over the squared distance between the cell and the light, 0 where the light faces away),
// runs §8d's pmf and Vose per cell and uploads cells * n_lights 16-byte entries; k_shade_grid is
// k_shade_pick with the table's base address taken from the cell of the hit point (light_grid_cell,
// rtg_dev.h) at its two pick sites. Built with rtg_shade.hip's flags (raytracingrenderer_amd/build.py).
#include "rtg_internal.h"
#include "rtg_env_alias.h"

#include <chrono>
#include <cmath>

// k_shade_pick (rtg_light_pick.hip) with one table per grid cell: kernels of their own name, taking the
// grid as an argument only they have: a pointer to its LightGrid record in device memory. The tables are read
// from global memory (cells * n_lights entries do not fit LDS); with TAB the material and light records stay
// in LDS. Launch bounds as k_shade_pick's.
#define RTG_SHADE_GRID 1
template <bool ALT, bool TAB, bool ENVT>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_shade_grid(
    SceneView s, ChunkArgs a, PathBufs p, int b, EnvTable et, const LightGrid* lgp) {
    // The record is read at the pick sites through the constant address space: uniform scalar loads that
    // depend on no lane's data, issued ahead of the draws. Passed by value its eleven words are kernel
    // arguments, live from the kernel's first instruction, and cost k_shade_grid<false, true, true> five
    // spilled SGPRs; read here the path tracer's four instantiations spill none.
    const __attribute__((address_space(4))) LightGrid& lgr = *(const __attribute__((address_space(4))) LightGrid*)lgp;
    constexpr bool ENV = ENVT;
    constexpr bool PICK = true;
    const LightPick lpk{nullptr};  // (unused: both pick sites read lgr)
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_GRID

// rtg_probe_light_grid: light_grid_cell and light_pick on given points and draws
__global__ void k_probe_light_grid(const LightGrid* lgp, unsigned nl, const float* pts, const unsigned* r0, const float* d1,
                                   unsigned n, int* cell, int* li, float* pmf) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const __attribute__((address_space(4))) LightGrid& lgr = *(const __attribute__((address_space(4))) LightGrid*)lgp;
    const uint32_t c = light_grid_cell(lgr, mk(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]));
    float pm;
    cell[i] = (int)c;
    li[i] = light_pick(lgr.table + c * nl, nl, r0[i], d1[i], pm);
    pmf[i] = pm;
}

int launch_shade_grid(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                      const PathBufs& p, int b) {
    const int sel = (m.alt ? 4 : 0) | (m.tab ? 2 : 0) | (m.env.table ? 1 : 0);
    void (*const kern[8])(SceneView, ChunkArgs, PathBufs, int, EnvTable, const LightGrid*) = {
        k_shade_grid<false, false, false>, k_shade_grid<false, false, true>, k_shade_grid<false, true, false>,
        k_shade_grid<false, true, true>,   k_shade_grid<true, false, false>, k_shade_grid<true, false, true>,
        k_shade_grid<true, true, false>,   k_shade_grid<true, true, true>};
    hipLaunchKernelGGL(kern[sel], dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b, m.env, m.grid);
    LAUNCH_OK("k_shade_grid");
    return RTG_OK;
}

#define RTG_GRID_MAX_CELLS 64u
#define RTG_GRID_MAX_ENTRIES (1ull << 24)

static bool finite_d(double x) { return x == x && x <= 1.7976931348623157e308 && x >= -1.7976931348623157e308; }

// the grid of include/rtg.h over root box rb: dims, and the kernel's float32 constants
static void grid_layout(const float* rb, uint32_t cells, uint32_t* dims, float* lo, float* scale) {
    double e[3], emax = 0.0;
    for (int a = 0; a < 3; ++a) {
        e[a] = (double)rb[3 + a] - (double)rb[a];
        if (e[a] > emax) emax = e[a];
    }
    for (int a = 0; a < 3; ++a) {
        const bool flat = !(e[a] > 0.0) || !(emax > 0.0) || !finite_d(emax);
        double d = flat ? 1.0 : std::ceil((double)cells * (e[a] / emax));
        if (!(d >= 1.0)) d = 1.0;
        if (d > (double)cells) d = (double)cells;
        dims[a] = (uint32_t)d;
        lo[a] = rb[a];
        scale[a] = flat ? 0.0f : (float)dims[a] / (rb[3 + a] - rb[a]);
    }
}

// every cell's table (include/rtg.h): entries[(c * n + k) * 4 ..]
static void grid_tables(const float* rec, uint32_t n, const double* w, const float* rb, const uint32_t* dims,
                        double lambda, uint32_t* entries) {
    double lo[3], e[3], s[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)rb[a];
        e[a] = (double)rb[3 + a] - (double)rb[a];
        s[a] = e[a] / (double)dims[a];
    }
    const double r2 = 0.25 * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const double R = 0.5 * std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    // per light: the triangle's box, v0 and gn in binary64
    std::vector<double> tlo((size_t)n * 3), thi((size_t)n * 3);
    std::vector<int> kind(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float* L = rec + (size_t)i * 20;
        std::memcpy(&kind[i], L + 7, 4);
        for (int a = 0; a < 3; ++a) {
            const double v0 = (double)L[a], v1 = (double)L[4 + a], v2 = (double)L[8 + a];
            tlo[(size_t)i * 3 + a] = std::min(std::min(v0, v1), v2);
            thi[(size_t)i * 3 + a] = std::max(std::max(v0, v1), v2);
        }
    }
    const float unif = (float)(1.0 / (double)n);
    std::vector<double> wc(n), pmf(n), p(n);
    rtg_env::Alias al;
    size_t c = 0;
    for (uint32_t iz = 0; iz < dims[2]; ++iz)
        for (uint32_t iy = 0; iy < dims[1]; ++iy)
            for (uint32_t ix = 0; ix < dims[0]; ++ix, ++c) {
                const uint32_t ii[3] = {ix, iy, iz};
                double clo[3], chi[3];
                for (int a = 0; a < 3; ++a) {
                    clo[a] = lo[a] + (double)ii[a] * s[a];
                    chi[a] = lo[a] + (double)(ii[a] + 1u) * s[a];
                }
                double sum = 0.0;
                for (uint32_t i = 0; i < n; ++i) {
                    double g;
                    if (kind[i] == 0) {
                        const float* L = rec + (size_t)i * 20;
                        double d[3];
                        for (int a = 0; a < 3; ++a)
                            d[a] = std::max(std::max(0.0, tlo[(size_t)i * 3 + a] - chi[a]), clo[a] - thi[(size_t)i * 3 + a]);
                        const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                        g = 1.0 / std::max(d2, r2);
                        bool faces = false;
                        for (int k = 0; k < 8; ++k) {
                            const double kx = (k & 1) ? chi[0] + s[0] / 2.0 : clo[0] - s[0] / 2.0;
                            const double ky = (k & 2) ? chi[1] + s[1] / 2.0 : clo[1] - s[1] / 2.0;
                            const double kz = (k & 4) ? chi[2] + s[2] / 2.0 : clo[2] - s[2] / 2.0;
                            const double dt = ((kx - (double)L[0]) * (double)L[12] + (ky - (double)L[1]) * (double)L[13]) +
                                              (kz - (double)L[2]) * (double)L[14];
                            if (dt > 0.0) faces = true;
                        }
                        if (!faces) g = 0.0;
                    } else {
                        g = 1.0 / (R * R);
                    }
                    wc[i] = w[i] * g;
                    sum += wc[i];
                }
                uint32_t* ent = entries + c * (size_t)n * 4;
                if (!(sum > 0.0) || !finite_d(sum)) {  // nothing to weigh by: the uniform table
                    const float one = 1.0f;
                    for (uint32_t i = 0; i < n; ++i) {
                        std::memcpy(ent + 4 * (size_t)i, &one, 4);
                        ent[4 * (size_t)i + 1] = i;
                        std::memcpy(ent + 4 * (size_t)i + 2, &unif, 4);
                        std::memcpy(ent + 4 * (size_t)i + 3, &unif, 4);
                    }
                    continue;
                }
                for (uint32_t i = 0; i < n; ++i) {
                    pmf[i] = ((1.0 - lambda) * wc[i]) / sum + lambda / (double)n;
                    p[i] = pmf[i] * (double)n;
                }
                rtg_env::vose(p, pmf.data(), n, al);
                for (uint32_t i = 0; i < n; ++i) {
                    const float pf = (float)al.prob[i], ps = (float)pmf[i], pa = (float)pmf[al.alias[i]];
                    std::memcpy(ent + 4 * (size_t)i, &pf, 4);
                    ent[4 * (size_t)i + 1] = al.alias[i];
                    std::memcpy(ent + 4 * (size_t)i + 2, &ps, 4);
                    std::memcpy(ent + 4 * (size_t)i + 3, &pa, 4);
                }
            }
}

// the entries a grid of `cells` over root box rb takes for n lights (rb null: the thinnest grid any box
// gives, cells x 1 x 1, the bound that needs no scene)
static unsigned long long grid_entries_for(const float* rb, uint32_t cells, uint32_t n) {
    uint32_t dims[3] = {cells, 1u, 1u};
    float lo[3], scale[3];
    if (rb) grid_layout(rb, cells, dims, lo, scale);
    return (unsigned long long)dims[0] * dims[1] * dims[2] * std::max<uint32_t>(n, 1u);
}

// include/rtg.h's ranges: cells <= 64, and at most 2^24 entries for the box rb (null: see above)
static int grid_check(const char* who, const rtg_light_grid* p, uint32_t n_lights, const float* rb) {
    if (!p) { g_err = std::string(who) + ": null argument"; return RTG_ERR_ARG; }
    if (p->cells == 0) return RTG_OK;
    if (p->cells <= RTG_GRID_MAX_CELLS && grid_entries_for(rb, p->cells, n_lights) <= RTG_GRID_MAX_ENTRIES) return RTG_OK;
    uint32_t most = std::min<uint32_t>(p->cells, RTG_GRID_MAX_CELLS);
    while (most > 0 && grid_entries_for(rb, most, n_lights) > RTG_GRID_MAX_ENTRIES) --most;
    g_err = std::string(who) + ": cells " + std::to_string(p->cells) + " is too many for " + std::to_string(n_lights) +
            " lights (at most 64, and cells * n_lights at most 2^24 entries): the largest admissible cells is " +
            std::to_string(most);
    return RTG_ERR_ARG;
}

int light_grid_check(const char* who, const rtg_handle* h, const rtg_light_grid* p) {
    return grid_check(who, p, (uint32_t)h->sv.n_lights, h->sv.root_box);
}

static bool grid_active(const rtg_handle* h) {
    return h->light_grid.cells != 0 && h->light_sampling.mode == RTG_LIGHTS_POWER && h->mt.light.p != nullptr &&
           h->mt.grid.p != nullptr && h->mt.grid_rec.p != nullptr;
}

static void drop_grid(rtg_handle* h) {
    h->mt.grid.reset();
    h->mt.grid_rec.reset();
    h->grid_built = false;
}

static int build_grid(rtg_handle* h, uint32_t cells, float share) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)h->sv.n_lights;
    std::vector<DevLight> rec(n);
    if (int rc = h->scene.lights.download(rec.data(), n)) return rc;
    LightGrid lg{};
    grid_layout(h->sv.root_box, cells, lg.dims, lg.lo, lg.scale);
    const size_t nc = (size_t)lg.dims[0] * lg.dims[1] * lg.dims[2];
    std::vector<uint32_t> entries(nc * n * 4);
    grid_tables((const float*)rec.data(), n, h->light_weights.data(), h->sv.root_box, lg.dims, (double)share, entries.data());
    DevBuf<uint4> d_tab;
    DevBuf<LightGrid> d_rec;
    if (int rc = d_tab.upload((const uint4*)entries.data(), nc * n)) return rc;
    lg.table = d_tab.p;
    if (int rc = d_rec.upload(&lg, 1)) return rc;
    h->mt.grid = std::move(d_tab);
    h->mt.grid_rec = std::move(d_rec);
    h->grid_built = true;
    h->grid_built_cells = cells;
    h->grid_built_share = share;
    for (int a = 0; a < 3; ++a) {
        h->grid_dims[a] = lg.dims[a];
        h->grid_lo[a] = lg.lo[a];
        h->grid_scale[a] = lg.scale[a];
    }
    h->grid_entries.swap(entries);
    h->grid_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RTG_OK;
}

// A build that fails leaves no grid at all: the tables it would have replaced belong to another cells or
// uniform_share than the handle's settings now say, and frames then run the power pick.
int light_grid_sync(rtg_handle* h) {
    const uint32_t cells = h->light_grid.cells;
    if (cells == 0 || h->light_sampling.mode != RTG_LIGHTS_POWER) return RTG_OK;  // (what is built is kept)
    if (!h->mt.light.p) {  // a fallback of the power mode leaves no grid either
        drop_grid(h);
        return RTG_OK;
    }
    const float share = h->light_sampling.uniform_share;
    if (h->grid_built && h->grid_built_cells == cells && h->grid_built_share == share) return RTG_OK;
    const int rc = build_grid(h, cells, share);
    if (rc) drop_grid(h);
    return rc;
}

extern "C" {

int rtg_light_grid_defaults(rtg_light_grid* p) {
    if (!p) { g_err = "rtg_light_grid_defaults: null argument"; return RTG_ERR_ARG; }
    p->cells = 0;
    return RTG_OK;
}

int rtg_light_grid_check(const rtg_light_grid* p, uint32_t n_lights) {
    return grid_check("rtg_light_grid_check", p, n_lights, nullptr);
}

int rtg_set_light_grid(rtg_handle* h, const rtg_light_grid* p) {
    if (!h) { g_err = "rtg_set_light_grid: null handle"; return RTG_ERR_ARG; }
    if (int rc = light_grid_check("rtg_set_light_grid", h, p)) return rc;
    if (int rc = settle(h)) return rc;
    const rtg_light_grid prev = h->light_grid;
    h->light_grid = *p;
    if (int rc = light_grid_sync(h)) {
        h->light_grid = prev;
        return rc;
    }
    return RTG_OK;
}

int rtg_get_light_grid(rtg_handle* h, rtg_light_grid* p) {
    if (!h || !p) { g_err = "rtg_get_light_grid: null argument"; return RTG_ERR_ARG; }
    *p = h->light_grid;
    return RTG_OK;
}

int rtg_light_grid_info(rtg_handle* h, uint32_t* dims, float* lo, float* scale, uint64_t* n_entries, double* build_ms) {
    if (!h) { g_err = "rtg_light_grid_info: null handle"; return RTG_ERR_ARG; }
    const bool on = grid_active(h);
    for (int a = 0; a < 3; ++a) {
        if (dims) dims[a] = on ? h->grid_dims[a] : 0u;
        if (lo) lo[a] = on ? h->grid_lo[a] : 0.0f;
        if (scale) scale[a] = on ? h->grid_scale[a] : 0.0f;
    }
    if (n_entries) *n_entries = on ? (uint64_t)(h->grid_entries.size() / 4) : 0u;
    if (build_ms) *build_ms = h->grid_build_ms;
    return RTG_OK;
}

int rtg_light_grid_table(rtg_handle* h, float* entries) {
    if (!h || !entries) { g_err = "rtg_light_grid_table: null argument"; return RTG_ERR_ARG; }
    if (!grid_active(h)) { g_err = "rtg_light_grid_table: no grid is active"; return RTG_ERR_ARG; }
    std::memcpy(entries, h->grid_entries.data(), h->grid_entries.size() * sizeof(uint32_t));
    return RTG_OK;
}

int rtg_probe_light_grid(rtg_handle* h, const float* points, const uint32_t* r0, const float* d1, uint32_t n,
                         int32_t* cell, int32_t* li, float* pmf) {
    if (!h || !points || !r0 || !d1 || !cell || !li || !pmf) {
        g_err = "rtg_probe_light_grid: null argument";
        return RTG_ERR_ARG;
    }
    if (!grid_active(h)) { g_err = "rtg_probe_light_grid: no grid is active"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 12u) { g_err = "rtg_probe_light_grid: too many cases"; return RTG_ERR_ARG; }
    if (n == 0) return RTG_OK;
    HIPOK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n * 4;
    return probe_run({{points, 3 * bytes}, {r0, bytes}, {d1, bytes}}, {{cell, bytes}, {li, bytes}, {pmf, bytes}},
                     [&](void* const* d) {
                         hipLaunchKernelGGL(k_probe_light_grid, dim3((n + 255) / 256), dim3(256), 0, nullptr, h->mt.grid_rec.p,
                                            (unsigned)h->sv.n_lights, (const float*)d[0], (const unsigned*)d[1],
                                            (const float*)d[2], (unsigned)n, (int*)d[3], (int*)d[4], (float*)d[5]);
                     });
}

int rtg_light_grid_build(const float* light_records, uint32_t n, const double* weights, const float* root_box,
                         uint32_t cells, double uniform_share, uint32_t* dims, float* lo, float* scale,
                         float* entries) {
    if (!light_records || !weights || !root_box || !dims || !lo || !scale || n == 0 || cells == 0 ||
        cells > RTG_GRID_MAX_CELLS || !(uniform_share >= 0.0 && uniform_share <= 1.0)) {
        g_err = "rtg_light_grid_build: bad argument";
        return RTG_ERR_ARG;
    }
    grid_layout(root_box, cells, dims, lo, scale);
    if (grid_entries_for(root_box, cells, n) > RTG_GRID_MAX_ENTRIES) {
        g_err = "rtg_light_grid_build: more than 2^24 entries";
        return RTG_ERR_ARG;
    }
    if (entries) grid_tables(light_records, n, weights, root_box, dims, uniform_share, reinterpret_cast<uint32_t*>(entries));
    return RTG_OK;
}

}  // extern "C"
