// rtg_env.hip — rtg_set_env_sampling (include/rtg.h): the alias table RTG_ENV_LUMINANCE samples the
// environment light from. k_env_weights takes each cell's footprint maximum of Colour::Lum from the
// texels already on the device; the host weighs it with the row's sin theta, runs Vose's algorithm
// (rtg_env_alias.h, plain C++) and uploads the 16-byte entries k_shade_env loads (rtg_shade.hip;
// env_sample_luminance in rtg_dev.h is the sampling function itself).
#include "rtg_internal.h"
#include "rtg_env_alias.h"

#include <chrono>
#include <cmath>

// One thread per cell, consecutive threads along x: the maximum of lum over the four texels
// Texture::sample blends in the cell, (cx, cy), (cx + 1 mod w, cy), (cx, cy + 1 mod h) and
// (cx + 1 mod w, cy + 1 mod h); a negative or non-finite lum counts as 0.
__global__ __launch_bounds__(256) void k_env_weights(const float4* texels, int w, int h, float* maxlum) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int cy = (int)(i / (unsigned)w), cx = (int)(i - (unsigned)cy * (unsigned)w);
    const int x1 = (cx + 1 == w) ? 0 : cx + 1, y1 = (cy + 1 == h) ? 0 : cy + 1;
    float m = 0.0f;
    const int tap[4] = {cy * w + cx, cy * w + x1, y1 * w + cx, y1 * w + x1};
    for (int k = 0; k < 4; ++k) {
        const float4 t = texels[tap[k]];
        const float l = lum(mk(t.x, t.y, t.z));
        const float c = (l > 0.0f && l <= RTG_FLT_MAX) ? l : 0.0f;
        m = c > m ? c : m;
    }
    maxlum[i] = m;
}

// rtg_probe_env_samples: env_sample_luminance on given draws
__global__ void k_probe_env(EnvTable et, const unsigned* r0, const float* d, unsigned n, float* out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    v3 wi;
    float pdf;
    env_sample_luminance(et, r0[i], d[3 * (size_t)i], d[3 * (size_t)i + 1], d[3 * (size_t)i + 2], wi, pdf);
    float* o = out + 4 * (size_t)i;
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = pdf;
}

static bool env_active(const rtg_handle* h) { return env_table_set(h).table != nullptr; }

// The map's w * h cell weights (include/rtg.h): the footprint maxima from the texels on the device,
// times the row's sin theta on the host. Waits for the handle's stream.
int env_cell_weights(rtg_handle* h, std::vector<double>& wts) {
    const int w = h->sv.env_w, hh = h->sv.env_h;
    const uint32_t n = (uint32_t)w * (uint32_t)hh;
    DevBuf<float> d_max;
    std::vector<float> maxlum(n);
    wts.assign(n, 0.0);
    if (int rc = d_max.alloc(n)) return rc;
    (void)hipGetLastError();  // drop any stale error left by other code on this thread (as render_impl does)
    hipLaunchKernelGGL(k_env_weights, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->sv.texels + h->sv.env_off, w, hh,
                       d_max.p);
    LAUNCH_OK("k_env_weights");
    HIPOK(hipMemcpyAsync(maxlum.data(), d_max.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    for (int cy = 0; cy < hh; ++cy) {
        const double rs = std::sin(3.14159265358979323846 * ((double)cy + 0.5) / (double)hh);
        for (int cx = 0; cx < w; ++cx) wts[(size_t)cy * w + cx] = (double)maxlum[(size_t)cy * w + cx] * rs;
    }
    return RTG_OK;
}

// The handle's table, once: weights on the device, Vose on the host, entries uploaded. A black map
// leaves no table (the sampler stays uniform).
static int build_env_table(rtg_handle* h) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)h->sv.env_w * (uint32_t)h->sv.env_h;
    DevBuf<uint4> d_tab;
    std::vector<uint32_t> entries;
    std::vector<double> wts;
    if (int rc = env_cell_weights(h, wts)) return rc;
    rtg_env::Alias al;
    if (rtg_env::build_alias(wts.data(), n, al)) {
        entries.resize((size_t)n * 4);
        rtg_env::pack_entries(al, entries.data());
        if (int rc = d_tab.upload((const uint4*)entries.data(), n)) return rc;
    }
    h->env_built = true;
    h->mt.env = std::move(d_tab);
    h->env_entries.swap(entries);
    h->env_weights.swap(wts);
    h->env_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RTG_OK;
}

extern "C" {

int rtg_env_sampling_check(int mode, uint32_t w, uint32_t h) {
    if (mode != RTG_ENV_UNIFORM && mode != RTG_ENV_LUMINANCE) {
        g_err = "rtg_set_env_sampling: unknown mode";
        return RTG_ERR_ARG;
    }
    if (mode == RTG_ENV_LUMINANCE && (uint64_t)w * (uint64_t)h > RTG_ENV_MAX_CELLS) {
        g_err = "rtg_set_env_sampling: the environment map has more than 2^24 texels";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

int rtg_set_env_sampling(rtg_handle* h, int mode) {
    if (!h) { g_err = "rtg_set_env_sampling: null handle"; return RTG_ERR_ARG; }
    const bool lit = h->env_light && h->sv.env_tex >= 0;  // else nothing to sample: accepted, stays uniform
    if (int rc = rtg_env_sampling_check(mode, lit ? (uint32_t)h->sv.env_w : 0u, lit ? (uint32_t)h->sv.env_h : 0u))
        return rc;
    if (int rc = settle(h)) return rc;
    if (mode == RTG_ENV_LUMINANCE && lit && !h->env_built)
        if (int rc = build_env_table(h)) return rc;
    h->env_mode = mode;
    return RTG_OK;
}

int rtg_get_env_sampling(rtg_handle* h, int* mode) {
    if (!h || !mode) { g_err = "rtg_get_env_sampling: null argument"; return RTG_ERR_ARG; }
    *mode = h->env_mode;
    return RTG_OK;
}

int rtg_env_table(rtg_handle* h, uint32_t* w, uint32_t* hh, float* entries, double* build_ms) {
    if (!h || !w || !hh) { g_err = "rtg_env_table: null argument"; return RTG_ERR_ARG; }
    *w = *hh = 0;
    if (build_ms) *build_ms = h->env_build_ms;
    if (!env_active(h)) return RTG_OK;
    *w = (uint32_t)h->sv.env_w;
    *hh = (uint32_t)h->sv.env_h;
    if (entries) std::memcpy(entries, h->env_entries.data(), h->env_entries.size() * sizeof(uint32_t));
    return RTG_OK;
}

int rtg_env_weights(rtg_handle* h, double* weights) {
    if (!h || !weights) { g_err = "rtg_env_weights: null argument"; return RTG_ERR_ARG; }
    if (!env_active(h)) { g_err = "rtg_env_weights: no table is active"; return RTG_ERR_ARG; }
    std::memcpy(weights, h->env_weights.data(), h->env_weights.size() * sizeof(double));
    return RTG_OK;
}

int rtg_env_alias_build(const double* weights, uint32_t n, double* prob, uint32_t* alias, float* entries) {
    if (!weights || !prob || !alias || !entries || n == 0 || n > RTG_ENV_MAX_CELLS) {
        g_err = "rtg_env_alias_build: bad argument";
        return RTG_ERR_ARG;
    }
    rtg_env::Alias al;
    if (!rtg_env::build_alias(weights, n, al)) { g_err = "rtg_env_alias_build: the weights sum to 0"; return RTG_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i) {
        prob[i] = al.prob[i];
        alias[i] = al.alias[i];
    }
    rtg_env::pack_entries(al, reinterpret_cast<uint32_t*>(entries));
    return RTG_OK;
}

int rtg_probe_env_samples(rtg_handle* h, const uint32_t* r0, const float* d, uint32_t n, float* out) {
    if (!h || !r0 || !d || !out) { g_err = "rtg_probe_env_samples: null argument"; return RTG_ERR_ARG; }
    if (!env_active(h)) { g_err = "rtg_probe_env_samples: no table is active"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 4u) { g_err = "rtg_probe_env_samples: too many cases"; return RTG_ERR_ARG; }
    if (n == 0) return RTG_OK;
    HIPOK(hipSetDevice(h->device));
    return probe_run({{r0, (size_t)n * sizeof(unsigned)}, {d, (size_t)n * 3 * sizeof(float)}},
                     {{out, (size_t)n * 4 * sizeof(float)}}, [&](void* const* p) {
                         hipLaunchKernelGGL(k_probe_env, dim3((n + 255) / 256), dim3(256), 0, nullptr, env_table_set(h),
                                            (const unsigned*)p[0], (const float*)p[1], (unsigned)n, (float*)p[2]);
                     });
}

}  // extern "C"
