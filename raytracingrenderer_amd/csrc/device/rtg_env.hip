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

static bool env_active(const rtg_handle* h) { return h->env_mode == RTG_ENV_LUMINANCE && h->d_env_table != nullptr; }

EnvTable env_table_of(const rtg_handle* h) {
    const bool samples_light = h->integrator == RTG_INTEGRATOR_PATH || h->integrator == RTG_INTEGRATOR_DIRECT ||
                               h->integrator == RTG_INTEGRATOR_DIRECT_MIS;
    if (!env_active(h) || !samples_light) return EnvTable{nullptr, 0u, 0u, 0u};
    const unsigned w = (unsigned)h->sv.env_w, hh = (unsigned)h->sv.env_h;
    return EnvTable{h->d_env_table, w * hh, w, hh};
}

// The map's w * h cell weights (include/rtg.h): the footprint maxima from the texels on the device,
// times the row's sin theta on the host. Waits for the handle's stream.
int env_cell_weights(rtg_handle* h, std::vector<double>& wts) {
    const int w = h->sv.env_w, hh = h->sv.env_h;
    const uint32_t n = (uint32_t)w * (uint32_t)hh;
    float* d_max = nullptr;
    std::vector<float> maxlum(n);
    wts.assign(n, 0.0);
    auto run = [&]() -> int {
        HIPOK(hipMalloc((void**)&d_max, (size_t)n * sizeof(float)));
        (void)hipGetLastError();  // drop any stale error left by other code on this thread (as render_impl does)
        hipLaunchKernelGGL(k_env_weights, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->sv.texels + h->sv.env_off, w,
                           hh, d_max);
        LAUNCH_OK("k_env_weights");
        HIPOK(hipMemcpyAsync(maxlum.data(), d_max, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (int cy = 0; cy < hh; ++cy) {
            const double rs = std::sin(3.14159265358979323846 * ((double)cy + 0.5) / (double)hh);
            for (int cx = 0; cx < w; ++cx) wts[(size_t)cy * w + cx] = (double)maxlum[(size_t)cy * w + cx] * rs;
        }
        return RTG_OK;
    };
    const int rc = run();
    (void)hipFree(d_max);
    return rc;
}

// The handle's table, once: weights on the device, Vose on the host, entries uploaded. A black map
// leaves no table (the sampler stays uniform).
static int build_env_table(rtg_handle* h) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)h->sv.env_w * (uint32_t)h->sv.env_h;
    uint4* d_tab = nullptr;
    std::vector<uint32_t> entries;
    std::vector<double> wts;
    bool have = false;
    auto run = [&]() -> int {
        if (int rc = env_cell_weights(h, wts)) return rc;
        rtg_env::Alias al;
        have = rtg_env::build_alias(wts.data(), n, al);
        if (!have) return RTG_OK;
        entries.resize((size_t)n * 4);
        rtg_env::pack_entries(al, entries.data());
        HIPOK(hipMalloc((void**)&d_tab, (size_t)n * 16));
        HIPOK(hipMemcpy(d_tab, entries.data(), (size_t)n * 16, hipMemcpyHostToDevice));
        return RTG_OK;
    };
    const int rc = run();
    if (rc != RTG_OK) {
        (void)hipFree(d_tab);
        return rc;
    }
    h->env_built = true;
    h->d_env_table = have ? d_tab : nullptr;
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
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;  // queued calls render with the settings they were queued under
    HIPOK(hipStreamSynchronize(h->stream));
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
    const unsigned w = (unsigned)h->sv.env_w, hh = (unsigned)h->sv.env_h;
    const EnvTable et{h->d_env_table, w * hh, w, hh};
    unsigned* d_r = nullptr;
    float *d_d = nullptr, *d_out = nullptr;
    auto run = [&]() -> int {
        HIPOK(hipMalloc((void**)&d_r, (size_t)n * sizeof(unsigned)));
        HIPOK(hipMalloc((void**)&d_d, (size_t)n * 3 * sizeof(float)));
        HIPOK(hipMalloc((void**)&d_out, (size_t)n * 4 * sizeof(float)));
        HIPOK(hipMemcpy(d_r, r0, (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_d, d, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
        (void)hipGetLastError();  // (a stale error of other code on this thread is not this launch's)
        hipLaunchKernelGGL(k_probe_env, dim3((n + 255) / 256), dim3(256), 0, nullptr, et, (const unsigned*)d_r,
                           (const float*)d_d, (unsigned)n, d_out);
        HIPOK(hipGetLastError());
        HIPOK(hipDeviceSynchronize());
        HIPOK(hipMemcpy(out, d_out, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost));
        return RTG_OK;
    };
    const int rc = run();
    (void)hipFree(d_r);
    (void)hipFree(d_d);
    (void)hipFree(d_out);
    return rc;
}

}  // extern "C"
