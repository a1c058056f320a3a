// rtg_denoise.hip — feature-guided film denoiser behind the C-ABI (include/rtg.h, rtg_denoise*).
//
// The counterpart of RayTracer::denoise() (RTBase/Renderer.h:752-793), which hands the film, the
// albedo and the view normals to OIDN and is never called by the reference (its two call sites,
// Renderer.h:230 and :850, are commented out). OIDN's network cannot be reproduced here, so this is
// the project's own classical filter with the same inputs: the edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010), guided by the scene's albedo and shading normals. It is NOT a
// reproduction of OIDN's output.
//
// Definition ("Denoiser"; tests/denoise_ref.py restates it in numpy): iteration i of K
// filters with the 5x5 B3-spline taps h = {1/16, 1/4, 3/8, 1/4, 1/16} at step 1 << i. A tap's
// weight is h[dy] h[dx], times a compactly supported colour and albedo stopping term
// max(0, 1 - |d|^2 / sigma^2)^2 (no exp), times the clamped normal dot product squared m times
// (1 where both pixels are background). Only + - * / and comparisons in IEEE float32 without
// contraction, taps in (dy, dx) order, so the result is pinned bit for bit against the numpy
// restatement.
//
// Data layout: the colour ping-pong holds one 16-B record per pixel (rgb of film / spp, pad); the
// guides one 32-B record, aligned for two dwordx4 loads: {albedo rgb, background flag} {normal
// xyz, pad}. A tap therefore costs three 16-B loads, and a block is 64 x 4 pixels with a wave on
// 64 consecutive x of one row: every tap of a wave is a contiguous row segment at any step, and
// the row tests are wave-uniform. One launch per iteration on the handle's stream, no host wait
// in between. No address depends on a pixel value.
#include "rtg_filter_state.h"

#include <cmath>

struct DenoiseArgs {
    const float4* cin;      // colour records of this iteration's input
    float4* cout;           // ... and output
    const float4* guide;    // two float4 per pixel
    int W, H, step, m;
    int col_on, alb_on;
    float ic, ia;           // 1 / sigma_colour_i^2, 1 / sigma_albedo^2
};

// film sum -> colour record: a true division by (float)spp per channel
__global__ __launch_bounds__(256) void k_dn_pack_colour(const float* __restrict__ sum, float spp, size_t n,
                                                        float4* __restrict__ col) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    col[i] = make_float4(sum[3 * i] / spp, sum[3 * i + 1] / spp, sum[3 * i + 2] / spp, 0.0f);
}

// albedo and normal images -> guide record; .w of the first half is 1 for a background pixel
// (zero normal: both guide integrators return black on a miss)
__global__ __launch_bounds__(256) void k_dn_pack_guide(const float* __restrict__ alb, const float* __restrict__ nrm,
                                                       size_t n, float4* __restrict__ guide) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    const float z = (((nx * nx + ny * ny) + nz * nz) == 0.0f) ? 1.0f : 0.0f;
    guide[2 * i] = make_float4(alb[3 * i], alb[3 * i + 1], alb[3 * i + 2], z);
    guide[2 * i + 1] = make_float4(nx, ny, nz, 0.0f);
}

__global__ __launch_bounds__(256) void k_dn_unpack(const float4* __restrict__ col, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    out[3 * i] = c.x;
    out[3 * i + 1] = c.y;
    out[3 * i + 2] = c.z;
}

static __device__ __forceinline__ float dn_tap(int d) {
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

// one tap: the weight of neighbour (cq, gq0, gq1) for centre (cp, gp0, gp1), folded into sw / acc
static __device__ __forceinline__ void dn_fold(const DenoiseArgs& a, float w, const float4& cp, const float4& gp0,
                                               const float4& gp1, const float4& cq, const float4& gq0,
                                               const float4& gq1, float& sw, float& ar, float& ag, float& ab) {
    if (a.col_on) {
        const float dx = cq.x - cp.x, dy = cq.y - cp.y, dz = cq.z - cp.z;
        const float dd = (dx * dx + dy * dy) + dz * dz;
        float t = 1.0f - dd * a.ic;
        t = t > 0.0f ? t : 0.0f;
        w = w * (t * t);
    }
    if (a.alb_on) {
        const float dx = gq0.x - gp0.x, dy = gq0.y - gp0.y, dz = gq0.z - gp0.z;
        const float dd = (dx * dx + dy * dy) + dz * dz;
        float t = 1.0f - dd * a.ia;
        t = t > 0.0f ? t : 0.0f;
        w = w * (t * t);
    }
    float nd = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
    nd = nd > 0.0f ? nd : 0.0f;
    nd = nd < 1.0f ? nd : 1.0f;
    for (int k = 0; k < a.m; ++k) nd = nd * nd;
    if (gp0.w != 0.0f && gq0.w != 0.0f) nd = 1.0f;
    w = w * nd;
    sw = sw + w;
    ar = ar + w * cq.x;
    ag = ag + w * cq.y;
    ab = ab + w * cq.z;
}

static __device__ __forceinline__ void dn_store(const DenoiseArgs& a, size_t p, const float4& cp, float sw, float ar,
                                                float ag, float ab) {
    float4 o = cp;
    if (sw > 0.0f) o = make_float4(ar / sw, ag / sw, ab / sw, 0.0f);
    a.cout[p] = o;
}

// Direct reads: every tap comes from global memory (L1 / L2 serve the 25-fold reuse). An LDS-staged
// variant for steps 1 and 2 measured slower and is archived (tools/experiments/rtg_denoise_lds.patch,
// DESIGN.md §8a).
__global__ __launch_bounds__(256) void k_dn_atrous(DenoiseArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 cp = a.cin[p], gp0 = a.guide[2 * p], gp1 = a.guide[2 * p + 1];
    float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.H) continue;  // the same for the whole wave (one row)
        const float hy = dn_tap(dy);
        const size_t row = (size_t)qy * (size_t)a.W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.W) continue;
            const size_t q = row + (size_t)qx;
            const float4 cq = a.cin[q], gq0 = a.guide[2 * q], gq1 = a.guide[2 * q + 1];
            dn_fold(a, hy * dn_tap(dx), cp, gp0, gp1, cq, gq0, gq1, sw, ar, ag, ab);
        }
    }
    dn_store(a, p, cp, sw, ar, ag, ab);
}

// ------------------------------------------------------------------ host side
int denoise_check_params(const char* who, const rtg_denoise_params* p) {
    auto bad = [&](const char* what) {
        g_err = std::string(who) + ": " + what;
        return RTG_ERR_ARG;
    };
    if (!p) return bad("null parameters");
    if (p->iterations == 0 || p->iterations > RTG_DENOISE_MAX_ITERATIONS) return bad("iterations must be 1..8");
    if (p->normal_squarings > 8) return bad("normal_squarings must be 0..8");
    for (const float s : {p->sigma_colour, p->sigma_albedo})
        if (!(s <= 0.0f) && !(std::isfinite(s) && s >= 1e-6f)) return bad("a sigma must be <= 0 (off) or finite and >= 1e-6");
    return RTG_OK;
}

// d's six buffers for n pixels
static int alloc_bufs(DenoiseState& d, size_t n) {
    for (DevBuf<float4>& b : d.col)
        if (int rc = b.alloc(n)) return rc;
    if (int rc = d.guide.alloc(2 * n)) return rc;
    for (DevBuf<float>* b : {&d.albedo, &d.normal, &d.out})
        if (int rc = b->alloc(3 * n)) return rc;
    d.n = n;
    return RTG_OK;
}

static int pack_guides(DenoiseState& d, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_pack_guide, dim3((unsigned)((d.n + 255) / 256)), dim3(256), 0, st, (const float*)d.albedo.p,
                       (const float*)d.normal.p, d.n, d.guide.p);
    LAUNCH_OK("k_dn_pack_guide");
    return RTG_OK;
}

// colour sum / spp filtered with the packed guides of d into d.out, all on st (no host wait)
static int filter(DenoiseState& d, hipStream_t st, uint32_t W, uint32_t H, const float* d_sum, uint32_t spp,
                  const rtg_denoise_params& p) {
    const size_t n = (size_t)W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_dn_pack_colour, lin, dim3(256), 0, st, d_sum, (float)spp, n, d.col[0].p);
    LAUNCH_OK("k_dn_pack_colour");
    DenoiseArgs a{};
    a.guide = d.guide.p;
    a.W = (int)W;
    a.H = (int)H;
    a.m = (int)p.normal_squarings;
    a.col_on = p.sigma_colour > 0.0f;
    a.alb_on = p.sigma_albedo > 0.0f;
    a.ia = a.alb_on ? 1.0f / (p.sigma_albedo * p.sigma_albedo) : 0.0f;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        a.cin = d.col[i & 1].p;
        a.cout = d.col[(i + 1) & 1].p;
        a.step = 1 << i;
        const float sc = ldexpf(p.sigma_colour, -(int)i);
        a.ic = a.col_on ? 1.0f / (sc * sc) : 0.0f;
        hipLaunchKernelGGL(k_dn_atrous, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, a);
        LAUNCH_OK("k_dn_atrous");
    }
    hipLaunchKernelGGL(k_dn_unpack, lin, dim3(256), 0, st, (const float4*)d.col[p.iterations & 1].p, n, d.out.p);
    LAUNCH_OK("k_dn_unpack");
    return RTG_OK;
}

void denoise_release(rtg_handle* h) {
    delete h->dn;  // (its buffers and its events with it)
    h->dn = nullptr;
}

void denoise_drop_guides(rtg_handle* h) {
    if (h->dn) h->dn->guides_ready = false;
}

// The handle's denoiser state, built on first use (the film's size never changes): a local one, handed to the
// handle by the last statement, so a failed allocation leaves the handle without one and the next call builds again.
int denoise_state(rtg_handle* h) {
    if (h->dn) return RTG_OK;
    auto d = std::make_unique<DenoiseState>();
    if (int rc = d->ev.create()) return rc;
    if (int rc = alloc_bufs(*d, (size_t)h->W * h->H)) return rc;
    h->dn = d.release();
    return RTG_OK;
}

// The guides, once per handle: 1 sample of the albedo and of the shading-normal integrator into
// scratch films (the film swap of rtg_render_adaptive), every tile, then packed. Both estimators
// stop at the first hit and draw no random number, so the seed and the sample index do not matter.
// The film, Film::SPP, the integrator, the options and the statistics are left as they were.
int ensure_guides(rtg_handle* h, bool wait) {
    DenoiseState& d = *h->dn;
    if (d.guides_ready) return RTG_OK;
    const size_t nf = d.n * 3 * sizeof(float);
    float* const keep_film = h->d_film;
    const int keep_int = h->integrator, keep_count = h->count, keep_timing = h->timing;
    const rtg_stats keep_stats = h->stats;
    const std::vector<double> keep_ms = h->launch_ms;
    const std::vector<unsigned long long> keep_rays = h->launch_rays;
    // the guides stay one centre / pinhole sample each, whatever rtg_set_camera_sampling says
    const rtg_camera_sampling keep_cam = h->cam_sampling;
    (void)rtg_camera_sampling_defaults(&h->cam_sampling);
    h->count = h->timing = 0;
    int rc = RTG_OK;
    const int modes[2] = {RTG_INTEGRATOR_ALBEDO, RTG_INTEGRATOR_NORMALS};
    float* const films[2] = {d.albedo.p, d.normal.p};
    for (int k = 0; k < 2 && rc == RTG_OK; ++k) {
        if (hipMemsetAsync(films[k], 0, nf, h->stream) != hipSuccess) {
            g_err = "rtg_denoise: clearing a guide film failed";
            rc = RTG_ERR_HIP;
            break;
        }
        h->d_film = films[k];
        h->integrator = modes[k];
        rc = render_impl(h, 0, 1, 0, nullptr, 0, h->stream, false, false);
    }
    h->d_film = keep_film;
    h->integrator = keep_int;
    h->cam_sampling = keep_cam;
    h->count = keep_count;
    h->timing = keep_timing;
    h->stats = keep_stats;
    h->launch_ms = keep_ms;
    h->launch_rays = keep_rays;
    if (rc) return rc;
    if ((rc = pack_guides(d, h->stream))) return rc;
    if (wait) HIPOK(hipStreamSynchronize(h->stream));  // otherwise the caller's own wait on h's stream covers them
    d.guides_ready = true;
    return RTG_OK;
}

// Filters d_sum / spp (a film on h's device, ready on h's stream or earlier) with h's guides into
// h's result buffer; waits for it, and copies it to `out` when given.
int denoise_film(rtg_handle* h, const float* d_sum, uint32_t spp, const rtg_denoise_params* p, float* out) {
    if (int rc = denoise_state(h)) return rc;
    if (int rc = ensure_guides(h)) return rc;
    DenoiseState& d = *h->dn;
    HIPOK(hipEventRecord(d.ev[0], h->stream));
    if (int rc = filter(d, h->stream, (uint32_t)h->W, (uint32_t)h->H, d_sum, spp, *p)) return rc;
    HIPOK(hipEventRecord(d.ev[1], h->stream));
    if (out) HIPOK(hipMemcpyAsync(out, d.out.p, d.n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, d.ev[0], d.ev[1]) == hipSuccess) d.ms = ms;
    d.have_result = true;
    return RTG_OK;
}

extern "C" {

int rtg_denoise_defaults(rtg_denoise_params* p) {
    if (!p) { g_err = "rtg_denoise_defaults: null argument"; return RTG_ERR_ARG; }
    p->iterations = 5;
    p->normal_squarings = 5;
    p->sigma_colour = 1.0f;
    p->sigma_albedo = 0.1f;
    return RTG_OK;
}

int rtg_denoise_images(int device, uint32_t w, uint32_t h, const float* colour, const float* albedo,
                       const float* normal, const rtg_denoise_params* p, float* out) {
    if (!colour || !albedo || !normal || !out) { g_err = "rtg_denoise_images: null image"; return RTG_ERR_ARG; }
    if (int rc = check_size("rtg_denoise_images", w, h, "image size")) return rc;
    if (int rc = denoise_check_params("rtg_denoise_images", p)) return rc;
    HIPOK(hipSetDevice(device));
    DenoiseState d;  // local: freed on every way out
    DevBuf<float> d_sum;
    const size_t n = (size_t)w * h;
    if (int rc = alloc_bufs(d, n)) return rc;
    if (int rc = d_sum.upload(colour, 3 * n)) return rc;
    HIPOK(hipMemcpy(d.albedo.p, albedo, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d.normal.p, normal, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = pack_guides(d, nullptr)) return rc;
    if (int rc = filter(d, nullptr, w, h, d_sum.p, 1u, *p)) return rc;  // x / 1.0f is x
    HIPOK(hipStreamSynchronize(nullptr));
    return d.out.download(out, 3 * n);
}

int rtg_denoise(rtg_handle* h, const rtg_denoise_params* p, float* out) {
    if (!h) { g_err = "rtg_denoise: null handle"; return RTG_ERR_ARG; }
    if (int rc = denoise_check_params("rtg_denoise", p)) return rc;
    if (h->spp == 0) { g_err = "rtg_denoise: the film holds no samples (spp == 0)"; return RTG_ERR_ARG; }
    if (int rc = check_size("rtg_denoise", h->W, h->H, "image size")) return rc;
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;  // the film holds every queued frame first
    return denoise_film(h, h->d_film, h->spp, p, out);
}

int rtg_denoise_guides(rtg_handle* h, float* albedo, float* normal) {
    if (!h) { g_err = "rtg_denoise_guides: null handle"; return RTG_ERR_ARG; }
    if (int rc = check_size("rtg_denoise_guides", h->W, h->H, "image size")) return rc;
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;
    if (int rc = denoise_state(h)) return rc;
    if (int rc = ensure_guides(h)) return rc;
    if (albedo)
        if (int rc = h->dn->albedo.download(albedo, 3 * h->dn->n)) return rc;
    if (normal)
        if (int rc = h->dn->normal.download(normal, 3 * h->dn->n)) return rc;
    return RTG_OK;
}

int rtg_denoise_copy_device(rtg_handle* h, void* dst_device) {
    const bool have = h && h->dn && h->dn->have_result;
    return copy_result("rtg_denoise_copy_device", h, have ? h->dn->out.p : nullptr, dst_device, "no denoised result yet");
}

double rtg_denoise_ms(rtg_handle* h) { return (h && h->dn) ? h->dn->ms : 0.0; }

}  // extern "C"
