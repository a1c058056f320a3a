// rtg_svgf_illum.hip — the illumination mode of the variance-guided chain behind the C-ABI (include/rtg.h,
// rtg_svgf_illum_*; tests/svgf_illum_ref.py restates it in numpy).
//
// rtg_svgf.hip's chain run on the film over the first hit's albedo, with the pixels that see an emitter
// directly kept apart from every surface: a prepare pass writes F' = film / d and the classed guide G' (an
// emitter's first hit becomes a miss record), the chain's own kernels (svgf_queue: k_svgf_temporal,
// k_svgf_variance, k_svgf_pack_pos, k_svgf_atrous, unchanged, with other pointers) run on F' and G' over a
// history, moments, history camera and history guide of the mode's own, and the unpack multiplies by d again.
// d.c = A.c > albedo_floor ? A.c : 1.0f is recomputed from the denoiser's planar albedo by both kernels, not
// stored. IEEE float32 without contraction; one division and one product per channel.
//
// Data per pixel: prepare reads the film (12 B), the albedo (12 B) and the guide record (32 B), for a hit the
// material index of its shading record (16 B of the 64) and the material's first 16 B; it writes 12 + 32 B. The
// unpack reads the 16-B colour record and the albedo (12 B) and writes 12 B. One thread per pixel, 256-thread
// blocks; no LDS, no atomics; no address depends on a colour.
#include "rtg_filter_state.h"

#include <cmath>

static __device__ __forceinline__ float il_div(float a, float floor) { return a > floor ? a : 1.0f; }  // NaN: 1

__global__ __launch_bounds__(256) void k_svgf_illum_prepare(const float* __restrict__ film, const float* __restrict__ albedo,
                                                            const float4* __restrict__ geo,
                                                            const DevShade* __restrict__ shade,
                                                            const DevMat* __restrict__ mats, float floor, size_t n,
                                                            float* __restrict__ fout, float4* __restrict__ gout) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 g0 = geo[2 * i], g1 = geo[2 * i + 1];
    const int id = __float_as_int(g1.w);
    if (id >= 0) {
        const DevMat& M = mats[__float_as_int(shade[id].d.w)];
        if (M.is_light) {  // k_gbuffer's test: an emitter's first hit is a class of its own, kept as a miss
            g0 = make_float4(0.0f, 0.0f, 0.0f, RTG_FLT_MAX);
            g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        }
    }
    gout[2 * i] = g0;
    gout[2 * i + 1] = g1;
    fout[3 * i] = film[3 * i] / il_div(albedo[3 * i], floor);
    fout[3 * i + 1] = film[3 * i + 1] / il_div(albedo[3 * i + 1], floor);
    fout[3 * i + 2] = film[3 * i + 2] / il_div(albedo[3 * i + 2], floor);
}

// k_svgf_unpack, remodulated
__global__ __launch_bounds__(256) void k_svgf_illum_unpack(const float4* __restrict__ col, const float* __restrict__ albedo,
                                                           float floor, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    out[3 * i] = c.x * il_div(albedo[3 * i], floor);
    out[3 * i + 1] = c.y * il_div(albedo[3 * i + 1], floor);
    out[3 * i + 2] = c.z * il_div(albedo[3 * i + 2], floor);
}

// ------------------------------------------------------------------ host side
// The temporal state's illumination part, built on first use: a local one, handed to t by the last statement.
static int build_state(TemporalState& t) {
    if (t.il) return RTG_OK;
    auto s = std::make_unique<SvgfIllumState>();
    if (int rc = svgf_alloc(s->sv, t.n)) return rc;
    for (DevBuf<float4>* b : {&s->k.hist[0], &s->k.hist[1]})
        if (int rc = b->alloc(t.n)) return rc;
    for (DevBuf<float4>* b : {&s->k.hguide, &s->guide})
        if (int rc = b->alloc(2 * t.n)) return rc;
    if (int rc = s->film.alloc(3 * t.n)) return rc;
    t.il = std::move(s);
    return RTG_OK;
}

static int illum_check(const char* who, const rtg_svgf_illum_params* p) {
    if (!p) { g_err = std::string(who) + ": null parameters"; return RTG_ERR_ARG; }
    if (int rc = svgf_check(who, &p->svgf)) return rc;
    if (!(std::isfinite(p->albedo_floor) && p->albedo_floor > 0.0f)) {
        g_err = std::string(who) + ": albedo_floor must be finite and > 0";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

// the state once a call has left a result (the history with it), or null with "who: ..." as the message
static SvgfIllumState* result_state(const char* who, rtg_handle* h) {
    if (!h) { g_err = std::string(who) + ": null argument"; return nullptr; }
    if (!h->tp || !h->tp->il || !h->tp->il->sv.have_result) { g_err = std::string(who) + ": no result yet"; return nullptr; }
    return h->tp->il.get();
}

extern "C" {

int rtg_svgf_illum_defaults(rtg_svgf_illum_params* p) {
    if (!p) { g_err = "rtg_svgf_illum_defaults: null argument"; return RTG_ERR_ARG; }
    (void)rtg_svgf_defaults(&p->svgf);
    p->albedo_floor = 1e-3f;
    return RTG_OK;
}

int rtg_svgf_illum_check(const rtg_svgf_illum_params* p) { return illum_check("rtg_svgf_illum_check", p); }

int rtg_svgf_illum_accumulate(rtg_handle* h, const rtg_svgf_illum_params* p, float* out) {
    if (!h) { g_err = "rtg_svgf_illum_accumulate: null handle"; return RTG_ERR_ARG; }
    if (int rc = illum_check("rtg_svgf_illum_accumulate", p)) return rc;
    if (h->spp == 0) { g_err = "rtg_svgf_illum_accumulate: the film holds no samples (spp == 0)"; return RTG_ERR_ARG; }
    if (int rc = settle(h)) return rc;  // the film holds every queued frame, and slot 0's buffers are free
    if (int rc = temporal_state("rtg_svgf_illum_accumulate", h)) return rc;
    TemporalState& t = *h->tp;
    if (int rc = build_state(t)) return rc;
    if (int rc = denoise_state(h)) return rc;
    SvgfIllumState& il = *t.il;
    SvgfState& s = il.sv;
    hipStream_t st = h->stream;
    const float4* g = nullptr;  // the unclassed guide of the current camera, from the caches as they are
    bool traced = false, unchanged = false;
    HIPOK(hipEventRecord(s.ev[0], st));
    if (int rc = current_guide(h, true, &g, &traced)) return rc;
    HIPOK(hipEventRecord(s.ev[1], st));
    const dim3 lin((unsigned)((t.n + 255) / 256));
    hipLaunchKernelGGL(k_svgf_illum_prepare, lin, dim3(256), 0, st, (const float*)h->d_film,
                       (const float*)h->dn->albedo.p, g, h->sv.shade, h->sv.mats, p->albedo_floor, t.n, il.film.p,
                       il.guide.p);
    LAUNCH_OK("k_svgf_illum_prepare");
    // (with the camera unchanged il.guide holds the bits of the history's own classed guide)
    if (int rc = svgf_queue(h, &p->svgf, il.k, s, il.film.p, il.guide.p, &unchanged)) return rc;
    hipLaunchKernelGGL(k_svgf_illum_unpack, lin, dim3(256), 0, st, (const float4*)s.col[p->svgf.iterations & 1].p,
                       (const float*)h->dn->albedo.p, p->albedo_floor, t.n, s.out.p);
    LAUNCH_OK("k_svgf_illum_unpack");
    HIPOK(hipEventRecord(s.ev[6], st));
    if (out) HIPOK(hipMemcpyAsync(out, s.out.p, t.n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    svgf_done(s, traced);
    il.prepare_ms = stage_ms(true, s.ev[1], s.ev[2]);
    il.unpack_ms = stage_ms(true, s.ev[5], s.ev[6]);
    t.gbuffer_ms = s.guide_ms;
    il.k.cur ^= 1;
    if (!unchanged) {  // the stored camera and classed guide become the current ones
        std::swap(il.k.hguide, il.guide);
        il.k.hcam = h->cam;
        il.k.hproj = h->proj;
        il.k.have_hist = true;
    }
    return RTG_OK;
}

int rtg_svgf_illum_history(rtg_handle* h, float* rgb_len) {
    SvgfIllumState* s = result_state("rtg_svgf_illum_history", rgb_len ? h : nullptr);
    if (!s) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(rgb_len, s->k.hist[s->k.cur].p, h->tp->n * sizeof(float4), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_svgf_illum_variance(rtg_handle* h, float* var) {
    SvgfIllumState* s = result_state("rtg_svgf_illum_variance", var ? h : nullptr);
    if (!s) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(var, s->sv.var.p, h->tp->n * sizeof(float), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_svgf_illum_moments(rtg_handle* h, float* mu) {
    SvgfIllumState* s = result_state("rtg_svgf_illum_moments", mu ? h : nullptr);
    if (!s) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(mu, s->sv.mom[s->sv.cur].p, h->tp->n * sizeof(float2), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_svgf_illum_guide(rtg_handle* h, float* pos_t, float* normal_id) {
    SvgfIllumState* s = result_state("rtg_svgf_illum_guide", h);
    if (!s) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    return download_guide(h, s->k.hguide.p, pos_t, normal_id);
}

int rtg_svgf_illum_copy_device(rtg_handle* h, void* dst_device) {
    const bool have = h && h->tp && h->tp->il && h->tp->il->sv.have_result;
    return copy_result("rtg_svgf_illum_copy_device", h, have ? h->tp->il->sv.out.p : nullptr, dst_device);
}

int rtg_svgf_illum_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms, double* variance_ms, double* filter_ms,
                      double* prepare_ms, double* unpack_ms) {
    if (!h) { g_err = "rtg_svgf_illum_ms: null handle"; return RTG_ERR_ARG; }
    const SvgfIllumState* s = h->tp ? h->tp->il.get() : nullptr;
    if (guide_ms) *guide_ms = s ? s->sv.guide_ms : 0.0;
    if (accumulate_ms) *accumulate_ms = s ? s->sv.accumulate_ms : 0.0;
    if (variance_ms) *variance_ms = s ? s->sv.variance_ms : 0.0;
    if (filter_ms) *filter_ms = s ? s->sv.filter_ms : 0.0;
    if (prepare_ms) *prepare_ms = s ? s->prepare_ms : 0.0;
    if (unpack_ms) *unpack_ms = s ? s->unpack_ms : 0.0;
    return RTG_OK;
}

}  // extern "C"
