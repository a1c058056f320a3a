// rtg_temporal.hip — the geometry guide and temporal accumulation by reprojection behind the C-ABI
// (include/rtg.h: rtg_geometry_guide, rtg_temporal_*; tests/temporal_ref.py restates
// both in numpy).
//
// A frame loop that moves its camera (Main.cpp:82-111) clears the film after every move and shows
// 1-spp frames. This unit carries the samples of earlier views into the new one: a per-pixel history
// {rgb, len} is kept with the camera it was seen from and that camera's geometry guide (per pixel the
// first hit's position, distance, unit geometric normal and triangle id). After a move the current
// pixel's surface point is projected into the history's camera with Camera::projectOntoCamera's own
// operations, the four history pixels around it are blended bilinearly, each tap admitted only when it
// lies on the same plane (within plane_tolerance * t) and faces the same way (normal_cos), and the
// film's mean is blended in with weight m / (n + m). Only + - * /, sqrtf, floorf and comparisons in
// IEEE float32 without contraction, taps in (dy, dx) order: pinned bit for bit against the restatement.
//
// Data layout: the history is one 16-B record per pixel (a ping-pong pair: a move reads the old one at
// four neighbours while the new one is written); a guide is one 32-B record, aligned for two dwordx4
// loads: {X.xyz, t} {Ng.xyz, triangle id}. A moved pixel therefore costs its own guide (2 loads), the
// film's three floats and at most 4 x 3 tap loads; it writes one history record and three floats.
// Blocks are 64 x 4 pixels with a wave on 64 consecutive x of one row, as k_dn_atrous lays them out.
// No atomics; no address depends on a colour (the tap addresses depend on geometry alone).
#include "rtg_reproject.h"

#include <cmath>
#include <cstring>

struct TemporalArgs {
    const float* film;     // the film's sums, 3 floats per pixel
    float m;               // (float)spp
    int mode;              // 0: no history; 1: camera unchanged (identity); 2: camera moved (reprojection)
    const float4* hin;     // history read (modes 1 and 2)
    float4* hout;          // history written
    const float4* gcur;    // the current camera's guide (mode 2)
    const float4* ghist;   // the history camera's guide (mode 2)
    float* out;            // the result, 3 floats per pixel
    int W, H;
    float max_history, plane_tolerance, normal_cos;
    TemporalProj cam;      // mode 2
};

// first hits -> guide records. One thread per pixel of the list (every tile: the whole film).
__global__ __launch_bounds__(256) void k_geometry_guide(const DevTri48* __restrict__ tris,
                                                        const unsigned* __restrict__ pixlist, unsigned npix,
                                                        const float4* __restrict__ hits,
                                                        const float4* __restrict__ ray_d, float ox, float oy,
                                                        float oz, float4* __restrict__ guide) {
    const unsigned lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= npix) return;
    const unsigned pixel = pixlist[lp];
    const float4 h = hits[lp];
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, RTG_FLT_MAX);
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    if (h.x < RTG_FLT_MAX) {
        const float4 d = ray_d[lp];
        const float t = h.x;
        const int id = __float_as_int(h.y);
        const DevTri48 T = tris[id];
        const v3 v0 = mk(T.a.w, T.b.x, T.b.y), v1 = mk(T.b.z, T.b.w, T.c.x), v2 = mk(T.c.y, T.c.z, T.c.w);
        const v3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z), e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
        const float cx = e1.y * e2.z - e1.z * e2.y;
        const float cy = e1.z * e2.x - e1.x * e2.z;
        const float cz = e1.x * e2.y - e1.y * e2.x;
        const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
        g0 = make_float4(ox + d.x * t, oy + d.y * t, oz + d.z * t, t);  // Ray::at
        g1 = make_float4(cx / l, cy / l, cz / l, __int_as_float(id));
    }
    guide[2 * (size_t)pixel] = g0;
    guide[2 * (size_t)pixel + 1] = g1;
}

__global__ __launch_bounds__(256) void k_temporal(TemporalArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float cr = a.film[3 * p] / a.m, cg = a.film[3 * p + 1] / a.m, cb = a.film[3 * p + 2] / a.m;
    bool have = false;
    float4 hist = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.mode == 1) {
        hist = a.hin[p];
        have = true;
    } else if (a.mode == 2) {
        const float4 g0 = a.gcur[2 * p], g1 = a.gcur[2 * p + 1];
        float fx, fy;
        if (__float_as_int(g1.w) >= 0 && rp_project(a.cam, g0.x, g0.y, g0.z, fx, fy)) {
            const float u = fx - 0.5f, v = fy - 0.5f;
            const float x0 = floorf(u), y0 = floorf(v);
            const float ax = u - x0, ay = v - y0;
            const float tol = a.plane_tolerance * g0.w;
            const float Wf = (float)a.W, Hf = (float)a.H;
            float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, al = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const float qyf = y0 + (float)dy;
                const float wy = dy ? ay : 1.0f - ay;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const float qxf = x0 + (float)dx;
                    const float w = (dx ? ax : 1.0f - ax) * wy;
                    // float comparisons: a NaN position fails them, and inside them the casts are exact
                    if (!(qxf >= 0.0f && qxf < Wf && qyf >= 0.0f && qyf < Hf) || !(w > 0.0f)) continue;
                    const size_t q = (size_t)(int)qyf * (size_t)a.W + (size_t)(int)qxf;
                    const float4 h1 = a.ghist[2 * q + 1];
                    if (__float_as_int(h1.w) < 0) continue;
                    const float4 h0 = a.ghist[2 * q];
                    const float pd = rp_dot(h0.x - g0.x, h0.y - g0.y, h0.z - g0.z, g1.x, g1.y, g1.z);
                    if (!(fabsf(pd) <= tol)) continue;
                    const float nd = rp_dot(h1.x, h1.y, h1.z, g1.x, g1.y, g1.z);
                    if (!(fabsf(nd) >= a.normal_cos)) continue;
                    const float4 hq = a.hin[q];
                    sw = sw + w;
                    ar = ar + w * hq.x;
                    ag = ag + w * hq.y;
                    ab = ab + w * hq.z;
                    al = al + w * hq.w;
                }
            }
            if (sw > 0.0f) {
                hist = make_float4(ar / sw, ag / sw, ab / sw, al / sw);
                have = true;
            }
        }
    }
    float4 o = make_float4(cr, cg, cb, a.m);
    if (have) {
        const float n = hist.w < a.max_history ? hist.w : a.max_history;
        const float al = a.m / (n + a.m);
        o = make_float4(hist.x + (cr - hist.x) * al, hist.y + (cg - hist.y) * al, hist.z + (cb - hist.z) * al, n + a.m);
    }
    a.hout[p] = o;
    a.out[3 * p] = o.x;
    a.out[3 * p + 1] = o.y;
    a.out[3 * p + 2] = o.z;
}

// ------------------------------------------------------------------ host side
void temporal_release(rtg_handle* h) {
    delete h->tp;  // (its buffers, its events and the variance-guided state with it)
    h->tp = nullptr;
}

int check_size(const char* who, int64_t W, int64_t H, const char* what) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || W * H > (1ll << 28)) {
        g_err = std::string(who) + ": " + what + " must be 1..65535 per side and at most 2^28 pixels";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

// The handle's temporal state, built on first use: a local one, handed to the handle by the last statement, so
// a failed allocation leaves the handle without one and the next call builds again.
static int build_state(rtg_handle* h) {
    if (h->tp) return RTG_OK;
    auto t = std::make_unique<TemporalState>();
    const size_t n = (size_t)h->W * h->H;
    if (int rc = t->ev.create()) return rc;
    for (DevBuf<float4>* b : {&t->hist[0], &t->hist[1]})
        if (int rc = b->alloc(n)) return rc;
    for (DevBuf<float4>* b : {&t->hguide, &t->cguide})
        if (int rc = b->alloc(2 * n)) return rc;
    if (int rc = t->out.alloc(3 * n)) return rc;
    t->n = n;
    h->tp = t.release();
    return RTG_OK;
}

bool same_camera(const DevCamera& a, const rtg_camera_proj& ap, const DevCamera& b, const rtg_camera_proj& bp) {
    return std::memcmp(&a, &b, sizeof(DevCamera)) == 0 && std::memcmp(&ap, &bp, sizeof(rtg_camera_proj)) == 0;
}

// The first hits of the handle's camera into slot 0's buffers, on h's stream (no host wait): one pinhole ray
// through every pixel centre, whatever rtg_set_camera_sampling says, by the generate and traversal kernels
// (the camera pass of rtg_render_instant_radiosity). The caller has joined the queued frames and waited for
// the stream (slot 0's buffers are free). The options, the statistics and the film are not touched: no
// counting kernels, no tally, no film write.
static int trace_first_hits(rtg_handle* h, PathBufs** out) {
    hipStream_t st = h->stream;
    int rc;
    if ((rc = set_pixels(h, nullptr, 0))) return rc;
    const unsigned npix = h->npix;
    if ((rc = ensure_chunk(h, h->slot[0], npix, std::max(h->slot[0].cap_maxb, 1), true))) return rc;
    if ((rc = ensure_ovf(h, h->slot[0]))) return rc;
    PathBufs& pb = h->slot[0].pb;
    ChunkArgs ca{};
    ca.pixlist = h->d_pix;
    ca.npix = npix;
    ca.ns = 1;
    ca.s0 = 0;
    ca.P = npix;
    ca.seed = 0;
    ca.max_depth = h->max_depth;
    ca.mode = RTG_INTEGRATOR_PATH;
    ca.cam = h->cam;
    HIPOK(hipMemsetAsync(pb.ctr, 0, 2 * sizeof(Counters), st));
    (void)hipGetLastError();  // drop any stale error left by other code on this thread (as render_impl does)
    if ((rc = launch_generate(h, ca, pb, st))) return rc;
    TraceIO io{};
    io.stats = h->d_stats;
    io.cull = h->cull;
    io.wide = h->wide;
    io.ovf = h->slot[0].d_ovf;
    io.queue = pb.q[0];
    io.ray_o = pb.ray_o;
    io.ray_d = pb.ray_d;
    io.count = &pb.ctr[0].n_ext;
    io.hits = pb.hits;
    io.fetch = &pb.ctr[0].f_ext;
    const int keep_count = h->count;
    h->count = 0;  // the plain traversal kernels: the counting ones would add to rtg_stats
    rc = launch_trace(h, io, st);
    h->count = keep_count;
    if (rc) return rc;
    *out = &pb;
    return RTG_OK;
}

// The guide of the handle's camera, on h's stream (no host wait): the history's own when the camera is its
// camera, the cache's when it holds this camera, else traced into the cache (trace_first_hits, then
// k_geometry_guide). with_denoiser: the denoiser's albedo / shading-normal guides with it (rtg_gbuffer.hip,
// DESIGN.md 8k). Then nothing runs only when the geometry guide is at hand and the denoiser's guides are ready
// as well; otherwise the one pass is trace_first_hits, then k_gbuffer into the guide cache and the denoiser's three
// guide buffers, and both caches are valid for this camera. Without it h->dn is not looked at (it may be null).
// The camera rays are traced once; the film, Film::SPP, the integrator, the options, the statistics, launch_ms /
// launch_rays and the camera-sampling record are not touched. The caller has joined the queued frames, waited
// for the stream, and built the states it asks for (temporal_state; denoise_state for with_denoiser).
int current_guide(rtg_handle* h, bool with_denoiser, const float4** guide, bool* traced) {
    TemporalState& t = *h->tp;
    DenoiseState* d = with_denoiser ? h->dn : nullptr;
    *traced = false;
    const bool own = t.have_hist && same_camera(h->cam, h->proj, t.hcam, t.hproj);
    const bool cached = t.cache_ready && same_camera(h->cam, h->proj, t.ccam, t.cproj);
    if ((own || cached) && (!d || d->guides_ready)) { *guide = own ? t.hguide.p : t.cguide.p; return RTG_OK; }
    t.cache_ready = false;
    if (d) d->guides_ready = false;
    PathBufs* pb = nullptr;
    if (int rc = trace_first_hits(h, &pb)) return rc;
    if (d) {
        if (int rc = launch_gbuffer(h, *pb, t.cguide.p, *d, h->stream)) return rc;
    } else {
        hipLaunchKernelGGL(k_geometry_guide, dim3((h->npix + 255) / 256), dim3(256), 0, h->stream, h->sv.tris48,
                           (const unsigned*)h->d_pix, h->npix, (const float4*)pb->hits, (const float4*)pb->ray_d,
                           h->cam.ox, h->cam.oy, h->cam.oz, t.cguide.p);
        LAUNCH_OK("k_geometry_guide");
    }
    t.ccam = h->cam;
    t.cproj = h->proj;
    t.cache_ready = true;
    if (d) d->guides_ready = true;
    *guide = own ? t.hguide.p : t.cguide.p;  // (the same bits; the history keeps its own buffer)
    *traced = true;
    return RTG_OK;
}

int download_guide(const rtg_handle* h, const float4* guide, float* pos_t, float* normal_id) {
    if (!pos_t && !normal_id) return RTG_OK;
    const size_t n = (size_t)h->W * h->H;
    std::vector<float4> rec(2 * n);  // the two halves of a record go to the caller's two images
    HIPOK(hipMemcpy(rec.data(), guide, rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (pos_t) std::memcpy(pos_t + 4 * i, &rec[2 * i], sizeof(float4));
        if (normal_id) std::memcpy(normal_id + 4 * i, &rec[2 * i + 1], sizeof(float4));
    }
    return RTG_OK;
}

int copy_result(const char* who, rtg_handle* h, const float* result, void* dst_device, const char* none) {
    if (!h || !dst_device) { g_err = std::string(who) + ": null argument"; return RTG_ERR_ARG; }
    if (!result) { g_err = std::string(who) + ": " + none; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipMemcpyAsync(dst_device, result, (size_t)h->W * h->H * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    return RTG_OK;
}

int temporal_state(const char* who, rtg_handle* h) {
    if (int rc = check_size(who, h->W, h->H)) return rc;
    return build_state(h);
}

void temporal_advance(rtg_handle* h, bool unchanged, const float4* g) {
    TemporalState& t = *h->tp;
    t.cur ^= 1;
    if (!unchanged) {  // the stored camera and guide become the current ones
        if (g == t.cguide.p) {
            // the cache's buffer becomes the history's; the history's old guide stays cached under its camera
            std::swap(t.hguide, t.cguide);
            const bool was = t.have_hist;
            t.ccam = t.hcam;
            t.cproj = t.hproj;
            t.cache_ready = was;
        }
        t.hcam = h->cam;
        t.hproj = h->proj;
        t.have_hist = true;
    }
}

int temporal_check(const char* who, const rtg_temporal_params* p) {
    auto bad = [&](const char* what) {
        g_err = std::string(who) + ": " + what;
        return RTG_ERR_ARG;
    };
    if (!p) return bad("null parameters");
    if (!(p->max_history > 0.0f)) return bad("max_history must be > 0 (+inf allowed)");
    if (!(std::isfinite(p->plane_tolerance) && p->plane_tolerance >= 0.0f)) return bad("plane_tolerance must be finite and >= 0");
    if (!(p->normal_cos >= 0.0f && p->normal_cos <= 1.0f)) return bad("normal_cos must be in [0, 1]");
    return RTG_OK;
}

extern "C" {

int rtg_temporal_defaults(rtg_temporal_params* p) {
    if (!p) { g_err = "rtg_temporal_defaults: null argument"; return RTG_ERR_ARG; }
    p->max_history = 64.0f;
    p->plane_tolerance = 0.01f;
    p->normal_cos = 0.9f;
    return RTG_OK;
}

int rtg_temporal_check(const rtg_temporal_params* p) { return temporal_check("rtg_temporal_check", p); }

int rtg_geometry_guide(rtg_handle* h, float* pos_t, float* normal_id) {
    if (!h) { g_err = "rtg_geometry_guide: null handle"; return RTG_ERR_ARG; }
    if (int rc = check_size("rtg_geometry_guide", h->W, h->H)) return rc;
    if (int rc = settle(h)) return rc;  // slot 0's buffers are free
    if (int rc = build_state(h)) return rc;
    TemporalState& t = *h->tp;
    const float4* g = nullptr;
    bool traced = false;
    HIPOK(hipEventRecord(t.ev[0], h->stream));
    if (int rc = current_guide(h, false, &g, &traced)) return rc;
    HIPOK(hipEventRecord(t.ev[1], h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    t.guide_ms = stage_ms(traced, t.ev[0], t.ev[1]);
    return download_guide(h, g, pos_t, normal_id);
}

int rtg_temporal_accumulate(rtg_handle* h, const rtg_temporal_params* p, float* out) {
    if (!h) { g_err = "rtg_temporal_accumulate: null handle"; return RTG_ERR_ARG; }
    if (int rc = temporal_check("rtg_temporal_accumulate", p)) return rc;
    if (h->spp == 0) { g_err = "rtg_temporal_accumulate: the film holds no samples (spp == 0)"; return RTG_ERR_ARG; }
    if (int rc = check_size("rtg_temporal_accumulate", h->W, h->H)) return rc;
    if (int rc = settle(h)) return rc;  // the film holds every queued frame, and slot 0's buffers are free
    if (int rc = build_state(h)) return rc;
    TemporalState& t = *h->tp;
    TemporalArgs a{};
    const bool unchanged = temporal_setup(h, t, *p, a);
    a.out = t.out.p;
    const float4* g = nullptr;
    bool traced = false;
    HIPOK(hipEventRecord(t.ev[0], h->stream));
    if (!unchanged)  // (the denoiser's guides are not this call's: h->dn may not exist)
        if (int rc = current_guide(h, false, &g, &traced)) return rc;
    HIPOK(hipEventRecord(t.ev[1], h->stream));
    if (a.mode == 2) a.gcur = g;
    HIPOK(hipEventRecord(t.ev[2], h->stream));
    hipLaunchKernelGGL(k_temporal, dim3((unsigned)(h->W + 63) / 64, (unsigned)(h->H + 3) / 4), dim3(256), 0, h->stream, a);
    LAUNCH_OK("k_temporal");
    HIPOK(hipEventRecord(t.ev[3], h->stream));
    if (out) HIPOK(hipMemcpyAsync(out, t.out.p, t.n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    t.guide_ms = stage_ms(traced, t.ev[0], t.ev[1]);
    if (hipEventElapsedTime(&ms, t.ev[2], t.ev[3]) == hipSuccess) t.accumulate_ms = ms;
    temporal_advance(h, unchanged, g);
    if (t.sv) t.sv->mom_valid = false;  // the moments history of rtg_svgf_accumulate no longer belongs to H
    t.have_result = true;
    return RTG_OK;
}

int rtg_temporal_history(rtg_handle* h, float* rgb_len) {
    if (!h || !rgb_len) { g_err = "rtg_temporal_history: null argument"; return RTG_ERR_ARG; }
    if (!h->tp || !h->tp->have_hist) { g_err = "rtg_temporal_history: no history yet"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(rgb_len, h->tp->hist[h->tp->cur].p, h->tp->n * sizeof(float4), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_temporal_copy_device(rtg_handle* h, void* dst_device) {
    const bool have = h && h->tp && h->tp->have_result;
    return copy_result("rtg_temporal_copy_device", h, have ? h->tp->out.p : nullptr, dst_device);
}

int rtg_temporal_reset(rtg_handle* h) {
    if (!h) { g_err = "rtg_temporal_reset: null handle"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    temporal_release(h);
    return RTG_OK;
}

int rtg_temporal_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms) {
    if (!h) { g_err = "rtg_temporal_ms: null handle"; return RTG_ERR_ARG; }
    if (guide_ms) *guide_ms = h->tp ? h->tp->guide_ms : 0.0;
    if (accumulate_ms) *accumulate_ms = h->tp ? h->tp->accumulate_ms : 0.0;
    return RTG_OK;
}

}  // extern "C"
