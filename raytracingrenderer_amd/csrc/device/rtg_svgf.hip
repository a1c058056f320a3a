// rtg_svgf.hip — variance-guided filtering of the temporal history behind the C-ABI (include/rtg.h,
// rtg_svgf_*; tests/svgf_ref.py restates it in numpy).
//
// Spatiotemporal variance-guided filtering (Schied et al. 2017) on what the two older units already keep on
// the device: rtg_temporal.hip's history {rgb, len}, its camera and geometry guides, and rtg_denoise.hip's
// albedo / shading-normal guides. One call advances the history exactly as rtg_temporal_accumulate does and
// carries the first two luminance moments along the same taps (k_svgf_temporal), turns them into a per-pixel
// variance, estimated over a 7 x 7 window where the history is short (k_svgf_variance), and runs K a-trous
// levels whose luminance term is scaled by that variance, filtered along with the colour (k_svgf_atrous).
// Only + - * /, floorf and comparisons in IEEE float32 without contraction, taps in (dy, dx) order: pinned bit
// for bit against the restatement.
//
// Data layout: the colour ping-pong holds one 16-B record per pixel {rgb, v}; the moments one 8-B record;
// the denoiser's guide is {albedo rgb, background flag} {normal xyz, pad}, the geometry guide {X.xyz, t}
// {Ng.xyz, triangle id}, and its {X, t} halves are copied into a 16-B stream once per call (read from the
// 32-B records each 128-B line would carry 64 B of normals along: the level measured 14 % slower). A filter
// tap costs four loads (colour, the denoiser's two, the position), the centre five, and the 3 x 3 variance
// prefilter nine 4-B ones. Blocks are 64 x 4 pixels with a wave on 64 consecutive x of one row, as
// k_dn_atrous lays them out: every tap of a wave is a contiguous row segment at any step and the row tests
// are wave-uniform. Direct reads (k_dn_atrous's LDS-staged variant measured slower). No
// atomics; no address depends on a colour.
#include "rtg_reproject.h"

#include <cmath>
#include <cstring>

struct SvgfTemporalArgs {
    const float* film;     // the film's sums, 3 floats per pixel
    float m;               // (float)spp
    int mode;              // 0: no history; 1: camera unchanged (identity); 2: camera moved (reprojection)
    int mom_on;            // M belongs to the history read
    const float4* hin;     // history read (modes 1 and 2)
    float4* hout;          // history written
    const float2* mom_in;  // moments read (mom_on)
    float2* mom_out;       // moments written
    const float4* gcur;    // the current camera's guide (mode 2)
    const float4* ghist;   // the history camera's guide (mode 2)
    int W, H;
    float max_history, plane_tolerance, normal_cos;
    TemporalProj cam;      // mode 2
};

struct SvgfVarianceArgs {
    const float4* hist;    // the new history
    const float2* mom;     // the new moments
    const float4* geo;     // the current geometry guide
    float4* col;           // {rgb, v}
    float* var;            // v
    int W, H;
    float min_history, plane_tolerance, normal_cos;
};

struct SvgfFilterArgs {
    const float4* cin;     // {rgb, v} of this level's input
    float4* cout;          // ... and output
    const float4* guide;   // the denoiser's guide, two float4 per pixel
    const float4* geo;     // the current geometry guide, two float4 per pixel (the centre's normal)
    const float4* xpos;    // its {X.xyz, t} halves, one float4 per pixel (the taps)
    int W, H, step, m;
    int alb_on;
    float s2, floor, ia;   // sigma_luminance^2, variance_floor, 1 / sigma_albedo^2
    float plane_tolerance;
};

static __device__ __forceinline__ float sv_lum(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

// k_temporal's definition for rgb and len, with the two moments carried over the same admitted taps
__global__ __launch_bounds__(256) void k_svgf_temporal(SvgfTemporalArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float cr = a.film[3 * p] / a.m, cg = a.film[3 * p + 1] / a.m, cb = a.film[3 * p + 2] / a.m;
    const float l = sv_lum(cr, cg, cb);
    const float s = l * l;
    bool have = false;
    float4 hist = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 hm = make_float2(0.0f, 0.0f);
    if (a.mode == 1) {
        hist = a.hin[p];
        if (a.mom_on) hm = a.mom_in[p];
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
            float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, al = 0.0f, a1 = 0.0f, a2 = 0.0f;
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
                    if (a.mom_on) {
                        const float2 mq = a.mom_in[q];
                        a1 = a1 + w * mq.x;
                        a2 = a2 + w * mq.y;
                    }
                }
            }
            if (sw > 0.0f) {
                hist = make_float4(ar / sw, ag / sw, ab / sw, al / sw);
                hm = make_float2(a1 / sw, a2 / sw);
                have = true;
            }
        }
    }
    float4 o = make_float4(cr, cg, cb, a.m);
    float2 mo = make_float2(l, s);
    if (have) {
        const float n = hist.w < a.max_history ? hist.w : a.max_history;
        const float al = a.m / (n + a.m);
        o = make_float4(hist.x + (cr - hist.x) * al, hist.y + (cg - hist.y) * al, hist.z + (cb - hist.z) * al, n + a.m);
        if (a.mom_on) mo = make_float2(hm.x + (l - hm.x) * al, hm.y + (s - hm.y) * al);
    }
    a.hout[p] = o;
    a.mom_out[p] = mo;
}

// the variance fed to level 0: temporal where the history is long enough, else spatial over 7 x 7
__global__ __launch_bounds__(256) void k_svgf_variance(SvgfVarianceArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 hp = a.hist[p];
    const float2 mp = a.mom[p];
    float v;
    if (hp.w >= a.min_history) {
        const float vt = mp.y - mp.x * mp.x;
        v = vt > 0.0f ? vt : 0.0f;
    } else {
        const float4 g0 = a.geo[2 * p], g1 = a.geo[2 * p + 1];
        const bool hit_p = __float_as_int(g1.w) >= 0;
        const float tol = a.plane_tolerance * g0.w;
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
#pragma unroll 1
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= a.H) continue;
            const size_t row = (size_t)qy * (size_t)a.W;
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= a.W) continue;
                const size_t q = row + (size_t)qx;
                if (dy != 0 || dx != 0) {
                    const float4 q1 = a.geo[2 * q + 1];
                    const bool hit_q = __float_as_int(q1.w) >= 0;
                    if (hit_p != hit_q) continue;
                    if (hit_p) {
                        const float4 q0 = a.geo[2 * q];
                        const float pd = rp_dot(q0.x - g0.x, q0.y - g0.y, q0.z - g0.z, g1.x, g1.y, g1.z);
                        if (!(fabsf(pd) <= tol)) continue;
                        const float nd = rp_dot(q1.x, q1.y, q1.z, g1.x, g1.y, g1.z);
                        if (!(fabsf(nd) >= a.normal_cos)) continue;
                    }
                }
                const float2 mq = a.mom[q];
                c0 = c0 + 1.0f;
                c1 = c1 + mq.x;
                c2 = c2 + mq.y;
            }
        }
        const float e1 = c1 / c0;
        const float vs = c2 / c0 - e1 * e1;
        v = (vs > 0.0f ? vs : 0.0f) * (a.min_history / hp.w);
    }
    a.col[p] = make_float4(hp.x, hp.y, hp.z, v);
    a.var[p] = v;
}

struct sv_f3 { float x, y, z; };

// The guide's position halves, packed: a tap needs {X, t} of its pixel only, and read from the 32-B guide
// records every 128-B line would carry 64 B of normals and ids along.
__global__ __launch_bounds__(256) void k_svgf_pack_pos(const float4* __restrict__ geo, size_t n, float4* __restrict__ xpos) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    xpos[i] = geo[2 * i];
}

static __device__ __forceinline__ float sv_tap(int d) {  // dn_tap's B3 weights
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

// One a-trous level. Direct reads: every tap comes from global memory (L1 / L2 serve the reuse). The kernel
// is all vector-memory requests and hides them behind other waves, so it asks for 8 waves per SIMD (<= 64
// VGPRs): pixel indices stay 32-bit (at most 2^28 pixels, widened at each load) and the centre's colour is not
// held across the taps; with 64-bit indices held the allocator needed 65-67 and spilled under the bound.
__global__ __launch_bounds__(256, 8) void k_svgf_atrous(SvgfFilterArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const unsigned p = (unsigned)y * (unsigned)a.W + (unsigned)x;
    // the variance around p, 3 x 3 at step 1 with clamped coordinates
    float gv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = min(max(y + dy, 0), a.H - 1);
        const float ky = dy == 0 ? 0.5f : 0.25f;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = min(max(x + dx, 0), a.W - 1);
            const float kx = dx == 0 ? 0.5f : 0.25f;
            gv = gv + (ky * kx) * a.cin[(unsigned)qy * (unsigned)a.W + (unsigned)qx].w;
        }
    }
    const float il = 1.0f / (a.s2 * gv + a.floor);
    const float4 gp0 = a.guide[2 * (size_t)p], gp1 = a.guide[2 * (size_t)p + 1];
    const float4 xp = a.xpos[p], np = a.geo[2 * (size_t)p + 1];
    const bool hit_p = __float_as_int(np.w) >= 0;
    const float tol = a.plane_tolerance * xp.w;
    float lp;
    {
        const float4 cp = a.cin[p];
        lp = sv_lum(cp.x, cp.y, cp.z);
    }
    float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.H) continue;  // the same for the whole wave (one row)
        const float hy = sv_tap(dy);
        const unsigned row = (unsigned)qy * (unsigned)a.W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.W) continue;
            const unsigned q = row + (unsigned)qx;
            const float4 cq = a.cin[q], gq0 = a.guide[2 * (size_t)q], xq = a.xpos[q];
            const sv_f3 gq1 = *reinterpret_cast<const sv_f3*>(&a.guide[2 * (size_t)q + 1]);  // the pad is not loaded
            float w = hy * sv_tap(dx);
            const float dl = sv_lum(cq.x, cq.y, cq.z) - lp;
            float t = 1.0f - (dl * dl) * il;
            t = t > 0.0f ? t : 0.0f;
            w = w * (t * t);
            if (a.alb_on) {
                const float ex = gq0.x - gp0.x, ey = gq0.y - gp0.y, ez = gq0.z - gp0.z;
                const float dd = (ex * ex + ey * ey) + ez * ez;
                float u = 1.0f - dd * a.ia;
                u = u > 0.0f ? u : 0.0f;
                w = w * (u * u);
            }
            float nd = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
            nd = nd > 0.0f ? nd : 0.0f;
            nd = nd < 1.0f ? nd : 1.0f;
            for (int k = 0; k < a.m; ++k) nd = nd * nd;
            if (gp0.w != 0.0f && gq0.w != 0.0f) nd = 1.0f;
            w = w * nd;
            {
                // a miss carries t = FLT_MAX in the guide: the hit flag of q without its second record. Selects,
                // not branches: a lane that fails the test keeps the wave's pace
                const bool hit_q = xq.w < RTG_FLT_MAX;
                const float pd = rp_dot(xq.x - xp.x, xq.y - xp.y, xq.z - xp.z, np.x, np.y, np.z);
                const bool pass = (dy == 0 && dx == 0) || (hit_p == hit_q && (!hit_p || fabsf(pd) <= tol));
                w = pass ? w : 0.0f;
            }
            sw = sw + w;
            ar = ar + w * cq.x;
            ag = ag + w * cq.y;
            ab = ab + w * cq.z;
            av = av + (w * w) * cq.w;
        }
    }
    // the centre's record, read again
    float4 o = a.cin[p];
    if (sw > 0.0f) o = make_float4(ar / sw, ag / sw, ab / sw, av / (sw * sw));
    a.cout[p] = o;
}

__global__ __launch_bounds__(256) void k_svgf_unpack(const float4* __restrict__ col, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    out[3 * i] = c.x;
    out[3 * i + 1] = c.y;
    out[3 * i + 2] = c.z;
}

// ------------------------------------------------------------------ host side
int svgf_alloc(SvgfState& s, size_t n) {
    if (int rc = s.ev.create()) return rc;
    for (DevBuf<float2>& b : s.mom)
        if (int rc = b.alloc(n)) return rc;
    for (DevBuf<float4>* b : {&s.col[0], &s.col[1], &s.xpos})
        if (int rc = b->alloc(n)) return rc;
    if (int rc = s.var.alloc(n)) return rc;
    return s.out.alloc(3 * n);
}

// The temporal state's variance-guided part, built on first use: a local one, handed to t by the last statement
// (a failed allocation leaves t.sv null and the next call builds again). t's destructor frees it.
static int build_state(TemporalState& t) {
    if (t.sv) return RTG_OK;
    auto s = std::make_unique<SvgfState>();
    if (int rc = svgf_alloc(*s, t.n)) return rc;
    t.sv = std::move(s);
    return RTG_OK;
}

int svgf_check(const char* who, const rtg_svgf_params* p) {
    auto bad = [&](const char* what) {
        g_err = std::string(who) + ": " + what;
        return RTG_ERR_ARG;
    };
    if (!p) return bad("null parameters");
    if (int rc = temporal_check(who, &p->temporal)) return rc;
    if (p->iterations == 0 || p->iterations > RTG_DENOISE_MAX_ITERATIONS) return bad("iterations must be 1..8");
    if (p->normal_squarings > 8) return bad("normal_squarings must be 0..8");
    if (!(std::isfinite(p->sigma_luminance) && p->sigma_luminance > 0.0f)) return bad("sigma_luminance must be finite and > 0");
    if (!(p->sigma_albedo <= 0.0f) && !(std::isfinite(p->sigma_albedo) && p->sigma_albedo >= 1e-6f))
        return bad("sigma_albedo must be <= 0 (off) or finite and >= 1e-6");
    if (!(std::isfinite(p->min_history) && p->min_history > 0.0f)) return bad("min_history must be finite and > 0");
    if (!(std::isfinite(p->variance_floor) && p->variance_floor > 0.0f)) return bad("variance_floor must be finite and > 0");
    return RTG_OK;
}

int svgf_queue(rtg_handle* h, const rtg_svgf_params* p, const HistoryTrack& k, SvgfState& s, const float* film,
               const float4* g, bool* unchanged) {
    hipStream_t st = h->stream;
    const size_t n = (size_t)h->W * h->H;
    const dim3 grid((unsigned)(h->W + 63) / 64, (unsigned)(h->H + 3) / 4);
    SvgfTemporalArgs a{};
    *unchanged = temporal_setup(h, k, p->temporal, a);
    a.film = film;
    a.mom_on = (k.have_hist && s.mom_valid) ? 1 : 0;
    a.mom_in = s.mom[s.cur].p;
    a.mom_out = s.mom[s.cur ^ 1].p;
    if (a.mode == 2) a.gcur = g;
    HIPOK(hipEventRecord(s.ev[2], st));
    hipLaunchKernelGGL(k_svgf_temporal, grid, dim3(256), 0, st, a);
    LAUNCH_OK("k_svgf_temporal");
    HIPOK(hipEventRecord(s.ev[3], st));

    SvgfVarianceArgs v{};
    v.hist = a.hout;
    v.mom = a.mom_out;
    v.geo = g;
    v.col = s.col[0].p;
    v.var = s.var.p;
    v.W = h->W;
    v.H = h->H;
    v.min_history = p->min_history;
    v.plane_tolerance = p->temporal.plane_tolerance;
    v.normal_cos = p->temporal.normal_cos;
    hipLaunchKernelGGL(k_svgf_variance, grid, dim3(256), 0, st, v);
    LAUNCH_OK("k_svgf_variance");
    HIPOK(hipEventRecord(s.ev[4], st));

    hipLaunchKernelGGL(k_svgf_pack_pos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, n, s.xpos.p);
    LAUNCH_OK("k_svgf_pack_pos");
    SvgfFilterArgs f{};
    f.guide = h->dn->guide.p;
    f.geo = g;
    f.xpos = s.xpos.p;
    f.W = h->W;
    f.H = h->H;
    f.m = (int)p->normal_squarings;
    f.alb_on = p->sigma_albedo > 0.0f;
    f.s2 = p->sigma_luminance * p->sigma_luminance;
    f.floor = p->variance_floor;
    f.ia = f.alb_on ? 1.0f / (p->sigma_albedo * p->sigma_albedo) : 0.0f;
    f.plane_tolerance = p->temporal.plane_tolerance;
    for (uint32_t i = 0; i < p->iterations; ++i) {
        f.cin = s.col[i & 1].p;
        f.cout = s.col[(i + 1) & 1].p;
        f.step = 1 << i;
        hipLaunchKernelGGL(k_svgf_atrous, grid, dim3(256), 0, st, f);
        LAUNCH_OK("k_svgf_atrous");
    }
    HIPOK(hipEventRecord(s.ev[5], st));
    return RTG_OK;
}

void svgf_done(SvgfState& s, bool traced) {
    float ms = 0.0f;
    s.guide_ms = stage_ms(traced, s.ev[0], s.ev[1]);
    if (hipEventElapsedTime(&ms, s.ev[2], s.ev[3]) == hipSuccess) s.accumulate_ms = ms;
    if (hipEventElapsedTime(&ms, s.ev[3], s.ev[4]) == hipSuccess) s.variance_ms = ms;
    if (hipEventElapsedTime(&ms, s.ev[4], s.ev[5]) == hipSuccess) s.filter_ms = ms;
    s.cur ^= 1;
    s.mom_valid = true;
    s.have_result = true;
}

static SvgfState* result_state(const char* who, rtg_handle* h) {
    if (!h) { g_err = std::string(who) + ": null argument"; return nullptr; }
    if (!h->tp || !h->tp->sv || !h->tp->sv->have_result) { g_err = std::string(who) + ": no result yet"; return nullptr; }
    return h->tp->sv.get();
}

extern "C" {

int rtg_svgf_defaults(rtg_svgf_params* p) {
    if (!p) { g_err = "rtg_svgf_defaults: null argument"; return RTG_ERR_ARG; }
    (void)rtg_temporal_defaults(&p->temporal);
    p->iterations = 5;
    p->normal_squarings = 5;
    p->sigma_luminance = 4.0f;
    p->sigma_albedo = 0.1f;
    p->min_history = 4.0f;
    p->variance_floor = 1e-8f;
    return RTG_OK;
}

int rtg_svgf_check(const rtg_svgf_params* p) { return svgf_check("rtg_svgf_check", p); }

int rtg_svgf_accumulate(rtg_handle* h, const rtg_svgf_params* p, float* out) {
    if (!h) { g_err = "rtg_svgf_accumulate: null handle"; return RTG_ERR_ARG; }
    if (int rc = svgf_check("rtg_svgf_accumulate", p)) return rc;
    if (h->spp == 0) { g_err = "rtg_svgf_accumulate: the film holds no samples (spp == 0)"; return RTG_ERR_ARG; }
    if (int rc = settle(h)) return rc;  // the film holds every queued frame, and slot 0's buffers are free
    if (int rc = temporal_state("rtg_svgf_accumulate", h)) return rc;
    TemporalState& t = *h->tp;
    if (int rc = build_state(t)) return rc;
    if (int rc = denoise_state(h)) return rc;
    SvgfState& s = *t.sv;
    hipStream_t st = h->stream;
    const float4* g = nullptr;  // the current geometry guide: the history's own when the camera is its camera
    bool traced = false, unchanged = false;
    HIPOK(hipEventRecord(s.ev[0], st));
    // one fused first-hit pass for the geometry guide and the denoiser's guides (nothing when both are at hand);
    // it renders nothing, so the statistics have nothing to be put back
    if (int rc = current_guide(h, true, &g, &traced)) return rc;
    HIPOK(hipEventRecord(s.ev[1], st));
    if (int rc = svgf_queue(h, p, t, s, h->d_film, g, &unchanged)) return rc;
    hipLaunchKernelGGL(k_svgf_unpack, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, st,
                       (const float4*)s.col[p->iterations & 1].p, t.n, s.out.p);
    LAUNCH_OK("k_svgf_unpack");
    if (out) HIPOK(hipMemcpyAsync(out, s.out.p, t.n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    svgf_done(s, traced);
    t.gbuffer_ms = s.guide_ms;
    temporal_advance(h, unchanged, g);
    return RTG_OK;
}

int rtg_svgf_variance(rtg_handle* h, float* var) {
    SvgfState* s = result_state("rtg_svgf_variance", var ? h : nullptr);
    if (!s) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(var, s->var.p, h->tp->n * sizeof(float), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_svgf_moments(rtg_handle* h, float* mu) {
    SvgfState* s = result_state("rtg_svgf_moments", mu ? h : nullptr);
    if (!s) return RTG_ERR_ARG;
    if (!s->mom_valid) { g_err = "rtg_svgf_moments: the moments were dropped by rtg_temporal_accumulate"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    HIPOK(hipMemcpy(mu, s->mom[s->cur].p, h->tp->n * sizeof(float2), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_svgf_copy_device(rtg_handle* h, void* dst_device) {
    const bool have = h && h->tp && h->tp->sv && h->tp->sv->have_result;
    return copy_result("rtg_svgf_copy_device", h, have ? h->tp->sv->out.p : nullptr, dst_device);
}

int rtg_svgf_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms, double* variance_ms, double* filter_ms) {
    if (!h) { g_err = "rtg_svgf_ms: null handle"; return RTG_ERR_ARG; }
    const SvgfState* s = h->tp ? h->tp->sv.get() : nullptr;
    if (guide_ms) *guide_ms = s ? s->guide_ms : 0.0;
    if (accumulate_ms) *accumulate_ms = s ? s->accumulate_ms : 0.0;
    if (variance_ms) *variance_ms = s ? s->variance_ms : 0.0;
    if (filter_ms) *filter_ms = s ? s->filter_ms : 0.0;
    return RTG_OK;
}

}  // extern "C"
