// rtg_gbuffer.hip — the fused first-hit pass behind the C-ABI (include/rtg.h: rtg_gbuffer, rtg_gbuffer_ms;
// DESIGN.md §8k): the geometry guide (rtg_temporal.hip, k_geometry_guide) and the denoiser's albedo and
// shading-normal guides (rtg_denoise.hip: two 1-sample renders of RTG_INTEGRATOR_ALBEDO and
// RTG_INTEGRATOR_NORMALS, then k_dn_pack_guide) from one traversal of the camera rays.
//
// Both guide integrators stop at the first hit and draw no random number, so all three outputs are functions
// of the pixel's (t, triangle, alpha, beta) record, which the geometry pass already holds. k_gbuffer reads that
// record once and writes what the three passes would have written, bit for bit: the geometry half in
// k_geometry_guide's operation order, the albedo and the normal in rtg_shade_body.h's (the ALT branches of
// RTG_INTEGRATOR_ALBEDO and RTG_INTEGRATOR_NORMALS) with rtg_dev.h's helpers, and `0 + c` where the renders
// add c to a zeroed film. IEEE float32 without contraction.
//
// Data per pixel: read hits and ray_d (2 x 16 B), the DevTri48 record (48 B), the shading record (64 B), the
// material (64 B) and at most one bilinear texel or environment lookup; written two 16-B geometry records, two
// planar 12-B images and the denoiser's two 16-B packed records (88 B). One thread per pixel of the pixel
// list; no LDS, no atomics.
#include "rtg_filter_state.h"

__global__ __launch_bounds__(256) void k_gbuffer(SceneView s, const unsigned* __restrict__ pixlist, unsigned npix,
                                                 const float4* __restrict__ hits, const float4* __restrict__ ray_d,
                                                 float ox, float oy, float oz, float4* __restrict__ geo,
                                                 float* __restrict__ albedo, float* __restrict__ normal,
                                                 float4* __restrict__ guide) {
    const unsigned lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= npix) return;
    const unsigned pixel = pixlist[lp];
    const float4 h = hits[lp];
    const float4 d4 = ray_d[lp];
    const v3 d = mk(d4.x, d4.y, d4.z);
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, RTG_FLT_MAX);
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    v3 c = mk(0.0f, 0.0f, 0.0f);   // the albedo integrator's value
    v3 nv = mk(0.0f, 0.0f, 0.0f);  // the normal integrator's: black on a miss
    if (h.x < RTG_FLT_MAX) {
        const float t = h.x;
        const int id = __float_as_int(h.y);
        {  // k_geometry_guide
            const DevTri48 T = s.tris48[id];
            const v3 v0 = mk(T.a.w, T.b.x, T.b.y), v1 = mk(T.b.z, T.b.w, T.c.x), v2 = mk(T.c.y, T.c.z, T.c.w);
            const v3 e1 = mk(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z), e2 = mk(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
            const float cx = e1.y * e2.z - e1.z * e2.y;
            const float cy = e1.z * e2.x - e1.x * e2.z;
            const float cz = e1.x * e2.y - e1.y * e2.x;
            const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
            g0 = make_float4(ox + d.x * t, oy + d.y * t, oz + d.z * t, t);  // Ray::at
            g1 = make_float4(cx / l, cy / l, cz / l, __int_as_float(id));
        }
        // rtg_shade_body.h, bounce 0 of a hit
        const DevShade S = s.shade[id];
        const float alpha = h.z, beta = h.w, gamma = 1.0f - (alpha + beta);
        const DevMat& M = s.mats[__float_as_int(S.d.w)];
        const v3 n0 = mk(S.a.x, S.a.y, S.a.z), n1 = mk(S.a.w, S.b.x, S.b.y), n2 = mk(S.b.z, S.b.w, S.c.x);
        v3 sn = normalize(add(add(muls(n0, alpha), muls(n1, beta)), muls(n2, gamma)));
        const float tu = (S.c.y * alpha + S.c.w * beta) + S.d.y * gamma;
        const float tv = (S.c.z * alpha + S.d.x * beta) + S.d.z * gamma;
        const v3 wo = neg(d);
        if (M.two_sided && dot(wo, sn) < 0) sn = neg(sn);
        nv = mk(fabsf(sn.x), fabsf(sn.y), fabsf(sn.z));  // viewNormals (Renderer.h:572-582)
        if (M.is_light) {
            c = mk(M.emission.x, M.emission.y, M.emission.z);  // emit()
        } else {  // BSDF::evaluate(sd, (0,1,0))
            const v3 alb = tex_sample(s, M, tu, tv);
            c = M.kind == RTG_MAT_MIRROR ? alb : (M.kind == RTG_MAT_GLASS ? mk(0.0f, 0.0f, 0.0f) : divs_pi(alb));
        }
    } else if (s.env_tex >= 0) {
        c = env_eval(s, d);  // background->evaluate(r.dir) (Renderer.h:390)
    }
    // what k_accumulate leaves in a zeroed film
    const float ar = 0.0f + c.x, ag = 0.0f + c.y, ab = 0.0f + c.z;
    const float nx = 0.0f + nv.x, ny = 0.0f + nv.y, nz = 0.0f + nv.z;
    const size_t p = (size_t)pixel;
    geo[2 * p] = g0;
    geo[2 * p + 1] = g1;
    albedo[3 * p] = ar;
    albedo[3 * p + 1] = ag;
    albedo[3 * p + 2] = ab;
    normal[3 * p] = nx;
    normal[3 * p + 1] = ny;
    normal[3 * p + 2] = nz;
    // k_dn_pack_guide
    const float z = (((nx * nx + ny * ny) + nz * nz) == 0.0f) ? 1.0f : 0.0f;
    guide[2 * p] = make_float4(ar, ag, ab, z);
    guide[2 * p + 1] = make_float4(nx, ny, nz, 0.0f);
}

// ------------------------------------------------------------------ host side
int launch_gbuffer(rtg_handle* h, const PathBufs& pb, float4* geo, DenoiseState& d, hipStream_t st) {
    const unsigned npix = h->npix;
    hipLaunchKernelGGL(k_gbuffer, dim3((npix + 255) / 256), dim3(256), 0, st, h->sv, (const unsigned*)h->d_pix, npix,
                       (const float4*)pb.hits, (const float4*)pb.ray_d, h->cam.ox, h->cam.oy, h->cam.oz, geo, d.albedo.p,
                       d.normal.p, d.guide.p);
    LAUNCH_OK("k_gbuffer");
    return RTG_OK;
}

extern "C" {

int rtg_gbuffer(rtg_handle* h, float* pos_t, float* normal_id, float* albedo, float* shading_normal) {
    if (!h) { g_err = "rtg_gbuffer: null handle"; return RTG_ERR_ARG; }
    if (int rc = settle(h)) return rc;  // slot 0's buffers are free
    if (int rc = temporal_state("rtg_gbuffer", h)) return rc;
    if (int rc = denoise_state(h)) return rc;
    TemporalState& t = *h->tp;
    const float4* g = nullptr;
    bool traced = false;
    HIPOK(hipEventRecord(t.ev[0], h->stream));
    if (int rc = current_guide(h, true, &g, &traced)) return rc;
    HIPOK(hipEventRecord(t.ev[1], h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    t.gbuffer_ms = stage_ms(traced, t.ev[0], t.ev[1]);
    if (int rc = download_guide(h, g, pos_t, normal_id)) return rc;
    if (albedo)
        if (int rc = h->dn->albedo.download(albedo, 3 * t.n)) return rc;
    if (shading_normal)
        if (int rc = h->dn->normal.download(shading_normal, 3 * t.n)) return rc;
    return RTG_OK;
}

int rtg_gbuffer_ms(rtg_handle* h, double* ms) {
    if (!h) { g_err = "rtg_gbuffer_ms: null handle"; return RTG_ERR_ARG; }
    if (ms) *ms = h->tp ? h->tp->gbuffer_ms : 0.0;
    return RTG_OK;
}

}  // extern "C"
