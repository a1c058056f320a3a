// rtg_api.hip — the handle and the plumbing of include/rtg.h's C-ABI: error text and build id, scene
// upload (the records rtg_scene.hip prepares), create / destroy / settings, the film and the stats,
// and the device-code probes of the test suite. Rendering is rtg_render.hip, traversal rtg_trace.hip.
#include "rtg_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

thread_local std::string g_err;

// ------------------------------------------------------------------ test probes
// BSDF probe: the exact device BSDF code on scripted inputs (unit parity vs RTBase's BSDF classes).
// in: 20 floats per case = kind, int_ior, ext_ior, albedo.rgb (1x1 texture), sN.xyz, wo.xyz, tu, tv,
//     draws[4], pad[2]; out: 11 floats = wi.xyz, refl.rgb, pdf, draws used, evaluate.rgb
__global__ void k_probe_bsdf(const float* in, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = in + (size_t)i * 20;
    const int kind = (int)c[0];
    const v3 alb = bilinear(Texels3{c + 3}, 1, 1, c[12], c[13]);  // albedo->sample(tu, tv)
    const frame fr = frame_from(mk(c[6], c[7], c[8]));
    const v3 wo = mk(c[9], c[10], c[11]);
    ScriptSampler smp{c + 14, 4, 0};
    v3 refl;
    float pdf;
    const v3 wi = bsdf_sample(kind, c[1], c[2], alb, fr, wo, smp, refl, pdf);
    const v3 ev = kind <= 1 ? divs_pi(alb) : (kind == 2 ? alb : mk(0.0f, 0.0f, 0.0f));
    float* o = out + (size_t)i * 11;
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z;
    o[3] = refl.x; o[4] = refl.y; o[5] = refl.z;
    o[6] = pdf;
    o[7] = (float)smp.i;
    o[8] = ev.x; o[9] = ev.y; o[10] = ev.z;
}

// Texture probe: k_shade's own bilinear<Texels4> (Texture::sample, as tex_sample calls it) and
// env_lookup (EnvironmentMap::evaluate, env_eval's body) on a texture in the device layout.
// env 0: in = (tu, tv) per case; env 1: in = dir.xyz per case. uni: the "uniform texture" short-cut
// (every tap is the first texel, held by the caller: DevMat::texel0 / SceneView::env_one).
__global__ void k_probe_texture(int env, int uni, const float4* texels, int w, int h, const float* in, int n,
                                float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 t0 = texels[0];
    const v3 one = mk(t0.x, t0.y, t0.z);
    const Texels4 tx{texels};
    const v3 r = env ? env_lookup(tx, w, h, mk(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]),
                                  uni != 0, one)
                     : bilinear(tx, w, h, in[2 * (size_t)i], in[2 * (size_t)i + 1], uni != 0, one);
    float* o = out + (size_t)i * 3;
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
}

// Transcendental probe: the device's include/rtg_math.h on given inputs (parity vs the host glibc).
// fn 0 sinf, 1 cosf, 2 sincosf (out: sin, cos per input), 3 acosf, 4 atan2f (in: y, x per input).
__global__ void k_probe_math(int fn, const float* in, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (fn) {
    case 0: out[i] = rtm_sinf(in[i]); break;
    case 1: out[i] = rtm_cosf(in[i]); break;
    case 2: rtm_sincosf(in[i], &out[2 * (size_t)i], &out[2 * (size_t)i + 1]); break;
    case 3: out[i] = rtm_acosf(in[i]); break;
    default: out[i] = rtm_atan2f(in[2 * (size_t)i], in[2 * (size_t)i + 1]); break;
    }
}

// The device half: upload the prepared records to `device`, allocate the film, size the launches.
int upload_scene(int device, const HostScene& hs, rtg_handle* h) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_err = "no HIP device available";
        return RTG_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return RTG_ERR_ARG; }
    h->device = device;
    HIPOK(hipSetDevice(device));
    HIPOK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIPOK(hipGetDeviceProperties(&prop, device));
    h->n_cu = prop.multiProcessorCount;
    h->bvh_depth = hs.bvh_depth;
    h->wide_depth = hs.wide_depth;
    h->rebuilt = hs.rebuilt;
    h->usew = hs.usew;
    int rc;
    SceneBufs& d = h->scene;
    if ((rc = d.nodes.upload(hs.nodes))) return rc;
    if ((rc = d.nodesq.upload(hs.nodesq))) return rc;
    if ((rc = d.leafbox.upload(hs.leafbox))) return rc;
    if (!hs.img.empty() && (rc = d.img.upload(hs.img))) return rc;
    if ((rc = d.tris48.upload(hs.tris48))) return rc;
    if ((rc = d.shade.upload(hs.shade))) return rc;
    if ((rc = d.mats.upload(hs.mats))) return rc;
    if ((rc = d.lights.upload(hs.lights))) return rc;
    if ((rc = d.texinfo.upload(hs.texinfo))) return rc;
    if ((rc = d.texels.upload(hs.texels))) return rc;

    SceneView& s = h->sv;
    s.nodes = d.nodes.p;
    s.tris48 = d.tris48.p;
    s.shade = d.shade.p;
    s.mats = d.mats.p;
    s.lights = d.lights.p;
    s.texinfo = d.texinfo.p;
    s.texels = (const float4*)d.texels.p;
    s.n_mats = (int)hs.mats.size();
    s.n_lights = hs.n_lights;
    s.pmf = 1.f / (float)hs.n_lights;  // Scene::sampleLight (Scene.h:137-138), the same IEEE division
    s.env_tex = hs.env_tex;
    s.env_off = hs.env_off;
    s.env_w = hs.env_w;
    s.env_h = hs.env_h;
    s.env_uniform = hs.env_uniform ? 1 : 0;
    for (int k = 0; k < 3; ++k) s.env_one[k] = hs.env_one[k];
    s.root_word = hs.root_word;
    s.nodesq = d.nodesq.p;
    s.leafbox = d.leafbox.p;
    s.root_wordw = hs.root_wordw;
    s.usew = hs.usew ? 1 : 0;
    s.img = d.img.p;
    s.img_n4 = (int)hs.img.size();
    s.img_tri = hs.img_tri;
    s.img_lb = hs.img_lb;
    for (int k = 0; k < 6; ++k) s.root_box[k] = hs.root_box[k];
    s.cull_scale = hs.cull_scale;
    for (const DevLight& L : hs.lights) {  // v1t.w: the light's type bits, 1 = the environment light
        int type;
        std::memcpy(&type, &L.v1t.w, 4);
        h->env_light = h->env_light || type == 1;
    }
    h->cam = hs.cam;
    h->proj = hs.proj;
    h->tri_mat = hs.tri_mat;
    h->n_desc_mats = hs.n_desc_mats;
    h->light_tri = hs.light_tri;
    h->W = (int)hs.cam.width;
    h->H = (int)hs.cam.height;
    HIPOK(hipMalloc((void**)&h->d_film, (size_t)h->W * h->H * 3 * sizeof(float)));
    HIPOK(hipMemset(h->d_film, 0, (size_t)h->W * h->H * 3 * sizeof(float)));
    HIPOK(hipMalloc((void**)&h->d_qctr, 4 * sizeof(unsigned)));
    HIPOK(hipMalloc((void**)&h->d_stats, RTG_NSTATS * sizeof(unsigned long long)));
    HIPOK(hipMemset(h->d_stats, 0, RTG_NSTATS * sizeof(unsigned long long)));
    for (auto& e : h->ev) HIPOK(hipEventCreate(&e));

    if ((rc = size_trace_grids(h))) return rc;
    HIPOK(hipEventCreateWithFlags(&h->entry, hipEventDisableTiming));
    return ensure_ovf(h, h->slot[0]);
}

int camera_check(const char* who, const rtg_handle* h, const rtg_camera* cam, const rtg_camera_proj* proj) {
    auto bad = [&](const char* what) {
        g_err = std::string(who) + ": " + what;
        return RTG_ERR_ARG;
    };
    if (!cam || !proj) return bad("both camera records are required");
    static_assert(sizeof(rtg_camera) == 37 * sizeof(float) && sizeof(rtg_camera_proj) == 36 * sizeof(float),
                  "the camera records are plain float arrays");
    const float* a = (const float*)cam;
    for (size_t k = 0; k < sizeof(rtg_camera) / sizeof(float); ++k)
        if (!std::isfinite(a[k])) return bad("a field of the camera record is not finite");
    const float* b = (const float*)proj;
    for (size_t k = 0; k < sizeof(rtg_camera_proj) / sizeof(float); ++k)
        if (!std::isfinite(b[k])) return bad("a field of the projection record is not finite");
    if (cam->width != (float)h->W || cam->height != (float)h->H) return bad("width and height must equal the handle's");
    return RTG_OK;
}

extern "C" {

int32_t rtg_abi_version(void) { return RTG_ABI_VERSION; }
#ifndef RTG_BUILD_ID
#define RTG_BUILD_ID "unknown"
#endif
// build.py passes the hash of the sources, headers and flags (source_hash("device")); the tagged
// copy lets the build find the id in the file without loading it
static const char k_build_tag[] __attribute__((used)) = "rtg-build-id:" RTG_BUILD_ID;
const char* rtg_build_id(void) { return k_build_tag + 13; }
const char* rtg_last_error(void) { return g_err.c_str(); }

int rtg_device_count(int* count) {
    if (!count) return RTG_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return RTG_OK;
}

int rtg_create(int device, const rtg_scene_desc* desc, rtg_handle** out) {
    if (!desc || !out) { g_err = "rtg_create: null argument"; return RTG_ERR_ARG; }
    rtg_handle* h = new rtg_handle();
    HostScene hs;
    int rc = prepare_scene(desc, hs);
    if (rc == RTG_OK) rc = upload_scene(device, hs, h);
    if (rc != RTG_OK) {
        rtg_destroy(h);
        return rc;
    }
    *out = h;
    return RTG_OK;
}

void rtg_destroy(rtg_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->pend_n = 0;  // queued calls not issued yet are dropped with the film
    if (h->stream) {
        (void)join_frames(h);
        (void)hipStreamSynchronize(h->stream);
    }
    for (ChunkSlot& sl : h->slot) {
        free_chunk(sl);
        (void)hipFree(sl.d_ovf);
        if (sl.fold) (void)hipEventDestroy(sl.fold);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
    }
    if (h->entry) (void)hipEventDestroy(h->entry);
    denoise_release(h);
    temporal_release(h);
    h->mt = ModeTables{};  // here, not in `delete h`: the device is the handle's and its streams still exist
    h->scene = SceneBufs{};
    (void)hipFree(h->d_film);
    (void)hipFree(h->d_pix); (void)hipFree(h->d_qctr); (void)hipFree(h->d_stats);
    for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->kev) (void)hipEventDestroy(e);
    for (auto& e : h->tev) (void)hipEventDestroy(e);
    if (h->h_cnt) (void)hipHostFree(h->h_cnt);
    (void)hipFree(h->d_cap); (void)hipFree(h->d_cap_len); (void)hipFree(h->d_cap_rays);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtg_set_integrator(rtg_handle* h, int integrator) {
    if (!h || integrator < RTG_INTEGRATOR_PATH || integrator > RTG_INTEGRATOR_DIRECT_MIS) {
        g_err = "rtg_set_integrator: bad argument";
        return RTG_ERR_ARG;
    }
    if (int rc = flush_pending(h)) return rc;  // queued calls render with the settings they were queued under
    h->integrator = integrator;
    return RTG_OK;
}

int rtg_set_camera(rtg_handle* h, const rtg_camera* cam, const rtg_camera_proj* proj) {
    if (!h) { g_err = "rtg_set_camera: null handle"; return RTG_ERR_ARG; }
    if (int rc = camera_check("rtg_set_camera", h, cam, proj)) return rc;
    if (int rc = settle(h)) return rc;
    std::memcpy(h->cam.ip, cam->inv_proj, sizeof(h->cam.ip));  // as prepare_scene takes them from the descriptor
    std::memcpy(h->cam.cm, cam->camera, sizeof(h->cam.cm));
    h->cam.ox = cam->origin[0];
    h->cam.oy = cam->origin[1];
    h->cam.oz = cam->origin[2];
    h->cam.width = cam->width;
    h->cam.height = cam->height;
    h->proj = *proj;
    denoise_drop_guides(h);
    return RTG_OK;
}

int rtg_get_camera(rtg_handle* h, rtg_camera* cam, rtg_camera_proj* proj) {
    if (!h) { g_err = "rtg_get_camera: null handle"; return RTG_ERR_ARG; }
    if (cam) {
        std::memcpy(cam->inv_proj, h->cam.ip, sizeof(h->cam.ip));
        std::memcpy(cam->camera, h->cam.cm, sizeof(h->cam.cm));
        cam->origin[0] = h->cam.ox;
        cam->origin[1] = h->cam.oy;
        cam->origin[2] = h->cam.oz;
        cam->width = h->cam.width;
        cam->height = h->cam.height;
    }
    if (proj) *proj = h->proj;
    return RTG_OK;
}

int rtg_set_options(rtg_handle* h, int max_depth, int cull, uint32_t max_paths) {
    if (!h || max_depth < 0 || max_depth > 250) { g_err = "rtg_set_options: bad argument"; return RTG_ERR_ARG; }
    if (int rc = flush_pending(h)) return rc;  // queued calls render with the settings they were queued under
    h->max_depth = max_depth;
    h->cull = cull & 1;
    h->count = (cull >> 1) & 1;   // bit 1: counting kernels (node/triangle tests)
    h->timing = (cull >> 2) & 1;  // bit 2: per-launch timing events
    h->wide = ((cull >> 3) & 1) ? 0 : 1;  // bit 3: force the reference BVH2 walk
    h->wavetime = RTG_DEBUG ? (cull >> 4) & 1 : 0;  // bit 4 (RTG_DEBUG builds): per-wave clocks
    h->serial = (cull >> 5) & 1;  // bit 5: no frame pipeline, read-back k_shade grids
    h->no_coalesce = (cull >> 6) & 1;  // bit 6: queued calls are issued one by one
    if (max_paths) h->max_paths = max_paths;
    return RTG_OK;
}

int rtg_synchronize(rtg_handle* h) {
    if (!h) return RTG_ERR_ARG;
    if (int rc = settle(h)) return rc;
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->stats.render_ms = ms;
    return RTG_OK;
}

int rtg_film_read(rtg_handle* h, float* rgb, uint32_t* spp) {
    if (!h) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    if (!rgb) {  // Film::SPP only: counts queued frames, waits for nothing
        if (spp) *spp = h->spp;
        return RTG_OK;
    }
    if (int rc = join_frames(h)) return rc;
    HIPOK(hipStreamSynchronize(h->stream));
    if (rgb) HIPOK(hipMemcpy(rgb, h->d_film, (size_t)h->W * h->H * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (spp) *spp = h->spp;
    return RTG_OK;
}

int rtg_film_copy_device(rtg_handle* h, void* dst) {
    if (!h || !dst) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;
    HIPOK(hipMemcpyAsync(dst, h->d_film, (size_t)h->W * h->H * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    return RTG_OK;
}

int rtg_film_load(rtg_handle* h, const float* rgb, uint32_t spp) {
    if (!h || !rgb) return RTG_ERR_ARG;
    if (int rc = settle(h)) return rc;
    HIPOK(hipMemcpy(h->d_film, rgb, (size_t)h->W * h->H * 3 * sizeof(float), hipMemcpyHostToDevice));
    h->spp = spp;
    return RTG_OK;
}

int rtg_clear(rtg_handle* h) {
    if (!h) return RTG_ERR_ARG;
    HIPOK(hipSetDevice(h->device));
    h->pend_n = 0;  // queued calls not issued yet: the clear would zero what they add
    if (int rc = join_frames(h)) return rc;
    HIPOK(hipMemsetAsync(h->d_film, 0, (size_t)h->W * h->H * 3 * sizeof(float), h->stream));
    HIPOK(hipMemsetAsync(h->d_stats, 0, RTG_NSTATS * sizeof(unsigned long long), h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    h->spp = 0;
    h->stats = rtg_stats{};
    return RTG_OK;
}

int rtg_get_stats(rtg_handle* h, rtg_stats* out) {
    if (!h || !out) return RTG_ERR_ARG;
    if (int rc = settle(h)) return rc;
    unsigned long long c[RTG_NSTATS] = {};
    HIPOK(hipMemcpy(c, h->d_stats, sizeof(c), hipMemcpyDeviceToHost));
    h->stats.node_visits = c[0];
    h->stats.tri_tests = c[1];
    h->stats.extension_rays = c[2];
    h->stats.shadow_rays = c[3];
    h->stats.shadow_node_visits = c[4];
    h->stats.shadow_tri_tests = c[5];
    h->stats.lane_slots = c[8];
    h->stats.node_lane_steps = c[9];
    h->stats.leaf_lane_steps = c[10];
    h->stats.leaf_phase_slots = c[13];
    h->stats.cullable_pops = c[11];
    h->stats.pops = c[12];
    h->stats.tri_tail_loads = c[6];
    h->stats.leafbox_tests = c[7];
    h->stats.traced_camera_rays = c[14];
    h->stats.lane_idle_no_ray = c[15];
    h->stats.lane_idle_last_leaf = c[16];
    h->stats.lane_idle_leaf_blocked = c[17];
    h->stats.lane_idle_retiring = c[18];
    h->stats.lane_idle_leaf_popped = c[19];
    *out = h->stats;
    return RTG_OK;
}

int rtg_probe_bsdf(const float* cases, uint32_t n, float* out) {
    if (!cases || !out) return RTG_ERR_ARG;
    if (n == 0) return RTG_OK;
    return probe_run({{cases, (size_t)n * 20 * sizeof(float)}}, {{out, (size_t)n * 11 * sizeof(float)}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_bsdf, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d[0], (int)n,
                           (float*)d[1]);
    });
}

int rtg_probe_texture(int mode, const float* texels_rgb, uint32_t w, uint32_t h, const float* in, uint32_t n,
                      float* out) {
    auto bad = [](const char* what) {
        g_err = std::string("rtg_probe_texture: ") + what;
        return RTG_ERR_ARG;
    };
    if (!texels_rgb || !in || !out) return bad("null argument");
    if (mode < 0 || mode > (RTG_PROBE_TEX_ENV | RTG_PROBE_TEX_UNIFORM)) return bad("unknown mode");
    if (w == 0 || h == 0 || w > 0xffffu || h > 0xffffu || (uint64_t)w * h > (1ull << 28))
        return bad("texture size must be 1..65535 per side and at most 2^28 texels");
    if (n > 0x7fffffffu / 3u) return bad("too many cases");
    const size_t nt = (size_t)w * h;
    const bool env = (mode & RTG_PROBE_TEX_ENV) != 0, uni = (mode & RTG_PROBE_TEX_UNIFORM) != 0;
    if (uni)  // the short-cut's precondition, as prepare_scene establishes it: every texel has the first one's bits
        for (size_t j = 1; j < nt; ++j)
            if (std::memcmp(texels_rgb + 3 * j, texels_rgb, 3 * sizeof(float)) != 0)
                return bad("RTG_PROBE_TEX_UNIFORM needs a texture whose texels all have the same bits");
    if (n == 0) return RTG_OK;
    std::vector<float> t4(nt * 4);  // RGB + pad: one 16-B load per texel, as prepare_scene uploads them
    for (size_t j = 0; j < nt; ++j) {
        t4[4 * j] = texels_rgb[3 * j];
        t4[4 * j + 1] = texels_rgb[3 * j + 1];
        t4[4 * j + 2] = texels_rgb[3 * j + 2];
        t4[4 * j + 3] = 0.0f;
    }
    const size_t nin = (size_t)n * (env ? 3 : 2), nout = (size_t)n * 3;
    return probe_run({{t4.data(), t4.size() * sizeof(float)}, {in, nin * sizeof(float)}}, {{out, nout * sizeof(float)}},
                     [&](void* const* d) {
                         hipLaunchKernelGGL(k_probe_texture, dim3((n + 255) / 256), dim3(256), 0, nullptr, env ? 1 : 0,
                                            uni ? 1 : 0, (const float4*)d[0], (int)w, (int)h, (const float*)d[1], (int)n,
                                            (float*)d[2]);
                     });
}

int rtg_probe_math(int fn, const float* in, uint32_t n, float* out) {
    if (!in || !out || fn < 0 || fn > 4 || n > 0x7fffffffu) return RTG_ERR_ARG;
    if (n == 0) return RTG_OK;
    const size_t nin = (size_t)n * (fn == 4 ? 2 : 1), nout = (size_t)n * (fn == 2 ? 2 : 1);
    return probe_run({{in, nin * sizeof(float)}}, {{out, nout * sizeof(float)}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_math, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, (const float*)d[0], (int)n,
                           (float*)d[1]);
    });
}

}  // extern "C"
