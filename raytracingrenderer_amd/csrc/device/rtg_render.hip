// rtg_render.hip — MI355X (gfx950) wavefront path tracer: its small kernels, the chunk scheduler and
// the render entry points of include/rtg.h (k_trace: rtg_trace.hip, k_shade: rtg_shade.hip).
//
// One RayTracer::render() (RTBase/Renderer.h:876) = one sample for every pixel. Here a "chunk" is
// ns samples x npix pixels = P paths in flight, advanced bounce by bounce:
//
//   k_generate        Camera::generateRay (Scene.h:43-54) at pixel centres, PCG32 seed, path state
//   for b in 0 .. max_depth+2:                                   (pathTrace recursion, depth = b)
//     k_shade (b > 0)  bounce b-1: calculateShadingData + emission + computeDirect (NEE sample,
//                      shadow ray) + Russian roulette + BSDF::sample + throughput
//                      (Renderer.h:328-392, 423-473) -> compacts continuing paths into the next
//                      extension queue and NEE rays into the shadow queue (one atomic per block)
//     k_trace          one launch for both ray kinds: Scene::traverse (Scene.h:107-130,
//                      Geometry.h:399-434) for the extension rays of bounce b and Scene::visible
//                      (Scene.h:161-169, Geometry.h:435-462) for the shadow rays of bounce b-1
//   k_accumulate      right-nested radiance sum d0 + (d1 + (... + dk)) (Renderer.h:388) per path,
//                      then film += L in sample order (Film::splat, Imaging.h:209-232)
//
// Exactness: each path's result is independent of queue order and of traversal order. Closest hit
// returns the (t, triangle index) lexicographic minimum over the reference's reachable triangles,
// which is what the reference's left-first DFS with strict '<' keeps; box tests use the reference's
// exact slab arithmetic, and distance culling only removes boxes whose conservatively inflated entry
// is beyond the current hit.
#include "rtg_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <thread>

// ------------------------------------------------------------------ generate
// lean (the path tracer): one thread per pixel. renderTile's camera ray goes through the pixel centre
// (Renderer.h:805-808: no jitter, a pinhole camera), so every sample of a pixel casts the same ray
// and finds the same first hit: the bounce-0 traversal traces one ray per pixel (ray_d[lp],
// hits[lp]) and k_shade's bounce 0 reads it for each of the pixel's samples. The rays counted in
// rtg_stats stay the reference's (one per sample); traced_camera_rays counts the traced ones.
// Otherwise (instant radiosity's camera pass, one sample): one thread per path, full path state.
__global__ __launch_bounds__(RTG_TB) void k_generate(ChunkArgs a, PathBufs p) {
    const unsigned pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (a.seg_tiles && pid < 8) {  // path tracer: the paths as queue segments (positions = path ids)
        const unsigned cap = a.seg_tiles * RTG_TB, lo = pid * cap;
        p.ctr[0].ne8[32 * pid] = a.P > lo ? min(cap, a.P - lo) : 0u;
    }
    if (a.seg_tiles && pid == 0) p.ctr[0].n_cam = a.npix;  // the bounce-0 traversal: a ray per pixel
    if (!a.seg_tiles && pid == 0) p.ctr[0].n_ext = a.P;  // instant radiosity's camera pass: one queue
    unsigned lp, sl;  // pixel-major path ids
    if (a.lean) {
        if (pid >= a.npix) return;
        lp = pid;
        sl = 0;
    } else {
        if (pid >= a.P) return;
        split_pid(a, pid, lp, sl);
    }
    const unsigned pixel = a.pixlist[lp];
    const unsigned W = (unsigned)a.cam.width;
    const unsigned x = pixel % W, y = pixel / W;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;  // renderTile: pixel centre
    // Camera::generateRay
    float xp = px / a.cam.width;
    float yp = 1.0f - (py / a.cam.height);
    xp = (xp * 2.0f) - 1.0f;
    yp = (yp * 2.0f) - 1.0f;
    const float* m = a.cam.ip;
    v3 dir = mk(((xp * m[0] + yp * m[1]) + 1.0f * m[2]) + m[3],
                ((xp * m[4] + yp * m[5]) + 1.0f * m[6]) + m[7],
                ((xp * m[8] + yp * m[9]) + 1.0f * m[10]) + m[11]);
    const float* c = a.cam.cm;
    dir = mk((dir.x * c[0] + dir.y * c[1]) + dir.z * c[2],
             (dir.x * c[4] + dir.y * c[5]) + dir.z * c[6],
             (dir.x * c[8] + dir.y * c[9]) + dir.z * c[10]);
    dir = normalize(dir);
    p.ray_d[pid] = make_float4(dir.x, dir.y, dir.z, 0.0f);  // (lean: pid = lp)
    if (a.lean) return;  // the rest is implied at bounce 0 (k_trace: io.cam_o / identity queue; k_shade)
    p.ray_o[pid] = make_float4(a.cam.ox, a.cam.oy, a.cam.oz, 0.0f);
    p.q[0][pid] = pid;
    p.thr[pid] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    p.rng[pid] = pcg_seed(a.seed, pcg_inc(pixel, a.s0 + sl));
    p.meta[pid] = 1 << 8;  // canHitLight = true
}

// rtg_set_camera_sampling with a filter or a lens: one thread per path, pixel-major (pid = lp * ns +
// sl, a wave is still one pixel's samples). Each sample has a camera ray of its own (camera_sample,
// rtg_dev.h) in ray_d[pid], and with a lens its origin in ray_o[pid] (the path id in .w, as later
// bounces carry it); the rest of the bounce-0 state stays implied, as in k_generate's lean branch.
// Bounce 0 is then a segmented queue of P rays at identity positions, like every later bounce.
template <bool SOBOL>
static __device__ __forceinline__ void generate_sampled(const ChunkArgs& a, const PathBufs& p, const CamSampling& cs) {
    const unsigned pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid < 8) {  // the paths as queue segments (positions = path ids), as k_generate
        const unsigned cap = a.seg_tiles * RTG_TB, lo = pid * cap;
        p.ctr[0].ne8[32 * pid] = a.P > lo ? min(cap, a.P - lo) : 0u;
    }
    if (pid == 0) p.ctr[0].n_cam = a.P;  // camera rays traced: one per path (k_tally, rtg_launch_rays)
    if (pid >= a.P) return;
    unsigned lp, sl;
    split_pid(a, pid, lp, sl);
    float fx, fy;
    v3 o, d;
    camera_sample<SOBOL>(a.cam, a.pixlist[lp], a.s0 + sl, a.seed, cs, fx, fy, o, d);
    p.ray_d[pid] = make_float4(d.x, d.y, d.z, 0.0f);
    if (a.cam_mode & RTG_CAM_LENS) p.ray_o[pid] = make_float4(o.x, o.y, o.z, __int_as_float((int)pid));
}
__global__ __launch_bounds__(RTG_TB) void k_generate_sampled(ChunkArgs a, PathBufs p, CamSampling cs) {
    generate_sampled<false>(a, p, cs);
}

// rtg_probe_camera_samples: camera_sample on given (pixel, sample) pairs
template <bool SOBOL>
static __device__ __forceinline__ void probe_camera(const DevCamera& cam, const CamSampling& cs, unsigned long long seed,
                                                    const unsigned* pixels, const unsigned* samples, unsigned n,
                                                    float* rays, float* film_xy) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float fx, fy;
    v3 o, d;
    camera_sample<SOBOL>(cam, pixels[i], samples[i], seed, cs, fx, fy, o, d);
    float* r = rays + (size_t)i * 8;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = 0.0f;
    r[4] = d.x; r[5] = d.y; r[6] = d.z; r[7] = 0.0f;
    if (film_xy) {
        film_xy[2 * (size_t)i] = fx;
        film_xy[2 * (size_t)i + 1] = fy;
    }
}
__global__ void k_probe_camera(DevCamera cam, CamSampling cs, unsigned long long seed, const unsigned* pixels,
                               const unsigned* samples, unsigned n, float* rays, float* film_xy) {
    probe_camera<false>(cam, cs, seed, pixels, samples, n, rays, film_xy);
}

// ------------------------------------------------------------------ shade: rtg_shade.hip (k_shade, launch_shade)

// ------------------------------------------------------------------ accumulate
__global__ __launch_bounds__(RTG_TB) void k_accumulate(ChunkArgs a, PathBufs p, float* film) {
    const unsigned lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= a.npix) return;
    const unsigned pixel = a.pixlist[lp];
    float fr = film[(size_t)pixel * 3 + 0], fg = film[(size_t)pixel * 3 + 1], fb = film[(size_t)pixel * 3 + 2];
    for (unsigned sl = 0; sl < a.ns; ++sl) {
        const unsigned pid = lp * a.ns + sl;
        const int nt = p.meta[pid] & 0xff;
        float4 acc = p.contrib[(size_t)(nt - 1) * a.P + pid];
        for (int j = nt - 2; j >= 0; --j) {
            const float4 c = p.contrib[(size_t)j * a.P + pid];
            acc = make_float4(c.x + acc.x, c.y + acc.y, c.z + acc.z, 0.0f);
        }
        fr = fr + acc.x;
        fg = fg + acc.y;
        fb = fb + acc.z;
    }
    film[(size_t)pixel * 3 + 0] = fr;
    film[(size_t)pixel * 3 + 1] = fg;
    film[(size_t)pixel * 3 + 2] = fb;
}

// Several samples per pixel (pid = lp * ns + sl): lane = sample, so the contrib reads are
// contiguous. ns >= 33: one wave per pixel, 64 samples at a time; ns <= 32: one group of
// max(ns, 4) lanes per pixel, as many groups as fit in a wave (C5's 16-sample chunks would otherwise
// leave 3/4 of the lanes idle). Each lane folds its path's right-nested sum; then lanes 0-2 of a pixel's group (R, G, B)
// add its samples to the film in sample order from LDS: the same additions in the same order as
// k_accumulate, so the same bits.
__global__ __launch_bounds__(RTG_TB) void k_accumulate_pm(ChunkArgs a, PathBufs p, float* film) {
    __shared__ float s_acc[RTG_TB / 64][64][4];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const unsigned gw = a.ns < 4 ? 4u : a.ns;          // lanes per pixel group (>= 3: R, G, B folds)
    const unsigned ppw = a.ns <= 32 ? 64u / gw : 1u;   // pixels per wave
    const unsigned grp = ppw > 1 ? (unsigned)lane / gw : 0u;
    const unsigned lp = (blockIdx.x * (RTG_TB / 64) + wave) * ppw + grp;
    const bool active = grp < ppw && lp < a.npix;
    const unsigned pixel = active ? a.pixlist[lp] : 0u;
    const unsigned first = ppw > 1 ? grp * gw : 0u;    // the group's first lane
    const unsigned ch = (unsigned)lane - first;        // the channel this lane folds (0-2)
    float fc = (active && ch < 3) ? film[(size_t)pixel * 3 + ch] : 0.0f;
    const unsigned step = ppw > 1 ? a.ns : 64u;
    for (unsigned s0 = 0; s0 < a.ns; s0 += step) {
        const unsigned sl = s0 + ((unsigned)lane - first);
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (active && sl < a.ns) {
            const unsigned pid = lp * a.ns + sl;
            const int nt = p.meta[pid] & 0xff;
            acc = p.contrib[(size_t)(nt - 1) * a.P + pid];
            for (int j = nt - 2; j >= 0; --j) {
                const float4 c = p.contrib[(size_t)j * a.P + pid];
                acc = make_float4(c.x + acc.x, c.y + acc.y, c.z + acc.z, 0.0f);
            }
        }
        s_acc[wave][lane][0] = acc.x;
        s_acc[wave][lane][1] = acc.y;
        s_acc[wave][lane][2] = acc.z;
        __syncthreads();
        const unsigned cnt = min(step, a.ns - s0);
        if (active && ch < 3)
            for (unsigned j = 0; j < cnt; ++j) fc = fc + s_acc[wave][first + j][ch];
        __syncthreads();
    }
    if (active && ch < 3) film[(size_t)pixel * 3 + ch] = fc;
}

// sampleTileWithWeight's splat (Renderer.h:661-670): film += (sum of n samples) / (float)n for the
// listed pixels; tmp holds the per-pixel sums of a scratch render.
__global__ __launch_bounds__(RTG_TB) void k_fold_mean(const unsigned* pixlist, unsigned npix, const float* tmp,
                                                      float count, float* film) {
    const unsigned lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    const size_t q = (size_t)pixlist[lp] * 3;
    for (int c = 0; c < 3; ++c) film[q + c] = film[q + c] + (tmp[q + c] / count);
}

// Per-chunk ray tally: extension + shadow queue lengths of every bounce into stats[2..3]. One wave:
// lane j reads the counters of (bounce, segment) pairs j, j + 64, ... (a lone thread's dependent
// walk over 9 x maxb counters took ~80 us, on the critical path of a 1-spp frame)
__global__ void k_tally(const Counters* ctr, int maxb, unsigned long long* stats) {
    const int lane = threadIdx.x;
    unsigned long long e = 0, sh = 0;
    for (int j = lane; j < maxb * 9; j += 64) {
        const int b = j / 9, k = j % 9;
        if (k == 8) {
            e += ctr[b].n_ext;
            sh += ctr[b].n_shadow;
        } else {  // segmented queues (path tracer)
            e += ctr[b].ne8[32 * k];
            sh += ctr[b].ns8[32 * k];
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        e += __shfl_down(e, off);
        sh += __shfl_down(sh, off);
    }
    if (lane == 0) {
        atomicAdd(&stats[2], e);  // chunks in flight tally concurrently
        atomicAdd(&stats[3], sh);
        atomicAdd(&stats[14], (unsigned long long)ctr[0].n_cam);  // camera rays traced (path tracer)
    }
}

// ------------------------------------------------------------------ the Sobol sampler's kernels (rtg_set_sampler)
// k_generate_sampled with the four draws from the Sobol sampler's camera stream
__global__ __launch_bounds__(RTG_TB) void k_sobol_generate_sampled(ChunkArgs a, PathBufs p, CamSampling cs) {
    generate_sampled<true>(a, p, cs);
}
// ... and k_probe_camera
__global__ void k_sobol_probe_camera(DevCamera cam, CamSampling cs, unsigned long long seed, const unsigned* pixels,
                                     const unsigned* samples, unsigned n, float* rays, float* film_xy) {
    probe_camera<true>(cam, cs, seed, pixels, samples, n, rays, film_xy);
}
// rtg_probe_sampler: draws first_draw .. first_draw + n_draws - 1 of each (pixel, sample), through the
// kernels' own sobol_draw (no rounding of the counter between them)
__global__ void k_probe_sampler(unsigned long long seed, unsigned stream, const unsigned* pixels, const unsigned* samples,
                                unsigned n, unsigned first_draw, unsigned n_draws, unsigned* out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = sobol_key(pixels[i], seed, stream);
    for (unsigned k = 0; k < n_draws; ++k) out[(size_t)i * n_draws + k] = sobol_draw(key, samples[i], first_draw + k);
}

// ================================================================== host side
void free_chunk(ChunkSlot& sl) {
    PathBufs& p = sl.pb;
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);  // queued launches may still use the buffers
    (void)hipFree(p.thr); (void)hipFree(p.rng); (void)hipFree(p.meta); (void)hipFree(p.contrib);
    (void)hipFree(p.q[0]); (void)hipFree(p.q[1]); (void)hipFree(p.hits); (void)hipFree(p.shq); (void)hipFree(p.ctr);
    (void)hipFree(p.ray_o); (void)hipFree(p.ray_d);
    (void)hipFree(p.thr2); (void)hipFree(p.rng2); (void)hipFree(p.ray_o2); (void)hipFree(p.ray_d2);
    (void)hipFree(p.sh_o); (void)hipFree(p.sh_d); (void)hipFree(p.sh_c);
    p = PathBufs{};
    sl.cap_P = 0;
    sl.cap_maxb = 0;
}

// bytes of path state per path: 200 B of payload and queue arrays, 16 B per contribution plane, and
// 8 B for the id queues (light tracer / instant radiosity only)
static size_t path_bytes(int planes, bool queues) { return (size_t)200 + (size_t)16 * (size_t)planes + (queues ? 8u : 0u); }
static size_t slot_bytes(const ChunkSlot& sl) { return sl.cap_P * path_bytes(sl.cap_maxb, sl.pb.q[0] != nullptr); }

// One stream priority per slot: plain streams beyond GPU_MAX_HW_QUEUES share HSA queues, and two
// slots on one queue run in turn (queued 1-spp frames 2.93 ms each). Streams of different priorities
// get queues of their own: 2.28 ms. (Full-CU-mask streams also do, 2.21 ms, but destroying them deadlocked the runtime after a
// few handles (ROCm 7.2, tools/r04_churn.py) and kept alive in a per-device pool they crashed the
// process at exit under rocprofv3: removed)
static int ensure_stream(rtg_handle* h, ChunkSlot& sl) {
    if (!sl.stream) {
        const int k = (int)(&sl - h->slot);
        int lo = 0, hi = 0;
        HIPOK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPOK(hipStreamCreateWithPriority(&sl.stream, hipStreamNonBlocking, k == 0 ? lo : k == 1 ? hi : (lo + hi) / 2));
    }
    if (!sl.fold) HIPOK(hipEventCreateWithFlags(&sl.fold, hipEventDisableTiming));
    return RTG_OK;
}

int ensure_chunk(rtg_handle* h, ChunkSlot& sl, size_t P, int maxb, bool queues) {
    int rc;
    if ((rc = ensure_stream(h, sl))) return rc;
    PathBufs& p = sl.pb;
    if (P <= sl.cap_P && maxb <= sl.cap_maxb) {
        if (queues && !p.q[0]) {
            if (sl.stream) HIPOK(hipStreamSynchronize(sl.stream));
            HIPOK(hipMalloc((void**)&p.q[0], sl.cap_P * sizeof(unsigned)));
            HIPOK(hipMalloc((void**)&p.q[1], sl.cap_P * sizeof(unsigned)));
        }
        return RTG_OK;
    }
    free_chunk(sl);
    const size_t Q = queue_slots(P);  // arrays indexed by queue position (segmented queues)
    HIPOK(hipMalloc((void**)&p.thr, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.rng, Q * sizeof(unsigned long long)));
    HIPOK(hipMalloc((void**)&p.meta, P * sizeof(int)));
    HIPOK(hipMalloc((void**)&p.contrib, P * (size_t)maxb * sizeof(float4)));
    if (queues) {
        HIPOK(hipMalloc((void**)&p.q[0], P * sizeof(unsigned)));
        HIPOK(hipMalloc((void**)&p.q[1], P * sizeof(unsigned)));
    }
    HIPOK(hipMalloc((void**)&p.shq, Q * sizeof(unsigned)));
    HIPOK(hipMalloc((void**)&p.hits, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.ray_o, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.ray_d, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.thr2, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.rng2, Q * sizeof(unsigned long long)));
    HIPOK(hipMalloc((void**)&p.ray_o2, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.ray_d2, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.sh_o, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.sh_d, Q * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.sh_c, P * sizeof(float4)));
    HIPOK(hipMalloc((void**)&p.ctr, (size_t)(maxb + 1) * sizeof(Counters)));
    sl.cap_P = P;
    sl.cap_maxb = maxb;
    return RTG_OK;
}

int ensure_ovf(rtg_handle* h, ChunkSlot& sl) {
    const int grid = trace_blocks_max(h);
    // deepest stack: one entry per BVH2 level, or up to 3 per wide level (each wide level descends
    // at least one BVH2 level); the small-scene variant keeps fewer entries in LDS
    size_t deep = std::max<size_t>(h->bvh_depth, (size_t)h->wide_depth * 3) + 2;
    const size_t lds = std::min(RTG_STACK, RTG_STACK_SMALL);
    size_t levels = deep > lds ? deep - lds : 1;
    size_t need = levels * (size_t)grid * RTG_TTB;
    if (need <= sl.cap_ovf) return RTG_OK;
    if (sl.stream) HIPOK(hipStreamSynchronize(sl.stream));
    (void)hipFree(sl.d_ovf);
    sl.d_ovf = nullptr;
    HIPOK(hipMalloc((void**)&sl.d_ovf, need * sizeof(int)));
    sl.cap_ovf = need;
    return RTG_OK;
}

int flush_pending(rtg_handle* h) {
    if (!h->pend_n) return RTG_OK;
    const uint32_t first = h->pend_first, n = h->pend_n;
    h->pend_n = 0;
    const bool all = h->pend_key.size() == 1 && h->pend_key[0] == 0xffffffffu;
    const std::vector<uint32_t> key = h->pend_key;
    const int rc = render_impl(h, first, n, h->pend_seed, all ? nullptr : key.data(), all ? 0u : (uint32_t)key.size(),
                               h->stream, true, false);
    // rtg_render_async counted the frames in Film::SPP when they were queued; frames whose issue
    // failed never reach the film (chunks issued before the failure may have: the film is then
    // partial, and the error says so)
    if (rc) h->spp -= std::min(h->spp, n);
    return rc;
}

int join_frames(rtg_handle* h) {
    if (int rc = flush_pending(h)) return rc;
    if (!h->inflight) return RTG_OK;
    h->inflight = false;
    HIPOK(hipStreamWaitEvent(h->stream, h->last_fold, 0));
    HIPOK(hipEventRecord(h->ev[1], h->stream));  // the end of the queued run (rtg_stats::render_ms)
    return RTG_OK;
}

int settle(rtg_handle* h) {
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;
    HIPOK(hipStreamSynchronize(h->stream));
    return RTG_OK;
}

// The one place that decides a frame's shading kernel (rtg_internal.h has the families)
ShadeMode shade_mode_of(const rtg_handle* h) {
    const int in = h->integrator;
    const bool path = in == RTG_INTEGRATOR_PATH, direct = in == RTG_INTEGRATOR_DIRECT;
    const bool samples_light = path || direct || in == RTG_INTEGRATOR_DIRECT_MIS;
    const bool physical = h->material_model == RTG_MATERIALS_PHYSICAL && h->phys_built && (path || direct);
    const bool mis = h->path_mis == RTG_PATH_MIS_POWER && path && h->mt.mis_index.p != nullptr;
    ShadeMode m{};
    m.alt = !path;
    m.env = samples_light ? env_table_set(h) : EnvTable{nullptr, 0u, 0u, 0u};
    m.pick = LightPick{samples_light && h->light_sampling.mode == RTG_LIGHTS_POWER ? h->mt.light.p : nullptr};
    m.phys = physical && h->phys_any ? PhysArgs{h->mt.phys.p, h->mt.phys_index.p, h->n_phys} : PhysArgs{nullptr, nullptr, 0};
    m.mis = MisArgs{mis ? h->mt.mis_index.p : nullptr};
    if (physical && h->trans_any) m.family = mis ? ShadeFamily::TransMis : ShadeFamily::Trans;
    else if (mis) m.family = ShadeFamily::Mis;
    else if (m.phys.table) m.family = ShadeFamily::Phys;
    else if (m.pick.table && h->light_grid.cells && h->mt.grid.p && h->mt.grid_rec.p) m.family = ShadeFamily::Grid;
    else if (m.pick.table) m.family = ShadeFamily::Pick;
    else m.family = m.env.table ? ShadeFamily::Env : ShadeFamily::Plain;
    // k_shade_mis under the reference model, or in a scene without a physical record: reference-kind
    // records for every index
    if (m.family == ShadeFamily::Mis && !m.phys.table) m.phys = PhysArgs{h->mt.mis_ref.p, nullptr, h->n_mis_ref};
    if (m.family == ShadeFamily::Grid) m.grid = h->mt.grid_rec.p;
    // rtg_set_sampler: the families with Sobol kernels, under the integrators that draw
    m.sobol = h->sampler == RTG_SAMPLER_SOBOL && samples_light &&
              (m.family == ShadeFamily::Plain || m.family == ShadeFamily::Env || m.family == ShadeFamily::Pick);
    m.tab = h->sv.n_mats <= RTG_LDS_MATS && h->sv.n_lights <= RTG_LDS_LIGHTS && m.phys.n <= RTG_LDS_PHYS;
    return m;
}

static int launch_shade_bounce(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                               const PathBufs& p, int b) {
    switch (m.family) {
    case ShadeFamily::Pick: return launch_shade_pick(m, grid, st, s, a, p, b);
    case ShadeFamily::Grid: return launch_shade_grid(m, grid, st, s, a, p, b);
    case ShadeFamily::Phys: return launch_shade_phys(m, grid, st, s, a, p, b);
    case ShadeFamily::Mis: return launch_shade_mis(m, grid, st, s, a, p, b);
    case ShadeFamily::Trans:
    case ShadeFamily::TransMis: return launch_shade_trans(m, grid, st, s, a, p, b);
    default: return launch_shade(m, grid, st, s, a, p, b);
    }
}

// Pixel list in tile order (32x32 tiles, row-major inside a tile), for the requested tiles.
int set_pixels(rtg_handle* h, const uint32_t* tiles, uint32_t n_tiles) {
    const int TS = 32;
    const uint32_t tx = (h->W + TS - 1) / TS, ty = (h->H + TS - 1) / TS;
    std::vector<uint32_t> key;
    if (tiles) key.assign(tiles, tiles + n_tiles);
    else key.push_back(0xffffffffu);
    if (h->d_pix && key == h->pix_key) return RTG_OK;
    std::vector<uint32_t> pix;
    auto add_tile = [&](uint32_t t) {
        uint32_t bx = (t % tx) * TS, by = (t / tx) * TS;
        for (uint32_t y = by; y < std::min<uint32_t>(by + TS, h->H); ++y)
            for (uint32_t x = bx; x < std::min<uint32_t>(bx + TS, h->W); ++x) pix.push_back(y * h->W + x);
    };
    if (tiles) {
        for (uint32_t i = 0; i < n_tiles; ++i) {
            if (tiles[i] >= tx * ty) { g_err = "tile id out of range"; return RTG_ERR_ARG; }
            add_tile(tiles[i]);
        }
    } else {
        for (uint32_t t = 0; t < tx * ty; ++t) add_tile(t);
    }
    // launches already queued may still read the old list (rtg_render_async, adaptive groups):
    // drain them before it is overwritten (hipMemcpy does not order against non-blocking streams)
    HIPOK(hipDeviceSynchronize());
    if (pix.size() > h->cap_pix) {
        (void)hipFree(h->d_pix);
        HIPOK(hipMalloc((void**)&h->d_pix, std::max<size_t>(pix.size(), 1) * 4));
        h->cap_pix = pix.size();
    }
    if (!pix.empty()) HIPOK(hipMemcpy(h->d_pix, pix.data(), pix.size() * 4, hipMemcpyHostToDevice));
    h->npix = (unsigned)pix.size();
    h->pix_key = key;
    return RTG_OK;
}

int launch_generate(rtg_handle* h, const ChunkArgs& a, const PathBufs& pb, hipStream_t st) {
    (void)h;
    hipLaunchKernelGGL(k_generate, dim3((a.P + RTG_TB - 1) / RTG_TB), dim3(RTG_TB), 0, st, a, pb);
    LAUNCH_OK("k_generate");
    return RTG_OK;
}

static void timed_begin(rtg_handle* h, hipStream_t st, size_t k) {
    if (!h->timing) return;
    while (h->kev.size() < 2 * (k + 1)) { hipEvent_t e; (void)hipEventCreate(&e); h->kev.push_back(e); }
    (void)hipEventRecord(h->kev[2 * k], st);
}
// kinds: the timed launches of this render so far (0 trace, 2 other); launch k uses kev[2k], kev[2k + 1]
static void timed_end(rtg_handle* h, hipStream_t st, std::vector<int>& kinds, int kind) {
    if (h->timing) (void)hipEventRecord(h->kev[2 * kinds.size() + 1], st);
    kinds.push_back(kind);
}

// RTG_DEBUG builds, RTG_OPT_WAVETIME: per launch, when the waves started, found the queue empty and ended
static void print_wavetime(const std::vector<unsigned long long>& wt, int maxb, size_t wt_waves) {
    for (int b = 0; b <= maxb; ++b) {
        const unsigned long long* w = wt.data() + (size_t)b * wt_waves * 3;
        unsigned long long t0 = ~0ull, e0 = ~0ull;
        std::vector<double> ends, starts;
        for (size_t i = 0; i < wt_waves; ++i) {
            if (!w[3 * i]) continue;
            t0 = std::min(t0, w[3 * i]);
            if (w[3 * i + 1]) e0 = std::min(e0, w[3 * i + 1]);
        }
        for (size_t i = 0; i < wt_waves; ++i) {
            if (!w[3 * i]) continue;
            starts.push_back((w[3 * i] - t0) * 0.01);  // 100 MHz clock -> us
            ends.push_back((w[3 * i + 2] - t0) * 0.01);
        }
        if (ends.empty()) continue;
        std::sort(ends.begin(), ends.end());
        std::sort(starts.begin(), starts.end());
        auto pct = [](const std::vector<double>& v, double q) { return v[std::min(v.size() - 1, (size_t)(q * v.size()))]; };
        std::fprintf(stderr, "[wavetime] launch %d waves %zu start p50 %.1f max %.1f | queue empty %.1f | "
                     "wave end p10 %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f us\n", b, ends.size(), pct(starts, 0.5),
                     starts.back(), (e0 - t0) * 0.01, pct(ends, 0.1), pct(ends, 0.5), pct(ends, 0.9), pct(ends, 0.99),
                     ends.back());
    }
}

// "rtg:trace b=<b>" / "rtg:shade b=<b>" names for b < 32 (static strings: roctx copies nothing)
static const char* roctx_stage_name(int kind, int b) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (const char* stage : {"rtg:trace b=", "rtg:shade b="})
            for (int i = 0; i < 32; ++i) v.push_back(stage + std::to_string(i));
        return v;
    }();
    if (b < 0 || b >= 32) return kind ? "rtg:shade" : "rtg:trace";
    return names[(kind ? 32 : 0) + b].c_str();
}

// The 8 segment counts of bounce b that k_trace(b)'s block 0 stores into h_cnt as it starts. The
// host polls the host-coherent words; a launch that ended (or failed) without writing them is an
// error, not a hang.
static int wait_counts(rtg_handle* h, int b) {
    unsigned* c = h->h_cnt + 8 * b;
    auto ready = [&]() {
        for (int k = 0; k < 8; ++k)
            if (__atomic_load_n(c + k, __ATOMIC_ACQUIRE) == RTG_CNT_PENDING) return false;
        return true;
    };
    for (unsigned spin = 1;; ++spin) {
        if (ready()) return RTG_OK;
        if ((spin & 255u) == 0) {
            const hipError_t e = hipEventQuery(h->tev[b]);
            if (e == hipSuccess) {
                if (ready()) return RTG_OK;
                g_err = "k_trace finished without storing its segment counts";
                return RTG_ERR_HIP;
            }
            if (e != hipErrorNotReady) {
                g_err = std::string("k_trace (segment counts): ") + hipGetErrorString(e);
                return RTG_ERR_HIP;
            }
            std::this_thread::yield();
        }
    }
}

// ------------------------------------------------------------------ render_impl: plan, issue, join
static const size_t MEM_UNKNOWN = ~(size_t)0;

// The chunk-size plan: samples per chunk. avail: the free HBM plus the path state the slots hold now
// (MEM_UNKNOWN: no reading, no memory bound); cap_P0, cap_maxb0: slot 0's buffers; may_pipe: a queued
// render outside the diagnostic modes, whose chunks may rotate through the slots.
static uint32_t plan_chunk_samples(uint32_t n_samples, uint32_t npix, int planes, uint32_t max_paths, size_t avail,
                                   size_t mem_cap, size_t cap_P0, int cap_maxb0, bool may_pipe) {
    uint32_t ns_chunk = std::max<uint32_t>(1, std::min<uint32_t>(n_samples, max_paths / std::max(1u, npix)));
    if (avail != MEM_UNKNOWN) {
        // path state of the chunks in flight takes at most RTG_MEM_PCT % of the free HBM (buffers held
        // now count as free); pipelined chunks keep RTG_SLOTS sets
        size_t budget = avail / 100 * RTG_MEM_PCT;
        if (mem_cap) budget = std::min(budget, mem_cap);
        const size_t per_pix = path_bytes(planes, false) * std::max<size_t>(1, npix);
        size_t max_ns = budget / per_pix;
        if (may_pipe && (size_t)ns_chunk * npix <= RTG_PIPE_MAX_P) max_ns = budget / RTG_SLOTS / per_pix;
        ns_chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(ns_chunk, max_ns));
    }
    // Keep the chunk buffers once they hold most of what the budget asks for: the free-memory
    // reading moves between calls, and growing a buffer of ~100 GB means a free and a new
    // hipMalloc that took 5.5 s on C4 with 1G paths in flight.
    const uint32_t fit = cap_maxb0 >= planes ? (uint32_t)(cap_P0 / std::max(1u, npix)) : 0u;
    if (fit >= 1 && ns_chunk > fit && (uint64_t)fit * 4 >= (uint64_t)ns_chunk * 3) ns_chunk = fit;
    // equal chunks: 256 samples at <= 123 per chunk run as 86 + 85 + 85, not 123 + 123 + 10 (a thin
    // last chunk is mostly drain tail)
    const uint32_t nchunks = (n_samples + ns_chunk - 1) / ns_chunk;
    return (n_samples + nchunks - 1) / nchunks;
}

// The host-coherent segment counts (rtg_handle::h_cnt) and the trace-finished events of maxb + 1 launches
static int ensure_counts(rtg_handle* h, int maxb) {
    if (h->cap_cnt < maxb + 1) {
        if (h->h_cnt) (void)hipHostFree(h->h_cnt);
        h->h_cnt = h->d_hcnt = nullptr;
        h->cap_cnt = 0;
        HIPOK(hipHostMalloc((void**)&h->h_cnt, (size_t)(maxb + 1) * 8 * sizeof(unsigned),
                            hipHostMallocCoherent | hipHostMallocMapped));
        HIPOK(hipHostGetDevicePointer((void**)&h->d_hcnt, h->h_cnt, 0));
        h->cap_cnt = maxb + 1;
    }
    while ((int)h->tev.size() < maxb + 1) {
        hipEvent_t e;
        HIPOK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->tev.push_back(e);
    }
    return RTG_OK;
}

static ChunkArgs chunk_args(const rtg_handle* h, uint32_t s0, uint32_t ns, uint64_t seed) {
    ChunkArgs a;
    a.pixlist = h->d_pix;
    a.npix = h->npix;
    a.ns = ns;
    a.s0 = s0;
    a.P = a.ns * h->npix;
    a.seed = seed;
    a.max_depth = h->max_depth;
    a.mode = h->integrator;
    a.cam = h->cam;
    a.lean = 1;
    a.cam_mode = cam_mode_of(h);
    a.seg_tiles = (unsigned)seg_tiles(a.P);
    set_ns_div(a);
    return a;
}

// k_shade(b - 1)'s grid, one 256-path tile per block: 8 x the largest segment's live tiles (hostgrid:
// the segment counts of bounce b - 1 arrived while k_trace(b - 1) ran; bounce 0: the camera rays)
static int shade_tiles(rtg_handle* h, const ChunkArgs& a, int b, bool hostgrid, unsigned& tiles) {
    tiles = hostgrid ? 0u : a.seg_tiles;
    const unsigned cap = a.seg_tiles * RTG_TB;
    for (int sgm = 0; hostgrid && sgm < 8; ++sgm) {
        unsigned live = 0;
        if (b == 1) {
            live = a.P > sgm * cap ? std::min(cap, a.P - sgm * cap) : 0u;
        } else {
            if (sgm == 0)
                if (int rc = wait_counts(h, b - 1)) return rc;
            live = h->h_cnt[8 * (b - 1) + sgm];
        }
        tiles = std::max(tiles, (live + RTG_TB - 1) / RTG_TB);
    }
    return RTG_OK;
}

// The path tracer's trace launch b: where its rays are and where their results go
static void wire_bounce(TraceIO& io, const ChunkArgs& a, const PathBufs& pb, int b, int maxb) {
    // extension payload by queue position (set b & 1; null queue: path id = position);
    // bounce 0: the camera origin, directions from k_generate in set 0
    // per-sample camera rays (rtg_set_camera_sampling): bounce 0 is wired like every later bounce,
    // the P rays k_generate_sampled wrote as the eight segments ctr[0].ne8 at identity positions (a
    // single counter would serialise 64M rays' fetches), their origins in ray_o with a lens
    const bool cam_seg = b == 0 && a.cam_mode != 0;
    const bool cam_one = b == 0 && a.cam_mode == 0;
    io.queue = nullptr;
    io.ray_o = b == 0 ? ((a.cam_mode & RTG_CAM_LENS) ? pb.ray_o : nullptr) : ((b & 1) ? pb.ray_o2 : pb.ray_o);
    io.cam_o = make_float4(a.cam.ox, a.cam.oy, a.cam.oz, 0.0f);
    io.ray_d = (b & 1) ? pb.ray_d2 : pb.ray_d;
    // segmented queues; bounce 0 by default: one queue of npix camera rays (a ray per pixel, shared
    // by the pixel's samples) at identity positions, one work counter
    io.count = cam_one ? &pb.ctr[0].n_cam : nullptr;
    io.seg_cap = cam_one ? 0u : a.seg_tiles * RTG_TB;
    io.seg_ne = ((b > 0 && b < maxb) || cam_seg) ? pb.ctr[b].ne8 : nullptr;
    io.seg_ns = b > 0 ? pb.ctr[b - 1].ns8 : nullptr;
    io.hits = pb.hits;
    io.squeue = pb.shq;
    io.sray_o = pb.sh_o;
    io.sray_d = pb.sh_d;
    io.sray_c = pb.sh_c;
    io.spos = 1;
    io.scount = nullptr;
    io.contrib = b > 0 ? pb.contrib + (size_t)(b - 1) * a.P : nullptr;
    io.visible = nullptr;
    io.fetch = &pb.ctr[b].f_ext;
    io.fetch8 = cam_one ? nullptr : pb.ctr[b].f8;
}

// the wave slots of the largest k_trace grid (RTG_OPT_WAVETIME: three clocks per wave and launch)
static size_t wavetime_waves(const rtg_handle* h) { return (size_t)trace_blocks_max(h) * (RTG_TTB / 64); }

// One chunk's launches up to its ray tally, on its slot's stream. first: chunk 0 of the render (the
// RTG_DEBUG capture); d_wt: its per-wave clocks, or null.
static int issue_chunk(rtg_handle* h, ChunkSlot& sl, const ChunkArgs& a, int maxb, bool hostgrid, bool first,
                       unsigned long long* d_wt, std::vector<int>& kinds) {
    const hipStream_t ss = sl.stream;
    const PathBufs& pb = sl.pb;
    const ShadeMode mode = shade_mode_of(h);
    int rc;
    TraceIO io{};
    io.stats = h->d_stats;
    io.cull = h->cull;
    io.wide = h->wide;
    io.ovf = sl.d_ovf;
    HIPOK(hipMemsetAsync(pb.ctr, 0, (size_t)(maxb + 1) * sizeof(Counters), ss));
    timed_begin(h, ss, kinds.size());
    {
        RoctxRange r_gen("rtg:generate");
        if (a.cam_mode) {  // rtg_set_camera_sampling: a camera ray per path
            hipLaunchKernelGGL(mode.sobol ? k_sobol_generate_sampled : k_generate_sampled,
                               dim3((a.P + RTG_TB - 1) / RTG_TB), dim3(RTG_TB), 0, ss, a, pb, cam_sampling_dev(h));
            LAUNCH_OK("k_generate_sampled");
        } else {
            hipLaunchKernelGGL(k_generate, dim3((a.npix + RTG_TB - 1) / RTG_TB), dim3(RTG_TB), 0, ss, a, pb);  // lean: per pixel
            LAUNCH_OK("k_generate");
        }
    }
    timed_end(h, ss, kinds, 2);
    // Trace launch L_b (b = 0..maxb) carries the extension rays of bounce b (from shade(b-1),
    // or generate) and the shadow rays of bounce b-1: one persistent launch, one drain tail.
    for (int b = 0; b <= maxb; ++b) {
        if (b > 0) {
            RoctxRange r_shade(roctx_stage_name(1, b - 1));
            unsigned tiles = 0;
            if ((rc = shade_tiles(h, a, b, hostgrid, tiles))) return rc;
            if (tiles) {
                timed_begin(h, ss, kinds.size());
                if ((rc = launch_shade_bounce(mode, 8 * tiles, ss, h->sv, a, pb, b - 1))) return rc;
                timed_end(h, ss, kinds, 2);
            }
        }
        wire_bounce(io, a, pb, b, maxb);
        io.wtime = d_wt ? d_wt + (size_t)b * wavetime_waves(h) * 3 : nullptr;
        io.cap = nullptr;
        io.cap_len = nullptr;
        // k_trace(b) hands the host bounce b's segment counts, for k_shade(b)'s grid
        io.hcnt = nullptr;
        if (hostgrid && b > 0 && b < maxb) {
            for (int k = 0; k < 8; ++k) __atomic_store_n(h->h_cnt + 8 * b + k, RTG_CNT_PENDING, __ATOMIC_RELAXED);
            io.hcnt = h->d_hcnt + 8 * b;
        }
        if (RTG_DEBUG && first && b == h->capture_launch && (rc = capture_begin(h, io, a.seg_tiles, ss))) return rc;
        timed_begin(h, ss, kinds.size());
        {
            RoctxRange r_trace(roctx_stage_name(0, b));
            // the camera launch (a ray per pixel, one work counter): no more one-wave blocks than it
            // has tail batches of rays, so waves without work do not queue their probes on the
            // counter (+0.5 %)
            const unsigned cam_blocks =
                (b == 0 && !a.cam_mode) ? std::max(8u, (a.npix + RTG_TAIL_BATCH - 1) / RTG_TAIL_BATCH) : 0u;
            if ((rc = launch_trace(h, io, ss, cam_blocks))) return rc;
        }
        timed_end(h, ss, kinds, 0);
        if (io.hcnt) HIPOK(hipEventRecord(h->tev[b], ss));
    }
    hipLaunchKernelGGL(k_tally, dim3(1), dim3(64), 0, ss, pb.ctr, maxb, h->d_stats);
    LAUNCH_OK("k_tally");
    return RTG_OK;
}

// The chunk's film fold. The film takes the chunks in sample order: it runs after the previous chunk's.
static int fold_chunk(rtg_handle* h, ChunkSlot& sl, const ChunkArgs& a, bool pipe, std::vector<int>& kinds) {
    const hipStream_t ss = sl.stream;
    const PathBufs& pb = sl.pb;
    RoctxRange r_acc("rtg:accumulate");
    if (h->last_fold) HIPOK(hipStreamWaitEvent(ss, h->last_fold, 0));
    if (pipe) HIPOK(hipStreamWaitEvent(ss, h->entry, 0));  // the film's readers and writers so far
    timed_begin(h, ss, kinds.size());
    if (a.ns > 1) {
        const unsigned ppw = a.ns <= 32 ? 64u / (a.ns < 4 ? 4u : a.ns) : 1u;  // pixels per wave (k_accumulate_pm)
        const unsigned waves = (h->npix + ppw - 1) / ppw;
        hipLaunchKernelGGL(k_accumulate_pm, dim3((waves + RTG_TB / 64 - 1) / (RTG_TB / 64)), dim3(RTG_TB), 0, ss, a,
                           pb, h->d_film);
    } else
        hipLaunchKernelGGL(k_accumulate, dim3((h->npix + RTG_TB - 1) / RTG_TB), dim3(RTG_TB), 0, ss, a, pb, h->d_film);
    LAUNCH_OK("k_accumulate");
    timed_end(h, ss, kinds, 2);
    HIPOK(hipEventRecord(sl.fold, ss));
    sl.used = true;
    h->last_fold = sl.fold;
    h->inflight = true;
    h->stats.paths += a.P;
    return RTG_OK;
}

// RTG_OPT_TIMING: the per-launch times of a waited-for render into the stats, and the rays of each
// trace launch of its last chunk (camera rays, then extension + shadow rays)
static int collect_timing(rtg_handle* h, int maxb, const std::vector<int>& kinds) {
    HIPOK(hipEventSynchronize(h->ev[1]));
    h->stats.extend_ms = h->stats.shadow_ms = h->stats.shade_ms = 0;
    h->stats.extend_launches = 0;
    h->launch_ms.clear();
    h->launch_rays.clear();
    std::vector<Counters> cc((size_t)maxb + 1);
    // (a waited-for render runs its chunks in slot 0)
    if (h->slot[0].pb.ctr &&
        hipMemcpy(cc.data(), h->slot[0].pb.ctr, cc.size() * sizeof(Counters), hipMemcpyDeviceToHost) == hipSuccess) {
        for (int b = 0; b <= maxb; ++b) {
            unsigned long long r = b == 0 ? cc[0].n_cam : 0ull;
            for (int k = 0; k < 8; ++k) {
                if (b > 0 && b < maxb) r += cc[b].ne8[32 * k];
                if (b > 0) r += cc[b - 1].ns8[32 * k];
            }
            h->launch_rays.push_back(r);
        }
    }
    for (size_t j = 0; j < kinds.size(); ++j) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, h->kev[2 * j], h->kev[2 * j + 1]);
        (kinds[j] == 0 ? h->stats.extend_ms : h->stats.shade_ms) += ms;
        if (kinds[j] == 0) {
            h->stats.extend_launches++;
            h->launch_ms.push_back(ms);
        }
    }
    return RTG_OK;
}

int render_impl(rtg_handle* h, uint32_t first, uint32_t n_samples, uint64_t seed,
                       const uint32_t* tiles, uint32_t n_tiles, hipStream_t st, bool lazy, bool add_spp) {
    RoctxRange r_render(lazy ? "rtg:render (queued chunks)" : "rtg:render");
    int rc = set_pixels(h, tiles, n_tiles);
    if (rc) return rc;
    if (h->npix == 0 || n_samples == 0) return RTG_OK;
    if ((uint64_t)first + n_samples > 65536u) { g_err = "sample index >= 65536 (PCG stream key)"; return RTG_ERR_ARG; }
    const int maxb = h->max_depth + 2;
    // computeDirectMIS keeps two scratch planes of per-path state in contrib planes 2 and 3
    const int planes = h->integrator == RTG_INTEGRATOR_DIRECT_MIS ? std::max(maxb, 4) : maxb;
    // the diagnostic modes read one chunk's launches in order on one stream (per-launch timing
    // events work across the slots' streams: overlapped launches then count their shared time twice)
    const bool diag = h->serial || (RTG_DEBUG && (h->wavetime || h->capture_launch >= 0));
    // ---- plan
    size_t freeb = 0, totalb = 0, avail = MEM_UNKNOWN;
    if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
        avail = freeb;
        for (const ChunkSlot& sl : h->slot) avail += slot_bytes(sl);
    }
    const uint32_t ns_chunk = plan_chunk_samples(n_samples, h->npix, planes, h->max_paths, avail, h->mem_cap,
                                                 h->slot[0].cap_P, h->slot[0].cap_maxb, lazy && !diag);
    const size_t P = (size_t)ns_chunk * h->npix;
    h->stats.chunk_samples = std::max<uint64_t>(h->stats.chunk_samples, ns_chunk);
    // the frame pipeline (rtg_internal.h, ChunkSlot): queued chunks of up to RTG_PIPE_MAX_P paths
    // rotate through the slots with no host wait, so the next queued frames run beside them. A call
    // that is waited for runs its chunks one at a time in slot 0: chunks of one render side by side
    // measured slower than one chunk (C3 at N = 1 and rank 0's share of 8: the traversals slow each
    // other down and add launches)
    const bool pipe = lazy && !diag && P <= RTG_PIPE_MAX_P;
    (void)hipGetLastError();  // drop any stale error left by other code on this thread
    if (!h->inflight) HIPOK(hipEventRecord(h->ev[0], st));  // start of this render (or of a queued run)
    HIPOK(hipEventRecord(h->entry, st));  // every chunk starts after the caller's earlier work on st
    if ((rc = ensure_counts(h, maxb))) return rc;
    std::vector<int> kinds;  // the timed launches (timed_end)
    // ---- for each chunk: issue, fold
    uint32_t c = 0;
    for (uint32_t s0 = first; s0 < first + n_samples; s0 += ns_chunk, ++c) {
        ChunkSlot& sl = pipe ? h->slot[h->next_slot++ % RTG_SLOTS] : h->slot[0];
        // back-pressure: a slot takes its next chunk once its previous one has left the GPU, so at
        // most RTG_SLOTS chunks are in flight and the host stays at most that far ahead
        if (pipe && sl.used) HIPOK(hipEventSynchronize(sl.fold));
        if ((rc = ensure_chunk(h, sl, P, planes, false))) return rc;
        if ((rc = ensure_ovf(h, sl))) return rc;
        // A chunk starts after the caller's earlier work on st. A queued (pipelined) chunk reads
        // nothing the caller's work on the handle's stream writes (film reads and gathers, film
        // loads; pixel lists and clears wait for the device on the host), so only its fold waits
        // for that work (fold_chunk): the chunk's traversal can start while earlier frames drain.
        if (!pipe) HIPOK(hipStreamWaitEvent(sl.stream, h->entry, 0));
        // RTG_DEBUG builds with RTG_OPT_WAVETIME: per-wave clocks of chunk 0's trace launches, on stderr
        unsigned long long* d_wt = nullptr;
        std::vector<unsigned long long> wt(RTG_DEBUG && h->wavetime && c == 0 ? (maxb + 1) * wavetime_waves(h) * 3 : 0);
        if (!wt.empty()) {
            HIPOK(hipMalloc((void**)&d_wt, wt.size() * sizeof(unsigned long long)));
            HIPOK(hipMemsetAsync(d_wt, 0, wt.size() * sizeof(unsigned long long), sl.stream));
        }
        const ChunkArgs a = chunk_args(h, s0, std::min(ns_chunk, first + n_samples - s0), seed);
        // k_shade grids from the live counts read back while the traversal runs (big chunks), or over
        // every tile a segment can hold (blocks past the live count exit at once): no host wait
        const bool hostgrid = !pipe && (a.seg_tiles >= RTG_HOSTGRID_MIN_TILES || h->serial);
        if ((rc = issue_chunk(h, sl, a, maxb, hostgrid, c == 0, d_wt, kinds))) return rc;
        if ((rc = fold_chunk(h, sl, a, pipe, kinds))) return rc;
        if (d_wt) {
            HIPOK(hipStreamSynchronize(sl.stream));
            HIPOK(hipMemcpy(wt.data(), d_wt, wt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            (void)hipFree(d_wt);
            print_wavetime(wt, maxb, wavetime_waves(h));
        }
    }
    if (add_spp) h->spp += n_samples;
    if (lazy) return RTG_OK;
    // ---- join
    // the caller's stream waits for the chunks (and for every chunk queued before them). The queued
    // chunks are joined to the handle's own stream only when that is the caller's stream; a render
    // on a user stream leaves them in flight, so join_frames (film read, clear, stats) still makes
    // the handle's stream wait for them
    if (st == h->stream) h->inflight = false;
    HIPOK(hipStreamWaitEvent(st, h->last_fold, 0));
    HIPOK(hipEventRecord(h->ev[1], st));
    return h->timing ? collect_timing(h, maxb, kinds) : RTG_OK;
}

// RTG_ERR_ARG (with "who: ..." as the message) for a setting outside include/rtg.h's ranges
int camera_sampling_check(const char* who, const rtg_camera_sampling* p) {
    auto bad = [&](const char* what) {
        g_err = std::string(who) + ": " + what;
        return RTG_ERR_ARG;
    };
    if (!p) return bad("null argument");
    if (p->filter < RTG_FILTER_NONE || p->filter > RTG_FILTER_TENT) return bad("unknown filter");
    if (!std::isfinite(p->filter_radius) || p->filter_radius < 0.0f || p->filter_radius > RTG_FILTER_MAX_RADIUS)
        return bad("filter_radius must be finite and in [0, RTG_FILTER_MAX_RADIUS]");
    if (!std::isfinite(p->lens_radius) || p->lens_radius < 0.0f) return bad("lens_radius must be finite and >= 0");
    if (p->lens_radius > 0.0f && !(std::isfinite(p->focal_distance) && p->focal_distance > 0.0f))
        return bad("focal_distance must be finite and > 0 with a lens");
    return RTG_OK;
}

extern "C" {

int rtg_camera_sampling_defaults(rtg_camera_sampling* p) {
    if (!p) { g_err = "rtg_camera_sampling_defaults: null argument"; return RTG_ERR_ARG; }
    *p = rtg_camera_sampling{RTG_FILTER_NONE, 0.5f, 0.0f, 1.0f};
    return RTG_OK;
}

int rtg_set_camera_sampling(rtg_handle* h, const rtg_camera_sampling* p) {
    if (!h) { g_err = "rtg_set_camera_sampling: null handle"; return RTG_ERR_ARG; }
    if (int rc = camera_sampling_check("rtg_set_camera_sampling", p)) return rc;
    if (int rc = settle(h)) return rc;
    h->cam_sampling = *p;
    return RTG_OK;
}

int rtg_get_camera_sampling(rtg_handle* h, rtg_camera_sampling* p) {
    if (!h || !p) { g_err = "rtg_get_camera_sampling: null argument"; return RTG_ERR_ARG; }
    *p = h->cam_sampling;
    return RTG_OK;
}

int rtg_probe_camera_samples(rtg_handle* h, const uint32_t* pixels, const uint32_t* samples, uint32_t n,
                             uint64_t seed, float* rays, float* film_xy) {
    if (!h || !pixels || !samples || !rays) { g_err = "rtg_probe_camera_samples: null argument"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 8u) { g_err = "rtg_probe_camera_samples: too many cases"; return RTG_ERR_ARG; }
    const uint64_t npix = (uint64_t)h->W * (uint64_t)h->H;
    for (uint32_t i = 0; i < n; ++i)
        if (pixels[i] >= npix || samples[i] >= RTG_MAX_SAMPLES_PER_KEY) {
            g_err = "rtg_probe_camera_samples: pixel or sample index out of range";
            return RTG_ERR_ARG;
        }
    if (n == 0) return RTG_OK;
    HIPOK(hipSetDevice(h->device));
    return probe_run({{pixels, (size_t)n * sizeof(unsigned)}, {samples, (size_t)n * sizeof(unsigned)}},
                     {{rays, (size_t)n * 8 * sizeof(float)}, {film_xy, (size_t)n * 2 * sizeof(float)}}, [&](void* const* d) {
                         hipLaunchKernelGGL(shade_mode_of(h).sobol ? k_sobol_probe_camera : k_probe_camera, dim3((n + 255) / 256), dim3(256), 0, nullptr, h->cam,
                                            cam_sampling_dev(h), (unsigned long long)seed, (const unsigned*)d[0],
                                            (const unsigned*)d[1], (unsigned)n, (float*)d[2], (float*)d[3]);
                     });
}

int rtg_sampler_check(int sampler) {
    if (sampler != RTG_SAMPLER_PCG && sampler != RTG_SAMPLER_SOBOL) {
        g_err = "rtg_set_sampler: unknown sampler";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

int rtg_set_sampler(rtg_handle* h, int sampler) {
    if (!h) { g_err = "rtg_set_sampler: null handle"; return RTG_ERR_ARG; }
    if (int rc = rtg_sampler_check(sampler)) return rc;
    if (int rc = settle(h)) return rc;
    h->sampler = sampler;
    return RTG_OK;
}

int rtg_get_sampler(rtg_handle* h, int* sampler) {
    if (!h || !sampler) { g_err = "rtg_get_sampler: null argument"; return RTG_ERR_ARG; }
    *sampler = h->sampler;
    return RTG_OK;
}

int rtg_sampler_active(rtg_handle* h, int* sampler) {
    if (!h || !sampler) { g_err = "rtg_sampler_active: null argument"; return RTG_ERR_ARG; }
    *sampler = shade_mode_of(h).sobol ? RTG_SAMPLER_SOBOL : RTG_SAMPLER_PCG;
    return RTG_OK;
}

int rtg_probe_sampler(uint64_t seed, uint32_t stream, const uint32_t* pixels, const uint32_t* samples, uint32_t n,
                      uint32_t first_draw, uint32_t n_draws, uint32_t* out_raw) {
    if (!pixels || !samples || !out_raw) { g_err = "rtg_probe_sampler: null argument"; return RTG_ERR_ARG; }
    if ((uint64_t)n * n_draws > 0x7fffffffu / 4u) { g_err = "rtg_probe_sampler: too many draws"; return RTG_ERR_ARG; }
    if (n == 0 || n_draws == 0) return RTG_OK;
    const size_t bytes = (size_t)n * sizeof(unsigned);
    return probe_run({{pixels, bytes}, {samples, bytes}}, {{out_raw, bytes * n_draws}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_sampler, dim3((n + 255) / 256), dim3(256), 0, nullptr, (unsigned long long)seed,
                           (unsigned)stream, (const unsigned*)d[0], (const unsigned*)d[1], (unsigned)n,
                           (unsigned)first_draw, (unsigned)n_draws, (unsigned*)d[2]);
    });
}

int rtg_render_async(rtg_handle* h, uint32_t first, uint32_t n, uint64_t seed, const uint32_t* tiles,
                     uint32_t n_tiles, void* stream) {
    if (!h) { g_err = "null handle"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    if (stream) {
        if (int rc = flush_pending(h)) return rc;
        return render_impl(h, first, n, seed, tiles, n_tiles, (hipStream_t)stream, false);
    }
    if (n == 0) return RTG_OK;
    if ((uint64_t)first + n > 65536u) { g_err = "sample index >= 65536 (PCG stream key)"; return RTG_ERR_ARG; }
    // queued: coalesced with the pending calls when it continues them (same seed and tiles, the
    // next sample indices); otherwise those are issued first
    std::vector<uint32_t> key;
    if (tiles) key.assign(tiles, tiles + n_tiles);
    else key.push_back(0xffffffffu);
    if (h->pend_n && (key != h->pend_key || seed != h->pend_seed || first != h->pend_first + h->pend_n))
        if (int rc = flush_pending(h)) return rc;
    if (int rc = set_pixels(h, tiles, n_tiles)) return rc;  // (validates the tiles; a no-op when unchanged)
    if (!h->pend_n) {
        h->pend_first = first;
        h->pend_seed = seed;
        h->pend_key.swap(key);
    }
    if (h->npix == 0) return RTG_OK;  // no pixels: nothing is rendered and Film::SPP stays (as rtg_render)
    h->pend_n += n;
    h->spp += n;  // Film::SPP counts the queued frames at once (taken back if their issue fails)
    if (h->no_coalesce || (uint64_t)h->pend_n * h->npix >= RTG_COALESCE_P) return flush_pending(h);
    return RTG_OK;
}

int rtg_render(rtg_handle* h, uint32_t first, uint32_t n, uint64_t seed, const uint32_t* tiles, uint32_t n_tiles) {
    if (!h) { g_err = "null handle"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    if (int rc = flush_pending(h)) return rc;
    int rc = render_impl(h, first, n, seed, tiles, n_tiles, h->stream, false);
    if (rc) return rc;
    return rtg_synchronize(h);
}

int rtg_render_idle(rtg_handle* h, int* idle) {
    if (!h || !idle) { g_err = "rtg_render_idle: null argument"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    if (int rc = flush_pending(h)) return rc;  // queued calls not issued yet are work left
    *idle = 1;
    if (h->last_fold) {
        const hipError_t e = hipEventQuery(h->last_fold);
        if (e == hipErrorNotReady) *idle = 0;
        else if (e != hipSuccess) { g_err = std::string("rtg_render_idle: ") + hipGetErrorString(e); return RTG_ERR_HIP; }
    }
    if (*idle) {
        const hipError_t e = hipStreamQuery(h->stream);
        if (e == hipErrorNotReady) *idle = 0;
        else if (e != hipSuccess) { g_err = std::string("rtg_render_idle: ") + hipGetErrorString(e); return RTG_ERR_HIP; }
    }
    return RTG_OK;
}

int rtg_render_adaptive(rtg_handle* h, uint32_t first, uint64_t seed, uint32_t init_samples, uint32_t max_samples,
                        uint32_t min_samples, uint32_t* tile_samples) {
    if (!h || init_samples == 0) { g_err = "rtg_render_adaptive: bad argument"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    if (int rc0 = join_frames(h)) return rc0;
    hipStream_t st = h->stream;
    const size_t nf = (size_t)h->W * h->H * 3;
    const uint32_t spp0 = h->spp;
    const int TS = 32;
    const uint32_t tx = (h->W + TS - 1) / TS, ty = (h->H + TS - 1) / TS, nt = tx * ty;
    float* d_tmp = nullptr;
    HIPOK(hipMalloc((void**)&d_tmp, nf * sizeof(float)));
    float* d_keep = h->d_film;
    auto fail = [&](int rc) { h->d_film = d_keep; (void)hipFree(d_tmp); h->spp = spp0; return rc; };
    // ---- pass 1 (adaptiveSampling, Renderer.h:583-638): per-pixel sums of init_samples samples
    h->d_film = d_tmp;
    if (hipMemsetAsync(d_tmp, 0, nf * sizeof(float), st) != hipSuccess) return fail(RTG_ERR_HIP);
    int rc = render_impl(h, first, init_samples, seed, nullptr, 0, st, false);
    if (rc) return fail(rc);
    std::vector<float> sums(nf);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(sums.data(), d_tmp, nf * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        g_err = "rtg_render_adaptive: pass-1 readback failed";
        return fail(RTG_ERR_HIP);
    }
    std::vector<float> var(nt, 0.0f);
    const float fi = (float)init_samples;
    std::vector<float> est;
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t x0 = (t % tx) * TS, y0 = (t / tx) * TS;
        const uint32_t x1 = std::min<uint32_t>(x0 + TS, h->W), y1 = std::min<uint32_t>(y0 + TS, h->H);
        est.clear();
        for (uint32_t y = y0; y < y1; ++y)
            for (uint32_t x = x0; x < x1; ++x)
                for (int c = 0; c < 3; ++c) est.push_back(sums[((size_t)y * h->W + x) * 3 + c] / fi);
        const int n = (int)(est.size() / 3);
        float gt[3] = {0.0f, 0.0f, 0.0f}, sq[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) gt[c] = gt[c] + est[3 * i + c];
        for (int c = 0; c < 3; ++c) gt[c] = gt[c] / (float)n;
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                const float d = est[3 * i + c] - gt[c];
                sq[c] = sq[c] + d * d;
            }
        var[t] = (((sq[0] + sq[1]) + sq[2]) / 3.0f) / (float)(n - 1);
    }
    float total = 0.0f;
    for (uint32_t t = 0; t < nt; ++t) total += var[t];
    // ---- pass 2 (sampleTileWithWeight, Renderer.h:640-672): tiles grouped by sample count
    std::vector<std::pair<uint32_t, uint32_t>> cnt(nt);  // (samples, tile)
    for (uint32_t t = 0; t < nt; ++t) {
        float w = (total > 0.0f) ? var[t] / total : 0.0f;
        w = std::sqrt(w);
        int smp = (int)(w * (float)max_samples);
        smp = smp > (int)min_samples ? smp : (int)min_samples;
        cnt[t] = {(uint32_t)smp, t};
        if (tile_samples) tile_samples[t] = (uint32_t)smp;
    }
    std::sort(cnt.begin(), cnt.end());
    // every pass-2 sample index must stay inside the PCG key (seq = pixel << 16 | sample): checked
    // before the film is touched
    if (!cnt.empty() && (uint64_t)first + init_samples + cnt.back().first > RTG_MAX_SAMPLES_PER_KEY) {
        g_err = "rtg_render_adaptive: first_sample + init_samples + max tile count exceeds 65536";
        return fail(RTG_ERR_ARG);
    }
    // pass 2 folds into a staged copy of the film, published only when every group succeeded
    float* d_acc = nullptr;
    if (hipMalloc((void**)&d_acc, nf * sizeof(float)) != hipSuccess) { g_err = "rtg_render_adaptive: out of memory"; return fail(RTG_ERR_HIP); }
    auto fail2 = [&](int rc) { (void)hipFree(d_acc); return fail(rc); };
    if (hipMemcpyAsync(d_acc, d_keep, nf * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail2(RTG_ERR_HIP);
    for (size_t i = 0; i < cnt.size();) {
        size_t j = i;
        std::vector<uint32_t> group;
        while (j < cnt.size() && cnt[j].first == cnt[i].first) group.push_back(cnt[j++].second);
        const uint32_t n = cnt[i].first;
        i = j;
        if (n == 0) continue;
        h->d_film = d_tmp;
        if (hipMemsetAsync(d_tmp, 0, nf * sizeof(float), st) != hipSuccess) return fail2(RTG_ERR_HIP);
        if ((rc = render_impl(h, first + init_samples, n, seed, group.data(), (uint32_t)group.size(), st, false))) return fail2(rc);
        h->d_film = d_keep;
        hipLaunchKernelGGL(k_fold_mean, dim3((h->npix + RTG_TB - 1) / RTG_TB), dim3(RTG_TB), 0, st, h->d_pix, h->npix,
                           (const float*)d_tmp, (float)n, d_acc);
        if (hipGetLastError() != hipSuccess) { g_err = "launch k_fold_mean failed"; return fail2(RTG_ERR_HIP); }
    }
    h->d_film = d_keep;
    if (hipMemcpyAsync(d_keep, d_acc, nf * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail2(RTG_ERR_HIP);
    HIPOK(hipStreamSynchronize(st));
    (void)hipFree(d_acc);
    (void)hipFree(d_tmp);
    h->spp = spp0 + 1;  // render(): film->incrementSPP() once per frame
    return RTG_OK;
}

int rtg_launch_times(rtg_handle* h, double* trace_ms, uint32_t max, uint32_t* n) {
    if (!h || !n) return RTG_ERR_ARG;
    *n = (uint32_t)h->launch_ms.size();
    for (uint32_t i = 0; trace_ms && i < std::min<uint32_t>(max, *n); ++i) trace_ms[i] = h->launch_ms[i];
    return RTG_OK;
}

int rtg_launch_rays(rtg_handle* h, uint64_t* rays, uint32_t max, uint32_t* n) {
    if (!h || !n) return RTG_ERR_ARG;
    *n = (uint32_t)h->launch_rays.size();
    for (uint32_t i = 0; rays && i < std::min<uint32_t>(max, *n); ++i) rays[i] = h->launch_rays[i];
    return RTG_OK;
}

}  // extern "C"
