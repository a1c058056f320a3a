/*
 * rtg.h — C-ABI of the MI355X wavefront path tracer (librtg.so).
 *
 * This is the drop-in boundary for RTBase's per-pixel render loop. It replaces, one for one:
 *
 *   RayTracer::render()                 RTBase/Renderer.h:876-885  -> rtg_render()
 *     pathTracerTileBased/getTileID     RTBase/Renderer.h:820-853  (tile selection: tile_ids)
 *     renderTile                        RTBase/Renderer.h:795-818  (pixel centre rays, splat)
 *     pathTrace / computeDirect         RTBase/Renderer.h:328-392, 423-473
 *     Scene::traverse / Scene::visible  RTBase/Scene.h:107-130, 161-169
 *   Film::film / Film::SPP              RTBase/Imaging.h:201-261   -> rtg_film_*()
 *   Film::clear                         RTBase/Imaging.h:252-256   -> rtg_clear()
 *   Sampler::next (per-thread MTRandom) RTBase/Sampling.h:7-26     -> counter-based PCG32 stream
 *                                       keyed by (seed, pixel, sample)
 *
 * Everything above the boundary (scene.json/.gem loading, texture decode, BVH build with its
 * triangle permutation, light list, camera matrices, HDR writing) stays in the host; the host
 * hands over the *flattened reference Scene* below. No C++ or torch types cross this ABI.
 *
 * Conventions: 0 = success, negative = error (rtg_last_error() gives a message, thread-local).
 * A handle owns one GPU's copy of the scene and film; it is not thread-safe (one host thread
 * per handle). Inputs are copied during rtg_create; the caller may free them afterwards.
 */
#ifndef RTG_H
#define RTG_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rtg_scene_desc.projection; 3: rtg_stats.tri_tail_loads / leafbox_tests appended;
 * 4: rtg_render_async queues frames (returns before any of its work has run), rtg_render_idle,
 *    rtg_stats.traced_camera_rays appended;
 * 5: rtg_build_id; the own-tile film exchange (rtg_tile_pixels, rtg_film_gather, rtg_film_scatter),
 *    which rtg_group_reduce now uses in place of a whole-film ncclReduce; rtg_stats.chunk_samples
 * 6: rtg_group_render_async / rtg_group_reduce_async / rtg_group_synchronize (queued group frames);
 *    rtg_film_scatter takes the film's pixel count; rtg_stats.lane_idle_* appended
 *    (additive, still 6: the denoiser, rtg_denoise_* and rtg_group_denoise; camera sampling,
 *    rtg_*_camera_sampling and rtg_probe_camera_samples; environment light sampling,
 *    rtg_*_env_sampling, rtg_env_* and rtg_probe_env_samples; rtg_probe_connect; light selection,
 *    rtg_*_light_sampling, rtg_light_* and rtg_probe_light_pick; its per-cell refinement,
 *    rtg_*_light_grid, rtg_light_grid_* and rtg_probe_light_grid; the material model,
 *    rtg_*_material_model, rtg_*_material_params and rtg_probe_material; path-tracer MIS,
 *    rtg_*_path_mis, rtg_probe_mis_weight, rtg_probe_env_pdf and rtg_light_of_triangle; rough dielectric
 *    transmission, RTG_MODEL_ROUGH_DIELECTRIC and rtg_probe_transmission; a movable camera, rtg_*_camera;
 *    the geometry guide and temporal accumulation, rtg_geometry_guide and rtg_temporal_*; the G-buffer,
 *    rtg_gbuffer and rtg_gbuffer_ms) */
#define RTG_ABI_VERSION 6

/* error codes */
#define RTG_OK              0
#define RTG_ERR_ARG        -1
#define RTG_ERR_HIP        -2
#define RTG_ERR_NO_DEVICE  -3
#define RTG_ERR_NO_LIGHTS  -4
#define RTG_ERR_ALLOC      -5

/* Effective material kinds: RTBase has 8 BSDF classes but only three distinct
 * behaviours plus a pdf quirk. */
#define RTG_MAT_DIFFUSE   0  /* DiffuseBSDF             Materials.h:118-156 (pdf = z>=0 ? z/pi : 0)   */
#define RTG_MAT_LAMBERT   1  /* Conductor/Dielectric/OrenNayar/Plastic stubs (pdf = z/pi, no clamp)  */
#define RTG_MAT_MIRROR    2  /* MirrorBSDF              Materials.h:158-201                          */
#define RTG_MAT_GLASS     3  /* GlassBSDF               Materials.h:252-318 (one-sided)              */

typedef struct rtg_camera {        /* Camera, RTBase/Scene.h:10-70 */
    float inv_proj[16];            /* inverseProjectionMatrix.m (row-major)   */
    float camera[16];              /* camera.m (view -> world)                */
    float origin[3];               /* origin = camera.mulPoint(0,0,0)         */
    float width, height;           /* film size as the reference floats       */
} rtg_camera;

typedef struct rtg_camera_proj {   /* Camera members used by projectOntoCamera / connectToCamera   */
    float proj[16];                /* projectionMatrix.m (Scene.h:22-32, after the flipX negation)  */
    float camera_to_view[16];      /* cameraToView.m = camera.invert() (Scene.h:33-41)             */
    float view_direction[3];       /* viewDirection (Scene.h:38-40)                                */
    float a_film;                  /* Afilm = Wlens * Hlens (Scene.h:28-31)                         */
} rtg_camera_proj;

typedef struct rtg_material {      /* BSDF* + emission, RTBase/Materials.h:94-116 */
    int32_t kind;                  /* RTG_MAT_*                                    */
    int32_t two_sided;             /* BSDF::isTwoSided()                           */
    int32_t texture;               /* albedo Texture* as an index into textures    */
    float int_ior, ext_ior;        /* GlassBSDF::intIOR / extIOR (ignored otherwise) */
    float emission[3];             /* BSDF::emission (isLight iff Lum > 0)         */
} rtg_material;

typedef struct rtg_texture {       /* Texture, RTBase/Imaging.h:16-130 */
    int32_t width, height;
    const float* texels;           /* width*height*3, Colour r,g,b row-major */
} rtg_texture;

typedef struct rtg_scene_desc {    /* Scene after Scene::build(), RTBase/Scene.h:72-106 */
    uint32_t n_tris;               /* triangles in post-BVH-build order (Geometry.h:351 sort)  */
    const float* positions;        /* n_tris*9: vertices[0..2].p                               */
    const float* normals;          /* n_tris*9: vertices[0..2].normal                          */
    const float* uvs;              /* n_tris*6: (u,v) of vertices[0..2]                        */
    const uint32_t* material;      /* n_tris: Triangle::materialIndex                          */
    uint32_t n_nodes;              /* BVHNode tree flattened in DFS pre-order, root = 0        */
    const float* node_bounds;      /* n_nodes*6: bounds.min.xyz, bounds.max.xyz                */
    const int32_t* node_links;     /* n_nodes*4: l, r (-1 = none), startIndex, endIndex        */
    uint32_t n_materials;
    const rtg_material* materials;
    uint32_t n_textures;
    const rtg_texture* textures;
    int32_t env_texture;           /* -1: BackgroundColour(0,0,0); else EnvironmentMap(tex)    */
    uint32_t n_lights;             /* Scene::lights in order                                   */
    const int32_t* lights;         /* -1 = the environment light, else a triangle index        */
    rtg_camera camera;
    rtg_camera_proj projection;    /* light tracing / instant radiosity only (ABI version 2)   */
} rtg_scene_desc;

typedef struct rtg_stats {
    uint64_t paths;                /* camera paths traced                                      */
    uint64_t extension_rays;       /* closest-hit queries (Scene::traverse)                    */
    uint64_t shadow_rays;          /* any-hit queries (Scene::visible)                         */
    uint64_t node_visits;          /* RTG_OPT_COUNT: box tests by closest-hit rays             */
    uint64_t tri_tests;            /* RTG_OPT_COUNT: triangle tests by closest-hit rays        */
    uint64_t shadow_node_visits;   /* RTG_OPT_COUNT: box tests by any-hit rays                 */
    uint64_t shadow_tri_tests;     /* RTG_OPT_COUNT: triangle tests by any-hit rays            */
    uint64_t extend_launches;      /* RTG_OPT_TIMING: traversal launches in the last call      */
    double   render_ms;            /* device time of the last rtg_render call                  */
    double   extend_ms;            /* RTG_OPT_TIMING: traversal kernel time, extension + shadow */
                                   /* rays (one k_trace launch per bounce; last call)          */
    double   shadow_ms;            /* unused since shadow rays share the traversal launches (0) */
    double   shade_ms;             /* device time spent in generate/shade/accumulate kernels   */
    uint64_t lane_slots;           /* RTG_OPT_COUNT: closest-hit loop iterations x 64 lanes     */
    uint64_t node_lane_steps;      /* RTG_OPT_COUNT: lanes doing a node step, summed            */
    uint64_t leaf_lane_steps;      /* RTG_OPT_COUNT: lanes doing a leaf step, summed            */
    uint64_t leaf_phase_slots;     /* RTG_OPT_COUNT: leaf-phase iterations x 64 lanes           */
    uint64_t pops;                 /* RTG_OPT_COUNT: closest-hit stack pops                     */
    uint64_t cullable_pops;        /* RTG_OPT_COUNT: pops whose entry distance was > the hit    */
    uint64_t tri_tail_loads;       /* RTG_OPT_COUNT: triangle records whose last 16 B were fetched */
                                   /* (the plane distance was a candidate), all rays             */
    uint64_t leafbox_tests;        /* RTG_OPT_COUNT: reference leaf-box records fetched, all rays */
    uint64_t traced_camera_rays;   /* path tracer: camera rays traced. renderTile's camera ray is the   */
                                   /* pixel centre's for every sample (Renderer.h:805-808), so a chunk  */
                                   /* traces one per pixel and its samples share the first hit;         */
                                   /* extension_rays counts one per sample, as the reference casts them */
                                   /* (rtg_set_camera_sampling with a filter or a lens: one per path)   */
    uint64_t chunk_samples;        /* samples per pixel of the largest wavefront chunk issued since the */
                                   /* last rtg_clear (ABI 5): the chunk shape of the render           */
    /* RTG_OPT_COUNT (ABI 6): lanes not stepping a node in a traversal loop iteration, by reason,   */
    /* summed like node_lane_steps (lane_slots = node_lane_steps + these five)                      */
    uint64_t lane_idle_no_ray;       /* no ray: waiting for the wave's refill                        */
    uint64_t lane_idle_last_leaf;    /* walk done, its parked leaf waiting for the wave's leaf phase */
    uint64_t lane_idle_leaf_blocked; /* reached a leaf while its parked-leaf slots are full (two)    */
    uint64_t lane_idle_retiring;     /* ray finished, retired at the next iteration                  */
    uint64_t lane_idle_leaf_popped;  /* popped a leaf last iteration; parked in this one             */
} rtg_stats;

typedef struct rtg_handle rtg_handle;

int32_t     rtg_abi_version(void);
/* Hash of the sources, headers and compile flags this library was built from (build.py
 * source_hash("device")): a test or smoke run checks it against the tree it runs in. */
const char* rtg_build_id(void);
const char* rtg_last_error(void);
int         rtg_device_count(int* count);

/* Upload the scene to device `device` (HBM); allocates the film (width*height RGB float). */
int  rtg_create(int device, const rtg_scene_desc* desc, rtg_handle** out);
void rtg_destroy(rtg_handle* h);

/* Tracing options. max_depth is RTBase's MAX_DEPTH (Renderer.h:20, default 4): a path has at
 * most max_depth+2 closest-hit segments. flags: RTG_OPT_CULL enables the conservative distance
 * culling (without it traversal visits exactly the reference's node set: verification mode);
 * RTG_OPT_COUNT runs the counting kernels (node / triangle tests in rtg_stats);
 * RTG_OPT_TIMING records HIP events around every launch (per-kernel-class ms in rtg_stats; launches
 * of chunks running side by side in the frame pipeline each count their shared time);
 * RTG_OPT_BVH2 forces the reference BVH2 walk (no 4-wide collapse; verification / A-B).
 * max_paths_in_flight bounds the paths of one wavefront chunk (0 = keep, default 1G; a chunk's path
 * state is also held to half the free HBM). */
#define RTG_OPT_CULL   1
#define RTG_OPT_COUNT  2
#define RTG_OPT_TIMING 4
#define RTG_OPT_BVH2   8
#define RTG_OPT_WAVETIME 16  /* diagnostic builds only (RTG_DEBUG=1): per-wave clocks of k_trace on stderr */
#define RTG_OPT_SERIAL  32   /* one chunk in flight at a time, every k_shade grid sized from the live counts
                                read back during the traversal (verification / A-B of the frame pipeline) */
#define RTG_OPT_NO_COALESCE 64  /* queued calls (rtg_render_async, no stream) are issued one by one */
int  rtg_set_options(rtg_handle* h, int max_depth, int flags, uint32_t max_paths_in_flight);

/* Per-pixel estimator (the alternative RayTracer methods of Renderer.h). PATH is RayTracer::render's
 * pathTrace (Renderer.h:328-392, the default). DIRECT = RayTracer::direct (:393-407): emission or one
 * NEE sample at the first hit, 0 on a miss. ALBEDO = RayTracer::albedo (:558-571): emission,
 * BSDF::evaluate(sd, (0,1,0)) or the background. NORMALS = RayTracer::viewNormals (:572-582):
 * |shading normal| at the first hit. DIRECT_MIS = RayTracer::direct with computeDirectMIS
 * (:474-557) in place of computeDirect: one light sample and one BSDF sample combined by the
 * balance heuristic (the reference defines it but never calls it). */
#define RTG_INTEGRATOR_PATH       0
#define RTG_INTEGRATOR_DIRECT     1
#define RTG_INTEGRATOR_ALBEDO     2
#define RTG_INTEGRATOR_NORMALS    3
#define RTG_INTEGRATOR_DIRECT_MIS 4
int  rtg_set_integrator(rtg_handle* h, int integrator);

/* ---- camera sampling: pixel-filter jitter and a thin-lens aperture (DESIGN.md "Camera sampling").
 * renderTile sends every sample of a pixel through the pixel centre of a pinhole camera; that is
 * the default here (RTG_FILTER_NONE, lens_radius 0), with one camera ray traced per pixel and
 * shared by its samples. With a filter or a lens, every sample gets a camera ray of its own.
 * Filter importance sampling: sample s of pixel (x, y) crosses the film at
 * (x + 0.5 + dx, y + 0.5 + dy), the offset drawn from the filter's own density, and is added with
 * weight 1 to pixel (x, y) alone (no splat to neighbours), so the sample-order fold, chunking, tiles
 * and queued frames stay invisible in the film's bits. The draws come from a PCG32 stream of their
 * own, pcg_seed(seed ^ 0x9E3779B97F4A7C15, pcg_inc(pixel, sample)), four in order and always all
 * four: u0 (x), u1 (y), u2, u3 (lens); the path's own stream draws what it draws without them.
 * IEEE float32 in the order written, no contraction:
 *   RTG_FILTER_BOX   d = (u * 2.0f - 1.0f) * r                                   (default r 0.5)
 *   RTG_FILTER_TENT  t = u < 0.5f ? sqrtf(2.0f * u) - 1.0f : 1.0f - sqrtf(2.0f - 2.0f * u),
 *                    d = t * r                                                   (r 1 is the usual tent)
 *   px = ((float)x + 0.5f) + dx, py likewise; Camera::generateRay's arithmetic on (px, py) gives the
 *   normalised direction d from the origin o.
 * filter_radius must be finite and in [0, RTG_FILTER_MAX_RADIUS]. (No Gaussian: sampling it needs
 * logf or an inverse erf, which include/rtg_math.h does not restate.)
 * Thin lens, lens_radius R >= 0 (finite; 0 = pinhole), focal_distance f finite and > 0 whenever
 * R > 0. With xc, yc, zc the first three columns of camera.m and dot(a, b) = (ax bx + ay by) + az bz:
 *   ft = f / fabsf(dot(d, zc));  P = o + d * ft  (component-wise)            the point in focus
 *   rr = R * sqrtf(u2);  (s, c) = sincosf(6.2831855f * u3)                   include/rtg_math.h's
 *   o' = (o + xc * (rr * c)) + yc * (rr * s);  d' = (P - o') * (1.0f / sqrtf(|P - o'|^2))
 * The setting applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls, for
 * every integrator of rtg_set_integrator. It does not apply to rtg_render_light (no camera rays), to
 * rtg_render_instant_radiosity's camera pass, or to the denoiser's guides (one centre / pinhole
 * sample each: rtg_denoise saves and restores the setting, as it does the integrator).
 * rtg_set_camera_sampling first issues and waits for queued frames; an argument error leaves the
 * previous setting in place. In per-sample mode rtg_stats.traced_camera_rays counts one ray per
 * path, and rtg_launch_rays' launch 0 is the chunk's paths. */
#define RTG_FILTER_NONE 0
#define RTG_FILTER_BOX  1
#define RTG_FILTER_TENT 2
#define RTG_FILTER_MAX_RADIUS 4.0f
typedef struct rtg_camera_sampling {
    int32_t filter;                /* RTG_FILTER_* */
    float filter_radius, lens_radius, focal_distance;
} rtg_camera_sampling;
int  rtg_camera_sampling_defaults(rtg_camera_sampling* p);  /* NONE, 0.5f, 0, 1 */
int  rtg_set_camera_sampling(rtg_handle* h, const rtg_camera_sampling* p);
int  rtg_get_camera_sampling(rtg_handle* h, rtg_camera_sampling* p);
/* The generate kernel's own function on n (pixel, sample) pairs under the handle's setting: rays
 * n*8 (o.xyz, 0, d.xyz, 0: the layout rtg_trace_closest takes), film_xy n*2 (px, py) or NULL.
 * A pixel >= width*height or a sample >= RTG_MAX_SAMPLES_PER_KEY: RTG_ERR_ARG. */
int  rtg_probe_camera_samples(rtg_handle* h, const uint32_t* pixels, const uint32_t* samples, uint32_t n,
                              uint64_t seed, float* rays, float* film_xy);

/* ---- environment light sampling (rtg_env.hip). EnvironmentMap::sample draws every NEE
 * direction towards the environment uniformly over the sphere (Lights.h:143-149; the reference leaves
 * luminance weighting as an assignment, :160). That is the default here, RTG_ENV_UNIFORM, untouched:
 * the same kernels, draws and bits. RTG_ENV_LUMINANCE draws (wi, pdf) from a piecewise-constant density
 * proportional to the map's filtered luminance times sin theta, through an alias table (one 16-byte
 * load per sample). Definition, for a W x H environment texture (N = W * H cells):
 *   cell (cx, cy)  the (u, v) with u W in [cx, cx+1), v H in [cy, cy+1): the footprint in which
 *                  Texture::sample (Imaging.h:72-94) blends texels (cx, cy), (cx+1 mod W, cy),
 *                  (cx, cy+1 mod H), (cx+1 mod W, cy+1 mod H)
 *   weight         w = (double)m * sin(pi * (cy + 0.5) / H) in binary64 (pi = M_PI, the product first),
 *                  m = the maximum over those four texels of Colour::Lum =
 *                  ((0.2126f r) + (0.7152f g)) + (0.0722f b) in float32, a negative or non-finite Lum
 *                  counting as 0. The maximum makes the density positive wherever the bilinear lookup
 *                  can return light (the estimator stays unbiased); a per-texel luminance would leave
 *                  the cell beside a bright texel at zero density.
 *   sum            the weights added in index order (k = cy * W + cx) in binary64
 *   table          N entries {prob (float), alias (uint32), cellpdf_self (float), cellpdf_alias (float)},
 *                  cellpdf_k = (float)(((w_k / sum) * N) / ((2.0 * pi) * pi)), built by Vose's algorithm
 *                  in binary64 (p_k = (w_k / sum) * N; prob is its keep probability rounded to float);
 *                  for every cell i, prob_i / N + sum over {j: alias_j = i} of (1 - prob_j) / N is
 *                  w_i / sum (to binary64 rounding before prob is rounded to float, which moves it by
 *                  at most 2^-25 / N per entry involved); a zero-weight cell has prob == 0 exactly.
 *   draws          the environment branch of the light sample takes four draws from the path's own PCG
 *                  stream, in this order and always all four: r0, the raw 32-bit output of a PCG step,
 *                  then d1, d2, d3, floats in [0, 1) as every other draw. (The uniform branch keeps its
 *                  two, so the two modes' path streams differ after the first environment sample.)
 *   sample         k = (uint32)(((uint64)r0 * N) >> 32); e = table[k]; keep = d1 < e.prob;
 *                  c = keep ? k : e.alias; cp = keep ? e.cellpdf_self : e.cellpdf_alias;
 *                  cx = c % W, cy = c / W; u = ((float)cx + d2) / (float)W; v = ((float)cy + d3) / (float)H;
 *                  theta = 3.14159265f * v; phi = 6.2831855f * u; (st, ct) = sincosf(theta),
 *                  (sp, cp') = sincosf(phi) of include/rtg_math.h; wi = (st * cp', ct, st * sp), the
 *                  inverse of EnvironmentMap::evaluate's (atan2f(z, x), acosf(y)); pdf = cp / st.
 *                  !(st > 0) or !(pdf > 0): the sample contributes nothing (no shadow ray).
 *                  IEEE float32 in the order written, no contraction. The radiance stays the one
 *                  EnvironmentMap::evaluate(wi), and the shadow ray and Ld = f E g / (pmf pdf) stay as
 *                  they are (pmf = 1 / n_lights, or the picked light's under rtg_set_light_sampling;
 *                  no MIS with BSDF-sampled environment hits).
 *   DIRECT_MIS     computeDirectMIS keeps its structure (Renderer.h:474-557): pdf is the one variable
 *                  the light sample sets and the BSDF half reads. A visible environment sample returns
 *                  f E g / (pmf pdf) at once, unweighted, as in uniform mode. Otherwise (rejected, g = 0
 *                  or occluded) the BSDF sample follows with pdf as the sampler left it: the table's
 *                  cp / st, or 0 after a rejected sample. A BSDF-sampled emitter hit then weights its
 *                  area light with balance(pdf_b, (pdf pmf) dist^2 / cos), i.e. with the environment
 *                  sample's pdf in the place of an area pdf: per-sample here where uniform mode has
 *                  the constant 1 / (4 pi), and weight 1 after a rejected sample. The quirk is the
 *                  reference's (it reuses the variable), inherited and not designed.
 *   unevenness    the integer cell pick gives each entry floor or ceil of 2^32 / N of the 2^32 values of
 *                  r0: uneven by at most N / 2^32 relative (under 0.05 % for a 2048 x 1024 map).
 * A scene without an environment light, or a map whose weights sum to 0, accepts the mode and keeps
 * sampling uniformly, with the launches it has today. W * H > RTG_ENV_MAX_CELLS: RTG_ERR_ARG
 * (rtg_env_sampling_check is the setter's argument check alone). The table is built on the first
 * RTG_ENV_LUMINANCE setting of a handle (a small kernel takes the footprint maxima from the texels on
 * the device, the host runs Vose and uploads the entries) and is kept until rtg_destroy; every rank
 * of a group builds its own, the same bits. rtg_set_env_sampling first issues and waits for queued
 * frames; an argument error leaves the previous setting in place.
 * The setting applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls, under
 * RTG_INTEGRATOR_PATH, _DIRECT and _DIRECT_MIS (kernels of their own, k_shade_env; the default's are
 * not touched). It does not apply to rtg_render_light and rtg_render_instant_radiosity (their
 * sampleDirectionFromLight / samplePositionFromLight stay uniform) or to the denoiser's guides, which
 * sample no light. */
#define RTG_ENV_UNIFORM   0
#define RTG_ENV_LUMINANCE 1
#define RTG_ENV_MAX_CELLS 16777216u  /* 2^24 */
int  rtg_env_sampling_check(int mode, uint32_t env_width, uint32_t env_height);
int  rtg_set_env_sampling(rtg_handle* h, int mode);
int  rtg_get_env_sampling(rtg_handle* h, int* mode);
/* The active table: *w, *h its size (0, 0 when no table is active: uniform mode, no environment light,
 * a black map), entries (or NULL) w*h*4 32-bit words, build_ms (or NULL) the host time of its build. */
int  rtg_env_table(rtg_handle* h, uint32_t* w, uint32_t* height, float* entries, double* build_ms);
/* The w*h cell weights the active table was built from (RTG_ERR_ARG when none is active). */
int  rtg_env_weights(rtg_handle* h, double* weights);
/* The kernel's own sampling function on n scripted draws (r0[n], d[n*3] = d1, d2, d3) against the
 * active table: out n*4 = wi.xyz, pdf (0 where the sample is rejected). No active table: RTG_ERR_ARG. */
int  rtg_probe_env_samples(rtg_handle* h, const uint32_t* r0, const float* d, uint32_t n, float* out);
/* The host's table builder alone (no device call): Vose on n weights; prob (binary64) and alias per
 * entry, and the n*4 words of the entries as uploaded. Weights summing to 0, n == 0 or
 * n > RTG_ENV_MAX_CELLS: RTG_ERR_ARG. */
int  rtg_env_alias_build(const double* weights, uint32_t n, double* prob, uint32_t* alias, float* entries);

/* ---- light selection for NEE (rtg_light_pick.hip). Scene::sampleLight picks the light
 * of every NEE sample uniformly from the light list, one entry per emissive triangle plus possibly the
 * environment: li = (int)(n_lights * u), pmf = 1 / n_lights (Scene.h:137-138). That is the default
 * here, RTG_LIGHTS_UNIFORM, untouched: the same kernels, draws and bits. RTG_LIGHTS_POWER picks light i
 * with a probability that grows with its emitted power, through an alias table over the light list
 * (one 16-byte load per pick), mixed with the uniform pick by uniform_share (lambda in [0, 1]).
 * Definition, for a light list of n entries:
 *   weights        binary64, in light-list order. Area light i: w_i = (double)Lum(em) * (double)area,
 *                  Lum = Colour::Lum in float32 on the device record's emission,
 *                  ((0.2126f r) + (0.7152f g)) + (0.0722f b), a negative or non-finite value counting
 *                  as 0, and area the float32 the device record holds (rtg_light_records: word 3).
 *                  The environment light: w_env = (2.0 * pi * pi) * R * R * (S / N), S the §8c sum of
 *                  the map's N = W * H cell weights (footprint maximum of Lum times sin theta, added in
 *                  index order; computed whether or not RTG_ENV_LUMINANCE is on, and without building
 *                  the environment's alias table), R = 0.5 * sqrt(dx*dx + dy*dy + dz*dz) half the
 *                  diagonal of the reference root box, from its six float32 bounds widened to
 *                  binary64 ((dx*dx + dy*dy) + dz*dz): the map's flux through the scene's bounding
 *                  sphere over pi, on the footing of area * L for a one-sided diffuse emitter.
 *   pmf            pmf_i = ((1 - lambda) * w_i) / sum + lambda / n in binary64, sum = the weights added
 *                  in index order, lambda = (double)uniform_share.
 *   table          n entries {prob (float), alias (uint32), pmf_self (float), pmf_alias (float)},
 *                  pmf_* = (float)pmf. prob and alias are Vose's algorithm of §8c (the same builder,
 *                  rtg_env_alias.h, in its fixed order, in binary64) run on p_k = pmf_k * n.
 *                  An entry with pmf == 0 has prob == 0 exactly and is named by no alias. For every
 *                  light i, prob_i / n + sum over {j: alias_j = i} of (1 - prob_j) / n is pmf_i (to
 *                  binary64 rounding before prob is rounded to float).
 *   draws          the pick takes two draws from the path's own PCG stream in place of the uniform
 *                  pick's one, always both: r0, the raw 32-bit output of a PCG step, then d1, a float in
 *                  [0, 1) as every other draw.
 *   pick           k = (uint32)(((uint64)r0 * n) >> 32); e = table[k]; keep = d1 < e.prob;
 *                  li = keep ? k : e.alias; pmf = keep ? e.pmf_self : e.pmf_alias.
 *   after it       everything is what it is under the uniform pick with that pmf in 1 / n_lights' place:
 *                  Triangle::sample's r1, r2 or the environment branch's two or four draws (according to
 *                  rtg_set_env_sampling), Ld = f E g / (pmf * pdf), the shadow ray. IEEE float32 in the
 *                  order written, no contraction. A power-mode film is another realisation of the same
 *                  expectation, not the uniform film.
 *   DIRECT_MIS     computeDirectMIS keeps its structure (Renderer.h:474-557), as in §8c: the value that
 *                  travels to the BSDF half is pdf * pmf of the *sampled* light, and a BSDF-sampled
 *                  emitter hit is weighted with it. That is the reference's reuse of the variable,
 *                  inherited and not designed: the BSDF-hit emitter is not looked up for its own pmf.
 *   fallbacks      n_lights == 1, a weight sum of 0 or not finite, or an environment light with R 0 or
 *                  not finite: the mode is accepted, no table is built, and the kernels, draws and bits
 *                  are the uniform pick's.
 * uniform_share defaults to 0.125: it bounds 1 / pmf by 8 n, so a dim light next to a surface cannot
 * produce unbounded weights. A robustness choice, not a measured optimum (DESIGN.md §8d has the error
 * at 0, 0.125 and 0.5). uniform_share outside [0, 1] or NaN, or an unknown mode: RTG_ERR_ARG before any
 * device call, and the previous setting stays. The weights, Vose and the upload run on the first
 * RTG_LIGHTS_POWER setting of a handle and again when uniform_share changes; the table is kept until
 * rtg_destroy; every rank of a group builds its own, the same bits. rtg_set_light_sampling first issues
 * and waits for queued frames.
 * The setting applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls, under
 * RTG_INTEGRATOR_PATH, _DIRECT and _DIRECT_MIS (kernels of their own, k_shade_pick; the default's are
 * not touched), with either environment sampling mode. It does not apply to rtg_render_light and
 * rtg_render_instant_radiosity (their light choice stays uniform), to the denoiser's guides or to
 * RTG_INTEGRATOR_ALBEDO and _NORMALS, which sample no light. */
#define RTG_LIGHTS_UNIFORM 0
#define RTG_LIGHTS_POWER   1
typedef struct rtg_light_sampling {
    int32_t mode;          /* RTG_LIGHTS_* */
    float uniform_share;   /* lambda in [0, 1] */
} rtg_light_sampling;
int  rtg_light_sampling_defaults(rtg_light_sampling* p);  /* {RTG_LIGHTS_UNIFORM, 0.125f} */
int  rtg_set_light_sampling(rtg_handle* h, const rtg_light_sampling* p);
int  rtg_get_light_sampling(rtg_handle* h, rtg_light_sampling* p);
/* The n_lights weights the active table was built from (RTG_ERR_ARG when none is active). */
int  rtg_light_weights(rtg_handle* h, double* weights);
/* The active table: *n its entries (0 when no table is active: uniform mode or a fallback), entries
 * (or NULL) n*4 32-bit words, build_ms (or NULL) the host time of its last build. */
int  rtg_light_table(rtg_handle* h, uint32_t* n, float* entries, double* build_ms);
/* The light records as uploaded, 20 floats per light: v0.xyz area | v1.xyz type bits (0 area, 1
 * environment) | v2.xyz 1/area | geometric normal.xyz - | emission.rgb - . */
int  rtg_light_records(rtg_handle* h, float* out /* n_lights * 20 */);
/* The kernel's own pick on n scripted draws against the active table: li[n], pmf[n]. No active table:
 * RTG_ERR_ARG. */
int  rtg_probe_light_pick(rtg_handle* h, const uint32_t* r0, const float* d1, uint32_t n, int32_t* li, float* pmf);
/* The host's builder alone (no device call): pmf, Vose's prob (binary64) and alias per entry, and the
 * n*4 words of the entries as uploaded. n == 0, a negative or non-finite weight, weights summing to 0 or
 * to a non-finite value, uniform_share outside [0, 1] or NaN: RTG_ERR_ARG. */
int  rtg_light_pick_build(const double* weights, uint32_t n, double uniform_share, double* pmf, double* prob,
                          uint32_t* alias, float* entries);

/* ---- per-shading-point light selection (rtg_light_grid.hip). RTG_LIGHTS_POWER's pmf is the
 * same at every shading point. rtg_set_light_grid refines it: with RTG_LIGHTS_POWER active and cells != 0,
 * the pmf of a pick is the one of the grid cell that holds the shading point, through one alias table per
 * cell in §8d's 16-byte format, so the pick stays one 16-byte load whose base address alone depends on the
 * point. Default off (cells = 0): nothing changes unless rtg_set_light_grid is called.
 * Definition, for a light list of n entries and lambda = (double)uniform_share of rtg_set_light_sampling:
 *   grid           the box is the reference root box, six float32 values widened to binary64, lo_a, hi_a,
 *                  e_a = hi_a - lo_a per axis a, E = the largest e_a. dims_a = max(1, (int)ceil((double)cells *
 *                  (e_a / E))), and 1 on a degenerate axis (e_a not > 0; all three when E is not > 0). The
 *                  kernel's constants are float32: lo_a as given, and scale_a = (float)dims_a / (hi_a - lo_a),
 *                  one float32 subtraction and one float32 division, 0 on a degenerate axis.
 *   cell of x      device, float32, no contraction: u = (x_a - lo_a) * scale_a; i_a = (int)u clamped to
 *                  [0, dims_a - 1], a NaN giving 0; c = (i_z * dims_y + i_y) * dims_x + i_x.
 *   weights        host, binary64, the operations in the order written. w_i is §8d's weight of light i,
 *                  unchanged. s_a = e_a / dims_a; cell (i_x, i_y, i_z) has the box clo_a = lo_a + i_a * s_a,
 *                  chi_a = lo_a + (i_a + 1) * s_a.
 *                  Area light: tlo_a, thi_a the smallest and largest of the a coordinates of the triangle's
 *                  three float32 vertices; d_a = max(0, tlo_a - chi_a, clo_a - thi_a); d2 = (d_x*d_x +
 *                  d_y*d_y) + d_z*d_z; r2 = 0.25 * ((s_x*s_x + s_y*s_y) + s_z*s_z); g = 1 / max(d2, r2).
 *                  Facing: the emitter is one-sided. With the cell's box widened by s_a / 2 on every side
 *                  (clo_a - s_a / 2, chi_a + s_a / 2), if none of its eight corners k has
 *                  ((k_x - v0_x)*gn_x + (k_y - v0_y)*gn_y) + (k_z - v0_z)*gn_z > 0 (v0 and the geometric
 *                  normal gn from the light record), then g = 0. The half cell of slack keeps a point that
 *                  float32 arithmetic puts in a neighbouring cell from meeting a pmf that should not be zero
 *                  at lambda = 0.
 *                  Environment light: g = 1 / (R * R) in every cell, R as in §8d; its weight per cell is
 *                  then 2 pi^2 S / N, on the footing of power over squared distance.
 *                  w_ic = w_i * g.
 *   per cell       pmf_ic = ((1 - lambda) * w_ic) / sum_c + lambda / n, sum_c = the w_ic added in light order.
 *                  A cell whose sum is 0 or not finite gets the uniform table: prob 1, alias self, pmf
 *                  (float)(1.0 / n). Otherwise §8d's Vose (rtg_env_alias.h, in its fixed order) on p_k =
 *                  pmf_k * n. Entries {prob, alias, pmf_self, pmf_alias} at table[c * n + k].
 *   pick           draws, order and count are the power pick's, r0 then d1: li = light_pick(table + c * n,
 *                  n, r0, d1, pmf), c the cell of the hit point x the NEE sample is drawn for. Everything
 *                  after the pick is unchanged; DIRECT_MIS keeps the reference's reuse of pdf * pmf of the
 *                  sampled light (§8d).
 * The setting is stored whatever the light mode; the tables are built when it and RTG_LIGHTS_POWER are both
 * set and the power mode has a table (a fallback of §8d, one light or no power, leaves no grid either),
 * rebuilt when cells or uniform_share changes, and kept until rtg_destroy. cells above 64, or a grid of more
 * than 2^24 entries (dims_x * dims_y * dims_z * n_lights, 256 MB) for the handle's root box: RTG_ERR_ARG before
 * any device call, the message naming the largest admissible cells, and the previous setting stays.
 * rtg_light_grid_check has no scene and refuses what no box admits: cells above 64, or cells * n_lights (the
 * thinnest grid, cells x 1 x 1) above 2^24. A build that fails on the device (RTG_ERR_HIP, from either
 * setter) leaves no grid, and frames run the power pick. A hierarchy for
 * longer light lists is not covered. rtg_set_light_grid first issues and waits for queued frames.
 * It applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls under
 * RTG_INTEGRATOR_PATH, _DIRECT and _DIRECT_MIS with the reference material model and either environment
 * mode (kernels of their own, k_shade_grid). A handle whose frames run k_shade_phys, k_shade_mis or
 * k_shade_trans (RTG_MATERIALS_PHYSICAL with such a record, RTG_PATH_MIS_POWER under PATH) keeps the power
 * pick and its one table: those kernels take their pick as a run-time argument, and a grid there would
 * change them. Not covered either: rtg_render_light, rtg_render_instant_radiosity, the denoiser's guides. */
typedef struct rtg_light_grid {
    uint32_t cells;        /* 0: off (default); else 1..64 cells on the longest axis of the root box */
} rtg_light_grid;
int  rtg_light_grid_defaults(rtg_light_grid* p);  /* {0} */
int  rtg_light_grid_check(const rtg_light_grid* p, uint32_t n_lights);  /* no device needed */
int  rtg_set_light_grid(rtg_handle* h, const rtg_light_grid* p);
int  rtg_get_light_grid(rtg_handle* h, rtg_light_grid* p);
/* dims[3], lo[3], scale[3] as the kernel uses them; *n_entries = cells of the grid * n_lights (0: no grid
 * is active, and the other outputs are 0); build_ms the host time of the last build. Any pointer but h may
 * be NULL. */
int  rtg_light_grid_info(rtg_handle* h, uint32_t* dims, float* lo, float* scale, uint64_t* n_entries, double* build_ms);
/* The active tables, n_entries * 4 32-bit words. No active grid: RTG_ERR_ARG. */
int  rtg_light_grid_table(rtg_handle* h, float* entries);
/* The kernel's own cell and pick for n points (n*3) and scripted draws against the active grid: cell[n],
 * li[n], pmf[n]. No active grid: RTG_ERR_ARG. */
int  rtg_probe_light_grid(rtg_handle* h, const float* points, const uint32_t* r0, const float* d1, uint32_t n,
                          int32_t* cell, int32_t* li, float* pmf);
/* The host's builder alone, binary64, no device call: from n light records (rtg_light_records' layout),
 * their §8d weights and the root box, dims[3], lo[3], scale[3] and (entries may be NULL, to learn dims
 * first) the dims product * n * 4 words. n == 0, cells outside 1..64, more than 2^24 entries, uniform_share
 * outside [0, 1] or NaN: RTG_ERR_ARG. */
int  rtg_light_grid_build(const float* light_records, uint32_t n, const double* weights, const float* root_box,
                          uint32_t cells, double uniform_share, uint32_t* dims, float* lo, float* scale,
                          float* entries);

/* ---- material model (rtg_shade_phys.hip, rtg_phys.h). RTBase's ConductorBSDF, PlasticBSDF
 * and OrenNayarBSDF are stubs that shade as a cosine-sampled Lambertian (RTG_MAT_LAMBERT), and
 * ShadingHelper::Dggx / lambdaGGX / Gggx return 1. That is the default here, RTG_MATERIALS_REFERENCE,
 * untouched: the same kernels, draws and bits. Under RTG_MATERIALS_PHYSICAL a material whose parameter
 * record (rtg_set_material_params, one per rtg_scene_desc.materials entry, in that order) carries the tag
 * RTG_MODEL_CONDUCTOR, _PLASTIC or _ORENNAYAR shades with the model below; a record tagged
 * RTG_MODEL_REFERENCE (diffuse, mirror, glass, and the rough dielectric where the caller leaves it the
 * Lambert stub; RTG_MODEL_ROUGH_DIELECTRIC, further below, gives it its own model) shades as it does by
 * default. Definition, in the local frame of the shading normal (z; the frame is
 * Frame::fromVector's), wo = the direction back along the ray after the two-sided flip, IEEE float32 in
 * the order written, no contraction; pi = (float)M_PI; dot(a, b) = (ax bx + ay by) + az bz:
 *   parameters     alpha = 1.62142f * sqrtf(roughness), formed by the host as the reference's constructors
 *                  form it; sigma = the Oren-Nayar width (scene.json "alpha"); eta, k the conductor's
 *                  complex index per channel; int_ior, ext_ior the plastic coat's.
 *   D(h)           a2 = alpha alpha; t = ((h.z h.z) (a2 - 1)) + 1; D = a2 / ((pi t) t)
 *   Lambda(w)      t2 = ((w.x w.x) + (w.y w.y)) / (w.z w.z); Lambda = (sqrtf(1 + (a2 t2)) - 1) 0.5
 *   G1(w), G       G1 = 1 / (1 + Lambda(w)); G(wi, wo) = G1(wi) G1(wo)
 *   half vector    hs = wo + wi; l2 = dot(hs, hs); inv = 1 / sqrtf(l2); h = hs inv;
 *                  ch = clamp01(0.5 (l2 inv)), the cosine wo.h = wi.h = |wo + wi| / 2 in a form that has
 *                  the same bits with wo and wi swapped (clamp01(x) = max(0, min(x, 1))). !(l2 > 0), i.e.
 *                  wo + wi = 0: the GGX lobe contributes 0 to evaluate and to PDF.
 *   F_c(c)         ShadingHelper::fresnelCondutor (Materials.h:78-91) per channel: cos2 = c c; sin2 = 1 -
 *                  cos2; n2k2 = (eta eta) + (k k); e = (eta 2) c; Fpa2 = (((n2k2 cos2) - e) + sin2) /
 *                  (((n2k2 cos2) + e) + sin2); Fpe2 = ((n2k2 - e) + cos2) / ((n2k2 + e) + cos2);
 *                  F = (Fpa2 + Fpe2) 0.5. A denominator that is not > 0 (eta = k = 0) makes its half 1.
 *   F_d(c)         fresnelDielectric (Materials.h:55-77) at clamp01(c), entering the coat from outside as
 *                  GlassBSDF calls it: iorInt = ext_ior, iorExt = int_ior (its clamp makes a NaN 1).
 *   conductor      evaluate = (albedo F_c(ch)) ((D(h) G(wi, wo)) / ((4 wo.z) wi.z));
 *                  PDF = (G1(wo) D(h)) / (4 wo.z); sample: visible normals (Heitz 2018), draws u1, u2:
 *                  vh = normalize(alpha wo.x, alpha wo.y, wo.z); lensq = (vh.x vh.x) + (vh.y vh.y);
 *                  t1 = lensq > 0 ? (-vh.y il, vh.x il, 0), il = 1 / sqrtf(lensq) : (1, 0, 0);
 *                  t2 = cross(vh, t1); r = sqrtf(u1); (sn, cs) = sincosf(6.2831855f u2) of
 *                  include/rtg_math.h; p1 = r cs; sh = 0.5 (1 + vh.z);
 *                  p2 = ((1 - sh) sqrtf(max(0, 1 - (p1 p1)))) + (sh (r sn));
 *                  p3 = sqrtf(max(0, (1 - (p1 p1)) - (p2 p2))); nh = ((t1 p1) + (t2 p2)) + (vh p3);
 *                  ne = normalize(alpha nh.x, alpha nh.y, max(0, nh.z)); wi = (ne (2 dot(wo, ne))) - wo.
 *   plastic        evaluate = fd + sp on every channel, fd = (albedo / pi) ((1 - F_d(wo.z)) (1 - F_d(wi.z))),
 *                  sp = F_d(ch) ((D G) / ((4 wo.z) wi.z)): an untinted dielectric GGX coat over the
 *                  diffuse base. Three draws, always all three: u0 chooses the lobe, the coat when
 *                  u0 < ps, ps = 0.25 + (0.5 F_d(wo.z)), which lies in [0.25, 0.75], so both lobes are
 *                  sampled wherever they are not zero; the coat takes (u1, u2) as the conductor does, the
 *                  base cosineSampleHemisphere(u2, u1) (the first of the two -> r2, as the Lambert family).
 *                  PDF = (ps pv) + ((1 - ps) (wi.z / M_PI)), pv the conductor's PDF, wi.z / M_PI in
 *                  binary64 rounded to float as cosineHemispherePDF.
 *   Oren-Nayar     s2 = sigma sigma; A = 1 - (s2 / (2 (s2 + 0.33))); B = (0.45 s2) / (s2 + 0.09);
 *                  evaluate = (albedo / pi) (A + ((B max(0, (wi.x wo.x) + (wi.y wo.y))) / max(wi.z, wo.z))):
 *                  the qualitative model with its sin alpha tan beta cos(dphi) reduced to products.
 *                  Sampling and PDF: cosineSampleHemisphere with the Lambert family's two draws in their
 *                  order, PDF = wi.z / M_PI.
 *   sample         returns colour = evaluate(wo, wi) and pdf = PDF(wo, wi), computed by those two functions
 *                  from the sampled wi.
 *   delta lobes    a GGX lobe with alpha < RTG_ALPHA_DELTA is a delta lobe (coffee's plastics have
 *                  roughness 0). The path tracer counts an emitter hit only after a camera or specular
 *                  bounce and by default has no MIS, so a lobe that narrow lit by NEE alone would be all fireflies.
 *                  A delta lobe is left out of evaluate, PDF and NEE; a ray sampled from it reflects about
 *                  the normal, wi = (-wo.x, -wo.y, wo.z), carries canHitLight = 1 and skips the cosine
 *                  factor, as MirrorBSDF does. Conductor: colour = albedo F_c(clamp01(wo.z)), pdf = 1, no
 *                  draws, no NEE at the vertex. Plastic: decided per sample: the coat is chosen as above
 *                  (u0 < ps), colour = F_d(wo.z) on every channel, pdf = ps; the base keeps its NEE and
 *                  its samples (PDF = (1 - ps) (wi.z / M_PI)). 0.01 is roughness below 3.8e-5: a
 *                  robustness choice, not a measured optimum.
 *   guards         evaluate and PDF are 0 unless wo.z > 0 and wi.z > 0. sample with !(wo.z > 0), a sampled
 *                  wi with !(wi.z > 0), or a PDF that is not in (0, FLT_MAX]: pdf = 0 and the path ends at
 *                  this vertex (its NEE term stays), where the reference model would carry a zero
 *                  throughput on. wo + wi = 0: see the half vector.
 *   in the path    NEE: Ld = f E g / (pmf pdf) with f = evaluate(wo, sd), sd the shadow ray's direction
 *                  normalize(p2 - x), in albedo / pi's place; everything else of computeDirect, and the
 *                  light and environment sampling modes, as they are. Bounce: after Russian roulette, thr =
 *                  ((thr colour) |dot(wi, sN)|) / pdf, or (thr colour) / pdf for a delta sample.
 * The setting applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls under
 * RTG_INTEGRATOR_PATH and _DIRECT (kernels of their own, k_shade_phys; the default's are not touched), with
 * either environment and light sampling mode, and only when the scene has a conductor, plastic or
 * Oren-Nayar record: a scene without one keeps today's kernels and bits under both settings. It does not
 * apply to RTG_INTEGRATOR_DIRECT_MIS, _ALBEDO and _NORMALS, to rtg_render_light and
 * rtg_render_instant_radiosity, or to the denoiser's guides: they keep the reference model. Not modelled:
 * LayeredBSDF (rough dielectric transmission is RTG_MODEL_ROUGH_DIELECTRIC, below). (MIS between NEE and BSDF-sampled emitter hits is
 * rtg_set_path_mis, below; RTG_ALPHA_DELTA and the delta-lobe rule are the same under it.)
 * rtg_set_material_params copies n records (n must equal rtg_scene_desc.n_materials);
 * rtg_material_params_check is its argument check alone (no handle, no device call): a null pointer, a
 * wrong n, an unknown tag, or an alpha, sigma, eta, k, int_ior or ext_ior that is negative or not finite
 * is RTG_ERR_ARG. rtg_set_material_model(PHYSICAL) before any parameters were set, or an unknown mode:
 * RTG_ERR_ARG. Argument errors are reported before any device call and leave the previous setting and
 * the film as they were. Both setters first issue and wait for queued frames. The device table (unique
 * records, and one index per triangle, fetched by the hit's triangle id beside its shading record) is
 * built when the mode is first switched on, rebuilt when the parameters change, and kept until
 * rtg_destroy; the default upload is not changed by it. */
#define RTG_MATERIALS_REFERENCE 0
#define RTG_MATERIALS_PHYSICAL  1
#define RTG_MODEL_REFERENCE 0   /* shade by rtg_material.kind, as the default does */
#define RTG_MODEL_CONDUCTOR 1
#define RTG_MODEL_PLASTIC   2
#define RTG_MODEL_ORENNAYAR 3
/* (4 is left unassigned: rtg_material_params_check rejects it) */
#define RTG_MODEL_ROUGH_DIELECTRIC 5   /* rough dielectric transmission, below */
#define RTG_ALPHA_DELTA 0.01f
typedef struct rtg_material_params {
    int32_t model;                 /* RTG_MODEL_* */
    float alpha;                   /* GGX width, 1.62142f * sqrtf(roughness) (conductor, plastic) */
    float sigma;                   /* Oren-Nayar width */
    float eta[3], k[3];            /* conductor */
    float int_ior, ext_ior;        /* plastic, rough dielectric */
} rtg_material_params;
int  rtg_material_params_check(const rtg_material_params* params, uint32_t n, uint32_t n_materials);
int  rtg_set_material_params(rtg_handle* h, const rtg_material_params* params, uint32_t n);
int  rtg_set_material_model(rtg_handle* h, int mode);
int  rtg_get_material_model(rtg_handle* h, int* mode);
/* The kernels' own sample / evaluate / PDF on n scripted cases, on the current device (no handle).
 * cases: n*28 floats (model, alpha, sigma, int_ior, ext_ior, eta[3], k[3], albedo.rgb, sNormal.xyz, wo.xyz,
 * draw[3], query wi.xyz, pad[2]; wo and the query in world space, taken into Frame::fromVector(sNormal));
 * out: n*16 floats (wi.xyz world, colour.rgb, pdf, draws consumed, delta flag, evaluate(query).rgb,
 * PDF(query), pad[3]). A model other than conductor, plastic or Oren-Nayar: RTG_ERR_ARG. */
int  rtg_probe_material(const float* cases, uint32_t n, float* out);

/* ---- rough dielectric transmission (rtg_shade_trans.hip, rtg_trans.h). RTBase's rough
 * DielectricBSDF ("bsdf": "dielectric" with roughness >= 0.001) is a stub that shades as a cosine-sampled
 * Lambertian, and under RTG_MATERIALS_PHYSICAL a record tagged RTG_MODEL_REFERENCE keeps it that way. A
 * record tagged RTG_MODEL_ROUGH_DIELECTRIC (5; 4 is left unassigned) shades with the microfacet refraction
 * model of Walter et al. 2007 on the GGX pieces above: alpha, int_ior and ext_ior are the record's.
 * rth_scene_material_params_transmissive (include/rth.h) hands out the loader's records with that tag;
 * rth_scene_material_params keeps RTG_MODEL_REFERENCE. Definition, in the local frame of the shading
 * normal as above, IEEE float32 in the order written, no contraction, with + - * /, sqrtf and sincosf only:
 *   side           a dielectric is one-sided (rtg_material.two_sided = 0): the shading normal is not flipped
 *                  and wo.z may be negative. s = wo.z > 0; eta_i = s ? ext_ior : int_ior, eta_t the other.
 *                  wo' = s ? wo : -wo and wi' = s ? wi : -wi (all three components), so wo'.z > 0; a
 *                  sampled wi' is mapped back the same way. wo.z == 0 (or not a number): evaluate and PDF
 *                  are 0 and sample ends the path. A two-sided material tagged 5 has its normal flipped
 *                  towards wo at every hit, so s is always true: a sheet that is entered from either side
 *                  and never left.
 *   F_out(c)       fresnelDielectric (Materials.h:55-77) at clamp01(c), c a cosine on the exterior side, with
 *                  iorInt = ext_ior, iorExt = int_ior, as GlassBSDF calls it from outside; total internal
 *                  reflection (an exterior denser than the interior) gives 1.
 *   F(c)           the interface's Fresnel term for a cosine c on wo's side, the same number from both sides:
 *                  s: F_out(c). Otherwise, from inside, at the exterior cosine of Snell's law: cc =
 *                  clamp01(c); r = int_ior / ext_ior; s2 = (r r) (1 - (cc cc)); s2 > 1: 1 (total internal
 *                  reflection); else F_out(sqrtf(1 - s2)). fresnelDielectric's own value from inside is not
 *                  used: its perpendicular term divides by (ior cos_i + ior cos_t) where Fresnel has (ior
 *                  cos_i + cos_t), so it differs between the two sides (0.05125 entering IOR 1.5 at the
 *                  normal, 0.03389 leaving), and a transmission lobe built on it is not reciprocal.
 *   reflection     wi'.z > 0: (h, ch) the half vector of (wo', wi') as above (wo' + wi' = 0: 0);
 *                  f = F(ch) ((D(h) G(wi', wo')) / ((4 wo'.z) wi'.z)); pdf = F(ch) ((G1(wo') D(h)) / (4 wo'.z)).
 *   transmission   wi'.z < 0: hs = -((wo' eta_i) + (wi' eta_t)); l2 = dot(hs, hs) (!(l2 > 0): 0);
 *                  h = hs (1 / sqrtf(l2)), negated when h.z < 0; coh = dot(wo', h); cih = dot(wi', h); the
 *                  lobe is 0 unless coh > 0 and cih < 0. aci = -cih; aiz = -wi'.z; T = 1 - F_out(s ? coh : aci),
 *                  the half vector's cosine on the exterior side itself;
 *                  den = (eta_i coh) + (eta_t cih); den2 = den den; et2 = eta_t eta_t; g1o = G1(wo');
 *                  f = (((coh aci) et2) (T (D(h) (G1(wi') g1o)))) / ((wo'.z aiz) den2);
 *                  pdf = (T (((g1o coh) D(h)) / wo'.z)) ((et2 aci) / den2).
 *                  Walter's form without a radiance-compression factor: the lobe integrates to 1 - F, as
 *                  GlassBSDF's (1 - R) does. wi'.z == 0: 0.
 *   evaluate, PDF  evaluate = albedo f on every channel, PDF = pdf, on the whole sphere.
 *   sample         three draws u0, u1, u2, always all three. m = the visible normal ne of wo' for (u1, u2)
 *                  (the conductor's sampler above up to ne); dm = dot(wo', m); c = clamp01(dm). u0 < F(c):
 *                  wi' = (m (2 dm)) - wo', kept when wi'.z > 0. Otherwise eta = eta_t / eta_i;
 *                  k = 1 - ((1 - (c c)) / (eta eta)); a = (c / eta) - sqrtf(k); wi' = (m a) - (wo' / eta),
 *                  kept when wi'.z < 0. colour = evaluate(wo, wi) and pdf = PDF(wo, wi) by the two functions
 *                  above from the sampled wi. A wi' that is not kept, or a pdf not in (0, FLT_MAX]: pdf = 0
 *                  and the path ends at this vertex (its NEE term stays). A kept sample's weight colour
 *                  |wi.z| / pdf is albedo G1(wi').
 *   delta limit    alpha < RTG_ALPHA_DELTA: GlassBSDF::sample with the record's IORs (the glass branch of
 *                  rtg_probe_bsdf: its draws, wi, colour and pdf bit for bit), a delta sample (no cosine
 *                  factor, canHitLight), no NEE at the vertex; evaluate and PDF are 0. The loader never
 *                  produces it (roughness < 0.001 is RTG_MAT_GLASS already); a caller's record can.
 *   in the path    NEE at a tag-5 vertex: the geometry term takes |dot(wi, sN)| where computeDirect has
 *                  max(dot(wi, sN), 0), for area lights and the environment alike, so a light behind the
 *                  surface is reached through the transmission lobe; f = evaluate(wo, sd); the shadow ray
 *                  starts at x + sd EPS, on the side it leaves by. Bounce: thr = ((thr colour) |dot(wi, sN)|)
 *                  / pdf from x + wi EPS; a non-delta sample does not carry canHitLight. Under
 *                  RTG_PATH_MIS_POWER p_b = PDF(wo, sd) with both lobes, and the sample's pdf travels in
 *                  thr.w; the emitter-hit and miss sites are as they are.
 * With F taken from the exterior side for both directions the transmission lobe is reciprocal up to the
 * squared indices, f_t(a, b) eta_a^2 = f_t(b, a) eta_b^2 (eta_x the index of the medium x lies in): in the
 * two evaluations h, den^2, D and the cosine handed to F_out have the same bits. Radiance is not scaled
 * across the interface. The delta limit is GlassBSDF as it is, with fresnelDielectric's own value per side.
 * The family (k_shade_trans<ALT, TAB> for PATH and DIRECT, k_shade_trans_mis<TAB> for PATH under
 * rtg_set_path_mis; it shades conductor, plastic and Oren-Nayar records as k_shade_phys and k_shade_mis do)
 * is launched only under RTG_MATERIALS_PHYSICAL with RTG_INTEGRATOR_PATH or _DIRECT when the parameter
 * table holds a tag-5 record that some triangle uses; everything else runs what it ran, with its bits, and
 * the exclusions are the material model's: _DIRECT_MIS, _ALBEDO, _NORMALS, rtg_render_light,
 * rtg_render_instant_radiosity and the denoiser's guides keep the reference model. Argument check, beside
 * the material model's: a tag-5 record whose int_ior or ext_ior is not > 0, or whose int_ior equals its
 * ext_ior (the lobe collapses to a delta straight through, which the model does not cover), is RTG_ERR_ARG.
 * Not covered: LayeredBSDF, radiance scaling across the interface, the C oracle, integration/rtg_rtbase.h. */
/* rtg_probe_material for the rough dielectric (rtg_shade_trans.hip): that probe's layout in and out, int_ior
 * and ext_ior the record's, wo and the query anywhere on the sphere. A model other than
 * RTG_MODEL_ROUGH_DIELECTRIC: RTG_ERR_ARG. */
int  rtg_probe_transmission(const float* cases, uint32_t n, float* out);

/* ---- multiple importance sampling of emitters in the path tracer (rtg_shade_mis.hip,
 * rtg_mis.h). pathTrace (Renderer.h:328-392) counts an emitter hit only after a camera or specular bounce,
 * so after any other bounce NEE alone lights the vertex, and on a miss it returns
 * background->evaluate(r.dir) without the path throughput at any depth (:390), so with the environment in
 * the light list it is counted twice after a diffuse bounce, once unweighted. That is the default here,
 * RTG_PATH_MIS_OFF, untouched: the same kernels, draws and bits. RTG_PATH_MIS_POWER combines the NEE
 * sample and the BSDF sample of every non-specular vertex with the power heuristic, and weighs a miss by
 * the throughput: it DELIBERATELY DEPARTS from Renderer.h:390, and is the project's correct path
 * estimator under an environment light. On a scene whose environment is not a light and whose emissive
 * triangles are all in the light list both settings have the same expectation; on an environment-lit
 * scene they do not, and the default is the one that is off. Definition, IEEE float32 in the order
 * written, no contraction:
 *   the path     draws exactly what PATH draws, in the same order (light pick, light sample, Russian
 *                roulette, BSDF sample; no other random numbers), so a film follows the paths of the PATH
 *                film of the same seed and only the weights differ.
 *   mis_w(p, q)  r = q / p; w = 1 / (1 + (r r)): the power heuristic with beta = 2 for a sample of density
 *                p against a technique of density q, in a form that cannot come to inf / inf for a finite
 *                p > 0. A w that is not a number (both densities 0, or both infinite) is 0.5, on both
 *                sides of the pair.
 *   NEE          at a non-specular vertex whose light sample has g > 0, computeDirect's Ld = f E g /
 *                (pmf pdf) is multiplied on every channel by mis_w(p_l, p_b). Area light:
 *                p_l = convertPDFAreaToSolidAngle(pmf pdf, l2, cos_l) = cos_l > 0 ? ((pmf pdf) l2) / cos_l
 *                : 0, with l2 and cos_l the squared distance and the light's cosine that form g.
 *                Environment light: p_l = pmf pdf. pmf is the pick's (1 / n_lights, or the table entry's
 *                under RTG_LIGHTS_POWER). p_b = BSDF::PDF(wo, sd), sd the shadow ray's direction
 *                normalize(p2 - x): cosineHemispherePDF (dot(sd, frame.w) >= 0 ? that / M_PI in binary64 :
 *                0) for a reference-kind record, PDF(wo, sd) of the material model above for a physical
 *                one (for a plastic with a delta coat: the base's share, (1 - ps) (wi.z / M_PI)).
 *   BSDF sample  its solid-angle pdf travels to the next vertex (path payload thr.w); a specular or delta
 *                sample carries canHitLight and weight 1, as does the camera ray. A sample whose pdf is not
 *                > 0 (a cosine sample on the horizon, wi.z = 0) ends the path at this vertex (its NEE term
 *                stays), for a reference-kind record as the material model's guard does for a physical
 *                one: PATH carries the throughput 0 / 0 on, which only a later visible NEE sample shows,
 *                while this mode's thr E on a miss would show it every time.
 *   emitter hit  with canHitLight: thr emission, as PATH. Otherwise, with i the hit triangle's index in
 *                the light list, L its light record, t the hit distance, d the ray's direction and
 *                cos_l = max(-dot(d, L.gNormal), 0): cos_l > 0: (thr emission) mis_w(p_b, p_l),
 *                p_l = convertPDFAreaToSolidAngle(pmf_i (1 / area_i), t t, cos_l), pmf_i = 1 / n_lights or
 *                entry i's own pmf under RTG_LIGHTS_POWER; the back side (cos_l = 0): 0, as PATH gives,
 *                for NEE cannot reach it either. An emissive triangle that is not in the light list
 *                contributes thr emission: no NEE sample can ever reach it. A triangle listed twice counts
 *                as its first entry.
 *   miss         bounce 0: E = background->evaluate(d). After a specular or delta sample: thr E. After
 *                any other sample: (thr E) mis_w(p_b, pmf_env p_env(d)) when the environment is in the
 *                light list (pmf_env as pmf_i), thr E when it is not.
 *   p_env(d)     RTG_ENV_UNIFORM (or no table): 1 / (4 pi), uniformSpherePDF. RTG_ENV_LUMINANCE: with
 *                (u, v) EnvironmentMap::evaluate's own coordinates of d (atan2f(d.z, d.x), plus 2 pi in
 *                binary64 when negative, over 2 pi; acosf(d.y) over pi), fx = floorf(u w), fy = floorf(v h),
 *                the cell (cx, cy) = (fx, fy) clamped to [0, w - 1] x [0, h - 1] (not a number: 0), cp that
 *                cell's own cellpdf (word 2 of entry cy w + cx), st = sqrtf((d.x d.x) + (d.z d.z)):
 *                !(st > 0) ? 0 : cp / st. For a direction the sampler produced from in-cell draws away
 *                from the cell's edges this is the sampler's own pdf up to the rounding of st (a few units
 *                in the last place).
 * The setting applies to rtg_render, rtg_render_async, rtg_render_adaptive and the group calls under
 * RTG_INTEGRATOR_PATH only (kernels of their own, k_shade_mis; the default's are not touched), with either
 * environment mode, light selection mode and material model and with camera sampling. It does not apply
 * to RTG_INTEGRATOR_DIRECT, _DIRECT_MIS, _ALBEDO and _NORMALS, to rtg_render_light and
 * rtg_render_instant_radiosity, or to the denoiser's guides: they keep today's kernels and bits under
 * either setting. A rough dielectric record (RTG_MODEL_ROUGH_DIELECTRIC) is covered: p_b is its PDF with both
 * lobes. Not covered: LayeredBSDF, per-shading-point light selection (rtg_set_light_grid leaves this mode the power pick), a lower RTG_ALPHA_DELTA. The setter first issues and waits for queued frames; an unknown
 * mode is RTG_ERR_ARG, reported before any device call, with the setting and the film left as they were
 * (rtg_path_mis_check is that check alone). The triangle -> light map (int32 per triangle, -1: no light)
 * is built on the host from the light list when the mode is first switched on and kept until
 * rtg_destroy; on the device it stands beside the triangle's parameter record index (one 8-byte load by
 * the hit's triangle id, beside its shading record), so it is uploaded again when rtg_set_material_params
 * rebuilds that index. The default upload is not changed by it. */
#define RTG_PATH_MIS_OFF   0
#define RTG_PATH_MIS_POWER 1
int  rtg_path_mis_check(int mode);
int  rtg_set_path_mis(rtg_handle* h, int mode);
int  rtg_get_path_mis(rtg_handle* h, int* mode);
/* The kernels' own weight function on n pairs, on the current device (no handle): w[i] = mis_w(p[i], q[i]). */
int  rtg_probe_mis_weight(const float* p, const float* q, uint32_t n, float* w);
/* The solid-angle density the handle's environment mode gives n directions (p_env above; under
 * RTG_ENV_UNIFORM, or when no table is active, uniformSpherePDF). */
int  rtg_probe_env_pdf(rtg_handle* h, const float* dirs /* n*3 */, uint32_t n, float* pdf);
/* The host copy of the triangle -> light map. Before the first RTG_PATH_MIS_POWER setting: RTG_ERR_ARG. */
int  rtg_light_of_triangle(rtg_handle* h, int32_t* out /* n_triangles */);

/* ---- the sampler: where a path's and a camera sample's random numbers come from (DESIGN.md §8m;
 * rtg_sampler.h). RTG_SAMPLER_PCG, the default, untouched: one PCG32 stream per (pixel, sample), white
 * noise. RTG_SAMPLER_SOBOL: Burley's hash-based Owen-scrambled Sobol sequence (JCGT 2020, "Practical
 * Hash-Based Owen Scrambling"), padded 4-D: each consecutive group of four draws of a path is one point of
 * a 4-D Sobol sequence indexed by the pixel's sample number, shuffled and scrambled with a hash seed of the
 * group's own, so the samples of a pixel are stratified against each other in every group, whatever the
 * chunking, tiling, queuing or rank split. It changes no estimator, only where the numbers come from: a
 * film stays a deterministic function of (pixel, sample, seed). Definition; all arithmetic is uint32 with
 * wrap-around, brev is a 32-bit bit reversal:
 *   mix32(x):   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   lk(x, s):   x += s; x ^= x * 0x6c50b47c; x ^= x * 0xb82f1e52; x ^= x * 0xc7afe638; x ^= x * 0x8d22f6e6
 *   owen(x, s): brev(lk(brev(x), s))
 *   key(pixel, seed, stream) = mix32(pixel ^ mix32((uint32)seed ^ mix32((uint32)(seed >> 32) ^ stream)))
 *        stream: 0 for the path, 0x9E3779B9 for the camera sample (the PCG mode keys its camera stream
 *        apart too)
 *   draw n of (pixel, sample):   g = n >> 2,  c = n & 3
 *        gs  = mix32(key ^ (g * 0x9E3779B9))
 *        idx = owen(sample, gs) & 0xFFFF            (the sample number enters by its low 16 bits)
 *        X   = owen(sobol_c(idx), mix32(gs + (c + 1) * 0x85EBCA6B))
 *        sobol_c(idx) = XOR over the set bits b < 16 of idx of D_c[b];   D_0[b] = 0x80000000 >> b
 *   raw 32-bit draw = X  (where the body uses pcg_step's output: the alias picks' r0)
 *   float draw      = (float)(X >> 8) * 2^-24       (exactly pcg_next's conversion)
 * D_1, D_2, D_3 are the Joe-Kuo direction words of dimensions 2, 3 and 4 (polynomial degree / a / m =
 * 1/0/(1), 2/1/(1,3), 3/1/(1,3,1); the standard recurrence with v_i = m_i << (31 - i)); the first 16 of each:
 *   D_1 = 80000000 c0000000 a0000000 f0000000 88000000 cc000000 aa000000 ff000000
 *         80800000 c0c00000 a0a00000 f0f00000 88880000 cccc0000 aaaa0000 ffff0000
 *   D_2 = 80000000 c0000000 60000000 90000000 e8000000 5c000000 8e000000 c5000000
 *         68800000 9cc00000 ee600000 55900000 80680000 c09c0000 60ee0000 90550000
 *   D_3 = 80000000 c0000000 20000000 50000000 f8000000 74000000 a2000000 93000000
 *         d8800000 25400000 59e00000 e6d00000 78080000 b40c0000 82020000 c3050000
 * Check values: mix32(5) = 0x5c45d53e; with key = mix32(5) and g = 0, sample 0 draws f71b8747 85be176b
 * 3945034a 6243e999 (components 0..3) and sample 65535 draws 73c1d462 9ef285ce 288746e5 5010ac28.
 * The draw counter n is 0 at the camera bounce and advances by one per draw, raw or float, at exactly the
 * sites where the PCG body draws, in the same order. It travels in the low 32 bits of the path's rng
 * payload word (the high 32 bits are the implementation's). When a bounce b >= 1 loads it, it is first
 * rounded up to a multiple of 4, so every bounce opens on a fresh 4-D point and the light sample's
 * (r0, d1, r1, r2) is one point. The camera sample (rtg_set_camera_sampling) takes draws 0..3 of the camera
 * stream: u0..u3 are one 4-D point, film x, film y and the lens.
 * Scope: rtg_render, rtg_render_async, rtg_render_adaptive and the group calls, under RTG_INTEGRATOR_PATH,
 * _DIRECT and _DIRECT_MIS, with either environment mode, the uniform and the power light pick, and both
 * camera modes (kernels of their own: k_sobol_shade, k_sobol_shade_env, k_sobol_shade_pick,
 * k_sobol_generate_sampled; the default's are not touched). A frame that runs the light grid's, the
 * physical material model's, rtg_set_path_mis's or the rough dielectric's kernels keeps the PCG streams,
 * camera samples included, and so do rtg_render_light and rtg_render_instant_radiosity; _ALBEDO, _NORMALS,
 * rtg_gbuffer and the denoiser's guides draw nothing. rtg_sampler_active reports what the next rtg_render
 * would run, so the fallback is not silent; rtg_probe_camera_samples follows it. The setter first issues
 * and waits for queued frames; an unknown value is RTG_ERR_ARG and leaves the previous setting in place. */
#define RTG_SAMPLER_PCG   0
#define RTG_SAMPLER_SOBOL 1
int  rtg_sampler_check(int sampler);  /* rtg_set_sampler's argument check alone (no device) */
int  rtg_set_sampler(rtg_handle* h, int sampler);
int  rtg_get_sampler(rtg_handle* h, int* sampler);
int  rtg_sampler_active(rtg_handle* h, int* sampler);
/* The kernels' own draw function on the current device (no handle): out_raw[i * n_draws + k] is raw draw
 * first_draw + k of (pixels[i], samples[i]) under key(pixels[i], seed, stream). No rounding of the counter
 * between draws. */
int  rtg_probe_sampler(uint64_t seed, uint32_t stream, const uint32_t* pixels, const uint32_t* samples, uint32_t n,
                       uint32_t first_draw, uint32_t n_draws, uint32_t* out_raw /* n * n_draws */);

/* ---- a movable camera (rtg_api.hip). The camera enters with rtg_scene_desc at rtg_create;
 * rtg_set_camera replaces both records on a live handle, so a frame loop that moves its camera
 * (Main.cpp:82-111: W/S/A/D/E/Q, then rt.clear()) keeps the handle, its tree and its upload.
 * rth_camera_look_at (include/rth.h) builds the records from a pose with the loader's own code.
 *   - Both records are required and every field of both must be finite; cam->width and cam->height must
 *     equal the handle's film size. Otherwise RTG_ERR_ARG, reported before any device call, and the camera,
 *     the film and every setting stay as they were.
 *   - Frames queued earlier (rtg_render_async) render with the camera they were queued under: the setter
 *     first issues and waits for them, as rtg_set_camera_sampling does.
 *   - The film and Film::SPP are left alone: the caller clears them (rtg_clear), as Main.cpp does.
 *   - The denoiser's cached guides are dropped and rendered again by the next rtg_denoise / rtg_denoise_guides.
 *   - From the next call on the new records are used by rtg_render, rtg_render_async and the group calls in
 *     both camera modes of rtg_set_camera_sampling and under every integrator (albedo and normals included),
 *     by rtg_render_adaptive, rtg_render_light and rtg_render_instant_radiosity (projectOntoCamera),
 *     rtg_probe_camera_samples, rtg_probe_connect, rtg_geometry_guide and rtg_temporal_accumulate.
 * rtg_get_camera returns the records in use (either pointer may be NULL). rtg_group_set_camera is
 * rtg_set_camera on every rank's handle, checked once for all ranks. No kernel is added or changed by
 * these calls: the kernels take the camera by value with every launch. */
int  rtg_set_camera(rtg_handle* h, const rtg_camera* cam, const rtg_camera_proj* proj);
int  rtg_get_camera(rtg_handle* h, rtg_camera* cam, rtg_camera_proj* proj);

/* ---- geometry guide and temporal accumulation by reprojection (rtg_temporal.hip,
 * tests/temporal_ref.py restates both in numpy). IEEE float32 in the order written, no contraction, plain
 * /, sqrtf and floorf; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 * rtg_geometry_guide: for every pixel the pinhole ray through the pixel centre (Camera::generateRay at
 * (x + 0.5, y + 0.5), whatever rtg_set_camera_sampling says, as the denoiser's guides) is traced by the
 * existing generate and traversal kernels; with (t, id) its closest hit, o the camera origin and d its
 * direction a small kernel writes two 16-byte records per pixel:
 *   pos_t[p]     = {X.xyz, t},   X = o + d t component-wise (Ray::at: the product, then the sum)
 *   normal_id[p] = {Ng.xyz, id as bits},  with v0, v1, v2 the triangle's positions (rtg_scene_desc.positions),
 *                  e1 = v1 - v0, e2 = v2 - v0, c = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *                  e1.x e2.y - e1.y e2.x), l = sqrtf((c.x c.x + c.y c.y) + c.z c.z), Ng = c / l (three divisions)
 *   a miss:      X = 0, t = FLT_MAX (3.40282347e+38f), Ng = 0, id = -1.
 * One guide is cached per camera (a byte comparison of both records) in the temporal state. The film,
 * Film::SPP, the integrator, the options and the statistics are left as they were; the call issues and waits
 * for queued frames first. Either output may be NULL.
 * rtg_temporal_accumulate blends the film's mean into a per-pixel history that follows the camera. The state
 * (allocated by the first call, freed by rtg_destroy, dropped by rtg_temporal_reset) holds the history
 * H[p] = {rgb, len} (16 B per pixel), the camera records it belongs to, and that camera's guide. The film
 * is expected to hold only samples not handed over yet: the loop is move, clear, render, accumulate.
 *   cur[p] = film[p] / m per channel, m = (float)spp; spp == 0: RTG_ERR_ARG.
 *   no history yet     hist is absent for every pixel; the guide of the current camera is computed and kept.
 *   camera unchanged   (both records equal the history's byte for byte) hist = H[p] for every pixel, miss
 *                      pixels included; nothing is traced.
 *   camera moved       the current guide G is computed. A pixel whose G is a miss (id < 0) has no history.
 *                      Otherwise X = G.X, N = G.Ng, t = G.t, and X is projected with the *history's* records by
 *                      Camera::projectOntoCamera's own operations (Scene.h:55-69): pv = cameraToView.mulPoint(X),
 *                      v1 = the first three rows of proj applied to pv, w = 1.0f / ((((q12 pv.x) + (q13 pv.y)) +
 *                      (q14 pv.z)) + q15), pp = v1 w, x = (pp.x + 1) 0.5, y = (pp.y + 1) 0.5; rejected (no
 *                      history) when x < 0, x > 1, y < 0 or y > 1; then x = x width, y = (1 - y) height.
 *                      u = x - 0.5f, v = y - 0.5f, x0 = floorf(u), y0 = floorf(v), ax = u - x0, ay = v - y0.
 *                      Four taps, dy = 0, 1 outer and dx = 0, 1 inner: q = (x0 + dx, y0 + dy) (the sums in
 *                      float), weight w = (dx ? ax : 1 - ax) (dy ? ay : 1 - ay). A tap is used only if
 *                      0 <= q.x < width and 0 <= q.y < height (as float comparisons: a NaN fails), w > 0, the
 *                      history's guide at q is a hit, |dot(X_hist[q] - X, N)| <= plane_tolerance t and
 *                      |dot(Ng_hist[q], N)| >= normal_cos. Used taps: sw = sw + w; acc = acc + w H[q] on all
 *                      four components. sw > 0: hist = acc / sw (four divisions); otherwise no history.
 *   blend              with history: n = hist.len < max_history ? hist.len : max_history; a = m / (n + m);
 *                      out = hist.rgb + (cur - hist.rgb) a; len = n + m. Without: out = cur, len = m.
 *   update             H[p] = {out, len}; after a move (and on the first call) the stored camera and guide
 *                      become the current ones.
 * Non-finite values follow the definition as written: it is not a NaN filter. max_history must be > 0 and may
 * be +inf (the plain running mean); plane_tolerance >= 0 and finite; normal_cos in [0, 1]; anything else, a
 * NaN included, is RTG_ERR_ARG before any device call (rtg_temporal_check is that check alone, no device
 * needed). The defaults (64, 0.01f, 0.9f) are choices, not measured optima. The film, Film::SPP, the
 * integrator, the options and the statistics are left as they were. The call issues and waits for queued
 * frames, runs the guide pass and k_temporal on the handle's stream with no host wait in between, and returns
 * when the result is in the handle's device buffer, and in out (host, w*h*3) when given.
 * rtg_temporal_history copies H (w*h*4; RTG_ERR_ARG before the first accumulate); rtg_temporal_copy_device the
 * last result (w*h*3 floats, device to device); rtg_temporal_ms the device time of the last call's guide pass
 * (0 when none ran) and of its k_temporal launch. Not covered: miss pixels after a move (the background is not
 * reprojected: they restart), groups (rtg_group_set_camera only), moving geometry. Chaining into an a-trous
 * filter on the device with variance-guided weights is rtg_svgf_accumulate, below. */
typedef struct rtg_temporal_params {
    float max_history, plane_tolerance, normal_cos;
} rtg_temporal_params;
int  rtg_temporal_defaults(rtg_temporal_params* p);  /* 64, 0.01f, 0.9f */
int  rtg_temporal_check(const rtg_temporal_params* p);
int  rtg_geometry_guide(rtg_handle* h, float* pos_t /* w*h*4 */, float* normal_id /* w*h*4 */);
int  rtg_temporal_accumulate(rtg_handle* h, const rtg_temporal_params* p, float* out /* w*h*3 or NULL */);
int  rtg_temporal_history(rtg_handle* h, float* rgb_len /* w*h*4 */);
int  rtg_temporal_copy_device(rtg_handle* h, void* dst_device);
int  rtg_temporal_reset(rtg_handle* h);
int  rtg_temporal_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms);

/* ---- variance-guided filtering of the temporal history (SVGF, Schied et al. 2017; DESIGN.md §8j;
 * rtg_svgf.hip, tests/svgf_ref.py restates it in numpy). rtg_svgf_accumulate advances the same per-handle
 * history H = {rgb, len}, history camera and guide as rtg_temporal_accumulate, keeps next to it a moments
 * history M = {mu1, mu2} (8 B per pixel, a ping-pong pair like H), and filters the new H with K a-trous levels
 * whose luminance term is scaled by a per-pixel variance. After any sequence of svgf calls rtg_temporal_history
 * returns the bits the same sequence of rtg_temporal_accumulate calls would have left. A
 * rtg_temporal_accumulate call invalidates M only: the next svgf call starts M from its frame and continues H.
 * rtg_temporal_reset drops both. The albedo / shading-normal guides are the denoiser's cached ones (dropped by
 * rtg_set_camera, rendered again on demand). The film, Film::SPP, the integrator, the options and the
 * statistics are left as they were.
 * IEEE float32 with one rounding per operation, no contraction; sums in the order written, taps in
 * (dy outer, dx inner) order. L(c) = (0.2126f r + 0.7152f g) + 0.0722f b. cur = film / (float)spp per channel,
 * m = (float)spp, l = L(cur), s = l l.
 *   1. temporal + moments   have, the admitted taps, their weights w, sw, n, a = m / (n + m), the output rgb and
 *        len are exactly those of rtg_temporal_accumulate (no history / camera unchanged / camera moved). With a
 *        history: hmu_k = (sum of w M[q].k) / sw over the same admitted taps in the same order; camera unchanged:
 *        M[p] itself. mu_k = hmu_k + (x - hmu_k) a, x = l for k = 1 and x = s for k = 2. Without a history, or
 *        with M invalid: mu1 = l, mu2 = s.
 *   2. variance   vt = mu2 - mu1 mu1, clamped as vt > 0 ? vt : 0. If len >= min_history, v = vt. Otherwise over
 *        the 7x7 window, dy, dx in -3..3, taps inside the image: the centre is always admitted; another tap q is
 *        admitted if p and q are both misses in the current guide, or both hits with
 *        fabsf(dot(X_q - X_p, Ng_p)) <= plane_tolerance t_p and fabsf(dot(Ng_q, Ng_p)) >= normal_cos (the two
 *        tests of rtg_temporal_accumulate on the *current* guide; with the camera unchanged that is the history's
 *        own). Admitted: c0 += 1, c1 += mu1_q, c2 += mu2_q. e1 = c1 / c0, vs = c2 / c0 - e1 e1, clamped at 0 as
 *        above; v = vs (min_history / len). v goes into the .w of the colour record {rgb, v}.
 *   3. filter   `iterations` levels, level i at step = 1 << i, the 5x5 B3 taps h of rtg_denoise. Per pixel p
 *        first gv = sum over the 3x3 neighbourhood at step 1, coordinates clamped to the image, of
 *        (k(dy) k(dx)) v_q with k = {0.25f, 0.5f, 0.25f}, and
 *        il = 1.0f / ((sigma_luminance sigma_luminance) gv + variance_floor). Per tap q inside the image:
 *        w = h[dy] h[dx]; luminance: dl = L(c_q) - L(c_p), t = 1 - (dl dl) il, clamped as t > 0 ? t : 0,
 *        w = w (t t); albedo (when sigma_albedo > 0) and shading normal with normal_squarings: rtg_denoise's two
 *        terms, "both background -> 1" included; plane, a hard test on the current geometry guide: both hits
 *        need fabsf(dot(X_q - X_p, Ng_p)) <= plane_tolerance t_p, else w = 0; a hit and a miss give w = 0; two
 *        misses pass; the centre tap passes by definition. sw += w, acc += w c_q.rgb, av += (w w) v_q. Out: if
 *        sw > 0, rgb = acc / sw and v = av / (sw sw); otherwise the centre's record is kept. No sigma is halved
 *        per level: the filtered variance does that job.
 * The result is the rgb of the last level; rtg_svgf_variance returns step 2's v (w*h), rtg_svgf_moments the new
 * M (w*h*2), rtg_svgf_copy_device the last result (w*h*3 floats, device to device). It is not a NaN filter:
 * non-finite values spread as the definition says. Parameters: temporal as rtg_temporal_accumulate;
 * iterations 1..RTG_DENOISE_MAX_ITERATIONS; normal_squarings 0..8; sigma_luminance > 0 finite; sigma_albedo
 * <= 0 off, else finite >= 1e-6; min_history > 0 finite; variance_floor > 0 finite. Anything else, a NaN
 * included, is RTG_ERR_ARG before any device call (rtg_svgf_check is that check alone, no device needed);
 * spp == 0 is RTG_ERR_ARG; a read-back before the first accumulate is RTG_ERR_ARG. A failed call leaves the
 * state and the film as they were. The defaults (64, 0.01f, 0.9f; 5, 5, 4, 0.1f, 4, 1e-8f) are choices, not
 * measured optima. The whole chain (the fused first-hit pass of rtg_gbuffer if a guide is missing, temporal + moments,
 * variance, a copy of the guide's positions, the levels, unpack) is queued on the handle's stream with no host
 * wait in between; the call returns when the result is in the handle's device buffer, and in out when given.
 * rtg_svgf_ms gives the device time of the last call's guide pass (0 when none ran), temporal + moments
 * kernel, variance kernel and all filter levels together (the copy of the positions included). Not covered:
 * feeding level 0's output back into the history, groups, integration/rtg_rtbase.h, reprojecting the background,
 * moving geometry. Albedo demodulation is rtg_svgf_illum_accumulate, below. */
typedef struct rtg_svgf_params {
    rtg_temporal_params temporal;   /* max_history, plane_tolerance, normal_cos: as rtg_temporal_accumulate */
    uint32_t iterations;            /* 1..RTG_DENOISE_MAX_ITERATIONS, default 5 */
    uint32_t normal_squarings;      /* 0..8, default 5: the shading-normal term of rtg_denoise */
    float sigma_luminance;          /* > 0 finite, default 4 */
    float sigma_albedo;             /* <= 0 off, else finite >= 1e-6, default 0.1 (rtg_denoise's rule) */
    float min_history;              /* > 0 finite, default 4: below it the variance is estimated spatially */
    float variance_floor;           /* > 0 finite, default 1e-8 */
} rtg_svgf_params;
int  rtg_svgf_defaults(rtg_svgf_params* p);  /* 64, 0.01f, 0.9f; 5, 5, 4.0f, 0.1f, 4.0f, 1e-8f */
int  rtg_svgf_check(const rtg_svgf_params* p);
int  rtg_svgf_accumulate(rtg_handle* h, const rtg_svgf_params* p, float* out /* w*h*3 or NULL */);
int  rtg_svgf_variance(rtg_handle* h, float* var /* w*h */);
int  rtg_svgf_moments(rtg_handle* h, float* mu /* w*h*2 */);
int  rtg_svgf_copy_device(rtg_handle* h, void* dst_device);
int  rtg_svgf_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms, double* variance_ms, double* filter_ms);

/* ---- the illumination mode of the variance-guided chain (rtg_svgf_illum.hip,
 * tests/svgf_illum_ref.py restates it in numpy): rtg_svgf_accumulate's chain run on the film over the first
 * hit's albedo, with the pixels that see an emitter directly kept in a class of their own. Opt-in: nothing
 * changes unless these calls are made. IEEE float32 with one rounding per operation, no contraction.
 *   inputs      A, the denoiser's albedo guide of the current camera (the `0 + c` image rtg_gbuffer writes), and G,
 *               its geometry guide.
 *   divisor     per channel d.c = A.c > albedo_floor ? A.c : 1.0f (a NaN fails the comparison and gives 1).
 *   classed G'  G, except that a pixel whose first-hit material is a light (L(emission) > 0, the test rtg_gbuffer
 *               makes first) gets the miss records {0, 0, 0, FLT_MAX} {0, 0, 0, id = -1}.
 *   prepare     F'[p].c = film[p].c / d.c: the film's sums, so cur = F' / m follows unchanged.
 *   chain       rtg_svgf_accumulate's steps 1-3, word for word, on F' and G': the temporal step reprojects with
 *               G', the stored history guide is G', the variance window and the filter's plane test use G'. The
 *               albedo and shading-normal terms read the denoiser's guide as it is (an emitter against the
 *               background still gets weight 0 from the normal term). An emitter pixel therefore restarts every
 *               frame (len = m) and exchanges nothing with surfaces.
 *   remodulate  out.c = rgb.c d.c on the last level's record.
 * State: the mode keeps a history H' (illumination and len), moments, history camera and history guide (G') of
 * its own. rtg_svgf_accumulate's and rtg_temporal_accumulate's H and M are not touched by it and do not touch
 * its: rtg_temporal_history returns what the default-mode calls alone left. rtg_temporal_reset drops both. The
 * guide caches stay unclassed: rtg_geometry_guide, rtg_gbuffer, rtg_temporal_accumulate and rtg_svgf_accumulate
 * return the same bits before and after illumination calls. The film, Film::SPP, the integrator, the options and
 * the statistics are left as they were; a failed call leaves both states and the film as they were.
 * albedo_floor must be finite and > 0 and svgf as rtg_svgf_check says; anything else is RTG_ERR_ARG before any
 * device call (rtg_svgf_illum_check is that check alone). The default floor 1e-3 is a stated choice, not an
 * optimum. The whole chain (the first-hit pass if a guide is missing, k_svgf_illum_prepare, rtg_svgf_accumulate's
 * kernels, k_svgf_illum_unpack) is queued on the handle's stream and waited for once.
 * Read-backs (RTG_ERR_ARG before the first illumination call): rtg_svgf_illum_history H' (w*h*4),
 * rtg_svgf_illum_variance step 2's v (w*h), rtg_svgf_illum_moments (w*h*2), rtg_svgf_illum_guide the classed
 * guide of the history camera (two w*h*4 images, either may be NULL), rtg_svgf_illum_copy_device the last result;
 * rtg_svgf_illum_ms rtg_svgf_ms's four times plus the device time of the prepare and of the unpack kernel.
 * Not covered: rtg_temporal_accumulate, which has the same bleed of a directly seen emitter into the surface
 * next to it; groups; feeding level 0 back into the history; integration/rtg_rtbase.h; a measured gain from
 * demodulation on high-frequency textures (none of this repository's scenes shows one). */
typedef struct rtg_svgf_illum_params {
    rtg_svgf_params svgf;           /* as rtg_svgf_accumulate */
    float albedo_floor;             /* > 0 finite, default 1e-3: channels at or below it are not divided */
} rtg_svgf_illum_params;
int  rtg_svgf_illum_defaults(rtg_svgf_illum_params* p);  /* rtg_svgf_defaults; 1e-3f */
int  rtg_svgf_illum_check(const rtg_svgf_illum_params* p);
int  rtg_svgf_illum_accumulate(rtg_handle* h, const rtg_svgf_illum_params* p, float* out /* w*h*3 or NULL */);
int  rtg_svgf_illum_history(rtg_handle* h, float* rgb_len /* w*h*4 */);
int  rtg_svgf_illum_variance(rtg_handle* h, float* var /* w*h */);
int  rtg_svgf_illum_moments(rtg_handle* h, float* mu /* w*h*2 */);
int  rtg_svgf_illum_guide(rtg_handle* h, float* pos_t /* w*h*4 */, float* normal_id /* w*h*4 */);
int  rtg_svgf_illum_copy_device(rtg_handle* h, void* dst_device);
int  rtg_svgf_illum_ms(rtg_handle* h, double* guide_ms, double* accumulate_ms, double* variance_ms,
                       double* filter_ms, double* prepare_ms, double* unpack_ms);

/* ---- the G-buffer: one first-hit pass for the geometry guide and the albedo / shading-normal guides (DESIGN.md
 * §8k; rtg_gbuffer.hip). The pinhole ray through every pixel centre (whatever rtg_set_camera_sampling says) is
 * traced once by the existing generate and traversal kernels; one kernel, k_gbuffer, then writes per pixel from
 * its closest hit (t, id, alpha, beta), gamma = 1 - (alpha + beta):
 *   pos_t, normal_id   the two records of rtg_geometry_guide, word for word.
 *   shading_normal     what 1 sample of RTG_INTEGRATOR_NORMALS leaves in a cleared film, i.e. the second output of
 *                      rtg_denoise_guides: sn = normalize(n0 alpha + n1 beta + n2 gamma) of the vertex normals,
 *                      negated when the material is two-sided and dot(-d, sn) < 0; the value is
 *                      0 + fabsf(sn) per component; a miss: 0.
 *   albedo             what 1 sample of RTG_INTEGRATOR_ALBEDO leaves in a cleared film, i.e. the first output of
 *                      rtg_denoise_guides: an emitter gives its emission; otherwise a = the material's texture at
 *                      (u, v) interpolated as the normals are (Texture::sample), and a mirror gives a, glass 0,
 *                      every other kind a / (float)M_PI; a miss gives the environment map in direction d
 *                      (EnvironmentMap::evaluate), 0 without one; each as 0 + c per component.
 * Neither integrator draws a random number, so the seed, the sample index, the integrator, the material model
 * and the light, environment, camera and path sampling modes do not reach any output.
 * rtg_gbuffer fills the temporal state's guide cache (rtg_geometry_guide, rtg_temporal_accumulate and
 * rtg_svgf_accumulate pick it up) and the denoiser's cached guides (rtg_denoise, rtg_denoise_guides,
 * rtg_group_denoise and rtg_svgf_accumulate pick them up), and marks both valid for the handle's camera: after
 * it none of those calls traces a camera ray until rtg_set_camera drops the guides. When both are already at
 * hand it runs nothing. rtg_svgf_accumulate runs the same pass in place of a guide pass and two renders. The
 * calls that need only one kind keep their own, cheaper or documented, path when they have to produce it
 * themselves. The film, Film::SPP, the integrator, the options, the statistics and the camera-sampling setting
 * are left as they were. The call issues and waits for queued frames first, queues the pass on the handle's
 * stream with no host wait, waits once and copies out what was asked for: any output may be NULL.
 * rtg_gbuffer_ms gives the device time of the pass (generate, traversal, k_gbuffer) in the last rtg_gbuffer or
 * rtg_svgf_accumulate call, 0 when the caches served it. Not covered: motion vectors, groups,
 * integration/rtg_rtbase.h, switching rtg_denoise to this pass. */
int  rtg_gbuffer(rtg_handle* h, float* pos_t /* w*h*4 */, float* normal_id /* w*h*4 */, float* albedo /* w*h*3 */,
                 float* shading_normal /* w*h*3 */);
int  rtg_gbuffer_ms(rtg_handle* h, double* ms);

/* Add samples [first_sample, first_sample+n_samples) of every pixel in the listed 32x32 tiles
 * (tile id = ty*tilesX + tx, RTBase TILE_SIZE=32; tile_ids=NULL = all tiles) to the film, in
 * sample order per pixel. Equivalent to n_samples calls of RayTracer::render() with the
 * deterministic sampler.
 * rtg_render returns when the samples are on the film. rtg_render_async only queues them:
 *   - with hip_stream NULL it is the drop-in RayTracer::render() of a frame loop (Main.cpp:74-118):
 *     the call is queued and returns before its work starts. Consecutive queued calls with the same
 *     seed and tiles whose samples follow on (frame f, f+1, ...) are coalesced and issued together
 *     once 64M paths are pending (64 frames of a 1-Mpixel film), or as soon as anything reads the
 *     film or the stats, waits, or changes a setting (RTG_OPT_NO_COALESCE issues every call at
 *     once). Issued work of at most 16M paths per chunk runs in a pipeline of 3 slots, each with its
 *     own path state and stream, with no host wait: chunks run side by side on the GPU, a call waits
 *     only for the chunk three before it to leave the GPU, and the film updates stay in sample
 *     order, so the film is bit-identical to one rtg_render of all the samples. A pipelined chunk's
 *     traversal may start before the caller's earlier film reads on the handle (rtg_film_gather,
 *     ...) have run; only its film fold waits for them. Larger chunks (the
 *     call that reaches the 64M threshold issues one) read each bounce's live count back during the
 *     traversal, so that call returns once the chunk's last bounce is issued; the calls before it
 *     return at once. rtg_film_read with a film pointer,
 *     rtg_film_copy_device, rtg_get_stats, rtg_synchronize, rtg_render_idle, rtg_clear ... first
 *     issue and wait for the queued calls; rtg_film_read(h, NULL, &spp) returns Film::SPP at once.
 *     An error of a coalesced call is reported by the call that issues it.
 *   - with a hip_stream, the work is ordered after the caller's earlier work on that stream, and
 *     the caller's later work on it sees the film updated.
 * rtg_render_idle sets *idle to 1 when no queued render work is left on the GPU.
 * Sample indices must stay below RTG_MAX_SAMPLES_PER_KEY: the PCG stream of (pixel, sample) is
 * keyed seq = pixel << 16 | sample; more samples take another seed. */
#define RTG_MAX_SAMPLES_PER_KEY 65536u
int  rtg_render(rtg_handle* h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                const uint32_t* tile_ids, uint32_t n_tiles);
int  rtg_render_async(rtg_handle* h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                      const uint32_t* tile_ids, uint32_t n_tiles, void* hip_stream);
int  rtg_synchronize(rtg_handle* h);
int  rtg_render_idle(rtg_handle* h, int* idle);

/* RayTracer::adaptiveRender (Renderer.h:583-749), one frame (Film::SPP += 1). Pass 1 renders
 * init_samples samples of every pixel (sample indices first_sample ...) into a scratch film and
 * takes each 32x32 tile's variance of the per-pixel means (adaptiveSampling, :583-638); a tile's
 * weight is its share of the total variance; pass 2 renders max((int)(sqrt(weight) * max_samples),
 * min_samples) samples of each pixel of the tile (indices first_sample + init_samples ...) and adds
 * their mean to the film (sampleTileWithWeight, :640-672). The reference constants are INIT_SAMPLES
 * 2, MAX_SAMPLES 10240, MIN_SAMPLES 1 (Renderer.h:20-23). tile_samples (optional, tilesX*tilesY)
 * receives each tile's pass-2 sample count. first_sample + init_samples + the largest tile count
 * must be <= RTG_MAX_SAMPLES_PER_KEY (checked before the film is touched: RTG_ERR_ARG). Pass 2 is
 * staged and published only when every tile group succeeded, so a failed call leaves the film and
 * SPP as they were. */
/* RayTracer::lightTracer (Renderer.h:221-326): each frame traces width*height light paths (path i
 * of frame f draws from the PCG stream keyed (seed, i, f)), connects every non-specular vertex to
 * the camera (connectToCamera: projectOntoCamera, importance W_e = 1/(Afilm cos^4), visibility)
 * and splats the result into the film in (path, vertex) order per pixel, as the reference's
 * single-threaded loop does. Film::SPP += 1 per frame. The film must have < 2^24 pixels. */
int  rtg_render_light(rtg_handle* h, uint32_t first_frame, uint32_t n_frames, uint64_t seed);
/* RayTracer::instantRadiosity (Renderer.h:82-218): each frame traces n_vpl_paths VPL paths
 * (traceVPLs; the reference uses MAX_VPL = 50) and then, for every pixel whose camera ray hits a
 * surface, sums vpl.Le * BSDF * G over every visible VPL in VPL order (computeVPLsContribution)
 * and splats it. Film::SPP += 1 per frame. */
#define RTG_MAX_VPL 50
int  rtg_render_instant_radiosity(rtg_handle* h, uint32_t first_frame, uint32_t n_frames, uint64_t seed,
                                  uint32_t n_vpl_paths);

#define RTG_ADAPTIVE_INIT_SAMPLES 2
#define RTG_ADAPTIVE_MAX_SAMPLES  10240
#define RTG_ADAPTIVE_MIN_SAMPLES  1
int  rtg_render_adaptive(rtg_handle* h, uint32_t first_sample, uint64_t seed, uint32_t init_samples,
                         uint32_t max_samples, uint32_t min_samples, uint32_t* tile_samples);

/* ---- one node, several GPUs (rtg_multi.hip). RayTracer::pathTracerTileBased spreads 32x32 tiles
 * over numProcs CPU threads (Renderer.h:836-853, numProcs from :52-54); here the tiles are spread
 * over devices: rank r of N renders every sample of the tiles with (tile_x + tile_y) % N == r
 * (rtg_tiles_for_rank; the partition of raytracingrenderer_amd/distributed.py), one host thread and
 * one handle per device, and rtg_group_reduce assembles the film on devices[0] from each rank's own
 * tiles only: every rank packs its tiles' pixels (rtg_film_gather), sends them to devices[0] with
 * one ncclSend (ncclCommInitAll, single process; devices[0] posts an ncclRecv per rank), and
 * devices[0] scatters them into the film (rtg_film_scatter). Tile supports are disjoint and cover
 * the image, so the assembled film is bit-identical to a one-device render (and to the sum of the
 * films), at 1/N of a whole-film reduce's bytes per rank. A device list with repeats (N ranks
 * rehearsed on fewer GPUs) renders the ranks in turn and moves the packed tiles with device copies.
 * The scene's device records are built on the host once and uploaded to the devices in parallel
 * (rtg_group_setup_ms). A failed rtg_group_render leaves the group poisoned (other ranks already
 * added their samples): rtg_group_reduce / film_read return RTG_ERR_ARG until rtg_group_clear. */
typedef struct rtg_group rtg_group;
int  rtg_tiles_for_rank(uint32_t width, uint32_t height, int rank, int world, uint32_t* tile_ids /* or NULL */,
                        uint32_t* n_tiles);
int  rtg_group_create(const int* devices, int n_devices, const rtg_scene_desc* desc, rtg_group** out);
void rtg_group_destroy(rtg_group* g);
int  rtg_group_size(rtg_group* g);
rtg_handle* rtg_group_handle(rtg_group* g, int rank);  /* e.g. for rtg_get_stats; owned by the group */
int  rtg_group_set_options(rtg_group* g, int max_depth, int flags, uint32_t max_paths);
int  rtg_group_set_camera_sampling(rtg_group* g, const rtg_camera_sampling* p);  /* every rank's handle */
int  rtg_group_set_env_sampling(rtg_group* g, int mode);  /* rtg_set_env_sampling on every rank's handle */
int  rtg_group_set_light_sampling(rtg_group* g, const rtg_light_sampling* p);  /* every rank's handle */
int  rtg_group_set_light_grid(rtg_group* g, const rtg_light_grid* p);          /* every rank's handle */
int  rtg_group_set_material_params(rtg_group* g, const rtg_material_params* params, uint32_t n);  /* every rank's */
int  rtg_group_set_material_model(rtg_group* g, int mode);  /* rtg_set_material_model on every rank's handle */
int  rtg_group_set_path_mis(rtg_group* g, int mode);  /* rtg_set_path_mis on every rank's handle */
int  rtg_group_set_sampler(rtg_group* g, int sampler);  /* rtg_set_sampler on every rank's handle */
int  rtg_group_set_camera(rtg_group* g, const rtg_camera* cam, const rtg_camera_proj* proj);  /* every rank's handle */
int  rtg_group_render(rtg_group* g, uint32_t first_sample, uint32_t n_samples, uint64_t seed);
int  rtg_group_reduce(rtg_group* g);  /* the films stay per device; the assembled film goes to a separate buffer */
/* Queued forms (the frame loop of Main.cpp:74-118 on N devices). rtg_group_render_async is every
 * rank's rtg_render_async (NULL stream) on its device: frames are coalesced and pipelined per rank
 * as on one handle, and the call returns without waiting for the GPUs. rtg_group_reduce_async
 * queues the own-tile exchange on per-rank exchange streams after each rank's queued frames (pack,
 * RCCL send/recv, scatter on devices[0]); the ranks' next frames start their traversal meanwhile
 * and only their film folds wait for the packs. rtg_group_synchronize waits for both;
 * rtg_group_film_read waits for the exchange it reads. */
int  rtg_group_render_async(rtg_group* g, uint32_t first_sample, uint32_t n_samples, uint64_t seed);
int  rtg_group_reduce_async(rtg_group* g);
int  rtg_group_synchronize(rtg_group* g);
int  rtg_group_film_read(rtg_group* g, float* rgb_sum /* width*height*3 */, uint32_t* spp);  /* reduces if needed */
int  rtg_group_clear(rtg_group* g);
double rtg_group_reduce_ms(rtg_group* g);  /* device time of the last reduce (set when the group is synchronized) */
int  rtg_group_uses_rccl(rtg_group* g);    /* 1: RCCL communicator; 0: device copies (repeated devices) or one
                                              device (no communicator unless RTG_GROUP_RCCL1=1 is set) */
int  rtg_group_setup_ms(rtg_group* g, double* prepare_ms, double* upload_ms);  /* host build, parallel uploads */

/* ---- own-tile film exchange (the data movement of rtg_group_reduce, exposed for hosts that run
 * one process per GPU, e.g. raytracingrenderer_amd/distributed.py over torch.distributed).
 * rtg_tile_pixels lists the film pixel indices (y * width + x) of the given 32x32 tiles in the
 * order rtg_film_gather packs them: tile by tile, row-major inside a tile, clipped at the film
 * edge (pixels NULL: only the count). rtg_film_gather copies the handle's film pixels listed in
 * pixels_dev (device array of n indices; 0xFFFFFFFF = padding, packed as zeros) to dst_dev (3n
 * floats), ordered after every render queued on the handle, and the handle's later film writes
 * (the folds of renders queued after it) wait for it; rtg_film_scatter writes src_dev's n
 * packed pixels into film_dev (film_pixels * 3 floats) at the listed indices (0xFFFFFFFF:
 * skipped). An index at or past the film's pixel count is treated as padding by both (never
 * read or written). Both run on hip_stream (NULL: the handle's stream / the device's null stream) and
 * return without waiting. */
int  rtg_tile_pixels(uint32_t width, uint32_t height, const uint32_t* tile_ids, uint32_t n_tiles,
                     uint32_t* pixels /* or NULL */, uint32_t* n_pixels);
int  rtg_film_gather(rtg_handle* h, const uint32_t* pixels_dev, uint32_t n, float* dst_dev, void* hip_stream);
int  rtg_film_scatter(int device, const float* src_dev, const uint32_t* pixels_dev, uint32_t n, float* film_dev,
                      uint32_t film_pixels /* width * height of film_dev */, void* hip_stream);

/* Film access: the unnormalised sum (Film::film) and the sample count (Film::SPP). */
int  rtg_film_read(rtg_handle* h, float* rgb_sum /* width*height*3 */, uint32_t* spp);
int  rtg_film_copy_device(rtg_handle* h, void* dst_device /* width*height*3 floats */);
int  rtg_film_load(rtg_handle* h, const float* rgb_sum, uint32_t spp);  /* resume */
int  rtg_clear(rtg_handle* h);
int  rtg_get_stats(rtg_handle* h, rtg_stats* out);
/* Per traversal launch (k_trace) device time of the last render with RTG_OPT_TIMING, in launch
 * order (chunk by chunk, bounce by bounce): n receives the count, at most max are written. */
int  rtg_launch_times(rtg_handle* h, double* trace_ms, uint32_t max, uint32_t* n);
/* The rays each trace launch of the last timed render's last chunk walked (path tracer: launch b =
 * bounce b's extension rays + bounce b-1's shadow rays; launch 0 the camera rays, one per pixel, or
 * one per path under rtg_set_camera_sampling with a filter or a lens). */
int  rtg_launch_rays(rtg_handle* h, uint64_t* rays, uint32_t max, uint32_t* n);
/* Diagnostics of the locality-matched roofline (builds with RTG_DEBUG=1 only; RTG_ERR_ARG
 * otherwise). rtg_debug_capture(h, b): the next render records every record fetch of trace launch
 * b of its first chunk, per ray in order (-1: off). rtg_debug_replay(h, out[4]) replays that
 * stream (same addresses, order, grouping and occupancy; nothing but the fetches and 64 VALU per
 * step) on the device: out = {best of 3 replay ms, fetches, extension rays, shadow rays}. */
int  rtg_debug_capture(rtg_handle* h, int launch);
int  rtg_debug_replay(rtg_handle* h, double* out);

/* ---- feature-guided film denoiser (rtg_denoise.hip). RayTracer::denoise() (Renderer.h:752-793)
 * hands the film, the albedo and the view normals to OIDN; the reference never calls it. This is the
 * project's own classical filter with the same inputs, not a reproduction of OIDN's output: the
 * edge-avoiding a-trous wavelet filter (Dammertz et al. 2010). Iteration i = 0..iterations-1 filters
 * with the 5x5 taps {1/16, 1/4, 3/8, 1/4, 1/16}^2 at step 1 << i; a tap's weight is multiplied by
 * max(0, 1 - |dC|^2 / sc^2)^2 with sc = sigma_colour / 2^i, by max(0, 1 - |dA|^2 / sigma_albedo^2)^2,
 * and by clamp(N[p].N[q], 0, 1) squared normal_squarings times (1 where both pixels have a zero
 * normal: background). A sigma <= 0 switches its term off; any other must be finite and >= 1e-6.
 * IEEE float32 without contraction in a fixed order: bit-reproducible (DESIGN.md "Denoiser").
 * Argument errors (RTG_ERR_ARG) are reported before any device call. */
#define RTG_DENOISE_MAX_ITERATIONS 8
typedef struct rtg_denoise_params {
    uint32_t iterations, normal_squarings;
    float sigma_colour, sigma_albedo;
} rtg_denoise_params;
int  rtg_denoise_defaults(rtg_denoise_params* p);  /* 5, 5, 1.0f, 0.1f */
/* The filter alone on caller-given host images (w*h*3 floats each; at most 65535 per side and 2^28
 * pixels); out: w*h*3. */
int  rtg_denoise_images(int device, uint32_t w, uint32_t h, const float* colour, const float* albedo,
                        const float* normal, const rtg_denoise_params* p, float* out);
/* film / spp of the handle, guided by the scene's own albedo and shading normals (1 sample of
 * RTG_INTEGRATOR_ALBEDO and _NORMALS each, rendered on the first call into scratch films and cached
 * until rtg_destroy). Issues and waits for queued frames first (as rtg_film_read); returns when the
 * result is in the handle's device buffer, and in out (host, w*h*3) when given. The film, Film::SPP,
 * the integrator and the options are left as they were (the call that renders the guides leaves their
 * two renders in rtg_stats.render_ms until the next render). spp == 0: RTG_ERR_ARG. */
int  rtg_denoise(rtg_handle* h, const rtg_denoise_params* p, float* out);
int  rtg_denoise_guides(rtg_handle* h, float* albedo, float* normal);  /* host, w*h*3 each, either may be NULL */
int  rtg_denoise_copy_device(rtg_handle* h, void* dst_device);         /* last result, w*h*3 floats */
double rtg_denoise_ms(rtg_handle* h);                                  /* device time of the last rtg_denoise */
/* Reduces if needed, then filters the assembled film on devices[0] with rank 0's guides. */
int  rtg_group_denoise(rtg_group* g, const rtg_denoise_params* p, float* out);

/* Low-level ray queries on the uploaded scene (test / oracle comparison surface).
 * rays: n*8 floats (o.xyz, tmax, dir.xyz, pad). For closest-hit, tmax is ignored and the result
 * is n*4 (t, id-as-float-bits, alpha, beta) with t = FLT_MAX on miss (IntersectionData,
 * Geometry.h:231-238). For any-hit, tmax is Scene::visible's maxT and the result is n int32
 * (1 = visible). Device-side arrays are allocated internally; inputs are host pointers. */
int  rtg_trace_closest(rtg_handle* h, const float* rays, uint32_t n, float* hits);
/* BSDF::sample / evaluate probe on the current device (Materials.h:118-318), scripted draws.
 * cases: n*20 floats (kind, int_ior, ext_ior, albedo.rgb of a 1x1 texture, sNormal.xyz, wo.xyz,
 * tu, tv, draw[4], pad[2]);
 * out: n*11 floats (wi.xyz, reflectedColour.rgb, pdf, draws consumed, evaluate(wi).rgb). */
int  rtg_probe_bsdf(const float* cases, uint32_t n, float* out);
int  rtg_trace_visible(rtg_handle* h, const float* rays, uint32_t n, int32_t* visible);
/* Transcendental probe on the current device: the kernels' acosf / sinf / cosf / atan2f
 * (include/rtg_math.h, the reference platform's glibc restated; RTBase/Sampling.h:35-61,
 * Core.h:549-557, Lights.h:152-155) on n inputs. fn: RTG_MATH_SINF, _COSF, _SINCOSF (out 2n:
 * sin, cos), _ACOSF, _ATAN2F (in 2n: y, x). n < 2^31. */
#define RTG_MATH_SINF   0
#define RTG_MATH_COSF   1
#define RTG_MATH_SINCOSF 2
#define RTG_MATH_ACOSF  3
#define RTG_MATH_ATAN2F 4
int  rtg_probe_math(int fn, const float* in, uint32_t n, float* out);
/* Texture probe on the current device: the shading kernel's own Texture::sample (Imaging.h:72-94) and
 * EnvironmentMap::evaluate (Lights.h:150-157) arithmetic on a caller-given texture. texels_rgb: w*h*3
 * floats, row-major (uploaded in the device layout, RGB + pad); 1..65535 per side, at most 2^28 texels.
 * mode: RTG_PROBE_TEX_SAMPLE (in: n*2 floats tu, tv) or RTG_PROBE_TEX_ENV (in: n*3 floats, the
 * direction wi), optionally | RTG_PROBE_TEX_UNIFORM: the short-cut the kernels take for a texture whose
 * texels all have the same bits (the first texel for all four taps, no fetch); such a texture only.
 * out: n*3 floats (rgb). n <= (2^31 - 1) / 3. Argument errors (RTG_ERR_ARG) are reported before any
 * device call. */
#define RTG_PROBE_TEX_SAMPLE  0
#define RTG_PROBE_TEX_ENV     1
#define RTG_PROBE_TEX_UNIFORM 2
int  rtg_probe_texture(int mode, const float* texels_rgb, uint32_t w, uint32_t h, const float* in, uint32_t n,
                       float* out);
/* Camera-connection probe: the light tracer's own connectToCamera (Renderer.h:236-262) on the handle's
 * camera, up to and apart from its visibility test, on n points. points, normals, colours: n*3 floats
 * each (the vertex, its shading normal, the colour thr * f * Le to connect). out: n*12 floats per point:
 * accepted (int32 1 / 0), the splat pixel y * width + x (int32), the splatted colour col * W_e * G (3),
 * Scene::visible(p, camera.origin)'s ray origin (3) and maxT, its direction (3); all zero where the
 * connection is not accepted (projectOntoCamera refuses the point, a cosine is negative, or the pixel
 * lies off the film). n <= (2^31 - 1) / 12. */
int  rtg_probe_connect(rtg_handle* h, const float* points, const float* normals, const float* colours, uint32_t n,
                       float* out);

#ifdef __cplusplus
}
#endif
#endif /* RTG_H */
