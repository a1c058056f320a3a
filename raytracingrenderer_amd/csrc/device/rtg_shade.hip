// rtg_shade.hip — k_shade, the shading stage of the wavefront path tracer (see rtg_render.hip's
// header for the bounce loop), in a translation unit of its own so that it can be compiled with its
// own instruction-scheduling strategy (raytracingrenderer_amd/build.py: SHADE_FLAGS).
#include "rtg_internal.h"

#include <hip/hip_runtime.h>

// ------------------------------------------------------------------ shade
// Path state travels with the queues: the extension payload of bounce b (origin with the path id
// in .w, direction with canHitLight in .w, throughput, PCG state) sits at the ray's position in
// the extension queue, in buffer set b & 1. k_trace and k_shade read it by position (contiguous, no
// id -> payload indirection in either kernel's dependent chain); k_shade writes a continuing
// path's next payload at its position in set (b + 1) & 1 and an NEE ray (staged in LDS: held in
// registers across the BSDF sample it spilled) at its shadow-queue position, the path id beside
// it. Per-path results (contrib, meta, and sh_c, the rare copy-on-visible NEE value) stay indexed by
// path id for k_accumulate.
// ALT = false: pathTrace only (RayTracer::render's estimator; the other modes compile away).
// ALT = true: every per-pixel estimator of rtg_set_integrator, selected by a.mode.
// TAB = true: the scene's material and light records (at most RTG_LDS_MATS / RTG_LDS_LIGHTS) are
// copied into LDS while the payload and the hit triangle's shading record load, so the material a
// shading record names is an LDS read, not a dependent global fetch: the chain per path is payload ->
// shading record -> (texels of a texture larger than 1x1).
// The body is rtg_shade_body.h, shared as text with k_shade_env below.
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, RTG_SHADE_WAVES) void k_shade(SceneView s, ChunkArgs a, PathBufs p, int b) {
    constexpr bool ENV = false;  // EnvironmentMap::sample's uniform sphere; the table branch compiles away
    const EnvTable et{nullptr, 0u, 0u, 0u};
    constexpr bool PICK = false;  // Scene::sampleLight's uniform pick (k_shade_pick: rtg_light_pick.hip)
    const LightPick lpk{nullptr};
#include "rtg_shade_body.h"
}
// k_shade with the environment light sampled through the alias table (RTG_ENV_LUMINANCE): kernels of
// their own name, taking the table as an argument only they have, so SceneView and ChunkArgs
// (k_trace's and k_generate's arguments too) and the four k_shade instantiations stay as they were.
// ALT = false: pathTrace alone, at k_shade<false, *>'s 7 waves per SIMD; ALT = true (DIRECT,
// DIRECT_MIS): RTG_SHADE_ENV_ALT_WAVES, the most at which the estimators' kernel holds its state in
// registers (k_shade<true, *> itself spills at 7).
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_shade_env(
    SceneView s, ChunkArgs a, PathBufs p, int b, EnvTable et) {
    constexpr bool ENV = true;
    constexpr bool PICK = false;
    const LightPick lpk{nullptr};
#include "rtg_shade_body.h"
}

// k_shade and k_shade_env drawing from the Owen-scrambled Sobol sampler (rtg_set_sampler, RTG_SAMPLER_SOBOL;
// rtg_sampler.h): the same body with RTG_SHADE_SOBOL set, in kernels of their own name, so the eight
// kernels above keep their instructions. The waves per SIMD are their parents', but for k_sobol_shade<true,
// *>: k_shade<true, *> spills at its 7 waves (46-60 VGPRs) and the draws add to that (57-75), so it takes
// k_shade_env<true, *>'s RTG_SHADE_ENV_ALT_WAVES, where it holds its state in registers (DESIGN.md §8m has
// the register table).
#define RTG_SHADE_SOBOL
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_sobol_shade(
    SceneView s, ChunkArgs a, PathBufs p, int b) {
    constexpr bool ENV = false;
    const EnvTable et{nullptr, 0u, 0u, 0u};
    constexpr bool PICK = false;
    const LightPick lpk{nullptr};
#include "rtg_shade_body.h"
}
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, ALT ? RTG_SHADE_ENV_ALT_WAVES : RTG_SHADE_WAVES) void k_sobol_shade_env(
    SceneView s, ChunkArgs a, PathBufs p, int b, EnvTable et) {
    constexpr bool ENV = true;
    constexpr bool PICK = false;
    const LightPick lpk{nullptr};
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_SOBOL

// The launch of one shading bounce (ShadeFamily::Plain and Env): the pathTrace-only kernel or the one
// holding every per-pixel estimator, with or without the LDS material / light tables.
int launch_shade(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                 const PathBufs& p, int b) {
    const bool alt = m.alt, tab = m.tab;
    // (the existing kernels are named first, the Sobol variants after them: a unit's kernels are emitted in
    // the order of their first use, and the existing ones keep their place in it)
    auto kenv = alt ? (tab ? k_shade_env<true, true> : k_shade_env<true, false>)
                    : (tab ? k_shade_env<false, true> : k_shade_env<false, false>);
    auto kern = alt ? (tab ? k_shade<true, true> : k_shade<true, false>)
                    : (tab ? k_shade<false, true> : k_shade<false, false>);
    if (m.sobol) {
        kenv = alt ? (tab ? k_sobol_shade_env<true, true> : k_sobol_shade_env<true, false>)
                   : (tab ? k_sobol_shade_env<false, true> : k_sobol_shade_env<false, false>);
        kern = alt ? (tab ? k_sobol_shade<true, true> : k_sobol_shade<true, false>)
                   : (tab ? k_sobol_shade<false, true> : k_sobol_shade<false, false>);
    }
    if (m.family == ShadeFamily::Env) {  // RTG_ENV_LUMINANCE with a table (PATH, DIRECT, DIRECT_MIS)
        hipLaunchKernelGGL(kenv, dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b, m.env);
        LAUNCH_OK((m.sobol ? "k_sobol_shade_env" : "k_shade_env"));
        return RTG_OK;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b);
    LAUNCH_OK((m.sobol ? "k_sobol_shade" : "k_shade"));
    return RTG_OK;
}
