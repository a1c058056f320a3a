// rtg_shade_mis.hip — rtg_set_path_mis (include/rtg.h): multiple importance sampling of emitters in the
// path tracer. k_shade_mis is the shading kernel with the power heuristic between the NEE sample and the
// BSDF sample (rtg_mis.h) at its NEE, emitter-hit and miss sites; the host builds the triangle -> light
// map the emitter-hit site needs from the scene's light list when the mode is first switched on. Built
// with rtg_shade.hip's flags (raytracingrenderer_amd/build.py: DEVICE_FLAGS).
#include "rtg_internal.h"

#include <cstring>

// k_shade_phys (rtg_shade_phys.hip) for pathTrace alone, with the weights: kernels of their own name,
// taking the per-triangle table as an argument only they have, so the twenty k_shade / k_shade_env /
// k_shade_pick / k_shade_phys instantiations stay as they were. The environment table, the light pick and
// the material model are run-time branches (the reference model, or a scene without a physical record,
// gets a table of reference-kind records), so the family is two kernels.
#ifndef RTG_SHADE_MIS_WAVES
#define RTG_SHADE_MIS_WAVES 6  // 75-76 VGPRs, no spills (7: 3-5 spilled VGPRs; DESIGN.md §8f has the table)
#endif
#define RTG_SHADE_PHYS 1
#define RTG_SHADE_MIS 1
template <bool TAB>
__global__ __launch_bounds__(RTG_TB, RTG_SHADE_MIS_WAVES) void k_shade_mis(SceneView s, ChunkArgs a, PathBufs p, int b,
                                                                           const uint4* env_table, LightPick lpk,
                                                                           const PhysMat* phys_table, int phys_n,
                                                                           MisArgs mis) {
    constexpr bool ALT = false;
    // (the table's size is the environment texture's: the kernel is short of SGPRs, and s has it already)
    const EnvTable et{env_table, (unsigned)s.env_w * (unsigned)s.env_h, (unsigned)s.env_w, (unsigned)s.env_h};
    const PhysArgs pm{phys_table, nullptr, phys_n};  // (the triangle's record index comes with mis.index)
    const bool ENV = et.table != nullptr;
    const bool PICK = lpk.table != nullptr;
    a.mode = RTG_INTEGRATOR_PATH;  // the one estimator it is launched for: the others compile away
    s.env_uniform = 0;  // a constant environment map fetches its texels like any other (the same operands, so
                        // the same bits): the short-cut's four SGPRs are what k_shade_mis<false> would spill
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_MIS
#undef RTG_SHADE_PHYS

// rtg_probe_mis_weight: mis_w on given densities
__global__ void k_probe_mis_weight(const float* p, const float* q, unsigned n, float* w) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    w[i] = mis_w(p[i], q[i]);
}

// rtg_probe_env_pdf: the density the active environment mode gives a direction
__global__ void k_probe_env_pdf(EnvTable et, const float* dirs, unsigned n, float* pdf) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const v3 d = mk(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
    pdf[i] = et.table ? env_pdf_luminance(et, d) : uniform_sphere_pdf();
}

int launch_shade_mis(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                     const PathBufs& p, int b) {
    hipLaunchKernelGGL(m.tab ? k_shade_mis<true> : k_shade_mis<false>, dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b,
                       m.env.table, m.pick, m.phys.table, m.phys.n, m.mis);
    LAUNCH_OK("k_shade_mis");
    return RTG_OK;
}

// The triangle -> light map from the light list (a triangle listed twice: its first entry) beside the
// triangle's parameter record index (0 before a parameter table was built), the environment light's
// index in entry 0, and as many reference-kind parameter records as the parameter table has
static int build_mis_tables(rtg_handle* h) {
    const size_t nt = h->tri_mat.size();
    std::vector<int32_t> of(nt, -1);
    int32_t env_li = -1;
    for (size_t i = 0; i < h->light_tri.size(); ++i) {
        const int32_t t = h->light_tri[i];
        int32_t& slot = t < 0 ? env_li : of[(size_t)t];  // (prepare_scene checked the triangle index)
        if (slot < 0) slot = (int32_t)i;
    }
    const bool have = h->phys_index.size() == nt;
    std::vector<uint2> ix(1 + nt);
    ix[0] = make_uint2(0u, (unsigned)env_li);
    for (size_t t = 0; t < nt; ++t) ix[1 + t] = make_uint2(have ? h->phys_index[t] : 0u, (unsigned)of[t]);
    const int n_ref = have && h->n_phys > 0 ? h->n_phys : 1;
    PhysMat zero;
    std::memset(&zero, 0, sizeof(zero));  // tag RTG_MODEL_REFERENCE: nothing else of it is read
    DevBuf<uint2> d_ix;
    DevBuf<PhysMat> d_ref;
    if (int rc = d_ix.upload(ix)) return rc;
    if (int rc = d_ref.upload(std::vector<PhysMat>((size_t)n_ref, zero))) return rc;
    h->mt.mis_index = std::move(d_ix);
    h->mt.mis_ref = std::move(d_ref);
    h->n_mis_ref = n_ref;
    h->light_of.swap(of);
    return RTG_OK;
}

int mis_sync_tables(rtg_handle* h) { return h->mt.mis_index.p ? build_mis_tables(h) : (int)RTG_OK; }

extern "C" {

int rtg_path_mis_check(int mode) {
    if (mode != RTG_PATH_MIS_OFF && mode != RTG_PATH_MIS_POWER) {
        g_err = "rtg_set_path_mis: unknown mode";
        return RTG_ERR_ARG;
    }
    return RTG_OK;
}

int rtg_set_path_mis(rtg_handle* h, int mode) {
    if (!h) { g_err = "rtg_set_path_mis: null handle"; return RTG_ERR_ARG; }
    if (int rc = rtg_path_mis_check(mode)) return rc;
    if (int rc = settle(h)) return rc;
    if (mode == RTG_PATH_MIS_POWER && !h->mt.mis_index.p)
        if (int rc = build_mis_tables(h)) return rc;
    h->path_mis = mode;
    return RTG_OK;
}

int rtg_get_path_mis(rtg_handle* h, int* mode) {
    if (!h || !mode) { g_err = "rtg_get_path_mis: null argument"; return RTG_ERR_ARG; }
    *mode = h->path_mis;
    return RTG_OK;
}

int rtg_light_of_triangle(rtg_handle* h, int32_t* out) {
    if (!h || !out) { g_err = "rtg_light_of_triangle: null argument"; return RTG_ERR_ARG; }
    if (!h->mt.mis_index.p) { g_err = "rtg_light_of_triangle: the map is built by the first RTG_PATH_MIS_POWER setting"; return RTG_ERR_ARG; }
    std::memcpy(out, h->light_of.data(), h->light_of.size() * sizeof(int32_t));
    return RTG_OK;
}

int rtg_probe_mis_weight(const float* p, const float* q, uint32_t n, float* w) {
    if (!p || !q || !w) { g_err = "rtg_probe_mis_weight: null argument"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 4u) { g_err = "rtg_probe_mis_weight: too many cases"; return RTG_ERR_ARG; }
    if (n == 0) return RTG_OK;
    const size_t bytes = (size_t)n * sizeof(float);
    return probe_run({{p, bytes}, {q, bytes}}, {{w, bytes}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_mis_weight, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d[0],
                           (const float*)d[1], (unsigned)n, (float*)d[2]);
    });
}

int rtg_probe_env_pdf(rtg_handle* h, const float* dirs, uint32_t n, float* pdf) {
    if (!h || !dirs || !pdf) { g_err = "rtg_probe_env_pdf: null argument"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 12u) { g_err = "rtg_probe_env_pdf: too many cases"; return RTG_ERR_ARG; }
    if (n == 0) return RTG_OK;
    HIPOK(hipSetDevice(h->device));
    return probe_run({{dirs, (size_t)n * 3 * sizeof(float)}}, {{pdf, (size_t)n * sizeof(float)}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_env_pdf, dim3((n + 255) / 256), dim3(256), 0, nullptr, env_table_set(h),
                           (const float*)d[0], (unsigned)n, (float*)d[1]);
    });
}

}  // extern "C"
