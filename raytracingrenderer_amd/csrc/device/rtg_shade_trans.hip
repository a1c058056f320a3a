// rtg_shade_trans.hip — rough dielectric transmission of the physical material model (include/rtg.h,
// RTG_MODEL_ROUGH_DIELECTRIC; rtg_trans.h has the model). k_shade_trans is k_shade_phys, and
// k_shade_trans_mis is k_shade_mis, with a record of that tag shaded by the model's reflection and
// transmission lobes; conductor, plastic and Oren-Nayar records shade as they do there, so a scene can
// mix all models. shade_mode_of chooses the family only under RTG_MATERIALS_PHYSICAL with PATH or DIRECT
// and a triangle that uses such a record. Built with rtg_shade.hip's flags
// (raytracingrenderer_amd/build.py: DEVICE_FLAGS).
#include "rtg_internal.h"
#include "rtg_trans.h"

// Kernels of their own name with k_shade_phys's and k_shade_mis's arguments, so the twenty-two existing
// shading instantiations stay as they were. The environment table and the light pick are run-time
// branches; PATH and DIRECT without MIS are the ALT pair, PATH under rtg_set_path_mis a pair of its own.
#ifndef RTG_SHADE_TRANS_WAVES
#define RTG_SHADE_TRANS_WAVES 6  // 72-80 VGPRs, no spills (7: 1-7 spilled VGPRs; DESIGN.md §8g has the table)
#endif
#define RTG_SHADE_PHYS 1
#define RTG_SHADE_TRANS 1
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, RTG_SHADE_TRANS_WAVES) void k_shade_trans(SceneView s, ChunkArgs a, PathBufs p, int b,
                                                                               EnvTable et, LightPick lpk, PhysArgs pm) {
    const bool ENV = et.table != nullptr;
    const bool PICK = lpk.table != nullptr;
    if (ALT) a.mode = RTG_INTEGRATOR_DIRECT;  // the one estimator it is launched for: the others compile away
#include "rtg_shade_body.h"
}

#define RTG_SHADE_MIS 1
template <bool TAB>
__global__ __launch_bounds__(RTG_TB, RTG_SHADE_TRANS_WAVES) void k_shade_trans_mis(SceneView s, ChunkArgs a, PathBufs p,
                                                                                   int b, const uint4* env_table,
                                                                                   LightPick lpk, const PhysMat* phys_table,
                                                                                   int phys_n, MisArgs mis) {
    constexpr bool ALT = false;
    const EnvTable et{env_table, (unsigned)s.env_w * (unsigned)s.env_h, (unsigned)s.env_w, (unsigned)s.env_h};
    const PhysArgs pm{phys_table, nullptr, phys_n};  // (the triangle's record index comes with mis.index)
    const bool ENV = et.table != nullptr;
    const bool PICK = lpk.table != nullptr;
    a.mode = RTG_INTEGRATOR_PATH;  // the one estimator it is launched for: the others compile away
    s.env_uniform = 0;  // as k_shade_mis: a constant environment map fetches its texels (the same bits)
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_MIS
#undef RTG_SHADE_TRANS
#undef RTG_SHADE_PHYS

// rtg_probe_transmission: trans_sample / trans_eval / trans_pdf on scripted cases (rtg_probe_material's layout)
__global__ void k_probe_transmission(const float* in, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = in + (size_t)i * 28;
    PhysMat q;
    q.a = make_float4(__int_as_float((int)c[0]), c[1], c[2], c[3]);
    q.b = make_float4(c[5], c[6], c[7], c[4]);
    q.c = make_float4(c[8], c[9], c[10], 0.0f);
    const v3 alb = mk(c[11], c[12], c[13]);
    const frame fr = frame_from(mk(c[14], c[15], c[16]));
    const v3 wo_w = mk(c[17], c[18], c[19]);
    const v3 wo = to_local(fr, wo_w);
    const v3 qi = to_local(fr, mk(c[23], c[24], c[25]));
    ScriptSampler smp{c + 20, 3, 0};
    v3 col;
    float pdf;
    bool delta;
    const v3 wi = trans_sample(q, alb, fr, wo_w, smp, col, pdf, delta);
    const v3 ev = trans_eval(q, alb, wo, qi);
    float* o = out + (size_t)i * 16;
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z;
    o[3] = col.x; o[4] = col.y; o[5] = col.z;
    o[6] = pdf;
    o[7] = (float)smp.i;
    o[8] = delta ? 1.0f : 0.0f;
    o[9] = ev.x; o[10] = ev.y; o[11] = ev.z;
    o[12] = trans_pdf(q, wo, qi);
    o[13] = o[14] = o[15] = 0.0f;
}

int launch_shade_trans(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                       const PathBufs& p, int b) {
    if (m.family == ShadeFamily::TransMis) {
        hipLaunchKernelGGL(m.tab ? k_shade_trans_mis<true> : k_shade_trans_mis<false>, dim3(grid), dim3(RTG_TB), 0, st, s,
                           a, p, b, m.env.table, m.pick, m.phys.table, m.phys.n, m.mis);
        LAUNCH_OK("k_shade_trans_mis");
        return RTG_OK;
    }
    auto kern = m.alt ? (m.tab ? k_shade_trans<true, true> : k_shade_trans<true, false>)
                      : (m.tab ? k_shade_trans<false, true> : k_shade_trans<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b, m.env, m.pick, m.phys);
    LAUNCH_OK("k_shade_trans");
    return RTG_OK;
}

extern "C" {

int rtg_probe_transmission(const float* cases, uint32_t n, float* out) {
    if (!cases || !out) { g_err = "rtg_probe_transmission: null argument"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 28u) { g_err = "rtg_probe_transmission: too many cases"; return RTG_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i) {
        if (!(cases[(size_t)i * 28] == (float)RTG_MODEL_ROUGH_DIELECTRIC)) {
            g_err = "rtg_probe_transmission: a model other than the rough dielectric";
            return RTG_ERR_ARG;
        }
    }
    if (n == 0) return RTG_OK;
    return probe_run({{cases, (size_t)n * 28 * sizeof(float)}}, {{out, (size_t)n * 16 * sizeof(float)}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_transmission, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d[0], (int)n,
                           (float*)d[1]);
    });
}

}  // extern "C"
