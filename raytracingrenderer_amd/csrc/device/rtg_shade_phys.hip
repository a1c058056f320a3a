// rtg_shade_phys.hip — rtg_set_material_model (include/rtg.h): the physical material model. The host
// keeps one parameter record per scene material (rtg_set_material_params), merges equal records into a
// device table and gives every triangle an index into it; k_shade_phys is the shading kernel with
// rtg_phys.h's conductor, plastic and Oren-Nayar models at its NEE and bounce sites. Built with
// rtg_shade.hip's flags (raytracingrenderer_amd/build.py: DEVICE_FLAGS).
#include "rtg_internal.h"

#include <cmath>
#include <cstring>

// k_shade (rtg_shade.hip) with the physical models: kernels of their own name, taking the tables as
// arguments only they have, so SceneView, ChunkArgs and the sixteen k_shade / k_shade_env / k_shade_pick
// instantiations stay as they were. The environment table and the light pick are run-time branches here
// (a null table: the uniform form), so the family is four kernels, not sixteen.
// ALT = false: pathTrace alone; ALT = true: RTG_INTEGRATOR_DIRECT (the other estimators never launch it).
#ifndef RTG_SHADE_PHYS_WAVES
#define RTG_SHADE_PHYS_WAVES 6  // 72-73 VGPRs, no spills (7: 3-4 spilled VGPRs; DESIGN.md §8e has the table)
#endif
#define RTG_SHADE_PHYS 1
template <bool ALT, bool TAB>
__global__ __launch_bounds__(RTG_TB, RTG_SHADE_PHYS_WAVES) void k_shade_phys(SceneView s, ChunkArgs a, PathBufs p, int b,
                                                                             EnvTable et, LightPick lpk, PhysArgs pm) {
    const bool ENV = et.table != nullptr;
    const bool PICK = lpk.table != nullptr;
    if (ALT) a.mode = RTG_INTEGRATOR_DIRECT;  // the one estimator it is launched for: the others compile away
#include "rtg_shade_body.h"
}
#undef RTG_SHADE_PHYS

// rtg_probe_material: phys_sample / phys_eval / phys_pdf on scripted cases (include/rtg.h has the layout)
__global__ void k_probe_material(const float* in, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = in + (size_t)i * 28;
    PhysMat q;
    q.a = make_float4(__int_as_float((int)c[0]), c[1], c[2], c[3]);
    q.b = make_float4(c[5], c[6], c[7], c[4]);
    q.c = make_float4(c[8], c[9], c[10], 0.0f);
    const v3 alb = mk(c[11], c[12], c[13]);
    const frame fr = frame_from(mk(c[14], c[15], c[16]));
    const v3 wo = to_local(fr, mk(c[17], c[18], c[19]));
    const v3 qi = to_local(fr, mk(c[23], c[24], c[25]));
    ScriptSampler smp{c + 20, 3, 0};
    v3 col;
    float pdf;
    bool delta;
    const v3 wi = to_world(fr, phys_sample(q, alb, wo, smp, col, pdf, delta));
    const v3 ev = phys_eval(q, alb, wo, qi);
    float* o = out + (size_t)i * 16;
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z;
    o[3] = col.x; o[4] = col.y; o[5] = col.z;
    o[6] = pdf;
    o[7] = (float)smp.i;
    o[8] = delta ? 1.0f : 0.0f;
    o[9] = ev.x; o[10] = ev.y; o[11] = ev.z;
    o[12] = phys_pdf(q, wo, qi);
    o[13] = o[14] = o[15] = 0.0f;
}

int launch_shade_phys(const ShadeMode& m, unsigned grid, hipStream_t st, const SceneView& s, const ChunkArgs& a,
                      const PathBufs& p, int b) {
    auto kern = m.alt ? (m.tab ? k_shade_phys<true, true> : k_shade_phys<true, false>)
                      : (m.tab ? k_shade_phys<false, true> : k_shade_phys<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RTG_TB), 0, st, s, a, p, b, m.env, m.pick, m.phys);
    LAUNCH_OK("k_shade_phys");
    return RTG_OK;
}

static bool param_ok(float x) { return x >= 0.0f && x <= RTG_FLT_MAX; }  // (false for NaN)

int material_params_check(const char* who, const rtg_material_params* params, uint32_t n, uint32_t n_materials) {
    if (!params) { g_err = std::string(who) + ": null argument"; return RTG_ERR_ARG; }
    if (n != n_materials) { g_err = std::string(who) + ": one record per scene material is needed"; return RTG_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i) {
        const rtg_material_params& m = params[i];
        if ((m.model < RTG_MODEL_REFERENCE || m.model > RTG_MODEL_ORENNAYAR) && m.model != RTG_MODEL_ROUGH_DIELECTRIC) {
            g_err = std::string(who) + ": unknown model tag";
            return RTG_ERR_ARG;
        }
        bool ok = param_ok(m.alpha) && param_ok(m.sigma) && param_ok(m.int_ior) && param_ok(m.ext_ior);
        for (int k = 0; k < 3; ++k) ok = ok && param_ok(m.eta[k]) && param_ok(m.k[k]);
        if (!ok) { g_err = std::string(who) + ": a negative or non-finite parameter"; return RTG_ERR_ARG; }
        if (m.model == RTG_MODEL_ROUGH_DIELECTRIC && !(m.int_ior > 0.0f && m.ext_ior > 0.0f && m.int_ior != m.ext_ior)) {
            g_err = std::string(who) + ": a rough dielectric needs int_ior and ext_ior above 0 and unequal";
            return RTG_ERR_ARG;
        }
    }
    return RTG_OK;
}

static PhysMat record_of(const rtg_material_params& m) {
    PhysMat q;
    float tag;
    std::memcpy(&tag, &m.model, 4);
    q.a = make_float4(tag, m.alpha, m.sigma, m.int_ior);
    q.b = make_float4(m.eta[0], m.eta[1], m.eta[2], m.ext_ior);
    q.c = make_float4(m.k[0], m.k[1], m.k[2], 0.0f);
    if (m.model == RTG_MODEL_REFERENCE) {  // nothing of a reference-kind record is read: one record for all
        q.a = make_float4(tag, 0.0f, 0.0f, 0.0f);
        q.b = q.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return q;
}

// The device table of the handle's parameter records: equal records merged, one index per triangle
static int build_phys_table(rtg_handle* h) {
    std::vector<PhysMat> uniq;
    std::vector<unsigned> of_mat(h->mat_params.size());
    for (size_t i = 0; i < h->mat_params.size(); ++i) {
        const PhysMat q = record_of(h->mat_params[i]);
        size_t j = 0;
        while (j < uniq.size() && std::memcmp(&uniq[j], &q, sizeof(PhysMat)) != 0) ++j;
        if (j == uniq.size()) uniq.push_back(q);
        of_mat[i] = (unsigned)j;
    }
    if (uniq.empty()) uniq.push_back(record_of(rtg_material_params{}));
    std::vector<unsigned> index(h->tri_mat.size());
    bool any = false, any_trans = false;
    for (size_t t = 0; t < index.size(); ++t) {
        index[t] = of_mat[h->tri_mat[t]];  // (prepare_scene checked the triangle's material index)
        any = any || h->mat_params[h->tri_mat[t]].model != RTG_MODEL_REFERENCE;
        any_trans = any_trans || h->mat_params[h->tri_mat[t]].model == RTG_MODEL_ROUGH_DIELECTRIC;
    }
    DevBuf<PhysMat> d_tab;
    DevBuf<unsigned> d_idx;
    if (int rc = d_tab.upload(uniq)) return rc;
    if (int rc = d_idx.upload(index)) return rc;
    h->mt.phys = std::move(d_tab);
    h->mt.phys_index = std::move(d_idx);
    h->n_phys = (int)uniq.size();
    h->phys_any = any;
    h->trans_any = any_trans;
    h->phys_built = true;
    h->phys_index.swap(index);
    return mis_sync_tables(h);  // (rtg_set_path_mis's table holds a copy of the index)
}

extern "C" {

int rtg_material_params_check(const rtg_material_params* params, uint32_t n, uint32_t n_materials) {
    return material_params_check("rtg_material_params_check", params, n, n_materials);
}

int rtg_set_material_params(rtg_handle* h, const rtg_material_params* params, uint32_t n) {
    if (!h) { g_err = "rtg_set_material_params: null handle"; return RTG_ERR_ARG; }
    if (int rc = material_params_check("rtg_set_material_params", params, n, h->n_desc_mats)) return rc;
    if (int rc = settle(h)) return rc;
    std::vector<rtg_material_params> prev(params, params + n);
    prev.swap(h->mat_params);
    h->phys_built = false;
    if (h->material_model == RTG_MATERIALS_PHYSICAL) {
        if (int rc = build_phys_table(h)) {
            h->mat_params.swap(prev);  // (the old table is still the one on the device)
            h->phys_built = true;
            return rc;
        }
    }
    return RTG_OK;
}

int rtg_set_material_model(rtg_handle* h, int mode) {
    if (!h) { g_err = "rtg_set_material_model: null handle"; return RTG_ERR_ARG; }
    if (mode != RTG_MATERIALS_REFERENCE && mode != RTG_MATERIALS_PHYSICAL) {
        g_err = "rtg_set_material_model: unknown mode";
        return RTG_ERR_ARG;
    }
    if (mode == RTG_MATERIALS_PHYSICAL && h->mat_params.size() != h->n_desc_mats) {
        g_err = "rtg_set_material_model: no material parameters were set (rtg_set_material_params)";
        return RTG_ERR_ARG;
    }
    if (mode == RTG_MATERIALS_PHYSICAL && h->n_desc_mats == 0) {
        g_err = "rtg_set_material_model: the scene has no materials";
        return RTG_ERR_ARG;
    }
    if (int rc = settle(h)) return rc;
    if (mode == RTG_MATERIALS_PHYSICAL && !h->phys_built)
        if (int rc = build_phys_table(h)) return rc;
    h->material_model = mode;
    return RTG_OK;
}

int rtg_get_material_model(rtg_handle* h, int* mode) {
    if (!h || !mode) { g_err = "rtg_get_material_model: null argument"; return RTG_ERR_ARG; }
    *mode = h->material_model;
    return RTG_OK;
}

int rtg_probe_material(const float* cases, uint32_t n, float* out) {
    if (!cases || !out) { g_err = "rtg_probe_material: null argument"; return RTG_ERR_ARG; }
    if (n > 0x7fffffffu / 28u) { g_err = "rtg_probe_material: too many cases"; return RTG_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i) {
        const float m = cases[(size_t)i * 28];
        if (!(m == (float)RTG_MODEL_CONDUCTOR || m == (float)RTG_MODEL_PLASTIC || m == (float)RTG_MODEL_ORENNAYAR)) {
            g_err = "rtg_probe_material: a model other than conductor, plastic or Oren-Nayar";
            return RTG_ERR_ARG;
        }
    }
    if (n == 0) return RTG_OK;
    return probe_run({{cases, (size_t)n * 28 * sizeof(float)}}, {{out, (size_t)n * 16 * sizeof(float)}}, [&](void* const* d) {
        hipLaunchKernelGGL(k_probe_material, dim3((n + 255) / 256), dim3(256), 0, nullptr, (const float*)d[0], (int)n,
                           (float*)d[1]);
    });
}

}  // extern "C"
