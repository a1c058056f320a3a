// rtg_mis.h — rtg_set_path_mis(.., RTG_PATH_MIS_POWER) (include/rtg.h has the definition): the weight
// that combines the path tracer's NEE sample with its BSDF sample, and the solid-angle density the
// luminance table gives a direction. IEEE float32 in the order written (the unit is compiled with
// -ffp-contract=off), so tests/path_mis_ref.py restates both bit for bit. k_shade_mis
// (rtg_shade_mis.hip) and the probes k_probe_mis_weight / k_probe_env_pdf share these bodies.
#pragma once
#include "rtg_dev.h"

namespace rtgd {

// kernel argument of the k_shade_mis family alone
struct MisArgs {
    // [1 + triangle]: x the triangle's parameter record (PhysArgs::index's entry, 0 without a physical
    // table), y its index in the light list, -1: it is no light; [0]: y the environment light's index in
    // the light list, -1: it is not in it (one pointer and one load: the kernel is short of SGPRs)
    const uint2* index;
};

// The power heuristic with beta = 2 for a sample drawn with density p against the other technique's q:
// p^2 / (p^2 + q^2) as 1 / (1 + (q / p)^2), which cannot come to inf / inf for a finite p > 0. Not a
// number (both densities 0, or both infinite): 0.5, so both sides of a pair get the same value.
RTG_D float mis_w(float p, float q) {
    const float r = q / p;
    const float w = 1.0f / (1.0f + (r * r));
    return (w == w) ? w : 0.5f;
}

// The density env_sample_luminance (rtg_dev.h) reports for direction d: the cell of d by
// EnvironmentMap::evaluate's own (atan2f(z, x), acosf(y)) mapping (env_lookup), the cell's own cellpdf
// (word 2 of its entry), over sin theta = sqrtf((d.x d.x) + (d.z d.z)). A pole (!(st > 0)): 0, as the
// sampler rejects it.
RTG_D float env_pdf_luminance(const EnvTable& e, v3 d) {
    float u = rtm_atan2f(d.z, d.x);
    u = (u < 0.0f) ? (float)((double)u + 2.0 * RTM_PI) : u;
    u = div_2pi_d(u);
    const float v = div_pi_d(rtm_acosf(d.y));
    const float fx = floorf(u * (float)e.w), fy = floorf(v * (float)e.h);
    // u = 1 or v = 1 (a rounded-up seam or the lower pole) belongs to the last cell; not a number: cell 0
    const unsigned cx = (fx >= 0.0f) ? ((fx < (float)e.w) ? (unsigned)fx : e.w - 1u) : 0u;
    const unsigned cy = (fy >= 0.0f) ? ((fy < (float)e.h) ? (unsigned)fy : e.h - 1u) : 0u;
    const float cp = __uint_as_float(e.table[cy * e.w + cx].z);
    const float st = sqrtf((d.x * d.x) + (d.z * d.z));
    if (!(st > 0.0f)) return 0.0f;
    return cp / st;
}

}  // namespace rtgd
