// rtg_phys.h — the physical material model of rtg_set_material_model(.., RTG_MATERIALS_PHYSICAL):
// GGX conductor, plastic (a dielectric GGX coat over a diffuse base) and Oren-Nayar, in the local
// shading frame (z = the shading normal). include/rtg.h has the definition; this is its device
// form, IEEE float32 in the order written (the unit is compiled with -ffp-contract=off), using only
// + - * /, sqrtf and rtm_sincosf / rtm_acosf, so tests/materials_ref.py restates it bit for bit.
// k_shade_phys (rtg_shade_phys.hip) and k_probe_material share these bodies.
#pragma once
#include "rtg_dev.h"
#include "../../../include/rtg.h"

namespace rtgd {

// One parameter record (48 B, three 16-byte pieces): the table k_shade_phys indexes per triangle.
struct __align__(16) PhysMat {
    float4 a;  // model tag (int bits), alpha, sigma, int_ior
    float4 b;  // eta.rgb, ext_ior
    float4 c;  // k.rgb, -
};
// kernel argument of the k_shade_phys family alone
struct PhysArgs {
    const PhysMat* table;    // unique parameter records
    const unsigned* index;   // [triangle] -> record
    int n;                   // records (TAB: at most RTG_LDS_PHYS, held in LDS)
};

RTG_D float phys_clamp01(float x) { return wmax(0.0f, wmin(x, 1.0f)); }

// ---- the three GGX functions the reference leaves empty (ShadingHelper::Dggx / lambdaGGX / Gggx)
RTG_D float ggx_d(v3 h, float alpha) {
    const float a2 = alpha * alpha;
    const float t = ((h.z * h.z) * (a2 - 1.0f)) + 1.0f;
    return a2 / ((RTG_PI_F * t) * t);
}
RTG_D float ggx_lambda(v3 w, float alpha) {
    const float a2 = alpha * alpha;
    const float t2 = ((w.x * w.x) + (w.y * w.y)) / (w.z * w.z);
    return (sqrtf(1.0f + (a2 * t2)) - 1.0f) * 0.5f;
}
RTG_D float ggx_g1(v3 w, float alpha) { return 1.0f / (1.0f + ggx_lambda(w, alpha)); }
RTG_D float ggx_g(v3 wi, v3 wo, float alpha) { return ggx_g1(wi, alpha) * ggx_g1(wo, alpha); }

// ShadingHelper::fresnelCondutor (Materials.h:78-91) for one channel, operation for operation; a zero
// denominator (eta = k = 0) gives that half 1
RTG_D float fresnel_conductor1(float c, float eta, float k) {
    const float cos2 = c * c;
    const float sin2 = 1 - cos2;
    const float n2k2 = (eta * eta) + (k * k);
    const float e2c = (eta * 2.0f) * c;
    const float pa_n = ((n2k2 * cos2) - e2c) + sin2, pa_d = ((n2k2 * cos2) + e2c) + sin2;
    const float pe_n = (n2k2 - e2c) + cos2, pe_d = (n2k2 + e2c) + cos2;
    const float pa = pa_d > 0.0f ? pa_n / pa_d : 1.0f;
    const float pe = pe_d > 0.0f ? pe_n / pe_d : 1.0f;
    return (pa + pe) * 0.5f;
}
RTG_D v3 fresnel_conductor(float c, const PhysMat& q) {
    return mk(fresnel_conductor1(c, q.b.x, q.c.x), fresnel_conductor1(c, q.b.y, q.c.y),
              fresnel_conductor1(c, q.b.z, q.c.z));
}
// fresnelDielectric entering the coat from outside, as GlassBSDF calls it (Materials.h:265-275)
RTG_D float fresnel_coat(float c, const PhysMat& q) {
    v3 wt = mk(0.0f, 0.0f, 0.0f);
    return fresnel_dielectric(phys_clamp01(c), q.b.w, q.a.w, wt, wt);
}

// The half vector of (wo, wi) and the cosine both make with it, ch = |wo + wi| / 2 (the same bits with
// the arguments swapped). False: wo + wi = 0.
RTG_D bool phys_half(v3 wo, v3 wi, v3& h, float& ch) {
    const v3 hs = add(wo, wi);
    const float l2 = length_sq(hs);
    if (!(l2 > 0.0f)) return false;
    const float inv = 1.0f / sqrtf(l2);
    h = muls(hs, inv);
    ch = phys_clamp01(0.5f * (l2 * inv));
    return true;
}
// D G / (4 wo.z wi.z)
RTG_D float ggx_spec(v3 wo, v3 wi, v3 h, float alpha) {
    return (ggx_d(h, alpha) * ggx_g(wi, wo, alpha)) / ((4.0f * wo.z) * wi.z);
}
// the visible-normal density of wi: G1(wo) D(h) / (4 wo.z)
RTG_D float ggx_vndf_pdf(v3 wo, v3 h, float alpha) { return (ggx_g1(wo, alpha) * ggx_d(h, alpha)) / (4.0f * wo.z); }
// the plastic's lobe choice: the coat with probability 0.25 + 0.5 F_d(wo.z), in [0.25, 0.75]
RTG_D float plastic_ps(float fo) { return 0.25f + (0.5f * fo); }

RTG_D float oren_nayar_scale(float sigma, v3 wo, v3 wi) {
    const float s2 = sigma * sigma;
    const float A = 1.0f - (s2 / (2.0f * (s2 + 0.33f)));
    const float B = (0.45f * s2) / (s2 + 0.09f);
    const float cp = wmax(0.0f, (wi.x * wo.x) + (wi.y * wo.y));
    return A + ((B * cp) / wmax(wi.z, wo.z));
}

// evaluate(wo, wi) of the non-delta lobes; local directions. 0 unless wo.z > 0 and wi.z > 0.
RTG_D v3 phys_eval(const PhysMat& q, v3 alb, v3 wo, v3 wi) {
    const v3 zero = mk(0.0f, 0.0f, 0.0f);
    if (!(wo.z > 0.0f) || !(wi.z > 0.0f)) return zero;
    const int tag = __float_as_int(q.a.x);
    const float alpha = q.a.y;
    if (tag == RTG_MODEL_ORENNAYAR) return muls(divs_pi(alb), oren_nayar_scale(q.a.z, wo, wi));
    v3 h;
    float ch;
    const bool lobe = !(alpha < RTG_ALPHA_DELTA) && phys_half(wo, wi, h, ch);
    if (tag == RTG_MODEL_CONDUCTOR) {
        if (!lobe) return zero;
        return muls(mul(alb, fresnel_conductor(ch, q)), ggx_spec(wo, wi, h, alpha));
    }
    // RTG_MODEL_PLASTIC
    const float kd = (1.0f - fresnel_coat(wo.z, q)) * (1.0f - fresnel_coat(wi.z, q));
    const v3 fd = muls(divs_pi(alb), kd);
    if (!lobe) return fd;
    const float sp = fresnel_coat(ch, q) * ggx_spec(wo, wi, h, alpha);
    return mk(fd.x + sp, fd.y + sp, fd.z + sp);
}

// PDF(wo, wi) of sample()'s non-delta part, with respect to solid angle
RTG_D float phys_pdf(const PhysMat& q, v3 wo, v3 wi) {
    if (!(wo.z > 0.0f) || !(wi.z > 0.0f)) return 0.0f;
    const int tag = __float_as_int(q.a.x);
    const float alpha = q.a.y;
    if (tag == RTG_MODEL_ORENNAYAR) return div_pi_d(wi.z);
    v3 h;
    float ch;
    const bool lobe = !(alpha < RTG_ALPHA_DELTA) && phys_half(wo, wi, h, ch);
    const float pv = lobe ? ggx_vndf_pdf(wo, h, alpha) : 0.0f;
    if (tag == RTG_MODEL_CONDUCTOR) return pv;
    const float ps = plastic_ps(fresnel_coat(wo.z, q));
    return (ps * pv) + ((1.0f - ps) * div_pi_d(wi.z));
}

// Visible-normal sampling (Heitz 2018) of the GGX lobe: the reflected direction for draws u1, u2
RTG_D v3 ggx_sample_vndf(v3 wo, float alpha, float u1, float u2) {
    const v3 vh = normalize(mk(alpha * wo.x, alpha * wo.y, wo.z));
    const float lensq = (vh.x * vh.x) + (vh.y * vh.y);
    v3 t1 = mk(1.0f, 0.0f, 0.0f);
    if (lensq > 0.0f) {
        const float il = 1.0f / sqrtf(lensq);
        t1 = mk(-vh.y * il, vh.x * il, 0.0f);
    }
    const v3 t2 = cross(vh, t1);
    const float r = sqrtf(u1);
    float sn, cs;
    rtm_sincosf(6.2831855f * u2, &sn, &cs);
    const float p1 = r * cs;
    const float sh = 0.5f * (1.0f + vh.z);
    const float p2 = ((1.0f - sh) * sqrtf(wmax(0.0f, 1.0f - (p1 * p1)))) + (sh * (r * sn));
    const float p3 = sqrtf(wmax(0.0f, (1.0f - (p1 * p1)) - (p2 * p2)));
    const v3 nh = add(add(muls(t1, p1), muls(t2, p2)), muls(vh, p3));
    const v3 ne = normalize(mk(alpha * nh.x, alpha * nh.y, wmax(0.0f, nh.z)));
    const float d2 = 2.0f * dot(wo, ne);
    return sub(muls(ne, d2), wo);
}

// sample(): the local wi for the sampler's draws; colour = evaluate(wo, wi) and pdf = PDF(wo, wi) for a
// non-delta sample, the lobe's weight and choice probability for a delta one (delta = true: no cosine
// factor, canHitLight). pdf == 0 (wo.z <= 0, or wi below the surface): the path ends.
// Draws: conductor two (none when delta), plastic three (always), Oren-Nayar two.
template <class S>
RTG_D v3 phys_sample(const PhysMat& q, v3 alb, v3 wo, S& smp, v3& colour, float& pdf, bool& delta) {
    const int tag = __float_as_int(q.a.x);
    const float alpha = q.a.y;
    const bool dl = alpha < RTG_ALPHA_DELTA;
    const v3 mirror = mk(-wo.x, -wo.y, wo.z);
    colour = mk(0.0f, 0.0f, 0.0f);
    pdf = 0.0f;
    delta = false;
    v3 wi;
    if (tag == RTG_MODEL_CONDUCTOR) {
        if (dl) {
            if (!(wo.z > 0.0f)) return mirror;
            delta = true;
            colour = mul(alb, fresnel_conductor(phys_clamp01(wo.z), q));
            pdf = 1.0f;
            return mirror;
        }
        const float u1 = smp.next();
        const float u2 = smp.next();
        if (!(wo.z > 0.0f)) return mirror;
        wi = ggx_sample_vndf(wo, alpha, u1, u2);
    } else if (tag == RTG_MODEL_PLASTIC) {
        const float u0 = smp.next();
        const float u1 = smp.next();
        const float u2 = smp.next();
        if (!(wo.z > 0.0f)) return mirror;
        const float fo = fresnel_coat(wo.z, q);
        const float ps = plastic_ps(fo);
        if (u0 < ps) {
            if (dl) {
                delta = true;
                colour = mk(fo, fo, fo);
                pdf = ps;
                return mirror;
            }
            wi = ggx_sample_vndf(wo, alpha, u1, u2);
        } else {
            wi = cosine_sample_hemisphere(u2, u1);  // the first of the two draws -> r2, as the Lambert family
        }
    } else {  // RTG_MODEL_ORENNAYAR
        const float q2 = smp.next();
        const float q1 = smp.next();
        if (!(wo.z > 0.0f)) return mirror;
        wi = cosine_sample_hemisphere(q1, q2);
    }
    const float p = phys_pdf(q, wo, wi);
    if (p > 0.0f && p <= RTG_FLT_MAX) {
        pdf = p;
        colour = phys_eval(q, alb, wo, wi);
    }
    return wi;
}

}  // namespace rtgd
