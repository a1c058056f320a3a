// rtg_trans.h — rough dielectric transmission (RTG_MODEL_ROUGH_DIELECTRIC) of the physical material
// model: the microfacet refraction model of Walter et al. 2007 on rtg_phys.h's GGX pieces, in the local
// shading frame (z = the shading normal, which is not flipped for a dielectric: wo.z may be negative).
// include/rtg.h has the definition; this is its device form, IEEE float32 in the order written (the unit
// is compiled with -ffp-contract=off), using only + - * /, sqrtf and rtm_sincosf, so
// tests/transmission_ref.py restates it bit for bit. k_shade_trans (rtg_shade_trans.hip) and
// k_probe_transmission share these bodies. The record is rtg_phys.h's PhysMat: a.y alpha, a.w int_ior,
// b.w ext_ior.
#pragma once
#include "rtg_phys.h"

namespace rtgd {

// ggx_sample_vndf (rtg_phys.h) up to its sampled normal ne: the visible normal of wo (wo.z > 0)
RTG_D v3 ggx_sample_vndf_normal(v3 wo, float alpha, float u1, float u2) {
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
    return normalize(mk(alpha * nh.x, alpha * nh.y, wmax(0.0f, nh.z)));
}

// F at the interface, the same number from both of its sides (the transmission lobe is reciprocal only then,
// and fresnelDielectric's own value is not: its perpendicular term is not Fresnel's). It is fresnelDielectric
// at the cosine on the exterior side, entering as GlassBSDF calls it from outside (iorInt = ext_ior, iorExt =
// int_ior; total internal reflection: 1) ...
RTG_D float trans_fresnel_out(float c_ext, const PhysMat& q) {
    v3 wt = mk(0.0f, 0.0f, 0.0f);
    return fresnel_dielectric(phys_clamp01(c_ext), q.b.w, q.a.w, wt, wt);
}
// ... so for a cosine c on wo's side: itself when wo is outside (s); from inside the exterior cosine Snell's law
// gives it, total internal reflection (1) when there is none
RTG_D float trans_fresnel(float c, bool s, const PhysMat& q) {
    if (s) return trans_fresnel_out(c, q);
    const float cc = phys_clamp01(c);
    const float r = q.a.w / q.b.w;
    const float s2 = (r * r) * (1.0f - (cc * cc));
    if (s2 > 1.0f) return 1.0f;
    return trans_fresnel_out(sqrtf(1.0f - s2), q);
}

// evaluate(wo, wi) / albedo (the lobes are not tinted per channel) and PDF(wo, wi) on the whole sphere.
// False: both are 0 (a delta record, wo or wi on the horizon, or a pair no microfacet connects).
RTG_D bool trans_terms(const PhysMat& q, v3 wo, v3 wi, float& f, float& pdf) {
    f = 0.0f;
    pdf = 0.0f;
    const float alpha = q.a.y;
    if (alpha < RTG_ALPHA_DELTA) return false;
    const bool s = wo.z > 0.0f;
    if (!s && !(wo.z < 0.0f)) return false;
    const float eta_i = s ? q.b.w : q.a.w, eta_t = s ? q.a.w : q.b.w;
    const v3 o = s ? wo : neg(wo), i = s ? wi : neg(wi);
    if (i.z > 0.0f) {  // the reflection side
        v3 h;
        float ch;
        if (!phys_half(o, i, h, ch)) return false;
        const float F = trans_fresnel(ch, s, q);
        f = F * ggx_spec(o, i, h, alpha);
        pdf = F * ggx_vndf_pdf(o, h, alpha);
        return true;
    }
    if (!(i.z < 0.0f)) return false;
    // the transmission side
    const v3 hs = neg(add(muls(o, eta_i), muls(i, eta_t)));
    const float l2 = length_sq(hs);
    if (!(l2 > 0.0f)) return false;
    v3 h = muls(hs, 1.0f / sqrtf(l2));
    if (h.z < 0.0f) h = neg(h);
    const float coh = dot(o, h), cih = dot(i, h);
    if (!(coh > 0.0f) || !(cih < 0.0f)) return false;
    const float aci = -cih, aiz = -i.z;
    const float T = 1.0f - trans_fresnel_out(s ? coh : aci, q);  // the half vector's cosine on the exterior side
    const float den = (eta_i * coh) + (eta_t * cih);
    const float den2 = den * den, et2 = eta_t * eta_t;
    const float D = ggx_d(h, alpha), g1o = ggx_g1(o, alpha);
    f = (((coh * aci) * et2) * (T * (D * (ggx_g1(i, alpha) * g1o)))) / ((o.z * aiz) * den2);
    pdf = (T * (((g1o * coh) * D) / o.z)) * ((et2 * aci) / den2);
    return true;
}
RTG_D v3 trans_eval(const PhysMat& q, v3 alb, v3 wo, v3 wi) {
    float f, pdf;
    if (!trans_terms(q, wo, wi, f, pdf)) return mk(0.0f, 0.0f, 0.0f);
    return muls(alb, f);
}
RTG_D float trans_pdf(const PhysMat& q, v3 wo, v3 wi) {
    float f, pdf;
    trans_terms(q, wo, wi, f, pdf);
    return pdf;
}

// sample(): the world wi for the sampler's draws, wo in world space (bsdf_sample's interface, whose glass
// branch the delta limit is). Non-delta: three draws u0, u1, u2, always all three; colour = evaluate(wo,
// wi) and pdf = PDF(wo, wi) of the sampled wi; pdf == 0: the path ends. delta = true (alpha <
// RTG_ALPHA_DELTA): GlassBSDF::sample with the record's IORs, no cosine factor, canHitLight.
template <class S>
RTG_D v3 trans_sample(const PhysMat& q, v3 alb, const frame& fr, v3 wo_w, S& smp, v3& colour, float& pdf, bool& delta) {
    const float alpha = q.a.y;
    delta = alpha < RTG_ALPHA_DELTA;
    if (delta) return bsdf_sample(RTG_MAT_GLASS, q.a.w, q.b.w, alb, fr, wo_w, smp, colour, pdf);
    const float u0 = smp.next();
    const float u1 = smp.next();
    const float u2 = smp.next();
    const v3 wo = to_local(fr, wo_w);
    colour = mk(0.0f, 0.0f, 0.0f);
    pdf = 0.0f;
    const bool s = wo.z > 0.0f;
    if (!s && !(wo.z < 0.0f)) return to_world(fr, mk(-wo.x, -wo.y, wo.z));
    const float eta_i = s ? q.b.w : q.a.w, eta_t = s ? q.a.w : q.b.w;
    const v3 o = s ? wo : neg(wo);
    const v3 m = ggx_sample_vndf_normal(o, alpha, u1, u2);
    const float dm = dot(o, m);
    const float c = phys_clamp01(dm);
    const float F = trans_fresnel(c, s, q);
    v3 i;
    bool ok;
    if (u0 < F) {
        i = sub(muls(m, 2.0f * dm), o);
        ok = i.z > 0.0f;
    } else {
        const float eta = eta_t / eta_i;
        const float k = 1.0f - ((1.0f - (c * c)) / (eta * eta));
        const float a = (c / eta) - sqrtf(k);
        i = sub(muls(m, a), divs(o, eta));
        ok = i.z < 0.0f;
    }
    const v3 wi = s ? i : neg(i);
    if (ok) {
        float f, p;
        trans_terms(q, wo, wi, f, p);
        if (p > 0.0f && p <= RTG_FLT_MAX) {
            pdf = p;
            colour = muls(alb, f);
        }
    }
    return to_world(fr, wi);
}

}  // namespace rtgd
