"""TEST INFRASTRUCTURE ONLY — numpy float32 restatement of the rough dielectric of include/rtg.h
(RTG_MODEL_ROUGH_DIELECTRIC under RTG_MATERIALS_PHYSICAL), written from the header's text, operation by
operation in the order it states, on tests/materials_ref.py's pieces (its GGX functions, fresnelDielectric,
frames and the oracle library's sincosf). Vectors are lists of three float32 arrays in the local shading
frame unless a function says otherwise; wo and wi may lie anywhere on the sphere.
"""
import numpy as np

import materials_ref as R

F = np.float32
ROUGH_DIELECTRIC = 5
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


class Params:
    """One tag-5 rtg_material_params record as float32 scalars."""

    def __init__(self, alpha, int_ior=1.5, ext_ior=1.0):
        self.model = ROUGH_DIELECTRIC
        self.alpha, self.int_ior, self.ext_ior = F(alpha), F(int_ior), F(ext_ior)

    @property
    def delta(self):
        return bool(self.alpha < R.ALPHA_DELTA)


def neg(a):
    return [-a[0], -a[1], -a[2]]


def pick(c, a, b):
    return [np.where(c, a[k], b[k]).astype(F) for k in range(3)]


def fresnel_out(q, c_ext):
    """F at the exterior-side cosine: fresnelDielectric at clamp01(c_ext) with iorInt = ext_ior, iorExt = int_ior."""
    with np.errstate(**_ERR):
        return R.fresnel_dielectric(R.clamp01(np.asarray(c_ext, F)), q.ext_ior, q.int_ior)


def fresnel(q, s, c):
    """F for a cosine c on wo's side: fresnel_out(c) where wo is outside (s); from inside at the exterior
    cosine of Snell's law, r = int_ior / ext_ior, s2 = (r r) (1 - (c c)), 1 when s2 > 1."""
    with np.errstate(**_ERR):
        cc = R.clamp01(np.asarray(c, F))
        r = q.int_ior / q.ext_ior
        s2 = (r * r) * (F(1) - (cc * cc))
        inner = np.where(s2 > F(1), F(1), fresnel_out(q, np.sqrt(F(1) - s2))).astype(F)
        return np.where(s, fresnel_out(q, c), inner).astype(F)


def sides(q, wo):
    """(s, eta_i, eta_t, wo'): the side wo lies on, the indices there and beyond, wo flipped into z > 0."""
    s = wo[2] > 0
    eta_i = np.where(s, q.ext_ior, q.int_ior).astype(F)
    eta_t = np.where(s, q.int_ior, q.ext_ior).astype(F)
    return s, eta_i, eta_t, pick(s, wo, neg(wo))


def vndf_normal(wo, alpha, u1, u2):
    """The sampled visible normal ne of wo (wo.z > 0): materials_ref.sample_vndf up to its last two lines."""
    with np.errstate(**_ERR):
        vh = R.normalize([alpha * wo[0], alpha * wo[1], wo[2]])
        lensq = (vh[0] * vh[0]) + (vh[1] * vh[1])
        il = F(1) / np.sqrt(lensq)
        pos = lensq > 0
        t1 = [np.where(pos, -vh[1] * il, F(1)).astype(F), np.where(pos, vh[0] * il, F(0)).astype(F),
              np.zeros_like(lensq)]
        t2 = R.cross(vh, t1)
        r = np.sqrt(u1)
        sn, cs = R.sincosf(F(6.2831855) * u2)
        p1 = r * cs
        sh = F(0.5) * (F(1) + vh[2])
        p2 = ((F(1) - sh) * np.sqrt(R.wmax(F(0), F(1) - (p1 * p1)))) + (sh * (r * sn))
        p3 = np.sqrt(R.wmax(F(0), (F(1) - (p1 * p1)) - (p2 * p2)))
        nh = [((t1[k] * p1) + (t2[k] * p2)) + (vh[k] * p3) for k in range(3)]
        return R.normalize([alpha * nh[0], alpha * nh[1], R.wmax(F(0), nh[2])])


def terms(q, wo, wi):
    """(f, pdf, reflection side, transmission side): evaluate / albedo and PDF, (n,) float32 each, and the
    masks of the pairs each lobe serves (both False: 0)."""
    wo = [np.asarray(c, F) for c in wo]
    wi = [np.asarray(c, F) for c in wi]
    n = len(wo[0])
    zero = np.zeros(n, F)
    if q.delta:
        return zero, zero.copy(), np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(**_ERR):
        s, eta_i, eta_t, o = sides(q, wo)
        side = s | (wo[2] < 0)
        i = pick(s, wi, neg(wi))
        # the reflection side
        okh, h, ch = R.half(o, i)
        Fr = fresnel(q, s, ch)
        f_r = Fr * R.ggx_spec(o, i, h, q.alpha)
        p_r = Fr * R.ggx_vndf_pdf(o, h, q.alpha)
        refl = side & (i[2] > 0) & okh
        # the transmission side
        hs = neg([(o[k] * eta_i) + (i[k] * eta_t) for k in range(3)])
        l2 = R.dot(hs, hs)
        inv = F(1) / np.sqrt(l2)
        h = [hs[k] * inv for k in range(3)]
        h = pick(h[2] < 0, neg(h), h)
        coh, cih = R.dot(o, h), R.dot(i, h)
        aci, aiz = -cih, -i[2]
        T = F(1) - fresnel_out(q, np.where(s, coh, aci))
        den = (eta_i * coh) + (eta_t * cih)
        den2, et2 = den * den, eta_t * eta_t
        D, g1o = R.ggx_d(h, q.alpha), R.ggx_g1(o, q.alpha)
        f_t = (((coh * aci) * et2) * (T * (D * (R.ggx_g1(i, q.alpha) * g1o)))) / ((o[2] * aiz) * den2)
        p_t = (T * (((g1o * coh) * D) / o[2])) * ((et2 * aci) / den2)
        tran = side & (i[2] < 0) & (l2 > 0) & (coh > 0) & (cih < 0)
        f = np.where(refl, f_r, np.where(tran, f_t, F(0))).astype(F)
        p = np.where(refl, p_r, np.where(tran, p_t, F(0))).astype(F)
    return f, p, refl, tran


def raw_pdfs(q, wo, wi):
    """The two lobes' densities of wi before the hemisphere test: the reflection about, and the refraction
    through, a visible normal of wo, wherever wi points (the part on the wrong side of the surface is what
    sample() discards). (p_r, p_t), (n,) float32 each."""
    wo = [np.asarray(c, F) for c in wo]
    wi = [np.asarray(c, F) for c in wi]
    with np.errstate(**_ERR):
        s, eta_i, eta_t, o = sides(q, wo)
        i = pick(s, wi, neg(wi))
        okh, h, ch = R.half(o, i)
        p_r = fresnel(q, s, ch) * R.ggx_vndf_pdf(o, h, q.alpha)
        p_r = np.where(okh & (h[2] > 0), p_r, F(0)).astype(F)
        hs = neg([(o[k] * eta_i) + (i[k] * eta_t) for k in range(3)])
        l2 = R.dot(hs, hs)
        inv = F(1) / np.sqrt(l2)
        h = [hs[k] * inv for k in range(3)]
        h = pick(h[2] < 0, neg(h), h)
        coh, cih = R.dot(o, h), R.dot(i, h)
        den = (eta_i * coh) + (eta_t * cih)
        T = F(1) - fresnel_out(q, np.where(s, coh, -cih))
        p_t = (T * (((R.ggx_g1(o, q.alpha) * coh) * R.ggx_d(h, q.alpha)) / o[2])) * (((eta_t * eta_t) * -cih) / (den * den))
        p_t = np.where((l2 > 0) & (coh > 0) & (cih < 0), p_t, F(0)).astype(F)
    return p_r, p_t


def transmission_factor(q, wo, wi):
    """1 - F at the half vector of the transmission side, as terms() forms it: (n,) float32."""
    wo = [np.asarray(c, F) for c in wo]
    wi = [np.asarray(c, F) for c in wi]
    with np.errstate(**_ERR):
        s, eta_i, eta_t, o = sides(q, wo)
        i = pick(s, wi, neg(wi))
        hs = neg([(o[k] * eta_i) + (i[k] * eta_t) for k in range(3)])
        inv = F(1) / np.sqrt(R.dot(hs, hs))
        h = [hs[k] * inv for k in range(3)]
        h = pick(h[2] < 0, neg(h), h)
        return F(1) - fresnel_out(q, np.where(s, R.dot(o, h), -R.dot(i, h)))


def evaluate(q, alb, wo, wi):
    """evaluate(wo, wi): (n, 3) float32. alb: three floats, or three arrays (one albedo per pair)."""
    f = terms(q, wo, wi)[0]
    return np.stack([(np.asarray(a, F) * f).astype(F) for a in alb], axis=1)


def pdf(q, wo, wi):
    return terms(q, wo, wi)[1]


def sample(q, alb, wo, draws):
    """The non-delta sample() for local wo and draws (n, 3): a dict of "wi" (local, list of 3), "colour"
    (n, 3), "pdf", "draws" (consumed: 3), "delta" (False), "reflect" (the lobe u0 chose), "F" and "c"."""
    assert not q.delta
    d = np.asarray(draws, F).reshape(-1, 3)
    n = len(d)
    wo = [np.asarray(c, F) for c in wo]
    with np.errstate(**_ERR):
        s, eta_i, eta_t, o = sides(q, wo)
        side = s | (wo[2] < 0)
        m = vndf_normal(o, q.alpha, d[:, 1], d[:, 2])
        dm = R.dot(o, m)
        c = R.clamp01(dm)
        Fr = fresnel(q, s, c)
        reflect = d[:, 0] < Fr
        i_r = [(m[k] * (F(2) * dm)) - o[k] for k in range(3)]
        eta = eta_t / eta_i
        kk = F(1) - ((F(1) - (c * c)) / (eta * eta))
        a = (c / eta) - np.sqrt(kk)
        i_t = [(m[k] * a) - (o[k] / eta) for k in range(3)]
        i = pick(reflect, i_r, i_t)
        ok = side & np.where(reflect, i[2] > 0, i[2] < 0)
        wi = pick(s, i, neg(i))
        wi = pick(side, wi, [-wo[0], -wo[1], wo[2]])
        f, p, _, _ = terms(q, wo, wi)
        good = ok & (p > 0) & (p <= R.FLT_MAX)
        p = np.where(good, p, F(0)).astype(F)
        col = np.stack([np.where(good, np.asarray(al, F) * f, F(0)).astype(F) for al in alb], axis=1)
    return {"wi": wi, "colour": col, "pdf": p, "draws": np.full(n, 3, np.int32), "delta": np.zeros(n, bool),
            "reflect": reflect, "F": Fr, "c": c}
