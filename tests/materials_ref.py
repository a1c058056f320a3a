"""TEST INFRASTRUCTURE ONLY — numpy float32 restatement of the physical material model of include/rtg.h
(rtg_set_material_model, RTG_MATERIALS_PHYSICAL), written from the header's text, operation by operation
in the order it states (numpy's float32 +, -, *, / and sqrt are IEEE, one rounding each, as the kernel's
without contraction). sincosf and acosf are include/rtg_math.h's, through the oracle library built from it
(or_math_eval). Vectors are lists of three float32 arrays; directions are in the local shading frame
unless a function says otherwise.
"""
import ctypes as C

import numpy as np

from oracle.pyoracle import lib

F = np.float32
CONDUCTOR, PLASTIC, ORENNAYAR = 1, 2, 3
ALPHA_DELTA = F(0.01)
PI_F = F(3.14159274)
FLT_MAX = F(3.40282347e+38)
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


class Params:
    """One rtg_material_params record as float32 scalars."""

    def __init__(self, model, alpha=0.0, sigma=0.0, eta=(0.0, 0.0, 0.0), k=(0.0, 0.0, 0.0), int_ior=1.33,
                 ext_ior=1.0):
        self.model = {"conductor": CONDUCTOR, "plastic": PLASTIC, "orennayar": ORENNAYAR}.get(model, model)
        self.alpha, self.sigma = F(alpha), F(sigma)
        self.eta, self.k = [F(v) for v in eta], [F(v) for v in k]
        self.int_ior, self.ext_ior = F(int_ior), F(ext_ior)

    @property
    def delta(self):
        return self.model != ORENNAYAR and bool(self.alpha < ALPHA_DELTA)


def _math(fn, x, per=1):
    t = np.ascontiguousarray(x, F).reshape(-1)
    out = np.zeros(per * len(t), F)
    lib("rtm").or_math_eval(fn, t.ctypes.data_as(C.POINTER(C.c_float)), len(t), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def sincosf(x):
    o = _math(2, x, 2)
    return o[0::2].copy(), o[1::2].copy()


def acosf(x):
    return _math(3, x)


def vec(a):
    """(n, 3) array -> list of three float32 arrays."""
    a = np.asarray(a, F).reshape(-1, 3)
    return [a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()]


def arr(v):
    return np.stack([np.asarray(c, F) for c in v], axis=1)


def dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def normalize(a):
    l = F(1) / np.sqrt(dot(a, a))
    return [a[0] * l, a[1] * l, a[2] * l]


def cross(a, b):
    return [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]


def wmax(a, b):
    return np.where(a > b, a, b).astype(F)


def wmin(a, b):
    return np.where(a < b, a, b).astype(F)


def clamp01(x):
    return wmax(F(0), wmin(x, F(1)))


def div_pi_f(x):  # x / (float)M_PI, as the kernels' product with the binary64 reciprocal
    return (np.asarray(x, F).astype(np.float64) * (1.0 / float(PI_F))).astype(F)


def div_pi_d(x):  # (float)((double)x / M_PI)
    return (np.asarray(x, F).astype(np.float64) * (1.0 / np.pi)).astype(F)


# ------------------------------------------------------------------ Frame::fromVector (Core.h:507-542)
def frame_from(n):
    """The frame (u, v, w) of shading normal(s) n: three floats, or an (m, 3) array (one frame per row)."""
    w = normalize(vec(np.asarray(n, F).reshape(-1, 3)))
    zero = np.zeros_like(w[0])
    with np.errstate(**_ERR):
        lx = F(1) / np.sqrt(w[0] * w[0] + w[2] * w[2])
        ly = F(1) / np.sqrt(w[1] * w[1] + w[2] * w[2])
        first = np.abs(w[0]) > np.abs(w[1])
        u = [np.where(first, w[2] * lx, zero).astype(F), np.where(first, zero, w[2] * ly).astype(F),
             np.where(first, -w[0] * lx, -w[1] * ly).astype(F)]
    return u, cross(w, u), w


def to_local(fr, a):
    return [dot(a, fr[0]), dot(a, fr[1]), dot(a, fr[2])]


def to_world(fr, a):
    return [((fr[0][k] * a[0]) + (fr[1][k] * a[1])) + (fr[2][k] * a[2]) for k in range(3)]


# ------------------------------------------------------------------ GGX pieces
def ggx_d(h, alpha):
    a2 = alpha * alpha
    t = ((h[2] * h[2]) * (a2 - F(1))) + F(1)
    return a2 / ((PI_F * t) * t)


def ggx_lambda(w, alpha):
    a2 = alpha * alpha
    t2 = ((w[0] * w[0]) + (w[1] * w[1])) / (w[2] * w[2])
    return (np.sqrt(F(1) + (a2 * t2)) - F(1)) * F(0.5)


def ggx_g1(w, alpha):
    return F(1) / (F(1) + ggx_lambda(w, alpha))


def ggx_g(wi, wo, alpha):
    return ggx_g1(wi, alpha) * ggx_g1(wo, alpha)


def fresnel_conductor1(c, eta, k):
    cos2 = c * c
    sin2 = F(1) - cos2
    n2k2 = (eta * eta) + (k * k)
    e = (eta * F(2)) * c
    pa_n, pa_d = ((n2k2 * cos2) - e) + sin2, ((n2k2 * cos2) + e) + sin2
    pe_n, pe_d = (n2k2 - e) + cos2, (n2k2 + e) + cos2
    pa = np.where(pa_d > 0, pa_n / pa_d, F(1)).astype(F)
    pe = np.where(pe_d > 0, pe_n / pe_d, F(1)).astype(F)
    return (pa + pe) * F(0.5)


def fresnel_conductor(c, q):
    return [fresnel_conductor1(c, q.eta[k], q.k[k]) for k in range(3)]


def fresnel_dielectric(cos_i, ior_int, ior_ext):
    """fresnelDielectric (Materials.h:55-77): R alone."""
    ior = ior_int / ior_ext
    sin_i = np.sqrt(F(1) - (cos_i * cos_i))
    sin_t = ior * sin_i
    ior2sin2 = (ior * ior) * (F(1) - (cos_i * cos_i))
    cos_t = np.sqrt(F(1) - (sin_t * sin_t))
    fpa = (cos_i - ior * cos_t) / (cos_i + ior * cos_t)
    fpe = (ior * cos_i - cos_t) / (ior * cos_i + ior * cos_t)
    avg = ((fpa * fpa) + (fpe * fpe)) * F(0.5)
    m = np.where(avg < F(1), avg, F(1)).astype(F)   # std::min(1, avg) = (avg < 1) ? avg : 1
    r = np.where(F(0) < m, m, F(0)).astype(F)       # std::max(0, m) = (0 < m) ? m : 0
    return np.where(ior2sin2 > F(1), F(1), r).astype(F)


def fresnel_coat(c, q):
    return fresnel_dielectric(clamp01(np.asarray(c, F)), q.ext_ior, q.int_ior)


def half(wo, wi):
    """(ok, h, ch)."""
    hs = [wo[k] + wi[k] for k in range(3)]
    l2 = dot(hs, hs)
    ok = l2 > 0
    inv = F(1) / np.sqrt(l2)
    return ok, [hs[k] * inv for k in range(3)], clamp01(F(0.5) * (l2 * inv))


def ggx_spec(wo, wi, h, alpha):
    return (ggx_d(h, alpha) * ggx_g(wi, wo, alpha)) / ((F(4) * wo[2]) * wi[2])


def ggx_vndf_pdf(wo, h, alpha):
    return (ggx_g1(wo, alpha) * ggx_d(h, alpha)) / (F(4) * wo[2])


def plastic_ps(fo):
    return F(0.25) + (F(0.5) * fo)


def oren_nayar_scale(sigma, wo, wi):
    s2 = sigma * sigma
    A = F(1) - (s2 / (F(2) * (s2 + F(0.33))))
    B = (F(0.45) * s2) / (s2 + F(0.09))
    cp = wmax(F(0), (wi[0] * wo[0]) + (wi[1] * wo[1]))
    return A + ((B * cp) / wmax(wi[2], wo[2]))


# ------------------------------------------------------------------ evaluate / PDF / sample
def evaluate(q, alb, wo, wi):
    """evaluate(wo, wi): (n, 3) float32. alb: three floats, or three arrays (one albedo per direction pair)."""
    alb = [np.asarray(c, F) for c in alb]
    with np.errstate(**_ERR):
        up = (wo[2] > 0) & (wi[2] > 0)
        if q.model == ORENNAYAR:
            sc = oren_nayar_scale(q.sigma, wo, wi)
            f = [div_pi_f(np.broadcast_to(a, sc.shape)) * sc for a in alb]
        else:
            ok, h, ch = half(wo, wi)
            lobe = ok & (not q.delta)
            sp = ggx_spec(wo, wi, h, q.alpha)
            if q.model == CONDUCTOR:
                Fc = fresnel_conductor(ch, q)
                f = [np.where(lobe, (alb[k] * Fc[k]) * sp, F(0)) for k in range(3)]
            else:
                kd = (F(1) - fresnel_coat(wo[2], q)) * (F(1) - fresnel_coat(wi[2], q))
                s = fresnel_coat(ch, q) * sp
                f = []
                for k in range(3):
                    fd = div_pi_f(np.broadcast_to(alb[k], kd.shape)) * kd
                    f.append(np.where(lobe, fd + s, fd))
        return np.stack([np.where(up, c, F(0)).astype(F) for c in f], axis=1)


def pdf(q, wo, wi):
    """PDF(wo, wi): (n,) float32."""
    with np.errstate(**_ERR):
        up = (wo[2] > 0) & (wi[2] > 0)
        if q.model == ORENNAYAR:
            p = div_pi_d(wi[2])
        else:
            ok, h, _ = half(wo, wi)
            lobe = ok & (not q.delta)
            pv = np.where(lobe, ggx_vndf_pdf(wo, h, q.alpha), F(0)).astype(F)
            if q.model == CONDUCTOR:
                p = pv
            else:
                ps = plastic_ps(fresnel_coat(wo[2], q))
                p = (ps * pv) + ((F(1) - ps) * div_pi_d(wi[2]))
        return np.where(up, p, F(0)).astype(F)


def sample_vndf(wo, alpha, u1, u2):
    with np.errstate(**_ERR):
        vh = normalize([alpha * wo[0], alpha * wo[1], wo[2]])
        lensq = (vh[0] * vh[0]) + (vh[1] * vh[1])
        il = F(1) / np.sqrt(lensq)
        pos = lensq > 0
        t1 = [np.where(pos, -vh[1] * il, F(1)).astype(F), np.where(pos, vh[0] * il, F(0)).astype(F),
              np.zeros_like(lensq)]
        t2 = cross(vh, t1)
        r = np.sqrt(u1)
        sn, cs = sincosf(F(6.2831855) * u2)
        p1 = r * cs
        sh = F(0.5) * (F(1) + vh[2])
        p2 = ((F(1) - sh) * np.sqrt(wmax(F(0), F(1) - (p1 * p1)))) + (sh * (r * sn))
        p3 = np.sqrt(wmax(F(0), (F(1) - (p1 * p1)) - (p2 * p2)))
        nh = [((t1[k] * p1) + (t2[k] * p2)) + (vh[k] * p3) for k in range(3)]
        ne = normalize([alpha * nh[0], alpha * nh[1], wmax(F(0), nh[2])])
        d2 = F(2) * dot(wo, ne)
        return [(ne[k] * d2) - wo[k] for k in range(3)]


def cosine_sample_hemisphere(r1, r2):
    theta = acosf(np.sqrt(r1))
    phi = ((2.0 * np.pi) * np.asarray(r2, F).astype(np.float64)).astype(F)
    st, ct = sincosf(theta)
    sp, cp = sincosf(phi)
    return [cp * st, sp * st, ct]


def sample(q, alb, wo, draws):
    """sample() for local wo and draws (n, 3): a dict of "wi" (local, list of 3), "colour" (n, 3), "pdf",
    "draws" (consumed), "delta"."""
    d = np.asarray(draws, F).reshape(-1, 3)
    n = len(d)
    alb3 = [F(c) for c in alb]
    mirror = [-wo[0], -wo[1], wo[2]]
    up = wo[2] > 0
    zero3 = np.zeros((n, 3), F)
    if q.model == CONDUCTOR and q.delta:
        Fc = fresnel_conductor(clamp01(wo[2]), q)
        col = np.stack([alb3[k] * Fc[k] for k in range(3)], axis=1)
        return {"wi": mirror, "colour": np.where(up[:, None], col, zero3).astype(F),
                "pdf": np.where(up, F(1), F(0)).astype(F), "draws": np.zeros(n, np.int32), "delta": up.copy()}
    used = np.full(n, 3 if q.model == PLASTIC else 2, np.int32)
    delta = np.zeros(n, bool)
    dcol = zero3.copy()
    dpdf = np.zeros(n, F)
    if q.model == CONDUCTOR:
        wi = sample_vndf(wo, q.alpha, d[:, 0], d[:, 1])
    elif q.model == PLASTIC:
        fo = fresnel_coat(wo[2], q)
        ps = plastic_ps(fo)
        coat = d[:, 0] < ps
        base = cosine_sample_hemisphere(d[:, 2], d[:, 1])
        if q.delta:
            delta = coat & up
            dcol = np.stack([fo, fo, fo], axis=1)
            dpdf = ps
            wi = [np.where(coat, mirror[k], base[k]).astype(F) for k in range(3)]
        else:
            spec = sample_vndf(wo, q.alpha, d[:, 1], d[:, 2])
            wi = [np.where(coat, spec[k], base[k]).astype(F) for k in range(3)]
    else:
        wi = cosine_sample_hemisphere(d[:, 1], d[:, 0])
    wi = [np.where(up, wi[k], mirror[k]).astype(F) for k in range(3)]
    p = pdf(q, wo, wi)
    good = (p > 0) & (p <= FLT_MAX) & up & ~delta
    col = evaluate(q, alb, wo, wi)
    col = np.where(good[:, None], col, zero3)
    col = np.where(delta[:, None], dcol, col).astype(F)
    p = np.where(delta, dpdf, np.where(good, p, F(0))).astype(F)
    return {"wi": wi, "colour": col, "pdf": p, "draws": used, "delta": delta}
