"""TEST INFRASTRUCTURE ONLY — numpy float32 restatement of the path tracer's multiple importance sampling of
include/rtg.h (rtg_set_path_mis, RTG_PATH_MIS_POWER), written from the header's text, operation by
operation in the order it states (numpy's float32 +, -, *, / and sqrt are IEEE, one rounding each, as the
kernel's without contraction). Built on tests/materials_ref.py (the material model's PDF and sample),
tests/light_sampling_ref.py (the pick, Triangle::sample) and tests/env_sampling_ref.py (the luminance
sampler, EnvironmentMap::evaluate's coordinates, the PCG stream).
"""
import numpy as np

import env_sampling_ref as er
import light_sampling_ref as lr
import materials_ref as R

F = np.float32
U32 = np.uint32
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
UNIFORM_SPHERE_PDF = F(1.0 / (4.0 * er.PI))


def mis_w(p, q):
    """r = q / p; w = 1 / (1 + (r r)); a w that is not a number is 0.5."""
    p, q = np.asarray(p, F), np.asarray(q, F)
    with np.errstate(**_ERR):
        r = q / p
        w = F(1) / (F(1) + (r * r))
    return np.where(np.isnan(w), F(0.5), w).astype(F)


def pdf_area_to_solid(pdf_area, dist2, cos_theta):
    """convertPDFAreaToSolidAngle: cos > 0 ? (pdf_area dist2) / cos : 0."""
    pdf_area, dist2, cos_theta = (np.asarray(v, F) for v in (pdf_area, dist2, cos_theta))
    with np.errstate(**_ERR):
        v = (pdf_area * dist2) / cos_theta
    return np.where(cos_theta > 0, v, F(0)).astype(F)


def bsdf_pdf_lambert(w, wi):
    """cosineHemispherePDF(frame.toLocal(wi)): z = dot(wi, frame.w); z >= 0 ? z / M_PI (binary64) : 0.
    w: the frame's third axis, a list of three arrays; wi (n, 3)."""
    wi = np.asarray(wi, F).reshape(-1, 3)
    z = ((wi[:, 0] * w[0]) + (wi[:, 1] * w[1])) + (wi[:, 2] * w[2])
    return np.where(z >= 0, R.div_pi_d(z), F(0)).astype(F)


def env_cell(W, H, d):
    """The cell (cx, cy) of direction(s) d: floorf(u W), floorf(v H) of EnvironmentMap::evaluate's (u, v),
    clamped to the map (not a number: 0)."""
    u, v = er.env_uv(d)
    with np.errstate(**_ERR):
        fx, fy = np.floor(u * F(W)), np.floor(v * F(H))
        cx = np.where(fx >= 0, np.where(fx < F(W), fx, F(W - 1)), F(0)).astype(np.int64)
        cy = np.where(fy >= 0, np.where(fy < F(H), fy, F(H - 1)), F(0)).astype(np.int64)
    return cx, cy


def env_pdf(entries, W, H, d):
    """p_env(d) under RTG_ENV_LUMINANCE: the cell's own cellpdf (word 2 of its entry) over
    st = sqrtf((d.x d.x) + (d.z d.z)); !(st > 0): 0. entries None: uniformSpherePDF."""
    d = np.asarray(d, F).reshape(-1, 3)
    if entries is None:
        return np.full(len(d), UNIFORM_SPHERE_PDF, F)
    e = np.asarray(entries, U32).reshape(-1, 4)
    cx, cy = env_cell(W, H, d)
    cp = e[cy * W + cx, 2].copy().view(F)
    st = np.sqrt((d[:, 0] * d[:, 0]) + (d[:, 2] * d[:, 2]))
    with np.errstate(**_ERR):
        p = cp / st
    return np.where(st > 0, p, F(0)).astype(F)


def lambert_sample(kind, alb, fr, q2, q1):
    """BSDF::sample of RTG_MAT_DIFFUSE (0) / RTG_MAT_LAMBERT (1): cosineSampleHemisphere(q1, q2), q2 the
    first draw. Returns (wi world as a list of three arrays, reflectedColour (n, 3), pdf (n,))."""
    wl = R.cosine_sample_hemisphere(q1, q2)
    pdf = R.div_pi_d(wl[2])
    if kind == 0:
        pdf = np.where(wl[2] >= 0, pdf, F(0)).astype(F)
    return R.to_world(fr, wl), R.div_pi_f(np.asarray(alb, F)), pdf


def nee_weight(pmf, l_pdf, l2, cos_l, is_env, p_b):
    """w_l = mis_w(p_l, p_b): p_l = convertPDFAreaToSolidAngle(pmf l_pdf, l2, cos_l) for an area light,
    pmf l_pdf for the environment."""
    pp = (np.asarray(pmf, F) * np.asarray(l_pdf, F)).astype(F)
    p_l = np.where(is_env, pp, pdf_area_to_solid(pp, l2, cos_l)).astype(F)
    return mis_w(p_l, p_b), p_l


def weight_grid():
    """The densities the weight is probed on: 0, the smallest and the largest denormal, FLT_MIN, a spread of
    ordinary values, FLT_MAX and infinity, as all ordered pairs (p, q)."""
    v = np.array([0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 1e-30, 1e-20, 1e-10, 1e-3, 0.07957747, 0.25, 0.5, 1.0,
                  1.5, 3.0, 7.0, 1e3, 1e10, 1e19, 1e20, 1e30, 3.40282347e+38, np.inf], F)
    p, q = np.meshgrid(v, v, indexing="ij")
    return p.reshape(-1).copy(), q.reshape(-1).copy()
