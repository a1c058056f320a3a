"""TEST INFRASTRUCTURE ONLY — numpy restatement of the light selection of include/rtg.h
(rtg_set_light_sampling, RTG_LIGHTS_POWER): the weights, the pmf, the alias table, the pick and
Triangle::sample, operation by operation in the order the header states. The cell weights, the PCG
stream, Colour::Lum and alias_mass are tests/env_sampling_ref.py's, unchanged; vose() is the loop of its
build_alias on probabilities that are already scaled.
"""
import math

import numpy as np

from env_sampling_ref import (PI, PathStream, alias_mass, bilinear, build_alias, cell_weights, env_eval,  # noqa: F401
                              lum32, sample as env_sample, uniform_sample)

F = np.float32
U32 = np.uint32
U64 = np.uint64


# ------------------------------------------------------------------ weights, pmf, table
def env_weight(env_texels, root_box):
    """w_env = (2.0 * pi * pi) * R * R * (S / N): S the cell weights added in index order, R half the
    diagonal of the root box (six float32 values widened to binary64). None when R is 0 or not finite."""
    cw = cell_weights(env_texels).reshape(-1)
    S = float(np.cumsum(cw)[-1])
    b = [float(F(v)) for v in np.asarray(root_box).reshape(-1)[:6]]
    dx, dy, dz = b[3] - b[0], b[4] - b[1], b[5] - b[2]
    R = 0.5 * math.sqrt((dx * dx + dy * dy) + dz * dz)
    if not (R > 0.0) or not math.isfinite(R):
        return None
    return (2.0 * PI * PI) * R * R * (S / float(len(cw)))


def light_weights(records, env_texels=None, root_box=None):
    """(n,) float64 from the (n, 20) float32 device records: (double)Lum(em) * (double)area for an area
    light (a negative or non-finite Lum counting as 0), env_weight for the environment light. None when
    the environment light's R is 0 or not finite."""
    rec = np.asarray(records, F).reshape(-1, 20)
    kind = rec[:, 7].copy().view(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        l = lum32(rec[:, 16:19])
        l = np.where((l > 0) & np.isfinite(l), l, F(0)).astype(F)
    w = l.astype(np.float64) * rec[:, 3].astype(np.float64)
    for i in np.flatnonzero(kind == 1):
        we = env_weight(env_texels, root_box)
        if we is None:
            return None
        w[i] = we
    return w


def light_pmf(weights, lam):
    """pmf_i = ((1 - lam) * w_i) / sum + lam / n in binary64, the sum in index order. None when the sum
    is 0 or not finite."""
    w = np.asarray(weights, np.float64).reshape(-1)
    n = len(w)
    total = float(np.cumsum(w)[-1])
    if not (total > 0.0) or not math.isfinite(total):
        return None
    lam = float(lam)
    return np.array([((1.0 - lam) * float(x)) / total + lam / float(n) for x in w], np.float64)


def vose(p, positive):
    """Vose's algorithm in binary64 on scaled probabilities p (p_k = probability_k * n), in the fixed
    order of env_sampling_ref.build_alias (its loop, which scales by the weights' sum first and so cannot
    be handed p_k = pmf_k * n itself; tests/test_light_sampling.py checks the two against each other).
    positive[k]: entry k has a positive probability. Returns (prob float64, alias uint32)."""
    p = [float(x) for x in p]
    n = len(p)
    prob = [1.0] * n
    alias = list(range(n))
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if not p[i] < 1.0]
    while small and large:
        s, l = small.pop(), large.pop()
        prob[s] = p[s]
        alias[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    for s in small:
        prob[s] = 1.0 if positive[s] else 0.0
    return np.array(prob, np.float64), np.array(alias, U32)


def build_table(weights, lam):
    """{"pmf", "prob" (float64), "alias" (uint32), "entries" (n, 4) uint32}: Vose on p_k = pmf_k * n;
    entries {(float)prob, alias, (float)pmf, (float)pmf[alias]}."""
    pmf = light_pmf(weights, lam)
    if pmf is None:
        return None
    n = len(pmf)
    prob, alias = vose([float(x) * float(n) for x in pmf], pmf > 0)
    al = {"prob": prob, "alias": alias}
    e = np.zeros((n, 4), U32)
    e[:, 0] = al["prob"].astype(F).view(U32)
    e[:, 1] = al["alias"]
    e[:, 2] = pmf.astype(F).view(U32)
    e[:, 3] = pmf.astype(F)[al["alias"]].view(U32)
    return {"pmf": pmf, "prob": al["prob"], "alias": al["alias"], "entries": e}


def pick(entries, r0, d1):
    """light_pick restated: (li (n,) int64, pmf (n,) float32)."""
    e = np.asarray(entries, U32).reshape(-1, 4)
    r0 = np.ascontiguousarray(r0, U32).reshape(-1)
    d1 = np.ascontiguousarray(d1, F).reshape(-1)
    n = len(e)
    k = ((r0.astype(U64) * U64(n)) >> U64(32)).astype(np.int64)
    t = e[k]
    keep = d1 < t[:, 0].copy().view(F)
    li = np.where(keep, k, t[:, 1].astype(np.int64))
    pmf = np.where(keep, t[:, 2], t[:, 3]).astype(U32).view(F)
    return li, pmf


# ------------------------------------------------------------------ the sample on an area light
def dot3(a, b):
    return ((a[:, 0] * b[:, 0]) + (a[:, 1] * b[:, 1])) + (a[:, 2] * b[:, 2])


def normalize3(a):
    l = F(1) / np.sqrt(dot3(a, a))
    return a * l[:, None]


def triangle_sample(rec, r1, r2):
    """Triangle::sample on the records rec (n, 20) with draws r1, r2: the point (n, 3) float32,
    (v0 * alpha + v1 * beta) + v2 * gamma with alpha = 1 - sqrt(r1), beta = r2 * sqrt(r1),
    gamma = 1 - (alpha + beta)."""
    rec = np.asarray(rec, F).reshape(-1, 20)
    r1, r2 = np.asarray(r1, F), np.asarray(r2, F)
    la = F(1) - np.sqrt(r1)
    lb = r2 * np.sqrt(r1)
    lg = F(1) - (la + lb)
    return (rec[:, 0:3] * la[:, None] + rec[:, 4:7] * lb[:, None]) + rec[:, 8:11] * lg[:, None]


def area_geometry(rec, p2, x, sn):
    """(g, wi): g = (max(wi . sn, 0) * max(-(wi . gn), 0)) / |p2 - x|^2 of computeDirect."""
    wi = p2 - x
    l2 = dot3(wi, wi)
    wi = normalize3(wi)
    a = dot3(wi, sn)
    b = -dot3(wi, np.asarray(rec, F).reshape(-1, 20)[:, 12:15])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (np.where(a > 0, a, F(0)).astype(F) * np.where(b > 0, b, F(0)).astype(F)) / l2
    return g.astype(F), wi


def shadow_ray(x, p2, eps=F(1e-4)):
    """Scene::visible(x, p2) as the kernel writes its ray: (n, 8) = origin, maxT, direction, 0."""
    sd = p2 - x
    l2 = dot3(sd, sd)
    maxt = np.sqrt(l2) - (F(2.0) * eps)
    sd = sd * (F(1) / np.sqrt(l2))[:, None]
    q = np.zeros((len(x), 8), F)
    q[:, 0:3], q[:, 3], q[:, 4:7] = x + sd * eps, maxt, sd
    return q
