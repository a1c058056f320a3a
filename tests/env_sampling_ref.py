"""TEST INFRASTRUCTURE ONLY — numpy restatement of the environment light sampling of include/rtg.h
(rtg_set_env_sampling, RTG_ENV_LUMINANCE): the cell weights, Vose's alias table, the sample itself and
the path's PCG32 draws, operation by operation in the order the header states (numpy's float32 +, -, *,
/ and sqrt are IEEE, one rounding each, as the kernel's without contraction). The transcendentals are
include/rtg_math.h's, through the oracle library built from it (or_math_eval). The row factor
sin(pi (cy + 0.5) / H) is math.sin, the C library's binary64 sin the host builder calls too.
"""
import ctypes as C
import math

import numpy as np

from oracle.pyoracle import lib

F = np.float32
U32 = np.uint32
U64 = np.uint64
PI = 3.14159265358979323846


# ------------------------------------------------------------------ transcendentals (include/rtg_math.h)
def _math(fn, x, nout):
    x = np.ascontiguousarray(x, F)
    out = np.zeros(nout, F)
    n = len(x) if fn != 4 else len(x) // 2
    lib("rtm").or_math_eval(fn, x.ctypes.data_as(C.POINTER(C.c_float)), n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def sincosf(t):
    o = _math(2, t, 2 * len(t))
    return o[0::2].copy(), o[1::2].copy()


def acosf(x):
    return _math(3, x, len(x))


def atan2f(y, x):
    yx = np.stack([np.asarray(y, F), np.asarray(x, F)], axis=1).reshape(-1)
    return _math(4, yx, len(y))


# ------------------------------------------------------------------ weights and table
def lum32(rgb):
    """Colour::Lum in float32: ((0.2126f r) + (0.7152f g)) + (0.0722f b)."""
    c = np.asarray(rgb, F)
    return ((F(0.2126) * c[..., 0]) + (F(0.7152) * c[..., 1])) + (F(0.0722) * c[..., 2])


def footprint_max(texels):
    """(H, W) float32: the maximum of Lum over the four texels Texture::sample blends in each cell
    (wrap-around in x and y), a negative or non-finite Lum counting as 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        l = lum32(texels)
        l = np.where((l > 0) & np.isfinite(l), l, F(0)).astype(F)
    lx = np.roll(l, -1, axis=1)
    return np.maximum(np.maximum(l, lx), np.maximum(np.roll(l, -1, axis=0), np.roll(lx, -1, axis=0)))


def cell_weights(texels):
    """(H, W) float64: w = (double)footprint_max * sin(pi (cy + 0.5) / H)."""
    m = footprint_max(texels).astype(np.float64)
    H = m.shape[0]
    rs = np.array([math.sin(PI * (cy + 0.5) / H) for cy in range(H)], np.float64)
    return m * rs[:, None]


def build_alias(weights):
    """Vose's algorithm in binary64 in the header's fixed order. Returns a dict: "sum", "prob" (n,)
    float64, "alias" (n,) uint32, "cellpdf" (n,) float32; None when the weights sum to 0."""
    w = np.asarray(weights, np.float64).reshape(-1)
    n = len(w)
    total = float(np.cumsum(w)[-1])  # added in index order
    if not (total > 0.0) or not math.isfinite(total):
        return None
    p = [(float(x) / total) * float(n) for x in w]
    cellpdf = np.array([pi / ((2.0 * PI) * PI) for pi in p], np.float64).astype(F)
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
        prob[s] = 1.0 if w[s] > 0.0 else 0.0
    return {"sum": total, "prob": np.array(prob, np.float64), "alias": np.array(alias, U32), "cellpdf": cellpdf}


def table_entries(al):
    """(n, 4) uint32: {(float)prob, alias, cellpdf of the cell, cellpdf of the alias} as the kernel loads them."""
    n = len(al["prob"])
    e = np.zeros((n, 4), U32)
    e[:, 0] = al["prob"].astype(F).view(U32)
    e[:, 1] = al["alias"]
    e[:, 2] = al["cellpdf"].view(U32)
    e[:, 3] = al["cellpdf"][al["alias"]].view(U32)
    return e


def alias_mass(prob, alias):
    """(n,) float64: the probability with which the table returns each cell,
    prob_i / n + sum over {j: alias_j = i} of (1 - prob_j) / n."""
    prob = np.asarray(prob, np.float64).reshape(-1)
    n = len(prob)
    mass = prob / n
    np.add.at(mass, np.asarray(alias).reshape(-1).astype(np.int64), (1.0 - prob) / n)
    return mass


# ------------------------------------------------------------------ the sample
def sample(entries, W, H, r0, d):
    """env_sample_luminance restated. entries (W*H, 4) uint32; r0 (n,) uint32; d (n, 3) float32.
    Returns (wi (n, 3) float32, pdf (n,) float32 with 0 where rejected, cell (n,) the cell drawn)."""
    e = np.asarray(entries, U32).reshape(-1, 4)
    r0 = np.ascontiguousarray(r0, U32).reshape(-1)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    N = W * H
    k = ((r0.astype(U64) * U64(N)) >> U64(32)).astype(np.int64)
    t = e[k]
    keep = d[:, 0] < t[:, 0].copy().view(F)
    c = np.where(keep, k, t[:, 1].astype(np.int64))
    cp = np.where(keep, t[:, 2], t[:, 3]).astype(U32).view(F)
    cx, cy = c % W, c // W
    u = (cx.astype(F) + d[:, 1]) / F(W)
    v = (cy.astype(F) + d[:, 2]) / F(H)
    theta = F(3.14159265) * v
    phi = F(6.2831855) * u
    st, ct = sincosf(theta)
    sp, cph = sincosf(phi)
    wi = np.stack([st * cph, ct, st * sp], axis=1).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = (cp / st).astype(F)
    ok = (st > 0) & (pdf > 0)
    return wi, np.where(ok, pdf, F(0)).astype(F), c


def uniform_sample(q1, q2):
    """EnvironmentMap::sample as the kernels restate it: uniformSampleSphere(q1, q2) and its pdf
    (rtg_dev.h uniform_sample_sphere; q2 is the path's first draw, q1 its second)."""
    q1, q2 = np.asarray(q1, F), np.asarray(q2, F)
    theta = acosf(F(1) - F(2) * q1)
    phi = ((2.0 * PI) * q2.astype(np.float64)).astype(F)
    st, ct = sincosf(theta)
    sp, cp = sincosf(phi)
    wi = np.stack([cp * st, sp * st, ct], axis=1).astype(F)
    return wi, F(1.0 / (4.0 * PI))


def env_uv(wi):
    """EnvironmentMap::evaluate's texture coordinates of direction(s) wi (Lights.h:150-157)."""
    wi = np.asarray(wi, F).reshape(-1, 3)
    u = atan2f(wi[:, 2], wi[:, 0])
    u = np.where(u < 0, (u.astype(np.float64) + 2.0 * PI).astype(F), u).astype(F)
    u = (u.astype(np.float64) * (1.0 / (2.0 * PI))).astype(F)
    v = (acosf(wi[:, 1]).astype(np.float64) * (1.0 / PI)).astype(F)
    return u, v


def bilinear(texels, tu, tv):
    """Texture::sample (Imaging.h:72-94) in float32, as rtg_dev.h's bilinear()."""
    t = np.asarray(texels, F)
    h, w = t.shape[:2]
    u = np.maximum(F(0), np.abs(np.asarray(tu, F))) * F(w)
    v = np.maximum(F(0), np.abs(np.asarray(tv, F))) * F(h)
    x, y = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - x.astype(F), v - y.astype(F)
    w0, w1 = (F(1) - fu) * (F(1) - fv), fu * (F(1) - fv)
    w2, w3 = (F(1) - fu) * fv, fu * fv
    x, y = x % w, y % h
    x1, y1 = (x + 1) % w, (y + 1) % h
    s0, s1, s2, s3 = t[y, x], t[y, x1], t[y1, x], t[y1, x1]
    return ((s0 * w0[:, None] + s1 * w1[:, None]) + s2 * w2[:, None]) + s3 * w3[:, None]


def env_eval(texels, wi):
    u, v = env_uv(wi)
    return bilinear(texels, u, v)


# ------------------------------------------------------------------ the path's PCG32 stream
class PathStream:
    """The PCG32 stream of paths (pixel, sample) under `seed`, as k_shade seeds and steps it: raw()
    is a pcg_step's 32-bit output, next() the float draw (output >> 8) * 2^-24."""

    def __init__(self, pixels, samples, seed):
        px = np.ascontiguousarray(pixels, U32).reshape(-1).astype(U64)
        sm = np.ascontiguousarray(samples, U32).reshape(-1).astype(U64)
        self.inc = (((px << U64(16)) | sm) << U64(1)) | U64(1)
        self.s = np.zeros(len(px), U64)
        self.raw()
        with np.errstate(over="ignore"):
            self.s = self.s + U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.raw()

    def raw(self):
        old = self.s
        with np.errstate(over="ignore"):
            self.s = old * U64(6364136223846793005) + self.inc
            xs = (((old >> U64(18)) ^ old) >> U64(27)).astype(U32)
            rot = (old >> U64(59)).astype(U32)
            return (xs >> rot) | (xs << ((np.zeros_like(rot) - rot) & U32(31)))

    def next(self):
        return (self.raw() >> U32(8)).astype(F) * F(1.0 / 16777216.0)
