"""TEST INFRASTRUCTURE ONLY — numpy float32 restatement of the camera sampling of include/rtg.h
(rtg_set_camera_sampling): the camera's own PCG32 stream, the pixel-filter offsets,
Camera::generateRay and the thin lens, operation by operation in the order the header states (numpy's
float32 +, -, *, / and sqrt are IEEE, one rounding each, as the kernel's without contraction). The lens
angle's sincosf is include/rtg_math.h's, through the oracle library built from it (or_math_eval).
"""
import ctypes as C

import numpy as np

from oracle.pyoracle import lib

F = np.float32
U64 = np.uint64
CAMERA_STREAM = 0x9E3779B97F4A7C15
FILTER_NONE, FILTER_BOX, FILTER_TENT = 0, 1, 2
FILTERS = {"none": FILTER_NONE, "box": FILTER_BOX, "tent": FILTER_TENT}


def _pcg_step(s, inc):
    old = s
    with np.errstate(over="ignore"):
        s = old * U64(6364136223846793005) + inc
        xs = (((old >> U64(18)) ^ old) >> U64(27)).astype(np.uint32)
        rot = (old >> U64(59)).astype(np.uint32)
        out = (xs >> rot) | (xs << ((np.zeros_like(rot) - rot) & np.uint32(31)))
    return s, out


def camera_draws(pixels, samples, seed):
    """(n, 4) float32: u0 (film x), u1 (film y), u2, u3 (lens) of each (pixel, sample) under `seed`."""
    px = np.ascontiguousarray(pixels, np.uint32).reshape(-1).astype(U64)
    sm = np.ascontiguousarray(samples, np.uint32).reshape(-1).astype(U64)
    inc = (((px << U64(16)) | sm) << U64(1)) | U64(1)  # pcg_inc
    s = np.zeros(len(px), U64)  # pcg_seed
    s, _ = _pcg_step(s, inc)
    with np.errstate(over="ignore"):
        s = s + U64((int(seed) ^ CAMERA_STREAM) & 0xFFFFFFFFFFFFFFFF)
    s, _ = _pcg_step(s, inc)
    u = np.zeros((len(px), 4), F)
    for k in range(4):  # pcg_next
        s, r = _pcg_step(s, inc)
        u[:, k] = (r >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
    return u


def filter_offset(filt, r, u):
    """The film offset of draw(s) u (float32 array) for filter `filt` (FILTER_*) of radius r."""
    u = np.asarray(u, F)
    r = F(r)
    if filt == FILTER_BOX:
        return (u * F(2) - F(1)) * r
    if filt == FILTER_TENT:
        lo = np.sqrt(F(2) * u) - F(1)
        hi = F(1) - np.sqrt(F(2) - F(2) * u)
        return np.where(u < F(0.5), lo, hi).astype(F) * r
    return np.zeros_like(u)


def _dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def _normalize(v):
    l = F(1) / np.sqrt(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]))
    return [v[0] * l, v[1] * l, v[2] * l]


def generate_ray(cam, px, py):
    """Camera::generateRay (Scene.h:43-54) at film positions (px, py), float32 arrays: the normalised
    direction as three arrays. cam: Scene.camera."""
    m = np.asarray(cam["inv_proj"], F).reshape(16)
    c = np.asarray(cam["camera"], F).reshape(16)
    xp = px / F(cam["width"])
    yp = F(1) - (py / F(cam["height"]))
    xp = (xp * F(2)) - F(1)
    yp = (yp * F(2)) - F(1)
    d = [((xp * m[4 * k] + yp * m[4 * k + 1]) + F(1) * m[4 * k + 2]) + m[4 * k + 3] for k in range(3)]
    d = [(d[0] * c[4 * k] + d[1] * c[4 * k + 1]) + d[2] * c[4 * k + 2] for k in range(3)]
    return _normalize(d)


def sincosf(theta):
    """include/rtg_math.h's sincosf on a float32 array: (sin, cos)."""
    t = np.ascontiguousarray(theta, F)
    out = np.zeros(2 * len(t), F)
    lib("rtm").or_math_eval(2, t.ctypes.data_as(C.POINTER(C.c_float)), len(t), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out[0::2].copy(), out[1::2].copy()


def lens_points(lens_radius, u2, u3):
    """(lx, ly): the point on the lens, in units of camera.m's first two columns."""
    rr = F(lens_radius) * np.sqrt(np.asarray(u2, F))
    s, c = sincosf(F(6.2831855) * np.asarray(u3, F))
    return rr * c, rr * s


def camera_samples_ref(cam, pixels, samples, seed, filt=FILTER_NONE, filter_radius=0.5, lens_radius=0.0,
                       focal_distance=1.0):
    """rtg_probe_camera_samples restated: (rays (n, 8) = o.xyz, 0, d.xyz, 0; film_xy (n, 2))."""
    pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
    n = len(pixels)
    W = np.uint32(int(F(cam["width"])))
    u = camera_draws(pixels, samples, seed)
    px = ((pixels % W).astype(F) + F(0.5)) + filter_offset(filt, filter_radius, u[:, 0])
    py = ((pixels // W).astype(F) + F(0.5)) + filter_offset(filt, filter_radius, u[:, 1])
    d = generate_ray(cam, px, py)
    o = [np.full(n, F(v), F) for v in np.asarray(cam["origin"], F)]
    if F(lens_radius) > 0:
        c = np.asarray(cam["camera"], F).reshape(16)
        xc, yc, zc = [c[0], c[4], c[8]], [c[1], c[5], c[9]], [c[2], c[6], c[10]]
        ft = F(focal_distance) / np.abs(_dot(d, zc))
        P = [o[k] + d[k] * ft for k in range(3)]
        lx, ly = lens_points(lens_radius, u[:, 2], u[:, 3])
        o = [(o[k] + xc[k] * lx) + yc[k] * ly for k in range(3)]
        d = _normalize([P[k] - o[k] for k in range(3)])
    rays = np.zeros((n, 8), F)
    for k in range(3):
        rays[:, k] = o[k]
        rays[:, 4 + k] = d[k]
    return rays, np.stack([px, py], axis=1).astype(F)
