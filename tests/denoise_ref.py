"""TEST INFRASTRUCTURE ONLY — numpy float32 restatement of the denoiser's filter (include/rtg.h,
rtg_denoise*; DESIGN.md "Denoiser"): the edge-avoiding a-trous wavelet filter guided by albedo and
normals. The same operations in the same order as rtg_denoise.hip, vectorised over pixels with the
tap loop sequential (dy outer, dx inner), so the device result is compared bit for bit.
"""
import numpy as np

F = np.float32
TAPS = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))


def _sqdist(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _stop(w, a, b, inv):
    t = F(1.0) - _sqdist(a, b) * inv
    t = np.where(t > 0, t, F(0.0))
    return w * (t * t)


def background(normal):
    n = np.asarray(normal, F)
    return ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) == 0


def denoise_ref(colour, albedo, normal, iterations=5, normal_squarings=5, sigma_colour=1.0, sigma_albedo=0.1):
    """colour, albedo, normal: (H, W, 3) float32. Returns the filtered (H, W, 3) float32 image."""
    C = np.array(colour, F)
    A = np.ascontiguousarray(albedo, F)
    N = np.ascontiguousarray(normal, F)
    assert C.ndim == 3 and C.shape[2] == 3 and A.shape == C.shape and N.shape == C.shape
    assert 1 <= iterations <= 8 and 0 <= normal_squarings <= 8
    H, W = C.shape[:2]
    z = background(N)
    sigma_colour, sigma_albedo = F(sigma_colour), F(sigma_albedo)
    col_on, alb_on = bool(sigma_colour > 0), bool(sigma_albedo > 0)
    ia = F(1.0) / (sigma_albedo * sigma_albedo) if alb_on else F(0.0)
    for i in range(iterations):
        s = 1 << i
        sc = F(np.ldexp(sigma_colour, -i))
        ic = F(1.0) / (sc * sc) if col_on else F(0.0)
        sw = np.zeros((H, W), F)
        acc = np.zeros((H, W, 3), F)
        for dy in range(-2, 3):
            oy = dy * s
            y0, y1 = max(0, -oy), min(H, H - oy)
            if y0 >= y1:
                continue
            for dx in range(-2, 3):
                ox = dx * s
                x0, x1 = max(0, -ox), min(W, W - ox)
                if x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                w = np.full((y1 - y0, x1 - x0), TAPS[dy + 2] * TAPS[dx + 2], F)
                if col_on:
                    w = _stop(w, C[Q], C[P], ic)
                if alb_on:
                    w = _stop(w, A[Q], A[P], ia)
                nd = (N[P][..., 0] * N[Q][..., 0] + N[P][..., 1] * N[Q][..., 1]) + N[P][..., 2] * N[Q][..., 2]
                nd = np.where(nd > 0, nd, F(0.0))
                nd = np.where(nd < 1, nd, F(1.0))
                for _ in range(normal_squarings):
                    nd = nd * nd
                nd = np.where(z[P] & z[Q], F(1.0), nd)
                w = w * nd
                sw[P] = sw[P] + w
                acc[P] = acc[P] + w[..., None] * C[Q]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = acc / sw[..., None]
        C = np.where((sw > 0)[..., None], out, C).astype(F)
    return C
