"""The denoiser without a GPU: exact properties of the numpy restatement (tests/denoise_ref.py, what
the device result is pinned against), the new C-ABI symbols and their bindings, and every argument
check of include/rtg.h's rtg_denoise_* (made before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest

from denoise_ref import denoise_ref
from raytracingrenderer_amd import _native as N

NEW = ["rtg_denoise_defaults", "rtg_denoise_images", "rtg_denoise", "rtg_denoise_guides", "rtg_denoise_copy_device",
       "rtg_denoise_ms", "rtg_group_denoise"]


def unit_normals(rng, h, w):
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    return (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)


def test_albedo_step_filters_as_two_independent_images():
    """Albedos further apart than sigma_albedo give the stopping term max(0, 1 - d^2/s^2) = 0 exactly:
    no tap crosses the step, and a zero weight adds +0 to the sums, so each side is bit-equal to the
    side filtered alone (where those taps fall outside the image and are skipped)."""
    rng = np.random.default_rng(1)
    h, w, k = 13, 22, 9
    c = rng.random((h, w, 3), dtype=np.float32)
    n = np.tile(np.array([0, 0, 1], np.float32), (h, w, 1))
    a = np.full((h, w, 3), 0.2, np.float32)
    a[:, k:] = 0.8  # |dA|^2 = 3 * 0.36 > 0.1^2
    for sc in (0.0, 1.0):
        full = denoise_ref(c, a, n, 5, 5, sc, 0.1)
        assert np.array_equal(full[:, :k], denoise_ref(c[:, :k], a[:, :k], n[:, :k], 5, 5, sc, 0.1))
        assert np.array_equal(full[:, k:], denoise_ref(c[:, k:], a[:, k:], n[:, k:], 5, 5, sc, 0.1))
        assert not np.array_equal(full, c)


def test_zero_normal_region_filters_as_an_independent_image():
    """Background pixels (zero normal) weigh each other by 1 and surface pixels by N.N = 0: the two
    regions never mix, with the albedo term off."""
    rng = np.random.default_rng(2)
    h, w, k = 12, 17, 5
    c = rng.random((h, w, 3), dtype=np.float32)
    a = rng.random((h, w, 3), dtype=np.float32)
    n = unit_normals(rng, h, w)
    n[k:] = 0.0
    full = denoise_ref(c, a, n, 4, 2, 0.0, 0.0)
    assert np.array_equal(full[:k], denoise_ref(c[:k], a[:k], n[:k], 4, 2, 0.0, 0.0))
    assert np.array_equal(full[k:], denoise_ref(c[k:], a[k:], n[k:], 4, 2, 0.0, 0.0))
    # the background block is a plain a-trous blur: it changed
    assert not np.array_equal(full[k:], c[k:])


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (3, 70)])
def test_small_shapes_stay_finite_and_in_range(shape):
    """K = 6: the step (32) exceeds every side but one. Every output is sum(w c) / sum(w) with
    w >= 0, a weighted mean of inputs: inside the input range up to the rounding of at most 25
    products, 24 adds and a division per iteration, (50 * 2^-24) relative per iteration."""
    rng = np.random.default_rng(3)
    h, w = shape
    c = (rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    a = rng.random((h, w, 3), dtype=np.float32)
    n = unit_normals(rng, h, w)
    for sc in (0.0, 1.0):
        out = denoise_ref(c, a, n, 6, 5, sc, 0.1)
        assert out.shape == c.shape and out.dtype == np.float32 and np.isfinite(out).all()
        slack = 6 * 50 * 2.0 ** -24
        assert out.min() >= c.min() * (1 - slack) and out.max() <= c.max() * (1 + slack)
    if shape == (1, 1):
        assert np.array_equal(out, c)


def _lib():
    from raytracingrenderer_amd import build
    if not os.path.exists(build.HIPCC) and not os.path.exists(os.path.join(N.LIB_DIR, "librtg.so")):
        pytest.skip("hipcc not available")
    return N.rtg()


def test_new_symbols_are_exported_and_bound():
    lib = _lib()
    so = C.CDLL(os.path.join(N.LIB_DIR, "librtg.so"))
    bound = {e[0] for e in N.RTG_EXPORTS}
    for name in NEW:
        assert hasattr(so, name), name
        assert name in bound, name
    p = N.rtg_denoise_params()
    assert lib.rtg_denoise_defaults(C.byref(p)) == 0
    assert (p.iterations, p.normal_squarings, p.sigma_colour, p.sigma_albedo) == (5, 5, 1.0, np.float32(0.1))
    from raytracingrenderer_amd import RayTracer, RayTracerGroup, denoise_images  # noqa: F401
    assert all(hasattr(RayTracer, m) for m in ("denoise", "guides", "denoise_ms")) and hasattr(RayTracerGroup, "denoise")


def test_argument_errors_need_no_gpu():
    """Every RTG_ERR_ARG case is decided before any device call (device -1 is never reached)."""
    lib = _lib()
    img = np.zeros((4, 5, 3), np.float32)
    ip = N.ptr(img, C.c_float)

    def call(w=5, h=4, c=ip, a=ip, n=ip, o=ip, params=(5, 5, 1.0, 0.1), null_params=False):
        p = N.rtg_denoise_params(*params)
        rc = lib.rtg_denoise_images(-1, w, h, c, a, n, None if null_params else C.byref(p), o)
        return rc, lib.rtg_last_error().decode()

    bad = [dict(null_params=True), dict(c=None), dict(a=None), dict(n=None), dict(o=None), dict(w=0), dict(h=0),
           dict(params=(0, 5, 1.0, 0.1)), dict(params=(9, 5, 1.0, 0.1)), dict(params=(5, 9, 1.0, 0.1)),
           dict(params=(5, 5, 1e-7, 0.1)), dict(params=(5, 5, 1.0, 1e-7)), dict(params=(5, 5, float("nan"), 0.1)),
           dict(params=(5, 5, float("inf"), 0.1)), dict(params=(5, 5, 1.0, float("nan"))),
           dict(params=(5, 5, 1.0, float("inf")))]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("rtg_denoise_images: "), (kw, rc, msg)
    # valid parameters (sigmas <= 0 switch a term off) pass the checks and reach the device call
    for params in [(1, 0, 0.0, 0.0), (8, 8, -1.0, float("-inf")), (5, 5, 1e-6, 1e-6)]:
        rc, msg = call(params=params)
        assert rc not in (0, -1), (params, rc, msg)
    p = N.rtg_denoise_params(5, 5, 1.0, 0.1)
    assert lib.rtg_denoise(None, C.byref(p), None) == -1
    assert lib.rtg_group_denoise(None, C.byref(p), None) == -1
    assert lib.rtg_denoise_guides(None, None, None) == -1
    assert lib.rtg_denoise_copy_device(None, None) == -1
    assert lib.rtg_denoise_ms(None) == 0.0
