"""The denoiser on the GPU (librtg.so, rtg_denoise.hip) against its numpy restatement
(tests/denoise_ref.py) and the C oracle's films, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from denoise_ref import denoise_ref
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import (NativeError, RayTracer, RayTracerGroup, denoise_images, loadScene, read_hdr,
                                    save_hdr)
from raytracingrenderer_amd import _native as N

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere((bits(got) != bits(want)).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ, first (%d, %d): %s vs %s" % (what, len(bad), y, x, got[y, x], want[y, x]))


def _nan_canon(a):
    return np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)


def synthetic(h, w):
    """Seeded random colour with a few 1e4 outliers, an albedo step, smooth random unit normals and
    a zero-normal block."""
    rng = np.random.default_rng(1000 * h + w)
    c = rng.random((h, w, 3), dtype=np.float32)
    for _ in range(max(1, h * w // 200)):
        c[rng.integers(h), rng.integers(w), rng.integers(3)] = np.float32(1e4)
    a = np.full((h, w, 3), 0.25, np.float32) + rng.random((h, w, 3), dtype=np.float32) * np.float32(0.02)
    a[:, w // 2:] += np.float32(0.5)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ph = rng.random(4).astype(np.float32) * np.float32(6.0)
    n = np.stack([np.sin(xx * np.float32(0.21) + ph[0]) + np.cos(yy * np.float32(0.13) + ph[1]),
                  np.sin(yy * np.float32(0.17) + ph[2]), np.float32(1.5) + np.cos(xx * np.float32(0.11) + ph[3])],
                 axis=-1).astype(np.float32)
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    n[h // 3: h // 3 + max(1, h // 4), w // 4: w // 4 + max(1, w // 3)] = 0.0
    return c, a, n


@pytest.mark.parametrize("sigma_colour", [0.0, 1.0])
@pytest.mark.parametrize("iterations", [1, 2, 5, 6, 7, 8])
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 65), (64, 64), (70, 100), (3, 260), (260, 3), (130, 270)])
def test_filter_equals_the_reference(shape, iterations, sigma_colour):
    """Every iteration count the API accepts (steps 1 ... 128) on shapes below, at and above a block
    (64 x 4 pixels). An axis of 257 or more has pixels with all five taps of step 64 in bounds (260 and
    270 here, as a single row, a single column and a 2-D image); at step 128 it puts the +-256 taps in
    bounds, which no smaller image does."""
    c, a, n = synthetic(*shape)
    got = denoise_images(c, a, n, iterations=iterations, sigma_colour=sigma_colour)
    assert_same_bits(got, denoise_ref(c, a, n, iterations, 5, sigma_colour, 0.1), "rtg_denoise_images")
    assert_same_bits(denoise_images(c, a, n, iterations=iterations, sigma_colour=sigma_colour), got, "second call")


def test_filter_parameters_reach_the_kernel():
    """normal_squarings and sigma_albedo other than the defaults, and both terms off."""
    c, a, n = synthetic(33, 65)
    for m, sa in [(0, 0.1), (8, 0.05), (2, 0.0)]:
        got = denoise_images(c, a, n, iterations=3, normal_squarings=m, sigma_colour=0.5, sigma_albedo=sa)
        assert_same_bits(got, denoise_ref(c, a, n, 3, m, 0.5, sa), "m=%d sigma_albedo=%g" % (m, sa))


def test_non_finite_pixels_spread_like_the_reference():
    """A NaN and a +inf colour pixel (33 x 65, 3 iterations, both sigma_colour settings): the stopping
    term gives such a tap the weight 0, and 0 * NaN / 0 * inf is NaN, so the pixel's whole footprint
    turns NaN, step by step. The device does exactly what the restatement does (any NaN equals any
    NaN); DESIGN.md 8a states this as the filter's definition."""
    c, a, n = synthetic(33, 65)
    c[7, 11, 1] = np.float32(np.nan)
    c[20, 50, :] = np.float32(np.inf)
    for sc in (0.0, 1.0):
        got = denoise_images(c, a, n, iterations=3, sigma_colour=sc)
        with np.errstate(invalid="ignore", over="ignore"):
            want = denoise_ref(c, a, n, 3, 5, sc, 0.1)
        assert np.isnan(want).any() and np.isfinite(want).any()
        assert_same_bits(_nan_canon(got), _nan_canon(want), "non-finite pixels, sigma_colour %g" % sc)


@pytest.fixture(scope="module", params=["cornell-box", "coffee-small"])
def scene_case(request):
    """The C oracle's films of one scene at 64x48: 4 and 5 spp (seed 1234), the albedo and normal
    guides at 1 sample; computed once and left unchanged."""
    s = loadScene(os.path.join(SCENES, request.param), width=64, height=48)
    o = Oracle(s, 4, "rtm")
    film4, _ = o.render(4, seed=1234, threads=8)
    film5, _ = o.render(5, seed=1234, threads=8)
    alb, _ = Oracle(s, 4, "rtm", integrator=2).render(1, seed=1234, threads=8)
    nrm, _ = Oracle(s, 4, "rtm", integrator=3).render(1, seed=1234, threads=8)
    for v in (film4, film5, alb, nrm):
        v.setflags(write=False)
    return {"name": request.param, "scene": s, "film4": film4, "film5": film5, "albedo": alb, "normal": nrm}


def test_handle_denoise_matches_oracle_and_leaves_the_film_alone(scene_case):
    k = scene_case
    rt = RayTracer(k["scene"], seed=1234)
    rt.render(4)
    mean4 = (k["film4"] / np.float32(4)).astype(np.float32)
    got = rt.denoise()
    alb, nrm = rt.guides()
    assert_same_bits(alb, k["albedo"], "albedo guide vs oracle integrator 2")
    assert_same_bits(nrm, k["normal"], "normal guide vs oracle integrator 3")
    assert_same_bits(got, denoise_ref(mean4, k["albedo"], k["normal"]), "denoise() vs denoise_ref(oracle)")
    assert rt.denoise_ms() > 0.0
    film, spp = rt.film()
    assert spp == 4 and rt.integrator == "path"
    assert_same_bits(film, k["film4"], "film after denoise()")
    rt.render(1)
    film, spp = rt.film()
    assert spp == 5
    assert_same_bits(film, k["film5"], "one more render() after denoise()")
    # denoising gains on the noisy film, measured against the handle's own 512-spp film
    conv = RayTracer(k["scene"], seed=1234)
    conv.render(512)
    f512, spp512 = conv.film()
    truth = f512 / np.float32(spp512)
    rt4 = RayTracer(k["scene"], seed=1234)
    rt4.load_film(k["film4"], 4)
    noisy = float(np.mean((mean4.astype(np.float64) - truth) ** 2))
    for sc in (0.0, 1.0, 4.0):
        den = rt4.denoise(sigma_colour=sc)
        mse = float(np.mean((den.astype(np.float64) - truth) ** 2))
        print("%s sigma_colour %g: MSE %.6g vs noisy %.6g (ratio %.3f)" % (k["name"], sc, mse, noisy, mse / noisy))
        assert mse < noisy, (k["name"], sc, mse, noisy)


def test_queued_frames_are_waited_for(scene_case):
    k = scene_case
    want = RayTracer(k["scene"], seed=1234)
    want.render(4)
    ref = want.denoise()
    rt = RayTracer(k["scene"], seed=1234)
    for _ in range(4):
        rt.render(1, sync=False)
    assert_same_bits(rt.denoise(), ref, "denoise() after four queued frames")
    assert rt.getSPP() == 4
    assert_same_bits(rt.film()[0], k["film4"], "film after the queued frames and denoise()")


def test_load_film_then_denoise_and_clear_raises(scene_case):
    k = scene_case
    rt = RayTracer(k["scene"], seed=1234)
    with pytest.raises(NativeError):
        rt.denoise()  # nothing rendered yet: spp == 0
    rt.load_film(k["film5"], 5)
    mean5 = (k["film5"] / np.float32(5)).astype(np.float32)
    assert_same_bits(rt.denoise(iterations=3), denoise_ref(mean5, k["albedo"], k["normal"], 3), "after load_film")
    rt.clear()
    with pytest.raises(NativeError):
        rt.denoise()
    rt.render(4)
    assert_same_bits(rt.film()[0], k["film4"], "render after a refused denoise()")


def test_result_stays_on_the_device():
    """rtg_denoise_copy_device hands the last result to device memory (a hipMalloc'ed buffer of the
    HIP runtime librtg.so is linked against)."""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")  # librtg.so's rpath
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=65, height=33)
    rt = RayTracer(s, seed=9)
    got = np.zeros((33, 65, 3), np.float32)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(got.nbytes)) == 0
    try:
        with pytest.raises(NativeError):
            rt.copy_denoised_to(d.value)  # no result yet
        rt.render(2)
        want = rt.denoise(iterations=4)
        rt.copy_denoised_to(d.value)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d, C.c_size_t(got.nbytes), 2) == 0  # device to host
    finally:
        hip.hipFree(d)
    assert_same_bits(got, want, "rtg_denoise_copy_device")


def test_group_denoise_equals_one_handle():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=100, height=70)
    rt = RayTracer(s, seed=5)
    rt.render(3)
    want = rt.denoise()
    film = rt.film()[0]
    g = RayTracerGroup(s, devices=(0, 0), seed=5)
    g.render(3)
    assert_same_bits(g.denoise(), want, "group denoise vs one handle")
    gf, spp = g.film()
    assert spp == 3
    assert_same_bits(gf, film, "group film after denoise()")
    assert_same_bits(g.denoise(iterations=2, sigma_colour=0.0), rt.denoise(iterations=2, sigma_colour=0.0), "second call")


def test_cli_denoise_writes_the_library_result(tmp_path):
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = os.path.join(SCENES, "cornell-box")
    base = [cli, "-scene", scene, "-SPP", "3", "-width", "64", "-height", "48", "-timeLimit", "0", "-outputFilename",
            "out.hdr"]
    for d, extra in (("plain", []), ("den", ["-denoise", "1"]), ("opt", ["-denoise", "1", "-denoiseIterations", "3",
                                                                       "-denoiseSigmaColour", "0.5",
                                                                       "-denoiseSigmaAlbedo", "0.2"])):
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    for f in ("out.hdr", "result_3.hdr"):
        assert (tmp_path / "den" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    assert sorted(os.listdir(tmp_path / "plain")) == ["out.hdr", "result_3.hdr"]
    assert sorted(os.listdir(tmp_path / "den")) == ["out.hdr", "out_denoised.hdr", "result_3.hdr"]
    rt = RayTracer(loadScene(scene, width=64, height=48), seed=1234)
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.denoise(), 1)
    assert (tmp_path / "den" / "out_denoised.hdr").read_bytes() == (tmp_path / "lib.hdr").read_bytes()
    save_hdr(str(tmp_path / "lib_opt.hdr"), rt.denoise(iterations=3, sigma_colour=0.5, sigma_albedo=0.2), 1)
    assert (tmp_path / "opt" / "out_denoised.hdr").read_bytes() == (tmp_path / "lib_opt.hdr").read_bytes()
    assert read_hdr(str(tmp_path / "den" / "out_denoised.hdr")).shape == (48, 64, 3)
