"""Camera sampling on the GPU (rtg_set_camera_sampling: pixel-filter jitter and a thin lens): the
generate kernel's function against its numpy restatement (tests/camera_ref.py) bit for bit, and the
per-sample bounce-0 pipeline against the C oracle, against exact integer films, and against itself
under every way of cutting a render into chunks, calls, tiles, queued frames and ranks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref as cr
from camera_scenes import emission_of, emitter_layout, write_emitter_scene
from conftest import SCENES
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, save_hdr
from raytracingrenderer_amd import _native as N
from shade_scenes import table_limits

pytestmark = pytest.mark.gpu

LENS = dict(lens_radius=0.05, focal_distance=5.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def film_of(scene, n, setting=None, seed=1234, **kw):
    rt = RayTracer(scene, seed=seed, **kw)
    if setting is not None:
        rt.set_camera_sampling(**setting)
    rt.render(n)
    return rt.film()[0], rt.stats()


# ---------------------------------------------------------------- 3. probe = restatement
@pytest.mark.parametrize("name,w,h", [("cornell-box", 70, 50), ("coffee-small", 64, 48)])
def test_probe_equals_the_restatement(name, w, h):
    s = loadScene(os.path.join(SCENES, name), width=w, height=h)
    rng = np.random.default_rng(3)
    corners = [0, w - 1, w * (h - 1), w * h - 1]
    pix = np.array(corners + list(rng.integers(0, w * h, 60)), np.uint32)
    pix, smp = np.repeat(pix, 3), np.tile(np.array([0, 1, 65535], np.uint32), len(pix))
    rt = RayTracer(s, seed=1234)
    centre = Oracle(s, 4, "rtm").camera_rays(pix)
    seen = set()
    for fname, r in (("none", None), ("box", None), ("box", 4.0), ("tent", None), ("tent", 1.5)):
        for lens in ({}, dict(lens_radius=0.07, focal_distance=4.5)):
            rt.set_camera_sampling(fname, r, **lens)
            cs = rt.camera_sampling()
            assert cs["filter"] == fname and cs["lens_radius"] == np.float32(lens.get("lens_radius", 0.0))
            for seed in (1234, 0xFEDCBA9876543210):
                rays, xy = rt.camera_samples(pix, smp, seed=seed)
                want, wxy = cr.camera_samples_ref(s.camera, pix, smp, seed, cr.FILTERS[fname], cs["filter_radius"],
                                                  cs["lens_radius"], cs["focal_distance"])
                what = "%s %s r=%g lens=%s seed=%x" % (name, fname, cs["filter_radius"], bool(lens), seed)
                assert_same_bits(xy, wxy, what + ": film position")
                assert_same_bits(rays, want, what + ": rays")
                seen.add(bits(rays).tobytes())
                if fname == "none" and not lens:
                    assert_same_bits(rays[:, 0:3], centre[:, 0:3], what + ": origin vs oracle")
                    assert_same_bits(rays[:, 4:7], centre[:, 3:6], what + ": direction vs oracle")
    # every setting and seed gives other rays (5 filters x 2 lenses x 2 seeds), but NONE / pinhole ignores the seed
    assert len(seen) == 5 * 2 * 2 - 1


# ---------------------------------------------------------------- 4. the per-sample pipeline against the oracle
@pytest.mark.parametrize("name,w,h,depth,ns", [("cornell-mat", 40, 30, 8, 5), ("cornell-box", 70, 50, 4, 3)])
def test_zero_radius_box_is_the_oracle_film_over_the_new_path(name, w, h, depth, ns):
    """BOX with r = 0 sends every sample through the pixel centre, over k_generate_sampled and the
    segmented bounce 0: the path-traced film is the default mode's and the C oracle's, bit for bit."""
    s = loadScene(os.path.join(SCENES, name), width=w, height=h)
    want, _ = Oracle(s, depth, "rtm").render(ns, seed=1234, threads=8)
    f_none, st_none = film_of(s, ns, None, max_depth=depth)
    f_box, st_box = film_of(s, ns, dict(filter="box", filter_radius=0.0), max_depth=depth)
    assert_same_bits(f_none, want, "default mode vs oracle")
    assert_same_bits(f_box, want, "box r = 0 vs oracle")
    assert st_box["paths"] == st_none["paths"] == w * h * ns
    assert st_box["traced_camera_rays"] == st_box["paths"]
    assert st_none["traced_camera_rays"] == w * h  # one chunk: a camera ray per pixel
    assert st_box["extension_rays"] == st_none["extension_rays"] >= w * h * ns
    assert st_box["shadow_rays"] == st_none["shadow_rays"] > 0


# ---------------------------------------------------------------- 5. jittered bounce 0 end to end, exact
@pytest.fixture(scope="module")
def emitter_scenes(tmp_path_factory):
    out = {}
    lm, ll = table_limits()
    for layout, (w, h) in (("few", (64, 48)), ("many", (70, 50))):
        s = loadScene(write_emitter_scene(tmp_path_factory.mktemp(layout), layout, w, h))
        n = len(emitter_layout(layout))
        assert len({emission_of(i) for i in range(n)}) == n
        em = np.array([list(m.emission) for m in s.materials], np.float32)
        assert (em == np.round(em)).all() and (em > 0).all()
        # "few" shades from k_shade's LDS tables, "many" from the global ones
        assert (len(s.materials) <= lm and len(s.lights) <= ll) == (layout == "few")
        out[(w, h)] = (s, em[s.material_index])
    return out


CASES5 = {"box": dict(filter="box", filter_radius=0.5), "tent": dict(filter="tent", filter_radius=1.5),
          "box+lens": dict(filter="box", filter_radius=0.5, lens_radius=0.08, focal_distance=5.8)}


@pytest.mark.parametrize("ns", [1, 3, 64])
@pytest.mark.parametrize("case", list(CASES5))
@pytest.mark.parametrize("size", [(64, 48), (70, 50)])
def test_emitter_film_is_the_sum_of_the_sampled_triangles(emitter_scenes, size, case, ns):
    """Every instance emits small integers and BSDF::emit returns them for any ray, so the ALBEDO
    film is exactly the sum over a pixel's samples of emission[triangle hit by the sample's camera
    ray] (a miss adds 0): integer-valued, hence independent of the order of the additions.
    Not vacuous: the film differs from the default mode's, and at least 5 % of the pixels have
    samples on two or more different triangles (a miss counting as one). One sample cannot land on
    two triangles, so for ns = 1 the 5 % are pixels whose sample lands elsewhere than the pixel
    centre's ray does. (CPU-side layout check, oracle trace_closest over the restated rays: "few"
    64x48 box 0.058 / 0.115 / 0.224 for ns = 1 / 3 / 64, every other case higher.)"""
    s, tri_em = emitter_scenes[size]
    w, h = size
    rt = RayTracer(s, seed=1234, integrator="albedo")
    rt.render(ns)
    plain = rt.film()[0]
    rt.clear()
    rt.set_camera_sampling(**CASES5[case])
    rt.render(ns)
    film = rt.film()[0]
    pix = np.repeat(np.arange(w * h, dtype=np.uint32), ns)
    smp = np.tile(np.arange(ns, dtype=np.uint32), w * h)
    rays, _ = rt.camera_samples(pix, smp)
    hits = rt.trace_closest(rays)
    orc = Oracle(s, 4, "rtm")
    assert_same_bits(hits, orc.trace_closest(rays), "trace_closest vs oracle")
    hit = hits[:, 0] < np.float32(3e38)
    tid = np.where(hit, hits[:, 1].view(np.int32), -1)
    contrib = np.where(hit[:, None], tri_em[np.maximum(tid, 0)], np.float32(0))
    want = contrib.reshape(h, w, ns, 3).sum(axis=2, dtype=np.float64).astype(np.float32)
    assert np.array_equal(film, want), "%d pixels differ" % int((film != want).any(axis=2).sum())
    assert not np.array_equal(film, plain)
    tid = tid.reshape(w * h, ns)
    if ns > 1:
        frac = np.mean((tid != tid[:, :1]).any(axis=1))
    else:
        c = orc.camera_rays(np.arange(w * h, dtype=np.uint32))
        c8 = np.zeros((w * h, 8), np.float32)
        c8[:, 0:3], c8[:, 4:7] = c[:, 0:3], c[:, 3:6]
        ch = orc.trace_closest(c8)
        frac = np.mean(tid[:, 0] != np.where(ch[:, 0] < np.float32(3e38), ch[:, 1].view(np.int32), -1))
    assert frac >= 0.05, frac


# ---------------------------------------------------------------- 6. composition
def test_every_way_of_cutting_the_render_gives_the_same_film():
    """BOX and the lens, path tracing, cornell-mat 40 x 30, 6 samples. Six chunks of one sample have
    no pixel-to-sample index to get wrong, so their equality with the one-chunk film pins that index
    and the bounce-0 origin read of k_shade's PATH variant."""
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=40, height=30)
    setting = dict(filter="box", **LENS)
    want, st = film_of(s, 6, setting)
    assert st["chunk_samples"] == 6 and st["traced_camera_rays"] == 40 * 30 * 6
    assert not np.array_equal(want, film_of(s, 6)[0])
    assert not np.array_equal(want, film_of(s, 6, dict(filter="box"))[0])  # the lens reaches the film

    def tracer(**kw):
        rt = RayTracer(s, seed=1234, **kw)
        rt.set_camera_sampling(**setting)
        return rt
    rt = tracer()
    for _ in range(6):
        rt.render(1)
    assert_same_bits(rt.film()[0], want, "six calls of one sample")
    rt = tracer(max_paths=40 * 30 * 2)
    rt.render(6)
    assert rt.stats()["chunk_samples"] == 2
    assert_same_bits(rt.film()[0], want, "three chunks of two samples")
    rt = tracer()
    assert (rt.tiles_x, rt.tiles_y) == (2, 1)
    rt.render(6, tiles=[1], first_sample=0)
    rt.render(6, tiles=[0], first_sample=0)
    assert_same_bits(rt.film()[0], want, "two calls over complementary tiles")
    for flags in (0, N.RTG_OPT_NO_COALESCE):
        rt = tracer()
        rt.set_options(flags=rt.flags | flags)
        for _ in range(6):
            rt.render(1, sync=False)
        film, spp = rt.film()
        assert spp == 6
        assert_same_bits(film, want, "queued frames, flags %d" % flags)
    g = RayTracerGroup(s, devices=(0, 0), seed=1234)
    g.set_camera_sampling(**setting)
    g.render(6)
    assert_same_bits(g.film()[0], want, "two ranks, reduced")
    g.clear()
    for _ in range(6):
        g.render(1, sync=False)
    assert_same_bits(g.film()[0], want, "two ranks, queued frames")


# ---------------------------------------------------------------- 7. the setting itself
def test_setting_round_trips_and_default_is_restored():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=70, height=50)
    plain, st_plain = film_of(s, 3)
    rt = RayTracer(s, seed=1234)
    assert rt.camera_sampling() == {"filter": "none", "filter_radius": 0.5, "lens_radius": 0.0, "focal_distance": 1.0}
    rt.set_camera_sampling("tent")
    assert rt.camera_sampling() == {"filter": "tent", "filter_radius": 1.0, "lens_radius": 0.0, "focal_distance": 1.0}
    rt.set_camera_sampling("box", 0.25, 0.5, 3.0)
    assert rt.camera_sampling() == {"filter": "box", "filter_radius": 0.25, "lens_radius": 0.5, "focal_distance": 3.0}
    rt.set_camera_sampling("box")
    rt.render(3)
    jit, st = rt.film()[0], rt.stats()
    assert st["traced_camera_rays"] == 70 * 50 * 3 and not np.array_equal(jit, plain)
    rt.clear()
    rt.set_camera_sampling()  # NONE, R = 0: today's lean path again
    rt.render(3)
    assert_same_bits(rt.film()[0], plain, "default film after switching the setting back")
    assert rt.stats()["traced_camera_rays"] == 70 * 50 == st_plain["traced_camera_rays"]
    other = film_of(s, 3, dict(filter="box"), seed=99)[0]
    assert not np.array_equal(other, jit) and not np.array_equal(other, film_of(s, 3, seed=99)[0])
    assert_same_bits(film_of(s, 3, dict(filter="box"))[0], jit, "same seed, same jittered film")
    # the lens alone (no filter) also runs per sample
    f_lens, st_lens = film_of(s, 3, dict(lens_radius=0.05, focal_distance=5.0))
    assert st_lens["traced_camera_rays"] == 70 * 50 * 3 and not np.array_equal(f_lens, plain)


def test_every_integrator_takes_the_setting():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=40, height=30)
    for integ in ("direct", "direct_mis", "albedo", "normals"):
        a = film_of(s, 2, dict(filter="tent"), integrator=integ)[0]
        assert_same_bits(film_of(s, 2, dict(filter="tent"), integrator=integ)[0], a, integ + ": repeatable")
        assert not np.array_equal(a, film_of(s, 2, integrator=integ)[0]), integ
        zero = film_of(s, 2, dict(filter="tent", filter_radius=0.0), integrator=integ)[0]
        assert_same_bits(zero, film_of(s, 2, integrator=integ)[0], integ + ": radius 0 is the default film")


def test_argument_errors_leave_the_setting_alone():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=40, height=30)
    rt = RayTracer(s, seed=1234)
    rt.set_camera_sampling("tent", 1.5, 0.1, 2.0)
    keep = rt.camera_sampling()
    lib, h = N.rtg(), rt.handle
    nan, inf = float("nan"), float("inf")
    bad = [(3, 0.5, 0.0, 1.0), (-1, 0.5, 0.0, 1.0), (1, -0.1, 0.0, 1.0), (1, 4.5, 0.0, 1.0), (1, nan, 0.0, 1.0),
           (1, inf, 0.0, 1.0), (1, 0.5, -1.0, 1.0), (1, 0.5, nan, 1.0), (1, 0.5, inf, 1.0), (1, 0.5, 0.1, 0.0),
           (1, 0.5, 0.1, -2.0), (1, 0.5, 0.1, nan), (1, 0.5, 0.1, inf)]
    for b in bad:
        p = N.rtg_camera_sampling(*b)
        assert lib.rtg_set_camera_sampling(h, C.byref(p)) == -1, b  # RTG_ERR_ARG
        assert lib.rtg_last_error()
        assert rt.camera_sampling() == keep, b
    ok = N.rtg_camera_sampling(1, 0.5, 0.0, nan)  # no lens: the focal distance is not looked at
    assert lib.rtg_set_camera_sampling(h, C.byref(ok)) == 0
    rt.set_camera_sampling(**keep)
    assert lib.rtg_set_camera_sampling(h, None) == -1 and lib.rtg_set_camera_sampling(None, C.byref(ok)) == -1
    assert lib.rtg_get_camera_sampling(h, None) == -1 and lib.rtg_get_camera_sampling(None, C.byref(ok)) == -1
    assert lib.rtg_camera_sampling_defaults(None) == -1
    d = N.rtg_camera_sampling(9, 9, 9, 9)
    assert lib.rtg_camera_sampling_defaults(C.byref(d)) == 0
    assert (d.filter, d.filter_radius, d.lens_radius, d.focal_distance) == (0, 0.5, 0.0, 1.0)
    with pytest.raises(NativeError):
        rt.set_camera_sampling("box", 5.0)
    with pytest.raises(ValueError):
        rt.set_camera_sampling("gaussian")
    assert rt.camera_sampling() == keep
    # the probe: pixel >= W * H, sample >= 65536, null pointers
    with pytest.raises(NativeError):
        rt.camera_samples([40 * 30], [0])
    with pytest.raises(NativeError):
        rt.camera_samples([0], [65536])
    one = np.zeros(1, np.uint32)
    out = np.zeros(8, np.float32)
    u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    args = [h, one.ctypes.data_as(u32), one.ctypes.data_as(u32), 1, 1234, out.ctypes.data_as(f32), None]
    assert lib.rtg_probe_camera_samples(*args) == 0  # film_xy may be NULL
    for k in (0, 1, 2, 5):
        a = list(args)
        a[k] = None
        assert lib.rtg_probe_camera_samples(*a) == -1, k
    # the group: an argument error leaves every rank as it was
    g = RayTracerGroup(s, devices=(0, 0), seed=1234)
    g.set_camera_sampling("box", 0.75)
    with pytest.raises(NativeError):
        g.set_camera_sampling("box", 0.5, 0.1, 0.0)
    assert lib.rtg_group_set_camera_sampling(None, C.byref(ok)) == -1
    for r in range(2):
        p = N.rtg_camera_sampling()
        assert lib.rtg_get_camera_sampling(lib.rtg_group_handle(g._g, r), C.byref(p)) == 0
        assert (p.filter, p.filter_radius, p.lens_radius) == (1, 0.75, 0.0)


def test_adaptive_render_takes_the_setting():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=70, height=50)

    def adaptive(setting):
        rt = RayTracer(s, seed=1234)
        if setting:
            rt.set_camera_sampling(**setting)
        counts = rt.adaptiveRender(init_samples=2, max_samples=12, min_samples=1, first_sample=0)
        return rt.film()[0], counts
    a, ca = adaptive(dict(filter="box"))
    b, cb = adaptive(dict(filter="box"))
    assert_same_bits(a, b, "adaptive render with a box filter, twice")
    assert np.array_equal(ca, cb)
    assert not np.array_equal(a, adaptive(None)[0])


def test_guides_stay_centre_pinhole_samples():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=70, height=50)
    alb, nrm = RayTracer(s, seed=1234).guides()
    rt = RayTracer(s, seed=1234)
    rt.set_camera_sampling("tent", 2.0, 0.1, 5.0)
    keep = rt.camera_sampling()
    a, n = rt.guides()
    assert_same_bits(a, alb, "albedo guide")
    assert_same_bits(n, nrm, "normal guide")
    assert rt.camera_sampling() == keep
    before = rt.stats()["traced_camera_rays"]  # (the guides' two renders: a camera ray per pixel each)
    assert before == 2 * 70 * 50
    rt.render(2)
    assert rt.stats()["traced_camera_rays"] - before == 70 * 50 * 2  # and the setting still renders


def test_render_sharded_forwards_the_setting():
    from raytracingrenderer_amd.distributed import render_sharded, tiles_for_rank
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=70, height=50)
    setting = dict(filter="tent", **LENS)
    want = film_of(s, 3, setting)[0]
    rt = RayTracer(s, seed=1234)
    assert_same_bits(render_sharded(rt, 3, 0, 1, camera_sampling=setting), want, "world 1")
    assert rt.camera_sampling()["filter"] == "tent"
    total = np.zeros_like(want)
    for rank in range(2):  # each rank's own tiles, zero elsewhere: disjoint supports
        r = RayTracer(s, seed=1234)
        r.set_camera_sampling(**setting)
        r.render(3, tiles=tiles_for_rank(70, 50, rank, 2), first_sample=0)
        total += r.film()[0]
    assert_same_bits(total, want, "two ranks' own tiles")


def test_cli_writes_the_library_film(tmp_path):
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = os.path.join(SCENES, "cornell-box")
    base = [cli, "-scene", scene, "-SPP", "3", "-width", "64", "-height", "48", "-timeLimit", "0", "-outputFilename",
            "out.hdr", "-pixelFilter", "box", "-lensRadius", "0.05", "-focalDistance", "5"]
    rt = RayTracer(loadScene(scene, width=64, height=48), seed=1234)
    rt.set_camera_sampling("box", **LENS)
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.film()[0], 3)
    rt.clear()
    rt.set_camera_sampling("tent", 1.5)
    rt.render(3)
    save_hdr(str(tmp_path / "lib_tent.hdr"), rt.film()[0], 3)
    runs = (("one", [], "lib.hdr"), ("group", ["-devices", "0,0"], "lib.hdr"),
            ("tent", ["-pixelFilter", "tent", "-filterRadius", "1.5", "-lensRadius", "0"], "lib_tent.hdr"))
    for d, extra, want in runs:
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / d / "out.hdr").read_bytes() == (tmp_path / want).read_bytes(), d
    r = subprocess.run(base + ["-pixelFilter", "gaussian"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "pixelFilter" in r.stderr
