"""The C oracle (oracle/rt_oracle.c) pinned against the reference: the survey's C1 known answer
(reference integrator built with glibc libm), the reference's own traversal / camera code
(golden fixtures from oracle/_ref) and the reference's prior render result_144.hdr."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLD, REF_ROOT, SCENES, require_reference_libm
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import loadScene, read_hdr

FILM_KAT = json.load(open(os.path.join(GOLD, "film_kat.json")))


@pytest.fixture(scope="module")
def cornell256():
    return loadScene(os.path.join(SCENES, "cornell-box"), width=256, height=256)


def md5(img):
    return hashlib.md5(np.ascontiguousarray(img, np.float32).tobytes()).hexdigest()


@pytest.mark.host_glibc
def test_c1_known_answer_glibc(cornell256):
    """cornell 256^2 x 4 spp, depth 4, PCG seed 1234 -> md5 2fe4126e... (glibc 2.35)."""
    kat = FILM_KAT["C1_libm"]
    film, counts = Oracle(cornell256, 4, "libm").render(4, seed=1234, threads=8, count=True)
    img = film / np.float32(4.0)
    assert md5(img) == kat["md5"]
    np.testing.assert_allclose(img.reshape(-1, 3).astype(np.float64).mean(0), kat["means"], rtol=1e-6)
    for (x, y), rgb in zip(kat["pixels_xy"], kat["pixels_rgb"]):
        np.testing.assert_array_equal(img[y, x], np.float32(rgb))
    assert int((img.reshape(-1, 3) == 0).all(1).sum()) == kat["zero_pixels"]
    # rays per path 4.32: 702961 closest-hit + 429793 shadow rays for 262144 paths
    assert counts.tolist()[:3] == [262144, 702961, 429793]


def test_c1_shared_math_known_answer(cornell256):
    """With include/rtg_math.h (the GPU's transcendentals) the oracle gives the survey's glibc md5."""
    film, _ = Oracle(cornell256, 4, "rtm").render(4, seed=1234, threads=8)
    assert FILM_KAT["C1_rtm"]["md5"] == FILM_KAT["C1_libm"]["md5"]
    assert md5(film / np.float32(4.0)) == FILM_KAT["C1_rtm"]["md5"]


def test_threads_and_tiles_do_not_change_bits(cornell256):
    o = Oracle(cornell256, 4, "rtm")
    a, _ = o.render(2, seed=5, threads=1)
    b, _ = o.render(2, seed=5, threads=7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    tiles = np.arange(64, dtype=np.uint32)
    c = np.zeros_like(a)
    for part in (tiles[tiles % 3 == 0], tiles[tiles % 3 == 1], tiles[tiles % 3 == 2]):
        o.render(2, seed=5, tiles=part, threads=4, film=c)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("name,scene", [("cornell256", ("cornell-box", 256, 256)), ("synth20k", None)])
def test_traversal_matches_reference(name, scene, tmp_path):
    g = np.load(os.path.join(GOLD, "%s_rays.npz" % name))
    if scene is None:
        from raytracingrenderer_amd import write_synthetic_scene
        write_synthetic_scene(str(tmp_path), n_tris=20000, seed=3, width=128, height=96)
        s = loadScene(str(tmp_path))
    else:
        s = loadScene(os.path.join(SCENES, scene[0]), width=scene[1], height=scene[2])
    o = Oracle(s, 4, "rtm")
    assert np.array_equal(o.trace_closest(g["rays"]).view(np.uint32), g["hits"].view(np.uint32))
    assert np.array_equal(o.trace_visible(g["rays"]), g["visible"])
    assert np.array_equal(o.camera_rays(g["pixels"]).view(np.uint32), g["camera_rays"].view(np.uint32))


def test_statistical_agreement_with_reference_render(cornell256, tmp_path):
    """result_144.hdr: a 1024^2 cornell render written by the reference (Main.cpp:132-136). Our
    16-spp oracle film goes through the same RGBE writer (its mantissa truncation biases values
    down ~0.3-0.5 %), then 8x8 grid block luminances are compared."""
    path = os.path.join(REF_ROOT, "result_144.hdr")
    if not os.path.exists(path):
        pytest.skip("reference outputs not available here")
    from raytracingrenderer_amd import save_hdr
    ref = read_hdr(path)
    s = loadScene(os.path.join(SCENES, "cornell-box"))
    film, _ = Oracle(s, 4, "libm").render(16, seed=1234, threads=os.cpu_count() or 8)
    ok = np.isfinite(film).all(axis=2)
    assert ok.mean() > 0.9999  # the reference's pdf=0 edge case yields a rare inf pixel
    film = np.where(ok[..., None], film, ref * np.float32(16))
    save_hdr(str(tmp_path / "o.hdr"), film, 16)
    img = read_hdr(str(tmp_path / "o.hdr"))
    lum = lambda a: (a.astype(np.float64) * [0.2126, 0.7152, 0.0722]).sum(-1).reshape(8, 128, 8, 128).mean((1, 3))
    rel = np.abs(lum(img) - lum(ref)) / lum(ref)
    assert np.median(rel) < 0.003 and rel.max() < 0.015


def test_oracle_alternative_integrators_plumbing():
    """direct / albedo / normals estimators in the oracle: sane values on cornell (CPU only)."""
    import os
    import numpy as np
    from conftest import SCENES
    from oracle.pyoracle import Oracle
    from raytracingrenderer_amd import loadScene
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=32, height=32)
    nrm, _ = Oracle(s, 4, "rtm", integrator=3).render(1, seed=1)
    assert np.all(nrm >= 0) and np.all(nrm <= 1.0001) and nrm.max() > 0.5
    alb, _ = Oracle(s, 4, "rtm", integrator=2).render(1, seed=1)
    assert np.isfinite(alb).all() and alb.max() > 0
    dr, _ = Oracle(s, 4, "rtm", integrator=1).render(2, seed=1)
    pt, _ = Oracle(s, 4, "rtm", integrator=0).render(2, seed=1)
    assert 0 < dr.mean() < pt.mean()  # direct light only is darker than full path tracing


LIGHT_KAT = os.path.join(GOLD, "light_kat.npz")


@pytest.mark.parametrize("tag,scene,w,h", [("cornell", "cornell-box", 96, 64), ("mat", "cornell-mat", 80, 60)])
def test_light_tracing_pieces_match_reference(tag, scene, w, h):
    """The camera members light tracing needs (projectionMatrix, cameraToView, viewDirection, Afilm)
    as librth computes them, Camera::projectOntoCamera (Scene.h:55-69) and AreaLight's emission
    sample (Lights.h:30-80) in the oracle, against the reference's own classes (light_kat.npz)."""
    z = np.load(LIGHT_KAT)
    s = loadScene(os.path.join(SCENES, scene), width=w, height=h)
    pr = s.desc.projection
    got = np.concatenate([np.array(pr.proj[:], np.float32), np.array(pr.camera_to_view[:], np.float32),
                          np.array(pr.view_direction[:], np.float32), np.float32([pr.a_film])])
    np.testing.assert_array_equal(got.view(np.uint32), z[tag + "_state"].view(np.uint32))
    o = Oracle(s, 4, "rtm")
    np.testing.assert_array_equal(o.camera_project(z[tag + "_pts"]).view(np.uint32), z[tag + "_proj"].view(np.uint32))
    emits = np.array([o.light_emit(li, d) for li, d in zip(z[tag + "_li"], z[tag + "_draws"])], np.float32)
    np.testing.assert_array_equal(emits.view(np.uint32), z[tag + "_emit"].view(np.uint32))


def test_light_tracer_and_radiosity_oracles_are_deterministic():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=40, height=32)
    o = Oracle(s, 4, "rtm")
    a = o.render_light(2, seed=3)
    b = o.render_light(1, first=1, seed=3, film=o.render_light(1, first=0, seed=3))
    np.testing.assert_array_equal(a, b)
    assert np.isfinite(a).all() and (a > 0).sum() > 100
    c = o.render_instant_radiosity(1, seed=3, n_vpl=10)
    assert np.isfinite(c).all() and (c > 0).sum() > 100


# ---- film-level pin on the reference's own classes (oracle/_ref ref_render)
REF_FILM_CASES = [
    # (scene, kwargs, max_depth, spp, seed): glass / mirror / env (cornell-mat), C4's bathroom_f with
    # JPEG/PNG textures at depth 16, C5's coffee_f + GI.hdr, and a synthetic env-lit scene
    ("cornell-mat", dict(width=80, height=60), 8, 3, 99),
    ("bathroom", dict(width=96, height=54, skip_missing=True), 16, 2, 7),
    ("coffee", dict(width=80, height=100, skip_missing=True, envmap="GI.hdr"), 4, 3, 5),
    # the one reference scene whose environment map is a light (lights[0], Scene.h:156-159;
    # EnvironmentMap, Lights.h:135-201): materialball_f (Mesh002.gem is missing)
    ("materialball", dict(width=96, height=54, skip_missing=True), 8, 2, 13),
]


def _ref_scene_dir(name):
    from conftest import scene_path
    p = scene_path(name)
    if p is None:
        pytest.skip("%s assets not available here" % name)
    return p


@pytest.mark.parametrize("flavour", ["libm", "rtm"])
@pytest.mark.parametrize("case", range(len(REF_FILM_CASES)))
def test_oracle_film_equals_reference_classes(case, flavour):
    """The C oracle's integrator against RayTracer::pathTrace restated on RTBase's own compiled
    classes (ref_render: Scene::traverse/visible, calculateShadingData, BSDF::sample/evaluate,
    Light::sample, Camera, Film::splat from /root/reference), with glibc and with the shared
    transcendentals: films identical bit for bit, and the same closest-hit / shadow ray counts."""
    if flavour == "libm":
        require_reference_libm()
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built")
    name, kw, depth, spp, seed = REF_FILM_CASES[case]
    path = _ref_scene_dir(name)
    r = pyref.RefScene(path, kw["width"], kw["height"], kw.get("skip_missing", False), kw.get("envmap"), flavour=flavour)
    ref, rc = r.render(spp, seed=seed, max_depth=depth, threads=8)
    s = loadScene(path, **kw)
    mine, oc = Oracle(s, depth, flavour).render(spp, seed=seed, threads=8, count=True)
    assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (mine != ref).sum()
    assert rc.tolist() == oc[:3].tolist()


@pytest.mark.parametrize("case", [3, 6])
def test_oracle_equals_reference_classes_at_the_table_limits(case, tmp_path):
    """The scenes of tests/test_shade_tables.py with 64 materials / 48 lights and with about 150
    materials / 281 lights (environment light included; every fixture scene has at most 6 lights): the C
    oracle's path tracer, light tracer and instant radiosity against the same integrators on RTBase's own
    compiled classes (oracle/_ref, shared transcendentals), bit for bit. The GPU is compared with the
    oracle on these scenes; this pins the oracle itself there, light selection included."""
    from oracle import pyref
    from shade_scenes import table_cases, table_counts, write_table_scene
    if not pyref.available():
        pytest.skip("oracle/_ref not built")
    n_emitters, n_extra, envmap, want_mats, want_lights, _ = table_cases()[case]
    path = write_table_scene(tmp_path / "scene", n_emitters, n_extra, envmap)
    s = loadScene(path)
    assert table_counts(s) == (want_mats, want_lights)
    r = pyref.RefScene(path, 64, 48, False, flavour="rtm")
    assert r.nlight == want_lights
    o = Oracle(s, 6, "rtm")
    a, ca = r.render(3, seed=31, max_depth=6, threads=8)
    b, cb = o.render(3, seed=31, threads=8, count=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a != b).sum()
    assert ca.tolist() == cb[:3].tolist()
    assert np.isfinite(b).all() and (b != 0).mean() > 0.5
    a, b = pyref.render_light(r, 1, seed=33), o.render_light(1, seed=33)
    assert (b != 0).sum() > 100
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a != b).sum()
    a, b = pyref.render_instant_radiosity(r, 1, seed=34, n_vpl=8), o.render_instant_radiosity(1, seed=34, n_vpl=8)
    assert (b != 0).sum() > 100
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a != b).sum()


@pytest.mark.host_glibc
def test_c1_known_answer_from_reference_classes():
    """SURVEY.md §8c's C1 md5 (the reference integrator built in the survey, glibc) is reproduced by
    ref_render on the reference's own classes, so both the oracle and ref_render are pinned to it."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built")
    r = pyref.RefScene(os.path.join(SCENES, "cornell-box"), 256, 256, False)
    film, c = r.render(4, seed=1234, max_depth=4, threads=8)
    assert hashlib.md5((film / np.float32(4)).astype(np.float32).tobytes()).hexdigest() == "2fe4126eaf3a9c654e6beea0a1da9ba9"
    assert c.tolist() == [262144, 702961, 429793]


@pytest.mark.host_glibc
@pytest.mark.parametrize("scene_name", ["cornell-box", "cornell-mat"])
def test_oracle_integrators_equal_reference_classes(scene_name):
    """f4: every alternative integrator of the oracle (direct, albedo, viewNormals, computeDirectMIS,
    lightTracer, instantRadiosity, adaptiveRender; Renderer.h:82-326, 393-749) against the same
    integrator restated on RTBase's own compiled classes (oracle/_ref), with glibc and with the
    shared transcendentals: films (and adaptive tile counts) identical bit for bit."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built")
    path = os.path.join(SCENES, scene_name)
    s = loadScene(path, width=64, height=48)
    for fl in ("libm", "rtm"):
        r = pyref.RefScene(path, 64, 48, False, flavour=fl)
        for mode in (1, 2, 3, 4):
            a, ca = r.render(3, seed=7, max_depth=4, mode=mode)
            b, cb = Oracle(s, 4, fl, integrator=mode).render(3, seed=7, threads=8, count=True)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (fl, mode)
            assert ca.tolist() == cb[:3].tolist()
        o = Oracle(s, 4, fl)
        assert np.array_equal(pyref.render_light(r, 2, seed=5).view(np.uint32), o.render_light(2, seed=5).view(np.uint32))
        assert np.array_equal(pyref.render_instant_radiosity(r, 2, seed=9, n_vpl=20).view(np.uint32),
                              o.render_instant_radiosity(2, seed=9, n_vpl=20).view(np.uint32))
        fa, ca = pyref.render_adaptive(r, seed=11, init=2, max_samples=12)
        fb, cb = o.render_adaptive(seed=11, init=2, max_samples=12)
        assert ca.tolist() == cb.tolist() and np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
