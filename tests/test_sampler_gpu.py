"""The Owen-scrambled Sobol sampler on the GPU (rtg_set_sampler, RTG_SAMPLER_SOBOL): the kernels' draw
function and the camera sample against the numpy restatement (tests/sobol_ref.py) bit for bit, DIRECT and
PATH films rebuilt sample by sample with SobolStream in PathStream's place (the uniform pick, the power
pick, the environment's luminance table), the draw counter across bounces, the two samplers' agreement in
expectation with less noise in the new one, and what the mode must leave alone."""
import json
import os
import subprocess

import numpy as np
import pytest

import camera_ref as cr
import env_sampling_ref as er
import light_sampling_ref as lr
import sobol_ref as sr
from conftest import SCENES
from env_scenes import smooth_map
from light_pick_scenes import write_emitters_env_scene, write_unequal_scene
from material_scenes import write_material_floor_scene
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, probe_texture, save_hdr
from raytracingrenderer_amd import _native as N

pytestmark = pytest.mark.gpu

F = np.float32
U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def cornell(w, h, name="cornell-box"):
    return loadScene(os.path.join(SCENES, name), width=w, height=h)


def tracer(s, seed, integrator="path", sampler="sobol", power=False, env_mode="uniform", **kw):
    rt = RayTracer(s, seed=seed, integrator=integrator, **kw)
    rt.set_env_sampling(env_mode)
    if power:
        rt.set_light_sampling("power")
    rt.set_sampler(sampler)
    return rt


# ---------------------------------------------------------------- 1. the probe
@pytest.mark.parametrize("stream", [0, sr.CAMERA_STREAM])
def test_probe_equals_the_restatement(stream):
    """256 (pixel, sample) pairs x 24 draws, on the path's and the camera's stream, with the corner pixels of
    a 4096^2 film and the sample numbers where a bit of the index turns; a probe that starts at draw 5
    agrees with the one from 0 on the overlap (the draw is a function of n alone)."""
    rng = np.random.default_rng(11)
    pix = np.concatenate([[0, 4096 * 4096 - 1] * 7, rng.integers(0, 4096 * 4096, 242)]).astype(U32)
    smp = np.concatenate([np.repeat([0, 1, 2, 3, 255, 256, 65535], 2), rng.integers(0, 65536, 242)]).astype(U32)
    assert len(pix) == len(smp) == 256
    for seed in (1234, 0xFEDCBA9876543210):
        got = N.probe_sampler(seed, pix, smp, 24, stream=stream)
        st = sr.SobolStream(pix, smp, seed, stream)
        want = np.stack([st.raw() for _ in range(24)], axis=1)
        assert got.dtype == U32 and np.array_equal(got, want), int((got != want).sum())
        late = N.probe_sampler(seed, pix, smp, 19, first_draw=5, stream=stream)
        assert np.array_equal(late, got[:, 5:])
    other = N.probe_sampler(1234, pix, smp, 24, stream=stream ^ 1)
    assert (other != N.probe_sampler(1234, pix, smp, 24, stream=stream)).mean() > 0.99


# ---------------------------------------------------------------- 2. camera samples
def test_camera_samples_equal_the_restatement(monkeypatch):
    """camera_samples under "tent" and a lens on cornell-box 33 x 31, samples 0..3: tests/camera_ref.py's
    restatement with its four draws taken from SobolStream's camera stream; the PCG rays are others."""
    s = cornell(33, 31)
    rt = RayTracer(s, seed=1234)
    rt.set_camera_sampling("tent", None, lens_radius=0.05, focal_distance=5.0)
    cs = rt.camera_sampling()
    pix = np.repeat(np.arange(33 * 31, dtype=U32), 4)
    smp = np.tile(np.arange(4, dtype=U32), 33 * 31)
    pcg_rays, _ = rt.camera_samples(pix, smp)
    rt.set_sampler("sobol")
    assert rt.sampler == "sobol" and rt.sampler_active == "sobol"

    def sobol_draws(pixels, samples, seed):
        st = sr.SobolStream(pixels, samples, seed, sr.CAMERA_STREAM)
        return np.stack([st.next() for _ in range(4)], axis=1)
    monkeypatch.setattr(cr, "camera_draws", sobol_draws)
    for seed in (1234, 0xFEDCBA9876543210):
        rays, xy = rt.camera_samples(pix, smp, seed=seed)
        want, wxy = cr.camera_samples_ref(s.camera, pix, smp, seed, cr.FILTER_TENT, cs["filter_radius"],
                                          cs["lens_radius"], cs["focal_distance"])
        assert_same_bits(xy, wxy, "film position")
        assert_same_bits(rays, want, "rays")
    assert not np.array_equal(bits(rt.camera_samples(pix, smp)[0]), bits(pcg_rays))


# ---------------------------------------------------------------- 3. exact films
def shading_normals(s, rays, hits, tri):
    """k_shade's shading normal of each first hit, in its float32 operations: the interpolated vertex
    normals, normalised, turned to the viewer on a two-sided material."""
    nrm = s.normals[tri]
    al, be = hits[:, 2], hits[:, 3]
    ga = F(1) - (al + be)
    v = (nrm[:, 0] * al[:, None] + nrm[:, 1] * be[:, None]) + nrm[:, 2] * ga[:, None]
    sn = lr.normalize3(v.astype(F))
    two = np.array([m.two_sided for m in s.materials], np.int32)[s.material_index[tri]] != 0
    back = lr.dot3(-rays[:, 4:7], sn) < 0
    return np.where((two & back)[:, None], -sn, sn).astype(F)


def film_ref(s, rt, ns, seed, power=False, luminance=False, stream=sr.SobolStream):
    """The DIRECT film of ns samples rebuilt in numpy, as tests/test_light_sampling_gpu.py's film_ref and
    tests/test_env_sampling_gpu.py's direct_film_ref do, with the draws from `stream`: per pixel whose
    camera ray hits a non-emissive surface, the sample-ordered sum of f E g / (pmf pdf) over visible
    samples (the uniform pick's one draw or the power pick's r0 and d1, then Triangle::sample's r1, r2 or
    the environment branch's two or four draws), from light_records(), the ALBEDO film for f, the shading
    normal restated (its absolute value is checked against the NORMALS film), trace_closest for the hit and
    trace_visible for the shadow ray; per pixel that sees an emitter, its emission per sample. Every
    material is diffuse. Returns (film (H, W, 3), surface mask, occluded count, visible count)."""
    W, H = s.width, s.height
    assert all(m.kind in (0, 1) for m in s.materials)
    rec = rt.light_records()
    nl = len(rec)
    ent = rt.light_table()["entries"] if power else None
    kind = rec[:, 7].copy().view(np.int32)
    has_env = (kind == 1).any()
    tex = s.texture(s.desc.env_texture).copy() if has_env else None
    eent = rt.env_table()["entries"] if luminance else None
    guide = RayTracer(s, seed=seed, integrator="albedo")
    guide.render(1)
    f = guide.film()[0].reshape(-1, 3)
    guide.clear()
    guide.set_integrator("normals")
    guide.render(1)
    abs_sn = guide.film()[0].reshape(-1, 3)
    pix = np.arange(W * H, dtype=np.uint32)
    plain = RayTracer(s, seed=seed)  # (pixel-centre rays: no camera sampling in these films)
    rays, _ = plain.camera_samples(pix, np.zeros(W * H, np.uint32))
    hits = rt.trace_closest(rays)
    hit = hits[:, 0] < F(3.0e38)
    tri = np.where(hit, hits[:, 1].copy().view(np.int32), 0)
    mat = s.material_index[tri]
    em_of = np.array([m.emission[:] for m in s.materials], F)
    emitter = hit & (em_of[mat].sum(1) > 0)
    surf = hit & ~emitter
    film = np.zeros((W * H, 3), F)
    n_occ = n_vis = 0
    old = np.seterr(all="ignore")  # (a missed pixel's t = FLT_MAX runs through the arithmetic unused)
    sn = shading_normals(s, rays, hits, tri)
    assert_same_bits(np.abs(sn)[surf], abs_sn[surf], "the restated shading normal against the NORMALS film")
    x = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]  # Ray::at
    for sl in range(ns):
        st = stream(pix, np.full(W * H, sl, np.uint32), seed)
        if power:
            r0 = st.raw()
            d1 = st.next()
            li, pmf = lr.pick(ent, r0, d1)
        else:
            li = np.minimum((F(nl) * st.next()).astype(np.int32), nl - 1)
            pmf = np.full(W * H, F(1) / F(nl), F)
        L = rec[li]
        a_raw = st.raw()
        a = (a_raw >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
        b = st.next()
        p2 = lr.triangle_sample(L, a, b)  # an area light: Triangle::sample(r1 = a, r2 = b)
        g, _ = lr.area_geometry(L, p2, x, sn)
        emitted = L[:, 16:19]
        pdf = L[:, 11]
        if has_env:
            if luminance:  # r0 = a's raw draw, then d1, d2, d3
                d = np.stack([b, st.next(), st.next()], axis=1)
                wi, epdf, _ = er.sample(eent, tex.shape[1], tex.shape[0], a_raw, d)
            else:          # uniformSampleSphere(q1, q2): q2 is the first draw
                wi, epdf = er.uniform_sample(b, a)
                epdf = np.full(W * H, epdf, F)
            ge = lr.dot3(wi, sn)
            ge = np.where((ge > 0) & (epdf > 0), ge, F(0)).astype(F)
            isenv = kind[li] == 1
            E = probe_texture(tex, wi, env=True)
            p2 = np.where(isenv[:, None], x + wi * F(10000.0), p2).astype(F)
            g = np.where(isenv, ge, g).astype(F)
            emitted = np.where(isenv[:, None], E, emitted).astype(F)
            pdf = np.where(isenv, epdf, pdf).astype(F)
        act = surf & (g > 0)
        ld = (((f * emitted) * g[:, None]) / (pmf * pdf)[:, None]).astype(F)
        q = lr.shadow_ray(x, p2)
        q[~act] = (0, 1e6, 0, 1, 0, 1, 0, 0)  # (unused lanes: a ray far above everything)
        vis = rt.trace_visible(q) != 0
        lit = surf & (f.sum(1) > 0)
        n_occ += int((act & ~vis & lit).sum())
        n_vis += int((act & vis & lit).sum())
        c = np.where((act & vis)[:, None], ld, F(0)).astype(F)
        c = np.where(emitter[:, None], em_of[mat], c).astype(F)
        film = film + c
    np.seterr(**old)
    return film.reshape(H, W, 3), surf.reshape(H, W), n_occ, n_vis


def check_cuts(s, rt, want, seed, integrator, power=False, env_mode="uniform", cuts="all"):
    """rt's film of 4 samples equals `want` bit for bit from one call, four 1-spp calls, queued frames,
    two complementary tile sets and a two-rank group on device 0 twice."""
    rt.clear()
    rt.render(4)
    assert_same_bits(rt.film()[0], want, "one call")
    if cuts != "all":
        return
    rt.clear()
    for _ in range(4):
        rt.render(1)
    assert_same_bits(rt.film()[0], want, "four 1-spp calls")
    rt.clear()
    for _ in range(4):
        rt.render(1, sync=False)
    assert_same_bits(rt.film()[0], want, "queued frames")
    rt.clear()
    tiles = np.arange(rt.tiles_x * rt.tiles_y, dtype=np.uint32)
    for part in (tiles[0::2], tiles[1::2]):
        if len(part):
            rt.render(4, tiles=part, first_sample=0)
    assert_same_bits(rt.film()[0], want, "two complementary tile sets")
    g = RayTracerGroup(s, devices=(0, 0), seed=seed)
    for r in range(2):  # (the group has no integrator setting of its own: through each rank's handle)
        assert g._lib.rtg_set_integrator(g._lib.rtg_group_handle(g._g, r), RayTracer.INTEGRATORS[integrator]) == 0
    g.set_env_sampling(env_mode)
    if power:
        g.set_light_sampling("power")
    g.set_sampler("sobol")
    g.render(4)
    assert_same_bits(g.film()[0], want, "two-rank group on device 0 twice")


@pytest.mark.parametrize("size", [(64, 48), (33, 31)])
def test_direct_film_is_the_restated_sum_however_it_is_cut(size):
    """cornell-box under DIRECT, 4 spp, the uniform pick (k_sobol_shade<true, *>): the film equals the sum
    rebuilt from SobolStream bit for bit however it is cut; the restatement itself is pinned by rebuilding
    the PCG film with PathStream; the two films differ."""
    s = cornell(*size)
    W, H = size
    rt = tracer(s, 77, "direct")
    assert rt.sampler_active == "sobol"
    want, surf, n_occ, n_vis = film_ref(s, rt, 4, 77)
    print("surface pixels %d of %d, occluded samples %d, visible %d" % (surf.sum(), W * H, n_occ, n_vis))
    assert surf.sum() > 0.5 * W * H and n_occ > 0 and n_vis > 0
    check_cuts(s, rt, want, 77, "direct", cuts="all" if size == (64, 48) else "one")
    pcg = tracer(s, 77, "direct", sampler="pcg")
    pcg.render(4)
    assert_same_bits(pcg.film()[0], film_ref(s, pcg, 4, 77, stream=er.PathStream)[0], "the PCG film, restated")
    assert not np.array_equal(bits(pcg.film()[0]), bits(want))


# ---------------------------------------------------------------- 4. with the modes
def test_power_pick_films_are_the_restated_sum(tmp_path):
    """The "unequal" scene (22 lights, the tables in LDS) under the power pick, 4 spp: DIRECT
    (k_sobol_shade_pick<true, *, false>) equals the rebuilt sum, and so does PATH at depth 4
    (k_sobol_shade_pick<false, *, false>): nothing a bounce can reach reflects light, so every later
    term is thr * 0 = +0 whatever the later bounces draw."""
    s = loadScene(write_unequal_scene(tmp_path / "u", 64, 48))
    assert len(s.lights) == 22 and s.desc.env_texture < 0
    rt = tracer(s, 77, "direct", power=True)
    want, surf, n_occ, n_vis = film_ref(s, rt, 4, 77, power=True)
    assert surf.sum() > 0.3 * 64 * 48 and n_occ > 0 and n_vis > 0 and (want[~surf] == 0).all()
    check_cuts(s, rt, want, 77, "direct", power=True, cuts="one")
    pt = tracer(s, 77, "path", power=True, max_depth=4)
    assert pt.sampler_active == "sobol"
    check_cuts(s, pt, want, 77, "path", power=True, cuts="one")
    pcg = tracer(s, 77, "direct", sampler="pcg", power=True)
    pcg.render(4)
    assert not np.array_equal(bits(pcg.film()[0]), bits(want))


@pytest.mark.parametrize("power", [False, True])
def test_luminance_film_is_the_restated_sum(tmp_path, power):
    """The floor under four emitters and a smooth 16 x 8 environment map in the light list (9 lights), the
    environment sampled through its luminance table, DIRECT, 4 spp: k_sobol_shade_env<true, *> with the
    uniform pick, k_sobol_shade_pick<true, *, true> with the power pick."""
    s = loadScene(write_emitters_env_scene(tmp_path / "e", smooth_map(16, 8), 4))
    assert len(s.lights) == 9 and (np.array(s.lights) == -1).sum() == 1
    rt = tracer(s, 78, "direct", power=power, env_mode="luminance")
    assert rt.env_table() is not None and rt.sampler_active == "sobol"
    want, surf, n_occ, n_vis = film_ref(s, rt, 4, 78, power=power, luminance=True)
    assert surf.sum() > 0.3 * surf.size and n_vis > 0
    check_cuts(s, rt, want, 78, "direct", power=power, env_mode="luminance", cuts="one")


# ---------------------------------------------------------------- 5. the counter across bounces
def test_path_film_does_not_depend_on_how_it_is_cut():
    """cornell-mat under PATH at depth 4, 32 x 24, 2 spp (glass, a mirror, an environment map: paths of
    every length, each bounce opening its own 4-D point from the counter in the payload): one call, two
    1-spp calls and two tile sets give one film, which is not the PCG film; and a depth-1 film equals it on
    the pixels whose path ends at the camera ray's hit (an emitter or a miss)."""
    s = cornell(32, 24, "cornell-mat")
    rt = tracer(s, 5, "path", max_depth=4)
    rt.render(2)
    want = rt.film()[0].copy()
    assert np.isfinite(want).all() and want.sum() > 0
    rt.clear()
    rt.render(1)
    rt.render(1)
    assert_same_bits(rt.film()[0], want, "two 1-spp calls")
    rt.clear()
    tiles = np.arange(rt.tiles_x * rt.tiles_y, dtype=np.uint32)
    parts = (tiles[0::2], tiles[1::2]) if len(tiles) > 1 else (tiles,)
    for part in parts:
        rt.render(2, tiles=part, first_sample=0)
    assert_same_bits(rt.film()[0], want, "tile sets")
    halves = tracer(s, 5, "path", max_depth=4, max_paths=32 * 24)  # two chunks of one sample
    halves.render(2)
    assert halves.stats()["chunk_samples"] == 1
    assert_same_bits(halves.film()[0], want, "two chunks")
    pcg = tracer(s, 5, "path", sampler="pcg", max_depth=4)
    pcg.render(2)
    assert not np.array_equal(bits(pcg.film()[0]), bits(want))
    shallow = tracer(s, 5, "path", max_depth=1)
    shallow.render(2)
    pix = np.arange(32 * 24, dtype=np.uint32)
    hits = rt.trace_closest(RayTracer(s).camera_samples(pix, np.zeros(32 * 24, np.uint32))[0])
    hit = hits[:, 0] < F(3.0e38)
    tri = np.where(hit, hits[:, 1].copy().view(np.int32), 0)
    em = np.array([m.emission[:] for m in s.materials], F)[s.material_index[tri]].sum(1) > 0
    ends = (~hit | em).reshape(24, 32)
    assert ends.sum() > 0
    assert_same_bits(shallow.film()[0][ends], want[ends], "paths that end at the camera ray's hit")


# ---------------------------------------------------------------- 6. same expectation
def test_path_means_agree_between_the_samplers():
    """PATH on cornell-box, depth 4, 32 x 32, 8 seeds x 64 spp per sampler: the image-mean luminances differ
    by at most 4 standard errors of the PCG seeds' spread (a guard against a wrong estimator: with 8 seeds
    a correct sampler exceeds it with probability < 1e-3)."""
    s = cornell(32, 32)
    means = {}
    for name in ("pcg", "sobol"):
        rt = tracer(s, 0, "path", sampler=name, max_depth=4)
        m = []
        for k in range(8):
            rt.seed = 3000 + k
            rt.clear()
            rt.render(64)
            f, spp = rt.film()
            m.append(float(er.lum32(f / F(spp)).astype(np.float64).mean()))
        means[name] = np.array(m)
    mu = {k: v.mean() for k, v in means.items()}
    se = means["pcg"].std(ddof=1) / np.sqrt(8)
    print("means %r, standard error of the PCG mean %g" % (mu, se))
    assert se <= 0.05 * mu["pcg"]
    assert abs(mu["pcg"] - mu["sobol"]) <= 4 * se


# ---------------------------------------------------------------- 7. less noise
def measured_ratio():
    with open(os.path.join(ROOT, "profiles", "sampler_time.json")) as f:
        return float(json.load(f)["test_mse_ratio"]["ratio"])


def mse_ratio_cornell_direct():
    """(MSE of Sobol, MSE of PCG): cornell-box DIRECT 64 x 64 at 16 spp, the mean squared error of the
    luminance over 8 seeds against a 4096-spp PCG film of the same scene."""
    s = cornell(64, 64)
    ref = tracer(s, 99991, "direct", sampler="pcg")
    ref.render(4096)
    f, spp = ref.film()
    truth = er.lum32(f / F(spp)).astype(np.float64)
    mse = {}
    for name in ("pcg", "sobol"):
        rt = tracer(s, 0, "direct", sampler=name)
        e = []
        for k in range(8):
            rt.seed = 4000 + k
            rt.clear()
            rt.render(16)
            f, spp = rt.film()
            e.append(float(((er.lum32(f / F(spp)).astype(np.float64) - truth) ** 2).mean()))
        mse[name] = float(np.mean(e))
    return mse["sobol"], mse["pcg"]


def test_sobol_is_less_noisy_at_equal_samples():
    """Sobol's MSE is below PCG's by at least half the measured gain in log terms: the bound is the
    geometric mean of 1 and the ratio tools/sampler_time.py measured (profiles/sampler_time.json, which must
    itself be below 0.8), well clear of the seed-to-seed spread."""
    measured = measured_ratio()
    assert measured < 0.8, measured
    sob, pcg = mse_ratio_cornell_direct()
    print("MSE sobol %g, pcg %g, ratio %g (measured %g, bound %g)" % (sob, pcg, sob / pcg, measured, np.sqrt(measured)))
    assert sob < pcg
    assert sob / pcg <= np.sqrt(measured)


# ---------------------------------------------------------------- 8. what the mode must leave alone
def test_pcg_set_explicitly_is_todays_film_and_fallbacks_keep_pcg(tmp_path):
    s = cornell(33, 31)
    never = RayTracer(s, seed=9)
    assert never.sampler == "pcg" and never.sampler_active == "pcg"
    never.render(3)
    rt = RayTracer(s, seed=9)
    rt.set_sampler("sobol")
    rt.set_sampler("pcg")
    rt.render(3)
    assert_same_bits(rt.film()[0], never.film()[0], "pcg after sobol")
    # an argument error keeps the previous setting
    rt.set_sampler("sobol")
    with pytest.raises(NativeError):
        rt.set_sampler(7)
    with pytest.raises(ValueError):
        rt.set_sampler("halton")
    assert rt.sampler == "sobol" and rt.sampler_active == "sobol"
    # integrators that draw nothing, and the light tracer: the PCG kernels
    for integ in ("albedo", "normals"):
        rt.set_integrator(integ)
        assert rt.sampler_active == "pcg"
    # kernels without a Sobol variant keep PCG: the films are the PCG films, and sampler_active says so
    phys = loadScene(write_material_floor_scene(tmp_path / "m", "orennayar", 33, 31))
    for setting in ("physical", "path_mis"):
        films = []
        for name in ("pcg", "sobol"):
            pt = RayTracer(phys if setting == "physical" else s, seed=9, integrator="path", max_depth=3)
            if setting == "physical":
                pt.set_material_model("physical")
            else:
                pt.set_path_mis("power")
            pt.set_sampler(name)
            assert pt.sampler == name and pt.sampler_active == "pcg", (setting, name)
            pt.render(2)
            films.append(pt.film()[0])
        assert_same_bits(films[1], films[0], setting)


def test_cli_sampler_writes_the_library_film(tmp_path):
    """-sampler sobol on cornell-box: the file is Film::save of the library's film, for one device and for
    a two-rank group; without the option the file is another."""
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = os.path.join(SCENES, "cornell-box")
    s = loadScene(scene, width=33, height=31)
    rt = tracer(s, 1234, "path")
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.film()[0], 3)
    base = [cli, "-scene", scene, "-SPP", "3", "-timeLimit", "0", "-outputFilename", "out.hdr", "-width", "33",
            "-height", "31"]
    out = {}
    for d, extra in (("sobol", ["-sampler", "sobol"]), ("pcg", []), ("group", ["-sampler", "sobol", "-devices", "0,0"])):
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[d] = (tmp_path / d / "out.hdr").read_bytes()
    assert out["sobol"] == (tmp_path / "lib.hdr").read_bytes()
    assert out["group"] == out["sobol"]
    assert out["pcg"] != out["sobol"]
