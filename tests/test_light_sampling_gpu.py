"""Light selection for NEE on the GPU (rtg_set_light_sampling, RTG_LIGHTS_POWER): the handle's weights
and table and the kernel's pick against the numpy restatement (tests/light_sampling_ref.py) bit for bit,
DIRECT and PATH films rebuilt sample by sample (with and without the environment's luminance table, with
the tables in LDS and in global memory), the two modes' agreement in expectation with less noise in the
new one, and the fall-backs and entry points that must keep today's films."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_sampling_ref as er
import light_sampling_ref as lr
from conftest import SCENES
from env_scenes import smooth_map
from light_pick_scenes import write_emitters_env_scene, write_one_triangle_scene, write_unequal_scene
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, probe_texture, save_hdr
from raytracingrenderer_amd import _native as N
from shade_scenes import table_limits, write_table_scene
from test_light_sampling import unequal_variance_ratio

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def env_texels(scene):
    return scene.texture(scene.desc.env_texture).copy()


def restated_table(s, rt, lam=0.125):
    """The restatement's weights and table from the device's own records (and, with an environment light,
    the loaded texels and the root box)."""
    rec = rt.light_records()
    has_env = (np.array(s.lights) == -1).any()
    w = lr.light_weights(rec, env_texels(s) if has_env else None, s.node_bounds[0] if has_env else None)
    return w, lr.build_table(w, lam)


# ---------------------------------------------------------------- 1. weights and table
@pytest.mark.parametrize("case", ["12", "48", "50", "281+env"])
def test_weights_and_table_equal_the_restatement(tmp_path, case):
    """write_table_scene with 12 lights, 48 (the LDS table exactly full), 50 (one emitter past it) and 281
    with the environment light, whose weight comes from the loaded texels and the root box."""
    ll = table_limits()[1]
    assert ll == 48
    n_em, env = {"12": (6, False), "48": (24, False), "50": (25, False), "281+env": (140, True)}[case]
    s = loadScene(write_table_scene(tmp_path / "t", n_em, 4, envmap=env), width=32, height=24)
    assert len(s.lights) == 2 * n_em + (1 if env else 0) and ((np.array(s.lights) == -1).sum() == 1) == env
    rt = RayTracer(s)
    assert rt.light_sampling() == {"mode": "uniform", "uniform_share": 0.125} and rt.light_table() is None
    rt.set_light_sampling("power")
    assert rt.light_sampling() == {"mode": "power", "uniform_share": 0.125}
    t = rt.light_table()
    w, want = restated_table(s, rt)
    assert (w > 0).all()
    assert np.array_equal(t["weights"].view(np.uint64), w.view(np.uint64)), (t["weights"], w)
    assert np.array_equal(t["entries"], want["entries"]), int((t["entries"] != want["entries"]).any(1).sum())
    assert t["build_ms"] > 0
    if env:  # the environment's weight is of the area lights' order, not 0 and not everything
        e = int(np.flatnonzero(np.array(s.lights) == -1)[0])
        assert 1e-3 < w[e] / w.sum() < 0.999, w[e] / w.sum()
    rt.set_light_sampling("power", 0.5)  # another share: rebuilt
    w2, want2 = restated_table(s, rt, 0.5)
    assert np.array_equal(rt.light_table()["entries"], want2["entries"])
    assert not np.array_equal(want2["entries"], want["entries"])
    rt.set_light_sampling("uniform")
    assert rt.light_table() is None


# ---------------------------------------------------------------- 2. the probe
@pytest.mark.parametrize("n_em", [6, 25])
def test_probe_equals_the_restatement(tmp_path, n_em):
    s = loadScene(write_table_scene(tmp_path / "t", n_em, 4), width=32, height=24)
    rt = RayTracer(s)
    with pytest.raises(NativeError):
        rt.light_picks(np.zeros(1, np.uint32), np.zeros(1, F))  # no active table
    rt.set_light_sampling("power")
    ent = rt.light_table()["entries"]
    n = len(ent)
    rng = np.random.default_rng(3)
    r0 = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    d1 = (rng.integers(0, 2 ** 24, 4096).astype(F) * F(2.0 ** -24)).astype(F)
    top = F(1.0 - 2.0 ** -24)
    prob = ent[:, 0].copy().view(F)
    first = np.array([-(-(k << 32) // n) for k in range(n)], np.uint64).astype(np.uint32)  # the first r0 of entry k
    below = np.nextafter(prob, F(-1.0)).astype(F)
    r0 = np.concatenate([r0, np.zeros(2, np.uint32), np.full(2, 2 ** 32 - 1, np.uint32), first, first])
    d1 = np.concatenate([d1, [F(0), top], [F(0), top], prob, below]).astype(F)
    li, pmf = rt.light_picks(r0, d1)
    rli, rpmf = lr.pick(ent, r0, d1)
    assert np.array_equal(li, rli.astype(np.int32))
    assert_same_bits(pmf, rpmf, "pmf")
    assert (li >= 0).all() and (li < n).all() and (pmf > 0).all()
    k0 = 4096 + 4
    assert np.array_equal(li[k0:k0 + n], ent[:, 1].astype(np.int32))  # d1 == prob: not kept, the alias
    kept = prob > 0
    assert np.array_equal(li[k0 + n:][kept], np.arange(n, dtype=np.int32)[kept])  # one ulp below: kept
    assert li[4096] == 0 and li[4098] in (n - 1, int(ent[n - 1, 1]))


# ---------------------------------------------------------------- 3. exact films
def film_ref(s, rt, ns, seed, luminance=False):
    """The DIRECT film of ns samples in power mode, rebuilt in numpy as tests/test_env_sampling_gpu.py's
    direct_film_ref does. Per pixel whose camera ray hits a non-emissive surface, the sample-ordered sum
    of f E g / (pmf pdf) over visible samples, from the restated PCG stream (the pick's r0 and d1, then
    Triangle::sample's r1, r2, or the environment branch's two or four draws), the handle's table,
    light_records(), the ALBEDO film for f and the NORMALS film for sn, trace_closest for the hit and
    trace_visible for the shadow ray; per pixel that sees an emitter, its emission per sample.
    Returns (film (H, W, 3), floor-or-cube mask, occluded count, visible count)."""
    W, H = s.width, s.height
    rec = rt.light_records()
    ent = rt.light_table()["entries"]
    kind = rec[:, 7].copy().view(np.int32)
    has_env = (kind == 1).any()
    tex = env_texels(s) if has_env else None
    eent = rt.env_table()["entries"] if luminance else None
    guide = RayTracer(s, seed=seed, integrator="albedo")
    guide.render(1)
    f = guide.film()[0].reshape(-1, 3)
    guide.clear()
    guide.set_integrator("normals")
    guide.render(1)
    sn = guide.film()[0].reshape(-1, 3)
    pix = np.arange(W * H, dtype=np.uint32)
    rays, _ = rt.camera_samples(pix, np.zeros(W * H, np.uint32))
    hits = rt.trace_closest(rays)
    hit = hits[:, 0] < F(3.0e38)
    tri = np.where(hit, hits[:, 1].copy().view(np.int32), 0)
    mat = s.material_index[tri]
    em_of = np.array([m.emission[:] for m in s.materials], F)
    emitter = hit & np.isin(tri, np.array(s.lights)[np.array(s.lights) >= 0])
    surf = hit & ~emitter
    x = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]  # Ray::at
    film = np.zeros((W * H, 3), F)
    n_occ = n_vis = 0
    old = np.seterr(all="ignore")  # (a missed pixel's t = FLT_MAX runs through the arithmetic unused)
    for sl in range(ns):
        st = er.PathStream(pix, np.full(W * H, sl, np.uint32), seed)
        r0 = st.raw()
        d1 = st.next()
        li, pmf = lr.pick(ent, r0, d1)
        L = rec[li]
        a_raw = st.raw()
        a = (a_raw >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
        b = st.next()
        # an area light: Triangle::sample(r1 = a, r2 = b)
        p2 = lr.triangle_sample(L, a, b)
        g, _ = lr.area_geometry(L, p2, x, sn)
        emitted = L[:, 16:19]
        pdf = L[:, 11]
        if has_env:
            if luminance:  # r0 = a's raw step, then d1, d2, d3
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
        lit = surf & (f.sum(1) > 0)  # (a black surface: f = 0, every term +0 whether visible or not)
        n_occ += int((act & ~vis & lit).sum())
        n_vis += int((act & vis & lit).sum())
        c = np.where((act & vis)[:, None], ld, F(0)).astype(F)
        c = np.where(emitter[:, None], em_of[mat], c).astype(F)
        film = film + c
    np.seterr(**old)
    return film.reshape(H, W, 3), surf.reshape(H, W), n_occ, n_vis


def check_cuts(s, rt, want, seed, integrator, env_mode="uniform", cuts="all"):
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
    g.set_light_sampling("power")
    g.render(4)
    assert_same_bits(g.film()[0], want, "two-rank group on device 0 twice")


@pytest.mark.parametrize("size", [(64, 48), (33, 31)])
def test_direct_and_path_films_are_the_restated_sum(tmp_path, size):
    """The "unequal" scene (a white floor, a bright panel, 10 dim rectangles, a black cube; 22 lights, the
    tables in LDS), 4 spp: DIRECT equals the rebuilt sum bit for bit however it is cut, and so does PATH at
    depth 4 (k_shade_pick<false, *, *>): nothing a bounce can reach reflects light (the cube is black, the
    emitters are seen by non-specular bounces, which may not collect emission, and a miss is black), so
    every later term is thr * 0 = +0."""
    s = loadScene(write_unequal_scene(tmp_path / "u", *size))
    W, H = size
    assert len(s.lights) == 22 and s.desc.env_texture < 0
    rt = RayTracer(s, seed=77, integrator="direct")
    rt.set_light_sampling("power")
    want, surf, n_occ, n_vis = film_ref(s, rt, 4, 77)
    print("surface pixels %d of %d, occluded samples %d, visible %d" % (surf.sum(), W * H, n_occ, n_vis))
    assert surf.sum() > 0.3 * W * H and n_occ > 0 and n_vis > 0 and (want[~surf] == 0).all()
    check_cuts(s, rt, want, 77, "direct", cuts="all" if size == (64, 48) else "one")
    pt = RayTracer(s, seed=77, integrator="path", max_depth=4)
    pt.set_light_sampling("power")
    check_cuts(s, pt, want, 77, "path", cuts="all" if size == (64, 48) else "one")
    un = RayTracer(s, seed=77, integrator="direct")
    un.render(4)
    assert not np.array_equal(bits(un.film()[0]), bits(want))  # other draws: another film


# ---------------------------------------------------------------- 4. both modes together
@pytest.mark.parametrize("n_em,luminance", [(4, True), (4, False), (26, True)])
def test_direct_film_with_the_environment_in_the_light_list(tmp_path, n_em, luminance):
    """The floor under n_em emitter rectangles and a smooth 16 x 8 environment map that is in the light
    list: 9 lights (tables in LDS) and 53 (global memory), with the environment sampled through its
    luminance table (k_shade_pick<*, *, true>) or uniformly."""
    s = loadScene(write_emitters_env_scene(tmp_path / "e", smooth_map(16, 8), n_em))
    assert len(s.lights) == 2 * n_em + 1 and (np.array(s.lights) == -1).sum() == 1
    assert (len(s.lights) <= table_limits()[1]) == (n_em == 4)
    mode = "luminance" if luminance else "uniform"
    rt = RayTracer(s, seed=78, integrator="direct")
    rt.set_env_sampling(mode)
    rt.set_light_sampling("power")
    assert (rt.env_table() is not None) == luminance
    w, t = restated_table(s, rt)
    assert np.array_equal(rt.light_table()["entries"], t["entries"])
    want, surf, n_occ, n_vis = film_ref(s, rt, 4, 78, luminance)
    li = lr.pick(t["entries"], np.arange(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32), np.zeros(4096, F))[0]
    assert (np.array(s.lights)[li] == -1).any() and (np.array(s.lights)[li] >= 0).any()  # both kinds get picked
    assert surf.sum() > 0.3 * surf.size and n_vis > 0
    check_cuts(s, rt, want, 78, "direct", mode, cuts="all" if n_em == 4 else "one")


# ---------------------------------------------------------------- 5. statistics
def test_path_means_agree_between_the_modes(tmp_path):
    """PATH on the closed 12-light table scene, depth 4, 32 x 24, 8 seeds x 256 spp per mode: the image-mean
    luminances differ by at most six standard errors of the difference (from the spread across seeds)."""
    s = loadScene(write_table_scene(tmp_path / "t", 6, 4), width=32, height=24)
    assert len(s.lights) == 12
    means = {}
    for mode in ("uniform", "power"):
        rt = RayTracer(s, max_depth=4)
        rt.set_light_sampling(mode)
        assert (rt.light_table() is not None) == (mode == "power")
        m = []
        for k in range(8):
            rt.seed = 2000 + k
            rt.clear()
            rt.render(256)
            f, spp = rt.film()
            m.append(float(er.lum32(f / F(spp)).astype(np.float64).mean()))
        means[mode] = np.array(m)
    mu = {k: v.mean() for k, v in means.items()}
    se = {k: v.std(ddof=1) / np.sqrt(len(v)) for k, v in means.items()}
    print("means %r, standard errors %r" % (mu, se))
    assert se["uniform"] <= 0.05 * mu["uniform"] and se["power"] <= 0.05 * mu["power"]
    assert abs(mu["uniform"] - mu["power"]) <= 6 * np.sqrt(se["uniform"] ** 2 + se["power"] ** 2)


def test_power_mode_is_less_noisy_on_unequal_lights(tmp_path):
    """The "unequal" scene, DIRECT, 64 x 48, 8 seeds x 64 spp per mode: the across-seed variance of a
    pixel's luminance, added over the surface pixels, is lower in power mode by at least half the
    per-sample variance ratio of the numpy restatement at one unoccluded floor point
    (tests/test_light_sampling.py: 76.3 there, so at least 38.1 here; halved because eight seeds scatter
    and because the film also holds the cube's penumbra, where visibility adds noise the pick cannot
    remove). Measured on an MI355X: 12.10 against 0.270, a ratio of 44.9. The image means agree within six
    standard errors."""
    u, p, _ = unequal_variance_ratio(tmp_path)
    cpu_ratio = u.var(ddof=1) / p.var(ddof=1)
    s = loadScene(write_unequal_scene(tmp_path / "u"))
    nrm = RayTracer(s, integrator="normals")
    nrm.render(1)
    surf = nrm.film()[0].sum(2) > 0
    lum = {}
    for mode in ("uniform", "power"):
        rt = RayTracer(s, integrator="direct")
        rt.set_light_sampling(mode)
        per_seed = []
        for k in range(8):
            rt.seed = 3000 + k
            rt.clear()
            rt.render(64)
            f, spp = rt.film()
            per_seed.append(er.lum32(f / F(spp)).astype(np.float64))
        lum[mode] = np.stack(per_seed)
    var = {k: float(v.var(axis=0, ddof=1)[surf].sum()) for k, v in lum.items()}
    means = {k: v.reshape(8, -1).mean(1) for k, v in lum.items()}
    se = {k: v.std(ddof=1) / np.sqrt(8) for k, v in means.items()}
    gpu_ratio = var["uniform"] / var["power"]
    print("CPU per-sample variance ratio %.3f; GPU summed across-seed variances %r, ratio %.3f; means %r"
          % (cpu_ratio, var, gpu_ratio, {k: v.mean() for k, v in means.items()}))
    assert abs(means["uniform"].mean() - means["power"].mean()) <= 6 * np.sqrt(se["uniform"] ** 2 + se["power"] ** 2)
    assert gpu_ratio >= 0.5 * cpu_ratio


# ---------------------------------------------------------------- 6. fall-backs and scope
def test_one_light_keeps_todays_film(tmp_path):
    """materialball-small (the environment is the only light) and a scene lit by one emissive triangle: power
    mode is accepted, no table is reported, and the film is the default's bit for bit."""
    for what, s in (("materialball-small", loadScene(os.path.join(SCENES, "materialball-small"), width=32, height=24)),
                    ("one triangle", loadScene(write_one_triangle_scene(tmp_path / "o")))):
        assert len(s.lights) == 1
        films = []
        for mode in ("uniform", "power"):
            rt = RayTracer(s, seed=1234)
            rt.set_light_sampling(mode)
            assert rt.light_sampling()["mode"] == mode and rt.light_table() is None
            rt.render(3)
            films.append(rt.film()[0])
        assert (films[0] != 0).sum() > 100
        assert_same_bits(films[1], films[0], what)


def test_what_the_mode_must_leave_alone(tmp_path):
    """With a table active: ALBEDO and NORMALS films equal the default's; so do rtg_render_light's and
    rtg_render_instant_radiosity's on cornell-box."""
    s = loadScene(write_unequal_scene(tmp_path / "u"))
    for integrator in ("albedo", "normals"):
        films = []
        for mode in ("uniform", "power"):
            rt = RayTracer(s, seed=7, integrator=integrator)
            rt.set_light_sampling(mode)
            assert (rt.light_table() is not None) == (mode == "power")
            rt.render(2)
            films.append(rt.film()[0])
        assert_same_bits(films[1], films[0], integrator)
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=64, height=48)
    for what in ("light tracer", "instant radiosity"):
        films = []
        for mode in ("uniform", "power"):
            rt = RayTracer(s, seed=5, max_paths=64 * 48 * 7)
            rt.set_light_sampling(mode)
            assert (rt.light_table() is not None) == (mode == "power")
            if what == "light tracer":
                rt.lightTracer(2, first_frame=0)
            else:
                rt.instantRadiosity(2, n_vpl=20, first_frame=0)
            films.append(rt.film()[0])
        assert (films[0] != 0).sum() > 100
        assert_same_bits(films[1], films[0], what)


def test_argument_errors_keep_the_previous_setting(tmp_path):
    s = loadScene(write_unequal_scene(tmp_path / "u", 33, 31))
    rt = RayTracer(s, seed=9, integrator="direct")
    rt.set_light_sampling("power", 0.25)
    rt.render(2)
    want = rt.film()[0]
    ent = rt.light_table()["entries"]
    for bad in ((2, 0.25), (-1, 0.25), ("power", -0.01), ("power", 1.5), ("power", float("nan"))):
        with pytest.raises(NativeError):
            rt.set_light_sampling(*bad)
        assert rt.light_sampling() == {"mode": "power", "uniform_share": 0.25}
        assert np.array_equal(rt.light_table()["entries"], ent)
    with pytest.raises(ValueError):
        rt.set_light_sampling("luminance")
    rt.clear()
    rt.render(2)
    assert_same_bits(rt.film()[0], want, "after the rejected settings")
    g = RayTracerGroup(s, devices=(0, 0))
    with pytest.raises(NativeError):
        g.set_light_sampling(7)
    with pytest.raises(NativeError):
        g.set_light_sampling("power", 2.0)
    p = N.rtg_light_sampling()
    assert N.rtg().rtg_get_light_sampling(g._lib.rtg_group_handle(g._g, 1), C.byref(p)) == 0
    assert p.mode == N.RTG_LIGHTS_UNIFORM


def test_cli_light_sampling_writes_the_library_film(tmp_path):
    """-lightSampling power on the "unequal" scene: the file is Film::save of the library's power-mode
    film; without the option the file is another; an unknown name is an error."""
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = write_unequal_scene(tmp_path / "u")
    s = loadScene(scene)
    rt = RayTracer(s, seed=1234)
    rt.set_light_sampling("power", 0.25)
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.film()[0], 3)
    base = [cli, "-scene", scene, "-SPP", "3", "-timeLimit", "0", "-outputFilename", "out.hdr"]
    out = {}
    for d, extra in (("power", ["-lightSampling", "power", "-lightUniformShare", "0.25"]), ("uniform", []),
                     ("group", ["-lightSampling", "power", "-lightUniformShare", "0.25", "-devices", "0,0"])):
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[d] = (tmp_path / d / "out.hdr").read_bytes()
    assert out["power"] == (tmp_path / "lib.hdr").read_bytes()
    assert out["group"] == out["power"]
    assert out["uniform"] != out["power"]
    r = subprocess.run(base + ["-lightSampling", "area"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "lightSampling" in r.stderr
