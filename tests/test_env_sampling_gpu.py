"""Environment light sampling on the GPU (rtg_set_env_sampling, RTG_ENV_LUMINANCE): the handle's alias
table and the kernel's sampling function against the numpy restatement (tests/env_sampling_ref.py) bit
for bit, a DIRECT film rebuilt sample by sample, the fall-backs that must leave today's films alone,
and the two modes' agreement in expectation (with less noise in the new one)."""
import ctypes as C
import os

import numpy as np
import pytest

import env_sampling_ref as er
from conftest import SCENES
from env_scenes import patch_map, smooth_map, spot_map, write_floor_scene, write_table_scene_with_map
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, probe_texture
from raytracingrenderer_amd import _native as N
from test_env_sampling import check_invariant, env_maps, scripted_draws

pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(1e-4)  # RTG_EPS


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def env_texels(scene):
    """The environment texture as loaded (the test's map after its RGBE round trip)."""
    return scene.texture(scene.desc.env_texture).copy()


@pytest.fixture(scope="module")
def floor_scenes(tmp_path_factory):
    """{name: Scene}: the floor under each 64 x 32 map of test_env_sampling.env_maps, a smooth 16 x 8
    map (32 x 24 and 64 x 24 films) and the spot map."""
    out = {}
    for name, m in env_maps(64, 32).items():
        out[name] = loadScene(write_floor_scene(tmp_path_factory.mktemp(name), m))
    out["smooth"] = loadScene(write_floor_scene(tmp_path_factory.mktemp("smooth"), smooth_map(16, 8)))
    out["smooth-wide"] = loadScene(write_floor_scene(tmp_path_factory.mktemp("smoothw"), smooth_map(16, 8), 64, 24))
    out["spot"] = loadScene(write_floor_scene(tmp_path_factory.mktemp("spot"), spot_map()))
    for s in out.values():
        assert list(s.lights) == [-1] and s.desc.n_tris == 2  # the environment is the only light
    return out


# ---------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("name", ["positive", "zeros", "one-hot"])
def test_table_equals_the_restatement(floor_scenes, name):
    """env_table() of a 64 x 32 map: the weights (k_env_weights' footprint maxima times the row's sin)
    and every entry equal the restatement's bit for bit, and the table returns each cell with its
    weight: to 1e-12 for the binary64 keep probabilities (the restated builder's, which the entries
    are the float32 rounding of), hence to 2^-25 / N per entry naming the cell for the float32 ones."""
    s = floor_scenes[name]
    tex = env_texels(s)
    assert tex.shape == (32, 64, 3)
    rt = RayTracer(s)
    assert rt.env_sampling() == "uniform" and rt.env_table() is None
    rt.set_env_sampling("luminance")
    assert rt.env_sampling() == "luminance"
    t = rt.env_table()
    wt = er.cell_weights(tex)
    assert np.array_equal(t["weights"].view(np.uint64), wt.view(np.uint64))
    al = er.build_alias(wt)
    check_invariant(al["prob"], al["alias"], wt, 1e-12)
    want = er.table_entries(al)
    assert np.array_equal(t["entries"], want), int((t["entries"] != want).any(1).sum())
    assert_same_bits(t["cellpdf_self"].reshape(-1), al["cellpdf"], "cellpdf_self")
    assert_same_bits(t["cellpdf_alias"].reshape(-1), al["cellpdf"][al["alias"]], "cellpdf_alias")
    n = 64 * 32
    named = 1 + np.bincount(t["alias"].reshape(-1), minlength=n)
    pf = t["prob"].reshape(-1).astype(np.float64)
    w1 = wt.reshape(-1)
    err = np.abs(er.alias_mass(pf, t["alias"]) - w1 / np.cumsum(w1)[-1])
    assert (err <= 1e-12 + named * 2.0 ** -25 / n).all(), float(err.max())
    assert (pf[w1 == 0] == 0).all() and t["build_ms"] > 0
    rt.set_env_sampling("uniform")
    assert rt.env_table() is None


# ---------------------------------------------------------------- 2. the probe
@pytest.mark.parametrize("name", ["positive", "zeros", "one-hot"])
def test_probe_equals_the_restatement(floor_scenes, name):
    s = floor_scenes[name]
    w, h = 64, 32
    rt = RayTracer(s)
    rt.set_env_sampling("luminance")
    ent = rt.env_table()["entries"]
    r0, d = scripted_draws(4096, 21)
    top = F(1.0 - 2.0 ** -24)
    corners = [(r, (a, b, c)) for r in (0, 2 ** 32 - 1) for a in (0.0, top) for b in (0.0, top) for c in (0.0, top)]
    # the polar rows, where sin theta is smallest: the first r0 of a few cells of rows 0 and h - 1, kept
    # (d1 = 0) or not (d1 = top), at v = cy / h exactly (theta = 0 in row 0: rejected), one step off and at the far edge
    n = w * h
    pole = [(-(-(k << 32) // n), (d1, d2, d3)) for k in (0, 1, w - 1, n - w, n - 2, n - 1)
            for d1 in (0.0, top) for d2 in (0.0, 0.5) for d3 in (0.0, F(2.0 ** -24), top)]
    r0 = np.concatenate([r0, np.array([c[0] for c in corners + pole], np.uint64).astype(np.uint32)])
    d = np.concatenate([d, np.array([c[1] for c in corners + pole], F)])
    wi, pdf = rt.env_samples(r0, d)
    rwi, rpdf, cell = er.sample(ent, w, h, r0, d)
    assert_same_bits(wi, rwi, name + ": wi")
    assert_same_bits(pdf, rpdf, name + ": pdf")
    assert (pdf[:4096] > 0).mean() > 0.99 and np.isfinite(pdf).all()
    if name == "positive":  # the kept row-0 cells at v = 0: sin theta = 0, rejected
        k0 = 4096 + len(corners)
        assert (cell[k0:] // w == 0).any() and (pdf[k0:][(d[k0:, 2] == 0) & (cell[k0:] // w == 0)] == 0).all()


# ---------------------------------------------------------------- 3. an exact film
def direct_film_ref(s, rt, ns, seed):
    """The DIRECT film of ns samples of a floor scene in luminance mode, rebuilt in numpy. Per pixel
    whose camera ray hits the floor, the sample-ordered sum of f E(wi) g / pdf (pmf = 1: one light; g =
    max(wi . sn, 0), wi.y up to the floor normal's last bits), from the restated PCG stream (the
    light-pick draw, then r0, d1, d2, d3), env_sampling_ref.sample on the handle's table,
    probe_texture(env=True) for E, the ALBEDO film for f = BSDF::evaluate = divs_pi(alb) and the
    NORMALS film for sn (k_shade's own values of both), and the shadow ray's any-hit query
    (trace_visible on the restated ray: the floor occludes nothing above it, up to a grazing ray that
    starts a rounding error below it). Returns (film (H, W, 3), hit mask (H, W))."""
    W, H = s.width, s.height
    tex = env_texels(s)
    ent = rt.env_table()["entries"]
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
    assert (hit == (sn.sum(1) > 0)).all() and (sn[hit, 1] > F(0.99)).all()
    x = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]  # Ray::at
    film = np.zeros((W * H, 3), F)
    th, tw = tex.shape[:2]
    old = np.seterr(all="ignore")  # (a missed pixel's t = FLT_MAX runs through the arithmetic unused)
    for sl in range(ns):
        st = er.PathStream(pix, np.full(W * H, sl, np.uint32), seed)
        st.next()  # the light pick: (int)(1 * u) = 0
        r0 = st.raw()
        d = np.stack([st.next(), st.next(), st.next()], axis=1)
        wi, pdf, _ = er.sample(ent, tw, th, r0, d)
        g = ((wi[:, 0] * sn[:, 0]) + (wi[:, 1] * sn[:, 1])) + (wi[:, 2] * sn[:, 2])
        g = np.where(g > 0, g, F(0)).astype(F)
        act = hit & (pdf > 0) & (g > 0)
        E = probe_texture(tex, wi, env=True)
        ld = (((f * E) * g[:, None]) / pdf[:, None]).astype(F)
        # Scene::visible(x, x + wi * 10000)
        sd = (x + wi * F(10000.0)) - x
        l2 = ((sd[:, 0] * sd[:, 0]) + (sd[:, 1] * sd[:, 1])) + (sd[:, 2] * sd[:, 2])
        maxt = np.sqrt(l2) - (F(2.0) * EPS)
        sd = sd * (F(1) / np.sqrt(l2))[:, None]
        so = x + sd * EPS
        q = np.zeros((W * H, 8), F)
        q[:, 0:3], q[:, 3], q[:, 4:7] = so, maxt, sd
        q[~act] = (0, 1e6, 0, 1, 0, 1, 0, 0)  # (unused lanes: a ray far above everything)
        vis = rt.trace_visible(q) != 0
        c = np.where((act & vis)[:, None], ld, F(0)).astype(F)
        film = film + c
    np.seterr(**old)
    return film.reshape(H, W, 3), hit.reshape(H, W)


@pytest.mark.parametrize("name", ["smooth", "smooth-wide"])
def test_direct_film_is_the_restated_sum_however_it_is_cut(floor_scenes, name):
    """4 spp of DIRECT under a smooth positive 16 x 8 map: every floor-hit pixel equals the rebuilt sum
    bit for bit, from one call, four 1-spp calls, queued frames, two complementary tile sets and a
    two-rank group on device 0 twice (the 64 x 24 film has two tiles, one per rank; the 32 x 24 film's
    single tile leaves the second set and the second rank empty)."""
    s = floor_scenes[name]
    W, H = s.width, s.height
    rt = RayTracer(s, seed=77, integrator="direct")
    rt.set_env_sampling("luminance")
    want, hit = direct_film_ref(s, rt, 4, 77)
    assert hit.sum() > 0.3 * W * H and (want[hit].sum(1) > 0).mean() > 0.8 and (want[~hit] == 0).all()
    rt.render(4)
    assert_same_bits(rt.film()[0], want, "one call")
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
    g = RayTracerGroup(s, devices=(0, 0), seed=77)
    for r in range(2):  # (the group has no integrator setting of its own: through each rank's handle)
        assert g._lib.rtg_set_integrator(g._lib.rtg_group_handle(g._g, r), N.RTG_INTEGRATOR_DIRECT) == 0
    g.set_env_sampling("luminance")
    g.render(4)
    assert_same_bits(g.film()[0], want, "two-rank group on device 0 twice")


# ---------------------------------------------------------------- 4. fall-backs change nothing
def test_nothing_to_sample_keeps_todays_films(tmp_path):
    """luminance mode with a black environment map (area emitters, depth 4) and without an environment
    light (cornell-box) gives the uniform mode's film, which is the oracle's; and a handle that had a
    table renders the oracle's film again once set back to uniform."""
    black = np.zeros((32, 64, 3), F)
    s = loadScene(write_table_scene_with_map(tmp_path / "black", black, 6, 4), width=32, height=24)
    # (the loader leaves a black map out of the light list: the 12 emitter triangles remain)
    assert -1 not in list(s.lights) and len(s.lights) == 12 and s.desc.env_texture >= 0
    # the same scene with the environment light in the list and its map black: a map with light, its
    # texels zeroed in the loaded scene (the weights then sum to 0: no table)
    z = loadScene(write_table_scene_with_map(tmp_path / "zeroed", patch_map(), 6, 4), width=32, height=24)
    z.texture(z.desc.env_texture)[:] = 0
    assert list(z.lights).count(-1) == 1 and len(z.lights) == 13
    for what, sc in (("black map", s), ("zeroed map", z)):
        want, _ = Oracle(sc, 4, "rtm").render(3, seed=1234, threads=8)
        for mode in ("uniform", "luminance"):
            rt = RayTracer(sc, seed=1234, max_depth=4)
            rt.set_env_sampling(mode)
            assert rt.env_sampling() == mode and rt.env_table() is None
            rt.render(3)
            assert_same_bits(rt.film()[0], want, "%s, %s" % (what, mode))
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=32, height=24)
    want, _ = Oracle(s, 4, "rtm").render(3, seed=1234, threads=8)
    rt = RayTracer(s, seed=1234)
    rt.set_env_sampling("luminance")
    assert rt.env_table() is None
    rt.render(3)
    assert_same_bits(rt.film()[0], want, "no environment light, luminance")
    s = loadScene(os.path.join(SCENES, "materialball-small"), width=32, height=24)
    want, _ = Oracle(s, 4, "rtm").render(3, seed=1234, threads=8)
    rt = RayTracer(s, seed=1234)
    rt.set_env_sampling("luminance")
    assert rt.env_table() is not None
    rt.render(3)
    assert not np.array_equal(bits(rt.film()[0]), bits(want))  # other draws: another film
    rt.clear()
    rt.set_env_sampling("uniform")
    rt.render(3)
    assert_same_bits(rt.film()[0], want, "back to uniform after a table")


# ---------------------------------------------------------------- 5. it samples the light
def test_a_small_bright_spot_is_found_by_every_sample(floor_scenes):
    """A 64 x 32 map black but for four texels of 1000: all density lies in the nine supporting cells,
    above the horizon, so 1 spp of DIRECT in luminance mode lights every floor-hit pixel, while the
    uniform mode lights under 5 % of them (the support is about 0.5 % of the sphere; the CPU oracle's
    uniform film at seed 1234: 3 of 508 floor-hit pixels)."""
    s = floor_scenes["spot"]
    tex = env_texels(s)
    assert set(np.unique(tex)) == {0.0, 1000.0} and (tex[8:10, 20:22] == 1000).all() and (tex > 0).sum() == 12
    nrm = RayTracer(s, integrator="normals")
    nrm.render(1)
    hit = nrm.film()[0].sum(2) > 0
    assert hit.sum() > 0.4 * hit.size
    lit = {}
    for mode in ("uniform", "luminance"):
        rt = RayTracer(s, seed=1234, integrator="direct")
        rt.set_env_sampling(mode)
        rt.render(1)
        f = rt.film()[0]
        assert (f[~hit] == 0).all()
        lit[mode] = int(((f.sum(2) > 0) & hit).sum())
    print("floor-hit pixels %d, lit: %r" % (hit.sum(), lit))
    t = rt.env_table()
    assert {(int(x), int(y)) for y, x in np.argwhere(t["weights"] > 0)} == {(x, y) for x in (19, 20, 21) for y in (7, 8, 9)}
    assert lit["luminance"] == hit.sum()
    assert lit["uniform"] < 0.05 * hit.sum()


# ---------------------------------------------------------------- 6. the same expectation, with occlusion
def test_both_modes_agree_in_expectation_and_luminance_is_less_noisy(tmp_path):
    """The table scene (cornell-mat's walls and cubes, 6 emitters, the environment seen through the
    open front) under a smooth 64 x 32 map with a patch 50 times brighter: PATH at depth 4, 32 x 24,
    8 seeds x 256 spp per mode. The image-mean luminances differ by at most six standard errors of
    the difference (from the spread across seeds), neither standard error exceeds 5 % of its mean
    (uniform side on the CPU oracle, same seeds: 0.8 %), and the spread across seeds is smaller in
    luminance mode. (The exact comparison of luminance-mode PATH films, bit for bit against the C oracle,
    lives in tests/test_sampling_modes_gpu.py; this test keeps the two modes' agreement and the gain.)"""
    s = loadScene(write_table_scene_with_map(tmp_path / "patch", patch_map(), 6, 4), width=32, height=24)
    assert (np.array(s.lights) == -1).sum() == 1 and len(s.lights) == 13
    means = {}
    for mode in ("uniform", "luminance"):
        rt = RayTracer(s, max_depth=4)
        rt.set_env_sampling(mode)
        assert (rt.env_table() is not None) == (mode == "luminance")
        m = []
        for k in range(8):
            rt.seed = 1000 + k
            rt.clear()
            rt.render(256)
            f, spp = rt.film()
            m.append(float(er.lum32(f / F(spp)).astype(np.float64).mean()))
        means[mode] = np.array(m)
    mu = {k: v.mean() for k, v in means.items()}
    se = {k: v.std(ddof=1) / np.sqrt(len(v)) for k, v in means.items()}
    print("means %r, standard errors %r, variances %r" % (mu, se, {k: v.var(ddof=1) for k, v in means.items()}))
    assert se["uniform"] <= 0.05 * mu["uniform"] and se["luminance"] <= 0.05 * mu["luminance"]
    assert abs(mu["uniform"] - mu["luminance"]) <= 6 * np.sqrt(se["uniform"] ** 2 + se["luminance"] ** 2)
    assert means["luminance"].var(ddof=1) < means["uniform"].var(ddof=1)


# ---------------------------------------------------------------- 7. arguments
def test_argument_errors_keep_the_previous_setting(floor_scenes):
    s = floor_scenes["smooth"]
    rt = RayTracer(s)
    rt.set_env_sampling("luminance")
    for bad in (2, -1, 1000):
        with pytest.raises(NativeError):
            rt.set_env_sampling(bad)
        assert rt.env_sampling() == "luminance" and rt.env_table() is not None
    with pytest.raises(ValueError):
        rt.set_env_sampling("cosine")
    g = RayTracerGroup(s, devices=(0, 0))
    with pytest.raises(NativeError):
        g.set_env_sampling(7)
    lib = N.rtg()
    # the setter's size check alone (no map of that size is uploaded): more than 2^24 texels
    assert lib.rtg_env_sampling_check(N.RTG_ENV_LUMINANCE, 8192, 4096) == -1
    assert b"2^24" in lib.rtg_last_error()
    assert lib.rtg_env_sampling_check(N.RTG_ENV_LUMINANCE, 4096, 4096) == 0
    rt.set_env_sampling("uniform")
    with pytest.raises(NativeError):
        rt.env_samples(np.zeros(1, np.uint32), np.zeros((1, 3), F))  # no active table
    m = C.c_int(-5)
    assert lib.rtg_get_env_sampling(rt.handle, C.byref(m)) == 0 and m.value == N.RTG_ENV_UNIFORM
