"""The C oracle's light pick, light grid and Sobol sampler (or_set_light_table, or_set_light_grid,
or_set_sampler), CPU side: the pick events of whole small films against the numpy restatements
(tests/light_sampling_ref.py, tests/light_grid_ref.py) on the restated draws, the Sobol draws and camera
rays against tests/sobol_ref.py and the header's check values, the draw counter's rounding, the modes
against each other in expectation, and the defaults, which must stay today's films. The tables are inputs
of the oracle: they come from the restatements on records built from the loaded scene, never from a device."""
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

import camera_ref as cr
import env_sampling_ref as er
import light_grid_ref as gr
import light_sampling_ref as lr
import sobol_ref as sr
from conftest import SCENES
from light_grid_scenes import write_room_scene
from oracle.pyoracle import Oracle, lib
from raytracingrenderer_amd import loadScene
from test_light_sampling import scene_light_records
from test_oracle_sampling import INTEGRATORS, LENS, bits, luminance_table

F = np.float32
U32 = np.uint32
LAM = 0.125


def light_records(scene):
    """(n, 20) float32 records of the scene's light list: scene_light_records' for the emissive triangles
    and, for the environment light (-1 in the list), a record of type 1."""
    lights = np.array(scene.lights)
    rec = np.zeros((len(lights), 20), F)
    area = np.flatnonzero(lights >= 0)
    sub = SimpleNamespace(positions=scene.positions, materials=scene.materials, material_index=scene.material_index,
                          lights=[int(t) for t in lights[area]])  # the area lights alone in the list
    rec[area] = scene_light_records(sub)
    rec[lights < 0, 7] = np.array([1], np.int32).view(F)[0]
    return rec


def power_table(scene, lam=LAM):
    """The restated RTG_LIGHTS_POWER table of a loaded scene: (weights, entries (n, 4) uint32)."""
    has_env = (np.array(scene.lights) == -1).any()
    tex = scene.texture(scene.desc.env_texture).copy() if has_env else None
    w = lr.light_weights(light_records(scene), tex, scene.node_bounds[0] if has_env else None)
    t = lr.build_table(w, lam)
    assert t is not None
    return w, t["entries"]


def grid_tables(scene, cells, lam=LAM):
    """The restated grid of a loaded scene (light_grid_ref.build's dictionary)."""
    w, _ = power_table(scene, lam)
    return gr.build(light_records(scene), w, scene.node_bounds[0], cells, lam)


def modes_oracle(scene, depth=4, integrator="path", power=None, grid=None, sobol=False, luminance=None, camera=None,
                 flavour="rtm"):
    """An Oracle under the given modes. power: the table's entries; grid: light_grid_ref.build's dictionary
    (needs power); luminance: test_oracle_sampling.luminance_table's triple; camera: set_camera_sampling's
    keywords."""
    o = Oracle(scene, depth, flavour, integrator=INTEGRATORS[integrator])
    if power is not None:
        o.set_light_table(power)
    if grid is not None:
        o.set_light_grid(grid["entries"], grid["dims"], grid["lo"], grid["scale"])
    if sobol:
        o.set_sampler("sobol")
    if luminance is not None:
        o.set_env_table(*luminance)
    if camera:
        o.set_camera_sampling(**camera)
    return o


def first_hits(o, pix):
    """(hit mask, hit point x (n, 3) float32 as Ray::at forms it, material kind of the hit triangle) of the
    pixel-centre camera rays."""
    rays = o.camera_rays(pix)
    q = np.zeros((len(pix), 8), F)
    q[:, 0:3], q[:, 3], q[:, 4:7] = rays[:, 0:3], F(3.4e38), rays[:, 3:6]
    h = o.trace_closest(q)
    hit = h[:, 0] < F(3e38)
    x = rays[:, 0:3] + rays[:, 3:6] * h[:, 0:1]
    tri = h[:, 1].copy().view(np.int32)
    return hit, x.astype(F), tri


# ---------------------------------------------------------------- the pick
def _scene(name, tmp_path, w=40, h=30):
    if name == "room":
        return loadScene(write_room_scene(tmp_path / "room"), width=w, height=h)
    return loadScene(os.path.join(SCENES, name), width=w, height=h)


@pytest.mark.parametrize("name", ["cornell-mat", "room"])
def test_first_pick_equals_the_restatement(tmp_path, name):
    """Every pixel of a 40 x 30 film, samples 0, 1 and 63: the first pick event {slot, light, pmf, cell} of
    the path equals light_sampling_ref.pick (one table) and light_grid_ref.pick (8 cells on the longest
    axis) on the PathStream draws r0, d1, bit for bit, and the cell equals light_grid_ref.cell_of of the
    restated hit point. A path whose camera ray misses, or hits an emitter, mirror or glass first, picks at
    a later hit or never; those are counted and skipped."""
    s = _scene(name, tmp_path)
    n = s.width * s.height
    w, power = power_table(s)
    grid = grid_tables(s, 8)
    assert int(grid["dims"].prod()) > 8 and not grid["uniform"].all()
    pix = np.arange(n, dtype=U32)
    seed = 4242
    for use_grid in (False, True):
        o = modes_oracle(s, 4, "path", power=power, grid=grid if use_grid else None)
        hit, x, tri = first_hits(o, pix)
        cells = gr.cell_of(x, grid["dims"], grid["lo"], grid["scale"]) if use_grid else np.zeros(n, np.int64)
        checked = other = 0
        for sample in (0, 1, 63):
            smp = np.full(n, sample, U32)
            st = er.PathStream(pix, smp, seed)
            r0, d1 = st.raw(), st.next()
            if use_grid:
                li, pmf = gr.pick(grid["entries"], cells, r0, d1)
            else:
                li, pmf = lr.pick(power, r0, d1)
            k = ((r0.astype(np.uint64) * np.uint64(len(s.lights))) >> np.uint64(32)).astype(np.int64)
            for p in range(n):
                ev, _ = o.path_events(p, sample, seed)
                picks = ev[ev[:, 0] == 7]
                first_shaded = (hit[p] and s.materials[s.material_index[tri[p]]].kind in (0, 1)
                                and not er.lum32(np.array([s.materials[s.material_index[tri[p]]].emission[:]], F))[0] > 0)
                if not first_shaded:
                    other += 1
                    continue
                assert ev[0, 0] == 1 and ev[1, 0] == 7, (p, sample)  # the closest hit, then the pick
                e = picks[0]
                assert (int(e[1]), int(e[2]), int(e[4])) == (int(k[p]), int(li[p]), int(cells[p])), (p, sample, e)
                assert np.array_equal(bits(e[3]), bits(pmf[p])), (p, sample)
                checked += 1
        c = o.mode_counts()
        print(name, "grid" if use_grid else "table", "checked", checked, "other", other, c)
        assert checked > 0.5 * 3 * n and c["picks"] >= checked and c["alias_picks"] >= 1 and c["picks_deep"] >= 1
        if use_grid:
            assert len(np.unique(cells[hit])) >= 3


# ---------------------------------------------------------------- Sobol
def test_sobol_check_values_of_the_header():
    """mix32(5) and the eight draws of samples 0 and 65535 that include/rtg.h lists."""
    L = lib("rtm")
    assert L.or_sobol_mix32(5) == 0x5c45d53e
    out = np.zeros(4, U32)
    L.or_sobol_draws(0x5c45d53e, 0, 0, 4, out.ctypes.data_as(L.or_sobol_draws.argtypes[4]))
    assert [hex(v) for v in out] == ["0xf71b8747", "0x85be176b", "0x3945034a", "0x6243e999"]
    L.or_sobol_draws(0x5c45d53e, 65535, 0, 4, out.ctypes.data_as(L.or_sobol_draws.argtypes[4]))
    assert [hex(v) for v in out] == ["0x73c1d462", "0x9ef285ce", "0x288746e5", "0x5010ac28"]


def test_sobol_draws_and_camera_rays_equal_the_restatement(monkeypatch):
    """The first sixteen raw draws of the path's stream and of the camera's equal sobol_ref.SobolStream for
    every pixel of a 40 x 30 film at samples 0, 1, 63 and 65535 under two seeds; under tent + lens the
    camera rays and film positions equal camera_ref.camera_samples_ref with its four draws replaced by the
    camera stream's (as tests/test_sampler_gpu.py restates them); PCG gives other rays."""
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=40, height=30)
    n = s.width * s.height
    o = modes_oracle(s, 4, "path", sobol=True, camera=dict(filter="tent", filter_radius=1.0, **LENS))
    samples = (0, 1, 63, 65535)
    pix = np.tile(np.arange(n, dtype=U32), len(samples))
    smp = np.repeat(np.array(samples, U32), n)
    for seed in (1234, 0xFEDCBA9876543210):
        for camera in (False, True):
            st = sr.SobolStream(pix, smp, seed, sr.CAMERA_STREAM if camera else 0)
            want = np.stack([st.raw() for _ in range(16)], axis=1)
            for i in range(len(pix)):
                got = o.sampler_draws(int(pix[i]), int(smp[i]), seed, 16, camera=camera)
                assert np.array_equal(got, want[i]), (seed, camera, pix[i], smp[i])
        rays, xy = o.camera_rays(pix, smp, seed=seed)
        st = sr.SobolStream(pix, smp, seed, sr.CAMERA_STREAM)
        u = np.stack([st.next() for _ in range(4)], axis=1)
        monkeypatch.setattr(cr, "camera_draws", lambda p, q, sd, u=u: u)
        want, wxy = cr.camera_samples_ref(s.camera, pix, smp, seed, cr.FILTERS["tent"], 1.0, LENS["lens_radius"],
                                          LENS["focal_distance"])
        assert np.array_equal(bits(xy), bits(wxy))
        assert np.array_equal(bits(rays[:, 0:3]), bits(want[:, 0:3])) and np.array_equal(bits(rays[:, 3:6]), bits(want[:, 4:7]))
        o.set_sampler("pcg")
        pcg, _ = o.camera_rays(pix, smp, seed=seed)
        assert (bits(pcg) != bits(rays)).any(1).mean() > 0.99
        o.set_sampler("sobol")


def test_sobol_counter_rounds_up_when_a_bounce_opens():
    """cornell-mat PATH at depth 8. Every bounce opens on a multiple of four, so the counter the next one
    loads is that multiple plus the bounce's draws: a diffuse bounce takes the pick's 1 (uniform) or 2
    (table), the light sample's 2 (a triangle, the uniform sphere) or 4 (the luminance table), the roulette's
    1 and the BSDF's 2; a mirror 1; glass 1 or 2. That is 6 under the defaults, 7 under the power pick, 9
    under the power pick with a luminance-mode environment sample, and 8, the one multiple of four, under
    the uniform pick with one. The Sobol bounce events show all four residues: loaded 1, 2 and 3 past a
    multiple and rounded up to the next, and loaded at a multiple and left there; the multiples come from
    the uniform pick under luminance mode alone. Every event's rounded value is (loaded + 3) & ~3."""
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=40, height=30)
    _, power = power_table(s)
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    lum = luminance_table(s)
    for kw in (dict(), dict(power=power), dict(power=power, luminance=lum), dict(luminance=lum)):
        o = modes_oracle(s, 8, "path", sobol=True, **kw)
        for p in range(0, s.width * s.height, 3):
            ev, _ = o.path_events(p, 2, 77)
            b = ev[ev[:, 0] == 8]
            for e in b:
                loaded, after = int(e[1]), int(e[2])
                assert after == (loaded + 3) & ~3 and e[3] >= 1
                seen[loaded & 3] += 1
        c = o.mode_counts()
        assert c["sobol_rounded"] > 0 and c["sobol_max_group"] >= 2
        assert (c["sobol_aligned"] > 0) == (sorted(kw) == ["luminance"]), (sorted(kw), c)
    print("counter loaded at n mod 4:", seen)
    assert all(v >= 1 for v in seen.values()), seen


# ---------------------------------------------------------------- one expectation
SPP = 64
SEEDS_A = [2000 + k for k in range(8)]
SEEDS_B = [3000 + k for k in range(8)]


def _mean_and_se(scene, spp, seeds, **kw):
    """(mean film luminance over all samples of all seeds, its standard error from the oracle's own
    per-sample values: each 1-spp frame's film mean is one value of the estimator, the counters summed)."""
    def one(seed):
        o = modes_oracle(scene, 4, "path", **kw)
        vals = []
        for k in range(spp):
            film, _ = o.render(1, first=k, seed=seed, threads=1)
            vals.append(float(er.lum32(film).astype(np.float64).mean()))
        return vals, o.mode_counts()
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, seeds))
    v = np.array([r[0] for r in res]).reshape(-1)
    counts = {k: sum(r[1][k] for r in res) for k in res[0][1]}
    return v.mean(), v.std(ddof=1) / np.sqrt(len(v)), counts


def test_the_modes_agree_in_expectation():
    """cornell-mat (reflecting walls, a mirror and a glass object, textures; two area lights and the
    environment, whose power weights are 1.1, 1.1 and 32.8) at 32 x 24, PATH depth 4: the film-mean radiance
    under the uniform pick, the power pick, the grid (4 cells) and Sobol (under the uniform and the power
    pick) agree. The power table is far from uniform (pmf 0.86 for the environment, 0.07 for each triangle,
    both triangles' slots aliased), and the grid's 64 tables differ from it and among themselves, so a pmf
    used wrongly past the camera hit moves the mean: the counters assert alias picks, picks and non-zero NEE
    samples at depth >= 1, and picks in other cells than the camera hit's. Each mode's standard error comes
    from its own per-sample film means, 8 seeds x 64 samples = 512 values; two modes differ by less than 5
    pooled standard errors. The count, 64 spp, was fixed on the CPU on this scene: with it uniform against
    uniform across the two seed lists passes with that margin (measured 0.08 pooled standard errors apart;
    32 spp gave 0.87), the standard error is 0.2 % of the mean, so 5 pooled ones resolve a bias of 1.4 %
    (taking the table's pmf for 1 / n at depth >= 1 moves the mean by 6 %), and the test takes 1.4 s.
    Measured against uniform: power 0.02, grid 0.68, Sobol 0.09; power against grid 0.81, against power under Sobol 0.71. Sobol's per-sample
    values of one pixel are stratified against each other, so its standard error computed this way is an
    upper bound."""
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=32, height=24)
    _, power = power_table(s)
    grid = grid_tables(s, 4)
    pmf = power[:, 2].copy().view(F)
    assert pmf.max() > 0.8 and pmf.min() < 0.1 and (power[:, 1] != np.arange(len(power))).any()
    assert not any(np.array_equal(e, power) for e in grid["entries"])
    assert len({e.tobytes() for e in grid["entries"]}) >= 8
    got = {"uniform": _mean_and_se(s, SPP, SEEDS_A), "uniform-b": _mean_and_se(s, SPP, SEEDS_B),
           "power": _mean_and_se(s, SPP, SEEDS_A, power=power),
           "grid": _mean_and_se(s, SPP, SEEDS_A, power=power, grid=grid),
           "sobol": _mean_and_se(s, SPP, SEEDS_A, sobol=True),
           "power+sobol": _mean_and_se(s, SPP, SEEDS_A, power=power, sobol=True)}
    for k, v in got.items():
        print(k, v)
    mu, se, c = got["uniform"]
    assert 0 < se < 0.005 * mu and c["picks"] == 0
    for k in ("power", "grid", "power+sobol"):
        c = got[k][2]
        assert c["alias_picks"] >= 1000 and c["picks_deep"] >= 1000 and c["nee_deep"] >= 1000, (k, c)
    assert got["grid"][2]["other_cell"] >= 1000 and got["grid"][2]["other_cells_distinct"] >= 8
    assert got["sobol"][2]["sobol_rounded"] >= 1000
    for a, b in (("uniform", "uniform-b"), ("uniform", "power"), ("uniform", "grid"), ("power", "grid"), ("uniform", "sobol"),
                 ("power", "power+sobol")):
        d = abs(got[a][0] - got[b][0])
        pooled = np.sqrt(got[a][1] ** 2 + got[b][1] ** 2)
        print("%s vs %s: %.3f pooled standard errors" % (a, b, d / pooled))
        assert d < 5 * pooled, (a, b, d, pooled)
    assert len({round(v[0], 12) for v in got.values()}) == len(got)  # six realisations, not one film


# ---------------------------------------------------------------- defaults
def test_defaults_are_todays_films(tmp_path):
    """With the three setters set and unset again, render, render_adaptive and trace_paths return what a
    fresh oracle returns, for every integrator that samples a light; set, each gives another film; the
    light tracer and instant radiosity ignore all three."""
    s = _scene("cornell-mat", tmp_path)
    _, power = power_table(s)
    grid = grid_tables(s, 4)
    pix = np.arange(0, s.width * s.height, 5, dtype=U32)
    smp = (pix % 3).astype(U32)
    for integ in ("path", "direct", "direct_mis"):
        fresh = Oracle(s, 4, "rtm", integrator=INTEGRATORS[integ])
        want, _ = fresh.render(2, seed=5, threads=4)
        want_ad = fresh.render_adaptive(seed=5, init=2, max_samples=6)
        want_tp = fresh.trace_paths(pix, smp, seed=5)
        o = Oracle(s, 4, "rtm", integrator=INTEGRATORS[integ])
        films = [want]
        for step in ("power", "grid", "sobol"):
            if step == "power":
                o.set_light_table(power)
            elif step == "grid":
                o.set_light_grid(grid["entries"], grid["dims"], grid["lo"], grid["scale"])
            else:
                o.set_sampler("sobol")
            f, _ = o.render(2, seed=5, threads=4)
            assert all(not np.array_equal(bits(f), bits(g)) for g in films), (integ, step)
            films.append(f)
        assert o.mode_counts()["picks"] > 0
        o.set_sampler("pcg")
        o.set_light_grid(None)
        f, _ = o.render(2, seed=5, threads=4)
        assert np.array_equal(bits(f), bits(films[1])), integ  # the power film again
        o.set_light_table(None)
        assert o.mode_counts()["picks"] > 0  # (and reset)
        again, _ = o.render(2, seed=5, threads=4)
        assert np.array_equal(bits(again), bits(want)), integ
        ad = o.render_adaptive(seed=5, init=2, max_samples=6)
        assert np.array_equal(bits(ad[0]), bits(want_ad[0])) and ad[1].tolist() == want_ad[1].tolist()
        assert np.array_equal(bits(o.trace_paths(pix, smp, seed=5)), bits(want_tp))
        assert o.mode_counts()["picks"] == 0
    fresh = Oracle(s, 4, "rtm")
    lt, ir = fresh.render_light(2, seed=5), fresh.render_instant_radiosity(1, seed=9, n_vpl=10)
    o = modes_oracle(s, 4, "path", power=power, grid=grid, sobol=True)
    assert np.array_equal(bits(o.render_light(2, seed=5)), bits(lt)) and (lt != 0).sum() > 100
    assert np.array_equal(bits(o.render_instant_radiosity(1, seed=9, n_vpl=10)), bits(ir)) and (ir != 0).sum() > 100
    assert o.mode_counts()["picks"] == 0


def test_setter_argument_errors(tmp_path):
    s = _scene("cornell-mat", tmp_path, 16, 16)
    n = len(s.lights)
    _, power = power_table(s)
    grid = grid_tables(s, 2)
    o = Oracle(s, 4, "rtm")
    with pytest.raises(ValueError):
        o.set_light_grid(grid["entries"], grid["dims"], grid["lo"], grid["scale"])  # a grid without a table
    with pytest.raises(ValueError):
        o.set_light_table(np.concatenate([power, power[:1]]))  # n is not the light count
    bad = power.copy()
    bad[0, 1] = n  # an alias past the table
    with pytest.raises(ValueError):
        o.set_light_table(bad)
    o.set_light_table(power)
    with pytest.raises(ValueError):
        o.set_light_grid(grid["entries"][:-1], grid["dims"], grid["lo"], grid["scale"])
    with pytest.raises(ValueError):
        o.set_light_grid(grid["entries"], [0, 1, 1], grid["lo"], grid["scale"])
    bad = grid["entries"].copy()
    bad[-1, 0, 1] = n
    with pytest.raises(ValueError):
        o.set_light_grid(bad, grid["dims"], grid["lo"], grid["scale"])
    o.set_light_grid(grid["entries"], grid["dims"], grid["lo"], grid["scale"])
    o.set_light_table(None)  # takes the grid with it
    with pytest.raises(ValueError):
        o.set_light_grid(grid["entries"], grid["dims"], grid["lo"], grid["scale"])
    for bad in ("halton", 2, -1):
        with pytest.raises(ValueError):
            o.set_sampler(bad)
