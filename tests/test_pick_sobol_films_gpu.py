"""Whole films under the power light pick (rtg_set_light_sampling), the light grid (rtg_set_light_grid) and
the Sobol sampler (rtg_set_sampler) against the C oracle restated from include/rtg.h, bit for bit: every
integrator the modes apply to, at every depth, on scenes with glass, mirror, textures, mixed light lists
and reflecting walls, both sides of the LDS table limits, together with luminance-mode environment sampling
and the sampled camera, adaptive renders, the product's fall-backs, and one cut of each family's film.

The oracle's tables are the numpy restatements' words (test_light_sampling_gpu.restated_table on the device's
light records, light_grid_ref.build), asserted equal to the handle's before use and never read from it. The
oracle's counters (Oracle.mode_counts) assert on the CPU side that a film holds the cases it is compared for;
the seeds were chosen on the CPU oracle so that the reference alone meets them. Where a condition cannot hold
for arithmetic reasons it is asserted to be exactly zero instead:
  - DIRECT and DIRECT_MIS shade the camera hit only: no pick, no NEE sample and no Sobol bounce at depth >= 1;
  - one cell (cells = 1) is every path's camera cell;
  - a Sobol bounce opens on a multiple of four, and the next loads that plus the bounce's draws: 6 (a diffuse
    hit under the uniform pick: 1 + 2 + roulette + 2), 7 (power pick), 9 (power pick, luminance-mode
    environment sample), 1 (mirror), 1 or 2 (glass) and 8, the one multiple of four, under the uniform pick
    with a luminance-mode environment sample. Only that combination can load the counter at a multiple."""
import os

import numpy as np
import pytest

import light_grid_ref as gr
from conftest import SCENES
from env_scenes import patch_map, write_table_scene_with_map
from light_grid_scenes import write_room_scene
from raytracingrenderer_amd import loadScene
from shade_scenes import table_cases, table_counts, table_limits
from test_light_sampling_gpu import restated_table
from test_oracle_modes import modes_oracle
from test_sampling_modes_gpu import CAMERAS, assert_same_bits, bits, gpu_tracer, scenes  # noqa: F401 (scenes: a fixture; "polar" is its polar_map() scene)

pytestmark = pytest.mark.gpu

SIZES = [(33, 31), (70, 50)]
INTEGRATORS = [("path", 1), ("path", 4), ("path", 8), ("direct", 4), ("direct_mis", 4)]


@pytest.fixture(scope="module")
def world(scenes, tmp_path_factory):  # noqa: F811
    """world(name, w, h) -> (Scene, luminance alias table or None): test_sampling_modes_gpu's cached scenes,
    and the scenes without an environment map: the room (32 emitters, 64 lights: records in global memory)
    and coffee-small. The restated grids cached by tables() go with the module."""
    cache = {}

    def get(name, w, h):
        if name in ("room", "coffee-small"):
            if (name, w, h) not in cache:
                if name == "coffee-small":
                    path = os.path.join(SCENES, name)
                else:
                    path = write_room_scene(tmp_path_factory.mktemp(name), 32)
                cache[(name, w, h)] = (loadScene(path, width=w, height=h), None)
            return cache[(name, w, h)]
        return scenes(name, w, h)
    yield get
    _grids.clear()


def tracer(scene, lam=None, cells=0, sobol=False, **kw):
    """test_sampling_modes_gpu.gpu_tracer (depth, integrator, seed, luminance, camera, table) under the power
    pick with uniform share lam, a grid of `cells` cells and the Sobol sampler."""
    rt = gpu_tracer(scene, **kw)
    if lam is not None:
        rt.set_light_sampling("power", lam)
    if cells:
        rt.set_light_grid(cells)
    if sobol:
        rt.set_sampler("sobol")
    return rt


_grids = {}


def tables(scene, rt, lam, cells=0, key=None):
    """(power entries, grid dictionary or None): the restated words, asserted equal to the handle's. A grid
    of more than 16 cells per axis comes from light_grid_ref.build_fast (tests/test_light_grid.py holds it
    equal to build()); `key` caches it across the cases of one scene."""
    w, t = restated_table(scene, rt, lam)
    assert t is not None and np.array_equal(rt.light_table()["entries"], t["entries"]), "the handle's light table"
    if not cells:
        return t["entries"], None
    g = _grids.get((key, lam, cells))
    if g is None:
        g = (gr.build_fast if cells > 16 else gr.build)(rt.light_records(), w, scene.node_bounds[0], cells, lam)
        if key is not None:
            _grids[(key, lam, cells)] = g
    info = rt.light_grid()
    assert info["active"] and np.array_equal(info["dims"], g["dims"]) and g["dims"].max() == cells
    assert np.array_equal(bits(info["lo"]), bits(g["lo"])) and np.array_equal(bits(info["scale"]), bits(g["scale"]))
    assert np.array_equal(rt.light_grid_table(), g["entries"]), "the handle's grid tables"
    return t["entries"], g


def film_of(rt, ns, first=0):
    rt.render(ns, first_sample=first)
    film, spp = rt.film()
    assert spp == ns
    return film


def reference(scene, ns, seed, first=0, **kw):
    """(film, counters) of the oracle under modes_oracle's keywords, 8 threads."""
    o = modes_oracle(scene, **kw)
    want, _ = o.render(ns, first=first, seed=seed, threads=8)
    c = o.mode_counts()
    c.update({"env_" + k: v for k, v in o.env_counts().items()})
    assert np.isfinite(want).all()
    return want, c


# ---------------------------------------------------------------- 1. power pick x integrator
@pytest.mark.parametrize("luminance", [False, True])
@pytest.mark.parametrize("lam", [0.125, 0.0])
@pytest.mark.parametrize("integrator,depth", INTEGRATORS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["cornell-mat", "table"])
def test_power_pick_films_equal_the_oracle(world, name, w, h, integrator, depth, lam, luminance):
    """3 spp, seed 1234: cornell-mat (glass, mirror, textures, two area lights and its environment) and the
    table scene (12 emitters plus the environment), uniform share 0.125 and 0, both environment modes. The
    counters: picks that took the alias branch everywhere; under PATH at depth >= 4 at least 100 NEE samples
    past the camera hit with a non-zero contribution (throughput times NEE at a later bounce, after two
    draws per pick have moved every later draw); under DIRECT_MIS on the table scene BSDF-sampled emitter
    hits, weighted with the sampled light's pdf * pmf. The film is not the uniform pick's."""
    s, lum = world(name, w, h)
    rt = tracer(s, lam, depth=depth, integrator=integrator, luminance=luminance, table=lum if luminance else None)
    power, _ = tables(s, rt, lam)
    kw = dict(depth=depth, integrator=integrator, luminance=lum if luminance else None)
    want, c = reference(s, 3, 1234, power=power, **kw)
    print(name, w, h, integrator, depth, lam, luminance, c)
    assert c["alias_picks"] >= 1 and c["picks"] > 100
    if integrator == "path" and depth >= 4:
        assert c["nee_deep"] >= 100
    if integrator != "path":
        assert c["picks_deep"] == 0
    if integrator == "direct_mis" and name == "table":
        assert c["mis_emitter"] >= 1
    uniform, _ = reference(s, 3, 1234, **kw)
    assert not np.array_equal(bits(want), bits(uniform))
    assert_same_bits(film_of(rt, 3), want, "%s %dx%d %s depth %d, power %g%s"
                     % (name, w, h, integrator, depth, lam, ", luminance" if luminance else ""))


# ---------------------------------------------------------------- 2. the global-table kernels
@pytest.mark.parametrize("cells", [0, 4])
@pytest.mark.parametrize("case", [4, 5])
def test_pick_and_grid_past_the_lds_table_limits(tmp_path, case, cells):
    """shade_scenes' cases one material and one emitter past the LDS limits (k_shade_pick<*, false>,
    k_shade_grid<*, false>), the environment in the light list, 32 x 24, 16 spp, PATH at depth 6 and
    DIRECT_MIS, under the power pick alone and under a grid of 4 cells."""
    n_emitters, n_extra = table_cases()[case][:2]
    s = loadScene(write_table_scene_with_map(tmp_path, patch_map(), n_emitters, n_extra), width=32, height=24)
    mats, lights = table_counts(s)
    lm, ll = table_limits()
    assert (mats > lm) if case == 4 else (mats <= lm and lights > ll), (mats, lights)
    for integrator in ("path", "direct_mis"):
        rt = tracer(s, 0.125, cells, depth=6, integrator=integrator, seed=31)
        power, grid = tables(s, rt, 0.125, cells, key=("case", case))
        want, c = reference(s, 16, 31, depth=6, integrator=integrator, power=power, grid=grid)
        print(case, mats, lights, integrator, cells, c)
        assert c["alias_picks"] >= 1
        if integrator == "path":
            assert c["nee_deep"] >= 100 and (not cells or c["other_cell"] >= 100)
        assert_same_bits(film_of(rt, 16), want, "case %d %s cells %d" % (case, integrator, cells))


# ---------------------------------------------------------------- 3. the grid
GRID_SCENES = [("room", 64, 48), ("cornell-mat", 33, 31), ("cornell-mat", 70, 50)]


@pytest.mark.parametrize("integrator,depth", [("path", 4), ("path", 8), ("direct", 4), ("direct_mis", 4)])
@pytest.mark.parametrize("cells", [1, 8, 64])
@pytest.mark.parametrize("name,w,h", GRID_SCENES)
def test_grid_films_equal_the_oracle(world, name, w, h, cells, integrator, depth):
    """3 spp, seed 1234, uniform share 0.125: the room (64 lights under the ceiling, their records in global
    memory; at 64 cells its 64 x 64 x 64 x 64 entries are exactly the admissible 2^24) and cornell-mat (walls,
    mirror, glass, the environment in the list). Under PATH with more than one cell at least 100 picks past
    the camera hit fall into another cell than the camera hit's, in at least 3 distinct cells: a path that
    leaves one cell shades in another; on cornell-mat at least 100 NEE samples past the camera hit contribute
    (the room has no walls: what its bounces reach is the black cubes, and theirs contribute nothing).
    DIRECT_MIS under the grid has its exact reference here. One cell: the film is the power pick's exactly
    when light_grid_ref's single table is the power table."""
    s, _ = world(name, w, h)
    rt = tracer(s, 0.125, cells, depth=depth, integrator=integrator)
    power, grid = tables(s, rt, 0.125, cells, key=(name, w, h))
    want, c = reference(s, 3, 1234, depth=depth, integrator=integrator, power=power, grid=grid)
    print(name, w, h, cells, integrator, depth, c)
    assert c["picks"] > 100 and c["alias_picks"] >= 1
    if integrator == "path" and cells > 1:
        assert c["other_cell"] >= 100 and c["other_cells_distinct"] >= 3
    if integrator == "path":
        assert (c["nee_deep"] >= 100) if name == "cornell-mat" else (c["nee_deep"] == 0 and c["picks_deep"] >= 100)
    if not (integrator == "path" and cells > 1):
        assert c["other_cell"] == 0
    pw, _ = reference(s, 3, 1234, depth=depth, integrator=integrator, power=power)
    if cells == 1:
        assert grid["entries"].shape[0] == 1
        same_table = np.array_equal(grid["entries"][0], power)
        assert np.array_equal(bits(want), bits(pw)) == same_table, same_table
    else:
        assert not np.array_equal(bits(want), bits(pw))
    assert_same_bits(film_of(rt, 3), want, "%s %dx%d cells %d %s depth %d" % (name, w, h, cells, integrator, depth))


# ---------------------------------------------------------------- 4. Sobol
SOBOL_CASES = [("cornell-mat", False), ("cornell-mat", True), ("coffee-small", False)]


@pytest.mark.parametrize("lam", [None, 0.125])
@pytest.mark.parametrize("integrator,depth", INTEGRATORS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,luminance", SOBOL_CASES)
def test_sobol_films_equal_the_oracle(world, name, luminance, w, h, integrator, depth, lam):
    """3 spp, seed 1234, the uniform and the power pick, cornell-mat under both environment modes and
    coffee-small (six area lights, no environment map: one mode). Under PATH at depth >= 4 at least 100
    bounces load a counter that is not a multiple of four and round it up, at depth 8 some path reaches draw
    group 6, and under the uniform pick with luminance mode (only there: the module's docstring) at least
    one bounce loads it at an exact multiple. The film is not the PCG film."""
    s, lum = world(name, w, h)
    assert (lum is not None) == (name == "cornell-mat")
    rt = tracer(s, lam, sobol=True, depth=depth, integrator=integrator, luminance=luminance, table=lum if luminance else None)
    assert rt.sampler_active == "sobol"
    power = tables(s, rt, lam)[0] if lam is not None else None
    kw = dict(depth=depth, integrator=integrator, power=power, luminance=lum if luminance else None)
    want, c = reference(s, 3, 1234, sobol=True, **kw)
    print(name, luminance, w, h, integrator, depth, lam, c)
    if integrator == "path" and depth >= 4:
        assert c["sobol_rounded"] >= 100
        assert depth < 8 or c["sobol_max_group"] >= 6
    if integrator != "path":
        assert c["sobol_rounded"] == 0 and c["sobol_aligned"] == 0
    if integrator == "path" and depth >= 4 and luminance and lam is None:
        assert c["sobol_aligned"] >= 1
    if not (luminance and lam is None):
        assert c["sobol_aligned"] == 0
    pcg, _ = reference(s, 3, 1234, **kw)
    assert not np.array_equal(bits(want), bits(pcg))
    assert_same_bits(film_of(rt, 3), want, "%s %dx%d %s depth %d, sobol, power %r%s"
                     % (name, w, h, integrator, depth, lam, ", luminance" if luminance else ""))


@pytest.mark.parametrize("integrator,depth", [("path", 8), ("direct_mis", 4)])
def test_sobol_films_at_the_last_sample_numbers_equal_the_oracle(world, integrator, depth):
    """first_sample = 65533 with 3 samples: 65533, 65534 and 65535, the last sample numbers below the 16-bit
    limit of a key (cornell-mat 33 x 31, the power pick, luminance mode)."""
    s, lum = world("cornell-mat", 33, 31)
    rt = tracer(s, 0.125, sobol=True, depth=depth, integrator=integrator, luminance=True, table=lum)
    power, _ = tables(s, rt, 0.125)
    kw = dict(depth=depth, integrator=integrator, power=power, luminance=lum, sobol=True)
    want, c = reference(s, 3, 1234, first=65533, **kw)
    first, _ = reference(s, 3, 1234, first=0, **kw)
    print(integrator, depth, c)
    assert c["picks"] > 100 and not np.array_equal(bits(want), bits(first))
    assert_same_bits(film_of(rt, 3, first=65533), want, "samples 65533..65535, %s" % integrator)


SOBOL_POLAR_SEED = 6


@pytest.mark.parametrize("integrator", ["direct_mis", "path"])
def test_rejected_environment_samples_under_sobol_equal_the_oracle(world, integrator):
    """The table scene under polar_map() at 70 x 50 under Sobol and luminance mode, the seed picked on the CPU
    oracle: at least one environment sample is rejected at the pole (sin theta <= 0), and its four draws are
    taken all the same, so every later draw of the path keeps its place in the sequence."""
    s, lum = world("polar", 70, 50)
    rt = tracer(s, sobol=True, depth=4, integrator=integrator, seed=SOBOL_POLAR_SEED, luminance=True, table=lum)
    want, c = reference(s, 3, SOBOL_POLAR_SEED, depth=4, integrator=integrator, luminance=lum, sobol=True)
    print(integrator, c)
    assert c["env_rejected"] >= 1 and c["env_samples"] > 100
    assert_same_bits(film_of(rt, 3), want, "polar map under sobol, %s" % integrator)


# ---------------------------------------------------------------- 5. all together
@pytest.mark.parametrize("integrator", ["path", "direct_mis"])
def test_all_modes_together_equal_the_oracle(world, integrator):
    """The table scene at 70 x 50 under the power pick, luminance mode, tent + lens and Sobol at once; the
    film differs from each of the four oracles that has one of the settings switched off."""
    s, lum = world("table", 70, 50)
    cam = CAMERAS["tent+lens"]
    rt = tracer(s, 0.125, sobol=True, depth=4, integrator=integrator, luminance=True, camera=cam, table=lum)
    assert rt.sampler_active == "sobol"
    power, _ = tables(s, rt, 0.125)
    full = dict(power=power, luminance=lum, camera=cam, sobol=True)
    want, c = reference(s, 3, 1234, depth=4, integrator=integrator, **full)
    print(integrator, c)
    assert c["alias_picks"] >= 1 and c["env_samples"] > 100 and c["env_occluded"] >= 1
    if integrator == "path":
        assert c["nee_deep"] >= 100 and c["sobol_rounded"] >= 100
    else:
        assert c["mis_emitter"] >= 1
    for off in sorted(full):
        f, _ = reference(s, 3, 1234, depth=4, integrator=integrator, **{k: v for k, v in full.items() if k != off})
        assert not np.array_equal(bits(f), bits(want)), off
    assert_same_bits(film_of(rt, 3), want, "power + luminance + tent + lens + sobol, %s" % integrator)


# ---------------------------------------------------------------- 6. the product's fall-backs
@pytest.mark.parametrize("integrator", ["path", "direct_mis"])
def test_fallbacks_render_what_the_oracle_is_told(world, integrator):
    """Sobol with the grid set: the frames keep PCG (sampler_active says so), camera samples included: the
    film is the oracle's (grid, PCG) film under tent + lens and no other. The grid set under the uniform
    light mode: nothing is built and the film is the default oracle's."""
    s, _ = world("room", 64, 48)
    cam = CAMERAS["tent+lens"]
    rt = tracer(s, 0.125, 8, sobol=True, depth=4, integrator=integrator, camera=cam)
    assert rt.sampler == "sobol" and rt.sampler_active == "pcg"
    power, grid = tables(s, rt, 0.125, 8, key=("room", 64, 48))
    want, c = reference(s, 3, 1234, depth=4, integrator=integrator, power=power, grid=grid, camera=cam)
    told, _ = reference(s, 3, 1234, depth=4, integrator=integrator, power=power, grid=grid, camera=cam, sobol=True)
    print(integrator, c)
    assert c["picks"] > 100 and not np.array_equal(bits(told), bits(want))
    assert_same_bits(film_of(rt, 3), want, "grid + sobol keeps pcg, %s" % integrator)
    rt = tracer(s, None, 8, depth=4, integrator=integrator)
    assert not rt.light_grid()["active"] and rt.light_table() is None
    plain, c = reference(s, 3, 1234, depth=4, integrator=integrator)
    assert c["picks"] == 0
    assert_same_bits(film_of(rt, 3), plain, "grid under the uniform light mode, %s" % integrator)


# ---------------------------------------------------------------- 7. adaptive
@pytest.mark.parametrize("mode", ["power", "grid", "sobol"])
def test_adaptive_render_under_the_modes_equals_the_oracle(world, mode):
    """rtg_render_adaptive against or_render_adaptive on cornell-mat 72 x 40, seed 11, 2 initial samples, at
    most 12 (test_sampling_modes_gpu's adaptive scene and sizes): tile counts and film."""
    s, _ = world("cornell-mat", 72, 40)
    lam = None if mode == "sobol" else 0.125
    cells = 8 if mode == "grid" else 0
    rt = tracer(s, lam, cells, sobol=mode == "sobol", depth=4, seed=11)
    power, grid = tables(s, rt, lam, cells) if lam is not None else (None, None)
    o = modes_oracle(s, 4, "path", power=power, grid=grid, sobol=mode == "sobol")
    want, want_counts = o.render_adaptive(first=0, seed=11, init=2, max_samples=12, min_samples=1)
    c = o.mode_counts()
    print(mode, c, want_counts.tolist())
    assert (c["sobol_rounded"] if mode == "sobol" else c["nee_deep"]) >= 100
    plain, _ = modes_oracle(s, 4, "path").render_adaptive(first=0, seed=11, init=2, max_samples=12, min_samples=1)
    assert not np.array_equal(bits(plain), bits(want))
    counts = rt.adaptiveRender(init_samples=2, max_samples=12, min_samples=1, first_sample=0)
    film, spp = rt.film()
    assert spp == 1 and counts.tolist() == want_counts.tolist() and counts.max() > counts.min()
    assert_same_bits(film, want, "adaptive, " + mode)


# ---------------------------------------------------------------- 8. one cut each
@pytest.mark.parametrize("family", ["power", "grid", "sobol"])
def test_one_cut_of_each_family_equals_the_film_of_one_call(world, family):
    """The 3-spp film of one call (section 1's cornell-mat PATH depth 4 film at 70 x 50, section 3's room film
    at 8 cells, section 4's first film), which the oracle's film pins, equals the film of three queued 1-spp
    frames and the film of two complementary tile sets. The modes' own test files hold the fuller matrix."""
    if family == "power":
        s, _ = world("cornell-mat", 70, 50)
        kw, lam, cells = dict(depth=4), 0.125, 0
    elif family == "grid":
        s, _ = world("room", 64, 48)
        kw, lam, cells = dict(depth=4), 0.125, 8
    else:
        s, _ = world("cornell-mat", 33, 31)
        kw, lam, cells = dict(depth=1), None, 0
    rt = tracer(s, lam, cells, sobol=family == "sobol", **kw)
    power, grid = tables(s, rt, lam, cells, key=("room", 64, 48)) if lam is not None else (None, None)
    want, c = reference(s, 3, 1234, power=power, grid=grid, sobol=family == "sobol", **kw)
    print(family, c)
    assert c["nee_deep" if family == "power" else "other_cell" if family == "grid" else "sobol_rounded"] >= 100
    assert_same_bits(film_of(rt, 3), want, family + ", one call")
    rt.clear()
    for _ in range(3):
        rt.render(1, sync=False)
    assert_same_bits(rt.film()[0], want, family + ", three queued frames")
    rt.clear()
    tiles = np.arange(rt.tiles_x * rt.tiles_y, dtype=np.uint32)
    assert len(tiles) > 1
    for part in (tiles[0::2], tiles[1::2]):
        rt.render(3, tiles=part, first_sample=0)
    assert_same_bits(rt.film()[0], want, family + ", two complementary tile sets")
