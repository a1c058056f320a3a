"""Per-shading-point light selection on the GPU (rtg_set_light_grid): the handle's tables and the kernel's
cell and pick against the numpy restatement (tests/light_grid_ref.py) bit for bit, DIRECT and PATH films
rebuilt sample by sample with the cell taken from the restated hit point (light records in global memory
and in LDS, the environment in the light list under both environment modes), the grid's agreement in
expectation with the uniform pick and its lower noise against the power pick, and the settings, fall-backs
and entry points that must keep today's films."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_sampling_ref as er
import light_grid_ref as gr
import light_sampling_ref as lr
from env_scenes import smooth_map
from light_grid_scenes import write_hall_scene
from light_pick_scenes import write_emitters_env_scene, write_one_triangle_scene
from material_scenes import write_material_floor_scene
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, probe_texture, save_hdr
from raytracingrenderer_amd import _native as N
from shade_scenes import table_limits, write_table_scene
from test_light_grid import hall_variance_ratio
from test_light_sampling_gpu import assert_same_bits, bits, env_texels, restated_table

pytestmark = pytest.mark.gpu

F = np.float32
LAM = 0.125


def restated_grid(s, rt, cells, lam=LAM):
    """The restatement's grid from the device's own records, the handle's §8d weights and the root box."""
    return gr.build(rt.light_records(), rt.light_table()["weights"], s.node_bounds[0], cells, lam)


def refusal(call, *args):
    """The message of the NativeError that call(*args) raises. The exception is gone when this returns: a
    test that kept it (pytest.raises(...) as e) would tie its own frame, and every handle in it, into a
    reference cycle through the traceback, and those handles would then be destroyed at some later
    collection, in the middle of another test."""
    try:
        call(*args)
    except NativeError as err:
        return str(err)
    raise AssertionError("not refused")


def grid_on(s, cells=8, **kw):
    rt = RayTracer(s, **kw)
    rt.set_light_sampling("power")
    rt.set_light_grid(cells)
    return rt


# ---------------------------------------------------------------- 1. the tables
@pytest.mark.parametrize("n_em,cells", [(32, 8), (12, 3)])
def test_uploaded_tables_equal_the_restatement(tmp_path, n_em, cells):
    s = loadScene(write_hall_scene(tmp_path / "h", n_em))
    assert len(s.lights) == 2 * n_em and (len(s.lights) <= table_limits()[1]) == (n_em == 12)
    rt = RayTracer(s)
    assert rt.light_grid()["cells"] == 0 and not rt.light_grid()["active"] and rt.light_grid_table() is None
    rt.set_light_grid(cells)  # stored, nothing built: the light mode is uniform
    assert rt.light_grid()["cells"] == cells and not rt.light_grid()["active"] and rt.light_grid_table() is None
    rt.set_light_sampling("power")
    g = rt.light_grid()
    want = restated_grid(s, rt, cells)
    assert g["active"] and g["n_entries"] == int(want["dims"].prod()) * len(s.lights) and g["build_ms"] > 0
    assert np.array_equal(g["dims"], want["dims"]) and g["dims"].max() == cells
    assert np.array_equal(bits(g["lo"]), bits(want["lo"])) and np.array_equal(bits(g["scale"]), bits(want["scale"]))
    t = rt.light_grid_table()
    assert np.array_equal(t, want["entries"]), int((t != want["entries"]).any(2).sum())
    assert not np.array_equal(t[0], t[-1])  # the two ends of the hall pick differently
    w, power = restated_table(s, rt)
    assert np.array_equal(rt.light_table()["entries"], power["entries"])  # the power table stays what it was
    rt.set_light_sampling("power", 0.5)  # another share: both rebuilt
    assert np.array_equal(rt.light_grid_table(), restated_grid(s, rt, cells, 0.5)["entries"])
    rt.set_light_grid(cells + 1)  # another cells: rebuilt
    assert np.array_equal(rt.light_grid_table(), restated_grid(s, rt, cells + 1, 0.5)["entries"])
    rt.set_light_grid(0)
    assert rt.light_grid_table() is None and rt.light_table() is not None


# ---------------------------------------------------------------- 2. the probe
def test_probe_equals_the_restated_cell_light_and_pmf(tmp_path):
    """Points on cell faces, outside the box, NaN and infinite ones, and 4096 random ones inside and around
    the box, each with its own draws."""
    s = loadScene(write_hall_scene(tmp_path / "h", 32))
    rt = RayTracer(s)
    with pytest.raises(NativeError):
        rt.light_grid_probe(np.zeros((1, 3), F), np.zeros(1, np.uint32), np.zeros(1, F))  # no active grid
    rt.set_light_sampling("power")
    rt.set_light_grid(16)
    g = rt.light_grid()
    ent = rt.light_grid_table()
    dims, lo, sc = g["dims"], g["lo"], g["scale"]
    assert tuple(dims) == (16, 2, 2)
    rng = np.random.default_rng(5)
    box = np.array(s.node_bounds[0], F)
    ext = box[3:6] - box[0:3]
    pts = (box[0:3] - F(0.25) * ext + rng.random((4096, 3)).astype(F) * (F(1.5) * ext)).astype(F)
    faces = np.array([[box[0] + F(k) * (ext[0] / F(16)), box[1] + F(j) * (ext[1] / F(2)), box[2] + F(i) * (ext[2] / F(2))]
                      for k in range(17) for j in range(3) for i in range(3)], F)
    near = np.concatenate([np.nextafter(faces, F(-1e9)), np.nextafter(faces, F(1e9))]).astype(F)
    odd = np.array([[np.nan, 0.5, 0.0], [0.0, np.nan, np.nan], [np.nan] * 3, [np.inf, 1.0, 0.0], [-np.inf, -np.inf, np.inf],
                    [1e30, -1e30, 0.0], [0.0, 1.0, 0.0]], F)
    pts = np.concatenate([pts, faces, near, odd]).astype(F)
    n = len(pts)
    r0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    d1 = (rng.integers(0, 2 ** 24, n).astype(F) * F(2.0 ** -24)).astype(F)
    cell, li, pmf = rt.light_grid_probe(pts, r0, d1)
    want_cell = gr.cell_of(pts, dims, lo, sc)
    assert np.array_equal(cell, want_cell.astype(np.int32)), np.flatnonzero(cell != want_cell)[:8]
    wli, wpmf = gr.pick(ent, want_cell, r0, d1)
    assert np.array_equal(li, wli.astype(np.int32))
    assert_same_bits(pmf, wpmf, "pmf")
    assert (cell >= 0).all() and (cell < int(dims.prod())).all() and (li >= 0).all() and (li < len(s.lights)).all()
    assert (pmf > 0).all() and len(np.unique(cell)) == int(dims.prod())
    assert list(cell[-7:-4]) == [(1 * 2 + 0) * 16 + 0, 8, 0]  # a NaN coordinate: index 0 on that axis


# ---------------------------------------------------------------- 3. exact films
def film_ref(s, rt, ns, seed, luminance=False):
    """tests/test_light_sampling_gpu.py's film_ref with the pick made from the table of the cell that holds
    the restated hit point x = o + d t: the DIRECT film of ns samples, rebuilt in numpy. Returns (film
    (H, W, 3), surface mask, occluded count, visible count, cells used)."""
    W, H = s.width, s.height
    rec = rt.light_records()
    g = rt.light_grid()
    ent = rt.light_grid_table()
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
    old = np.seterr(all="ignore")  # (a missed pixel's t = FLT_MAX runs through the arithmetic unused)
    x = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]  # Ray::at
    cell = gr.cell_of(x, g["dims"], g["lo"], g["scale"])
    film = np.zeros((W * H, 3), F)
    n_occ = n_vis = 0
    for sl in range(ns):
        st = er.PathStream(pix, np.full(W * H, sl, np.uint32), seed)
        r0 = st.raw()
        d1 = st.next()
        li, pmf = gr.pick(ent, cell, r0, d1)
        L = rec[li]
        a_raw = st.raw()
        a = (a_raw >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
        b = st.next()
        p2 = lr.triangle_sample(L, a, b)
        gg, _ = lr.area_geometry(L, p2, x, sn)
        emitted = L[:, 16:19]
        pdf = L[:, 11]
        if has_env:
            if luminance:
                d = np.stack([b, st.next(), st.next()], axis=1)
                wi, epdf, _ = er.sample(eent, tex.shape[1], tex.shape[0], a_raw, d)
            else:
                wi, epdf = er.uniform_sample(b, a)
                epdf = np.full(W * H, epdf, F)
            ge = lr.dot3(wi, sn)
            ge = np.where((ge > 0) & (epdf > 0), ge, F(0)).astype(F)
            isenv = kind[li] == 1
            E = probe_texture(tex, wi, env=True)
            p2 = np.where(isenv[:, None], x + wi * F(10000.0), p2).astype(F)
            gg = np.where(isenv, ge, gg).astype(F)
            emitted = np.where(isenv[:, None], E, emitted).astype(F)
            pdf = np.where(isenv, epdf, pdf).astype(F)
        act = surf & (gg > 0)
        ld = (((f * emitted) * gg[:, None]) / (pmf * pdf)[:, None]).astype(F)
        q = lr.shadow_ray(x, p2)
        q[~act] = (0, 1e6, 0, 1, 0, 1, 0, 0)
        vis = rt.trace_visible(q) != 0
        lit = surf & (f.sum(1) > 0)
        n_occ += int((act & ~vis & lit).sum())
        n_vis += int((act & vis & lit).sum())
        c = np.where((act & vis)[:, None], ld, F(0)).astype(F)
        c = np.where(emitter[:, None], em_of[mat], c).astype(F)
        film = film + c
    np.seterr(**old)
    return film.reshape(H, W, 3), surf.reshape(H, W), n_occ, n_vis, len(np.unique(cell[surf]))


def check_cuts(s, rt, want, seed, integrator, cells, env_mode="uniform", cuts="all"):
    """rt's film of 4 samples equals `want` bit for bit from one call, four 1-spp calls, queued frames, two
    complementary tile sets, chunks of a quarter of the paths and a two-rank group on device 0 twice."""
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
    small = RayTracer(s, seed=seed, integrator=integrator, max_depth=4, max_paths=s.width * s.height)
    small.set_env_sampling(env_mode)
    small.set_light_sampling("power")
    small.set_light_grid(cells)
    small.render(4)
    assert_same_bits(small.film()[0], want, "chunks of one sample per pixel")
    g = RayTracerGroup(s, devices=(0, 0), seed=seed)
    for r in range(2):  # (the group has no integrator setting of its own: through each rank's handle)
        assert g._lib.rtg_set_integrator(g._lib.rtg_group_handle(g._g, r), RayTracer.INTEGRATORS[integrator]) == 0
    g.set_env_sampling(env_mode)
    g.set_light_sampling("power")
    g.set_light_grid(cells)
    g.render(4)
    assert_same_bits(g.film()[0], want, "two-rank group on device 0 twice")


@pytest.mark.parametrize("n_em,size", [(32, (64, 48)), (12, (33, 31))])
def test_direct_and_path_films_are_the_restated_sum(tmp_path, n_em, size):
    """The hall with 64 lights (records in global memory) and with 24 (in LDS), 8 cells along it, 4 spp:
    DIRECT equals the rebuilt sum bit for bit however it is cut, and so does PATH at depth 4: nothing a bounce
    can reach reflects light (the cubes are black, the floor is flat, a miss is black, and an emitter met by a
    non-specular bounce gives nothing), so every later term is thr * 0 = +0."""
    s = loadScene(write_hall_scene(tmp_path / "h", n_em, *size))
    W, H = size
    assert len(s.lights) == 2 * n_em and s.desc.env_texture < 0
    rt = grid_on(s, 8, seed=77, integrator="direct")
    want, surf, n_occ, n_vis, n_cells = film_ref(s, rt, 4, 77)
    print("surface pixels %d of %d, occluded samples %d, visible %d, cells under the camera %d"
          % (surf.sum(), W * H, n_occ, n_vis, n_cells))
    assert surf.sum() > 0.3 * W * H and n_occ > 0 and n_vis > 0 and n_cells >= 6
    check_cuts(s, rt, want, 77, "direct", 8)
    pt = grid_on(s, 8, seed=77, integrator="path", max_depth=4)
    check_cuts(s, pt, want, 77, "path", 8)
    pw = RayTracer(s, seed=77, integrator="direct")
    pw.set_light_sampling("power")
    pw.render(4)
    assert not np.array_equal(bits(pw.film()[0]), bits(want))  # other tables: another film


@pytest.mark.parametrize("luminance", [True, False])
def test_direct_film_with_the_environment_in_the_light_list(tmp_path, luminance):
    """tests/light_pick_scenes.py's floor under four emitters and a smooth environment map that is in the
    light list (9 lights), 4 cells: the environment sampled through its luminance table
    (k_shade_grid<*, *, true>) or uniformly."""
    s = loadScene(write_emitters_env_scene(tmp_path / "e", smooth_map(16, 8), 4))
    assert len(s.lights) == 9 and (np.array(s.lights) == -1).sum() == 1
    mode = "luminance" if luminance else "uniform"
    rt = RayTracer(s, seed=78, integrator="direct")
    rt.set_env_sampling(mode)
    rt.set_light_sampling("power")
    rt.set_light_grid(4)
    assert (rt.env_table() is not None) == luminance
    want_g = restated_grid(s, rt, 4)
    assert np.array_equal(rt.light_grid_table(), want_g["entries"])
    e = int(np.flatnonzero(np.array(s.lights) == -1)[0])
    assert (want_g["pmf"][:, e] > LAM / 9).all() and not want_g["uniform"].any()
    want, surf, n_occ, n_vis, n_cells = film_ref(s, rt, 4, 78, luminance)
    assert surf.sum() > 0.3 * surf.size and n_vis > 0 and n_cells >= 2
    check_cuts(s, rt, want, 78, "direct", 4, mode)


def test_direct_mis_runs_the_grid_and_keeps_the_expectation(tmp_path):
    """DIRECT_MIS on the 24-light hall: the grid's film is its own (not the power pick's), the same bits from
    one call, 1-spp calls, queued frames, tile sets, one-sample chunks and a two-rank group, and its image mean
    over 8 seeds x 64 spp agrees with the power pick's within six standard errors. (No restated DIRECT_MIS film:
    the BSDF half reads the pdf * pmf its light half stored, code the grid does not touch.)"""
    s = loadScene(write_hall_scene(tmp_path / "h", 12))
    one = grid_on(s, 8, seed=79, integrator="direct_mis")
    one.render(4)
    want = one.film()[0].copy()
    assert (want != 0).sum() > 1000
    check_cuts(s, one, want, 79, "direct_mis", 8)
    means = {}
    for what in ("power", "grid"):
        rt = RayTracer(s, integrator="direct_mis")
        rt.set_light_sampling("power")
        rt.set_light_grid(8 if what == "grid" else 0)
        m = []
        for k in range(8):
            rt.seed = 4000 + k
            rt.clear()
            rt.render(64)
            f, spp = rt.film()
            m.append(float(er.lum32(f / F(spp)).astype(np.float64).mean()))
        means[what] = np.array(m)
        if what == "grid":
            whole = f.copy()
            rt.clear()
            for _ in range(4):
                rt.render(16, sync=False)
            assert_same_bits(rt.film()[0], whole, "queued frames")
        else:
            other = f.copy()
    assert not np.array_equal(bits(whole), bits(other))
    mu = {k: v.mean() for k, v in means.items()}
    se = {k: v.std(ddof=1) / np.sqrt(8) for k, v in means.items()}
    print("means %r, standard errors %r" % (mu, se))
    assert abs(mu["power"] - mu["grid"]) <= 6 * np.sqrt(se["power"] ** 2 + se["grid"] ** 2)


# ---------------------------------------------------------------- 4. statistics
@pytest.fixture(scope="module")
def hall_seed_films(tmp_path_factory):
    """({mode: (8, H, W) float64 luminance of the DIRECT film of 64 spp, one per seed} on the 64-light hall for
    the uniform pick, the power pick and the grid of 8 cells, the surface mask); rendered once for the module
    and left unchanged."""
    s = loadScene(write_hall_scene(tmp_path_factory.mktemp("hall64") / "h", 32))
    nrm = RayTracer(s, integrator="normals")
    nrm.render(1)
    surf = nrm.film()[0].sum(2) > 0
    lum = {}
    for what in ("uniform", "power", "grid"):
        rt = RayTracer(s, integrator="direct")
        rt.set_light_sampling("uniform" if what == "uniform" else "power")
        rt.set_light_grid(8 if what == "grid" else 0)
        assert rt.light_grid()["active"] == (what == "grid")
        per_seed = []
        for k in range(8):
            rt.seed = 3000 + k
            rt.clear()
            rt.render(64)
            f, spp = rt.film()
            per_seed.append(er.lum32(f / F(spp)).astype(np.float64))
        lum[what] = np.stack(per_seed)
    return lum, surf


def test_grid_and_uniform_means_agree(hall_seed_films):
    """The 64-light hall, DIRECT, 64 x 48, 8 seeds x 64 spp per mode: the image means of the grid and of the
    uniform pick agree within six standard errors of their difference (from the spread across seeds)."""
    lum, surf = hall_seed_films
    means = {k: v.reshape(8, -1).mean(1) for k, v in lum.items()}
    se = {k: v.std(ddof=1) / np.sqrt(8) for k, v in means.items()}
    print("means %r, standard errors %r" % ({k: v.mean() for k, v in means.items()}, se))
    assert means["uniform"].mean() > 0
    assert abs(means["uniform"].mean() - means["grid"].mean()) <= 6 * np.sqrt(se["uniform"] ** 2 + se["grid"] ** 2)


def test_grid_is_less_noisy_than_the_power_pick_in_the_hall(tmp_path, hall_seed_films):
    """The same films: the across-seed variance of a pixel's luminance, added over the surface pixels, is lower
    under the grid than under the *power* pick by at least half the per-sample variance ratio of the numpy
    restatement at unoccluded floor points (tests/test_light_grid.py: 3.47 there, so at least 1.73 here; halved
    because eight seeds scatter and because the film also holds the cubes' penumbrae, where visibility adds
    noise the pick cannot remove). Measured on an MI355X: 0.637 against 0.218, a ratio of 2.92."""
    vp, vg, _ = hall_variance_ratio(tmp_path, 32)
    cpu_ratio = vp.sum() / vg.sum()
    assert cpu_ratio >= 2.0
    lum, surf = hall_seed_films
    var = {k: float(v.var(axis=0, ddof=1)[surf].sum()) for k, v in lum.items()}
    gpu_ratio = var["power"] / var["grid"]
    print("CPU per-sample variance ratio %.3f; GPU summed across-seed variances %r, power / grid %.3f, "
          "uniform / grid %.3f" % (cpu_ratio, var, gpu_ratio, var["uniform"] / var["grid"]))
    assert gpu_ratio >= 0.5 * cpu_ratio


# ---------------------------------------------------------------- 5. the setting and its fall-backs
def test_setting_and_fallbacks(tmp_path):
    """Off by default; cells = 0 and the uniform mode give the power / uniform film's bits; the cap and a
    bad argument are refused and keep films and tables; a handle under the physical material model or path MIS
    renders the power-mode film."""
    s = loadScene(write_hall_scene(tmp_path / "h", 12, 33, 31))
    films = {}
    for what in ("uniform", "power"):
        rt = RayTracer(s, seed=9, integrator="direct")
        rt.set_light_sampling(what)
        assert rt.light_grid()["cells"] == 0
        rt.render(2)
        films[what] = rt.film()[0]
    rt = grid_on(s, 8, seed=9, integrator="direct")
    rt.render(2)
    films["grid"] = rt.film()[0]
    ent = rt.light_grid_table()
    assert not np.array_equal(bits(films["grid"]), bits(films["power"]))
    for bad in (65, 1000):  # the cap: 24 lights admit 64 cells at most
        assert "largest admissible cells is 64" in refusal(rt.set_light_grid, bad)
        assert rt.light_grid()["cells"] == 8 and np.array_equal(rt.light_grid_table(), ent)
    with pytest.raises(NativeError):
        rt.set_light_sampling("power", 1.5)
    assert np.array_equal(rt.light_grid_table(), ent)
    rt.clear()
    rt.render(2)
    assert_same_bits(rt.film()[0], films["grid"], "after the refused settings")
    rt.set_light_grid(0)
    rt.clear()
    rt.render(2)
    assert_same_bits(rt.film()[0], films["power"], "cells = 0")
    rt.set_light_grid(8)
    rt.set_light_sampling("uniform")
    assert rt.light_grid()["cells"] == 8 and not rt.light_grid()["active"]
    rt.clear()
    rt.render(2)
    assert_same_bits(rt.film()[0], films["uniform"], "the uniform mode with a grid set")
    # kernels that take their pick at run time keep the power pick and its table
    phys = loadScene(write_material_floor_scene(tmp_path / "m", "orennayar", 33, 31))  # 22 lights, an Oren-Nayar floor
    for setting in ("physical", "pathMIS"):
        got = []
        for cells in (0, 8):
            pt = RayTracer(phys if setting == "physical" else s, seed=9, integrator="path", max_depth=3)
            pt.set_light_sampling("power")
            if setting == "physical":
                pt.set_material_model("physical")
            else:
                pt.set_path_mis("power")
            pt.set_light_grid(cells)
            assert pt.light_grid()["active"] == (cells == 8)  # built, and not what these kernels read
            pt.render(2)
            got.append(pt.film()[0])
        assert (got[0] != 0).sum() > 100
        assert_same_bits(got[1], got[0], setting)
    # the entry cap, from the handle's own box: the 281-light table scene is a 2 x 2 x 2 room, cells^3 cells
    room = loadScene(write_table_scene(tmp_path / "t", 140, 5, envmap=True), width=32, height=24)
    assert len(room.lights) == 281
    rr = grid_on(room, 4)
    ent4 = rr.light_grid_table()
    assert ent4.shape[0] == 64 and 39 ** 3 * 281 <= 2 ** 24 < 40 ** 3 * 281
    assert "largest admissible cells is 39" in refusal(rr.set_light_grid, 40)
    assert rr.light_grid()["cells"] == 4 and np.array_equal(rr.light_grid_table(), ent4)
    wide = grid_on(s, 64)  # the hall's box is long and thin: 64 x 8 x 8 cells of 24 lights fit
    assert tuple(wide.light_grid()["dims"]) == (64, 8, 8) and wide.light_grid()["active"]
    g = RayTracerGroup(s, devices=(0, 0))
    with pytest.raises(NativeError):
        g.set_light_grid(65)
    p = N.rtg_light_grid(5)
    assert N.rtg().rtg_get_light_grid(g._lib.rtg_group_handle(g._g, 1), C.byref(p)) == 0 and p.cells == 0
    g.render(2)  # the group after the refused setting: the default's film
    one = RayTracer(s)
    one.render(2)
    assert_same_bits(g.film()[0], one.film()[0], "the group after the refused setting")


def test_one_light_leaves_no_grid(tmp_path):
    """A scene lit by one emissive triangle: the power mode falls back, the grid setting is accepted and
    stored, no grid is reported, and the film is the default's bit for bit."""
    s = loadScene(write_one_triangle_scene(tmp_path / "o"))
    assert len(s.lights) == 1
    base = RayTracer(s, seed=1234)
    base.render(3)
    rt = grid_on(s, 8, seed=1234)
    assert rt.light_grid()["cells"] == 8 and not rt.light_grid()["active"] and rt.light_grid_table() is None
    assert rt.light_table() is None
    rt.render(3)
    assert (base.film()[0] != 0).sum() > 100
    assert_same_bits(rt.film()[0], base.film()[0], "one light")


def test_the_setter_leaves_everything_else_alone(tmp_path):
    """rtg_set_light_grid waits for queued frames and then changes nothing but its own state: the film, the
    sample count, the statistics and every other setting are what they were."""
    s = loadScene(write_hall_scene(tmp_path / "h", 12, 33, 31))
    rt = RayTracer(s, seed=3, integrator="direct")
    rt.set_light_sampling("power", 0.25)
    rt.set_env_sampling("luminance")
    for _ in range(3):
        rt.render(1, sync=False)
    ref = RayTracer(s, seed=3, integrator="direct")
    ref.set_light_sampling("power", 0.25)
    for _ in range(3):
        ref.render(1, sync=False)
    before = (rt.light_sampling(), rt.env_sampling(), rt.material_model(), rt.path_mis(), rt.light_table()["entries"])
    rt.set_light_grid(8)  # (issues and waits for the three queued frames first)
    f, spp = rt.film()
    assert spp == 3
    assert_same_bits(f, ref.film()[0], "the film across the setter")
    st0, st1 = ref.stats(), rt.stats()
    assert st1["paths"] == st0["paths"] > 0 and st1["shadow_rays"] == st0["shadow_rays"]
    assert st1["extension_rays"] == st0["extension_rays"]
    after = (rt.light_sampling(), rt.env_sampling(), rt.material_model(), rt.path_mis(), rt.light_table()["entries"])
    assert before[:4] == after[:4] and np.array_equal(before[4], after[4])
    assert rt.light_sampling() == {"mode": "power", "uniform_share": 0.25}


# ---------------------------------------------------------------- 6. the command line
def test_cli_light_grid_writes_the_library_film(tmp_path):
    """-lightSampling power -lightGrid 8 on the 24-light hall: the file is Film::save of the library's film,
    for one device and for a group; without -lightGrid the file is another; a refused value is an error."""
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = write_hall_scene(tmp_path / "h", 12)
    s = loadScene(scene)
    rt = grid_on(s, 8, seed=1234)
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.film()[0], 3)
    base = [cli, "-scene", scene, "-SPP", "3", "-timeLimit", "0", "-outputFilename", "out.hdr", "-lightSampling", "power"]
    out = {}
    for d, extra in (("grid", ["-lightGrid", "8"]), ("power", []), ("group", ["-lightGrid", "8", "-devices", "0,0"])):
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[d] = (tmp_path / d / "out.hdr").read_bytes()
    assert out["grid"] == (tmp_path / "lib.hdr").read_bytes()
    assert out["group"] == out["grid"]
    assert out["power"] != out["grid"]
    r = subprocess.run(base + ["-lightGrid", "65"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "rtg_set_light_grid" in r.stderr
