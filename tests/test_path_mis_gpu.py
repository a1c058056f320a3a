"""Multiple importance sampling of emitters in the path tracer on the GPU (rtg_set_path_mis,
RTG_PATH_MIS_POWER): the kernels' own weight, environment density and triangle -> light map equal the numpy
restatement (tests/path_mis_ref.py) bit for bit; whole one-bounce films equal the restated sum bit for bit;
the film does not depend on how the render is cut; the default and everything the mode does not apply to
are left alone; where PATH is correct the two have the same expectation, and under an environment light
the mode agrees with the restatement's quadrature while PATH does not."""
import os
import subprocess

import numpy as np
import pytest

import env_sampling_ref as er
import light_sampling_ref as lr
import materials_ref as R
import path_mis_ref as M
from conftest import SCENES
from env_scenes import patch_map, smooth_map
from material_scenes import write_material_floor_scene
from path_mis_scenes import write_mis_floor_scene
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, probe_texture, save_hdr
from raytracingrenderer_amd import _native as N
from raytracingrenderer_amd.renderer import mis_weight_probe

pytestmark = pytest.mark.gpu

F = np.float32
LUM = np.array([0.2126, 0.7152, 0.0722])


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def params_of(p):
    return R.Params(p.model, p.alpha, p.sigma, tuple(p.eta), tuple(p.k), p.int_ior, p.ext_ior)


def tracer(s, seed, mis="power", power=False, luminance=False, physical=True, **kw):
    rt = RayTracer(s, seed=seed, **kw)
    rt.set_env_sampling("luminance" if luminance else "uniform")
    rt.set_light_sampling("power" if power else "uniform")
    rt.set_material_model("physical" if physical else "reference")
    rt.set_path_mis(mis)
    return rt


# ---------------------------------------------------------------- 1. the probes
def test_weight_probe_equals_the_restatement():
    p, q = M.weight_grid()
    got = mis_weight_probe(p, q)
    assert_same_bits(got, M.mis_w(p, q), "mis_w")
    assert_same_bits(got[(p == 0) & (q == 0)], [0.5], "both zero")
    assert_same_bits(got[np.isinf(p) & np.isinf(q)], [0.5], "both infinite")
    with pytest.raises(ValueError):
        mis_weight_probe(p, q[:-1])


@pytest.mark.parametrize("luminance", [False, True])
def test_env_pdf_probe_equals_the_restatement(tmp_path, luminance):
    """The kernel's own env_samples directions (in-cell draws in [0.25, 0.75]: the cell is the sampled one
    for every sample), the poles and the +x / -x seams, under both environment modes."""
    tex = patch_map(16, 8)
    s = loadScene(write_material_floor_scene(tmp_path / "e", "conductor", 33, 31, env=tex, emitters=False, cube=False))
    W, H = 16, 8
    rt = RayTracer(s, seed=1)
    rt.set_env_sampling("luminance")
    ent = rt.env_table()["entries"]
    rng = np.random.default_rng(5)
    n = 4096
    r0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    d = np.stack([rng.random(n), 0.25 + 0.5 * rng.random(n), 0.25 + 0.5 * rng.random(n)], axis=1).astype(F)
    wi, pdf = rt.env_samples(r0, d)
    wi_r, pdf_r, cell = er.sample(ent, W, H, r0, d)
    assert_same_bits(wi, wi_r, "env_samples")
    cx, cy = M.env_cell(W, H, wi)
    assert np.array_equal(cy * W + cx, cell)  # every sample: no exception
    edge = np.array([(0, 1, 0), (0, -1, 0), (-1, 0, 1e-3), (-1, 0, -1e-3), (-1, 0, 0), (1, 0, -1e-30), (1, 0, 0),
                     (1, 0, 1e-30), (0.6, 0.8, 0), (0, 0.6, -0.8)], F)
    dirs = np.concatenate([wi, edge])
    rt.set_env_sampling("luminance" if luminance else "uniform")
    got = rt.env_pdf(dirs)
    want = M.env_pdf(ent if luminance else None, W, H, dirs)
    assert_same_bits(got, want, "p_env")
    if luminance:
        assert got[n] == 0 and got[n + 1] == 0 and (got[n + 2:] > 0).all()
        rel = np.abs(got[:n].astype(np.float64) - pdf) / pdf
        assert rel.max() <= 8 * 2.0 ** -24, rel.max()  # the sampler's own density (tests/test_path_mis.py)
    else:
        assert (got == M.UNIFORM_SPHERE_PDF).all()


def test_light_of_triangle_is_the_inverse_of_the_light_list(tmp_path):
    s = loadScene(write_mis_floor_scene(tmp_path / "m", "conductor", 33, 31, env=smooth_map(16, 8)))
    lights = np.array(s.lights)
    assert len(lights) == 25 and (lights == -1).sum() == 1
    rt = RayTracer(s, seed=1)
    with pytest.raises(NativeError):
        rt.light_of_triangle()  # the map is built by the first "power" setting
    rt.set_path_mis("power")
    lof = rt.light_of_triangle()
    want = np.full(s.desc.n_tris, -1, np.int32)
    for i, t in enumerate(lights):
        if t >= 0 and want[t] < 0:
            want[t] = i
    assert np.array_equal(lof, want) and (lof >= 0).sum() == 24


# ---------------------------------------------------------------- 2. exact films
def film_ref(s, rt, ns, seed, power=False, luminance=False, counts=None):
    """The PATH + MIS film of ns samples at max_depth 0 (one bounce), rebuilt in numpy from include/rtg.h's
    text as tests/test_materials_gpu.py's film_ref rebuilds DIRECT: per sample the weighted NEE term of the
    first hit, then Russian roulette (thr = 1: survival below 0.9f, thr = 1 / 0.9f), the BSDF sample, its ray
    through trace_closest, and the weighted emitter or miss term; every other second term is thr * 0 (the
    cube is black). From the restated PCG stream, light_records(), light_of_triangle(), the tables' host
    copies, the NORMALS film, trace_closest and trace_visible. counts (a dict) gains the number of samples
    that took the weighted emitter-hit, the back-side and the weighted environment-miss branch."""
    W, H = s.width, s.height
    rec = rt.light_records()
    nl = len(rec)
    ent = rt.light_table()["entries"] if power else None
    kind = rec[:, 7].copy().view(np.int32)
    has_env = (kind == 1).any()
    env_li = int(np.flatnonzero(kind == 1)[0]) if has_env else -1
    tex = s.texture(s.desc.env_texture).copy() if s.desc.env_texture >= 0 else None
    eent = rt.env_table()["entries"] if luminance else None
    EW, EH = (tex.shape[1], tex.shape[0]) if tex is not None else (1, 1)
    lof = rt.light_of_triangle()
    physical = rt.material_model() == "physical"
    guide = RayTracer(s, seed=seed, integrator="normals")
    guide.render(1)
    sn = guide.film()[0].reshape(-1, 3)
    n = W * H
    pix = np.arange(n, dtype=np.uint32)
    rays, _ = rt.camera_samples(pix, np.zeros(n, np.uint32))
    hits = rt.trace_closest(rays)
    hit = hits[:, 0] < F(3.0e38)
    tri = np.where(hit, hits[:, 1].copy().view(np.int32), 0)
    mat = s.material_index[tri]
    mats, par = s.materials, s.material_params
    em_of = np.array([m.emission[:] for m in mats], F)
    al, be = hits[:, 2], hits[:, 3]
    ga = F(1) - (al + be)
    uv = s.uvs[tri]
    tu = (uv[:, 0, 0] * al + uv[:, 1, 0] * be) + uv[:, 2, 0] * ga
    tv = (uv[:, 0, 1] * al + uv[:, 1, 1] * be) + uv[:, 2, 1] * ga
    alb = np.zeros((n, 3), F)
    old = np.seterr(all="ignore")  # (a missed pixel's t = FLT_MAX runs through the arithmetic unused)
    for m in np.unique(mat[hit]):
        sel = hit & (mat == m)
        alb[sel] = er.bilinear(s.texture(mats[m].texture), tu[sel], tv[sel])
    emitter = hit & (em_of[mat].sum(1) > 0)
    surf = hit & ~emitter
    lit = surf & (alb.sum(1) > 0)  # the floor (the NORMALS film's |sN| is sN itself there); the cube is black
    assert (sn[lit][:, 1] > 0.99).all()
    x = rays[:, 0:3] + rays[:, 4:7] * hits[:, 0:1]  # Ray::at
    E0 = probe_texture(tex, rays[:, 4:7], env=True) if tex is not None else np.zeros((n, 3), F)
    pmf_u = F(1) / F(nl)
    film = np.zeros((n, 3), F)
    tally = dict(emitter=0, back=0, env_miss=0, nee=0)
    for sl in range(ns):
        st = er.PathStream(pix, np.full(n, sl, np.uint32), seed)
        if power:
            li, pmf = lr.pick(ent, st.raw(), st.next())
        else:
            li = np.minimum((F(nl) * st.next()).astype(np.int64), nl - 1)
            pmf = np.full(n, pmf_u, F)
        L = rec[li]
        a_raw = st.raw()
        a = (a_raw >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)
        b = st.next()
        p2 = lr.triangle_sample(L, a, b)
        g, _ = lr.area_geometry(L, p2, x, sn)
        wr = p2 - x
        l2 = lr.dot3(wr, wr)
        cb = -lr.dot3(lr.normalize3(wr), L[:, 12:15])
        cos_l = np.where(cb > 0, cb, F(0)).astype(F)
        emitted = L[:, 16:19]
        pdf = L[:, 11]
        isenv = kind[li] == 1
        if has_env:
            if luminance:  # r0 = a's raw step, then d1, d2, d3: the two further draws are the environment's alone
                keep = st.s.copy()
                d = np.stack([b, st.next(), st.next()], axis=1)
                st.s = np.where(isenv, st.s, keep)
                wi, epdf, _ = er.sample(eent, EW, EH, a_raw, d)
            else:          # uniformSampleSphere(q1, q2): q2 is the first draw
                wi, epdf = er.uniform_sample(b, a)
                epdf = np.full(n, epdf, F)
            ge = lr.dot3(wi, sn)
            ge = np.where((ge > 0) & (epdf > 0), ge, F(0)).astype(F)
            E = probe_texture(tex, wi, env=True)
            p2 = np.where(isenv[:, None], x + wi * F(10000.0), p2).astype(F)
            g = np.where(isenv, ge, g).astype(F)
            emitted = np.where(isenv[:, None], E, emitted).astype(F)
            pdf = np.where(isenv, epdf, pdf).astype(F)
        act = surf & (g > 0)
        q = lr.shadow_ray(x, p2)
        sd = q[:, 4:7].copy()
        f = R.div_pi_f(alb)
        p_b = np.zeros(n, F)
        for m in np.unique(mat[surf]):
            sel = surf & (mat == m)
            fr = R.frame_from(sn[sel])
            if physical and par[m].model != N.RTG_MODEL_REFERENCE:
                wo = R.to_local(fr, R.vec(-rays[sel, 4:7]))
                sdl = R.to_local(fr, R.vec(sd[sel]))
                f[sel] = R.evaluate(params_of(par[m]), R.vec(alb[sel]), wo, sdl)
                p_b[sel] = R.pdf(params_of(par[m]), wo, sdl)
            else:
                p_b[sel] = M.bsdf_pdf_lambert(fr[2], sd[sel])
        ld = (((f * emitted) * g[:, None]) / (pmf * pdf)[:, None]).astype(F)
        w_l, _ = M.nee_weight(pmf, pdf, l2, cos_l, isenv, p_b)
        ld = (ld * w_l[:, None]).astype(F)
        q[~act] = (0, 1e6, 0, 1, 0, 1, 0, 0)  # (unused lanes: a ray far above everything)
        vis = rt.trace_visible(q) != 0
        tally["nee"] += int((lit & act & vis & (ld.sum(1) > 0)).sum())
        c = np.where((act & vis)[:, None], ld, F(0)).astype(F)
        c = np.where(emitter[:, None], em_of[mat], c).astype(F)
        c = np.where(hit[:, None], c, E0).astype(F)
        # ---- the bounce
        cont = st.next() < F(0.9)  # wmin(Lum(1, 1, 1), 0.9f)
        thr0 = F(1) / F(0.9)
        dr = np.stack([st.next(), st.next(), st.next()], axis=1)
        c1 = np.zeros((n, 3), F)
        for m in np.unique(mat[surf]):
            sel = np.flatnonzero(surf & (mat == m))
            fr = R.frame_from(sn[sel])
            if physical and par[m].model != N.RTG_MODEL_REFERENCE:
                smp = R.sample(params_of(par[m]), R.vec(alb[sel]), R.to_local(fr, R.vec(-rays[sel, 4:7])), dr[sel])
                wi, col, pb, delta = R.arr(R.to_world(fr, smp["wi"])), smp["colour"], smp["pdf"], smp["delta"]
                live = pb > 0
            else:
                assert mats[m].kind in (N.RTG_MAT_DIFFUSE, N.RTG_MAT_LAMBERT)
                wiw, col, pb = M.lambert_sample(mats[m].kind, alb[sel], fr, dr[sel, 0], dr[sel, 1])
                wi, delta, live = R.arr(wiw), np.zeros(len(sel), bool), pb > 0
            go = cont[sel] & live
            cosn = np.abs(lr.dot3(wi, sn[sel]))
            thr = np.where(delta[:, None], (thr0 * col) / pb[:, None], ((thr0 * col) * cosn[:, None]) / pb[:, None]).astype(F)
            br = np.zeros((len(sel), 8), F)
            br[:, 0:3], br[:, 4:7] = x[sel] + wi * F(1e-4), wi
            br[~go] = (0, 1e6, 0, 0, 0, 1, 0, 0)  # (unused lanes: a ray that leaves the scene)
            bh = rt.trace_closest(br)
            bhit = bh[:, 0] < F(3.0e38)
            btri = np.where(bhit, bh[:, 1].copy().view(np.int32), 0)
            em = em_of[s.material_index[btri]]
            isem = go & bhit & (em.sum(1) > 0)
            # an emitter hit: thr emission, weighted after a non-specular sample
            lh = lof[btri]
            Lh = rec[np.maximum(lh, 0)]
            ch = -lr.dot3(wi, Lh[:, 12:15])
            cos_h = np.where(ch > 0, ch, F(0)).astype(F)
            pmf_h = ent[np.maximum(lh, 0), 2].copy().view(F) if power else np.full(len(sel), pmf_u, F)
            p_l = M.pdf_area_to_solid(pmf_h * Lh[:, 11], bh[:, 0] * bh[:, 0], cos_h)
            base = (thr * em).astype(F)
            front = (base * M.mis_w(pb, p_l)[:, None]).astype(F)
            ce = np.where((delta | (lh < 0))[:, None], base, np.where((cos_h > 0)[:, None], front, F(0))).astype(F)
            tally["emitter"] += int((lit[sel] & isem & ~delta & (lh >= 0) & (cos_h > 0)).sum())
            tally["back"] += int((lit[sel] & isem & ~delta & (lh >= 0) & ~(cos_h > 0)).sum())
            # a miss: thr E, weighted after a non-specular sample when the environment is a light
            ismiss = go & ~bhit
            cm = np.zeros((len(sel), 3), F)
            if tex is not None:
                cm = (thr * probe_texture(tex, wi, env=True)).astype(F)
                if env_li >= 0:
                    pmf_e = ent[env_li, 2:3].copy().view(F)[0] if power else pmf_u
                    w_e = M.mis_w(pb, pmf_e * M.env_pdf(eent, EW, EH, wi))
                    cm = np.where(delta[:, None], cm, cm * w_e[:, None]).astype(F)
                    tally["env_miss"] += int((lit[sel] & ismiss & ~delta).sum())
            c1[sel] = np.where(isem[:, None], ce, np.where(ismiss[:, None], cm, F(0)))
            assert np.isfinite(thr[go]).all()  # (thr * 0 is +0 only for a finite thr)
        film = film + (c + c1).astype(F)
    np.seterr(**old)
    if counts is not None:
        counts.update(tally)
    return film.reshape(H, W, 3)


def check_film(s, seed, power=False, luminance=False, physical=True, need=("emitter", "back", "nee"), ns=4):
    rt = tracer(s, seed, power=power, luminance=luminance, physical=physical, max_depth=0)
    assert rt.path_mis() == "power"
    counts = {}
    want = film_ref(s, rt, ns, seed, power, luminance, counts)
    print("branch counts: %r" % counts)
    for k in need:
        assert counts[k] > 0, (k, counts)
    rt.render(ns)
    got = rt.film()[0]
    assert_same_bits(got, want, "PATH + MIS")
    off = tracer(s, seed, "off", power=power, luminance=luminance, physical=physical, max_depth=0)
    off.render(ns)
    assert not np.array_equal(bits(off.film()[0]), bits(got))
    return rt, want


@pytest.mark.parametrize("power", [False, True])
@pytest.mark.parametrize("floor", ["conductor", "plastic", "plastic-delta", "orennayar", "reference"])
def test_one_bounce_films_are_the_restated_sum(tmp_path, floor, power):
    """The "unequal" scene plus an emitter that faces up, 64 x 48, 4 spp, max_depth 0, each floor under the
    uniform and the power pick. "reference": the conductor floor under the reference material model, a
    cosine-sampled Lambertian, through the same kernels."""
    name = "conductor" if floor == "reference" else floor
    s = loadScene(write_mis_floor_scene(tmp_path / "m", name, 64, 48, back=(floor == "plastic-delta")))
    assert len(s.lights) == (26 if floor == "plastic-delta" else 24) and s.desc.env_texture < 0
    check_film(s, 77, power, physical=(floor != "reference"))


@pytest.mark.parametrize("luminance", [False, True])
@pytest.mark.parametrize("power", [False, True])
def test_one_bounce_film_with_the_environment_in_the_light_list(tmp_path, power, luminance):
    """The same scene under a smooth 16 x 8 environment map that is in the light list (25 lights), under
    both environment modes and both picks: a BSDF ray that leaves the scene takes the weighted miss branch."""
    s = loadScene(write_mis_floor_scene(tmp_path / "e", "conductor", 64, 48, env=smooth_map(16, 8)))
    assert len(s.lights) == 25 and (np.array(s.lights) == -1).sum() == 1
    check_film(s, 78, power, luminance, need=("emitter", "back", "env_miss", "nee"))


@pytest.mark.parametrize("power", [False, True])
def test_one_bounce_film_with_the_tables_in_global_memory(tmp_path, power):
    """13 more emitters: 50 lights, past RTG_LDS_LIGHTS, so k_shade_mis<false> reads every table, the hit
    light's record and its pmf from global memory."""
    s = loadScene(write_mis_floor_scene(tmp_path / "g", "plastic", 64, 48, extra=13))
    assert len(s.lights) == 50
    check_film(s, 79, power)


# ---------------------------------------------------------------- 3. cuts
@pytest.mark.parametrize("power", [False, True])
def test_film_does_not_depend_on_how_the_render_is_cut(tmp_path, power):
    """The rough-conductor MIS film of 4 samples from four 1-spp calls, queued frames, two complementary
    tile sets and a two-rank group; the adaptive render is repeatable."""
    s = loadScene(write_mis_floor_scene(tmp_path / "m", "conductor", 64, 48))
    rt = tracer(s, 77, power=power, max_depth=4)
    rt.render(4)
    want = rt.film()[0]
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
        rt.render(4, tiles=part, first_sample=0)
    assert_same_bits(rt.film()[0], want, "two complementary tile sets")
    g = RayTracerGroup(s, devices=(0, 0), seed=77)
    g.set_options(max_depth=4)
    g.set_light_sampling("power" if power else "uniform")
    g.set_material_model("physical")
    g.set_path_mis("power")
    g.render(4)
    assert_same_bits(g.film()[0], want, "two-rank group on device 0 twice")
    films = []
    for _ in range(2):
        rt.clear()
        rt.adaptiveRender(init_samples=2, max_samples=8, min_samples=1, first_sample=0)
        films.append(rt.film()[0])
    assert_same_bits(films[1], films[0], "adaptive render")
    assert (films[0] != 0).sum() > 100


# ---------------------------------------------------------------- 4. what must not move
def test_off_after_power_is_the_never_set_film():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=64, height=48)
    never = RayTracer(s, seed=11)
    never.render(3)
    rt = RayTracer(s, seed=11)
    assert rt.path_mis() == "off"
    rt.set_path_mis("power")
    rt.render(3)
    assert not np.array_equal(bits(rt.film()[0]), bits(never.film()[0]))
    rt.set_path_mis("off")
    rt.clear()
    rt.render(3)
    assert_same_bits(rt.film()[0], never.film()[0], "power, then off")


def test_what_the_mode_must_leave_alone():
    """DIRECT, DIRECT_MIS, ALBEDO, NORMALS, the light tracer, instant radiosity and the denoiser's guides
    give the same films on cornell-mat with the mode on (under the physical model, which DIRECT follows)."""
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=64, height=48)

    def run(what, mis):
        rt = RayTracer(s, seed=5, max_paths=64 * 48 * 7, integrator=what if what in RayTracer.INTEGRATORS else "path")
        rt.set_material_model("physical")
        rt.set_path_mis(mis)
        if what == "light tracer":
            rt.lightTracer(2, first_frame=0)
        elif what == "instant radiosity":
            rt.instantRadiosity(2, n_vpl=20, first_frame=0)
        elif what == "guides":
            return np.concatenate(rt.guides())
        else:
            rt.render(2)
        return rt.film()[0]

    for what in ("direct", "direct_mis", "albedo", "normals", "light tracer", "instant radiosity", "guides"):
        a, b = run(what, "off"), run(what, "power")
        assert (a != 0).sum() > 100, what
        assert_same_bits(b, a, what)
    assert not np.array_equal(bits(run("path", "off")), bits(run("path", "power")))


def test_setter_errors_keep_the_setting_and_the_film(tmp_path):
    import ctypes as C
    s = loadScene(write_mis_floor_scene(tmp_path / "m", "plastic", 33, 31))
    lib = N.rtg()
    rt = tracer(s, 9)
    rt.render(2)
    want = rt.film()[0]
    for mode in (2, -1):
        with pytest.raises(NativeError):
            rt.set_path_mis(mode)
    with pytest.raises(ValueError):
        rt.set_path_mis("balance")
    assert lib.rtg_set_path_mis(None, 1) == -1 and lib.rtg_get_path_mis(rt.handle, None) == -1
    assert rt.path_mis() == "power"
    rt.clear()
    rt.render(2)
    assert_same_bits(rt.film()[0], want, "after the rejected settings")
    g = RayTracerGroup(s, devices=(0, 0))
    with pytest.raises(NativeError):
        g.set_path_mis(3)
    m = C.c_int(-1)
    assert lib.rtg_get_path_mis(lib.rtg_group_handle(g._g, 1), C.byref(m)) == 0 and m.value == 0


def test_changing_the_material_parameters_keeps_the_map(tmp_path):
    """The device table holds the triangle's parameter index beside its light: it follows a later
    rtg_set_material_params / model change, in either order of the settings."""
    s = loadScene(write_mis_floor_scene(tmp_path / "m", "plastic", 33, 31))
    a = tracer(s, 21)  # the model first, then the mode
    a.render(2)
    b = RayTracer(s, seed=21)
    b.set_path_mis("power")  # the mode first: the table is rebuilt when the model builds its index
    b.render(1)
    b.clear()
    b.set_material_model("physical")
    b.render(2)
    assert_same_bits(b.film()[0], a.film()[0], "mode, then model")
    b.set_material_model("reference")
    b.clear()
    b.render(2)
    c = tracer(s, 21, physical=False)
    c.render(2)
    assert_same_bits(b.film()[0], c.film()[0], "back to the reference model")
    assert not np.array_equal(bits(c.film()[0]), bits(a.film()[0]))


def test_cli_path_mis_writes_the_library_film(tmp_path):
    """-pathMIS power on the conductor floor: the file is Film::save of the library's film, for one device
    and for a two-rank group; without the option the file is another; an unknown name is an error."""
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = write_mis_floor_scene(tmp_path / "m", "conductor")
    s = loadScene(scene)
    rt = tracer(s, 1234)
    rt.render(3)
    save_hdr(str(tmp_path / "lib.hdr"), rt.film()[0], 3)
    base = [cli, "-scene", scene, "-SPP", "3", "-timeLimit", "0", "-outputFilename", "out.hdr", "-materials", "physical"]
    out = {}
    for d, extra in (("power", ["-pathMIS", "power"]), ("off", []), ("group", ["-pathMIS", "power", "-devices", "0,0"])):
        (tmp_path / d).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / d), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[d] = (tmp_path / d / "out.hdr").read_bytes()
    assert out["power"] == (tmp_path / "lib.hdr").read_bytes()
    assert out["group"] == out["power"]
    assert out["off"] != out["power"]
    r = subprocess.run(base + ["-pathMIS", "balance"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "pathMIS" in r.stderr


# ---------------------------------------------------------------- 5. expectation
K_REPLICATES, N_SPP = 16, 32


@pytest.mark.parametrize("scene", ["cornell-box", "conductor floor"])
def test_same_expectation_as_path_without_an_environment_light(tmp_path, scene):
    """No environment light, every emissive triangle in the light list: PATH and PATH + MIS estimate the same
    integral. K = 16 independent seeds of N = 32 spp each at 32 x 24, depth 4, per mode (the two sets use
    different seeds, so they are independent): the sets' film means differ by at most 4 standard errors of
    the difference, the standard errors from the K replicates of each set.
    Measured on an MI355X: cornell-box 0.050883 against 0.050817 (0.56 standard errors), the conductor floor
    0.051801 against 0.051615 (0.92)."""
    if scene == "cornell-box":
        s = loadScene(os.path.join(SCENES, "cornell-box"), width=32, height=24)
    else:
        s = loadScene(write_material_floor_scene(tmp_path / "m", "conductor", 32, 24))
    assert s.desc.env_texture < 0
    means = {}
    for mis, seed0 in (("off", 1000), ("power", 2000)):
        rt = tracer(s, seed0, mis, max_depth=4)
        vals = []
        for k in range(K_REPLICATES):
            rt.seed = seed0 + k
            rt.clear()
            rt.render(N_SPP)
            vals.append(float(rt.film()[0].astype(np.float64).mean() / N_SPP))
        means[mis] = np.array(vals)
    a, b = means["off"], means["power"]
    se = np.sqrt(a.var(ddof=1) / K_REPLICATES + b.var(ddof=1) / K_REPLICATES)
    diff = abs(a.mean() - b.mean())
    print("%s: PATH %.6f (sd %.3g) MIS %.6f (sd %.3g) difference %.3g = %.2f se"
          % (scene, a.mean(), a.std(ddof=1), b.mean(), b.std(ddof=1), diff, diff / se))
    assert diff <= 4 * se, (a.mean(), b.mean(), se)
    same = tracer(s, 1000, "power", max_depth=4)
    same.render(N_SPP)
    ref = tracer(s, 1000, "off", max_depth=4)
    ref.render(N_SPP)
    assert not np.array_equal(bits(same.film()[0]), bits(ref.film()[0]))  # the mode did something


@pytest.mark.parametrize("env_case", ["constant", "patch"])
def test_mean_under_an_environment_light_agrees_with_the_quadrature(tmp_path, env_case):
    """The rough-conductor floor alone under an environment map that is the only light: a constant map
    under the uniform mode, and patch_map (the 50 x patch) under luminance. One pixel, N = 16384 samples.
    A BSDF ray from the floor always leaves the scene, so the pixel's radiance is the integral of f E cos
    over the hemisphere. The estimator is X = A + B: A = f E cos w_l / p_l for a direction drawn with p_l,
    B = (f E cos w_b / p_b) / 0.9f with probability 0.9 (Russian roulette at thr = 1) for a direction drawn
    with p_b, independent; its mean and second moment come from the restatement by quadrature, and the
    margin is four standard errors sqrt(Var X / N). The default PATH misses the same quadrature by more
    than that margin: it adds E(wi) unweighted for every BSDF sample that leaves the scene.
    Measured on an MI355X: constant map, mean 0.278927 against 0.278779, 0.10 standard errors (PATH 0.806427,
    342); patch map, 0.516756 against 0.518404, 0.58 (PATH 1.543436, 362)."""
    n_s = 16384
    if env_case == "constant":
        env, luminance = np.full((8, 16, 3), (1.0, 0.75, 0.5), F), False
    else:
        env, luminance = patch_map(), True
    s = loadScene(write_material_floor_scene(tmp_path / "c", "conductor", 64, 48, env=env, emitters=False, cube=False))
    assert len(s.lights) == 1 and s.lights[0] == -1
    tex = s.texture(s.desc.env_texture).copy()
    EH, EW = tex.shape[:2]
    px = (s.height // 2) * s.width + s.width // 2
    got = {}
    for mis in ("power", "off"):
        rt = tracer(s, 5, mis, luminance=luminance, max_depth=4)
        tile = (s.height // 2 // 32) * rt.tiles_x + (s.width // 2 // 32)
        rt.render(n_s, tiles=[tile], first_sample=0)
        got[mis] = float((rt.film()[0].reshape(-1, 3)[px].astype(np.float64) / n_s) @ LUM)
    eent = rt.env_table()["entries"] if luminance else None
    rays, _ = rt.camera_samples([px], [0])
    assert rt.trace_closest(rays)[0, 0] < 3e38
    fr = R.frame_from((0.0, 1.0, 0.0))
    wo1 = R.to_local(fr, R.vec(-rays[:, 4:7]))
    q = params_of([p for p in s.material_params if p.model == N.RTG_MODEL_CONDUCTOR][0])
    alb = s.texture(s.materials[0].texture)[0, 0]

    def moments(nq):
        th = (np.arange(nq) + 0.5) * (0.5 * np.pi / nq)
        ph = (np.arange(2 * nq) + 0.5) * (np.pi / nq)
        T, P = [a.reshape(-1) for a in np.meshgrid(th, ph, indexing="ij")]
        wi = [(np.sin(T) * np.cos(P)).astype(F), (np.sin(T) * np.sin(P)).astype(F), np.cos(T).astype(F)]
        wo = [np.full(len(T), c[0], F) for c in wo1]
        ww = R.arr(R.to_world(fr, wi))
        E = er.env_eval(tex, ww).astype(np.float64)
        v = (R.evaluate(q, alb, wo, wi).astype(np.float64) * E) @ LUM * np.cos(T)
        p_b = R.pdf(q, wo, wi)
        p_l = M.env_pdf(eent, EW, EH, ww)  # pmf = 1: the environment is the only light
        w_l, w_b = M.mis_w(p_l, p_b).astype(np.float64), M.mis_w(p_b, p_l).astype(np.float64)
        dw = np.sin(T) * (0.5 * np.pi / nq) * (np.pi / nq)
        with np.errstate(divide="ignore", invalid="ignore"):
            a2 = np.where(p_l > 0, (v * w_l) ** 2 / p_l, 0.0)
            b2 = np.where(p_b > 0, (v * w_b) ** 2 / p_b, 0.0)
        ea, eb = float(np.sum(v * w_l * dw)), float(np.sum(v * w_b * dw))
        rr = float(F(0.9))
        var = (float(np.sum(a2 * dw)) - ea * ea) + (float(np.sum(b2 * dw)) / rr - eb * eb)
        return float(np.sum(v * dw)), ea + eb, var

    (i1, m1, v1), (i2, m2, v2) = moments(384), moments(768)
    assert abs(i2 - i1) <= 2e-3 * i2 and abs(v2 - v1) <= 3e-2 * v2, (i1, i2, v1, v2)  # the quadrature has converged
    assert abs(m2 - i2) <= 1e-5 * i2  # the weights of a pair sum to one
    se = np.sqrt(max(v2, 0.0) / n_s)
    dev, dev_off = abs(got["power"] - i2), abs(got["off"] - i2)
    print("%s: MIS mean %.6f PATH mean %.6f quadrature %.6f standard error %.3g: MIS %.2f se, PATH %.1f se"
          % (env_case, got["power"], got["off"], i2, se, dev / se, dev_off / se))
    assert dev <= 4 * se, (got["power"], i2, se)
    assert dev_off > 4 * se, (got["off"], i2, se)  # the departure from Renderer.h:390
