"""Variance-guided filtering of the temporal history on the GPU (rtg_svgf_accumulate) against its numpy
restatement (tests/svgf_ref.py) bit for bit, every pixel: output, variance, moments and the shared history.
The restatement's geometry guides come from the C oracle (as in tests/test_temporal_gpu.py), its albedo and
shading-normal guides from rt.guides() (pinned against the oracle in tests/test_denoise_gpu.py), the films it
blends are the GPU's own. rt.guides() is read after svgf(), so the call under test renders the dropped guides
itself, inside its chain."""
import os

import numpy as np
import pytest

import svgf_ref as sr
import temporal_ref as tr
from conftest import SCENES
from raytracingrenderer_amd import NativeError, RayTracer, loadScene, write_synthetic_scene
from test_temporal_gpu import SIZES, SPPS, assert_same_bits, oracle_guide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene_dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("syn20k")
    return {"cornell-box": os.path.join(SCENES, "cornell-box"),
            "syn20k": write_synthetic_scene(str(d), n_tris=20000, seed=7, width=64, height=48),  # test_temporal_gpu's
            "cornell-mat": os.path.join(SCENES, "cornell-mat")}


def frame(rt, s, pose, spp, planted=None):
    """Move, clear, render (or load `planted`): the posed scene and the film."""
    ps = tr.posed(s, pose)
    rt.set_camera(ps.desc.camera, ps.desc.projection)
    rt.clear()
    if planted is None:
        rt.render(spp, first_sample=0)
    else:
        rt.load_film(planted, spp)
    film, got = rt.film()
    assert got == spp
    return ps, film


def check(rt, ref, ps, film, spp, key, what, nan_equal=False, **kw):
    """One svgf() call against the restatement: output, variance, moments, history."""
    out = rt.svgf(**kw)
    alb, nrm = rt.guides()
    want = ref.accumulate(film, spp, ps.desc.camera, ps.desc.projection, lambda: oracle_guide(ps, key), alb, nrm, **kw)
    assert_same_bits(rt.temporal_history(), ref.t.H, what + ": history", nan_equal)
    assert_same_bits(rt.svgf_moments(), ref.M, what + ": moments", nan_equal)
    assert_same_bits(rt.svgf_variance(), ref.var, what + ": variance", nan_equal)
    assert_same_bits(out, want, what + ": output", nan_equal)
    return out


def play(rt, s, name, size, steps, ref, spps, **kw):
    seen = [0, 0]
    for (label, pose), spp in zip(steps, spps):
        ps, film = frame(rt, s, pose, spp)
        check(rt, ref, ps, film, spp, (name, size, label), "%s %s %s %s" % (name, size, label, kw), **kw)
        seen[0] += int(ref.spatial.sum())
        seen[1] += int((~ref.spatial).sum())
    return seen


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["cornell-box", "cornell-mat", "syn20k"])
def test_sequence_equals_the_restatement(scene_dirs, name, size):
    """first call, unchanged camera, small move, dolly-in, 90 degree turn, looking away at 2, 1, 1, 3, 1, 2 spp,
    then the whole sequence again after temporal_reset(): the three modes of the temporal step, the spatial
    variance on the first frame and on disocclusions, the temporal one once len >= 4 (len is 2, 3, then up to
    4 after the small move and 7 after the dolly-in where the history holds). Both branches must occur."""
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    steps = tr.move_sequence(s)
    for call in (rt.svgf_variance, rt.svgf_moments, rt.svgf):
        with pytest.raises(NativeError):
            call()  # nothing accumulated yet; spp == 0
    for _ in range(2):
        spatial, temporal = play(rt, s, name, size, steps, sr.SvgfRef(), SPPS)
        assert spatial > 0 and temporal > 0, (spatial, temporal)
        rt.temporal_reset()
        with pytest.raises(NativeError):
            rt.svgf_variance()


CASES = [dict(iterations=1), dict(iterations=8), dict(normal_squarings=0), dict(sigma_albedo=0.0),
         dict(sigma_luminance=0.5), dict(min_history=1.0), dict(min_history=1e9), dict(variance_floor=1.0),
         dict(plane_tolerance=0.0), dict(normal_cos=1.0), dict(max_history=2.0)]


@pytest.mark.parametrize("kw", CASES, ids=str)
def test_parameters_equal_the_restatement(scene_dirs, kw):
    name, size = "cornell-box", (64, 48)
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    steps = tr.move_sequence(s)
    steps = steps[:2] + steps[1:2] * 3 + steps[2:4]  # five frames at A (len reaches 5), small move, dolly-in
    ref = sr.SvgfRef()
    spatial, temporal = play(rt, s, name, size, steps, ref, [1] * len(steps), **kw)
    if kw.get("min_history") == 1.0:
        assert spatial == 0  # len >= 1 holds from the first frame on: the 7x7 branch is never taken
    if kw.get("min_history") == 1e9:
        assert temporal == 0  # ... and here always


def test_the_history_is_the_temporal_call_s(scene_dirs):
    """Two handles, the same frames, one through svgf() and one through temporal(): the same history bits, a
    different picture."""
    s = loadScene(scene_dirs["cornell-mat"], width=33, height=31)
    a, b = RayTracer(s, seed=1234), RayTracer(s, seed=1234)
    differ = 0
    for (label, pose), spp in zip(tr.move_sequence(s), SPPS):
        outs = []
        for rt in (a, b):
            frame(rt, s, pose, spp)
            outs.append(rt.svgf() if rt is a else rt.temporal())
        assert_same_bits(a.temporal_history(), b.temporal_history(), label + ": history")
        differ += int(not np.array_equal(outs[0], outs[1]))
    assert differ >= 3


def test_mixing_with_temporal_restarts_the_moments(scene_dirs):
    """svgf, temporal, svgf: the restatement with M restarted at the third call. Afterwards denoise() is a
    fresh handle's at that pose, and temporal() continues the shared history."""
    name, size = "cornell-box", (64, 48)
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    ref = sr.SvgfRef()
    steps = tr.move_sequence(s)
    (l0, p0), (l1, p1), (l2, p2) = steps[0], steps[1], steps[2]
    ps, film = frame(rt, s, p0, 1)
    check(rt, ref, ps, film, 1, (name, size, l0), "svgf 1")
    ps, film = frame(rt, s, p1, 1)
    out = rt.temporal()
    want = ref.temporal(film, 1, ps.desc.camera, ps.desc.projection, lambda: oracle_guide(ps, (name, size, l1)))
    assert_same_bits(out, want, "temporal in between")
    with pytest.raises(NativeError):
        rt.svgf_moments()  # dropped
    ps, film = frame(rt, s, p2, 1)
    check(rt, ref, ps, film, 1, (name, size, l2), "svgf 2")
    cur = film / np.float32(1)
    assert_same_bits(rt.svgf_moments()[..., 0], sr.lum32(cur), "restarted moments")
    fresh = RayTracer(ps, seed=1234)
    fresh.render(1, first_sample=0)
    assert_same_bits(fresh.film()[0], film, "a fresh handle at that pose renders the same film")
    assert_same_bits(rt.denoise(), fresh.denoise(), "denoise after svgf")
    out = rt.temporal()
    want = ref.temporal(film, 1, ps.desc.camera, ps.desc.projection, lambda: oracle_guide(ps, (name, size, l2)))
    assert_same_bits(out, want, "temporal continues the shared history")
    assert_same_bits(rt.temporal_history(), ref.t.H, "history")


def test_non_finite_pixels_follow_the_definition(scene_dirs):
    """One NaN and one +inf pixel planted through load_film on a wall: they spread through the filter's taps
    and, after the small move, through the reprojection's, exactly as the restatement says."""
    name, size = "cornell-box", (64, 48)
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    ref = sr.SvgfRef()
    steps = tr.move_sequence(s)
    rt.render(1)
    film = rt.film()[0]
    film[24, 20, 1] = np.nan
    film[30, 40, :] = np.inf
    nonfinite = []
    for (label, pose), planted in [(steps[0], film), (steps[1], None), (steps[2], None), (steps[3], None)]:
        ps, f = frame(rt, s, pose, 1, planted)
        out = check(rt, ref, ps, f, 1, (name, size, label), label, nan_equal=True)
        nonfinite.append(int((~np.isfinite(out)).any(axis=2).sum()))
    assert nonfinite[0] >= 2, nonfinite


def test_the_handle_is_left_as_it_was(scene_dirs):
    s = loadScene(scene_dirs["cornell-box"], width=64, height=48)
    rt = RayTracer(s, seed=1234, integrator="direct", max_depth=3)
    rt.set_options(flags=rt.flags | 2)  # RTG_OPT_COUNT
    rt.set_camera_sampling("box", 0.5)
    rt.render(2)
    film, spp = rt.film()
    st = rt.stats()
    a = rt.svgf()
    hist, var, mom = rt.temporal_history(), rt.svgf_variance(), rt.svgf_moments()
    for kw in (dict(iterations=0), dict(sigma_luminance=np.nan), dict(min_history=0.0), dict(normal_cos=2.0)):
        with pytest.raises(NativeError):
            rt.svgf(**kw)
    assert_same_bits(rt.temporal_history(), hist, "history after refused calls")
    assert_same_bits(rt.svgf_variance(), var, "variance after refused calls")
    assert_same_bits(rt.svgf_moments(), mom, "moments after refused calls")
    small = tr.posed(s, dict(tr.move_sequence(s))["small move"])
    rt.set_camera(small.desc.camera, small.desc.projection)
    b = rt.svgf()  # a moved call: guide pass, guides, reprojection
    f2, spp2 = rt.film()
    assert_same_bits(f2, film, "film")
    assert spp2 == spp == 2
    st2 = rt.stats()
    for k in st:
        if not k.endswith("_ms"):
            assert st2[k] == st[k], k
    assert rt.camera_sampling()["filter"] == "box"
    assert rt.integrator == "direct" and rt.max_depth == 3 and rt.flags & 2
    rt.clear()
    with pytest.raises(NativeError):
        rt.svgf()  # spp == 0
    rt.set_camera(s.desc.camera, s.desc.projection)
    rt.render(2, first_sample=0)
    assert_same_bits(rt.film()[0], film, "the same settings render the same film afterwards")
    assert a.shape == b.shape == (48, 64, 3)


def test_two_runs_give_the_same_bits(scene_dirs):
    s = loadScene(scene_dirs["syn20k"], width=33, height=31)
    outs = []
    for _ in range(2):
        rt = RayTracer(s, seed=1234)
        run = []
        for (label, pose), spp in zip(tr.move_sequence(s), SPPS):
            frame(rt, s, pose, spp)
            run += [rt.svgf(), rt.svgf_variance(), rt.svgf_moments(), rt.temporal_history()]
        outs.append(run)
        g, a, v, f = rt.svgf_ms()
        assert g > 0 and a > 0 and v > 0 and f > 0
    for x, y in zip(*outs):
        assert_same_bits(x, y, "second run")


def test_orbit_quality():
    """test_temporal_gpu's 8-pose orbit of cornell-box (14 degrees, 64 x 48), 1 spp per pose under seeds
    1234 + i, plane_tolerance 0.001, everything else at its default (5 levels): the luminance MSE of svgf()
    against the handle's own 1024-spp film at the last pose (seed 99) is below that of temporal() over the
    same frames. The restated sequence run through the C oracle gave the ratio 0.349 beforehand (svgf 7.30e-5,
    temporal 2.09e-4, the raw frame 3.29e-3; temporal / raw 0.064 as recorded in test_temporal_gpu), so the
    iterations did not have to be lowered; fewer levels blur less and gave 0.347, 0.338, 0.285 and 0.276 for
    4, 3, 2 and 1. With the default plane_tolerance 0.01 the temporal step bleeds the emitter into the ceiling
    as DESIGN.md 8h describes, and the plane term of the filter does not undo it: svgf is at 0.060 of temporal
    there but only at 0.92 of the raw frame. The assertion is only < 1."""
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=64, height=48)
    a, b = RayTracer(s, seed=1234), RayTracer(s, seed=1234)
    for i, pose in enumerate(tr.orbit(s, 8, 14.0)):
        for rt in (a, b):
            rt.set_camera(*tr.pose_records(s, pose))
            rt.clear()
            rt.seed = 1234 + i
            rt.render(1, first_sample=0)
        out_s = a.svgf(plane_tolerance=0.001)
        out_t = b.temporal(plane_tolerance=0.001)
    a.clear()
    a.seed = 99
    a.render(1024, first_sample=0)
    truth = tr.lum(a.film()[0] / np.float32(1024))
    mse_s = ((tr.lum(out_s) - truth) ** 2).mean()
    mse_t = ((tr.lum(out_t) - truth) ** 2).mean()
    print("orbit: temporal %.6g svgf %.6g ratio %.4f" % (mse_t, mse_s, mse_s / mse_t))
    assert mse_s / mse_t < 1.0
