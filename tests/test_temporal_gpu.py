"""The geometry guide and temporal accumulation on the GPU (rtg_geometry_guide, rtg_temporal_accumulate)
against their numpy restatement (tests/temporal_ref.py) bit for bit, every pixel: the guides of the
restatement come from the C oracle, the films it blends are the GPU's own (the film is the input of the
definition; the renders are pinned against the oracle in tests/test_camera_move_gpu.py)."""
import os

import numpy as np
import pytest

import temporal_ref as tr
from conftest import SCENES
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import NativeError, RayTracer, loadScene, write_synthetic_scene

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (33, 31)]  # partial blocks and waves, odd rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what, nan_equal=False):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    if nan_equal:  # any NaN equals any NaN
        diff &= ~(np.isnan(got) & np.isnan(want))
    if diff.any():
        bad = np.argwhere(diff)
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def scene_dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("syn20k")
    return {"cornell-box": os.path.join(SCENES, "cornell-box"),  # 36 triangles: the LDS-resident walk
            "syn20k": write_synthetic_scene(str(d), n_tris=20000, seed=7, width=64, height=48),  # the general walk
            "cornell-mat": os.path.join(SCENES, "cornell-mat")}


_ORACLES = {}


def oracle_guide(ps, key):
    """The restated guide of a posed scene, computed once per (scene, size, pose) and shared."""
    if key not in _ORACLES:
        _ORACLES[key] = tr.guide_ref(Oracle(ps, 4, "rtm"), ps)
    return _ORACLES[key]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["cornell-box", "syn20k"])
def test_geometry_guide_equals_the_restatement(scene_dirs, name, size):
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    rt.set_camera_sampling("tent", 2.0, 0.1, 5.0)  # the guide stays a centre / pinhole ray
    seen = 0
    for label, pose in tr.move_sequence(s)[1:5]:
        ps = tr.posed(s, pose)
        rt.set_camera(ps.desc.camera, ps.desc.projection)
        pos_t, nid = rt.geometry_guide()
        want_p, want_n = oracle_guide(ps, (name, size, label))
        assert_same_bits(nid, want_n, "%s %s %s: normal and id" % (name, size, label))
        assert_same_bits(pos_t, want_p, "%s %s %s: position and t" % (name, size, label))
        hit = nid[..., 3].view(np.int32) >= 0
        seen += int(hit.sum())
        ln = np.linalg.norm(nid[..., :3][hit].astype(np.float64), axis=1)
        assert np.allclose(ln, 1.0, atol=1e-6)
        again = rt.geometry_guide()  # the cached guide
        assert_same_bits(again[0], pos_t, "cached: position and t")
        assert_same_bits(again[1], nid, "cached: normal and id")
    assert seen > 100
    assert rt.camera_sampling()["filter"] == "tent"


def play(rt, s, name, size, steps, ref, spps, **kw):
    """Move, clear, render, accumulate over `steps`; every output and history against the restatement."""
    shares = {}
    for (label, pose), spp in zip(steps, spps):
        ps = tr.posed(s, pose)
        rt.set_camera(ps.desc.camera, ps.desc.projection)
        rt.clear()
        rt.render(spp, first_sample=0)
        film, got_spp = rt.film()
        assert got_spp == spp
        out = rt.temporal(**kw)
        want = ref.accumulate(film, spp, ps.desc.camera, ps.desc.projection,
                              lambda: oracle_guide(ps, (name, size, label)), **kw)
        what = "%s %s %s %s" % (name, size, label, kw)
        assert_same_bits(out, want, what + ": output")
        hist = rt.temporal_history()
        assert_same_bits(hist, ref.H, what + ": history")
        shares[label] = float((hist[..., 3] > spp).mean())
    return shares


SPPS = [2, 1, 1, 3, 1, 2]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["cornell-box", "cornell-mat", "syn20k"])
def test_sequence_equals_the_restatement(scene_dirs, name, size):
    """first call, unchanged camera, small move, dolly-in, 90 degree turn, looking away; then the whole
    sequence again after temporal_reset(). The restatement gives >= 50 % of the pixels a history after the
    small move on the two Cornell scenes (tests/test_temporal.py); on the 20k scene, whose triangles are
    smaller than a pixel's footprint, the plane test leaves 4-5 % (measured with the restatement), so there
    the share only has to be above zero."""
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    steps = tr.move_sequence(s)
    with pytest.raises(NativeError):
        rt.temporal_history()  # nothing accumulated yet
    with pytest.raises(NativeError):
        rt.temporal()  # spp == 0
    for _ in range(2):
        sh = play(rt, s, name, size, steps, tr.TemporalRef(), SPPS)
        assert sh["first"] == 0.0 and sh["unchanged"] == 1.0 and sh["looking away"] == 0.0, sh
        assert sh["small move"] >= (0.5 if name != "syn20k" else 0.01), sh
        rt.temporal_reset()


CASES = [dict(max_history=4.0), dict(max_history=np.inf), dict(plane_tolerance=0.0), dict(normal_cos=1.0),
         dict(max_history=2.0, plane_tolerance=0.001, normal_cos=0.0)]


@pytest.mark.parametrize("kw", CASES, ids=str)
def test_parameters_equal_the_restatement(scene_dirs, kw):
    name, size = "cornell-box", (64, 48)
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    steps = tr.move_sequence(s)
    steps = steps[:2] + steps[1:2] * 4 + steps[2:]  # six frames at A: max_history 4 saturates
    ref = tr.TemporalRef()
    play(rt, s, name, size, steps[:6], ref, [1] * 6, **kw)
    if kw.get("max_history") == 4.0:
        assert (ref.H[..., 3] == 5.0).all()
    elif "max_history" not in kw or kw["max_history"] == np.inf:
        assert (ref.H[..., 3] == 6.0).all()
    play(rt, s, name, size, steps[6:], ref, [1] * len(steps[6:]), **kw)


def test_non_finite_pixels_follow_the_definition(scene_dirs):
    """One NaN pixel and one +inf pixel planted through film_load on a wall: unchanged they stay where they
    are, after the small move they spread to the pixels whose taps read them, as in the restatement."""
    name, size = "cornell-box", (64, 48)
    s = loadScene(scene_dirs[name], width=size[0], height=size[1])
    rt = RayTracer(s, seed=1234)
    ref = tr.TemporalRef()
    steps = tr.move_sequence(s)
    rt.render(1)
    film = rt.film()[0]
    film[24, 20, 1] = np.nan
    film[30, 40, :] = np.inf
    seq = [(steps[0], film), (steps[1], None), (steps[2], None), (steps[3], None)]
    nonfinite = []
    for (label, pose), planted in seq:
        ps = tr.posed(s, pose)
        rt.set_camera(ps.desc.camera, ps.desc.projection)
        rt.clear()
        if planted is None:
            rt.render(1, first_sample=0)
        else:
            rt.load_film(planted, 1)
        f = rt.film()[0]
        out = rt.temporal()
        want = ref.accumulate(f, 1, ps.desc.camera, ps.desc.projection, lambda: oracle_guide(ps, (name, size, label)))
        assert_same_bits(out, want, label, nan_equal=True)
        assert_same_bits(rt.temporal_history(), ref.H, label + ": history", nan_equal=True)
        nonfinite.append(int((~np.isfinite(out)).any(axis=2).sum()))
    assert nonfinite[0] == 2 and nonfinite[1] == 2 and nonfinite[2] > 2, nonfinite


def test_the_handle_is_left_as_it_was(scene_dirs):
    s = loadScene(scene_dirs["cornell-box"], width=64, height=48)
    rt = RayTracer(s, seed=1234, integrator="direct", max_depth=3)
    rt.set_options(flags=rt.flags | 2)  # RTG_OPT_COUNT
    rt.set_camera_sampling("box", 0.5)
    rt.render(2)
    film, spp = rt.film()
    st = rt.stats()
    a = rt.temporal()
    g = rt.geometry_guide()
    small = tr.posed(s, dict(tr.move_sequence(s))["small move"])
    rt.set_camera(small.desc.camera, small.desc.projection)
    b = rt.temporal()  # a moved accumulate: guide pass and reprojection
    g2 = rt.geometry_guide()
    assert not np.array_equal(g[0], g2[0])
    f2, spp2 = rt.film()
    assert_same_bits(f2, film, "film")
    assert spp2 == spp == 2
    st2 = rt.stats()
    for k in st:
        if not k.endswith("_ms"):
            assert st2[k] == st[k], k
    assert rt.camera_sampling()["filter"] == "box"
    rt.clear()
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
            rt.set_camera(*tr.pose_records(s, pose))
            rt.clear()
            rt.render(spp, first_sample=0)
            run.append(rt.temporal())
            run.append(rt.temporal_history())
        outs.append(run)
        g, a = rt.temporal_ms()
        assert g > 0 and a > 0
    for x, y in zip(*outs):
        assert_same_bits(x, y, "second run")


def test_orbit_quality():
    """An 8-pose orbit of cornell-box (14 degrees about the centre of its bounds, 64 x 48), 1 spp per pose
    under seeds 1234 + i, plane_tolerance 0.001: the temporal output's luminance MSE against the handle's own
    1024-spp film at the last pose (seed 99) is below the raw last frame's. The restated sequence run
    through the C oracle gave the ratio 0.064 beforehand (every step keeps 0.73-0.77 of the pixels' history;
    the other quarter is background).
    With the default plane_tolerance 0.01 the same sequence gives 15.3, worse than the raw frame: the box's
    emitter hangs 0.02 below the ceiling, 0.01 t is 0.07 there, so the emitter's pixels (17, 12, 4) pass
    the plane test of ceiling pixels and bleed into them. The assertion is only < 1."""
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=64, height=48)
    rt = RayTracer(s, seed=1234)
    raw = out = None
    for i, pose in enumerate(tr.orbit(s, 8, 14.0)):
        rt.set_camera(*tr.pose_records(s, pose))
        rt.clear()
        rt.seed = 1234 + i
        rt.render(1, first_sample=0)
        raw = rt.film()[0]
        out = rt.temporal(plane_tolerance=0.001)
        if i:
            assert (rt.temporal_history()[..., 3] > 1).mean() >= 0.5, i
    rt.clear()
    rt.seed = 99
    rt.render(1024, first_sample=0)
    truth = tr.lum(rt.film()[0] / np.float32(1024))
    mse_raw = ((tr.lum(raw) - truth) ** 2).mean()
    mse_out = ((tr.lum(out) - truth) ** 2).mean()
    print("orbit: raw %.6g temporal %.6g ratio %.4f" % (mse_raw, mse_out, mse_out / mse_raw))
    assert mse_out / mse_raw < 1.0
