"""Variance-guided filtering of the temporal history without a GPU: the argument check and the defaults of the
library (host code of rtg_svgf.hip that needs no device), and what the numpy restatement (tests/svgf_ref.py)
gives on its own on guides and films from the C oracle, before the kernels are compared with it bit for bit
(tests/test_svgf_gpu.py)."""
import os

import numpy as np
import pytest

import svgf_ref as sr
import temporal_ref as tr
from conftest import SCENES
from denoise_ref import TAPS
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import NativeError, loadScene
from raytracingrenderer_amd.renderer import svgf_check, svgf_defaults, write_mesh_scene

F = np.float32
W, H = 64, 48
SPPS = [2, 1, 1, 3, 1, 2]


def test_the_defaults_are_accepted_and_equal_the_header():
    svgf_check()
    d = svgf_defaults()
    want = {"max_history": 64.0, "plane_tolerance": F(0.01), "normal_cos": F(0.9), "iterations": 5,
            "normal_squarings": 5, "sigma_luminance": 4.0, "sigma_albedo": F(0.1), "min_history": 4.0,
            "variance_floor": F(1e-8)}
    assert set(d) == set(want)
    for k, v in want.items():
        assert F(d[k]) == F(v), (k, d[k])
    svgf_check(**d)


BAD = [dict(max_history=0.0), dict(max_history=np.nan), dict(plane_tolerance=-1.0), dict(plane_tolerance=np.inf),
       dict(plane_tolerance=np.nan), dict(normal_cos=1.5), dict(normal_cos=-0.1), dict(normal_cos=np.nan),
       dict(iterations=0), dict(iterations=9), dict(normal_squarings=9),
       dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=np.inf), dict(sigma_luminance=np.nan),
       dict(sigma_albedo=1e-7), dict(sigma_albedo=np.inf), dict(sigma_albedo=np.nan),
       dict(min_history=0.0), dict(min_history=np.inf), dict(min_history=np.nan),
       dict(variance_floor=0.0), dict(variance_floor=-1.0), dict(variance_floor=np.inf), dict(variance_floor=np.nan)]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_a_bad_parameter_is_rejected(kw):
    with pytest.raises(NativeError):
        svgf_check(**kw)


GOOD = [dict(max_history=np.inf), dict(plane_tolerance=0.0), dict(normal_cos=1.0), dict(normal_cos=0.0),
        dict(iterations=1), dict(iterations=8), dict(normal_squarings=0), dict(normal_squarings=8),
        dict(sigma_albedo=0.0), dict(sigma_albedo=-3.0), dict(sigma_albedo=1e-6), dict(min_history=1e9),
        dict(variance_floor=1.0), dict(sigma_luminance=0.5)]


@pytest.mark.parametrize("kw", GOOD, ids=str)
def test_the_edges_of_the_ranges_are_accepted(kw):
    svgf_check(**kw)


# ------------------------------------------------------------------ the restatement on the oracle's data
def oracle_inputs(ps):
    """(geometry guide, albedo, normal) of a posed scene from the C oracle: the guide integrators stop at the
    first hit and draw no random number."""
    guide = tr.guide_ref(Oracle(ps, 4, "rtm"), ps)
    alb = Oracle(ps, 4, "rtm", integrator=2).render(1, seed=1234, threads=8)[0]
    nrm = Oracle(ps, 4, "rtm", integrator=3).render(1, seed=1234, threads=8)[0]
    return guide, alb, nrm


@pytest.fixture(scope="module")
def box():
    return loadScene(os.path.join(SCENES, "cornell-box"), width=W, height=H)


@pytest.fixture(scope="module")
def box_inputs(box):
    return oracle_inputs(box)


def test_a_constant_film_stays_as_it_is(box, box_inputs):
    """The same value in every pixel and every frame: every blend adds (c - c) a = 0, every weighted mean of
    equal values divides w c by w, and the moments stay {l, l l}, so the variance is 0 on both branches. The
    value is grey 0.5, whose luminance is exactly 0.5 in float32: the 7x7 window's sums of up to 49 equal terms
    are then exact, as is w c for every weight. (A luminance with a full mantissa leaves the spatial branch a
    rounding residue of a few ulp of l l: c1 and c2 round as they grow.)"""
    guide, alb, nrm = box_inputs
    c = np.array([0.5, 0.5, 0.5], F)
    assert sr.lum32(c) == F(0.5)
    ref = sr.SvgfRef()
    l = sr.lum32(c)
    for k in range(6):
        out = ref.accumulate(np.broadcast_to(c, (H, W, 3)).copy(), 1, box.desc.camera, box.desc.projection,
                             lambda: guide, alb, nrm)
        assert (ref.var == 0).all(), k
        assert (ref.M[..., 0] == l).all() and (ref.M[..., 1] == l * l).all(), k
        assert (out == c).all(), k
        assert ref.spatial.all() == (k < 3)  # len = k + 1 against min_history 4: both branches were taken


@pytest.fixture(scope="module")
def box_sequence(box):
    """Per step of move_sequence: the posed scene, its oracle inputs and its 1..3-spp film."""
    steps = []
    for (label, pose), spp in zip(tr.move_sequence(box), SPPS):
        ps = tr.posed(box, pose)
        film = Oracle(ps, 4, "rtm").render(spp, seed=1234, threads=8)[0]
        steps.append((label, ps, oracle_inputs(ps), film, spp))
    return steps


def test_rgb_and_len_equal_the_temporal_restatement(box_sequence):
    """The svgf step leaves the history TemporalRef leaves, bit for bit, and both variance branches occur."""
    ref, tref = sr.SvgfRef(), tr.TemporalRef()
    spatial = temporal = 0
    for label, ps, (guide, alb, nrm), film, spp in box_sequence:
        out = ref.accumulate(film, spp, ps.desc.camera, ps.desc.projection, lambda: guide, alb, nrm)
        want = tref.accumulate(film, spp, ps.desc.camera, ps.desc.projection, lambda: guide)
        assert np.array_equal(ref.t.H.view(np.uint32), tref.H.view(np.uint32)), label
        assert np.array_equal(ref.t.H[..., :3], want), label
        assert out.shape == want.shape
        if film.any():  # the 90 degree turn looks at nothing: a black film stays black
            assert not np.array_equal(out, want), label
        assert (ref.var >= 0).all() and np.isfinite(ref.records).all(), label
        spatial += int(ref.spatial.sum())
        temporal += int((~ref.spatial).sum())
    assert spatial > 0 and temporal > 0, (spatial, temporal)


def test_mixing_restarts_the_moments(box_sequence):
    """svgf, temporal, svgf: the third call's moments are its own frame's, the history is the shared one."""
    ref, tref = sr.SvgfRef(), tr.TemporalRef()
    for i, (label, ps, (guide, alb, nrm), film, spp) in enumerate(box_sequence[:3]):
        args = (film, spp, ps.desc.camera, ps.desc.projection, lambda: guide)
        if i == 1:
            ref.temporal(*args)
        else:
            ref.accumulate(*args, alb, nrm)
        tref.accumulate(*args)
        assert np.array_equal(ref.t.H.view(np.uint32), tref.H.view(np.uint32)), label
    cur = film / F(spp)
    l = sr.lum32(cur)
    assert np.array_equal(ref.M[..., 0], l) and np.array_equal(ref.M[..., 1], l * l)


def test_one_level_on_noise_gives_the_b3_variance(tmp_path):
    """One plane filling the view, every stopping term at 1 (albedo off, no normal squaring on a constant
    normal, a huge plane_tolerance, and sigma_luminance 1e18, for which (dl dl) il is below 2^-25 and t rounds
    to 1): the weights are the B3 taps themselves, their sum is exactly 1 (dyadic), so an interior pixel's
    filtered variance is sum((h x h)^2) sigma^2. The float32 sum takes 25 products and 25 additions of
    non-negative terms, each rounding by at most 2^-24 of a value no larger than the result: the bound is
    50 * 2^-24 relative against the binary64 figure. The filtered noise itself must show that variance too:
    its sample variance over the interior (n pixels, correlated over 5 x 5) is checked to 25 %."""
    d = write_mesh_scene(str(tmp_path / "probe"), np.zeros((1, 3, 3), F) + np.eye(3, dtype=F), W, H)
    p = loadScene(d).camera_pose
    frm, to, up = (np.asarray(p[k], np.float64) for k in ("from_", "to", "up"))
    view = (to - frm) / np.linalg.norm(to - frm)
    side = np.cross(view, up / np.linalg.norm(up))
    side /= np.linalg.norm(side)
    u2 = np.cross(side, view)
    c, r = to, 1e3
    q = [c - r * side - r * u2, c + r * side - r * u2, c + r * side + r * u2, c - r * side + r * u2]
    s = loadScene(write_mesh_scene(str(tmp_path / "plane"), np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], F), W, H))
    guide = tr.guide_ref(Oracle(s, 4, "rtm"), s)
    assert (np.ascontiguousarray(guide[1][..., 3]).view(np.int32) >= 0).all()
    sigma = 0.1
    rng = np.random.default_rng(5)
    noise = (0.5 + sigma * rng.standard_normal((H, W))).astype(F)
    C4 = np.concatenate([np.repeat(noise[..., None], 3, axis=2), np.full((H, W, 1), F(sigma * sigma))], axis=2)
    alb = np.ones((H, W, 3), F)
    nrm = np.zeros((H, W, 3), F)
    nrm[..., 2] = 1
    out = sr.filter_ref(C4, alb, nrm, guide, iterations=1, normal_squarings=0, sigma_luminance=1e18, sigma_albedo=0.0,
                        variance_floor=1e-8, plane_tolerance=1e30)
    h2 = np.outer(np.array(TAPS, np.float64), np.array(TAPS, np.float64))
    want = (h2 ** 2).sum() * float(F(sigma * sigma))
    inner = out[2:-2, 2:-2]
    assert np.abs(inner[..., 3].astype(np.float64) - want).max() <= 50 * 2.0 ** -24 * want
    measured = inner[..., 0].astype(np.float64).var()
    assert abs(measured / want - 1) < 0.25, (measured, want)
    assert (out[0, 0, 3] > want)  # a corner keeps 9 of 25 taps: less averaging
