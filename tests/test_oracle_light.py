"""The C oracle's light tracer, instant radiosity and camera-connection probe (oracle/rt_oracle.c) pinned
against the same code restated on the reference's own compiled classes (oracle/_ref), on the scenes that
tests/test_light_paths_gpu.py compares the GPU with the oracle on: the textured and mixed-material scenes
and the closed white box. tests/test_oracle.py makes the film check on the two Cornell scenes only.
CPU only."""
import os

import numpy as np
import pytest

from conftest import SCENES
from light_scenes import connection_points, write_closed_white_box
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import loadScene


def _pyref():
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built")
    return pyref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nan_canon(a):
    b = _bits(a).copy()
    b[np.isnan(np.ascontiguousarray(a, np.float32))] = 0x7FC00000
    return b


@pytest.mark.parametrize("name,w,h", [("bathroom-small", 72, 40), ("coffee-small", 72, 40), ("cornell-mat", 72, 40),
                                      ("white-box", 64, 48), ("white-box", 5, 3)])
def test_light_oracles_equal_reference_classes(name, w, h, tmp_path):
    """Oracle.render_light / render_instant_radiosity against pyref.render_light /
    render_instant_radiosity (RayTracer::lightTracer / instantRadiosity on RTBase's classes, shared
    transcendentals), bit for bit: 2 frames, 20 VPL paths."""
    pyref = _pyref()
    path = write_closed_white_box(tmp_path / "box") if name == "white-box" else os.path.join(SCENES, name)
    s = loadScene(path, width=w, height=h)
    r = pyref.RefScene(path, w, h, False, flavour="rtm")
    assert (r.W, r.H, r.nlight) == (w, h, len(s.lights))
    o = Oracle(s, 4, "rtm")
    a, (b, c) = pyref.render_light(r, 2, seed=5), o.render_light(2, seed=5, count=True)
    assert np.array_equal(_bits(a), _bits(b)), (a != b).sum()
    assert (b != 0).any(axis=2).sum() > (100 if w * h > 100 else 10)
    # what the counts must obey whatever the scene: a path per pixel and frame; a splat needs a shadow ray
    assert c["paths"] == 2 * w * h and c["splats"] <= c["shadow_rays"] - c["off_film"]
    a = pyref.render_instant_radiosity(r, 2, seed=9, n_vpl=20)
    b, c = o.render_instant_radiosity(2, seed=9, n_vpl=20, count=True)
    assert np.array_equal(_bits(a), _bits(b)), (a != b).sum()
    assert (b != 0).any(axis=2).sum() > (100 if w * h > 100 else 10)
    assert c["paths"] == 2 * (w * h + 20) and 2 * w * h <= c["extension_rays"] and c["splats"] <= 2 * w * h


def test_light_oracle_counts_are_per_call_and_additive():
    """The counts of two one-frame calls add up to those of one two-frame call, and count=False changes
    no film."""
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=40, height=32)
    o = Oracle(s, 4, "rtm")
    f2, c2 = o.render_light(2, seed=3, count=True)
    fa, ca = o.render_light(1, first=0, seed=3, count=True)
    fb, cb = o.render_light(1, first=1, seed=3, film=fa, count=True)
    assert np.array_equal(_bits(f2), _bits(fb)) and np.array_equal(_bits(f2), _bits(o.render_light(2, seed=3)))
    assert c2 == {k: ca[k] + cb[k] for k in c2} and c2["splats"] > 100 and c2["extension_rays"] > c2["paths"]
    g2, d2 = o.render_instant_radiosity(2, seed=3, n_vpl=10, count=True)
    ga, da = o.render_instant_radiosity(1, first=0, seed=3, n_vpl=10, count=True)
    gb, db = o.render_instant_radiosity(1, first=1, seed=3, n_vpl=10, film=ga, count=True)
    assert np.array_equal(_bits(g2), _bits(gb)) and d2 == {k: da[k] + db[k] for k in d2}
    assert d2["paths"] == 2 * (40 * 32 + 10) and d2["shadow_rays"] > 40 * 32


@pytest.mark.parametrize("w,h", [(96, 64), (40, 72)])
def test_connection_probe_matches_reference_classes(w, h):
    """or_connect_probe on the point set of the GPU's connection test against connectToCamera restated
    on the reference's Camera, Colour and Film (ref_connect_probe): the stage at which a connection ends,
    projectOntoCamera's x and y, the colour handed to Film::splat and the pixel Film::splat adds to. The
    reference's Film::splat is found by splatting, so its (int) conversion is the compiler's."""
    pyref = _pyref()
    path = os.path.join(SCENES, "cornell-box")
    s = loadScene(path, width=w, height=h)
    o = Oracle(s, 4, "rtm")
    pts, nrm, col = connection_points(o, s)
    out, stage, xy = o.connect_probe(pts, nrm, col)
    r = pyref.RefScene(path, w, h, False, flavour="rtm")
    rstage, rpix, rcol, rxy = r.connect_probe(pts, nrm, col)
    assert np.array_equal(stage, rstage), np.flatnonzero(stage != rstage)[:8]
    assert np.array_equal(_nan_canon(xy), _nan_canon(rxy))
    ok = stage == 0
    assert np.array_equal(out[:, 0].view(np.int32) == 1, ok)
    assert np.array_equal(out[ok, 1].view(np.int32), rpix[ok])
    assert np.array_equal(_nan_canon(out[ok, 2:5]), _nan_canon(rcol[ok]))
    assert not out[~ok].view(np.uint32).any()
    # the projection part is also what Oracle.camera_project and the reference's own call give
    proj, _ = r.camera_project(pts)
    assert np.array_equal(proj[:, 0] == 1.0, stage != 1)
    assert np.array_equal(_nan_canon(proj[:, 1:]), _nan_canon(xy))
    assert np.array_equal(_nan_canon(o.camera_project(pts)), _nan_canon(proj))


@pytest.mark.parametrize("w,h", [(96, 64), (40, 72)])
def test_connection_point_set_holds_every_class(w, h):
    """The point set reaches every way a connection can end, and the shadow ray of an accepted one is
    Scene::visible's: it starts EPSILON along the unit direction to the camera and stops 2 EPSILON short."""
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=w, height=h)
    o = Oracle(s, 4, "rtm")
    pts, nrm, col = connection_points(o, s)
    out, stage, xy = o.connect_probe(pts, nrm, col)
    n = {k: int((stage == k).sum()) for k in Oracle.CONN_STAGES}
    print(len(pts), n)
    assert n[0] > 100 and n[1] > 100 and n[2] > 100 and n[3] >= 2, n
    assert np.isnan(xy[stage != 1]).any()  # a NaN film coordinate passes projectOntoCamera's comparisons
    pix = out[stage == 0, 1].view(np.int32)
    assert pix.min() >= 0 and pix.max() < w * h and len(np.unique(pix)) > 50
    assert {0, w - 1} <= set((pix % w).tolist()) and {0, h - 1} <= set((pix // w).tolist())  # the film's edges
    origin = np.array(s.desc.camera.origin[:], np.float32)  # EPSILON = 1e-4 (Core.h)
    ok = (stage == 0) & np.isfinite(out).all(axis=1)
    d = origin[None].astype(np.float64) - pts[ok]
    dist = np.linalg.norm(d, axis=1)
    np.testing.assert_allclose(out[ok, 9:12], d / dist[:, None], atol=1e-6)
    np.testing.assert_allclose(out[ok, 8], dist - 2e-4, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out[ok, 5:8], pts[ok] + 1e-4 * d / dist[:, None], atol=1e-5)
