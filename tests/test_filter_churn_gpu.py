"""The five film-filter entry points (gbuffer, temporal, svgf, denoise, geometry_guide) on one handle, sharing
its temporal, variance and denoiser states and the two guide caches: every image against the numpy restatements
(tests/temporal_ref.py, tests/svgf_ref.py, tests/denoise_ref.py) bit for bit, the caches by the stage times they
leave, and the final state against a handle that was never churned.

cornell-box at 72 x 38: the width is no multiple of 64 and the height none of 4, so the edge blocks of the 64 x 4
layout are live, and the 7 x 7 variance window and the filter's steps up to 16 (iterations = 5) cross the border.
The geometry guides of the restatements come from the C oracle and the albedo / shading-normal guides from
guides(), as in tests/test_svgf_gpu.py; the films are the handle's own.

The sequence:
  1. render 1 spp; gbuffer(); temporal()
  2. move; render 1 spp; svgf(); denoise(); geometry_guide()
  3. temporal_reset(); render 1 spp; svgf()
  4. move; render 1 spp; temporal(); svgf()
  5. gbuffer(); svgf() once more: both served by the caches (no earlier svgf() of the sequence finds both of
     its guides at hand, so the zero guide time of svgf_ms() is asserted here)
The unchurned handle takes the films since the reset through load_film and makes only the accumulate calls that
define the state: step 3's svgf(), then step 4's temporal() and svgf(), whose every output must be the churned
handle's (step 4's two calls alone start from an empty history on a fresh handle, so step 3's call goes with them)."""
import ctypes as C
import os

import numpy as np
import pytest

import svgf_ref as sr
import temporal_ref as tr
from conftest import SCENES
from denoise_ref import denoise_ref
from raytracingrenderer_amd import NativeError, RayTracer, loadScene
from test_svgf_gpu import check, frame
from test_temporal_gpu import assert_same_bits, oracle_guide

pytestmark = pytest.mark.gpu

NAME, SIZE, KW = "cornell-box", (72, 38), dict(iterations=5)


class DeviceImage:
    """A hipMalloc'ed (38, 72, 3) float32 buffer of the HIP runtime librtg.so is linked against."""

    def __init__(self):
        try:
            self.hip = C.CDLL("libamdhip64.so")
        except OSError:
            self.hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")  # librtg.so's rpath
        self.d = C.c_void_p()
        self.nbytes = SIZE[0] * SIZE[1] * 3 * 4
        assert self.hip.hipMalloc(C.byref(self.d), C.c_size_t(self.nbytes)) == 0

    def read(self):
        got = np.zeros((SIZE[1], SIZE[0], 3), np.float32)
        assert self.hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), self.d, C.c_size_t(self.nbytes), 2) == 0
        return got

    def free(self):
        self.hip.hipFree(self.d)


@pytest.fixture
def dev():
    d = DeviceImage()
    yield d
    d.free()


def test_five_entry_points_share_one_handle(dev):
    s = loadScene(os.path.join(SCENES, NAME), width=SIZE[0], height=SIZE[1])
    poses = dict(tr.move_sequence(s))
    rt = RayTracer(s, seed=1234)
    ref = sr.SvgfRef()

    def guide_of(ps, label):
        return lambda: oracle_guide(ps, (NAME, SIZE, label))

    def temporal(ps, film, label, what):
        out = rt.temporal()
        want = ref.temporal(film, 1, ps.desc.camera, ps.desc.projection, guide_of(ps, label))
        assert_same_bits(out, want, what + ": output")
        assert_same_bits(rt.temporal_history(), ref.t.H, what + ": history")
        return out

    # 1. the fused pass fills both caches; temporal() finds its guide there
    ps, film = frame(rt, s, poses["first"], 1)
    g = rt.gbuffer()
    assert rt.gbuffer_ms() > 0.0
    want_p, want_n = oracle_guide(ps, (NAME, SIZE, "first"))
    assert_same_bits(g["pos_t"], want_p, "1 gbuffer: position and t")
    assert_same_bits(g["normal_id"], want_n, "1 gbuffer: normal and id")
    temporal(ps, film, "first", "1 temporal")
    assert rt.temporal_ms()[0] == 0.0 and rt.temporal_ms()[1] > 0.0
    with pytest.raises(NativeError, match="no result yet"):
        rt.copy_svgf_to(dev.d.value)  # the temporal state is there, the variance-guided one is not

    # 2. a move: svgf() traces once for all three guides; denoise() and geometry_guide() read what it left
    ps, film = frame(rt, s, poses["small move"], 1)
    check(rt, ref, ps, film, 1, (NAME, SIZE, "small move"), "2 svgf", **KW)
    assert rt.svgf_ms()[0] > 0.0 and rt.svgf_ms()[0] == rt.gbuffer_ms()
    alb, nrm = rt.guides()
    assert_same_bits(rt.denoise(**KW), denoise_ref(film / np.float32(1), alb, nrm, **KW), "2 denoise")
    pos_t, nid = rt.geometry_guide()
    assert rt.temporal_ms()[0] == 0.0  # the history's own guide
    want_p, want_n = oracle_guide(ps, (NAME, SIZE, "small move"))
    assert_same_bits(pos_t, want_p, "2 geometry_guide: position and t")
    assert_same_bits(nid, want_n, "2 geometry_guide: normal and id")

    # 3. reset: no result, no history; the next svgf() is a first call (the denoiser's state is kept)
    rt.temporal_reset()
    assert rt.gbuffer_ms() == 0.0
    with pytest.raises(NativeError, match="rtg_svgf_copy_device: no result yet"):
        rt.copy_svgf_to(dev.d.value)
    with pytest.raises(NativeError, match="rtg_temporal_copy_device: no result yet"):
        rt.copy_temporal_to(dev.d.value)
    with pytest.raises(NativeError, match="rtg_temporal_history: no history yet"):
        rt.temporal_history()
    ref = sr.SvgfRef()
    rt.clear()
    rt.render(1, first_sample=0)
    film3 = rt.film()[0]
    ps3 = ps
    check(rt, ref, ps3, film3, 1, (NAME, SIZE, "small move"), "3 svgf", **KW)
    assert rt.svgf_ms()[0] > 0.0  # the guide cache went with the state
    assert ref.spatial.all()  # len is 1 everywhere: the 7 x 7 window at every border

    # 4. a move: temporal() traces the geometry guide alone and drops the moments; svgf() restarts them
    ps4, film4 = frame(rt, s, poses["dolly-in"], 1)
    out_t = temporal(ps4, film4, "dolly-in", "4 temporal")
    assert rt.temporal_ms()[0] > 0.0
    with pytest.raises(NativeError):
        rt.svgf_moments()  # dropped
    rt.copy_temporal_to(dev.d.value)
    assert_same_bits(dev.read(), out_t, "4 copy_temporal_to")
    out_s = check(rt, ref, ps4, film4, 1, (NAME, SIZE, "dolly-in"), "4 svgf", **KW)
    assert_same_bits(rt.svgf_moments()[..., 0], sr.lum32(film4 / np.float32(1)), "4 restarted moments")
    assert rt.svgf_ms()[0] > 0.0  # set_camera dropped the denoiser's guides: one fused pass
    rt.copy_svgf_to(dev.d.value)
    assert_same_bits(dev.read(), out_s, "4 copy_svgf_to")
    state = [rt.temporal_history(), rt.svgf_moments(), rt.svgf_variance()]

    # the same films on a handle that was never churned
    plain = RayTracer(s, seed=1234)
    frame(plain, s, poses["small move"], 1, film3)
    plain.svgf(**KW)
    frame(plain, s, poses["dolly-in"], 1, film4)
    assert_same_bits(plain.temporal(), out_t, "unchurned: temporal")
    assert_same_bits(plain.svgf(**KW), out_s, "unchurned: svgf")
    for got, want, what in zip([plain.temporal_history(), plain.svgf_moments(), plain.svgf_variance()], state,
                               ["history", "moments", "variance"]):
        assert_same_bits(got, want, "unchurned: " + what)

    # 5. everything is cached for this camera: neither call traces
    g = rt.gbuffer()
    assert rt.gbuffer_ms() == 0.0
    want_p, want_n = oracle_guide(ps4, (NAME, SIZE, "dolly-in"))
    assert_same_bits(g["pos_t"], want_p, "5 gbuffer: position and t")
    assert_same_bits(g["normal_id"], want_n, "5 gbuffer: normal and id")
    assert_same_bits(g["albedo"], rt.guides()[0], "5 gbuffer: albedo")
    check(rt, ref, ps4, film4, 1, (NAME, SIZE, "dolly-in"), "5 svgf", **KW)
    assert rt.svgf_ms()[0] == 0.0 and rt.gbuffer_ms() == 0.0
