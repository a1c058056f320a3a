"""A movable camera on the GPU (rtg_set_camera): a handle created at pose A, moved to pose B and cleared
renders, bit for bit, the film of a fresh handle created from a descriptor carrying B, and the film the C
oracle builds from that descriptor; for every consumer of the camera records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as tr
from conftest import SCENES
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import NativeError, RayTracer, RayTracerGroup, loadScene, look_at, save_hdr, write_synthetic_scene
from raytracingrenderer_amd import _native as N

pytestmark = pytest.mark.gpu

W, H = 64, 48


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError("%s: %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("syn20k")
    dirs = {"cornell-box": os.path.join(SCENES, "cornell-box"), "cornell-mat": os.path.join(SCENES, "cornell-mat"),
            "syn20k": write_synthetic_scene(str(d), n_tris=20000, seed=7, width=W, height=H)}
    out = {}
    for name, path in dirs.items():
        s = loadScene(path, width=W, height=H)
        b = tr.posed(s, dict(tr.move_sequence(s))["small move"])  # pose B: sideways and a 3 degree turn
        out[name] = (s, b)
    return out


def moved(s, b, **kw):
    """A tracer created at the scene's pose A, moved to B and cleared."""
    rt = RayTracer(s, seed=1234, **kw)
    rt.render(1)  # something on the film and in the pipeline before the move
    rt.set_camera(b.desc.camera, b.desc.projection)
    rt.clear()
    return rt


@pytest.mark.parametrize("name", ["cornell-box", "cornell-mat", "syn20k"])
def test_path_film_after_a_move(scenes, name):
    s, b = scenes[name]
    rt = moved(s, b, max_depth=4)
    rt.render(4)
    got = rt.film()[0]
    fresh = RayTracer(b, seed=1234, max_depth=4)
    fresh.render(4)
    assert_same_bits(got, fresh.film()[0], name + ": moved vs a fresh handle at B")
    want, _ = Oracle(b, 4, "rtm").render(4, seed=1234, threads=8)
    assert_same_bits(got, want, name + ": moved vs the oracle at B")
    a = RayTracer(s, seed=1234, max_depth=4)
    a.render(4)
    assert not np.array_equal(got, a.film()[0])  # B is another view
    cam, proj = rt.camera()
    assert bytes(cam) == bytes(b.desc.camera) and bytes(proj) == bytes(b.desc.projection)


def test_tent_filter_and_lens_after_a_move(scenes):
    s, b = scenes["cornell-mat"]
    setting = dict(filter="tent", filter_radius=1.5, lens_radius=0.05, focal_distance=5.0)
    rt = moved(s, b)
    rt.set_camera_sampling(**setting)
    rt.render(3)
    fresh = RayTracer(b, seed=1234)
    fresh.set_camera_sampling(**setting)
    fresh.render(3)
    assert_same_bits(rt.film()[0], fresh.film()[0], "tent + lens: moved vs fresh")
    orc = Oracle(b, 4, "rtm")
    orc.set_camera_sampling(**setting)
    assert_same_bits(rt.film()[0], orc.render(3, seed=1234, threads=8)[0], "tent + lens: moved vs the oracle")
    pix = np.arange(0, W * H, 7, dtype=np.uint32)
    assert_same_bits(rt.camera_samples(pix, pix % 5)[0], fresh.camera_samples(pix, pix % 5)[0], "camera_samples")


@pytest.mark.parametrize("integrator", ["direct_mis", "albedo", "normals"])
def test_first_hit_integrators_after_a_move(scenes, integrator):
    s, b = scenes["cornell-mat"]
    rt = moved(s, b, integrator=integrator)
    rt.render(2)
    fresh = RayTracer(b, seed=1234, integrator=integrator)
    fresh.render(2)
    assert_same_bits(rt.film()[0], fresh.film()[0], integrator + ": moved vs fresh")
    want, _ = Oracle(b, 4, "rtm", integrator=RayTracer.INTEGRATORS[integrator]).render(2, seed=1234, threads=8)
    assert_same_bits(rt.film()[0], want, integrator + ": moved vs the oracle")


def test_light_tracer_and_instant_radiosity_after_a_move(scenes):
    s, b = scenes["cornell-box"]
    orc = Oracle(b, 4, "rtm")
    rt = moved(s, b)
    rt.lightTracer(1, first_frame=0)
    fresh = RayTracer(b, seed=1234)
    fresh.lightTracer(1, first_frame=0)
    assert_same_bits(rt.film()[0], fresh.film()[0], "light tracer: moved vs fresh")
    assert_same_bits(rt.film()[0], orc.render_light(1, first=0, seed=1234), "light tracer: moved vs the oracle")
    pts = np.random.default_rng(1).uniform(-1, 2, (200, 3)).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (200, 1))
    assert_same_bits(rt.connect_probe(pts, nrm, nrm), fresh.connect_probe(pts, nrm, nrm), "connect_probe")
    rt.clear()
    fresh.clear()
    rt.instantRadiosity(1, n_vpl=8, first_frame=0)
    fresh.instantRadiosity(1, n_vpl=8, first_frame=0)
    assert_same_bits(rt.film()[0], fresh.film()[0], "instant radiosity: moved vs fresh")
    assert_same_bits(rt.film()[0], orc.render_instant_radiosity(1, first=0, seed=1234, n_vpl=8),
                     "instant radiosity: moved vs the oracle")


def test_adaptive_render_after_a_move(scenes):
    s, b = scenes["cornell-box"]
    rt = moved(s, b)
    ca = rt.adaptiveRender(init_samples=2, max_samples=12, min_samples=1, first_sample=0)
    fresh = RayTracer(b, seed=1234)
    cb = fresh.adaptiveRender(init_samples=2, max_samples=12, min_samples=1, first_sample=0)
    assert_same_bits(rt.film()[0], fresh.film()[0], "adaptive: moved vs fresh")
    assert np.array_equal(ca, cb)


def test_denoise_after_a_move(scenes):
    s, b = scenes["cornell-mat"]
    rt = RayTracer(s, seed=1234)
    rt.render(2)
    at_a = rt.denoise()  # the guides of pose A are cached now
    rt.set_camera(b.desc.camera, b.desc.projection)
    rt.clear()
    rt.render(2, first_sample=0)
    fresh = RayTracer(b, seed=1234)
    fresh.render(2)
    got, want = rt.denoise(), fresh.denoise()
    assert_same_bits(got, want, "denoise: moved vs fresh")
    assert not np.array_equal(got, at_a)
    for g, w in zip(rt.guides(), fresh.guides()):
        assert_same_bits(g, w, "guides after the move")


def test_queued_frames_keep_the_camera_they_were_queued_under(scenes):
    s, b = scenes["cornell-box"]
    rt = RayTracer(s, seed=1234)
    for i in range(3):
        rt.render(1, first_sample=i, sync=False)  # queued under A, not issued yet
    rt.set_camera(b.desc.camera, b.desc.projection)
    for i in range(3, 5):
        rt.render(1, first_sample=i, sync=False)  # queued under B
    got, spp = rt.film()
    assert spp == 5
    a = RayTracer(s, seed=1234)
    a.render(3)
    fresh = RayTracer(b, seed=1234)
    fresh.load_film(a.film()[0], 3)
    fresh.render(2, first_sample=3)
    assert_same_bits(got, fresh.film()[0], "A's three frames, then B's two")


def test_group_after_a_move(scenes):
    s, b = scenes["cornell-box"]
    g = RayTracerGroup(s, devices=(0, 0), seed=1234)
    g.render(1)
    g.set_camera(b.desc.camera, b.desc.projection)
    g.clear()
    g.render(3)
    one = RayTracer(b, seed=1234)
    one.render(3)
    assert_same_bits(g.film()[0], one.film()[0], "two ranks on one device vs a single handle at B")
    lib = N.rtg()
    for r in range(2):
        cam, proj = N.rtg_camera(), N.rtg_camera_proj()
        assert lib.rtg_get_camera(lib.rtg_group_handle(g._g, r), C.byref(cam), C.byref(proj)) == 0
        assert bytes(cam) == bytes(b.desc.camera) and bytes(proj) == bytes(b.desc.projection)
    bad = N.rtg_camera.from_buffer_copy(bytes(b.desc.camera))
    bad.width = W + 1
    with pytest.raises(NativeError):
        g.set_camera(bad, b.desc.projection)
    assert lib.rtg_group_set_camera(None, C.byref(bad), C.byref(b.desc.projection)) == -1
    for r in range(2):
        cam = N.rtg_camera()
        assert lib.rtg_get_camera(lib.rtg_group_handle(g._g, r), C.byref(cam), None) == 0
        assert bytes(cam) == bytes(b.desc.camera)


def test_setter_errors_keep_the_camera_and_the_film(scenes):
    s, b = scenes["cornell-box"]
    rt = RayTracer(s, seed=1234)
    rt.render(2)
    film = rt.film()[0]
    lib, h = rt._lib, rt._h
    good_c, good_p = b.desc.camera, b.desc.projection

    def variant(rec, field, index, value):
        r = type(rec).from_buffer_copy(bytes(rec))
        if index is None:
            setattr(r, field, value)
        else:
            getattr(r, field)[index] = value
        return r

    bad = [(variant(good_c, "width", None, W + 1), good_p), (variant(good_c, "height", None, H - 1), good_p),
           (variant(good_c, "inv_proj", 5, np.nan), good_p), (variant(good_c, "camera", 15, np.inf), good_p),
           (variant(good_c, "origin", 2, -np.inf), good_p), (good_c, variant(good_p, "proj", 0, np.nan)),
           (good_c, variant(good_p, "camera_to_view", 7, np.inf)), (good_c, variant(good_p, "view_direction", 1, np.nan)),
           (good_c, variant(good_p, "a_film", None, np.inf))]
    for c, p in bad:
        with pytest.raises(NativeError):
            rt.set_camera(c, p)
    assert lib.rtg_set_camera(h, None, C.byref(good_p)) == -1
    assert lib.rtg_set_camera(h, C.byref(good_c), None) == -1
    assert lib.rtg_set_camera(None, C.byref(good_c), C.byref(good_p)) == -1
    assert lib.rtg_get_camera(None, None, None) == -1
    cam, proj = rt.camera()
    assert bytes(cam) == bytes(s.desc.camera) and bytes(proj) == bytes(s.desc.projection)
    got, spp = rt.film()
    assert spp == 2
    assert_same_bits(got, film, "the film after rejected setters")
    rt.render(1)  # and the camera still renders A
    a = RayTracer(s, seed=1234)
    a.render(3)
    assert_same_bits(rt.film()[0], a.film()[0], "A goes on")
    rt.set_camera(good_c, good_p)  # the film and SPP are left alone by a good setter too
    got, spp = rt.film()
    assert spp == 3
    assert_same_bits(got, a.film()[0], "set_camera leaves the film")


def test_look_at_method(scenes):
    s, b = scenes["cornell-box"]
    pose = dict(tr.move_sequence(s))["small move"]
    rt = RayTracer(s, seed=1234)
    rt.look_at(pose["from_"], pose["to"], s.camera_pose["up"])
    cam, proj = rt.camera()
    assert bytes(cam) == bytes(b.desc.camera) and bytes(proj) == bytes(b.desc.projection)
    rt.look_at(pose["from_"], pose["to"], s.camera_pose["up"], fov=30.0)
    want = look_at(pose["from_"], pose["to"], s.camera_pose["up"], 30.0, W, H)
    assert bytes(rt.camera()[0]) == bytes(want[0])


def test_cli_pose_flags_write_the_library_film(tmp_path, scenes):
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    scene = os.path.join(SCENES, "cornell-box")
    s, _ = scenes["cornell-box"]
    base = [cli, "-scene", scene, "-SPP", "3", "-width", str(W), "-height", str(H), "-timeLimit", "0",
            "-outputFilename", "out.hdr"]
    pose = s.camera_pose
    full = dict(from_=[0.3, 1.2, 6.5], to=[0.0, 1.0, 0.0], up=[0.1, 1.0, 0.0], fov=25.0)
    runs = {"all": (["-from", "0.3 1.2 6.5", "-to", "0.0 1.0 0.0", "-up", "0.1 1.0 0.0", "-fov", "25"], full),
            "from only": (["-from", "0.3 1.2 6.5"], dict(from_=[0.3, 1.2, 6.5], to=pose["to"], up=pose["up"], fov=pose["fov"])),
            "fov only": (["-fov", "25"], dict(from_=pose["from_"], to=pose["to"], up=pose["up"], fov=25.0)),
            "group": (["-devices", "0,0", "-to", "0.25 1.0 0.0"], dict(from_=pose["from_"], to=[0.25, 1, 0], up=pose["up"], fov=pose["fov"])),
            "none": ([], dict(from_=pose["from_"], to=pose["to"], up=pose["up"], fov=pose["fov"]))}
    films = set()
    for k, (d, (extra, p)) in enumerate(runs.items()):
        rt = RayTracer(s, seed=1234)
        rt.set_camera(*look_at(p["from_"], p["to"], p["up"], p["fov"], W, H, pose["flip_x"]))
        rt.render(3)
        lib_file = tmp_path / ("lib%d.hdr" % k)
        save_hdr(str(lib_file), rt.film()[0], 3)
        (tmp_path / str(k)).mkdir()
        r = subprocess.run(base + extra, cwd=str(tmp_path / str(k)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / str(k) / "out.hdr").read_bytes() == lib_file.read_bytes(), d
        films.add(lib_file.read_bytes())
    assert len(films) == len(runs)
    for bad in (["-from", "1 2"], ["-to", "0 1 6.8"], ["-up", "0 0 1"], ["-from", "1 2 3 4"]):
        r = subprocess.run(base + bad, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode != 0, bad
