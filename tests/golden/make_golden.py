"""Regenerate the golden fixtures in tests/golden/ (build container only).

Sources of truth:
  * oracle/_ref/libref.so — RTBase's own code compiled from /root/reference (loader classes,
    Triangle/AABB/BVH, Scene::traverse/visible, Camera, BSDFs, EnvironmentMap, Texture, Film::save);
  * SURVEY.md §8(c) known answer for C1 (pinned by the reference integrator built in the survey).
The scene assets used are data files of the reference (RTBase/*/scene.json, .gem, .png, .hdr).

Usage: python tests/golden/make_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference/RTBase"

from oracle import pyref  # noqa: E402
from raytracingrenderer_amd import write_synthetic_scene  # noqa: E402

SCENES = {
    # name: (dir, width, height, skip_missing)
    "cornell256": (os.path.join(GOLD, "scenes", "cornell-box"), 256, 256, False),
    "synth20k": ("/tmp/rtg_golden_synth20k", 0, 0, False),
    "coffee_f": (os.path.join(REF, "coffee"), 400, 500, True),
    "bathroom_f": (os.path.join(REF, "bathroom"), 480, 270, True),
    "materialball_f": (os.path.join(REF, "materialball"), 320, 180, True),
}
ARRAYS = ("positions", "normals", "uvs", "material", "node_bounds", "node_links", "lights", "camera")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def random_rays(rng, n, lo, hi, tmax=(0.05, 4.0)):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a slice of axis-parallel and exactly-zero-component directions (inf invDir, NaN slab terms)
    k = n // 16
    d[:k] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.choice([-1, 1], (k, 1)).astype(np.float32)
    d[k:2 * k, rng.integers(0, 3)] = 0.0
    d[k:2 * k] /= np.linalg.norm(d[k:2 * k], axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = o
    r[:, 4:7] = d
    r[:, 3] = rng.uniform(*tmax, n)
    return r


def main():
    assert pyref.available(), "build oracle/_ref first (raytracingrenderer_amd.build.build_ref)"
    write_synthetic_scene(SCENES["synth20k"][0], n_tris=20000, seed=3, width=128, height=96)
    digests = {}
    for name, (path, w, h, skip) in SCENES.items():
        if not os.path.isdir(path):
            continue
        r = pyref.RefScene(path, w, h, skip)
        d = r.export()
        digests[name] = {k: digest(d[k]) for k in ARRAYS}
        digests[name].update(n_tris=r.ntri, n_nodes=r.nnode, n_lights=r.nlight, width=r.W, height=r.H,
                             mat_info=digest(d["mat_info"][:, :2]), mat_f=digest(d["mat_f"]))
        if name in ("cornell256", "synth20k"):
            rng = np.random.default_rng(12345)
            lo, hi = (np.array([-1.5, -0.5, -1.5]), np.array([1.5, 2.5, 1.5])) if name == "cornell256" else (-1.3, 1.3)
            rays = random_rays(rng, 4096, lo, hi)
            pix = rng.integers(0, r.W * r.H, 4096).astype(np.uint32)
            np.savez_compressed(os.path.join(GOLD, "%s_rays.npz" % name), rays=rays, hits=r.traverse(rays),
                                visible=r.traverse_visible(rays), pixels=pix, camera_rays=r.camera_rays(pix),
                                **({k: d[k] for k in ARRAYS} if name == "cornell256" else {}))
    json.dump(digests, open(os.path.join(GOLD, "scene_digests.json"), "w"), indent=1, sort_keys=True)

    # BSDF::sample / evaluate known answers (scripted sampler draws)
    rng = np.random.default_rng(7)
    kat = []
    for kind in range(7):
        for _ in range(24):
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            wo = rng.normal(size=3); wo /= np.linalg.norm(wo)
            sd = np.concatenate([n, wo, rng.uniform(0, 3, 2)]).astype(np.float32)
            draws = rng.random(4).astype(np.float32)
            if rng.random() < 0.1:
                draws[:2] = 0.0  # r1 = 0 -> theta = acos(0) -> cos(theta) slightly negative (pdf quirk)
            alb = rng.uniform(0.05, 1, 3).astype(np.float32)
            ii, ee = (1.5, 1.0) if rng.random() < 0.5 else (1.33, 1.0)
            out = pyref.bsdf_sample(kind, alb, sd, draws, ii, ee, "libm")
            out_rtm = pyref.bsdf_sample(kind, alb, sd, draws, ii, ee, "rtm")
            kat.append({"kind": kind, "albedo": alb.tolist(), "sd": sd.tolist(), "draws": draws.tolist(),
                        "int_ior": ii, "ext_ior": ee, "out": out.tolist(),
                        "out_bits_libm": out.view(np.uint32).tolist(),
                        "out_bits_rtm": out_rtm.view(np.uint32).tolist()})
    json.dump(kat, open(os.path.join(GOLD, "bsdf_kat.json"), "w"))

    # Texture decode + sample, EnvironmentMap::evaluate, Film::save bytes
    env_dir = os.path.join(GOLD, "scenes", "cornell-mat")
    rs = pyref.RefScene(env_dir, 64, 48, False)
    tex_kat = {}
    dirs = rng.normal(size=(2048, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs[:8] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 1.0000001, 0], [-1, -0.0, 0]], np.float32)
    uv = rng.uniform(-3, 3, (2048, 2)).astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "env_tex_kat.npz"), dirs=dirs, env=rs.env_eval(rs.env_tex, dirs), uv=uv,
                        tex=rs.tex_sample(rs.env_tex, uv))
    for fn in ("bathroom/floor_tiles.png", "bathroom/rug_mask.png", "GI.hdr", "materialball/envmap.hdr",
               "bathroom/marble.jpg", "bathroom/picture1.jpg", "bathroom/wallpaper-1.jpg",
               "bathroom/wallpaper-2.jpg", "bathroom/wood.jpg", "bathroom/wood2.jpg"):
        p = os.path.join(REF, fn)
        if os.path.exists(p):
            t = pyref.load_texture(p)
            tex_kat[fn] = {"shape": list(t.shape), "sha256": digest(t)}
    json.dump(tex_kat, open(os.path.join(GOLD, "texture_decode_kat.json"), "w"), indent=1)
    film = np.random.default_rng(3).gamma(0.5, 2.0, (24, 40, 3)).astype(np.float32)
    film[0, :5] = 0.0
    film[1, :] = film[1, 0]  # long runs for the RLE encoder
    pyref.save_hdr("/tmp/rtg_golden_film.hdr", film, 3)
    np.savez_compressed(os.path.join(GOLD, "rgbe_kat.npz"), film=film, spp=3,
                        hdr=np.frombuffer(open("/tmp/rtg_golden_film.hdr", "rb").read(), np.uint8))
    light_fixtures()
    synth1m_digests()
    tonemap_fixture()
    print("golden fixtures written to", GOLD)


def light_fixtures():
    """Light tracing / instant radiosity pieces from the reference's own classes: the Camera members
    and Camera::projectOntoCamera (Scene.h:14-69) on random points, and AreaLight's emission sample
    (samplePositionFromLight + sampleDirectionFromLight + evaluate(-wi), Lights.h:30-80) on scripted
    draws, with the shared transcendentals (libref_rtm) so the oracle must match bit for bit.
    -> light_kat.npz"""
    rng = np.random.default_rng(99)
    out = {}
    for tag, (path, w, h) in {"cornell": (os.path.join(GOLD, "scenes", "cornell-box"), 96, 64),
                              "mat": (os.path.join(GOLD, "scenes", "cornell-mat"), 80, 60)}.items():
        r = pyref.RefScene(path, w, h, False, flavour="rtm")
        pts = rng.uniform(-1.2, 1.2, (2048, 3)).astype(np.float32) + np.float32([0, 1, 0])
        pts[:64] = rng.uniform(-50, 50, (64, 3)).astype(np.float32)  # many outside the frustum
        proj, state = r.camera_project(pts)
        area = [i for i, l in enumerate(r.export()["lights"].tolist()) if l >= 0]
        draws = rng.random((256, 4)).astype(np.float32)
        draws[:8, 2] = 0.0
        li = np.array([area[k % len(area)] for k in range(len(draws))], np.int32)
        emits = np.array([r.light_emit(li[k], draws[k]) for k in range(len(draws))], np.float32)
        out.update({tag + "_pts": pts, tag + "_proj": proj, tag + "_state": state, tag + "_draws": draws,
                    tag + "_li": li, tag + "_emit": emits})
    np.savez_compressed(os.path.join(GOLD, "light_kat.npz"), **out)


def synth1m_digests():
    """Config C3's scene (1M splitmix64 triangles, seed 20251015, 1024^2) through the reference loader
    and Scene::build (Geometry.h:325-398): digests of positions (the std::sort permutation), BVH
    nodes, lights and camera -> scene_digests.json["synth1m"]."""
    path = "/tmp/rtg_golden_synth1m"
    write_synthetic_scene(path, n_tris=1_000_000, seed=20251015, width=1024, height=1024)
    r = pyref.RefScene(path, 0, 0, False)
    d = r.export()
    dg = json.load(open(os.path.join(GOLD, "scene_digests.json")))
    dg["synth1m"] = {k: digest(d[k]) for k in ARRAYS}
    dg["synth1m"].update(n_tris=r.ntri, n_nodes=r.nnode, n_lights=r.nlight, width=r.W, height=r.H,
                         mat_info=digest(d["mat_info"][:, :2]), mat_f=digest(d["mat_f"]))
    json.dump(dg, open(os.path.join(GOLD, "scene_digests.json"), "w"), indent=1, sort_keys=True)


def add_scene_digests(names):
    """Loader + BVH digests of the listed SCENES entries only, merged into scene_digests.json (the
    other entries are left as they are)."""
    dg = json.load(open(os.path.join(GOLD, "scene_digests.json")))
    for name in names:
        path, w, h, skip = SCENES[name]
        r = pyref.RefScene(path, w, h, skip)
        d = r.export()
        dg[name] = {k: digest(d[k]) for k in ARRAYS}
        dg[name].update(n_tris=r.ntri, n_nodes=r.nnode, n_lights=r.nlight, width=r.W, height=r.H,
                        mat_info=digest(d["mat_info"][:, :2]), mat_f=digest(d["mat_f"]))
    json.dump(dg, open(os.path.join(GOLD, "scene_digests.json"), "w"), indent=1, sort_keys=True)


def rtm_digest_fixture(stride=127):
    """include/rtg_math.h's own outputs (no C library call) on every stride-th float and 2^20 atan2f
    pairs, as FNV-1a digests, with the platform they were checked on (glibc 2.35, FMA build: the
    exhaustive match of profiles/r03_libm_exhaustive.txt) -> rtm_digest.json. The CPU suite then
    pins the restatement itself on any host, and compares with the host's C library only where that
    library is the reference platform's."""
    import subprocess
    from oracle.pyoracle import BUILD
    out = subprocess.run([os.path.join(BUILD, "libm_check"), "digest", str(stride)], capture_output=True, text=True,
                         check=True).stdout.split()
    # "glibc 2.35 fma 1 avx2 1" / "stride N sinf H cosf H ..."
    plat = dict(zip(out[0:6:2], out[1:6:2]))
    dig = dict(zip(out[6::2], out[7::2]))
    json.dump({"platform": plat, "digests": dig, "command": "oracle/_build/libm_check digest %d" % stride},
              open(os.path.join(GOLD, "rtm_digest.json"), "w"), indent=1, sort_keys=True)


def device_digest_fixture():
    """The device records prepare_scene builds (tests/native/scene_digest, linked with this tree's
    librth / librtg) for the inputs of tests/test_scene_digest.py -> device_scene_digests.json.
    Regenerate only for an intended change of the records: the committed values were recorded from
    the tree before rtg_kernels.hip was split, and a refactor must reproduce them."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from raytracingrenderer_amd import build
    from test_scene_digest import INPUTS, run_digest
    build.build_host()
    build.build_device()
    exe = build.build_scene_digest()
    with tempfile.TemporaryDirectory() as tmp:
        out = {name: run_digest(exe, name, tmp) for name in INPUTS}
    json.dump(out, open(os.path.join(GOLD, "device_scene_digests.json"), "w"), indent=1, sort_keys=True)


def tonemap_fixture():
    """Film::tonemap (Imaging.h:233-242) of the reference's own Film class on a random film with
    negative, zero, tiny, saturating and non-finite values, at two exposures -> tonemap_kat.npz."""
    rng = np.random.default_rng(8)
    film = rng.gamma(0.7, 2.0, (17, 23, 3)).astype(np.float32)
    film[0, :6] = [[-1.0, 0.0, 1e9], [np.inf, -np.inf, np.nan], [1e-30, 1e-7, 3.0],
                   [2.99, 3.01, 2.2], [0.5, 0.25, 0.125], [-0.0, 7.5, 1e38]]
    out = {"film": film, "spp": np.int32(3)}
    for k, e in enumerate((1.0, 0.37)):
        out["exposure%d" % k] = np.float32(e)
        out["rgb%d" % k] = pyref.tonemap(film, 3, e)
    np.savez_compressed(os.path.join(GOLD, "tonemap_kat.npz"), **out)



# ---- reduced copies of the large reference scenes (tests/golden/scenes/<name>-small) ----
# The GPU parity tests render coffee_f, bathroom_f and materialball_f; the reference's folders hold
# 14 / 51 / 4 MB. These are subsets small enough to commit (every file far below 1 MiB): scene.json
# keeps the camera and the chosen instances unchanged, meshes and textures are byte copies, and the
# two files of materialball that are too large on their own are thinned (every 4th triangle of
# Mesh001.gem, envmap.hdr box-filtered to half size). Tests compare renderers on the same scene, so
# a subset checks the same code paths: textures (PNG, JPEG), every BSDF kind, area and env lights.
SMALL_BUDGET = {"coffee": 1300 << 10, "bathroom": 1800 << 10}
SMALL_MESH_CAP = {"coffee": 400 << 10, "bathroom": 160 << 10}
GEM_MAGIC = 4058972161
GEM_VERTEX = 44  # GEMStaticVertex on disk


def thin_gem(src, dst, keep_every):
    """Copy a static .gem keeping every `keep_every`-th triangle of each mesh (unused vertices dropped)."""
    import struct
    b = open(src, "rb").read()
    magic, animated, n_meshes = struct.unpack_from("<III", b, 0)
    assert magic == GEM_MAGIC and not animated
    at, out = 12, [struct.pack("<III", magic, 0, n_meshes)]
    for _ in range(n_meshes):
        start = at
        (n_props,) = struct.unpack_from("<I", b, at)
        at += 4
        for _ in range(2 * n_props):
            (ln,) = struct.unpack_from("<i", b, at)
            at += 4 + ln
        out.append(b[start:at])
        (nv,) = struct.unpack_from("<I", b, at)
        at += 4
        verts = np.frombuffer(b, np.uint8, nv * GEM_VERTEX, at).reshape(nv, GEM_VERTEX)
        at += nv * GEM_VERTEX
        (ni,) = struct.unpack_from("<I", b, at)
        at += 4
        idx = np.frombuffer(b, np.uint32, ni, at).reshape(-1, 3)[::keep_every]
        at += ni * 4
        used, inv = np.unique(idx, return_inverse=True)
        out += [struct.pack("<I", len(used)), verts[used].tobytes(), struct.pack("<I", inv.size),
                inv.astype(np.uint32).tobytes()]
    open(dst, "wb").write(b"".join(out))


def small_scene_fixtures():
    import shutil
    from raytracingrenderer_amd import read_hdr, save_hdr
    for name in ("coffee", "bathroom", "materialball"):
        src, dst = os.path.join(REF, name), os.path.join(GOLD, "scenes", name + "-small")
        os.makedirs(dst, exist_ok=True)
        scene = json.load(open(os.path.join(src, "scene.json")))
        size = lambda f: os.path.getsize(os.path.join(src, f))
        have = [i for i in scene["instances"]
                if all(os.path.exists(os.path.join(src, f)) for f in (i["filename"], i.get("reflectance", "")))]
        if name == "materialball":
            keep = have
        else:
            # lights first, then one round over the BSDF kinds and texture formats at a time, smallest
            # meshes first, until the byte budget is spent
            cand = [i for i in have if size(i["filename"]) <= SMALL_MESH_CAP[name] and size(i["reflectance"]) <= 512 << 10]
            kind = lambda i: (i["bsdf"], os.path.splitext(i["reflectance"])[1])
            groups = {}
            for i in sorted(cand, key=lambda i: size(i["filename"])):
                groups.setdefault(kind(i), []).append(i)
            keep, files, spent = [i for i in cand if "emission" in i], set(), 0
            order = [i for i in keep]
            while any(groups.values()):
                for k in sorted(groups):
                    if groups[k]:
                        order.append(groups[k].pop(len(groups[k]) // 2 if len(order) % 2 else 0))
            keep = []
            for i in order:
                if any(i is j for j in keep):
                    continue
                add = sum(size(f) for f in {i["filename"], i["reflectance"]} - files)
                if spent + add > SMALL_BUDGET[name]:
                    continue
                keep.append(i)
                files |= {i["filename"], i["reflectance"]}
                spent += add
            keep = [i for i in have if any(i is j for j in keep)]  # the scene's own order
        for i in keep:
            for f in (i["filename"], i["reflectance"]):
                if not os.path.exists(os.path.join(dst, f)) and size(f) <= 1000 << 10:
                    shutil.copyfile(os.path.join(src, f), os.path.join(dst, f))
        if name == "materialball":
            thin_gem(os.path.join(src, "Mesh001.gem"), os.path.join(dst, "Mesh001.gem"), 4)
            env = read_hdr(os.path.join(src, "envmap.hdr"))
            h, w = env.shape[0] // 2 * 2, env.shape[1] // 2 * 2
            half = env[:h, :w].reshape(h // 2, 2, w // 2, 2, 3).astype(np.float64).mean(axis=(1, 3)).astype(np.float32)
            save_hdr(os.path.join(dst, "envmap.hdr"), half, 1)
        if name == "coffee":
            shutil.copyfile(os.path.join(REF, "GI.hdr"), os.path.join(dst, "GI.hdr"))
        scene["instances"] = keep
        with open(os.path.join(dst, "scene.json"), "w") as f:
            json.dump(scene, f, indent=1)
        total = sum(os.path.getsize(os.path.join(dst, f)) for f in os.listdir(dst))
        print("%s-small: %d of %d instances, %d files, %.2f MB, largest %d KiB" % (
            name, len(keep), len(have), len(os.listdir(dst)), total / 1e6,
            max(os.path.getsize(os.path.join(dst, f)) for f in os.listdir(dst)) >> 10))


if __name__ == "__main__":
    if "--small-scenes" in sys.argv:
        small_scene_fixtures()
        sys.exit(0)
    if "--light-only" in sys.argv:
        light_fixtures()
    elif "--synth1m" in sys.argv:
        synth1m_digests()
    elif "--rtm-digest" in sys.argv:
        rtm_digest_fixture()
    elif "--materialball" in sys.argv:
        add_scene_digests(["materialball_f"])
    elif "--tonemap" in sys.argv:
        tonemap_fixture()
    elif "--device-digests" in sys.argv:
        device_digest_fixture()
    else:
        main()
