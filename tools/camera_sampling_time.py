#!/usr/bin/env python3
"""What per-sample camera rays cost (rtg_set_camera_sampling): a 64-spp frame of the C3 scene
(synthetic 1M triangles) and of cornell-box at 1024x1024, best of 3 waited-for renders after a
warm-up, with no filter (one camera ray per pixel, shared by its samples), a box filter, a tent
filter, and a box filter with the thin lens on. Per case: wall and device ms, the rays of
rtg_stats, traced_camera_rays, rtg_launch_rays[0] (from one more render with RTG_OPT_TIMING) and
the time relative to the default mode. RTG_LIB selects an A/B build (tools/mkab.sh). Writes one JSON
object (default profiles/camera_sampling_time.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("none", dict(filter="none")), ("box", dict(filter="box")), ("tent", dict(filter="tent")),
            ("box+lens", dict(filter="box", lens_radius=0.05, focal_distance=5.0))]


def launch_rays(rt):
    from raytracingrenderer_amd import _native as N
    lib = N.rtg()
    n = C.c_uint32()
    buf = (C.c_uint64 * 64)()
    if lib.rtg_launch_rays(rt.handle, buf, 64, C.byref(n)) != 0:
        raise RuntimeError(lib.rtg_last_error().decode())
    return [int(buf[i]) for i in range(min(n.value, 64))]


def measure(name, scene, spp, reps):
    from raytracingrenderer_amd import RayTracer
    from raytracingrenderer_amd import _native as N
    out = {"scene": name, "width": scene.width, "height": scene.height, "spp": spp, "settings": []}
    for label, setting in SETTINGS:
        rt = RayTracer(scene, seed=1234)
        rt.set_camera_sampling(**setting)
        rt.render(spp, first_sample=0)  # warm-up: allocates the chunk buffers
        wall, dev, st = [], [], None
        for _ in range(reps):
            rt.clear()
            t0 = time.perf_counter()
            rt.render(spp, first_sample=0)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = rt.stats()
            dev.append(st["render_ms"])
        cast = st["extension_rays"] + st["shadow_rays"]  # as the reference casts them: a camera ray per sample
        traced = cast - st["paths"] + st["traced_camera_rays"]  # what the traversal walked
        rt.clear()
        rt.set_options(flags=rt.flags | N.RTG_OPT_TIMING)
        rt.render(spp, first_sample=0)
        lr = launch_rays(rt)
        out["settings"].append({"setting": label, **rt.camera_sampling(), "render_ms_wall": round(min(wall), 3),
                                "render_ms_device": round(min(dev), 3), "paths": st["paths"],
                                "extension_rays": st["extension_rays"], "shadow_rays": st["shadow_rays"],
                                "traced_camera_rays": st["traced_camera_rays"], "chunk_samples": st["chunk_samples"],
                                "launch_rays_0": lr[0] if lr else None,
                                "mrays_traced_per_s": round(traced / (min(dev) * 1e-3) / 1e6, 1),
                                "mrays_reference_equivalent_per_s": round(cast / (min(dev) * 1e-3) / 1e6, 1)})
        del rt
    base = out["settings"][0]["render_ms_device"]
    for s in out["settings"]:
        s["time_vs_none"] = round(s["render_ms_device"] / base, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_sampling_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "bounce0": "eight segments (Counters::ne8, fetch8)", "cases": []}
    with tempfile.TemporaryDirectory(prefix="rtg_camera_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a.spp, a.reps))
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a.spp, a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
