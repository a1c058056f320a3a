#!/usr/bin/env python3
"""What per-shading-point light selection costs and gains (rtg_set_light_grid), with the method of
tools/light_sampling_time.py: per scene, the device time of an --spp PATH frame (best of --reps waited-for
renders after a warm-up) under the uniform pick, under RTG_LIGHTS_POWER and under the grid at cells 4, 8 and
16, each against the same run's power frame; the grid's host build time (the best of three builds, and the
first, which also pays first touches) and table bytes; and the mean squared
error of the frame's luminance against one --ref-spp film of the uniform pick (another seed), per frame and
at equal time (the per-frame error times the frame's time over the power frame's: the error of a Monte Carlo
frame falls as one over its samples). Scenes: the 64-light hall and a 512-light hall of
tests/light_grid_scenes.py, the 281-light table scene of tests/shade_scenes.py, and the committed
bathroom-small, whose two lights show the grid's pure cost. RTG_LIB selects an A/B build. Writes one JSON object
(default profiles/light_grid_time.json)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from env_sampling_time import frame, lum, mse  # noqa: E402

CELLS = (4, 8, 16)


def measure(name, scene, spp, ref_spp, reps):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "lights": len(scene.lights), "spp": spp,
           "ref_spp": ref_spp, "settings": {}}
    rt = RayTracer(scene, seed=99991)  # the reference: the uniform pick, in chunks of sample indices
    for s0 in range(0, ref_spp, 4096):
        rt.render(min(4096, ref_spp - s0), first_sample=s0)
    f, n = rt.film()
    ref = lum(f, n)
    del rt
    for key, mode, cells in [("uniform", "uniform", 0), ("power", "power", 0)] + [("grid %d" % c, "power", c) for c in CELLS]:
        rt = RayTracer(scene, seed=1234)
        rt.set_light_sampling(mode)
        rt.set_light_grid(cells)
        g = rt.light_grid()
        build_ms = [g["build_ms"]]
        for _ in range(2 if g["active"] else 0):  # the build again, twice (the first one also pays first touches)
            rt.set_light_grid(cells + 1)  # (another cells and back: both rebuild)
            rt.set_light_grid(cells)
            build_ms.append(rt.light_grid()["build_ms"])
        frame(rt, spp, 1234)  # warm-up: allocates the chunk buffers
        img, ms = frame(rt, spp, 1234, reps)
        e, bad = mse(img, ref)
        out["settings"][key] = {"render_ms_device": round(ms, 3), "grid_active": g["active"],
                                "dims": [int(d) for d in g["dims"]], "table_bytes": 16 * g["n_entries"],
                                "grid_build_ms": round(min(build_ms), 3) if g["active"] else None,
                                "grid_build_ms_first": round(build_ms[0], 3) if g["active"] else None,
                                "mse_per_frame": e, "non_finite_pixels": bad}
        del rt
    p = out["settings"]["power"]
    for key, v in out["settings"].items():
        v["time_vs_power"] = round(v["render_ms_device"] / p["render_ms_device"], 4)
        v["mse_power_vs_this_per_frame"] = round(p["mse_per_frame"] / v["mse_per_frame"], 3)
        v["mse_power_vs_this_equal_time"] = round(p["mse_per_frame"] / (v["mse_per_frame"] * v["time_vs_power"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_grid_time.json"))
    a = ap.parse_args()
    from light_grid_scenes import write_hall_scene
    from raytracingrenderer_amd import loadScene
    from shade_scenes import write_table_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "cases": []}
    gold = os.path.join(ROOT, "tests", "golden", "scenes")
    with tempfile.TemporaryDirectory() as tmp:  # (a scene is in memory once loaded)
        scenes = [("hall, 64 lights", loadScene(write_hall_scene(os.path.join(tmp, "h64"), 32, a.size, a.size))),
                  ("hall, 512 lights", loadScene(write_hall_scene(os.path.join(tmp, "h512"), 256, a.size, a.size))),
                  ("table scene, 281 lights", loadScene(write_table_scene(os.path.join(tmp, "t"), 140, 5, envmap=True),
                                                        width=a.size, height=a.size)),
                  ("bathroom-small", loadScene(os.path.join(gold, "bathroom-small"), width=a.size, height=a.size))]
    for name, s in scenes:
        res["cases"].append(measure(name, s, a.spp, a.ref_spp, a.reps))
        print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
