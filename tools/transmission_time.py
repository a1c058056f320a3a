#!/usr/bin/env python3
"""What rough dielectric transmission costs (RayTracer.set_material_model("physical", transmission=True)):
on the committed cornell-mat scene at --size squared, the device time of an --spp PATH frame at depth 4
(--reps waited-for renders after a warm-up, all times kept, the best one compared) under "physical",
"physical + transmission" and "physical" again on one handle, then the same under set_path_mis("power").
There is no pass mark: the mode shades another surface (the rough dielectric refracts paths into the box
behind it where the stub scatters them back), so the two frames do different work. RTG_LIB selects an A/B
build. Writes one JSON object (default profiles/transmission_time.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "scenes")


def frames(rt, spp, reps):
    """Device ms of `reps` waited-for spp-sample frames, and the last film's mean (H, W, 3)."""
    ms = []
    for _ in range(reps):
        rt.clear()
        rt.render(spp, first_sample=0)
        ms.append(rt.stats()["render_ms"])
    return ms, rt.film()[0].astype(np.float64) / spp


def measure(scene, spp, reps, mis):
    from raytracingrenderer_amd import RayTracer
    rt = RayTracer(scene, seed=1234, max_depth=4)
    rt.set_path_mis(mis)
    out = {"path_mis": mis, "modes": {}}
    for mode, tr in (("physical", False), ("physical + transmission", True), ("physical again", False)):
        rt.set_material_model("physical", transmission=tr)
        frames(rt, spp, 1)  # warm-up: allocates the chunk buffers
        ms, film = frames(rt, spp, reps)
        out["modes"][mode] = {"render_ms_device": [round(m, 3) for m in ms], "best_ms": round(min(ms), 3),
                              "finite_film": bool(np.isfinite(film).all()),
                              "mean_luminance": float(np.mean(film[np.isfinite(film).all(axis=2)] @ [0.2126, 0.7152, 0.0722]))}
    out["transmission_vs_physical_time"] = round(out["modes"]["physical + transmission"]["best_ms"] /
                                                 out["modes"]["physical"]["best_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmission_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    s = loadScene(os.path.join(GOLD, "cornell-mat"), width=a.size, height=a.size)
    res = {"lib": os.environ.get("RTG_LIB", "product"), "scene": "cornell-mat", "width": s.width, "height": s.height,
           "spp": a.spp, "max_depth": 4, "reps": a.reps, "cases": []}
    for mis in ("off", "power"):
        res["cases"].append(measure(s, a.spp, a.reps, mis))
        print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
