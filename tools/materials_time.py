#!/usr/bin/env python3
"""What the physical material model costs (rtg_set_material_model): per scene, the device time of an
--spp PATH frame at depth 4 (best of --reps waited-for renders after a warm-up, all --reps times kept)
under the reference model and under RTG_MATERIALS_PHYSICAL on the same handle, and their ratio. There is
no pass mark: the physical frame shades other surfaces (glossy bounces reach other parts of the scene, and
delta coats continue as specular paths). Scenes: the committed cornell-mat and coffee-small.
RTG_LIB selects an A/B build. Writes one JSON object (default profiles/materials_time.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(rt, spp, reps):
    """Device ms of `reps` waited-for spp-sample frames, and whether the last film is finite."""
    ms = []
    for _ in range(reps):
        rt.clear()
        rt.render(spp, first_sample=0)
        ms.append(rt.stats()["render_ms"])
    return ms, bool(np.isfinite(rt.film()[0]).all())


def measure(name, scene, spp, reps):
    from raytracingrenderer_amd import RayTracer
    from raytracingrenderer_amd import _native as N
    tags = [p.model for p in scene.material_params]
    out = {"scene": name, "width": scene.width, "height": scene.height, "spp": spp, "max_depth": 4, "reps": reps,
           "materials": {k: tags.count(v) for k, v in (("conductor", N.RTG_MODEL_CONDUCTOR), ("plastic", N.RTG_MODEL_PLASTIC),
                                                       ("orennayar", N.RTG_MODEL_ORENNAYAR),
                                                       ("reference", N.RTG_MODEL_REFERENCE))},
           "modes": {}}
    rt = RayTracer(scene, seed=1234, max_depth=4)
    for mode in ("reference", "physical", "reference again"):
        rt.set_material_model(mode.split()[0])
        frames(rt, spp, 1)  # warm-up: allocates the chunk buffers
        ms, finite = frames(rt, spp, reps)
        out["modes"][mode] = {"render_ms_device": [round(m, 3) for m in ms], "best_ms": round(min(ms), 3),
                              "finite_film": finite}
    out["physical_vs_reference"] = round(out["modes"]["physical"]["best_ms"] / out["modes"]["reference"]["best_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "cases": []}
    gold = os.path.join(ROOT, "tests", "golden", "scenes")
    for name in ("cornell-mat", "coffee-small"):
        s = loadScene(os.path.join(gold, name), width=a.size, height=a.size)
        res["cases"].append(measure(name, s, a.spp, a.reps))
        print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
