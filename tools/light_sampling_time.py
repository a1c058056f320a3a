#!/usr/bin/env python3
"""What power-weighted light selection costs and gains (rtg_set_light_sampling), with the method of
tools/env_sampling_time.py: per scene, the device time of an --spp PATH frame (best of --reps waited-for
renders after a warm-up) under the uniform pick and under RTG_LIGHTS_POWER at the default uniform_share,
the table's build time, and the mean squared error of the frame's luminance against the same handle's
own --ref-spp film (rendered under another seed) for the uniform pick and for uniform_share 0, 0.125 and
0.5. Scenes: the 281-light table scene of tests/shade_scenes.py (140 emitter rectangles and the
environment), the committed bathroom-small and, when the full assets are staged (assets/), the bathroom.
RTG_LIB selects an A/B build. Writes one JSON object (default profiles/light_sampling_time.json)."""
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

SHARES = (0.0, 0.125, 0.5)


def measure(name, scene, spp, ref_spp, reps):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "lights": len(scene.lights), "spp": spp,
           "ref_spp": ref_spp, "settings": {}}
    for key, mode, share in [("uniform", "uniform", 0.125)] + [("power %g" % s, "power", s) for s in SHARES]:
        rt = RayTracer(scene, seed=1234)
        rt.set_light_sampling(mode, share)
        t = rt.light_table()
        frame(rt, spp, 1234)  # warm-up: allocates the chunk buffers
        img, ms = frame(rt, spp, 1234, reps)
        chunk = 4096  # the reference in chunks of sample indices below RTG_MAX_SAMPLES_PER_KEY
        rt.seed = 99991
        rt.clear()
        for s0 in range(0, ref_spp, chunk):
            rt.render(min(chunk, ref_spp - s0), first_sample=s0)
        f, n = rt.film()
        ref = lum(f, n)
        e, bad = mse(img, ref)
        out["settings"][key] = {"render_ms_device": round(ms, 3), "table": None if t is None else len(t["prob"]),
                                "table_build_ms": None if t is None else round(t["build_ms"], 3),
                                "max_pmf_times_n": None if t is None else
                                round(float(max(t["pmf_self"].max(), t["pmf_alias"].max())) * len(t["prob"]), 3),
                                "mse_equal_spp": e, "non_finite_pixels": bad,
                                "ref_mean": float(ref[np.isfinite(ref)].mean())}
        del rt
    u = out["settings"]["uniform"]
    for s in SHARES:
        p = out["settings"]["power %g" % s]
        p["time_vs_uniform"] = round(p["render_ms_device"] / u["render_ms_device"], 4)
        p["mse_uniform_vs_this"] = round(u["mse_equal_spp"] / p["mse_equal_spp"], 3)
        p["ref_mean_vs_uniform"] = round(p["ref_mean"] / u["ref_mean"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_sampling_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    from shade_scenes import write_table_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "cases": []}
    gold = os.path.join(ROOT, "tests", "golden", "scenes")
    with tempfile.TemporaryDirectory() as tmp:  # (the scene is in memory once loaded)
        scenes = [("table scene, 281 lights", loadScene(write_table_scene(tmp, 140, 5, envmap=True), width=a.size,
                                                        height=a.size)),
                  ("bathroom-small", loadScene(os.path.join(gold, "bathroom-small"), width=a.size, height=a.size))]
        bath = os.path.join(ROOT, "assets", "bathroom")
        if os.path.isdir(bath):
            scenes.append(("bathroom", loadScene(bath, width=a.size, height=a.size, skip_missing=True)))
        else:
            res["note"] = "assets/ not staged: the full bathroom was not measured"
    for name, s in scenes:
        res["cases"].append(measure(name, s, a.spp, a.ref_spp, a.reps))
        print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
