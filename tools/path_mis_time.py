#!/usr/bin/env python3
"""What the path tracer's MIS costs and buys (rtg_set_path_mis): per scene, the device time of an --spp PATH
frame at depth 4 (best of --reps waited-for renders after a warm-up, all --reps times kept) with the mode
off, on and off again on the same handle, and the mean squared error of the --spp film's luminance
against a --ref-spp render of another seed: of the same mode where the two modes have different
expectations (an environment light: PATH counts it twice), of PATH where they have the same. The
reference's own noise (spp / ref-spp of the frame's) is inside both errors. equal_time_gain =
(mse_off * ms_off) / (mse_on * ms_on): above 1 the mode wins at equal time, below 1 it loses. There is no
pass mark. Scenes: the committed cornell-box; a conductor floor of roughness 1e-4 (alpha 0.0162, just
above RTG_ALPHA_DELTA) under a 1.6 x 1.6 emitter above its far edge, where the camera's reflections arrive,
written here from cornell-box's meshes, under the physical material model; the committed materialball-small under luminance sampling of its environment.
RTG_LIB selects an A/B build. Writes one JSON object (default profiles/path_mis_time.json)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "scenes")
LUM = np.array([0.2126, 0.7152, 0.0722])


def write_glossy_floor(out_dir, size):
    """cornell-box's floor as a conductor of roughness 1e-4 and one large emitter at y = 1.98 above its far
    edge, seen from above (the camera of the tests' floor scenes): the floor shows the emitter's reflection."""
    box = os.path.relpath(os.path.join(GOLD, "cornell-box"), out_dir)
    base = json.load(open(os.path.join(GOLD, "cornell-box", "scene.json")))
    floor = {k: v for k, v in base["instances"][0].items() if k in ("filename", "world", "reflectance")}
    floor["filename"] = os.path.join(box, floor["filename"])
    floor["reflectance"] = os.path.join(box, floor["reflectance"])
    floor.update({"bsdf": "conductor", "roughness": "0.0001", "eta": "1.65 0.88 0.52", "k": "9.2 6.3 4.8"})
    emitter = {"filename": os.path.join(box, "Rectangle.gem"),
               "world": [0.8, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.98, 0.0, 0.8, 0.0, -1.5, 0.0, 0.0, 0.0, 1.0],
               "reflectance": os.path.join(box, "0_0_0_1.0.png"), "bsdf": "diffuse", "emission": "6 5 4"}
    scene = {"fov": base["fov"], "from": "0.0 2.5 4.0", "to": "0.0 0.0 0.0", "up": base["up"],
             "width": str(size), "height": str(size), "instances": [floor, emitter]}
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(scene, f)
    return out_dir


def frames(rt, spp, reps):
    """Device ms of `reps` waited-for spp-sample frames, and the last film's mean (H, W, 3)."""
    ms = []
    for _ in range(reps):
        rt.clear()
        rt.render(spp, first_sample=0)
        ms.append(rt.stats()["render_ms"])
    return ms, rt.film()[0].astype(np.float64) / spp


def reference(rt, spp):
    """The mean of `spp` samples under the handle's settings and another seed, in chunks the sample key allows."""
    seed, rt.seed = rt.seed, rt.seed + 7919
    rt.clear()
    done = 0
    while done < spp:
        n = min(256, spp - done)
        rt.render(n, first_sample=done)
        done += n
    film = rt.film()[0].astype(np.float64) / spp
    rt.seed = seed
    return film


def measure(name, scene, spp, reps, ref_spp, physical=False, luminance=False):
    from raytracingrenderer_amd import RayTracer
    env_light = any(t < 0 for t in scene.lights)
    out = {"scene": name, "width": scene.width, "height": scene.height, "spp": spp, "max_depth": 4, "reps": reps,
           "ref_spp": ref_spp, "lights": len(scene.lights), "environment_light": env_light,
           "material_model": "physical" if physical else "reference",
           "env_sampling": "luminance" if luminance else "uniform", "modes": {}}
    rt = RayTracer(scene, seed=1234, max_depth=4)
    rt.set_material_model("physical" if physical else "reference")
    rt.set_env_sampling("luminance" if luminance else "uniform")
    films = {}
    for mode in ("off", "power", "off again"):
        rt.set_path_mis(mode.split()[0])
        frames(rt, spp, 1)  # warm-up: allocates the chunk buffers
        ms, films[mode] = frames(rt, spp, reps)
        out["modes"][mode] = {"render_ms_device": [round(m, 3) for m in ms], "best_ms": round(min(ms), 3),
                              "finite_film": bool(np.isfinite(films[mode]).all())}
    refs = {}
    for mode in ("off", "power") if env_light else ("off",):
        rt.set_path_mis(mode)
        refs[mode] = reference(rt, ref_spp)
    # pixels that are finite in every film compared (PATH carries a 0 / 0 throughput on after a cosine sample
    # on the horizon: a few pixels per frame are not)
    ok = np.ones(films["off"].shape[:2], bool)
    for f in list(refs.values()) + [films["off"], films["power"]]:
        ok &= np.isfinite(f).all(axis=2)
    out["pixels_compared"] = int(ok.sum())
    for mode in ("off", "power"):
        ref = refs.get(mode, refs["off"])
        out["modes"][mode]["non_finite_pixels"] = int((~np.isfinite(films[mode]).all(axis=2)).sum())
        err = (films[mode][ok] - ref[ok]) @ LUM
        out["modes"][mode]["mse_luminance"] = float(np.mean(err * err))
        out["modes"][mode]["mse_against"] = "%d spp of PATH%s" % (ref_spp, " + MIS" if mode in refs and mode == "power" else "")
        out["modes"][mode]["mean_luminance"] = float(np.mean(films[mode][ok] @ LUM))
    off, on = out["modes"]["off"], out["modes"]["power"]
    out["power_vs_off_time"] = round(on["best_ms"] / off["best_ms"], 4)
    out["power_vs_off_mse"] = round(on["mse_luminance"] / off["mse_luminance"], 4)
    out["equal_time_gain"] = round((off["mse_luminance"] * off["best_ms"]) / (on["mse_luminance"] * on["best_ms"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_mis_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        cases = [("cornell-box", os.path.join(GOLD, "cornell-box"), {}),
                 ("glossy floor (conductor, roughness 1e-4) under a large emitter", write_glossy_floor(tmp, a.size),
                  {"physical": True}),
                 ("materialball-small", os.path.join(GOLD, "materialball-small"), {"luminance": True})]
        for name, path, kw in cases:
            s = loadScene(path, width=a.size, height=a.size)
            res["cases"].append(measure(name, s, a.spp, a.reps, a.ref_spp, **kw))
            print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
