#!/usr/bin/env python3
"""What the illumination mode of variance-guided filtering costs and buys (rtg_svgf_illum_accumulate), on one
GPU at --size x --size for cornell-box and the C3 scene (synthetic 1M triangles). Per scene, best of --reps with
all kept, everything of one mode beside the other mode's in the same run and process:
  device ms of k_svgf_illum_prepare and k_svgf_illum_unpack on a moved frame, beside one k_svgf_atrous level of
  the same run (the filter time of a 5-level call over 5, and the difference between a 2-level and a 1-level
  call) and the chain's other stages in both modes;
  wall time of one moved frame through svgf(illumination=True) and through svgf().
Quality: tools/svgf_time.py's orbit (--poses poses, --degrees in all, 1 spp each under seeds seed + i): luminance
MSE against the handle's own --ref-spp film at the last pose under another seed of the raw last frame, of
svgf() and of svgf(illumination=True), each at plane_tolerance 0.01 and 0.001; non-finite pixels are left out
of every mean and counted. The figures are reported; there is no pass mark. RTG_LIB selects an A/B build.
Writes one JSON object (default profiles/svgf_illum_time.json)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from svgf_time import best  # noqa: E402
from temporal_time import LUM, orbit, records  # noqa: E402


def measure(name, scene, a):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "triangles": int(scene.desc.n_tris)}
    rt = RayTracer(scene, seed=a.seed)
    recs = [records(scene, f, t) for f, t in orbit(scene, a.poses, a.degrees)]
    nxt = [0]

    def move():
        nxt[0] += 1
        rt.set_camera(*recs[nxt[0] % len(recs)])
        rt.clear()
        rt.render(1, first_sample=0)

    rt.render(1)
    rt.svgf()  # warm-up: allocates both states, traces the first guides
    rt.svgf(illumination=True)

    # ---- device times of a moved frame, both modes, alternating
    keys = ("guide_pass_ms", "temporal_moments_ms", "variance_ms", "filter_5_levels_ms", "prepare_ms", "unpack_ms")
    dev = {"svgf": {k: [] for k in keys[:4]}, "illumination": {k: [] for k in keys}}
    wall = {"svgf": [], "illumination": []}
    for r in range(a.reps):
        for mode in ("svgf", "illumination") if r % 2 == 0 else ("illumination", "svgf"):
            illum = mode == "illumination"
            move()
            t0 = time.perf_counter()
            rt.svgf(illumination=illum)
            wall[mode].append((time.perf_counter() - t0) * 1e3)
            for k, v in zip(keys, rt.svgf_ms(illumination=illum)):
                dev[mode][k].append(v)
    out["moved_frame_device_ms"] = {m: {k: best(v) for k, v in d.items()} for m, d in dev.items()}
    out["moved_frame_wall_ms"] = {m: best(v) for m, v in wall.items()}
    out["moved_frame_wall_ratio_illumination_over_svgf"] = round(min(wall["illumination"]) / min(wall["svgf"]), 3)

    # ---- one k_svgf_atrous level of the same run
    def filter_ms(k):
        rt.svgf(iterations=k)
        return rt.svgf_ms()[3]

    one = min(filter_ms(1) for _ in range(a.reps))
    two = min(filter_ms(2) for _ in range(a.reps))
    five = min(filter_ms(5) for _ in range(a.reps))
    level = {"five_levels_over_5": round(five / 5, 4), "second_level_alone": round(two - one, 4)}
    both = min(dev["illumination"]["prepare_ms"]) + min(dev["illumination"]["unpack_ms"])
    out["one_k_svgf_atrous_level_ms"] = level
    out["prepare_plus_unpack_ms"] = round(both, 4)
    out["prepare_plus_unpack_below_one_level"] = bool(both < min(level.values()))

    # ---- quality over the orbit: both modes on one handle (their states are separate)
    rt.set_camera(*recs[-1])
    rt.seed = a.seed + 7919
    rt.clear()
    rt.render(a.ref_spp, first_sample=0)
    truth = (rt.film()[0].astype(np.float64) / a.ref_spp) @ LUM
    out["quality"] = {"poses": a.poses, "degrees": a.degrees, "ref_spp": a.ref_spp}
    for tol in (0.01, 0.001):
        rt.temporal_reset()
        for i, rec in enumerate(recs):
            rt.set_camera(*rec)
            rt.clear()
            rt.seed = a.seed + i
            rt.render(1, first_sample=0)
            raw = rt.film()[0].astype(np.float64)
            sv = rt.svgf(plane_tolerance=tol)
            il = rt.svgf(plane_tolerance=tol, illumination=True)
        lum = {"raw": raw @ LUM, "svgf": sv.astype(np.float64) @ LUM, "illumination": il.astype(np.float64) @ LUM}
        ok = np.isfinite(truth)
        for v in lum.values():
            ok &= np.isfinite(v)
        mse = {k: float(((v[ok] - truth[ok]) ** 2).mean()) for k, v in lum.items()}
        out["quality"]["plane_tolerance_%g" % tol] = {
            "mse": mse,
            "svgf_over_raw": round(mse["svgf"] / mse["raw"], 4),
            "illumination_over_raw": round(mse["illumination"] / mse["raw"], 4),
            "illumination_over_svgf": round(mse["illumination"] / mse["svgf"], 4),
            "non_finite_pixels_left_out": int((~ok).sum())}
    rt.seed = a.seed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--degrees", type=float, default=15.0)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_illum_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"),
           "bytes_per_pixel": {"prepare_read": 12 + 12 + 32 + 16 + 16, "prepare_written": 12 + 32, "unpack_read": 16 + 12,
                               "unpack_written": 12, "filter_tap": 64},
           "cases": []}
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a))
    with tempfile.TemporaryDirectory(prefix="rtg_svgf_illum_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
