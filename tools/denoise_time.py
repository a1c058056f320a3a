#!/usr/bin/env python3
"""Device time of the denoiser (rtg_denoise_ms: pack, K a-trous launches, unpack) on the C3 scene
(synthetic 1M triangles) and cornell-box at 1024x1024, best of 5 after a warm-up with the guides
cached, for K = 1, 2 and 5 (the differences give the step-1 and step-2 launches: the small-step LDS
A/B of DESIGN.md "Denoiser"), with a 64-spp frame of the same process for scale, and the bytes an
iteration requests against the L2 rate of MI355X_MICROARCH.md. RTG_LIB selects an A/B build
(tools/mkab.sh). Writes one JSON object (default profiles/denoise_time.json)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLOUR_BYTES, GUIDE_BYTES, TAPS = 16, 32, 25
L2_BYTES_PER_S = 34.5e12  # MI355X_MICROARCH.md "L2 (per XCD)": 34.5 TB/s aggregate


def measure(name, scene, size, reps):
    from raytracingrenderer_amd import RayTracer
    rt = RayTracer(scene, seed=1234)
    rt.render(1)
    rt.denoise()  # warm-up: renders and caches the guides, allocates the buffers
    out = {"scene": name, "width": size, "height": size}
    for k in (1, 2, 5):
        best = min((rt.denoise(iterations=k), rt.denoise_ms())[1] for _ in range(reps))
        out["denoise_ms_k%d" % k] = round(best, 4)
    out["step2_launch_ms"] = round(out["denoise_ms_k2"] - out["denoise_ms_k1"], 4)  # K = 2 adds the step-2 launch
    out["per_iteration_ms_k5"] = round(out["denoise_ms_k5"] / 5, 4)
    frames = []
    for _ in range(3):
        rt.clear()
        t0 = time.perf_counter()
        rt.render(64, first_sample=0)
        frames.append((time.perf_counter() - t0) * 1e3)
    out["render_64spp_ms"] = round(min(frames), 3)
    rt.clear()
    t0 = time.perf_counter()
    rt.render(1, first_sample=0)
    out["render_1spp_ms_waited"] = round((time.perf_counter() - t0) * 1e3, 3)
    pix = size * size
    req = TAPS * (COLOUR_BYTES + GUIDE_BYTES) * pix + COLOUR_BYTES * pix
    out["bytes_requested_per_iteration"] = req
    out["l2_time_for_those_bytes_ms"] = round(req / L2_BYTES_PER_S * 1e3, 4)
    out["fraction_of_l2_rate_k5"] = round(req / L2_BYTES_PER_S * 1e3 / out["per_iteration_ms_k5"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "record_bytes": {"colour": COLOUR_BYTES, "guide": GUIDE_BYTES},
           "l2_bytes_per_s": L2_BYTES_PER_S, "cases": []}
    with tempfile.TemporaryDirectory(prefix="rtg_denoise_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a.size, a.reps))
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a.size, a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
