#!/usr/bin/env python3
"""What variance-guided filtering of the temporal history costs and buys (rtg_svgf_accumulate), on one GPU at
--size x --size for cornell-box and the C3 scene (synthetic 1M triangles). Per scene, best of --reps with
all kept:
  device ms of each stage of the chain: the geometry guide pass, the temporal + moments kernel (camera moved
  and unchanged), the variance kernel on a first frame (every pixel takes the 7x7 branch) and on a steady one
  (none does), and each filter level (the filter time of a call with i + 1 levels minus that of one with i),
  beside k_dn_atrous's levels measured the same way in the same run (rtg_denoise_ms, whose pack and unpack
  cancel in the difference); the albedo / normal guides as the wall time of rtg_denoise_guides without a
  copy (two 1-sample renders and a host wait: the library reports no device time for them);
  a queued 1-spp frame of the same process; rt.temporal() alone;
  wall time of one moved frame through svgf() and through the host-chained path there was before it:
  temporal() -> guides() -> denoise_images().
Quality: an orbit of --poses poses (--degrees in all), 1 spp each under seeds seed + i: luminance MSE against
the handle's own --ref-spp film at the last pose under another seed of the raw last frame, of temporal(), of
temporal() then the a-trous denoiser at its defaults, and of svgf(), each at plane_tolerance 0.01 and 0.001;
non-finite pixels are left out of every mean and counted (tools/temporal_time.py's rule). The figures are
reported; there is no pass mark. RTG_LIB selects an A/B build. Writes one JSON object (default
profiles/svgf_time.json)."""
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
from temporal_time import LUM, orbit, records  # noqa: E402


def best(v):
    return {"best": round(min(v), 4), "all": [round(x, 4) for x in v]}


def levels(totals):
    """Per-level times from the totals of calls with 1, 2, ... levels."""
    return [round(totals[0], 4)] + [round(b - a, 4) for a, b in zip(totals, totals[1:])]


def measure(name, scene, a):
    from raytracingrenderer_amd import RayTracer, denoise_images
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
    rt.svgf()  # warm-up: allocates the states, traces the first guides
    rt.temporal()
    rt.denoise()

    # ---- device times of the stages
    g_ms, acc_moved, acc_same, var_first, var_steady, guides_wall = [], [], [], [], [], []
    for r in range(a.reps):
        rt.temporal_reset()
        move()
        rt.svgf()  # a first frame: no history, every pixel's variance is spatial
        var_first.append(rt.svgf_ms()[2])
        for _ in range(4):
            rt.svgf()  # camera unchanged: len grows to 5 >= min_history
        _, acc, var, _ = rt.svgf_ms()
        acc_same.append(acc)
        var_steady.append(var)
        move()
        rt.svgf()  # moved: guide pass, guides, reprojection
        g, acc, _, _ = rt.svgf_ms()
        g_ms.append(g)
        acc_moved.append(acc)
        rt.set_camera(*recs[(nxt[0] + 5) % len(recs)])  # drops the guides
        t0 = time.perf_counter()
        assert rt._lib.rtg_denoise_guides(rt.handle, None, None) == 0
        guides_wall.append((time.perf_counter() - t0) * 1e3)
    out["guide_pass_ms"] = best(g_ms)
    out["albedo_normal_guides_wall_ms"] = best(guides_wall)
    out["temporal_moments_moved_ms"] = best(acc_moved)
    out["temporal_moments_unchanged_ms"] = best(acc_same)
    out["variance_first_frame_ms"] = best(var_first)
    out["variance_steady_frame_ms"] = best(var_steady)

    # ---- the filter's levels beside k_dn_atrous's, the same frame, the same run
    move()
    for _ in range(5):
        rt.svgf()

    def svgf_filter_ms(k):
        rt.svgf(iterations=k)
        return rt.svgf_ms()[3]

    def denoise_ms(k):
        rt.denoise(iterations=k)
        return rt.denoise_ms()

    sv_tot = [min(svgf_filter_ms(k) for _ in range(a.reps)) for k in range(1, 6)]
    dn_tot = [min(denoise_ms(k) for _ in range(a.reps)) for k in range(1, 6)]
    out["svgf_filter_total_ms_by_iterations"] = [round(x, 4) for x in sv_tot]
    out["denoise_total_ms_by_iterations"] = [round(x, 4) for x in dn_tot]
    out["k_svgf_atrous_level_ms"] = levels(sv_tot)
    out["k_dn_atrous_level_ms"] = levels(dn_tot)[1:]  # the first total holds the pack and the unpack
    pairs = list(zip(out["k_svgf_atrous_level_ms"][1:], out["k_dn_atrous_level_ms"]))
    out["level_ratio_svgf_over_dn"] = [round(s / d, 3) for s, d in pairs]
    out["level_ratio_expected_from_load_counts"] = round(109 / 75, 3)

    # ---- a queued 1-spp frame of the same process (best of three rounds: the first allocates the slots)
    rounds = []
    for _ in range(3):
        rt.clear()
        rt.render(1, first_sample=0)
        t0 = time.perf_counter()
        for i in range(a.frames):
            rt.render(1, first_sample=1 + i, sync=False)
        rt.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / a.frames)
    out["queued_1spp_frame_ms"] = best(rounds)

    # ---- rt.temporal() alone, and one moved frame through both chains (wall)
    t_g, t_a, w_svgf, w_host, w_temporal = [], [], [], [], []
    for r in range(a.reps):
        move()
        t0 = time.perf_counter()
        rt.temporal()
        w_temporal.append((time.perf_counter() - t0) * 1e3)
        g, acc = rt.temporal_ms()
        t_g.append(g)
        t_a.append(acc)
        move()
        t0 = time.perf_counter()
        tmp = rt.temporal()
        alb, nrm = rt.guides()
        denoise_images(tmp, alb, nrm)
        w_host.append((time.perf_counter() - t0) * 1e3)
        move()
        t0 = time.perf_counter()
        rt.svgf()
        w_svgf.append((time.perf_counter() - t0) * 1e3)
    out["temporal_alone_moved"] = {"guide_pass_ms": best(t_g), "k_temporal_ms": best(t_a), "wall_ms": best(w_temporal)}
    out["moved_frame_wall_ms"] = {"svgf": best(w_svgf), "temporal_guides_denoise_images": best(w_host)}
    out["moved_frame_wall_ratio_svgf_over_host_chain"] = round(min(w_svgf) / min(w_host), 3)

    # ---- quality over the orbit
    b = RayTracer(scene, seed=a.seed)
    rt.set_camera(*recs[-1])
    rt.seed = a.seed + 7919
    rt.clear()
    rt.render(a.ref_spp, first_sample=0)
    truth = (rt.film()[0].astype(np.float64) / a.ref_spp) @ LUM
    rt.seed = a.seed
    out["quality"] = {"poses": a.poses, "degrees": a.degrees, "ref_spp": a.ref_spp}
    for tol in (0.01, 0.001):
        rt.temporal_reset()
        b.temporal_reset()
        for i, rec in enumerate(recs):
            for h in (rt, b):
                h.set_camera(*rec)
                h.clear()
                h.seed = a.seed + i
                h.render(1, first_sample=0)
            raw = rt.film()[0].astype(np.float64)
            sv = rt.svgf(plane_tolerance=tol)
            tmp = b.temporal(plane_tolerance=tol)
        dn = denoise_images(tmp, *b.guides())
        lum = {"raw": raw @ LUM, "temporal": tmp.astype(np.float64) @ LUM,
               "temporal_then_denoise": dn.astype(np.float64) @ LUM, "svgf": sv.astype(np.float64) @ LUM}
        ok = np.isfinite(truth)
        for v in lum.values():
            ok &= np.isfinite(v)
        mse = {k: float(((v[ok] - truth[ok]) ** 2).mean()) for k, v in lum.items()}
        out["quality"]["plane_tolerance_%g" % tol] = {
            "mse": mse,
            "svgf_over_raw": round(mse["svgf"] / mse["raw"], 4),
            "svgf_over_temporal": round(mse["svgf"] / mse["temporal"], 4),
            "svgf_over_temporal_then_denoise": round(mse["svgf"] / mse["temporal_then_denoise"], 4),
            "temporal_over_raw": round(mse["temporal"] / mse["raw"], 4),
            "non_finite_pixels_left_out": int((~ok).sum()),
            "of_them_non_finite_in_the_reference": int((~np.isfinite(truth)).sum())}
    rt.seed = a.seed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--degrees", type=float, default=15.0)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"),
           "record_bytes": {"history": 16, "moments": 8, "colour_variance": 16, "denoiser_guide": 32, "geometry_guide": 32},
           "cases": []}
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a))
    with tempfile.TemporaryDirectory(prefix="rtg_svgf_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
