#!/usr/bin/env python3
"""What a moving camera costs and what temporal accumulation buys (rtg_set_camera, rtg_geometry_guide,
rtg_temporal_accumulate), on one GPU at --size x --size for cornell-box and the C3 scene (synthetic 1M
triangles). Per scene, device ms (best of --reps, all kept) of the guide pass, of an accumulate with the
camera unchanged and of one after a move (guide pass + k_temporal), beside a queued 1-spp frame of the same
process (wall time of --frames queued frames over their count) and the host time of rtg_set_camera beside
a destroy + create of the same scene. Quality: an orbit of --poses poses (--degrees in all, about the
centre of the scene's bounds), 1 spp each under seeds seed + i: luminance MSE of the last raw frame and of
the temporal output against the handle's own --ref-spp film at the last pose under another seed, for the
default parameters and for plane_tolerance 0.001. The figures are reported; there is no pass mark.
RTG_LIB selects an A/B build. Writes one JSON object (default profiles/temporal_time.json)."""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LUM = np.array([0.2126, 0.7152, 0.0722])


def rot(v, axis, deg):
    k = axis / np.linalg.norm(axis)
    a = math.radians(deg)
    return v * math.cos(a) + np.cross(k, v) * math.sin(a) + k * np.dot(k, v) * (1 - math.cos(a))


def orbit(scene, n, degrees):
    p = scene.camera_pose
    frm, up = np.asarray(p["from_"], np.float64), np.asarray(p["up"], np.float64)
    c = 0.5 * (np.asarray(scene.info.bounds_min[:], np.float64) + np.asarray(scene.info.bounds_max[:], np.float64))
    return [(c + rot(frm - c, up, degrees * i / max(n - 1, 1)), c) for i in range(n)]


def records(scene, frm, to):
    from raytracingrenderer_amd import look_at
    p = scene.camera_pose
    return look_at(frm, to, p["up"], p["fov"], scene.width, scene.height, p["flip_x"])


def measure(name, scene, a):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "triangles": int(scene.desc.n_tris)}
    t0 = time.perf_counter()
    rt = RayTracer(scene, seed=a.seed)
    out["create_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    poses = orbit(scene, a.poses, a.degrees)
    recs = [records(scene, f, t) for f, t in poses]
    rt.render(1)
    rt.temporal()  # warm-up: allocates the state, traces the first guide

    # device times: guide pass, unchanged accumulate, moved accumulate
    guide, same, moved_g, moved_a = [], [], [], []
    for r in range(a.reps):
        rt.set_camera(*recs[(r + 1) % len(recs)])
        rt.clear()
        rt.render(1, first_sample=0)
        rt.temporal()  # moved: guide pass + reprojection
        g, acc = rt.temporal_ms()
        moved_g.append(round(g, 4))
        moved_a.append(round(acc, 4))
        rt.temporal()  # unchanged: the identity blend, nothing traced
        g2, acc2 = rt.temporal_ms()
        assert g2 == 0.0
        same.append(round(acc2, 4))
        rt.set_camera(*recs[(r + 8) % len(recs)])  # a pose neither the history nor the cache holds
        rt.geometry_guide()
        guide.append(round(rt.temporal_ms()[0], 4))
    out["guide_pass_ms"] = {"best": min(guide), "all": guide}
    out["accumulate_unchanged_ms"] = {"best": min(same), "all": same}
    out["accumulate_moved_ms"] = {"best_k_temporal": min(moved_a), "best_guide_pass": min(moved_g),
                                  "k_temporal_all": moved_a, "guide_pass_all": moved_g}

    # a queued 1-spp frame of the same process
    # (best of three rounds: the first allocates the pipeline's slots)
    rounds = []
    for _ in range(3):
        rt.clear()
        rt.render(1, first_sample=0)
        t0 = time.perf_counter()
        for i in range(a.frames):
            rt.render(1, first_sample=1 + i, sync=False)
        rt.synchronize()
        rounds.append(round((time.perf_counter() - t0) * 1e3 / a.frames, 4))
    out["queued_1spp_frame_ms"] = min(rounds)
    out["queued_1spp_frame_ms_all"] = rounds
    out["guide_pass_over_queued_frame"] = round(out["guide_pass_ms"]["best"] / out["queued_1spp_frame_ms"], 3)

    # host time of the setter beside destroy + create
    ts = []
    for r in range(a.reps):
        t0 = time.perf_counter()
        rt.set_camera(*recs[r % len(recs)])
        ts.append((time.perf_counter() - t0) * 1e3)
    out["set_camera_host_ms"] = {"best": round(min(ts), 4), "all": [round(t, 4) for t in ts]}
    tc = []
    for r in range(2):
        t0 = time.perf_counter()
        del rt
        rt = RayTracer(scene, seed=a.seed)
        tc.append((time.perf_counter() - t0) * 1e3)
    out["destroy_create_host_ms"] = {"best": round(min(tc), 3), "all": [round(t, 3) for t in tc]}

    # quality over the orbit
    out["quality"] = {"poses": a.poses, "degrees": a.degrees, "ref_spp": a.ref_spp}
    for label, kw in (("default", {}), ("plane_tolerance_0.001", {"plane_tolerance": 0.001})):
        rt.temporal_reset()
        shares = []
        for i, rec in enumerate(recs):
            rt.set_camera(*rec)
            rt.clear()
            rt.seed = a.seed + i
            rt.render(1, first_sample=0)
            raw = rt.film()[0].astype(np.float64)
            tmp = rt.temporal(**kw).astype(np.float64)
            shares.append(round(float((rt.temporal_history()[..., 3] > 1).mean()), 3))
        rt.seed = a.seed + 7919
        rt.clear()
        rt.render(a.ref_spp, first_sample=0)
        truth = (rt.film()[0].astype(np.float64) / a.ref_spp) @ LUM
        rt.seed = a.seed
        # the path tracer's film can hold a non-finite pixel (a 0 / 0 throughput, as the reference's), and
        # the accumulation is not a NaN filter: such pixels are left out of all three means and counted
        lr, lt = raw @ LUM, tmp @ LUM
        ok = np.isfinite(lr) & np.isfinite(lt) & np.isfinite(truth)
        mse_raw = float(((lr[ok] - truth[ok]) ** 2).mean())
        mse_tmp = float(((lt[ok] - truth[ok]) ** 2).mean())
        out["quality"][label] = {"mse_raw_last_frame": mse_raw, "mse_temporal": mse_tmp,
                                 "ratio": round(mse_tmp / mse_raw, 4), "history_share_per_pose": shares,
                                 "non_finite_pixels_left_out": int((~ok).sum()),
                                 "of_them_non_finite_in_the_reference": int((~np.isfinite(truth)).sum())}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "record_bytes": {"history": 16, "guide": 32}, "cases": []}
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a))
    with tempfile.TemporaryDirectory(prefix="rtg_temporal_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
