#!/usr/bin/env python3
"""What the Sobol sampler costs and buys (rtg_set_sampler): on one handle per case, in one session,
  frames    the device time (HIP events, rtg_stats.render_ms) of --spp frames at --size^2 with the samplers
            interleaved pcg, sobol, pcg, sobol, ... for --reps rounds after a warm-up of each; the medians,
            and the shading kernels' share of such a frame (rtg_stats.shade_ms under RTG_OPT_TIMING, one
            frame each): cornell-box under DIRECT and PATH, the synthetic scene of bench.py's C3, cornell-box
            with a tent filter and a lens, and the kernels with tables (the environment's luminance table on
            materialball-small, the power pick on cornell-box);
  mse       the mean squared error of the film's luminance at --mse-size^2 and 4, 16, 64 and 256 spp, the
            mean over --seeds seeds, against a --ref-spp PCG film of another seed (its own noise is inside
            both errors): sobol / pcg at equal samples, and at equal time with the frame times above
            (equal_time_gain = (mse_pcg * ms_pcg) / (mse_sobol * ms_sobol): above 1 the mode wins, below 1
            it loses);
  test      the ratio tests/test_sampler_gpu.py's noise test bounds itself by (cornell-box DIRECT 64 x 64,
            16 spp, 8 seeds, against 4096 spp of PCG), computed by that test's own function.
There is no pass mark. RTG_LIB selects an A/B build. Writes one JSON object (default
profiles/sampler_time.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "scenes")
LUM = np.array([0.2126, 0.7152, 0.0722])
SAMPLERS = ("pcg", "sobol")


def make(scene, integrator="path", camera=None, env_mode="uniform", power=False, seed=1234):
    from raytracingrenderer_amd import RayTracer
    rt = RayTracer(scene, seed=seed, integrator=integrator, max_depth=4)
    if camera:
        rt.set_camera_sampling(**camera)
    rt.set_env_sampling(env_mode)
    if power:
        rt.set_light_sampling("power")
    return rt


def frame_ms(rt, spp):
    rt.clear()
    rt.render(spp, first_sample=0)
    return rt.stats()["render_ms"]


def time_case(name, scene, spp, reps, **kw):
    from raytracingrenderer_amd import _native as N
    rt = make(scene, **kw)
    ms = {s: [] for s in SAMPLERS}
    active = {}
    for s in SAMPLERS:  # warm-up: allocates the chunk buffers
        rt.set_sampler(s)
        active[s] = rt.sampler_active
        frame_ms(rt, spp)
    for _ in range(reps):  # interleaved
        for s in SAMPLERS:
            rt.set_sampler(s)
            ms[s].append(frame_ms(rt, spp))
    shade = {}
    rt.set_options(flags=rt.flags | N.RTG_OPT_TIMING)
    for s in SAMPLERS:
        rt.set_sampler(s)
        frame_ms(rt, spp)
        shade[s] = rt.stats()["shade_ms"]
    med = {s: statistics.median(ms[s]) for s in SAMPLERS}
    out = {"case": name, "width": scene.width, "height": scene.height, "spp": spp, "reps": reps, "settings": kw and
           {k: v for k, v in kw.items()}, "sampler_active": active,
           "render_ms_device": {s: [round(m, 3) for m in ms[s]] for s in SAMPLERS},
           "median_ms": {s: round(med[s], 3) for s in SAMPLERS},
           "sobol_over_pcg_time": round(med["sobol"] / med["pcg"], 4),
           "shade_ms_timed_frame": {s: round(shade[s], 3) for s in SAMPLERS},
           "sobol_over_pcg_shade": round(shade["sobol"] / shade["pcg"], 4) if shade["pcg"] > 0 else None}
    print(json.dumps(out), flush=True)
    return out


def mean_film(rt, spp, seed):
    rt.seed = seed
    rt.clear()
    done = 0
    while done < spp:
        n = min(1024, spp - done)
        rt.render(n, first_sample=done)
        done += n
    return rt.film()[0].astype(np.float64) / spp


def mse_case(name, scene, ref_spp, seeds, time_ratio, **kw):
    rt = make(scene, **kw)
    rt.set_sampler("pcg")
    truth = mean_film(rt, ref_spp, 99991) @ LUM
    ok = np.isfinite(truth)
    out = {"case": name, "width": scene.width, "height": scene.height, "ref_spp": ref_spp, "seeds": seeds,
           "settings": {k: v for k, v in kw.items()}, "sobol_over_pcg_time": time_ratio, "spp": {}}
    for spp in (4, 16, 64, 256):
        mse = {}
        for s in SAMPLERS:
            rt.set_sampler(s)
            e = []
            for k in range(seeds):
                lum = mean_film(rt, spp, 4000 + k) @ LUM
                good = ok & np.isfinite(lum)
                e.append(float(np.mean((lum[good] - truth[good]) ** 2)))
            mse[s] = float(np.mean(e))
        ratio = mse["sobol"] / mse["pcg"]
        out["spp"][str(spp)] = {"mse_pcg": mse["pcg"], "mse_sobol": mse["sobol"], "sobol_over_pcg_mse": round(ratio, 4),
                                "equal_time_gain": round(1.0 / (ratio * time_ratio), 4) if time_ratio else None}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mse-size", type=int, default=256)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--synthetic-tris", type=int, default=1_000_000, help="0: skip the C3 scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    from raytracingrenderer_amd import _native as N
    from raytracingrenderer_amd.renderer import write_synthetic_scene
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    lens = dict(filter="tent", lens_radius=0.05, focal_distance=5.0)
    res = {"lib": os.environ.get("RTG_LIB", "product"), "build_id": N.rtg().rtg_build_id().decode(), "frames": [], "mse": []}
    box = os.path.join(GOLD, "cornell-box")
    ball = os.path.join(GOLD, "materialball-small")
    big = loadScene(box, width=a.size, height=a.size)
    t = {}
    t["direct"] = time_case("cornell-box DIRECT", big, a.spp, a.reps, integrator="direct")
    t["path"] = time_case("cornell-box PATH", big, a.spp, a.reps, integrator="path")
    t["lens"] = time_case("cornell-box PATH, tent filter and lens", big, a.spp, a.reps, integrator="path", camera=lens)
    t["pick"] = time_case("cornell-box PATH, power pick", big, a.spp, a.reps, integrator="path", power=True)
    t["ball"] = time_case("materialball-small PATH, luminance table", loadScene(ball, width=a.size, height=a.size),
                          a.spp, a.reps, integrator="path", env_mode="luminance")
    if a.synthetic_tris:
        with tempfile.TemporaryDirectory() as tmp:
            write_synthetic_scene(tmp, a.synthetic_tris, width=a.size, height=a.size)
            t["c3"] = time_case("synthetic %d triangles (C3's scene) PATH" % a.synthetic_tris, loadScene(tmp), a.spp,
                                a.reps, integrator="path")
    res["frames"] = list(t.values())
    small = loadScene(box, width=a.mse_size, height=a.mse_size)
    res["mse"].append(mse_case("cornell-box DIRECT", small, a.ref_spp, a.seeds, t["direct"]["sobol_over_pcg_time"],
                               integrator="direct"))
    res["mse"].append(mse_case("cornell-box PATH", small, a.ref_spp, a.seeds, t["path"]["sobol_over_pcg_time"],
                               integrator="path"))
    res["mse"].append(mse_case("cornell-box PATH, tent filter and lens", small, a.ref_spp, a.seeds,
                               t["lens"]["sobol_over_pcg_time"], integrator="path", camera=lens))
    res["mse"].append(mse_case("materialball-small PATH, luminance table",
                               loadScene(ball, width=a.mse_size, height=a.mse_size), a.ref_spp, a.seeds,
                               t["ball"]["sobol_over_pcg_time"], integrator="path", env_mode="luminance"))
    import test_sampler_gpu as tg
    sob, pcg = tg.mse_ratio_cornell_direct()
    res["test_mse_ratio"] = {"case": "cornell-box DIRECT 64 x 64, 16 spp, 8 seeds, against 4096 spp of PCG",
                             "mse_sobol": sob, "mse_pcg": pcg, "ratio": sob / pcg,
                             "test_bound": float(np.sqrt(sob / pcg))}
    print(json.dumps(res["test_mse_ratio"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
