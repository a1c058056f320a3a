#!/usr/bin/env python3
"""What luminance sampling of the environment light costs and gains (rtg_set_env_sampling): per scene
and mode (uniform, luminance), the device time of an --spp frame (best of --reps waited-for renders
after a warm-up), the alias table's build time, and the mean squared error of the frame's luminance
against the same handle's own --ref-spp film (rendered under another seed), at equal samples and, for
the luminance mode, at the sample count that takes the uniform frame's time. Scenes: the committed
coffee-small and materialball-small, and, when the full assets are staged (assets/), materialball and
the coffee scene under GI.hdr (config C5's). A scene whose environment is no light (coffee-small has
none; a black map is left out of the light list) renders the same film in both modes. RTG_LIB selects an A/B build. Writes one JSON object (default
profiles/env_sampling_time.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lum(film, spp):
    f = film.astype(np.float64) / spp
    return 0.2126 * f[..., 0] + 0.7152 * f[..., 1] + 0.0722 * f[..., 2]


def mse(img, ref):
    """(mean squared error over the pixels finite in both images, the number of the others): a path
    with a non-finite throughput leaves a non-finite pixel in either mode, as in the reference."""
    ok = np.isfinite(img) & np.isfinite(ref)
    return float(np.mean((img[ok] - ref[ok]) ** 2)), int((~ok).sum())


def frame(rt, spp, seed, reps=1):
    """(luminance image, best device ms) of an spp-sample frame under `seed`."""
    rt.seed = seed
    ms = []
    for _ in range(reps):
        rt.clear()
        rt.render(spp, first_sample=0)
        ms.append(rt.stats()["render_ms"])
    f, n = rt.film()
    return lum(f, n), min(ms)


def measure(name, scene, spp, ref_spp, reps):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "spp": spp, "ref_spp": ref_spp, "modes": {}}
    rts = {}
    for mode in ("uniform", "luminance"):
        rt = RayTracer(scene, seed=1234)
        rt.set_env_sampling(mode)
        t = rt.env_table()
        frame(rt, spp, 1234)  # warm-up: allocates the chunk buffers
        img, ms = frame(rt, spp, 1234, reps)
        chunk = 4096  # the reference in chunks of sample indices below RTG_MAX_SAMPLES_PER_KEY
        rt.seed = 99991
        rt.clear()
        for s0 in range(0, ref_spp, chunk):
            rt.render(min(chunk, ref_spp - s0), first_sample=s0)
        f, n = rt.film()
        ref = lum(f, n)
        rts[mode] = (rt, ref)
        out["modes"][mode] = {"render_ms_device": round(ms, 3), "table": None if t is None else list(t["prob"].shape[::-1]),
                              "table_build_ms": None if t is None else round(t["build_ms"], 3),
                              "mse_equal_spp": mse(img, ref)[0], "non_finite_pixels": mse(img, ref)[1],
                              "ref_mean": float(ref[np.isfinite(ref)].mean())}
    u, l = out["modes"]["uniform"], out["modes"]["luminance"]
    spp_t = max(1, int(round(spp * u["render_ms_device"] / l["render_ms_device"])))
    rt, ref = rts["luminance"]
    img, ms = frame(rt, spp_t, 1234, reps)
    l["equal_time_spp"] = spp_t
    l["equal_time_render_ms_device"] = round(ms, 3)
    l["mse_equal_time"] = mse(img, ref)[0]
    out["time_luminance_vs_uniform"] = round(l["render_ms_device"] / u["render_ms_device"], 4)
    out["mse_uniform_vs_luminance_equal_spp"] = round(u["mse_equal_spp"] / l["mse_equal_spp"], 3)
    out["mse_uniform_vs_luminance_equal_time"] = round(u["mse_equal_spp"] / l["mse_equal_time"], 3)
    out["ref_mean_luminance_vs_uniform"] = round(l["ref_mean"] / u["ref_mean"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_sampling_time.json"))
    a = ap.parse_args()
    from raytracingrenderer_amd import loadScene
    res = {"lib": os.environ.get("RTG_LIB", "product"), "cases": []}
    gold = os.path.join(ROOT, "tests", "golden", "scenes")
    scenes = [(n, loadScene(os.path.join(gold, n), width=a.size, height=a.size))
              for n in ("coffee-small", "materialball-small")]
    ball = os.path.join(ROOT, "assets", "materialball")
    if os.path.isdir(ball):
        scenes.insert(0, ("materialball", loadScene(ball, width=a.size, height=a.size, skip_missing=True)))
    coffee = os.path.join(ROOT, "assets", "coffee")
    if os.path.exists(os.path.join(coffee, "GI.hdr")):  # (the map's name is relative to the scene directory)
        scenes.insert(0, ("coffee + GI.hdr", loadScene(coffee, width=a.size, height=a.size, skip_missing=True,
                                                       envmap="GI.hdr")))
    for name, s in scenes:
        res["cases"].append(measure(name, s, a.spp, a.ref_spp, a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
