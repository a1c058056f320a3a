#!/usr/bin/env python3
"""What the fused first-hit pass costs and saves (rtg_gbuffer, rtg_gbuffer.hip), on one GPU at --size x --size
for cornell-box and the C3 scene (synthetic 1M triangles), by tools/svgf_time.py's method: best of --reps with
all kept. Per scene:
  device ms of the fused pass (generate, traversal, k_gbuffer: rtg_gbuffer_ms after a moved svgf()) next to the
  geometry guide pass (generate, traversal, k_geometry_guide: rtg_temporal_ms after a moved temporal());
  wall time of one moved frame through svgf(), measured as svgf_time.py measures "moved_frame_wall_ms";
  wall time of gbuffer() against geometry_guide() + guides() on a fresh camera, with the copies to the host and,
  through the C entry points with null outputs, without them.
Measure mode (the default) writes one JSON object to --out. Combine mode, --combine P1 T1 P2 T2 ..., takes the
interleaved runs of one session (P: tools/svgf_time.py's output on the parent tree, T: this tool's on this
tree, in the order they ran), writes all of them to --out (default profiles/gbuffer_time.json) and states the
pass mark per scene: the best moved-frame wall time here is at most the parent's best moved-frame wall time
minus half of the parent's best "albedo + normal guides" wall time. RTG_LIB selects an A/B build."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from temporal_time import orbit, records  # noqa: E402


def best(v):
    return {"best": round(min(v), 4), "all": [round(x, 4) for x in v]}


def measure(name, scene, a):
    from raytracingrenderer_amd import RayTracer
    out = {"scene": name, "width": scene.width, "height": scene.height, "triangles": int(scene.desc.n_tris)}
    rt = RayTracer(scene, seed=a.seed)
    recs = [records(scene, f, t) for f, t in orbit(scene, a.poses, a.degrees)]
    nxt = [0]

    def pose():
        nxt[0] += 1
        rt.set_camera(*recs[nxt[0] % len(recs)])

    def move():
        pose()
        rt.clear()
        rt.render(1, first_sample=0)

    rt.render(1)
    rt.svgf()  # warm-up: allocates the states
    rt.temporal()
    rt.gbuffer()

    fused, geo, w_svgf = [], [], []
    for r in range(a.reps):
        move()
        rt.temporal()  # moved: the geometry guide pass alone
        geo.append(rt.temporal_ms()[0])
        move()
        t0 = time.perf_counter()
        rt.svgf()  # moved: the fused pass, reprojection, variance, the levels
        w_svgf.append((time.perf_counter() - t0) * 1e3)
        fused.append(rt.gbuffer_ms())
        assert rt.svgf_ms()[0] == fused[-1] > 0.0
    out["fused_pass_ms"] = best(fused)
    out["geometry_guide_pass_ms"] = best(geo)
    out["fused_minus_geometry_ms"] = round(min(fused) - min(geo), 4)
    out["moved_frame_wall_ms"] = {"svgf": best(w_svgf)}

    w_gb, w_sep, w_gb_nc, w_sep_nc = [], [], [], []
    lib, h = rt._lib, rt.handle
    for r in range(a.reps):
        pose()
        t0 = time.perf_counter()
        rt.gbuffer()
        w_gb.append((time.perf_counter() - t0) * 1e3)
        pose()
        t0 = time.perf_counter()
        rt.geometry_guide()
        rt.guides()
        w_sep.append((time.perf_counter() - t0) * 1e3)
        pose()
        t0 = time.perf_counter()
        assert lib.rtg_gbuffer(h, None, None, None, None) == 0
        w_gb_nc.append((time.perf_counter() - t0) * 1e3)
        pose()
        t0 = time.perf_counter()
        assert lib.rtg_geometry_guide(h, None, None) == 0 and lib.rtg_denoise_guides(h, None, None) == 0
        w_sep_nc.append((time.perf_counter() - t0) * 1e3)
    out["fresh_camera_wall_ms"] = {"gbuffer": best(w_gb), "geometry_guide_plus_guides": best(w_sep),
                                   "gbuffer_no_copy": best(w_gb_nc), "geometry_guide_plus_guides_no_copy": best(w_sep_nc)}
    return out


def combine(paths, out_path):
    runs = []
    for i, p in enumerate(paths):
        with open(p) as f:
            d = json.load(f)
        runs.append({"order": i, "tree": "parent" if i % 2 == 0 else "this", "tool": d.get("tool", "tools/svgf_time.py"),
                     "file": os.path.basename(p), "cases": d["cases"]})
    res = {"method": "interleaved runs of one session on one GPU (parent, this, parent, this): tools/svgf_time.py on "
                     "the parent tree, tools/gbuffer_time.py on this one; best of each tree's runs",
           "pass_mark": "moved-frame wall here <= parent's moved-frame wall - 0.5 * parent's albedo + normal guides wall",
           "scenes": [], "runs": runs}
    names = [c["scene"] for c in runs[0]["cases"]]
    for k, name in enumerate(names):
        par = [r["cases"][k] for r in runs if r["tree"] == "parent"]
        new = [r["cases"][k] for r in runs if r["tree"] == "this"]
        p_wall = min(c["moved_frame_wall_ms"]["svgf"]["best"] for c in par)
        p_guides = min(c["albedo_normal_guides_wall_ms"]["best"] for c in par)
        n_wall = min(c["moved_frame_wall_ms"]["svgf"]["best"] for c in new)
        bound = p_wall - 0.5 * p_guides
        res["scenes"].append({
            "scene": name,
            "parent_moved_frame_wall_ms": {"best": p_wall, "per_run": [c["moved_frame_wall_ms"]["svgf"]["best"] for c in par]},
            "parent_albedo_normal_guides_wall_ms": {"best": p_guides,
                                                    "per_run": [c["albedo_normal_guides_wall_ms"]["best"] for c in par]},
            "parent_guide_pass_ms": {"per_run": [c["guide_pass_ms"]["best"] for c in par]},
            "this_moved_frame_wall_ms": {"best": n_wall, "per_run": [c["moved_frame_wall_ms"]["svgf"]["best"] for c in new]},
            "this_fused_pass_ms": {"per_run": [c["fused_pass_ms"]["best"] for c in new]},
            "this_geometry_guide_pass_ms": {"per_run": [c["geometry_guide_pass_ms"]["best"] for c in new]},
            "bound_ms": round(bound, 4), "pass_mark_met": bool(n_wall <= bound)})
    res["pass_mark_met"] = all(s["pass_mark_met"] for s in res["scenes"])
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"pass_mark_met": res["pass_mark_met"], "scenes": res["scenes"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--degrees", type=float, default=15.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--combine", nargs="+", metavar="JSON", help="parent, this, parent, this, ... runs to put together")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer_time.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.combine:
        return combine(a.combine, a.out)
    from raytracingrenderer_amd import loadScene, write_synthetic_scene
    res = {"tool": "tools/gbuffer_time.py", "lib": os.environ.get("RTG_LIB", "product"),
           "bytes_per_pixel": {"read_hits_ray": 32, "read_triangle": 48, "read_shading": 64, "read_material": 64,
                               "written": 88, "written_by_k_geometry_guide": 32},
           "cases": []}
    cornell = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box")
    res["cases"].append(measure("cornell-box", loadScene(cornell, width=a.size, height=a.size), a))
    with tempfile.TemporaryDirectory(prefix="rtg_gbuffer_time_") as work:
        write_synthetic_scene(work, n_tris=a.tris, seed=20251015, width=a.size, height=a.size)
        res["cases"].append(measure("C3 synthetic %d triangles" % a.tris, loadScene(work), a))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
