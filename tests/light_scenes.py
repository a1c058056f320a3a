"""TEST INFRASTRUCTURE ONLY — scenes and point sets for the light tracer's and instant radiosity's tests
(tests/test_light_paths_gpu.py on the GPU against the C oracle, tests/test_oracle_light.py the oracle
against the reference's classes on the CPU).

write_closed_white_box() writes a scene.json that references the committed cornell-box mesh and 1x1
textures by relative path, as shade_scenes.py does. connection_points() is the point set of the
camera-connection probe.
"""
import json
import os

import numpy as np

from conftest import GOLD, SCENES

BACK_WALL, EMITTER = 2, 7  # cornell-box's instances: floor, ceiling, back, right, left, two cubes, emitter


def write_closed_white_box(out_dir):
    """cornell-box's five walls and its emitter, every wall white (1_1_1.png), the two cubes dropped and
    the open side closed by a copy of the back wall at z = +1; the camera stands inside, just in front of
    that sixth wall, with a 100 degree field of view. A light path in it can leave only by Russian
    roulette (albedo 1: continuation probability 0.9), and most of its vertices see the camera: several
    camera connections per path, where cornell-box has 2.5 and the other fixture scenes about one.
    Returns out_dir."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    base = json.load(open(os.path.join(SCENES, "cornell-box", "scene.json")))
    inst = []
    for n, i in enumerate(base["instances"]):
        if i["filename"] != "Rectangle.gem":
            continue
        i = dict(i)
        i["filename"] = os.path.join(box, i["filename"])
        i["reflectance"] = os.path.join(box, i["reflectance"] if "emission" in i else "1_1_1.png")
        inst.append(i)
        if n == BACK_WALL:
            assert i["world"][11] == -1.0 and "emission" not in i
            front = dict(i)
            front["world"] = list(i["world"])
            front["world"][11] = 1.0
            inst.append(front)
    assert len(inst) == 7 and "emission" in inst[-1] and base["instances"][EMITTER] is not None
    scene = {"width": "64", "height": "48", "fov": "100", "from": "0 1 0.9", "to": "0 1 -1", "up": base["up"],
             "instances": inst}
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(scene, f)
    return out_dir


def far_points():
    """The 64 far points of light_kat.npz's cornell point set (golden/make_golden.py light_fixtures:
    uniform in [-50, 50]^3, most of them outside the frustum)."""
    return np.load(os.path.join(GOLD, "light_kat.npz"))["cornell_pts"][:64].astype(np.float32)


def _frustum_walks(oracle, origin, steps=6):
    """Points walked with np.nextafter across each of the four frustum planes. Starting points: on a
    coarse grid of view rays, bisect one world coordinate between a point the oracle's projection accepts
    and one it refuses until the two are neighbouring floats; then step `steps` floats to either side of
    the boundary. The oracle's film x or y is 0 or 1 (before scaling: W, H or 0 after) at or next to such
    points, so accepted, rejected and px == W / py == H cases all occur."""
    out = []
    # a box around the camera's view: points at depth 1 and 2.5 in front of it, swept left/right and up/down
    for depth in (1.0, 2.5):
        for fixed in np.linspace(-0.12, 0.12, 4, dtype=np.float32):
            for axis in (0, 1):  # the coordinate that crosses the plane: world x (left/right), y (bottom/top)
                for sign in (-1.0, 1.0):
                    inside = np.array(origin, np.float32) + np.float32([0, 0, -depth])
                    inside[1 - axis] += fixed * np.float32(depth)
                    outside = inside.copy()
                    outside[axis] += np.float32(sign * 50.0)
                    ok = lambda p: oracle.camera_project(p[None])[0, 0] == 1.0
                    if not ok(inside) or ok(outside):
                        continue
                    lo, hi = inside[axis], outside[axis]  # lo accepted, hi refused
                    for _ in range(200):
                        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
                        if mid == lo or mid == hi:
                            break
                        p = inside.copy()
                        p[axis] = mid
                        if ok(p):
                            lo = mid
                        else:
                            hi = mid
                    v = lo
                    for _ in range(steps):
                        v = np.nextafter(v, np.float32(-sign * np.inf), dtype=np.float32)
                    for _ in range(2 * steps + 1):
                        p = inside.copy()
                        p[axis] = v
                        out.append(p)
                        v = np.nextafter(v, np.float32(sign * np.inf), dtype=np.float32)
    return np.array(out, np.float32)


def connection_points(oracle, scene, seed=7):
    """(points, normals, colours), (n, 3) float32 each, for the camera-connection probe on `scene`'s
    camera (looking down -z, as the Cornell scenes' do): 2048 random points in and around the box with
    normals towards and away from the camera, 64 far points, the camera origin, points behind the camera,
    coordinates of +-1e30 and +-inf, a NaN in each input component, and walks across the four frustum
    planes."""
    rng = np.random.default_rng(seed)
    origin = np.array(scene.desc.camera.origin[:], np.float32)
    pts = rng.uniform(-1.2, 1.2, (2048, 3)).astype(np.float32) + np.float32([0, 1, 0])
    towards = origin[None] - pts
    towards /= np.maximum(np.linalg.norm(towards, axis=1, keepdims=True), 1e-20).astype(np.float32)
    nrm = rng.normal(size=pts.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    nrm[::3] = towards[::3]
    nrm[1::3] = -towards[1::3]
    blocks = [(pts, nrm)]

    def add(p, n=None):
        p = np.array(p, np.float32).reshape(-1, 3)
        if n is None:
            n = np.tile(np.float32([0, 0, 1]), (len(p), 1))  # faces a camera that looks down -z
        blocks.append((p, np.array(n, np.float32).reshape(-1, 3)))

    add(far_points())
    add([origin, origin, origin], [[0, 0, 1], [0, 0, -1], [0, 0, 0]])
    add(origin[None] + np.float32([[0, 0, 1], [0.3, -0.2, 5], [0, 0, 1e-3], [-2, 1, 0.5]]))  # behind the camera
    p = np.tile(np.float32([0.1, 1.1, 0.2]), (12, 1))
    for k in range(12):  # one coordinate of each point replaced
        p[k, k // 4] = (1e30, -1e30, np.inf, -np.inf)[k % 4]
    add(p)
    add([[np.inf, np.inf, -np.inf], [-np.inf, np.inf, np.inf], [1e30, -1e30, -1e30], [3e38, 3e38, -3e38]])
    base = np.float32([0.2, 0.9, -0.3, 0, 0, 1, 0.5, 0.25, 0.125])  # point, normal, colour
    nan_rows = np.tile(base, (9, 1))
    for k in range(9):
        nan_rows[k, k] = np.nan
    add(_frustum_walks(oracle, origin))
    p = np.concatenate([b[0] for b in blocks])
    n = np.concatenate([b[1] for b in blocks])
    c = rng.uniform(0.05, 4.0, p.shape).astype(np.float32)
    p = np.concatenate([p, nan_rows[:, 0:3]])
    n = np.concatenate([n, nan_rows[:, 3:6]])
    c = np.concatenate([c, nan_rows[:, 6:9]])
    return np.ascontiguousarray(p), np.ascontiguousarray(n), np.ascontiguousarray(c)
