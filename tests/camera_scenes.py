"""TEST INFRASTRUCTURE ONLY — scenes of overlapping emitters for the end-to-end camera-sampling
tests: every instance is an emitter with a small-integer emission of its own, over a black background,
so a first-hit film is an exact, order-free sum of per-triangle integers.

write_emitter_scene() writes a scene.json that references the committed cornell-box meshes by relative
path (as tests/shade_scenes.py does). Layout "few": 20 camera-facing quads in two overlapping layers (20
materials, 40 light triangles: k_shade's tables fit in LDS). Layout "many": a denser grid of quads plus
tilted cubes in front of it (more lights than the LDS table holds: the global-table kernels run).
"""
import json
import os

from conftest import SCENES


def _quad(cx, cy, cz, hx, hy):
    # Rectangle.gem spans [-1, 1]^2 of its local xy plane: scaled, facing the camera, at depth cz
    return ("Rectangle.gem", [hx, 0.0, 0.0, cx, 0.0, hy, 0.0, cy, 0.0, 0.0, 1.0, cz, 0.0, 0.0, 0.0, 1.0])


def _cube(cx, cy, cz, h):
    # Cube.gem, turned about y and x so that three faces show
    a, b = 0.8660254 * h, 0.5 * h
    return ("Cube.gem", [a, 0.0, b, cx, 0.25 * h, a, -0.4330127 * h, cy, -0.4330127 * h, b, 0.75 * h, cz, 0.0, 0.0, 0.0, 1.0])


def emitter_layout(layout):
    """[(mesh, world)] of the layout; the camera (cornell-box's) sees about x in [-1.33, 1.33], y in
    [0, 2] at these depths."""
    inst = []
    if layout == "few":
        for j in range(3):
            for i in range(4):
                inst.append(_quad(-0.9 + 0.6 * i, 0.4 + 0.6 * j, 0.0, 0.22, 0.2))
        for j in range(2):
            for i in range(4):
                inst.append(_quad(-0.75 + 0.5 * i + 0.07 * j, 0.72 + 0.58 * j, 1.0, 0.16, 0.17))
    elif layout == "many":
        for j in range(7):
            for i in range(9):
                inst.append(_quad(-1.2 + 0.3 * i, 0.1 + 0.3 * j, -0.5 + 0.1 * ((i + 2 * j) % 5), 0.11, 0.12))
        for k in range(6):
            inst.append(_cube(-1.0 + 0.4 * k, 0.55 + 0.45 * (k % 3), 1.5, 0.13))
    else:
        raise ValueError(layout)
    return inst


def emission_of(i):
    """Instance i's emission: three small integers, a different triple for every instance."""
    return (1 + i % 16, 1 + (i // 16) + 2 * (i % 3), 1 + (7 * i) % 23)


def write_emitter_scene(out_dir, layout, width, height):
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    base = json.load(open(os.path.join(SCENES, "cornell-box", "scene.json")))
    scene = {k: base[k] for k in ("fov", "from", "to", "up")}
    scene["width"], scene["height"] = str(width), str(height)
    scene["instances"] = [{"filename": os.path.join(box, mesh), "world": world,
                           "reflectance": os.path.join(box, "0_0_0_1.0.png"), "bsdf": "diffuse",
                           "emission": "%d %d %d" % emission_of(i)}
                          for i, (mesh, world) in enumerate(emitter_layout(layout))]
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(scene, f)
    return out_dir
