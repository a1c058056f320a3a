"""TEST INFRASTRUCTURE ONLY — scenes of the path-tracer MIS tests (tests/test_path_mis_gpu.py):
tests/material_scenes.py's floors with one more emitter that faces up, so a BSDF ray from the floor meets
its back.
"""
import json
import os

from conftest import SCENES
from material_scenes import write_material_floor_scene


def write_mis_floor_scene(out_dir, floor, width=64, height=48, **kw):
    """write_material_floor_scene(out_dir, floor, ...) plus a 0.6 x 0.5 emitter at y = 0.7 above the back
    left of the floor that faces up (two more light triangles): NEE from the floor finds its cosine zero,
    and a BSDF ray from the floor hits its back side. Returns out_dir."""
    out_dir = write_material_floor_scene(out_dir, floor, width, height, **kw)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    path = os.path.join(out_dir, "scene.json")
    scene = json.load(open(path))
    # Rectangle.gem turned about x so that its normal points to +y (light_pick_scenes._emitter's faces -y)
    scene["instances"].append({"filename": os.path.join(box, "Rectangle.gem"),
                               "world": [0.3, 0.0, 0.0, -0.45, 0.0, 0.0, 1.0, 0.7, 0.0, -0.25, 0.0, -0.4,
                                         0.0, 0.0, 0.0, 1.0],
                               "reflectance": os.path.join(box, "0_0_0_1.0.png"), "bsdf": "diffuse",
                               "emission": "4 3 2"})
    with open(path, "w") as f:
        json.dump(scene, f)
    return out_dir
