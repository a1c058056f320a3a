"""TEST INFRASTRUCTURE ONLY — scenes of the material-model tests (tests/test_materials_gpu.py): the floor
of tests/light_pick_scenes.py's "unequal" scene with a conductor, plastic or Oren-Nayar bsdf, under its
emitters and black cube, or under an environment map alone.
"""
import os

from conftest import SCENES
from light_pick_scenes import _emitter, _floor, _write, unequal_emitters

# scene.json material entries of the floors (the gold-like conductor is cornell-mat's)
FLOORS = {
    "conductor": {"bsdf": "conductor", "roughness": "0.2", "eta": "1.65 0.88 0.52", "k": "9.2 6.3 4.8"},
    "plastic": {"bsdf": "plastic", "roughness": "0.1", "intIOR": "1.5", "extIOR": "1.0"},
    "plastic-delta": {"bsdf": "plastic", "roughness": "0", "intIOR": "1.5", "extIOR": "1.0"},
    "orennayar": {"bsdf": "orennayar", "alpha": "0.3"},
}


def write_material_floor_scene(out_dir, floor, width=64, height=48, env=None, emitters=True, cube=True, extra=0, back=False):
    """The "unequal" scene (22 light triangles facing down from y = 1.98, a black cube) with the floor
    FLOORS[floor] (cornell-box's floor albedo), optionally under the environment map `env` ((H, W, 3)
    float32, in the light list when it has power). emitters=False, cube=False: the floor under the
    environment alone. extra: that many more small dim emitter rectangles in a row at the back (two
    light triangles each), to take the light list past the shading kernels' LDS table. back: a 2 x 1.6 emitter behind the floor at z = -2.2,
    where the camera rays' mirror reflections off the front half of the floor arrive. Returns out_dir."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    base, fl = _floor(box, white=False)
    fl = {k: v for k, v in fl.items() if k in ("filename", "world", "reflectance")}
    fl.update(FLOORS[floor])
    inst = [fl]
    if emitters:
        inst += [_emitter(box, *e) for e in unequal_emitters()]
    for k in range(extra):
        inst.append(_emitter(box, -0.95 + 1.9 * (k + 0.5) / extra, -0.95, 0.02, 0.02,
                             (0.4 + 0.03 * k, 0.3 + 0.02 * k, 0.2 + 0.01 * k)))
    if back:
        inst.append(_emitter(box, 0.0, -2.2, 1.0, 0.8, (3.0, 2.5, 2.0)))
    if cube:
        inst.append({"filename": os.path.join(box, "Cube.gem"),
                     "world": [0.25, 0.0, 0.0, 0.3, 0.0, 0.25, 0.0, 0.25, 0.0, 0.0, 0.25, 0.1, 0.0, 0.0, 0.0, 1.0],
                     "reflectance": os.path.join(box, "0_0_0.png"), "bsdf": "diffuse"})
    return _write(out_dir, base, inst, width, height, env)
