"""TEST INFRASTRUCTURE ONLY — the "pane" scene of the rough dielectric's tests
(tests/test_transmission_gpu.py): the floor of tests/light_pick_scenes.py's "unequal" scene as a pane of
frosted glass, lit from above and from below.
"""
import os

from conftest import SCENES
from light_pick_scenes import _emitter, _floor, _write, unequal_emitters

PANE = {"bsdf": "dielectric", "roughness": "0.5", "intIOR": "1.5", "extIOR": "1.0"}
LOWER = (0.1, -0.1, 0.45, 0.35, (12.0, 10.0, 8.0))  # cx, cz, sx, sz, emission of the emitter below the pane


def write_pane_scene(out_dir, width=64, height=48, flipped=False, env=None, emitters=True, cube=True, extra=0,
                     pane=None):
    """The "unequal" scene (22 light triangles facing down from y = 1.98, a black cube) over a floor that is
    a rough dielectric (PANE, cornell-box's floor albedo; `pane` overrides entries), plus one emitter
    rectangle at y = -1 that faces up: 24 light triangles. The floor is a single quad, so a shadow ray to the
    lower emitter, which starts just below it, meets nothing. flipped: the floor's world matrix turned over
    about the x axis (rows y and z negated), so its normal points down, the camera sees its back and wo.z <
    0 at every first hit. env, emitters, cube, extra: as material_scenes.write_material_floor_scene (without
    emitters the lower one is left out too). Returns out_dir."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    base, fl = _floor(box, white=False)
    fl = {k: v for k, v in fl.items() if k in ("filename", "world", "reflectance")}
    fl.update(PANE)
    fl.update(pane or {})
    if flipped:
        w = list(fl["world"])
        fl["world"] = w[0:4] + [-v for v in w[4:12]] + w[12:16]
    inst = [fl]
    if emitters:
        inst += [_emitter(box, *e) for e in unequal_emitters()]
        cx, cz, sx, sz, em = LOWER
        up = _emitter(box, cx, cz, sx, sz, em, y=-1.0)
        up["world"] = [sx, 0.0, 0.0, cx, 0.0, 0.0, 1.0, -1.0, 0.0, -sz, 0.0, cz, 0.0, 0.0, 0.0, 1.0]  # facing up
        inst.append(up)
    for k in range(extra):
        inst.append(_emitter(box, -0.95 + 1.9 * (k + 0.5) / extra, -0.95, 0.02, 0.02,
                             (0.4 + 0.03 * k, 0.3 + 0.02 * k, 0.2 + 0.01 * k)))
    if cube:
        inst.append({"filename": os.path.join(box, "Cube.gem"),
                     "world": [0.25, 0.0, 0.0, 0.3, 0.0, 0.25, 0.0, 0.25, 0.0, 0.0, 0.25, 0.1, 0.0, 0.0, 0.0, 1.0],
                     "reflectance": os.path.join(box, "0_0_0.png"), "bsdf": "diffuse"})
    return _write(out_dir, base, inst, width, height, env)
