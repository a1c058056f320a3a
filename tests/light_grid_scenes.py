"""TEST INFRASTRUCTURE ONLY — scenes of the light-grid tests (tests/test_light_grid.py,
tests/test_light_grid_gpu.py): a long hall and a square room lit by many small emitters under the ceiling,
the case in which a position-independent pick wastes most NEE samples. The scene.json files reference the
committed cornell-box meshes and 1x1 textures by relative path, as tests/light_pick_scenes.py's do.
"""
import json
import os

from conftest import SCENES
from light_pick_scenes import _emitter


def _floor(box, hx, hz):
    """Rectangle.gem as a white floor of 2 hx by 2 hz at y = 0, facing up (cornell-box's floor matrix with
    the two in-plane axes scaled)."""
    return {"filename": os.path.join(box, "Rectangle.gem"),
            "world": [0.0, hx, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, hz, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
            "reflectance": os.path.join(box, "1_1_1.png"), "bsdf": "diffuse"}


def _cube(box, cx, cz, h=0.25):
    return {"filename": os.path.join(box, "Cube.gem"),
            "world": [h, 0.0, 0.0, cx, 0.0, h, 0.0, h, 0.0, 0.0, h, cz, 0.0, 0.0, 0.0, 1.0],
            "reflectance": os.path.join(box, "0_0_0.png"), "bsdf": "diffuse"}


def _write(out_dir, inst, width, height, frm, to, fov):
    scene = {"fov": fov, "from": frm, "to": to, "up": "0.0 1.0 0.0", "width": str(width), "height": str(height),
             "instances": inst}
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(scene, f)
    return out_dir


def hall_emitters(n_emitters, hx=8.0):
    """[(cx, cz, sx, sz, emission)]: n_emitters equal 0.1 x 0.1 emitters in two rows (z = -0.5 and 0.5),
    evenly spaced along the hall."""
    per_row = n_emitters // 2
    assert per_row * 2 == n_emitters
    out = []
    for k in range(n_emitters):
        cx = -hx + 2.0 * hx * ((k % per_row) + 0.5) / per_row
        out.append((cx, -0.5 if k < per_row else 0.5, 0.05, 0.05, (40.0, 36.0, 30.0)))
    return out


def write_hall_scene(out_dir, n_emitters=32, width=64, height=48):
    """A white 16 x 2 floor, n_emitters equal 0.1 x 0.1 emitters facing down from y = 1.98 in two rows
    (2 n_emitters light triangles: 32 emitters make 64 lights, past RTG_LDS_LIGHTS; 12 make 24, in LDS) and
    two black cubes standing on the floor; no walls, no environment. The camera stands at one end and looks
    along the hall. Returns out_dir."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    inst = [_floor(box, 8.0, 1.0)]
    inst += [_emitter(box, *e) for e in hall_emitters(n_emitters)]
    inst += [_cube(box, -4.0, 0.3), _cube(box, 1.0, -0.4)]
    return _write(out_dir, inst, width, height, "-7.9 1.2 0.0", "-2.0 0.0 0.0", "30")


def room_emitters(n_emitters=32):
    """[(cx, cz, sx, sz, emission)]: a grid of 0.1 x 0.1 emitters over the 2 x 2 room, their emission
    varying between 0.2 and 5 times (4, 3.6, 3)."""
    nx = 8
    nz = (n_emitters + nx - 1) // nx
    out = []
    for k in range(n_emitters):
        cx = -1.0 + 2.0 * ((k % nx) + 0.5) / nx
        cz = -1.0 + 2.0 * ((k // nx) + 0.5) / nz
        m = 0.2 + 4.8 * ((k * 7) % n_emitters) / float(n_emitters - 1)
        out.append((cx, cz, 0.05, 0.05, (4.0 * m, 3.6 * m, 3.0 * m)))
    return out


def write_room_scene(out_dir, n_emitters=32, width=64, height=48):
    """The same over a 2 x 2 floor: n_emitters emitters of unequal emission in a grid, two black cubes, the
    raised cornell-box camera of tests/light_pick_scenes.py. Returns out_dir."""
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), out_dir)
    inst = [_floor(box, 1.0, 1.0)]
    inst += [_emitter(box, *e) for e in room_emitters(n_emitters)]
    inst += [_cube(box, -0.4, 0.3, 0.15), _cube(box, 0.5, -0.4, 0.15)]
    return _write(out_dir, inst, width, height, "0.0 2.5 4.0", "0.0 0.0 0.0", "19.5")
