"""The device records of a scene (rtg_scene.hip prepare_scene: BVH2 and wide nodes, leaf boxes, the
small-scene image, triangle / shading / material / light / texture records and the scalars beside
them), pinned on the CPU: tests/native/scene_digest prints one digest per HostScene array, and
tests/golden/device_scene_digests.json holds the values (tests/golden/make_golden.py
--device-digests). The scenes stay below the 50,000 triangles from which build_sbvh builds subtrees
on several threads, so the records do not depend on the host's core count."""
import json
import os
import subprocess

import pytest

from conftest import SCENES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_scene_digests.json")
INPUTS = {"cornell-box": ["cornell-box"], "cornell-mat": ["cornell-mat"], "synth20k": ["synth", "20000", "20251015"]}


def run_digest(exe, name, tmp):
    """scene_digest's "name value" lines for INPUTS[name] as a dict (tmp: a folder for the synthetic scene)."""
    a = INPUTS[name]
    args = a + [os.path.join(str(tmp), "synth")] if a[0] == "synth" else [os.path.join(SCENES, a[0])]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(line.split(" ", 1) for line in r.stdout.splitlines())


@pytest.fixture(scope="module")
def digest_exe():
    from raytracingrenderer_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    build.build_host()
    build.build_device()
    return build.build_scene_digest()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_device_records_match_the_golden_digests(digest_exe, name, tmp_path):
    got = run_digest(digest_exe, name, tmp_path)
    want = json.load(open(GOLDEN))[name]
    assert {k: got.get(k) for k in want} == want
    assert set(got) == set(want)
