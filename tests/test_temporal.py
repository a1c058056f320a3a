"""The numpy restatement of temporal accumulation (tests/temporal_ref.py) on guides and films taken from
the C oracle, no GPU: what the definition of include/rtg.h gives on its own, before the kernels are
compared with it bit for bit (tests/test_temporal_gpu.py)."""
import os

import numpy as np
import pytest

import temporal_ref as tr
from conftest import SCENES
from oracle.pyoracle import Oracle
from raytracingrenderer_amd import loadScene

W, H = 64, 48


@pytest.fixture(scope="module")
def box():
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=W, height=H)
    orc = Oracle(s, 4, "rtm")
    frames = [orc.render(1, first=i, seed=1234, threads=8)[0] for i in range(8)]
    return s, orc, frames


def run(s, orc, frames, **kw):
    ref = tr.TemporalRef()
    out = None
    for f in frames:
        out = ref.accumulate(f, 1, s.desc.camera, s.desc.projection, lambda: tr.guide_ref(orc, s), **kw)
    return ref, out


def test_unchanged_camera_is_the_running_mean(box):
    """max_history = inf, k = 8 frames of 1 spp: every update out = h + (cur - h) * (1 / (n + 1)) rounds
    three times (the quotient, the product, the sum), each by at most 2^-24 of a value no larger than the
    largest frame value of the pixel, so after k updates the output is within 3 k 2^-24 max(pixel over the
    frames) of the frames' mean. Miss pixels are included (the mapping is the identity)."""
    s, orc, frames = box
    k = len(frames)
    ref, out = run(s, orc, frames, max_history=np.inf)
    stack = np.stack(frames).astype(np.float64)
    bound = 3 * k * 2.0 ** -24 * stack.max(axis=0)
    err = np.abs(out.astype(np.float64) - stack.mean(axis=0))
    assert (err <= bound).all(), (err.max(), bound[err > bound])
    assert (stack.max(axis=0) > 0).mean() > 0.5  # not vacuous: most pixels carry light
    assert (ref.H[..., 3] == k).all()
    assert np.array_equal(ref.H[..., :3], out)


def test_history_length_saturates(box):
    s, orc, frames = box
    ref, _ = run(s, orc, frames, max_history=4.0)
    assert (ref.H[..., 3] == 5.0).all()  # n = min(len, 4), len = n + 1
    ref, _ = run(s, orc, frames[:3], max_history=4.0)
    assert (ref.H[..., 3] == 3.0).all()


def test_a_pose_looking_the_other_way_has_no_history(box):
    s, orc, frames = box
    ref, _ = run(s, orc, frames[:2])
    away = tr.posed(s, dict(tr.move_sequence(s))["looking away"])
    o2 = Oracle(away, 4, "rtm")
    film = o2.render(3, seed=1234, threads=8)[0]
    out = ref.accumulate(film, 3, away.desc.camera, away.desc.projection, lambda: tr.guide_ref(o2, away))
    assert (ref.H[..., 3] == 3.0).all()
    assert np.array_equal(out, film / np.float32(3))


@pytest.mark.parametrize("size", [(64, 48), (33, 31)])
def test_the_small_move_keeps_most_of_the_history(size):
    """The condition the GPU sequence relies on, from the restatement alone: after the small move at least
    half of the pixels have len > spp (measured: 0.75 at 64 x 48, 0.85 at 33 x 31), and every other step of
    the sequence behaves as named."""
    s = loadScene(os.path.join(SCENES, "cornell-box"), width=size[0], height=size[1])
    ref = tr.TemporalRef()
    share = {}
    for label, pose in tr.move_sequence(s):
        ps = tr.posed(s, pose)
        orc = Oracle(ps, 4, "rtm")
        film = orc.render(1, seed=1234, threads=8)[0]
        ref.accumulate(film, 1, ps.desc.camera, ps.desc.projection, lambda: tr.guide_ref(orc, ps))
        share[label] = float((ref.H[..., 3] > 1).mean())
    assert share["first"] == 0.0 and share["unchanged"] == 1.0
    assert share["small move"] >= 0.5 and share["dolly-in"] >= 0.5, share
    assert share["looking away"] == 0.0, share
