"""Per-shading-point light selection (rtg_set_light_grid), CPU side: the host's own C++ builder
(rtg_light_grid_build, no device call) against the numpy restatement of tests/light_grid_ref.py bit for bit,
the alias identity of every cell's table, the facing rule, the all-zero cell, the argument check, and the
restated DIRECT estimate at unoccluded floor points of the hall under the power pick and under the grid:
the variance ratio that tests/test_light_grid_gpu.py takes its threshold from."""
import ctypes as C
import os

import numpy as np
import pytest

import light_grid_ref as gr
import light_sampling_ref as lr
from light_grid_scenes import write_hall_scene, write_room_scene
from raytracingrenderer_amd import _native as N
from raytracingrenderer_amd import loadScene
from test_light_sampling import direct_estimates, scene_light_records

F = np.float32
LAM = 0.125


def lib():
    if not os.path.exists(os.path.join(N.LIB_DIR, "librtg.so")):
        pytest.skip("hipcc not available")
    return N.rtg()


def host_build(rec, w, root_box, cells, lam):
    """(rc, dims, lo, scale, entries (cells, n, 4) uint32) of rtg_light_grid_build."""
    L = lib()
    rec = np.ascontiguousarray(rec, F).reshape(-1, 20)
    w = np.ascontiguousarray(w, np.float64)
    rb = np.ascontiguousarray(root_box, F).reshape(-1)[:6].copy()
    n = len(rec)
    dims, lo, sc = np.zeros(3, np.uint32), np.zeros(3, F), np.zeros(3, F)
    args = (N.ptr(rec, C.c_float), n, N.ptr(w, C.c_double), N.ptr(rb, C.c_float), int(cells), float(lam),
            N.ptr(dims, C.c_uint32), N.ptr(lo, C.c_float), N.ptr(sc, C.c_float))
    rc = L.rtg_light_grid_build(*args, None)  # the layout first
    if rc:
        return rc, dims, lo, sc, None
    ent = np.zeros((int(dims.prod()), n, 4), F)
    rc = L.rtg_light_grid_build(*args, N.ptr(ent, C.c_float))
    return rc, dims, lo, sc, ent.view(np.uint32)


def scene_case(tmp_path, name):
    """(records, §8d weights, root box) of a test scene."""
    if name.startswith("hall"):
        s = loadScene(write_hall_scene(tmp_path / name, int(name[4:])))
    else:
        s = loadScene(write_room_scene(tmp_path / name))
    rec = scene_light_records(s)
    return rec, lr.light_weights(rec), np.array(s.node_bounds[0], F)


def with_environment(rec, w):
    """The list with an environment record (type bits 1) put in the middle, its weight of the order of the
    area lights' sum."""
    k = len(rec) // 2
    env = np.zeros((1, 20), F)
    env[0, 7] = np.array([1], np.int32).view(F)[0]
    return (np.concatenate([rec[:k], env, rec[k:]]), np.concatenate([w[:k], [0.3 * w.sum()], w[k:]]))


def check_alias_identity(ent, pmf):
    """Every cell: the pmf sums to 1, and prob_k / n + sum over {j: alias_j = k} of (1 - prob_j) / n is pmf_k
    (§8d's identity; prob is the float32 the entry holds, hence the 2^-24 per entry)."""
    n = ent.shape[1]
    for c in range(len(ent)):
        assert abs(np.cumsum(pmf[c])[-1] - 1.0) <= 1e-12, c
        prob = ent[c, :, 0].copy().view(F).astype(np.float64)
        err = np.abs(lr.alias_mass(prob, ent[c, :, 1]) - pmf[c])
        assert (err <= 2.0 ** -23).all(), (c, float(err.max()))
        assert (ent[c, :, 1] < n).all() and ((prob >= 0) & (prob <= 1)).all()
        assert np.array_equal(ent[c, :, 2].copy().view(F), pmf[c].astype(F))
        assert np.array_equal(ent[c, :, 3].copy().view(F), pmf[c].astype(F)[ent[c, :, 1]])


# ---------------------------------------------------------------- the argument check
def test_defaults_and_argument_check():
    L = lib()
    p = N.rtg_light_grid(7)
    assert L.rtg_light_grid_defaults(C.byref(p)) == 0 and p.cells == 0
    # without a scene: cells <= 64, and the thinnest grid any box gives (cells x 1 x 1) within 2^24 entries
    for cells, n, ok in ((0, 64, True), (1, 64, True), (64, 64, True), (65, 64, False), (64, 1 << 18, True),
                         (64, (1 << 18) + 1, False), (63, (1 << 18) + 1, True), (1, 1 << 24, True),
                         (1, (1 << 24) + 1, False), (0, 1 << 30, True)):
        rc = L.rtg_light_grid_check(C.byref(N.rtg_light_grid(cells)), n)
        assert (rc == 0) == ok, (cells, n, rc)
    assert L.rtg_light_grid_check(C.byref(N.rtg_light_grid(64)), (1 << 18) + 1) == -1
    assert b"largest admissible cells is 63" in L.rtg_last_error()
    assert L.rtg_light_grid_check(C.byref(N.rtg_light_grid(1000)), 4) == -1
    assert b"largest admissible cells is 64" in L.rtg_last_error()
    assert L.rtg_light_grid_check(None, 4) == -1
    rec, w, rb = np.zeros((2, 20), F), np.ones(2), np.array([0, 0, 0, 1, 1, 1], F)
    for cells, lam in ((0, LAM), (65, LAM), (4, -0.1), (4, 1.5), (4, float("nan"))):
        assert host_build(rec, w, rb, cells, lam)[0] == -1, (cells, lam)
    assert host_build(np.zeros((0, 20), F), np.zeros(0), rb, 4, LAM)[0] == -1
    # the builder counts the box's own cells: 40^3 cells of 281 lights are too many, 40 x 1 x 1 are not
    rec281, w281 = np.zeros((281, 20), F), np.ones(281)
    assert host_build(rec281, w281, rb, 40, LAM)[0] == -1
    assert host_build(rec281, w281, np.array([0, 0, 0, 40, 1, 1], F), 40, LAM)[0] == 0


# ---------------------------------------------------------------- the builder against the restatement
@pytest.mark.parametrize("name,cells,env", [("hall32", 1, False), ("hall32", 3, False), ("hall32", 8, False),
                                            ("hall12", 8, False), ("room", 4, False), ("hall12", 5, True)])
def test_host_builder_equals_the_restatement(tmp_path, name, cells, env):
    """dims, the float32 constants and every entry bit for bit; every cell's pmf sums to 1 and its table
    satisfies the alias identity."""
    rec, w, rb = scene_case(tmp_path, name)
    if env:
        rec, w = with_environment(rec, w)
    rc, dims, lo, sc, ent = host_build(rec, w, rb, cells, LAM)
    assert rc == 0
    want = gr.build(rec, w, rb, cells, LAM)
    assert np.array_equal(dims, want["dims"]) and dims.max() == cells, (dims, want["dims"])
    assert np.array_equal(lo.view(np.uint32), want["lo"].view(np.uint32))
    assert np.array_equal(sc.view(np.uint32), want["scale"].view(np.uint32))
    assert ent.shape == want["entries"].shape
    assert np.array_equal(ent, want["entries"]), int((ent != want["entries"]).any(2).sum())
    assert not want["uniform"].any()
    check_alias_identity(ent, want["pmf"])
    if name.startswith("hall"):
        assert tuple(dims) == (cells, max(1, int(np.ceil(cells * 1.98 / 16.0))), max(1, int(np.ceil(cells * 2 / 16.0))))
    if env:  # the environment's weight is the same share of every cell's scale: picked everywhere
        k = len(rec) // 2
        assert (want["pmf"][:, k] > LAM / len(rec)).all()


def test_one_cell_orders_the_lights_as_the_restatement_does(tmp_path):
    """cells = 1: one table, whose pmf is the restatement's w_i * g_i (one g per light, not constant across
    lights, so not §8d's pmf); in the room, where emission varies, a brighter light of two at the same
    distance from the box has the larger pmf."""
    rec, w, rb = scene_case(tmp_path, "room")
    rc, dims, lo, sc, ent = host_build(rec, w, rb, 1, LAM)
    want = gr.build(rec, w, rb, 1, LAM)
    assert rc == 0 and tuple(dims) == (1, 1, 1) and ent.shape[0] == 1
    assert np.array_equal(ent, want["entries"])
    pmf = ent[0, :, 2].copy().view(F)
    assert np.array_equal(np.argsort(pmf, kind="stable"), np.argsort(want["pmf"][0].astype(F), kind="stable"))
    # every light lies inside the one cell: d2 = 0, g = 1 / r2 for all, and the order is the power's
    assert np.array_equal(np.argsort(pmf, kind="stable"), np.argsort(lr.light_pmf(w, LAM).astype(F), kind="stable"))


def test_a_light_facing_away_from_a_widened_cell_has_the_uniform_share_only():
    """Two one-sided emitters in the middle of a box of 4 x 1 x 1 cells, one facing -x and one facing +x:
    in the cells two or more away on the side a light faces away from, its pmf is exactly lambda / n; in
    the neighbouring cell (inside the half cell of slack) it is not."""
    rec = np.zeros((2, 20), F)
    for k, gx in enumerate((-1.0, 1.0)):
        rec[k, 0:3], rec[k, 4:7], rec[k, 8:11] = (2.0, 0.4, 0.4), (2.0, 0.6, 0.4), (2.0, 0.4, 0.6)
        rec[k, 3], rec[k, 11], rec[k, 12] = 0.02, 50.0, gx
        rec[k, 16:19] = (3.0, 3.0, 3.0)
    w = lr.light_weights(rec)
    rb = np.array([0, 0, 0, 4, 1, 1], F)
    for lam in (0.0, 0.25):
        rc, dims, lo, sc, ent = host_build(rec, w, rb, 4, lam)
        assert rc == 0 and tuple(dims) == (4, 1, 1)
        want = gr.build(rec, w, rb, 4, lam)
        assert np.array_equal(ent, want["entries"])
        pmf = ent[:, :, 2].copy().view(F)
        # light 0 faces -x: cells 0, 1 (x < 2) see it; cell 2 touches its plane (slack); cell 3 is behind
        assert pmf[3, 0] == F(lam / 2.0) and pmf[0, 1] == F(lam / 2.0)
        assert pmf[2, 0] > F(lam / 2.0) and pmf[1, 1] > F(lam / 2.0)
        assert pmf[0, 0] == F((1.0 - lam) + lam / 2.0) and pmf[3, 1] == F((1.0 - lam) + lam / 2.0)


def test_an_all_zero_cell_is_uniform():
    """Both emitters face -x from x = 2: the cell at x in [3, 4] weighs every light 0 and gets the uniform
    table (prob 1, alias self, pmf 1 / n), at lambda = 0 as well."""
    rec = np.zeros((3, 20), F)
    for k in range(3):
        rec[k, 0:3], rec[k, 4:7], rec[k, 8:11] = (2.0, 0.2 + 0.1 * k, 0.4), (2.0, 0.6, 0.4), (2.0, 0.4, 0.6)
        rec[k, 3], rec[k, 11], rec[k, 12] = 0.02, 50.0, -1.0
        rec[k, 16:19] = (1.0 + k, 1.0, 1.0)
    w = lr.light_weights(rec)
    rb = np.array([0, 0, 0, 4, 1, 1], F)
    for lam in (0.0, LAM):
        rc, dims, lo, sc, ent = host_build(rec, w, rb, 4, lam)
        want = gr.build(rec, w, rb, 4, lam)
        assert rc == 0 and np.array_equal(ent, want["entries"])
        assert list(want["uniform"]) == [False, False, False, True]
        assert np.array_equal(ent[3], gr.uniform_entries(3))
        assert (ent[3, :, 0].copy().view(F) == 1).all() and list(ent[3, :, 1]) == [0, 1, 2]
        assert (ent[3, :, 2].copy().view(F) == F(1.0 / 3.0)).all()


@pytest.mark.parametrize("name,cells,env", [("hall32", 8, False), ("room", 5, False), ("hall12", 5, True)])
def test_slab_wise_restatement_equals_the_cell_wise_one(tmp_path, name, cells, env):
    """light_grid_ref.build_fast (a z slab of cells at once, Vose in lockstep; the whole-film GPU tests use it
    at 64 cells) gives build()'s layout and entries bit for bit, at lambda 0 and 0.125, and on
    test_an_all_zero_cell_is_uniform's box, where one cell takes the uniform table."""
    rec, w, rb = scene_case(tmp_path, name)
    if env:
        rec, w = with_environment(rec, w)
    for lam in (0.0, LAM):
        a, b = gr.build(rec, w, rb, cells, lam), gr.build_fast(rec, w, rb, cells, lam)
        assert np.array_equal(a["dims"], b["dims"]) and np.array_equal(a["lo"].view(np.uint32), b["lo"].view(np.uint32))
        assert np.array_equal(a["scale"].view(np.uint32), b["scale"].view(np.uint32))
        assert np.array_equal(a["entries"], b["entries"]), (name, lam, int((a["entries"] != b["entries"]).any(2).sum()))
    rec3 = np.zeros((3, 20), F)
    for k in range(3):
        rec3[k, 0:3], rec3[k, 4:7], rec3[k, 8:11] = (2.0, 0.2 + 0.1 * k, 0.4), (2.0, 0.6, 0.4), (2.0, 0.4, 0.6)
        rec3[k, 3], rec3[k, 11], rec3[k, 12] = 0.02, 50.0, -1.0
        rec3[k, 16:19] = (1.0 + k, 1.0, 1.0)
    box = np.array([0, 0, 0, 4, 1, 1], F)
    a, b = gr.build(rec3, lr.light_weights(rec3), box, 4, 0.0), gr.build_fast(rec3, lr.light_weights(rec3), box, 4, 0.0)
    assert a["uniform"].any() and np.array_equal(a["entries"], b["entries"])


def test_restated_cell_of_a_point():
    """Faces, the outside, NaN and infinities, on a grid with a degenerate axis."""
    dims, lo, sc = gr.layout(np.array([-8, 0, -1, 8, 0, 1], F), 8)
    assert list(dims) == [8, 1, 1] and sc[1] == 0 and sc[0] == F(0.5)
    x = np.array([[-8, 0, 0], [-6, 0, 0], [-6.0001, 5, 0], [7.9999, 0, 0], [8, 0, 0], [100, 0, 0], [-100, 0, 0],
                  [np.nan, np.nan, np.nan], [np.inf, 0, -np.inf], [0, np.inf, 0]], F)
    assert list(gr.cell_of(x, dims, lo, sc)) == [0, 1, 0, 7, 7, 7, 0, 0, 7, 4]


# ---------------------------------------------------------------- the expected gain
def hall_points():
    """Unoccluded floor points spread over the hall's length and width (away from the two cubes)."""
    return np.array([(x, 0.0, z) for x in (-7.0, -5.5, -2.5, -1.0, 0.0, 2.5, 4.0, 5.5, 7.0) for z in (-0.7, 0.0, 0.7)
                     if not (abs(x + 4.0) < 0.6 or abs(x - 1.0) < 0.6)], F)


def hall_variance_ratio(tmp_path, n_emitters, cells=8, n=1 << 15):
    """(power variances, grid variances, means) of the restated one-sample DIRECT estimator at hall_points():
    the per-sample variance under the power table and under the table of the point's cell."""
    rec, w, rb = scene_case(tmp_path, "hall%d" % n_emitters)
    power = lr.build_table(w, LAM)["entries"]
    g = gr.build(rec, w, rb, cells, LAM)
    pts = hall_points()
    cell = gr.cell_of(pts, g["dims"], g["lo"], g["scale"])
    sn, f = np.array([0.0, 1.0, 0.0], F), F(1.0 / np.pi)
    vp, vg, mean = [], [], []
    for k, x in enumerate(pts):
        a = direct_estimates(rec, power, x, sn, f, n, 100 + k)
        b = direct_estimates(rec, g["entries"][cell[k]], x, sn, f, n, 200 + k)
        vp.append(a.var(ddof=1))
        vg.append(b.var(ddof=1))
        mean.append((a.mean(), b.mean(), np.sqrt(a.var(ddof=1) / n + b.var(ddof=1) / n)))
    return np.array(vp), np.array(vg), np.array(mean)


@pytest.mark.parametrize("n_emitters", [32, 12])
def test_grid_and_power_estimate_the_same_direct_light_with_less_noise(tmp_path, n_emitters):
    """At each point the two picks' means agree within six standard errors of their difference, and the
    variance summed over the points falls. The ratio printed here for the 64-light hall is the yardstick of
    tests/test_light_grid_gpu.py's noise test (half of it), and must be at least 2 for that test to mean
    anything."""
    vp, vg, mean = hall_variance_ratio(tmp_path, n_emitters)
    ratio = vp.sum() / vg.sum()
    print("%d lights: per-sample variance summed over %d points: power %.6g, grid %.6g, ratio %.3f (per point %s)"
          % (2 * n_emitters, len(vp), vp.sum(), vg.sum(), ratio, np.round(vp / vg, 2)))
    assert (np.abs(mean[:, 0] - mean[:, 1]) <= 6 * mean[:, 2]).all(), mean
    assert ratio >= 2.0
