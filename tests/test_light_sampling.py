"""Light selection for NEE (rtg_set_light_sampling, RTG_LIGHTS_POWER), CPU side: the host's own C++
builder (rtg_light_pick_build, no device call) against the numpy restatement of
tests/light_sampling_ref.py bit for bit and against the alias invariant, the restated pick's histogram,
the builder's argument errors, and the restated DIRECT estimate at one floor point under the "unequal"
scene's lights in both modes."""
import ctypes as C
import os

import numpy as np
import pytest

import light_sampling_ref as lr
from light_pick_scenes import write_unequal_scene
from raytracingrenderer_amd import _native as N
from raytracingrenderer_amd import loadScene

F = np.float32


def host_build(weights, lam):
    path = os.path.join(N.LIB_DIR, "librtg.so")
    if not os.path.exists(path):
        pytest.skip("hipcc not available")
    lib = N.rtg()
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    n = len(w)
    pmf = np.zeros(max(n, 1), np.float64)
    prob = np.zeros(max(n, 1), np.float64)
    alias = np.zeros(max(n, 1), np.uint32)
    ent = np.zeros((max(n, 1), 4), F)
    rc = lib.rtg_light_pick_build(N.ptr(w, C.c_double) if n else N.ptr(np.zeros(1), C.c_double), n, float(lam),
                                  N.ptr(pmf, C.c_double), N.ptr(prob, C.c_double), N.ptr(alias, C.c_uint32),
                                  N.ptr(ent, C.c_float))
    return rc, pmf[:n], prob[:n], alias[:n], ent.view(np.uint32)[:n]


def weight_cases():
    rng = np.random.default_rng(281)
    w50 = rng.uniform(0.1, 3.0, 50)
    w50[[4, 17, 49]] = 0.0
    return {
        "one": np.array([2.5]),
        "two-equal": np.array([1.75, 1.75]),
        "one-bright-of-12": np.array([0.02] * 5 + [20.0] + [0.02] * 6),
        "three-zeros-of-50": w50,
        "random-281": rng.uniform(0.0, 1.0, 281) ** 4 * 10.0,
    }


def check_invariant(prob, alias, pmf, tol):
    """prob_i / n + sum over {j: alias_j = i} of (1 - prob_j) / n = pmf_i, prob == 0 exactly where
    pmf == 0, and such an entry is no alias."""
    err = np.abs(lr.alias_mass(prob, alias) - pmf)
    assert (err <= tol).all(), (float(err.max()), int(err.argmax()))
    assert abs(np.cumsum(pmf)[-1] - 1.0) <= 1e-12
    zero = pmf == 0
    assert (prob[zero] == 0).all() and not np.isin(alias, np.flatnonzero(zero)).any()
    assert ((prob >= 0) & (prob <= 1)).all() and (alias < len(pmf)).all()


@pytest.mark.parametrize("lam", [0.0, 0.125, 0.5, 1.0])
@pytest.mark.parametrize("name", sorted(weight_cases()))
def test_host_builder_equals_the_restatement(name, lam):
    """pmf, prob, alias and the entries bit for bit; the alias invariant to 1e-12."""
    w = weight_cases()[name]
    rc, pmf, prob, alias, ent = host_build(w, lam)
    assert rc == 0
    t = lr.build_table(w, lam)
    assert np.array_equal(pmf.view(np.uint64), t["pmf"].view(np.uint64))
    assert np.array_equal(prob.view(np.uint64), t["prob"].view(np.uint64))
    assert np.array_equal(alias, t["alias"])
    assert np.array_equal(ent, t["entries"])
    check_invariant(prob, alias, pmf, 1e-12)
    n = len(w)
    if name == "three-zeros-of-50":
        z = np.flatnonzero(w == 0)
        assert len(z) == 3
        if lam == 0.0:  # prob == 0 exactly, never an alias
            assert (pmf[z] == 0).all() and (prob[z] == 0).all() and not np.isin(alias, z).any()
            assert (ent[z, 0] == 0).all() and (ent[z, 2] == 0).all()
        else:           # pmf = lam / n
            assert (pmf[z] == lam / n).all()
    if lam == 1.0:
        assert (ent[:, 2].copy().view(F) == F(1.0) / F(n)).all()
        assert (ent[:, 3].copy().view(F) == F(1.0) / F(n)).all()
    if name == "one":
        assert pmf[0] == 1.0 and prob[0] == 1.0 and alias[0] == 0


@pytest.mark.parametrize("name", sorted(weight_cases()))
def test_restated_vose_is_env_sampling_refs_loop(name):
    """light_sampling_ref.vose on p = (w / sum) * n equals env_sampling_ref.build_alias(w), the loop it
    restates, bit for bit."""
    w = weight_cases()[name]
    al = lr.build_alias(w)
    total = float(np.cumsum(w)[-1])
    prob, alias = lr.vose([(float(x) / total) * float(len(w)) for x in w], w > 0)
    assert np.array_equal(prob.view(np.uint64), al["prob"].view(np.uint64)) and np.array_equal(alias, al["alias"])


def test_restated_picks_follow_the_pmf():
    """2^20 scripted draws on the 281-light and the one-bright-of-12 tables: each light's count within six
    standard errors of n * pmf (the project's criterion, tests/test_env_sampling.py), a pmf-0 light never."""
    rng = np.random.default_rng(7)
    n = 1 << 20
    r0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    d1 = (rng.integers(0, 2 ** 24, n).astype(F) * F(2.0 ** -24)).astype(F)
    for name, lam in (("random-281", 0.125), ("one-bright-of-12", 0.125), ("three-zeros-of-50", 0.0)):
        t = lr.build_table(weight_cases()[name], lam)
        li, pmf = lr.pick(t["entries"], r0, d1)
        p = t["pmf"]
        cnt = np.bincount(li, minlength=len(p))
        se = np.sqrt(n * p * (1 - p))
        z = np.abs(cnt - n * p) / np.maximum(se, 1e-300)
        assert (np.abs(cnt - n * p) <= 6 * se).all(), (name, float(z.max()))
        assert (cnt[p == 0] == 0).all()
        assert np.array_equal(pmf.view(np.uint32), p.astype(F)[li].view(np.uint32))


def test_builder_rejects_what_the_header_says():
    ok = np.array([1.0, 2.0, 3.0])
    assert host_build(ok, 0.125)[0] == 0
    assert host_build(np.zeros(0), 0.125)[0] == -1              # n == 0
    assert host_build(np.array([1.0, -0.5, 2.0]), 0.125)[0] == -1  # a negative weight
    assert host_build(np.array([1.0, np.nan]), 0.125)[0] == -1
    assert host_build(np.array([1.0, np.inf]), 0.125)[0] == -1
    assert host_build(np.zeros(5), 0.125)[0] == -1                # the weights sum to 0
    assert host_build(np.array([1e308, 1e308]), 0.125)[0] == -1   # ... to a non-finite value
    for lam in (-0.01, 1.01, np.nan, np.inf):
        assert host_build(ok, lam)[0] == -1
    assert b"rtg_light_pick_build" in N.rtg().rtg_last_error()
    p = N.rtg_light_sampling(7, 7.0)
    assert N.rtg().rtg_light_sampling_defaults(C.byref(p)) == 0
    assert p.mode == N.RTG_LIGHTS_UNIFORM and p.uniform_share == 0.125


# ---------------------------------------------------------------- the estimate at one point
def scene_light_records(scene):
    """(n, 20) float32 light records of a loaded scene, as light_sampling_ref reads them (area and normal
    from the vertices in binary64, rounded: this test compares distributions, not bits)."""
    P = scene.positions.astype(np.float64)
    rec = np.zeros((len(scene.lights), 20), F)
    for k, t in enumerate(scene.lights):
        v0, v1, v2 = P[t]
        c = np.cross(v1 - v0, v2 - v0)
        area = 0.5 * np.linalg.norm(c)
        m = scene.materials[scene.material_index[t]]
        rec[k, 0:3], rec[k, 3] = v0, area
        rec[k, 4:7] = v1
        rec[k, 8:11], rec[k, 11] = v2, 1.0 / area
        gn = c / np.linalg.norm(c)
        rec[k, 12:15] = gn if gn[1] < 0 else -gn  # the emitters face down
        rec[k, 16:19] = m.emission[:]
    return rec


def direct_estimates(rec, entries, x, sn, f, n, seed):
    """n restated DIRECT samples (luminance of f E g / (pmf pdf), no occluder) at point x with normal sn:
    the uniform pick when entries is None."""
    rng = np.random.default_rng(seed)
    draw = lambda: (rng.integers(0, 2 ** 24, n).astype(F) * F(2.0 ** -24)).astype(F)  # noqa: E731
    nl = len(rec)
    if entries is None:
        li = np.minimum((F(nl) * draw()).astype(np.int64), nl - 1)
        pmf = np.full(n, F(1.0) / F(nl), F)
    else:
        r0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        li, pmf = lr.pick(entries, r0, draw())
    L = rec[li]
    p2 = lr.triangle_sample(L, draw(), draw())
    g, _ = lr.area_geometry(L, p2, np.broadcast_to(x, (n, 3)).astype(F), np.broadcast_to(sn, (n, 3)).astype(F))
    ld = ((f * L[:, 16:19]) * g[:, None]) / (pmf * L[:, 11])[:, None]
    return np.where(g > 0, lr.lum32(ld), F(0)).astype(np.float64)


def unequal_variance_ratio(tmp_path, n=1 << 18):
    s = loadScene(write_unequal_scene(tmp_path / "unequal"))
    assert len(s.lights) == 22
    rec = scene_light_records(s)
    w = lr.light_weights(rec)
    t = lr.build_table(w, 0.125)
    x, sn, f = np.array([-0.45, 0.0, 0.35], F), np.array([0.0, 1.0, 0.0], F), F(1.0 / np.pi)
    u = direct_estimates(rec, None, x, sn, f, n, 1)
    p = direct_estimates(rec, t["entries"], x, sn, f, n, 2)
    return u, p, w


def test_both_picks_estimate_the_same_direct_light(tmp_path):
    """The restated DIRECT estimate at a floor point of the "unequal" scene (2^18 samples per mode): the
    uniform and power means agree within six standard errors of their difference. The variance ratio
    uniform / power printed here (4.9 with these seeds) is where tests/test_light_sampling_gpu.py takes its
    threshold from: half of it."""
    u, p, w = unequal_variance_ratio(tmp_path)
    n = len(u)
    se = np.sqrt(u.var(ddof=1) / n + p.var(ddof=1) / n)
    ratio = u.var(ddof=1) / p.var(ddof=1)
    print("uniform mean %.6g var %.6g; power mean %.6g var %.6g; variance ratio %.3f; panel share of the power %.3f"
          % (u.mean(), u.var(ddof=1), p.mean(), p.var(ddof=1), ratio, np.sort(w)[-2:].sum() / w.sum()))
    assert abs(u.mean() - p.mean()) <= 6 * se, (u.mean(), p.mean(), se)
    assert ratio > 1.0
