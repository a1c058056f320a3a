"""The physical material model without a GPU: the loader's parameter records, the host-side argument
checks, and properties of the model itself on its numpy restatement (tests/materials_ref.py, which
tests/test_materials_gpu.py holds the kernels to bit for bit).

Quadrature: the midpoint rule over (theta, phi) at two resolutions N and 2N. The rule converges at least
linearly here (the integrands are bounded; the visible-normal density has a jump where the half vector
reaches the horizon), so |I_2N - I_N| estimates I_2N's error; every bound below is twice that, plus 1e-5
for the float32 rounding of an integrand of about 40 operations (40 * 2^-24 = 2.4e-6, rounded up)."""
import os

import numpy as np
import pytest

import materials_ref as R
from conftest import SCENES
from raytracingrenderer_amd import NativeError, loadScene
from raytracingrenderer_amd import _native as N
from raytracingrenderer_amd.renderer import material_params_check

F = np.float32
GOLD = dict(eta=(1.65, 0.88, 0.52), k=(9.2, 6.3, 4.8))
ALPHAS = (0.1, 0.51, 1.62142)


def _alpha(r):
    return F(1.62142) * np.sqrt(F(r))


# ------------------------------------------------------------------ loader
def test_cornell_mat_parameters():
    s = loadScene(os.path.join(SCENES, "cornell-mat"), width=32, height=32)
    p = s.material_params
    assert len(p) == len(s.materials) == s.desc.n_materials
    tags = [q.model for q in p]
    assert tags == [N.RTG_MODEL_REFERENCE, N.RTG_MODEL_ORENNAYAR, N.RTG_MODEL_REFERENCE, N.RTG_MODEL_CONDUCTOR,
                    N.RTG_MODEL_PLASTIC, N.RTG_MODEL_REFERENCE, N.RTG_MODEL_REFERENCE, N.RTG_MODEL_REFERENCE]
    # alpha = 1.62142f * sqrtf(roughness), formed as the constructors form it: conductor 0.2, plastic 0.1
    # and the rough dielectric's 0.5 (kept, although it stays the Lambert stub)
    for i, r in ((3, 0.2), (4, 0.1), (2, 0.5)):
        assert F(p[i].alpha).tobytes() == _alpha(r).tobytes(), (i, p[i].alpha)
    assert [F(v) for v in p[3].eta] == [F(1.65), F(0.88), F(0.52)]
    assert [F(v) for v in p[3].k] == [F(9.2), F(6.3), F(4.8)]
    assert F(p[1].sigma) == F(0.3)
    assert (F(p[4].int_ior), F(p[4].ext_ior)) == (F(1.5), F(1.0))
    for i in (0, 5, 6, 7):  # diffuse, glass, mirror, emitter: nothing
        q = p[i]
        assert (q.alpha, q.sigma, q.int_ior, q.ext_ior, list(q.eta), list(q.k)) == (0, 0, 0, 0, [0] * 3, [0] * 3)
    # the material records themselves are what they were (the digests cover them): kinds only
    assert [m.kind for m in s.materials] == [0, 1, 1, 1, 1, 3, 2, 0]
    assert all(m.int_ior == 0 and m.ext_ior == 0 for m in s.materials if m.kind != N.RTG_MAT_GLASS)


def test_coffee_small_has_delta_plastics():
    s = loadScene(os.path.join(SCENES, "coffee-small"), width=32, height=32)
    p = s.material_params
    plastics = [q for q in p if q.model == N.RTG_MODEL_PLASTIC]
    assert len(plastics) == 6
    assert sorted(q.alpha for q in plastics)[:3] == [0.0, 0.0, 0.0]
    rough = [q for q in plastics if q.alpha != 0]
    assert len(rough) == 3
    for q in rough:
        assert F(q.alpha).tobytes() == _alpha(0.003803723578239983).tobytes()
        assert F(q.alpha) >= F(N.RTG_ALPHA_DELTA)  # 0.1 > 0.01: a GGX lobe, not a delta one
        assert (F(q.int_ior), F(q.ext_ior)) == (F(1.5), F(1.0))


def test_loader_defaults(tmp_path):
    """Missing keys take SceneLoader.h's defaults: roughness 1, intIOR 1.33, extIOR 1, alpha 1, eta = k = 0."""
    import json
    base = json.load(open(os.path.join(SCENES, "cornell-mat", "scene.json")))
    box = os.path.relpath(os.path.join(SCENES, "cornell-box"), str(tmp_path))
    inst = []
    for i, bsdf in enumerate(("conductor", "plastic", "orennayar")):
        d = {k: v for k, v in base["instances"][i].items() if k in ("filename", "world")}
        d["filename"] = os.path.join(box, os.path.basename(d["filename"]))
        d["reflectance"] = os.path.join(box, "1_1_1.png")
        d["bsdf"] = bsdf
        inst.append(d)
    inst.append(dict(base["instances"][7], filename=os.path.join(box, os.path.basename(base["instances"][7]["filename"])),
                     reflectance=os.path.join(box, "0_0_0_1.0.png")))
    base["instances"] = inst
    json.dump(base, open(os.path.join(str(tmp_path), "scene.json"), "w"))
    p = loadScene(str(tmp_path), width=32, height=32).material_params
    assert [q.model for q in p[:3]] == [N.RTG_MODEL_CONDUCTOR, N.RTG_MODEL_PLASTIC, N.RTG_MODEL_ORENNAYAR]
    assert F(p[0].alpha).tobytes() == _alpha(1.0).tobytes() and list(p[0].eta) == [0] * 3 and list(p[0].k) == [0] * 3
    assert F(p[1].alpha).tobytes() == _alpha(1.0).tobytes()
    assert (F(p[1].int_ior), F(p[1].ext_ior)) == (F(1.33), F(1.0))
    assert p[2].sigma == 1.0


# ------------------------------------------------------------------ argument checks (no device call)
def _rec(model=N.RTG_MODEL_PLASTIC, alpha=0.5, sigma=0.0):
    return N.rtg_material_params(model, alpha, sigma, (N.C.c_float * 3)(1, 1, 1), (N.C.c_float * 3)(2, 2, 2), 1.5, 1.0)


def test_params_check():
    ok = [_rec(), _rec(N.RTG_MODEL_REFERENCE, 0, 0), _rec(N.RTG_MODEL_ORENNAYAR, 0, 0.3)]
    material_params_check(ok, 3)
    for n in (2, 4):
        with pytest.raises(NativeError, match="one record per scene material"):
            material_params_check(ok, n)
    for bad in (_rec(alpha=-0.1), _rec(alpha=float("nan")), _rec(alpha=float("inf")), _rec(sigma=-1.0),
                _rec(sigma=float("nan"))):
        with pytest.raises(NativeError, match="negative or non-finite"):
            material_params_check(ok[:2] + [bad], 3)
    for tag in (-1, 4, 99):
        with pytest.raises(NativeError, match="unknown model tag"):
            material_params_check(ok[:2] + [_rec(model=tag)], 3)
    assert N.rtg().rtg_material_params_check(None, 0, 0) == -1


# ------------------------------------------------------------------ the restatement's own properties
def _dirs(theta, phi):
    st, ct = np.sin(theta), np.cos(theta)
    return [(st * np.cos(phi)).astype(F), (st * np.sin(phi)).astype(F), ct.astype(F)]


def _wo(cos_t, n):
    s = np.sqrt(max(0.0, 1.0 - cos_t * cos_t))
    return [np.full(n, s, F), np.zeros(n, F), np.full(n, cos_t, F)]


def _quad(fn, n, sphere):
    """Midpoint rule of fn(wi) sin(theta) over the hemisphere or the sphere, n x 2n cells, in binary64."""
    top = np.pi if sphere else 0.5 * np.pi
    th = (np.arange(n) + 0.5) * (top / n)
    ph = (np.arange(2 * n) + 0.5) * (np.pi / n)
    T, P = [a.reshape(-1) for a in np.meshgrid(th, ph, indexing="ij")]
    v = np.asarray(fn(_dirs(T, P)), np.float64)
    w = np.sin(T) * (top / n) * (np.pi / n)
    return float(np.sum(v * (w if v.ndim == 1 else w[:, None]), axis=0).max())


def _quad2(fn, sphere=False, n=384):
    a, b = _quad(fn, n, sphere), _quad(fn, 2 * n, sphere)
    return b, 2.0 * abs(b - a) + 1e-5


def _models():
    out = [R.Params("orennayar", sigma=0.3)]
    for a in ALPHAS:
        out += [R.Params("conductor", alpha=a, **GOLD), R.Params("plastic", alpha=a, int_ior=1.5, ext_ior=1.0)]
    return out


def test_reciprocity_is_exact():
    """f(wo, wi) = f(wi, wo) bit for bit for all three models: every operand order in include/rtg.h's
    evaluate is symmetric (wo + wi, |wo + wi| / 2 as the Fresnel cosine, G1(wi) G1(wo), (4 wo.z) wi.z,
    (1 - F(wo.z)) (1 - F(wi.z)), max(wi.z, wo.z)), and IEEE + and * commute."""
    rng = np.random.default_rng(7)
    n = 4000
    a = _dirs(np.arccos(rng.random(n)), 2 * np.pi * rng.random(n))
    b = _dirs(np.arccos(rng.random(n)), 2 * np.pi * rng.random(n))
    for q in _models():
        f1, f2 = R.evaluate(q, (0.8, 0.5, 0.3), a, b), R.evaluate(q, (0.8, 0.5, 0.3), b, a)
        assert f1.tobytes() == f2.tobytes(), q.model
        assert np.isfinite(f1).all() and (f1 >= 0).all()


@pytest.mark.parametrize("cos_o", [1.0, 0.70710678, 0.25881905])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_visible_normal_pdf_integrates_to_one_over_the_sphere(alpha, cos_o):
    """G1(wo) D(h) / (4 wo.z) over every wi whose half vector lies above the surface (reflections below
    the horizon included: those end the path). The conductor's PDF is its upper-hemisphere part."""
    q = R.Params("conductor", alpha=alpha, **GOLD)

    def raw(wi):
        wo = _wo(cos_o, len(wi[0]))
        with np.errstate(all="ignore"):
            ok, h, _ = R.half(wo, wi)
            p = R.ggx_vndf_pdf(wo, h, q.alpha)
            up = R.pdf(q, wo, wi)
        assert np.array_equal(up[wi[2] > 0], np.where(ok, p, 0).astype(F)[wi[2] > 0])
        return np.where(ok & (h[2] > 0), p, 0)

    total, bound = _quad2(raw, sphere=True)
    assert abs(total - 1.0) <= bound, (total, bound)


@pytest.mark.parametrize("cos_o", [1.0, 0.70710678, 0.25881905])
@pytest.mark.parametrize("alpha", ALPHAS + (0.0,))
def test_plastic_mixture_pdf(alpha, cos_o):
    """The mixture's PDF over the hemisphere, plus ps times the visible-normal mass that falls below the
    horizon (samples that end the path), is 1. A delta coat (alpha 0) leaves (1 - ps) on the hemisphere."""
    q = R.Params("plastic", alpha=alpha, int_ior=1.5, ext_ior=1.0)
    ps = float(R.plastic_ps(R.fresnel_coat(np.array([cos_o], F), q))[0])
    assert 0.25 <= ps <= 0.75
    hemi, b1 = _quad2(lambda wi: R.pdf(q, _wo(cos_o, len(wi[0])), wi))
    if q.delta:
        assert abs(hemi - (1.0 - ps)) <= b1, (hemi, ps, b1)
        return

    def lost(wi):
        wo = _wo(cos_o, len(wi[0]))
        with np.errstate(all="ignore"):
            ok, h, _ = R.half(wo, wi)
            return np.where(ok & (h[2] > 0) & ~(wi[2] > 0), R.ggx_vndf_pdf(wo, h, q.alpha), 0)

    low, b2 = _quad2(lost, sphere=True)
    assert abs(hemi + ps * low - 1.0) <= b1 + b2, (hemi, low, ps)


@pytest.mark.parametrize("cos_o", [1.0, 0.70710678, 0.25881905, 1e-3])
def test_energy(cos_o):
    """Integral of f cos over the hemisphere with albedo 1. Conductor with F = 1 (eta = k = 0 makes both
    Fresnel halves 1) and the plastic: at most 1. Oren-Nayar: at most A + B / 2, which bounds the model
    from the integral of max(0, cos dphi) (2) and of sin^2 (pi / 4), and at most 1 up to 75 degrees (at
    grazing wo the qualitative model with sigma 0.3 reaches 1.005: a property of the model)."""
    def albedo(q):
        return _quad2(lambda wi: R.evaluate(q, (1, 1, 1), _wo(cos_o, len(wi[0])), wi) * wi[2][:, None])

    for a in ALPHAS:
        if cos_o < 0.01 and a < 0.2:
            continue  # (a 0.1-wide lobe at the horizon is not resolved by this grid)
        for q in (R.Params("conductor", alpha=a), R.Params("plastic", alpha=a, int_ior=1.5, ext_ior=1.0)):
            v, bound = albedo(q)
            assert v <= 1.0 + bound, (q.model, a, v, bound)
    s2 = 0.3 * 0.3
    A, B = 1 - s2 / (2 * (s2 + 0.33)), 0.45 * s2 / (s2 + 0.09)
    v, bound = albedo(R.Params("orennayar", sigma=0.3))
    assert v <= A + B / 2 + bound, (v, bound)
    if cos_o > 0.25:
        assert v <= 1.0 + bound, (v, bound)


def test_sample_returns_evaluate_and_pdf():
    """For scripted draws, sample()'s colour and pdf are evaluate(wi) and PDF(wi) bit for bit on non-delta
    samples; delta samples reflect about the normal and carry the lobe's weight."""
    draws = np.array([(a, b, c) for a in (0.0, 0.5, 1 - 2.0 ** -24) for b in (0.0, 0.5, 1 - 2.0 ** -24)
                      for c in (0.0, 0.5, 1 - 2.0 ** -24)], F)
    n = len(draws)
    alb = (0.8, 0.5, 0.3)
    for cos_o in (1.0, 0.70710678, 1e-3):
        wo = _wo(cos_o, n)
        for q in _models() + [R.Params("conductor", alpha=0.0, **GOLD), R.Params("plastic", alpha=0.0099)]:
            s = R.sample(q, alb, wo, draws)
            live = (s["pdf"] > 0) & ~s["delta"]
            assert np.isfinite(s["colour"]).all() and np.isfinite(s["pdf"]).all()
            assert s["colour"][live].tobytes() == R.evaluate(q, alb, wo, s["wi"])[live].tobytes()
            assert s["pdf"][live].tobytes() == R.pdf(q, wo, s["wi"])[live].tobytes()
            d = s["delta"]
            assert d.any() == q.delta
            assert np.array_equal(R.arr(s["wi"])[d], R.arr([-wo[0], -wo[1], wo[2]])[d])
            if q.model == R.CONDUCTOR:  # a delta lobe is left out of evaluate and PDF
                assert not R.evaluate(q, alb, wo, s["wi"])[d].any() and not R.pdf(q, wo, s["wi"])[d].any()
