"""Numpy restatement of the illumination mode of variance-guided filtering (include/rtg.h:
rtg_svgf_illum_accumulate; csrc/device/rtg_svgf_illum.hip), composed from the unchanged svgf_ref.SvgfRef.

IEEE float32 with one rounding per operation. A is the denoiser's albedo guide of the current camera, G its
geometry guide.
  divisor     per channel d.c = A.c > albedo_floor ? A.c : 1.0f (a NaN fails the comparison and gives 1).
  classed G'  G, except that a pixel whose first-hit material is a light (L(emission) > 0 in float32, as
              rtg_scene.hip derives DevMat::is_light) gets the miss records {0, 0, 0, FLT_MAX} {0, 0, 0, id = -1}.
  prepare     F' = film / d (the film's sums).
  chain       SvgfRef.accumulate on F' and G' (its history, moments, history camera and stored guide are this
              mode's own); the albedo and shading-normal terms read the denoiser's guides as they are.
  remodulate  out = rgb * d."""
import numpy as np

from svgf_ref import SvgfRef, lum32
from temporal_ref import FLT_MAX

F = np.float32


def divisor(albedo, albedo_floor=1e-3):
    A = np.ascontiguousarray(albedo, F)
    with np.errstate(invalid="ignore"):
        return np.where(A > F(albedo_floor), A, F(1.0)).astype(F)


def emitter_triangles(scene):
    """Per triangle: its material is a light, triangle -> material -> L(emission) > 0."""
    lit = np.array([bool(lum32(np.array(m.emission[:], F)) > 0) for m in scene.materials], bool)
    return lit[scene.material_index]


def emitter_mask(guide, scene):
    """(h, w) bool: the pixels whose first hit (the guide's triangle id) lies on an emitter."""
    ids = np.ascontiguousarray(guide[1][..., 3]).view(np.int32)
    hit = ids >= 0
    mask = np.zeros(ids.shape, bool)
    mask[hit] = emitter_triangles(scene)[ids[hit]]
    return mask


def classed(guide, mask):
    """The guide with the miss records at the masked pixels."""
    pos_t, nid = guide[0].copy(), guide[1].copy()
    pos_t[mask] = np.array([0, 0, 0, FLT_MAX], F)
    nid[mask] = np.array([0, 0, 0, np.array(-1, np.int32).view(F)], F)
    return pos_t, nid


class SvgfIllumRef:
    """The state of rtg_svgf_illum_accumulate: a SvgfRef of its own (self.s) run on demodulated films and
    classed guides. scene: whose materials decide the emitter class (None: no pixel is masked)."""

    def __init__(self, scene=None):
        self.s = SvgfRef()
        self.scene = scene
        self.d = None        # the last call's divisor
        self.mask = None     # ... and emitter mask (of the guide the call computed; None when it needed none)

    def _classed(self, guide_of):
        g = guide_of()
        self.mask = emitter_mask(g, self.scene) if self.scene is not None else np.zeros(g[0].shape[:2], bool)
        return classed(g, self.mask)

    def accumulate(self, film, spp, cam, proj, guide_of, albedo, normal, albedo_floor=1e-3, **kw):
        """As SvgfRef.accumulate, plus albedo_floor. Returns the (h, w, 3) output; self.H, self.M, self.var and
        self.guide are the new state."""
        self.d = d = divisor(albedo, albedo_floor)
        self.mask = None
        with np.errstate(all="ignore"):
            out = self.s.accumulate((np.ascontiguousarray(film, F) / d).astype(F), spp, cam, proj,
                                    lambda: self._classed(guide_of), albedo, normal, **kw)
            return (out * d).astype(F)

    H = property(lambda self: self.s.t.H)          # illumination and len
    M = property(lambda self: self.s.M)
    var = property(lambda self: self.s.var)
    spatial = property(lambda self: self.s.spatial)
    guide = property(lambda self: self.s.t.guide)  # the classed guide of the history camera
