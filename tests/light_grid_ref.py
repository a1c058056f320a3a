"""TEST INFRASTRUCTURE ONLY — numpy restatement of the per-shading-point light selection of include/rtg.h
(rtg_set_light_grid): the grid over the root box, the cell of a point, the per-cell weights, pmf and alias
tables and the pick, operation by operation in the order the header states. The per-light weights, Vose
and light_pick are tests/light_sampling_ref.py's, unchanged.

  grid           the box is the reference root box, six float32 values widened to binary64, lo_a, hi_a,
                 e_a = hi_a - lo_a, E the largest e_a. dims_a = max(1, ceil(cells * (e_a / E))), 1 on a
                 degenerate axis. float32 constants: lo_a, scale_a = (float)dims_a / (hi_a - lo_a) (float32
                 subtraction and division), 0 on a degenerate axis.
  cell of x      float32: u = (x_a - lo_a) * scale_a; i_a = (int)u clamped to [0, dims_a - 1], NaN -> 0;
                 c = (i_z * dims_y + i_y) * dims_x + i_x.
  weights        binary64. s_a = e_a / dims_a; the cell's box clo_a = lo_a + i_a * s_a, chi_a = lo_a +
                 (i_a + 1) * s_a. Area light: d_a = max(0, tlo_a - chi_a, clo_a - thi_a) against the box of the
                 three float32 vertices; d2 = (d_x^2 + d_y^2) + d_z^2; r2 = 0.25 * ((s_x^2 + s_y^2) + s_z^2);
                 g = 1 / max(d2, r2); g = 0 when no corner k of the box widened by s_a / 2 on every side has
                 ((k_x - v0_x) gn_x + (k_y - v0_y) gn_y) + (k_z - v0_z) gn_z > 0. Environment: g = 1 / (R * R).
                 w_ic = w_i * g.
  per cell       pmf_ic = ((1 - lambda) * w_ic) / sum_c + lambda / n, sum_c in light order; a sum that is 0 or
                 not finite: the uniform table (prob 1, alias self, pmf (float)(1.0 / n)); else Vose on
                 pmf * n. Entries {prob, alias, pmf_self, pmf_alias} at table[c * n + k].
  pick           li = light_pick(table + c * n, n, r0, d1, pmf).
"""
import math

import numpy as np

import light_sampling_ref as lr

F = np.float32
U32 = np.uint32


def layout(root_box, cells):
    """(dims (3,) int, lo (3,) float32, scale (3,) float32)."""
    rb = np.asarray(root_box, F).reshape(-1)[:6]
    e = [float(rb[3 + a]) - float(rb[a]) for a in range(3)]
    emax = max([0.0] + [x for x in e if x > 0.0])
    dims, scale = [], []
    for a in range(3):
        flat = not (e[a] > 0.0) or not (emax > 0.0) or not math.isfinite(emax)
        d = 1.0 if flat else math.ceil(float(cells) * (e[a] / emax))
        d = min(max(d, 1.0), float(cells))
        dims.append(int(d))
        with np.errstate(all="ignore"):
            scale.append(F(0) if flat else F(int(d)) / (rb[3 + a] - rb[a]))
    return np.array(dims, np.int64), rb[:3].copy(), np.array(scale, F)


def cell_of(points, dims, lo, scale):
    """(n,) int64 cell index of points (n, 3) float32."""
    x = np.asarray(points, F).reshape(-1, 3)
    idx = []
    with np.errstate(all="ignore"):
        for a in range(3):
            u = ((x[:, a] - F(lo[a])) * F(scale[a])).astype(F)
            u = np.where(np.isnan(u), F(0), u)
            u = np.minimum(np.maximum(u, F(0)), F(int(dims[a]) - 1)).astype(F)
            idx.append(u.astype(np.int64))  # (truncation: u is in [0, dims - 1])
    return (idx[2] * int(dims[1]) + idx[1]) * int(dims[0]) + idx[0]


def cell_weights(records, weights, root_box, dims):
    """(cells, n) float64: w_ic = w_i * g."""
    rec = np.asarray(records, F).reshape(-1, 20)
    w = np.asarray(weights, np.float64).reshape(-1)
    rb = np.asarray(root_box, F).reshape(-1)[:6].astype(np.float64)
    lo, e = rb[:3], rb[3:6] - rb[:3]
    s = e / np.asarray(dims, np.float64)
    r2 = 0.25 * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    R = 0.5 * math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    kind = rec[:, 7].copy().view(np.int32)
    v = rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].astype(np.float64).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    v0, gn = rec[:, 0:3].astype(np.float64), rec[:, 12:15].astype(np.float64)
    out = np.zeros((int(np.prod(dims)), len(w)), np.float64)
    c = 0
    with np.errstate(all="ignore"):
        for iz in range(int(dims[2])):
            for iy in range(int(dims[1])):
                for ix in range(int(dims[0])):
                    ii = np.array([ix, iy, iz], np.float64)
                    clo, chi = lo + ii * s, lo + (ii + 1.0) * s
                    d = np.maximum(np.maximum(0.0, tlo - chi), clo - thi)
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    g = 1.0 / np.maximum(d2, r2)
                    faces = np.zeros(len(w), bool)
                    for k in range(8):
                        kx = chi[0] + s[0] / 2.0 if k & 1 else clo[0] - s[0] / 2.0
                        ky = chi[1] + s[1] / 2.0 if k & 2 else clo[1] - s[1] / 2.0
                        kz = chi[2] + s[2] / 2.0 if k & 4 else clo[2] - s[2] / 2.0
                        dt = ((kx - v0[:, 0]) * gn[:, 0] + (ky - v0[:, 1]) * gn[:, 1]) + (kz - v0[:, 2]) * gn[:, 2]
                        faces |= dt > 0.0
                    g = np.where(faces, g, 0.0)
                    g = np.where(kind == 0, g, 1.0 / (R * R))
                    out[c] = w * g
                    c += 1
    return out


def uniform_entries(n):
    e = np.zeros((n, 4), U32)
    e[:, 0] = np.array([1.0], F).view(U32)[0]
    e[:, 1] = np.arange(n)
    e[:, 2] = e[:, 3] = np.array([1.0 / float(n)], np.float64).astype(F).view(U32)[0]
    return e


def build(records, weights, root_box, cells, lam):
    """{"dims", "lo", "scale", "weights" (cells, n), "pmf" (cells, n) float64, "entries" (cells, n, 4) uint32,
    "uniform" (cells,) bool: the cell got the uniform table}."""
    dims, lo, scale = layout(root_box, cells)
    wc = cell_weights(records, weights, root_box, dims)
    n = wc.shape[1]
    ent = np.zeros((len(wc), n, 4), U32)
    pmf = np.zeros_like(wc)
    unif = np.zeros(len(wc), bool)
    for c in range(len(wc)):
        t = None
        if np.isfinite(wc[c]).all():
            t = lr.build_table(wc[c], lam)
        if t is None:
            ent[c], pmf[c], unif[c] = uniform_entries(n), 1.0 / float(n), True
        else:
            ent[c], pmf[c] = t["entries"], t["pmf"]
    return {"dims": dims, "lo": lo, "scale": scale, "weights": wc, "pmf": pmf, "entries": ent, "uniform": unif}


def pick(entries, cell, r0, d1):
    """light_pick against the table of each point's cell: (li (n,) int64, pmf (n,) float32)."""
    ent = np.asarray(entries, U32)
    nc, n = ent.shape[0], ent.shape[1]
    r0 = np.ascontiguousarray(r0, U32).reshape(-1)
    d1 = np.ascontiguousarray(d1, F).reshape(-1)
    k = ((r0.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    t = ent.reshape(nc * n, 4)[np.asarray(cell, np.int64) * n + k]
    keep = d1 < t[:, 0].copy().view(F)
    li = np.where(keep, k, t[:, 1].astype(np.int64))
    pmf = np.where(keep, t[:, 2], t[:, 3]).astype(U32).view(F)
    return li, pmf
