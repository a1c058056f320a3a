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


def _vose_lockstep(p, positive):
    """light_sampling_ref.vose on every row of p (cells, n) at once: the same stacks, pops and pushes per
    row, the rows advancing together (a row whose stacks ran out waits). Returns (prob float64, alias)."""
    nc, n = p.shape
    p = p.copy()
    prob = np.ones((nc, n), np.float64)
    alias = np.tile(np.arange(n, dtype=np.int64), (nc, 1))
    is_small = p < 1.0
    # stacks as index arrays filled from the left in increasing index order, and their sizes
    order = np.argsort(~is_small, axis=1, kind="stable")   # the small indices first, increasing
    small, n_small = order.copy(), is_small.sum(1)
    order = np.argsort(is_small, axis=1, kind="stable")    # the large indices first, increasing
    large, n_large = order.copy(), n - n_small
    for _ in range(n):
        act = np.flatnonzero((n_small > 0) & (n_large > 0))
        if not len(act):
            break
        s = small[act, n_small[act] - 1]
        l = large[act, n_large[act] - 1]
        n_small[act] -= 1
        n_large[act] -= 1
        prob[act, s] = p[act, s]
        alias[act, s] = l
        p[act, l] = (p[act, l] + p[act, s]) - 1.0
        to_small = p[act, l] < 1.0
        a, b = act[to_small], act[~to_small]
        small[a, n_small[a]] = l[to_small]
        n_small[a] += 1
        large[b, n_large[b]] = l[~to_small]
        n_large[b] += 1
    left = np.arange(n)[None, :] < n_small[:, None]          # what stayed on the small stacks
    r, k = np.nonzero(left)
    idx = small[r, k]
    prob[r, idx] = np.where(positive[r, idx], 1.0, 0.0)
    return prob, alias.astype(U32)


def build_fast(records, weights, root_box, cells, lam):
    """build()'s "dims", "lo", "scale" and "entries", computed for a slab of z layers of cells at once, for grids
    whose cells a Python loop would take minutes over (64 x 64 x 64). The same binary64 operations in the
    same order per cell; tests/test_light_grid.py holds it equal to build() bit for bit."""
    dims, lo32, scale = layout(root_box, cells)
    rec = np.asarray(records, F).reshape(-1, 20)
    w = np.asarray(weights, np.float64).reshape(-1)
    n = len(w)
    rb = np.asarray(root_box, F).reshape(-1)[:6].astype(np.float64)
    lo, e = rb[:3], rb[3:6] - rb[:3]
    s = e / np.asarray(dims, np.float64)
    r2 = 0.25 * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    R = 0.5 * math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    kind = rec[:, 7].copy().view(np.int32)
    v = rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].astype(np.float64).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    v0, gn = rec[:, 0:3].astype(np.float64), rec[:, 12:15].astype(np.float64)
    lam = float(lam)
    dx, dy, dz = (int(d) for d in dims)
    ent = np.zeros((dx * dy * dz, n, 4), U32)
    nz = max(1, 4096 // (dx * dy))  # z layers per slab (larger slabs fall out of the cache and run slower)
    uni = uniform_entries(n)
    with np.errstate(all="ignore"):
        for z0 in range(0, dz, nz):
            iz, iy, ix = (a.reshape(-1).astype(np.float64) for a in
                          np.meshgrid(np.arange(z0, min(z0 + nz, dz)), np.arange(dy), np.arange(dx), indexing="ij"))
            ii = np.stack([ix, iy, iz], axis=1)                                   # (c, 3), x fastest
            clo, chi = lo + ii * s, lo + (ii + 1.0) * s
            d = np.maximum(np.maximum(0.0, tlo[None] - chi[:, None]), clo[:, None] - thi[None])  # (c, n, 3)
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            g = 1.0 / np.maximum(d2, r2)
            faces = np.zeros(g.shape, bool)
            for k in range(8):
                kx = chi[:, 0] + s[0] / 2.0 if k & 1 else clo[:, 0] - s[0] / 2.0
                ky = chi[:, 1] + s[1] / 2.0 if k & 2 else clo[:, 1] - s[1] / 2.0
                kz = chi[:, 2] + s[2] / 2.0 if k & 4 else clo[:, 2] - s[2] / 2.0
                dt = (((kx[:, None] - v0[None, :, 0]) * gn[None, :, 0] + (ky[:, None] - v0[None, :, 1]) * gn[None, :, 1])
                      + (kz[:, None] - v0[None, :, 2]) * gn[None, :, 2])
                faces |= dt > 0.0
            g = np.where(faces, g, 0.0)
            g = np.where(kind[None] == 0, g, 1.0 / (R * R))
            wc = w[None] * g                                                       # (c, n)
            total = np.cumsum(wc, axis=1)[:, -1]
            ok = np.isfinite(wc).all(1) & (total > 0.0) & np.isfinite(total)
            pmf = ((1.0 - lam) * wc) / total[:, None] + lam / float(n)
            pmf = np.where(ok[:, None], pmf, 1.0)
            prob, alias = _vose_lockstep(pmf * float(n), pmf > 0)
            pf = pmf.astype(F)
            slab = np.zeros((len(ix), n, 4), U32)
            slab[..., 0] = prob.astype(F).view(U32)
            slab[..., 1] = alias
            slab[..., 2] = pf.view(U32)
            slab[..., 3] = np.take_along_axis(pf, alias.astype(np.int64), axis=1).view(U32)
            slab[~ok] = uni
            ent[z0 * dx * dy:z0 * dx * dy + len(ix)] = slab
    return {"dims": dims, "lo": lo32, "scale": scale, "entries": ent}


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
