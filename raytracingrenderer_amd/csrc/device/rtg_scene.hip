// rtg_scene.hip — the host half of rtg_create: an rtg_scene_desc (the flattened reference Scene)
// turned into the device records of HostScene (prepare_scene), among them the trees k_trace walks.
// Host code only: no kernel and no HIP runtime call (tests/native/scene_digest.cpp pins its output
// on the CPU). rtg_api.hip's upload_scene copies the records to a device.
#include "rtg_internal.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

static float host_bits_f(int v) { float f; std::memcpy(&f, &v, 4); return f; }

// Compressed 4-wide node: per axis the smallest power-of-two step with origin + 255*step >= max,
// then each slot bound rounded outward and verified with the device's decode (qdecode), so the
// decoded box contains the exact one. Returns false if a step would leave the exponent range.
static bool encode_qnode(const float* bounds, const std::vector<int>& slots, const int32_t* words, DevNodeQ& out) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = bounds[(size_t)slots[0] * 6 + a];
        hi[a] = bounds[(size_t)slots[0] * 6 + 3 + a];
        for (int k = 1; k < (int)slots.size(); ++k) {
            lo[a] = std::min(lo[a], bounds[(size_t)slots[k] * 6 + a]);
            hi[a] = std::max(hi[a], bounds[(size_t)slots[k] * 6 + 3 + a]);
        }
    }
    unsigned planes[6] = {0, 0, 0, 0, 0, 0};
    unsigned bexp[3];
    for (int a = 0; a < 3; ++a) {
        const double ext = (double)hi[a] - (double)lo[a];
        int e = ext > 0 ? (int)std::ceil(std::log2(ext / 255.0)) : -126;
        e = std::max(e, -126);
        for (;; ++e) {
            if (e > 119) return false;
            if (rtgd::qdecode(lo[a], 255u, 0, host_bits_f((e + 127) << 23)) >= hi[a]) break;
        }
        bexp[a] = (unsigned)(e + 127);
        const float sc = host_bits_f((e + 127) << 23);
        for (int k = 0; k < (int)slots.size(); ++k) {
            const float mn = bounds[(size_t)slots[k] * 6 + a], mx = bounds[(size_t)slots[k] * 6 + 3 + a];
            int ql = (int)std::floor(((double)mn - (double)lo[a]) / std::ldexp(1.0, e));
            int qh = (int)std::ceil(((double)mx - (double)lo[a]) / std::ldexp(1.0, e));
            ql = std::min(std::max(ql, 0), 255);
            qh = std::min(std::max(qh, 0), 255);
            while (ql > 0 && rtgd::qdecode(lo[a], (unsigned)ql, 0, sc) > mn) --ql;
            while (qh < 255 && rtgd::qdecode(lo[a], (unsigned)qh, 0, sc) < mx) ++qh;
            if (rtgd::qdecode(lo[a], (unsigned)ql, 0, sc) > mn || rtgd::qdecode(lo[a], (unsigned)qh, 0, sc) < mx)
                return false;
            planes[a] |= (unsigned)ql << (8 * k);
            planes[3 + a] |= (unsigned)qh << (8 * k);
        }
    }
    auto uf = [](unsigned v) { float f; std::memcpy(&f, &v, 4); return f; };
    out.q[0] = make_float4(lo[0], lo[1], lo[2], uf(bexp[0] | (bexp[1] << 8) | (bexp[2] << 16)));
    out.q[1] = make_float4(uf(planes[0]), uf(planes[1]), uf(planes[2]), uf(planes[3]));
    out.q[2] = make_float4(uf(planes[4]), uf(planes[5]), host_bits_f(words[0]), host_bits_f(words[1]));
    out.q[3] = make_float4(host_bits_f(words[2]), host_bits_f(words[3]), 0.0f, 0.0f);
    return true;
}
static float host_dot(const float* a, const float* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
static void host_cross(const float* a, const float* b, float* o) {
    o[0] = (a[1] * b[2]) - (a[2] * b[1]);
    o[1] = (a[2] * b[0]) - (a[0] * b[2]);
    o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}

// Own binary SAH tree over the scene's triangles (or the reference's leaves), in the descriptor's node
// format (links {left, right, start, end}, bounds {min xyz, max xyz}; node 0 is the root). Internal
// boxes are float min/max unions, so containment is exact and the wide walk built from this tree
// reaches every primitive whose box the ray passes; k_trace's leaf-box test keeps reachability the
// reference's. The reference splits along the longest axis only (Geometry.h:343-386); this build
// tries all three: full SAH sweep below 2048 primitives, 64 centroid bins per axis above.
static bool rebuild_over_leaves(const rtg_scene_desc* d, std::vector<int32_t>& lk, std::vector<float>& bd) {
    // Primitives (round 5): every triangle alone, its box inflated by 2^-17 of the scene scale and
    // rounded outward (a hit that rayIntersect reports lies within rounding of its triangle, far inside
    // that margin plus the slot test's), so a wide leaf slot holds one triangle
    // and its box is the triangle's, not its reference leaf's. C3: triangle tests per ray 11.7 -> 6.4,
    // node steps 25.3 -> 27.0, traversal -12.5 %; C4 -40 %. (Keeping two consecutive triangles in one
    // slot when their union box is no larger than their two boxes measured slower everywhere, even on
    // quads: the leaf's two tests are one dependent chain.) Acceptance is unchanged: a candidate hit
    // counts only if its reference leaf box passes the exact test (leafbox). Non-finite positions:
    // the primitives are the reference leaves, kept whole (as in rounds 2-4).
    std::vector<float> pbox;
    std::vector<std::array<int32_t, 4>> plink;
    bool tri_ok = true;
    for (size_t k = 0; tri_ok && k < (size_t)d->n_tris * 9; ++k) tri_ok = std::isfinite(d->positions[k]);
    if (tri_ok) {
        float scale = 0.0f;
        for (int k = 0; k < 6; ++k)
            if (std::isfinite(d->node_bounds[k])) scale = std::max(scale, std::fabs(d->node_bounds[k]));
        const double eps = std::ldexp((double)scale, -17);
        for (uint32_t t = 0; t < d->n_tris; ++t) {
            const float* P = d->positions + (size_t)t * 9;
            for (int a = 0; a < 3; ++a) {
                const double lo = std::min(std::min(P[a], P[3 + a]), P[6 + a]) - eps;
                pbox.push_back(std::nextafter((float)lo, -INFINITY));
            }
            for (int a = 0; a < 3; ++a) {
                const double hi = std::max(std::max(P[a], P[3 + a]), P[6 + a]) + eps;
                pbox.push_back(std::nextafter((float)hi, INFINITY));
            }
            plink.push_back({-1, -1, (int32_t)t, (int32_t)t + 1});
        }
    } else {
        for (uint32_t i = 0; i < d->n_nodes; ++i) {
            const int32_t* L = d->node_links + (size_t)i * 4;
            if (L[0] >= 0) continue;
            pbox.insert(pbox.end(), d->node_bounds + (size_t)i * 6, d->node_bounds + (size_t)i * 6 + 6);
            plink.push_back({L[0], L[1], L[2], L[3]});
        }
    }
    const size_t n = plink.size();
    if (n < 2) return false;
    auto box = [&](int p) { return pbox.data() + (size_t)p * 6; };
    std::vector<float> cen(n * 3);
    for (size_t p = 0; p < n; ++p)
        for (int a = 0; a < 3; ++a) cen[p * 3 + a] = 0.5f * (box((int)p)[a] + box((int)p)[a + 3]);
    struct Bx {
        float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        void add(const float* o) {
            for (int a = 0; a < 3; ++a) { b[a] = std::min(b[a], o[a]); b[a + 3] = std::max(b[a + 3], o[a + 3]); }
        }
        double area() const {
            if (b[0] > b[3]) return 0.0;
            const double x = (double)b[3] - b[0], y = (double)b[4] - b[1], z = (double)b[5] - b[2];
            return x * y + y * z + z * x;
        }
    };
    // SAH weight of a leaf: its triangle count (1-2); full sweep below 2048 leaves, 64 centroid
    // bins per axis above (a full sweep to 16384 leaves or 256 bins measured no better)
    const int sweep_max = RTG_SAH_SWEEP, nbins = RTG_SAH_BINS;
    std::vector<double> wt(n), pre;
    for (size_t p = 0; p < n; ++p) wt[p] = (double)(plink[p][3] - plink[p][2]);
    std::vector<int> idx(n);
    for (size_t p = 0; p < n; ++p) idx[p] = (int)p;
    lk.assign((2 * n - 1) * 4, -1);
    bd.assign((2 * n - 1) * 6, 0.0f);
    int next = 1;
    std::vector<std::array<int, 4>> st{{0, 0, (int)n, 0}};  // node id, range [lo, hi) of idx, depth
    std::vector<Bx> suf;
    while (!st.empty()) {
        auto [node, lo, hi, dep] = st.back();
        st.pop_back();
        if (dep > 96) return false;  // degenerate SAH chain: keep the reference tree (bounded stacks)
        const int m = hi - lo;
        Bx all;
        for (int p = lo; p < hi; ++p) all.add(box(idx[p]));
        std::memcpy(&bd[(size_t)node * 6], all.b, sizeof(all.b));
        if (m == 1) {
            std::memcpy(&lk[(size_t)node * 4], plink[idx[lo]].data(), 4 * sizeof(int32_t));
            continue;
        }
        double best = INFINITY;
        int bax = -1, bsplit = lo + m / 2;  // fallback: median of the current order
        int bbin = 0;
        if (m <= sweep_max) {
            for (int a = 0; a < 3; ++a) {
                std::sort(idx.begin() + lo, idx.begin() + hi, [&](int x, int y) {
                    return cen[x * 3 + a] < cen[y * 3 + a] || (cen[x * 3 + a] == cen[y * 3 + a] && x < y);
                });
                suf.assign(m + 1, Bx());
                for (int p = m - 1; p >= 0; --p) { suf[p] = suf[p + 1]; suf[p].add(box(idx[lo + p])); }
                pre.assign(m + 1, 0.0);
                for (int p = 0; p < m; ++p) pre[p + 1] = pre[p] + wt[idx[lo + p]];
                Bx left;
                for (int p = 1; p < m; ++p) {
                    left.add(box(idx[lo + p - 1]));
                    const double c = left.area() * pre[p] + suf[p].area() * (pre[m] - pre[p]);
                    if (c < best) { best = c; bax = a; bsplit = lo + p; }
                }
            }
            if (bax >= 0) {
                std::sort(idx.begin() + lo, idx.begin() + hi, [&](int x, int y) {
                    return cen[x * 3 + bax] < cen[y * 3 + bax] || (cen[x * 3 + bax] == cen[y * 3 + bax] && x < y);
                });
            }
        } else {
            const int NB = nbins;
            Bx cb;
            for (int p = lo; p < hi; ++p) {
                const float* c = &cen[(size_t)idx[p] * 3];
                const float cc[6] = {c[0], c[1], c[2], c[0], c[1], c[2]};
                cb.add(cc);
            }
            for (int a = 0; a < 3; ++a) {
                const float ext = cb.b[a + 3] - cb.b[a];
                if (!(ext > 0.0f)) continue;
                std::vector<Bx> bins(NB), right(NB + 1);
                std::vector<double> cnt(NB, 0.0), rc(NB + 1, 0.0);
                for (int p = lo; p < hi; ++p) {
                    const int b = std::min(NB - 1, (int)((cen[(size_t)idx[p] * 3 + a] - cb.b[a]) / ext * NB));
                    bins[b].add(box(idx[p]));
                    cnt[b] += wt[idx[p]];
                }
                for (int b = NB - 1; b >= 0; --b) { right[b] = right[b + 1]; right[b].add(bins[b].b); rc[b] = rc[b + 1] + cnt[b]; }
                Bx left;
                double lc = 0;
                for (int b = 1; b < NB; ++b) {
                    left.add(bins[b - 1].b);
                    lc += cnt[b - 1];
                    if (lc == 0 || rc[b] == 0) continue;
                    const double c = left.area() * lc + right[b].area() * rc[b];
                    if (c < best) { best = c; bax = a; bbin = b; }
                }
            }
            if (bax >= 0) {
                const float ext = cb.b[bax + 3] - cb.b[bax];
                auto mid = std::partition(idx.begin() + lo, idx.begin() + hi, [&](int x) {
                    return std::min(NB - 1, (int)((cen[(size_t)x * 3 + bax] - cb.b[bax]) / ext * NB)) < bbin;
                });
                bsplit = (int)(mid - idx.begin());
                if (bsplit == lo || bsplit == hi) bsplit = lo + m / 2;
            }
        }
        const int l = next++, r = next++;
        lk[(size_t)node * 4] = l;
        lk[(size_t)node * 4 + 1] = r;
        lk[(size_t)node * 4 + 2] = lk[(size_t)node * 4 + 3] = 0;
        st.push_back({r, bsplit, hi, dep + 1});
        st.push_back({l, lo, bsplit, dep + 1});
    }
    return next == (int)(2 * n - 1);
}

// The host half of rtg_create: the descriptor (the flattened reference Scene) turned into the device
// records. No HIP calls: a group builds this once and uploads it to every device in parallel.
int prepare_scene(const rtg_scene_desc* d, HostScene& hs) {
    if (d->n_lights == 0) {
        g_err = "scene has no lights (RTBase's Scene::sampleLight indexes an empty list: Scene.h:137-138)";
        return RTG_ERR_NO_LIGHTS;
    }
    const uint32_t nt = d->n_tris;

    // ---- triangles: Triangle::init (Geometry.h:72-83) + gNormal (:127-130)
    std::vector<DevTri48> tris48(nt);
    std::vector<DevShade> shade(nt);
    std::vector<float> tri_area(nt), tri_gn(nt * 3);
    for (uint32_t i = 0; i < nt; ++i) {
        const float* P = d->positions + (size_t)i * 9;
        const float *v0 = P, *v1 = P + 3, *v2 = P + 6;
        float e1[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
        float e2[3] = {v0[0] - v2[0], v0[1] - v2[1], v0[2] - v2[2]};
        float c[3];
        host_cross(e1, e2, c);
        float l = 1.0f / std::sqrt(((c[0] * c[0]) + (c[1] * c[1])) + (c[2] * c[2]));
        float n[3] = {c[0] * l, c[1] * l, c[2] * l};
        tri_area[i] = std::sqrt(((c[0] * c[0]) + (c[1] * c[1])) + (c[2] * c[2])) * 0.5f;
        const float* N = d->normals + (size_t)i * 9;
        float s = host_dot(N, n) > 0 ? 1.0f : -1.0f;
        for (int k = 0; k < 3; ++k) tri_gn[i * 3 + k] = n[k] * s;
        tris48[i].a = make_float4(n[0], n[1], n[2], v0[0]);
        tris48[i].b = make_float4(v0[1], v0[2], v1[0], v1[1]);
        tris48[i].c = make_float4(v1[2], v2[0], v2[1], v2[2]);
        const float* U = d->uvs + (size_t)i * 6;
        if (d->material[i] >= d->n_materials) { g_err = "triangle material index out of range"; return RTG_ERR_ARG; }
        shade[i].a = make_float4(N[0], N[1], N[2], N[3]);
        shade[i].b = make_float4(N[4], N[5], N[6], N[7]);
        shade[i].c = make_float4(N[8], U[0], U[1], U[2]);
        shade[i].d = make_float4(U[3], U[4], U[5], host_bits_f((int)d->material[i]));
    }
    // ---- BVH: reference DFS nodes -> child-pair internal nodes
    const uint32_t nn = d->n_nodes;
    if (nn == 0) { g_err = "BVH has no nodes"; return RTG_ERR_ARG; }
    std::vector<int> internal_id(nn, -1);
    int n_internal = 0;
    for (uint32_t i = 0; i < nn; ++i)
        if (d->node_links[i * 4 + 0] >= 0) internal_id[i] = n_internal++;
    auto word = [&](int node, int& out) -> bool {
        const int32_t* L = d->node_links + (size_t)node * 4;
        if (L[0] >= 0) { out = internal_id[node]; return true; }
        int cnt = L[3] - L[2];
        if (cnt < 1 || cnt > 2 || L[2] < 0 || (uint32_t)L[3] > nt) return false;
        out = ~(L[2] * RTG_LEAF_SPAN + (cnt - 1));
        return true;
    };
    std::vector<DevNode> nodes(std::max(n_internal, 1));
    uint32_t depth = 0;
    {
        std::vector<std::pair<int, uint32_t>> st{{0, 0}};
        while (!st.empty()) {
            auto [i, dep] = st.back();
            st.pop_back();
            depth = std::max(depth, dep);
            const int32_t* L = d->node_links + (size_t)i * 4;
            if (L[0] < 0) continue;
            if (L[0] >= (int)nn || L[1] < 0 || L[1] >= (int)nn) { g_err = "bad BVH link"; return RTG_ERR_ARG; }
            const float* bl = d->node_bounds + (size_t)L[0] * 6;
            const float* br = d->node_bounds + (size_t)L[1] * 6;
            DevNode& dn = nodes[internal_id[i]];
            dn.a = make_float4(bl[0], bl[1], bl[2], bl[3]);
            dn.b = make_float4(bl[4], bl[5], br[0], br[1]);
            dn.c = make_float4(br[2], br[3], br[4], br[5]);
            int wl, wr;
            if (!word(L[0], wl) || !word(L[1], wr)) {
                g_err = "BVH leaf with other than 1-2 triangles (MAXNODE_TRIANGLES = 2)";
                return RTG_ERR_ARG;
            }
            dn.d = make_int4(wl, wr, 0, 0);
            st.push_back({L[1], dep + 1});
            st.push_back({L[0], dep + 1});
        }
    }
    hs.bvh_depth = depth;
    int root_word = RTG_EXIT;
    if (nt > 0) {
        if (!word(0, root_word)) { g_err = "bad BVH root"; return RTG_ERR_ARG; }
    }
    // ---- wide collapse: each node's slots are a cut of the BVH2 subtree below it, grown by
    // repeatedly opening the internal slot of largest surface area (leaves stay slots). Exact
    // boxes are kept, so reachability is the reference's (see k_trace).
    std::vector<DevNodeQ> nodesq;
    bool qok = true;
    int root_wordw = root_word;
    bool finite = true;
    for (size_t k = 0; k < (size_t)nn * 6; ++k) finite = finite && std::isfinite(d->node_bounds[k]);
    // Skipping levels is exact only if every child box lies inside its parent's (true for
    // Scene::build's bounds; checked so that a foreign descriptor degrades to the BVH2 walk).
    for (uint32_t i = 0; finite && i < nn; ++i) {
        const int32_t* L = d->node_links + (size_t)i * 4;
        if (L[0] < 0) continue;
        const float* P = d->node_bounds + (size_t)i * 6;
        for (int c : {L[0], L[1]}) {
            const float* Cb = d->node_bounds + (size_t)c * 6;
            for (int q = 0; q < 3; ++q) finite = finite && Cb[q] >= P[q] && Cb[q + 3] <= P[q + 3];
        }
    }
    if (nt > 0 && finite && d->node_links[0] >= 0) {
        // the tree the wide nodes are cut from: an own SAH tree with spatial splits (build_sbvh), else
        // with object splits only (rebuild_over_leaves), or the reference BVH2 when neither can be built
        std::vector<int32_t> rlk;
        std::vector<float> rbd;
        const bool rebuilt = build_sbvh(d, rlk, rbd) || rebuild_over_leaves(d, rlk, rbd);
        const int32_t* LK = rebuilt ? rlk.data() : d->node_links;
        const float* BD = rebuilt ? rbd.data() : d->node_bounds;
        const uint32_t nn = rebuilt ? (uint32_t)(rlk.size() / 4) : d->n_nodes;
        auto wordw = [&](int node, int& out) -> bool {  // leaf word (leaves are the reference's)
            const int32_t* L = LK + (size_t)node * 4;
            const int cnt = L[3] - L[2];
            if (L[0] >= 0 || cnt < 1 || cnt > 2 || L[2] < 0 || (uint32_t)L[3] > nt) return false;
            out = ~(L[2] * RTG_LEAF_SPAN + (cnt - 1));
            return true;
        };
        hs.rebuilt = rebuilt;
        auto internal = [&](int i) { return LK[(size_t)i * 4] >= 0; };
        // the slots of the wide node made from BVH2 node n2: a cut of its subtree below it (wide_cut)
        auto cut = [&](int n2) {
            int s[4];
            const int n = wide_cut(LK, BD, n2, s);
            return std::vector<int>(s, s + n);
        };
        nodesq.emplace_back();
        root_wordw = 0;
        std::vector<std::array<int, 3>> work{{0, 0, 1}};  // BVH2 node, wide node, wide level
        while (!work.empty()) {
            auto [n2, nw, lvl] = work.back();
            work.pop_back();
            hs.wide_depth = std::max(hs.wide_depth, (uint32_t)lvl);
            const std::vector<int> slots = cut(n2);
            int32_t wq[4] = {RTG_EXIT, RTG_EXIT, RTG_EXIT, RTG_EXIT};
            for (int k = 0; k < (int)slots.size(); ++k) {
                if (internal(slots[k])) {
                    wq[k] = (int)nodesq.size();
                    nodesq.emplace_back();
                    work.push_back({slots[k], wq[k], lvl + 1});
                } else if (!wordw(slots[k], wq[k])) {
                    g_err = "bad BVH leaf";
                    return RTG_ERR_ARG;
                }
            }
            if (!encode_qnode(BD, slots, wq, nodesq[nw])) { qok = false; break; }
        }
    }
    float cull_scale = 0.0f;
    for (int k = 0; k < 6; ++k)
        if (std::isfinite(d->node_bounds[k])) cull_scale = std::max(cull_scale, std::fabs(d->node_bounds[k]));
    // the compressed walk's rounding margin is stated relative to the scene scale (k_trace)
    hs.usew = finite && qok && nt > 0 && cull_scale >= 0x1p-60f && cull_scale <= 0x1p60f;
    // exact leaf boxes per triangle (compressed walk: candidate hits re-test their leaf)
    std::vector<float4> leafbox(std::max<size_t>((size_t)nt * 2, 2));
    for (uint32_t i = 0; i < nn; ++i) {
        const int32_t* L = d->node_links + (size_t)i * 4;
        if (L[0] >= 0) continue;
        const float* b = d->node_bounds + (size_t)i * 6;
        for (int t = L[2]; t < L[3]; ++t) {
            leafbox[2 * (size_t)t] = make_float4(b[0], b[1], b[2], b[3]);
            leafbox[2 * (size_t)t + 1] = make_float4(b[4], b[5], 0.0f, 0.0f);
        }
    }
    // (the leaf boxes stay in global memory, read once per candidate hit)
    const bool small = hs.usew && nodesq.size() * 4 + (size_t)nt * 3 <= RTG_SMALL_F4;
    // small scenes: the image k_trace<.., SMALL> copies into LDS (wide nodes | triangles)
    if (small) {
        hs.img.clear();
        for (const DevNodeQ& q : nodesq) hs.img.insert(hs.img.end(), q.q, q.q + 4);
        hs.img_tri = (int)hs.img.size();
        for (const DevTri48& t : tris48) hs.img.insert(hs.img.end(), {t.a, t.b, t.c});
        hs.img_lb = (int)hs.img.size();
    }
    // ---- materials, textures, lights
    std::vector<DevMat> mats(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const rtg_material& m = d->materials[i];
        if (m.texture < 0 || (uint32_t)m.texture >= d->n_textures) { g_err = "material texture out of range"; return RTG_ERR_ARG; }
        mats[i].kind = m.kind;
        mats[i].two_sided = m.two_sided;
        mats[i].tex = m.texture;
        const float lm = ((0.2126f * m.emission[0]) + (0.7152f * m.emission[1])) + (0.0722f * m.emission[2]);
        mats[i].is_light = lm > 0 ? 1 : 0;
        mats[i].int_ior = m.int_ior;
        mats[i].ext_ior = m.ext_ior;
        mats[i].emission = make_float4(m.emission[0], m.emission[1], m.emission[2], 0.0f);
    }
    std::vector<DevTex> texinfo(d->n_textures);
    std::vector<float> texels;
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const rtg_texture& t = d->textures[i];
        if (t.width <= 0 || t.height <= 0 || !t.texels) { g_err = "empty texture"; return RTG_ERR_ARG; }
        texinfo[i] = DevTex{(int)(texels.size() / 4), t.width, t.height, 0};
        for (size_t j = 0; j < (size_t)t.width * t.height; ++j)  // RGB + pad: one 16-B load per texel
            texels.insert(texels.end(), {t.texels[3 * j], t.texels[3 * j + 1], t.texels[3 * j + 2], 0.0f});
    }
    if (d->env_texture >= (int)d->n_textures) { g_err = "env texture out of range"; return RTG_ERR_ARG; }
    // textures whose texels all have the same bits (1x1, or constant like C3's environment): the
    // kernels' bilinear taps use the first texel instead of four dependent fetches (the same operands)
    std::vector<char> uniform_tex(d->n_textures, 1);
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const rtg_texture& t = d->textures[i];
        const size_t n = (size_t)t.width * t.height;
        for (size_t j = 1; j < n && uniform_tex[i]; ++j)
            uniform_tex[i] = std::memcmp(t.texels + 3 * j, t.texels, 3 * sizeof(float)) == 0;
    }
    for (uint32_t i = 0; i < d->n_materials; ++i) {  // texture offset and size into the material record
        const DevTex& t = texinfo[mats[i].tex];
        if (t.w > 0xffff || t.h > 0xffff) { g_err = "texture larger than 65535 texels per side"; return RTG_ERR_ARG; }
        mats[i].tex = t.off;
        mats[i].tex_wh = (int)((unsigned)t.w | ((unsigned)t.h << 16));
        mats[i].uniform = uniform_tex[(size_t)(&t - texinfo.data())] ? 1 : 0;
        mats[i].texel0 = make_float4(texels[(size_t)t.off * 4], texels[(size_t)t.off * 4 + 1], texels[(size_t)t.off * 4 + 2], 0.0f);
    }
    // Identical material records merged (a scene file gives every instance its own BSDF: bathroom_f
    // has 852 for 24 distinct ones), so k_shade can hold the table in LDS; the triangles' shading
    // records are remapped. Same record, same arithmetic: the output does not change.
    {
        std::vector<DevMat> uniq;
        std::vector<int> remap(mats.size());
        for (size_t i = 0; i < mats.size(); ++i) {
            size_t j = 0;
            while (j < uniq.size() && std::memcmp(&uniq[j], &mats[i], sizeof(DevMat)) != 0) ++j;
            if (j == uniq.size()) uniq.push_back(mats[i]);
            remap[i] = (int)j;
        }
        for (uint32_t i = 0; i < nt; ++i) shade[i].d.w = host_bits_f(remap[d->material[i]]);
        mats.swap(uniq);
    }
    std::vector<DevLight> lights(d->n_lights);
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        int li = d->lights[i];
        DevLight& L = lights[i];
        std::memset(&L, 0, sizeof(L));
        if (li < 0) {
            if (d->env_texture < 0) { g_err = "environment light without an env texture"; return RTG_ERR_ARG; }
            L.v1t.w = host_bits_f(1);
            continue;
        }
        if ((uint32_t)li >= nt) { g_err = "light triangle out of range"; return RTG_ERR_ARG; }
        const float* P = d->positions + (size_t)li * 9;
        const float* em = d->materials[d->material[li]].emission;
        L.v0a = make_float4(P[0], P[1], P[2], tri_area[li]);
        L.v1t = make_float4(P[3], P[4], P[5], host_bits_f(0));
        L.v2 = make_float4(P[6], P[7], P[8], 1.0f / tri_area[li]);  // Triangle::sample's pdf
        L.gn = make_float4(tri_gn[li * 3], tri_gn[li * 3 + 1], tri_gn[li * 3 + 2], 0.0f);
        L.em = make_float4(em[0], em[1], em[2], 0.0f);
    }
    if (d->camera.width < 1.0f || d->camera.height < 1.0f) { g_err = "bad film size"; return RTG_ERR_ARG; }
    hs.nodes = std::move(nodes);
    hs.nodesq = std::move(nodesq);
    hs.leafbox = std::move(leafbox);
    hs.tris48 = std::move(tris48);
    hs.shade = std::move(shade);
    hs.mats = std::move(mats);
    hs.lights = std::move(lights);
    hs.texinfo = std::move(texinfo);
    hs.texels = std::move(texels);
    hs.n_lights = (int)d->n_lights;
    hs.env_tex = d->env_texture;
    hs.env_off = d->env_texture >= 0 ? hs.texinfo[d->env_texture].off : 0;
    hs.env_w = d->env_texture >= 0 ? hs.texinfo[d->env_texture].w : 1;
    hs.env_h = d->env_texture >= 0 ? hs.texinfo[d->env_texture].h : 1;
    hs.env_uniform = d->env_texture >= 0 && uniform_tex[d->env_texture];
    for (int k = 0; k < 3; ++k) hs.env_one[k] = d->env_texture >= 0 ? d->textures[d->env_texture].texels[k] : 0.0f;
    hs.root_word = root_word;
    hs.root_wordw = root_wordw;
    for (int k = 0; k < 6; ++k) hs.root_box[k] = d->node_bounds[k];
    hs.cull_scale = cull_scale;
    std::memcpy(hs.cam.ip, d->camera.inv_proj, sizeof(hs.cam.ip));
    std::memcpy(hs.cam.cm, d->camera.camera, sizeof(hs.cam.cm));
    hs.cam.ox = d->camera.origin[0];
    hs.cam.oy = d->camera.origin[1];
    hs.cam.oz = d->camera.origin[2];
    hs.cam.width = d->camera.width;
    hs.cam.height = d->camera.height;
    hs.proj = d->projection;
    hs.tri_mat.assign(d->material, d->material + nt);
    hs.n_desc_mats = d->n_materials;
    hs.light_tri.assign(d->lights, d->lights + d->n_lights);
    return RTG_OK;
}
