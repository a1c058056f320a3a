// walk_model — TEST INFRASTRUCTURE ONLY (tests/test_bvh_opt.py). A CPU model of
// what the 4-wide walk pays on a tree of rtg_bvh.hip's build_sbvh: the binary tree is built as
// sbvh_check builds it, cut into 4-wide nodes by prepare_scene's own rule (wide_cut, rtg_internal.h),
// and a fixed seeded ray set is walked near-first with a stack: closest-hit rays culled by distance,
// any-hit rays leaving at the first hit, on the slots' boxes snapped to their node's 8-bit planes (or
// the float boxes, --float-boxes). It counts node steps and triangle tests per ray. It is a model, not
// an oracle: no parked leaves, its own triangle test.
//
// The ray set is the mix of the path tracer's launches 0-2 on the synthetic scene: pixel-centre camera
// rays on a coarse grid, and from each hit (twice over) one cosine-hemisphere continuation ray and one
// uniform-sphere any-hit ray.
//
// One line per tree: the tree as built (passes 0) and, with --passes P > 0, the tree after optimise_bvh2.
// Built by build.py build_walk_model; run:
//   walk_model <scene dir> [options] | walk_model x synth <n> [options] | walk_model x mesh <kind> [options]
//   kinds: two, identical3, centroid64, chain28
//   options: --passes P  --frac F  --priority K  --grid G (camera rays: G x G)  --seed S
//            --stop F (the last pass: one that gains less than F of the area sum)
//            --min-tris N (no pass below N triangles; 0 here, RTG_BVH_OPT_MIN_TRIS in the product)
//            --check (every ray against a loop over all triangles)  --only-opt (skip the passes-0 tree)
//            --float-boxes (walk the slots' float boxes, not their 8-bit planes)
#include "../../include/rth.h"
#include "../../raytracingrenderer_amd/csrc/device/rtg_internal.h"

#include <unistd.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace {

struct V { double x, y, z; };
V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V norm(V a) { return a * (1.0 / std::sqrt(dot(a, a))); }

struct Ray { V o, d; double tmax; };
struct Hit { double t = INFINITY; int tri = -1; };

uint64_t mix(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
double unit(uint64_t seed, uint64_t ray, uint64_t k) { return (double)(mix(mix(seed ^ mix(ray)) + k) >> 11) * 0x1p-53; }

// the one triangle test of the walk and of the loop over all triangles (two-sided, 0 < t < tmax)
bool tri_test(const float* P, const Ray& r, double& t) {
    const V a{P[0], P[1], P[2]}, e1 = V{P[3], P[4], P[5]} - a, e2 = V{P[6], P[7], P[8]} - a;
    const V p = cross(r.d, e2);
    const double det = dot(e1, p);
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const V s = r.o - a;
    const double u = dot(s, p) * inv;
    if (u < 0.0 || u > 1.0) return false;
    const V q = cross(s, e1);
    const double v = dot(r.d, q) * inv;
    if (v < 0.0 || u + v > 1.0) return false;
    t = dot(e2, q) * inv;
    return t > 0.0 && t < r.tmax;
}

// slab test on a float box, widened a little so that it never rejects a point tri_test accepts
bool box_test(const float* b, const Ray& r, double tmax, double& tn) {
    double t0 = 0.0, t1 = tmax;
    const double o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
    for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.0) {
            if (o[k] < b[k] || o[k] > b[k + 3]) return false;
            continue;
        }
        double a = (b[k] - o[k]) / d[k], c = (b[k + 3] - o[k]) / d[k];
        if (a > c) std::swap(a, c);
        a -= 1e-9 * (1.0 + std::fabs(a));
        c += 1e-9 * (1.0 + std::fabs(c));
        t0 = std::max(t0, a);
        t1 = std::min(t1, c);
    }
    tn = t0;
    return t0 <= t1;
}

struct Wide {
    std::vector<std::array<int, 4>> slot;  // >= 0: a wide node; < 0: ~(binary leaf node); RTG_EXIT: unused
    std::vector<std::array<int, 4>> bin;   // the binary node of each slot
    std::vector<std::array<float, 24>> box;  // the slots' boxes as the walk tests them
    std::vector<int> n;
    int depth = 0;
    double area_sum = 0.0;  // over the binary nodes that became wide nodes, / the root's
    long fill[5] = {0, 0, 0, 0, 0};
};

struct Tree {
    std::vector<int32_t> lk;
    std::vector<float> bd;
    Wide w;
    double build_ms = 0.0, opt_ms = 0.0, sah = 0.0;
    int depth = 0;
    bool order_ok = true;
    uint64_t digest = 0, leaf_digest = 0;
    size_t leaves = 0;
};

double area(const std::vector<float>& bd, int n) {
    const float* b = &bd[(size_t)n * 6];
    const double x = b[3] - b[0], y = b[4] - b[1], z = b[5] - b[2];
    return x * y + y * z + z * x;
}

uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 0x100000001b3ull;
    return h;
}

// quant: the slots' boxes snapped outward to the 8-bit planes of their wide node (255 steps of a power
// of two per axis from the node's lower corner, as encode_qnode lays them); else the float boxes
void measure_tree(Tree& T, bool quant) {
    const std::vector<int32_t>& lk = T.lk;
    const size_t nn = lk.size() / 4;
    const double ra = area(T.bd, 0);
    std::vector<std::pair<int, int>> st{{0, 0}};
    std::vector<std::array<uint32_t, 7>> leaves;
    while (!st.empty()) {
        const auto [n, dep] = st.back();
        st.pop_back();
        T.depth = std::max(T.depth, dep);
        if (lk[(size_t)n * 4] < 0) {
            std::array<uint32_t, 7> e;
            e[0] = (uint32_t)lk[(size_t)n * 4 + 2];
            std::memcpy(&e[1], &T.bd[(size_t)n * 6], 24);
            leaves.push_back(e);
            continue;
        }
        T.sah += area(T.bd, n) / ra;
        for (int k = 0; k < 2; ++k) {
            const int c = lk[(size_t)n * 4 + k];
            if (c <= n || (size_t)c >= nn) { T.order_ok = false; return; }
            st.push_back({c, dep + 1});
        }
    }
    std::sort(leaves.begin(), leaves.end());
    T.leaves = leaves.size();
    T.leaf_digest = fnv(0xcbf29ce484222325ull, leaves.data(), leaves.size() * sizeof(leaves[0]));
    T.digest = fnv(fnv(0xcbf29ce484222325ull, lk.data(), lk.size() * 4), T.bd.data(), T.bd.size() * 4);
    // the wide nodes, as prepare_scene makes them
    Wide& w = T.w;
    auto add = [&] {
        w.slot.push_back({RTG_EXIT, RTG_EXIT, RTG_EXIT, RTG_EXIT});
        w.bin.push_back({0, 0, 0, 0});
        w.box.emplace_back();
        w.n.push_back(0);
        return (int)w.n.size() - 1;
    };
    add();
    std::vector<std::array<int, 3>> work{{0, 0, 1}};  // binary node, wide node, wide level
    while (!work.empty()) {
        const auto [n2, nw, lvl] = work.back();
        work.pop_back();
        w.depth = std::max(w.depth, lvl);
        w.area_sum += area(T.bd, n2) / ra;
        int s[4];
        const int n = wide_cut(lk.data(), T.bd.data(), n2, s);
        w.n[nw] = n;
        ++w.fill[n];
        for (int a = 0; a < 3; ++a) {
            float lo = INFINITY, hi = -INFINITY;
            for (int k = 0; k < n; ++k) {
                lo = std::min(lo, T.bd[(size_t)s[k] * 6 + a]);
                hi = std::max(hi, T.bd[(size_t)s[k] * 6 + 3 + a]);
            }
            const double ext = (double)hi - lo, step = ext > 0 ? std::exp2(std::ceil(std::log2(ext / 255.0))) : 0.0;
            for (int k = 0; k < n; ++k) {
                const float mn = T.bd[(size_t)s[k] * 6 + a], mx = T.bd[(size_t)s[k] * 6 + 3 + a];
                const bool q = quant && step > 0;
                w.box[nw][k * 6 + a] = q ? (float)(lo + std::floor(((double)mn - lo) / step) * step) : mn;
                w.box[nw][k * 6 + 3 + a] = q ? (float)(lo + std::ceil(((double)mx - lo) / step) * step) : mx;
            }
        }
        for (int k = 0; k < n; ++k) {
            w.bin[nw][k] = s[k];
            if (lk[(size_t)s[k] * 4] >= 0) {
                const int id = add();
                w.slot[nw][k] = id;
                work.push_back({s[k], id, lvl + 1});
            } else {
                w.slot[nw][k] = ~s[k];
            }
        }
    }
}

struct Count { double rays = 0, steps = 0, tests = 0, stack = 0, deep = 0; };

// the walk: entries (entry distance, slot word) on a stack, the nearest of a node's hit slots on top
Hit walk(const Tree& T, const float* pos, const Ray& r, bool any, Count& c) {
    struct E { double tn; int w; };
    E st[512];
    int sp = 0, top = 0;
    st[sp++] = {0.0, 0};
    Hit h;
    double steps = 0, tests = 0;
    while (sp > 0) {
        const E e = st[--sp];
        if (e.tn > h.t) continue;
        if (e.w < 0) {
            const int leaf = ~e.w, t = T.lk[(size_t)leaf * 4 + 2];
            ++tests;
            double tt;
            if (tri_test(pos + (size_t)t * 9, r, tt) && (tt < h.t || (tt == h.t && t < h.tri))) {
                h.t = tt;
                h.tri = t;
                if (any) break;
            }
            continue;
        }
        ++steps;
        E hit[4];
        int m = 0;
        for (int k = 0; k < T.w.n[e.w]; ++k) {
            double tn;
            if (box_test(&T.w.box[e.w][k * 6], r, std::min(r.tmax, h.t), tn)) hit[m++] = {tn, T.w.slot[e.w][k]};
        }
        std::sort(hit, hit + m, [](const E& a, const E& b) { return a.tn > b.tn; });  // the farthest first
        for (int k = 0; k < m && sp < 512; ++k) st[sp++] = hit[k];
        top = std::max(top, sp);
    }
    c.rays += 1;
    c.steps += steps;
    c.tests += tests;
    c.stack += top;
    c.deep += top > RTG_STACK;
    return h;
}

Hit brute(const float* pos, uint32_t nt, const Ray& r) {
    Hit h;
    for (uint32_t t = 0; t < nt; ++t) {
        double tt;
        if (tri_test(pos + (size_t)t * 9, r, tt) && tt < h.t) { h.t = tt; h.tri = (int)t; }
    }
    return h;
}

struct Walked { Count closest, any; long mismatch = 0; };

Walked walk_rays(const Tree& T, const rtg_scene_desc* d, int grid, uint64_t seed, bool check) {
    Walked out;
    const float* pos = d->positions;
    const rtg_camera& cam = d->camera;
    std::vector<Ray> rays;
    for (int y = 0; y < grid; ++y)
        for (int x = 0; x < grid; ++x) {  // the pixel centres of a grid x grid film
            const double xp = ((x + 0.5) / grid) * 2.0 - 1.0, yp = (1.0 - (y + 0.5) / grid) * 2.0 - 1.0;
            const float* m = cam.inv_proj;
            const V v{xp * m[0] + yp * m[1] + m[2] + m[3], xp * m[4] + yp * m[5] + m[6] + m[7], xp * m[8] + yp * m[9] + m[10] + m[11]};
            const float* k = cam.camera;
            const V w{v.x * k[0] + v.y * k[1] + v.z * k[2], v.x * k[4] + v.y * k[5] + v.z * k[6], v.x * k[8] + v.y * k[9] + v.z * k[10]};
            rays.push_back({{cam.origin[0], cam.origin[1], cam.origin[2]}, norm(w), INFINITY});
        }
    double scale = 0.0;
    for (int k = 0; k < 6; ++k) scale = std::max(scale, (double)std::fabs(T.bd[k]));
    uint64_t id = 0;
    for (int gen = 0; gen < 3; ++gen) {
        std::vector<Ray> next;
        for (const Ray& r : rays) {
            ++id;
            const Hit h = walk(T, pos, r, false, out.closest);
            if (check) {
                const Hit b = brute(pos, d->n_tris, r);
                out.mismatch += b.t != h.t || b.tri != h.tri;
            }
            if (h.tri < 0 || gen == 2) continue;
            const float* P = pos + (size_t)h.tri * 9;
            const V a{P[0], P[1], P[2]};
            V n = cross(V{P[3], P[4], P[5]} - a, V{P[6], P[7], P[8]} - a);
            if (!(dot(n, n) > 0.0)) continue;
            n = norm(n);
            if (dot(n, r.d) > 0.0) n = n * -1.0;
            const V p = r.o + r.d * h.t;
            // the any-hit ray: a uniform direction of the sphere, unbounded (the environment's)
            const double z = 1.0 - 2.0 * unit(seed, id, 0), ph = 6.283185307179586 * unit(seed, id, 1), s = std::sqrt(std::max(0.0, 1.0 - z * z));
            const V sd{s * std::cos(ph), s * std::sin(ph), z};
            const Ray sr{p + n * ((dot(sd, n) < 0.0 ? -1e-4 : 1e-4) * scale), sd, INFINITY};
            const Hit sh = walk(T, pos, sr, true, out.any);
            if (check) out.mismatch += (sh.tri >= 0) != (brute(pos, d->n_tris, sr).tri >= 0);
            // the continuation ray: cosine-distributed about the normal
            const double u1 = unit(seed, id, 2), u2 = 6.283185307179586 * unit(seed, id, 3), rr = std::sqrt(u1);
            const V t1 = norm(std::fabs(n.x) > 0.5 ? cross(n, V{0, 1, 0}) : cross(n, V{1, 0, 0})), t2 = cross(n, t1);
            const V cd = norm(t1 * (rr * std::cos(u2)) + t2 * (rr * std::sin(u2)) + n * std::sqrt(std::max(0.0, 1.0 - u1)));
            next.push_back({p + n * (1e-4 * scale), cd, INFINITY});
        }
        rays.swap(next);
    }
    return out;
}

std::vector<float> mesh(const std::string& kind) {
    std::vector<float> P;
    auto tri = [&](std::array<float, 9> t) { P.insert(P.end(), t.begin(), t.end()); };
    if (kind == "two") {
        tri({-1, -1, 0, 1, -1, 0, 0, 1, 0});
        tri({-1, -1, 0.5f, 1, -1, 0.5f, 0, 1, 0.25f});
    } else if (kind == "identical3") {
        for (int k = 0; k < 3; ++k) tri({-1, -1, 0, 1, -1, 0, 0, 1, 0});
    } else if (kind == "centroid64") {  // the vertex mean and the box centre of every triangle: the origin
        for (int k = 0; k < 64; ++k) {
            const float s = 0.25f + k / 64.0f, t = 1.25f - k / 64.0f;
            float v[3][3] = {{-s, 0, 0}, {0, -t, 0}, {s, t, 0}};
            std::array<float, 9> o;
            for (int i = 0; i < 3; ++i)
                for (int a = 0; a < 3; ++a) o[i * 3 + (a + k) % 3] = v[i][a];
            tri(o);
        }
    } else if (kind == "chain28") {  // boxes at x = 2^k: a chain-like tree
        for (int k = 0; k < 28; ++k) {
            const float x = std::ldexp(1.0f, k);
            tri({x, -1, -1, x, 1, -1, x, 0, 1});
        }
    }
    return P;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: walk_model <scene dir> | x synth <n> | x mesh <kind> [options]\n"); return 2; }
    SbvhOpt opt;
    opt.passes = 0;
    opt.min_tris = 0;  // (the product runs the pass from RTG_BVH_OPT_MIN_TRIS triangles; here every tree can have it)
    int grid = 192, first_opt = 2;
    uint64_t seed = 1;
    bool check = false, only_opt = false, float_boxes = false;
    std::string dir = argv[1], tmp;
    if (argc > 3 && (std::string(argv[2]) == "synth" || std::string(argv[2]) == "mesh")) {
        tmp = (std::filesystem::temp_directory_path() / ("walk_model_" + std::to_string((long)getpid()))).string();
        int rc;
        if (std::string(argv[2]) == "synth") {
            rc = rth_write_synthetic(tmp.c_str(), (uint32_t)atoi(argv[3]), 20251015, 1024, 1024);
        } else {
            const std::vector<float> P = mesh(argv[3]);
            if (P.empty()) { std::printf("unknown mesh kind %s\n", argv[3]); return 2; }
            rc = rth_write_mesh_scene(tmp.c_str(), P.data(), (uint32_t)(P.size() / 9), 64, 64);
        }
        if (rc) { std::printf("writing the scene failed: %s\n", rth_last_error()); return 2; }
        dir = tmp;
        first_opt = 4;
    }
    for (int i = first_opt; i < argc; ++i) {
        const std::string a = argv[i];
        const char* v = i + 1 < argc ? argv[i + 1] : "0";
        if (a == "--passes") { opt.passes = atoi(v); ++i; }
        else if (a == "--frac") { opt.frac = atof(v); ++i; }
        else if (a == "--priority") { opt.priority = atoi(v); ++i; }
        else if (a == "--grid") { grid = atoi(v); ++i; }
        else if (a == "--seed") { seed = (uint64_t)atoll(v); ++i; }
        else if (a == "--check") check = true;
        else if (a == "--only-opt") only_opt = true;
        else if (a == "--float-boxes") float_boxes = true;
        else if (a == "--stop") { opt.stop = atof(v); ++i; }
        else if (a == "--min-tris") { opt.min_tris = (uint32_t)atoll(v); ++i; }
        else { std::printf("unknown option %s\n", a.c_str()); return 2; }
    }
    rth_load_options o{};
    o.skip_missing = 1;
    rth_scene* s = nullptr;
    const int rc = rth_load_scene(dir.c_str(), &o, &s);
    if (!tmp.empty()) std::filesystem::remove_all(tmp);
    if (rc) { std::printf("load failed: %s\n", rth_last_error()); return 2; }
    const rtg_scene_desc* d = rth_scene_desc(s);
    int bad = 0;
    uint64_t leaf_digest[2] = {0, 0};
    for (int side = only_opt ? 1 : 0; side < (opt.passes > 0 ? 2 : 1); ++side) {
        Tree T;
        SbvhOpt so = opt;
        if (side == 0) so.passes = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (!build_sbvh_opt(d, T.lk, T.bd, so)) { std::printf("build_sbvh failed\n"); return 1; }
        T.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        T.opt_ms = so.ms;
        measure_tree(T, !float_boxes);
        if (!T.order_ok) { std::printf("passes %d: a child's id is not above its parent's\n", so.passes); return 1; }
        const Walked w = walk_rays(T, d, grid, seed, check);
        const Count &c = w.closest, &a = w.any;
        std::printf("tree passes %d tris %u nodes %zu leaves %zu depth %d wide_depth %d sah %.4f wide_area %.4f wide_nodes %zu "
                    "fill %ld %ld %ld %ld build_ms %.0f opt_ms %.0f digest %016llx leaf_digest %016llx | closest rays %.0f "
                    "steps %.3f tests %.3f stack %.2f deep %.5f | any rays %.0f steps %.3f tests %.3f stack %.2f deep %.5f | "
                    "fetches %.3f mismatch %ld\n",
                    so.passes, d->n_tris, T.lk.size() / 4, T.leaves, T.depth, T.w.depth, T.sah, T.w.area_sum, T.w.n.size(),
                    T.w.fill[1], T.w.fill[2], T.w.fill[3], T.w.fill[4], T.build_ms, T.opt_ms, (unsigned long long)T.digest,
                    (unsigned long long)T.leaf_digest, c.rays, c.steps / std::max(1.0, c.rays), c.tests / std::max(1.0, c.rays),
                    c.stack / std::max(1.0, c.rays), c.deep / std::max(1.0, c.rays), a.rays, a.steps / std::max(1.0, a.rays),
                    a.tests / std::max(1.0, a.rays), a.stack / std::max(1.0, a.rays), a.deep / std::max(1.0, a.rays),
                    (c.steps + c.tests + a.steps + a.tests) / std::max(1.0, c.rays + a.rays), check ? w.mismatch : -1L);
        leaf_digest[side] = T.leaf_digest;
        bad += T.depth > 120 || (check && w.mismatch);
    }
    if (opt.passes > 0 && !only_opt && leaf_digest[0] != leaf_digest[1]) {
        std::printf("the optimised tree's leaves differ from the built tree's\n");
        bad = 1;
    }
    rth_free_scene(s);
    return bad ? 1 : 0;
}
