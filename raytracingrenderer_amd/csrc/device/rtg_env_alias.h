// rtg_env_alias.h — the alias table of rtg_set_env_sampling(.., RTG_ENV_LUMINANCE), built on the host
// from the cell weights (include/rtg.h has the definition). Plain C++, no HIP types: rtg_env.hip builds
// the handle's table with it and rtg_env_alias_build exposes it to the CPU tests.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace rtg_env {

// (The caller supplies the cell weights, w = (double)maxlum * sin(pi (cy + 0.5) / H): build_env_table.)
struct Alias {
    double sum = 0.0;               // the weights added in index order
    std::vector<double> prob;       // Vose's keep probability per entry, in [0, 1]
    std::vector<uint32_t> alias;    // the other cell of the entry (itself when prob == 1)
    std::vector<float> cellpdf;     // (float)(((w / sum) * n) / ((2.0 * pi) * pi)) per cell
};

// Vose's algorithm in double, in a fixed order, on scaled probabilities p (p_k = probability_k * n;
// consumed): cells are put on the "small" (p < 1) or "large" stack in ascending index order; while both
// hold cells, the top small cell s takes prob p[s] and the top large cell l as its alias,
// p[l] = (p[l] + p[s]) - 1.0, and l goes back on the stack its new p belongs to. What remains keeps
// itself (prob 1). A zero weight (w: the values p was scaled from) gives p = 0 exactly, hence prob 0.
// Fills out.prob and out.alias. (rtg_light_pick.hip runs it on p_k = pmf_k * n.)
static inline void vose(std::vector<double>& p, const double* w, uint32_t n, Alias& out) {
    out.prob.assign(n, 1.0);
    out.alias.resize(n);
    std::vector<uint32_t> small, large;
    small.reserve(n);
    large.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        out.alias[i] = i;
        (p[i] < 1.0 ? small : large).push_back(i);
    }
    while (!small.empty() && !large.empty()) {
        const uint32_t s = small.back(), l = large.back();
        small.pop_back();
        large.pop_back();
        out.prob[s] = p[s];
        out.alias[s] = l;
        p[l] = (p[l] + p[s]) - 1.0;
        (p[l] < 1.0 ? small : large).push_back(l);
    }
    // left on the small stack by rounding alone (p within a few ulp of 1), or with a zero weight when
    // no large cell is left (not reachable with sum > 0): a zero-weight cell keeps prob 0 regardless
    for (uint32_t s : small) out.prob[s] = (w[s] > 0.0) ? 1.0 : 0.0;
}

// The environment table: cells are scaled to p = (w / sum) * n, then vose(). sum == 0 (nothing to
// sample): returns false.
static inline bool build_alias(const double* w, uint32_t n, Alias& out) {
    const double pi = 3.14159265358979323846;
    out.prob.assign(n, 1.0);
    out.alias.resize(n);
    out.cellpdf.resize(n);
    double sum = 0.0;
    for (uint32_t i = 0; i < n; ++i) sum += w[i];
    out.sum = sum;
    if (!(sum > 0.0) || !(sum <= 1.7976931348623157e308)) return false;
    std::vector<double> p(n);
    for (uint32_t i = 0; i < n; ++i) {
        p[i] = (w[i] / sum) * (double)n;
        out.cellpdf[i] = (float)(p[i] / ((2.0 * pi) * pi));
    }
    vose(p, w, n, out);
    return true;
}

// The 16-byte entries the kernel loads: {(float)prob, alias, cellpdf of the cell, cellpdf of the alias}.
// Rounding prob to float32 moves a cell's sampled mass by at most 2^-25 / n per entry that names it.
static inline void pack_entries(const Alias& a, uint32_t* entries /* n * 4 */) {
    const uint32_t n = (uint32_t)a.prob.size();
    for (uint32_t i = 0; i < n; ++i) {
        const float pf = (float)a.prob[i];
        const float cs = a.cellpdf[i], ca = a.cellpdf[a.alias[i]];
        uint32_t* e = entries + 4 * (size_t)i;
        std::memcpy(e + 0, &pf, 4);
        e[1] = a.alias[i];
        std::memcpy(e + 2, &cs, 4);
        std::memcpy(e + 3, &ca, 4);
    }
}

}  // namespace rtg_env
