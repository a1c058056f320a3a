// rtg_sampler.h — rtg_set_sampler(.., RTG_SAMPLER_SOBOL) (include/rtg.h has the normative definition):
// Burley's hash-based Owen-scrambled Sobol sequence (JCGT 2020), padded 4-D. Draw n of (pixel, sample)
// is component n & 3 of the 4-D point of group n >> 2, indexed by the sample number, shuffled and
// scrambled with hash seeds of the group's own. uint32 arithmetic with wrap-around; the tables are
// compile-time constants (no memory loads), __brev is v_bfrev_b32. The shading kernels' Sobol
// variants, k_sobol_generate_sampled and k_probe_sampler share sobol_draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef RTG_D
#define RTG_D __device__ __forceinline__
#endif

namespace rtgd {

#define RTG_SOBOL_CAMERA_STREAM 0x9E3779B9u  // the camera sample's stream (the path's: 0)

RTG_D uint32_t sobol_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// the Laine-Karras permutation on the reversed word; sobol_owen is the nested uniform scramble
RTG_D uint32_t sobol_lk(uint32_t x, uint32_t s) {
    x += s;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return x;
}
RTG_D uint32_t sobol_owen(uint32_t x, uint32_t s) { return __brev(sobol_lk(__brev(x), s)); }

RTG_D uint32_t sobol_key(uint32_t pixel, uint64_t seed, uint32_t stream) {
    return sobol_mix32(pixel ^ sobol_mix32((uint32_t)seed ^ sobol_mix32((uint32_t)(seed >> 32) ^ stream)));
}

// Joe-Kuo direction words of dimensions 2, 3 and 4 (component 0's are 0x80000000 >> b: a bit reversal)
struct SobolWords { uint32_t w[16]; };
constexpr SobolWords SOBOL_D1 = {{0x80000000u, 0xc0000000u, 0xa0000000u, 0xf0000000u, 0x88000000u, 0xcc000000u,
                                  0xaa000000u, 0xff000000u, 0x80800000u, 0xc0c00000u, 0xa0a00000u, 0xf0f00000u,
                                  0x88880000u, 0xcccc0000u, 0xaaaa0000u, 0xffff0000u}};
constexpr SobolWords SOBOL_D2 = {{0x80000000u, 0xc0000000u, 0x60000000u, 0x90000000u, 0xe8000000u, 0x5c000000u,
                                  0x8e000000u, 0xc5000000u, 0x68800000u, 0x9cc00000u, 0xee600000u, 0x55900000u,
                                  0x80680000u, 0xc09c0000u, 0x60ee0000u, 0x90550000u}};
constexpr SobolWords SOBOL_D3 = {{0x80000000u, 0xc0000000u, 0x20000000u, 0x50000000u, 0xf8000000u, 0x74000000u,
                                  0xa2000000u, 0x93000000u, 0xd8800000u, 0x25400000u, 0x59e00000u, 0xe6d00000u,
                                  0x78080000u, 0xb40c0000u, 0x82020000u, 0xc3050000u}};
constexpr uint32_t sobol_brev_c(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
// brev(sobol_c(idx)): the XOR of the reversed words of idx's set bits (owen() reverses its argument
// first, so the reversal is folded into the constants; bit b's word is a literal operand)
template <int C, int B = 15>
RTG_D uint32_t sobol_xor_rev(uint32_t idx) {
    constexpr uint32_t word = sobol_brev_c((C == 1 ? SOBOL_D1 : C == 2 ? SOBOL_D2 : SOBOL_D3).w[B]);
    const uint32_t t = (0u - ((idx >> B) & 1u)) & word;
    if constexpr (B == 0) return t;
    else return t ^ sobol_xor_rev<C, B - 1>(idx);
}

// the raw 32-bit draw n of (key, sample)
RTG_D uint32_t sobol_draw(uint32_t key, uint32_t sample, uint32_t n) {
    const uint32_t g = n >> 2, c = n & 3u;
    const uint32_t gs = sobol_mix32(key ^ (g * 0x9E3779B9u));
    const uint32_t idx = sobol_owen(sample, gs) & 0xFFFFu;
    uint32_t r;  // brev(sobol_c(idx))
    if (c == 0u) r = idx;
    else if (c == 1u) r = sobol_xor_rev<1>(idx);
    else if (c == 2u) r = sobol_xor_rev<2>(idx);
    else r = sobol_xor_rev<3>(idx);
    return __brev(sobol_lk(r, sobol_mix32(gs + (c + 1u) * 0x85EBCA6Bu)));
}

// The path's sampler state in the shading body's two 64-bit words: st, the draw counter in the low 32
// bits of the payload's rng word; inc = key | sample << 32 (recomputed per bounce, as the PCG increment)
RTG_D uint64_t sobol_inc(uint32_t pixel, uint32_t sample, uint64_t seed) {
    return (uint64_t)sobol_key(pixel, seed, 0u) | ((uint64_t)sample << 32);
}
RTG_D uint64_t sobol_load(uint64_t rng) { return (uint64_t)(((uint32_t)rng + 3u) & ~3u); }  // a bounce opens a point
RTG_D uint32_t sobol_step(uint64_t& s, uint64_t inc) {
    const uint32_t n = (uint32_t)s;
    s = (uint64_t)(n + 1u);
    return sobol_draw((uint32_t)inc, (uint32_t)(inc >> 32), n);
}
RTG_D float sobol_next(uint64_t& s, uint64_t inc) {
    return (float)(sobol_step(s, inc) >> 8) * (1.0f / 16777216.0f);
}
struct SobolSampler {
    uint64_t s;
    uint64_t inc;
    RTG_D float next() { return sobol_next(s, inc); }
};

}  // namespace rtgd
