"""TEST INFRASTRUCTURE ONLY — numpy restatement of the Owen-scrambled Sobol sampler of include/rtg.h
(rtg_set_sampler, RTG_SAMPLER_SOBOL): mix32, lk, owen, the direction words from the Joe-Kuo recurrence,
the draw, and SobolStream, which stands where tests/env_sampling_ref.py's PathStream stands for the PCG
mode (raw() / next(), plus new_bounce() for the rounding of the draw counter when a bounce loads it).
All arithmetic is uint32 with wrap-around.
"""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64

CAMERA_STREAM = 0x9E3779B9

# the words as include/rtg.h lists them (tests/test_sampler.py checks the recurrence against them)
D1_HEADER = ("80000000 c0000000 a0000000 f0000000 88000000 cc000000 aa000000 ff000000 "
             "80800000 c0c00000 a0a00000 f0f00000 88880000 cccc0000 aaaa0000 ffff0000")
D2_HEADER = ("80000000 c0000000 60000000 90000000 e8000000 5c000000 8e000000 c5000000 "
             "68800000 9cc00000 ee600000 55900000 80680000 c09c0000 60ee0000 90550000")
D3_HEADER = ("80000000 c0000000 20000000 50000000 f8000000 74000000 a2000000 93000000 "
             "d8800000 25400000 59e00000 e6d00000 78080000 b40c0000 82020000 c3050000")


def _u32(x):
    return np.ascontiguousarray(x).astype(U64).astype(U32) if not isinstance(x, np.ndarray) or x.dtype != U32 else x


def _mul(x, k):
    return ((x.astype(U64) * U64(k)) & U64(0xFFFFFFFF)).astype(U32)


def _add(x, y):
    return ((x.astype(U64) + np.asarray(y).astype(U64)) & U64(0xFFFFFFFF)).astype(U32)


def mix32(x):
    x = np.atleast_1d(_u32(x)).copy()
    x ^= x >> U32(16)
    x = _mul(x, 0x7feb352d)
    x ^= x >> U32(15)
    x = _mul(x, 0x846ca68b)
    x ^= x >> U32(16)
    return x


def lk(x, s):
    x = _add(np.atleast_1d(_u32(x)), np.atleast_1d(_u32(s)))
    for k in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
        x = x ^ _mul(x, k)
    return x


def brev(x):
    x = np.atleast_1d(_u32(x)).copy()
    x = ((x >> U32(1)) & U32(0x55555555)) | ((x & U32(0x55555555)) << U32(1))
    x = ((x >> U32(2)) & U32(0x33333333)) | ((x & U32(0x33333333)) << U32(2))
    x = ((x >> U32(4)) & U32(0x0F0F0F0F)) | ((x & U32(0x0F0F0F0F)) << U32(4))
    x = ((x >> U32(8)) & U32(0x00FF00FF)) | ((x & U32(0x00FF00FF)) << U32(8))
    return (x >> U32(16)) | (x << U32(16))


def owen(x, s):
    return brev(lk(brev(x), s))


def direction_words(degree, a, m, n=16):
    """The first n direction words v_i << (31 - i) of a Joe-Kuo dimension: primitive polynomial of
    `degree` with inner coefficients `a`, initial values m (the standard recurrence)."""
    m = list(m)
    for i in range(degree, n):
        v = m[i - degree] ^ (m[i - degree] << degree)
        for k in range(1, degree):
            if (a >> (degree - 1 - k)) & 1:
                v ^= m[i - k] << k
        m.append(v)
    return np.array([m[i] << (31 - i) for i in range(n)], U64).astype(U32)


def tables():
    """(4, 16) uint32: D_0 (0x80000000 >> b) and the Joe-Kuo words of dimensions 2, 3 and 4."""
    d0 = np.array([0x80000000 >> b for b in range(16)], U64).astype(U32)
    return np.stack([d0, direction_words(1, 0, [1]), direction_words(2, 1, [1, 3]), direction_words(3, 1, [1, 3, 1])])


TABLES = tables()


def sobol(idx, c):
    """sobol_c(idx): the XOR over the set bits b < 16 of idx of D_c[b]; c a scalar or per element."""
    idx = np.atleast_1d(_u32(idx))
    c = np.broadcast_to(np.asarray(c, np.int64), idx.shape)
    x = np.zeros(idx.shape, U32)
    for b in range(16):
        x ^= np.where((idx >> U32(b)) & U32(1), TABLES[c, b], U32(0)).astype(U32)
    return x


def key(pixels, seed, stream=0):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    inner = mix32(np.array([(seed >> 32) ^ stream], U64) & U64(0xFFFFFFFF))
    mid = mix32(U32(seed & 0xFFFFFFFF) ^ inner)
    return mix32(np.atleast_1d(_u32(pixels)) ^ mid)


def draw(k, samples, n):
    """Raw draw n (a scalar or per element) of the paths with keys k and sample numbers `samples`."""
    k = np.atleast_1d(_u32(k))
    n = np.broadcast_to(np.asarray(n, np.int64), k.shape)
    g, c = (n >> 2).astype(U64).astype(U32), n & 3
    gs = mix32(k ^ _mul(g, 0x9E3779B9))
    idx = owen(np.broadcast_to(np.atleast_1d(_u32(samples)), k.shape), gs) & U32(0xFFFF)
    return owen(sobol(idx, c), mix32(_add(gs, _mul((c + 1).astype(U64).astype(U32), 0x85EBCA6B))))


class SobolStream:
    """The draws of paths (pixel, sample) under `seed`: raw() is the 32-bit draw, next() the float draw
    (X >> 8) * 2^-24, both advancing the counter by one; new_bounce() rounds it up to a multiple of 4, as
    the kernels do when a bounce b >= 1 loads it."""

    def __init__(self, pixels, samples, seed, stream=0):
        self.key = key(np.ascontiguousarray(pixels, U32).reshape(-1), seed, stream)
        self.sample = np.ascontiguousarray(samples, U32).reshape(-1)
        self.n = np.zeros(len(self.key), np.int64)

    def raw(self):
        x = draw(self.key, self.sample, self.n)
        self.n = self.n + 1
        return x

    def next(self):
        return (self.raw() >> U32(8)).astype(F) * F(1.0 / 16777216.0)

    def new_bounce(self):
        self.n = (self.n + 3) & ~np.int64(3)
