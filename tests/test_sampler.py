"""The Owen-scrambled Sobol sampler (rtg_set_sampler, RTG_SAMPLER_SOBOL) on the CPU: the numpy restatement
of include/rtg.h's definition (tests/sobol_ref.py) against the header's tables and check values, against
torch's unscrambled Sobol engine, and against the properties the mode is there for (every aligned block of
2^m consecutive samples of a pixel is a (0, m, 2)-net in the first two components of a group, and
stratified in each component alone); and the argument checks that need no device."""
import os
import subprocess

import numpy as np
import pytest

import sobol_ref as sr
from conftest import SCENES

U32 = np.uint32


def test_recurrence_gives_the_headers_words():
    """The Joe-Kuo recurrence (degree / a / m = 1/0/(1), 2/1/(1,3), 3/1/(1,3,1)) reproduces the 3 x 16 words
    include/rtg.h lists, and the header lists what this file's copy says."""
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "rtg.h")).read()
    flat = " ".join(hdr.replace("*", " ").split())
    for c, words in ((1, sr.D1_HEADER), (2, sr.D2_HEADER), (3, sr.D3_HEADER)):
        assert ["%08x" % int(v) for v in sr.TABLES[c]] == words.split(), c
        assert "D_%d = %s" % (c, words) in flat, c
    assert [int(v) for v in sr.TABLES[0]] == [0x80000000 >> b for b in range(16)]


def test_tables_equal_torchs_sobol_engine_in_gray_code_order():
    """torch.quasirandom.SobolEngine(4, scramble=False) walks the sequence in Gray-code order: its point i
    is index i ^ (i >> 1) here, value * 2^32, over 1024 points and all four components."""
    torch = pytest.importorskip("torch")
    pts = torch.quasirandom.SobolEngine(4, scramble=False).draw(1024, dtype=torch.float64).numpy()
    i = np.arange(1024, dtype=np.uint32)
    gray = i ^ (i >> U32(1))
    for c in range(4):
        want = np.round(pts[:, c] * 2.0 ** 32).astype(np.uint64).astype(U32)
        assert np.array_equal(sr.sobol(gray, c), want), c


CHECK = {0: "f71b8747 4afdb22b 34d9b6cd 902fcf82 73c1d462",
         1: "85be176b 788797ea e4b6ff25 269995b0 9ef285ce",
         2: "3945034a fa4b272f 469d293c b73d6981 288746e5",
         3: "6243e999 9c2575a8 0b7d3887 d37ce5ad 5010ac28"}


def test_check_values():
    """mix32(5) and, with key = mix32(5) and g = 0, the draws of samples 0, 1, 2, 3 and 65535."""
    assert int(sr.mix32(5)[0]) == 0x5c45d53e
    k = sr.mix32(5)
    for c, row in CHECK.items():
        got = ["%08x" % int(sr.draw(k, [s], c)[0]) for s in (0, 1, 2, 3, 65535)]
        assert got == row.split(), (c, got)
    # the stream: draws in order, the float conversion, and the rounding of the counter at a bounce
    st = sr.SobolStream([0], [3], 0)
    st.key = k
    assert int(st.raw()[0]) == 0x902fcf82
    assert st.next()[0] == np.float32(0x269995) * np.float32(2.0 ** -24)
    st.new_bounce()
    assert st.n[0] == 4
    st.new_bounce()
    assert st.n[0] == 4


@pytest.fixture(scope="module")
def keyed_points():
    """(100 keys, 4096 samples, 4 components) raw draws of group 0."""
    keys = sr.key(np.arange(100, dtype=U32) * U32(7919), 1234)
    smp = np.arange(4096, dtype=U32)
    k = np.repeat(keys, len(smp))
    s = np.tile(smp, len(keys))
    return np.stack([sr.draw(k, s, c).reshape(100, 4096) for c in range(4)], axis=2)


def blocks(m):
    n = 1 << m
    return [np.arange(start, start + n) for start in (0, n, 3 * n)]


@pytest.mark.parametrize("m", range(1, 11))
def test_aligned_blocks_are_nets_in_the_first_two_components(keyed_points, m):
    """Blocks of 2^m consecutive samples starting at 0, n and 3n: exactly one point in every elementary
    interval 2^-a x 2^-(m - a), a = 0..m, of components (0, 1), for every key."""
    for blk in blocks(m):
        x = keyed_points[:, blk, 0].astype(np.uint64)
        y = keyed_points[:, blk, 1].astype(np.uint64)
        for a in range(m + 1):
            # (uint64 words: a shift by 32 leaves 0, the one interval of that axis)
            cell = ((x >> np.uint64(32 - a)) << np.uint64(m - a)) | (y >> np.uint64(32 - (m - a)))
            assert (np.sort(cell, axis=1) == np.arange(1 << m, dtype=np.uint64)).all(), (m, a, int(blk[0]))


@pytest.mark.parametrize("m", range(1, 11))
def test_every_component_alone_is_stratified(keyed_points, m):
    for blk in blocks(m):
        for c in range(4):
            cell = keyed_points[:, blk, c].astype(np.uint64) >> np.uint64(32 - m)
            assert (np.sort(cell, axis=1) == np.arange(1 << m, dtype=np.uint64)).all(), (m, c, int(blk[0]))


def test_the_shuffled_index_is_a_bijection():
    """idx = owen(sample, gs) & 0xFFFF over samples 0..65535 takes every value once, for several group seeds."""
    smp = np.arange(65536, dtype=U32)
    for gs in (0, 1, 0x5c45d53e, 0xFFFFFFFF, 0x9E3779B9):
        idx = sr.owen(smp, np.full(65536, gs, U32)) & U32(0xFFFF)
        assert np.array_equal(np.sort(idx), smp), hex(gs)


def test_setter_argument_check_without_a_device():
    """rtg_sampler_check (rtg_set_sampler's argument check alone): pcg and sobol pass, anything else is
    RTG_ERR_ARG; an unknown name never reaches the library; a null handle is an argument error too."""
    from raytracingrenderer_amd import NativeError
    from raytracingrenderer_amd import _native as N
    from raytracingrenderer_amd.renderer import SAMPLERS, sampler_check
    assert SAMPLERS == {"pcg": N.RTG_SAMPLER_PCG, "sobol": N.RTG_SAMPLER_SOBOL} == {"pcg": 0, "sobol": 1}
    for ok in ("pcg", "sobol", 0, 1):
        sampler_check(ok)
    for bad in (2, -1, 99):
        with pytest.raises(NativeError):
            sampler_check(bad)
    assert b"rtg_set_sampler" in N.rtg().rtg_last_error()
    with pytest.raises(ValueError):
        sampler_check("halton")
    assert N.rtg().rtg_set_sampler(None, 7) != 0 and N.rtg().rtg_group_set_sampler(None, 1) != 0


def test_cli_rejects_an_unknown_sampler(tmp_path):
    """-sampler halton is an error that names the option, reported before any device is opened."""
    from raytracingrenderer_amd import _native as N
    cli = os.path.join(os.path.dirname(N.__file__), "lib", "rtg_render")
    r = subprocess.run([cli, "-scene", os.path.join(SCENES, "cornell-box"), "-SPP", "1", "-timeLimit", "0", "-width", "16",
                        "-height", "16", "-sampler", "halton"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-sampler" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "GI.hdr")
