"""The compiler's view of the device units, for the *_resources tests (no GPU needed): a unit of build.py's
DEVICE_SRC is compiled to gfx950 assembly with the flags the build gives it (DEVICE_CXXFLAGS + the unit's
DEVICE_FLAGS), once per test session however many tests ask for it.

  asm(rel)           the unit's device assembly, as text
  kernels(rel, ...)  {kernel symbol: its amdhsa.kernels metadata figures (KEYS)} of the units named
"""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "max_flat_workgroup_size")


@functools.lru_cache(maxsize=None)
def asm(rel):
    from raytracingrenderer_amd.build import ARCH, CSRC, DEVICE_CXXFLAGS, DEVICE_FLAGS, DEVICE_SRC, HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    assert rel in DEVICE_SRC, rel
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run([HIPCC, "--offload-arch=" + ARCH] + DEVICE_CXXFLAGS + DEVICE_FLAGS.get(rel, []) +
                           ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, rel)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")
        with open(out) as f:
            return f.read()


@functools.lru_cache(maxsize=None)
def _unit_kernels(rel):
    s = asm(rel)
    res = {}
    for blk in s[s.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in KEYS}
    return res


def kernels(*rels):
    res = {}
    for rel in rels:
        res.update({name: dict(k) for name, k in _unit_kernels(rel).items()})
    return res
