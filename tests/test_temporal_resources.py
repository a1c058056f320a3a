"""Register budget of the temporal unit's kernels (compiled here for gfx950, no GPU needed): neither
kernel of rtg_temporal.hip may spill or use scratch memory (k_temporal is all vector-memory requests: a
scratch reload per tap would be one more), and neither uses LDS."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "raytracingrenderer_amd", "csrc", "device")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNIT = "device/rtg_temporal.hip"


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    from raytracingrenderer_amd.build import DEVICE_FLAGS, DEVICE_SRC  # the unit with the flags the build uses
    assert UNIT in DEVICE_SRC
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"] +
                       DEVICE_FLAGS.get(UNIT, []) + ["--cuda-device-only", "-S", "-o", out,
                                                     os.path.join(DEVICE, os.path.basename(UNIT))],
                       check=True, capture_output=True)
        s = open(out).read()
    res = {}
    md = s[s.index("amdhsa.kernels"):]
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count",
                               "private_segment_fixed_size", "group_segment_fixed_size")}
    print(res)
    return res


def test_every_temporal_kernel_is_found(kernels):
    for want in ("k_geometry_guide", "k_temporal"):
        assert any(want in name for name in kernels), (want, sorted(kernels))


def test_no_temporal_kernel_spills(kernels):
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)


def test_temporal_kernel_keeps_full_occupancy(kernels):
    """k_temporal hides its tap loads behind other waves: 8 waves per SIMD need <= 64 VGPRs (512 / 8)
    and <= 96 SGPRs."""
    k = [v for n, v in kernels.items() if "k_temporal" in n][0]
    assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 96, k
