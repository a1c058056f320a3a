"""Register budget of the rough dielectric's kernels (compiled here for gfx950, no GPU needed): the family
lives in a unit of its own (rtg_shade_trans.hip) built with rtg_shade.hip's flags, holds its state in
registers at its launch bound of six waves per SIMD, is no larger than DESIGN.md 8g records, and carries
none of the pinned families' names (tests/test_materials_resources.py and tests/test_path_mis_resources.py
count those)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "raytracingrenderer_amd", "csrc", "device")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size")
# DESIGN.md 8g, the measured figures as upper bounds: (VGPRs, SGPRs, LDS bytes)
TRANS = {
    "_Z13k_shade_transILb0ELb0EEv": (80, 104, 8232),
    "_Z13k_shade_transILb0ELb1EEv": (79, 98, 20008),
    "_Z13k_shade_transILb1ELb0EEv": (72, 104, 8232),
    "_Z13k_shade_transILb1ELb1EEv": (73, 98, 20008),
    "_Z17k_shade_trans_misILb0EEv": (80, 106, 8232),
    "_Z17k_shade_trans_misILb1EEv": (80, 98, 20008),
    "_Z20k_probe_transmissionPKfiPf": (62, 37, 0),
}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    from raytracingrenderer_amd.build import DEVICE_CXXFLAGS, DEVICE_FLAGS, DEVICE_SRC
    rel = "device/rtg_shade_trans.hip"
    assert rel in DEVICE_SRC
    assert DEVICE_FLAGS[rel] == DEVICE_FLAGS["device/rtg_shade.hip"]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rtg_shade_trans.s")
        flags = [f for f in DEVICE_CXXFLAGS if f != "-fPIC"]
        r = subprocess.run([HIPCC, "--offload-arch=gfx950"] + flags + DEVICE_FLAGS[rel] +
                           ["--cuda-device-only", "-S", "-o", out, os.path.join(DEVICE, os.path.basename(rel))],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")
        s = open(out).read()
    res = {}
    md = s[s.index("amdhsa.kernels"):]
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in KEYS}
        res[name]["max_flat_workgroup_size"] = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk).group(1))
    return res


def test_the_unit_holds_the_family_and_its_probe(kernels):
    assert len(kernels) == 7, sorted(kernels)
    for prefix in TRANS:
        assert sum(k.startswith(prefix) for k in kernels) == 1, prefix
    for name in kernels:
        assert not any(pinned in name for pinned in ("k_shade_phys", "k_shade_pick", "k_shade_mis")), name


def test_kernels_hold_their_state_in_registers(kernels):
    """No scratch, no spilled VGPR or SGPR, no larger than measured; the shading kernels at most 80 VGPRs:
    six waves per SIMD, their launch bound (at seven, every instantiation but one spills)."""
    for prefix, (vgpr, sgpr, lds) in TRANS.items():
        k = [v for n, v in kernels.items() if n.startswith(prefix)][0]
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (prefix, k)
        assert k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr and k["group_segment_fixed_size"] <= lds, (prefix, k)
        if "k_shade_trans" in prefix:
            assert k["vgpr_count"] <= 80 and k["max_flat_workgroup_size"] == 256, (prefix, k)
    # the TAB instantiations' LDS is k_shade_phys's: the parameter and pick tables beside k_shade's
    assert TRANS["_Z13k_shade_transILb0ELb1EEv"][2] == 16168 + 3072 + 768
