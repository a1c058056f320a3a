"""Register budget of the rough dielectric's kernels (compiled here for gfx950, no GPU needed): the family
lives in a unit of its own (rtg_shade_trans.hip) built with rtg_shade.hip's flags, holds its state in
registers at its launch bound of six waves per SIMD, is no larger than DESIGN.md 8g records, and carries
none of the pinned families' names (tests/test_materials_resources.py and tests/test_path_mis_resources.py
count those)."""
import pytest

import kernel_meta

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
    from raytracingrenderer_amd.build import DEVICE_FLAGS
    rel = "device/rtg_shade_trans.hip"
    assert DEVICE_FLAGS[rel] == DEVICE_FLAGS["device/rtg_shade.hip"]
    return kernel_meta.kernels(rel)


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
