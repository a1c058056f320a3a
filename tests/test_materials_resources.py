"""Register budget around the material-model kernels (compiled here for gfx950, no GPU needed):
RTG_MATERIALS_PHYSICAL lives in kernels of its own (k_shade_phys, rtg_shade_phys.hip), so the sixteen
existing k_shade / k_shade_env / k_shade_pick instantiations must be no larger than DESIGN.md 8c / 8d
record them, and the new kernels must hold their state in registers (DESIGN.md 8e has the table)."""
import pytest

import kernel_meta

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size")
# (VGPRs, SGPRs, LDS bytes, spilled VGPRs, spilled SGPRs, scratch bytes)
EXISTING = {
    "_Z7k_shadeILb0ELb1EEv": (64, 88, 16168, 0, 0, 0),
    "_Z7k_shadeILb0ELb0EEv": (62, 87, 8232, 0, 0, 0),
    "_Z7k_shadeILb1ELb1EEv": (72, 94, 16168, 60, 6, 128),
    "_Z7k_shadeILb1ELb0EEv": (72, 94, 8232, 46, 20, 128),
    "_Z11k_shade_envILb0ELb1EEv": (64, 92, 16168, 0, 0, 0),
    "_Z11k_shade_envILb0ELb0EEv": (64, 91, 8232, 0, 0, 0),
    "_Z11k_shade_envILb1ELb1EEv": (108, 106, 16168, 0, 0, 0),
    "_Z11k_shade_envILb1ELb0EEv": (108, 106, 8232, 0, 4, 0),
    "_Z12k_shade_pickILb0ELb0ELb0EEv": (62, 85, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb0ELb1EEv": (62, 85, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb1ELb0EEv": (64, 84, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb1ELb1EEv": (64, 88, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb0ELb0EEv": (105, 104, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb0ELb1EEv": (108, 106, 8232, 0, 2, 0),
    "_Z12k_shade_pickILb1ELb1ELb0EEv": (106, 100, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb1ELb1EEv": (109, 106, 16936, 0, 0, 0),
}
# DESIGN.md 8e, the measured figures as upper bounds: <ALT, TAB> -> (VGPRs, SGPRs, LDS bytes)
PHYS = {
    "_Z12k_shade_physILb0ELb0EEv": (73, 104, 8232),
    "_Z12k_shade_physILb0ELb1EEv": (72, 98, 20008),
    "_Z12k_shade_physILb1ELb0EEv": (69, 104, 8232),
    "_Z12k_shade_physILb1ELb1EEv": (70, 98, 20008),
    "_Z16k_probe_materialPKfiPf": (83, 44, 0),
}


@pytest.fixture(scope="module")
def kernels():
    from raytracingrenderer_amd.build import DEVICE_FLAGS
    assert DEVICE_FLAGS["device/rtg_shade_phys.hip"] == DEVICE_FLAGS["device/rtg_shade.hip"]
    return kernel_meta.kernels("device/rtg_shade.hip", "device/rtg_light_pick.hip", "device/rtg_shade_phys.hip")


def _find(kernels, prefix):
    names = [k for k in kernels if k.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_new_kernels_hold_their_state_in_registers(kernels):
    """The four k_shade_phys instantiations and the probe: no scratch, no spilled VGPR, no spilled SGPR, and
    no larger than measured. At most 80 VGPRs: six waves per SIMD (the launch bound); the LDS copy of the
    parameter table and of the pick table cost the TAB instantiations 3,072 + 768 bytes."""
    phys = [k for k in kernels if "k_shade_phys" in k]
    assert len(phys) == 4 and not any("k_shade_pick" in k for k in phys), phys
    assert sum("k_shade_pick" in k for k in kernels) == 8
    for prefix, (vgpr, sgpr, lds) in PHYS.items():
        k = _find(kernels, prefix)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (prefix, k)
        assert k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr and k["group_segment_fixed_size"] <= lds, (prefix, k)
        if "k_shade_phys" in prefix:
            assert k["vgpr_count"] <= 80, (prefix, k)
    assert PHYS["_Z12k_shade_physILb0ELb1EEv"][2] == 16168 + 3072 + 768


@pytest.mark.parametrize("name", sorted(EXISTING))
def test_existing_shading_kernels_are_no_larger_than_recorded(kernels, name):
    k = _find(kernels, name)
    for key, before in zip(KEYS, EXISTING[name]):
        assert k[key] <= before, (key, k)
