"""Register budget of the path-tracer MIS kernels (compiled here for gfx950, no GPU needed): rtg_set_path_mis
lives in kernels of its own (k_shade_mis, rtg_shade_mis.hip), which must hold their state in registers at
the six waves per SIMD they are bounded for (DESIGN.md 8f has the table). The twenty existing shading
kernels are pinned by tests/test_materials_resources.py, which compiles the units they live in."""
import pytest

import kernel_meta

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size")
# DESIGN.md 8f, the measured figures as upper bounds: (VGPRs, SGPRs, LDS bytes)
MIS = {
    "_Z11k_shade_misILb1EEv": (75, 98, 20008),
    "_Z11k_shade_misILb0EEv": (76, 106, 8232),
    "_Z18k_probe_mis_weight": (9, 14, 0),
    "_Z15k_probe_env_pdf": (22, 24, 0),
}


@pytest.fixture(scope="module")
def kernels():
    from raytracingrenderer_amd.build import DEVICE_FLAGS
    rel = "device/rtg_shade_mis.hip"
    assert DEVICE_FLAGS[rel] == DEVICE_FLAGS["device/rtg_shade.hip"]
    return kernel_meta.kernels(rel)


def _find(kernels, prefix):
    names = [k for k in kernels if k.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_the_family_is_two_kernels_of_its_own_name(kernels):
    """Two instantiations (TAB), neither counted among k_shade_phys or k_shade_pick, and nothing else in
    the unit but the two probes."""
    assert len(kernels) == len(MIS) and all(len([k for k in kernels if k.startswith(p)]) == 1 for p in MIS), sorted(kernels)
    assert not any("k_shade_phys" in k or "k_shade_pick" in k for k in kernels)


@pytest.mark.parametrize("prefix", sorted(MIS))
def test_new_kernels_hold_their_state_in_registers(kernels, prefix):
    """No scratch, no spilled VGPR, no spilled SGPR, and no larger than measured. The shading kernels take
    at most 80 VGPRs: six waves per SIMD, the launch bound. The LDS of the TAB instantiation is
    k_shade_phys<*, true>'s (the material, light, pick and parameter tables)."""
    vgpr, sgpr, lds = MIS[prefix]
    k = _find(kernels, prefix)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr and k["group_segment_fixed_size"] <= lds, k
    if "k_shade_mis" in prefix:
        assert k["vgpr_count"] <= 80 and k["max_flat_workgroup_size"] == 256, k
    assert MIS["_Z11k_shade_misILb1EEv"][2] == 16168 + 3072 + 768
