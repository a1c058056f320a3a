"""Register budget of the fused first-hit unit (compiled here for gfx950, no GPU needed): rtg_gbuffer.hip is
part of the build and holds k_gbuffer alone; it may not spill, use scratch memory or LDS, and keeps at least the
6 waves per SIMD of the project's shading kernels (<= 80 VGPRs)."""
import pytest

import kernel_meta
from raytracingrenderer_amd.build import DEVICE_FLAGS, DEVICE_SRC

UNIT = "device/rtg_gbuffer.hip"


@pytest.fixture(scope="module")
def kernels():
    assert UNIT in DEVICE_SRC
    res = kernel_meta.kernels(UNIT)
    print(res)
    return res


def test_the_unit_is_built_like_the_units_it_shares_headers_with():
    assert UNIT in DEVICE_SRC
    assert DEVICE_FLAGS[UNIT] == ["-fno-slp-vectorize"]


def test_the_unit_holds_k_gbuffer_alone(kernels):
    assert len(kernels) == 1 and "k_gbuffer" in next(iter(kernels)), sorted(kernels)


def test_k_gbuffer_does_not_spill(kernels):
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)


def test_k_gbuffer_keeps_its_occupancy(kernels):
    """What the build achieves (DESIGN.md 8k's table): k_gbuffer 41 VGPRs / 32 SGPRs. The floor is the shading
    kernels' 6 waves per SIMD (<= 80 VGPRs); the build keeps 8, which need <= 64 VGPRs (512 / 8) and, for 8
    blocks of 256 threads per CU, <= 80 SGPRs."""
    for name, k in kernels.items():
        assert k["vgpr_count"] <= 80, (name, k)
        assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 80, (name, k)
