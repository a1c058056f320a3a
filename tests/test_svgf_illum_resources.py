"""Register budget of the illumination unit's two kernels (compiled here for gfx950, no GPU needed): the unit is
part of the build, holds the kernels DESIGN.md 8n's table names and no others, and neither spills, uses scratch
memory or LDS, or falls below 8 waves per SIMD."""
import pytest

import kernel_meta

UNIT = "device/rtg_svgf_illum.hip"


@pytest.fixture(scope="module")
def kernels():
    res = kernel_meta.kernels(UNIT)
    print(res)
    return res


def test_the_unit_is_built_with_the_svgf_unit_s_flags():
    from raytracingrenderer_amd.build import DEVICE_FLAGS, DEVICE_SRC
    assert UNIT in DEVICE_SRC
    assert DEVICE_FLAGS.get(UNIT, []) == DEVICE_FLAGS.get("device/rtg_svgf.hip", [])


def test_the_unit_holds_its_two_kernels_and_no_others(kernels):
    for want in ("k_svgf_illum_prepare", "k_svgf_illum_unpack"):
        assert any(want in name for name in kernels), (want, sorted(kernels))
    assert len(kernels) == 2, sorted(kernels)  # the chain's kernels are rtg_svgf.hip's own, not copies


def test_neither_kernel_spills(kernels):
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)


def test_both_kernels_keep_full_occupancy(kernels):
    """8 waves per SIMD need <= 64 VGPRs (512 / 8) and, for 8 blocks of 256 threads per CU, <= 80 SGPRs."""
    for name, k in kernels.items():
        assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 80, (name, k)
