"""Register budget of the temporal unit's kernels (compiled here for gfx950, no GPU needed): neither
kernel of rtg_temporal.hip may spill or use scratch memory (k_temporal is all vector-memory requests: a
scratch reload per tap would be one more), and neither uses LDS."""
import pytest

import kernel_meta


@pytest.fixture(scope="module")
def kernels():
    res = kernel_meta.kernels("device/rtg_temporal.hip")
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
