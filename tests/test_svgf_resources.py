"""Register budget of the svgf unit's kernels (compiled here for gfx950, no GPU needed): no kernel of
rtg_svgf.hip may spill or use scratch memory (the three large ones are vector-memory-request loops: a scratch
reload per tap would be one more), none uses LDS, and every one keeps 8 waves per SIMD."""
import pytest

import kernel_meta


@pytest.fixture(scope="module")
def kernels():
    res = kernel_meta.kernels("device/rtg_svgf.hip")
    print(res)
    return res


def test_every_svgf_kernel_is_found(kernels):
    for want in ("k_svgf_temporal", "k_svgf_variance", "k_svgf_pack_pos", "k_svgf_atrous", "k_svgf_unpack"):
        assert any(want in name for name in kernels), (want, sorted(kernels))
    assert len(kernels) == 5, sorted(kernels)


def test_no_svgf_kernel_spills(kernels):
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)


def test_every_svgf_kernel_keeps_full_occupancy(kernels):
    """What the build achieves (DESIGN.md 8j's table): k_svgf_atrous 61 VGPRs / 52 SGPRs, k_svgf_temporal 48 /
    62, k_svgf_variance 47 / 54, the two copies 6-7 / 12. 8 waves per SIMD need <= 64 VGPRs (512 / 8) and, for
    8 blocks of 256 threads per CU, <= 80 SGPRs."""
    for name, k in kernels.items():
        assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 80, (name, k)
