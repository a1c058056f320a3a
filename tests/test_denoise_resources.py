"""Register budget of the denoiser's kernels (compiled here for gfx950, no GPU needed): none of the
kernels of rtg_denoise.hip may spill or use scratch memory (a scratch reload per tap is a vector-
memory request in a loop that is all vector-memory requests)."""
import pytest

import kernel_meta


@pytest.fixture(scope="module")
def kernels():
    return kernel_meta.kernels("device/rtg_denoise.hip")


def test_every_denoise_kernel_is_found(kernels):
    for want in ("k_dn_pack_colour", "k_dn_pack_guide", "k_dn_atrous", "k_dn_unpack"):
        assert any(want in name for name in kernels), (want, sorted(kernels))


def test_no_denoise_kernel_spills(kernels):
    for name, k in kernels.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


def test_atrous_kernel_keeps_full_occupancy(kernels):
    """The direct-read a-trous kernel hides its tap loads behind other waves: 8 waves per SIMD need
    <= 64 VGPRs (512 / 8) and <= 96 SGPRs; it uses no LDS."""
    k = [v for n, v in kernels.items() if "k_dn_atrous" in n and "lds" not in n][0]
    assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 96 and k["group_segment_fixed_size"] == 0, k
