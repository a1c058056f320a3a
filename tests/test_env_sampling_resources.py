"""Register budget around the environment-sampling kernels (compiled here for gfx950, no GPU needed):
RTG_ENV_LUMINANCE lives in kernels of its own (k_shade_env, rtg_shade.hip), so the default's k_shade
instantiations must come out of the compiler as they did before it existed, and the new kernels (and
rtg_env.hip's) must hold their state in registers."""
import pytest

import kernel_meta

# The figures of the commit before k_shade_env, same flags: (VGPRs, SGPRs, LDS bytes,
# spilled VGPRs). k_shade<true, *> spilled then as it does now; it is pinned so that it gets no worse.
BEFORE = {
    "_Z7k_shadeILb0ELb1E": (64, 88, 16168, 0),
    "_Z7k_shadeILb0ELb0E": (62, 87, 8232, 0),
    "_Z7k_shadeILb1ELb1E": (72, 94, 16168, 60),
    "_Z7k_shadeILb1ELb0E": (72, 94, 8232, 46),
}


@pytest.fixture(scope="module")
def kernels():
    return kernel_meta.kernels("device/rtg_shade.hip", "device/rtg_env.hip")


def _find(kernels, prefix):
    names = [k for k in kernels if k.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_new_kernels_do_not_spill(kernels):
    """The four k_shade_env instantiations and rtg_env.hip's kernels: no spilled VGPR, no scratch.
    k_shade_env<false, *> (pathTrace) keeps k_shade<false, *>'s 7 waves per SIMD (<= 72 VGPRs)."""
    new = [k for k in kernels if "k_shade_env" in k or "k_env_weights" in k or "k_probe_env" in k]
    assert len([k for k in new if "k_shade_env" in k]) == 4 and len(new) == 6, new
    for name in new:
        k = kernels[name]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    for tab in ("Lb0E", "Lb1E"):
        k = _find(kernels, "_Z11k_shade_envILb0E" + tab)
        assert k["vgpr_count"] <= 72 and k["sgpr_count"] <= 96, k


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_k_shade_is_no_larger_than_before(kernels, name):
    k = _find(kernels, name + "Ev")
    v, s, lds, spilled = BEFORE[name]
    assert k["vgpr_count"] <= v and k["sgpr_count"] <= s and k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_spill_count"] <= spilled, k
    if spilled == 0:
        assert k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
