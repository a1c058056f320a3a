"""Register budget of the light-grid kernels (compiled here for gfx950, no GPU needed): rtg_set_light_grid
lives in kernels of its own (k_shade_grid, rtg_light_grid.hip), each the counterpart of a k_shade_pick
instantiation (rtg_light_pick.hip). A grid kernel must hold its state in registers and reach at least its
counterpart's waves per SIMD (DESIGN.md §8l has the table)."""
import pytest

import kernel_meta


@pytest.fixture(scope="module")
def kernels():
    from raytracingrenderer_amd.build import DEVICE_FLAGS
    assert DEVICE_FLAGS["device/rtg_light_grid.hip"] == DEVICE_FLAGS["device/rtg_shade.hip"]
    return kernel_meta.kernels("device/rtg_light_grid.hip", "device/rtg_light_pick.hip")


def waves_per_simd(k):
    """Waves of this kernel a gfx950 SIMD holds by its registers: 512 VGPRs per lane in blocks of 8, at most
    8 waves, and the eighth only at 80 SGPRs or fewer ("Seven waves per SIMD")."""
    v = (k["vgpr_count"] + 7) // 8 * 8
    return min(8 if k["sgpr_count"] <= 80 else 7, 512 // v)


def _find(kernels, prefix):
    names = [k for k in kernels if k.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_grid_kernels_hold_their_state_in_registers(kernels):
    """The eight k_shade_grid instantiations and the probe: no spilled VGPR and no scratch. The path tracer's
    four spill no SGPR either, as k_shade_pick<false, *, *> (tests/test_light_sampling_resources.py); the
    estimators' four park at most 2 SGPRs in VGPR lanes, the most any k_shade_pick<true, *, *> does. The
    tables stay in global memory, so a TAB instantiation's LDS is k_shade's 16168 bytes, 768 below
    k_shade_pick's."""
    grid = [k for k in kernels if "k_shade_grid" in k]
    probe = [k for k in kernels if "k_probe_light_grid" in k]
    assert len(grid) == 8 and len(probe) == 1, (grid, probe)
    for name in grid + probe:
        k = kernels[name]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    for tab in ("Lb0E", "Lb1E"):
        for alt in ("Lb0E", "Lb1E"):
            for env in ("Lb0E", "Lb1E"):
                k = _find(kernels, "_Z12k_shade_gridI" + alt + tab + env)
                assert k["group_segment_fixed_size"] == (16168 if tab == "Lb1E" else 8232), k
                assert k["sgpr_spill_count"] <= (0 if alt == "Lb0E" else 2), k
    assert max(kernels[k]["sgpr_spill_count"] for k in kernels if "k_shade_pickILb1E" in k) == 2


@pytest.mark.parametrize("alt", ["Lb0E", "Lb1E"])
@pytest.mark.parametrize("tab", ["Lb0E", "Lb1E"])
@pytest.mark.parametrize("env", ["Lb0E", "Lb1E"])
def test_waves_per_simd_are_not_below_the_pick_kernels(kernels, alt, tab, env):
    """k_shade_grid<alt, tab, env> against k_shade_pick<alt, tab, env>: the path tracer's keep 7 waves per SIMD
    (<= 72 VGPRs, <= 96 SGPRs), the estimators' kernel its counterpart's 4."""
    g = _find(kernels, "_Z12k_shade_gridI" + alt + tab + env)
    p = _find(kernels, "_Z12k_shade_pickI" + alt + tab + env)
    assert waves_per_simd(g) >= waves_per_simd(p), (g, p)
    if alt == "Lb0E":
        assert g["vgpr_count"] <= 72 and g["sgpr_count"] <= 96 and waves_per_simd(g) >= 7, g
    else:
        assert g["vgpr_count"] <= 128 and waves_per_simd(g) >= 4, g
