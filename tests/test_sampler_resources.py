"""Register budget around the Sobol sampler's kernels (compiled here for gfx950, no GPU needed):
RTG_SAMPLER_SOBOL lives in kernels of its own (k_sobol_shade and k_sobol_shade_env in rtg_shade.hip,
k_sobol_shade_pick in rtg_light_pick.hip, k_sobol_generate_sampled in rtg_render.hip), so the existing
kernels of those units must keep the figures of the commit before it, and the new ones must hold their
state in registers at the waves per SIMD DESIGN.md §8m states."""
import re

import pytest

import kernel_meta

UNITS = ("device/rtg_shade.hip", "device/rtg_light_pick.hip", "device/rtg_render.hip")
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size")
# The figures of the commit before the sampler, same flags: (VGPRs, SGPRs, LDS bytes, spilled VGPRs,
# spilled SGPRs, scratch bytes). k_shade<true, *> spilled then as it does now.
BEFORE = {
    "_Z7k_shadeILb0ELb1E": (64, 88, 16168, 0, 0, 0),
    "_Z7k_shadeILb0ELb0E": (62, 87, 8232, 0, 0, 0),
    "_Z7k_shadeILb1ELb1E": (72, 94, 16168, 60, 6, 128),
    "_Z7k_shadeILb1ELb0E": (72, 94, 8232, 46, 20, 128),
    "_Z11k_shade_envILb0ELb1E": (64, 92, 16168, 0, 0, 0),
    "_Z11k_shade_envILb0ELb0E": (64, 91, 8232, 0, 0, 0),
    "_Z11k_shade_envILb1ELb1E": (108, 106, 16168, 0, 0, 0),
    "_Z11k_shade_envILb1ELb0E": (108, 106, 8232, 0, 4, 0),
    "_Z12k_shade_pickILb0ELb0ELb0E": (62, 85, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb0ELb1E": (62, 85, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb1ELb0E": (64, 84, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb0ELb1ELb1E": (64, 88, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb0ELb0E": (105, 104, 8232, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb0ELb1E": (108, 106, 8232, 0, 2, 0),
    "_Z12k_shade_pickILb1ELb1ELb0E": (106, 100, 16936, 0, 0, 0),
    "_Z12k_shade_pickILb1ELb1ELb1E": (109, 106, 16936, 0, 0, 0),
    "_Z10k_generate9ChunkArgs": (17, 58, 0, 0, 0, 0),
    "_Z18k_generate_sampled9ChunkArgs": (19, 54, 0, 0, 0, 0),
    "_Z14k_probe_camera": (22, 50, 0, 0, 0, 0),
    "_Z12k_accumulate9ChunkArgs": (21, 24, 0, 0, 0, 0),
    "_Z15k_accumulate_pm": (26, 33, 4096, 0, 0, 0),
}
# DESIGN.md §8m's table: kernel prefix -> (waves per SIMD, the VGPRs that many waves leave: 512 / waves
# rounded down to the granule of 8)
WAVES = {"_Z13k_sobol_shadeILb0E": (7, 72), "_Z13k_sobol_shadeILb1E": (4, 128),
         "_Z17k_sobol_shade_envILb0E": (7, 72), "_Z17k_sobol_shade_envILb1E": (4, 128),
         "_Z18k_sobol_shade_pickILb0E": (7, 72), "_Z18k_sobol_shade_pickILb1E": (4, 128)}
SMALL = ("k_sobol_generate_sampled", "k_sobol_probe_camera", "k_probe_sampler")


@pytest.fixture(scope="module")
def kernels():
    from raytracingrenderer_amd.build import DEVICE_FLAGS
    assert DEVICE_FLAGS["device/rtg_light_pick.hip"] == DEVICE_FLAGS["device/rtg_shade.hip"]
    return kernel_meta.kernels(*UNITS)


def test_new_kernels_hold_their_state_in_registers(kernels):
    """The 16 shading variants, the camera-ray generator, and the two probes: no scratch, no spilled VGPR.
    The pathTrace variants (ALT = false) keep their parents' 7 waves per SIMD (<= 72 VGPRs); the
    estimators' variants (ALT = true) run at 4 (<= 128), as k_shade_env<true, *> and k_shade_pick<true, *, *>
    do and k_shade<true, *> does not (it spills at 7, and so would its variant). The LDS figures are the
    parents': the sampler adds no table."""
    new = [k for k in kernels if "sobol" in k or "k_probe_sampler" in k]
    assert len(new) == 4 + 4 + 8 + 3, sorted(new)
    for name in new:
        k = kernels[name]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
    for prefix, (waves, vgprs) in WAVES.items():
        names = [k for k in kernels if k.startswith(prefix)]
        assert len(names) == (4 if "pick" in prefix else 2), (prefix, names)
        for name in names:
            k = kernels[name]
            assert k["vgpr_count"] <= vgprs, (name, k)
            assert k["sgpr_count"] <= 106, (name, k)
            tab = name[len(prefix):].startswith("Lb1E")
            pick = "pick" in prefix
            assert k["group_segment_fixed_size"] == ((16168 + (768 if pick else 0)) if tab else 8232), (name, k)
    for s in SMALL:
        names = [k for k in kernels if s in k]
        assert len(names) == 1 and kernels[names[0]]["vgpr_count"] <= 32 and kernels[names[0]]["group_segment_fixed_size"] == 0


def test_design_states_the_same_waves():
    """DESIGN.md §8m's table gives each new shading kernel the waves per SIMD this file checks."""
    import os
    text = open(os.path.join(kernel_meta.ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 8m."):]
    for kern, waves in (("k_sobol_shade<false, *>", 7), ("k_sobol_shade<true, *>", 4),
                        ("k_sobol_shade_env<false, *>", 7), ("k_sobol_shade_env<true, *>", 4),
                        ("k_sobol_shade_pick<false, *, *>", 7), ("k_sobol_shade_pick<true, *, *>", 4)):
        row = re.search(r"^\| `%s` \|.*$" % re.escape(kern), sec, re.M)
        assert row, kern
        assert int(row.group(0).split("|")[2]) == waves, row.group(0)


def test_draws_read_no_memory(kernels):
    """The tables are literal operands: a Sobol variant has exactly its parent's count of global, scalar and
    LDS loads, and it reverses bits with v_bfrev_b32 (more of them than the parent's own uses)."""
    s = kernel_meta.asm("device/rtg_shade.hip")

    def body(sym):
        return re.search(r"^%s\w*:.*?^\.Lfunc_end\d+:" % re.escape(sym), s, re.S | re.M).group(0)

    for tab in ("Lb0E", "Lb1E"):
        new, old = body("_Z13k_sobol_shadeILb0E" + tab), body("_Z7k_shadeILb0E" + tab)
        for op in ("global_load", "s_load", "s_buffer_load", "ds_read", "scratch_"):
            assert len(re.findall(r"\b" + op, new)) == len(re.findall(r"\b" + op, old)), (tab, op)
        assert new.count("v_bfrev_b32") > old.count("v_bfrev_b32"), tab


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_existing_kernels_keep_their_figures(kernels, name):
    names = [k for k in kernels if k.startswith(name)]
    assert len(names) == 1, (name, names)
    assert tuple(kernels[names[0]][key] for key in KEYS) == BEFORE[name], (name, kernels[names[0]])
