"""CPU: what the compiler made of the flux-table kernels (csrc/cpf_inflow.hip) for gfx950, through tools/resource_usage.py: the five
kernels exist, use no scratch memory, spill no register, their static LDS is the sum of their declarations -- and no other
collector lists them, nor this one any of theirs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::inflow_apply_kernel", "cpf::inflow_flux_kernel", "cpf::inflow_fused_kernel", "cpf::inflow_scan_kernel",
           "cpf::inflow_sums_kernel"]
BLOCK = 256                                  # kInflowBlock: lanes of a workgroup of the four passes
FUSED = 1024                                 # kInflowFused: lanes of the fused kernel
SELECTORS = ("age_", "inlet_", "tag_", "route_", "exposure_", "zone_", "sink_log_")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_inflow_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_inflow()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name in KERNELS:
        r = rows[name]
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        print("MEASURED %s | VGPRs %s | SGPRs %s | waves/SIMD %s | LDS %d" % (r[0], r[1], r[3], r[5], lds))
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, r
        # one 64-bit word per wave, shared by the maximum and the scan
        waves = (FUSED if name == "cpf::inflow_fused_kernel" else BLOCK) // 64
        assert lds == waves * 8, r
    assert int(rows["cpf::inflow_fused_kernel"][8]) == 16 * 8 == 128 and int(rows["cpf::inflow_apply_kernel"][8]) == 4 * 8 == 32
    # the fused kernel is launched with 1024 lanes, sixteen waves, four a SIMD: its registers must allow them
    assert int(rows["cpf::inflow_fused_kernel"][5]) >= 4 and int(rows["cpf::inflow_fused_kernel"][1]) <= 128


def test_no_other_collector_lists_the_kernels():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    # (collect() itself -- the step, occupancy and recycling kernels, minutes of compiling -- selects by LISTED, checked below)
    others = (tool.collect_age, tool.collect_inlet, tool.collect_tags, tool.collect_routes, tool.collect_exposure, tool.collect_zones,
              tool.collect_sinklog)
    for collect in others:
        names = [r[0] for r in collect()]
        assert names and not any("inflow_" in n for n in names), (collect.__name__, names)
    # ... nor do the new names carry a part the other resource tests select their rows by ("age_" hides in words like "stage_")
    assert not any(k in n for n in KERNELS for k in tool.LISTED + SELECTORS)
    # ... and this collector lists none of theirs
    mine = [r[0] for r in tool.collect_inflow()]
    assert sorted(mine) == KERNELS and all("inflow_" in n for n in mine)
