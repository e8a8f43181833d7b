"""CPU: what the compiler made of the sink log's kernel (csrc/cpf_sinklog.hip) for gfx950, through tools/resource_usage.py: it
exists, uses no scratch memory, spills no register, its static LDS is the sum of its declarations -- and no other collector lists
it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::sink_log_kernel"]
SLICE = 4096                                 # ids per workgroup: 256 threads, four 16-byte loads each
WAVES = 4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_sink_log_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_sinklog()}
    assert sorted(rows) == KERNELS, sorted(rows)
    r = rows["cpf::sink_log_kernel"]
    scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
    print("MEASURED %s | VGPRs %s | SGPRs %s | waves/SIMD %s | LDS %d" % (r[0], r[1], r[3], r[5], lds))
    assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, r
    mask = 2048 * 4                          # the staged mask: kSinkLdsWords words
    lists = WAVES * (SLICE // 4) * 2         # per wave a list of 16-bit slots, at most 16 per lane
    reservation = WAVES * 4 + 8              # the four waves' totals, and the 64-bit base the cursor returned
    any_hit = 4                              # workgroup_any's word
    total = mask + lists + reservation + any_hit
    assert total == 16412
    # the 64-bit base is 8-byte aligned, so the block is laid out in a multiple of 8 bytes: 4 bytes of padding
    assert lds == (total + 7) // 8 * 8 == 16416, r
    # the leave pass of zones, whose shape this is, holds a table row where this holds the reservation
    zones = {z[0]: z for z in _tool().collect_zones()}
    assert int(zones["cpf::zone_leave_kernel"][8]) == 64 * 4 + mask + lists + any_hit


def test_no_other_collector_lists_the_kernel():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    # (collect() itself -- the step, occupancy and recycling kernels, minutes of compiling -- selects by LISTED, checked below)
    others = (tool.collect_age, tool.collect_inlet, tool.collect_tags, tool.collect_routes, tool.collect_exposure, tool.collect_zones)
    for collect in others:
        names = [r[0] for r in collect()]
        assert names and not any("sink_log" in n for n in names), (collect.__name__, names)
    # ... nor does its name carry a part the other resource tests select their rows by
    assert not any(k in n for n in KERNELS for k in tool.LISTED + ("age_", "tag_", "inlet_", "route_", "exposure_", "zone_"))
