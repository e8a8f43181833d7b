"""CPU: what the compiler made of the exposure kernels (csrc/cpf_exposure.hip) for gfx950, through tools/resource_usage.py: the
accumulate, the absorb and the stamp kernel exist, use no scratch memory, spill no register and keep their LDS within 64 KB a
workgroup, the absorb kernel's dynamic part included -- and collect(), collect_age(), collect_tags(), collect_inlet() and
collect_routes() list the kernels they listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::exposure_absorb_kernel", "cpf::exposure_accumulate_kernel", "cpf::exposure_stamp_kernel"]
SLICE = 4096                                 # ids per workgroup: 256 threads, four 16-byte loads each
WAVES = 4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_exposure_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_exposure()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        print("MEASURED %s | VGPRs %s | SGPRs %s | waves/SIMD %s | LDS %d" % (name, r[1], r[3], r[5], lds))
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    lists = WAVES * (SLICE // 4) * 2         # per wave a list of 16-bit slots, at most 16 per lane
    # the accumulate kernel: the one word of "does anybody here have something to add"
    assert int(rows["cpf::exposure_accumulate_kernel"][8]) == 4
    # the absorb kernel: the staged mask (2048 words), the four waves' hit lists, the word of "any hit"
    static = 2048 * 4 + lists + 4
    assert int(rows["cpf::exposure_absorb_kernel"][8]) == static
    # ... and its dynamic part at its largest, 4096 words of 4 bytes
    assert static + 16 * 1024 <= 65536
    # the stamp kernel: the lists and the word of "any dead slot"
    assert int(rows["cpf::exposure_stamp_kernel"][8]) == lists + 4


def test_the_other_collectors_list_what_they_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("exposure_" in n or "route_" in n or "tag_" in n or "age_" in n for n in names)
    other = [n for n in names if "step_kernel" not in n and "occupancy_kernel" not in n]
    assert sorted(other) == ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel",
                             "void cpf::sink_kernel<false>", "void cpf::sink_kernel<true>"]
    assert sum("occupancy_kernel" in n for n in names) == 2
    assert sorted(r[0] for r in tool.collect_age()) == ["cpf::age_absorb_kernel", "cpf::age_field_kernel", "cpf::age_stamp_kernel"]
    assert sorted(r[0] for r in tool.collect_tags()) == ["cpf::tag_field_kernel", "cpf::tag_stamp_kernel", "cpf::tag_transfer_kernel"]
    assert [r[0] for r in tool.collect_inlet()] == ["cpf::inlet_place_kernel"]
    assert sorted(r[0] for r in tool.collect_routes()) == ["cpf::route_absorb_kernel", "cpf::route_field_kernel"]
    # no new kernel carries a name the other resource tests select their rows by
    assert not any(k in n for n in KERNELS for k in tool.LISTED + ("age_", "tag_", "inlet_", "route_"))
