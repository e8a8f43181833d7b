"""CPU: what the compiler made of the zone kernels (csrc/cpf_zones.hip) for gfx950, through tools/resource_usage.py: the sample,
the leave and the stamp kernel exist, use no scratch memory, spill no register and keep their LDS within 64 KB a workgroup, the
sample kernel's dynamic part included -- and the other collectors list the kernels they listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::zone_leave_kernel", "cpf::zone_sample_kernel", "cpf::zone_stamp_kernel"]
SLICE = 4096                                 # ids per workgroup: 256 threads, four 16-byte loads each
WAVES = 4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_zone_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_zones()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        print("MEASURED %s | VGPRs %s | SGPRs %s | waves/SIMD %s | LDS %d" % (name, r[1], r[3], r[5], lds))
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    lists = WAVES * (SLICE // 4) * 2         # per wave a list of 16-bit slots, at most 16 per lane
    # the sample kernel: the one word of "is anybody here live" ...
    assert int(rows["cpf::zone_sample_kernel"][8]) == 4
    # ... and its dynamic part at its largest, 64 x 64 words of 4 bytes
    assert 4 + 64 * 64 * 4 <= 65536
    # the leave kernel: a word per row of the table (64), the staged mask (2048 words), the four waves' hit lists, "any hit"
    assert int(rows["cpf::zone_leave_kernel"][8]) == 64 * 4 + 2048 * 4 + lists + 4
    # the stamp kernel: the four lists and the word of "any dead slot", as for exposure's
    assert int(rows["cpf::zone_stamp_kernel"][8]) == lists + 4
    exposure = {r[0]: r for r in _tool().collect_exposure()}
    assert int(rows["cpf::zone_stamp_kernel"][8]) == int(exposure["cpf::exposure_stamp_kernel"][8])


def test_the_other_collectors_list_what_they_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("zone_" in n for n in names)
    assert sorted(r[0] for r in tool.collect_age()) == ["cpf::age_absorb_kernel", "cpf::age_field_kernel", "cpf::age_stamp_kernel"]
    assert sorted(r[0] for r in tool.collect_tags()) == ["cpf::tag_field_kernel", "cpf::tag_stamp_kernel", "cpf::tag_transfer_kernel"]
    assert [r[0] for r in tool.collect_inlet()] == ["cpf::inlet_place_kernel"]
    assert sorted(r[0] for r in tool.collect_routes()) == ["cpf::route_absorb_kernel", "cpf::route_field_kernel"]
    assert sorted(r[0] for r in tool.collect_exposure()) == ["cpf::exposure_absorb_kernel", "cpf::exposure_accumulate_kernel",
                                                             "cpf::exposure_stamp_kernel"]
    # no new kernel carries a name the other resource tests select their rows by
    assert not any(k in n for n in KERNELS for k in tool.LISTED + ("age_", "tag_", "inlet_", "route_", "exposure_"))
