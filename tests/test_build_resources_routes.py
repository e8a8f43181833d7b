"""CPU: what the compiler made of the route kernels (csrc/cpf_routes.hip) for gfx950, through tools/resource_usage.py: the absorb
and the field kernel exist, use no scratch memory, spill no register and keep their LDS within 64 KB a workgroup, dynamic part
included -- and collect(), collect_age(), collect_tags() and collect_inlet() list the kernels they listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::route_absorb_kernel", "cpf::route_field_kernel"]
SLICE = 4096                                 # ids per workgroup: 256 threads, four 16-byte loads each
WAVES = 4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_route_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_routes()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    lists = WAVES * (SLICE // 4) * 2         # per wave a list of 16-bit slots, at most 16 per lane
    # the absorb kernel: sink_pass's staged mask (2048 words) and its sum, the four waves' hit lists, a byte per slot of the slice
    # for the sink group of a hit, the 16 x 16 matrix of 32-bit words
    static = 2048 * 4 + 4 + lists + SLICE + 16 * 16 * 4
    assert int(rows["cpf::route_absorb_kernel"][8]) == static
    # ... and its dynamic part at its largest: 4096 age bins and a staged joint histogram of 4096 words (one route), 4 bytes each
    assert static + (4096 + 4096) * 4 <= 65536
    # the field kernel: 2048 bins of one 64-bit word and the waves' window bounds
    assert int(rows["cpf::route_field_kernel"][8]) == 2048 * 8 + 2 * WAVES * 4


def test_the_other_collectors_list_what_they_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("route_" in n or "tag_" in n or "age_" in n for n in names)
    other = [n for n in names if "step_kernel" not in n and "occupancy_kernel" not in n]
    assert sorted(other) == ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel",
                             "void cpf::sink_kernel<false>", "void cpf::sink_kernel<true>"]
    assert sum("occupancy_kernel" in n for n in names) == 2
    assert sorted(r[0] for r in tool.collect_age()) == ["cpf::age_absorb_kernel", "cpf::age_field_kernel", "cpf::age_stamp_kernel"]
    assert sorted(r[0] for r in tool.collect_tags()) == ["cpf::tag_field_kernel", "cpf::tag_stamp_kernel", "cpf::tag_transfer_kernel"]
    assert [r[0] for r in tool.collect_inlet()] == ["cpf::inlet_place_kernel"]
    # neither new kernel carries a name the other resource tests select their rows by
    assert not any(k in n for n in KERNELS for k in tool.LISTED + ("age_", "tag_", "inlet_"))
