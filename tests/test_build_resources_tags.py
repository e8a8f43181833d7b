"""CPU: what the compiler made of the tracer-tag kernels (csrc/cpf_tags.hip) for gfx950, through tools/resource_usage.py: the
transfer, the stamp and the field kernel exist, use no scratch memory, spill no register and keep their LDS within 64 KB a
workgroup -- and collect() and collect_age() list the kernels they listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::tag_field_kernel", "cpf::tag_stamp_kernel", "cpf::tag_transfer_kernel"]
SLICE = 4096                                 # ids per workgroup: 256 threads, four 16-byte loads each
WAVES = 4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_tag_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_tags()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    lists = WAVES * (SLICE // 4) * 2         # per wave a list of 16-bit slots, at most 16 per lane
    any_flag = 4                             # workgroup_any's word
    # the transfer kernel: the staged mask (2048 words), the four waves' hit lists, the 16 x 16 matrix of 32-bit words, the flag
    assert int(rows["cpf::tag_transfer_kernel"][8]) == 2048 * 4 + lists + 16 * 16 * 4 + any_flag
    # the stamp kernel: the four waves' lists of dead slots and the flag -- the bounds are searched in memory, not staged
    assert int(rows["cpf::tag_stamp_kernel"][8]) == lists + any_flag
    # the field kernel: 4096 bins of one 32-bit word and the waves' window bounds
    assert int(rows["cpf::tag_field_kernel"][8]) == 4096 * 4 + 2 * WAVES * 4


def test_collect_and_collect_age_list_what_they_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("tag_" in n or "age_" in n for n in names)
    other = [n for n in names if "step_kernel" not in n and "occupancy_kernel" not in n]
    assert sorted(other) == ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel",
                             "void cpf::sink_kernel<false>", "void cpf::sink_kernel<true>"]
    assert sum("occupancy_kernel" in n for n in names) == 2
    assert sorted(r[0] for r in tool.collect_age()) == ["cpf::age_absorb_kernel", "cpf::age_field_kernel", "cpf::age_stamp_kernel"]
    assert [r[0] for r in tool.collect_inlet()] == ["cpf::inlet_place_kernel"]
    # none of the new kernels carries a name the other resource tests select their rows by
    assert not any(k in n for n in KERNELS for k in tool.LISTED + ("age_", "inlet_"))
