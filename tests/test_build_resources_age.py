"""CPU: what the compiler made of the tracer-age kernels (csrc/cpf_age.hip) for gfx950, through tools/resource_usage.py: the absorb,
the stamp and the field kernel exist, use no scratch memory, spill no register and keep
their LDS within 64 KB a workgroup -- and collect() lists the kernels it listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::age_absorb_kernel", "cpf::age_field_kernel", "cpf::age_stamp_kernel"]
MAX_BINS = 4096                              # cpf_age_enable's limit: the absorb kernel's dynamic LDS is 4 bytes a bin


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_age_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_age()}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    # the absorb kernel: the staged mask, the four waves' hit lists and the hit count; with the largest histogram still within 64 KB
    absorb = int(rows["cpf::age_absorb_kernel"][8])
    assert absorb == 2048 * 4 + 4 * 1024 * 2 + 4
    assert absorb + 4 * MAX_BINS <= 65536
    # the field kernel: 2048 bins of one 64-bit word and the waves' window bounds
    assert int(rows["cpf::age_field_kernel"][8]) == 2048 * 8 + 2 * 4 * 4


def test_collect_lists_what_it_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("age_" in n for n in names)
    other = [n for n in names if "step_kernel" not in n and "occupancy_kernel" not in n]
    assert sorted(other) == ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel",
                             "void cpf::sink_kernel<false>", "void cpf::sink_kernel<true>"]
    assert sum("occupancy_kernel" in n for n in names) == 2
    # none of the new kernels carries a name the other resource tests select their rows by
    assert not any(k in n for n in (r[0] for r in tool.collect_age()) for k in tool.LISTED)
