"""CPU: what the compiler made of the patch-source kernel (csrc/cpf_inlet.hip) for gfx950, through tools/resource_usage.py: the
place kernel exists, uses no scratch memory, spills no register, and its LDS is what the source declares -- and collect() lists the
kernels it listed before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::inlet_place_kernel"]
# the staged bounds (4096 words), the four waves' ranks and slot lists, drawn / placed / any, the bin grid (12 doubles, 3 ints and
# their padding, 2 pointers), rounded up to a multiple of 8
LDS = 4096 * 4 + 4 * 4 + 4 * 256 * 4 + 3 * 4 + (12 * 8 + 16 + 2 * 8)
LDS = (LDS + 7) // 8 * 8                     # 20 640 bytes


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    return resource_usage


def test_inlet_kernel_resources():
    rows = {r[0]: r for r in _tool().collect_inlet()}
    assert sorted(rows) == KERNELS, sorted(rows)
    r = rows["cpf::inlet_place_kernel"]
    scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
    assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, r
    assert lds == LDS == 20640, r
    # 20 640 bytes: seven workgroups of four waves share a CU's 160 KB (28 of its 32 wave slots); sixteen -- 10 KB each -- would
    # need the staged bounds cut to 1024 entries.  The kernel's registers allow five waves a SIMD, 20 a CU, five workgroups: LDS
    # is not what limits it.
    assert 7 * lds <= 160 * 1024 < 8 * lds
    assert int(r[5]) <= 7                                                    # waves a SIMD by registers == workgroups a CU (a wave of each per SIMD)


def test_collect_lists_what_it_listed_before():
    tool = _tool()
    assert tool.LISTED == ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")
    names = [r[0] for r in tool.collect()]
    assert names and not any("inlet_" in n for n in names)
    other = [n for n in names if "step_kernel" not in n and "occupancy_kernel" not in n]
    assert sorted(other) == ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel",
                             "void cpf::sink_kernel<false>", "void cpf::sink_kernel<true>"]
    assert sum("occupancy_kernel" in n for n in names) == 2
    # the new kernel carries no name the other resource tests select their rows by (theirs, and the age tests' "age_")
    new = [r[0] for r in tool.collect_inlet()]
    assert new and not any(k in n for n in new for k in tool.LISTED + ("age_",))
    assert not any("inlet_" in r[0] for r in tool.collect_age())
