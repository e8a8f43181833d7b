"""CPU: what the compiler made of the recycling kernels (csrc/cpf_recycle.hip) for gfx950, through tools/resource_usage.py: the sink
kernel in both its instantiations and the three respawn passes exist, use no scratch memory, spill no register and keep their LDS
within 64 KB a workgroup -- and the rows the other resource tests read are the ones they read before."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["cpf::respawn_count_kernel", "cpf::respawn_place_kernel", "cpf::respawn_scan_kernel", "void cpf::sink_kernel<false>",
           "void cpf::sink_kernel<true>"]


def test_recycle_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.collect()
    mine = {r[0]: r for r in rows if "step_kernel" not in r[0] and "occupancy_kernel" not in r[0]}
    assert sorted(mine) == KERNELS, sorted(mine)
    for name, r in mine.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
    # the sink's mask stage is its LDS: 2048 words and the hit count
    assert int(mine["void cpf::sink_kernel<true>"][8]) == int(mine["void cpf::sink_kernel<false>"][8]) == 2048 * 4 + 4
    # nobody else's row carries one of the new names
    assert not any(k in r[0] for r in rows if r[0] not in mine for k in ("sink_kernel", "respawn_"))
