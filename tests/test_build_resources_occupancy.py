"""CPU: what the compiler made of the occupancy kernel (csrc/cpf_occupancy.hip) for gfx950, through tools/resource_usage.py: it
exists in both its instantiations, uses no scratch memory, spills no register and keeps its LDS bins within 64 KB a workgroup."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_occupancy_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = {r[0]: r for r in resource_usage.collect() if "occupancy_kernel" in r[0]}
    assert sorted(rows) == ["void cpf::occupancy_kernel<false>", "void cpf::occupancy_kernel<true>"], sorted(rows)
    for name, r in rows.items():
        scratch, sgpr_spill, vgpr_spill, lds = int(r[4]), int(r[6]), int(r[7]), int(r[8])
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (name, r)
        assert 0 < lds <= 65536, (name, r)
