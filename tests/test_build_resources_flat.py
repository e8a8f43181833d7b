"""CPU: what the compiler made of step_kernel_stream_flat, the flat walk's body without z (hipcc cross-compiles gfx950 without a
GPU).  The headline's entry, ``step_kernel_stream_flat<true, false, false, 8>``: the seven-wave bounds that
tests/test_build_resources.py applies to ``step_kernel_stream<false, true, false, false, 8>``, no scratch, no spills of either
register file, and fewer vector registers (and less LDS) than that kernel, which it replaces on a settled cloud.  Every
instantiation: no scratch and no VGPR spills, the rule of test_build_resources.py for every streaming kernel; the plain ones
within the seven-wave register and LDS bounds.

SGPR spills are asserted for the loop lookup (8) only.  The fixed lookup (9) keeps one compare mask per record slot in scalar
registers (nine pairs) and sits at the 96-SGPR ceiling with two SGPRs spilled to vector-register lanes, no scratch: 94 SGPRs + 2
spills in ``step_kernel_stream_flat<true, false, false, 9>``, exactly the figures of the parent's
``step_kernel_stream<false, true, false, false, 9>`` (94 + 2, profiles/r06_resource_usage.txt).  The body without z did not
add them and did not remove them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flat_body_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = {r[0]: r for r in resource_usage.collect()}
    flat = {n: r for n, r in rows.items() if "step_kernel_stream_flat<" in n}
    # reflect x stored velocity x statistics, lookups 8 and 9: every combination plan_step can ask for on a settled cloud
    assert len(flat) == 16 and all(n.endswith((", 8>", ", 9>")) for n in flat), sorted(flat)
    for name, r in flat.items():
        print(name, r[1:])
        assert int(r[4]) == 0 and int(r[7]) == 0, (name, r)                         # no scratch, no VGPR spills
        if name.endswith(", 8>"):
            assert int(r[6]) == 0, (name, r)                                        # no SGPR spills
    for lookup in (8, 9):
        for reflect in ("true", "false"):
            new = flat["void cpf::step_kernel_stream_flat<%s, false, false, %d>" % (reflect, lookup)]
            # 7 waves per SIMD: <= 72 VGPRs, <= 96 SGPRs, <= 160 KB / 28 of LDS
            assert int(new[1]) <= 72 and int(new[3]) <= 96 and int(new[8]) <= 160 * 1024 // 28, new
    old = rows["void cpf::step_kernel_stream<false, true, false, false, 8>"]
    head = flat["void cpf::step_kernel_stream_flat<true, false, false, 8>"]
    assert int(head[1]) < int(old[1]) and int(head[8]) < int(old[8]), (head, old)
