"""CPU: the round of the flat walk's body without z (csrc/cpf_stream.hip, ``step_kernel_stream_flat``) as the compiler emits it
for gfx950 -- one cross-compile of cpf_stream.hip to assembly with the product's flags (tools/resource_usage.py) and the
compiler's resource remarks.

The headline's entry, ``step_kernel_stream_flat<true, false, false, 8>``, keeps its eighth wave per SIMD: at most 64 VGPRs, at most
80 scalar registers in all, at most 5 120 bytes of LDS (160 KB / 32 waves), no scratch, no spill of either register file.  Its static
instruction count is below the parent commit's 1 442 and it holds at most 8 ``v_rcp_f64``, one per IEEE division: four faces in
the LDS walk and four in the flat gather walk.  Both parent figures are the parent's own: 1 442 is round 8's record
(docs/experiments.md, "Round 8": "Static (cross-compile): 1 689 -> 1 442 instructions"), 10 ``v_rcp_f64`` -- the four of the LDS
walk and the six of ``trace_fixed<6>`` on the global record -- is a ``hipcc -S`` compile of the parent commit with the same flags.
The fixed lookup's entry (9) is no worse off than its parent: 94 scalar registers and two of them spilled to vector lanes."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_INSTRUCTIONS = 1442        # docs/experiments.md, round 8
MAX_DIVISIONS = 8                 # the parent: 10 (hipcc -S of the parent commit)


def test_flat_round_resources_and_code(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    _kernel_bodies = resource_usage.kernel_bodies          # (lives with the digest mode that shares it)
    asm_path = str(tmp_path / "cpf_stream.s")
    r = subprocess.run(resource_usage.hipcc_cmd("cpf_stream.hip") + ["-S", "--cuda-device-only", "-o", asm_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {row[0]: row for row in resource_usage.parse(r.stderr)}
    head = rows["void cpf::step_kernel_stream_flat<true, false, false, 8>"]
    print("headline", head[1:])
    # eight waves per SIMD: <= 64 VGPRs, <= 80 SGPRs in all, <= 160 KB / 32 of LDS; no scratch, no spills
    assert int(head[1]) <= 64 and int(head[3]) <= 80 and int(head[8]) <= 5120, head
    assert int(head[4]) == 0 and int(head[6]) == 0 and int(head[7]) == 0, head
    nine = rows["void cpf::step_kernel_stream_flat<true, false, false, 9>"]
    print("lookup 9", nine[1:])
    assert int(nine[3]) <= 94 and int(nine[6]) <= 2 and int(nine[4]) == 0 and int(nine[7]) == 0, nine
    bodies = _kernel_bodies(open(asm_path).read())
    names = subprocess.run(["c++filt"], input="\n".join(bodies), capture_output=True, text=True).stdout.split("\n")
    by_name = {d.split("(")[0]: bodies[n] for n, d in zip(bodies, names)}
    body = by_name["void cpf::step_kernel_stream_flat<true, false, false, 8>"]
    n_rcp = sum(1 for t in body if t.startswith("v_rcp_f64"))
    print("headline: %d instructions, %d v_rcp_f64" % (len(body), n_rcp))
    assert 0 < len(body) < PARENT_INSTRUCTIONS, len(body)
    assert 4 <= n_rcp <= MAX_DIVISIONS, n_rcp
