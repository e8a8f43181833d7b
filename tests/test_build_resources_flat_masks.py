"""CPU: the round of the flat walk's body without z after round 15 (csrc/cpf_walk.h, trace_lds4_flat's EXIT_ALWAYS: the exit point
without its select; csrc/cpf_stream_ops.h, wait_vmcnt_flat: the counted wait as one hand-written block) as it stands in the code
object's listing -- one cross-compile of cpf_stream.hip to gfx950 assembly with the product's flags (tools/resource_usage.py), counted
with ``classes()`` of tests/test_build_resources_flat_face.py.

The headline's entry, ``step_kernel_stream_flat<true, false, false, 8>``, has fewer scalar-ALU plus branch instructions AND fewer vector
instructions than its parent.  The parent's figures are the same counting on the parent commit's listing: 419 scalar ALU + 86
branches, 410 vector (docs/experiments.md, round 15, has both sets).
The exit point stands behind both visits as two multiply-adds with nothing selected: between the last face block of a visit and the
next write of EXEC there is no v_cndmask.  The counted wait is in the listing as written: one block of four waits."""
import os
import re
import subprocess
import sys

import pytest

from test_build_resources_flat_face import classes, face_blocks, headline_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parent commit's headline entry, counted by classes()
PARENT_SCALAR_ALU, PARENT_BRANCH, PARENT_VECTOR = 419, 86, 410


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    asm_path = str(tmp_path_factory.mktemp("flat_masks") / "cpf_stream.s")
    r = subprocess.run(resource_usage.hipcc_cmd("cpf_stream.hip")[:-1] + ["-S", "--cuda-device-only", "-o", asm_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return headline_lines(open(asm_path).read())


def test_headline_counts_below_parent_on_both_pipes(listing):
    body, _ = listing
    c = classes(body)
    print("headline classes:", c)
    assert c["scalar_alu"] + c["branch"] < PARENT_SCALAR_ALU + PARENT_BRANCH, c
    assert c["scalar_alu"] < PARENT_SCALAR_ALU and c["branch"] <= PARENT_BRANCH, c
    assert c["vector"] < PARENT_VECTOR, c


def test_exit_point_is_not_selected(listing):
    _, lines = listing
    blocks = face_blocks(lines)
    assert len(blocks) == 8, len(blocks)
    for end, _ in (blocks[3], blocks[7]):                 # the fourth face block of the LDS visit and of the gather visit
        # from the block to the first join or branch behind the exit point's second multiply-add
        window, fmas = [], 0
        for t in lines[end:end + 60]:
            if t.startswith(";;#") or t.endswith(":") or t.startswith(("s_waitcnt", "s_nop")):
                continue
            if fmas >= 2 and (t.startswith(("s_branch", "s_cbranch")) or re.match(r"s_or_b64 exec, exec,", t)):
                break
            window.append(t)
            fmas += t.startswith(("v_fma_f64", "v_fmac_f64"))
        assert fmas == 2, window
        assert not any(t.startswith("v_cndmask") for t in window), window
        assert not any(re.match(r"v_cmp_lt_i32\w* [^,]+, -1,", t) for t in window), window


def test_counted_wait_as_written(listing):
    _, lines = listing
    blocks = []
    for i, t in enumerate(lines):
        if t == ";;#ASMSTART":
            blk = lines[i + 1:lines.index(";;#ASMEND", i)]
            if any(x.startswith(".Lcpf_wait_done_") for x in blk):
                blocks.append(blk)
    assert len(blocks) == 1, len(blocks)
    blk = blocks[0]
    assert [t for t in blk if t.startswith("s_waitcnt")] == ["s_waitcnt vmcnt(%d)" % k for k in (5, 3, 2, 0)], blk
    c = classes(blk)
    assert c["vector"] == 0 and c["scalar_alu"] == 3 and c["branch"] == 6, c
