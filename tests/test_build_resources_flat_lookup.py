"""CPU: the round's bookkeeping around the face blocks of the flat walk's body without z (csrc/cpf_stream.hip, stream_body under ZSET:
the lookup trip in hand-written ISA, the vote from masks, the j test in the wall branch) as it stands in the code object's listing -- one cross-compile of
cpf_stream.hip to gfx950 assembly with the product's flags (tools/resource_usage.py), counted with ``classes()`` of
tests/test_build_resources_flat_face.py.

The headline's entry, ``step_kernel_stream_flat<true, false, false, 8>``, has fewer scalar-ALU plus branch instructions AND fewer
vector instructions than its parent.  The parent's figures are the same counting on the parent commit's listing: 432 scalar ALU +
90 branches, 411 vector (docs/experiments.md, round 13, has both sets; round 12's table has the same three as "this commit").
The loop lookup's trip is in the listing as written: one block whose hit path holds seven scalar-issue instructions, one of them a
pad, and five vector instructions, and in which two wait states or more lie between a VALU write of a scalar register and a VALU that
reads it (gfx950 wants two; the compiler pads nothing inside an asm string)."""
import os
import re
import subprocess
import sys

import pytest

from test_build_resources_flat_face import classes, headline_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parent commit's headline entry, counted by classes()
PARENT_SCALAR_ALU, PARENT_BRANCH, PARENT_VECTOR = 432, 90, 411


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    asm_path = str(tmp_path_factory.mktemp("flat_lookup") / "cpf_stream.s")
    r = subprocess.run(resource_usage.hipcc_cmd("cpf_stream.hip")[:-1] + ["-S", "--cuda-device-only", "-o", asm_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return headline_lines(open(asm_path).read())


def test_headline_counts_below_parent_on_both_pipes(listing):
    body, _ = listing
    c = classes(body)
    print("headline classes:", c)
    assert c["scalar_alu"] + c["branch"] < PARENT_SCALAR_ALU + PARENT_BRANCH, c
    assert c["vector"] < PARENT_VECTOR, c


def test_lookup_trip_as_written(listing):
    _, lines = listing
    blocks = []
    for i, t in enumerate(lines):
        if t == ";;#ASMSTART":
            blk = lines[i + 1:lines.index(";;#ASMEND", i)]
            if any(x.startswith(".Lcpf_lk_trip_") for x in blk):
                blocks.append(blk)
    assert len(blocks) == 1, len(blocks)
    blk = blocks[0]
    trip = next(k for k, t in enumerate(blk) if t.startswith(".Lcpf_lk_trip_"))
    miss = next(k for k, t in enumerate(blk) if t.startswith(".Lcpf_lk_miss_"))
    hit = [t for t in blk[trip + 1:miss] if not t.startswith("s_branch")]          # (the hit path leaves through its conditional branch)
    c = classes(hit)
    print("lookup trip, hit path:", hit)
    assert c["vector"] == 5 and c["scalar_alu"] + c["branch"] + c["wait_nop"] == 7, c
    # a VALU write of an SGPR wants two wait states on gfx950 before a VALU reads it as an operand, and hipcc pads nothing inside
    # the string: behind every VALU instruction of the block that writes a scalar register (v_readlane's result, a v_cmp's mask), the next
    # two issue slots hold no VALU reader of it -- an `s_nop N` counts N + 1 states, any other instruction one
    for k, t in enumerate(blk):
        op, _, rest = t.partition(" ")
        dst = rest.split(",")[0].strip()
        if not op.startswith("v_") or not (dst.startswith("s") or dst == "vcc"):
            continue
        states = 0
        for u in blk[k + 1:]:
            if states >= 2 or u.endswith(":"):
                break
            uop, _, urest = u.partition(" ")
            if uop.startswith("v_"):
                assert not re.search(r"(?<![\w\[])" + re.escape(dst) + r"(?![\w:])", urest.split(",", 1)[1] if "," in urest else ""), (t, u, blk)
            states += int(urest) + 1 if uop == "s_nop" else 1
    # no write of EXEC and no memory operation in the block
    assert not any(t.split()[0].endswith("saveexec_b64") or " exec" in t.split(",")[0] for t in blk), blk
    assert not any(t.startswith(("global_", "ds_", "buffer_", "flat_", "s_load")) for t in blk), blk
