"""CPU: the hand-written face block of the flat walk's body without z (csrc/cpf_walk.h, ``face_accept_flat_asm``; called from
``stream_body`` under ``ZSET`` in csrc/cpf_stream.hip) as it stands in the code object's listing -- one cross-compile of cpf_stream.hip to
gfx950 assembly with the product's flags (tools/resource_usage.py).

The headline's entry, ``step_kernel_stream_flat<true, false, false, 8>``:
  * has strictly fewer scalar-ALU plus branch instructions than its parent and not more vector instructions.  The parent's
    figures are this file's own counting (``classes`` below) on the parent commit's listing: 510 scalar ALU + 100 branches,
    447 vector (docs/experiments.md, round 12, has both sets);
  * holds eight face blocks -- four faces in the LDS visit, four in the gather visit -- and each of them saves EXEC in its first
    instruction, narrows it with ``v_cmpx`` only, branches on ``execz`` to a label of its own inside the block and restores EXEC
    from the saved pair in its last instruction;
  * is followed, behind each block, by no lane-crossing read (DPP, ``v_readlane``, ``v_readfirstlane``, ``v_permlane*``,
    ``ds_swizzle``/``ds_bpermute`` excluded: they are LDS instructions) within five instructions: a VALU write of EXEC wants five
    wait states in front of one, and the compiler does not see the ``v_cmpx`` in the string."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "void cpf::step_kernel_stream_flat<true, false, false, 8>"

# the parent commit's headline entry, counted by classes() below
PARENT_SCALAR_ALU, PARENT_BRANCH, PARENT_VECTOR = 510, 100, 447

NOT_ALU = ("s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_sleep", "s_sethalt", "s_setprio", "s_code_end", "s_inst_prefetch")


def classes(body):
    """Static instruction classes of one kernel's instructions (tools/resource_usage.py, kernel_bodies)."""
    c = {"all": len(body), "vector": 0, "scalar_alu": 0, "branch": 0, "wait_nop": 0, "v_cmp": 0, "v_cmpx": 0, "v_mov": 0}
    for t in body:
        op = t.split()[0]
        if op.startswith("v_"):
            c["vector"] += 1
            c["v_cmp"] += op.startswith("v_cmp")
            c["v_cmpx"] += op.startswith("v_cmpx")
            c["v_mov"] += op.startswith("v_mov")
        elif op.startswith("s_branch") or op.startswith("s_cbranch"):
            c["branch"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            c["wait_nop"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_ALU):
            c["scalar_alu"] += 1          # (scalar memory reads included: they issue on the scalar pipe)
    return c


def headline_lines(asm):
    """The headline entry's listing, labels and asm markers kept."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    bodies = resource_usage.kernel_bodies(asm)
    names = subprocess.run(["c++filt"], input="\n".join(bodies), capture_output=True, text=True).stdout.split("\n")
    mangled = [m for m, d in zip(bodies, names) if d.split("(")[0] == HEADLINE]
    assert len(mangled) == 1, mangled
    lines, on = [], False
    for line in asm.splitlines():
        if line.startswith(mangled[0] + ":"):
            on = True
            continue
        if on and line.startswith(".Lfunc_end"):
            break
        if on:
            t = line.strip()
            if t.startswith(";;#ASM"):
                lines.append(t)
                continue
            t = line.split(";")[0].strip()
            if t and (not t.startswith(".") or t.endswith(":")):
                lines.append(t)
    return bodies[mangled[0]], lines


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    asm_path = str(tmp_path_factory.mktemp("flat_face") / "cpf_stream.s")
    r = subprocess.run(resource_usage.hipcc_cmd("cpf_stream.hip")[:-1] + ["-S", "--cuda-device-only", "-o", asm_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return headline_lines(open(asm_path).read())


def face_blocks(lines):
    """(index behind the block, the block's lines) of every asm statement that saves EXEC."""
    out, i = [], 0
    while i < len(lines):
        if lines[i] == ";;#ASMSTART":
            j = lines.index(";;#ASMEND", i)
            blk = lines[i + 1:j]
            if any(re.match(r"s_mov_b64 s\[\d+:\d+\], exec$", t) for t in blk):
                out.append((j + 1, blk))
            i = j
        i += 1
    return out


def test_headline_counts_below_parent(listing):
    body, _ = listing
    c = classes(body)
    print("headline classes:", c)
    assert c["scalar_alu"] + c["branch"] < PARENT_SCALAR_ALU + PARENT_BRANCH, c
    assert c["vector"] <= PARENT_VECTOR, c


def test_face_blocks_save_and_restore_exec(listing):
    _, lines = listing
    blocks = face_blocks(lines)
    print("face blocks:", len(blocks))
    assert len(blocks) == 8, len(blocks)
    for _, blk in blocks:
        m = re.match(r"s_mov_b64 (s\[\d+:\d+\]), exec$", blk[0])
        assert m, blk[0]
        assert blk[-1] == "s_mov_b64 exec, " + m.group(1), blk[-1]
        label = blk[-2]
        assert label.endswith(":") and label.startswith(".Lcpf_face_"), label
        assert blk.count("s_cbranch_execz " + label[:-1]) == 1, blk
        inner = blk[1:-2]
        # EXEC is written by v_cmpx alone in between, the saved pair by nothing, and no other label or branch is in the block
        assert sum(t.startswith("v_cmpx") for t in inner) == 5, inner
        assert not any(re.search(r"\bexec\b", t) for t in inner), inner
        assert not any(t.split(None, 1)[1].split(",")[0].strip() == m.group(1) for t in inner if " " in t), inner
        assert sum(t.endswith(":") or t.startswith(("s_branch", "s_cbranch")) for t in inner) == 1, inner
        assert sum(t.startswith("v_rcp_f64") for t in inner) == 1, inner
        # v_div_scale's VCC reaches v_div_fmas after four wait states or more
        scale = max(k for k, t in enumerate(inner) if t.startswith("v_div_scale_f64"))
        fmas = min(k for k, t in enumerate(inner) if t.startswith("v_div_fmas_f64"))
        assert fmas - scale - 1 >= 4, inner


def test_no_lane_crossing_read_behind_a_face_block(listing):
    _, lines = listing
    for end, _ in face_blocks(lines):
        behind = [t for t in lines[end:end + 12] if not t.endswith(":") and not t.startswith(";;#")][:5]
        for t in behind:
            assert not re.search(r"v_readlane|v_readfirstlane|v_writelane|v_permlane|_dpp|dpp_ctrl|row_|quad_perm|wave_sh|bank_mask", t), behind
