#!/usr/bin/env python3
"""Compiler resource usage of every step-kernel instantiation, of the occupancy kernel and of the recycling kernels -> profiles/<label>_resource_usage.txt
(hipcc -Rpass-analysis=kernel-resource-usage; runs without a GPU).  python tools/resource_usage.py r02

python tools/resource_usage.py --digest <label> [--root <checkout>] [file.hip ...] -> profiles/<label>_code_digest.txt: one line
per kernel of cpf_stream.hip, cpf_kernels.hip and cpf_sort.hip -- demangled name | instruction count | SHA-256 of its normalised instruction
stream -- to compare the generated code of two commits (the other one through ``git worktree add`` and --root).  A refactor
that claims "no instruction changes" shows two listings that ``diff`` finds equal."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "cudaparticlesfoam_amd", "csrc")


# the kernels collect() lists, by a part of their names (cpf_recycle.hip: sink_kernel, respawn_count / _scan / _place_kernel)
LISTED = ("step_kernel", "occupancy_kernel", "sink_kernel", "respawn_")


def hipcc_cmd(src, root=ROOT):
    """The product's compile of one csrc file (csrc/Makefile's flags), without its output option; root: the checkout to compile."""
    cs = os.path.join(root, "cudaparticlesfoam_amd", "csrc")
    extra = ["-mllvm", "--amdgpu-sched-strategy=max-ilp"] if src == "cpf_stream.hip" else []      # as in csrc/Makefile
    return (["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off"] + extra +
            ["-I" + os.path.join(root, "include"), "-I" + cs, os.path.join(cs, src), "-Rpass-analysis=kernel-resource-usage"])


def parse(remarks, listed=LISTED):
    """Rows (name, VGPRs, AGPRs, SGPRs, scratch, waves, SGPR spills, VGPR spills, LDS) from the compiler's remarks (stderr)."""
    rows = []
    txt = re.sub(r" \[-Rpass-analysis=kernel-resource-usage\]", "", remarks)
    for b in re.split(r"(?=remark: [^\n]*Function Name:)", txt):
        m = re.search(r"Function Name:\s*(\S+)", b)
        if not m:
            continue
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0]
        if not any(k in name for k in listed):
            continue
        g = lambda k: (re.search(k + r":\s*(\S+)", b) or [None, "?"])[1]   # noqa: E731
        rows.append((name, g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g(r"ScratchSize \[bytes/lane\]"),
                     g(r"Occupancy \[waves/SIMD\]"), g("SGPRs Spill"), g("VGPRs Spill"), g(r"LDS Size \[bytes/block\]")))
    return rows


def collect():
    rows = []
    for src in ("cpf_stream.hip", "cpf_kernels.hip", "cpf_occupancy.hip", "cpf_recycle.hip"):
        r = subprocess.run(hipcc_cmd(src) + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
        rows += parse(r.stderr)
    return rows


def collect_age():
    """The same rows for the tracer-age kernels (cpf_age.hip: age_absorb_kernel, age_stamp_kernel, age_field_kernel); collect()
    does not list them.  The absorb kernel's LDS is its static part: its histogram (4 bytes a bin, 16 KB at most) is dynamic."""
    r = subprocess.run(hipcc_cmd("cpf_age.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("age_",))


def collect_inlet():
    """The same rows for the patch-source kernel (cpf_inlet.hip: inlet_place_kernel); collect() does not list it."""
    r = subprocess.run(hipcc_cmd("cpf_inlet.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("inlet_",))


def collect_inflow():
    """The same rows for the flux-table kernels (cpf_inflow.hip: inflow_fused_kernel, inflow_flux_kernel, inflow_sums_kernel,
    inflow_scan_kernel, inflow_apply_kernel); collect() does not list them.  All their LDS is static."""
    r = subprocess.run(hipcc_cmd("cpf_inflow.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("inflow_",))


def collect_tags():
    """The same rows for the tracer-tag kernels (cpf_tags.hip: tag_transfer_kernel, tag_stamp_kernel, tag_field_kernel); collect()
    does not list them.  All their LDS is static."""
    r = subprocess.run(hipcc_cmd("cpf_tags.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("tag_",))


def collect_routes():
    """The same rows for the route kernels (cpf_routes.hip: route_absorb_kernel, route_field_kernel); collect() does not list
    them.  The absorb kernel's LDS is its static part: its age histogram and its staged joint histogram (4 bytes a word, 32 KB
    at most) are dynamic."""
    r = subprocess.run(hipcc_cmd("cpf_routes.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("route_",))


def collect_exposure():
    """The same rows for the exposure kernels (cpf_exposure.hip: exposure_accumulate_kernel, exposure_absorb_kernel,
    exposure_stamp_kernel); collect() does not list them.  The absorb kernel's LDS is its static part: its histogram (4 bytes a
    word, 16 KB at most) is dynamic."""
    r = subprocess.run(hipcc_cmd("cpf_exposure.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("exposure_",))


def collect_zones():
    """The same rows for the zone kernels (cpf_zones.hip: zone_sample_kernel, zone_leave_kernel, zone_stamp_kernel); collect()
    does not list them.  The sample kernel's LDS is its static part: its table ((nZones + 1)^2 words of 4 bytes, 16 KB at most) is
    dynamic."""
    r = subprocess.run(hipcc_cmd("cpf_zones.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("zone_",))


def collect_sinklog():
    """The same rows for the sink log's kernel (cpf_sinklog.hip: sink_log_kernel); collect() does not list it.  All its LDS is
    static."""
    r = subprocess.run(hipcc_cmd("cpf_sinklog.hip") + ["-c", "-o", "/dev/null"], capture_output=True, text=True)
    return parse(r.stderr, ("sink_log_",))


def kernel_bodies(asm):
    """mangled kernel name -> its instructions (labels, directives and comments dropped).  Only what the listing types as a
    function: a library's constant table (rocprim has one) is a _Z label too, and the text behind the last one is the metadata."""
    out, name = {}, None
    functions = set(re.findall(r"^\s*\.type\s+(_Z\w+),@function", asm, re.M))
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and m.group(1) not in functions:
            name = None
            continue
        if m:
            name = m.group(1); out[name] = []
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        t = line.split(";")[0].strip()
        if name is None or not t or t.startswith(".") or t.endswith(":"):
            continue
        out[name].append(t)
    return out


def digests(asm):
    """Rows (demangled name, instruction count, SHA-256) of every kernel in a ``hipcc -S --cuda-device-only`` listing.  The
    hash is over kernel_bodies' instructions, one per line, single-spaced, with the function index taken out of the block labels
    that branches name (.LBB<function>_<block>): a kernel that only moved within its file keeps its digest."""
    bodies = kernel_bodies(asm)
    names = subprocess.run(["c++filt"], input="\n".join(bodies), capture_output=True, text=True).stdout.split("\n")
    rows = []
    for mangled, name in zip(bodies, names):
        text = "\n".join(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(t.split())) for t in bodies[mangled])
        rows.append((name.split("(")[0], str(len(bodies[mangled])), hashlib.sha256(text.encode()).hexdigest()))
    return sorted(rows)


def main_digest(argv):
    root = ROOT
    if "--root" in argv:
        i = argv.index("--root"); root = os.path.abspath(argv[i + 1]); del argv[i:i + 2]
    label, srcs = argv[0], argv[1:] or ["cpf_stream.hip", "cpf_kernels.hip", "cpf_sort.hip"]
    out = ["# Generated code of the kernels: hipcc -S --cuda-device-only with csrc/Makefile's flags (gfx950), per kernel the",
           "# SHA-256 of its instructions without comments, directives, labels and the function index of .LBB<function>_<block>.",
           "# tools/resource_usage.py --digest " + label,
           "# file | kernel | instructions | sha256"]
    for src in srcs:
        asm_path = os.path.join(tempfile.mkdtemp(), src + ".s")
        r = subprocess.run(hipcc_cmd(src, root)[:-1] + ["-S", "--cuda-device-only", "-o", asm_path], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr[-4000:])
        out += [" | ".join((src,) + row) for row in digests(open(asm_path).read())]
    path = os.path.join(ROOT, "profiles", label + "_code_digest.txt")
    open(path, "w").write("\n".join(out) + "\n")
    print("%s: %d kernels" % (path, len(out) - 4))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--digest":
        return main_digest(sys.argv[2:])
    label = sys.argv[1] if len(sys.argv) > 1 else "r03"
    rows = collect()
    out = ["# Compiler resource usage of the step kernels, the occupancy kernel and the recycling kernels: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off",
           "# -Rpass-analysis=kernel-resource-usage (ROCm 7.2).  tools/resource_usage.py " + label,
           "# kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | waves/SIMD (registers) | SGPR spills | VGPR spills | LDS B/block"]
    out += [" | ".join(r) for r in rows]
    path = os.path.join(ROOT, "profiles", label + "_resource_usage.txt")
    open(path, "w").write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
