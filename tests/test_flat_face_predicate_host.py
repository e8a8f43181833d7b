"""CPU: the chain form of the face acceptance -- c4, c3, then ONE unsigned comparison of the bit patterns of fd and den in place of
"|fd| <= |den|" and "den < 0 or fd >= 0"; csrc/cpf_accept.h, face_accept_chain: what the hand-written face block of the flat walk
executes -- against ``face_accept<false>``.

tests/flat_face_host/flat_face_host.cpp is a plain executable built here with the host compiler, with the address and undefined-
behaviour sanitizers where the compiler has them.  Its grid is +-0, the smallest and largest denormals and normals, +-inf and NaN for
fd and den (every pair, so |fd| == |den| too), fd at tol and one ulp either side, dT one ulp either side of tol and of dTmin, dT ==
dTmin, bs == token, and a million random pairs; accepted set, dTmin, next and best must be equal, bit for bit."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cudaparticlesfoam_amd", "csrc")
SRC = os.path.join(HERE, "flat_face_host", "flat_face_host.cpp")


def _build(cxx, exe, extra):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe] + extra,
                          capture_output=True, text=True)


def test_chain_equals_face_accept(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "flat_face_host")
    r = _build(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    sanitized = r.returncode == 0
    if not sanitized:                      # a compiler without the sanitizers' runtimes: the comparison itself still runs
        r = _build(cxx, exe, [])
        assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", sanitized)
    print(run.stdout[-1500:])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-1500:])
    m = re.search(r"cases (\d+) accepted (\d+) mismatches 0\s*$", run.stdout)
    assert m, run.stdout[-500:]
    assert int(m.group(1)) > 1000000 and int(m.group(2)) > 10000, m.groups()
