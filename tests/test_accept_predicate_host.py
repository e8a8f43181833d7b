"""The walk's acceptance rule on the CPU: cudaparticlesfoam_amd/csrc/cpf_accept.h is plain C++, so the host compiler builds it
(-ffp-contract=off, as the product) and the predicate the step kernels' face tests run is compared, case by case, with a numpy
statement of the reference's rule (query/ConvexQuery.cu:86-95): dT = fd / den; an infinite dT becomes -1; the face is accepted
iff fd < 1e-13 and 1e-13 < dT <= 1.  The pruned predicate's pre-filter claims to be EXACT -- fl(fd / den) <= 1 <=> |fd| <= |den|
for equal signs, everything else rejected by a later comparison -- and this is where that claim is tested: special values, the
ulps around |fd| == |den|, the quotients around the tolerance, and random pairs.  Zero disagreements."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cudaparticlesfoam_amd", "csrc")
TOL = 1e-13
NB_CELL = 3                              # an ordinary neighbour cell
NB_GROUP = -(2 ** 31) + 16 + 2           # a face-group code (cpf_internal.h: kGroupBase + g)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("accept_host") / "libcpf_accept_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-I" + CSRC,
                    os.path.join(HERE, "accept_host", "accept_host.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.accept_pruned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    lib.accept_pruned.restype = None
    lib.accept_tol.restype = C.c_double
    return lib


def run(fn, den, fd, groups=False, nb=NB_CELL):
    den, fd = np.ascontiguousarray(den, np.float64), np.ascontiguousarray(fd, np.float64)
    out = np.empty(den.shape[0], np.uint8)
    fn(den.ctypes.data, fd.ctypes.data, den.shape[0], int(groups), nb, out.ctypes.data)
    return out.astype(bool)


def reference_rule(den, fd):
    with np.errstate(all="ignore"):
        dT = fd / den
    dT = np.where(np.isinf(dT), -1.0, dT)
    return (fd < TOL) & (dT > TOL) & (dT <= 1.0)


def ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


@pytest.fixture(scope="module")
def cases():
    """(den, fd) of every case, in four families."""
    inf, nan = np.inf, np.nan
    up, dn = np.nextafter(TOL, 1.0), np.nextafter(TOL, 0.0)
    special = np.array([0.0, -0.0, inf, -inf, nan, 5e-324, -5e-324, 2.2e-308, -2.2e-308, TOL, -TOL, up, dn, 1.0, -1.0, 1e300, -1e300])
    assert special.size == 17
    g_den, g_fd = [a.ravel() for a in np.meshgrid(special, special, indexing="ij")]
    rng = np.random.default_rng(20241)
    n = 400_000
    den = np.exp(rng.uniform(-40.0, 5.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    # |fd| within two ulps of |den|, the sign of den: quotients at 1 -+ 2^-52 and 1 itself
    u_den = np.concatenate([den] * 5)
    u_fd = np.concatenate([np.copysign(ulps(np.abs(den), k), den) for k in (-2, -1, 0, 1, 2)])
    # quotients around the tolerance, and at 1
    r_den = np.concatenate([den] * 4)
    r_fd = np.concatenate([den * r for r in (1e-14, 1e-13, 1.0000001e-13, 1.0)])
    # random pairs: a start point inside or a rounding outside the face, moving either way, a step of up to twice the distance
    m = 1_000_000
    p_fd = -np.exp(rng.uniform(-40.0, 5.0, m)) * np.where(rng.random(m) < 0.9, 1.0, -1.0)
    p_den = p_fd / rng.uniform(-2.0, 2.0, m)
    return np.concatenate([g_den, u_den, r_den, p_den]), np.concatenate([g_fd, u_fd, r_fd, p_fd])


def test_tolerance_is_the_references(lib):
    assert lib.accept_tol() == TOL                       # query/ConvexQuery.cu:42
    assert lib.accept_is_group(NB_GROUP) and not lib.accept_is_group(NB_CELL) and not lib.accept_is_group(-5)


def test_pruned_predicate_is_the_reference_rule(lib, cases):
    den, fd = cases
    ref = reference_rule(den, fd)
    got = run(lib.accept_pruned, den, fd)
    bad = np.nonzero(got != ref)[0]
    print("cases %d, accepted by the reference %d, disagreements %d" % (den.size, int(ref.sum()), bad.size))
    assert bad.size == 0, [(den[i], fd[i], bool(got[i])) for i in bad[:10]]
    assert ref.sum() * 4 >= den.size, "the reference accepts too few of the cases for the comparison to mean much"


def test_groups_change_nothing_for_an_ordinary_slot(lib, cases):
    den, fd = cases
    assert np.array_equal(run(lib.accept_pruned, den, fd, groups=True), reference_rule(den, fd))


def test_group_slot_is_left_outwards_only(lib, cases):
    """Face groups (cpf_accept.h): a group slot is accepted only with den < 0 -- the reference's rule and that, nothing else."""
    den, fd = cases
    ref = reference_rule(den, fd)
    got = run(lib.accept_pruned, den, fd, groups=True, nb=NB_GROUP)
    assert np.array_equal(got, ref & (den < 0.0))
    assert (ref & ~(den < 0.0)).sum() > 1000 and got.sum() * 8 >= den.size          # both sides of the clause are exercised
    # without GROUPS the code is an ordinary neighbour (a mesh without groups never holds one)
    assert np.array_equal(run(lib.accept_pruned, den, fd, groups=False, nb=NB_GROUP), ref)
