"""CPU: the statement of the "VertexVelocity" cycle that tests/test_gpu_vertex_cycle.py holds the kernels against
(tests/vertexcycle.py) is the reference's cycle, and the bar of that comparison is one the reference itself meets.

1. On the inputs of tests/golden/vertex_box.npz -- the reference's own functions, 60 cycles with wall reflections -- the helper
   on the plain-C tet walk gives the golden's positions, tet ids and velocities bit for bit.
2. On every mesh, cloud and time step of the GPU file the strict and the contracting build of the reference's own functions
   (oracle/_ref, where it was built) walk through identical cells at every checkpoint, their positions agree within the bar the
   GPU file uses and nobody dies.  Rounding grows along trajectories in an interpolated field -- measured on these inputs, max
   |dx| / diagonal strict against contracting: see the figures this test prints (docs/experiments.md quotes them) -- which is
   why the checkpoints stop at 20 cycles."""
import os

import numpy as np
import pytest

import vertexcycle as V

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_helper_reproduces_the_reference_golden_bitwise(oracle_libs):
    from cudaparticlesfoam_amd.cases import box_mesh
    g = np.load(os.path.join(G, "vertex_box.npz"))
    c = V.Case("golden box", box_mesh(10, 9, 8), vertex_u=g["vertex_U"], dt=float(g["dt"]))
    tw = oracle_libs.TetWalk()
    cell0 = (g["tet0"] // 12).astype(np.int32)
    out = V.run_cpu(tw, c, g["xyz0"], cell0, checkpoints=tuple(int(k) for k in g["checkpoints"]))
    assert np.array_equal(out["ids0"], g["tet0"])                       # ids = 12 * cell0, then bary_query
    for k in g["checkpoints"]:
        s = out[int(k)]
        assert np.array_equal(s.P, g["P_%d" % k]) and np.array_equal(s.ids, g["tet_%d" % k]), k
        assert np.array_equal(s.vels, g["vel_%d" % k]), k
        assert np.array_equal(s.state, g["tet_%d" % k] // 12)


def test_states_of_a_particle_that_leaves(oracle_libs):
    """NO_REFLECT on the CPU: a particle that crosses a wall is moved to where its displacement ends and keeps w = 1 with a
    negative id for that cycle (the library's CPF_CELL_LOST), the next advect switches it off where it is (CPF_CELL_FROZEN);
    one that starts with cell -1 is switched off by the first advect."""
    tw = oracle_libs.TetWalk()
    c = V.case("block A")
    xyz, cell0 = V.cloud("block A", 3000)
    out = V.run_cpu(tw, c, xyz, cell0, checkpoints=(1, 2, 6), reflect=False)
    started_out = cell0 < 0
    assert started_out.sum() == len(V.OUTSIDE_AT)
    assert (out[1].state[started_out] == -2).all() and np.array_equal(out[6].P[started_out, :3], xyz[started_out])
    lost1 = (out[1].state == -1)
    assert lost1.sum() > 0 and (out[1].P[lost1, 3] == 1).all() and (out[2].state[lost1] == -2).all()
    assert np.array_equal(out[2].P[lost1, :3], out[1].P[lost1, :3]) and (out[2].P[lost1, 3] == 0).all()
    assert (V.inward_distance(c.mesh, out[1].P[lost1, :3], cell0[lost1]) < 0).all()            # outside where it started
    later = (out[6].state < 0) & (out[1].state >= 0)
    assert later.sum() > 0


@pytest.mark.parametrize("name", list(V.MESHES))
def test_reference_builds_agree_within_the_gpu_bar(name, oracle_libs):
    if not oracle_libs.have_ref_fma():
        pytest.skip("oracle/_ref (strict and contracting builds) exists only where the reference tree was present")
    strict, fma = oracle_libs.RefLib(), oracle_libs.RefLib(fma=True)
    c = V.case(name)
    for n in V.MESHES[name][2]:
        xyz, cell0 = V.cloud(name, n)
        a = V.run_cpu(strict, c, xyz, cell0)
        b = V.run_cpu(fma, c, xyz, cell0)
        live = cell0 >= 0
        for k in V.CHECKPOINTS:
            r = V.rel(a[k].P, b[k].P, c.diag)
            print("%s n=%d k=%d: strict vs contracting max |dx|/L %.3e, cells differ %d" %
                  (name, n, k, r.max(), (a[k].ids // 12 != b[k].ids // 12).sum()))
            assert np.array_equal(a[k].ids // 12, b[k].ids // 12), (name, n, k)
            assert r.max() <= V.REL_TOL, (name, n, k, r.max())
            assert (a[k].P[live, 3] == 1).all() and (b[k].P[live, 3] == 1).all() and (a[k].ids[live] >= 0).all(), (name, n, k)


def test_tetwalk_is_the_strict_reference_on_these_inputs(oracle_libs):
    """The GPU file's CPU side is TetWalk (it exists on the GPU machine); where the reference's own build exists too, the two
    are the same bits through all 20 cycles, with the kick and without reflection as well."""
    if not oracle_libs.have_ref():
        pytest.skip("oracle/_ref exists only where the reference tree was present")
    tw, ref = oracle_libs.TetWalk(), oracle_libs.RefLib()
    for name in ("block A", "thin box"):
        c = V.case(name)
        xyz, cell0 = V.cloud(name, V.MESHES[name][2][0])
        for D, reflect in ((0.0, True), (c.D, True), (0.0, False), (c.D, False)):
            a = V.run_cpu(tw, c, xyz, cell0, D=D, reflect=reflect)
            b = V.run_cpu(ref, c, xyz, cell0, D=D, reflect=reflect)
            for k in V.CHECKPOINTS:
                assert np.array_equal(a[k].P, b[k].P) and np.array_equal(a[k].ids, b[k].ids) and np.array_equal(a[k].vels, b[k].vels)
