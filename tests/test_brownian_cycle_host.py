"""CPU: oracle/cellwalk.c's cycle with the kick's deviates GIVEN as data (cw_step_given / CellWalk.step_given) -- the statement the
kicked kernels are compared with bit for bit in tests/test_gpu_brownian_cycle.py, there on the device's own deviates, here on libm's:

* fed with cw_normal3's deviates, reflect = 1 and zfold = 0 it IS cw_step(D > 0): one body, the same bits, statistics included;
* reflect = 0 (CPF_STEP_NO_REFLECT) loses exactly the particles that reflect = 1 reflects in that cycle, and moves them to P + disp;
* zfold = 1 (fold_z of csrc/cpf_walk.h) is the reference's order of operations up to the rounding of one hit point: the figures
  test_front_and_back_planes_mirrored_before_the_walk_equal_the_reference_order asserts GPU to GPU;
* and the inputs the GPU tests run on do go through the hard paths (tests/browniancycle.py, hard_paths)."""
import numpy as np
import pytest

import browniancycle as B


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", B.MESHES_3D + B.MESHES_THIN)
def test_step_given_on_cw_normal3s_deviates_is_cw_step(name, oracle_libs):
    c, cw = B.case(name), B.cellwalk()
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    assert not np.array_equal(gid, np.arange(n)) and np.array_equal(np.sort(gid), np.arange(n))          # a real permutation
    xi = B.libm_deviates(gid, B.STEP0, 20)
    ref, _ = B.run_cpu(c, xyz, cell0, xi, reflect=1, zfold=0)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    cell, vel, done = cell0.copy(), np.zeros((n, 3)), 0
    for k in B.CHECKPOINTS:
        st = cw.step(x, y, z, cell, c.dt, k - done, c.tables, c.U, vel_out=vel, nthreads=cw.max_threads, D=c.D, gid=gid,
                     step0=B.STEP0 + done, seed=B.SEED)
        done = k
        s = ref[k]
        assert np.array_equal(cell, s.cell), (name, k)
        assert np.array_equal(_bits(np.stack([x, y, z], 1)), _bits(s.xyz)), (name, k)
        assert np.array_equal(_bits(vel), _bits(s.vel)), (name, k)
        assert [int(v) for v in st] == s.stats[:3], (name, k, st, s.stats)
    assert ref[20].stats[1] > 0 and (ref[20].cell == B.CELL_FROZEN).sum() == sum(i < n for i in B.START_DEAD)


@pytest.mark.parametrize("name", B.MESHES_3D + B.MESHES_THIN)
def test_no_reflect_loses_exactly_who_would_reflect(name, oracle_libs):
    c, cw = B.case(name), B.cellwalk()
    n = 4000
    xyz, cell0, gid = B.cloud(name, n)
    xi = B.libm_deviates(gid, B.STEP0, 6)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    cell = cell0.copy()
    met_a_wall = 0
    for cyc in range(6):
        live = cell >= 0
        x0, y0, z0, c0 = x.copy(), y.copy(), z.copy(), cell.copy()
        diag = np.zeros((1, n, 3), np.int32)
        cw.step_given(x0, y0, z0, c0, c.dt, 1, c.tables, c.U, c.sigma, xi[cyc:cyc + 1], reflect=0, nthreads=cw.max_threads)
        cw.step_given(x, y, z, cell, c.dt, 1, c.tables, c.U, c.sigma, xi[cyc:cyc + 1], reflect=1, nthreads=cw.max_threads, diag=diag)
        walls = diag[0, :, 1] > 0
        assert np.array_equal(c0 == B.CELL_LOST, walls & live), (name, cyc)
        met_a_wall += int(walls.sum())
        # whoever met no wall is where the reflecting run put it; whoever did is at P + disp = P + (dt U + sigma xi), to a rounding
        same = live & ~walls
        assert np.array_equal(_bits(np.stack([x0, y0, z0], 1)[same]), _bits(np.stack([x, y, z], 1)[same])) and np.array_equal(c0[same], cell[same])
    assert met_a_wall > 0.01 * n


def test_no_reflect_moves_the_lost_particle_to_the_end_of_its_displacement(oracle_libs):
    c, cw = B.case("graded box"), B.cellwalk()
    n = 4000
    xyz, cell0, gid = B.cloud("graded box", n)
    xi = B.libm_deviates(gid, B.STEP0, 1)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    cell = cell0.copy()
    cw.step_given(x, y, z, cell, c.dt, 1, c.tables, c.U, c.sigma, xi, reflect=0, nthreads=cw.max_threads)
    lost = cell == B.CELL_LOST
    assert lost.sum() > 0.01 * n
    want = xyz[lost] + (c.dt * c.U[cell0[lost]] + c.sigma * xi[0][lost])
    assert np.abs(np.stack([x, y, z], 1)[lost] - want).max() <= 1e-15 * float(np.abs(c.hi - c.lo).max()) * 8
    outside = ((want < c.lo) | (want > c.hi)).any(1)
    assert outside.all()                                                   # a convex box: beyond the wall it stopped at
    # and the next cycle freezes it where it is
    x1, y1, z1 = x.copy(), y.copy(), z.copy()
    cw.step_given(x, y, z, cell, c.dt, 1, c.tables, c.U, c.sigma, xi, reflect=0, nthreads=cw.max_threads)
    assert (cell[lost] == B.CELL_FROZEN).all() and np.array_equal(x[lost], x1[lost]) and np.array_equal(z[lost], z1[lost])


def test_fold_against_the_reference_order_on_pitzdaily(oracle_libs):
    """zfold = 1 against zfold = 0, one cycle at 100 x the tutorial's D: same cell for at least 0.99999 of the cloud and positions
    within 1e-12 where the cell is the same; as many mirrorings as the reference order counts reflections, to the few that differ."""
    c, cw = B.case("pitzDaily"), B.cellwalk()
    n = 10000
    xyz, cell0, gid = B.cloud("pitzDaily", n)
    xi = B.libm_deviates(gid, B.STEP0, 1)
    res = {}
    for zfold in (0, 1):
        out, diag = B.run_cpu(c, xyz, cell0, xi, reflect=1, zfold=zfold, checkpoints=(1,))
        res[zfold] = (out[1], diag[0])
    a, b = res[0][0], res[1][0]
    same = a.cell == b.cell
    assert same.mean() >= 0.99999, float(same.mean())
    assert np.abs(a.xyz - b.xyz)[same].max() < 1e-12
    assert (res[1][1][:, 2] > 0).mean() > 0.2 and (res[1][1][:, 2] >= 2).sum() > 0          # a fifth is mirrored, some of them twice
    assert abs(a.stats[1] - b.stats[1]) <= 3e-4 * n
    zlo, zhi = c.lo[2], c.hi[2]
    assert b.xyz[:, 2].min() >= zlo and b.xyz[:, 2].max() <= zhi
    # the stored velocity's z flips once per mirroring: the side walls of this mesh have nz == 0 exactly and leave it alone
    live = cell0 >= 0
    sign = np.where(res[1][1][:, 2] % 2 == 1, -1.0, 1.0)
    assert np.array_equal(b.vel[live, 2], (sign * c.U[np.maximum(cell0, 0), 2])[live])
    assert np.array_equal(_bits(a.vel[same & live]), _bits(b.vel[same & live]))              # ... as the reference order leaves it


@pytest.mark.parametrize("name", B.MESHES_3D + B.MESHES_THIN)
def test_the_inputs_go_through_the_hard_paths(name, oracle_libs):
    """What tests/test_gpu_brownian_cycle.py asserts again on the device's deviates: over the 20 cycles the CPU statement shows face
    crossings, wall reflections, two walls in one cycle, three crossings in one cycle, losses without reflection, and on the
    meshes one cell thick in z mirrorings, some of them double."""
    c = B.case(name)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    xi = B.libm_deviates(gid, B.STEP0, 20)
    thin = name in B.MESHES_THIN
    out, diag = B.run_cpu(c, xyz, cell0, xi, reflect=1, zfold=1 if thin else 0)
    hp = B.hard_paths(diag)
    print("MEASURED %s | sigma / h %.2f | %s" % (name, c.sigma / c.h, hp))
    assert hp["crossing"] >= 0.10 and hp["reflecting"] >= 0.01 and hp["three_hops"] >= 1
    if thin:
        assert hp["folded"] >= 0.20 and hp["folded_twice"] >= 1
    else:
        assert hp["two_walls"] >= 1
        out0, _ = B.run_cpu(c, xyz, cell0, xi, reflect=0)
        assert (out0[20].cell < 0).mean() >= 0.01
