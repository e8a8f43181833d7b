"""CPU: oracle/cellwalk.c's cycle WITHOUT the kick as cw_step_given states it (CellWalk.step_given(xi = None)) -- the statement the
unkicked kernels are compared with bit for bit in tests/test_gpu_plain_cycle.py:

* with reflect = 1 it IS cw_step(D = 0): one body, the same bits, stored velocities and statistics included, on every mesh and in
  both fields (the case's random one and U0, the one with exact zeros);
* the inputs the GPU tests run on do go through the hard paths (tests/browniancycle.py, hard_paths), asserted on the statement's own
  per-particle-cycle counters;
* the clouds ordered by cell hold what the wave-uniform paths of the kernels need: a whole 64-particle tile in at-rest cells, on the
  meshes of boxes a whole tile in U.x == +-0 cells of which a lane crosses a y or z face, and on the chamfered grid driven into a
  corner a tile of which more than 16 lanes reflect in one cycle."""
import numpy as np
import pytest

import browniancycle as B

MESHES = B.MESHES_3D + ("thin box",)
N = 6000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("field", ["U", "U0"])
@pytest.mark.parametrize("name", MESHES)
def test_step_given_without_deviates_is_cw_step_without_diffusion(name, field, oracle_libs):
    c, cw = B.case(name), B.cellwalk()
    xyz, cell0, gid = B.cloud(name, N, sort=True)
    U = c.field(field)
    ref, _ = B.plain_ref(name, field, N, True, 1)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    cell, vel, done = cell0.copy(), np.zeros((N, 3)), 0
    for k in B.CHECKPOINTS:
        st = cw.step(x, y, z, cell, c.dt, k - done, c.tables, U, vel_out=vel, nthreads=cw.max_threads)
        done = k
        s = ref[k]
        assert np.array_equal(cell, s.cell), (name, k)
        assert np.array_equal(_bits(np.stack([x, y, z], 1)), _bits(s.xyz)), (name, k)
        assert np.array_equal(_bits(vel), _bits(s.vel)), (name, k)
        assert [int(v) for v in st] == s.stats[:3], (name, k, st, s.stats)
    assert ref[20].stats[1] > 0 and (ref[20].cell == B.CELL_FROZEN).sum() >= len(B.START_DEAD)
    assert c.sigma > 0                       # (handed to step_given all the same: without deviates it must not count)


def test_the_second_field_is_what_it_says():
    for name in MESHES:
        c = B.case(name)
        n, third = c.mesh.n_cells, c.mesh.n_cells // 3
        assert third >= 8
        assert not c.U0[:third].any() and not c.U0[n - third:, 0].any()
        assert np.signbit(c.U0[:third]).any() and not np.signbit(c.U0[:third]).all()              # +0.0 and -0.0
        assert np.signbit(c.U0[n - third:, 0]).any() and not np.signbit(c.U0[n - third:, 0]).all()
        assert np.array_equal(_bits(c.U0[third:n - third]), _bits(c.U[third:n - third]))
        assert np.array_equal(_bits(c.U0[n - third:, 1:]), _bits(c.U[n - third:, 1:])) and c.U0[n - third:, 1:].all()


@pytest.mark.parametrize("name", MESHES)
def test_the_inputs_go_through_the_hard_paths(name, oracle_libs):
    """What tests/test_gpu_plain_cycle.py asserts again before it compares: over the 20 cycles of the reflecting run a tenth of
    the live particle-cycles cross a face, a hundredth meet a wall, some meet two walls in a cycle and some cross three faces in
    a cycle (thin box: the first three; no three-crossing cycle turns up there), and the run without reflection leaves at least
    a hundredth of the cloud lost or frozen."""
    c = B.case(name)
    _, diag = B.plain_ref(name, "U", N, True, 1)
    hp = B.hard_paths(diag)
    lost = float((B.plain_ref(name, "U", N, True, 0)[0][20].cell < 0).mean())
    print("MEASURED %s | dt |U|max / h %.2f | %s | lost or frozen without reflection %.3f" % (name, c.dt * np.abs(c.U).max() / c.h, hp, lost))
    assert hp["crossing"] >= 0.10 and hp["reflecting"] >= 0.01 and hp["two_walls"] >= 1
    assert hp["folded"] == 0                                               # (no kick, no fold)
    if name != "thin box":
        assert hp["three_hops"] >= 1
        assert lost >= 0.01


@pytest.mark.parametrize("name", B.MESHES_3D)
def test_whole_tiles_in_at_rest_cells_and_in_cells_without_an_x_component(name, oracle_libs):
    c = B.case(name)
    _, cell0, _ = B.cloud(name, N, sort=True)
    ref, diag = B.plain_ref(name, "U0", N, True, 1)
    rest = B.at_rest_tiles(c, cell0)
    assert rest.size >= 1
    # ... and they are at rest: one visit per cycle, no wall, the same bits after 20 cycles
    lanes = (rest[:, None] * 64 + np.arange(64)).ravel()
    xyz, _, _ = B.cloud(name, N, sort=True)
    assert (diag[:, lanes, 0] == 1).all() and not diag[:, lanes, 1].any()
    assert np.array_equal(_bits(ref[20].xyz[lanes]), _bits(xyz[lanes])) and np.array_equal(ref[20].cell[lanes], cell0[lanes])
    zx = B.zero_x_crossing_tiles(c, cell0, diag)
    print("MEASURED %s | %d tiles | %d at rest | %d in U.x == 0 cells with a crossing in the first cycle" % (name, N // 64, rest.size, zx.size))
    if name in ("graded box", "refined box"):
        assert zx.size >= 1
        lanes = (zx[:, None] * 64 + np.arange(64)).ravel()
        assert np.array_equal(_bits(ref[1].xyz[lanes, 0]), _bits(xyz[lanes, 0]))                  # nobody there moved in x


def test_more_than_16_lanes_of_a_tile_reflect_in_one_cycle_on_the_chamfered_grid(oracle_libs):
    _, diag = B.plain_ref("chamfered", "Ucorner", N, True, 1)
    most = B.most_lanes_of_a_tile_reflecting(diag)
    print("MEASURED chamfered, driven into a corner | most lanes of a tile reflecting in one cycle: %d" % most)
    assert most > 16
