"""GPU: the round's bookkeeping around the face blocks of the flat walk's body without z (csrc/cpf_stream.hip, stream_body under ZSET:
the loop lookup's trip as a hand-written block, csrc/cpf_stream_ops.h lookup_loop_asm; outcome_flat, the
visit's outcome applied behind the busy lanes' region and the j test in the wall branch), BIT FOR BIT in x, y, the
cell and the stored velocity against two statements of the same cycle, the way tests/test_gpu_flat_face.py does it:

  1. the CPU statement, oracle/cellwalk.c (CellWalk.step_given(xi = None) through tests/browniancycle.py, run_cpu);
  2. the same library with option "flat_z" 0: the three-coordinate body, which none of the three touches.

What runs: cpf_step on the context's own cloud, never re-sorted.  One cycle of dt = 0 settles z; the launches behind it -- one
cycle, three cycles, and launches of zero cycles between and behind them, all with CPF_STEP_FUSE_CYCLES -- report
step_kernel_stream_flat<REFLECT, STORE_VEL, false, 8>, asserted after each launch.

THE LOOP LOOKUP (8) is the planner's choice from 128 particles per cell of the mesh (csrc/cpf_stream.hip, stream_lookup_mode; the
count is the cloud's size, frozen slots included, and "stream_lookup" cannot name 8): on box_mesh(2, 2, 1), the smallest mesh of
tests/test_gpu_flat_face.py, from 512.  A cloud of 1, 63, 64, 65 or 200 particles is therefore that many particles -- ordered by
cell, in the cloud's first tiles -- followed by 512 frozen slots: a first tile with one busy lane, tiles one lane short of full,
full, one lane over, partial last tiles of 1, 63, 0, 1 and 8 lanes, and always far fewer tiles than the chip has waves.  One
case runs the fixed compare (9) on 200 particles without the filler: what is not the lookup's is in that entry too.

The other shapes, all through the loop lookup:
  * every tile in one cell (four tiles per cell): one trip per round, a hit from the second tile on;
  * box_mesh(6, 5, 1) with 4 096 + 13 particles as drawn: about 27 distinct cells in a tile against six record slots and four
    requests per round, so the first round of a tile leaves 32 lanes or more without a slot -- asserted on the cloud -- and runs the
    gather visit and its exit point; in later rounds fewer are left and they sit the round out;
  * a cloud whose every particle is within one step of a wall, with reflection and with CPF_STEP_NO_REFLECT;
  * a corner: the cell at (2, 2) moves its particles by (11, 9.5), five and a half domain widths -- five bounces, then lost -- while
    its diagonal neighbour moves them by (-3, 1/8): two bounces, alive (the j test in the wall branch);
  * CPF_STEP_STORE_VEL (the entry with one wave per SIMD; the mirrored velocity)."""
import functools

import numpy as np
import pytest

import browniancycle as B
import test_gpu_flat_face as F
from cudaparticlesfoam_amd import _lib as L

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 3)
CHECKPOINTS = (1, 4)
FLAT = "cpf::step_kernel_stream_flat<%s, %s, false, %d>"
STREAM = "cpf::step_kernel_stream<false, %s, %s, false, %d>"
FILLER = 512                      # 128 particles per cell of box_mesh(2, 2, 1)


def _tf(b):
    return "true" if b else "false"


@functools.lru_cache(maxsize=None)
def corner_case():
    """box_mesh(2, 2, 1) with a field that drives its particles into the walls (the field of tests/test_gpu_flat_face.py points
    inwards in every cell): dt = 1 / 8 and, by the cell's place, displacements of (-3, 1 / 8) at the origin -- two bounces --,
    (1 / 4, -1 / 8) right of it, (1 / 16, -1 / 4) above it and (11, 9.5) in the cell at the corner (2, 2): five bounces, then lost"""
    base = F.case("four cells")
    centres, _ = base.mesh.cell_centres_volumes()
    U = np.zeros((base.mesh.n_cells, 3))
    for k, (x, y, _) in enumerate(centres):
        U[k, :2] = {(False, False): (-24.0, 1.0), (True, False): (2.0, -1.0), (False, True): (0.5, -2.0), (True, True): (88.0, 76.0)}[(x > 1, y > 1)]
    return F._case("four cells, corner", base.mesh, U, 0.125)


def _freeze(a):
    for x in a:
        x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sized_cloud(k, filler):
    """k particles ordered by cell, then `filler` frozen slots"""
    xyz, cell = (np.array(a) for a in F.cloud("four cells", k + filler, False))
    o = np.argsort(cell[:k], kind="stable")
    xyz[:k], cell[:k] = xyz[:k][o], cell[:k][o]
    cell[k:] = B.CELL_FROZEN
    if k == 1:
        assert cell[0] >= 0
    return _freeze((xyz, cell))


@functools.lru_cache(maxsize=None)
def one_cell_tiles():
    """1 024 particles, 256 of each cell: every tile sits in one cell"""
    xyz, cell = F.cloud("four cells", 2400, True)
    keep = np.concatenate([np.nonzero(cell == c)[0][:256] for c in range(4)])
    assert keep.size == 1024
    xyz, cell = np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(cell[keep])
    assert all(np.unique(cell[t:t + 64]).size == 1 for t in range(0, 1024, 64))
    return _freeze((xyz, cell))


@functools.lru_cache(maxsize=None)
def wall_cloud():
    """1 024 particles of corner_case(), every one within a step of a wall it moves towards: those of the cell above the origin, which
    would cross into the cell below, are moved into the cell right of the origin, and every particle there to within three quarters of its step
    (1 / 4, -1 / 8) of the walls x = 2 and y = 0; the other two cells reach a wall from anywhere"""
    c = corner_case()
    xyz, cell = (np.array(a) for a in F.cloud("four cells", 1024, True))
    up = (xyz[:, 0] < 1) & (xyz[:, 1] > 1)
    xyz[up, 0] += 1.0; xyz[up, 1] -= 1.0
    right = (xyz[:, 0] > 1) & (xyz[:, 1] < 1)
    i = np.arange(xyz.shape[0])
    xyz[right, 0] = (2.0 - 0.75 * 0.25 * (1 + i % 4) / 4.0)[right]
    xyz[right, 1] = (0.75 * 0.125 * (1 + (i // 4) % 4) / 4.0)[right]
    live = cell >= 0
    cell[live] = F._locate(c, xyz)[live]
    assert (cell[live] >= 0).all()
    o = np.argsort(cell, kind="stable")
    return _freeze((np.ascontiguousarray(xyz[o]), np.ascontiguousarray(cell[o])))


_state = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for ctx in _state.values():
        ctx.close()
    _state.clear()


def _ctx(c, make):
    if c.name not in _state:
        ctx = make()
        ctx.set_mesh(c.mesh); ctx.set_velocity(c.U); ctx.synchronize()
        _state[c.name] = ctx
    return _state[c.name]


def gpu_run(ctx, c, xyz, cell0, lookup, flat_z, reflect, sv):
    """{cycles: (xyz, cell, vel or None)} behind launches of 1 and 3 cycles on a cloud whose z one cycle of dt = 0 has settled, with
    launches of zero cycles in front of, between and behind them"""
    flags = L.STEP_FUSE_CYCLES | (0 if reflect else L.STEP_NO_REFLECT) | (L.STEP_STORE_VEL if sv else 0)
    want = (FLAT % (_tf(reflect), _tf(sv), lookup)) if flat_z else (STREAM % (_tf(reflect), _tf(sv), lookup))
    out = {}
    for k, v in (("stats", 0), ("sort_interval", 0), ("flat_z", flat_z)):
        ctx.set_option(k, v)
    try:
        ctx.set_particles(xyz, cell0)
        ctx.step(0.0, 0.0, 1, flags)

        def snapshot():
            if sv:
                xyzw, cell, vel = ctx.get_particles(want_vel=True)
                return xyzw[:, :3].copy(), cell.copy(), vel[:, :3].copy()
            xyzw, cell = ctx.get_particles()
            return xyzw[:, :3].copy(), cell.copy(), None

        def zero_cycles(before):
            ctx.step(c.dt, 0.0, 0, flags)
            assert ctx.step_kernel_name(0.0, flags) == want
            p, cell, _ = snapshot()
            # (a particle lost in the launch before is frozen by the next one, of however many cycles: w = 0 from then on)
            same_cell = np.where(before[1] == B.CELL_LOST, B.CELL_FROZEN, before[1])
            assert np.array_equal(F._bits(p), F._bits(before[0])) and np.array_equal(cell, same_cell), "a launch of zero cycles moved somebody"
        zero_cycles(snapshot())
        done = 0
        for k in LAUNCHES:
            ctx.step(c.dt, 0.0, k, flags)
            name = ctx.step_kernel_name(0.0, flags)
            assert name == want, (name, want)
            done += k
            out[done] = snapshot()
            zero_cycles(out[done])
    finally:
        for k, v in (("stats", 1), ("sort_interval", 50), ("flat_z", 1)):
            ctx.set_option(k, v)
    return out


def check(c, xyz, cell0, lookup, make, what, reflect=1, sv=0):
    ctx = _ctx(c, make)
    ref, diag = B.run_cpu(c, xyz, cell0, None, reflect=reflect, checkpoints=CHECKPOINTS, U=c.U)
    got = gpu_run(ctx, c, xyz, cell0, lookup, 1, reflect, sv)
    three = gpu_run(ctx, c, xyz, cell0, lookup, 0, reflect, sv)
    live = np.asarray(cell0) >= 0                     # (a frame holds the velocities of the particles that launch stepped)
    for k in CHECKPOINTS:
        (p, cell, vel), (p3, cell3, vel3), s = got[k], three[k], ref[k]
        for other, oc, ov, who in ((p3, cell3, vel3, "the three-coordinate body"), (s.xyz, s.cell, s.vel, "the CPU")):
            bad = np.nonzero(cell != oc)[0]
            assert bad.size == 0, (what, k, "cells differ from " + who, bad.size, bad[:5], cell[bad[:5]], oc[bad[:5]])
            bad = np.nonzero((F._bits(p[:, :2]) != F._bits(other[:, :2])).any(1))[0]
            assert bad.size == 0, (what, k, "x, y differ from " + who, bad.size, bad[:5], p[bad[:5]], other[bad[:5]])
            if sv:
                bad = np.nonzero((F._bits(vel[live]) != F._bits(ov[live])).any(1))[0]
                assert bad.size == 0, (what, k, "stored velocities differ from " + who, bad.size, bad[:5], vel[live][bad[:5]], ov[live][bad[:5]])
        live = cell >= 0
    return ref, diag, got


@pytest.mark.parametrize("k", [1, 63, 64, 65, 200])
def test_small_clouds_through_the_loop_lookup(k, gpu_ctx_factory, oracle_libs):
    xyz, cell0 = sized_cloud(k, FILLER)
    _, diag, _ = check(corner_case(), xyz, cell0, 8, gpu_ctx_factory, "%d particles + %d frozen slots" % (k, FILLER))
    assert (diag[:, k:, 0] == 0).all() and (diag[0, :k, 0] > 0).sum() >= k - 3      # the filler never walks; the particles do
    if k >= 63:
        hp = B.hard_paths(diag)
        print("MEASURED k=%d: %s" % (k, hp))
        assert hp["crossing"] >= 0.05 and hp["reflecting"] >= 0.005, hp


def test_small_cloud_through_the_fixed_compare(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = sized_cloud(200, 0)
    check(corner_case(), xyz, cell0, 9, gpu_ctx_factory, "200 particles, fixed compare")


def test_every_tile_in_one_cell(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = one_cell_tiles()
    _, diag, _ = check(corner_case(), xyz, cell0, 8, gpu_ctx_factory, "every tile in one cell")
    assert B.hard_paths(diag)["crossing"] >= 0.05


def test_more_cells_in_a_round_than_slots(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = F.cloud("unit box", 4096 + 13, False)
    # a tile's first round places the first four distinct cells of its busy lanes; 32 lanes or more are left: the gather visit
    left = []
    for t in range(0, 4096, 64):
        cells = cell0[t:t + 64]
        first4 = list(dict.fromkeys(int(x) for x in cells if x >= 0))[:4]
        left.append(int(((cells >= 0) & ~np.isin(cells, first4)).sum()))
        assert np.unique(cells[cells >= 0]).size > 6
    assert min(left) >= 32, min(left)
    _, diag, _ = check(F.case("unit box"), xyz, cell0, 8, gpu_ctx_factory, "as drawn: gather visits, lanes sitting out")
    hp = B.hard_paths(diag)
    print("MEASURED as drawn:", hp)
    assert hp["crossing"] >= 0.05 and hp["reflecting"] >= 0.005, hp


@pytest.mark.parametrize("reflect", [1, 0], ids=["reflect", "no-reflect"])
def test_within_one_step_of_a_wall(reflect, gpu_ctx_factory, oracle_libs):
    xyz, cell0 = wall_cloud()
    ref, diag, _ = check(corner_case(), xyz, cell0, 8, gpu_ctx_factory, "near a wall, reflect %d" % reflect, reflect=reflect)
    live = cell0 >= 0
    if reflect:
        assert (diag[0, live, 1] >= 1).all()                      # every particle met a wall in its first cycle
        assert (ref[1].cell[live & ~((xyz[:, 0] > 1) & (xyz[:, 1] > 1))] >= 0).all()
    else:
        assert (ref[1].cell[live] == B.CELL_LOST).all()           # ... and without reflection that is the end of it


def test_five_bounces_in_a_corner(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = F.cloud("four cells", 1024, True)
    ref, diag, _ = check(corner_case(), xyz, cell0, 8, gpu_ctx_factory, "corner")
    live = cell0 >= 0
    fast = live & (xyz[:, 0] > 1) & (xyz[:, 1] > 1)
    slow = live & (xyz[:, 0] < 1) & (xyz[:, 1] < 1)
    assert fast.sum() >= 100 and slow.sum() >= 100
    walls = diag[0, :, 1]
    assert (walls[fast] == 5).all() and (ref[1].cell[fast] == B.CELL_LOST).all(), (walls[fast][:8], ref[1].cell[fast][:8])
    assert (walls[slow] == 2).all() and (ref[1].cell[slow] >= 0).all(), (walls[slow][:8], ref[1].cell[slow][:8])
    assert (ref[4].cell[fast] == B.CELL_FROZEN).all()             # lost in the first cycle: frozen from the second on


def test_stored_velocities(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = wall_cloud()
    check(corner_case(), xyz, cell0, 8, gpu_ctx_factory, "stored velocities", sv=1)
