"""GPU: what the round of the flat walk's body without z leaves unselected and untested since round 15 (csrc/cpf_walk.h,
trace_lds4_flat's EXIT_ALWAYS: the exit point computed for every visiting lane, `best` unset until a face is accepted;
csrc/cpf_stream.hip: one test in front of miss jobs, hook and counted wait; csrc/cpf_stream_ops.h, wait_vmcnt_flat: the counted wait as
one block), BIT FOR BIT in x, y and the cell against two statements of the same cycle, the way tests/test_gpu_flat_lookup.py does it:

  1. the CPU statement, oracle/cellwalk.c (tests/browniancycle.py, run_cpu);
  2. the same library with option "flat_z" 0: the three-coordinate body, which has none of the three.

What runs is test_gpu_flat_lookup's gpu_run: one cycle of dt = 0 settles z, then launches of 0, 1, 0, 3 and 0 cycles, each reporting
step_kernel_stream_flat<REFLECT, false, false, 8> (asserted there after every launch); checkpoints behind 1 and 4 cycles.

THE LOOP LOOKUP (8) needs 128 particles per cell of the mesh, frozen slots included: every cloud is its live particles IN FRONT of that
many frozen slots.  The cases, each a property of the cloud that is asserted on the cloud or on the CPU statement's per-lane counters:

  1. box_mesh(8, 1, 1), 63 live particles dealt over 7 cells lane by lane: a round places four cells, so 27 lanes of the first tile's
     first round are without a slot -- fewer than 32: they sit the round out and advect in a later round of the cycle;
  2. the same mesh, 64 particles over 8 cells: 32 lanes without a slot, which is the gather visit (and its exit point);
  3. box_mesh(2, 2, 1): a cloud within one step of the walls, with and without reflection; five bounces in a corner; and tiles in
     which only some lanes hit a wall (the wall branch under a partial mask);
  4. box_mesh(64, 1, 1), a displacement of 60 cells: the hop cap (50) ends the cycle in the fiftieth cell downstream;
  5. lanes that visit and accept no face -- the lanes whose exit point is now computed from dTmin = 2 and must not be seen -- next to
     lanes that cross, in one tile; and partial last tiles of 1 particle (behind 0 and behind 64 more: 1 and 65 particles), with lost
     and frozen lanes among the live ones;
  6. NaN and infinities in x or y of live lanes: no face is accepted, the exit point is NaN until the cycle's move overwrites it.
     The CPU's default NaN and the GPU's differ in the sign bit: cell and NaN-ness against the CPU, bits against "flat_z" 0."""
import functools

import numpy as np
import pytest

import browniancycle as B
import test_gpu_flat_face as F
import test_gpu_flat_lookup as K

pytestmark = pytest.mark.gpu

CHECKPOINTS = K.CHECKPOINTS
HOP_CAP = 50                          # csrc/cpf_device.h, kMaxHops


@functools.lru_cache(maxsize=None)
def row_case(nx):
    """box_mesh(nx, 1, 1), unit cells, dt = 1 / 8.  nx = 8: per cell a dyadic field that crosses into both neighbours and meets the
    walls y = 0 and y = 1.  nx = 64: cell 0 moves its particles by 60 cells, every other cell by 1 / 4."""
    from cudaparticlesfoam_amd.cases import box_mesh
    mesh = box_mesh(nx, 1, 1)
    centres, _ = mesh.cell_centres_volumes()
    i = np.floor(centres[:, 0]).astype(int)
    U = np.zeros((mesh.n_cells, 3))
    if nx == 8:
        ux = np.array([4.0, -2.0, 6.0, -4.0, 2.0, -6.0, 3.0, -3.0])
        uy = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0, -3.0])
        U[:, 0], U[:, 1] = ux[i], uy[i]
    else:
        U[:, 0] = np.where(i == 0, 480.0, 2.0)
        U[:, 1] = np.where(i == 0, 0.0, 0.25)
    return F._case("row of %d" % nx, mesh, U, 0.125)


def _frozen(a):
    for x in a:
        x.setflags(write=False)
    return a


def with_filler(c, live_xyz, tail_xyz=None, dead=()):
    """live particles (cells from the CPU statement), then frozen slots up to 128 per cell of the mesh and a whole number of tiles, then the
    tail's particles; dead: {index: state} among the live ones"""
    n_fill = 128 * c.mesh.n_cells
    n_fill += -(live_xyz.shape[0] + n_fill) % 64
    parts = [live_xyz, np.tile([[0.5, 0.5, 0.5]], (n_fill, 1))] + ([tail_xyz] if tail_xyz is not None else [])
    xyz = np.ascontiguousarray(np.concatenate(parts))
    probe = np.where(np.isfinite(xyz), xyz, 0.5)
    cell = F._locate(c, probe)
    assert (cell >= 0).all()
    cell[live_xyz.shape[0]:live_xyz.shape[0] + n_fill] = B.CELL_FROZEN
    for k, state in dict(dead).items():
        cell[k] = state
    return _frozen((xyz, cell))


def dealt(c, n_live, n_cells, seed):
    """n_live particles, lane k in cell k mod n_cells of the row, anywhere inside it"""
    rng = np.random.default_rng(seed)
    k = np.arange(n_live)
    return np.stack([(k % n_cells) + rng.uniform(0.0625, 0.9375, n_live), rng.uniform(0.0625, 0.9375, n_live), np.full(n_live, 0.5)], 1)


def without_slot(cell):
    """lanes of the first tile that its first round leaves without a record slot: four requests per round, in lane order"""
    t = cell[:64]
    first4 = list(dict.fromkeys(int(x) for x in t if x >= 0))[:4]
    return int(((t >= 0) & ~np.isin(t, first4)).sum())


def check(c, xyz, cell0, make, what, reflect=1):
    ctx = K._ctx(c, make)
    ref, diag = B.run_cpu(c, xyz, cell0, None, reflect=reflect, checkpoints=CHECKPOINTS, U=c.U)
    got = K.gpu_run(ctx, c, xyz, cell0, 8, 1, reflect, 0)
    three = K.gpu_run(ctx, c, xyz, cell0, 8, 0, reflect, 0)
    finite = np.isfinite(xyz[:, :2]).all(1)
    for k in CHECKPOINTS:
        (p, cell, _), (p3, cell3, _), s = got[k], three[k], ref[k]
        bad = np.nonzero(cell != cell3)[0]
        assert bad.size == 0, (what, k, "cells differ from the three-coordinate body", bad.size, bad[:5], cell[bad[:5]], cell3[bad[:5]])
        bad = np.nonzero((F._bits(p[:, :2]) != F._bits(p3[:, :2])).any(1))[0]
        assert bad.size == 0, (what, k, "x, y differ from the three-coordinate body", bad.size, bad[:5], p[bad[:5]], p3[bad[:5]])
        bad = np.nonzero(cell != s.cell)[0]
        assert bad.size == 0, (what, k, "cells differ from the CPU", bad.size, bad[:5], cell[bad[:5]], s.cell[bad[:5]])
        bad = np.nonzero((F._bits(p[finite, :2]) != F._bits(s.xyz[finite, :2])).any(1))[0]
        assert bad.size == 0, (what, k, "x, y differ from the CPU", bad.size, bad[:5], p[finite][bad[:5]], s.xyz[finite][bad[:5]])
        assert np.array_equal(np.isnan(p[~finite, :2]), np.isnan(s.xyz[~finite, :2])), (what, k, "NaN lanes")
    return ref, diag, got


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for ctx in K._state.values():
        ctx.close()
    K._state.clear()


def test_lanes_without_a_slot_sit_out(gpu_ctx_factory, oracle_libs):
    c = row_case(8)
    xyz, cell0 = with_filler(c, dealt(c, 63, 7, 5))
    assert without_slot(cell0) == 27 and np.unique(cell0[:63]).size == 7
    _, diag, _ = check(c, xyz, cell0, gpu_ctx_factory, "63 over 7 cells")
    hp = B.hard_paths(diag)
    print("MEASURED 63 over 7:", hp)
    assert hp["crossing"] >= 0.05 and hp["reflecting"] >= 0.005, hp


def test_gather_visit(gpu_ctx_factory, oracle_libs):
    c = row_case(8)
    xyz, cell0 = with_filler(c, dealt(c, 64, 8, 6))
    assert without_slot(cell0) == 32 and np.unique(cell0[:64]).size == 8
    _, diag, _ = check(c, xyz, cell0, gpu_ctx_factory, "64 over 8 cells")
    hp = B.hard_paths(diag)
    print("MEASURED 64 over 8:", hp)
    assert hp["crossing"] >= 0.05 and hp["reflecting"] >= 0.005, hp


@pytest.mark.parametrize("reflect", [1, 0], ids=["reflect", "no-reflect"])
def test_within_one_step_of_a_wall(reflect, gpu_ctx_factory, oracle_libs):
    xyz, cell0 = K.wall_cloud()
    ref, diag, _ = check(K.corner_case(), xyz, cell0, gpu_ctx_factory, "near a wall, reflect %d" % reflect, reflect=reflect)
    live = cell0 >= 0
    if reflect:
        assert (diag[0, live, 1] >= 1).all()
    else:
        assert (ref[1].cell[live] == B.CELL_LOST).all()


def test_five_bounces_and_tiles_with_some_lanes_on_a_wall(gpu_ctx_factory, oracle_libs):
    xyz, cell0 = F.cloud("four cells", 1024, True)
    ref, diag, _ = check(K.corner_case(), xyz, cell0, gpu_ctx_factory, "corner")
    live = cell0 >= 0
    fast = live & (xyz[:, 0] > 1) & (xyz[:, 1] > 1)
    assert fast.sum() >= 100
    walls = diag[0, :, 1]
    assert (walls[fast] == 5).all() and (ref[1].cell[fast] == B.CELL_LOST).all(), (walls[fast][:8], ref[1].cell[fast][:8])
    # tiles in which some live lanes met a wall in the first cycle and others did not
    hit = B.tiles(walls > 0) & B.tiles(live)
    miss = B.tiles(walls == 0) & B.tiles(live)
    mixed = int((hit.any(1) & miss.any(1)).sum())
    print("MEASURED tiles with some lanes on a wall:", mixed)
    assert mixed >= 2, mixed


def test_hop_cap(gpu_ctx_factory, oracle_libs):
    c = row_case(64)
    rng = np.random.default_rng(9)
    n_live = 192
    k = np.arange(n_live)
    # two tiles of cell 0 -- lanes 3 mod 4 elsewhere, which end their cycle in their first or second visit -- and a third tile further down
    cx = np.where(k < 128, np.where(k % 4 == 3, 1 + k % 7, 0), 20 + k % 5)
    live = np.stack([cx + rng.uniform(0.0625, 0.9375, n_live), rng.uniform(0.0625, 0.6, n_live), np.full(n_live, 0.5)], 1)
    xyz, cell0 = with_filler(c, live)
    far = np.nonzero(cx == 0)[0]
    ref, diag, _ = check(c, xyz, cell0, gpu_ctx_factory, "hop cap")
    # 60 cells of displacement, 50 crossings allowed: the cell is the fiftieth downstream, the position is the end point all the same
    fiftieth = int(F._locate(c, np.array([[HOP_CAP + 0.5, 0.5, 0.5]]))[0])
    assert far.size == 96 and (ref[1].cell[far] == fiftieth).all(), (fiftieth, ref[1].cell[far][:8])
    assert (diag[0, far, 0] >= HOP_CAP).all(), diag[0, far, 0][:8]
    assert (ref[1].xyz[far, 0] > 60.0).all()


@pytest.mark.parametrize("tail", [1, 65])
def test_no_face_accepted_beside_crossings_and_partial_last_tile(tail, gpu_ctx_factory, oracle_libs):
    c = K.corner_case()
    src, _ = F.cloud("four cells", 2400, False)
    front = np.array(src[:65])
    rear = np.array(src[100:100 + tail])
    dead = {5: B.CELL_LOST, 40: B.CELL_FROZEN, 64: B.CELL_FROZEN}
    xyz, cell0 = with_filler(c, front, rear, dead)
    n = xyz.shape[0]
    assert n % 64 == 1 and (cell0[n - tail:] >= 0).all()
    if tail == 65:                                    # lost and frozen lanes in the tail's full tile too
        cell0 = np.array(cell0); cell0[n - 65 + 7] = B.CELL_LOST; cell0[n - 65 + 8] = B.CELL_FROZEN
        cell0.setflags(write=False)
    ref, diag, got = check(c, xyz, cell0, gpu_ctx_factory, "tail of %d" % tail)
    visits, walls = diag[0, :64, 0], diag[0, :64, 1]
    stay = int(((visits == 1) & (walls == 0)).sum())           # one visit, no face accepted
    go = int((visits - walls > 1).sum())                       # crossed a face
    print("MEASURED first tile: %d lanes accept no face, %d cross" % (stay, go))
    assert stay >= 8 and go >= 8, (stay, go)
    # the dead lanes kept their bytes
    for k in dead:
        assert got[4][1][k] < 0 and np.array_equal(F._bits(got[4][0][k]), F._bits(xyz[k]))


def test_non_finite_live_lanes(gpu_ctx_factory, oracle_libs):
    c = K.corner_case()
    src, _ = F.cloud("four cells", 2400, False)
    live = np.array(src[200:328])
    bad = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, np.inf), (-np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan), (np.inf, -np.inf)]
    for q, k in enumerate(range(1, 128, 4)):          # every fourth lane of both tiles; the lanes beside them cross and bounce
        bx, by = bad[q % 8]
        live[k, 0] = bx if not np.isfinite(bx) else live[k, 0]
        live[k, 1] = by if not np.isfinite(by) else live[k, 1]
    xyz, cell0 = with_filler(c, live)
    nonfinite = ~np.isfinite(xyz[:, :2]).all(1)
    assert nonfinite.sum() == 32 and (cell0[nonfinite] >= 0).all()
    ref, diag, got = check(c, xyz, cell0, gpu_ctx_factory, "non-finite")
    # no face is accepted with a NaN in the segment: one visit, the cell kept
    assert np.array_equal(got[4][1][nonfinite], cell0[nonfinite])
    assert (diag[0, nonfinite, 0] == 1).all()
