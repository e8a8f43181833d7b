"""GPU: the patch source (include/cpf.h "patch source"; csrc/cpf_inlet.hip).  A particle respawned on the source sits at
``source_positions_host`` of its own id, bit for bit, in the cell the initial locate gives that point; the candidates, the order, the
counters and the epoch are the box respawn's; a table on each side of the LDS staging limit; a warped boundary face; age stamps;
a whole recycled run (D = 0) against its CPU statement (tests/sourcepatch.py) bit for bit, on the box walk and on the flat walk."""
import re

import numpy as np
import pytest

import recycle as R
import sourcepatch as SP
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = R.N                                      # 10 007: a multiple of neither 64, 256 nor 1024
SEED = R.SEED
LDS_BOUNDS = 4096                            # csrc/cpf_inlet.hip, kSourceLdsBounds: larger tables are searched in global memory
DEPTH = (0.0, 0.5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(8, 3, 2)
    sink = _last_x_layer(mesh)
    faces = SP.boundary_faces_at_x0(mesh)
    tri, of = mesh.face_triangles(faces)
    assert sink.size == 6 and faces.size == 6 and tri.shape == (12, 3, 3)
    rec, hi = api.source_table_host(tri, None, DEPTH)
    return dict(mesh=mesh, sink=sink, xyz=pz.uniform_points(78, N, (0.0, 0.0, 0.0), (8.0, 3.0, 2.0)), tri=tri, rec=rec, hi=hi)


def _located(ctx, b, cell=None, source=True):
    ctx.set_mesh(b["mesh"]); ctx.set_seed(SEED)
    if source:
        ctx.set_source_triangles(b["tri"], None, DEPTH)
    ctx.set_particles(b["xyz"], cell)
    if cell is None:
        assert ctx.locate_initial() == 0
    return ctx.get_particles()


def _dev(a, offset=0, guard=None):
    """(whole tensor, its view from `offset` elements on) on cuda:0: the view starts 4 * offset bytes past a 16-byte boundary"""
    import torch
    parts = [np.full(offset, 3, a.dtype), a] + ([] if guard is None else [guard])
    whole = torch.from_numpy(np.concatenate(parts)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return whole, whole[offset:]


def _locate_dev(ctx, pts):
    """cpf_locate_initial_dev of the points: derived cell ids"""
    import torch
    n = pts.shape[0]
    t = [_dev(np.ascontiguousarray(pts[:, k]))[1] for k in range(3)]
    c = torch.full((max(n, 1),), -7, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.locate_initial_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), c.data_ptr(), n)
    ctx.synchronize()
    return c.cpu().numpy()[:n]


# ------------------------------------------------------------------------------------------------ 6. respawn, unlimited
def test_6_unlimited_respawn_puts_every_dead_particle_at_its_own_position(box, gpu_ctx_factory):
    mesh, rec, hi = box["mesh"], box["rec"], box["hi"]
    ctx = gpu_ctx_factory()
    xyzw0, cell0 = _located(ctx, box)
    got_rec, got_hi = ctx.source_table()
    assert np.array_equal(_bits(got_rec), _bits(rec)) and np.array_equal(got_hi, hi)
    ctx.set_sink_cells(box["sink"]); ctx.sink_apply()
    killed = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert killed.size == ctx.recycle_counts()["absorbed"] > 0.08 * N
    ctx.respawn_source()
    xyzw, cell = ctx.get_particles()
    want = api.source_positions_host(SEED, killed, 0, rec, hi)
    assert np.array_equal(_bits(xyzw[killed, :3]), _bits(want))
    assert (want[:, 0] >= 0.0).all() and (want[:, 0] <= 0.5).all() and np.unique(want[:, 0]).size > killed.size // 2
    assert np.array_equal(cell[killed], _locate_dev(ctx, want)) and (cell[killed] >= 0).all()
    others = np.setdiff1d(np.arange(N), killed)
    assert np.array_equal(_bits(xyzw[others]), _bits(xyzw0[others])) and np.array_equal(cell[others], cell0[others])
    assert ctx.recycle_counts() == dict(absorbed=killed.size, drawn=killed.size, placed=killed.size, epochs=1)
    # the epoch is the box respawn's: a box call between two source calls shifts the second one's epoch to 2
    first_layer = np.nonzero(mesh.cell_centres_volumes()[0][:, 0] < 1.0)[0]
    ctx.set_sink_cells(first_layer); ctx.sink_apply()
    again = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert np.intersect1d(again, killed).size > 0 and np.setdiff1d(again, killed).size > 0
    lo, up = (6.5, 0.5, 0.5), (9.5, 2.5, 1.5)                                # x in (8, 9.5] is outside the mesh
    ctx.respawn_box(lo, up)
    xyzw1, cell1 = ctx.get_particles()
    p_box = api.respawn_positions_host(SEED, again, 1, lo, up)
    assert np.array_equal(_bits(xyzw1[again, :3]), _bits(p_box))
    still = again[p_box[:, 0] > 8.0]
    assert 0 < still.size < again.size and np.array_equal(np.nonzero(cell1 < 0)[0], still)
    ctx.respawn_source()
    xyzw2, cell2 = ctx.get_particles()
    want2 = api.source_positions_host(SEED, still, 2, rec, hi)
    assert np.array_equal(_bits(xyzw2[still, :3]), _bits(want2))
    for other in (0, 1):
        assert (api.source_positions_host(SEED, still, other, rec, hi) != want2).any(1).all()
    assert np.array_equal(cell2[still], _locate_dev(ctx, want2)) and (cell2 >= 0).all()
    rest = np.setdiff1d(np.arange(N), still)
    assert np.array_equal(_bits(xyzw2[rest]), _bits(xyzw1[rest])) and np.array_equal(cell2[rest], cell1[rest])
    n1, n2, n3 = killed.size, again.size, still.size
    assert ctx.recycle_counts() == dict(absorbed=n1 + n2, drawn=n1 + n2 + n3, placed=n1 + n2, epochs=3)
    # a new cloud starts again at epoch 0; a new mesh drops the source
    ctx.set_particles(box["xyz"])
    assert ctx.recycle_counts()["epochs"] == 0
    ctx.set_mesh(mesh)
    assert ctx.source_table()[1].size == 0


# ------------------------------------------------------------------------------------------------ 7. a source that sticks out
def test_7_a_source_that_sticks_out_leaves_the_outside_draws_dead(box, gpu_ctx_factory):
    tri = box["tri"]
    centre = tri.mean(1, keepdims=True)
    big = centre + 1.2 * (tri - centre)                                      # scaled about the centroid: over the patch's edges
    rec, hi = api.source_table_host(big, None, DEPTH)
    ctx = gpu_ctx_factory()
    xyzw0, cell0 = _located(ctx, box, source=False)
    ctx.set_source_triangles(big, None, DEPTH)
    ctx.set_sink_cells(box["sink"]); ctx.sink_apply()
    killed = np.nonzero(ctx.get_particles()[1] < 0)[0]
    ctx.respawn_source()
    xyzw, cell = ctx.get_particles()
    p0 = api.source_positions_host(SEED, killed, 0, rec, hi)
    outside = (p0[:, 1] < 0.0) | (p0[:, 1] > 3.0) | (p0[:, 2] < 0.0) | (p0[:, 2] > 2.0)
    assert 0.02 * killed.size < outside.sum() < 0.5 * killed.size
    assert np.array_equal(_bits(xyzw[killed, :3]), _bits(p0))                # the outside draws stay at the drawn point ...
    assert (cell[killed][outside] == L.CELL_LOST).all() and (cell[killed][~outside] >= 0).all()       # ... dead
    counts = ctx.recycle_counts()
    assert counts["drawn"] == killed.size and counts["drawn"] - counts["placed"] == int(outside.sum())
    # they are drawn again, elsewhere, at the next epoch -- and nobody else is
    still = killed[outside]
    ctx.respawn_source()
    xyzw2, cell2 = ctx.get_particles()
    p1 = api.source_positions_host(SEED, still, 1, rec, hi)
    out1 = (p1[:, 1] < 0.0) | (p1[:, 1] > 3.0) | (p1[:, 2] < 0.0) | (p1[:, 2] > 2.0)
    assert np.array_equal(_bits(xyzw2[still, :3]), _bits(p1)) and (p1 != p0[outside]).any(1).all()
    assert np.array_equal(cell2[still] >= 0, ~out1)
    rest = np.setdiff1d(np.arange(N), still)
    assert np.array_equal(_bits(xyzw2[rest]), _bits(xyzw[rest])) and np.array_equal(cell2[rest], cell[rest])
    counts2 = ctx.recycle_counts()
    assert counts2["drawn"] - counts["drawn"] == still.size and counts2["epochs"] == 2
    assert counts2["placed"] - counts["placed"] == int((~out1).sum())


# ------------------------------------------------------------------------------------------------ 8. respawn, limited
DEAD_AT = np.array([64, 256, 257, 1023, 1024, 4095, 4096, N - 1])            # lane 0 of the second wave (256: four ids a lane), slice ends, the last slot


def _limited_arrays(n):
    rng = np.random.default_rng(66 + n)
    cell = rng.integers(0, 48, size=n).astype(np.int32)
    dead = np.unique(np.concatenate([DEAD_AT[DEAD_AT < n], rng.choice(n, size=min(300, n), replace=False)])) if n else np.zeros(0, np.int64)
    cell[dead] = np.where(rng.random(dead.size) < 0.5, L.CELL_LOST, L.CELL_FROZEN)
    xyz = 100.0 + rng.random((n, 3))                                         # (what an untouched slot must still hold)
    return xyz, cell, dead


@pytest.mark.parametrize("gids", ["null", "large"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [N, 1, 63, 4099, 0])
def test_8_limited_respawn_takes_the_first_dead_slots_in_array_order(box, gpu_ctx_factory, n, offset, gids):
    ctx = gpu_ctx_factory()
    ctx.set_mesh(box["mesh"]); ctx.set_seed(SEED); ctx.set_source_triangles(box["tri"], None, DEPTH)
    tables = ctx.mesh_tables()
    xyz, cell, dead = _limited_arrays(n)
    nd = dead.size
    gid = None if gids == "null" else (2 ** 32 + 7 * np.arange(n, dtype=np.int64))[::-1].copy()
    ids = np.arange(n, dtype=np.int64) if gid is None else gid
    epoch = 5
    for k in sorted({0, 1, min(64, nd), nd, nd + 1}) + [-1]:
        wholes = [_dev(np.ascontiguousarray(xyz[:, a]), 0, np.full(7, -5.0)) for a in range(3)]    # (room behind the end, which must stay)
        tx, ty, tz = (w[1] for w in wholes)
        wc, tc = _dev(cell, offset, np.full(7, L.CELL_LOST, np.int32))       # (dead slots behind the end: not the array's)
        tg = None if gid is None else _dev(gid, 0, np.zeros(1, np.int64))[1]
        before = ctx.recycle_counts()
        ctx.respawn_source_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), None if tg is None else tg.data_ptr(), n,
                               k, epoch)
        ctx.synchronize()
        chosen = dead if k < 0 else dead[:min(k, nd)]
        want_xyz, want_cell = xyz.copy(), cell.copy()
        p = api.source_positions_host(SEED, ids[chosen], epoch, box["rec"], box["hi"])
        want_xyz[chosen] = p
        want_cell[chosen] = R.brute_locate(p, tables)
        assert (want_cell[chosen] >= 0).all()
        got = np.stack([w[0].cpu().numpy() for w in wholes], 1)
        assert (got[n:] == -5.0).all()
        got = got[:n]
        got_cell = wc.cpu().numpy()
        assert np.array_equal(got_cell[offset:offset + n], want_cell), (k, np.nonzero(got_cell[offset:offset + n] != want_cell)[0][:8])
        assert (got_cell[:offset] == 3).all() and (got_cell[offset + n:] == L.CELL_LOST).all()
        assert np.array_equal(_bits(got), _bits(want_xyz)), k
        after = ctx.recycle_counts()
        assert after["drawn"] - before["drawn"] == after["placed"] - before["placed"] == chosen.size, k
        assert after["epochs"] == 0                                          # (the caller's epoch, not the context's cloud's)


def test_8_limited_respawn_through_the_context_on_a_sorted_cloud(box, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    xyzw0, cell0 = _located(ctx, box)
    ctx.set_sink_cells(box["sink"]); ctx.sink_apply()
    ctx.sort_by_cell()                                                       # dead slots go to the tail
    dead = np.nonzero(ctx.get_particles()[1] < 0)[0]
    k = 100
    assert dead.size > k
    ctx.respawn_source(k)
    xyzw, cell = ctx.get_particles()
    moved = np.nonzero((_bits(xyzw[:, :3]) != _bits(xyzw0[:, :3])).any(1))[0]
    assert moved.size == k and np.isin(moved, dead).all()                    # the count is exact, the chosen are dead ones
    assert np.array_equal(_bits(xyzw[moved, :3]), _bits(api.source_positions_host(SEED, moved, 0, box["rec"], box["hi"])))
    assert (cell[moved] >= 0).all() and np.array_equal(cell[np.setdiff1d(dead, moved)], np.full(dead.size - k, -1, np.int32))
    c = ctx.recycle_counts()
    assert c["drawn"] == c["placed"] == k and c["epochs"] == 1
    ctx.respawn_source(dead.size)                                            # more than are left: the rest, at epoch 1
    xyzw2, cell2 = ctx.get_particles()
    rest = np.setdiff1d(dead, moved)
    assert (cell2 >= 0).all() and ctx.recycle_counts()["drawn"] == dead.size
    assert np.array_equal(_bits(xyzw2[rest, :3]), _bits(api.source_positions_host(SEED, rest, 1, box["rec"], box["hi"])))
    assert np.array_equal(_bits(xyzw2[moved]), _bits(xyzw[moved]))


# ------------------------------------------------------------------------------------------------ 9. the LDS staging limit
@pytest.fixture(scope="module")
def slab():
    mesh = box_mesh(32, 32, 2)
    faces = np.arange(mesh.n_internal, mesh.n_faces)
    assert faces.size == 2304
    return dict(mesh=mesh, faces=faces)


@pytest.mark.parametrize("quads", [LDS_BOUNDS // 2, LDS_BOUNDS // 2 + 1])
def test_9_a_table_on_each_side_of_the_lds_staging_limit(slab, gpu_ctx_factory, oracle_libs, quads):
    mesh = slab["mesh"]
    tri, of = mesh.face_triangles(slab["faces"][:quads])
    m = tri.shape[0]
    assert m == 2 * quads and (m <= LDS_BOUNDS) == (quads == LDS_BOUNDS // 2)
    weights = 1.0 + (np.arange(m) % 7)                                       # unequal shares
    depth = (0.01, 0.25)
    rec, hi = api.source_table_host(tri, weights, depth)
    assert hi.size == m
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_seed(SEED); ctx.set_source_triangles(tri, weights, depth)
    got_rec, got_hi = ctx.source_table()
    assert np.array_equal(_bits(got_rec), _bits(rec)) and np.array_equal(got_hi, hi)
    xyz = np.full((N, 3), -1.0)
    ctx.set_particles(xyz, np.full(N, L.CELL_LOST, np.int32))                # everybody dead
    ctx.respawn_source()
    xyzw, cell = ctx.get_particles()
    ids = np.arange(N)
    want = api.source_positions_host(SEED, ids, 0, rec, hi)
    assert np.array_equal(_bits(xyzw[:, :3]), _bits(want))
    assert np.array_equal(_bits(want), _bits(SP.positions(SEED, ids, 0, rec, hi)))
    assert np.array_equal(cell, _locate_dev(ctx, want)) and (cell >= 0).all()
    assert ctx.recycle_counts() == dict(absorbed=0, drawn=N, placed=N, epochs=1)
    # every triangle with a draw expected is hit: the point of particle i lies on the triangle the statement picks for it, and the
    # picks reach both ends of the table (past the staged 4096 where there are more)
    t = SP.pick(hi, SP.words(SEED, ids, 0)[:, 0])
    u1, u2, d = SP.recompute(xyzw[:, :3], rec, t)
    assert (u1 >= -1e-12).all() and (u2 >= -1e-12).all() and (u1 + u2 <= 1 + 1e-12).all()
    assert (d >= depth[0] - 1e-12).all() and (d <= depth[1] + 1e-12).all()
    hit = np.unique(t)
    assert hit.size > 0.8 * m * (1.0 - np.exp(-N / m)) and hit.min() < 8 and hit.max() > m - 8
    if m > LDS_BOUNDS:
        assert (hit >= LDS_BOUNDS).any()


# ------------------------------------------------------------------------------------------------ 10. a warped mesh
def test_10_a_warped_boundary_face(gpu_ctx_factory, oracle_libs):
    import torch
    plain = box_mesh(6, 5, 4)
    mesh = W.warp_mesh(plain, 0.05)
    pts = mesh.points
    inner = (pts[:, 0] == 0.0) & (pts[:, 1] > 0.0) & (pts[:, 1] < 5.0) & (pts[:, 2] > 0.0) & (pts[:, 2] < 4.0)
    pts[inner, 0] += np.random.default_rng(4).uniform(-0.05, 0.05, size=int(inner.sum()))       # the x = 0 patch is warped too
    faces = SP.boundary_faces_at_x0(plain)
    tri, of = mesh.face_triangles(faces)
    first = api.build_derived_mesh_host(mesh)[1]
    assert faces.size == 20 and (np.diff(first)[mesh.owner[faces]] > 1).all()                   # every owner cell is decomposed
    assert np.unique(tri[:, :, 0]).size > 5
    # d0 > 0.  The slab is thin on purpose: a warped triangle's normal is tilted against its neighbours' by up to ~0.1, so a point
    # at depth d within d * 0.1 of the face's rim can lie behind the NEIGHBOUR cell's side face -- a strip of 1e-7 of the face at
    # d = 1e-6, 0.004 expected particles of 10 007 (at d = 1e-3 the CPU statement finds two)
    depth = (1e-7, 1e-6)
    rec, hi = api.source_table_host(tri, None, depth)
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_seed(SEED); ctx.set_source_triangles(tri, None, depth)
    assert ctx.mesh_quality()["n_derived"] > mesh.n_cells
    dev = torch.device("cuda", 0)
    tx, ty, tz = (torch.full((N,), -1.0, dtype=torch.float64, device=dev) for _ in range(3))
    tc = torch.full((N,), L.CELL_LOST, dtype=torch.int32, device=dev); tp = torch.empty_like(tc)
    torch.cuda.synchronize()
    ctx.respawn_source_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), None, N, -1, 3)
    ctx.cells_to_parent_dev(tc.data_ptr(), tp.data_ptr(), N)
    ctx.synchronize()
    got = np.stack([t.cpu().numpy() for t in (tx, ty, tz)], 1)
    want = api.source_positions_host(SEED, None, 3, rec, hi, n=N)
    assert np.array_equal(_bits(got), _bits(want))
    cell, parent = tc.cpu().numpy(), tp.cpu().numpy()
    assert (cell >= 0).all() and cell.max() >= mesh.n_cells                  # derived ids indeed
    assert np.array_equal(cell, _locate_dev(ctx, want))
    picked = SP.pick(hi, SP.words(SEED, np.arange(N), 3)[:, 0])
    face = of[rec[picked, 14].astype(np.int64)]
    assert np.array_equal(parent, mesh.owner[face])                          # the derived cell's parent is the face's owner
    assert np.unique(face).size == 20


# ------------------------------------------------------------------------------------------------ 11. age
def test_11_a_source_respawn_stamps_the_births(box, gpu_ctx_factory):
    mesh = box["mesh"]
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    U = np.tile([1.0, 0.0, 0.0], (mesh.n_cells, 1))
    for c in (ctx, twin):
        _located(c, box)
        c.set_velocity(U)
        c.set_sink_cells(box["sink"])
    ctx.age_enable(2, 8)
    now = 0
    for k in range(3):
        for c in (ctx, twin):
            c.step(0.125, 0.0, 4)
        now += 4
        before = ctx.age_births()
        for c in (ctx, twin):
            c.sink_apply()
        dead = np.nonzero(ctx.get_particles()[1] < 0)[0]
        assert dead.size > 0
        for c in (ctx, twin):
            c.respawn_source()
        births = ctx.age_births()
        assert (births[dead] == now).all() and (ctx.get_particles()[1] >= 0).all()              # made live: born now
        rest = np.setdiff1d(np.arange(N), dead)
        assert np.array_equal(births[rest], before[rest])
        assert (ctx.ages()[dead] == 0).all()
    assert np.unique(ctx.age_births()).size >= 3 and ctx.age_histogram().sum() == ctx.recycle_counts()["absorbed"]
    a, b = ctx.get_particles(), twin.get_particles()                        # the cloud is the twin's, bit for bit
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    assert ctx.recycle_counts() == twin.recycle_counts()


# ------------------------------------------------------------------------------------------------ 12. a whole run against the CPU
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_12_a_recycled_run_is_its_cpu_statement_bit_for_bit(name, gpu_ctx_factory, oracle_libs):
    """K rounds of: n cycles of cpf_step (D = 0), cpf_sink_apply, cpf_respawn_source(all) -- against CellWalk's unkicked cycle, the
    numpy sink, the position statement and a brute-force locate over mesh_tables().  The source is the x = 0 patch, weighted by
    inflow, with the depth per triangle |U.n| * dt * cycles (d0 = 0: the CPU statement places every draw, test_source_host.py)."""
    r = SP.run(name)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", r.sort_interval)
    ctx.set_mesh(r.mesh); ctx.set_velocity(r.U); ctx.set_seed(SEED)
    ctx.set_source_triangles(r.tri, r.weights, r.depth)
    ctx.synchronize()
    ctx.set_particles(r.xyz)
    assert ctx.locate_initial() == 0
    tables = ctx.mesh_tables()
    _, cell0 = ctx.get_particles()
    assert np.array_equal(cell0, R.brute_locate(r.xyz, tables))
    rec, hi = ctx.source_table()
    same, same_hi = SP.table(r.tri, r.weights, r.depth, exact=False)
    assert np.array_equal(hi, same_hi) and np.array_equal(_bits(rec), _bits(same))
    ctx.set_sink_cells(r.sink_cells)
    want_xyz, want_cell, absorbed, drawn, placed, times = r.cpu(tables, cell0)
    assert absorbed >= 0.05 * N and (times >= 2).any() and drawn == placed   # conditions (tests/test_source_host.py has them too)
    flat = name == "thin box"
    for k in range(r.rounds):
        if flat:
            streams_z = ctx.step_kernel_name(0.0, 0)
            assert re.fullmatch(r"cpf::step_kernel_stream<false, true, false, (true|false), 8>", streams_z), (k, streams_z)
        ctx.step(r.dt, 0.0, r.cycles)
        if flat:
            body = ctx.step_kernel_name(0.0, 0)
            assert re.fullmatch(r"cpf::step_kernel_stream_flat<true, false, (true|false), 8>", body), (k, body)
        ctx.sink_apply()
        ctx.respawn_source()
    xyzw, cell = ctx.get_particles()
    bad = np.nonzero(cell != want_cell)[0]
    assert bad.size == 0, (name, "cells differ", bad.size, bad[:5], cell[bad[:5]], want_cell[bad[:5]])
    bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(want_xyz)).any(1))[0]
    assert bad.size == 0, (name, "positions differ", bad.size, bad[:5], xyzw[bad[:5], :3], want_xyz[bad[:5]])
    assert ctx.recycle_counts() == dict(absorbed=absorbed, drawn=drawn, placed=placed, epochs=r.rounds)
    print("source run %s: %d absorbed, %d drawn, %d placed, %d particles respawned twice or more: the CPU's bits"
          % (name, absorbed, drawn, placed, int((times >= 2).sum())))


def test_12_cuda_particles_recycles_a_channel_through_its_inlet():
    mesh = box_mesh(12, 3, 3)
    U = np.tile([1.0, 0.0, 0.0], (mesh.n_cells, 1))
    dt = 2.0 ** -3
    whole = ((0.0, 0.0, 0.0), (12.0, 3.0, 3.0))
    tri, of = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
    keys = dict(sinkCells=_last_x_layer(mesh), sourceTriangles=tri, sourceWeights=api.inflow_weights(mesh, U, tri, of),
                sourceDepth=(0.0, 2 * dt))
    p = api.CudaParticles(mesh, U, dict(numParticles=N, dt=dt, saveInterval=10, diffusionCoeff=1e-2, seedingBox=whole,
                                        recycleInterval=2, occupancyInterval=2, **keys))
    try:
        before = p.recycle_counts()
        for k in range(3):
            assert p.advect(k * 10 * dt, 10 * dt) == 10
            _, cell = p.particles()
            after = p.recycle_counts()
            d = {key: after[key] - before[key] for key in after}
            assert d["absorbed"] > 0 and d["epochs"] == 5 and d["drawn"] == d["placed"] == d["absorbed"] and (cell >= 0).all()
            before = after
        conc = p.concentration()
        assert np.isfinite(conc).all() and conc.sum() > 0
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 13. state and argument errors
def test_13_state_and_argument_errors(box):
    tri = box["tri"]

    def refused(status, call):
        with pytest.raises(L.CpfError) as e:
            call()
        assert e.value.status == status, str(e.value)

    with api.Context(0) as ctx:
        for call in (lambda: ctx.set_source_triangles(tri), ctx.respawn_source,
                     lambda: ctx.respawn_source_dev(None, None, None, None, None, 0)):
            refused(L.CPF_ERR_STATE, call)                                   # no mesh
        assert ctx.source_table()[1].size == 0
        ctx.set_mesh(box["mesh"])
        refused(L.CPF_ERR_STATE, ctx.respawn_source)                         # no source
        refused(L.CPF_ERR_STATE, lambda: ctx.respawn_source_dev(None, None, None, None, None, 0))
        ctx.set_source_triangles(tri, None, DEPTH)
        refused(L.CPF_ERR_STATE, ctx.respawn_source)                         # no located particles
        ctx.set_particles(box["xyz"])
        refused(L.CPF_ERR_STATE, ctx.respawn_source)                         # ... set, but not located
        ctx.respawn_source_dev(None, None, None, None, None, 0)              # nothing to do is no error
        refused(L.CPF_ERR_ARG, lambda: ctx.respawn_source_dev(None, None, None, None, None, 5))
        refused(L.CPF_ERR_ARG, lambda: ctx.respawn_source_dev(None, None, None, None, None, -1))
        for bad in (dict(weights=np.full(12, -1.0)), dict(weights=np.zeros(12)), dict(depth=(0.5, 0.1)),
                    dict(depth=(0.0, float("nan"))), dict(weights=np.where(np.arange(12) == 3, np.inf, 1.0))):
            refused(L.CPF_ERR_ARG, lambda: ctx.set_source_triangles(tri, bad.get("weights"), bad.get("depth", DEPTH)))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_source_triangles(np.zeros((4, 3, 3))))          # all degenerate
        # a refused set leaves the source that was there; no triangle clears it; a new mesh drops it
        assert np.array_equal(ctx.source_table()[1], box["hi"])
        ctx.locate_initial()
        ctx.set_sink_cells(box["sink"]); ctx.sink_apply(); ctx.respawn_source()
        c = ctx.recycle_counts()
        assert c["drawn"] == c["placed"] == c["absorbed"] > 0
        ctx.set_source_triangles(np.zeros((0, 3, 3)))
        assert ctx.source_table()[1].size == 0
        refused(L.CPF_ERR_STATE, ctx.respawn_source)
        ctx.set_source_triangles(tri, None, DEPTH)
        ctx.set_mesh(box["mesh"]); ctx.set_particles(box["xyz"]); ctx.locate_initial()
        refused(L.CPF_ERR_STATE, ctx.respawn_source)
