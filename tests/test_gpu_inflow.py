"""GPU: the patch source follows the velocity field (include/cpf.h "flux table"; csrc/cpf_inflow.hip).  After ``source_follow`` every
``set_velocity`` / ``set_velocity_dev`` leaves the table cpf_source_flux_host makes of the table before -- hi and column 13 bit for
bit, every other column untouched -- at every size at which the kernels change path; a field without inflow changes nothing and is
counted; a whole recycled run under a field that changes every round is its CPU statement's bits; tagging keeps its origins;
and a context that never follows keeps the tables it had."""
import numpy as np
import pytest

import inflow as IF
import recycle as R
import sourcepatch as SP
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = R.N
SEED = R.SEED
DEPTH = (0.001, 0.003)
BLOCK = 256                                  # csrc/cpf_inflow.hip, kInflowBlock: lanes of a workgroup == records of its tile
FUSED = 1024                                 # csrc/cpf_inflow.hip, kInflowFused: larger tables take the four launches
LDS_BOUNDS = 4096                            # csrc/cpf_inlet.hip, kSourceLdsBounds: the place kernel's staged bounds
# 1, 3, 64, 65: one lane, part of a wave, a wave, a wave and a lane.  Then one below, at and one above: BLOCK (the tile and the block
# are the same constant; below FUSED it is the fused kernel's fourth wave that starts there), FUSED, a tile boundary of the four
# launches (5 * BLOCK), LDS_BOUNDS, and BLOCK tiles -- where the scan of the tiles' sums takes a second trip.
SIZES = [1, 3, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, FUSED - 1, FUSED, FUSED + 1, 5 * BLOCK - 1, 5 * BLOCK, 5 * BLOCK + 1,
         LDS_BOUNDS - 1, LDS_BOUNDS, LDS_BOUNDS + 1, BLOCK * BLOCK - 1, BLOCK * BLOCK, BLOCK * BLOCK + 1, 70001]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def mesh():
    return box_mesh(8, 3, 2)


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


def _source(ctx, mesh, k, seed):
    """a fresh mesh, a synthetic source of k kept triangles with random owner cells; returns (rec, hi, cells) as built"""
    ctx.set_mesh(mesh)
    tri = IF.soup(seed, k)
    ctx.set_source_triangles(tri, None, DEPTH)
    rec, hi = ctx.source_table()
    assert rec.shape[0] == k
    cells = np.random.default_rng(seed + 1).integers(0, mesh.n_cells, size=k).astype(np.int32)
    return rec, hi, cells


def _expect(rec, hi, cells, U, s):
    """the host statement's table after one refresh"""
    span, new_hi, _, empty = api.source_flux_host(rec, cells, U, s)
    out = rec.copy()
    if empty:
        return out, hi.copy()
    if s > 0:
        out[:, 13] = span
    return out, new_hi


def _assert_table(ctx, rec, hi, what=""):
    got_rec, got_hi = ctx.source_table()
    bad = np.nonzero(got_hi != hi)[0]
    assert bad.size == 0, (what, "hi differs", bad.size, bad[:5], got_hi[bad[:5]], hi[bad[:5]])
    bad = np.nonzero((_bits(got_rec) != _bits(rec)).any(1))[0]
    assert bad.size == 0, (what, "rec differs", bad.size, bad[:5])
    return got_rec, got_hi


# ------------------------------------------------------------------------------------------------ 1. the table against the host statement
@pytest.mark.parametrize("k", SIZES)
def test_1_a_refreshed_table_is_the_host_statement(ctx, mesh, k):
    rec, hi, cells = _source(ctx, mesh, k, 1000 + k)
    ctx.source_follow(cells, 0.0125)                                    # no velocity yet: nothing is refreshed
    _assert_table(ctx, rec, hi, "before U")
    assert ctx.source_follow_counts() == dict(on=True, refreshes=0, skipped=0)
    for seed in range(k, k + 64):                                       # (the first field with inflow: a single triangle may face away)
        U = np.random.default_rng(seed).normal(size=(mesh.n_cells, 3))
        if not api.source_flux_host(rec, cells, U, 0.0125)[3]:
            break
    ctx.set_velocity(U)
    want, want_hi = _expect(rec, hi, cells, U, 0.0125)
    assert not np.array_equal(want_hi, hi) or k == 1
    assert not np.array_equal(want[:, 13], rec[:, 13])
    got, _ = _assert_table(ctx, want, want_hi, k)
    assert np.array_equal(_bits(got[:, :13]), _bits(rec[:, :13])) and np.array_equal(_bits(got[:, 14:]), _bits(rec[:, 14:]))
    assert ctx.source_follow_counts() == dict(on=True, refreshes=1, skipped=0)


def test_1_two_million_equal_triangles(mesh):
    """2^21 + 3 triangles with q = 2^32 - 5 each (tests/test_inflow_host.py): Q passes 2^53 and the conversions round"""
    k = 2 ** 21 + 3
    tri = np.zeros((k, 3, 3))
    tri[:, 1, 0] = 1.0
    tri[:, 2, 1] = 1.0
    cells = np.zeros(k, np.int32)
    U = np.zeros((mesh.n_cells, 3))
    U[0, 2] = -(2.0 - 2.0 ** -29 - 2.0 ** -31)
    with api.Context(0) as c:
        c.set_mesh(mesh)
        c.set_source_triangles(tri, None, (0.0, 0.0))
        del tri
        rec, hi = c.source_table()
        assert rec.shape[0] == k
        c.set_velocity(U)
        c.source_follow(cells, 0.5)                                     # a velocity is there: refreshed at once
        span, want_hi, q, empty = api.source_flux_host(rec, cells, U, 0.5)
        assert not empty and (q == 2 ** 32 - 5).all() and int(q.sum(dtype=np.uint64)) > 2 ** 53
        got, got_hi = c.source_table()
        assert np.array_equal(got_hi, want_hi)
        assert np.array_equal(_bits(got[:, 13]), _bits(span)) and (span == span[0]).all() and span[0] > 0
        assert np.array_equal(got[:, :13], rec[:, :13]) and np.array_equal(got[:, 14:], rec[:, 14:])
        assert c.source_follow_counts() == dict(on=True, refreshes=1, skipped=0)


# ------------------------------------------------------------------------------------------------ 2. field variants
@pytest.mark.parametrize("k", [65, FUSED + 1])
def test_2_through_set_velocity_dev(ctx, mesh, k):
    import torch
    rec, hi, cells = _source(ctx, mesh, k, 2000 + k)
    ctx.source_follow(cells, 0.25)
    U = np.random.default_rng(k).normal(size=(mesh.n_cells, 3))
    t = torch.from_numpy(U).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.set_velocity_dev(t.data_ptr(), mesh.n_cells)
    want, want_hi = _expect(rec, hi, cells, U, 0.25)
    _assert_table(ctx, want, want_hi, k)
    # a refresh on its own reads the context's field, not the caller's array
    t.zero_()
    torch.cuda.synchronize()
    ctx.source_refresh()
    _assert_table(ctx, want, want_hi, k)
    assert ctx.source_follow_counts() == dict(on=True, refreshes=2, skipped=0)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("k", [40, FUSED + 1])
def test_2_on_a_mesh_with_decomposed_cells(ctx, k, dev):
    import torch
    warped = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    ctx.set_mesh(warped)
    assert ctx.mesh_quality()["n_derived"] > warped.n_cells
    tri = IF.soup(3000 + k, k)
    ctx.set_source_triangles(tri, None, DEPTH)
    rec, hi = ctx.source_table()
    cells = np.random.default_rng(k).integers(0, warped.n_cells, size=k).astype(np.int32)      # cells of the mesh AS GIVEN
    ctx.source_follow(cells, 0.25)
    U = np.random.default_rng(k + 1).normal(size=(warped.n_cells, 3))
    if dev:
        t = torch.from_numpy(U).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx.set_velocity_dev(t.data_ptr(), warped.n_cells)
    else:
        ctx.set_velocity(U)
    want, want_hi = _expect(rec, hi, cells, U, 0.25)
    _assert_table(ctx, want, want_hi, (k, dev))


@pytest.mark.parametrize("k", [65, FUSED + 1])
def test_2_without_a_depth_scale_the_depths_stay(ctx, mesh, k):
    rec, hi, cells = _source(ctx, mesh, k, 4000 + k)
    ctx.source_follow(cells, 0.0)
    U = np.random.default_rng(k).normal(size=(mesh.n_cells, 3))
    ctx.set_velocity(U)
    want, want_hi = _expect(rec, hi, cells, U, 0.0)
    got, _ = _assert_table(ctx, want, want_hi, k)
    assert np.array_equal(_bits(got[:, 13]), _bits(rec[:, 13])) and (got[:, 13] == DEPTH[1] - DEPTH[0]).all()


# ------------------------------------------------------------------------------------------------ 3. successive fields
@pytest.mark.parametrize("k", [300, 3000])
def test_3_successive_fields(ctx, mesh, k):
    rec, hi, cells = _source(ctx, mesh, k, 5000 + k)
    ctx.source_follow(cells, 0.125)
    seen = []
    for round_ in range(3):
        U = np.random.default_rng(10 * k + round_).normal(size=(mesh.n_cells, 3)) * 10.0 ** round_
        ctx.set_velocity(U)
        want, want_hi = _expect(rec, hi, cells, U, 0.125)
        rec, hi = _assert_table(ctx, want, want_hi, (k, round_))
        assert rec.shape[0] == k and np.array_equal(rec[:, 14], np.arange(k))
        seen.append(hi)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert ctx.source_follow_counts() == dict(on=True, refreshes=3, skipped=0)


# ------------------------------------------------------------------------------------------------ 4. zero inflow
@pytest.mark.parametrize("k", [40, FUSED + 500])
def test_4_a_field_without_inflow_changes_nothing_and_is_counted(ctx, mesh, k):
    rec, hi, cells = _source(ctx, mesh, k, 6000 + k)
    ctx.source_follow(cells, 0.5)
    U = np.random.default_rng(k).normal(size=(mesh.n_cells, 3))
    ctx.set_velocity(U)
    rec1, hi1 = _assert_table(ctx, *_expect(rec, hi, cells, U, 0.5), what=k)
    ctx.set_velocity(np.zeros((mesh.n_cells, 3)))
    assert api.source_flux_host(rec1, cells, np.zeros((mesh.n_cells, 3)), 0.5)[3]
    _assert_table(ctx, rec1, hi1, "no inflow")
    assert ctx.source_follow_counts() == dict(on=True, refreshes=2, skipped=1)
    ctx.set_velocity(-U)
    rec2, hi2 = _assert_table(ctx, *_expect(rec1, hi1, cells, -U, 0.5), what="inflow again")
    assert not np.array_equal(hi2, hi1)
    assert ctx.source_follow_counts() == dict(on=True, refreshes=3, skipped=1)


def test_4_all_outward_flow(ctx, mesh):
    """every triangle has a cell of its own whose U points out of it"""
    ctx.set_mesh(mesh)
    k = 40
    ctx.set_source_triangles(IF.soup(77, k), None, DEPTH)
    rec, hi = ctx.source_table()
    cells = np.arange(k, dtype=np.int32)
    U = np.zeros((mesh.n_cells, 3))
    U[:k] = -rec[:, 9:12]
    ctx.set_velocity(U)
    ctx.source_follow(cells, 0.5)
    _assert_table(ctx, rec, hi, "outward")
    assert ctx.source_follow_counts() == dict(on=True, refreshes=1, skipped=1)


# ------------------------------------------------------------------------------------------------ 5. a whole recycled run
def _fields(U, rounds):
    """the run's field per round: scaled, and the cross-stream component reversed every other round"""
    out = []
    for e in range(rounds):
        f = U * (1.0 + 0.125 * (e % 3))
        if e % 2:
            f[:, 1] = -f[:, 1]
        out.append(np.ascontiguousarray(f))
    return out


@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_5_a_recycled_run_under_a_changing_field_is_its_cpu_statement(name, gpu_ctx_factory, oracle_libs):
    """K rounds of: cpf_set_velocity (the table follows), n cycles of cpf_step (D = 0), cpf_sink_apply, cpf_respawn_source(all) --
    against sourcepatch.cpu_recycled_run's pieces with the host statement's table for each round."""
    r = SP.run(name)
    cells = r.mesh.owner[r.face_of_tri].astype(np.int32)
    scale = r.dt * r.cycles
    fields = _fields(r.U, r.rounds)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", r.sort_interval)
    ctx.set_mesh(r.mesh); ctx.set_seed(SEED)
    ctx.set_source_triangles(r.tri, None, (0.0, 0.0))                    # the areas: no triangle with inflow later is dropped now
    rec0, hi0 = ctx.source_table()
    assert rec0.shape[0] == r.tri.shape[0]
    ctx.source_follow(cells, scale)
    ctx.set_velocity(fields[0])
    ctx.set_particles(r.xyz)
    assert ctx.locate_initial() == 0
    tables = ctx.mesh_tables()
    _, cell0 = ctx.get_particles()
    ctx.set_sink_cells(r.sink_cells)
    want_xyz, want_cell, absorbed, drawn, placed = IF.cpu_followed_run(
        r.mesh, tables, fields, r.xyz, cell0, r.dt, r.rounds, r.cycles, r.sink_cells, rec0, hi0, cells, scale, SEED, refresh=_expect)
    assert absorbed >= 0.05 * N and drawn > 0
    for e in range(r.rounds):
        ctx.set_velocity(fields[e])
        ctx.step(r.dt, 0.0, r.cycles)
        ctx.sink_apply()
        ctx.respawn_source()
    xyzw, cell = ctx.get_particles()
    bad = np.nonzero(cell != want_cell)[0]
    assert bad.size == 0, (name, "cells differ", bad.size, bad[:5], cell[bad[:5]], want_cell[bad[:5]])
    bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(want_xyz)).any(1))[0]
    assert bad.size == 0, (name, "positions differ", bad.size, bad[:5], xyzw[bad[:5], :3], want_xyz[bad[:5]])
    assert ctx.recycle_counts() == dict(absorbed=absorbed, drawn=drawn, placed=placed, epochs=r.rounds)
    assert ctx.source_follow_counts() == dict(on=True, refreshes=r.rounds + 1, skipped=0)
    print("followed run %s: %d absorbed, %d drawn, %d placed: the CPU's bits" % (name, absorbed, drawn, placed))


# ------------------------------------------------------------------------------------------------ 6. through CudaParticles
def test_6_cuda_particles_follows_advect_u():
    mesh = box_mesh(12, 3, 3)
    U = np.tile([1.0, 0.0, 0.0], (mesh.n_cells, 1))
    dt = 2.0 ** -3
    whole = ((0.0, 0.0, 0.0), (12.0, 3.0, 3.0))
    tri, of = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
    cells = mesh.owner[of].astype(np.int32)
    keys = dict(sinkCells=np.nonzero(mesh.cell_centres_volumes()[0][:, 0] > 11.0)[0].astype(np.int32), sourceTriangles=tri,
                sourceCells=cells, sourceFollowU=True, sourceDepthScale=2 * dt)
    base = dict(numParticles=N, dt=dt, saveInterval=10, diffusionCoeff=0.0, seedingBox=whole, recycleInterval=2)
    for bad in (dict(sourceWeights=np.ones(tri.shape[0])), dict(sourceCells=None), dict(recycleInterval=0)):
        with pytest.raises(ValueError):
            api.CudaParticles(mesh, U, {**base, **keys, **bad})
    p = api.CudaParticles(mesh, U, {**base, **keys})
    try:
        rec0, hi0 = api.source_table_host(tri, None, (0.0, 0.0))
        want, want_hi = _expect(rec0, hi0, cells, U, 2 * dt)
        _assert_table(p.ctx, want, want_hi, "at construction")
        assert (want[:, 13] == 2 * dt).all()
        # a field that enters through the upper half of the inlet only, three times as fast
        U2 = U.copy()
        centres = mesh.cell_centres_volumes()[0]
        U2[centres[:, 2] < 1.75, 0] = 0.0                                # (the cells' centres are at z = 0.5, 1.5, 2.5)
        U2[centres[:, 2] >= 1.75, 0] = 3.0
        assert p.advect(0.0, 10 * dt, U=U2) == 10
        want, want_hi = _expect(want, want_hi, cells, U2, 2 * dt)
        got, _ = _assert_table(p.ctx, want, want_hi, "after advect(U=...)")
        upper = centres[cells[got[:, 14].astype(np.int64)], 2] >= 1.75
        assert (got[upper, 13] == 6 * dt).all() and (got[~upper, 13] == 0.0).all() and upper.any() and (~upper).any()
        c = p.recycle_counts()
        assert c["absorbed"] > 0 and c["drawn"] == c["placed"] == c["absorbed"]
        assert p.ctx.source_follow_counts() == dict(on=True, refreshes=2, skipped=0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7. tagging
def test_7_tagging_keeps_its_origins_across_a_refresh(gpu_ctx_factory):
    mesh = box_mesh(8, 3, 2)
    tri, of = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
    cells = mesh.owner[of].astype(np.int32)
    origins = (tri.mean(1)[:, 1] > 1.5).astype(np.int32) + 1            # origin 1 below y = 1.5, origin 2 above
    xyz = pz.uniform_points(78, N, (0.0, 0.0, 0.0), (8.0, 3.0, 2.0))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_seed(SEED)
    ctx.set_source_triangles(tri, None, (0.0, 0.0))
    ctx.set_particles(xyz)
    assert ctx.locate_initial() == 0
    ctx.set_sink_cells(np.nonzero(mesh.cell_centres_volumes()[0][:, 0] > 7.0)[0].astype(np.int32))
    ctx.tag_enable(3, 1)
    ctx.set_source_origins(origins)
    ctx.source_follow(cells, 0.5)
    U = np.tile([1.0, 0.0, 0.0], (mesh.n_cells, 1))
    U[:, 0] += np.random.default_rng(5).random(mesh.n_cells) * 4.0     # unequal inflow
    U[mesh.owner[of[3]], 0] = -1.0                                       # and none through one face
    ctx.set_velocity(U)
    rec, hi = ctx.source_table()
    assert np.array_equal(hi, api.source_flux_host(rec, cells, U, 0.5)[1]) and np.unique(hi).size < hi.size
    ctx.sink_apply()
    dead = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert dead.size > 100
    ctx.respawn_source()
    picked = SP.pick(hi, SP.words(SEED, dead, 0)[:, 0])
    assert np.array_equal(picked, api.source_picks_host(SEED, dead, 0, hi))
    got = ctx.tag_origins()
    assert np.array_equal(got[dead], origins[rec[picked, 14].astype(np.int64)].astype(np.uint8))
    assert set(np.unique(got[dead])) == {1, 2} and (np.delete(got, dead) == 0).all()
    assert not np.isin(rec[picked, 14].astype(np.int64), np.nonzero(of == of[3])[0]).any()     # the dry face is never picked


# ------------------------------------------------------------------------------------------------ 8. life cycle
def _refused(ctx, status, text, call):
    with pytest.raises(L.CpfError) as e:
        call()
    assert e.value.status == status and text in str(e.value), str(e.value)
    assert text in ctx.lib.cpf_last_error(ctx.h).decode()


def test_8_life_cycle_and_refusals(mesh):
    k = 70
    tri = IF.soup(8, k)
    cells = np.random.default_rng(9).integers(0, mesh.n_cells, size=k).astype(np.int32)
    rng = np.random.default_rng(10)
    U1, U2 = rng.normal(size=(mesh.n_cells, 3)), rng.normal(size=(mesh.n_cells, 3))
    with api.Context(0) as ctx:
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_follow: call cpf_set_mesh first", lambda: ctx.source_follow(cells))
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_refresh: call cpf_source_follow first", ctx.source_refresh)
        ctx.source_unfollow()                                           # off already: no error
        assert ctx.source_follow_counts() == dict(on=False, refreshes=0, skipped=0)
        ctx.set_mesh(mesh)
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_follow: call cpf_set_source_triangles first", lambda: ctx.source_follow(cells))
        ctx.set_source_triangles(tri, None, DEPTH)
        rec, hi = ctx.source_table()
        # bad arguments
        bad = cells.copy(); bad[5] = mesh.n_cells
        _refused(ctx, L.CPF_ERR_ARG, "cpf_source_follow: cell %d is not in [0, nCells)" % mesh.n_cells, lambda: ctx.source_follow(bad))
        bad[5] = -1
        _refused(ctx, L.CPF_ERR_ARG, "cpf_source_follow: cell -1 is not in [0, nCells)", lambda: ctx.source_follow(bad))
        _refused(ctx, L.CPF_ERR_ARG, "beyond nTriangles", lambda: ctx.source_follow(cells[:k - 1]))
        _refused(ctx, L.CPF_ERR_ARG, "cpf_source_follow: bad arguments", lambda: ctx.source_follow(cells[:0]))
        for s in (-1.0, float("nan"), float("inf")):
            _refused(ctx, L.CPF_ERR_ARG, "cpf_source_follow: depthScale must be finite and >= 0", lambda: ctx.source_follow(cells, s))
        assert ctx.source_follow_counts()["on"] is False
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_refresh: call cpf_source_follow first", ctx.source_refresh)
        # following on, no velocity: a refresh refuses
        ctx.source_follow(cells, 0.5)
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_refresh: call cpf_set_velocity first", ctx.source_refresh)
        ctx.set_velocity(U1)
        rec1, hi1 = _assert_table(ctx, *_expect(rec, hi, cells, U1, 0.5), what="U1")
        # unfollow freezes the table
        ctx.source_unfollow()
        assert ctx.source_follow_counts() == dict(on=False, refreshes=0, skipped=0)
        ctx.set_velocity(U2)
        _assert_table(ctx, rec1, hi1, "frozen")
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_refresh: call cpf_source_follow first", ctx.source_refresh)
        # following again: refreshed at once from the field that is there
        ctx.source_follow(cells, 0.5)
        rec2, hi2 = _assert_table(ctx, *_expect(rec1, hi1, cells, U2, 0.5), what="U2")
        assert ctx.source_follow_counts() == dict(on=True, refreshes=1, skipped=0)
        # a new table turns following off
        ctx.set_source_triangles(tri, None, DEPTH)
        assert ctx.source_follow_counts()["on"] is False
        ctx.set_velocity(U1)
        _assert_table(ctx, rec, hi, "a new table does not follow")
        # a new mesh drops it
        ctx.source_follow(cells, 0.5)
        assert ctx.source_follow_counts()["on"] is True
        ctx.set_mesh(mesh)
        assert ctx.source_follow_counts() == dict(on=False, refreshes=0, skipped=0)
        assert ctx.source_table()[1].size == 0
        _refused(ctx, L.CPF_ERR_STATE, "cpf_source_follow: call cpf_set_source_triangles first", lambda: ctx.source_follow(cells))


# ------------------------------------------------------------------------------------------------ 9. no following, no change
@pytest.mark.parametrize("k", [12, FUSED + 1])
def test_9_a_context_that_never_follows_keeps_its_table(ctx, mesh, k):
    ctx.set_mesh(mesh)
    tri = IF.soup(9000 + k, k)
    w = np.random.default_rng(k).uniform(0.1, 2.0, size=k)
    ctx.set_source_triangles(tri, w, DEPTH)
    rec, hi = api.source_table_host(tri, w, DEPTH)
    for seed in range(2):
        ctx.set_velocity(np.random.default_rng(seed).normal(size=(mesh.n_cells, 3)))
        _assert_table(ctx, rec, hi, (k, seed))
    assert ctx.source_follow_counts() == dict(on=False, refreshes=0, skipped=0)
