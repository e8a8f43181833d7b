"""GPU: tracer tags (include/cpf.h "tracer tags"; csrc/cpf_tags.hip).  Everything is integers and every comparison is exact: the
transfer matrix, the stamped origins and the per-origin field against the numpy statements of tests/tags.py over what
``get_particles()`` returns, whole recycled runs against the CPU statement, and the cloud itself against a twin context without
tagging."""
import numpy as np
import pytest

import age as A
import recycle as R
import sourcepatch as SP
import tags as T
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = R.N                                      # 10 007: a multiple of neither 64, 256 nor 1024
N_T = 2 * 4096 + 37                          # the transfer tests': two slices and a tail
SEED = R.SEED
DEPTH = (0.0, 0.5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


def _located(ctx, mesh, xyz, sort, cell=None):
    ctx.set_mesh(mesh); ctx.set_velocity(np.zeros((mesh.n_cells, 3))); ctx.set_seed(SEED)
    ctx.set_particles(xyz, cell)
    if cell is None:
        assert ctx.locate_initial() == 0
    if sort:
        ctx.sort_by_cell()


def _origins(n, n_origins, seed):
    o = np.random.default_rng(seed).integers(0, n_origins, size=n).astype(np.uint8)
    o[::5] = n_origins - 1
    return o


# ------------------------------------------------------------------------------------------------ 1. transfer against numpy
@pytest.fixture(scope="module")
def sinkbox():
    """5 x 4 x 4 unit cells, the last x layer (16 cells) the sink; half the cloud lies in it, so that 16 x 16 entries all get hits"""
    mesh = box_mesh(5, 4, 4)
    sink = _last_x_layer(mesh)
    assert sink.size == 16
    xyz = np.concatenate([pz.uniform_points(77, N_T // 2, (0.0, 0.0, 0.0), (5.0, 4.0, 4.0)),
                          pz.uniform_points(78, N_T - N_T // 2, (4.0, 0.0, 0.0), (5.0, 4.0, 4.0))])
    xyz = xyz[np.random.default_rng(1).permutation(N_T)]                     # unsorted: hits scattered over the array
    return dict(mesh=mesh, sink=sink, xyz=xyz)


@pytest.mark.parametrize("n_origins,n_sinks", [(1, 1), (3, 2), (16, 16)])
@pytest.mark.parametrize("sort", [True, False])
def test_1_transfer_counts_exactly_the_absorbed(sinkbox, gpu_ctx_factory, sort, n_origins, n_sinks):
    """sort: fresh from cpf_sort_by_cell (gid permuted, hits in runs); without: gid = index, hits scattered"""
    mesh, sink = sinkbox["mesh"], sinkbox["sink"]
    groups = (np.arange(sink.size) * 5 + 2) % n_sinks
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, sinkbox["xyz"], sort)
    twin.set_sink_cells(sink)
    _, cell0 = ctx.get_particles()
    ctx.tag_enable(n_origins, n_sinks)
    assert not ctx.tag_origins().any() and not ctx.transfer().any()          # everybody starts in origin 0
    ctx.set_sink_groups(sink, groups)
    origin = _origins(N_T, n_origins, 40 + n_origins)
    ctx.tag_set_origins(origin)
    assert np.array_equal(ctx.tag_origins(), origin)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert 0.5 * N_T < hit.sum() < 0.7 * N_T
    want = T.transfer(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, hit, n_origins, n_sinks)
    got = ctx.transfer()
    assert got.dtype == np.uint64 and got.shape == (n_origins, n_sinks) and np.array_equal(got, want), (got, want)
    assert (want > 0).all()                                                  # every entry of the matrix is hit
    assert int(got.sum()) == int(hit.sum()) == ctx.recycle_counts()["absorbed"]
    # the cloud is the twin's, which ran the plain sink: cells, positions, the counters
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], R.sink(cell0, sink)) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert ctx.recycle_counts() == twin.recycle_counts() == dict(absorbed=int(hit.sum()), drawn=0, placed=0, epochs=0)
    assert np.array_equal(ctx.tag_origins(), origin)                         # the pass writes nothing
    ctx.sink_apply()                                                         # a second apply finds nobody
    assert np.array_equal(ctx.transfer(), want)
    # a plain set_sink_cells while tagging is on: all its cells in group 0
    ctx.set_particles(sinkbox["xyz"], cell0)                                 # (a new cloud turns tagging off)
    ctx.tag_enable(n_origins, n_sinks); ctx.set_sink_groups(sink, groups); ctx.set_sink_cells(sink); ctx.tag_set_origins(origin)
    ctx.sink_apply()
    got = ctx.transfer()
    assert np.array_equal(got[:, 0], want.sum(1)) and not got[:, 1:].any()


@pytest.mark.parametrize("sort", [True, False])
def test_1_every_particle_of_two_slices_and_a_tail_is_absorbed(gpu_ctx_factory, sort):
    mesh = box_mesh(5, 4, 3)
    sink = _last_x_layer(mesh)
    xyz = pz.uniform_points(5, N_T, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))        # all in the last x layer
    groups = np.arange(sink.size) % 2
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, sort)
    _, cell0 = ctx.get_particles()
    ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups)
    origin = _origins(N_T, 3, 8)
    ctx.tag_set_origins(origin)
    ctx.sink_apply()
    want = T.transfer(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, np.ones(N_T, bool), 3, 2)
    assert np.array_equal(ctx.transfer(), want) and int(want.sum()) == N_T
    assert ctx.recycle_counts()["absorbed"] == N_T and (ctx.get_particles()[1] == -1).all()


BIG_SINK = (41, 40, 40)                                                      # 65 600 cells: more bits than the 2048 staged words hold
N_BIG = 36_000


def test_1_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(*BIG_SINK)
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    groups = (sink // 3) % 2
    xyz = pz.uniform_points(79, N_BIG, (0.0, 0.0, 0.0), tuple(float(v) for v in BIG_SINK))
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, xyz, True)
    twin.set_sink_cells(sink)
    _, cell0 = ctx.get_particles()
    ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups)
    origin = _origins(N_BIG, 3, 9)
    ctx.tag_set_origins(origin)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert hit.sum() > 500
    want = T.transfer(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, hit, 3, 2)
    assert np.array_equal(ctx.transfer(), want) and (want > 0).all()
    assert np.array_equal(ctx.get_particles()[1], twin.get_particles()[1]) and ctx.recycle_counts() == twin.recycle_counts()
    assert ctx.recycle_counts()["absorbed"] == int(hit.sum()) == int(want.sum())


def test_1_with_age_tracking_on_the_histogram_is_the_untagged_one(sinkbox, gpu_ctx_factory):
    mesh, sink = sinkbox["mesh"], sinkbox["sink"]
    groups = np.arange(sink.size) % 2
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    births = np.random.default_rng(3).integers(0, 40, size=N_T).astype(np.uint32)
    for c in (ctx, twin):
        _located(c, mesh, sinkbox["xyz"], True)
        c.step(0.1, 0.0, 40)                                                 # (at rest: the cycle counter is 40)
        c.set_sink_cells(sink)
        c.age_enable(7, 8)
        c.age_set_births(births)
    _, cell0 = ctx.get_particles()
    ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups)
    origin = _origins(N_T, 3, 10)
    ctx.tag_set_origins(origin)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    hist = ctx.age_histogram()
    assert np.array_equal(hist, twin.age_histogram()) and np.array_equal(hist, A.rtd(A.ages(40, births[hit]), 7, 8))
    assert np.array_equal(ctx.transfer(), T.transfer(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, hit, 3, 2))
    assert int(ctx.transfer().sum()) == int(hist.sum()) == ctx.recycle_counts()["absorbed"]
    assert np.array_equal(ctx.get_particles()[1], twin.get_particles()[1]) and np.array_equal(ctx.ages(), twin.ages())


# ------------------------------------------------------------------------------------------------ 2. the stamp
@pytest.fixture(scope="module")
def srcbox():
    """tests/test_gpu_source.py's box: 8 x 3 x 2 cells, the x = 0 patch (12 triangles) the source, the last x layer the sink"""
    mesh = box_mesh(8, 3, 2)
    tri, _ = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
    assert tri.shape == (12, 3, 3)
    rec, hi = api.source_table_host(tri, None, DEPTH)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(78, N, (0.0, 0.0, 0.0), (8.0, 3.0, 2.0)), tri=tri, rec=rec,
                hi=hi, origin_of_triangle=(np.arange(12) % 3 + 1).astype(np.int32))


def _source_ctx(ctx, b, sort):
    ctx.set_mesh(b["mesh"]); ctx.set_seed(SEED)
    ctx.set_source_triangles(b["tri"], None, DEPTH)
    ctx.set_particles(b["xyz"])
    assert ctx.locate_initial() == 0
    if sort:
        ctx.sort_by_cell()
    ctx.tag_enable(5, 1)
    ctx.set_source_origins(b["origin_of_triangle"])
    return T.origin_of_kept(b["rec"], b["origin_of_triangle"])


def test_2_box_and_source_calls_mixed_on_one_cloud(srcbox, gpu_ctx_factory, oracle_libs):
    """three respawns share one epoch counter: source (0), box (1), source (2); the cloud is a twin's that runs untagged"""
    mesh, hi = srcbox["mesh"], srcbox["hi"]
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    okept = _source_ctx(ctx, srcbox, True)
    _source_ctx(twin, srcbox, True); twin.tag_disable()
    want = _origins(N, 5, 21)
    ctx.tag_set_origins(want)
    for c in (ctx, twin):
        c.set_sink_cells(srcbox["sink"]); c.sink_apply()
    dead = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert dead.size > 0.08 * N
    for c in (ctx, twin):
        c.respawn_source()
    pick = api.source_picks_host(SEED, dead, 0, hi)
    assert np.array_equal(pick, T.picks(SEED, dead, 0, hi))                  # the host entry is the statement's pick
    want[dead] = okept[pick]
    got = ctx.tag_origins()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert set(np.unique(want[dead])) == {1, 2, 3}
    # a box call: everybody dead gets the box's origin, also who the call leaves dead (x in (8, 9.5] is outside the mesh)
    first_layer = np.nonzero(mesh.cell_centres_volumes()[0][:, 0] < 1.0)[0]
    ctx.set_box_origin(4)
    for c in (ctx, twin):
        c.set_sink_cells(first_layer); c.sink_apply()
    again = np.nonzero(ctx.get_particles()[1] < 0)[0]
    for c in (ctx, twin):
        c.respawn_box((6.5, 0.5, 0.5), (9.5, 2.5, 1.5))
    want[again] = 4
    assert np.array_equal(ctx.tag_origins(), want)
    still = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert 0 < still.size < again.size and np.isin(still, again).all()
    # ... and the source call that places them stamps them again, at epoch 2
    for c in (ctx, twin):
        c.respawn_source()
    want[still] = okept[api.source_picks_host(SEED, still, 2, hi)]
    assert np.array_equal(ctx.tag_origins(), want) and (want[still] != 4).all()
    assert (api.source_picks_host(SEED, still, 1, hi) != api.source_picks_host(SEED, still, 2, hi)).any()
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and (a[1] >= 0).all()
    assert ctx.recycle_counts() == twin.recycle_counts() and ctx.recycle_counts()["epochs"] == 3
    # the position lies on the triangle whose origin the particle carries
    _, t, _, _, _ = SP.positions(SEED, still, 2, srcbox["rec"], hi, want_parts=True)
    assert np.array_equal(want[still], srcbox["origin_of_triangle"][srcbox["rec"][t, 14].astype(np.int64)])


def test_2_a_limited_respawn_and_the_call_that_places_the_rest(srcbox, gpu_ctx_factory):
    hi = srcbox["hi"]
    ctx = gpu_ctx_factory()
    okept = _source_ctx(ctx, srcbox, False)                                  # unsorted: array order is id order
    want = _origins(N, 5, 22)
    ctx.tag_set_origins(want)
    ctx.set_sink_cells(srcbox["sink"]); ctx.sink_apply()
    dead = np.nonzero(ctx.get_particles()[1] < 0)[0]
    ctx.respawn_source(dead.size // 2)                                       # EVERY candidate is stamped, also who stays dead
    want[dead] = okept[api.source_picks_host(SEED, dead, 0, hi)]
    assert np.array_equal(ctx.tag_origins(), want)
    rest = np.nonzero(ctx.get_particles()[1] < 0)[0]
    assert np.array_equal(rest, dead[dead.size // 2:])
    ctx.respawn_source()                                                     # the rest: stamped again, by this call's epoch
    want[rest] = okept[api.source_picks_host(SEED, rest, 1, hi)]
    got = ctx.tag_origins()
    assert np.array_equal(got, want) and (ctx.get_particles()[1] >= 0).all()
    assert (api.source_picks_host(SEED, rest, 0, hi) != api.source_picks_host(SEED, rest, 1, hi)).any()
    ctx.respawn_source(0)                                                    # max_count 0: no stamp, no respawn
    assert np.array_equal(ctx.tag_origins(), want)


@pytest.mark.parametrize("quads,drop", [(2048, False), (2049, False), (30, True)])
def test_2_tables_on_each_side_of_4096_and_one_with_dropped_triangles(gpu_ctx_factory, oracle_libs, quads, drop):
    mesh = box_mesh(32, 32, 2)
    tri, _ = mesh.face_triangles(np.arange(mesh.n_internal, mesh.n_faces)[:quads])
    m = tri.shape[0]
    assert m == 2 * quads
    weights = 1.0 + (np.arange(m) % 7)
    if drop:
        weights[::5] = 0.0
    rec, hi = api.source_table_host(tri, weights, (0.01, 0.25))
    assert hi.size == (m if not drop else m - m // 5)
    origin_of_triangle = (np.arange(m) * 7 + 3) % 16
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_seed(SEED); ctx.set_source_triangles(tri, weights, (0.01, 0.25))
    ctx.set_particles(np.full((N, 3), -1.0), np.full(N, L.CELL_LOST, np.int32))      # everybody dead
    ctx.tag_enable(16, 1)
    ctx.set_source_origins(origin_of_triangle)
    ctx.respawn_source()
    pick = T.picks(SEED, np.arange(N), 0, hi)                                # the numpy pick on the oracle's Philox
    assert np.array_equal(api.source_picks_host(SEED, None, 0, hi, n=N), pick)
    want = T.origin_of_kept(rec, origin_of_triangle)[pick]
    got = ctx.tag_origins()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert pick.min() < 8 and pick.max() > hi.size - 8 and np.unique(want).size == 16
    assert (ctx.get_particles()[1] >= 0).all()
    # a new table resets every triangle to origin 0
    ctx.set_particles(np.full((N, 3), -1.0), np.full(N, L.CELL_LOST, np.int32))
    ctx.tag_enable(16, 1); ctx.set_source_origins(origin_of_triangle)
    ctx.set_source_triangles(tri, weights, (0.01, 0.25))
    ctx.respawn_source()
    assert not ctx.tag_origins().any()


def test_2_a_cloud_without_a_dead_slot(srcbox, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    _source_ctx(ctx, srcbox, True)
    want = _origins(N, 5, 23)
    ctx.tag_set_origins(want)
    ctx.set_box_origin(4)
    ctx.respawn_source(); ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 3.0, 2.0))
    assert np.array_equal(ctx.tag_origins(), want)
    assert ctx.recycle_counts() == dict(absorbed=0, drawn=0, placed=0, epochs=2)


# ------------------------------------------------------------------------------------------------ 3. the field against numpy
@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)))


@pytest.mark.parametrize("n_origins", [1, 3, 16])
@pytest.mark.parametrize("sort", [True, False])
def test_3_one_sample_is_the_bincount_of_the_virtual_id(box, gpu_ctx_factory, sort, n_origins):
    """sort: a slice spans a handful of cells (the dense window); all of these windows fit the bins (60 cells x 16 origins)"""
    ctx = gpu_ctx_factory()
    _located(ctx, box["mesh"], box["xyz"], sort)
    ctx.tag_enable(n_origins, 1)
    f, ns = ctx.tag_field()
    assert f.dtype == np.uint64 and f.shape == (n_origins, 60) and not f.any() and ns == 0
    origin = _origins(N, n_origins, 50 + n_origins)
    ctx.tag_set_origins(origin)
    ctx.tag_sample()
    f, ns = ctx.tag_field()
    want = T.field(ctx.get_particles()[1], origin, 60, n_origins)
    assert ns == 1 and np.array_equal(f, want) and int(f.sum()) == N and (f.sum(1) > 0).all()
    ctx.occupancy_sample()
    assert np.array_equal(f.sum(0), ctx.occupancy()[0])                      # summed over the origins: an occupancy sample
    V = ctx.cell_volumes()
    assert np.array_equal(ctx.origin_concentration(), want.astype(np.float64) / (1.0 * V[None, :]))
    frac = ctx.origin_fraction()
    assert frac.shape == (n_origins, 60) and np.allclose(frac.sum(0), 1.0, rtol=0, atol=1e-14)


def test_3_a_window_wider_than_the_bins_goes_through_the_cache(gpu_ctx_factory):
    """an unsorted cloud on 1200 cells with 16 origins: every slice's window of virtual ids is wider than the 4096 bins"""
    mesh = box_mesh(12, 10, 10)
    xyz = pz.uniform_points(81, N, (0.0, 0.0, 0.0), (12.0, 10.0, 10.0))
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, False)
    cell = ctx.get_particles()[1]
    origin = _origins(N, 16, 60)
    for lo in range(0, N, 4096):
        v = cell[lo:lo + 4096].astype(np.int64) * 16 + origin[lo:lo + 4096]
        assert v.max() - v.min() + 1 > T.FIELD_BINS
    ctx.tag_enable(16, 1); ctx.tag_set_origins(origin)
    ctx.tag_sample(); ctx.tag_sample()
    f, ns = ctx.tag_field()
    assert ns == 2 and np.array_equal(f, 2 * T.field(cell, origin, mesh.n_cells, 16)) and int(f.sum()) == 2 * N


def test_3_decomposed_cells_sum_per_parent(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(20_000, 3))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    assert ctx.mesh_quality()["n_derived"] > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.step(0.05, 0.0, 5)
    ctx.tag_enable(3, 1)
    origin = _origins(20_000, 3, 61)
    ctx.tag_set_origins(origin)
    ctx.tag_sample()
    f, ns = ctx.tag_field()
    want = T.field(ctx.get_particles()[1], origin, 120, 3)                   # parent ids
    assert f.shape == (3, 120) and ns == 1 and np.array_equal(f, want) and int(f.sum()) == 20_000


def test_3_samples_accumulate_across_steps_resorts_and_recycling(box, gpu_ctx_factory):
    mesh = box["mesh"]
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", 3)
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.5
    U[:, 0] += 1.0
    ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(box["xyz"]); ctx.set_seed(SEED)
    ctx.locate_initial()
    ctx.tag_enable(3, 2)
    ctx.set_sink_groups(box["sink"], np.arange(box["sink"].size) % 2)
    ctx.set_box_origin(2)
    ctx.tag_set_origins(_origins(N, 2, 62))                                  # origins 0 and 1; 2 is the box's
    want = np.zeros((3, 60), np.uint64)
    for k in range(3):
        ctx.step(0.05, 1e-3, 4)                                              # (a re-sort falls into every one of these)
        ctx.sink_apply()
        if k == 1:
            ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))                # k == 0, 2: the absorbed stay dead through the sample
        ctx.tag_sample(); ctx.occupancy_sample()
        cell = ctx.get_particles()[1]
        dead = int((cell < 0).sum())
        assert (dead > 0) == (k != 1)
        want += T.field(cell, ctx.tag_origins(), 60, 3)
        f, ns = ctx.tag_field()
        occ, ns_occ = ctx.occupancy()
        assert ns == ns_occ == k + 1 and np.array_equal(f, want)
        assert np.array_equal(f.sum(0), occ)                                 # at every sample: summed over origins, the occupancy
    assert want[2].any() and (ctx.tag_origins() == 2).any()                  # the respawned carry the box's origin
    assert int(ctx.transfer().sum()) == ctx.recycle_counts()["absorbed"] > 0
    # reset zeroes the matrix, the field and the sample count and leaves the origins
    origins = ctx.tag_origins()
    ctx.tag_reset()
    f, ns = ctx.tag_field()
    assert ns == 0 and not f.any() and not ctx.transfer().any() and np.array_equal(ctx.tag_origins(), origins)
    assert np.isnan(ctx.origin_fraction()).all()
    with pytest.raises(ValueError):
        ctx.origin_concentration()
    ctx.tag_sample()                                                         # ... and it starts again from zero
    f, ns = ctx.tag_field()
    assert ns == 1 and np.array_equal(f, T.field(ctx.get_particles()[1], origins, 60, 3))


# ---- the adversarial id arrays of tests/test_gpu_occupancy.py / test_gpu_age.py as the cells of the context's own cloud
BIG = (40, 30, 30)


@pytest.fixture(scope="module")
def big_ctx():
    with api.Context(0) as ctx:
        ctx.set_mesh(box_mesh(*BIG))
        yield ctx


@pytest.mark.parametrize("n_origins", [16, 1])
@pytest.mark.parametrize("name", T.ADVERSARIAL)
def test_3_adversarial_cell_arrays(big_ctx, name, n_origins):
    c, o = T.adversarial(name, n_origins)
    big_ctx.set_particles(np.zeros((c.size, 3)), c)                          # the cells as given; gid = index
    big_ctx.tag_enable(n_origins, 1)
    big_ctx.tag_set_origins(o)
    big_ctx.tag_sample()
    f, ns = big_ctx.tag_field()
    want = T.field(np.where((c >= 0) & (c < T.N_BIG), c, -1), o, T.N_BIG, n_origins)
    assert ns == 1 and np.array_equal(f, want), (name, np.nonzero(f != want))


# ------------------------------------------------------------------------------------------------ 4. whole recycled runs
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_4_a_recycled_run_carries_its_tags(name, gpu_ctx_factory, oracle_libs):
    """tests/test_gpu_source.py's whole runs with tagging on and off: the same bits either way, and the CPU statement's; the
    transfer matrix, the origins and the field are the statement's (tests/tags.py)."""
    r, c = T.run(name), T.cpu(name)
    b = r.base
    out = {}
    for tagged in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", b.sort_interval)
        ctx.set_mesh(b.mesh); ctx.set_velocity(b.U); ctx.set_seed(SEED)
        ctx.synchronize()
        ctx.set_source_triangles(b.tri, b.weights, b.depth)
        ctx.set_particles(b.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(b.sink_cells)
        if tagged:
            ctx.tag_enable(T.N_ORIGINS, T.N_SINKS)
            ctx.set_sink_groups(b.sink_cells, r.groups)
            ctx.set_source_origins(r.origin_of_triangle)
        for k in range(b.rounds):
            ctx.step(b.dt, 0.0, b.cycles)
            ctx.sink_apply()
            ctx.respawn_source()
            if tagged:
                ctx.tag_sample(); ctx.occupancy_sample()
        out[tagged] = ctx.get_particles()
        assert ctx.recycle_counts() == dict(absorbed=c["absorbed"], drawn=c["drawn"], placed=c["placed"], epochs=b.rounds)
        if tagged:
            origin, transfer, (field, ns), occ = ctx.tag_origins(), ctx.transfer(), ctx.tag_field(), ctx.occupancy()[0]
    for tagged in (True, False):
        xyzw, cell = out[tagged]
        bad = np.nonzero(cell != c["cell"])[0]
        assert bad.size == 0, (name, tagged, "cells differ", bad.size, bad[:5], cell[bad[:5]], c["cell"][bad[:5]])
        bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(c["xyz"])).any(1))[0]
        assert bad.size == 0, (name, tagged, "positions differ", bad.size, bad[:5])
    assert np.array_equal(_bits(out[True][0]), _bits(out[False][0]))
    bad = np.nonzero(origin != c["origin"])[0]
    assert bad.size == 0, (name, "origins differ", bad.size, bad[:5], origin[bad[:5]], c["origin"][bad[:5]])
    assert np.array_equal(transfer, c["transfer"]), (transfer, c["transfer"])
    assert int(transfer.sum()) == c["absorbed"] >= 200 and (transfer[1:] > 0).all()
    assert ns == c["samples"] and np.array_equal(field, c["field"]) and np.array_equal(field.sum(0), occ)
    assert np.array_equal(occ, c["occupancy"])


# ------------------------------------------------------------------------------------------------ 5. state and errors
def test_5_state_and_argument_errors(box, srcbox):
    def refused(status, call):
        with pytest.raises(L.CpfError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert str(e.value)                                                  # ... with a message

    sink, mesh = box["sink"], box["mesh"]
    with api.Context(0) as ctx:
        needs_on = (ctx.tag_sample, ctx.tag_reset, ctx.transfer, ctx.tag_field, ctx.tag_origins, lambda: ctx.set_box_origin(0),
                    lambda: ctx.set_sink_groups(sink, np.zeros(sink.size)), lambda: ctx.set_source_origins(np.zeros(12)),
                    lambda: ctx._ck(ctx.lib.cpf_tag_set_origins(ctx.h, api._ptr(np.zeros(N, np.uint8)))))
        refused(L.CPF_ERR_STATE, lambda: ctx.tag_enable(1, 1))               # no mesh
        ctx.set_mesh(mesh)
        refused(L.CPF_ERR_STATE, lambda: ctx.tag_enable(1, 1))               # no cloud
        ctx.set_particles(box["xyz"])
        refused(L.CPF_ERR_STATE, lambda: ctx.tag_enable(1, 1))               # ... set, but not located
        for g in needs_on:
            refused(L.CPF_ERR_STATE, g)
        ctx.tag_disable()                                                    # off already: no error
        ctx.locate_initial()
        for no, nk in ((0, 1), (17, 1), (1, 0), (1, 17), (-1, 1), (1, -1)):  # sizes outside [1, 16]
            refused(L.CPF_ERR_ARG, lambda: ctx.tag_enable(no, nk))
        for g in needs_on:
            refused(L.CPF_ERR_STATE, g)                                      # a refused enable leaves tagging off
        ctx.tag_enable(16, 16)
        ctx.tag_enable(3, 2)                                                 # again: everything anew
        assert ctx.transfer().shape == (3, 2) and ctx.tag_field()[0].shape == (3, 60)
        # a group outside [0, nSinks), a cell outside the mesh: the sink set stays as it was
        ctx.set_sink_groups(sink, np.arange(sink.size) % 2)
        refused(L.CPF_ERR_ARG, lambda: ctx.set_sink_groups(sink, np.full(sink.size, 2)))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_sink_groups(sink, np.full(sink.size, -1)))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_sink_groups([60], [0]))
        with pytest.raises(ValueError):
            ctx.set_sink_groups(sink, [0])
        # an origin outside [0, nOrigins)
        refused(L.CPF_ERR_ARG, lambda: ctx.set_box_origin(3))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_box_origin(-1))
        refused(L.CPF_ERR_ARG, lambda: ctx.tag_set_origins(np.full(N, 3, np.uint8)))
        with pytest.raises(ValueError):
            ctx.tag_set_origins(np.zeros(3, np.uint8))
        refused(L.CPF_ERR_STATE, lambda: ctx.set_source_origins(np.zeros(12)))                   # no source yet
        ctx.set_source_triangles(srcbox["tri"][:, :, [0, 1, 2]] * [1.0, 4.0 / 3.0, 1.5], None, DEPTH)
        refused(L.CPF_ERR_ARG, lambda: ctx.set_source_origins(np.full(12, 3)))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_source_origins(np.full(12, -1)))
        refused(L.CPF_ERR_ARG, lambda: ctx.set_source_origins(np.zeros(11)))                     # fewer entries than triangles
        ctx.set_source_origins(np.arange(12) % 3)
        assert ctx.lib.cpf_get_transfer(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_tag_get_origins(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_tag_set_origins(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_tag_field(ctx.h, None, None) == L.CPF_OK                          # each output is nullable
        # the groups that were accepted are still in force
        ctx.tag_set_origins(np.full(N, 1, np.uint8))
        _, cell = ctx.get_particles()
        ctx.sink_apply()
        want = T.transfer(np.full(N, 1), T.group_of_cell(60, sink, np.arange(sink.size) % 2), cell, np.isin(cell, sink), 3, 2)
        assert np.array_equal(ctx.transfer(), want) and (want[1] > 0).all()
        # a new cloud and a new mesh each turn tagging off
        ctx.seed_box(N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        refused(L.CPF_ERR_STATE, ctx.transfer)
        ctx.locate_initial(); ctx.tag_enable(2, 2)
        ctx.set_particles(box["xyz"])
        refused(L.CPF_ERR_STATE, ctx.tag_origins)
        ctx.locate_initial(); ctx.tag_enable(2, 2)
        ctx.set_mesh(mesh)
        refused(L.CPF_ERR_STATE, ctx.tag_field)
        ctx.set_particles(box["xyz"]); ctx.locate_initial(); ctx.tag_enable(2, 2); ctx.tag_sample()
        assert ctx.tag_field()[1] == 1
        ctx.tag_disable()
        refused(L.CPF_ERR_STATE, ctx.tag_sample)
        # with tagging off again the sink and the respawn are the plain ones
        ctx.recycle_reset_counts()                                           # (the counters belong to the context: the sink above counted)
        ctx.set_sink_cells(sink); ctx.sink_apply()
        ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))
        k = ctx.recycle_counts()
        assert k["absorbed"] == k["drawn"] == k["placed"] > 0 and (ctx.get_particles()[1] >= 0).all()


# ------------------------------------------------------------------------------------------------ 6. through CudaParticles
def test_6_cuda_particles_sink_groups_and_source_origins(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13                                                          # 10 * dt / dt == 10 exactly
    sink = mesh.patch_cells("outlet")
    centres = pitz["centres"]
    groups = (centres[sink, 1] > np.median(centres[sink, 1])).astype(np.int32)
    tri, of = mesh.face_triangles(mesh.patch_faces("inlet"))
    y = tri.mean(1)[:, 1]
    origins = np.where(y > np.median(y), 2, 1).astype(np.int32)              # 0 is the initial cloud
    # seeded over the whole domain, so that the outlet's cells hold particles from the first recycle point on
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=2,
             occupancyInterval=4, sinkCells=sink, sourceTriangles=tri, sourceWeights=api.inflow_weights(mesh, U, tri, of),
             sourceDepth=(0.0, 1e-4))
    p = api.CudaParticles(mesh, U, dict(d, sinkGroups=groups, sourceOrigins=origins))
    q = api.CudaParticles(mesh, U, d)
    only_groups = api.CudaParticles(mesh, U, dict(d, sinkGroups=groups))
    try:
        assert p.tags and not q.tags and only_groups.tags
        for k in range(3):
            for run in (p, q, only_groups):
                assert run.advect(k * 10 * dt, 10 * dt) == 10
        T_ = p.transfer()
        absorbed = p.recycle_counts()["absorbed"]
        assert T_.shape == (3, 2) and int(T_.sum()) == absorbed > 0 and (T_[0] > 0).all()
        assert only_groups.transfer().shape == (1, 2) and np.array_equal(only_groups.transfer()[0], T_.sum(0))
        f, ns = p.ctx.tag_field()
        occ, ns_occ = p.ctx.occupancy()
        assert ns == ns_occ == 7 and np.array_equal(f.sum(0), occ)
        frac = p.origin_fraction()
        seen = occ > 0
        assert frac.shape == (3, mesh.n_cells) and np.isnan(frac[:, ~seen]).all()
        assert np.allclose(frac[:, seen].sum(0), 1.0, rtol=0, atol=1e-14) and (frac[:, seen] >= 0).all()
        got = p.ctx.tag_origins()
        assert set(np.unique(got)) == {0, 1, 2}                              # both halves of the inlet have fed the cloud
        # tagging changes nothing of the run
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        assert np.array_equal(p.concentration(), q.concentration())
        with pytest.raises(L.CpfError):
            q.transfer()
        with pytest.raises(ValueError):
            api.CudaParticles(mesh, U, dict(d, sinkGroups=groups, recycleInterval=0)).close()
    finally:
        p.close(); q.close(); only_groups.close()
