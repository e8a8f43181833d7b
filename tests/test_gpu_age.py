"""GPU: tracer age (include/cpf.h "tracer age"; csrc/cpf_age.hip).  Everything is integers and every comparison is exact: the
residence-time histogram and the age field against the numpy statement of tests/age.py over what ``get_particles()`` returns, the
stamps through whole recycled runs against the CPU statement, and the cloud itself against a twin context without tracking."""
import numpy as np
import pytest

import age as A
import recycle as R
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = R.N                                      # 10 007: a multiple of neither 64, 256 nor 1024
NOW = 5                                      # cycles the clouds of tests 1, 2 and 4 have run (at rest) when tracking starts


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


def _births(want_ages, now=NOW):
    return ((np.int64(now) - np.asarray(want_ages, np.int64)) % (2 ** 32)).astype(np.uint32)


def _at_rest(ctx, mesh, xyz, sort, cell=None):
    """a located cloud that has run NOW cycles in a fluid at rest: the cycle counter is NOW, nobody moved"""
    ctx.set_mesh(mesh); ctx.set_velocity(np.zeros((mesh.n_cells, 3))); ctx.set_seed(R.SEED)
    ctx.set_particles(xyz, cell)
    if cell is None:
        assert ctx.locate_initial() == 0
    ctx.step(0.1, 0.0, NOW)
    if sort:
        ctx.sort_by_cell()


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)))


def _edge_ages(bin_cycles, n_bins, n, seed):
    """ages on every bin edge the issue names -- 0, binCycles - 1, binCycles, the open bin's lower edge - 1, + 0, + 1000, and a birth
    one cycle AFTER now (age 2^32 - 1) -- on every third id, random ones over all bins elsewhere"""
    rng = np.random.default_rng(seed)
    top = (n_bins - 1) * bin_cycles
    edges = np.array([0, bin_cycles - 1, bin_cycles, top - 1, top, top + 1000, -1], np.int64) % (2 ** 32)
    a = rng.integers(0, n_bins * bin_cycles + 5, size=n).astype(np.int64)
    a[::3] = edges[np.arange(a[::3].size) % edges.size]
    return a


# ------------------------------------------------------------------------------------------------ 1. absorb against numpy
@pytest.mark.parametrize("bin_cycles,n_bins", [(1, 1), (1, 4096), (7, 16), (1000, 3)])
@pytest.mark.parametrize("sort", [True, False])
def test_1_absorb_bins_the_ages_of_exactly_the_absorbed(box, gpu_ctx_factory, sort, bin_cycles, n_bins):
    """sort: fresh from cpf_sort_by_cell (gid permuted, hits in runs); without: gid = index, hits scattered"""
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _at_rest(c, box["mesh"], box["xyz"], sort)
        c.set_sink_cells(box["sink"])
    _, cell0 = ctx.get_particles()
    want_ages = _edge_ages(bin_cycles, n_bins, N, 40 + n_bins)
    ctx.age_enable(bin_cycles, n_bins)
    assert np.array_equal(ctx.age_births(), np.full(N, NOW, np.uint32)) and not ctx.ages().any()      # everybody is born now
    ctx.age_set_births(_births(want_ages))
    assert np.array_equal(ctx.ages(), want_ages)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, box["sink"])
    assert 0.15 * N < hit.sum() < 0.25 * N                                   # one layer in five
    want = A.rtd(want_ages[hit], bin_cycles, n_bins)
    got = ctx.age_histogram()
    assert got.dtype == np.uint64 and np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    assert int(got.sum()) == int(hit.sum())
    if n_bins >= 3:
        assert want[0] > 0 and want[1] > 0 and want[-1] > 0 and want[-2] > 0
    # the cloud is the twin's, which ran the plain sink: cells, positions, the count
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], R.sink(cell0, box["sink"])) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert ctx.recycle_counts() == twin.recycle_counts() == dict(absorbed=int(hit.sum()), drawn=0, placed=0, epochs=0)
    assert np.array_equal(ctx.ages(), np.where(hit, -1, want_ages))          # the absorbed are dead slots: no age
    ctx.sink_apply()                                                         # a second apply finds nobody
    assert np.array_equal(ctx.age_histogram(), want)
    edges, counts = ctx.rtd(0.5)
    assert np.array_equal(counts, want) and edges.shape == (n_bins + 1,) and edges[0] == 0.0 and np.isinf(edges[-1])
    assert n_bins == 1 or edges[1] == 0.5 * bin_cycles


# ------------------------------------------------------------------------------------------------ 2. all-hit slices, the mask outside LDS
@pytest.mark.parametrize("sort", [True, False])
def test_2_every_particle_of_two_slices_and_a_tail_is_absorbed(gpu_ctx_factory, sort):
    mesh = box_mesh(5, 4, 3)
    n = 8200                                                                 # two slices of 4096 ids and a tail of 8
    xyz = pz.uniform_points(5, n, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))          # all in the last x layer
    ctx = gpu_ctx_factory()
    _at_rest(ctx, mesh, xyz, sort)
    ctx.set_sink_cells(_last_x_layer(mesh))
    ctx.age_enable(7, 16)
    want_ages = _edge_ages(7, 16, n, 8)
    ctx.age_set_births(_births(want_ages))
    ctx.sink_apply()
    assert np.array_equal(ctx.age_histogram(), A.rtd(want_ages, 7, 16))
    assert ctx.recycle_counts()["absorbed"] == n and (ctx.get_particles()[1] == -1).all() and (ctx.ages() == -1).all()


BIG_SINK = (41, 40, 40)                                                      # 65 600 cells: more bits than the 2048 staged words hold
N_BIG = 36_000


def test_2_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(*BIG_SINK)
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    xyz = pz.uniform_points(79, N_BIG, (0.0, 0.0, 0.0), tuple(float(v) for v in BIG_SINK))
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _at_rest(c, mesh, xyz, True)
        c.set_sink_cells(sink)
    _, cell0 = ctx.get_particles()
    ctx.age_enable(7, 16)
    want_ages = _edge_ages(7, 16, N_BIG, 9)
    ctx.age_set_births(_births(want_ages))
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert hit.sum() > 500
    assert np.array_equal(ctx.age_histogram(), A.rtd(want_ages[hit], 7, 16))
    assert np.array_equal(ctx.get_particles()[1], twin.get_particles()[1]) and ctx.recycle_counts() == twin.recycle_counts()
    assert ctx.recycle_counts()["absorbed"] == int(hit.sum())


# ------------------------------------------------------------------------------------------------ 3. stamps through a recycled run
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_3_a_recycled_run_carries_its_stamps(name, gpu_ctx_factory, oracle_libs):
    """tests/test_gpu_recycle.py's whole runs with tracking on and off: the same bits either way, and the CPU statement's; births,
    ages and the residence-time histogram are the statement's (tests/age.py).  "thin box" takes one LIMITED respawn (half the dead) in
    its sixth round: the slots it leaves dead have no age, and get the stamp of the round that places them."""
    r, c = R.run(name), A.cpu(name)
    limited = A.LIMITED_ROUND[name]
    out = {}
    for track in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", r.sort_interval)
        ctx.set_mesh(r.mesh); ctx.set_velocity(r.U); ctx.set_seed(R.SEED)
        ctx.synchronize()
        ctx.set_particles(r.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(r.sink_cells)
        if track:
            ctx.age_enable(A.BIN_CYCLES, A.N_BINS)
        for k in range(r.rounds):
            ctx.step(r.dt, 0.0, r.cycles)
            ctx.sink_apply()
            if k == limited:
                ctx.respawn_box(r.box[0], r.box[1], c["limited_count"])
                if track:
                    mid = ctx.ages()
                    assert np.array_equal(mid, c["mid_ages"])
                    assert (mid[c["left_dead"]] == -1).all() and (mid == -1).sum() == c["left_dead"].size
            else:
                ctx.respawn_box(r.box[0], r.box[1])
        out[track] = ctx.get_particles()
        assert ctx.recycle_counts() == dict(absorbed=c["absorbed"], drawn=c["drawn"], placed=c["placed"], epochs=r.rounds)
        if track:
            births, ages, hist = ctx.age_births(), ctx.ages(), ctx.age_histogram()
    for track in (True, False):
        xyzw, cell = out[track]
        bad = np.nonzero(cell != c["cell"])[0]
        assert bad.size == 0, (name, track, "cells differ", bad.size, bad[:5], cell[bad[:5]], c["cell"][bad[:5]])
        bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(c["xyz"])).any(1))[0]
        assert bad.size == 0, (name, track, "positions differ", bad.size, bad[:5])
    assert np.array_equal(_bits(out[True][0]), _bits(out[False][0]))
    bad = np.nonzero(births != c["births"])[0]
    assert bad.size == 0, (name, "births differ", bad.size, bad[:5], births[bad[:5]], c["births"][bad[:5]])
    assert np.array_equal(ages, c["ages"]) and ((ages == -1) == (c["cell"] < 0)).all()
    assert np.array_equal(hist, c["hist"]), (hist, c["hist"])
    assert int(hist.sum()) == c["absorbed"] >= 200 and (hist > 0).sum() >= 4 and (c["times_absorbed"] >= 2).any()
    if name == "graded box":
        assert (ages == -1).any()                                            # the dead slots the sticking-out box leaves


# ------------------------------------------------------------------------------------------------ 4. the age field against numpy
def _want_field(ctx, now, n_cells):
    return A.field(ctx.get_particles()[1], A.ages(now, ctx.age_births()), n_cells)


def test_4_one_sample_is_the_two_bincounts(box, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    _at_rest(ctx, box["mesh"], box["xyz"], True)
    ctx.age_enable(1, 4)
    s, c, ns = ctx.age_field()
    assert s.dtype == c.dtype == np.uint64 and s.shape == c.shape == (60,) and not s.any() and not c.any() and ns == 0
    want_ages = _edge_ages(1000, 3, N, 4)                                    # among them 2^32 - 1: sums beyond 32 bits
    ctx.age_set_births(_births(want_ages))
    ctx.age_sample()
    s, c, ns = ctx.age_field()
    ws, wc = A.field(ctx.get_particles()[1], want_ages, 60)
    assert ns == 1 and np.array_equal(c, wc) and np.array_equal(s, ws) and int(c.sum()) == N and s.max() > 2 ** 32
    m = ctx.mean_age(0.25)
    assert np.array_equal(m, ws.astype(np.float64) / wc.astype(np.float64) * 0.25)
    ctx.occupancy_sample()
    assert np.array_equal(c, ctx.occupancy()[0])                             # the count is an occupancy sample's


def test_4_samples_accumulate_across_steps_resorts_and_recycling(box, gpu_ctx_factory):
    mesh = box["mesh"]
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", 3)
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.5
    U[:, 0] += 1.0
    ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(box["xyz"]); ctx.set_seed(R.SEED)
    ctx.locate_initial()
    ctx.set_sink_cells(box["sink"])
    ctx.age_enable(2, 8)
    ws, wc, now = np.zeros(60, np.uint64), np.zeros(60, np.uint64), 0
    for k in range(3):
        ctx.step(0.05, 1e-3, 4); now += 4                                    # (a re-sort falls into every one of these)
        ctx.sink_apply()
        if k == 1:
            ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))                # k == 0, 2: the absorbed stay dead through the sample
        ctx.age_sample()
        s, c = _want_field(ctx, now, 60)
        dead = int((ctx.get_particles()[1] < 0).sum())
        assert int(c.sum()) == N - dead and (dead > 0) == (k != 1)           # dead slots are not counted
        ws += s; wc += c
    s, c, ns = ctx.age_field()
    assert ns == 3 and np.array_equal(c, wc) and np.array_equal(s, ws) and s.any()
    assert np.unique(ctx.age_births()).size >= 2                             # the respawned carry another stamp
    # reset zeroes the histogram and the field and leaves the stamps
    births = ctx.age_births()
    assert ctx.age_histogram().any()
    ctx.age_reset()
    s, c, ns = ctx.age_field()
    assert ns == 0 and not s.any() and not c.any() and not ctx.age_histogram().any()
    assert np.array_equal(ctx.age_births(), births)
    assert np.isnan(ctx.mean_age(1.0)).all()
    ctx.age_sample()                                                         # ... and it starts again from zero
    s, c, ns = ctx.age_field()
    w = _want_field(ctx, now, 60)
    assert ns == 1 and np.array_equal(s, w[0]) and np.array_equal(c, w[1])


def test_4_decomposed_cells_sum_per_parent(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(20_000, 3))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    assert ctx.mesh_quality()["n_derived"] > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.step(0.05, 0.0, 5)
    ctx.age_enable(1, 2)
    want_ages = rng.integers(0, 2 ** 32, size=20_000)
    ctx.age_set_births(_births(want_ages, 5))
    ctx.age_sample()
    s, c, ns = ctx.age_field()
    ws, wc = A.field(ctx.get_particles()[1], want_ages, 120)                 # parent ids
    assert s.size == 120 and ns == 1 and np.array_equal(c, wc) and np.array_equal(s, ws) and int(c.sum()) == 20_000


# ---- the adversarial id arrays of tests/test_gpu_occupancy.py as the cells of the context's own cloud: 36 000 cells
BIG = (40, 30, 30)


def _adversarial(name):
    rng = np.random.default_rng(11)
    if name == "one_cell":
        return np.full(70_001, 12_345, np.int32)
    if name == "two_alternating":
        return np.where(np.arange(4097) % 2 == 0, 7, 35_999).astype(np.int32)
    if name == "two_aliasing":                                               # far apart and in the same bin modulo 1024 and 2048
        return np.where(np.arange(4097) % 2 == 0, 5, 5 + 3 * 2048 * 5).astype(np.int32)
    if name == "permutation_with_lost":
        c = rng.permutation(N_BIG).astype(np.int32)
        c[::7] = -1
        return c
    if name == "sorted_sparse":                                              # the window of a slice overflows the LDS bins
        return np.sort(rng.choice(N_BIG, size=5000, replace=False)).astype(np.int32)
    if name == "sorted_dense":                                               # several workgroups, each with a wide LDS window
        return np.sort(rng.integers(0, N_BIG, size=50_001)).astype(np.int32)
    if name == "window_edge":                                                # windows of exactly 2048 and 2049 cells, one slice each
        a = np.concatenate([[100], rng.integers(100, 100 + 2048, size=4094), [100 + 2047]])
        b = np.concatenate([[9000], rng.integers(9000, 9000 + 2049, size=4094), [9000 + 2048]])
        return np.concatenate([a, b]).astype(np.int32)
    if name == "codes_and_foreign_ids":                                      # frozen, lost, ids that are no cells of the mesh
        c = rng.integers(0, N_BIG, size=9001).astype(np.int32)
        c[::5] = -2; c[1::5] = N_BIG; c[2::5] = np.iinfo(np.int32).max; c[3::11] = np.iinfo(np.int32).min
        return c
    return rng.integers(0, N_BIG, size=int(name[1:])).astype(np.int32)       # "n<length>"


@pytest.fixture(scope="module")
def big_ctx():
    with api.Context(0) as ctx:
        ctx.set_mesh(box_mesh(*BIG))
        yield ctx


@pytest.mark.parametrize("name", ["one_cell", "two_alternating", "two_aliasing", "permutation_with_lost", "sorted_sparse", "sorted_dense",
                                  "window_edge", "codes_and_foreign_ids", "n1", "n63", "n64", "n65", "n4099"])
def test_4_adversarial_cell_arrays(big_ctx, name):
    c = _adversarial(name)
    rng = np.random.default_rng(c.size)
    big_ctx.set_particles(np.zeros((c.size, 3)), c)                          # the cells as given; gid = index
    big_ctx.age_enable(1, 1)
    want_ages = rng.integers(0, 2 ** 32, size=c.size)
    want_ages[::4] = 2 ** 32 - 1
    big_ctx.age_set_births(_births(want_ages, 0))
    big_ctx.age_sample()
    s, cnt, ns = big_ctx.age_field()
    ws, wc = A.field(np.where((c >= 0) & (c < N_BIG), c, -1), want_ages, N_BIG)
    assert ns == 1 and np.array_equal(cnt, wc), name
    assert np.array_equal(s, ws), name


# ------------------------------------------------------------------------------------------------ 5. state and errors
def test_5_state_and_argument_errors(box):
    def refused(status, call):
        with pytest.raises(L.CpfError) as e:
            call()
        assert e.value.status == status, str(e.value)

    with api.Context(0) as ctx:
        getters = (ctx.age_histogram, ctx.age_field, ctx.ages, ctx.age_births, ctx.age_sample, ctx.age_reset)
        refused(L.CPF_ERR_STATE, lambda: ctx.age_enable(1, 4))               # no mesh
        ctx.set_mesh(box["mesh"])
        refused(L.CPF_ERR_STATE, lambda: ctx.age_enable(1, 4))               # no cloud
        ctx.set_particles(box["xyz"])
        refused(L.CPF_ERR_STATE, lambda: ctx.age_enable(1, 4))               # ... set, but not located
        for g in getters:
            refused(L.CPF_ERR_STATE, g)
        assert ctx.lib.cpf_age_set_births(ctx.h, api._ptr(np.zeros(N, np.uint32))) == L.CPF_ERR_STATE
        assert ctx.lib.cpf_get_age_histogram(ctx.h, api._ptr(np.zeros(4, np.uint64)), 4) == L.CPF_ERR_STATE
        ctx.age_disable()                                                    # off already: no error
        ctx.locate_initial()
        for bc, nb in ((1, 0), (1, 4097), (0, 4), (-1, 4), (1, -1)):
            refused(L.CPF_ERR_ARG, lambda: ctx.age_enable(bc, nb))
        for g in getters:
            refused(L.CPF_ERR_STATE, g)                                      # a refused enable leaves tracking off
        ctx.age_enable(1, 4096)
        ctx.age_enable(3, 4)                                                 # again: everything anew
        assert ctx.age_histogram().shape == (4,)
        assert ctx.lib.cpf_get_age_histogram(ctx.h, api._ptr(np.zeros(8, np.uint64)), 8) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_age_histogram(ctx.h, None, 4) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_age_field(ctx.h, None, None, None) == L.CPF_OK                    # each output is nullable
        with pytest.raises(ValueError):
            ctx.age_set_births(np.zeros(3, np.uint32))
        # a new cloud and a new mesh each turn tracking off
        ctx.seed_box(N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        refused(L.CPF_ERR_STATE, ctx.age_histogram)
        ctx.locate_initial(); ctx.age_enable(1, 4)
        ctx.set_particles(box["xyz"])
        refused(L.CPF_ERR_STATE, ctx.ages)
        ctx.locate_initial(); ctx.age_enable(1, 4)
        ctx.set_mesh(box["mesh"])
        refused(L.CPF_ERR_STATE, ctx.age_field)
        ctx.set_particles(box["xyz"]); ctx.locate_initial(); ctx.age_enable(1, 4); ctx.age_sample()
        assert ctx.age_field()[2] == 1
        ctx.age_disable()
        refused(L.CPF_ERR_STATE, ctx.age_sample)
        # with tracking off again the sink and the respawn are the plain ones
        ctx.set_sink_cells(box["sink"]); ctx.sink_apply()
        ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))
        k = ctx.recycle_counts()
        assert k["absorbed"] == k["drawn"] == k["placed"] > 0 and (ctx.get_particles()[1] >= 0).all()


# ------------------------------------------------------------------------------------------------ 6. through CudaParticles
def test_6_cuda_particles_age_bins(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13                                                          # 10 * dt / dt == 10 exactly
    lo, hi = pz.DOMAIN_BOX
    # seeded over the whole domain, so that the outlet's cells hold particles from the first recycle point on
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=2,
             occupancyInterval=4, sinkCells=mesh.patch_cells("outlet"), sourceBox=(lo, (lo[0] + 0.1 * (hi[0] - lo[0]), hi[1], hi[2])),
             ageBins=8)
    p = api.CudaParticles(mesh, U, d)
    q = api.CudaParticles(mesh, U, {k: v for k, v in d.items() if k != "ageBins"})
    try:
        assert (p.ageBins, p.ageBinCycles) == (8, 2)
        for k in range(3):
            assert p.advect(k * 10 * dt, 10 * dt) == 10 and q.advect(k * 10 * dt, 10 * dt) == 10
        edges, counts = p.rtd()
        absorbed = p.recycle_counts()["absorbed"]
        assert int(counts.sum()) == absorbed > 0 and edges[1] == 2 * dt
        s, c, ns = p.ctx.age_field()
        occ, ns_occ = p.ctx.occupancy()
        assert ns == ns_occ == 7 and np.array_equal(c, occ)
        conc, m = p.concentration(), p.mean_age()
        assert np.isfinite(m[conc > 0]).all() and np.isnan(m[conc == 0]).all() and (m[conc > 0] >= 0).all()
        assert m[conc > 0].max() <= 30 * dt and m[conc > 0].max() > 0
        # tracking changes nothing of the run
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        with pytest.raises(L.CpfError):
            q.rtd()
    finally:
        p.close(); q.close()
