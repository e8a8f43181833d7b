"""GPU: zones (include/cpf.h "zones"; csrc/cpf_zones.hip).  Every comparison is equality of integers: the table and the last zones
against the numpy statement of tests/zones.py over what ``get_particles()`` returns, whole recycled runs against the statement at
every recycle point, and the cloud, the counters and every other table against a twin context with zones off."""
import numpy as np
import pytest

import recycle as R
import sourcepatch as SP
import warped as W
import zones as Z
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N_T = 2 * 4096 + 37                          # two full slices and a ragged one
SEED = R.SEED
MODES = ["sorted", "permuted", "index"]      # fresh from a sort (gid permuted, cells in runs); gid permuted and the cells scattered
#                                              again; gid = index, cells scattered
OUT = Z.OUTSIDE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


def _located(ctx, mesh, xyz, mode, cell=None):
    """a located cloud at rest, in one of MODES"""
    ctx.set_mesh(mesh); ctx.set_velocity(np.zeros((mesh.n_cells, 3))); ctx.set_seed(SEED)
    ctx.set_particles(xyz, cell)
    if cell is None:
        assert ctx.locate_initial() == 0
    if mode in ("sorted", "permuted"):
        ctx.sort_by_cell()
    if mode == "permuted":                                                   # three cycles in a random field scatter the cells again
        U = np.random.default_rng(17).normal(size=(mesh.n_cells, 3))
        ctx.set_velocity(U); ctx.step(0.3, 0.0, 3); ctx.set_velocity(np.zeros((mesh.n_cells, 3)))


def _refused(status, call):
    with pytest.raises(L.CpfError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert str(e.value)                                                      # ... with a message


def _lasts(n, n_zones, seed):
    """last zones that no sample of this file produces: random zones, a third of them outside"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.33, OUT, rng.integers(0, n_zones, size=n)).astype(np.uint8)


def _same(ctx, flow, last, n_samples=None):
    got, ns = ctx.zone_flows()
    assert got.dtype == np.uint64 and got.shape == flow.shape
    assert np.array_equal(got, flow), (np.argwhere(got != flow)[:8], got[got != flow][:8], flow[got != flow][:8])
    bad = np.nonzero(ctx.zone_last() != last)[0]
    assert bad.size == 0, (bad.size, bad[:5], ctx.zone_last()[bad[:5]], last[bad[:5]])
    assert n_samples is None or ns == n_samples


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)),
                zone_of=np.random.default_rng(2).integers(0, 5, size=60).astype(np.int32),
                U=np.random.default_rng(18).normal(size=(60, 3)))


# ------------------------------------------------------------------------------------------------ 1. lifecycle
def test_1_lifecycle(box):
    mesh, xyz = box["mesh"], box["xyz"]
    with api.Context(0) as ctx:
        needs_on = (lambda: ctx.set_zone_map(np.zeros(60, np.int32)), ctx.zone_sample, ctx.zone_reset, ctx.zone_flows, ctx.zone_last,
                    lambda: ctx.zone_set_last(np.zeros(N_T, np.uint8)), lambda: ctx.zone_exchange_rates(1.0),
                    lambda: ctx.zone_residence(1.0))

        def off():
            for g in needs_on:
                _refused(L.CPF_ERR_STATE, g)

        _refused(L.CPF_ERR_STATE, lambda: ctx.zone_enable(4))                # no mesh
        ctx.set_mesh(mesh)
        _refused(L.CPF_ERR_STATE, lambda: ctx.zone_enable(4))                # no cloud
        ctx.zone_disable()                                                   # off already: no error
        ctx.set_particles(xyz)
        _refused(L.CPF_ERR_STATE, lambda: ctx.zone_enable(4))                # ... set, but not located
        off()
        ctx.locate_initial()
        for n_zones in (0, 64, -1, 255):
            _refused(L.CPF_ERR_ARG, lambda: ctx.zone_enable(n_zones))
        off()                                                                # a refused enable leaves it off
        ctx.zone_enable(63)
        f, ns = ctx.zone_flows()
        assert f.dtype == np.uint64 and f.shape == (64, 64) and not f.any() and ns == 0
        assert (ctx.zone_last() == OUT).all()
        ctx.zone_enable(4)
        # the map: one value per cell of the mesh, in [0, nZones); a refused map leaves the old one
        good = (np.arange(60) % 4).astype(np.int32)
        ctx.set_zone_map(good)
        bad4, badneg = good.copy(), good.copy()
        bad4[59] = 4; badneg[0] = -1
        for bad in (np.zeros(59, np.int32), np.zeros(61, np.int32), bad4, badneg):
            _refused(L.CPF_ERR_ARG, lambda: ctx.set_zone_map(bad))
        cell = ctx.get_particles()[1]
        ctx.zone_sample()
        flow, last = Z.sample(Z.table(4), np.full(N_T, OUT, np.uint8), cell, good, 4)
        _same(ctx, flow, last, 1)
        assert np.unique(last).size == 4
        # the raw table of last zones: round trip, and a byte that is neither a zone nor 0xFF is refused
        pattern = _lasts(N_T, 4, 5)
        ctx.zone_set_last(pattern)
        assert np.array_equal(ctx.zone_last(), pattern)
        for byte in (4, 0xFE, 63):
            bad = pattern.copy(); bad[N_T // 2] = byte
            _refused(L.CPF_ERR_ARG, lambda: ctx.zone_set_last(bad))
        assert np.array_equal(ctx.zone_last(), pattern)
        with pytest.raises(ValueError):
            ctx.zone_set_last(np.zeros(3, np.uint8))
        assert ctx.lib.cpf_zone_get_last(ctx.h, None) == L.CPF_ERR_ARG and ctx.lib.cpf_zone_set_last(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_zone_flows(ctx.h, None, None) == L.CPF_OK     # each argument nullable
        # reset: the table and the count; last and the map stay
        ctx.zone_reset()
        _same(ctx, Z.table(4), pattern, 0)
        ctx.zone_sample()
        flow, last = Z.sample(Z.table(4), pattern, cell, good, 4)
        _same(ctx, flow, last, 1)
        # enable again starts anew and zeroes the map as well
        ctx.zone_enable(4)
        _same(ctx, Z.table(4), np.full(N_T, OUT, np.uint8), 0)
        ctx.zone_sample()
        want = Z.table(4); want[4, 0] = N_T
        _same(ctx, want, np.zeros(N_T, np.uint8), 1)
        # everything that replaces the cloud or the mesh turns it off; age, tags, routes and exposure do not
        for turn_off in (lambda: ctx.set_particles(xyz), lambda: ctx.set_mesh(mesh),
                         lambda: ctx.seed_box(N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0))):
            ctx.set_particles(xyz); ctx.locate_initial()
            ctx.zone_enable(4); ctx.zone_sample()
            turn_off()
            off()
        ctx.set_particles(xyz); ctx.locate_initial()
        ctx.zone_enable(4); ctx.zone_sample()
        assert ctx.lib.cpf_alloc_particles(ctx.h, 2 * N_T) == L.CPF_OK       # (a new allocation: no cloud until it is set)
        assert ctx.lib.cpf_zone_sample(ctx.h) == L.CPF_ERR_STATE and ctx.lib.cpf_zone_reset(ctx.h) == L.CPF_ERR_STATE
        assert ctx.lib.cpf_get_zone_flows(ctx.h, None, None) == L.CPF_ERR_STATE
        ctx.set_particles(xyz); ctx.locate_initial()
        off()
        ctx.zone_enable(4); ctx.set_zone_map(good); ctx.zone_sample()
        ctx.age_enable(2, 4); ctx.tag_enable(3, 2); ctx.route_enable(); ctx.exposure_enable(0.5, 4)
        ctx.route_disable(); ctx.exposure_disable(); ctx.tag_disable(); ctx.age_disable()
        flow, last = Z.sample(Z.table(4), np.full(N_T, OUT, np.uint8), cell, good, 4)
        _same(ctx, flow, last, 1)
        ctx.age_enable(2, 4); ctx.exposure_enable(0.5, 4)
        ctx.zone_disable()
        off()
        assert ctx.age_histogram().shape == (4,) and ctx.dose_histogram().shape == (1, 1, 4)   # ... nor they by zones
        # with zones off again the sink and the respawn are the ones of before
        ctx.set_sink_cells(box["sink"]); ctx.sink_apply()
        ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))
        k = ctx.recycle_counts()
        assert k["absorbed"] == k["drawn"] == k["placed"] > 0


# ------------------------------------------------------------------------------------------------ 2. sample against the statement
@pytest.mark.parametrize("n", [N_T, 4096, 4095, 1])
@pytest.mark.parametrize("mode", MODES)
def test_2_three_samples_count_exactly_what_numpy_counts(box, gpu_ctx_factory, mode, n):
    """three samples with a cycle in a random field between them; dead slots (CPF_CELL_LOST, and CPF_CELL_FROZEN where the cells can
    be given) are skipped"""
    mesh, xyz, zone_of = box["mesh"], box["xyz"][:n], box["zone_of"]
    ctx = gpu_ctx_factory()
    if mode == "index":                                                      # the cells as given: every ninth lost, every tenth frozen
        _located(ctx, mesh, xyz, mode)
        cell = ctx.get_particles()[1].copy()
        cell[4::9] = -1; cell[5::10] = -2
        _located(ctx, mesh, xyz, mode, cell if n > 1 else None)
    else:
        _located(ctx, mesh, xyz, mode)
        ctx.set_sink_cells(np.arange(0, 60, 7).astype(np.int32)); ctx.sink_apply()          # the absorbed are dead slots
        ctx.set_sink_cells([])
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    flow, last = Z.table(5), np.full(n, OUT, np.uint8)
    for k in range(3):
        if k:
            ctx.set_velocity(box["U"]); ctx.step(0.3, 0.0, 1)
        cell = ctx.get_particles()[1]
        assert n < 100 or ((cell < 0).sum() > n // 20 and (cell >= 0).sum() > n // 2)
        ctx.zone_sample()
        flow, after = Z.sample(flow, last, cell, zone_of, 5)
        _same(ctx, flow, after, k + 1)
        assert n < 100 or k == 0 or (after != last).sum() > n // 20          # (somebody moved to another zone)
        last = after
    # (every zone was stayed in, and more than a third of the twenty moves between two zones were made)
    assert n < 100 or ((np.diagonal(flow)[:5] > 0).all() and (flow[:5, :5] > 0).sum() > 5 + 7 and (last[cell < 0] == OUT).any())
    assert int(flow.sum()) <= 3 * n and np.array_equal(ctx.get_particles()[1], cell)         # nothing of the cloud is written


def test_2_a_slice_without_a_live_slot_next_to_a_live_one(box, gpu_ctx_factory):
    mesh, zone_of = box["mesh"], box["zone_of"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], "index")
    cell = ctx.get_particles()[1].copy()
    cell[:4096] = -1                                                         # the first slice: nobody live
    cell[4096:4096 + 2048] = np.where(np.arange(2048) % 2 == 0, -2, cell[4096:4096 + 2048])
    _located(ctx, mesh, box["xyz"], "index", cell)
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    pattern = _lasts(N_T, 5, 9)
    ctx.zone_set_last(pattern)
    ctx.zone_sample()
    flow, last = Z.sample(Z.table(5), pattern, cell, zone_of, 5)
    _same(ctx, flow, last, 1)
    assert np.array_equal(last[:4096], pattern[:4096]) and (last[4096:] != pattern[4096:]).sum() > 1000
    assert int(flow.sum()) == int((cell >= 0).sum())


@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_2_every_particle_in_one_cell_is_one_key_a_slice(box, gpu_ctx_factory, mode):
    mesh, zone_of = box["mesh"], box["zone_of"]
    xyz = pz.uniform_points(5, N_T, (2.0, 1.0, 1.0), (3.0, 2.0, 2.0))        # all in one cell
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, mode)
    cell = ctx.get_particles()[1]
    assert (cell == cell[0]).all()
    z = int(zone_of[cell[0]])
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    ctx.zone_sample()
    want = Z.table(5); want[5, z] = N_T
    _same(ctx, want, np.full(N_T, z, np.uint8), 1)
    ctx.zone_sample()
    want[z, z] = N_T
    _same(ctx, want, np.full(N_T, z, np.uint8), 2)


@pytest.mark.parametrize("n_zones", [1, 63])
@pytest.mark.parametrize("pattern", ["a key a lane", "every word"])
def test_2_one_zone_and_sixty_three(gpu_ctx_factory, n_zones, pattern):
    """gid = index and the cells as given, so that slot s holds a chosen (last, zone) pair.  "a key a lane": the 64 lanes of a wave
    hold slots 4 apart, and slot s has last = (s / 4) mod 64 (63: outside): with 63 zones no two lanes of a wave share a key, the
    path count_runs leaves to every lane for itself.  "every word": pair number s mod (64 x 63) -- every word of the table a
    sample can add to is hit, twice."""
    mesh = box_mesh(8, 4, 2)                                                 # 64 cells, cell c in zone c mod n_zones
    zone_of = (np.arange(64) % n_zones).astype(np.int32)
    s = np.arange(N_T)
    if pattern == "a key a lane":
        p, cell = (s // 4) % 64, ((s // 4) % 63).astype(np.int32)
    else:
        q = s % (64 * 63)
        p, cell = q // 63, (q % 63).astype(np.int32)
    cell[N_T - 5] = -1; cell[N_T - 9] = -2
    last0 = np.where((p >= n_zones) | (p == 63), OUT, p).astype(np.uint8)
    xyz = pz.uniform_points(5, N_T, (0.0, 0.0, 0.0), (8.0, 4.0, 2.0))        # (at rest: the positions are never read)
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, "index", cell)
    ctx.zone_enable(n_zones); ctx.set_zone_map(zone_of)
    ctx.zone_set_last(last0)
    ctx.zone_sample()
    flow, last = Z.sample(Z.table(n_zones), last0, cell, zone_of, n_zones)
    _same(ctx, flow, last, 1)
    if n_zones == 63 and pattern == "every word":
        assert (flow[:, :63] >= 2).all() and not flow[:, 63].any()           # all 64 x 63 sample words
    if n_zones == 63 and pattern == "a key a lane":
        key = (np.where(last0 == OUT, 63, last0).astype(np.int64) * 64 + zone_of[np.maximum(cell, 0)])[:8192].reshape(2, 4, 4, 64, 4)
        lanes = np.moveaxis(key, 3, -1).reshape(-1, 64)                      # [slice, round, wave, element][lane]
        assert all(np.unique(row).size == 64 for row in lanes)
    ctx.zone_sample()                                                        # at rest: the diagonal
    flow, last = Z.sample(flow, last, cell, zone_of, n_zones)
    _same(ctx, flow, last, 2)


def test_2_on_a_warped_mesh_every_derived_cell_of_a_parent_has_its_zone(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    n = N_T
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(n, 3))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    n_derived = int(ctx.mesh_quality()["n_derived"])
    assert n_derived > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.zone_enable(7)
    _refused(L.CPF_ERR_ARG, lambda: ctx.set_zone_map(np.zeros(n_derived, np.int32)))         # per cell AS GIVEN
    zone_of = ((np.arange(120) * 5) % 7).astype(np.int32)                    # neighbours in different zones
    ctx.set_zone_map(zone_of)
    flow, last = Z.table(7), np.full(n, OUT, np.uint8)
    for k in range(3):
        ctx.step(0.05, 0.0, 2)
        if k == 1:
            ctx.sort_by_cell()
        ctx.zone_sample()
        cell = ctx.get_particles()[1]                                        # parent ids
        assert cell.max() < 120
        flow, last = Z.sample(flow, last, cell, zone_of, 7)
        _same(ctx, flow, last, k + 1)
    assert (flow[:7, :7] > 0).sum() > 30


# ------------------------------------------------------------------------------------------------ 3. no needless stores
@pytest.mark.parametrize("mode", MODES)
def test_3_a_cloud_that_did_not_move_adds_to_the_diagonal_only(box, gpu_ctx_factory, mode):
    mesh, zone_of = box["mesh"], box["zone_of"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], mode)
    cell = ctx.get_particles()[1]
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    ctx.zone_sample()
    f1, last = ctx.zone_flows()[0], ctx.zone_last()
    assert np.array_equal(last, zone_of[cell].astype(np.uint8)) and not f1[:5, :].any()
    ctx.zone_sample()
    f2 = ctx.zone_flows()[0]
    assert np.array_equal(ctx.zone_last(), last)                             # no byte of last changed
    d = (f2 - f1).astype(np.int64)
    assert np.array_equal(np.diagonal(d)[:5], np.bincount(zone_of[cell], minlength=5)) and d.sum() == np.trace(d) == N_T


# ------------------------------------------------------------------------------------------------ 4. leave
@pytest.mark.parametrize("n", [N_T, 1, 4095])
@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_4_the_outside_column_counts_exactly_the_absorbed(box, gpu_ctx_factory, mode, n):
    mesh, sink, zone_of = box["mesh"], box["sink"], box["zone_of"]
    xyz = box["xyz"][:n].copy()
    xyz[0] = (4.5, 0.5, 0.5)                                                 # (somebody is absorbed)
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, mode)
    ctx.set_sink_cells(sink)
    cell0 = ctx.get_particles()[1]
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    last = _lasts(n, 5, 21)
    ctx.zone_set_last(last)
    before = ctx.recycle_counts()["absorbed"]
    ctx.sink_apply()
    flow = Z.leave(Z.table(5), last, cell0, sink, 5)
    _same(ctx, flow, last, 0)                                                # last is not written
    absorbed = ctx.recycle_counts()["absorbed"] - before
    assert int(flow[:, 5].sum()) == absorbed == int(np.isin(cell0, sink).sum()) >= 1 and not flow[:, :5].any()
    assert n < 100 or (flow[:, 5] > 0).all()                                 # from every zone and from outside
    assert np.array_equal(ctx.get_particles()[1], R.sink(cell0, sink))
    ctx.sink_apply()                                                         # a second apply finds nobody
    _same(ctx, flow, last, 0)


@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_4_every_particle_of_two_slices_and_a_tail_is_absorbed(box, gpu_ctx_factory, mode):
    mesh, sink, zone_of = box["mesh"], box["sink"], box["zone_of"]
    xyz = pz.uniform_points(5, N_T, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))        # all in the last x layer
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, mode)
    ctx.set_sink_cells(sink)
    cell0 = ctx.get_particles()[1]
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    last = _lasts(N_T, 5, 22)
    ctx.zone_set_last(last)
    ctx.sink_apply()
    flow = Z.leave(Z.table(5), last, cell0, sink, 5)
    _same(ctx, flow, last, 0)
    assert int(flow[:, 5].sum()) == N_T == ctx.recycle_counts()["absorbed"] and (ctx.get_particles()[1] == -1).all()


def test_4_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(41, 40, 40)                                              # 65 600 cells: more bits than the 2048 staged words hold
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    n = 36_000
    xyz = pz.uniform_points(79, n, (0.0, 0.0, 0.0), (41.0, 40.0, 40.0))
    zone_of = Z.x_slabs(mesh, 8)
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, "sorted")
    ctx.set_sink_cells(sink)
    cell0 = ctx.get_particles()[1]
    ctx.zone_enable(8); ctx.set_zone_map(zone_of)
    ctx.zone_sample()                                                        # ... and the map over 65 600 cells: one gather a particle
    flow, last = Z.sample(Z.table(8), np.full(n, OUT, np.uint8), cell0, zone_of, 8)
    ctx.sink_apply()
    flow = Z.leave(flow, last, cell0, sink, 8)
    _same(ctx, flow, last, 1)
    hit = int(np.isin(cell0, sink).sum())
    assert hit > 500 and int(flow[:, 8].sum()) == int(flow[7, 8]) == hit == ctx.recycle_counts()["absorbed"]


# ------------------------------------------------------------------------------------------------ 5. the twin, on each absorb path
@pytest.mark.parametrize("path", ["plain", "age and tags", "routes", "exposure"])
@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_5_the_sink_does_what_it_does_without_zones(box, gpu_ctx_factory, mode, path):
    mesh, sink, xyz, zone_of = box["mesh"], box["sink"], box["xyz"], box["zone_of"]
    groups = np.arange(sink.size) % 2
    origin = np.random.default_rng(12).integers(0, 3, size=N_T).astype(np.uint8)
    births = np.random.default_rng(13).integers(0, 6, size=N_T).astype(np.uint32)
    dose = np.random.default_rng(14).uniform(0.0, 2.0, size=N_T)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, xyz, mode)
        c.step(0.1, 0.0, 5)                                                  # (at rest: the cycle counter is 5)
        c.set_sink_cells(sink)
        if path in ("age and tags", "routes"):
            c.age_enable(2, 4); c.age_set_births(births)
            c.tag_enable(3, 2); c.set_sink_groups(sink, groups); c.tag_set_origins(origin)
        if path == "routes":
            c.route_enable()
        if path == "exposure":
            c.exposure_enable(0.1, 16); c.exposure_set_doses(dose)
    cell0 = ctx.get_particles()[1]
    ctx.zone_enable(5); ctx.set_zone_map(zone_of)
    last = _lasts(N_T, 5, 23)
    ctx.zone_set_last(last)
    for k in range(2):                                                       # the second apply finds nobody
        ctx.sink_apply(); twin.sink_apply()
        a, b = ctx.get_particles(), twin.get_particles()
        assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        assert ctx.recycle_counts() == twin.recycle_counts()
        if path in ("age and tags", "routes"):
            assert np.array_equal(ctx.transfer(), twin.transfer()) and np.array_equal(ctx.age_histogram(), twin.age_histogram())
            assert np.array_equal(ctx.age_births(), twin.age_births()) and np.array_equal(ctx.tag_origins(), twin.tag_origins())
            assert ctx.transfer().sum() == ctx.recycle_counts()["absorbed"]
        if path == "routes":
            assert np.array_equal(ctx.route_histogram(), twin.route_histogram()) and ctx.route_histogram().any()
        if path == "exposure":
            assert np.array_equal(ctx.dose_histogram(), twin.dose_histogram()) and ctx.dose_histogram().any()
            assert np.array_equal(_bits(ctx.exposure_doses()), _bits(twin.exposure_doses()))
    flow = Z.leave(Z.table(5), last, cell0, sink, 5)
    _same(ctx, flow, last, 0)
    assert int(flow[:, 5].sum()) == ctx.recycle_counts()["absorbed"] > 1000


# ------------------------------------------------------------------------------------------------ 6. the stamp
@pytest.mark.parametrize("source", [False, True])
def test_6_a_limited_respawn_puts_every_candidate_outside(box, gpu_ctx_factory, source):
    mesh, sink = box["mesh"], box["sink"]
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, box["xyz"], "index")
        c.set_sink_cells(sink)
        if source:
            tri, _ = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
            c.set_source_triangles(tri, None, (0.0, 0.5))
    ctx.zone_enable(5); ctx.set_zone_map(box["zone_of"])
    pattern = np.random.default_rng(11).integers(0, 5, size=N_T).astype(np.uint8)            # nobody outside
    ctx.zone_set_last(pattern)
    cell0 = ctx.get_particles()[1]
    respawn = (lambda c, k: c.respawn_source(k)) if source else (lambda c, k: c.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0), k))
    # nobody is dead: the stamp finds no candidate
    respawn(ctx, -1); respawn(twin, -1)
    assert np.array_equal(ctx.zone_last(), pattern)
    ctx.sink_apply(); twin.sink_apply()
    dead = np.nonzero(np.isin(cell0, sink))[0]
    assert dead.size > 1000
    assert np.array_equal(ctx.zone_last(), pattern)                          # the leave writes no byte
    respawn(ctx, 0); respawn(twin, 0)                                        # maxCount 0: no stamp, as for age
    assert np.array_equal(ctx.zone_last(), pattern)
    if not source:                                                           # a box the respawn refuses: no stamp either
        _refused(L.CPF_ERR_ARG, lambda: ctx.respawn_box((1.0, 0.0, 0.0), (0.0, 4.0, 3.0), -1))
        assert np.array_equal(ctx.zone_last(), pattern)
    half = dead.size // 2
    respawn(ctx, half); respawn(twin, half)                                  # gid = index: the first half of the dead in id order
    cell = ctx.get_particles()[1]
    assert (cell[dead[:half]] >= 0).all() and (cell[dead[half:]] < 0).all()
    want = pattern.copy(); want[dead] = OUT                                  # the placed and the left-dead alike; no live one
    assert np.array_equal(ctx.zone_last(), want) and np.array_equal(want, Z.stamp(pattern, R.sink(cell0, sink)))
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0])) and ctx.recycle_counts() == twin.recycle_counts()
    flow = Z.leave(Z.table(5), pattern, cell0, sink, 5)
    _same(ctx, flow, want, 0)


# ------------------------------------------------------------------------------------------------ 7. whole recycled runs
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_7_a_recycled_run_keeps_its_books(name, interval, gpu_ctx_factory):
    """tests/test_gpu_recycle.py's whole runs (D = 0; "graded box" re-sorts every round, "thin box" is the flat walk), a cycle a
    launch, with zones on and off: the same bits either way; the table and the last zones are the statement's (tests/zones.py) at
    every recycle point; the zone columns add up to the occupancy sampled at the same points, and what entered a zone less what
    left it is who is in it."""
    r = R.run(name)
    n, n_zones = r.xyz.shape[0], 4
    zone_of = Z.x_slabs(r.mesh, n_zones)
    assert np.unique(zone_of).size == n_zones
    out = {}
    for zoned in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", r.sort_interval)
        ctx.set_mesh(r.mesh); ctx.set_velocity(r.U); ctx.set_seed(SEED)
        ctx.synchronize()
        ctx.set_particles(r.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(r.sink_cells)
        if zoned:
            ctx.zone_enable(n_zones); ctx.set_zone_map(zone_of)
        flow, last, samples = Z.table(n_zones), np.full(n, OUT, np.uint8), 0
        for k in range(r.rounds):
            for j in range(r.cycles):
                ctx.step(r.dt, 0.0, 1)
                if zoned and (j + 1) % interval == 0:
                    cell = ctx.get_particles()[1]
                    ctx.zone_sample(); ctx.occupancy_sample()
                    flow, last = Z.sample(flow, last, cell, zone_of, n_zones)
                    samples += 1
            if zoned:
                cell = ctx.get_particles()[1]
                flow = Z.leave(flow, last, cell, r.sink_cells, n_zones)
                last = Z.stamp(last, R.sink(cell, r.sink_cells))
            ctx.sink_apply()
            ctx.respawn_box(r.box[0], r.box[1])
            if zoned:
                _same(ctx, flow, last, samples)
                lost = ctx.counters()["lost"]
                print("MEASURED %s interval %d round %d: lost %d, samples %d" % (name, interval, k, lost, samples))
                assert lost == 0, (name, k, lost)                            # the sink is the only way to die: else no balance
                got = ctx.zone_flows()[0].astype(np.int64)
                counts, ns = ctx.occupancy()
                assert ns == samples
                per_zone = np.bincount(zone_of, weights=counts.astype(np.float64), minlength=n_zones).astype(np.int64)
                assert np.array_equal(got[:, :n_zones].sum(axis=0), per_zone), (name, k)
                inside = np.bincount(ctx.zone_last()[ctx.zone_last() != OUT], minlength=n_zones)
                assert np.array_equal(got[:, :n_zones].sum(axis=0) - got[:n_zones, :].sum(axis=1), inside), (name, k)
        out[zoned] = ctx.get_particles()
        if zoned:
            assert int(flow[:n_zones, n_zones].sum()) == ctx.recycle_counts()["absorbed"] >= 200
            # (the last slab is left out: it holds the sink's layer, and at a sample every 3 cycles nobody is found in it twice)
            assert (np.diagonal(flow)[:n_zones - 1] > 0).all() and flow[n_zones, 0] > 0 and flow[n_zones - 1, n_zones] > 0
    assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(_bits(out[True][0]), _bits(out[False][0]))


# ------------------------------------------------------------------------------------------------ 8. through CudaParticles
def test_8_cuda_particles_zone_map(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13
    lo, hi = pz.DOMAIN_BOX
    sink = mesh.patch_cells("outlet")
    zmap = Z.x_slabs(mesh, 4)
    box = (lo, (lo[0] + 0.1 * (hi[0] - lo[0]), hi[1], hi[2]))
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=4,
             occupancyInterval=4, sinkCells=sink, sourceBox=box, ageBins=8)
    p = api.CudaParticles(mesh, U, dict(d, zoneMap=zmap, zoneInterval=2))
    q = api.CudaParticles(mesh, U, d)
    # the same calls by hand, on a context of its own
    h = api.Context(0)
    try:
        for k in range(3):
            for run in (p, q):
                assert run.advect(k * 10 * dt, 10 * dt) == 10
        h.set_option("sort_interval", 25)
        h.set_mesh(mesh); h.set_velocity(U); h.set_sink_cells(sink)
        h.seed_box(20_000, pz.DOMAIN_BOX[0], pz.DOMAIN_BOX[1], 1)
        h.locate_initial(); h.sort_by_cell()
        h.age_enable(4, 8)
        h.zone_enable(4); h.set_zone_map(zmap)
        for step in range(2, 31, 2):                                         # a launch ends at every zone point; every other is a recycle point
            h.step(10 * dt / 10, 1.5e-5, 2, L.STEP_FUSE_CYCLES)
            h.zone_sample()
            if step % 4 == 0:
                h.sink_apply(); h.respawn_box(box[0], box[1], -1)
                h.occupancy_sample(); h.age_sample()
        flow, ns = p.zone_flows()
        want, want_ns = h.zone_flows()
        assert ns == want_ns == 15 and flow.shape == (5, 5)
        assert np.array_equal(flow, want)
        absorbed = p.recycle_counts()["absorbed"]
        assert int(flow[:, 4].sum()) == absorbed > 0 and int(flow[3, 4]) == absorbed      # the outlet lies in the last slab
        assert int(flow[:, :4].sum()) <= 15 * 20_000 and (np.diagonal(flow)[:4] > 0).all()
        res = p.zone_residence()
        assert res.shape == (4,) and (res[np.isfinite(res)] >= 2 * dt).all() and np.isfinite(res).any()
        # zones change nothing of the run, nor of what age reports
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        assert np.array_equal(a[1], h.get_particles()[1]) and np.array_equal(_bits(a[0]), _bits(h.get_particles()[0]))
        assert np.array_equal(p.rtd()[1], q.rtd()[1]) and np.array_equal(p.concentration(), q.concentration())
        with pytest.raises(L.CpfError):
            q.zone_flows()
        with pytest.raises(L.CpfError):                                      # a map of the wrong length: caught once the mesh is set
            api.CudaParticles(mesh, U, dict(d, zoneMap=zmap[:-1]))
    finally:
        p.close(); q.close(); h.close()
