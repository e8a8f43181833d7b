"""GPU: exposure (include/cpf.h "exposure"; csrc/cpf_exposure.hip).  Every comparison is exact equality of bits: the doses against
the numpy statement of tests/exposure.py over what ``get_particles()`` returns (one rounding per operation, one add per particle
and call), the dose histogram against ``np.add.at`` over the particles ``numpy.isin`` calls absorbed, whole recycled runs against
the CPU statement at every recycle point, and the cloud, the counters and every other table against a twin context with
exposure off."""
import numpy as np
import pytest

import exposure as E
import recycle as R
import sourcepatch as SP
import tags as T
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N_T = 2 * 4096 + 37                          # two full slices and a ragged one
N_H = 5 * 4096 + 37                          # the histogram's cloud: more hits than 4096 bins have edges and neighbours
SEED = R.SEED
MODES = ["sorted", "permuted", "index"]      # fresh from a sort (gid permuted, cells in runs); gid permuted and the cells scattered
#                                              again; gid = index, cells scattered


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want):
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (bad.size, bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


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


def _rate(n_cells, seed):
    r = np.random.default_rng(seed).uniform(0.0, 3.0, size=n_cells)
    r[::4] = 0.0                                                             # cells that add nothing
    return r


def _pattern(n, seed):
    """doses that no sum of this file produces: random bits of non-negative doubles, an inf among them"""
    d = np.random.default_rng(seed).integers(0, 0x7FF0000000000000, size=n, dtype=np.int64).view(np.float64).copy()
    d[::7] = 0.0
    d[n // 2] = np.inf
    return d


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)))


# ------------------------------------------------------------------------------------------------ 1. lifecycle
def test_1_lifecycle(box):
    mesh, xyz = box["mesh"], box["xyz"]
    with api.Context(0) as ctx:
        needs_on = (lambda: ctx.set_exposure_field(np.zeros(60)), lambda: ctx.exposure_accumulate(1.0), ctx.exposure_reset,
                    ctx.dose_histogram, ctx.doses, ctx.exposure_doses, lambda: ctx.exposure_set_doses(np.zeros(N_T)))

        def off():
            for g in needs_on:
                _refused(L.CPF_ERR_STATE, g)

        def fresh(tags=None):
            ctx.set_particles(xyz); ctx.locate_initial()
            if tags:
                ctx.tag_enable(*tags)

        _refused(L.CPF_ERR_STATE, lambda: ctx.exposure_enable(0.5, 4))       # no mesh
        ctx.set_mesh(mesh)
        _refused(L.CPF_ERR_STATE, lambda: ctx.exposure_enable(0.5, 4))       # no cloud
        ctx.exposure_disable()                                               # off already: no error
        ctx.set_particles(xyz)
        _refused(L.CPF_ERR_STATE, lambda: ctx.exposure_enable(0.5, 4))       # ... set, but not located
        off()
        ctx.locate_initial()
        for width, n_bins in ((0.0, 4), (-1.0, 4), (np.inf, 4), (np.nan, 4), (0.5, 0), (0.5, -1), (0.5, 4097)):
            _refused(L.CPF_ERR_ARG, lambda: ctx.exposure_enable(width, n_bins))
        off()                                                                # a refused enable leaves it off
        ctx.exposure_enable(0.5, 4096)                                       # 4096 words without tags
        h = ctx.dose_histogram()
        assert h.dtype == np.uint64 and h.shape == (1, 1, 4096) and not h.any()
        assert _bits(ctx.exposure_doses()).any() == 0 and _bits(ctx.doses()).any() == 0      # +0.0 everywhere
        # the field: one value per cell of the mesh, finite and >= 0
        for bad in (np.zeros(59), np.zeros(61), np.full(60, np.nan), np.full(60, -1e-300), np.full(60, np.inf)):
            _refused(L.CPF_ERR_ARG, lambda: ctx.set_exposure_field(bad))
        for bad in (-1.0, np.inf, np.nan):
            _refused(L.CPF_ERR_ARG, lambda: ctx.exposure_accumulate(bad))
        for bad in (np.full(N_T, -1.0), np.full(N_T, np.nan), np.full(N_T, -0.0)):
            _refused(L.CPF_ERR_ARG, lambda: ctx.exposure_set_doses(bad))
        with pytest.raises(ValueError):
            ctx.exposure_set_doses(np.zeros(3))
        assert ctx.lib.cpf_get_dose_histogram(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_doses(ctx.h, None) == L.CPF_ERR_ARG and ctx.lib.cpf_exposure_get_doses(ctx.h, None) == L.CPF_ERR_ARG
        # enable again starts anew and zeroes the rate as well
        ctx.set_exposure_field(np.ones(60)); ctx.exposure_accumulate(2.0)
        assert (ctx.doses() == 2.0).all()
        ctx.exposure_enable(0.25, 8)
        assert ctx.dose_histogram().shape == (1, 1, 8) and not ctx.doses().any()
        ctx.exposure_accumulate(2.0)
        assert not ctx.doses().any()
        # the table bound is on nOrigins * nSinks * nBins, the shape tagging's at enable time
        ctx.tag_enable(16, 16)
        off()                                                                # cpf_tag_enable turns it off
        ctx.exposure_enable(0.5, 16)
        assert ctx.dose_histogram().shape == (16, 16, 16)                    # exactly 4096 words
        _refused(L.CPF_ERR_ARG, lambda: ctx.exposure_enable(0.5, 17))        # 4352 words: refused, and what was on stays
        assert ctx.lib.cpf_exposure_reset(ctx.h) == L.CPF_OK
        ctx.tag_enable(1, 1)
        _refused(L.CPF_ERR_ARG, lambda: ctx.exposure_enable(0.5, 4097))      # 4097 words
        ctx.tag_enable(3, 2); ctx.exposure_enable(0.5, 16)
        assert ctx.dose_histogram().shape == (3, 2, 16)
        ctx.tag_disable()
        off()                                                                # ... and so does cpf_tag_disable
        ctx.exposure_enable(0.5, 16)
        assert ctx.dose_histogram().shape == (1, 1, 16)
        ctx.tag_disable()                                                    # (tagging off already: exposure goes all the same)
        off()
        # everything that replaces the cloud or the mesh turns it off; age and routes do not
        for turn_off in (lambda: ctx.set_particles(xyz), lambda: ctx.set_mesh(mesh), lambda: ctx.seed_box(N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)),
                         lambda: ctx.tag_enable(2, 2), ctx.tag_disable):
            fresh(tags=(3, 2))
            ctx.exposure_enable(0.5, 4); ctx.exposure_accumulate(1.0)
            turn_off()
            off()
        fresh(tags=(3, 2))
        ctx.exposure_enable(0.5, 4)
        ctx.age_enable(2, 4); ctx.route_enable(); ctx.route_disable(); ctx.age_enable(3, 5); ctx.age_disable()
        assert ctx.dose_histogram().shape == (3, 2, 4)
        ctx.exposure_disable()
        off()
        # with exposure off again the sink and the respawn are the ones of before
        ctx.set_sink_groups(box["sink"], np.zeros(box["sink"].size)); ctx.sink_apply()
        ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))
        k = ctx.recycle_counts()
        assert k["absorbed"] == k["drawn"] == k["placed"] == int(ctx.transfer().sum()) > 0


# ------------------------------------------------------------------------------------------------ 2. accumulate against numpy
@pytest.mark.parametrize("n", [N_T, 1, 4095])
@pytest.mark.parametrize("mode", MODES)
def test_2_three_calls_add_exactly_what_numpy_adds(box, gpu_ctx_factory, mode, n):
    """three calls with different scales, dead slots (CPF_CELL_LOST, and CPF_CELL_FROZEN where the cells can be given) skipped, cells
    whose rate is zero among the rest; then the raw table's round trip"""
    mesh, xyz = box["mesh"], box["xyz"][:n]
    ctx = gpu_ctx_factory()
    if mode == "index":                                                      # the cells as given: every ninth lost, every tenth frozen
        _located(ctx, mesh, xyz, mode)
        cell = ctx.get_particles()[1].copy()
        cell[4::9] = -1; cell[5::10] = -2
        _located(ctx, mesh, xyz, mode, cell if n > 1 else None)
    else:
        _located(ctx, mesh, xyz, mode)
        ctx.set_sink_cells(np.arange(0, 60, 7).astype(np.int32)); ctx.sink_apply()          # the absorbed are dead slots
    cell = ctx.get_particles()[1]
    assert n < 100 or ((cell < 0).sum() > n // 20 and (cell >= 0).sum() > n // 2)
    rate = _rate(60, 3)
    ctx.exposure_enable(0.5, 4)
    ctx.set_exposure_field(rate)
    want = np.zeros(n)
    for scale in (0.1, 0.3, 1e-4 / 3.0):
        ctx.exposure_accumulate(scale)
        want = E.accumulate(want, cell, rate, scale)
        _same_bits(ctx.exposure_doses(), want)
    assert n < 100 or (np.unique(want).size > 20 and (want[cell < 0] == 0.0).all())          # (at rest: a dose per cell)
    _same_bits(ctx.doses(), np.where(cell >= 0, want, -1.0))                 # -1 for the dead
    ctx.exposure_accumulate(0.0)                                             # a scale of zero adds +0.0: the same bits
    _same_bits(ctx.exposure_doses(), want)
    pattern = _pattern(n, 5)
    ctx.exposure_set_doses(pattern)
    _same_bits(ctx.exposure_doses(), pattern)
    ctx.exposure_accumulate(0.7)
    _same_bits(ctx.exposure_doses(), E.accumulate(pattern, cell, rate, 0.7))
    _same_bits(ctx.get_particles()[1], cell)                                 # nothing of the cloud is written


@pytest.mark.parametrize("mode", MODES)
def test_2_a_zero_field_touches_nothing_and_a_zone_field_its_zone(box, gpu_ctx_factory, mode):
    mesh = box["mesh"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], mode)
    cell = ctx.get_particles()[1]
    ctx.exposure_enable(0.5, 4)
    pattern = _pattern(N_T, 6)
    ctx.exposure_set_doses(pattern)
    ctx.exposure_accumulate(3.0)                                             # the default field: all zero
    _same_bits(ctx.exposure_doses(), pattern)
    ctx.set_exposure_field(np.zeros(60)); ctx.exposure_accumulate(3.0)
    _same_bits(ctx.exposure_doses(), pattern)
    zone = np.zeros(60); zone[37] = 1.0                                      # an indicator field: the time spent in cell 37
    ctx.set_exposure_field(zone)
    ctx.exposure_set_doses(np.zeros(N_T))
    ctx.exposure_accumulate(0.25); ctx.exposure_accumulate(0.25)
    got = ctx.exposure_doses()
    assert 50 < (cell == 37).sum() < 300
    _same_bits(got, np.where(cell == 37, 0.5, 0.0))
    ctx.exposure_set_doses(pattern); ctx.exposure_accumulate(0.125)
    _same_bits(ctx.exposure_doses(), E.accumulate(pattern, cell, zone, 0.125))


def test_2_a_slice_without_a_live_slot_next_to_a_live_one(box, gpu_ctx_factory):
    mesh = box["mesh"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], "index")
    cell = ctx.get_particles()[1].copy()
    cell[:4096] = -1                                                         # the first slice: nobody live
    cell[4096:4096 + 2048] = np.where(np.arange(2048) % 2 == 0, -2, cell[4096:4096 + 2048])
    _located(ctx, mesh, box["xyz"], "index", cell)
    rate = _rate(60, 8)
    ctx.exposure_enable(0.5, 4); ctx.set_exposure_field(rate)
    pattern = _pattern(N_T, 9)
    ctx.exposure_set_doses(pattern)
    ctx.exposure_accumulate(0.3)
    want = E.accumulate(pattern, cell, rate, 0.3)
    _same_bits(ctx.exposure_doses(), want)
    _same_bits(want[:4096], pattern[:4096])
    assert (_bits(want[4096:]) != _bits(pattern[4096:])).sum() > 1000


def test_2_on_a_warped_mesh_every_derived_cell_of_a_parent_has_its_rate(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    n = N_T
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(n, 3))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    assert ctx.mesh_quality()["n_derived"] > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.exposure_enable(0.5, 4)
    _refused(L.CPF_ERR_ARG, lambda: ctx.set_exposure_field(np.zeros(int(ctx.mesh_quality()["n_derived"]))))      # per cell AS GIVEN
    rate = 0.5 + np.arange(120, dtype=np.float64) / 7.0                      # no two cells alike
    ctx.set_exposure_field(rate)
    want = np.zeros(n)
    for k in range(3):
        ctx.step(0.05, 0.0, 2)
        if k == 1:
            ctx.sort_by_cell()
        ctx.exposure_accumulate(0.1)
        cell = ctx.get_particles()[1]                                        # parent ids
        assert cell.max() < 120
        want = E.accumulate(want, cell, rate, 0.1)
        _same_bits(ctx.exposure_doses(), want)
    assert np.unique(want).size > 200


# ------------------------------------------------------------------------------------------------ 3. the histogram
@pytest.fixture(scope="module")
def sinkbox():
    """5 x 4 x 4 unit cells, the last x layer (16 cells) the sink; most of the cloud lies in it, so that 16 x 16 routes all get
    hits and 4096 bins all their edges"""
    mesh = box_mesh(5, 4, 4)
    sink = _last_x_layer(mesh)
    assert sink.size == 16
    n_in = 13_100
    xyz = np.concatenate([pz.uniform_points(77, N_H - n_in, (0.0, 0.0, 0.0), (5.0, 4.0, 4.0)),
                          pz.uniform_points(78, n_in, (4.0, 0.0, 0.0), (5.0, 4.0, 4.0))])
    xyz = xyz[np.random.default_rng(1).permutation(N_H)]                     # unsorted: hits scattered over the array
    return dict(mesh=mesh, sink=sink, xyz=xyz)


def _edge_doses(bin_width, n_bins):
    """0, every bin edge b * bin_width, one ulp either side of each, and inf"""
    e = np.arange(n_bins + 1, dtype=np.float64) * np.float64(bin_width)
    return np.concatenate([[0.0], e, np.nextafter(e[1:], 0.0), np.nextafter(e, np.inf), [np.inf]])


def _doses_on_edges(cell0, sink, bin_width, n_bins, seed):
    """in id order: the absorbed get the edge doses in turn, everybody else a random dose"""
    n = cell0.size
    d = np.random.default_rng(seed).uniform(0.0, (n_bins + 1) * bin_width, size=n)
    hit = np.nonzero(np.isin(cell0, sink))[0]
    edges = _edge_doses(bin_width, n_bins)
    assert hit.size >= edges.size, (hit.size, edges.size)
    d[hit] = edges[np.arange(hit.size) % edges.size]
    return d


SHAPES = [(1, 1, 1, 0.1), (1, 1, 4096, 0.1), (3, 2, 16, 0.1), (16, 16, 16, 0.25), (1, 1, 4096, 3e-9)]


@pytest.mark.parametrize("n_origins,n_sinks,n_bins,bin_width", SHAPES)
@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_3_the_histogram_counts_exactly_the_absorbed(sinkbox, gpu_ctx_factory, mode, n_origins, n_sinks, n_bins, bin_width):
    """without tags where the shape is (1, 1, .), with tags otherwise; (16, 16, 16) is exactly 4096 words with every route hit;
    doses on every bin edge and one ulp either side of each; the twin runs the same sink without exposure"""
    mesh, sink = sinkbox["mesh"], sinkbox["sink"]
    tagged = (n_origins, n_sinks) != (1, 1)
    groups = (np.arange(sink.size) * 5 + 2) % n_sinks
    origin = np.random.default_rng(40 + n_origins).integers(0, n_origins, size=N_H).astype(np.uint8)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, sinkbox["xyz"], mode)
        c.set_sink_cells(sink)
        if tagged:
            c.tag_enable(n_origins, n_sinks); c.set_sink_groups(sink, groups); c.tag_set_origins(origin)
    cell0 = ctx.get_particles()[1]
    ctx.exposure_enable(bin_width, n_bins)
    dose = _doses_on_edges(cell0, sink, bin_width, n_bins, n_bins)
    ctx.exposure_set_doses(dose)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert 0.6 * N_H < hit.sum() < 0.8 * N_H
    group = T.group_of_cell(mesh.n_cells, sink, groups)
    want = E.histogram(cell0, sink, dose, bin_width, n_bins, origin if tagged else None, group if tagged else None, n_origins, n_sinks)
    got = ctx.dose_histogram()
    assert got.dtype == np.uint64 and got.shape == (n_origins, n_sinks, n_bins)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert int(got.sum()) == int(hit.sum()) == ctx.recycle_counts()["absorbed"]
    assert (want.sum(axis=2) > 0).all() and (want.sum(axis=(0, 1)) > 0).all()        # every route is hit, and every bin
    # the bins are cpf_exposure_bins_host's
    host = np.zeros(N_H, np.int32)
    assert ctx.lib.cpf_exposure_bins_host(api._ptr(dose), N_H, bin_width, n_bins, api._ptr(host)) == L.CPF_OK
    assert np.array_equal(host, E.bins(dose, bin_width, n_bins))
    if tagged:                                                               # the marginal over the bins is the transfer matrix
        assert np.array_equal(got.sum(axis=2), ctx.transfer())
        assert np.array_equal(ctx.transfer(), twin.transfer())
    # the cloud and the counters are the twin's; the doses are untouched
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], R.sink(cell0, sink)) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert ctx.recycle_counts() == twin.recycle_counts() == dict(absorbed=int(hit.sum()), drawn=0, placed=0, epochs=0)
    _same_bits(ctx.exposure_doses(), dose)
    _same_bits(ctx.doses(), np.where(hit, -1.0, dose))
    ctx.sink_apply()                                                         # a second apply finds nobody
    assert np.array_equal(ctx.dose_histogram(), want)
    edges, counts = ctx.dose_distribution()
    assert np.array_equal(counts, want) and edges.shape == (n_bins + 1,) and edges[0] == 0.0 and np.isinf(edges[-1])
    assert n_bins == 1 or edges[1] == bin_width
    ctx.exposure_reset()                                                     # zeroes the histogram only
    assert not ctx.dose_histogram().any()
    _same_bits(ctx.exposure_doses(), dose)


@pytest.mark.parametrize("n", [1, 4095])
def test_3_small_clouds(gpu_ctx_factory, n):
    mesh = box_mesh(5, 4, 3)
    sink = _last_x_layer(mesh)
    xyz = pz.uniform_points(5, n, (3.5, 0.0, 0.0), (5.0, 4.0, 3.0))
    xyz[0] = (4.5, 0.5, 0.5)                                                 # (somebody is absorbed)
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, "sorted")
    ctx.set_sink_cells(sink)
    cell0 = ctx.get_particles()[1]
    ctx.exposure_enable(0.1, 16)
    dose = np.random.default_rng(n).uniform(0.0, 1.8, size=n)
    ctx.exposure_set_doses(dose)
    ctx.sink_apply()
    want = E.histogram(cell0, sink, dose, 0.1, 16)
    assert np.array_equal(ctx.dose_histogram(), want) and int(want.sum()) == ctx.recycle_counts()["absorbed"] >= 1


@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_3_every_particle_of_two_slices_and_a_tail_is_absorbed(gpu_ctx_factory, mode):
    mesh = box_mesh(5, 4, 3)
    sink = _last_x_layer(mesh)
    xyz = pz.uniform_points(5, N_T, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))        # all in the last x layer
    groups = np.arange(sink.size) % 2
    origin = np.random.default_rng(8).integers(0, 3, size=N_T).astype(np.uint8)
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, mode)
    ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups); ctx.tag_set_origins(origin)
    cell0 = ctx.get_particles()[1]
    ctx.exposure_enable(0.1, 16)
    dose = _doses_on_edges(cell0, sink, 0.1, 16, 3)
    ctx.exposure_set_doses(dose)
    ctx.sink_apply()
    want = E.histogram(cell0, sink, dose, 0.1, 16, origin, T.group_of_cell(mesh.n_cells, sink, groups), 3, 2)
    assert np.array_equal(ctx.dose_histogram(), want) and int(want.sum()) == N_T
    assert ctx.recycle_counts()["absorbed"] == N_T and (ctx.get_particles()[1] == -1).all() and (ctx.doses() == -1.0).all()
    assert np.array_equal(want.sum(axis=2), ctx.transfer())


BIG_SINK = (41, 40, 40)                                                      # 65 600 cells: more bits than the 2048 staged words hold
N_BIG = 36_000


def test_3_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(*BIG_SINK)
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    groups = (sink // 3) % 2
    xyz = pz.uniform_points(79, N_BIG, (0.0, 0.0, 0.0), tuple(float(v) for v in BIG_SINK))
    origin = np.random.default_rng(9).integers(0, 3, size=N_BIG).astype(np.uint8)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, xyz, "sorted")
        c.tag_enable(3, 2); c.set_sink_groups(sink, groups); c.tag_set_origins(origin)
    cell0 = ctx.get_particles()[1]
    ctx.exposure_enable(0.1, 16)
    dose = _doses_on_edges(cell0, sink, 0.1, 16, 5)
    ctx.exposure_set_doses(dose)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert hit.sum() > 500
    want = E.histogram(cell0, sink, dose, 0.1, 16, origin, T.group_of_cell(mesh.n_cells, sink, groups), 3, 2)
    assert np.array_equal(ctx.dose_histogram(), want) and (want.sum(axis=2) > 0).all()
    assert ctx.recycle_counts()["absorbed"] == int(hit.sum()) == int(want.sum())
    assert np.array_equal(ctx.get_particles()[1], twin.get_particles()[1]) and np.array_equal(ctx.transfer(), twin.transfer())
    # ... and the field over 65 600 cells: one gather a particle
    rate = _rate(mesh.n_cells, 4)
    ctx.set_exposure_field(rate)
    cell = ctx.get_particles()[1]
    ctx.exposure_accumulate(0.3)
    _same_bits(ctx.exposure_doses(), E.accumulate(dose, cell, rate, 0.3))


# ------------------------------------------------------------------------------------------------ 4. the twin, on each absorb path
@pytest.mark.parametrize("path", ["plain", "age and tags", "routes"])
@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_4_the_sink_does_what_it_does_without_exposure(box, gpu_ctx_factory, mode, path):
    mesh, sink, xyz = box["mesh"], box["sink"], box["xyz"]
    groups = np.arange(sink.size) % 2
    origin = np.random.default_rng(12).integers(0, 3, size=N_T).astype(np.uint8)
    births = np.random.default_rng(13).integers(0, 6, size=N_T).astype(np.uint32)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, xyz, mode)
        c.step(0.1, 0.0, 5)                                                  # (at rest: the cycle counter is 5)
        c.set_sink_cells(sink)
        if path != "plain":
            c.age_enable(2, 4); c.age_set_births(births)
            c.tag_enable(3, 2); c.set_sink_groups(sink, groups); c.tag_set_origins(origin)
        if path == "routes":
            c.route_enable()
    cell0 = ctx.get_particles()[1]
    ctx.exposure_enable(0.1, 16)
    dose = _doses_on_edges(cell0, sink, 0.1, 16, 7)
    ctx.exposure_set_doses(dose)
    for k in range(2):                                                       # the second apply finds nobody
        ctx.sink_apply(); twin.sink_apply()
        a, b = ctx.get_particles(), twin.get_particles()
        assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        assert ctx.recycle_counts() == twin.recycle_counts()
        if path != "plain":
            assert np.array_equal(ctx.transfer(), twin.transfer()) and np.array_equal(ctx.age_histogram(), twin.age_histogram())
            assert np.array_equal(ctx.age_births(), twin.age_births()) and np.array_equal(ctx.tag_origins(), twin.tag_origins())
            assert ctx.transfer().sum() == ctx.recycle_counts()["absorbed"]
        if path == "routes":
            assert np.array_equal(ctx.route_histogram(), twin.route_histogram()) and ctx.route_histogram().any()
    tagged = path != "plain"
    want = E.histogram(cell0, sink, dose, 0.1, 16, origin if tagged else None,
                       T.group_of_cell(mesh.n_cells, sink, groups) if tagged else None, 3 if tagged else 1, 2 if tagged else 1)
    assert np.array_equal(ctx.dose_histogram(), want) and int(want.sum()) == ctx.recycle_counts()["absorbed"] > 1000


# ------------------------------------------------------------------------------------------------ 5. the stamp
@pytest.mark.parametrize("source", [False, True])
def test_5_a_limited_respawn_zeroes_every_candidate(box, gpu_ctx_factory, source):
    mesh, sink = box["mesh"], box["sink"]
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, box["xyz"], "index")
        c.set_sink_cells(sink)
        if source:
            tri, _ = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
            c.set_source_triangles(tri, None, (0.0, 0.5))
    ctx.exposure_enable(0.5, 4)
    pattern = np.where(_pattern(N_T, 11) == 0.0, 1.5, _pattern(N_T, 11))     # nobody at 0
    ctx.exposure_set_doses(pattern)
    cell0 = ctx.get_particles()[1]
    respawn = (lambda c, k: c.respawn_source(k)) if source else (lambda c, k: c.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0), k))
    # nobody is dead: the stamp finds no candidate
    respawn(ctx, -1); respawn(twin, -1)
    _same_bits(ctx.exposure_doses(), pattern)
    ctx.sink_apply(); twin.sink_apply()
    dead = np.nonzero(np.isin(cell0, sink))[0]
    assert dead.size > 1000
    respawn(ctx, 0); respawn(twin, 0)                                        # maxCount 0: no stamp, as for age
    _same_bits(ctx.exposure_doses(), pattern)
    if not source:                                                           # a box the respawn refuses: no stamp either
        _refused(L.CPF_ERR_ARG, lambda: ctx.respawn_box((1.0, 0.0, 0.0), (0.0, 4.0, 3.0), -1))
        _same_bits(ctx.exposure_doses(), pattern)
    half = dead.size // 2
    respawn(ctx, half); respawn(twin, half)                                  # gid = index: the first half of the dead in id order
    cell = ctx.get_particles()[1]
    assert (cell[dead[:half]] >= 0).all() and (cell[dead[half:]] < 0).all()
    want = pattern.copy(); want[dead] = 0.0                                  # the placed and the left-dead alike
    _same_bits(ctx.exposure_doses(), want)
    _same_bits(ctx.doses(), np.where(cell >= 0, want, -1.0))
    assert (ctx.doses() == -1.0).sum() == dead.size - half
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0])) and ctx.recycle_counts() == twin.recycle_counts()


# ------------------------------------------------------------------------------------------------ 6. whole recycled runs
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_6_a_recycled_run_carries_its_doses(name, interval, gpu_ctx_factory, oracle_libs):
    """tests/test_gpu_recycle.py's whole runs (D = 0; "graded box" re-sorts every round, "thin box" is the flat walk), a cycle a
    launch, with exposure on and off: the same bits either way, and the CPU statement's; doses and histogram are the statement's
    (tests/exposure.py) at every recycle point."""
    r, c = R.run(name), E.cpu(name, interval)
    rate = E.run_rate(r.mesh)
    out = {}
    for exposed in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", r.sort_interval)
        ctx.set_mesh(r.mesh); ctx.set_velocity(r.U); ctx.set_seed(SEED)
        ctx.synchronize()
        ctx.set_particles(r.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(r.sink_cells)
        if exposed:
            ctx.exposure_enable(E.BIN_WIDTH, E.N_BINS)
            ctx.set_exposure_field(rate)
        pending = 0.0
        for k in range(r.rounds):
            for j in range(r.cycles):
                ctx.step(r.dt, 0.0, 1)
                pending += r.dt * 1
                if (j + 1) % interval == 0:
                    if exposed:
                        ctx.exposure_accumulate(pending)
                    pending = 0.0
            ctx.sink_apply()
            ctx.respawn_box(r.box[0], r.box[1])
            if exposed:
                want = c["points"][k]
                _same_bits(ctx.exposure_doses(), want["dose"])
                assert np.array_equal(ctx.dose_histogram(), want["hist"]), (name, k)
                if k in (0, r.rounds - 1):
                    _same_bits(ctx.doses(), want["doses"])
        out[exposed] = ctx.get_particles()
        assert ctx.recycle_counts()["absorbed"] == c["absorbed"]
    for exposed in (True, False):
        xyzw, cell = out[exposed]
        bad = np.nonzero(cell != c["cell"])[0]
        assert bad.size == 0, (name, exposed, "cells differ", bad.size, bad[:5], cell[bad[:5]], c["cell"][bad[:5]])
        bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(c["xyz"])).any(1))[0]
        assert bad.size == 0, (name, exposed, "positions differ", bad.size, bad[:5])
    assert np.array_equal(_bits(out[True][0]), _bits(out[False][0]))
    hist = c["points"][-1]["hist"]
    assert int(hist.sum()) == c["absorbed"] >= 200 and (hist > 0).sum() >= 4


# ------------------------------------------------------------------------------------------------ 7. through CudaParticles
def test_7_cuda_particles_exposure_field(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13                                                          # 10 * dt / dt == 10 exactly
    lo, hi = pz.DOMAIN_BOX
    sink = mesh.patch_cells("outlet")
    field = np.zeros(mesh.n_cells); field[sink] = 1.0                        # the time spent in the outlet's cells ...
    field += 100.0 * (pitz["centres"][:, 0] < 0.0)                           # ... and a dense part upstream of the step
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=4,
             occupancyInterval=4, sinkCells=sink, sourceBox=(lo, (lo[0] + 0.1 * (hi[0] - lo[0]), hi[1], hi[2])), ageBins=8)
    p = api.CudaParticles(mesh, U, dict(d, exposureField=field, exposureInterval=2, doseBins=32, doseBinWidth=2 * dt))
    q = api.CudaParticles(mesh, U, d)
    try:
        for k in range(3):
            for run in (p, q):
                assert run.advect(k * 10 * dt, 10 * dt) == 10
        edges, counts = p.dose_distribution()
        absorbed = p.recycle_counts()["absorbed"]
        assert counts.shape == (1, 1, 32) and int(counts.sum()) == absorbed > 0 and edges[1] == 2 * dt and np.isinf(edges[-1])
        # everybody absorbed sat in an outlet cell at the exposure point just before: at least one interval of rate 1
        assert counts[0, 0, 0] == 0 and counts[0, 0, 1:].any()
        doses = p.doses()
        cell = p.particles()[1]
        assert np.array_equal(doses == -1.0, cell < 0) and (doses[cell >= 0] >= 0.0).all() and (doses > 0.0).any()
        assert doses.max() <= 100.0 * 30 * dt
        # exposure changes nothing of the run, nor of what age reports
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        assert np.array_equal(p.rtd()[1], q.rtd()[1]) and np.array_equal(p.concentration(), q.concentration())
        with pytest.raises(L.CpfError):
            q.dose_distribution()
        with pytest.raises(L.CpfError):                                      # a field of the wrong length: caught once the mesh is set
            api.CudaParticles(mesh, U, dict(d, exposureField=field[:-1]))
    finally:
        p.close(); q.close()
