"""GPU: routes (include/cpf.h "routes"; csrc/cpf_routes.hip).  Everything is integers and every comparison is exact: the joint
histogram and the age field per origin against the numpy statements of tests/routes.py over what ``get_particles()`` returns,
their marginals against the age and tag entries, whole recycled runs against the CPU statement, and the cloud, the counters, the
transfer matrix and the age histogram against a twin context with tags and age on and routes off."""
import numpy as np
import pytest

import age as A
import recycle as R
import routes as RT
import tags as T
import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = R.N                                      # 10 007: a multiple of neither 64, 256 nor 1024
N_T = 2 * 4096 + 37                          # two slices and a tail
SEED = R.SEED
NOW = 40                                     # the cycle counter of the absorb tests: 40 cycles at rest


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


def _edge_ages(n, bin_cycles, n_bins, seed):
    """ages on, just below and just above every bin edge (the open bin's lower edge and beyond included)"""
    e = np.arange(n_bins + 2, dtype=np.int64) * bin_cycles
    e = np.unique(np.concatenate([e, e[1:] - 1, e + 1, [0]]))
    a = e[np.random.default_rng(seed).integers(0, e.size, size=n)]
    a[:e.size] = e[:n]                                                       # (every edge at least once where the cloud is large enough)
    return np.random.default_rng(seed + 1).permutation(a)


def _births(now, ages):
    return ((np.int64(now) - np.asarray(ages, np.int64)) % (1 << 32)).astype(np.uint32)


def _pair(gpu_ctx_factory, mesh, xyz, sort, sink, groups, n_origins, n_sinks, bin_cycles, n_bins, origin, ages_of, cell=None, steps=NOW):
    """a context with routes and its twin with tags + age only, on the same cloud, births and origins set; returns
    (ctx, twin, cells before the sink, births)"""
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    births = None
    for c in (ctx, twin):
        _located(c, mesh, xyz, sort, cell)
        if steps:
            c.step(0.1, 0.0, steps)                                          # (at rest: the cycle counter is `steps`)
        c.age_enable(bin_cycles, n_bins)
        c.tag_enable(n_origins, n_sinks)
        c.set_sink_groups(sink, groups)
        c.tag_set_origins(origin)
        if births is None:
            cell0 = c.get_particles()[1]
            births = _births(steps, ages_of(cell0))
        c.age_set_births(births)
    ctx.route_enable()
    return ctx, twin, cell0, births


def _same_as_twin(ctx, twin):
    a, b = ctx.get_particles(), twin.get_particles()
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert ctx.recycle_counts() == twin.recycle_counts()
    assert np.array_equal(ctx.transfer(), twin.transfer()) and np.array_equal(ctx.age_histogram(), twin.age_histogram())
    assert np.array_equal(ctx.age_births(), twin.age_births()) and np.array_equal(ctx.tag_origins(), twin.tag_origins())


def _refused(status, call):
    with pytest.raises(L.CpfError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert str(e.value)                                                      # ... with a message


# ------------------------------------------------------------------------------------------------ 1. lifecycle
@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)))


def test_1_lifecycle(box):
    mesh, sink = box["mesh"], box["sink"]
    with api.Context(0) as ctx:
        needs_on = (ctx.route_sample, ctx.route_reset, ctx.route_histogram, ctx.route_field)

        def off():
            for g in needs_on:
                _refused(L.CPF_ERR_STATE, g)

        def fresh(age=True, tags=True):
            ctx.set_particles(box["xyz"]); ctx.locate_initial()
            if age:
                ctx.age_enable(2, 4)
            if tags:
                ctx.tag_enable(3, 2)

        _refused(L.CPF_ERR_STATE, ctx.route_enable)                          # no mesh, no cloud: neither is on
        ctx.set_mesh(mesh)
        ctx.route_disable()                                                  # off already: no error
        fresh(age=False, tags=False)
        _refused(L.CPF_ERR_STATE, ctx.route_enable)
        off()
        ctx.age_enable(2, 4)
        _refused(L.CPF_ERR_STATE, ctx.route_enable)                          # only age
        ctx.age_disable(); ctx.tag_enable(3, 2)
        _refused(L.CPF_ERR_STATE, ctx.route_enable)                          # only tags
        off()
        ctx.age_enable(2, 4)
        ctx.route_enable()
        h = ctx.route_histogram()
        s, c, ns = ctx.route_field()
        assert h.dtype == np.uint64 and h.shape == (3, 2, 4) and not h.any()
        assert s.shape == c.shape == (60, 3) and s.dtype == c.dtype == np.uint64 and not s.any() and not c.any() and ns == 0
        ctx.route_sample()
        assert ctx.route_field()[2] == 1
        ctx.route_enable()                                                   # again: anew
        assert ctx.route_field()[2] == 0 and not ctx.route_field()[1].any()
        assert ctx.lib.cpf_get_route_histogram(ctx.h, None) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_get_route_field(ctx.h, None, None, None) == L.CPF_OK                  # each output is nullable
        ctx.route_disable()
        off()
        # everything that turns age or tags off, or starts either anew, turns routes off
        for turn_off in (lambda: ctx.age_enable(3, 5), lambda: ctx.tag_enable(2, 2), ctx.age_disable, ctx.tag_disable,
                         lambda: ctx.set_particles(box["xyz"]), lambda: ctx.set_mesh(mesh),
                         lambda: ctx.seed_box(N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0))):
            fresh()
            ctx.route_enable(); ctx.route_sample()
            turn_off()
            off()
        # the tables take the sizes of the enables before them
        fresh()
        ctx.age_enable(3, 5); ctx.tag_enable(2, 1); ctx.route_enable()
        assert ctx.route_histogram().shape == (2, 1, 5) and ctx.route_field()[0].shape == (60, 2)
        # with routes off again the sink is the two-pass one, and counts as before
        ctx.route_disable()
        ctx.set_sink_groups(sink, np.zeros(sink.size)); ctx.sink_apply()
        assert int(ctx.transfer().sum()) == int(ctx.age_histogram().sum()) == ctx.recycle_counts()["absorbed"] > 0


# ------------------------------------------------------------------------------------------------ 2. absorb: exact results
@pytest.fixture(scope="module")
def sinkbox():
    """5 x 4 x 4 unit cells, the last x layer (16 cells) the sink; half the cloud lies in it, so that 16 x 16 routes all get hits"""
    mesh = box_mesh(5, 4, 4)
    sink = _last_x_layer(mesh)
    assert sink.size == 16
    xyz = np.concatenate([pz.uniform_points(77, N_T // 2, (0.0, 0.0, 0.0), (5.0, 4.0, 4.0)),
                          pz.uniform_points(78, N_T - N_T // 2, (4.0, 0.0, 0.0), (5.0, 4.0, 4.0))])
    xyz = xyz[np.random.default_rng(1).permutation(N_T)]                     # unsorted: hits scattered over the array
    return dict(mesh=mesh, sink=sink, xyz=xyz)


CASES = [(1, 1, 1, 1), (3, 2, 7, 16), (16, 16, 1, 16), (4, 4, 1, 257), (2, 2, 1000, 4096)]


@pytest.mark.parametrize("n_origins,n_sinks,bin_cycles,n_bins", CASES)
@pytest.mark.parametrize("sort", [True, False])
def test_2_the_joint_histogram_counts_exactly_the_absorbed(sinkbox, gpu_ctx_factory, sort, n_origins, n_sinks, bin_cycles, n_bins):
    """(16, 16, 1, 16): 4096 joint words, the staged limit; (4, 4, 1, 257): 4112, the global path; (2, 2, 1000, 4096): the global
    path with the largest nBins.  sort: gid permuted, hits in runs; without: gid = index, hits scattered"""
    mesh, sink = sinkbox["mesh"], sinkbox["sink"]
    words = n_origins * n_sinks * n_bins
    assert (words <= RT.JOINT_WORDS) == ((n_origins, n_sinks, n_bins) in [(1, 1, 1), (3, 2, 16), (16, 16, 16)])
    groups = (np.arange(sink.size) * 5 + 2) % n_sinks
    origin = _origins(N_T, n_origins, 40 + n_origins)
    ages = _edge_ages(N_T, bin_cycles, n_bins, n_bins)

    def ages_of(cell0):                                                      # in id order; one wrapped stamp, on somebody absorbed
        first = np.nonzero(np.isin(cell0, sink))[0][:2]
        ages[first[0]] = 2 ** 32 - 1                                         # birth = now + 1
        ages[first[1]] = 0                                                   # ... and somebody absorbed in the cycle of its birth
        return ages
    ctx, twin, cell0, births = _pair(gpu_ctx_factory, mesh, sinkbox["xyz"], sort, sink, groups, n_origins, n_sinks, bin_cycles, n_bins,
                                     origin, ages_of)
    assert (births > NOW).any() and np.array_equal(A.ages(NOW, births), ages)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert 0.5 * N_T < hit.sum() < 0.7 * N_T
    group = T.group_of_cell(mesh.n_cells, sink, groups)
    want = RT.hist(origin, group, cell0, hit, ages, bin_cycles, n_bins, n_origins, n_sinks)
    got = ctx.route_histogram()
    assert got.dtype == np.uint64 and got.shape == (n_origins, n_sinks, n_bins)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (want.sum(axis=2) > 0).all()                                      # every route is hit
    assert want[..., -1].any() and want[..., 0].any()                        # ... and the first and the open bin
    # its two marginals are the entries of tags and age
    assert np.array_equal(got.sum(axis=2), ctx.transfer()) and np.array_equal(got.sum(axis=(0, 1)), ctx.age_histogram())
    assert np.array_equal(ctx.transfer(), T.transfer(origin, group, cell0, hit, n_origins, n_sinks))
    assert np.array_equal(ctx.age_histogram(), A.rtd(ages[hit], bin_cycles, n_bins))
    assert int(got.sum()) == int(hit.sum()) == ctx.recycle_counts()["absorbed"]
    # the cloud, the counters, the matrix and the age histogram are the twin's, which ran the two passes
    _same_as_twin(ctx, twin)
    assert np.array_equal(ctx.get_particles()[1], R.sink(cell0, sink))
    assert ctx.recycle_counts() == dict(absorbed=int(hit.sum()), drawn=0, placed=0, epochs=0)
    edges, counts = ctx.rtd_by_route(0.5)
    assert np.array_equal(counts, want) and np.array_equal(edges, ctx.rtd(0.5)[0])
    ctx.sink_apply(); twin.sink_apply()                                      # a second apply finds nobody
    assert np.array_equal(ctx.route_histogram(), want)
    _same_as_twin(ctx, twin)


# ------------------------------------------------------------------------------------------------ 3. absorb: slices and masks
@pytest.mark.parametrize("sort", [True, False])
def test_3_every_particle_of_two_slices_and_a_tail_is_absorbed(gpu_ctx_factory, sort):
    mesh = box_mesh(5, 4, 3)
    sink = _last_x_layer(mesh)
    xyz = pz.uniform_points(5, N_T, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))        # all in the last x layer
    groups = np.arange(sink.size) % 2
    origin = _origins(N_T, 3, 8)
    ages = _edge_ages(N_T, 7, 16, 3)
    ctx, twin, cell0, _ = _pair(gpu_ctx_factory, mesh, xyz, sort, sink, groups, 3, 2, 7, 16, origin, lambda c: ages)
    ctx.sink_apply(); twin.sink_apply()
    want = RT.hist(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, np.ones(N_T, bool), ages, 7, 16, 3, 2)
    assert np.array_equal(ctx.route_histogram(), want) and int(want.sum()) == N_T
    assert ctx.recycle_counts()["absorbed"] == N_T and (ctx.get_particles()[1] == -1).all()
    _same_as_twin(ctx, twin)


def test_3_a_slice_without_a_hit_next_to_one_with_hits(gpu_ctx_factory):
    mesh = box_mesh(5, 4, 3)
    sink = _last_x_layer(mesh)
    xyz = np.concatenate([pz.uniform_points(6, 4096, (0.0, 0.0, 0.0), (4.0, 4.0, 3.0)),          # the first slice: nobody in the sink
                          pz.uniform_points(7, N_T - 4096, (3.0, 0.0, 0.0), (5.0, 4.0, 3.0))])
    groups = np.arange(sink.size) % 2
    origin = _origins(N_T, 3, 9)
    ages = _edge_ages(N_T, 7, 16, 4)
    ctx, twin, cell0, _ = _pair(gpu_ctx_factory, mesh, xyz, False, sink, groups, 3, 2, 7, 16, origin, lambda c: ages)
    hit = np.isin(cell0, sink)
    assert not hit[:4096].any() and 1000 < hit[4096:8192].sum() < 3000 and hit[8192:].any()
    ctx.sink_apply(); twin.sink_apply()
    want = RT.hist(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, hit, ages, 7, 16, 3, 2)
    assert np.array_equal(ctx.route_histogram(), want) and int(want.sum()) == int(hit.sum())
    _same_as_twin(ctx, twin)


BIG_SINK = (41, 40, 40)                                                      # 65 600 cells: more bits than the 2048 staged words hold
N_BIG = 36_000


def test_3_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(*BIG_SINK)
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    groups = (sink // 3) % 2
    xyz = pz.uniform_points(79, N_BIG, (0.0, 0.0, 0.0), tuple(float(v) for v in BIG_SINK))
    origin = _origins(N_BIG, 3, 9)
    ages = _edge_ages(N_BIG, 7, 16, 5)
    ctx, twin, cell0, _ = _pair(gpu_ctx_factory, mesh, xyz, True, sink, groups, 3, 2, 7, 16, origin, lambda c: ages)
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert hit.sum() > 500
    want = RT.hist(origin, T.group_of_cell(mesh.n_cells, sink, groups), cell0, hit, ages, 7, 16, 3, 2)
    assert np.array_equal(ctx.route_histogram(), want) and (want.sum(axis=2) > 0).all()
    assert ctx.recycle_counts()["absorbed"] == int(hit.sum()) == int(want.sum())
    _same_as_twin(ctx, twin)


def test_3_on_a_warped_mesh_the_derived_cells_of_a_parent_carry_its_group(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    sink = _last_x_layer(box_mesh(6, 5, 4))
    assert sink.size == 20
    groups = np.arange(sink.size) % 3
    rng = np.random.default_rng(3)
    n = 20_000
    xyz = rng.uniform((3.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(n, 3))
    origin = _origins(n, 2, 12)
    ages = _edge_ages(n, 7, 16, 6)
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        c.set_mesh(mesh); c.set_velocity(np.zeros((mesh.n_cells, 3))); c.set_particles(xyz)
        assert c.mesh_quality()["n_derived"] > mesh.n_cells == 120
        assert c.locate_initial() == 0
        c.sort_by_cell()
        c.age_enable(7, 16); c.tag_enable(2, 3); c.set_sink_groups(sink, groups); c.tag_set_origins(origin)
        c.age_set_births(_births(0, ages))
    ctx.route_enable()
    cell0 = ctx.get_particles()[1]                                           # parent ids
    ctx.sink_apply(); twin.sink_apply()
    hit = np.isin(cell0, sink)
    assert hit.sum() > 0.2 * n
    want = RT.hist(origin, T.group_of_cell(120, sink, groups), cell0, hit, ages, 7, 16, 2, 3)
    assert np.array_equal(ctx.route_histogram(), want) and (want.sum(axis=2) > 0).all()
    _same_as_twin(ctx, twin)


# ------------------------------------------------------------------------------------------------ 4. the field
def _field_ctx(ctx, n_origins, origin, births):
    ctx.age_enable(1, 1); ctx.tag_enable(n_origins, 1)
    ctx.tag_set_origins(origin); ctx.age_set_births(births)
    ctx.route_enable()


@pytest.mark.parametrize("n_origins", [1, 3, 16])
@pytest.mark.parametrize("sort", [True, False])
def test_4_one_sample_is_two_bincounts_of_the_virtual_id(box, gpu_ctx_factory, sort, n_origins):
    ctx = gpu_ctx_factory()
    _located(ctx, box["mesh"], box["xyz"], sort)
    ctx.step(0.1, 0.0, NOW)
    origin = _origins(N, n_origins, 50 + n_origins)
    ages = np.random.default_rng(n_origins).integers(0, 5000, size=N)
    ages[::101] = 2 ** 32 - 1 - np.arange(ages[::101].size)                  # wrapped stamps: the 64-bit sums must carry them
    _field_ctx(ctx, n_origins, origin, _births(NOW, ages))
    ctx.route_sample()
    s, c, ns = ctx.route_field()
    ws, wc = RT.field(ctx.get_particles()[1], origin, ages, 60, n_origins)
    assert ns == 1 and np.array_equal(c, wc) and np.array_equal(s, ws) and int(c.sum()) == N and (c.sum(0) > 0).all()
    # at the same point its counts are a tag sample's and its sums, over the origins, an age sample's
    ctx.tag_sample(); ctx.age_sample()
    assert np.array_equal(c, ctx.tag_field()[0].T)
    asum, acount, _ = ctx.age_field()
    assert np.array_equal(s.sum(1), asum) and np.array_equal(c.sum(1), acount)
    m = ctx.mean_age_by_origin(0.5)
    assert m.shape == (60, n_origins) and np.array_equal(np.isnan(m), wc == 0)
    assert np.array_equal(m[wc > 0], ws[wc > 0].astype(np.float64) / wc[wc > 0].astype(np.float64) * 0.5)


def test_4_a_window_wider_than_the_bins_goes_through_the_cache(gpu_ctx_factory):
    """an unsorted cloud on 1200 cells with 16 origins: every slice's window of virtual ids is wider than the 2048 bins"""
    mesh = box_mesh(12, 10, 10)
    xyz = pz.uniform_points(81, N, (0.0, 0.0, 0.0), (12.0, 10.0, 10.0))
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, False)
    cell = ctx.get_particles()[1]
    origin = _origins(N, 16, 60)
    for lo in range(0, N, 4096):
        v = cell[lo:lo + 4096].astype(np.int64) * 16 + origin[lo:lo + 4096]
        assert v.max() - v.min() + 1 > RT.FIELD_BINS
    ages = np.random.default_rng(2).integers(0, 2 ** 32, size=N)
    _field_ctx(ctx, 16, origin, _births(0, ages))
    ctx.route_sample(); ctx.route_sample()
    s, c, ns = ctx.route_field()
    ws, wc = RT.field(cell, origin, ages, mesh.n_cells, 16)
    assert ns == 2 and np.array_equal(c, 2 * wc) and np.array_equal(s, 2 * ws) and int(c.sum()) == 2 * N


BIG = (40, 30, 30)


@pytest.fixture(scope="module")
def big_ctx():
    with api.Context(0) as ctx:
        ctx.set_mesh(box_mesh(*BIG))
        yield ctx


def _adversarial_case(big_ctx, c, o, n_origins, name):
    ages = np.random.default_rng(c.size).integers(0, 2 ** 32, size=c.size)
    big_ctx.set_particles(np.zeros((c.size, 3)), c)                          # the cells as given; gid = index
    _field_ctx(big_ctx, n_origins, o, _births(0, ages))
    big_ctx.route_sample()
    s, k, ns = big_ctx.route_field()
    ws, wc = RT.field(np.where((c >= 0) & (c < T.N_BIG), c, -1), o, ages, T.N_BIG, n_origins)
    assert ns == 1 and np.array_equal(k, wc) and np.array_equal(s, ws), (name, np.argwhere(k != wc)[:8], np.argwhere(s != ws)[:8])


@pytest.mark.parametrize("n_origins", [16, 1])
def test_4_windows_of_exactly_2048_and_2049_virtual_ids(big_ctx, n_origins):
    c, o = RT.window_edge(n_origins)
    _adversarial_case(big_ctx, c, o, n_origins, "window_edge")


@pytest.mark.parametrize("n_origins", [16, 1])
@pytest.mark.parametrize("name", T.ADVERSARIAL)
def test_4_adversarial_cell_arrays(big_ctx, name, n_origins):
    c, o = T.adversarial(name, n_origins)
    _adversarial_case(big_ctx, c, o, n_origins, name)


def test_4_decomposed_cells_sum_per_parent(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(20_000, 3))
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    assert ctx.mesh_quality()["n_derived"] > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.step(0.05, 0.0, 5)
    origin = _origins(20_000, 3, 61)
    ages = rng.integers(0, 1000, size=20_000)
    _field_ctx(ctx, 3, origin, _births(5, ages))
    ctx.route_sample()
    s, c, ns = ctx.route_field()
    ws, wc = RT.field(ctx.get_particles()[1], origin, ages, 120, 3)          # parent ids
    assert s.shape == (120, 3) and ns == 1 and np.array_equal(c, wc) and np.array_equal(s, ws) and int(c.sum()) == 20_000


def test_4_samples_agree_with_age_and_tags_across_steps_resorts_and_recycling(box, gpu_ctx_factory):
    mesh = box["mesh"]
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", 3)
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.5
    U[:, 0] += 1.0
    ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(box["xyz"]); ctx.set_seed(SEED)
    ctx.locate_initial()
    ctx.age_enable(2, 8); ctx.tag_enable(3, 2)
    ctx.set_sink_groups(box["sink"], np.arange(box["sink"].size) % 2)
    ctx.set_box_origin(2)
    ctx.tag_set_origins(_origins(N, 2, 62))                                  # origins 0 and 1; 2 is the box's
    ctx.route_enable()
    ctx.age_reset(); ctx.tag_reset(); ctx.route_reset()                      # the common reset
    ws, wc = np.zeros((60, 3), np.uint64), np.zeros((60, 3), np.uint64)
    wh = np.zeros((3, 2, 8), np.uint64)
    group = T.group_of_cell(60, box["sink"], np.arange(box["sink"].size) % 2)
    for k in range(3):
        ctx.step(0.05, 1e-3, 4)                                              # (a re-sort falls into every one of these)
        now = 4 * (k + 1)
        cell0, origin, ages = ctx.get_particles()[1], ctx.tag_origins(), A.ages(now, ctx.age_births())
        ctx.sink_apply()
        wh += RT.hist(origin, group, cell0, np.isin(cell0, box["sink"]), ages, 2, 8, 3, 2)
        if k == 1:
            ctx.respawn_box((0.0, 0.0, 0.0), (1.0, 4.0, 3.0))                # k == 0, 2: the absorbed stay dead through the sample
        ctx.route_sample(); ctx.age_sample(); ctx.tag_sample()
        cell = ctx.get_particles()[1]
        assert ((cell < 0).sum() > 0) == (k != 1)
        ds, dc = RT.field(cell, ctx.tag_origins(), A.ages(now, ctx.age_births()), 60, 3)
        ws += ds; wc += dc
        s, c, ns = ctx.route_field()
        assert ns == k + 1 and np.array_equal(s, ws) and np.array_equal(c, wc)
        tf, tns = ctx.tag_field()
        asum, acount, ans = ctx.age_field()
        assert tns == ans == ns and np.array_equal(c, tf.T) and np.array_equal(s.sum(1), asum) and np.array_equal(c.sum(1), acount)
        h = ctx.route_histogram()
        assert np.array_equal(h, wh) and np.array_equal(h.sum(2), ctx.transfer()) and np.array_equal(h.sum((0, 1)), ctx.age_histogram())
    assert wc[:, 2].any() and int(wh.sum()) == ctx.recycle_counts()["absorbed"] > 0


# ------------------------------------------------------------------------------------------------ 5. resets
def test_5_each_reset_zeroes_its_own_tables_only(box, gpu_ctx_factory):
    mesh, sink = box["mesh"], box["sink"]
    origin, births = _origins(N, 3, 70), _births(NOW, _edge_ages(N, 7, 16, 7))

    def routed():
        ctx = gpu_ctx_factory()
        _located(ctx, mesh, box["xyz"], True)
        ctx.step(0.1, 0.0, NOW)
        ctx.age_enable(7, 16); ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, np.arange(sink.size) % 2)
        ctx.tag_set_origins(origin); ctx.age_set_births(births)
        ctx.route_enable()
        return ctx
    ctx = routed()
    ctx.route_sample(); ctx.age_sample(); ctx.tag_sample(); ctx.sink_apply()
    h, (s, c, ns) = ctx.route_histogram(), ctx.route_field()
    transfer, hist, tfield, afield = ctx.transfer(), ctx.age_histogram(), ctx.tag_field(), ctx.age_field()
    assert h.any() and s.any() and c.any() and ns == 1 and transfer.any() and hist.any()
    ctx.route_reset()                                                        # ... leaves transfer, the age histogram, origins, births
    assert not ctx.route_histogram().any() and not ctx.route_field()[0].any() and not ctx.route_field()[1].any()
    assert ctx.route_field()[2] == 0
    assert np.array_equal(ctx.transfer(), transfer) and np.array_equal(ctx.age_histogram(), hist)
    assert np.array_equal(ctx.tag_origins(), origin) and np.array_equal(ctx.age_births(), births)
    assert np.array_equal(ctx.tag_field()[0], tfield[0]) and ctx.tag_field()[1] == 1
    assert np.array_equal(ctx.age_field()[0], afield[0]) and ctx.age_field()[2] == 1
    # cpf_age_reset and cpf_tag_reset leave the route tables alone
    ctx = routed()
    ctx.route_sample(); ctx.sink_apply()
    h2, (s2, c2, ns2) = ctx.route_histogram(), ctx.route_field()
    assert np.array_equal(h2, h) and np.array_equal(s2, s) and np.array_equal(c2, c)
    ctx.age_reset(); ctx.tag_reset()
    assert not ctx.transfer().any() and not ctx.age_histogram().any()
    assert np.array_equal(ctx.route_histogram(), h) and ctx.route_field()[2] == 1
    assert np.array_equal(ctx.route_field()[0], s) and np.array_equal(ctx.route_field()[1], c)


# ------------------------------------------------------------------------------------------------ 6. whole recycled runs
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_6_a_recycled_run_carries_its_routes(name, gpu_ctx_factory, oracle_libs):
    """tests/test_gpu_tags.py's whole runs with age on, once with routes and once without: the same bits either way, and the CPU
    statement's; the joint histogram and the field are the statement's (tests/routes.py) at every recycle point.  "thin box"
    takes one LIMITED respawn (half the dead) in its sixth round."""
    r, c = T.run(name), RT.cpu(name)
    b = r.base
    limited = RT.LIMITED_ROUND[name]
    out = {}
    for routed in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", b.sort_interval)
        ctx.set_mesh(b.mesh); ctx.set_velocity(b.U); ctx.set_seed(SEED)
        ctx.synchronize()
        ctx.set_source_triangles(b.tri, b.weights, b.depth)
        ctx.set_particles(b.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(b.sink_cells)
        ctx.age_enable(RT.BIN_CYCLES, RT.N_BINS)
        ctx.tag_enable(T.N_ORIGINS, T.N_SINKS)
        ctx.set_sink_groups(b.sink_cells, r.groups)
        ctx.set_source_origins(r.origin_of_triangle)
        if routed:
            ctx.route_enable()
        for k in range(b.rounds):
            ctx.step(b.dt, 0.0, b.cycles)
            ctx.sink_apply()
            ctx.respawn_source(c["limited_count"] if k == limited else -1)
            if routed:
                ctx.route_sample()
                want = c["rounds"][k]
                s, cnt, ns = ctx.route_field()
                assert ns == k + 1 and np.array_equal(ctx.route_histogram(), want["hist"]), (name, k)
                assert np.array_equal(s, want["field_sum"]) and np.array_equal(cnt, want["field_count"]), (name, k)
        out[routed] = (ctx.get_particles(), ctx.transfer(), ctx.age_histogram(), ctx.age_births(), ctx.tag_origins())
        assert ctx.recycle_counts() == dict(absorbed=c["absorbed"], drawn=c["drawn"], placed=c["placed"], epochs=b.rounds)
    for routed in (True, False):
        (xyzw, cell), transfer, hist, births, origin = out[routed]
        bad = np.nonzero(cell != c["cell"])[0]
        assert bad.size == 0, (name, routed, "cells differ", bad.size, bad[:5], cell[bad[:5]], c["cell"][bad[:5]])
        bad = np.nonzero((_bits(xyzw[:, :3]) != _bits(c["xyz"])).any(1))[0]
        assert bad.size == 0, (name, routed, "positions differ", bad.size, bad[:5])
        assert np.array_equal(transfer, c["hist"].sum(2)) and np.array_equal(hist, c["hist"].sum((0, 1)))
        assert np.array_equal(births, c["births"]) and np.array_equal(origin, c["origin"])
    assert np.array_equal(_bits(out[True][0][0]), _bits(out[False][0][0]))
    assert int(c["hist"].sum()) == c["absorbed"] >= 200 and (c["hist"].sum(2)[1:] > 0).all()
    assert (c["hist"].sum((0, 1)) > 0).sum() >= 2                            # more than one residence time


# ------------------------------------------------------------------------------------------------ 7. through CudaParticles
def test_7_cuda_particles_route_stats(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13                                                          # 10 * dt / dt == 10 exactly
    sink = mesh.patch_cells("outlet")
    centres = pitz["centres"]
    groups = (centres[sink, 1] > np.median(centres[sink, 1])).astype(np.int32)
    tri, of = mesh.face_triangles(mesh.patch_faces("inlet"))
    y = tri.mean(1)[:, 1]
    origins = np.where(y > np.median(y), 2, 1).astype(np.int32)              # 0 is the initial cloud
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=2,
             occupancyInterval=4, sinkCells=sink, sourceTriangles=tri, sourceWeights=api.inflow_weights(mesh, U, tri, of),
             sourceDepth=(0.0, 1e-4), sinkGroups=groups, sourceOrigins=origins, ageBins=8)
    p = api.CudaParticles(mesh, U, dict(d, routeStats=True))
    q = api.CudaParticles(mesh, U, d)
    try:
        assert p.routeStats and not q.routeStats
        for k in range(3):
            for run in (p, q):
                assert run.advect(k * 10 * dt, 10 * dt) == 10
        edges, counts = p.rtd_by_route()
        assert counts.shape == (3, 2, 8) and np.array_equal(edges, p.rtd()[0])
        assert np.array_equal(counts.sum((0, 1)), p.rtd()[1]) and np.array_equal(counts.sum(2), p.transfer())
        assert int(counts.sum()) == p.recycle_counts()["absorbed"] > 0
        s, c, ns = p.ctx.route_field()
        assert ns == 7 and np.array_equal(c, p.ctx.tag_field()[0].T) and np.array_equal(s.sum(1), p.ctx.age_field()[0])
        m = p.mean_age_by_origin()
        assert m.shape == (mesh.n_cells, 3) and np.array_equal(np.isnan(m), c == 0) and (m[c > 0] >= 0).all()
        # routes change nothing of the run, nor of what age and tags report
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        assert np.array_equal(p.transfer(), q.transfer()) and np.array_equal(p.rtd()[1], q.rtd()[1])
        assert np.array_equal(p.concentration(), q.concentration())
        assert np.array_equal(p.mean_age(), q.mean_age(), equal_nan=True)
        with pytest.raises(L.CpfError):
            q.rtd_by_route()
        with pytest.raises(ValueError):
            api.CudaParticles(mesh, U, dict(d, routeStats=True, ageBins=0)).close()
    finally:
        p.close(); q.close()
