"""GPU: the sink log (include/cpf.h "sink log"; csrc/cpf_sinklog.hip).  Every comparison is equality of bytes: the records against
the numpy statement of tests/sinklog.py over what ``get_particles()`` and the groups' tables held before the apply, every table
of the five groups rebuilt from the records of whole recycled runs, and the cloud, the counters and every table against a twin
context without the log."""
import ctypes as C

import numpy as np
import pytest

import recycle as R
import sinklog as S
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
ALL = ("age", "tags", "routes", "exposure", "zones")
N_ZONES, AGE_BINS, AGE_BIN_CYCLES, DOSE_BINS, DOSE_WIDTH = 5, 4, 2, 16, 0.1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


def _located(ctx, mesh, xyz, mode, cell=None):
    """a located cloud at rest, in one of MODES; returns the context's cycle counter (a fresh context starts at 0)"""
    ctx.set_mesh(mesh); ctx.set_velocity(np.zeros((mesh.n_cells, 3))); ctx.set_seed(SEED)
    ctx.set_particles(xyz, cell)
    if cell is None:
        assert ctx.locate_initial() == 0
    if mode in ("sorted", "permuted"):
        ctx.sort_by_cell()
    if mode == "permuted":                                                   # three cycles in a random field scatter the cells again
        U = np.random.default_rng(17).normal(size=(mesh.n_cells, 3))
        ctx.set_velocity(U); ctx.step(0.3, 0.0, 3); ctx.set_velocity(np.zeros((mesh.n_cells, 3)))
        return 3
    return 0


def _refused(status, call):
    with pytest.raises(L.CpfError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert str(e.value)                                                      # ... with a message


def _groups_on(ctx, which, n, now, sink, n_cells, seed=40):
    """turns the groups of ``which`` on, in CudaParticles' order, and gives their tables values no run of this file produces"""
    rng = np.random.default_rng(seed)
    groups = np.arange(sink.size) % 2
    if "age" in which:
        ctx.age_enable(AGE_BIN_CYCLES, AGE_BINS)
        ctx.age_set_births(rng.integers(0, now + 3, size=n).astype(np.uint32))      # (some "after" now: the difference wraps)
    if "tags" in which:
        ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups)
        ctx.tag_set_origins(rng.integers(0, 3, size=n).astype(np.uint8))
    if "routes" in which:
        ctx.route_enable()
    if "exposure" in which:
        ctx.exposure_enable(DOSE_WIDTH, DOSE_BINS); ctx.exposure_set_doses(rng.uniform(0.0, 2.0, size=n))
    if "zones" in which:
        ctx.zone_enable(N_ZONES); ctx.set_zone_map((np.arange(n_cells) % N_ZONES).astype(np.int32))
        ctx.zone_set_last(np.where(rng.random(n) < 0.33, Z.OUTSIDE, rng.integers(0, N_ZONES, size=n)).astype(np.uint8))
    return S.group_of_cells(n_cells, sink, groups)


def _want(ctx, which, sink, now, apply, group_of):
    """the statement's records of the next apply, from what the context holds now"""
    xyzw, cell = ctx.get_particles()
    return S.records(xyzw, cell, sink, now, apply,
                     births=ctx.age_births() if "age" in which else None,
                     origins=ctx.tag_origins() if "tags" in which else None, sink_group_of=group_of,
                     doses=ctx.exposure_doses() if "exposure" in which else None,
                     last=ctx.zone_last() if "zones" in which else None)


def _tables(ctx, which):
    """the cloud, the counters and every table of every group that is on, as bytes"""
    xyzw, cell = ctx.get_particles()
    out = dict(x=_bits(xyzw).tobytes(), cell=cell.tobytes(), recycle=repr(sorted(ctx.recycle_counts().items())),
               counters=repr(sorted(ctx.counters().items())))
    if "age" in which:
        out.update(age_hist=ctx.age_histogram().tobytes(), births=ctx.age_births().tobytes())
    if "tags" in which:
        out.update(transfer=ctx.transfer().tobytes(), origins=ctx.tag_origins().tobytes())
    if "routes" in which:
        out.update(routes=ctx.route_histogram().tobytes())
    if "exposure" in which:
        out.update(dose_hist=ctx.dose_histogram().tobytes(), doses=_bits(ctx.exposure_doses()).tobytes())
    if "zones" in which:
        out.update(flows=ctx.zone_flows()[0].tobytes(), last=ctx.zone_last().tobytes())
    return out


def _same_tables(ctx, twin, which):
    a, b = _tables(ctx, which), _tables(twin, which)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] == b[k], k


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, sink=_last_x_layer(mesh), xyz=pz.uniform_points(77, N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)),
                U=np.random.default_rng(18).normal(size=(60, 3)))


# ------------------------------------------------------------------------------------------------ 1. lifecycle
def test_1_lifecycle(box):
    mesh, xyz, sink = box["mesh"], box["xyz"], box["sink"]
    with api.Context(0) as ctx:
        needs_on = (ctx.sink_log_clear, ctx.sink_log_counts, ctx.sink_log_read, lambda: ctx.sink_log_read(3), ctx.sink_log_drain)

        def off():
            for g in needs_on:
                _refused(L.CPF_ERR_STATE, g)

        _refused(L.CPF_ERR_STATE, lambda: ctx.sink_log_enable(8))            # no mesh
        ctx.set_mesh(mesh)
        _refused(L.CPF_ERR_STATE, lambda: ctx.sink_log_enable(8))            # no cloud
        ctx.sink_log_disable()                                               # off already: no error
        ctx.set_particles(xyz)
        _refused(L.CPF_ERR_STATE, lambda: ctx.sink_log_enable(8))            # ... set, but not located
        off()
        ctx.locate_initial()
        for capacity in (0, -1, -2 ** 40):
            _refused(L.CPF_ERR_ARG, lambda: ctx.sink_log_enable(capacity))
        off()                                                                # a refused enable leaves it off
        # on, without a sink set: an apply logs nothing and is not counted
        ctx.sink_log_enable(N_T)
        assert ctx.sink_log_counts() == (0, 0) and ctx.sink_log_read().shape == (0,) and ctx.sink_log_read().dtype == api.SINK_LOG_DTYPE
        ctx.sink_apply()
        assert ctx.sink_log_counts() == (0, 0)
        ctx.set_sink_cells(sink)
        want = _want(ctx, (), sink, 0, 0, None)
        ctx.sink_apply()
        assert ctx.sink_log_counts() == (want.size, 0) and want.size > 1000
        S.same(ctx.sink_log_read(), want)
        S.same(ctx.sink_log_read(), want)                                    # a read changes nothing
        # the C entry: nullable counts, a null buffer only with room for nothing, no negative room
        got = C.c_int64(-1)
        assert ctx.lib.cpf_sink_log_counts(ctx.h, None, None) == L.CPF_OK
        assert ctx.lib.cpf_sink_log_read(ctx.h, None, 0, C.byref(got)) == L.CPF_OK and got.value == 0
        assert ctx.lib.cpf_sink_log_read(ctx.h, None, 5, C.byref(got)) == L.CPF_ERR_ARG
        assert ctx.lib.cpf_sink_log_read(ctx.h, None, -1, None) == L.CPF_ERR_ARG
        # clear keeps apply counting: the next apply is number 1, and the first record again
        ctx.sink_log_clear()
        assert ctx.sink_log_counts() == (0, 0)
        ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))                    # into the sink's layer
        want1 = _want(ctx, (), sink, 0, 1, None)
        ctx.sink_apply()
        assert want1.size == want.size
        S.same(ctx.sink_log_read(), want1)
        # drain: read, then clear
        S.same(ctx.sink_log_drain(), want1)
        assert ctx.sink_log_counts() == (0, 0)
        # enabling again resets the cursor and apply
        ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        ctx.sink_apply()
        assert ctx.sink_log_counts() == (want.size, 0) and (ctx.sink_log_read()["apply"] == 2).all()
        ctx.sink_log_enable(N_T)
        assert ctx.sink_log_counts() == (0, 0)
        ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        want0 = _want(ctx, (), sink, 0, 0, None)
        ctx.sink_apply()
        S.same(ctx.sink_log_read(), want0)
        # the _dev entry does not log
        ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        before = ctx.recycle_counts()["absorbed"]
        ctx.sink_log_clear()
        # (the context's own cell array has no public address: a caller's array stands in)
        dev = C.c_void_p()
        cells = np.full(64, int(sink[0]), np.int32)
        ctx._ck(ctx.lib.cpf_dev_alloc(ctx.h, cells.nbytes, C.byref(dev)))
        ctx._ck(ctx.lib.cpf_copy_to_device(ctx.h, dev, api._ptr(cells), cells.nbytes))
        ctx.sink_apply_dev(dev, 64)
        assert ctx.recycle_counts()["absorbed"] == before + 64 and ctx.sink_log_counts() == (0, 0)
        ctx._ck(ctx.lib.cpf_dev_free(ctx.h, dev))
        # everything that replaces the cloud or the mesh turns it off; the five other groups do not
        for turn_off in (lambda: ctx.set_particles(xyz), lambda: ctx.set_mesh(mesh),
                         lambda: ctx.seed_box(N_T, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0))):
            ctx.set_particles(xyz); ctx.locate_initial()
            ctx.sink_log_enable(16)
            turn_off()
            off()
        ctx.set_particles(xyz); ctx.locate_initial()
        ctx.sink_log_enable(16)
        assert ctx.lib.cpf_alloc_particles(ctx.h, 2 * N_T) == L.CPF_OK       # (a new allocation: no cloud until it is set)
        assert ctx.lib.cpf_sink_log_clear(ctx.h) == L.CPF_ERR_STATE and ctx.lib.cpf_sink_log_counts(ctx.h, None, None) == L.CPF_ERR_STATE
        ctx.set_particles(xyz); ctx.locate_initial()
        off()
        ctx.set_sink_cells(sink)
        ctx.sink_log_enable(N_T)
        ctx.age_enable(2, 4); ctx.tag_enable(3, 2); ctx.route_enable(); ctx.exposure_enable(0.5, 4); ctx.zone_enable(4)
        ctx.route_disable(); ctx.exposure_disable(); ctx.tag_disable(); ctx.age_disable(); ctx.zone_disable()
        want = _want(ctx, (), sink, 0, 0, None)
        ctx.sink_apply()
        S.same(ctx.sink_log_read(), want)
        ctx.age_enable(2, 4); ctx.zone_enable(4)
        ctx.sink_log_disable()
        off()
        assert ctx.age_histogram().shape == (4,) and ctx.zone_flows()[0].shape == (5, 5)      # ... nor they by the log
        # with the log off again the sink is the one of before
        ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
        before = ctx.recycle_counts()["absorbed"]
        ctx.sink_apply()
        assert ctx.recycle_counts()["absorbed"] == before + want.size


# ------------------------------------------------------------------------------------------------ 2. one apply against the statement
@pytest.mark.parametrize("n", [N_T, 4096, 4095, 1])
@pytest.mark.parametrize("mode", MODES)
def test_2_one_apply_appends_exactly_the_records_of_the_statement(box, gpu_ctx_factory, mode, n):
    """all five groups on, tables of random values; dead slots (CPF_CELL_LOST, and CPF_CELL_FROZEN where the cells can be given)
    are not logged"""
    mesh, sink = box["mesh"], box["sink"]
    xyz = box["xyz"][:n].copy()
    xyz[0] = (4.5, 0.5, 0.5)                                                 # (somebody is absorbed)
    ctx = gpu_ctx_factory()
    if mode == "index":                                                      # the cells as given: every ninth lost, every tenth frozen
        now = _located(ctx, mesh, xyz, mode)
        cell = ctx.get_particles()[1].copy()
        cell[4::9] = -1; cell[5::10] = -2
        now = _located(ctx, mesh, xyz, mode, cell if n > 1 else None)
    elif mode == "permuted" and n == 1:                                      # a start from which the three cycles end in the sink
        now = 0
        for start in box["xyz"][:200]:
            xyz[0] = start
            now += _located(ctx, mesh, xyz, mode)                            # (the cycle counter goes on counting)
            if np.isin(ctx.get_particles()[1], sink).all():
                break
    else:
        now = _located(ctx, mesh, xyz, mode)
        if n > 1:
            ctx.set_sink_cells(np.arange(0, 60, 7).astype(np.int32)); ctx.sink_apply()      # the absorbed are dead slots
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ALL, n, now, sink, 60)
    ctx.sink_log_enable(n)
    xyzw, cell0 = ctx.get_particles()
    assert n < 100 or ((cell0 < 0).sum() > n // 20 and np.isin(cell0[cell0 < 0], [-1, -2]).all())
    want = _want(ctx, ALL, sink, now, 0, group_of)
    before = ctx.recycle_counts()["absorbed"]
    ctx.sink_apply()
    got = ctx.sink_log_read()
    S.same(got, want)
    assert ctx.sink_log_counts() == (want.size, 0) and want.size == ctx.recycle_counts()["absorbed"] - before >= 1
    assert n < 100 or want.size > n // 10
    # the positions are the bits get_particles() held for that id, the cell the one it was found in
    assert np.array_equal(_bits(got["x"]), _bits(xyzw[got["id"], 0])) and np.array_equal(_bits(got["z"]), _bits(xyzw[got["id"], 2]))
    assert np.array_equal(got["cell"], cell0[got["id"]]) and np.isin(got["cell"], sink).all()
    assert (got["fields"] == 15).all() and (got["cycle"] == now).all() and not got["reserved"].any()
    assert n < 100 or (np.unique(got["origin"]).size == 3 and np.unique(got["group"]).size == 2 and (got["zone"] == 0xFF).any()
                       and (got["age"] > 2 ** 31).any())
    assert np.array_equal(ctx.get_particles()[1], R.sink(cell0, sink))
    ctx.sink_apply()                                                         # a second apply finds nobody
    assert ctx.sink_log_counts() == (want.size, 0)


# ------------------------------------------------------------------------------------------------ 3. slices, workgroups, the mask
def test_3_a_slice_without_a_hit_next_to_one_with_hits(box, gpu_ctx_factory):
    mesh, sink = box["mesh"], box["sink"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], "index")
    cell = ctx.get_particles()[1].copy()
    cell[:4096] = np.where(np.isin(cell[:4096], sink), 0, cell[:4096])       # the first slice: nobody in the sink
    cell[4096:4096 + 64] = sink[0]                                           # the second: its first wave's first round all hits
    _located(ctx, mesh, box["xyz"], "index", cell)
    ctx.set_sink_cells(sink)
    ctx.sink_log_enable(N_T)
    want = _want(ctx, (), sink, 0, 0, None)
    ctx.sink_apply()
    S.same(ctx.sink_log_read(), want)
    assert want["id"].min() == 4096 and want.size > 500 and (want["fields"] == 0).all()


@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_3_every_particle_of_two_slices_and_a_tail_is_logged(box, gpu_ctx_factory, mode):
    """all-hit slices: every wave's list is full (1024 entries), a workgroup reserves 4096 records at once"""
    mesh, sink = box["mesh"], box["sink"]
    xyz = pz.uniform_points(5, N_T, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))        # all in the last x layer
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, mode)
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ALL, N_T, 0, sink, 60)
    ctx.sink_log_enable(N_T)
    want = _want(ctx, ALL, sink, 0, 0, group_of)
    ctx.sink_apply()
    S.same(ctx.sink_log_read(), want)
    assert want.size == N_T == ctx.recycle_counts()["absorbed"] and np.array_equal(want["id"], np.arange(N_T))
    assert (ctx.get_particles()[1] == -1).all()


def test_3_a_mask_too_large_for_lds_is_read_from_memory(gpu_ctx_factory):
    mesh = box_mesh(41, 40, 40)                                              # 65 600 cells: more bits than the 2048 staged words hold
    assert mesh.n_cells > 2048 * 32
    sink = _last_x_layer(mesh)
    assert sink.max() > 2048 * 32
    n = 36_000
    xyz = pz.uniform_points(79, n, (0.0, 0.0, 0.0), (41.0, 40.0, 40.0))
    xyz[:8] = pz.uniform_points(80, 8, (40.0, 39.0, 39.0), (41.0, 40.0, 40.0))              # the last cell: a bit beyond the staged words
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, "sorted")
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ("age", "tags"), n, 0, sink, mesh.n_cells)
    ctx.sink_log_enable(n)
    want = _want(ctx, ("age", "tags"), sink, 0, 0, group_of)
    ctx.sink_apply()
    S.same(ctx.sink_log_read(), want)
    assert want.size > 500 and want.size == ctx.recycle_counts()["absorbed"] and want["cell"].max() > 2048 * 32


def test_3_on_a_warped_mesh_the_cell_is_the_parent(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    n = N_T
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(n, 3))
    sink = _last_x_layer(box_mesh(6, 5, 4))                                  # (the warp keeps the numbering)
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(xyz)
    n_derived = int(ctx.mesh_quality()["n_derived"])
    assert n_derived > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.step(0.05, 0.0, 2); ctx.sort_by_cell()
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ("age", "tags"), n, 2, sink, 120)
    ctx.sink_log_enable(n)
    want = _want(ctx, ("age", "tags"), sink, 2, 0, group_of)               # (get_particles gives parent ids)
    ctx.sink_apply()
    got = ctx.sink_log_read()
    S.same(got, want)
    assert got.size > 1000 and got["cell"].max() < 120 and np.array_equal(np.unique(got["cell"]), np.sort(sink))
    assert np.unique(got["group"]).size == 2


# ------------------------------------------------------------------------------------------------ 4. groups
COMBOS = [(), ("age",), ("tags",), ("exposure",), ("zones",), ("age", "tags"), ("age", "tags", "routes"), ALL]


@pytest.mark.parametrize("which", COMBOS, ids=lambda w: "+".join(w) or "none")
@pytest.mark.parametrize("mode", ["sorted", "index"])
def test_4_fields_and_off_values_and_the_twin_without_the_log(box, gpu_ctx_factory, mode, which):
    mesh, sink, xyz = box["mesh"], box["sink"], box["xyz"]
    ctx, twin = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (ctx, twin):
        _located(c, mesh, xyz, mode)
        c.step(0.1, 0.0, 5)                                                  # (at rest: the cycle counter is 5)
        c.set_sink_cells(sink)
        group_of = _groups_on(c, which, N_T, 5, sink, 60)
    ctx.sink_log_enable(N_T)
    want = _want(ctx, which, sink, 5, 0, group_of)
    for k in range(2):                                                       # the second apply finds nobody
        ctx.sink_apply(); twin.sink_apply()
        _same_tables(ctx, twin, which)
    got = ctx.sink_log_read()
    S.same(got, want)
    bits = ("age" in which) * 1 + ("tags" in which) * 2 + ("exposure" in which) * 4 + ("zones" in which) * 8
    assert (got["fields"] == bits).all() and got.size == ctx.recycle_counts()["absorbed"] > 1000
    if "age" not in which:
        assert not got["age"].any()
    if "tags" not in which:
        assert (got["origin"] == 0xFF).all() and (got["group"] == 0xFF).all()
    else:
        assert got["origin"].max() == 2 and got["group"].max() == 1
    if "exposure" not in which:
        assert not _bits(got["dose"]).any()                                  # +0.0
    if "zones" not in which:
        assert (got["zone"] == 0xFF).all()
    # a group switched on or off between two applies shows in `fields`
    # zones go off where they were on; else age goes off (and takes routes with it) where it was on, and on where it was off
    if "zones" in which:
        now_on = tuple(g for g in which if g != "zones")
    elif "age" in which:
        now_on = tuple(g for g in which if g not in ("age", "routes"))
    else:
        now_on = which + ("age",)
    for c in (ctx, twin):
        c.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))                      # everybody absorbed comes back in the sink's layer
        if "zones" in which:
            c.zone_disable()
        elif "age" in which:
            c.age_disable()
        else:
            c.age_enable(AGE_BIN_CYCLES, AGE_BINS)
    want2 = _want(ctx, now_on, sink, 5, 2, group_of)                         # (the apply that found nobody was number 1)
    ctx.sink_apply(); twin.sink_apply()
    _same_tables(ctx, twin, now_on)
    got = ctx.sink_log_read()
    S.same(got, np.concatenate([want, want2]))
    bits2 = ("age" in now_on) * 1 + ("tags" in now_on) * 2 + ("exposure" in now_on) * 4 + ("zones" in now_on) * 8
    assert bits2 != bits and (got["fields"][want.size:] == bits2).all() and want2.size == want.size


# ------------------------------------------------------------------------------------------------ 5. capacity
def _overflowed(ctx, want, capacity):
    """`capacity` stored, the rest dropped; every stored record is the statement's for its id, no id twice"""
    assert ctx.sink_log_counts() == (capacity, want.size - capacity)
    got = ctx.sink_log_read()
    assert got.size == capacity and np.unique(got["id"]).size == capacity and (np.diff(got["id"]) > 0).all()
    at = np.searchsorted(want["id"], got["id"])
    assert np.array_equal(want["id"][at], got["id"])
    S.same(got, want[at])


def test_5_capacity(box, gpu_ctx_factory):
    mesh, sink = box["mesh"], box["sink"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], "sorted")
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ("age", "tags"), N_T, 0, sink, 60)
    which = ("age", "tags")
    hits = int(np.isin(ctx.get_particles()[1], sink).sum())
    assert hits > 1000
    # capacity == hits: everything, nothing dropped
    ctx.sink_log_enable(hits)
    want = _want(ctx, which, sink, 0, 0, group_of)
    ctx.sink_apply()
    assert ctx.sink_log_counts() == (hits, 0)
    S.same(ctx.sink_log_read(), want)
    # capacity == hits - 1: one record is dropped, the others are whole
    ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
    ctx.sink_log_enable(hits - 1)
    want = _want(ctx, which, sink, 0, 0, group_of)
    assert want.size == hits
    ctx.sink_apply()
    _overflowed(ctx, want, hits - 1)
    # a second apply after the overflow stores nothing and adds its hits to dropped
    stored = ctx.sink_log_read()
    ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0))
    ctx.sink_apply()
    assert ctx.sink_log_counts() == (hits - 1, 1 + hits)
    S.same(ctx.sink_log_read(), stored)
    # after a clear the next apply is complete (five fewer are respawned, so that it fits) and is apply 2
    ctx.sink_log_clear()
    ctx.respawn_box((4.0, 0.0, 0.0), (5.0, 4.0, 3.0), hits - 5)
    want = _want(ctx, which, sink, 0, 2, group_of)
    assert want.size == hits - 5
    ctx.sink_apply()
    assert ctx.sink_log_counts() == (hits - 5, 0)
    S.same(ctx.sink_log_read(), want)


def test_5_room_for_one_record_and_4096_hits(box, gpu_ctx_factory):
    mesh, sink = box["mesh"], box["sink"]
    xyz = pz.uniform_points(6, 4096, (4.0, 0.0, 0.0), (5.0, 4.0, 3.0))       # one slice, every slot a hit
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, xyz, "sorted")
    ctx.set_sink_cells(sink)
    group_of = _groups_on(ctx, ALL, 4096, 0, sink, 60)
    ctx.sink_log_enable(1)
    want = _want(ctx, ALL, sink, 0, 0, group_of)
    assert want.size == 4096
    ctx.sink_apply()
    _overflowed(ctx, want, 1)
    got = C.c_int64(-1)
    rec = np.zeros(4, api.SINK_LOG_DTYPE)
    assert ctx.lib.cpf_sink_log_read(ctx.h, api._ptr(rec), 4, C.byref(got)) == L.CPF_OK and got.value == 1
    assert not rec[1:].view(np.uint8).any()                                  # nothing is written behind the stored records


# ------------------------------------------------------------------------------------------------ 6. two applies
@pytest.mark.parametrize("source", [False, True])
def test_6_two_applies_with_a_respawn_of_all_between(box, gpu_ctx_factory, source):
    """apply 0 takes the last x layer of the initial cloud; everybody is respawned at the inlet end (in the box, or on the source's
    triangles), one cycle in a field with a random part carries them and others into the sink's layer, apply 1 takes those"""
    mesh, sink = box["mesh"], box["sink"]
    ctx = gpu_ctx_factory()
    _located(ctx, mesh, box["xyz"], "sorted")
    ctx.set_sink_cells(sink)
    if source:
        tri, _ = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
        ctx.set_source_triangles(tri, None, (0.0, 0.5))
    group_of = _groups_on(ctx, ALL, N_T, 0, sink, 60)
    ctx.set_box_origin(2)
    if source:
        ctx.set_source_origins(np.arange(tri.shape[0]) % 3)
    ctx.set_exposure_field(np.random.default_rng(8).uniform(0.0, 1.0, size=60))
    ctx.sink_log_enable(2 * N_T)
    want0 = _want(ctx, ALL, sink, 0, 0, group_of)
    ctx.sink_apply()
    if source:
        ctx.respawn_source(-1)
    else:
        ctx.respawn_box((0.0, 0.0, 0.0), (0.5, 4.0, 3.0), -1)
    assert (ctx.get_particles()[1] >= 0).all()
    U = box["U"] * 0.1
    U[:, 0] += 4.2
    ctx.set_velocity(U); ctx.step(1.0, 0.0, 1)
    ctx.exposure_accumulate(1.0); ctx.zone_sample()
    want1 = _want(ctx, ALL, sink, 1, 1, group_of)
    respawned = np.isin(want1["id"], want0["id"])
    assert respawned.sum() > 500 and (~respawned).sum() > 500
    assert (want1["age"][respawned] == 1).all() and (want1["zone"] != 0xFF).all() and (want1["dose"] > 0).any()
    ctx.sink_apply()
    want = np.concatenate([want0, want1])
    got = ctx.sink_log_read()
    S.same(got, want)
    assert ctx.sink_log_counts() == (want.size, 0)
    assert (got["apply"][:want0.size] == 0).all() and (got["apply"][want0.size:] == 1).all()
    assert (got["cycle"][:want0.size] == 0).all() and (got["cycle"][want0.size:] == 1).all()
    # a read with less room than records returns the sorted prefix
    for room in (1, want0.size - 1, want0.size + 7):
        S.same(ctx.sink_log_read(room), want[:room])
    S.same(ctx.sink_log_read(want.size + 100), want)
    assert ctx.sink_log_counts() == (want.size, 0)


# ------------------------------------------------------------------------------------------------ 7. whole recycled runs
def _age_bin(age, bin_cycles, n_bins):
    return np.minimum(age.astype(np.int64) // bin_cycles, n_bins - 1)


def _dose_bin(dose, width, n_bins):
    out = np.empty(dose.size, np.int32)
    d = np.ascontiguousarray(dose, np.float64)
    assert L.load().cpf_exposure_bins_host(api._ptr(d), d.size, float(width), int(n_bins), api._ptr(out)) == L.CPF_OK
    return out


@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_7_every_table_of_a_recycled_run_is_a_reduction_of_the_records(name, gpu_ctx_factory):
    """tests/test_gpu_recycle.py's whole runs (D = 0; "graded box" re-sorts every round, "thin box" is the flat walk), 36 cycles, a
    cycle a launch, all five groups on, with the log and without"""
    r = R.run(name)
    n, n_zones, bin_cycles, n_bins, dose_bins = r.xyz.shape[0], 4, 2, 8, 8
    zone_of = Z.x_slabs(r.mesh, n_zones)
    rate = np.random.default_rng(5).uniform(0.0, 1.0, size=r.mesh.n_cells)
    width = 0.25 * r.dt * r.rounds * r.cycles / dose_bins
    groups = np.arange(r.sink_cells.size) % 2
    out = {}
    for logged in (True, False):
        ctx = gpu_ctx_factory()
        ctx.set_option("sort_interval", r.sort_interval)
        ctx.set_mesh(r.mesh); ctx.set_velocity(r.U); ctx.set_seed(SEED)
        ctx.synchronize()
        ctx.set_particles(r.xyz)
        assert ctx.locate_initial() == 0
        ctx.set_sink_cells(r.sink_cells)
        ctx.age_enable(bin_cycles, n_bins)
        ctx.tag_enable(2, 2); ctx.set_sink_groups(r.sink_cells, groups); ctx.set_box_origin(1)
        ctx.route_enable()
        ctx.exposure_enable(width, dose_bins); ctx.set_exposure_field(rate)
        ctx.zone_enable(n_zones); ctx.set_zone_map(zone_of)
        if logged:
            ctx.sink_log_enable(n * r.rounds)
        for k in range(r.rounds):
            for j in range(r.cycles):
                ctx.step(r.dt, 0.0, 1)
                ctx.exposure_accumulate(r.dt); ctx.zone_sample()
            ctx.sink_apply()
            ctx.respawn_box(r.box[0], r.box[1])
        lost = ctx.counters()["lost"]
        print("MEASURED %s logged %s: lost %d, absorbed %d" % (name, logged, lost, ctx.recycle_counts()["absorbed"]))
        assert lost == 0, (name, lost)                                       # the sink is the only way to die
        out[logged] = _tables(ctx, ALL)
        if not logged:
            continue
        assert r.rounds * r.cycles <= 40
        rec = ctx.sink_log_read()
        absorbed = ctx.recycle_counts()["absorbed"]
        assert ctx.sink_log_counts() == (absorbed, 0) and len(rec) == absorbed >= 200
        assert np.array_equal(rec["cycle"], (rec["apply"].astype(np.int64) + 1) * r.cycles) and rec["apply"].max() == r.rounds - 1
        assert (rec["fields"] == 15).all()
        a = _age_bin(rec["age"], bin_cycles, n_bins)
        assert np.array_equal(np.bincount(a, minlength=n_bins).astype(np.uint64), ctx.rtd(r.dt)[1])
        o, g = rec["origin"].astype(np.int64), rec["group"].astype(np.int64)
        transfer = np.zeros((2, 2), np.uint64)
        np.add.at(transfer, (o, g), np.uint64(1))
        assert np.array_equal(transfer, ctx.transfer()) and (transfer[0] > 0).all() and int(transfer.sum()) == absorbed
        routes = np.zeros((2, 2, n_bins), np.uint64)
        np.add.at(routes, (o, g, a), np.uint64(1))
        assert np.array_equal(routes, ctx.rtd_by_route(r.dt)[1])
        d = _dose_bin(rec["dose"], width, dose_bins)
        assert (d >= 0).all()
        doses = np.zeros((2, 2, dose_bins), np.uint64)
        np.add.at(doses, (o, g, d), np.uint64(1))
        assert np.array_equal(doses, ctx.dose_distribution()[1]) and (doses.sum(axis=(0, 1)) > 0).sum() > 2
        outside = np.bincount(Z.row_of(rec["zone"], n_zones), minlength=n_zones + 1).astype(np.uint64)
        assert np.array_equal(outside, ctx.zone_flows()[0][:, n_zones])
        # what no table holds: an exact median of the residence time, and every id that left
        assert np.median(rec["age"]) > 0 and np.unique(rec["id"]).size <= n
    assert sorted(out[True]) == sorted(out[False])
    for k in out[True]:
        assert out[True][k] == out[False][k], k


# ------------------------------------------------------------------------------------------------ 8. through CudaParticles
def test_8_cuda_particles_sink_log(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13
    lo, hi = pz.DOMAIN_BOX
    sink = mesh.patch_cells("outlet")
    src = (lo, (lo[0] + 0.1 * (hi[0] - lo[0]), hi[1], hi[2]))
    d = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX, recycleInterval=4,
             occupancyInterval=4, sinkCells=sink, sourceBox=src, ageBins=8)
    p = api.CudaParticles(mesh, U, dict(d, sinkLog=100_000))
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
        h.sink_log_enable(100_000)
        step = 0
        while step < 30:                                                     # a launch ends at every recycle point and at every advect's end
            chunk = min(4 - step % 4, 10 - step % 10)
            h.step(dt, 1.5e-5, chunk, L.STEP_FUSE_CYCLES if chunk > 1 else 0)
            step += chunk
            if step % 4 == 0:
                h.sink_apply(); h.respawn_box(src[0], src[1], -1)
                h.occupancy_sample(); h.age_sample()
        assert p.ctx.sink_log_counts() == h.sink_log_counts()                # nobody drained on the way
        want = h.sink_log_read()
        rec, dropped = p.sink_log()
        S.same(rec, want)
        absorbed = p.recycle_counts()["absorbed"]
        assert dropped == 0 and rec.size == absorbed > 0 and (rec["fields"] == 1).all() and rec["apply"].max() == 6
        assert np.isin(rec["cell"], sink).all() and np.array_equal(rec["cycle"], (rec["apply"].astype(np.int64) + 1) * 4)
        assert np.array_equal(np.bincount(_age_bin(rec["age"], 4, 8), minlength=8).astype(np.uint64), p.rtd()[1])
        again, dropped = p.sink_log()                                        # drained: empty until the next absorption
        assert again.size == 0 and dropped == 0
        # the log changes nothing of the run, nor of what age reports
        a, b = p.particles(), q.particles()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and p.recycle_counts() == q.recycle_counts()
        assert np.array_equal(a[1], h.get_particles()[1]) and np.array_equal(_bits(a[0]), _bits(h.get_particles()[0]))
        assert np.array_equal(p.rtd()[1], q.rtd()[1]) and np.array_equal(p.concentration(), q.concentration())
        with pytest.raises(L.CpfError):
            q.sink_log()
    finally:
        p.close(); q.close(); h.close()
