"""No GPU.  tests/ledger.py, the numpy model of the whole tracer ledger, against what is already pinned: replayed through ``Ledger``
with one group (or the groups a run needs) on, the recycled runs "graded box" and "thin box" of tests/recycle.py give exactly what
the cached CPU runs of tests/age.py, tags.py, routes.py and exposure.py give, and the books tests/test_gpu_zones.py keeps; integers
as integers, doses and positions bit for bit.  Then the script generator: every default seed, run on the model alone, satisfies the
coverage conditions the GPU fuzz (tests/test_gpu_ledger_fuzz.py) relies on.  These are conditions on the inputs."""
import numpy as np
import pytest

import age as A
import exposure as X
import ledger as G
import recycle as R
import routes as RT
import tags as T
import zones as Z
from cudaparticlesfoam_amd import _lib as L

NAMES = ["graded box", "thin box"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _seated(name):
    r = R.run(name)
    m = G.Ledger(r.mesh, r.U, R.SEED, sort_interval=r.sort_interval)
    m.set_particles(r.xyz)
    assert m.locate_initial() == 0
    m.set_sink_cells(r.sink_cells)
    return r, m


def _same_cloud(m, xyz, cell):
    got_xyz, got_cell = m.get_particles()
    assert np.array_equal(_bits(got_xyz), _bits(xyz))
    assert np.array_equal(got_cell, np.where(np.asarray(cell) < 0, -1, cell))


def _limit(m, name, epoch, table):
    """the limited round of a run: the first half of the dead, in id order (the run has not re-sorted)"""
    if epoch != table[name]:
        return -1
    assert m.id_order
    return m.dead_ids().size // 2


# ------------------------------------------------------------------------------------------------ 1. the model alone is the statements
@pytest.mark.parametrize("name", NAMES)
def test_1_age_replayed_is_the_cached_cpu_run(name):
    r, m = _seated(name)
    want = A.cpu(name)
    m.age_enable(A.BIN_CYCLES, A.N_BINS)
    for epoch in range(r.rounds):
        m.step(r.dt, 0.0, r.cycles)
        m.sink_apply()
        m.respawn_box(r.box[0], r.box[1], _limit(m, name, epoch, A.LIMITED_ROUND))
        if epoch == A.LIMITED_ROUND[name]:
            assert np.array_equal(m.ages(), want["mid_ages"]) and (m.ages() < 0).sum() > 0
            assert np.array_equal(m.dead_ids(), want["left_dead"])
    _same_cloud(m, want["xyz"], want["cell"])
    assert m.recycle_counts() == dict(absorbed=want["absorbed"], drawn=want["drawn"], placed=want["placed"], epochs=r.rounds)
    assert np.array_equal(m.age_births(), want["births"]) and np.array_equal(m.age_histogram(), want["hist"])
    assert np.array_equal(m.ages(), want["ages"]) and m.now == want["now"]
    assert int(m.age_histogram().sum()) == want["absorbed"] > 0


def _tagged(name):
    r, m = _seated(name)
    t = T.run(name)
    b = t.base
    m.set_source_triangles(b.tri, b.weights, b.depth)
    return r, m, t


@pytest.mark.parametrize("name", NAMES)
def test_1_tags_replayed_is_the_cached_cpu_run(name):
    r, m, t = _tagged(name)
    want = T.cpu(name)
    m.tag_enable(T.N_ORIGINS, T.N_SINKS)
    m.set_sink_groups(r.sink_cells, t.groups)
    m.set_source_origins(t.origin_of_triangle)
    for _ in range(r.rounds):
        m.step(r.dt, 0.0, r.cycles)
        m.sink_apply()
        m.respawn_source(-1)
        m.tag_sample(); m.occupancy_sample()
    _same_cloud(m, want["xyz"], want["cell"])
    assert m.recycle_counts() == dict(absorbed=want["absorbed"], drawn=want["drawn"], placed=want["placed"], epochs=r.rounds)
    assert np.array_equal(m.tag_origins(), want["origin"]) and np.array_equal(m.transfer(), want["transfer"])
    assert G.same(m.tag_field(), (want["field"], want["samples"])) and G.same(m.occupancy(), (want["occupancy"], want["samples"]))
    assert int(m.transfer().sum()) == want["absorbed"] > 0 and (m.transfer()[1:] > 0).any()


@pytest.mark.parametrize("name", NAMES)
def test_1_routes_replayed_is_the_cached_cpu_run_at_every_recycle_point(name):
    r, m, t = _tagged(name)
    want = RT.cpu(name)
    m.age_enable(RT.BIN_CYCLES, RT.N_BINS)
    m.tag_enable(T.N_ORIGINS, T.N_SINKS)
    m.set_sink_groups(r.sink_cells, t.groups)
    m.set_source_origins(t.origin_of_triangle)
    m.route_enable()
    for epoch in range(r.rounds):
        m.step(r.dt, 0.0, r.cycles)
        m.sink_apply()
        m.respawn_source(_limit(m, name, epoch, RT.LIMITED_ROUND))
        m.route_sample()
        w = want["rounds"][epoch]
        assert np.array_equal(m.route_histogram(), w["hist"]), (name, epoch)
        assert G.same(m.route_field(), (w["field_sum"], w["field_count"], epoch + 1)), (name, epoch)
    _same_cloud(m, want["xyz"], want["cell"])
    assert m.recycle_counts() == dict(absorbed=want["absorbed"], drawn=want["drawn"], placed=want["placed"], epochs=r.rounds)
    assert np.array_equal(m.tag_origins(), want["origin"]) and np.array_equal(m.age_births(), want["births"])
    # the one pass adds what the two passes add
    assert np.array_equal(m.route_histogram().sum(2), m.transfer()) and np.array_equal(m.route_histogram().sum((0, 1)), m.age_histogram())
    assert int(m.route_histogram().sum()) == want["absorbed"] > 0


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_1_exposure_replayed_is_the_cached_cpu_run_at_every_recycle_point(name, interval):
    r, m = _seated(name)
    want = X.cpu(name, interval)
    m.exposure_enable(X.BIN_WIDTH, X.N_BINS)
    m.set_exposure_field(X.run_rate(r.mesh))
    assert (X.run_rate(r.mesh) == 0.0).any()
    pending = 0.0
    for epoch in range(r.rounds):
        for k in range(r.cycles):
            m.step(r.dt, 0.0, 1)
            pending += r.dt * 1
            if (k + 1) % interval == 0:
                m.exposure_accumulate(pending)
                pending = 0.0
        m.sink_apply()
        m.respawn_box(r.box[0], r.box[1], -1)
        w = want["points"][epoch]
        assert np.array_equal(_bits(m.exposure_doses()), _bits(w["dose"])), (name, epoch)
        assert np.array_equal(_bits(m.doses()), _bits(w["doses"])) and np.array_equal(m.dose_histogram(), w["hist"]), (name, epoch)
        assert np.array_equal(m.get_particles()[1], np.where(w["cell"] < 0, -1, w["cell"]))
    _same_cloud(m, want["xyz"], want["cell"])
    assert m.recycle_counts()["absorbed"] == want["absorbed"] == int(m.dose_histogram().sum()) > 0


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_1_zones_replayed_keep_the_books_of_the_gpu_test(name, interval):
    """the books of tests/test_gpu_zones.py::test_7: Z.sample at every zone point, Z.leave and Z.stamp at every recycle point, kept
    here over the cells of a twin model with zones off"""
    r, m = _seated(name)
    _, twin = _seated(name)
    n_zones = 4
    zone_of = Z.x_slabs(r.mesh, n_zones)
    m.zone_enable(n_zones); m.set_zone_map(zone_of)
    flow, last, samples = Z.table(n_zones), np.full(m.n, Z.OUTSIDE, np.uint8), 0
    for epoch in range(r.rounds):
        for j in range(r.cycles):
            m.step(r.dt, 0.0, 1); twin.step(r.dt, 0.0, 1)
            if (j + 1) % interval == 0:
                m.zone_sample(); m.occupancy_sample()
                flow, last = Z.sample(flow, last, twin.get_particles()[1], zone_of, n_zones)
                samples += 1
        cell = twin.get_particles()[1]
        flow = Z.leave(flow, last, cell, r.sink_cells, n_zones)
        last = Z.stamp(last, R.sink(cell, r.sink_cells))
        m.sink_apply(); twin.sink_apply()
        m.respawn_box(r.box[0], r.box[1]); twin.respawn_box(r.box[0], r.box[1])
        assert G.same(m.zone_flows(), (flow, samples)) and np.array_equal(m.zone_last(), last), (name, epoch)
        got = m.zone_flows()[0].astype(np.int64)
        per_zone = np.bincount(zone_of, weights=m.occupancy()[0].astype(np.float64), minlength=n_zones).astype(np.int64)
        assert np.array_equal(got[:, :n_zones].sum(axis=0), per_zone)
    assert G.same(m.get_particles(), twin.get_particles()) and m.recycle_counts() == twin.recycle_counts()
    assert int(flow[:, n_zones].sum()) == m.recycle_counts()["absorbed"] >= 200


# ------------------------------------------------------------------------------------------------ 2. the script generator
SEEDS = list(range(G.SEEDS))


def _sinks(m):
    return [e for e in m.log if e["kind"] == "sink"]


def _respawns(m):
    return [e for e in m.log if e["kind"] == "respawn"]


@pytest.mark.parametrize("seed", SEEDS)
def test_2_every_default_script_meets_its_own_conditions(seed):
    s, m, states = G.dry_run(seed)
    assert 10 <= len(s["ops"]) <= 25 and 1 <= s["n"] <= 12_000
    assert m.absorbed >= 0.05 * s["n"], (seed, m.absorbed)                   # at least 5 % of the cloud is absorbed
    assert m.respawns.max() >= 2, seed                                       # somebody is respawned twice
    # every rung of the ladder the cloud is ever stepped under meets a sink that absorbs somebody
    allowed = set().union(*[rungs for op, _, rungs, _ in states if op[0] == "step"])
    met = set().union(*[e["rungs"] for e in _sinks(m) if e["absorbed"] > 0])
    print("seed %d: n %d, %d cells, %d + %d operations, absorbed %d, rungs %s" % (seed, s["n"], s["mesh"].n_cells, len(s["setup"]),
                                                                                 len(s["ops"]), m.absorbed, sorted(met)))
    assert allowed <= met, (seed, sorted(allowed - met))
    assert (s["rate"] == 0.0).any() and (s["rate"] > 0.0).any()              # a rate field with zero cells
    # the script is the same list every time it is asked for, and runs to the same model
    again = G.start(s)
    G.run(again, s["setup"] + s["ops"])
    assert G.same(again.get_particles(), m.get_particles()) and again.recycle_counts() == m.recycle_counts()
    # ... and its getters obey the identities that need no model
    spans, probe = G.Spans(), G.start(s)
    for op in s["setup"] + s["ops"]:
        if op[0] != "refused":
            G.apply(probe, op)
            spans.note(op, probe.recycle_counts()["absorbed"])
    assert G.conservation(probe, spans) == []


def test_2_the_default_set_covers_every_path_the_issue_names():
    runs = [G.dry_run(seed) for seed in SEEDS]
    sinks = [(s, e) for s, m, _ in runs for e in _sinks(m) if e["absorbed"] > 0]
    assert any(all(e["on"].values()) for _, e in sinks)                                        # all five groups on
    assert any(e["on"]["route"] and not e["on"]["exposure"] for _, e in sinks)                 # routes on, exposure off
    # exposure enabled while tagging was off (1 x 1 x nBins) meets a sink; tags come on, the dose calls are refused, a sink again
    found = False
    for s, m, states in runs:
        ops = [st[0] for st in states]
        for k, (op, on, _, _) in enumerate(states):
            if op[0] == "tag_enable" and on["exposure"] and not on["tag"]:
                before = [e for e in _sinks(m) if e["dose_shape"] == (1, 1) and e["absorbed"] > 0]
                refused = [o[1][0] for o in ops[k:] if o[0] == "refused"]
                later = any(o[0] == "sink_apply" for o in ops[k:])
                found = found or (bool(before) and "exposure_accumulate" in refused and "exposure_reset" in refused and later)
    assert found
    # a plain sink set while tags and routes are on, then a sink: everybody lands in group 0 (the groups were spread before)
    found = False
    for s, m, states in runs:
        for k, (op, on, _, _) in enumerate(states):
            if op[0] == "set_sink_cells" and on["tag"] and on["route"]:
                nxt = [o[0] for o, *_ in states[k + 1:]]
                found = found or ("sink_apply" in nxt and "set_sink_groups" not in nxt[:nxt.index("sink_apply")])
    assert found
    assert any(e["groups_seen"] == [0] and e["on"]["route"] for _, e in sinks) and any(len(e["groups_seen"]) > 1 for _, e in sinks)
    rs = [e for _, m, _ in runs for e in _respawns(m)]
    limited = [e for e in rs if 0 < e["max_count"] < e["dead"]]
    assert any(e["id_order"] for e in limited) and any(not e["id_order"] for e in limited)    # in id order, and after a re-sort
    assert any(e["who"] == "cpf_respawn_source" for e in limited) and any(e["who"] == "cpf_respawn_box" for e in limited)
    found = False                                                            # a limited box respawn, then the source places the rest
    for _, m, _ in runs:
        r = _respawns(m)
        for a, b in zip(r, r[1:]):
            found = found or (a["who"] == "cpf_respawn_box" and 0 < a["max_count"] < a["dead"] and b["who"] == "cpf_respawn_source"
                              and b["max_count"] < 0 and b["dead"] == a["dead"] - a["max_count"] and b["taken"] == b["dead"])
    assert found
    assert any(e["max_count"] > e["dead"] > 0 for e in rs)                                    # more asked for than are dead
    assert any(e["dead"] == 0 and e["max_count"] != 0 for e in rs)                            # nobody is dead
    # a reseat in the middle of a run: a call of every group is refused behind it, until the group is enabled again
    found = False
    for s, m, states in runs:
        ops = [st[0] for st in states[len(s["setup"]):]]
        for k, op in enumerate(ops):
            if op[0] == "set_particles" and k > 0:
                refused = {o[1][0] for o in ops[k:] if o[0] == "refused"}
                found = found or ({"age_reset", "set_box_origin", "route_enable", "set_exposure_field", "set_zone_map"} <= refused
                                  and any(o[0] == "age_enable" for o in ops[k:]))
    assert found
    for reset in ("age_reset", "tag_reset", "route_reset", "exposure_reset", "zone_reset"):   # each between two sinks
        found = False
        for s, m, states in runs:
            names = [st[0][0] for st in states]
            for k, nm in enumerate(names):
                found = found or (nm == reset and "sink_apply" in names[:k] and "sink_apply" in names[k:])
        assert found, reset
    warped = [s for s, m, _ in runs if s["warped"] and any(op[0] == "set_zone_map" for op in s["setup"] + s["ops"])]
    assert warped and all(G.start(s).w.warped and G.start(s).w.parent_of.size > s["mesh"].n_cells for s in warped)
    assert any(s["thin"] for s, _, _ in runs)
    sizes = {s["n"] for s, _, _ in runs}
    assert {1, 4095, 4097} <= sizes and any(n % 64 and n % 256 and n % 4096 and n > 4097 for n in sizes)
    intervals = {op[2] for s, _, _ in runs for op in s["ops"] if op[:2] == ("set_option", "sort_interval")} | {s["sort_interval"] for s, _, _ in runs}
    methods = {op[2] for s, _, _ in runs for op in s["ops"] if op[:2] == ("set_option", "sort_method")}
    assert {0, 1, 3, 7} <= intervals and methods == {0, 2} and any(op[0] == "sort_by_cell" for s, _, _ in runs for op in s["ops"])


# ------------------------------------------------------------------------------------------------ 3. bad calls in the model
@pytest.mark.parametrize("bad", [("age_sample",), ("tag_reset",), ("set_sink_groups", [0], [0]), ("route_enable",), ("route_sample",),
                                 ("exposure_accumulate", 1.0), ("set_exposure_field", None), ("zone_sample",), ("set_zone_map", None),
                                 ("respawn_source", -1), ("age_histogram",), ("zone_flows",)])
def test_3_a_call_of_a_group_that_is_off_raises_at_its_operation(bad):
    s = G.script(0)
    m = G.start(s)
    ops = [("set_particles", s["xyz"]), ("locate_initial",), ("set_sink_cells", s["sink"]), ("step", 0.1, 0.0, 1, 0), bad, ("sink_apply",)]
    with pytest.raises(G.StateError) as e:
        G.run(m, ops)
    assert e.value.index == 4 and e.value.status == L.CPF_ERR_STATE and isinstance(e.value, L.CpfError) and "operation 4" in str(e.value)
    assert m.recycle_counts()["absorbed"] == 0                               # (the run stopped there)


def test_3_before_the_cloud_is_located_every_entry_is_refused():
    s = G.script(0)
    m = G.start(s)
    m.set_particles(s["xyz"])
    for op in (("age_enable", 1, 4), ("tag_enable", 2, 2), ("exposure_enable", 0.5, 4), ("zone_enable", 3), ("sink_apply",),
               ("respawn_box", (0, 0, 0), (1, 1, 1), -1), ("step", 0.1, 0.0, 1, 0), ("occupancy_sample",), ("sort_by_cell",)):
        with pytest.raises(G.StateError):
            G.apply(m, op)
    with pytest.raises(AssertionError):                                      # a script that expects a refusal the model does not give
        G.run(m, [("locate_initial",), ("refused", ("age_enable", 1, 4))])
