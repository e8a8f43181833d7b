"""GPU: the tracer ledger as it is used -- age, tags, routes, exposure and zones on ONE context-owned cloud, switched on, off and
reset in the middle of a run, with re-sorts, limited respawns and both respawn kinds interleaved (cpf_sink_apply's ladder of
passes, the stamps of cpf_respawn_box / cpf_respawn_source, the lifecycle rules of include/cpf.h) -- against tests/ledger.py, the
numpy model composed of the statements each group is already pinned to.  Random scripts (``ledger.script(seed)``; their coverage is
asserted on the CPU by tests/test_ledger_host.py) run operation by operation on a context and on the model: positions bit for bit,
every table integer for integer, doses bit for bit; a call the header refuses must be refused and change nothing.  Nothing here
tries a step again: the first difference, or the first HIP error, ends the test."""
import os

import numpy as np
import pytest

import ledger as G
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

pytestmark = pytest.mark.gpu
RESPAWNS = ("respawn_box", "respawn_source")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _show(op):
    """an operation in a line: arrays by their shape"""
    if op[0] == "refused":
        return "refused " + _show(op[1])
    args = ["%s%s" % (a.dtype, list(a.shape)) if isinstance(a, np.ndarray) else repr(a) for a in op[1:]]
    return "%s(%s)" % (op[0], ", ".join(args))


class Trail:
    """what every assert of a run says: the seed, the operation's index, the operation, the last few before it"""

    def __init__(self, seed):
        self.seed, self.k, self.ops = seed, -1, []

    def at(self, k, op):
        self.k = k
        self.ops.append(_show(op))

    def __call__(self, what, *more):
        return "seed %s, operation %d %s: %s %s\n  before it: %s" % (self.seed, self.k, self.ops[-1] if self.ops else "", what,
                                                                    " ".join(str(m) for m in more), " | ".join(self.ops[-6:-1]))


def _diff(a, b):
    """where two getter results differ, in a line"""
    if isinstance(a, (tuple, list)):
        return "; ".join("[%d] %s" % (i, _diff(p, q)) for i, (p, q) in enumerate(zip(a, b)) if not G.same(p, q))
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape:
        bad = np.argwhere(_bits(a) != _bits(b)) if a.dtype.kind == "f" else np.argwhere(a.astype(np.int64) != b.astype(np.int64))
        first = [tuple(int(v) for v in i) for i in bad[:4]]
        return "%d differ, first at %s: got %s, want %s" % (len(bad), first, [a[i] for i in first], [b[i] for i in first])
    return "got %r, want %r" % (a, b)


def _refusal(call):
    """the CpfError a call raises, None if it raises none"""
    try:
        call()
    except L.CpfError as e:
        return e
    return None


def _cloud(ctx):
    xyzw, cell = ctx.get_particles()
    return xyzw[:, :3], np.where(cell < 0, -1, cell).astype(np.int32)


def _compare(ctx, m, say, everything, rng):
    """the cloud, the counters and every getter of every group that is on (a random third of them unless `everything`); a group
    that is off in the model answers CPF_ERR_STATE on the device"""
    def wanted():
        return everything or rng.integers(0, 3) == 0
    if wanted():
        xyz, cell = _cloud(ctx)
        want_xyz, want_cell = m.get_particles()
        assert np.array_equal(cell, want_cell), say("cells", _diff(cell, want_cell))
        assert np.array_equal(_bits(xyz), _bits(want_xyz)), say("positions", _diff(xyz, want_xyz))
    names = list(G.COMMON)
    for g in G.GROUPS:
        if m.on[g]:
            names += G.GETTERS[g]
        else:
            e = _refusal(getattr(ctx, G.PROBE[g]))
            assert e is not None and e.status == L.CPF_ERR_STATE, say("%s is off in the model; on the device %s answers" % (g, G.PROBE[g]), e)
    for name in names:
        if wanted():
            got, want = getattr(ctx, name)(), getattr(m, name)()
            assert G.same(got, want), say(name, _diff(got, want))


def _readable(ctx, m):
    """every table the context can still read, for a before / after comparison around a refused call"""
    out = dict(cloud=_cloud(ctx))
    for name in list(G.COMMON) + [n for g in G.GROUPS if m.on[g] for n in G.GETTERS[g]]:
        out[name] = getattr(ctx, name)()
    return out


def _run_script(seed, ctx, m, ops, check_rng):
    say, spans = Trail(seed), G.Spans()
    for k, op in enumerate(ops):
        say.at(k, op)
        if op[0] == "refused":
            e = _refusal(lambda: G.apply(m, op[1]))
            assert isinstance(e, G.StateError), say("the model does not refuse it:", e)
            before = _readable(ctx, m)
            e = _refusal(lambda: G.apply(ctx, op[1]))
            assert e is not None and e.status == L.CPF_ERR_STATE, say("the device must refuse it for the state; it answers", e)
            after = _readable(ctx, m)
            for name in before:
                assert G.same(before[name], after[name]), say("a refused call changed", name, _diff(after[name], before[name]))
            _compare(ctx, m, say, False, check_rng)
            continue
        if op[0] == "zone_sample":
            flow0 = ctx.zone_flows()[0]
        if op[0] == "age_sample":
            field0 = ctx.age_field()
        if op[0] in RESPAWNS and m.needs_readback(op[-1]):
            # a limited respawn on a re-sorted cloud: WHICH dead ids it took is the array order's; their number is exact, all of
            # them were dead, and the model goes on from that set (tests/test_gpu_recycle.py, test_6, does the same)
            dead, (xyz0, _) = m.dead_ids(), m.get_particles()
            G.apply(ctx, op)
            xyz, cell = _cloud(ctx)
            moved = np.nonzero((_bits(xyz) != _bits(xyz0)).any(1))[0]
            assert moved.size == min(op[-1], dead.size) and np.isin(moved, dead).all(), say(
                "a limited respawn took", moved.size, "ids, of them dead before:", int(np.isin(moved, dead).sum()), "; dead", dead.size)
            G.apply(m, op, chosen=moved)
        else:
            G.apply(ctx, op)
            G.apply(m, op)
        if op[0] in G.Spans.START:
            spans.note(op, ctx.recycle_counts()["absorbed"])
        if op[0] == "zone_sample":
            assert G.zone_sample_identity(flow0, ctx.zone_flows()[0], _cloud(ctx)[1]), say("a zone sample does not add one count per live particle")
        if op[0] == "age_sample":
            assert G.age_sample_identity(field0, ctx.age_field(), ctx.ages()), say("an age sample does not add the ages of the live")
        _compare(ctx, m, say, op[0] == "sink_apply" or op[0] in RESPAWNS, check_rng)
    say.at(len(ops), ("end of the script",))
    _compare(ctx, m, say, True, check_rng)
    bad = G.conservation(ctx, spans)                                         # on the device's own numbers
    assert bad == [], say("conservation", bad)
    return spans


@pytest.mark.parametrize("seed", range(int(os.environ.get("CPF_FUZZ_LEDGER", "8"))))    # (a longer campaign: CPF_FUZZ_LEDGER=200)
def test_random_scripts_on_the_whole_ledger(seed, gpu_ctx_factory, oracle_libs):
    s = G.script(seed)
    m = G.start(s)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", s["sort_interval"])
    ctx.set_mesh(s["mesh"]); ctx.set_velocity(s["U"]); ctx.set_seed(s["cloud_seed"])
    assert (int(ctx.mesh_quality()["n_derived"]) > s["mesh"].n_cells) == s["warped"] == m.w.warped
    _run_script(seed, ctx, m, s["setup"] + s["ops"], np.random.default_rng(50 + seed))
    k = ctx.recycle_counts()
    assert k["absorbed"] == m.absorbed >= 0.05 * s["n"] and k["epochs"] == m.epoch


# ------------------------------------------------------------------------------------------------ the driver, every key at once
def test_cuda_particles_with_every_ledger_key_is_the_model(oracle_libs):
    """``CudaParticles`` on the channel of tests/test_gpu_recycle.py::test_8 at D = 0 with recycling, a source box that sticks out
    of the mesh (one draw in five stays dead and is drawn again -- the driver has no key for a limited count, this is the limit it
    can be given), age, sink groups (the box has origin 0, the only one the driver's keys give it), routes, exposure, zones and
    occupancy, at intervals 4, 3, 2 and 5: a launch ends at every kind of point.  ``advect``'s documented order -- accumulate, zone
    sample, sink and respawn, then the occupancy point's samples -- replayed on the model; every result compared after each call."""
    from cudaparticlesfoam_amd.cases import box_mesh
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    import exposure as X
    import zones as Z
    mesh = box_mesh(12, 3, 3)
    rng = np.random.default_rng(5)
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.3 + np.array([2.0, 0.0, 0.0])
    n, dt = 6007, 2.0 ** -2                                                   # 10 * dt / dt == 10 exactly; half a cell per cycle
    xyz = pz.uniform_points(12, n, (0.0, 0.0, 0.0), (12.0, 3.0, 3.0))
    sink = G._last_x_layer(mesh)
    groups = (np.arange(sink.size) % 3).astype(np.int32)
    box = ((-0.25, 0.0, 0.0), (1.0, 3.0, 3.0))
    rate, zone_of = X.run_rate(mesh), Z.x_slabs(mesh, 4)
    every = dict(recycle=4, exposure=3, zone=2, occupancy=5)
    d = dict(numParticles=n, dt=dt, saveInterval=10, diffusionCoeff=0.0, seedingBox=((0.0, 0.0, 0.0), (12.0, 3.0, 3.0)),
             recycleInterval=every["recycle"], sinkCells=sink, sourceBox=box, ageBins=6, sinkGroups=groups, routeStats=True,
             exposureField=rate, exposureInterval=every["exposure"], doseBins=8, doseBinWidth=0.5, zoneMap=zone_of,
             zoneInterval=every["zone"], occupancyInterval=every["occupancy"])
    p = api.CudaParticles(mesh, U, d, positions=xyz)
    try:
        m = G.Ledger(mesh, U, 1591593751)                                    # the seed and the sort cadence a context starts with
        for op in [("set_sink_cells", sink), ("set_particles", xyz), ("locate_initial",), ("sort_by_cell",), ("age_enable", 4, 6),
                   ("tag_enable", 1, 3), ("set_sink_groups", sink, groups), ("route_enable",), ("exposure_enable", 0.5, 8),
                   ("set_exposure_field", rate), ("zone_enable", 4), ("set_zone_map", zone_of)]:
            G.apply(m, op)
        say, check_rng = Trail("driver"), np.random.default_rng(1)
        step, pending, launches = 0, 0.0, set()
        for call in range(3):
            assert p.advect(call * 10 * dt, 10 * dt) == 10
            done = 0
            while done < 10:
                chunk = min([10 - done] + [i - step % i for i in every.values()])
                launches.add(chunk)
                m.step(dt, 0.0, chunk, G.FUSE if chunk > 1 else 0)
                step += chunk; done += chunk
                pending += dt * chunk
                if step % every["exposure"] == 0:
                    m.exposure_accumulate(pending)
                    pending = 0.0
                if step % every["zone"] == 0:
                    m.zone_sample()
                if step % every["recycle"] == 0:
                    m.sink_apply(); m.respawn_box(box[0], box[1], -1)
                if step % every["occupancy"] == 0:
                    m.occupancy_sample(); m.age_sample(); m.tag_sample(); m.route_sample()
            say.at(call, ("advect", call))
            assert p.step == step
            _compare(p.ctx, m, say, True, check_rng)
            # ... and what the driver's own methods hand out is those tables
            assert G.same(p.particles()[1], p.ctx.get_particles()[1]) and p.recycle_counts() == m.recycle_counts()
            assert G.same(p.rtd()[1], m.age_histogram()) and G.same(p.transfer(), m.transfer())
            assert G.same(p.rtd_by_route()[1], m.route_histogram()) and G.same(p.dose_distribution()[1], m.dose_histogram())
            assert G.same(p.doses(), m.doses()) and G.same(p.zone_flows(), m.zone_flows())
        assert launches == {1, 2}                                            # the points cut every launch to one or two cycles
        k = p.recycle_counts()
        assert k["absorbed"] > n // 4 and k["drawn"] > k["placed"] > 0 and m.respawns.max() >= 1
        assert int(m.dose_histogram().sum()) == int(m.route_histogram().sum()) == int(m.zone_flows()[0][:, -1].sum()) == k["absorbed"]
    finally:
        p.close()
