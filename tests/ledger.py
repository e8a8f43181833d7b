"""TEST INFRASTRUCTURE ONLY.  The whole tracer ledger of one context-owned cloud (include/cpf.h: "recycling", "patch source", "tracer
age", "tracer tags", "routes", "exposure", "zones", "per-cell occupancy") as ONE numpy model, everything in particle-id order.

``Ledger`` has one method per public ``Context`` call that touches the ledger, with the binding's name and arguments, and one getter
per getter of the binding, so that a test runs the same list of operations on both and compares getter by getter.  Every rule of a
group is the statement its own module already exports (``age.ages / rtd / field``, ``tags.transfer / field / picks /
origin_of_kept``, ``routes.hist / field``, ``exposure.accumulate / histogram``, ``zones.sample / leave / stamp``, ``recycle.sink /
positions / brute_locate``, ``sourcepatch.table / positions``); the model adds only the glue that had no statement yet: which group
is on, what turns it off, in which order a sink or a respawn applies the groups, and that a call does nothing to the tables of a
group that is off.  The lifecycle rules are the comments of include/cpf.h.  A call the header answers with CPF_ERR_STATE raises
``StateError`` -- a ``CpfError`` of that status, as the binding raises.

``script(seed)`` generates one fuzz case (mesh, fields, sink, source, maps and the list of operations); ``Spans`` and
``conservation`` state identities between the getters that need no model.  Shared by tests/test_ledger_host.py (no GPU) and
tests/test_gpu_ledger_fuzz.py."""
from __future__ import annotations

import functools

import numpy as np

import age as A
import exposure as X
import recycle as R
import routes as RT
import sourcepatch as SP
import tags as T
import warped as W
import zones as Z
from cudaparticlesfoam_amd import _lib as L

GROUPS = ("age", "tag", "route", "exposure", "zone")
FUSE = 4                                     # CPF_STEP_FUSE_CYCLES: the same bits in one launch


class StateError(L.CpfError):
    """what the binding raises for CPF_ERR_STATE; ``index`` is the operation's index in a script (``run``), else None"""

    def __init__(self, message, index=None):
        super().__init__(L.CPF_ERR_STATE, message if index is None else "operation %d: %s" % (index, message))
        self.index = index


class Walk:
    """what the model needs of a mesh: the oracle's tables of the mesh the walk runs on (the derived mesh where cells are warped),
    the parent of every derived cell, and the initial-locate rule"""

    def __init__(self, mesh):
        self.mesh = mesh
        self.cw = R.cellwalk()
        st = W.quality(mesh, L.NONPLANAR_TOL)["state"]
        self.warped = bool((st == 2).any())
        if self.warped:
            assert (st != 1).all()
            derived, first, _ = W.derived_mesh(mesh, st, mesh.cell_centres_volumes()[0])
            self.parent_of = W.parent_of(first)
        else:
            derived, self.parent_of = mesh, np.arange(mesh.n_cells, dtype=np.int32)
        self.t = self.cw.build(derived)
        self.tables = (self.t.cell_off, self.t.planes, self.t.nbr)
        self.n_cells = mesh.n_cells

    def locate(self, xyz):
        """cells of the WALK's mesh.  Axis-aligned boxes: ``recycle.brute_locate`` (every plane distance one rounding).  Warped
        cells: the oracle's initial locate, whose dot product is the kernel's chain of fused operations."""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        if not self.warped:
            return R.brute_locate(xyz, self.tables)
        x, y, z = (np.ascontiguousarray(xyz[:, k]) for k in range(3))
        return self.cw.locate_initial(x, y, z, self.t, nthreads=self.cw.max_threads)

    def parents(self, cell):
        cell = np.asarray(cell)
        return np.where(cell >= 0, self.parent_of[np.maximum(cell, 0)], -1).astype(np.int32)


_WALKS = {}


def _walk_of(mesh):
    """one ``Walk`` per mesh object (a PolyMesh does not hash; the entry keeps the mesh alive, so its id stays its own)"""
    if id(mesh) not in _WALKS:
        _WALKS[id(mesh)] = Walk(mesh)
    return _WALKS[id(mesh)]


class Ledger:
    def __init__(self, mesh, U, seed, sort_interval=50):
        self.w = _walk_of(mesh)
        self.nc = mesh.n_cells
        self.U = np.ascontiguousarray(np.asarray(U, np.float64)[self.w.parent_of])
        self.seed = int(seed)
        self.now = 0                          # ctx->stepCounter
        self.sort_interval, self.last_sort = int(sort_interval), 0
        self.n = 0
        self.located = False
        self.id_order = True                  # array order is id order: never sorted since the cloud was seated
        self.epoch = 0
        self.absorbed = self.drawn = self.placed = 0
        self.sink_cells = np.empty(0, np.int32)
        self.source = None                    # (rec, hi, n triangles)
        self.origin_of_triangle = None
        self.occ, self.occ_samples = np.zeros(self.nc, np.uint64), 0
        self.on = dict.fromkeys(GROUPS, False)
        self.respawns = None                  # per id: how often it was placed
        self.log = []                         # what the coverage conditions of a script are read from

    # ------------------------------------------------------------------------------------------------ helpers
    def _need(self, cond, what):
        if not cond:
            raise StateError(what)

    def _need_cloud(self, who):
        self._need(self.n > 0 and self.located, who + ": no located particles")

    def _need_on(self, group, who):
        self._need(self.on[group], "%s: %s is off" % (who, group))

    def parents(self):
        return self.w.parents(self.cell)

    def _ages(self):
        return A.ages(self.now, self.birth)

    def _group_of_cell(self):
        return self.group_of_cell if self.on["tag"] else np.zeros(self.nc, np.int64)

    def _off(self, *groups):
        for g in groups:
            self.on[g] = False

    def rungs(self):
        """the passes cpf_sink_apply runs in the present state"""
        r = set()
        if self.on["exposure"]:
            r.add("dose")
        if self.on["zone"]:
            r.add("leave")
        if self.on["route"]:
            r.add("route")
        else:
            if self.on["tag"]:
                r.add("transfer")
            r.add("age_absorb" if self.on["age"] else "plain")
        return r

    # ------------------------------------------------------------------------------------------------ the cloud
    def set_option(self, key, value):
        if key == "sort_interval":
            self.sort_interval = int(value)

    def set_particles(self, xyz, cell=None):
        assert cell is None
        xyz = np.ascontiguousarray(xyz, np.float64)
        self.n = xyz.shape[0]
        self.x, self.y, self.z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
        self.cell = np.full(self.n, -1, np.int32)
        self.located, self.id_order, self.epoch = False, True, 0
        self._off(*GROUPS)                    # the tables by id were the old cloud's
        self.respawns = np.zeros(self.n, np.int64)

    def locate_initial(self):
        self._need(self.n > 0, "cpf_locate_initial: no particles")
        self.cell = self.w.locate(np.stack([self.x, self.y, self.z], 1)).astype(np.int32)
        self.located = True
        return int((self.cell < 0).sum())

    def step(self, dt, D=0.0, n_cycles=1, flags=0):
        self._need_cloud("cpf_step")
        assert D == 0.0 and not (dt == 0.0) and flags in (0, FUSE)
        cw = self.w.cw
        cw.step_given(self.x, self.y, self.z, self.cell, dt, n_cycles, self.w.t, self.U, 0.0, None, nthreads=cw.max_threads)
        self.now += n_cycles
        if self.sort_interval > 0 and self.now - self.last_sort >= self.sort_interval:
            self._sorted()
            self.last_sort = self.now

    def _sorted(self):
        if self.n > 1:                        # (a cloud of one is not reordered)
            self.id_order = False

    def sort_by_cell(self):
        self._need_cloud("cpf_sort_by_cell")
        self._sorted()

    def get_particles(self):
        """(xyz [n][3], parent cell [n] with every negative code as -1)"""
        return np.stack([self.x, self.y, self.z], 1), self.parents()

    # ------------------------------------------------------------------------------------------------ occupancy
    def occupancy_sample(self):
        self._need_cloud("cpf_occupancy_sample")
        p = self.parents()
        self.occ = self.occ + np.bincount(p[p >= 0], minlength=self.nc).astype(np.uint64)
        self.occ_samples += 1

    def occupancy(self):
        return self.occ.copy(), self.occ_samples

    # ------------------------------------------------------------------------------------------------ sink and source
    def set_sink_cells(self, cells):
        self.sink_cells = np.asarray(cells, np.int32).reshape(-1).copy()
        if self.on["tag"]:
            self.group_of_cell = np.zeros(self.nc, np.int64)      # a plain sink set: everybody in group 0

    def set_sink_groups(self, cells, groups):
        self._need_on("tag", "cpf_set_sink_groups")
        self.set_sink_cells(cells)
        self.group_of_cell = T.group_of_cell(self.nc, self.sink_cells, groups) if self.sink_cells.size else np.zeros(self.nc, np.int64)

    def set_box_origin(self, origin):
        self._need_on("tag", "cpf_set_box_origin")
        self.box_origin = int(origin)

    def set_source_triangles(self, tri, weights=None, depth=(0.0, 0.0)):
        tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
        if tri.shape[0] == 0:
            self.source, self.origin_of_triangle = None, None
            return
        rec, hi = SP.table(tri, weights, depth, exact=False)
        self.source = (rec, hi, tri.shape[0])
        self.origin_of_triangle = np.zeros(tri.shape[0], np.int64)     # a new source: every triangle in origin 0

    def set_source_origins(self, origin_of_triangle):
        self._need_on("tag", "cpf_set_source_origins")
        self._need(self.source is not None, "cpf_set_source_origins: no source")
        o = np.asarray(origin_of_triangle, np.int64).reshape(-1)
        assert o.size >= self.source[2]
        self.origin_of_triangle = o.copy()

    def sink_apply(self):
        self._need_cloud("cpf_sink_apply")
        if self.sink_cells.size == 0:
            return
        p = self.parents()
        after = R.sink(p, self.sink_cells)
        hit = after != p
        rungs = self.rungs()
        if self.on["exposure"]:                                   # the dose pass, before anyone is marked
            tagged = self.dose_tagged                             # (tagging is then still on: its going off turns exposure off)
            self.dose_hist = self.dose_hist + X.histogram(
                p, self.sink_cells, self.dose, self.bin_width, self.dose_bins, self.origin if tagged else None,
                self._group_of_cell() if tagged else None, *self.dose_shape)
        if self.on["zone"]:                                       # the leave pass
            self.flow = Z.leave(self.flow, self.last, p, self.sink_cells, self.n_zones)
        if self.on["route"]:                                      # one pass for the three tables
            age = self._ages()
            self.route_hist = self.route_hist + RT.hist(self.origin, self.group_of_cell, p, hit, age, self.bin_cycles, self.age_bins,
                                                        self.n_origins, self.n_sinks)
            self.age_hist = self.age_hist + A.rtd(age[hit], self.bin_cycles, self.age_bins)
            self.transfer_m = self.transfer_m + T.transfer(self.origin, self.group_of_cell, p, hit, self.n_origins, self.n_sinks)
        else:
            if self.on["tag"]:
                self.transfer_m = self.transfer_m + T.transfer(self.origin, self.group_of_cell, p, hit, self.n_origins, self.n_sinks)
            if self.on["age"]:
                self.age_hist = self.age_hist + A.rtd(self._ages()[hit], self.bin_cycles, self.age_bins)
        self.absorbed += int(hit.sum())
        self.cell[hit] = -1
        self.log.append(dict(kind="sink", rungs=rungs, absorbed=int(hit.sum()), on=dict(self.on),
                             dose_shape=self.dose_shape if self.on["exposure"] else None,
                             groups_seen=np.unique(self._group_of_cell()[p[hit]]).tolist() if hit.any() else []))

    def dead_ids(self):
        return np.nonzero(self.cell < 0)[0]

    def needs_readback(self, max_count):
        """a limited respawn on a re-sorted cloud: WHICH dead ids it takes is the array order's, which the model does not carry"""
        return (not self.id_order) and 0 < max_count < self.dead_ids().size

    def _respawn(self, who, max_count, origin_of, positions_of, chosen):
        self._need_cloud(who)
        dead = self.dead_ids()
        entry = dict(kind="respawn", who=who, dead=int(dead.size), max_count=int(max_count), id_order=self.id_order, taken=0)
        if max_count != 0:
            # every candidate is stamped, the ones this call leaves dead included
            if self.on["age"]:
                self.birth[dead] = self.now
            if self.on["tag"]:
                self.origin[dead] = origin_of(dead)
            if self.on["exposure"]:
                self.dose[dead] = 0.0
            if self.on["zone"]:
                self.last = Z.stamp(self.last, self.cell)
            take = dead if max_count < 0 else dead[:max_count]
            if self.needs_readback(max_count) and chosen is not None:
                chosen = np.sort(np.asarray(chosen, np.int64))
                assert chosen.size == min(max_count, dead.size) and np.isin(chosen, dead).all(), (chosen.size, max_count, dead.size)
                take = chosen
            pos = positions_of(take)
            where = self.w.locate(pos)
            self.x[take], self.y[take], self.z[take] = pos[:, 0], pos[:, 1], pos[:, 2]
            self.cell[take] = where
            self.drawn += int(take.size)
            self.placed += int((where >= 0).sum())
            self.respawns[take[where >= 0]] += 1
            entry["taken"] = int(take.size)
        self.epoch += 1
        self.log.append(entry)

    def respawn_box(self, lower, upper, max_count=-1, chosen=None):
        """chosen: the ids the call took, read back from the device -- for a limited respawn on a re-sorted cloud
        (``needs_readback``); without it the model takes the first dead ids in id order there, a stand-in of the right count."""
        self._respawn("cpf_respawn_box", max_count, lambda ids: self.box_origin,
                      lambda ids: R.positions(self.seed, ids, self.epoch, lower, upper).reshape(-1, 3), chosen)

    def respawn_source(self, max_count=-1, chosen=None):
        self._need(self.source is not None, "cpf_respawn_source: no source")
        rec, hi, _ = self.source
        okept = T.origin_of_kept(rec, self.origin_of_triangle)
        self._respawn("cpf_respawn_source", max_count, lambda ids: okept[T.picks(self.seed, ids, self.epoch, hi)] if ids.size else 0,
                      lambda ids: SP.positions(self.seed, ids, self.epoch, rec, hi) if ids.size else np.empty((0, 3)), chosen)

    def recycle_counts(self):
        return dict(absorbed=self.absorbed, drawn=self.drawn, placed=self.placed, epochs=self.epoch)

    # ------------------------------------------------------------------------------------------------ age
    def age_enable(self, bin_cycles, n_bins):
        self._need_cloud("cpf_age_enable")
        self._off("route")
        self.on["age"] = True
        self.bin_cycles, self.age_bins = int(bin_cycles), int(n_bins)
        self.birth = np.full(self.n, self.now, np.uint32)
        self.age_reset()

    def age_disable(self):
        self._off("age", "route")

    def age_reset(self):
        self._need_on("age", "cpf_age_reset")
        self.age_hist = np.zeros(self.age_bins, np.uint64)
        self.age_sum, self.age_count, self.age_samples = np.zeros(self.nc, np.uint64), np.zeros(self.nc, np.uint64), 0

    def age_sample(self):
        self._need_on("age", "cpf_age_sample")
        s, c = A.field(self.parents(), self._ages(), self.nc)
        self.age_sum, self.age_count, self.age_samples = self.age_sum + s, self.age_count + c, self.age_samples + 1

    def age_births(self):
        self._need_on("age", "cpf_age_get_births")
        return self.birth.copy()

    def ages(self):
        self._need_on("age", "cpf_get_ages")
        return np.where(self.cell >= 0, self._ages(), -1)

    def age_histogram(self):
        self._need_on("age", "cpf_get_age_histogram")
        return self.age_hist.copy()

    def age_field(self):
        self._need_on("age", "cpf_get_age_field")
        return self.age_sum.copy(), self.age_count.copy(), self.age_samples

    # ------------------------------------------------------------------------------------------------ tags
    def tag_enable(self, n_origins=1, n_sinks=1):
        self._need_cloud("cpf_tag_enable")
        self._off("route", "exposure")        # (the dose histogram's shape was taken from the old tagging)
        self.on["tag"] = True
        self.n_origins, self.n_sinks = int(n_origins), int(n_sinks)
        self.origin = np.zeros(self.n, np.uint8)
        self.group_of_cell = np.zeros(self.nc, np.int64)
        self.box_origin = 0
        if self.source is not None:
            self.origin_of_triangle = np.zeros(self.source[2], np.int64)
        self.tag_reset()

    def tag_disable(self):
        self._off("tag", "route", "exposure")

    def tag_reset(self):
        self._need_on("tag", "cpf_tag_reset")
        self.transfer_m = np.zeros((self.n_origins, self.n_sinks), np.uint64)
        self.tag_counts, self.tag_samples = np.zeros((self.n_origins, self.nc), np.uint64), 0

    def tag_sample(self):
        self._need_on("tag", "cpf_tag_sample")
        self.tag_counts = self.tag_counts + T.field(self.parents(), self.origin, self.nc, self.n_origins)
        self.tag_samples += 1

    def tag_origins(self):
        self._need_on("tag", "cpf_tag_get_origins")
        return self.origin.copy()

    def transfer(self):
        self._need_on("tag", "cpf_get_transfer")
        return self.transfer_m.copy()

    def tag_field(self):
        self._need_on("tag", "cpf_get_tag_field")
        return self.tag_counts.copy(), self.tag_samples

    # ------------------------------------------------------------------------------------------------ routes
    def route_enable(self):
        self._need(self.on["age"] and self.on["tag"], "cpf_route_enable: age tracking and tagging must both be on")
        self.on["route"] = True
        self.route_reset()

    def route_disable(self):
        self._off("route")

    def route_reset(self):
        self._need_on("route", "cpf_route_reset")
        self.route_hist = np.zeros((self.n_origins, self.n_sinks, self.age_bins), np.uint64)
        self.route_sum, self.route_count = (np.zeros((self.nc, self.n_origins), np.uint64) for _ in range(2))
        self.route_samples = 0

    def route_sample(self):
        self._need_on("route", "cpf_route_sample")
        s, c = RT.field(self.parents(), self.origin, self._ages(), self.nc, self.n_origins)
        self.route_sum, self.route_count, self.route_samples = self.route_sum + s, self.route_count + c, self.route_samples + 1

    def route_histogram(self):
        self._need_on("route", "cpf_get_route_histogram")
        return self.route_hist.copy()

    def route_field(self):
        self._need_on("route", "cpf_get_route_field")
        return self.route_sum.copy(), self.route_count.copy(), self.route_samples

    # ------------------------------------------------------------------------------------------------ exposure
    dose_shape = (1, 1)

    def exposure_enable(self, bin_width, n_bins=1):
        self._need_cloud("cpf_exposure_enable")
        self.on["exposure"] = True
        self.bin_width, self.dose_bins = float(bin_width), int(n_bins)
        self.dose_tagged = self.on["tag"]
        self.dose_shape = (self.n_origins, self.n_sinks) if self.on["tag"] else (1, 1)     # ... as tagging is NOW
        self.dose = np.zeros(self.n, np.float64)
        self.rate = np.zeros(self.nc, np.float64)
        self.exposure_reset()

    def exposure_disable(self):
        self._off("exposure")

    def exposure_reset(self):
        self._need_on("exposure", "cpf_exposure_reset")
        self.dose_hist = np.zeros(self.dose_shape + (self.dose_bins,), np.uint64)

    def set_exposure_field(self, rate):
        self._need_on("exposure", "cpf_set_exposure_field")
        self.rate = np.asarray(rate, np.float64).reshape(-1).copy()
        assert self.rate.size == self.nc

    def exposure_accumulate(self, scale):
        self._need_on("exposure", "cpf_exposure_accumulate")
        self.dose = X.accumulate(self.dose, self.parents(), self.rate, scale)

    def exposure_doses(self):
        self._need_on("exposure", "cpf_exposure_get_doses")
        return self.dose.copy()

    def doses(self):
        self._need_on("exposure", "cpf_get_doses")
        return np.where(self.cell >= 0, self.dose, -1.0)

    def dose_histogram(self):
        self._need_on("exposure", "cpf_get_dose_histogram")
        return self.dose_hist.copy()

    # ------------------------------------------------------------------------------------------------ zones
    def zone_enable(self, n_zones):
        self._need_cloud("cpf_zone_enable")
        self.on["zone"] = True
        self.n_zones = int(n_zones)
        self.last = np.full(self.n, Z.OUTSIDE, np.uint8)
        self.zone_of = np.zeros(self.nc, np.int32)
        self.zone_reset()

    def zone_disable(self):
        self._off("zone")

    def zone_reset(self):
        self._need_on("zone", "cpf_zone_reset")
        self.flow, self.zone_samples = Z.table(self.n_zones), 0

    def set_zone_map(self, zone):
        self._need_on("zone", "cpf_set_zone_map")
        self.zone_of = np.asarray(zone, np.int32).reshape(-1).copy()
        assert self.zone_of.size == self.nc and self.zone_of.max() < self.n_zones

    def zone_sample(self):
        self._need_on("zone", "cpf_zone_sample")
        self.flow, self.last = Z.sample(self.flow, self.last, self.parents(), self.zone_of, self.n_zones)
        self.zone_samples += 1

    def zone_last(self):
        self._need_on("zone", "cpf_zone_get_last")
        return self.last.copy()

    def zone_flows(self):
        self._need_on("zone", "cpf_get_zone_flows")
        return self.flow.copy(), self.zone_samples


# what a test compares: the getters of each group, and one of each that answers if and only if the group is on
GETTERS = dict(age=("age_births", "ages", "age_histogram", "age_field"), tag=("tag_origins", "transfer", "tag_field"),
               route=("route_histogram", "route_field"), exposure=("exposure_doses", "doses", "dose_histogram"),
               zone=("zone_last", "zone_flows"))
PROBE = dict(age="age_histogram", tag="transfer", route="route_histogram", exposure="dose_histogram", zone="zone_flows")
COMMON = ("recycle_counts", "occupancy")


def same(a, b):
    """equality of what two getters return: integers as integers, doubles bit for bit"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if isinstance(a, dict):
        return a == b
    if isinstance(a, np.ndarray):
        b = np.asarray(b)
        if a.shape != b.shape:
            return False
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))
        return np.array_equal(a.astype(np.int64), b.astype(np.int64))
    return a == b


def apply(target, op, **extra):
    """one operation of a script on a ``Ledger`` or on a ``Context``: (name, arguments ...)"""
    return getattr(target, op[0])(*op[1:], **extra)


def run(model, ops, before=None):
    """The operations on the model alone.  A call the model refuses raises ``StateError`` with the operation's index -- unless
    the script says so itself, ("refused", op): then it must be refused.  before(k, op): called ahead of every operation."""
    for k, op in enumerate(ops):
        if before is not None:
            before(k, op)
        if op[0] == "refused":
            try:
                apply(model, op[1])
            except StateError:
                continue
            raise AssertionError("operation %d %s: the model does not refuse it" % (k, op[1][0]))
        try:
            apply(model, op)
        except StateError as e:
            raise StateError(str(e), k) from None


# ---------------------------------------------------------------------------------------------------- identities without a model
class Spans:
    """since when each group's absorption table has been counting: ``note(op, absorbed)`` after every operation that SUCCEEDED,
    with cpf_get_recycle_counts' ``absorbed`` at that moment.  An enable or a reset of a group zeroes its table: its span starts."""
    START = dict(age_enable="age", age_reset="age", tag_enable="tag", tag_reset="tag", route_enable="route", route_reset="route",
                 exposure_enable="exposure", exposure_reset="exposure", zone_enable="zone", zone_reset="zone")

    def __init__(self):
        self.since = {}

    def note(self, op, absorbed):
        g = self.START.get(op[0])
        if g is not None:
            self.since[g] = int(absorbed)


def _if_on(call):
    try:
        return call()
    except L.CpfError as e:
        if e.status != L.CPF_ERR_STATE:
            raise
        return None


def conservation(c, spans):
    """On the getters of ``c`` (a ``Context`` or a ``Ledger``) alone: every group that is on has counted, since its span began,
    exactly the absorptions cpf_get_recycle_counts counted.  Returns the list of (what, got, want) that do not hold."""
    absorbed = c.recycle_counts()["absorbed"]
    bad = []
    sums = dict(age=_if_on(lambda: int(c.age_histogram().sum())), tag=_if_on(lambda: int(c.transfer().sum())),
                route=_if_on(lambda: int(c.route_histogram().sum())), exposure=_if_on(lambda: int(c.dose_histogram().sum())),
                zone=_if_on(lambda: int(c.zone_flows()[0][:, -1].sum())))
    for g, got in sums.items():
        if got is not None and got != absorbed - spans.since[g]:
            bad.append((g, got, absorbed - spans.since[g]))
    rh = _if_on(c.route_histogram)                                # (comparable where both tables count the same absorptions)
    if rh is not None and spans.since["route"] == spans.since["tag"] and not np.array_equal(rh.sum(2), c.transfer()):
        bad.append(("route histogram summed over its bins is the transfer matrix", rh.sum(2).tolist(), c.transfer().tolist()))
    if rh is not None and spans.since["route"] == spans.since["age"] and not np.array_equal(rh.sum((0, 1)), c.age_histogram()):
        bad.append(("route histogram summed over its routes is the age histogram", rh.sum((0, 1)).tolist(), c.age_histogram().tolist()))
    return bad


def zone_sample_identity(flow_before, flow_after, cell):
    """one zone sample adds exactly one count per live particle, none of them to the outside column"""
    d = flow_after.astype(np.int64) - flow_before.astype(np.int64)
    return int(d[:, :-1].sum()) == int((np.asarray(cell) >= 0).sum()) and not d[:, -1].any()


def age_sample_identity(field_before, field_after, ages):
    """one age sample adds the ages of the live to the sums and their number to the counts"""
    ages = np.asarray(ages)
    ds = int(field_after[0].astype(np.int64).sum() - field_before[0].astype(np.int64).sum())
    dc = int(field_after[1].astype(np.int64).sum() - field_before[1].astype(np.int64).sum())
    return ds == int(ages[ages >= 0].sum()) and dc == int((ages >= 0).sum()) and field_after[2] == field_before[2] + 1


# ---------------------------------------------------------------------------------------------------- the script generator
SEEDS = 8
SIZES = (4097, 1, 4095, 10007, 2311, 3000, 5003, 777)         # per seed mod 8: 1, 4095, 4097 and 10007 (no multiple of 64)
SEED_OF_CLOUD = 9


def _last_x_layer(mesh):
    c = mesh.cell_centres_volumes()[0][:, 0]
    return np.nonzero(c >= c.max() - 1e-9)[0].astype(np.int32)


@functools.lru_cache(maxsize=None)
def script(seed):
    """One fuzz case: dict(mesh, U, n, xyz, sort_interval, setup, ops, ...).  ``setup`` and ``ops`` are lists of operations
    (name, arguments ...) named after the ``Context`` methods; ``("refused", op)`` wraps a call that must raise the state error.
    ``setup`` seats the cloud and switches the seed's groups on; ``ops`` is the run: 10 to 25 operations in rounds of (a change of
    state), a step, samples, the sink and respawns -- so every state the cloud is stepped in meets a sink."""
    from cudaparticlesfoam_amd.cases import box_mesh
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    rng = np.random.default_rng(7100 + seed)
    kind = seed % 8
    n = SIZES[kind]
    thin, warped = kind == 2, kind in (3, 7)
    if thin:
        mesh = box_mesh(6, 5, 1)
    elif warped:
        mesh = W.warp_mesh(box_mesh(4, 4, 3), 0.05, seed=seed)
    elif n == 1:
        mesh = box_mesh(3, 3, 3)
    else:
        mesh = box_mesh(int(rng.integers(3, 5)), int(rng.integers(3, 9)), int(rng.integers(3, 9)))
    nc = mesh.n_cells
    lo, hi = mesh.bounds()
    U = rng.normal(size=(nc, 3)) * 0.25
    U[:, 0] = 1.0 + 0.2 * rng.normal(size=nc)
    if thin:
        U[:, 2] = 0.0
    if n == 1:
        U = np.tile([1.0, 0.0, 0.0], (nc, 1))
    U = np.ascontiguousarray(U)
    sink = _last_x_layer(mesh)
    n_origins, n_sinks, n_zones = 3, int(rng.integers(2, 4)), int(rng.integers(3, 7))
    groups = (np.arange(sink.size) % n_sinks).astype(np.int32)
    tri, _ = mesh.face_triangles(SP.boundary_faces_at_x0(mesh))
    origins = (1 + np.arange(tri.shape[0]) % 2).astype(np.int32)
    depth = (0.0, 0.4)
    rate = X.run_rate(mesh)                                       # zero in every fifth cell
    zone_of = (rng.integers(0, n_zones, size=nc)).astype(np.int32) if warped else Z.x_slabs(mesh, n_zones)
    zone_of[0], zone_of[-1] = 0, n_zones - 1
    inside = (tuple(lo + 0.05), (float(lo[0]) + 1.0, float(hi[1]) - 0.05, float(hi[2]) - 0.05))
    sticking = ((float(lo[0]) - 0.1, float(lo[1]), float(lo[2])), (float(lo[0]) + 1.0, float(hi[1]), float(hi[2])))
    xyz = pz.uniform_points(4000 + seed, n, tuple(lo + 0.02), tuple(hi - 0.02))
    if n == 1:
        xyz[0] = (float(hi[0]) - 1.5, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2]))
    dt = 0.2 if n == 1 else 0.45 if thin else 0.3               # a cell in two to five cycles: whoever is respawned comes back
    s = dict(seed=seed, mesh=mesh, U=U, n=n, xyz=xyz, sink=sink, groups=groups, tri=tri, origins=origins, depth=depth, rate=rate,
             zone_of=zone_of, n_zones=n_zones, n_origins=n_origins, n_sinks=n_sinks, sort_interval=int(rng.choice([0, 1, 3, 7])),
             warped=warped, thin=thin, cloud_seed=SEED_OF_CLOUD + seed)

    def enable(which):
        """the operations that switch the groups `which` on, in the order that leaves them all on"""
        out = []
        if "age" in which:
            out.append(("age_enable", int(rng.integers(1, 4)), int(rng.integers(3, 9))))
        if "tag" in which:
            out += [("tag_enable", n_origins, n_sinks), ("set_sink_groups", sink, groups), ("set_box_origin", 1), ("set_source_origins", origins)]
        if "route" in which:
            out.append(("route_enable",))
        if "exposure" in which:
            out += [("exposure_enable", float(rng.choice([0.25, 0.5])), int(rng.integers(2, 9))), ("set_exposure_field", rate)]
        if "zone" in which:
            out += [("zone_enable", n_zones), ("set_zone_map", zone_of)]
        return out

    setup = [("set_particles", xyz), ("locate_initial",), ("set_sink_cells", sink), ("set_source_triangles", tri, None, depth)]
    ops = []
    steps = lambda: ("step", dt, 0.0, int(rng.integers(4, 7) if n == 1 else rng.integers(3, 7) if thin else rng.integers(1, 7)), int(rng.choice([0, FUSE])))   # noqa: E731
    samples = [("age_sample",), ("tag_sample",), ("route_sample",), ("zone_sample",), ("occupancy_sample",), ("exposure_accumulate", 0.5)]
    all_off = [("refused", ("age_reset",)), ("refused", ("set_box_origin", 1)), ("refused", ("route_enable",)),
               ("refused", ("set_exposure_field", rate)), ("refused", ("set_zone_map", zone_of))]

    def rnd(state, change=(), respawns=None, sample_ops=None):
        """a round: changes of state, a step, samples of the groups `state` has on, the sink, respawns"""
        out = list(change) + [steps()]
        pool = [o for o in samples if o[0] == "occupancy_sample" or {"age_sample": "age", "tag_sample": "tag", "route_sample": "route",
                                                                       "zone_sample": "zone", "exposure_accumulate": "exposure"}[o[0]] in state]
        if sample_ops is None:
            pick = rng.permutation(len(pool))[:int(rng.integers(1, 3))]
            sample_ops = [pool[i] for i in sorted(pick)]
        out += sample_ops
        out.append(("sink_apply",))
        if respawns is None:
            respawns = [[("respawn_box", inside[0], inside[1], -1)], [("respawn_source", -1)],
                        [("respawn_box", sticking[0], sticking[1], -1)]][int(rng.integers(0, 3))]
        return out + list(respawns)

    ALL = ("age", "tag", "route", "exposure", "zone")
    few = max(1, n // 40)                                         # fewer than a round absorbs of a cloud of thousands
    if kind == 0:
        # all five on; a limited box respawn in id order, the source places the rest; each group reset between two sinks
        s["sort_interval"] = 0
        setup += [("sink_apply",), ("respawn_box", inside[0], inside[1], -1)] + enable(ALL)
        ops += rnd(ALL, respawns=[("respawn_box", inside[0], inside[1], few), ("respawn_source", -1)])
        ops += rnd(ALL, change=[("age_reset",), ("tag_reset",)], respawns=[("respawn_source", 10 * n), ("respawn_box", inside[0], inside[1], -1)])
        ops += rnd(ALL, change=[("route_reset",), ("exposure_reset",), ("zone_reset",), ("set_option", "sort_interval", 1)])
    elif kind == 1:
        # a cloud of one: absorbed and respawned round after round
        setup += enable(ALL)
        for _ in range(4):
            ops += rnd(ALL, respawns=[("respawn_box", inside[0], inside[1], int(rng.choice([-1, 1, 5])))])
        ops += [("respawn_source", 3)]
    elif kind == 2:
        # the flat walk; routes on and exposure off; a plain sink set under tags and routes: everybody lands in group 0
        s["sort_interval"] = 7
        on = ("age", "tag", "route", "zone")
        setup += enable(on)
        ops += rnd(on)
        ops += rnd(on, change=[("set_sink_cells", sink), ("refused", ("exposure_accumulate", 1.0))])
        ops += rnd(on, change=[("sort_by_cell",)], respawns=[("respawn_box", inside[0], inside[1], few), ("respawn_source", -1)])
        ops += rnd(("age", "tag", "zone"), change=[("route_disable",), ("set_sink_groups", sink, groups)])
    elif kind == 3:
        # warped cells: derived ids inside, parent ids outside; exposure enabled while tagging is off, then tags come on
        on = ("age", "exposure", "zone")
        setup += enable(on)
        ops += rnd(on)
        ops += rnd(("age", "tag", "zone"), change=enable(("tag",)) + [("refused", ("exposure_accumulate", 1.0)), ("refused", ("exposure_reset",))])
        ops += rnd(ALL, change=enable(("route", "exposure")), respawns=[("respawn_source", -1), ("respawn_box", inside[0], inside[1], -1)])
    elif kind == 4:
        # a reseat in the middle: everything is off until it is enabled again
        setup += enable(ALL)
        ops += rnd(ALL)
        ops += [("set_particles", xyz[::-1].copy()), ("locate_initial",)] + all_off
        ops += rnd((), sample_ops=[("occupancy_sample",)])
        ops += rnd(("age", "tag", "route"), change=enable(("age", "tag", "route")))
    elif kind == 5:
        # limited respawns on a re-sorted cloud, from both sources; nobody dead; more asked for than are dead
        s["sort_interval"] = 1
        setup += enable(ALL)
        ops += rnd(ALL, respawns=[("respawn_box", inside[0], inside[1], few), ("respawn_source", few), ("respawn_box", sticking[0], sticking[1], -1)])
        ops += rnd(ALL, change=[("set_option", "sort_method", 0)], respawns=[("respawn_source", -1), ("respawn_source", -1), ("respawn_box", inside[0], inside[1], 7)])
        ops += rnd(ALL, change=[("set_option", "sort_interval", 3), ("set_option", "sort_method", 2), ("sort_by_cell",)],
                   respawns=[("respawn_source", few), ("respawn_box", inside[0], inside[1], 10 * n)])
    elif kind == 6:
        # groups going off and on in the run: each rung of the ladder with the others around it
        setup += enable(ALL)
        ops += rnd(ALL)
        ops += rnd(("tag", "exposure", "zone"), change=[("age_disable",), ("refused", ("route_sample",))])
        ops += rnd(("zone",), change=[("tag_disable",)])
        ops += rnd(("age", "exposure"), change=[("zone_disable",)] + enable(("age", "exposure")))
    else:
        # warped cells again, a zone map that follows no slab; a source whose triangles were set after tagging came on
        s["sort_interval"] = 3
        setup += enable(ALL)
        ops += rnd(ALL, respawns=[("respawn_box", sticking[0], sticking[1], -1)])
        ops += rnd(ALL, change=[("set_source_triangles", tri[::2], None, (0.0, 0.2)), ("set_source_origins", origins[::2])],
                   respawns=[("respawn_source", few), ("respawn_source", -1)])
        ops += rnd(ALL, change=[("set_sink_cells", sink), ("tag_reset",)])
        ops += rnd(ALL, change=[("set_sink_groups", sink, groups), ("exposure_disable",)] + enable(("exposure",)))
    s["setup"], s["ops"] = setup, ops
    return s


def start(s):
    """the model of a script, before its first operation"""
    return Ledger(s["mesh"], s["U"], s["cloud_seed"], sort_interval=s["sort_interval"])


@functools.lru_cache(maxsize=None)
def dry_run(seed):
    """the script on the model alone, every refused call checked: (script, model, the state of the groups before every operation)"""
    s = script(seed)
    m = start(s)
    states = []
    run(m, s["setup"] + s["ops"], before=lambda k, op: states.append((op, dict(m.on), m.rungs(), m.located)))
    return s, m, states
