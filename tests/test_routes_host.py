"""CPU: the host side of the routes (include/cpf.h "routes"): the numpy statements of tests/routes.py against those of
tests/age.py and tests/tags.py -- the joint histogram's two marginals are the transfer matrix and the residence-time histogram, the
field per origin sums to the age field and counts what the tag field counts --, the six entries in ``_lib``, the calls
``CudaParticles`` makes with ``routeStats`` and what it refuses before any device call."""
import ctypes as C

import numpy as np
import pytest

import age as A
import routes as RT
import tags as T
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

ENTRIES = ("cpf_route_enable", "cpf_route_disable", "cpf_route_sample", "cpf_route_reset", "cpf_get_route_histogram",
           "cpf_get_route_field")


# ------------------------------------------------------------------------------------------------ 1. the statements
def test_1_the_statements_on_a_case_counted_by_hand():
    cell = np.array([0, 2, 2, -1, 3, 2, 1], np.int32)
    origin = np.array([0, 1, 2, 2, 1, 1, 0], np.uint8)
    age = np.array([9, 0, 5, 7, 6, 100, 2], np.int64)
    group = T.group_of_cell(4, [2, 3], [1, 0])
    hit = np.isin(cell, [2, 3])
    H = RT.hist(origin, group, cell, hit, age, 3, 3, 3, 2)                   # bins [0, 3), [3, 6), [6, inf)
    want = np.zeros((3, 2, 3), np.uint64)
    want[1, 1, 0] = 1                                                        # particle 1: origin 1, cell 2 (group 1), age 0
    want[2, 1, 1] = 1                                                        # particle 2: origin 2, cell 2, age 5
    want[1, 0, 2] = 1                                                        # particle 4: origin 1, cell 3 (group 0), age 6
    want[1, 1, 2] = 1                                                        # particle 5: origin 1, cell 2, age 100 (the open bin)
    assert H.dtype == np.uint64 and np.array_equal(H, want)
    s, c = RT.field(cell, origin, age, 4, 3)
    assert s.tolist() == [[9, 0, 0], [2, 0, 0], [0, 100, 5], [0, 6, 0]] and c.tolist() == [[1, 0, 0], [1, 0, 0], [0, 2, 1], [0, 1, 0]]


@pytest.mark.parametrize("n_origins,n_sinks,bin_cycles,n_bins", [(1, 1, 1, 1), (3, 2, 7, 16), (16, 16, 1, 16), (4, 4, 1, 257)])
def test_1_the_marginals_are_the_statements_of_age_and_tags(n_origins, n_sinks, bin_cycles, n_bins):
    rng = np.random.default_rng(n_bins)
    n, n_cells = 20_011, 97
    cell = rng.integers(-2, n_cells, size=n).astype(np.int32)
    origin = rng.integers(0, n_origins, size=n).astype(np.uint8)
    now = 1000
    births = rng.integers(0, now + 1, size=n).astype(np.uint32)
    births[::13] = now + 1 + rng.integers(0, 5, size=births[::13].size)      # wrapped stamps: ages just below 2^32
    age = A.ages(now, births)
    sink = rng.choice(n_cells, size=31, replace=False)
    groups = rng.integers(0, n_sinks, size=sink.size)
    group = T.group_of_cell(n_cells, sink, groups)
    hit = np.isin(cell, sink)
    H = RT.hist(origin, group, cell, hit, age, bin_cycles, n_bins, n_origins, n_sinks)
    assert H.shape == (n_origins, n_sinks, n_bins) and int(H.sum()) == int(hit.sum()) > 0
    assert np.array_equal(H.sum(axis=2), T.transfer(origin, group, cell, hit, n_origins, n_sinks))
    assert np.array_equal(H.sum(axis=(0, 1)), A.rtd(age[hit], bin_cycles, n_bins))
    parent = np.where(cell >= 0, cell, -1)
    s, c = RT.field(parent, origin, age, n_cells, n_origins)
    assert np.array_equal(c, T.field(parent, origin, n_cells, n_origins).T)
    total, count = A.field(parent, age, n_cells)
    assert np.array_equal(s.sum(axis=1), total) and np.array_equal(c.sum(axis=1), count)


def test_1_window_edge_arrays():
    for n_origins in (1, 16):
        c, o = RT.window_edge(n_origins)
        assert c.dtype == np.int32 and o.dtype == np.uint8 and c.size == o.size == 8192 and o.max() == n_origins - 1


# ------------------------------------------------------------------------------------------------ 2. the entries
def test_2_lib_declares_the_six_entries():
    for name in ENTRIES:
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[0] is C.c_void_p
    assert len(L.SIGNATURES["cpf_get_route_histogram"][1]) == 2 and len(L.SIGNATURES["cpf_get_route_field"][1]) == 4
    for name in ("cpf_route_enable", "cpf_route_disable", "cpf_route_sample", "cpf_route_reset"):
        assert len(L.SIGNATURES[name][1]) == 1
    text = open(api.__file__.replace("api.py", "../include/cpf.h")).read()
    for name in ENTRIES:
        assert "int %s(cpf_context* ctx" % name in text, name


# ------------------------------------------------------------------------------------------------ 3. CudaParticles
class _Recorder:
    """Stands in for ``api.Context``: records the calls ``CudaParticles`` makes (no library, no GPU)."""

    def __init__(self, device=0):
        self.calls = []

    def set_option(self, key, value): pass
    def set_mesh(self, mesh): pass
    def set_velocity(self, U): pass
    def set_sink_cells(self, cells): pass
    def seed_box(self, n, lo, hi, order=1): pass
    def locate_initial(self): self.calls.append(("locate",)); return 0
    def sort_by_cell(self): pass
    def step(self, dt, D, n, flags): self.calls.append(("step", n))
    def occupancy_sample(self): self.calls.append(("sample",))
    def sink_apply(self): self.calls.append(("sink",))
    def respawn_box(self, lo, hi, max_count): self.calls.append(("respawn",))
    def age_enable(self, bin_cycles, n_bins): self.calls.append(("age_enable", bin_cycles, n_bins))
    def age_sample(self): self.calls.append(("age_sample",))
    def tag_enable(self, n_origins, n_sinks): self.calls.append(("tag_enable", n_origins, n_sinks))
    def set_sink_groups(self, cells, groups): self.calls.append(("sink_groups",))
    def tag_sample(self): self.calls.append(("tag_sample",))
    def route_enable(self): self.calls.append(("route_enable",))
    def route_sample(self): self.calls.append(("route_sample",))
    def rtd_by_route(self, dt): return ("rtd_by_route", dt)
    def mean_age_by_origin(self, dt): return ("mean_age_by_origin", dt)
    def close(self): pass


class _NoDevice:
    """Stands in for ``api.Context``: any use is a failure"""

    def __init__(self, device=0):
        raise AssertionError("a context was made")


def test_3_route_stats_needs_age_bins_and_tags(monkeypatch):
    monkeypatch.setattr(api, "Context", _NoDevice)
    assert "routeStats" not in api.DICT_DEFAULTS                             # this library's own key
    dt = 2.0 ** -13
    base = dict(dt=dt, recycleInterval=2, occupancyInterval=4, sinkCells=[0, 1])
    with pytest.raises(ValueError):
        api.CudaParticles(None, np.zeros((4, 3)), dict(base, routeStats=True, sinkGroups=[0, 1]))                # no ageBins
    with pytest.raises(ValueError):
        api.CudaParticles(None, np.zeros((4, 3)), dict(base, routeStats=True, ageBins=5))                        # no tags
    with pytest.raises(ValueError):
        api.CudaParticles(None, np.zeros((4, 3)), dict(base, routeStats=True))                                   # neither


def test_3_route_stats_enables_behind_age_and_tags_and_samples_behind_them(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    dt = 2.0 ** -13
    base = dict(dt=dt, recycleInterval=2, occupancyInterval=4, sinkCells=[0, 1], sinkGroups=[0, 1], ageBins=5)
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(base, routeStats=True))
    assert p.routeStats
    p.advect(0.0, 6 * dt)
    K, Rs = ("sink",), ("respawn",)
    samples = [("sample",), ("age_sample",), ("tag_sample",), ("route_sample",)]
    assert p.ctx.calls == [("locate",), ("age_enable", 2, 5), ("tag_enable", 1, 2), ("sink_groups",), ("route_enable",), ("step", 2), K, Rs,
                           ("step", 2), K, Rs] + samples + [("step", 2), K, Rs]
    assert p.rtd_by_route() == ("rtd_by_route", dt) and p.mean_age_by_origin() == ("mean_age_by_origin", dt)
    # without the key: the calls of today
    q = api.CudaParticles(None, np.zeros((4, 3)), base)
    assert not q.routeStats
    q.advect(0.0, 6 * dt)
    assert q.ctx.calls == [c for c in p.ctx.calls if not c[0].startswith("route")]
