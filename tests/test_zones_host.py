"""CPU: zones (include/cpf.h "zones") without a device -- the numpy statement of tests/zones.py against a brute-force loop,
``_next_chunk`` with a zone interval, the calls ``CudaParticles`` makes with ``zoneMap`` and what it refuses before any context
exists, the two helpers on a table made by hand, the entries in ``_lib`` and in the header."""
import ctypes as C

import numpy as np
import pytest

import zones as Z
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

ENTRIES = ("cpf_zone_enable", "cpf_zone_disable", "cpf_set_zone_map", "cpf_zone_sample", "cpf_zone_reset", "cpf_get_zone_flows",
           "cpf_zone_get_last", "cpf_zone_set_last")


# ------------------------------------------------------------------------------------------------ 1. the statement
def _loop(flow, last, cell, zone_of, sink_cells, n_zones):
    """sample, then leave, then the sink and a stamp, one particle at a time"""
    flow, last, cell = flow.copy(), last.copy(), cell.copy()
    for i in range(cell.size):
        if cell[i] < 0:
            continue
        p = n_zones if last[i] == 0xFF else int(last[i])
        z = int(zone_of[cell[i]])
        flow[p, z] += 1
        if p != z:
            last[i] = z
    for i in range(cell.size):
        if cell[i] >= 0 and cell[i] in sink_cells:
            flow[n_zones if last[i] == 0xFF else int(last[i]), n_zones] += 1
            cell[i] = -1
    for i in range(cell.size):
        if cell[i] < 0:
            last[i] = 0xFF
    return flow, last, cell


@pytest.mark.parametrize("n_zones", [1, 4, 63])
def test_1_the_statement_against_a_loop(n_zones):
    rng = np.random.default_rng(n_zones)
    n, n_cells = 400, 90
    zone_of = rng.integers(0, n_zones, size=n_cells).astype(np.int32)
    sink_cells = np.array([3, 17, 40, 41, 89], np.int32)
    flow = Z.table(n_zones)
    last = np.where(rng.random(n) < 0.3, 0xFF, rng.integers(0, n_zones, size=n)).astype(np.uint8)
    for _ in range(3):
        cell = rng.integers(0, n_cells, size=n).astype(np.int32)
        cell[rng.random(n) < 0.1] = -1
        cell[rng.random(n) < 0.05] = -2
        want_flow, want_last, want_cell = _loop(flow, last, cell, zone_of, set(sink_cells.tolist()), n_zones)
        flow, after = Z.sample(flow, last, cell, zone_of, n_zones)
        assert np.array_equal(after[cell < 0], last[cell < 0])                # the dead keep their byte
        flow = Z.leave(flow, after, cell, sink_cells, n_zones)
        cell = np.where(np.isin(cell, sink_cells), -1, cell)
        last = Z.stamp(after, cell)
        assert np.array_equal(flow, want_flow) and np.array_equal(last, want_last) and np.array_equal(cell, want_cell)
    assert flow.dtype == np.uint64 and flow.shape == (n_zones + 1, n_zones + 1)
    assert flow[n_zones, :n_zones].sum() > 0 and flow[:n_zones, n_zones].sum() > 0 and flow[n_zones, n_zones] == 0


def test_1_the_statement_on_a_case_counted_by_hand():
    zone_of = np.array([0, 0, 1, 2], np.int32)
    cell = np.array([0, 2, -1, 3, 1], np.int32)
    last = np.array([0xFF, 1, 2, 0, 0], np.uint8)
    flow, after = Z.sample(Z.table(3), last, cell, zone_of, 3)
    assert after.tolist() == [0, 1, 2, 2, 0]
    want = np.zeros((4, 4), np.uint64)
    want[3, 0] = 1; want[1, 1] = 1; want[0, 2] = 1; want[0, 0] = 1
    assert np.array_equal(flow, want)
    flow = Z.leave(flow, after, cell, np.array([3, 2], np.int32), 3)
    want[1, 3] = 1; want[2, 3] = 1                                           # ids 1 and 3; id 2 is dead already
    assert np.array_equal(flow, want)
    assert Z.stamp(after, np.array([0, -1, -1, -1, 1])).tolist() == [0, 0xFF, 0xFF, 0xFF, 0]


# ------------------------------------------------------------------------------------------------ 2. the helpers
def test_2_residence_and_exchange_rates_on_a_table_made_by_hand():
    #             to: 0   1   out
    f = np.array([[30, 6, 2],                                                # from zone 0
                  [4, 10, 1],                                                # from zone 1
                  [3, 0, 0]], np.uint64)                                     # from outside: three entered zone 0
    rates = api.zone_exchange_rates(f, 10, 0.5)
    want = np.array([[0.0, 6 / 5.0, 2 / 5.0], [4 / 5.0, 0.0, 1 / 5.0], [3 / 5.0, 0.0, 0.0]])
    assert np.array_equal(rates, want)
    assert np.isnan(api.zone_exchange_rates(f, 0, 0.5)[0, 1])
    # zone 0: 37 samples found somebody in it, 7 of them for the first time of a visit; zone 1: 16 and 6
    res = api.zone_residence(f, 0.5)
    assert np.array_equal(res, np.array([0.5 * 37.0 / 7.0, 0.5 * 16.0 / 6.0]))
    g = f.copy(); g[:, 1] = 0; g[1, 1] = 5                                   # nobody entered zone 1
    res = api.zone_residence(g, 0.5)
    assert res[0] == 0.5 * 37.0 / 7.0 and np.isnan(res[1])


# ------------------------------------------------------------------------------------------------ 3. _next_chunk
def test_3_next_chunk_ends_a_fused_launch_at_a_zone_point():
    nc = api._next_chunk
    assert nc(0, 7, 10, 0, False, False, 0) == 7 == nc(0, 7, 10, 0, False, False, 0, zone_interval=0)
    assert nc(0, 7, 10, 0, False, False, 0, zone_interval=3) == 3
    assert nc(4, 7, 10, 0, False, False, 0, zone_interval=3) == 2
    assert nc(6, 7, 10, 0, False, False, 0, zone_interval=3) == 3
    assert nc(0, 7, 10, 0, False, False, 0, zone_interval=1) == 1
    assert nc(0, 2, 10, 0, False, False, 0, zone_interval=5) == 2              # the end of the call comes first
    assert nc(0, 7, 10, 4, False, False, 2, zone_interval=3) == 2              # the recycle point comes first
    assert nc(0, 7, 10, 0, False, False, 4, zone_interval=3) == 3              # ... or the zone point
    assert nc(0, 7, 10, 0, False, False, 6, exposure_interval=4, zone_interval=5) == 4      # with an exposure interval as well
    assert nc(4, 7, 10, 0, False, False, 6, exposure_interval=4, zone_interval=5) == 1
    assert nc(5, 7, 10, 0, False, False, 6, exposure_interval=4, zone_interval=5) == 1
    assert nc(0, 7, 10, 0, True, True, 0, zone_interval=5) == 1                # a cycle that writes runs alone
    with pytest.raises(TypeError):                                           # by keyword only
        nc(0, 7, 10, 0, False, False, 0, 0, 3)
    assert nc(0, 7, 10, 0, False, False, 0, exposure_interval=3) == 3          # the existing keyword keeps its meaning


# ------------------------------------------------------------------------------------------------ 4. CudaParticles
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
    def exposure_enable(self, bin_width, n_bins): self.calls.append(("exposure_enable",))
    def set_exposure_field(self, rate): self.calls.append(("exposure_field",))
    def exposure_accumulate(self, scale): self.calls.append(("accumulate",))
    def zone_enable(self, n_zones): self.calls.append(("zone_enable", n_zones))
    def set_zone_map(self, zone): self.calls.append(("zone_map", np.asarray(zone).tolist()))
    def zone_sample(self): self.calls.append(("zone_sample",))
    def zone_flows(self): return ("zone_flows",)
    def zone_residence(self, sample_dt): return ("zone_residence", sample_dt)
    def close(self): pass


class _NoDevice:
    """Stands in for ``api.Context``: any use is a failure"""

    def __init__(self, device=0):
        raise AssertionError("a context was made")


def test_4_what_cuda_particles_refuses_before_any_context_exists(monkeypatch):
    monkeypatch.setattr(api, "Context", _NoDevice)
    for key in ("zoneMap", "zoneInterval"):
        assert key not in api.DICT_DEFAULTS                                  # this library's own keys
    U, zmap = np.zeros((4, 3)), [0, 1, 1, 2]
    bad = [dict(zoneMap=[0, -1, 1, 1]), dict(zoneMap=[0, 63, 1, 1]), dict(zoneMap=zmap, zoneInterval=0),
           dict(zoneMap=zmap, zoneInterval=-2), dict(zoneInterval=2), dict(zoneInterval=1)]
    for d in bad:
        with pytest.raises(ValueError):
            api.CudaParticles(None, U, d)
    for ok in (dict(zoneMap=zmap, zoneInterval=3), dict(zoneMap=[0, 62, 1, 1])):     # ... and these are accepted
        with pytest.raises(AssertionError, match="a context was made"):
            api.CudaParticles(None, U, ok)


def test_4_the_zone_sample_comes_before_the_sink(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    dt = 2.0 ** -13
    zmap = [0, 1, 1, 2]
    base = dict(dt=dt, recycleInterval=4, occupancyInterval=4, sinkCells=[0, 1])
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(base, zoneMap=zmap, zoneInterval=2))
    assert p.zoneInterval == 2 and p.zoneMap.dtype == np.int32
    assert p.ctx.calls == [("locate",), ("zone_enable", 3), ("zone_map", zmap)]
    del p.ctx.calls[:]
    assert p.advect(0.0, 7 * dt) == 7
    Zs, K, Rs, S = ("zone_sample",), ("sink",), ("respawn",), ("sample",)
    assert p.ctx.calls == [("step", 2), Zs, ("step", 2), Zs, K, Rs, S, ("step", 2), Zs, ("step", 1)]
    assert p.zone_flows() == ("zone_flows",) and p.zone_residence() == ("zone_residence", 2 * dt)
    # interval 3 against a recycle interval of 2 and an exposure interval of 4: whichever comes first ends the launch; at a
    # common point the accumulate, then the zone sample, then the sink
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=2, sinkCells=[0], zoneMap=zmap, zoneInterval=3,
                                                       exposureField=[0.0, 1.0, 2.0, 0.5], exposureInterval=4))
    assert q.ctx.calls == [("locate",), ("exposure_enable",), ("exposure_field",), ("zone_enable", 3), ("zone_map", zmap)]
    del q.ctx.calls[:]
    q.advect(0.0, 12 * dt)
    A = ("accumulate",)
    assert q.ctx.calls == [("step", 2), K, Rs, ("step", 1), Zs, ("step", 1), A, K, Rs, ("step", 2), Zs, K, Rs,
                           ("step", 2), A, K, Rs, ("step", 1), Zs, ("step", 1), K, Rs, ("step", 2), A, Zs, K, Rs]
    # the default interval is every cycle
    d = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, zoneMap=zmap))
    del d.ctx.calls[:]
    d.advect(0.0, 3 * dt)
    assert d.ctx.calls == [("step", 1), Zs] * 3
    # without the key: the calls of today
    r = api.CudaParticles(None, np.zeros((4, 3)), base)
    assert r.zoneMap is None
    del r.ctx.calls[:]
    r.advect(0.0, 7 * dt)
    assert r.ctx.calls == [("step", 4), K, Rs, S, ("step", 3)]


# ------------------------------------------------------------------------------------------------ 5. the entries
def test_5_lib_and_header_declare_the_entries():
    for name in ENTRIES:
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[0] is C.c_void_p
    assert L.SIGNATURES["cpf_zone_enable"][1][1:] == [C.c_int32]
    assert L.SIGNATURES["cpf_set_zone_map"][1][1:] == [C.c_void_p, C.c_int64]
    assert L.SIGNATURES["cpf_get_zone_flows"][1][1:] == [C.c_void_p, C.c_void_p]
    text = open(api.__file__.replace("api.py", "../include/cpf.h")).read()
    for name in ENTRIES:
        assert "int %s(cpf_context* ctx" % name in text, name


def test_5_null_contexts_are_refused_without_a_device():
    lib = L.load()
    out = np.zeros(16, np.uint64)
    p = api._ptr
    assert lib.cpf_zone_enable(None, 4) == L.CPF_ERR_ARG
    assert lib.cpf_zone_disable(None) == L.CPF_ERR_ARG
    assert lib.cpf_set_zone_map(None, p(out), 4) == L.CPF_ERR_ARG
    assert lib.cpf_zone_sample(None) == L.CPF_ERR_ARG
    assert lib.cpf_zone_reset(None) == L.CPF_ERR_ARG
    assert lib.cpf_get_zone_flows(None, p(out), None) == L.CPF_ERR_ARG
    assert lib.cpf_zone_get_last(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_zone_set_last(None, p(out)) == L.CPF_ERR_ARG
