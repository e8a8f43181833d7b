"""CPU: the host side of exposure (include/cpf.h "exposure"): the numpy statement's own arithmetic (tests/exposure.py),
``cpf_exposure_bins_host`` against it on every bin edge and one ulp either side, conditions on the CPU statement of the recycled runs
that tests/test_gpu_exposure.py compares against, ``_next_chunk`` with an exposure interval, the calls ``CudaParticles`` makes with
``exposureField`` and what it refuses before any context exists, the entries in ``_lib`` and in the header."""
import ctypes as C

import numpy as np
import pytest

import exposure as E
import recycle as R
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

ENTRIES = ("cpf_exposure_enable", "cpf_exposure_disable", "cpf_set_exposure_field", "cpf_exposure_accumulate", "cpf_exposure_reset",
           "cpf_get_dose_histogram", "cpf_get_doses", "cpf_exposure_get_doses", "cpf_exposure_set_doses")


def _bins_host(dose, bin_width, n_bins):
    dose = np.ascontiguousarray(dose, dtype=np.float64)
    out = np.full(dose.size, -7, np.int32)
    assert L.load().cpf_exposure_bins_host(api._ptr(dose), dose.size, float(bin_width), int(n_bins), api._ptr(out)) == L.CPF_OK
    return out


def edge_doses(bin_width, n_bins):
    """0, every bin edge b * bin_width, one ulp either side of each, and inf"""
    e = np.arange(n_bins + 1, dtype=np.float64) * np.float64(bin_width)
    return np.concatenate([[0.0], e, np.nextafter(e[1:], 0.0), np.nextafter(e, np.inf), [np.inf]])


# ------------------------------------------------------------------------------------------------ 1. the statement's arithmetic
def test_1_the_statement_on_a_case_counted_by_hand():
    cell = np.array([0, 2, -1, 3, 2, 7], np.int32)
    rate = np.array([1.0, 0.0, 0.5, 4.0])
    d = E.accumulate(np.array([0.0, 1.0, 9.0, 0.25, 0.0, 3.0]), cell, rate, 0.5)
    assert d.tolist() == [0.5, 1.25, 9.0, 2.25, 0.25, 3.0]                   # the dead slot and the foreign id keep theirs
    # each operation is rounded on its own: 0.1 * 3.0 is not 0.3
    d = E.accumulate(np.array([1.0]), np.array([0]), np.array([3.0]), 0.1)
    assert d[0] == 1.0 + np.float64(0.1) * np.float64(3.0)
    assert E.bins([0.0, 0.49, 0.5, 1.49, 1.5, 100.0, np.inf], 0.5, 4).tolist() == [0, 0, 1, 2, 3, 3, 3]
    assert E.bins([0.0, 5.0, np.inf], 0.5, 1).tolist() == [0, 0, 0]
    group = np.array([0, 0, 1, 0])
    h = E.histogram(cell, [2, 3], [0.0, 0.6, 0.0, 0.1, 9.0, 0.0], 0.5, 4, origin=[0, 1, 0, 1, 1, 0], group_of_cell=group, n_origins=2,
                    n_sinks=2)
    want = np.zeros((2, 2, 4), np.uint64)
    want[1, 1, 1] = 1                                                        # particle 1: origin 1, cell 2 (group 1), dose 0.6
    want[1, 0, 0] = 1                                                        # particle 3: origin 1, cell 3 (group 0), dose 0.1
    want[1, 1, 3] = 1                                                        # particle 4: origin 1, cell 2, dose 9 (the open bin)
    assert h.dtype == np.uint64 and np.array_equal(h, want)


# ------------------------------------------------------------------------------------------------ 2. the bin rule on the host
@pytest.mark.parametrize("bin_width", [0.25, 0.1, 3.0, 1e-7, 1e300])
@pytest.mark.parametrize("n_bins", [1, 16, 4096])
def test_2_bins_host_is_the_numpy_rule_on_every_edge(n_bins, bin_width):
    dose = edge_doses(bin_width, n_bins)
    got, want = _bins_host(dose, bin_width, n_bins), E.bins(dose, bin_width, n_bins)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], dose[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert got.min() == 0 and got.max() == n_bins - 1 and got[0] == 0 and got[-1] == n_bins - 1
    if n_bins > 1 and bin_width == 0.25:                                     # a power of two: the edges are exact
        e = np.arange(n_bins, dtype=np.float64) * bin_width
        assert np.array_equal(_bins_host(e, bin_width, n_bins), np.arange(n_bins))
        assert np.array_equal(_bins_host(np.nextafter(e[1:], 0.0), bin_width, n_bins), np.arange(n_bins - 1))


def test_2_bins_host_arguments():
    lib = L.load()
    d, b = np.array([0.0, 1.0, -1.0, np.nan, -0.0]), np.zeros(5, np.int32)
    assert lib.cpf_exposure_bins_host(api._ptr(d), 5, 0.5, 4, api._ptr(b)) == L.CPF_OK
    assert b.tolist() == [0, 2, -1, -1, 0]                                   # no bin for what is no dose
    for width, n_bins in ((0.0, 4), (-1.0, 4), (np.inf, 4), (np.nan, 4), (0.5, 0), (0.5, -3)):
        assert lib.cpf_exposure_bins_host(api._ptr(d), 5, width, n_bins, api._ptr(b)) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_bins_host(None, 5, 0.5, 4, api._ptr(b)) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_bins_host(api._ptr(d), 5, 0.5, 4, None) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_bins_host(api._ptr(d), -1, 0.5, 4, api._ptr(b)) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_bins_host(None, 0, 0.5, 4, None) == L.CPF_OK


# ------------------------------------------------------------------------------------------------ 3. conditions on the inputs
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_3_the_cpu_statement_of_the_recycled_runs_has_doses(oracle_libs, name, interval):
    """On the runs of tests/recycle.py: at least 200 absorptions in at least 4 distinct dose bins, respawned particles that start
    from 0 again -- and the cloud is tests/recycle.py's own, stepped a cycle at a time."""
    r = R.run(name)
    c = E.cpu(name, interval)
    last = c["points"][-1]
    hist = last["hist"]
    print("MEASURED %s, every %d | absorbed %d | histogram %s | largest dose %.3f"
          % (name, interval, c["absorbed"], hist[0, 0].tolist(), last["dose"].max()))
    assert hist.shape == (1, 1, E.N_BINS) and int(hist.sum()) == c["absorbed"] >= 200
    assert int((hist > 0).sum()) >= 4
    assert len(c["points"]) == r.rounds
    live = last["cell"] >= 0
    assert (last["doses"][~live] == -1.0).all() and (last["dose"][~live] == 0.0).all() and (last["doses"][live] >= 0.0).all()
    assert np.unique(last["dose"]).size > 100 and (E.run_rate(r.mesh) == 0.0).any()
    from cudaparticlesfoam_amd import api as _api
    t = _api.build_mesh_tables_host(r.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    xyz, cell, absorbed, _, _, _ = r.cpu(tables, R.brute_locate(r.xyz, tables))
    assert np.array_equal(xyz.view(np.int64), c["xyz"].view(np.int64)) and np.array_equal(cell, c["cell"]) and absorbed == c["absorbed"]


def test_3_the_interval_matters_and_the_absorbed_carry_their_last_interval(oracle_libs):
    a, b = E.cpu("thin box", 1), E.cpu("thin box", 3)
    assert not np.array_equal(a["points"][-1]["dose"], b["points"][-1]["dose"])
    assert np.array_equal(a["cell"], b["cell"])


# ------------------------------------------------------------------------------------------------ 4. _next_chunk
def test_4_next_chunk_ends_a_fused_launch_at_an_exposure_point():
    nc = api._next_chunk
    assert nc(0, 7, 10, 0, False, False, 0) == 7 == nc(0, 7, 10, 0, False, False, 0, exposure_interval=0)
    assert nc(0, 7, 10, 0, False, False, 0, exposure_interval=3) == 3
    assert nc(4, 7, 10, 0, False, False, 0, exposure_interval=3) == 2
    assert nc(6, 7, 10, 0, False, False, 0, exposure_interval=3) == 3
    assert nc(0, 7, 10, 0, False, False, 0, exposure_interval=1) == 1
    assert nc(0, 2, 10, 0, False, False, 0, exposure_interval=5) == 2          # the end of the call comes first
    assert nc(0, 7, 10, 4, False, False, 2, exposure_interval=3) == 2          # the recycle point comes first
    assert nc(2, 7, 10, 4, False, False, 6, exposure_interval=5) == 2          # the occupancy sample comes first
    assert nc(0, 7, 10, 0, True, True, 0, exposure_interval=5) == 1            # a cycle that writes runs alone
    assert nc(7, 9, 10, 0, True, False, 0, exposure_interval=5) == 3           # an output point or an exposure point
    # existing positional calls keep their meaning, and the new argument is by keyword only
    assert nc(0, 7, 10, 4, False, False, 2) == 2
    with pytest.raises(TypeError):
        nc(0, 7, 10, 0, False, False, 0, 3)


# ------------------------------------------------------------------------------------------------ 5. CudaParticles
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
    def exposure_enable(self, bin_width, n_bins): self.calls.append(("exposure_enable", bin_width, n_bins))
    def set_exposure_field(self, rate): self.calls.append(("exposure_field", np.asarray(rate).tolist()))
    def exposure_accumulate(self, scale): self.calls.append(("accumulate", scale))
    def dose_distribution(self): return ("dose_distribution",)
    def doses(self): return ("doses",)
    def close(self): pass


class _NoDevice:
    """Stands in for ``api.Context``: any use is a failure"""

    def __init__(self, device=0):
        raise AssertionError("a context was made")


def test_5_what_cuda_particles_refuses_before_any_context_exists(monkeypatch):
    monkeypatch.setattr(api, "Context", _NoDevice)
    for key in ("exposureField", "exposureInterval", "doseBins", "doseBinWidth"):
        assert key not in api.DICT_DEFAULTS                                  # this library's own keys
    U, field = np.zeros((4, 3)), [0.0, 1.0, 2.0, 0.5]
    bad = [dict(exposureField=[0.0, np.nan, 1.0, 1.0]), dict(exposureField=[0.0, np.inf, 1.0, 1.0]), dict(exposureField=[0.0, -1e-300, 1.0, 1.0]),
           dict(exposureField=field, exposureInterval=0), dict(exposureField=field, exposureInterval=-2),
           dict(exposureField=field, doseBins=4), dict(exposureField=field, doseBins=4, doseBinWidth=0.0),
           dict(exposureField=field, doseBins=4, doseBinWidth=-1.0), dict(exposureField=field, doseBins=4, doseBinWidth=np.nan),
           dict(exposureField=field, doseBins=0, doseBinWidth=1.0),
           dict(exposureInterval=2), dict(doseBins=4), dict(doseBinWidth=0.5), dict(exposureInterval=1, doseBins=1, doseBinWidth=0.5)]
    for d in bad:
        with pytest.raises(ValueError):
            api.CudaParticles(None, U, d)
    with pytest.raises(AssertionError, match="a context was made"):         # ... and this one is accepted
        api.CudaParticles(None, U, dict(exposureField=field, doseBins=4, doseBinWidth=0.5, exposureInterval=3))


def test_5_accumulate_comes_before_the_sink_with_the_time_since_the_last_point(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    dt = 2.0 ** -13
    field = [0.0, 1.0, 2.0, 0.5]
    base = dict(dt=dt, recycleInterval=4, occupancyInterval=4, sinkCells=[0, 1], sinkGroups=[0, 1], ageBins=5, routeStats=True)
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(base, exposureField=field, exposureInterval=2, doseBins=8, doseBinWidth=0.25))
    assert (p.exposureInterval, p.doseBins, p.doseBinWidth) == (2, 8, 0.25)
    # enabled behind age, tags and routes; then the field
    assert p.ctx.calls == [("locate",), ("age_enable", 4, 5), ("tag_enable", 1, 2), ("sink_groups",), ("route_enable",),
                           ("exposure_enable", 0.25, 8), ("exposure_field", field)]
    del p.ctx.calls[:]
    assert p.advect(0.0, 7 * dt) == 7
    cdt = 7 * dt / 7
    A2, A1 = ("accumulate", cdt * 2), ("accumulate", cdt * 1)
    K, Rs = ("sink",), ("respawn",)
    samples = [("sample",), ("age_sample",), ("tag_sample",), ("route_sample",)]
    assert p.ctx.calls == [("step", 2), A2, ("step", 2), A2, K, Rs] + samples + [("step", 2), A2, ("step", 1)]
    assert p._exposure_pending == cdt * 1                                    # carried into the next advect
    del p.ctx.calls[:]
    assert p.advect(7 * dt, 1 * dt) == 1
    assert p.ctx.calls == [("step", 1), ("accumulate", cdt * 1 + dt), K, Rs] + samples
    assert p.dose_distribution() == ("dose_distribution",) and p.doses() == ("doses",)
    # interval 3 against a recycle interval of 2: whichever comes first ends the launch
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=2, sinkCells=[0], exposureField=field, exposureInterval=3))
    assert (q.doseBins, q.doseBinWidth) == (1, 1.0)
    del q.ctx.calls[:]
    q.advect(0.0, 6 * dt)
    assert q.ctx.calls == [("step", 2), K, Rs, ("step", 1), ("accumulate", dt * 2 + dt * 1), ("step", 1), K, Rs,
                           ("step", 2), ("accumulate", dt * 1 + dt * 2), K, Rs]
    # without the key: the calls of today
    r = api.CudaParticles(None, np.zeros((4, 3)), base)
    assert r.exposureField is None
    del r.ctx.calls[:]
    r.advect(0.0, 7 * dt)
    assert r.ctx.calls == [("step", 4), K, Rs] + samples + [("step", 3)]


# ------------------------------------------------------------------------------------------------ 6. the entries
def test_6_lib_and_header_declare_the_entries():
    for name in ENTRIES:
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[0] is C.c_void_p
    assert L.SIGNATURES["cpf_exposure_enable"][1][1:] == [C.c_double, C.c_int32]
    assert L.SIGNATURES["cpf_exposure_accumulate"][1][1:] == [C.c_double]
    assert L.SIGNATURES["cpf_set_exposure_field"][1][1:] == [C.c_void_p, C.c_int64]
    assert L.SIGNATURES["cpf_exposure_bins_host"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p])
    text = open(api.__file__.replace("api.py", "../include/cpf.h")).read()
    for name in ENTRIES:
        assert "int %s(cpf_context* ctx" % name in text, name
    assert "int cpf_exposure_bins_host(const double* dose, int64_t n, double binWidth, int32_t nBins, int32_t* bin);" in text


def test_6_null_contexts_are_refused_without_a_device():
    lib = L.load()
    out = np.zeros(4, np.float64)
    p = api._ptr
    assert lib.cpf_exposure_enable(None, 1.0, 1) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_disable(None) == L.CPF_ERR_ARG
    assert lib.cpf_set_exposure_field(None, p(out), 4) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_accumulate(None, 1.0) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_reset(None) == L.CPF_ERR_ARG
    assert lib.cpf_get_dose_histogram(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_get_doses(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_get_doses(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_exposure_set_doses(None, p(out)) == L.CPF_ERR_ARG
