"""CPU: the host side of the tracer age (include/cpf.h "tracer age"): conditions on the CPU statement of the recycled runs that
tests/test_gpu_age.py compares against (a comparison of empty histograms would show nothing), the numpy statement's own arithmetic,
the calls ``CudaParticles`` makes with ``ageBins``, argument handling without a device."""
import numpy as np
import pytest

import age as A
import recycle as R
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api


# ------------------------------------------------------------------------------------------------ the statement's arithmetic
def test_ages_are_modular_and_the_last_bin_is_open():
    births = np.array([0, 5, 10, 11, 2 ** 32 - 1], np.uint32)
    assert A.ages(10, births).tolist() == [10, 5, 0, 2 ** 32 - 1, 11]                # a birth after `now` wraps
    assert A.rtd([0, 2, 3, 5, 6, 8, 9, 1000], 3, 4).tolist() == [2, 2, 2, 2]
    assert A.rtd([0, 7], 1, 1).tolist() == [2]
    s, c = A.field(np.array([0, 2, 2, -1, 0]), np.array([1, 10, 2 ** 32 - 1, 99, 4]), 4)
    assert s.tolist() == [5, 0, 2 ** 32 + 9, 0] and c.tolist() == [2, 0, 2, 0]


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_the_cpu_statement_of_the_recycled_runs_has_residence_times(oracle_libs, name):
    """On the runs of tests/recycle.py (12 rounds of 3 cycles, binCycles = 3): at least 200 absorptions in at least 4 distinct bins,
    at least one particle absorbed twice -- and without the limited round the run is tests/recycle.py's own."""
    r = R.run(name)
    assert (r.rounds, r.cycles, A.BIN_CYCLES) == (12, 3, 3)
    c = A.cpu(name)
    hist = c["hist"]
    print("MEASURED %s | absorbed %d | histogram %s | absorbed twice or more: %d | dead at the end: %d"
          % (name, c["absorbed"], hist.tolist(), int((c["times_absorbed"] >= 2).sum()), int((c["cell"] < 0).sum())))
    assert int(hist.sum()) == c["absorbed"] >= 200
    assert int((hist > 0).sum()) >= 4
    assert (c["times_absorbed"] >= 2).any()
    assert c["now"] == 36 and c["births"].max() <= 36 and (c["births"][c["times_absorbed"] == 0] % 3 == 0).all()
    live = c["cell"] >= 0
    assert np.array_equal(c["ages"][live], 36 - c["births"][live].astype(np.int64)) and (c["ages"][~live] == -1).all()
    if A.LIMITED_ROUND[name] is None:
        t = api.build_mesh_tables_host(r.mesh)
        tables = (t["cell_off"], t["planes"], t["nbr"])
        xyz, cell, absorbed, drawn, placed, _ = r.cpu(tables, R.brute_locate(r.xyz, tables))
        assert np.array_equal(xyz.view(np.int64), c["xyz"].view(np.int64)) and np.array_equal(cell, c["cell"])
        assert (absorbed, drawn, placed) == (c["absorbed"], c["drawn"], c["placed"])
        assert (~live).any()                                                 # the box sticks out: dead slots at the end, age -1
    else:
        assert c["left_dead"].size > 0 and r.sort_interval > r.rounds * r.cycles      # array order = id order: no re-sort


# ------------------------------------------------------------------------------------------------ CudaParticles
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
    def rtd(self, dt): return ("rtd", dt)
    def mean_age(self, dt): return ("mean_age", dt)
    def close(self): pass


def test_age_bins_alone_are_accepted_and_take_no_samples(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    for key in ("ageBins", "ageBinCycles"):
        assert key not in api.DICT_DEFAULTS                                  # this library's own keys
    dt = 2.0 ** -13
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, ageBins=16))
    assert (p.ageBins, p.ageBinCycles) == (16, 1)                            # no recycleInterval: bins of one cycle
    assert p.advect(0.0, 7 * dt) == 7
    # the chunks are the ones of a run without the key: nothing ends a fused launch, nothing is sampled
    assert p.ctx.calls == [("locate",), ("age_enable", 1, 16), ("step", 7)]
    assert api._next_chunk(0, 7, 10, 0, False, False, 0) == 7
    assert p.rtd() == ("rtd", dt) and p.mean_age() == ("mean_age", dt)
    # off by default: no call at all
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=2, occupancyInterval=4, sinkCells=[0]))
    q.advect(0.0, 4 * dt)
    assert not any(c[0].startswith("age") for c in q.ctx.calls)


def test_age_sample_follows_the_occupancy_sample_after_recycling(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    dt = 2.0 ** -13
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=2, occupancyInterval=4, sinkCells=[0], ageBins=5))
    assert p.ageBinCycles == 2                                               # defaults to the recycle interval
    p.advect(0.0, 6 * dt)
    K, Rs, S, AS = ("sink",), ("respawn",), ("sample",), ("age_sample",)
    assert p.ctx.calls == [("locate",), ("age_enable", 2, 5), ("step", 2), K, Rs, ("step", 2), K, Rs, S, AS, ("step", 2), K, Rs]
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=2, ageBins=5, ageBinCycles=7))
    assert q.ctx.calls == [("locate",), ("age_enable", 7, 5)]


# ------------------------------------------------------------------------------------------------ without a device
def test_null_contexts_are_refused_without_a_device():
    lib = L.load()
    out = np.zeros(4, np.uint64)
    p = api._ptr
    assert lib.cpf_age_enable(None, 1, 1) == L.CPF_ERR_ARG
    assert lib.cpf_age_disable(None) == L.CPF_ERR_ARG
    assert lib.cpf_age_sample(None) == L.CPF_ERR_ARG
    assert lib.cpf_age_reset(None) == L.CPF_ERR_ARG
    assert lib.cpf_get_age_histogram(None, p(out), 4) == L.CPF_ERR_ARG
    assert lib.cpf_get_age_field(None, p(out), p(out), None) == L.CPF_ERR_ARG
    assert lib.cpf_get_ages(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_age_get_births(None, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_age_set_births(None, p(out)) == L.CPF_ERR_ARG
