"""CPU: the sink log (include/cpf.h "sink log") without a device -- the numpy statement of tests/sinklog.py against a loop over
one particle at a time, the record's layout in ``api.SINK_LOG_DTYPE``, in ``_lib.SinkRecord`` and in the header, the entries in
``_lib`` and in the header, what ``CudaParticles`` refuses before any context exists and the calls it makes with ``sinkLog``."""
import ctypes as C
import re

import numpy as np
import pytest

import sinklog as S
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

ENTRIES = ("cpf_sink_log_enable", "cpf_sink_log_disable", "cpf_sink_log_clear", "cpf_sink_log_counts", "cpf_sink_log_read")
OFFSETS = dict(id=0, apply=8, cycle=12, x=16, y=24, z=32, dose=40, age=48, cell=52, origin=56, group=57, zone=58, fields=59,
               reserved=60)


# ------------------------------------------------------------------------------------------------ 1. the statement
def _loop(xyzw, cell, sink_cells, now, apply, births, origins, group_of, doses, last):
    out = []
    for i in range(cell.size):                                               # ids ascending: sorted by id
        if cell[i] < 0 or int(cell[i]) not in sink_cells:
            continue
        r = np.zeros((), api.SINK_LOG_DTYPE)
        r["id"], r["apply"], r["cycle"] = i, apply, now
        r["x"], r["y"], r["z"] = xyzw[i, 0], xyzw[i, 1], xyzw[i, 2]
        r["cell"] = cell[i]
        r["age"] = (now - int(births[i])) % 2 ** 32 if births is not None else 0
        r["origin"] = origins[i] if origins is not None else 0xFF
        r["group"] = group_of[cell[i]] if origins is not None else 0xFF
        r["dose"] = doses[i] if doses is not None else 0.0
        r["zone"] = last[i] if last is not None else 0xFF
        r["fields"] = ((births is not None) * 1 + (origins is not None) * 2 + (doses is not None) * 4 + (last is not None) * 8)
        out.append(r)
    return np.array(out, api.SINK_LOG_DTYPE).reshape(-1)


@pytest.mark.parametrize("on", range(16))
def test_1_the_statement_against_a_loop(on):
    rng = np.random.default_rng(on)
    n, n_cells = 300, 40
    sink_cells = np.array([3, 17, 38, 39], np.int32)
    xyzw = rng.normal(size=(n, 4))
    cell = rng.integers(0, n_cells, size=n).astype(np.int32)
    cell[rng.random(n) < 0.1] = -1
    cell[rng.random(n) < 0.05] = -2
    now = 7
    births = rng.integers(0, 12, size=n).astype(np.uint32) if on & 1 else None            # some born "after" now: the difference wraps
    origins = rng.integers(0, 5, size=n).astype(np.uint8) if on & 2 else None
    group_of = S.group_of_cells(n_cells, sink_cells, [0, 1, 2, 1])
    doses = rng.uniform(0.0, 3.0, size=n) if on & 4 else None
    last = np.where(rng.random(n) < 0.3, 0xFF, rng.integers(0, 6, size=n)).astype(np.uint8) if on & 8 else None
    got = S.records(xyzw, cell, sink_cells, now, 4, births, origins, group_of, doses, last)
    want = _loop(xyzw, cell, set(sink_cells.tolist()), now, 4, births, origins, group_of, doses, last)
    S.same(got, want)
    assert got.size == int(np.isin(cell, sink_cells).sum()) > 10 and (np.diff(got["id"]) > 0).all()
    assert (got["fields"] == on).all() and (got["apply"] == 4).all() and not got["reserved"].any()
    if on & 1:
        assert (got["age"] > 2 ** 31).any() and (got["age"] < 8).any()
    with pytest.raises(AssertionError):
        bad = want.copy(); bad["dose"][1] = -0.0 if bad["dose"][1] == 0.0 else 0.0
        S.same(got, bad)


def test_1_the_statement_on_a_case_written_by_hand():
    xyzw = np.arange(20.0).reshape(5, 4)
    cell = np.array([0, 2, -1, 3, 2], np.int32)
    r = S.records(xyzw, cell, np.array([2, 3], np.int32), 9, 1, births=np.array([0, 4, 0, 10, 9], np.uint32))
    assert r["id"].tolist() == [1, 3, 4] and r["cell"].tolist() == [2, 3, 2] and r["age"].tolist() == [5, 2 ** 32 - 1, 0]
    assert r["x"].tolist() == [4.0, 12.0, 16.0] and r["z"].tolist() == [6.0, 14.0, 18.0] and r["dose"].tolist() == [0.0] * 3
    assert r["origin"].tolist() == r["group"].tolist() == r["zone"].tolist() == [0xFF] * 3 and r["fields"].tolist() == [1] * 3
    assert r["cycle"].tolist() == [9] * 3 and r["apply"].tolist() == [1] * 3


# ------------------------------------------------------------------------------------------------ 2. the record
def test_2_the_dtype_is_the_record_of_the_header():
    dt = api.SINK_LOG_DTYPE
    assert dt.itemsize == 64 and set(dt.names) == set(OFFSETS)
    for name, off in OFFSETS.items():
        assert dt.fields[name][1] == off, name
    kinds = {name: dt.fields[name][0].str for name in dt.names}
    assert kinds == dict(id="<i8", apply="<u4", cycle="<u4", x="<f8", y="<f8", z="<f8", dose="<f8", age="<u4", cell="<i4",
                         origin="|u1", group="|u1", zone="|u1", fields="|u1", reserved="<u4")
    assert S.OFF == 0xFF and (S.AGE, S.TAGS, S.EXPOSURE, S.ZONES) == (1, 2, 4, 8)
    assert (L.SINK_LOG_AGE, L.SINK_LOG_TAGS, L.SINK_LOG_EXPOSURE, L.SINK_LOG_ZONES) == (1, 2, 4, 8)


def test_2_the_ctypes_structure_agrees_with_the_dtype():
    assert C.sizeof(L.SinkRecord) == 64
    dt = api.SINK_LOG_DTYPE
    assert [f[0] for f in L.SinkRecord._fields_] == sorted(dt.names, key=lambda k: dt.fields[k][1])
    for name, ctype in L.SinkRecord._fields_:
        field = getattr(L.SinkRecord, name)
        assert field.offset == dt.fields[name][1] and field.size == dt.fields[name][0].itemsize, name
        assert np.dtype(ctype) == dt.fields[name][0].newbyteorder("="), name
    # one record written through ctypes reads the same through numpy
    r = L.SinkRecord(id=-5, apply=3, cycle=77, x=1.5, y=-2.5, z=3.25, dose=0.125, age=9, cell=-1, origin=2, group=1, zone=0xFF,
                     fields=15, reserved=0)
    a = np.frombuffer(bytes(r), dt)[0]
    assert (a["id"], a["apply"], a["cycle"], a["x"], a["y"], a["z"], a["dose"], a["age"], a["cell"]) == (-5, 3, 77, 1.5, -2.5, 3.25,
                                                                                                         0.125, 9, -1)
    assert (a["origin"], a["group"], a["zone"], a["fields"], a["reserved"]) == (2, 1, 0xFF, 15, 0)


def test_2_the_header_declares_the_record_with_these_offsets():
    text = open(L.HEADER_PATH).read()
    m = re.search(r"typedef struct cpf_sink_record \{(.*?)\} cpf_sink_record;", text, re.S)
    assert m
    body = m.group(1)
    for name, off in OFFSETS.items():
        assert re.search(r"\b%s\b[^\n]*/\*\s+%d\s" % (name, off), body), name
    order = [re.sub(r"/\*.*", "", line) for line in body.splitlines()]
    names = re.findall(r"\b([a-z]+)\s*[,;]", " ".join(order))
    assert names == sorted(OFFSETS, key=OFFSETS.get)                         # declared in the order of their offsets
    assert "static_assert(sizeof(cpf_sink_record) == 64" in text


# ------------------------------------------------------------------------------------------------ 3. the entries
def test_3_lib_and_header_declare_the_entries():
    for name in ENTRIES:
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[0] is C.c_void_p
    assert L.SIGNATURES["cpf_sink_log_enable"][1][1:] == [C.c_int64]
    assert L.SIGNATURES["cpf_sink_log_counts"][1][1:] == [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert L.SIGNATURES["cpf_sink_log_read"][1][1:] == [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    text = open(L.HEADER_PATH).read()
    for name in ENTRIES:
        assert "int %s(cpf_context* ctx" % name in text, name
    assert set(ENTRIES) <= set(L.header_symbols())
    assert "unspecified" in text[text.index("typedef struct cpf_sink_record"):text.index("int cpf_sink_log_enable")]


def test_3_null_contexts_are_refused_without_a_device():
    lib = L.load()
    rec = np.zeros(2, api.SINK_LOG_DTYPE)
    k = C.c_int64()
    assert lib.cpf_sink_log_enable(None, 4) == L.CPF_ERR_ARG
    assert lib.cpf_sink_log_disable(None) == L.CPF_ERR_ARG
    assert lib.cpf_sink_log_clear(None) == L.CPF_ERR_ARG
    assert lib.cpf_sink_log_counts(None, C.byref(k), C.byref(k)) == L.CPF_ERR_ARG
    assert lib.cpf_sink_log_read(None, api._ptr(rec), 2, C.byref(k)) == L.CPF_ERR_ARG


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
    def zone_enable(self, n_zones): self.calls.append(("zone_enable", n_zones))
    def set_zone_map(self, zone): self.calls.append(("zone_map",))
    def zone_sample(self): self.calls.append(("zone_sample",))
    def sink_log_enable(self, capacity): self.calls.append(("log_enable", capacity))
    def sink_log_counts(self): self.calls.append(("log_counts",)); return (3, 2)
    def sink_log_drain(self): self.calls.append(("log_drain",)); return "records"
    def close(self): pass


class _NoDevice:
    """Stands in for ``api.Context``: any use is a failure"""

    def __init__(self, device=0):
        raise AssertionError("a context was made")


def test_4_what_cuda_particles_refuses_before_any_context_exists(monkeypatch):
    monkeypatch.setattr(api, "Context", _NoDevice)
    assert "sinkLog" not in api.DICT_DEFAULTS                                # this library's own key
    U = np.zeros((4, 3))
    base = dict(recycleInterval=2, sinkCells=[0, 1])
    bad = [dict(base, sinkLog=-1), dict(base, sinkLog=2.0), dict(base, sinkLog=2.5), dict(base, sinkLog="64"),
           dict(base, sinkLog=True), dict(base, sinkLog=None), dict(sinkLog=8), dict(recycleInterval=2, sinkLog=8),
           dict(sinkCells=[0, 1], sinkLog=8)]
    for d in bad:
        with pytest.raises(ValueError):
            api.CudaParticles(None, U, d)
    for ok in (dict(base, sinkLog=8), dict(base, sinkLog=np.int64(8)), dict(base, sinkLog=0), dict(sinkLog=0)):
        with pytest.raises(AssertionError, match="a context was made"):
            api.CudaParticles(None, U, ok)


def test_4_the_log_is_enabled_behind_zones_and_never_drained_by_the_run(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    dt = 2.0 ** -13
    base = dict(dt=dt, recycleInterval=4, occupancyInterval=4, sinkCells=[0, 1])
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(base, zoneMap=[0, 1, 1, 2], zoneInterval=2, sinkLog=1000))
    assert p.sinkLog == 1000
    assert p.ctx.calls == [("locate",), ("zone_enable", 3), ("zone_map",), ("log_enable", 1000)]
    del p.ctx.calls[:]
    assert p.advect(0.0, 7 * dt) == 7
    Zs, K, Rs, Sm = ("zone_sample",), ("sink",), ("respawn",), ("sample",)
    assert p.ctx.calls == [("step", 2), Zs, ("step", 2), Zs, K, Rs, Sm, ("step", 2), Zs, ("step", 1)]      # as without the key
    del p.ctx.calls[:]
    assert p.sink_log() == ("records", 2)
    assert p.ctx.calls == [("log_counts",), ("log_drain",)]                  # the dropped count is read before the drain clears it
    # the log alone: the calls of a run without it, and one enable
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(base, sinkLog=np.int32(5)))
    assert q.ctx.calls == [("locate",), ("log_enable", 5)] and type(q.sinkLog) is int
    del q.ctx.calls[:]
    q.advect(0.0, 7 * dt)
    assert q.ctx.calls == [("step", 4), K, Rs, Sm, ("step", 3)]
    # without the key, or with 0: the calls of today
    for d in (base, dict(base, sinkLog=0)):
        r = api.CudaParticles(None, np.zeros((4, 3)), d)
        assert r.sinkLog == 0 and r.ctx.calls == [("locate",)]
        del r.ctx.calls[:]
        r.advect(0.0, 7 * dt)
        assert r.ctx.calls == [("step", 4), K, Rs, Sm, ("step", 3)]
