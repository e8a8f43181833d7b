"""GPU: what the tracer ledger's entry points answer when they refuse a call -- return code and ``cpf_last_error`` text of every
refusal, as one table, compared with ``tests/golden/ledger_messages.json``.

The ledger's host entries share their refusals (cpf_ledger.cpp builds "<entry>: call <enable> first" from the entry's own name), so
a helper handed the wrong name, or a check that moved in front of another, changes a message and nothing else: no other test reads
the texts.  The table pins them.  Every call in it is refused on the host before anything is launched (a ``*_disable`` of a group
that is off does nothing, and answers CPF_OK); what does run on the device is the set-up between them: a mesh, 64 particles, and
each group switched on in turn.

The fixture was recorded from a build of the commit BEFORE the entries moved into cpf_ledger.cpp::

    python tests/test_gpu_ledger_messages.py --record --root <tree of that commit, built> [--out FILE]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ledger_messages.json")
PREFIXES = ("cpf_age_", "cpf_tag_", "cpf_route_", "cpf_exposure_", "cpf_zone_", "cpf_sink_log_")
GETTERS_AND_SETTERS = ("cpf_get_age_histogram", "cpf_get_age_field", "cpf_get_ages", "cpf_get_transfer", "cpf_get_tag_field",
                       "cpf_get_route_histogram", "cpf_get_route_field", "cpf_get_dose_histogram", "cpf_get_doses",
                       "cpf_get_zone_flows", "cpf_set_sink_groups", "cpf_set_source_origins", "cpf_set_box_origin",
                       "cpf_set_exposure_field", "cpf_set_zone_map")
N = 64                                          # particles: the smallest cloud worth the name


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def collect():
    """The table: one ``dict(state, call, code, message)`` per call, in call order; and the set of entry points called."""
    from cudaparticlesfoam_amd import _lib as L
    from cudaparticlesfoam_amd.api import Context
    from cudaparticlesfoam_amd.cases import box_mesh
    lib = L.load()
    mesh = box_mesh(6, 5, 1)                    # the "thin box" of tests/ledger.py
    nc = mesh.n_cells
    lo, hi = mesh.bounds()
    table, called = [], set()
    ctx = Context(0)
    state = [""]

    def call(what, fn, *args, refused=True):
        """one call of the table: ``fn(ctx, *args)``, or ``fn(*args)`` for the one host function"""
        called.add(fn)
        code = getattr(lib, fn)(*(args if fn.endswith("_host") else (ctx.h,) + args))
        message = (lib.cpf_last_error(ctx.h) or b"").decode()
        assert (code != L.CPF_OK) == refused, (state[0], fn, what, code, message)
        table.append(dict(state=state[0], call="%s: %s" % (fn, what), code=int(code), message=message))

    def ok(fn, *args):
        """set-up between the refusals: must succeed"""
        ctx._ck(getattr(lib, fn)(ctx.h, *args))

    def enables(what):
        call(what, "cpf_age_enable", 1, 4)
        call(what, "cpf_tag_enable", 3, 2)
        call(what, "cpf_exposure_enable", 0.5, 4)
        call(what, "cpf_zone_enable", 4)
        call(what, "cpf_sink_log_enable", 16)

    u64 = np.zeros(4096, dtype=np.uint64)       # room for every table read below, were it read
    u64b = np.zeros(4096, dtype=np.uint64)
    i64 = np.zeros(N, dtype=np.int64)
    u32 = np.zeros(N, dtype=np.uint32)
    u8 = np.zeros(N, dtype=np.uint8)
    f64 = np.zeros(N, dtype=np.float64)
    ns = C.c_int64(0)
    nsp = C.pointer(ns)
    one_cell, one_group = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    rate = np.ones(nc, dtype=np.float64)
    zone = np.zeros(nc, dtype=np.int32)
    rec = np.zeros(16 * 64, dtype=np.uint8)     # room for sixteen records of any layout up to 64 bytes
    try:
        state[0] = "1 fresh context"
        enables("no mesh")

        state[0] = "2 mesh, no cloud"
        ctx.set_mesh(mesh)
        enables("no cloud")

        state[0] = "3 mesh and located cloud, nothing on"
        ctx.seed_box(N, tuple(lo + 0.05), tuple(hi - 0.05), 1)
        assert ctx.locate_initial() == 0
        for g in ("age", "tag", "route", "exposure", "zone", "sink_log"):
            call("off already", "cpf_%s_disable" % g, refused=False)
        call("off", "cpf_age_sample")
        call("off", "cpf_age_reset")
        call("off", "cpf_get_age_histogram", _p(u64), 4)
        call("off", "cpf_get_age_field", _p(u64), _p(u64b), nsp)
        call("off", "cpf_get_ages", _p(i64))
        call("off", "cpf_age_get_births", _p(u32))
        call("off", "cpf_age_set_births", _p(u32))
        call("off", "cpf_set_sink_groups", _p(one_cell), _p(one_group), 1)
        call("off", "cpf_set_source_origins", _p(one_group), 1)
        call("off", "cpf_set_box_origin", 0)
        call("off", "cpf_tag_sample")
        call("off", "cpf_tag_reset")
        call("off", "cpf_get_transfer", _p(u64))
        call("off", "cpf_get_tag_field", _p(u64), nsp)
        call("off", "cpf_tag_get_origins", _p(u8))
        call("off", "cpf_tag_set_origins", _p(u8))
        call("age and tags off", "cpf_route_enable")
        call("off", "cpf_route_sample")
        call("off", "cpf_route_reset")
        call("off", "cpf_get_route_histogram", _p(u64))
        call("off", "cpf_get_route_field", _p(u64), _p(u64b), nsp)
        call("off", "cpf_set_exposure_field", _p(rate), nc)
        call("off", "cpf_exposure_accumulate", 1.0)
        call("off", "cpf_exposure_reset")
        call("off", "cpf_get_dose_histogram", _p(u64))
        call("off", "cpf_get_doses", _p(f64))
        call("off", "cpf_exposure_get_doses", _p(f64))
        call("off", "cpf_exposure_set_doses", _p(f64))
        call("n < 0", "cpf_exposure_bins_host", _p(f64), -1, 0.5, 4, _p(one_group))
        call("off", "cpf_set_zone_map", _p(zone), nc)
        call("off", "cpf_zone_sample")
        call("off", "cpf_zone_reset")
        call("off", "cpf_get_zone_flows", _p(u64), nsp)
        call("off", "cpf_zone_get_last", _p(u8))
        call("off", "cpf_zone_set_last", _p(u8))
        call("off", "cpf_sink_log_clear")
        call("off", "cpf_sink_log_counts", nsp, nsp)
        call("off", "cpf_sink_log_read", _p(rec), 16, nsp)
        ok("cpf_age_enable", 1, 4)
        call("only age on", "cpf_route_enable")
        ok("cpf_age_disable")
        ok("cpf_tag_enable", 3, 2)
        call("only tags on", "cpf_route_enable")
        ok("cpf_tag_disable")

        state[0] = "4 age"
        call("binCycles 0", "cpf_age_enable", 0, 4)
        call("nBins 0", "cpf_age_enable", 1, 0)
        call("nBins 4097", "cpf_age_enable", 1, 4097)
        ok("cpf_age_enable", 1, 4)
        call("nBins 5 of 4", "cpf_get_age_histogram", _p(u64), 5)
        call("null array", "cpf_get_age_histogram", None, 4)
        call("null array", "cpf_get_ages", None)
        call("null array", "cpf_age_get_births", None)
        call("null array", "cpf_age_set_births", None)
        ok("cpf_age_disable")

        state[0] = "4 tags"
        call("nOrigins 0", "cpf_tag_enable", 0, 1)
        call("nOrigins 17", "cpf_tag_enable", 17, 1)
        call("nSinks 17", "cpf_tag_enable", 1, 17)
        ok("cpf_tag_enable", 3, 2)
        for what, c, g in (("cell -1", -1, 0), ("cell nCells", nc, 0), ("group nSinks", 0, 2)):
            call(what, "cpf_set_sink_groups", _p(np.array([c], dtype=np.int32)), _p(np.array([g], dtype=np.int32)), 1)
        call("null arrays", "cpf_set_sink_groups", None, None, 1)
        call("no source", "cpf_set_source_origins", _p(one_group), 1)
        call("origin nOrigins", "cpf_set_box_origin", 3)
        bad = u8.copy()
        bad[5] = 3
        call("byte nOrigins at particle 5", "cpf_tag_set_origins", _p(bad))
        call("null array", "cpf_get_transfer", None)
        call("null array", "cpf_tag_get_origins", None)
        call("null array", "cpf_tag_set_origins", None)
        ok("cpf_tag_disable")

        state[0] = "4 routes"
        ok("cpf_age_enable", 1, 4)
        ok("cpf_tag_enable", 3, 2)
        ok("cpf_route_enable")
        call("null array", "cpf_get_route_histogram", None)
        ok("cpf_route_disable")
        ok("cpf_tag_disable")
        ok("cpf_age_disable")

        state[0] = "4 exposure"
        call("binWidth 0", "cpf_exposure_enable", 0.0, 4)
        call("binWidth inf", "cpf_exposure_enable", float("inf"), 4)
        call("binWidth nan", "cpf_exposure_enable", float("nan"), 4)
        call("nBins 0", "cpf_exposure_enable", 0.5, 0)
        ok("cpf_tag_enable", 1, 1)
        call("4097 words, tags on", "cpf_exposure_enable", 0.5, 4097)
        ok("cpf_tag_disable")
        ok("cpf_exposure_enable", 0.5, 4)
        call("nCells + 1 values", "cpf_set_exposure_field", _p(np.ones(nc + 1, dtype=np.float64)), nc + 1)
        bad = rate.copy()
        bad[3] = -1.0
        call("negative rate at cell 3", "cpf_set_exposure_field", _p(bad), nc)
        call("null array", "cpf_set_exposure_field", None, nc)
        call("scale -1", "cpf_exposure_accumulate", -1.0)
        bad = f64.copy()
        bad[7] = -0.0
        call("-0.0 at particle 7", "cpf_exposure_set_doses", _p(bad))
        call("null array", "cpf_get_dose_histogram", None)
        call("null array", "cpf_get_doses", None)
        call("null array", "cpf_exposure_get_doses", None)
        call("null array", "cpf_exposure_set_doses", None)
        ok("cpf_exposure_disable")

        state[0] = "4 zones"
        call("nZones 0", "cpf_zone_enable", 0)
        call("nZones 64", "cpf_zone_enable", 64)
        ok("cpf_zone_enable", 4)
        call("nCells + 1 values", "cpf_set_zone_map", _p(np.zeros(nc + 1, dtype=np.int32)), nc + 1)
        bad = zone.copy()
        bad[2] = 4
        call("zone nZones at cell 2", "cpf_set_zone_map", _p(bad), nc)
        call("null array", "cpf_set_zone_map", None, nc)
        bad = u8.copy()
        bad[9] = 4
        call("byte nZones at particle 9", "cpf_zone_set_last", _p(bad))
        call("null array", "cpf_zone_get_last", None)
        call("null array", "cpf_zone_set_last", None)
        ok("cpf_zone_disable")

        state[0] = "4 sink log"
        call("capacity 0", "cpf_sink_log_enable", 0)
        call("capacity 2^40", "cpf_sink_log_enable", 1 << 40)
        ok("cpf_sink_log_enable", 16)
        call("null buffer, maxRecords 1", "cpf_sink_log_read", None, 1, nsp)
        call("maxRecords -1", "cpf_sink_log_read", _p(rec), -1, nsp)
        ok("cpf_sink_log_disable")
    finally:
        ctx.close()
    return table, called


def test_every_ledger_entry_refuses_as_the_fixture_says():
    from cudaparticlesfoam_amd import _lib as L
    table, called = collect()
    ledger = {s for s in L.header_symbols() if s.startswith(PREFIXES)} | set(GETTERS_AND_SETTERS)
    assert len(ledger) == 49 and not ledger - called, sorted(ledger - called)
    with open(GOLDEN) as f:
        want = json.load(f)["table"]
    for got, exp in zip(table, want):
        assert got == exp
    assert len(table) == len(want)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="write the fixture instead of comparing with it")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the built tree whose library answers (default: this one)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    rows, _ = collect()
    if a.record:
        with open(a.out, "w") as f:                     # (one call per line)
            f.write('{"what": "(return code, cpf_last_error) of every ledger call of tests/test_gpu_ledger_messages.py",\n "table": [\n')
            f.write(",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
        print("recorded %d calls to %s" % (len(rows), a.out))
    else:
        with open(GOLDEN) as f:
            want = json.load(f)["table"]
        diff = [(g, w) for g, w in zip(rows, want) if g != w]
        print("%d calls, %d differ from %s" % (len(rows), len(diff) + abs(len(rows) - len(want)), GOLDEN))
        for g, w in diff:
            print("  got  %r\n  want %r" % (g, w))
        sys.exit(1 if diff or len(rows) != len(want) else 0)
