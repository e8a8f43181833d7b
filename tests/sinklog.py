"""TEST INFRASTRUCTURE ONLY.  The sink log (include/cpf.h "sink log") stated in numpy: the records one ``sink_apply`` appends, from
what ``get_particles()`` returned before the apply -- positions and parent cells in particle-id order --, the sink cells, the
context's cycle counter, the index of the apply and the id-keyed tables of the groups that are on (``None``: off).  Shared by
tests/test_sinklog_host.py (no GPU) and tests/test_gpu_sinklog.py."""
from __future__ import annotations

import numpy as np

from cudaparticlesfoam_amd.api import SINK_LOG_DTYPE

AGE, TAGS, EXPOSURE, ZONES = 1, 2, 4, 8      # bits of `fields`
OFF = 0xFF


def records(xyzw, cell, sink_cells, now, apply, births=None, origins=None, sink_group_of=None, doses=None, last=None):
    """The records of one apply, sorted by id (so a concatenation over applies in order is sorted by (apply, id)).
    ``sink_group_of`` is the sink group of every cell of the mesh as given (read at the sink's cells only); tagging is on when
    ``origins`` is not None, and then it is needed."""
    xyzw, cell = np.asarray(xyzw, np.float64), np.asarray(cell)
    ids = np.nonzero(np.isin(cell, sink_cells) & (cell >= 0))[0]
    r = np.zeros(ids.size, SINK_LOG_DTYPE)
    r["id"] = ids
    r["apply"] = apply
    r["cycle"] = np.uint32(now)
    r["x"], r["y"], r["z"] = xyzw[ids, 0], xyzw[ids, 1], xyzw[ids, 2]
    r["cell"] = cell[ids]
    fields = 0
    if births is not None:
        r["age"] = (np.uint32(now) - np.asarray(births, np.uint32)[ids]).astype(np.uint32)     # the unsigned 32-bit difference
        fields |= AGE
    r["origin"], r["group"], r["zone"] = OFF, OFF, OFF
    if origins is not None:
        r["origin"] = np.asarray(origins, np.uint8)[ids]
        r["group"] = np.asarray(sink_group_of, np.uint8)[cell[ids]]
        fields |= TAGS
    if doses is not None:
        r["dose"] = np.asarray(doses, np.float64)[ids]
        fields |= EXPOSURE
    if last is not None:
        r["zone"] = np.asarray(last, np.uint8)[ids]
        fields |= ZONES
    r["fields"] = fields
    return r


def group_of_cells(n_cells, sink_cells, groups):
    """the sink group of every cell of the mesh as given, from ``set_sink_groups``' two lists (cells outside the sink: 0)"""
    g = np.zeros(n_cells, np.uint8)
    g[np.asarray(sink_cells)] = np.asarray(groups, np.uint8)
    return g


def same(got, want):
    """byte equality of two record arrays, with the first differing records in the message"""
    assert got.dtype == SINK_LOG_DTYPE and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64))[0]
        raise AssertionError((np.unique(bad).size, got[bad[:3]], want[bad[:3]]))
