"""TEST INFRASTRUCTURE ONLY.  Zones (include/cpf.h "zones") stated in numpy on integers: the sample, the leave and the stamp on
(cell, last, zone_of, sink cells), everything in particle-id order -- ``cell`` is what ``get_particles()`` returns (parent ids),
``zone_of`` the caller's map over the mesh as given, ``last`` the byte table with 0xFF for outside.  The table is
[n_zones + 1][n_zones + 1] uint64, index n_zones = outside.  Shared by tests/test_zones_host.py (no GPU) and
tests/test_gpu_zones.py."""
from __future__ import annotations

import numpy as np

OUTSIDE = 0xFF


def table(n_zones):
    return np.zeros((n_zones + 1, n_zones + 1), np.uint64)


def row_of(last, n_zones):
    """the table's row of a byte of ``last``: 0xFF is row n_zones"""
    last = np.asarray(last, np.int64)
    return np.where(last == OUTSIDE, n_zones, last)


def sample(flow, last, cell, zone_of, n_zones):
    """for every live id (cell >= 0): flow[row_of(last)][zone_of[cell]] += 1, last = zone_of[cell]; dead ids: nothing.  Returns
    (flow, last), new arrays."""
    flow, last, cell = np.array(flow, np.uint64), np.array(last, np.uint8), np.asarray(cell)
    live = cell >= 0
    z = np.asarray(zone_of, np.int64)[cell[live]]
    np.add.at(flow, (row_of(last[live], n_zones), z), np.uint64(1))
    last[live] = z.astype(np.uint8)
    return flow, last


def leave(flow, last, cell, sink_cells, n_zones):
    """flow[row_of(last)][n_zones] += 1 for every id numpy.isin calls absorbed; last is not written.  Returns flow, a new array."""
    flow = np.array(flow, np.uint64)
    hit = np.isin(np.asarray(cell), sink_cells)
    np.add.at(flow, (row_of(np.asarray(last)[hit], n_zones), n_zones), np.uint64(1))
    return flow


def stamp(last, cell):
    """last = 0xFF for every candidate of a respawn (cell < 0).  Returns a new array."""
    last = np.array(last, np.uint8)
    last[np.asarray(cell) < 0] = OUTSIDE
    return last


def x_slabs(mesh, n_zones):
    """a zone map of n_zones slabs of equal width along x"""
    centres, _ = mesh.cell_centres_volumes()
    lo, hi = mesh.bounds()
    z = np.floor((centres[:, 0] - lo[0]) / (hi[0] - lo[0]) * n_zones).astype(np.int32)
    return np.clip(z, 0, n_zones - 1).astype(np.int32)
