"""TEST INFRASTRUCTURE ONLY.  The flux table (include/cpf.h "flux table") stated in numpy: what a refresh makes of a source table
under a velocity field -- one numpy operation per rounding, the quanta scaled with ldexp, the running sums in uint64 -- and a
whole recycled run like ``sourcepatch.cpu_recycled_run`` whose table and field change every round.  Shared by
tests/test_inflow_host.py (no GPU) and tests/test_gpu_inflow.py."""
from __future__ import annotations

import numpy as np

import recycle as R
import sourcepatch as SP

TWO32 = 2 ** 32


def lengths(rec):
    """len of every record from its e1, e2 (columns 3..8), in the table builder's order of operations"""
    r = np.asarray(rec, np.float64).reshape(-1, 16)
    e1, e2 = r[:, 3:6], r[:, 6:9]
    c = np.empty_like(e1)
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        p = e1[:, b] * e2[:, d]
        q = e1[:, d] * e2[:, b]
        c[:, a] = p - q
    sq = c * c
    s = sq[:, 0] + sq[:, 1]
    s = s + sq[:, 2]
    return np.sqrt(s)


def flux(rec, cells, U, depth_scale):
    """(span [k], hi [k] uint32, q [k] uint64, empty) of the table rec [k][16] under U [nCells][3]; cells: the owner cell per INPUT
    triangle (column 14 of a record is its triangle).  empty: no inflow anywhere -- then the three arrays are None."""
    r = np.asarray(rec, np.float64).reshape(-1, 16)
    u = np.asarray(U, np.float64).reshape(-1, 3)[np.asarray(cells, np.int64)[r[:, 14].astype(np.int64)]]
    with np.errstate(all="ignore"):
        a = u[:, 0] * r[:, 9]
        b = u[:, 1] * r[:, 10]
        c = u[:, 2] * r[:, 11]
        ab = a + b
        un = ab + c
        v = np.where(un > 0.0, un, 0.0)                                 # (a NaN compares false)
        area = lengths(r) / 2.0
        w = area * v
        w = np.where(np.isfinite(w), w, 0.0)
        span = np.float64(depth_scale) * v
        span = np.where(np.isfinite(span), span, 0.0)
    wmax = w.max()
    if wmax == 0.0:
        return None, None, None, True
    _, E = np.frexp(wmax)                                               # wmax = f * 2^E, f in [0.5, 1)
    # (exact wherever the result is >= 1; below 1 its floor is 0 however the subnormal result was rounded)
    q = np.floor(np.ldexp(w, 32 - int(E))).astype(np.uint64)
    assert int(q.max()) >= 2 ** 31 and int(q.max()) < TWO32
    Q = np.cumsum(q, dtype=np.uint64)
    last = Q[-1]
    share = Q.astype(np.float64) / np.float64(last)
    scaled = share * 4294967296.0
    b = np.minimum(np.floor(scaled), 4294967296.0).astype(np.uint64)
    b = np.where(Q == last, np.uint64(TWO32), b)
    hi = (np.maximum(b, np.uint64(1)) - np.uint64(1)).astype(np.uint32)
    return span, hi, q, False


def refreshed(rec, hi, cells, U, depth_scale):
    """(rec, hi) after one refresh: hi replaced, column 13 replaced where depth_scale > 0 -- or both as they were, without inflow"""
    span, new_hi, _, empty = flux(rec, cells, U, depth_scale)
    if empty:
        return np.array(rec, np.float64), np.array(hi, np.uint32)
    out = np.array(rec, np.float64)
    if depth_scale > 0:
        out[:, 13] = span
    return out, new_hi


def soup(seed, m, spread=1.0):
    """m random triangles [m][3][3] in the unit cube, sizes spread over a factor of `spread`"""
    rng = np.random.default_rng(seed)
    a = rng.random((m, 1, 3))
    size = spread ** -rng.random((m, 1, 1)) if spread != 1.0 else 1.0
    return a + (rng.random((m, 3, 3)) - 0.5) * 0.2 * size


def cpu_followed_run(mesh, tables, fields, xyz, cell0, dt, rounds, cycles, sink_cells, rec, hi, cells, depth_scale, seed,
                     refresh=None):
    """``sourcepatch.cpu_recycled_run`` with a source that follows U: round e runs under fields[e], on the table refreshed from it
    by ``refresh(rec, hi, cells, U, depth_scale) -> (rec, hi)`` (default: the numpy statement).  Returns (xyz, cell, absorbed,
    drawn, placed)."""
    refresh = refresh or refreshed
    cw = R.cellwalk()
    t = cw.build(mesh)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    absorbed = drawn = placed = 0
    for epoch in range(rounds):
        rec, hi = refresh(rec, hi, cells, fields[epoch], depth_scale)
        cw.step_given(x, y, z, cell, dt, cycles, t, fields[epoch], 0.0, None, nthreads=cw.max_threads)
        after = R.sink(cell, sink_cells)
        absorbed += int((after != cell).sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        p = SP.positions(seed, dead, epoch, rec, hi)
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
    return np.stack([x, y, z], 1), cell, absorbed, drawn, placed
