"""TEST INFRASTRUCTURE ONLY.  Exposure (include/cpf.h "exposure") stated in numpy: the doses as an array indexed by particle id, one
add per live particle and call, each operation a numpy operation of its own (one rounding each); the bin rule; the histogram as an
``np.add.at`` over the particles ``numpy.isin`` calls absorbed; and the recycled runs of tests/recycle.py carried through with
doses, accumulating every ``interval`` cycles.  Shared by tests/test_exposure_host.py (no GPU) and tests/test_gpu_exposure.py."""
from __future__ import annotations

import functools

import numpy as np

import recycle as R

BIN_WIDTH, N_BINS = 0.25, 16         # of the recycled runs: their doses spread over the sixteen bins, the last one open-ended


def accumulate(dose, cell, rate, scale, n_cells=None):
    """dose[id] = dose[id] + scale * rate[cell[id]] for every live id (0 <= cell < n_cells); cell is in id order.  Returns a new
    array; dead ids keep their bits."""
    dose, cell, rate = np.array(dose, np.float64), np.asarray(cell), np.asarray(rate, np.float64)
    n_cells = rate.size if n_cells is None else n_cells
    live = (cell >= 0) & (cell < n_cells)
    step = np.float64(scale) * rate[cell[live]]              # one rounding
    dose[live] = dose[live] + step                           # ... and another
    return dose


def bins(dose, bin_width, n_bins):
    """k = dose * (1 / bin_width); n_bins - 1 where k >= n_bins - 1, else int(k)"""
    inv = np.float64(1.0) / np.float64(bin_width)
    k = np.asarray(dose, np.float64) * inv
    top = k >= np.float64(n_bins - 1)
    return np.where(top, n_bins - 1, np.where(top, 0.0, k).astype(np.int64)).astype(np.int32)


def histogram(cell, sink_cells, dose, bin_width, n_bins, origin=None, group_of_cell=None, n_origins=1, n_sinks=1):
    """uint64 [n_origins][n_sinks][n_bins]: 1 for every particle numpy.isin calls absorbed, at (its origin, the group of its cell,
    the bin of its dose); everything in id order; origin / group_of_cell None: 0"""
    cell = np.asarray(cell)
    hit = np.isin(cell, sink_cells)
    h = np.zeros((n_origins, n_sinks, n_bins), np.uint64)
    o = np.zeros(int(hit.sum()), np.int64) if origin is None else np.asarray(origin, np.int64)[hit]
    g = np.zeros(int(hit.sum()), np.int64) if group_of_cell is None else np.asarray(group_of_cell, np.int64)[cell[hit]]
    np.add.at(h, (o, g, bins(np.asarray(dose, np.float64)[hit], bin_width, n_bins)), np.uint64(1))
    return h


def run_rate(mesh):
    """the non-uniform rate field of the recycled runs: grows along x, zero in every fifth cell"""
    centres, _ = mesh.cell_centres_volumes()
    lo, hi = mesh.bounds()
    rate = 0.25 + (centres[:, 0] - lo[0]) / (hi[0] - lo[0]) + 0.5 * np.abs(np.sin(7.0 * centres[:, 1]))
    rate[::5] = 0.0
    return np.ascontiguousarray(rate)


def cpu_recycled_run(mesh, tables, U, xyz, cell0, dt, rounds, cycles, sink_cells, box, seed, rate, interval, bin_width, n_bins):
    """tests/recycle.py's cpu_recycled_run carrying the doses and the dose histogram, one cycle at a time: after every `interval`-th
    cycle everybody live adds (interval * dt, summed cycle by cycle as CudaParticles.advect sums it) x (the rate of the cell it is
    in); a round is `cycles` cycles (a multiple of interval), then the sink -- the absorbed add the bin of their dose to the
    histogram --, then a respawn at epoch = round which sets the dose of EVERY dead slot to 0 before it draws.  Returns a dict
    with the state at every recycle point."""
    assert cycles % interval == 0
    cw = R.cellwalk()
    t = cw.build(mesh)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    dose = np.zeros(cell.size, np.float64)
    hist = np.zeros((1, 1, n_bins), np.uint64)
    absorbed, pending, points = 0, 0.0, []
    for epoch in range(rounds):
        for k in range(cycles):
            cw.step_given(x, y, z, cell, dt, 1, t, U, 0.0, None, nthreads=cw.max_threads)
            pending += dt * 1
            if (k + 1) % interval == 0:
                dose = accumulate(dose, cell, rate, pending)
                pending = 0.0
        hist += histogram(cell, sink_cells, dose, bin_width, n_bins)
        after = R.sink(cell, sink_cells)
        absorbed += int((after != cell).sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        dose[dead] = 0.0
        p = R.positions(seed, dead, epoch, box[0], box[1])
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        points.append(dict(dose=dose.copy(), doses=np.where(cell >= 0, dose, -1.0), hist=hist.copy(), cell=cell.copy()))
    return dict(xyz=np.stack([x, y, z], 1), cell=cell, absorbed=absorbed, points=points)


@functools.lru_cache(maxsize=None)
def cpu(name, interval):
    """the recycled run `name` of tests/recycle.py with doses, from its brute-force initial locate"""
    from cudaparticlesfoam_amd import api
    r = R.run(name)
    t = api.build_mesh_tables_host(r.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    cell0 = R.brute_locate(r.xyz, tables)
    return cpu_recycled_run(r.mesh, tables, r.U, r.xyz, cell0, r.dt, r.rounds, r.cycles, r.sink_cells, r.box, R.SEED, run_rate(r.mesh),
                            interval, BIN_WIDTH, N_BINS)
