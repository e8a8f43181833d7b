"""TEST INFRASTRUCTURE ONLY.  Tracer age (include/cpf.h "tracer age") stated in numpy: births as an array indexed by particle id, the
residence-time histogram as a bincount over the absorbed, the age field as two bincounts per parent cell, and the recycled runs of
tests/recycle.py carried through with births and the histogram.  Shared by tests/test_age_host.py (no GPU) and
tests/test_gpu_age.py."""
from __future__ import annotations

import functools

import numpy as np

import recycle as R

BIN_CYCLES, N_BINS = 3, 8            # of the recycled runs: a round is 3 cycles, so bin b = absorbed after b whole rounds


def ages(now, births):
    """uint32 arithmetic modulo 2^32, as int64"""
    return ((np.uint64(now) + np.uint64(2 ** 32) - np.asarray(births, np.uint32).astype(np.uint64)) % np.uint64(2 ** 32)).astype(np.int64)


def rtd(age, bin_cycles, n_bins):
    """absorptions per bin: age // bin_cycles, the last bin open-ended"""
    age = np.asarray(age, np.int64)
    return np.bincount(np.minimum(age // bin_cycles, n_bins - 1), minlength=n_bins).astype(np.uint64)


def field(parent, age, n_cells):
    """(age sum, count) per parent cell over the live particles (parent >= 0), int64 sums"""
    parent, age = np.asarray(parent), np.asarray(age, np.int64)
    live = parent >= 0
    count = np.bincount(parent[live], minlength=n_cells).astype(np.uint64)
    total = np.zeros(n_cells, np.int64)
    np.add.at(total, parent[live], age[live])
    return total.astype(np.uint64), count


def cpu_recycled_run(mesh, tables, U, xyz, cell0, dt, rounds, cycles, sink_cells, box, seed, bin_cycles, n_bins, limited_round=None):
    """tests/recycle.py's cpu_recycled_run carrying the births and the residence-time histogram: tracking starts at cycle 0 with
    everybody born then; a round is `cycles` cycles, the sink (the absorbed add their age to the histogram), a respawn at epoch =
    round which stamps EVERY dead slot with the cycle count before it draws.  limited_round: in that round the respawn takes only the
    first half of the dead slots in ARRAY order -- which is id order here: the caller's run must not re-sort (gid = index).
    Returns a dict."""
    cw = R.cellwalk()
    t = cw.build(mesh)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    births = np.zeros(cell.size, np.uint32)
    hist = np.zeros(n_bins, np.uint64)
    absorbed = drawn = placed = now = 0
    times_absorbed = np.zeros(cell.size, np.int64)
    left_dead, limited_count, mid_ages = None, None, None
    for epoch in range(rounds):
        cw.step_given(x, y, z, cell, dt, cycles, t, U, 0.0, None, nthreads=cw.max_threads)
        now += cycles
        after = R.sink(cell, sink_cells)
        hit = after != cell
        hist += rtd(ages(now, births[hit]), bin_cycles, n_bins)
        times_absorbed[hit] += 1
        absorbed += int(hit.sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        births[dead] = now
        if epoch == limited_round:
            limited_count = dead.size // 2
            left_dead = dead[limited_count:]
            dead = dead[:limited_count]
        p = R.positions(seed, dead, epoch, box[0], box[1])
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
        if epoch == limited_round:
            mid_ages = np.where(cell >= 0, ages(now, births), -1)
    return dict(mid_ages=mid_ages,xyz=np.stack([x, y, z], 1), cell=cell, absorbed=absorbed, drawn=drawn, placed=placed, births=births, hist=hist,
                now=now, ages=np.where(cell >= 0, ages(now, births), -1), times_absorbed=times_absorbed, left_dead=left_dead,
                limited_count=limited_count)


# which round of a run takes a limited respawn: the thin box never re-sorts in its 36 cycles (sort_interval 50), so its array order
# is the id order; the graded box re-sorts every round and recycles without a limit
LIMITED_ROUND = {"graded box": None, "thin box": 5}


@functools.lru_cache(maxsize=None)
def cpu(name):
    """the recycled run `name` of tests/recycle.py with births, from its brute-force initial locate"""
    from cudaparticlesfoam_amd import api
    r = R.run(name)
    t = api.build_mesh_tables_host(r.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    cell0 = R.brute_locate(r.xyz, tables)
    return cpu_recycled_run(r.mesh, tables, r.U, r.xyz, cell0, r.dt, r.rounds, r.cycles, r.sink_cells, r.box, R.SEED, BIN_CYCLES, N_BINS,
                            LIMITED_ROUND[name])
