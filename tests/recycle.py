"""TEST INFRASTRUCTURE ONLY.  The recycling cloud (include/cpf.h "recycling") stated in numpy: the respawn position on the oracle's
Philox, the sink as a set operation, a brute-force locate over the mesh tables, and a whole recycled run on ``CellWalk``.  Shared by
tests/test_recycle_host.py (no GPU) and tests/test_gpu_recycle.py."""
from __future__ import annotations

import functools

import numpy as np

KEY1 = 0x43504632                  # "CPF2": the respawn stream's second key word (the kick's is ...31)
N = 10_007                         # a multiple of none of 64, 256 and 1024


@functools.lru_cache(maxsize=None)
def cellwalk():
    from oracle import oracle as O
    O.build()
    return O.CellWalk()


def positions(seed, gids, epoch, lower, upper):
    """[n][3]: Philox4x32-7, counter (gid low, gid high, epoch, 0), key (seed, KEY1); u_k = w_k * 2^-32; lower + u * (upper -
    lower), every operation a numpy operation of its own -- one rounding each."""
    cw = cellwalk()
    gids = np.asarray(gids, np.int64).reshape(-1)
    w = np.empty((gids.size, 3), np.uint32)
    for i, g in enumerate(gids):
        g = int(g)
        w[i] = cw.philox(np.array([g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, epoch, 0], np.uint32),
                         np.array([seed & 0xFFFFFFFF, KEY1], np.uint32), rounds=7)[:3]
    u = w.astype(np.float64) * 2.0 ** -32
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    span = upper - lower
    off = u * span
    return lower + off


def sink(cell, sink_cells):
    """the sink as a set operation: who sits in a sink cell is lost"""
    return np.where(np.isin(cell, sink_cells), -1, cell).astype(np.int32)


def brute_locate(xyz, tables):
    """The initial-locate rule without a bin grid: the lowest-numbered cell whose every plane has the point on its inner side,
    d - n.P <= 0, else -1.  tables = (cell_off, planes, nbr) of ``Context.mesh_tables()``.  On axis-aligned boxes n.P has one
    non-zero term and d - n.P is one rounding, as in the kernel's fma chain."""
    off, planes, _ = tables
    xyz = np.asarray(xyz, np.float64)
    found = np.full(xyz.shape[0], -1, np.int32)
    for c in range(off.size - 2, -1, -1):                       # descending: the lowest id is written last
        pl = planes[off[c]:off[c + 1]]
        d = pl[None, :, 3] - (pl[None, :, 0] * xyz[:, None, 0] + pl[None, :, 1] * xyz[:, None, 1] + pl[None, :, 2] * xyz[:, None, 2])
        found[(d <= 0.0).all(1)] = c
    return found


def cpu_recycled_run(mesh, tables, U, xyz, cell0, dt, rounds, cycles, sink_cells, box, seed):
    """K rounds of: `cycles` cycles of the unkicked CPU statement (CellWalk.step_given(xi = None)), the sink, a respawn of every dead
    slot at epoch = round.  gid = index.  Returns (xyz, cell, absorbed, drawn, placed, respawns per particle)."""
    cw = cellwalk()
    t = cw.build(mesh)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    absorbed = drawn = placed = 0
    times = np.zeros(cell.size, np.int64)
    for epoch in range(rounds):
        cw.step_given(x, y, z, cell, dt, cycles, t, U, 0.0, None, nthreads=cw.max_threads)
        after = sink(cell, sink_cells)
        absorbed += int((after != cell).sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        p = positions(seed, dead, epoch, box[0], box[1])
        where = brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
        times[dead[where >= 0]] += 1
    return np.stack([x, y, z], 1), cell, absorbed, drawn, placed, times


# ------------------------------------------------------------------------------------------------ the whole recycled runs (D = 0)
SEED = 9


class Run:
    """A recycled run on a mesh of axis-aligned boxes (plane distances exact): the flow goes along +x, the sink is the last x
    layer of cells, the source box lies at the inlet end."""

    def __init__(self, name):
        from cudaparticlesfoam_amd.cases import box_mesh
        from cudaparticlesfoam_amd.cases import pitzdaily as pz
        rng = np.random.default_rng(31)
        self.name = name
        if name == "graded box":                                   # tests/browniancycle.py's: 720 boxes, LOOKUP 6
            self.mesh = box_mesh(10, 9, 8, upper=(1.0, 0.9, 0.8), grading=(2.0, 1.0, 0.5))
            U = rng.normal(size=(self.mesh.n_cells, 3)) * 0.3
            U[:, 0] = 1.0 + 0.2 * rng.normal(size=self.mesh.n_cells)
            # the box sticks out at x < 0: one draw in eleven stays dead, is frozen by the next launch and drawn again
            self.dt, self.box, self.sort_interval = 0.05, ((-0.02, 0.05, 0.05), (0.2, 0.85, 0.75)), 3
        else:                                                      # "thin box": box_mesh(6, 5, 1), a field without z: the flat walk
            self.mesh = box_mesh(6, 5, 1)
            U = rng.normal(size=(self.mesh.n_cells, 3)) * 0.3
            U[:, 0] = 1.0 + 0.2 * rng.normal(size=self.mesh.n_cells)
            U[:, 2] = 0.0
            self.dt, self.box, self.sort_interval = 0.2, ((0.0, 0.25, 0.125), (1.0, 4.75, 0.875)), 50
        self.U = np.ascontiguousarray(U)
        self.rounds, self.cycles = 12, 3
        lo, hi = self.mesh.bounds()
        centres, _ = self.mesh.cell_centres_volumes()
        self.sink_cells = np.nonzero(centres[:, 0] >= centres[:, 0].max() - 1e-9)[0].astype(np.int32)
        self.xyz = pz.uniform_points(4321, N, tuple(lo), tuple(hi))

    def cpu(self, tables, cell0):
        return cpu_recycled_run(self.mesh, tables, self.U, self.xyz, cell0, self.dt, self.rounds, self.cycles, self.sink_cells,
                                self.box, SEED)


@functools.lru_cache(maxsize=None)
def run(name) -> Run:
    return Run(name)
