"""TEST INFRASTRUCTURE ONLY.  A CPU statement of the whole "VertexVelocity" cycle (cpf_step with CPF_STEP_VERTEX_VELOCITY),
composed from the oracle's stage functions the way tests/golden/make_golden.py builds vertex_box.npz:

    advect_vertex -> [kick, D > 0] -> locate -> [reflect, unless NO_REFLECT] -> move

on the reference's own tet walk (``lib``: oracle.TetWalk, the plain-C restatement that exists wherever build() ran, or
oracle.RefLib -- strict or contracting -- where oracle/_ref was built), plus the meshes, vertex fields, clouds and time steps
that tests/test_vertex_cycle_host.py and tests/test_gpu_vertex_cycle.py share.

States.  The tet walk keeps tet ids and w, the library keeps cell ids: ``state()`` maps (id, w) to what cpf_get_particles
reports -- the cell (id // 12) of a live particle, CPF_CELL_LOST (-1) for one that left in its last cycle (negative id, w still 1,
moved to where its displacement ends), CPF_CELL_FROZEN (-2) for one the next advect switched off (negative id, w = 0).

Checkpoints.  Rounding grows along a trajectory in an interpolated field: the strict and the contracting build of the reference
itself stay within 1e-5 of the domain diagonal of each other for 20 cycles at DT_FRACTION of a cell per cycle and not for 60
(tests/test_vertex_cycle_host.py asserts the former on every mesh here; docs/experiments.md has the figures), so CHECKPOINTS ends at 20."""
from __future__ import annotations

import functools

import numpy as np

CHECKPOINTS = (1, 6, 20)
REL_TOL = 1e-5                       # the project's contract: |dx| / domain diagonal (tests/test_gpu_goldens.py)
DT_FRACTION = 0.6                    # dt = DT_FRACTION * cbrt(min cell volume) / max |vertex U|
# The kick's bars are those of tests/test_gpu_nonplanar.py::test_walk_matches_cellwalk_on_the_derived_mesh (D = 1.5e-5, dt = 0.01,
# cells of 1 / 8): D is scaled so that sqrt(2 D dt) is the same share of a cell here as there
KICK_D0, KICK_DT0, KICK_H0 = 1.5e-5, 0.01, 0.125
KICK_SEED = 9


class Case:
    """One mesh with its tet decomposition (oracle.tetmesh.poly_to_tets), a vertex field and the time step / diffusion of the tests."""

    def __init__(self, name, mesh, field_seed=None, vertex_u=None, dt=None):
        from oracle.tetmesh import poly_to_tets
        self.name, self.mesh = name, mesh
        self.centres, vols = mesh.cell_centres_volumes()
        self.pos, self.tets, _, _ = poly_to_tets(mesh, self.centres, np.zeros((mesh.n_cells, 3)))
        assert self.tets.shape[0] == 12 * mesh.n_cells                   # all-hex
        self.vU = np.random.default_rng(field_seed).normal(size=self.pos.shape) if vertex_u is None else np.asarray(vertex_u)
        self.lo, self.hi = mesh.bounds()
        self.diag = float(np.linalg.norm(self.hi - self.lo))
        self.umax = float(np.abs(self.vU).max())
        self.h = float(np.cbrt(vols.min()))
        self.dt = DT_FRACTION * self.h / self.umax if dt is None else float(dt)
        self.D = KICK_D0 * (self.h / KICK_H0) ** 2 * (KICK_DT0 / self.dt)
        self._tables = {}

    def tables(self, lib):
        key = (type(lib).__name__, getattr(lib, "lib", None) and lib.lib._name)
        if key not in self._tables:
            self._tables[key] = lib.tables(self.pos, self.tets, np.zeros((self.tets.shape[0], 3)))
        return self._tables[key]


def _block(seed):
    from test_oracle_random import _case
    return _case(seed)[1]


def _graded():
    from cudaparticlesfoam_amd.cases import box_mesh
    return box_mesh(12, 7, 5, lower=(0.0, 0.0, 0.0), upper=(0.3, 0.05, 0.02), grading=(4.0, 0.3, 2.0))


def _thin():
    from cudaparticlesfoam_amd.cases import box_mesh
    return box_mesh(6, 5, 1)


def _pitz():
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    return pz.pitzdaily_mesh()


BLOCK_A_SEED, BLOCK_B_SEED = 168, 18     # sheared, graded blocks of test_oracle_random._case: 4 x 3 x 2 = 24 and 96 cells
# name -> (mesh builder, seed of the vertex field, cloud sizes compared with the CPU)
MESHES = {
    "block A": (lambda: _block(BLOCK_A_SEED), 101, (3000, 3137, 1, 65)),    # 24 cells: LOOKUP switches at 128 * 24 = 3072
    "block B": (lambda: _block(BLOCK_B_SEED), 102, (4000,)),
    "thin box": (_thin, 103, (4000,)),                                    # one cell thick in z (fold_z under the kick)
    "graded box": (_graded, 104, (4000,)),
    "pitzDaily": (_pitz, 105, (4000,)),
}
BLOCK_A_CELLS = 24


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    build, seed, _ = MESHES[name]
    return Case(name, build(), field_seed=seed)


@functools.lru_cache(maxsize=None)
def _cellwalk():
    from oracle import oracle as O
    O.build()
    return O.CellWalk()


@functools.lru_cache(maxsize=None)
def cloud(name, n, seed=7, n_outside=True):
    """(xyz [n][3], cell0 [n]): uniform random points located inside the mesh; a handful (indices OUTSIDE_AT below n) are
    given cell -1 from the start, as a caller's own initial locate might."""
    c, cw = case(name), _cellwalk()
    t = cw.build(c.mesh)
    rng = np.random.default_rng(seed + 1000 * n)
    xyz = np.empty((0, 3)); cell = np.empty(0, np.int32)
    while xyz.shape[0] < n:
        p = rng.uniform(c.lo, c.hi, size=(2 * n + 64, 3))
        k = cw.locate_initial(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), t, nthreads=cw.max_threads)
        xyz = np.concatenate([xyz, p[k >= 0]]); cell = np.concatenate([cell, k[k >= 0]])
    xyz, cell = np.ascontiguousarray(xyz[:n]), cell[:n].astype(np.int32)
    if n_outside:
        cell[[i for i in OUTSIDE_AT if i < n and n > 1]] = -1
    xyz.setflags(write=False); cell.setflags(write=False)
    return xyz, cell


OUTSIDE_AT = (5, 64, 130, 1001, 2999)        # (64: the first lane of a second tile)


@functools.lru_cache(maxsize=None)
def normals(n, step, seed):
    """CellWalk.normal3(gid, step, seed) for gid = 0 .. n-1: the kick's deviates as the kernels key them."""
    cw = _cellwalk()
    out = np.array([cw.normal3(g, step, seed) for g in range(n)]).reshape(n, 3)
    out.setflags(write=False)
    return out


def state(P, ids, tets_per_cell=12):
    """What cpf_get_particles reports for the tet walk's (id, w): cell, CPF_CELL_LOST or CPF_CELL_FROZEN."""
    ids = np.asarray(ids)
    return np.where(ids >= 0, ids // tets_per_cell, np.where(P[:, 3] != 0, -1, -2)).astype(np.int32)


class Snapshot:
    def __init__(self, P, ids, vels):
        self.P, self.ids, self.vels = P.copy(), ids.copy(), vels.copy()
        self.state = state(P, ids)


def run_cpu(lib, c: Case, xyz, cell0, checkpoints=CHECKPOINTS, D=0.0, reflect=True, seed=KICK_SEED, ids0=None):
    """{k: Snapshot after k cycles}.  Start ids are 12 * cell0 followed by the library's bary_query (ids0: given instead);
    the kick's step counter runs over all cycles from 0, gid = arange(n)."""
    m = c.tables(lib)
    n = xyz.shape[0]
    P = np.ones((n, 4)); P[:, :3] = xyz
    if ids0 is None:
        ids = (12 * np.asarray(cell0)).astype(np.int32)
        lib.bary_query(P, ids, m, nthreads=lib.max_threads)
    else:
        ids = np.array(ids0, np.int32)
    vels = np.zeros((n, 4)); disps = np.zeros((n, 4))
    sigma = np.sqrt(2.0 * D * c.dt)
    out, step = {"ids0": ids.copy()}, 0
    for k in checkpoints:
        while step < k:
            lib.advect_vertex(P, ids, vels, disps, c.dt, m, c.vU, nthreads=lib.max_threads)
            if D > 0.0:
                disps[:, :3] += sigma * normals(n, step, seed)
            lib.locate(P, ids, disps, m, nthreads=lib.max_threads)
            if reflect:
                lib.reflect(P, ids, disps, vels, m, nthreads=lib.max_threads)
            lib.move(P, disps, ids, nthreads=lib.max_threads)
            step += 1
        out[int(k)] = Snapshot(P, ids, vels)
    return out


def rel(a, b, diag):
    return np.sqrt(((a[:, :3] - b[:, :3]) ** 2).sum(1)) / diag


def inward_distance(mesh, xyz, cells):
    """Smallest signed distance of each point to the planes of the cell it claims (>= 0: inside); the tables are CellWalk.build's."""
    cw = _cellwalk()
    t = cw.build(mesh)
    out = np.full(xyz.shape[0], np.inf)
    ns = np.diff(t.cell_off)
    assert (ns == 6).all()
    for s in range(6):
        pl = t.planes[t.cell_off[cells] + s]
        out = np.minimum(out, -(pl[:, 3] - (pl[:, :3] * xyz).sum(1)))
    return out
