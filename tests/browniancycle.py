"""TEST INFRASTRUCTURE ONLY.  The kicked cycle (cpf_step with D > 0) against a CPU statement, bit for bit.

The kick's deviates are a pure function of (gid, step, seed) -- Philox + Box-Muller, csrc/cpf_walk.h normal3 -- evaluated with the
fp32 hardware transcendentals on the device and with libm in oracle/cellwalk.c: they differ in their last bits, and that is all
that ever stood between the kicked kernels and a CPU result.  So the deviates are taken FROM THE DEVICE as data, by two independent
routes, and handed to ``CellWalk.step_given`` (oracle/cellwalk.c, cw_step_given), which runs the same cycle -- advect, kick, [fold_z],
walk, reflect, move -- on them:

* staged route: ``StagedCloud.cudaBrownianMotion(dt = 1, D = 0.5, step)`` on zeroed displacements with w = 1.  sigma = sqrt(2 * 0.5 * 1)
  is exactly 1 and fma(1, xi, 0) is xi: disps[:, :3] ARE the deviates of gid = index;
* fused route: a mesh of ONE cell spanning +-10, U = 0, every particle at the origin, one kicked cycle with dt = 1, D = 0.5: the
  positions afterwards are the deviates (|xi| < 6.77 by construction of the transform, so nobody meets a wall), for any gid array --
  the only route for gids >= 2^32 -- and for gid == NULL.

This module holds what tests/test_brownian_cycle_host.py (no GPU: libm's deviates) and tests/test_gpu_brownian_cycle.py share: the
meshes with their fields, time steps and diffusion coefficients, the clouds, the CPU run and the two extractors.

The UNKICKED cycle (D = 0) is the same statement without deviates (``step_given(xi = None)``: ``run_cpu(..., xi=None)``) and needs no
extractor; tests/test_plain_cycle_host.py and tests/test_gpu_plain_cycle.py run it on the same meshes and clouds, in the case's
field and in three more (``Case.U0`` with exact zeros, ``Case.Uflat`` without a z component, ``Case.Ucorner`` towards a corner),
with the reference results cached here (``plain_ref``) and the conditions on whole 64-particle tiles stated here (``tiles``)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

CHECKPOINTS = (1, 6, 20)
STEP0 = 1000                       # the kick's step counter at the first cycle of every step_dev run
SEED = 9
CELL_LOST, CELL_FROZEN = -1, -2
# lanes that BEGIN the first launch lost / frozen (64: the first lane of a second tile), in every cloud that has them
START_DEAD = {5: CELL_LOST, 64: CELL_FROZEN, 130: CELL_LOST}


def _block_a():
    from test_oracle_random import _case
    return _case(168)[1]


def _graded_box():
    from cudaparticlesfoam_amd.cases import box_mesh
    return box_mesh(10, 9, 8, upper=(1.0, 0.9, 0.8), grading=(2.0, 1.0, 0.5))


def _refined_box():
    from cudaparticlesfoam_amd.cases import refined_box
    return refined_box(10, 9, 8, (-0.2, 0.0, 0.1), (1.0, 0.9, 0.9), ((0.1, 0.2, 0.3), (0.7, 0.7, 0.7)), grading=(2.0, 1.0, 0.5))[0]


def _cut_corners():
    from cudaparticlesfoam_amd.cases.polygons import cut_corner_box
    return cut_corner_box(11, 8, 3, every=4)[0]


def _chamfered():
    from cudaparticlesfoam_amd.cases.polygons import chamfered_box
    return chamfered_box(12, 9, 3, 1)[0]


def _thin_box():
    from cudaparticlesfoam_amd.cases import box_mesh
    return box_mesh(6, 5, 1)


def _pitz():
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    return pz.pitzdaily_mesh()


# name -> (mesh, seed of the cell field, advective step and sigma = sqrt(2 D dt), both as a share of h = cbrt(smallest cell volume)).
# sigma is a sizeable share of the smallest cell everywhere: that is what sends particles across faces, into walls twice in a cycle
# and through three cells (hard_paths below says how often, and the tests assert it).
MESHES = {
    "block A": (_block_a, 201, 0.5, 0.45),               # 24 sheared cells: LOOKUP 0 / 1 / 4 by cloud size
    "graded box": (_graded_box, 202, 0.5, 0.6),          # 720 boxes: LOOKUP 6, "box_records" 0 -> 1
    "refined box": (_refined_box, 203, 0.5, 0.6),        # 2:1-refined boxes, face groups: LOOKUP 11, 3, 5
    "cut corners": (_cut_corners, 204, 0.4, 0.3),        # seven-slot cells (two records), prisms, face groups: LOOKUP 2
    "chamfered": (_chamfered, 205, 0.4, 0.3),            # ten-slot cells: LOOKUP 2
    "thin box": (_thin_box, 206, 0.4, 0.45),             # one cell thick in z: fold_z
    "pitzDaily": (_pitz, None, None, None),              # the tutorial's mesh, its analytic step flow, dt = 1e-4, 100 x its D
}
MESHES_3D = ("block A", "graded box", "refined box", "cut corners", "chamfered")
MESHES_THIN = ("thin box", "pitzDaily")


class Case:
    def __init__(self, name):
        build, seed, u_frac, s_frac = MESHES[name]
        self.name, self.mesh = name, build()
        centres, vols = self.mesh.cell_centres_volumes()
        self.h = float(np.cbrt(vols.min()))
        if name == "pitzDaily":
            from cudaparticlesfoam_amd.cases import pitzdaily as pz
            self.U = np.ascontiguousarray(pz.analytic_step_u(self.mesh, centres))
            self.U[:, 2] = 0.3 * np.random.default_rng(207).normal(size=self.mesh.n_cells)       # a z component for the fold to flip
            self.dt, self.D = 1e-4, 1.5e-3
        else:
            self.U = np.random.default_rng(seed).normal(size=(self.mesh.n_cells, 3))
            self.dt = u_frac * self.h / float(np.abs(self.U).max())
            self.D = (s_frac * self.h) ** 2 / (2.0 * self.dt)
        self.U2 = np.ascontiguousarray(self.U[::-1] * np.array([1.0, -1.0, 0.5]))                # the refreshed field of part (c)
        self.sigma = float(np.sqrt(2.00 * self.D * self.dt))                                      # as both sides compute it
        self.lo, self.hi = self.mesh.bounds()

    @functools.cached_property
    def U0(self):
        """The second field, with exact zeros (the unkicked cycle's zero-denominator skips, tests/test_gpu_plain_cycle.py): the
        first third of the cell ids at rest -- all three components zero, +0.0 and -0.0 mixed --, the last third with U.x exactly
        +-0.0, the rest the case's random field."""
        n = self.mesh.n_cells
        rng = np.random.default_rng(7000 + n)
        U0 = self.U.copy()
        U0[:n // 3] = rng.choice([0.0, -0.0], size=(n // 3, 3))
        U0[n - n // 3:, 0] = rng.choice([0.0, -0.0], size=n // 3)
        U0.setflags(write=False)
        return U0

    @functools.cached_property
    def Uflat(self):
        """the case's field without a z component: the flat walk's (a mesh extruded in z)"""
        U = self.U.copy()
        U[:, 2] = 0.0
        U.setflags(write=False)
        return U

    @functools.cached_property
    def Ucorner(self):
        """one velocity everywhere, towards the corner at self.hi: the cloud piles up against three walls, whole tiles reflect"""
        U = np.tile(float(np.abs(self.U).max()) * np.array([1.0, 0.9, 0.8]), (self.mesh.n_cells, 1))
        U.setflags(write=False)
        return U

    def field(self, which):
        return {"U": self.U, "U0": self.U0, "Uflat": self.Uflat, "U2": self.U2, "Ucorner": self.Ucorner}[which]

    @functools.cached_property
    def tables(self):
        return cellwalk().build(self.mesh)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name)


@functools.lru_cache(maxsize=None)
def cellwalk():
    from oracle import oracle as O
    O.build()
    return O.CellWalk()


@functools.lru_cache(maxsize=None)
def cloud(name, n, sort=False, seed=11):
    """(xyz [n][3], cell0 [n], gid [n]): uniform random points inside the mesh with the cell the CPU statement's initial locate
    gives them, as drawn (gid = index) or -- sort -- ordered by cell as the product keeps its clouds, gid = the index the point
    was drawn with: a permutation.  The lanes of START_DEAD (array positions; those below n) begin lost / frozen."""
    c, cw = case(name), cellwalk()
    rng = np.random.default_rng(seed + 1000 * n)
    xyz = np.empty((0, 3)); cell = np.empty(0, np.int32)
    while xyz.shape[0] < n:
        p = rng.uniform(c.lo, c.hi, size=(2 * n + 64, 3))
        k = cw.locate_initial(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), c.tables, nthreads=cw.max_threads)
        xyz = np.concatenate([xyz, p[k >= 0]]); cell = np.concatenate([cell, k[k >= 0]])
    xyz, cell = xyz[:n], cell[:n].astype(np.int32)
    gid = np.argsort(cell, kind="stable").astype(np.int64) if sort else np.arange(n, dtype=np.int64)
    xyz, cell = np.ascontiguousarray(xyz[gid]), np.ascontiguousarray(cell[gid])
    for i, state in START_DEAD.items():
        if i < n and n > 1:
            cell[i] = state
    for a in (xyz, cell, gid):
        a.setflags(write=False)
    return xyz, cell, gid


def libm_deviates(gids, step0, cycles, seed=SEED):
    """[cycles][n][3]: cw_normal3(gid, step0 + c, seed), the deviates as oracle/cellwalk.c draws them (libm)"""
    cw = cellwalk()
    return np.stack([cw.normal3_many(gids, step0 + c, seed) for c in range(cycles)])


class Snapshot:
    def __init__(self, x, y, z, cell, vel, stats):
        self.xyz = np.stack([x, y, z], 1); self.cell = cell.copy(); self.vel = vel.copy()
        self.stats = stats                      # [cells visited, reflections, lost, live particle-cycles] since the last checkpoint


def run_cpu(c: Case, xyz, cell0, xi=None, reflect=1, zfold=0, checkpoints=CHECKPOINTS, refresh_after=None, U=None):
    """({k: Snapshot after k cycles}, diag [cycles][n][3]) of CellWalk.step_given on the deviates xi [cycles][n][3] -- None: the
    unkicked cycle (D = 0) --; refresh_after: the checkpoint behind which the field becomes c.U2; U: the field (None: c.U)."""
    cw = cellwalk()
    n = xyz.shape[0]
    x, y, z = (xyz[:, k].copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    vel = np.zeros((n, 3))
    diag = np.zeros((max(checkpoints), n, 3), np.int32)
    out, done, U = {}, 0, (c.U if U is None else U)
    for k in checkpoints:
        live = 0
        st = np.zeros(3, np.int64)
        for cyc in range(done, k):                                       # cycle by cycle: the live count is the fourth counter
            live += int((cell >= 0).sum())
            st += cw.step_given(x, y, z, cell, c.dt, 1, c.tables, U, c.sigma, None if xi is None else xi[cyc:cyc + 1],
                                reflect=reflect, zfold=zfold, vel_out=vel, nthreads=cw.max_threads, diag=diag[cyc:cyc + 1])
        done = k
        out[k] = Snapshot(x, y, z, cell, vel, [int(st[0]), int(st[1]), int(st[2]), live])
        if refresh_after == k:
            U = c.U2
    return out, diag


def hard_paths(diag):
    """What the cycles of a reflecting run went through, from step_given's per-particle-cycle counters: the shares of live
    particle-cycles that crossed a face / met a wall / were mirrored about a z plane, and the counts of the rare ones (a cycle's
    visits are its face crossings + its wall hits + the visit in which the segment ends)."""
    visits, walls, folds = diag[..., 0], diag[..., 1], diag[..., 2]
    live = max(int((visits > 0).sum()), 1)
    return dict(crossing=float((visits - walls > 1).sum()) / live, reflecting=float((walls > 0).sum()) / live,
                two_walls=int((walls >= 2).sum()), three_hops=int((visits - walls >= 4).sum()),
                folded=float((folds > 0).sum()) / live, folded_twice=int((folds >= 2).sum()), live=live)


# ------------------------------------------------------------------------------------------------ the unkicked cycle (D = 0)
@functools.lru_cache(maxsize=None)
def flat_cloud(n):
    """cloud("thin box", n, sort = True) with z == -0.0 for every fifth particle: on the z = 0 plane, where the flat walk (no z
    component in the field) leaves it for good and the first cycle rewrites the zero's sign"""
    xyz, cell0, gid = cloud("thin box", n, sort=True)
    xyz = xyz.copy()
    xyz[::5, 2] = -0.0
    xyz.setflags(write=False)
    return xyz, cell0, gid


@functools.lru_cache(maxsize=None)
def plain_ref(name, field, n, sort, reflect, refresh_after=None, flat=False):
    """(snapshots, diag) of the CPU statement WITHOUT the kick (step_given(xi = None)) for cloud(name, n, sort) -- flat:
    flat_cloud(n) -- in the field c.field(field); computed once and shared: nobody writes into it"""
    xyz, cell0, _ = flat_cloud(n) if flat else cloud(name, n, sort=sort)
    c = case(name)
    return run_cpu(c, xyz, cell0, None, reflect=reflect, refresh_after=refresh_after, U=c.field(field))


def tiles(a):
    """[tiles][64]: the whole 64-particle tiles of a per-particle array in storage order (array positions 64 k ... 64 k + 63)"""
    return a[:(a.shape[0] // 64) * 64].reshape(-1, 64)


def at_rest_tiles(c: Case, cell0):
    """the tiles whose 64 lanes all sit in at-rest cells of c.U0 (its first third of the cell ids)"""
    t = tiles(cell0)
    return np.nonzero(((t >= 0) & (t < c.mesh.n_cells // 3)).all(1))[0]


def zero_x_crossing_tiles(c: Case, cell0, diag):
    """the tiles whose 64 lanes all begin in U.x == +-0 cells of c.U0 (its last third of the cell ids) and of which a lane crosses a
    face in the first cycle -- a y or a z face on a mesh of boxes: nobody there moves in x"""
    t = tiles(cell0)
    crossed = tiles((diag[0, :, 0] - diag[0, :, 1] > 1))
    return np.nonzero((t >= c.mesh.n_cells - c.mesh.n_cells // 3).all(1) & crossed.any(1))[0]


def most_lanes_of_a_tile_reflecting(diag):
    """the largest number of lanes of one tile that meet a wall in one and the same cycle"""
    return max(int(tiles(diag[cyc, :, 1] > 0).sum(1).max()) for cyc in range(diag.shape[0]))


# ------------------------------------------------------------------------------------------------ the device side
class DeviceCloud:
    """x, y, z, cell, gid, vel of n particles in device memory through the C-ABI's own helpers (cpf_dev_alloc, cpf_copy_*)."""

    def __init__(self, ctx, xyz, cell, gid=None):
        self.ctx, self.n = ctx, int(xyz.shape[0])
        self._p = {}
        n = self.n
        for name, nbytes in (("x", 8 * n), ("y", 8 * n), ("z", 8 * n), ("cell", 4 * n), ("gid", 8 * n), ("vel", 24 * n)):
            p = C.c_void_p()
            ctx._ck(ctx.lib.cpf_dev_alloc(ctx.h, max(nbytes, 16), C.byref(p)))
            ctx._ck(ctx.lib.cpf_dev_memset(ctx.h, p, 0, max(nbytes, 16)))
            self._p[name] = p
        self.has_gid = gid is not None
        self.put(xyz, cell, gid)

    def put(self, xyz, cell, gid=None):
        for k, name in enumerate("xyz"):
            self._put(name, np.ascontiguousarray(xyz[:, k], dtype=np.float64))
        self._put("cell", np.ascontiguousarray(cell, dtype=np.int32))
        if gid is not None:
            self._put("gid", np.ascontiguousarray(gid, dtype=np.int64))
        self.ctx._ck(self.ctx.lib.cpf_dev_memset(self.ctx.h, self._p["vel"], 0, max(24 * self.n, 16)))

    def _put(self, name, a):
        self.ctx._ck(self.ctx.lib.cpf_copy_to_device(self.ctx.h, self._p[name], a.ctypes.data_as(C.c_void_p), a.nbytes))

    def _get(self, name, shape, dtype):
        a = np.empty(shape, dtype)
        self.ctx._ck(self.ctx.lib.cpf_copy_to_host(self.ctx.h, a.ctypes.data_as(C.c_void_p), self._p[name], a.nbytes))
        return a

    def step(self, dt, D, step0, cycles, flags, store_vel=False):
        p = self._p
        self.ctx.step_dev(p["x"], p["y"], p["z"], p["cell"], p["gid"] if self.has_gid else None, p["vel"] if store_vel else None,
                          self.n, dt, D, step0, cycles, flags)

    def get(self):
        """(xyz [n][3], cell [n], vel [n][3]); synchronises"""
        n = self.n
        xyz = np.stack([self._get(k, (n,), np.float64) for k in "xyz"], 1)
        return xyz, self._get("cell", (n,), np.int32), self._get("vel", (n, 3), np.float64)

    def close(self):
        for p in self._p.values():
            self.ctx.lib.cpf_dev_free(self.ctx.h, p)
        self._p = {}


def one_cell_context(make_ctx, seed=SEED):
    """A context whose mesh is ONE cell spanning +-10 with U = 0: the fused route's"""
    from cudaparticlesfoam_amd.cases import box_mesh
    mesh = box_mesh(1, 1, 1, lower=(-10.0, -10.0, -10.0), upper=(10.0, 10.0, 10.0))
    ctx = make_ctx()
    ctx.set_mesh(mesh); ctx.set_velocity(np.zeros((1, 3))); ctx.set_seed(seed)
    return ctx


def fused_deviates(ctx, gids, n, step0, cycles):
    """[cycles][n][3] by the fused route on one_cell_context's ctx: gids an int64 array, or None for the kernels' gid == NULL
    path (gid = index)."""
    zero = np.zeros((n, 3)); cell = np.zeros(n, np.int32)
    dc = DeviceCloud(ctx, zero, cell, gids)
    out = np.empty((cycles, n, 3))
    try:
        for c in range(cycles):
            if c:
                dc.put(zero, cell)
            dc.step(1.0, 0.5, step0 + c, 1, 0)
            name = ctx.step_kernel_name(0.5, 0)
            assert "step_kernel_stream<true, true, false, " in name, name
            xyz, cl, _ = dc.get()
            assert (cl == 0).all()
            out[c] = xyz
    finally:
        dc.close()
    return out


def staged_deviates(ctx, n, step0, cycles):
    """[cycles][n][3] by the staged route (gid = index) on any context"""
    from cudaparticlesfoam_amd.api import StagedCloud
    sc = StagedCloud(ctx, n)
    out = np.empty((cycles, n, 3))
    try:
        P = np.zeros((n, 4)); P[:, 3] = 1.0
        sc.set(P, np.zeros(n, np.int32))
        for c in range(cycles):
            sc._put("disps", np.zeros((n, 4)))
            sc.cudaBrownianMotion(1.0, 0.5, step0 + c)
            out[c] = sc.disps[:, :3]
    finally:
        sc.close()
    return out
