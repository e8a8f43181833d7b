"""GPU: the "VertexVelocity" cycle on the streaming kernel (cpf_step with CPF_STEP_VERTEX_VELOCITY, step_kernel_stream_vertex
<BROWNIAN, REFLECT, STORE_VEL, STATS, LOOKUP>) -- all 32 instantiations against a CPU statement of the whole cycle
(tests/vertexcycle.py: the reference's tet walk, stage by stage), and bit for bit against every other route the library has
to the same result.  Before each comparison the test asserts the exact name of the kernel the launch runs; part (a) on the
24-cell block meets every one of

    cpf::step_kernel_stream_vertex<false, false, false, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, false, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, false, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, false, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, true, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, true, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, true, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, false, true, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, false, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, false, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, false, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, false, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, true, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, true, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, true, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<false, true, true, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, false, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, false, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, false, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, false, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, true, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, true, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, true, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, false, true, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, false, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, false, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, false, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, false, true, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, true, false, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, true, false, 1> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, true, true, 0> (cone locate)
    cpf::step_kernel_stream_vertex<true, true, true, true, 1> (cone locate)

(test_part_a_names_are_the_32_of_the_header checks the list against the parametrisation; every run prints the name it asserted).

(a) Against the CPU.  D = 0: cells (and CPF_CELL_LOST / CPF_CELL_FROZEN, and w) identical for every particle after 1, 6 and 20
    cycles, positions within 1e-5 of the domain diagonal with zero outliers -- the project's contract, which the reference's own
    strict and contracting builds meet on these inputs for 20 cycles and not for 60 (tests/test_vertex_cycle_host.py) --; after
    the first cycle positions within 1e-13 of the diagonal and stored velocities within 1e-13 of max |vertex U|, the bar
    test_vertex_velocity_vs_reference_golden has for the advect stage.  With the kick the device deviates differ from the CPU's in
    their last bits: the bars of test_walk_matches_cellwalk_on_the_derived_mesh after 1 and 6 cycles, after 20 only that nobody is
    missing or outside the cell it claims.
(b) Inside the library everything is the same arithmetic ("same stages, same arithmetic as the five staged calls"): positions,
    w, cells and stored velocities are equal bit for bit between stats 0 and 1, single-cycle and fused launches, an unsorted and
    a sorted cloud, LOOKUP 0 and 1, the streaming kernel and the generic walk over all tets, and the five (six with the kick)
    staged calls, whose advect equals cw_advect_vertex at every cycle.  The clouds are (a)'s plus one that sits on the tet fans'
    structure and a rounding off it.  One documented exception: with the kick and reflecting walls on a mesh one cell thick in z
    the kernels mirror the end point before the walk (fold_z); there the staged calls equal the run with option "z_fold" 0.
(c) The staging loop of cycle_begin handles four distinct cells of a wave per pass: waves with exactly 4, 5-6 and 64 distinct
    cells, a ragged last tile, and lanes that start a launch lost or frozen."""
import functools
import itertools

import numpy as np
import pytest

import vertexcycle as V
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd.api import mesh_flags_host

pytestmark = pytest.mark.gpu

_B = ("false", "true")
KERNELS = frozenset(line.strip() for line in __doc__.splitlines() if line.strip().startswith("cpf::step_kernel_stream_vertex<"))


def _stream_name(kick, reflect, sv, stats, lookup):
    return "cpf::step_kernel_stream_vertex<%s, %s, %s, %s, %d> (cone locate)" % (_B[kick], _B[reflect], _B[sv], _B[stats], lookup)


def _generic_name(kick, reflect, sv):
    return "cpf::step_kernel_vertex<%s, %s, %s> (all tets)" % (_B[kick], _B[reflect], _B[sv])


def _auto_lookup(n, n_cells):
    return 1 if n < 128 * n_cells else 0                      # stream_lookup_mode: fixed compare below 128 particles per cell


def _context(c, stats, opts=()):
    from cudaparticlesfoam_amd.api import Context
    ctx = Context(0)
    ctx.set_option("stats", stats)
    for k, v in opts:
        ctx.set_option(k, v)
    ctx.set_mesh(c.mesh); ctx.set_velocity(np.zeros((c.mesh.n_cells, 3)))
    ctx.set_tets(c.pos, c.tets, 12); ctx.set_vertex_velocity(c.vU)
    ctx.set_seed(V.KICK_SEED)
    return ctx


def gpu_run(c, xyz, cell0, kick, reflect, sv, stats, expect, fused=True, sort=False, opts=(), checkpoints=V.CHECKPOINTS):
    """{k: (xyzw, cell, vel | None)} after k cycles on a fresh context (its step counter starts at 0, as the CPU's does);
    `expect`: the kernel name every launch must report."""
    D = c.D if kick else 0.0
    fl = (L.STEP_VERTEX_VELOCITY | (0 if reflect else L.STEP_NO_REFLECT) | (L.STEP_STORE_VEL if sv else 0) |
          (L.STEP_FUSE_CYCLES if fused else 0))
    out, done = {}, 0
    ctx = _context(c, stats, opts)
    try:
        ctx.set_particles(xyz, cell0)
        if sort:
            ctx.sort_by_cell()
        for k in checkpoints:
            name = ctx.step_kernel_name(D, fl)
            assert name == expect, (name, expect)
            ctx.step(c.dt, D, k - done, fl)
            done = k
            r = ctx.get_particles(want_vel=bool(sv))
            out[k] = (r[0], r[1], r[2][:, :3].copy() if sv else None)
    finally:
        ctx.close()
    print("ran %s: %s n=%d %s%s" % (expect, c.name, xyz.shape[0], "fused" if fused else "single", " sorted" if sort else ""))
    return out


def staged_run(c, xyz, cell0, kick, reflect, checkpoints=V.CHECKPOINTS):
    """The same cycles as the reference's staged calls (cudaAdvect "VertexVelocity", [cudaBrownianMotion], convexTetQuery,
    [convexWallReflect], cudaMoveParticles); at EVERY cycle the advect stage equals cw_advect_vertex on the state it was given."""
    from cudaparticlesfoam_amd.api import StagedCloud
    from oracle import oracle as O
    cw = O.CellWalk()
    D = c.D if kick else 0.0
    n = xyz.shape[0]
    P4 = np.ones((n, 4)); P4[:, :3] = xyz
    out, step = {}, 0
    ctx = _context(c, 0)
    sc = StagedCloud(ctx, n)
    try:
        sc.set(P4, cell0)
        for k in checkpoints:
            while step < k:
                Pc, ic, vc, dc = sc.particles, sc.ids, sc.vels, sc.disps
                cw.advect_vertex(Pc, ic, vc, dc, c.dt, c.tets, 12, c.pos, c.vU, nthreads=cw.max_threads)
                sc.cudaAdvect(c.dt, "VertexVelocity")
                assert np.array_equal(sc.vels, vc, equal_nan=True) and np.array_equal(sc.disps, dc, equal_nan=True), (c.name, step)
                assert np.array_equal(sc.particles, Pc, equal_nan=True), (c.name, step)
                if kick:
                    sc.cudaBrownianMotion(c.dt, D, step)             # the fused launch's step0 + c: the context starts at 0
                sc.convexTetQuery()
                if reflect:
                    sc.convexWallReflect()
                sc.cudaMoveParticles()
                step += 1
            P, ids = sc.particles, sc.ids
            out[k] = (P, np.where(ids >= 0, ids, np.where(P[:, 3] != 0, L.CELL_LOST, L.CELL_FROZEN)).astype(np.int32), sc.vels[:, :3].copy())
    finally:
        sc.close(); ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def cpu_ref(name, n, kick, reflect, checkpoints=V.CHECKPOINTS, cloud_key=None):
    from oracle import oracle as O
    O.build()
    c = V.case(name)
    xyz, cell0 = V.cloud(name, n) if cloud_key is None else _EDGE_CLOUDS[cloud_key]()
    return V.run_cpu(O.TetWalk(), c, xyz, cell0, checkpoints=checkpoints, D=c.D if kick else 0.0, reflect=bool(reflect))


def compare_with_cpu(c, ref, got, cell0, kick, reflect, sv, what, checkpoints=V.CHECKPOINTS):
    D = c.D if kick else 0.0
    started = cell0 >= 0
    for k in checkpoints:
        xyzw, cell, vel = got[k]
        s = ref[k]
        r = V.rel(xyzw, s.P, c.diag)
        same = cell == s.state
        print("MEASURED %s | %s | k=%d | max |dx|/L %.3e | states differ %d of %d" % (c.name, what, k, r.max(), (~same).sum(), same.size))
        if not kick:
            assert same.all(), (what, k, int((~same).sum()))                     # cells, lost and frozen alike
            assert np.array_equal(xyzw[:, 3], s.P[:, 3]), (what, k)              # w = 0: on both sides or on neither
            assert (r <= V.REL_TOL).all(), (what, k, r.max())
            if k == 1:
                assert np.abs(xyzw[:, :3] - s.P[:, :3]).max() <= 1e-13 * c.diag, (what, np.abs(xyzw[:, :3] - s.P[:, :3]).max())
                if sv:
                    dv = np.abs(vel[started] - s.vels[started, :3]).max() if started.any() else 0.0
                    print("MEASURED %s | %s | k=1 | max |dv|/max|U| %.3e" % (c.name, what, dv / c.umax))
                    assert dv <= 1e-13 * c.umax, (what, dv)
        elif k <= 6:
            sigma = np.sqrt(2.0 * D * c.dt * k)
            dx = np.abs(xyzw[:, :3] - s.P[:, :3])[same].max(initial=0.0)
            print("MEASURED %s | %s | k=%d | kick: equal states %.6f, max |dx|/sigma %.3e" % (c.name, what, k, same.mean(), dx / sigma))
            assert same.mean() > 0.9999 and dx < 2e-4 * sigma, (what, k, same.mean(), dx / sigma)
        else:
            # count conservation: everybody is still there, live, lost or frozen, and whoever is live is inside the cell it claims
            assert cell.shape[0] == cell0.shape[0] and ((cell >= 0) | (cell == L.CELL_LOST) | (cell == L.CELL_FROZEN)).all()
            assert np.array_equal(xyzw[:, 3] == 0, cell == L.CELL_FROZEN)
            live = cell >= 0
            if reflect:
                assert np.array_equal(live, started), (what, int(live.sum()), int(started.sum()))
            assert (cell[live] < c.mesh.n_cells).all()
            assert (V.inward_distance(c.mesh, xyzw[live, :3], cell[live]) >= -1e-9 * c.diag).all(), what
    if not reflect:
        # some particles leave during cycles 2 to 6 -- inside one fused launch -- and are frozen behind it, as on the CPU
        left = (ref[6].state < 0) & (ref[1].state >= 0)
        assert left.sum() > 0 or cell0.size < 1000                               # (the clouds of 1 and 65 need not lose anybody)
        if not kick:
            assert (got[6][1][left] < 0).all() and ((got[6][0][left, 3] == 0) == (ref[6].state[left] == L.CELL_FROZEN)).all()
            assert ((got[20][1][left] == L.CELL_FROZEN) & (got[20][0][left, 3] == 0)).all()


# ------------------------------------------------------------------------------------------------ (a)
def _part_a_cases():
    for name, (_, _, sizes) in V.MESHES.items():
        for n in sizes:
            for kick, reflect in itertools.product((0, 1), (1, 0)):
                if name == "pitzDaily" and not reflect:
                    continue
                yield name, n, kick, reflect


def _part_a_names():
    names = set()
    for name, n, kick, reflect in _part_a_cases():
        if name == "block A" and n in (3000, 3137):
            for sv, st in itertools.product((0, 1), (0, 1)):
                names.add(_stream_name(kick, reflect, sv, st, _auto_lookup(n, V.BLOCK_A_CELLS)))
    return names


def test_part_a_names_are_the_32_of_the_header():
    assert len(KERNELS) == 32 and _part_a_names() == KERNELS
    assert _auto_lookup(3000, V.BLOCK_A_CELLS) == 1 and _auto_lookup(3137, V.BLOCK_A_CELLS) == 0        # 128 * 24 = 3072 between them
    assert 3000 % 64 != 0 and 3137 % 64 != 0                                                            # both leave a ragged last tile
    print("all 32 instantiations of step_kernel_stream_vertex are asserted by name in part (a) on the 24-cell block")


@pytest.mark.parametrize("name,n,kick,reflect", list(_part_a_cases()),
                         ids=["%s-n%d-%s-%s" % (a, b, "kick" if k else "D0", "reflect" if r else "noreflect") for a, b, k, r in _part_a_cases()])
def test_a_cycle_against_the_cpu_statement(name, n, kick, reflect):
    c = V.case(name)
    if name == "block A":
        assert c.mesh.n_cells == V.BLOCK_A_CELLS
    xyz, cell0 = V.cloud(name, n)
    ref = cpu_ref(name, n, kick, reflect)
    lookup = _auto_lookup(n, c.mesh.n_cells)
    for sv, st in itertools.product((0, 1), (0, 1)):
        expect = _stream_name(kick, reflect, sv, st, lookup)
        assert expect in KERNELS and expect.endswith(", %d> (cone locate)" % lookup)
        got = gpu_run(c, xyz, cell0, kick, reflect, sv, st, expect, fused=True)
        compare_with_cpu(c, ref, got, cell0, kick, reflect, sv, expect + " n=%d" % n)


def test_the_thin_box_is_one_cell_thick():
    c = V.case("thin box")
    ctx = _context(c, 0)
    try:
        assert ctx.mesh_flags()["z_thin"] == 1 and ctx.mesh_flags()["all_hex"] == 1
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (b)
@functools.lru_cache(maxsize=None)
def _part_b_cloud(name):
    """(a)'s cloud and, behind it, one that sits on the structure of the tet fans and a rounding off it"""
    from test_gpu_vertex_fast import _adversarial_points
    c = V.case(name)
    xyz, cell0 = V.cloud(name, V.MESHES[name][2][0])
    adv, acell = _adversarial_points(c.mesh, c.centres, c.pos, c.tets, np.random.default_rng(606), per_kind=40)
    P = np.ascontiguousarray(np.concatenate([xyz, adv])); cell = np.concatenate([cell0, acell]).astype(np.int32)
    P.setflags(write=False); cell.setflags(write=False)
    return P, cell


def _equal(a, b, what, vel_mask=None):
    bad = np.nonzero(a[1] != b[1])[0]
    assert bad.size == 0, (what, "cells", bad.size, bad[:5], a[1][bad[:5]], b[1][bad[:5]])
    bad = np.nonzero(~((a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))).all(1))[0]
    assert bad.size == 0, (what, "positions", bad.size, bad[:5], a[0][bad[:5]], b[0][bad[:5]])
    if a[2] is not None and b[2] is not None:
        m = slice(None) if vel_mask is None else vel_mask
        assert np.array_equal(a[2][m], b[2][m], equal_nan=True), (what, "velocities", int((a[2][m] != b[2][m]).any(1).sum()))


@pytest.mark.parametrize("name,kick,reflect", [(a, k, r) for a in V.MESHES for k, r in itertools.product((0, 1), (1, 0))
                                               if r or a != "pitzDaily"],
                         ids=lambda v: v if isinstance(v, str) else str(v))
def test_b_every_route_of_the_library_gives_the_same_bits(name, kick, reflect):
    c = V.case(name)
    xyz, cell0 = _part_b_cloud(name)
    n = xyz.shape[0]
    lookup = _auto_lookup(n, c.mesh.n_cells)
    staged = staged_run(c, xyz, cell0, kick, reflect)
    # The one place where the fused cycle's arithmetic legitimately differs from the staged calls': with the kick and reflecting
    # walls on a mesh one cell thick in z the kernels mirror the END POINT about the z planes before the walk (csrc/cpf_walk.h,
    # fold_z), the staged calls walk to the plane and mirror at the hit point as the reference does -- the same trajectory in exact
    # arithmetic, final coordinates that differ by the rounding of the hit point.  Option "z_fold" 0 switches the shortcut off:
    # THAT run equals the staged calls bit for bit; the run with the shortcut is held to a rounding after the first cycle.
    folds = bool(kick and reflect and mesh_flags_host(c.mesh)["z_thin"])
    assert folds == bool(kick and reflect and name in ("thin box", "pitzDaily"))
    for sv in (0, 1):
        what = "%s kick=%d reflect=%d store_vel=%d" % (name, kick, reflect, sv)
        base = gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _stream_name(kick, reflect, sv, 0, lookup), fused=False)
        routes = {
            "stats 1": gpu_run(c, xyz, cell0, kick, reflect, sv, 1, _stream_name(kick, reflect, sv, 1, lookup), fused=False),
            "fused launches": gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _stream_name(kick, reflect, sv, 0, lookup), fused=True),
            "sorted": gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _stream_name(kick, reflect, sv, 0, lookup), fused=False, sort=True),
            "other LOOKUP": gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _stream_name(kick, reflect, sv, 0, 1 - lookup), fused=False,
                                    opts=(("stream_lookup", 1 - lookup),)),
            "other LOOKUP, fused, stats": gpu_run(c, xyz, cell0, kick, reflect, sv, 1, _stream_name(kick, reflect, sv, 1, 1 - lookup),
                                                  fused=True, opts=(("stream_lookup", 1 - lookup),)),
            "generic walk, all tets": gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _generic_name(kick, reflect, sv), fused=False,
                                              opts=(("step_variant", 0), ("vertex_fast", 0))),
        }
        if folds:
            unfolded = gpu_run(c, xyz, cell0, kick, reflect, sv, 0, _stream_name(kick, reflect, sv, 0, lookup), fused=False, opts=(("z_fold", 0),))
        for k in V.CHECKPOINTS:
            live = base[k][1] >= 0
            for route, got in routes.items():
                # a fused launch leaves a particle it lost the velocity of its last live cycle, a launch that does not step it leaves 0
                _equal(got[k], base[k], (what, route, k), vel_mask=live if "fused" in route else None)
            sP, sstate, svel = staged[k]
            if not folds:
                _equal((sP, sstate, svel if sv else None), base[k], (what, "staged calls", k), vel_mask=live)
            else:
                _equal((sP, sstate, svel if sv else None), unfolded[k], (what, "staged calls, z_fold 0", k), vel_mask=unfolded[k][1] >= 0)
                if k == 1:
                    # (of the particles that START inside the cell they claim by more than the walk's tolerance, 1e-13: the structure
                    # cloud also has points ON a z plane and 1e-15 ... 1e-5 beyond it.  The reference's walk does not see a plane its
                    # start point lies on -- dT = 0 is not above the tolerance -- and lets such a particle through that wall, and it
                    # reflects one that starts beyond the plane off it from behind; the mirrored end point does neither)
                    inside = (cell0 >= 0) & (V.inward_distance(c.mesh, xyz, np.maximum(cell0, 0)) > 1e-13)
                    assert inside.sum() > 0.9 * n
                    same = (sstate == base[k][1])[inside]
                    dx = np.abs(sP[:, :3] - base[k][0][:, :3])[inside][same].max(initial=0.0)
                    print("MEASURED %s | fold_z against the staged calls | k=1 | equal cells %.6f, max |dx|/L %.3e" % (what, same.mean(), dx / c.diag))
                    assert same.mean() > 0.9999 and dx <= 1e-13 * c.diag, (what, same.mean(), dx)


def test_b_the_fold_does_not_depend_on_who_shares_a_wave():
    """The kick on a mesh one cell thick in z: a wave whose lanes' mirrored end points are all clear of the z planes leaves the z
    faces out of its rounds (csrc/cpf_walk.h, fold_z).  That is the reference's result only for a lane that STARTS between the
    planes; one that starts a rounding beyond a plane -- the structure cloud has such points, and the move's hit + (E - hit) can
    leave one there -- has that face accepted by the reference's walk, so it has to count as not clear.  Before fold_z looked at
    the start point, three particles of this cloud depended on which particles shared their wave: the sorted cloud differed from
    the unsorted one.  The same walk serves the cell-constant cycle: both cycles, unsorted / sorted / the generic walk."""
    from cudaparticlesfoam_amd.api import Context
    c = V.case("thin box")
    xyz, cell0 = _part_b_cloud("thin box")
    beyond = (cell0 >= 0) & (V.inward_distance(c.mesh, xyz, np.maximum(cell0, 0)) < 0)
    assert ((xyz[beyond, 2] < c.lo[2]) | (xyz[beyond, 2] > c.hi[2])).sum() > 10            # starts beyond a z plane are in the cloud
    U = np.random.default_rng(3).normal(size=(c.mesh.n_cells, 3))
    for flags in (L.STEP_VERTEX_VELOCITY, 0):
        res = []
        for sort, opts in ((False, ()), (True, ()), (False, (("step_variant", 0),))):
            ctx = Context(0)
            try:
                ctx.set_option("stats", 0)
                for k, v in opts:
                    ctx.set_option(k, v)
                ctx.set_mesh(c.mesh); ctx.set_velocity(U)
                ctx.set_tets(c.pos, c.tets, 12); ctx.set_vertex_velocity(c.vU); ctx.set_seed(V.KICK_SEED)
                ctx.set_particles(xyz, cell0)
                if sort:
                    ctx.sort_by_cell()
                name = ctx.step_kernel_name(c.D, flags)
                assert ("<true, true, false, false, " in name and "step_kernel_stream" in name) if not opts else "step_kernel_stream" not in name, name
                ctx.step(c.dt, c.D, 3, flags)
                res.append(ctx.get_particles() + (None,))
            finally:
                ctx.close()
        _equal(res[1], res[0], ("thin box, kick", flags, "sorted"))
        _equal(res[2], res[0], ("thin box, kick", flags, "generic walk"))


# ------------------------------------------------------------------------------------------------ (c)
EDGE_MESH = "block B"


def _per_cell_cloud(per_cell, n_cells, seed):
    """`per_cell` points inside each of the cells 0 .. n_cells - 1, in cell order (a sorted cloud)"""
    def make():
        c = V.case(EDGE_MESH)
        assert c.mesh.n_cells >= n_cells
        rng = np.random.default_rng(seed)
        t = c.tets.reshape(c.mesh.n_cells, 12, 4)
        pts = []
        for cell in range(n_cells):
            corners = c.pos[np.unique(t[cell, :, 1:])]
            assert corners.shape[0] == 8
            pts.append(rng.dirichlet(np.full(8, 0.6), per_cell) @ corners)       # convex combinations of the hex's corners
        return np.ascontiguousarray(np.concatenate(pts)), np.repeat(np.arange(n_cells, dtype=np.int32), per_cell)
    return make


_EDGE_CLOUDS = {
    "16 a cell, 64 cells": _per_cell_cloud(16, 64, 1),      # 4 distinct cells in every wave: one staging pass
    "13 a cell, 64 cells": _per_cell_cloud(13, 64, 2),      # 5 or 6 distinct cells: two passes (13 tiles exactly)
    "13 a cell, 63 cells": _per_cell_cloud(13, 63, 3),      # ... and a last tile of 51
    "1 a cell, 64 cells": _per_cell_cloud(1, 64, 4),        # 64 distinct cells: 16 passes
}


@pytest.mark.parametrize("key", list(_EDGE_CLOUDS))
@pytest.mark.parametrize("lookup", [0, 1])
def test_c_staging_passes(key, lookup):
    c = V.case(EDGE_MESH)
    xyz, cell0 = _EDGE_CLOUDS[key]()
    per_wave = [np.unique(cell0[i:i + 64]).size for i in range(0, cell0.size, 64)]
    assert {"16 a cell, 64 cells": set(per_wave) == {4}, "13 a cell, 64 cells": set(per_wave) <= {5, 6} and len(per_wave) == 13,
            "13 a cell, 63 cells": set(per_wave) <= {4, 5, 6} and cell0.size % 64 == 51, "1 a cell, 64 cells": per_wave == [64]}[key]
    assert (V.inward_distance(c.mesh, xyz, cell0) > 0).all()
    cps = (1, 6)
    ref = cpu_ref(EDGE_MESH, xyz.shape[0], 0, 1, checkpoints=cps, cloud_key=key)
    expect = _stream_name(0, 1, 0, 0, lookup)
    got = gpu_run(c, xyz, cell0, 0, 1, 0, 0, expect, fused=True, opts=(("stream_lookup", lookup),), checkpoints=cps)
    gen = gpu_run(c, xyz, cell0, 0, 1, 0, 0, _generic_name(0, 1, 0), fused=True, opts=(("step_variant", 0), ("vertex_fast", 0)), checkpoints=cps)
    for k in cps:
        _equal(got[k], gen[k], (key, lookup, k))
    compare_with_cpu(c, ref, got, cell0, 0, 1, 0, "%s, LOOKUP %d" % (key, lookup), checkpoints=cps)


@pytest.mark.parametrize("lookup", [0, 1])
def test_c_a_launch_that_begins_with_lost_and_frozen_lanes(lookup):
    """A fused launch without reflection loses particles in its cycles 1 to 6; the next launch on the same cloud begins with lanes
    that are CPF_CELL_LOST (lost in cycle 6) and CPF_CELL_FROZEN (before): cycle_begin's cur = CPF_CELL_FROZEN, slow = busy = false."""
    key = "16 a cell, 64 cells"
    c = V.case(EDGE_MESH)
    xyz, cell0 = _EDGE_CLOUDS[key]()
    cps = (6, 12)
    ref = cpu_ref(EDGE_MESH, xyz.shape[0], 0, 0, checkpoints=cps, cloud_key=key)
    assert (ref[6].state == L.CELL_FROZEN).sum() > 0 and (ref[6].state >= 0).sum() > 0
    expect = _stream_name(0, 0, 0, 0, lookup)
    got = gpu_run(c, xyz, cell0, 0, 0, 0, 0, expect, fused=True, opts=(("stream_lookup", lookup),), checkpoints=cps)
    gen = gpu_run(c, xyz, cell0, 0, 0, 0, 0, _generic_name(0, 0, 0), fused=True, opts=(("step_variant", 0), ("vertex_fast", 0)), checkpoints=cps)
    for k in cps:
        _equal(got[k], gen[k], (lookup, k))
        assert np.array_equal(got[k][1], ref[k].state) and np.array_equal(got[k][0][:, 3], ref[k].P[:, 3])
        r = V.rel(got[k][0], ref[k].P, c.diag)
        print("MEASURED %s | %s after a launch that lost particles | k=%d | max |dx|/L %.3e" % (c.name, expect, k, r.max()))
        assert (r <= V.REL_TOL).all()
    assert (got[12][1] == L.CELL_FROZEN).sum() > (got[6][1] == L.CELL_FROZEN).sum() > 0
