"""GPU: the UNKICKED cycle (cpf_step / cpf_step_dev with D = 0) -- every one of the 80 instantiations step_kernel_stream<false, REFLECT,
STORE_VEL, STATS, LOOKUP> and the 16 of step_kernel_stream_flat<REFLECT, STORE_VEL, STATS, LOOKUP> -- against the CPU statement
(CellWalk.step_given(xi = None), oracle/cellwalk.c; tests/test_plain_cycle_host.py shows it to be cw_step(D = 0)), BIT FOR BIT:
positions (compared as int64 bits), cells (CPF_CELL_LOST and CPF_CELL_FROZEN included), stored velocities, and with statistics on
the visit, reflection, lost and particle-step counters as deltas per checkpoint -- with statistics off the counters must not move --,
after 1, 6 and 20 cycles, no tolerance, no particle left out.

The point is the LEAN instantiations <false, true | false, false, false, L>: what a run without velocity output launches, squeezed
into 5-7 waves per SIMD around hand-counted waits, where the suite's parity tests -- "stats" on -- run the one-wave STATS
instantiations.  And the paths only the unkicked kernels have: the wall hit point kept in registers, the z pair skipped while
nobody moves in z, the wave-uniform zero-denominator skip, the sparse mode's fifth wave.

Before each comparison the test asserts the exact name of the kernel the launch ran; parts (a) and (c) meet every one of

    cpf::step_kernel_stream<false, false, false, false, 0>
    cpf::step_kernel_stream<false, false, false, true, 0>
    cpf::step_kernel_stream<false, false, true, false, 0>
    cpf::step_kernel_stream<false, false, true, true, 0>
    cpf::step_kernel_stream<false, true, false, false, 0>
    cpf::step_kernel_stream<false, true, false, true, 0>
    cpf::step_kernel_stream<false, true, true, false, 0>
    cpf::step_kernel_stream<false, true, true, true, 0>
    cpf::step_kernel_stream<false, false, false, false, 1>
    cpf::step_kernel_stream<false, false, false, true, 1>
    cpf::step_kernel_stream<false, false, true, false, 1>
    cpf::step_kernel_stream<false, false, true, true, 1>
    cpf::step_kernel_stream<false, true, false, false, 1>
    cpf::step_kernel_stream<false, true, false, true, 1>
    cpf::step_kernel_stream<false, true, true, false, 1>
    cpf::step_kernel_stream<false, true, true, true, 1>
    cpf::step_kernel_stream<false, false, false, false, 2>
    cpf::step_kernel_stream<false, false, false, true, 2>
    cpf::step_kernel_stream<false, false, true, false, 2>
    cpf::step_kernel_stream<false, false, true, true, 2>
    cpf::step_kernel_stream<false, true, false, false, 2>
    cpf::step_kernel_stream<false, true, false, true, 2>
    cpf::step_kernel_stream<false, true, true, false, 2>
    cpf::step_kernel_stream<false, true, true, true, 2>
    cpf::step_kernel_stream<false, false, false, false, 3>
    cpf::step_kernel_stream<false, false, false, true, 3>
    cpf::step_kernel_stream<false, false, true, false, 3>
    cpf::step_kernel_stream<false, false, true, true, 3>
    cpf::step_kernel_stream<false, true, false, false, 3>
    cpf::step_kernel_stream<false, true, false, true, 3>
    cpf::step_kernel_stream<false, true, true, false, 3>
    cpf::step_kernel_stream<false, true, true, true, 3>
    cpf::step_kernel_stream<false, false, false, false, 4>
    cpf::step_kernel_stream<false, false, false, true, 4>
    cpf::step_kernel_stream<false, false, true, false, 4>
    cpf::step_kernel_stream<false, false, true, true, 4>
    cpf::step_kernel_stream<false, true, false, false, 4>
    cpf::step_kernel_stream<false, true, false, true, 4>
    cpf::step_kernel_stream<false, true, true, false, 4>
    cpf::step_kernel_stream<false, true, true, true, 4>
    cpf::step_kernel_stream<false, false, false, false, 5>
    cpf::step_kernel_stream<false, false, false, true, 5>
    cpf::step_kernel_stream<false, false, true, false, 5>
    cpf::step_kernel_stream<false, false, true, true, 5>
    cpf::step_kernel_stream<false, true, false, false, 5>
    cpf::step_kernel_stream<false, true, false, true, 5>
    cpf::step_kernel_stream<false, true, true, false, 5>
    cpf::step_kernel_stream<false, true, true, true, 5>
    cpf::step_kernel_stream<false, false, false, false, 6>
    cpf::step_kernel_stream<false, false, false, true, 6>
    cpf::step_kernel_stream<false, false, true, false, 6>
    cpf::step_kernel_stream<false, false, true, true, 6>
    cpf::step_kernel_stream<false, true, false, false, 6>
    cpf::step_kernel_stream<false, true, false, true, 6>
    cpf::step_kernel_stream<false, true, true, false, 6>
    cpf::step_kernel_stream<false, true, true, true, 6>
    cpf::step_kernel_stream<false, false, false, false, 11>
    cpf::step_kernel_stream<false, false, false, true, 11>
    cpf::step_kernel_stream<false, false, true, false, 11>
    cpf::step_kernel_stream<false, false, true, true, 11>
    cpf::step_kernel_stream<false, true, false, false, 11>
    cpf::step_kernel_stream<false, true, false, true, 11>
    cpf::step_kernel_stream<false, true, true, false, 11>
    cpf::step_kernel_stream<false, true, true, true, 11>
    cpf::step_kernel_stream<false, false, false, false, 8>
    cpf::step_kernel_stream<false, false, false, true, 8>
    cpf::step_kernel_stream<false, false, true, false, 8>
    cpf::step_kernel_stream<false, false, true, true, 8>
    cpf::step_kernel_stream<false, true, false, false, 8>
    cpf::step_kernel_stream<false, true, false, true, 8>
    cpf::step_kernel_stream<false, true, true, false, 8>
    cpf::step_kernel_stream<false, true, true, true, 8>
    cpf::step_kernel_stream<false, false, false, false, 9>
    cpf::step_kernel_stream<false, false, false, true, 9>
    cpf::step_kernel_stream<false, false, true, false, 9>
    cpf::step_kernel_stream<false, false, true, true, 9>
    cpf::step_kernel_stream<false, true, false, false, 9>
    cpf::step_kernel_stream<false, true, false, true, 9>
    cpf::step_kernel_stream<false, true, true, false, 9>
    cpf::step_kernel_stream<false, true, true, true, 9>
    cpf::step_kernel_stream_flat<false, false, false, 8>
    cpf::step_kernel_stream_flat<false, false, true, 8>
    cpf::step_kernel_stream_flat<false, true, false, 8>
    cpf::step_kernel_stream_flat<false, true, true, 8>
    cpf::step_kernel_stream_flat<true, false, false, 8>
    cpf::step_kernel_stream_flat<true, false, true, 8>
    cpf::step_kernel_stream_flat<true, true, false, 8>
    cpf::step_kernel_stream_flat<true, true, true, 8>
    cpf::step_kernel_stream_flat<false, false, false, 9>
    cpf::step_kernel_stream_flat<false, false, true, 9>
    cpf::step_kernel_stream_flat<false, true, false, 9>
    cpf::step_kernel_stream_flat<false, true, true, 9>
    cpf::step_kernel_stream_flat<true, false, false, 9>
    cpf::step_kernel_stream_flat<true, false, true, 9>
    cpf::step_kernel_stream_flat<true, true, false, 9>
    cpf::step_kernel_stream_flat<true, true, true, 9>

(test_the_names_are_the_96_of_the_header checks the list against the parametrisations).

(a) The 64 that are not the flat walk, on the smallest meshes that reach their lookups (tests/browniancycle.py, MESHES): the 24-cell
    sheared block (LOOKUP 0, 1, 4 by cloud size; also clouds of 1 and 65), 720 graded boxes (6; "box_records" 0: 1), the 2:1-refined
    box (11; "box_records" 0: 3; and "stream_lookup" 0: 5), the cut-corner and the chamfered grid (2).  Clouds ordered by cell;
    for two flag sets per case also as drawn (the per-lane gather walk); one fused launch per checkpoint, and on the lean flag
    sets single-cycle launches as well.  Every cloud begins with lost and frozen lanes at those of positions 5, 64 and 130 it has.
(b) A field with exact zeros (Case.U0): a third of the cells at rest (+0.0 and -0.0 mixed), a third with U.x == +-0.0.  The skip of
    a zero denominator is wave-uniform, so it takes whole tiles in such cells: the host file asserts that the clouds have them.
(c) The flat walk on box_mesh(6, 5, 1) in a field without z: cpf_step on the context's own cloud, the first launch streaming z
    (step_kernel_stream<false, ..., 8 | 9>), the later ones the body without z (step_kernel_stream_flat), z == -0.0 for every fifth
    particle; and with a z component the same mesh on LOOKUP 0, 1 and 4: the z pair tested last (zLast).
(d) Every route gives the CPU's bits on the lean instantiations: cpf_step on the context's own cloud never sorted and re-sorted every
    three cycles, twenty single-cycle launches against one fused launch, a velocity refresh between two launches, and the
    chamfered grid driven into a corner -- more than 16 lanes of a tile reflect in one cycle, LOOKUP 2's hit pool of 16 overflows
    on the six-wave kernel.
The inputs go through the hard paths, asserted on the CPU statement's own counters: face crossings, wall reflections, two walls
in a cycle, three crossings in a cycle, losses without reflection."""
import itertools
import types

import numpy as np
import pytest

import browniancycle as B
from cudaparticlesfoam_amd import _lib as L

pytestmark = pytest.mark.gpu

_TF = ("false", "true")
KERNELS = frozenset(line.strip() for line in __doc__.splitlines() if line.strip().startswith("cpf::step_kernel_stream"))
LOOKUPS = (0, 1, 2, 3, 4, 5, 6, 11)
FLAT_LOOKUPS = (8, 9)
ALL8 = tuple(itertools.product((1, 0), (0, 1), (0, 1)))            # (reflect, store velocities, statistics)
FOUR = ((1, 0, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1))                # REFLECT x {lean, STORE_VEL + STATS}
LEAN = ((1, 0, 0), (0, 0, 0))                                      # what a run without velocity output launches
AS_DRAWN = ((1, 0, 0), (0, 1, 1))                                  # what also runs on the cloud as drawn
ZEROS = ((1, 0, 0), (1, 1, 1))                                     # part (b)
DEFAULTS = (("stream_lookup", -1), ("box_records", 1), ("sort_interval", 50), ("stats", 1))
N_BASE = 6000                                                      # the largest cloud here


def _stream(reflect, sv, st, lookup):
    return "cpf::step_kernel_stream<false, %s, %s, %s, %d>" % (_TF[reflect], _TF[sv], _TF[st], lookup)


def _flat(reflect, sv, st, lookup):
    return "cpf::step_kernel_stream_flat<%s, %s, %s, %d>" % (_TF[reflect], _TF[sv], _TF[st], lookup)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# The module's contexts (one per mesh and field kind), closed when the file's last test has run; the CPU results are cached in
# tests/browniancycle.py (plain_ref) per (mesh, field, cloud, reflect) and never written to.
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for value in _state.values():
        value.close()                        # (closing twice is harmless: the factory's own teardown finds the handle gone)
    _state.clear()


def _ctx(name, make, field="U", n=None):
    """the context of a mesh with the case's field; field "Uflat": a context of its own per cloud size, which keeps that field (and
    has launched nothing but that cloud: cpf_step_kernel_name goes by the most recent launch's particle count)"""
    key = (name, "Uflat" if field == "Uflat" else "U", n)
    if key not in _state:
        c = B.case(name)
        ctx = make()
        ctx.set_mesh(c.mesh); ctx.set_velocity(c.field(key[1])); ctx.set_seed(B.SEED)
        ctx.synchronize()                    # (the note "this field has no z component" has arrived)
        _state[key] = ctx
    return _state[key]


def _flags(reflect, sv, fused=True):
    return (0 if reflect else L.STEP_NO_REFLECT) | (L.STEP_STORE_VEL if sv else 0) | (L.STEP_FUSE_CYCLES if fused else 0)


def _set(ctx, opts):
    for k, v in opts:
        ctx.set_option(k, v)


def _delta(after, before):
    return {q: after[q] - before[q] for q in after}


def gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, opts=(), fused=True, checkpoints=B.CHECKPOINTS, refresh_after=None,
            field="U", how=""):
    """{k: (xyz, cell, vel | None, counter deltas, statistics on)} after k cycles of cpf_step_dev with D = 0 on device arrays;
    `expect`: the kernel name every launch must report."""
    out, done = {}, 0
    flags = _flags(reflect, sv, fused)
    _set(ctx, (("stats", st),) + tuple(opts))
    if field != "U":
        ctx.set_velocity(c.field(field))
    dc = B.DeviceCloud(ctx, xyz, cell0, gid)
    try:
        for k in checkpoints:
            before = ctx.counters()
            dc.step(c.dt, 0.0, B.STEP0 + done, k - done, flags, store_vel=bool(sv))
            name = ctx.step_kernel_name(0.0, flags)
            assert name == expect, (name, expect)
            after = ctx.counters()
            done = k
            p, cell, vel = dc.get()
            out[k] = (p, cell, vel if sv else None, _delta(after, before), st)
            if refresh_after == k:
                ctx.set_velocity(c.U2)
    finally:
        dc.close()
        if refresh_after is not None or field != "U":
            ctx.set_velocity(c.U)
        _set(ctx, DEFAULTS)
    print("ran %s: %s n=%d %s, %s%s" % (expect, c.name, xyz.shape[0], "by cell" if gid is not None else "as drawn",
                                        "fused launches" if fused else "single-cycle launches", how))
    return out


def compare(ref, got, what, vel_live_at=None):
    """positions as bits, cells, stored velocities as bits, the four counters (statistics off: they did not move): for every particle"""
    for k in got:
        p, cell, vel, cnt, st = got[k]
        s = ref[k]
        bad = np.nonzero(cell != s.cell)[0]
        assert bad.size == 0, (what, k, "cells differ", bad.size, bad[:5], cell[bad[:5]], s.cell[bad[:5]])
        bad = np.nonzero((_bits(p) != _bits(s.xyz)).any(1))[0]
        assert bad.size == 0, (what, k, "positions differ", bad.size, bad[:5], p[bad[:5]], s.xyz[bad[:5]])
        if vel is not None:
            m = slice(None) if vel_live_at is None else vel_live_at[k]
            bad = np.nonzero((_bits(vel[m]) != _bits(s.vel[m])).any(1))[0]
            assert bad.size == 0, (what, k, "stored velocities differ", bad.size, bad[:5], vel[m][bad[:5]], s.vel[m][bad[:5]])
        if st:
            want = dict(cells_visited=s.stats[0], reflections=s.stats[1], lost=s.stats[2], particle_steps=s.stats[3])
        else:
            want = dict(cells_visited=0, reflections=0, lost=0, particle_steps=0)
        assert cnt == want, (what, k, cnt, want)


def _end_only(ref):
    """the reference of ONE launch of all twenty cycles: the last snapshot, with the counters of the whole run"""
    end = ref[20]
    return {20: types.SimpleNamespace(xyz=end.xyz, cell=end.cell, vel=end.vel, stats=[sum(ref[k].stats[q] for k in B.CHECKPOINTS) for q in range(4)])}


def assert_hard_paths(name, n):
    """the reflecting run being compared did go where the kernels are hard (the bars of the kicked cycle's file)"""
    hp = B.hard_paths(B.plain_ref(name, "U", n, True, 1)[1])
    lost = float((B.plain_ref(name, "U", n, True, 0)[0][20].cell < 0).mean())
    print("MEASURED %s n=%d | %s | lost or frozen without reflection %.3f" % (name, n, hp, lost))
    assert hp["crossing"] >= 0.10 and hp["reflecting"] >= 0.01 and hp["two_walls"] >= 1, hp
    if name != "thin box":
        assert hp["three_hops"] >= 1, hp
        assert lost >= 0.01, lost


# ------------------------------------------------------------------------------------------------ (a)
# (mesh, cloud size, LOOKUP the launch must run, options, flag sets)
A_RUNS = [
    ("block A", 6000, 0, (), ALL8),                                 # 24 cells: n >= 128 * 24
    ("block A", 700, 1, (), ALL8),                                  # ... below it
    ("block A", 150, 4, (), ALL8),                                  # ... below 8 * 24
    ("block A", 65, 4, (), FOUR),                                   # a tile and one lane
    ("block A", 1, 4, (), FOUR),
    ("graded box", 6000, 6, (), ALL8),
    ("graded box", 6000, 1, (("box_records", 0),), FOUR),           # (n >= 8 * 720: below it the sparse lookup takes over)
    ("refined box", 6000, 11, (), ALL8),
    ("refined box", 6000, 3, (("box_records", 0),), ALL8),
    ("refined box", 6000, 5, (("box_records", 0), ("stream_lookup", 0)), ALL8),
    ("cut corners", 6000, 2, (), ALL8),
    ("chamfered", 6000, 2, (), FOUR),
]
B_RUNS = [r for r in A_RUNS if r[1] >= 150]                         # every lookup of (a), on clouds with whole tiles
# (cloud size, LOOKUP) on box_mesh(6, 5, 1), 30 cells -- in the field without z: n >= 128 * 30 the flat loop lookup, below it the fixed one
C_FLAT = [(6000, 8), (2000, 9)]
# ... and with a z component: the plain lookups, the z pair last (below 8 * 30: the sparse one)
C_ZLAST = [(6000, 0), (2000, 1), (150, 4)]
ZLAST_SETS = ((1, 0, 0), (0, 0, 0), (0, 1, 1))


def test_the_names_are_the_96_of_the_header():
    a = {_stream(r, sv, st, lookup) for _, _, lookup, _, sets in A_RUNS for r, sv, st in sets}
    assert len(a) == 64 and a == {_stream(r, sv, st, lookup) for lookup in LOOKUPS for r, sv, st in ALL8}
    c = {f(r, sv, st, lookup) for _, lookup in C_FLAT for r, sv, st in ALL8 for f in (_stream, _flat)}
    assert len(c) == 32 and c == {f(r, sv, st, lookup) for lookup in FLAT_LOOKUPS for r, sv, st in ALL8 for f in (_stream, _flat)}
    assert len(KERNELS) == 96 and a | c == KERNELS
    # the lean names of (a) run by cell fused and in single cycles, and the reflecting one as drawn both ways: the test's own loops
    assert all(set(LEAN) <= set(sets) for *_, sets in A_RUNS) and (1, 0, 0) in AS_DRAWN
    assert {lookup for _, _, lookup, _, _ in B_RUNS} == set(LOOKUPS)
    assert 6000 >= 128 * 24 > 700 >= 8 * 24 > 150 and 6000 >= 8 * 720
    assert 6000 >= 128 * 30 > 2000 >= 8 * 30 > 150
    print("all 80 unkicked instantiations of step_kernel_stream and the 16 of step_kernel_stream_flat are asserted by name")


@pytest.mark.parametrize("name,n,lookup,opts,flagsets", A_RUNS, ids=["%s-n%d-lookup%d" % r[:3] for r in A_RUNS])
def test_a_every_unkicked_instantiation_against_the_cpu_statement(name, n, lookup, opts, flagsets, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    if name == "block A":
        assert c.mesh.n_cells == 24
    if n >= 3000:
        assert_hard_paths(name, n)
    for sort in (True, False):
        xyz, cell0, gid = B.cloud(name, n, sort=sort)
        how = "by cell" if sort else "as drawn"
        for reflect, sv, st in (flagsets if sort else AS_DRAWN):
            expect = _stream(reflect, sv, st, lookup)
            assert expect in KERNELS
            ref, _ = B.plain_ref(name, "U", n, sort, reflect)
            got = gpu_run(ctx, c, xyz, cell0, gid if sort else None, reflect, sv, st, expect, opts)
            compare(ref, got, "%s n=%d %s" % (expect, n, how))
            if (reflect, sv, st) in LEAN and (sort or reflect):
                got = gpu_run(ctx, c, xyz, cell0, gid if sort else None, reflect, sv, st, expect, opts, fused=False)
                compare(ref, got, "%s n=%d %s, single-cycle launches" % (expect, n, how))


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name,n,lookup,opts", [r[:4] for r in B_RUNS], ids=["%s-n%d-lookup%d" % r[:3] for r in B_RUNS])
def test_b_a_field_with_exact_zeros(name, n, lookup, opts, gpu_ctx_factory, oracle_libs):
    """Whole tiles at rest, whole tiles without an x component (tests/test_plain_cycle_host.py asserts that the cloud of 6000 has
    them on every mesh; here again for the cloud that runs, where it is that large)"""
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    ref, diag = B.plain_ref(name, "U0", n, True, 1)
    if n == N_BASE:
        assert B.at_rest_tiles(c, cell0).size >= 1
        if name in ("graded box", "refined box"):
            assert B.zero_x_crossing_tiles(c, cell0, diag).size >= 1
    for reflect, sv, st in ZEROS:
        expect = _stream(reflect, sv, st, lookup)
        got = gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, opts, field="U0", how=", the field with zeros")
        compare(ref, got, "%s %s n=%d, the field with zeros" % (expect, name, n))
        if not sv:
            got = gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, opts, fused=False, field="U0", how=", the field with zeros")
            compare(ref, got, "%s %s n=%d, the field with zeros, single-cycle launches" % (expect, name, n))


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("reflect,sv,st", ALL8, ids=["reflect%d-vel%d-stats%d" % f for f in ALL8])
@pytest.mark.parametrize("n,lookup", C_FLAT)
def test_c_the_flat_walk_streams_z_once_and_then_runs_the_body_without_z(n, lookup, reflect, sv, st, gpu_ctx_factory, oracle_libs):
    """cpf_step on the context's own cloud: the first launch is step_kernel_stream<false, ..., 8 | 9>, every later one
    step_kernel_stream_flat<..., 8 | 9>; both names are asserted before the launch they name."""
    c, ctx = B.case("thin box"), _ctx("thin box", gpu_ctx_factory, "Uflat", n)
    xyz, cell0, _ = B.flat_cloud(n)
    assert np.signbit(xyz[::5, 2]).all() and not xyz[::5, 2].any()
    ref, diag = B.plain_ref("thin box", "Uflat", n, True, reflect, flat=True)
    if reflect:
        hp = B.hard_paths(diag)
        assert hp["crossing"] >= 0.10 and hp["reflecting"] >= 0.01 and hp["two_walls"] >= 1, hp
    flags = _flags(reflect, sv)
    got, live_at, done, ran = {}, {}, 0, []
    _set(ctx, (("stats", st), ("sort_interval", 0)))
    try:
        ctx.set_particles(xyz, cell0)        # (a cloud set anew: its z is not settled)
        live = cell0 >= 0
        for k in B.CHECKPOINTS:
            expect = _flat(reflect, sv, st, lookup) if done else _stream(reflect, sv, st, lookup)
            assert expect in KERNELS
            name = ctx.step_kernel_name(0.0, flags)
            assert name == expect, (name, expect)
            ran.append(name)
            before = ctx.counters()
            ctx.step(c.dt, 0.0, k - done, flags)
            after = ctx.counters()
            done = k
            xyzw, cell, vel = ctx.get_particles(want_vel=True) if sv else ctx.get_particles() + (None,)
            got[k] = (xyzw[:, :3].copy(), cell, vel[:, :3].copy() if sv else None, _delta(after, before), st)
            live_at[k] = live                    # (a frame holds the velocities of the particles that launch stepped)
            live = cell >= 0
        assert ctx.step_kernel_name(0.0, flags) == _flat(reflect, sv, st, lookup)
    finally:
        _set(ctx, DEFAULTS)
    assert ran == [_stream(reflect, sv, st, lookup)] + 2 * [_flat(reflect, sv, st, lookup)]
    print("ran %s, then %s: thin box n=%d" % (ran[0], ran[1], n))
    compare(ref, got, "cpf_step, thin box without z, n=%d, %s then %s" % (n, ran[0], ran[1]), vel_live_at=live_at)
    # the first cycle rewrote -0.0 for whoever it stepped; who began lost or frozen keeps the z it had
    assert not np.signbit(got[1][0][cell0 >= 0, 2]).any() and np.signbit(got[20][0][[5, 130], 2]).all()


@pytest.mark.parametrize("n,lookup", C_ZLAST)
def test_c_with_a_z_component_the_z_pair_is_tested_last(n, lookup, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case("thin box"), _ctx("thin box", gpu_ctx_factory)
    assert ctx.mesh_flags()["all_hex"] == 1 and c.U[:, 2].all()
    if n >= 3000:
        assert_hard_paths("thin box", n)
    xyz, cell0, gid = B.cloud("thin box", n, sort=True)
    for reflect, sv, st in ZLAST_SETS:
        expect = _stream(reflect, sv, st, lookup)
        ref, _ = B.plain_ref("thin box", "U", n, True, reflect)
        for fused in (True, False) if not sv else (True,):
            got = gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, fused=fused)
            compare(ref, got, "%s thin box n=%d" % (expect, n))


# ------------------------------------------------------------------------------------------------ (d)
D_MESHES = (("block A", 0), ("graded box", 6), ("refined box", 11))


@pytest.mark.parametrize("sort_interval", [0, 3])
@pytest.mark.parametrize("name,lookup", D_MESHES)
def test_d_the_contexts_own_cloud(name, lookup, sort_interval, gpu_ctx_factory, oracle_libs):
    """cpf_step on the context's own cloud, set as drawn: never sorted ("sort_interval" 0), or re-sorted every three cycles; the
    particles come back by the position they were set with either way."""
    c = B.case(name)
    n = N_BASE
    xyz, cell0, _ = B.cloud(name, n, sort=False)
    ctx = gpu_ctx_factory()
    try:
        _set(ctx, (("stats", 0), ("sort_interval", sort_interval)))
        ctx.set_mesh(c.mesh); ctx.set_velocity(c.U); ctx.set_seed(B.SEED)
        for reflect in (1, 0):
            expect = _stream(reflect, 0, 0, lookup)
            flags = _flags(reflect, 0)
            ref, _ = B.plain_ref(name, "U", n, False, reflect)
            ctx.set_particles(xyz, cell0)
            got, done = {}, 0
            for k in B.CHECKPOINTS:
                before = ctx.counters()
                ctx.step(c.dt, 0.0, k - done, flags)
                name_ran = ctx.step_kernel_name(0.0, flags)
                assert name_ran == expect, (name_ran, expect)
                done = k
                xyzw, cell = ctx.get_particles()
                got[k] = (xyzw[:, :3].copy(), cell, None, _delta(ctx.counters(), before), 0)
            print("ran %s: cpf_step, %s n=%d as drawn, sort_interval %d" % (expect, name, n, sort_interval))
            compare(ref, got, "cpf_step, %s, sort_interval %d, %s" % (name, sort_interval, expect))
    finally:
        ctx.close()


@pytest.mark.parametrize("name,lookup", D_MESHES)
def test_d_twenty_single_cycle_launches_one_fused_launch_and_a_velocity_refresh(name, lookup, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    n = N_BASE
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    for reflect in (1, 0):
        expect = _stream(reflect, 0, 0, lookup)
        plain, _ = B.plain_ref(name, "U", n, True, reflect)
        for fused in (True, False):
            got = gpu_run(ctx, c, xyz, cell0, gid, reflect, 0, 0, expect, fused=fused, checkpoints=(20,))
            compare(_end_only(plain), got, "%s %s %s" % (expect, name, "one launch of 20" if fused else "20 launches of 1"))
        # the field changes behind the sixth cycle (cpf_set_velocity between two launches)
        ref, _ = B.plain_ref(name, "U", n, True, reflect, refresh_after=6)
        assert np.array_equal(ref[6].xyz, plain[6].xyz) and not np.array_equal(ref[20].xyz, plain[20].xyz)
        got = gpu_run(ctx, c, xyz, cell0, gid, reflect, 0, 0, expect, refresh_after=6, how=", velocity refresh")
        compare(ref, got, "%s %s velocity refresh" % (expect, name))


def test_d_more_than_16_lanes_of_a_tile_reflect_the_hit_pool_of_lookup_2_overflows(gpu_ctx_factory, oracle_libs):
    """The chamfered grid (LOOKUP 2: a hit pool of 16 entries per wave, no hit point in registers) with one velocity everywhere,
    towards a corner: whole tiles of the cloud ordered by cell reflect in one cycle -- on the six-wave lean kernels."""
    name = "chamfered"
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    xyz, cell0, gid = B.cloud(name, N_BASE, sort=True)
    ref, diag = B.plain_ref(name, "Ucorner", N_BASE, True, 1)
    most = B.most_lanes_of_a_tile_reflecting(diag)
    print("MEASURED chamfered, driven into a corner | most lanes of a tile reflecting in one cycle: %d | %s" % (most, B.hard_paths(diag)))
    assert most > 16
    for reflect in (1, 0):
        expect = _stream(reflect, 0, 0, 2)
        ref, _ = B.plain_ref(name, "Ucorner", N_BASE, True, reflect)
        for fused in (True, False):
            got = gpu_run(ctx, c, xyz, cell0, gid, reflect, 0, 0, expect, fused=fused, field="Ucorner", how=", driven into a corner")
            compare(ref, got, "%s chamfered, driven into a corner" % expect)
