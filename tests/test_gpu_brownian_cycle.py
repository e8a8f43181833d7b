"""GPU: the kicked cycle (cpf_step / cpf_step_dev with D > 0) -- every one of the 64 instantiations step_kernel_stream<true, REFLECT,
STORE_VEL, STATS, LOOKUP> and every other route the library has to the same result -- against a CPU statement, BIT FOR BIT: positions
(compared as int64 bits), cells (CPF_CELL_LOST and CPF_CELL_FROZEN included), stored velocities, and with statistics on the visit,
reflection, lost and particle-step counters, after 1, 6 and 20 cycles, no tolerance, no particle left out.

What makes that possible: the kick's deviates are a pure function of (gid, step, seed), so they are taken from the device as data
and handed to CellWalk.step_given (oracle/cellwalk.c, cw_step_given; tests/browniancycle.py has the two extractors and the cases).
What remains between the device and libm is the deviates themselves, held here to 2e-5 over 320 000 (gid, step) pairs -- the bar
test_tail_of_the_deviates_reaches_beyond_the_23_bit_cap has for one 5.9 sigma deviate; a wrong Philox word is an O(1) difference.

Before each comparison the test asserts the exact name of the kernel the launch ran; part (a) meets every one of

    cpf::step_kernel_stream<true, false, false, false, 0>
    cpf::step_kernel_stream<true, false, false, true, 0>
    cpf::step_kernel_stream<true, false, true, false, 0>
    cpf::step_kernel_stream<true, false, true, true, 0>
    cpf::step_kernel_stream<true, true, false, false, 0>
    cpf::step_kernel_stream<true, true, false, true, 0>
    cpf::step_kernel_stream<true, true, true, false, 0>
    cpf::step_kernel_stream<true, true, true, true, 0>
    cpf::step_kernel_stream<true, false, false, false, 1>
    cpf::step_kernel_stream<true, false, false, true, 1>
    cpf::step_kernel_stream<true, false, true, false, 1>
    cpf::step_kernel_stream<true, false, true, true, 1>
    cpf::step_kernel_stream<true, true, false, false, 1>
    cpf::step_kernel_stream<true, true, false, true, 1>
    cpf::step_kernel_stream<true, true, true, false, 1>
    cpf::step_kernel_stream<true, true, true, true, 1>
    cpf::step_kernel_stream<true, false, false, false, 2>
    cpf::step_kernel_stream<true, false, false, true, 2>
    cpf::step_kernel_stream<true, false, true, false, 2>
    cpf::step_kernel_stream<true, false, true, true, 2>
    cpf::step_kernel_stream<true, true, false, false, 2>
    cpf::step_kernel_stream<true, true, false, true, 2>
    cpf::step_kernel_stream<true, true, true, false, 2>
    cpf::step_kernel_stream<true, true, true, true, 2>
    cpf::step_kernel_stream<true, false, false, false, 3>
    cpf::step_kernel_stream<true, false, false, true, 3>
    cpf::step_kernel_stream<true, false, true, false, 3>
    cpf::step_kernel_stream<true, false, true, true, 3>
    cpf::step_kernel_stream<true, true, false, false, 3>
    cpf::step_kernel_stream<true, true, false, true, 3>
    cpf::step_kernel_stream<true, true, true, false, 3>
    cpf::step_kernel_stream<true, true, true, true, 3>
    cpf::step_kernel_stream<true, false, false, false, 4>
    cpf::step_kernel_stream<true, false, false, true, 4>
    cpf::step_kernel_stream<true, false, true, false, 4>
    cpf::step_kernel_stream<true, false, true, true, 4>
    cpf::step_kernel_stream<true, true, false, false, 4>
    cpf::step_kernel_stream<true, true, false, true, 4>
    cpf::step_kernel_stream<true, true, true, false, 4>
    cpf::step_kernel_stream<true, true, true, true, 4>
    cpf::step_kernel_stream<true, false, false, false, 5>
    cpf::step_kernel_stream<true, false, false, true, 5>
    cpf::step_kernel_stream<true, false, true, false, 5>
    cpf::step_kernel_stream<true, false, true, true, 5>
    cpf::step_kernel_stream<true, true, false, false, 5>
    cpf::step_kernel_stream<true, true, false, true, 5>
    cpf::step_kernel_stream<true, true, true, false, 5>
    cpf::step_kernel_stream<true, true, true, true, 5>
    cpf::step_kernel_stream<true, false, false, false, 6>
    cpf::step_kernel_stream<true, false, false, true, 6>
    cpf::step_kernel_stream<true, false, true, false, 6>
    cpf::step_kernel_stream<true, false, true, true, 6>
    cpf::step_kernel_stream<true, true, false, false, 6>
    cpf::step_kernel_stream<true, true, false, true, 6>
    cpf::step_kernel_stream<true, true, true, false, 6>
    cpf::step_kernel_stream<true, true, true, true, 6>
    cpf::step_kernel_stream<true, false, false, false, 11>
    cpf::step_kernel_stream<true, false, false, true, 11>
    cpf::step_kernel_stream<true, false, true, false, 11>
    cpf::step_kernel_stream<true, false, true, true, 11>
    cpf::step_kernel_stream<true, true, false, false, 11>
    cpf::step_kernel_stream<true, true, false, true, 11>
    cpf::step_kernel_stream<true, true, true, false, 11>
    cpf::step_kernel_stream<true, true, true, true, 11>

(test_part_a_names_are_the_64_of_the_header checks the list against the parametrisation).

(a) All 64 by name, on the smallest meshes that reach their lookups (tests/browniancycle.py, MESHES): the 24-cell sheared block
    (LOOKUP 0, 1, 4 by cloud size; also clouds of 1 and 65), 720 graded boxes (6; "box_records" 0: 1), the 2:1-refined box (11;
    "box_records" 0: 3; and "stream_lookup" 0: 5), the cut-corner and the chamfered grid (2: two-record and header cells).  Clouds
    ordered by cell with gid a permutation -- the product's layout -- and, for two flag sets per case, as drawn with gid == NULL.
(b) One cell thick in z -- pitzDaily and box_mesh(6, 5, 1) --: option "z_fold" 1 against step_given(zfold = 1), which states
    fold_z of csrc/cpf_walk.h, and "z_fold" 0 against zfold = 0, the reference's order; LOOKUP 0, 1 and 4.
(c) Every route gives the CPU's bits: step variants 0 and 3, twenty single-cycle launches, the context's own cloud sorted, shuffled
    and re-sorted on the way, gids beyond 2^32, a velocity refresh between two launches (gid == NULL: the as-drawn clouds of (a) and
    (b), pitzDaily among them); every cloud begins with lost and frozen lanes at those of positions 5, 64 and 130 that it has.
(d) The inputs go through the hard paths, asserted on the CPU statement's own counters for the very deviates of the run: face
    crossings, wall reflections, two walls in a cycle, three crossings in a cycle, losses without reflection, z mirrorings."""
import itertools
import types

import numpy as np
import pytest

import browniancycle as B
from cudaparticlesfoam_amd import _lib as L

pytestmark = pytest.mark.gpu

_TF = ("false", "true")
KERNELS = frozenset(line.strip() for line in __doc__.splitlines() if line.strip().startswith("cpf::step_kernel_stream<true,"))
LOOKUPS = (0, 1, 2, 3, 4, 5, 6, 11)
ALL8 = tuple(itertools.product((1, 0), (0, 1), (0, 1)))            # (reflect, store velocities, statistics)
FOUR = ((1, 0, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1))                # REFLECT x {lean, STORE_VEL + STATS}
AS_DRAWN = ((1, 0, 0), (0, 1, 1))                                  # what also runs on the cloud as drawn, gid == NULL
DEFAULTS = (("stream_lookup", -1), ("box_records", 1), ("z_fold", 1), ("step_variant", -1), ("sort_interval", 50), ("stats", 1))
N_BASE = 6000                                                      # the largest cloud here
GID_OFFSET = 5 * 10 ** 9                                           # beyond 2^32: the Philox counter's second word is 1
N_OFFSET = 4000


def _stream(reflect, sv, st, lookup):
    return "cpf::step_kernel_stream<true, %s, %s, %s, %d>" % (_TF[reflect], _TF[sv], _TF[st], lookup)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# The module's contexts (one per mesh, and the one-cell mesh of the extractor), the device's deviates and the CPU results, shared by
# the tests of this file.  The contexts come from gpu_ctx_factory, which is session-scoped and would keep them to the session's end:
# _module_state closes them and drops everything when the file's last test has run.
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for key, value in list(_state.items()):
        if key == "one cell" or (isinstance(key, tuple) and key[0] == "ctx"):
            value.close()                    # (closing twice is harmless: the factory's own teardown finds the handle gone)
    _state.clear()


def _ctx(name, make):
    if ("ctx", name) not in _state:
        c = B.case(name)
        ctx = make()
        ctx.set_mesh(c.mesh); ctx.set_velocity(c.U); ctx.set_seed(B.SEED)
        _state["ctx", name] = ctx
    return _state["ctx", name]


def _one_cell(make):
    if "one cell" not in _state:
        _state["one cell"] = B.one_cell_context(make)
    return _state["one cell"]


def _base(make, step0):
    """the device's deviates for gid = 0 .. N_BASE - 1 at steps step0 .. step0 + 19, through the kernels' gid == NULL path"""
    if ("base", step0) not in _state:
        _state["base", step0] = B.fused_deviates(_one_cell(make), None, N_BASE, step0, 20)
    return _state["base", step0]


def _offset(make):
    if "offset" not in _state:
        _state["offset"] = B.fused_deviates(_one_cell(make), np.arange(N_OFFSET, dtype=np.int64) + GID_OFFSET, N_OFFSET, B.STEP0, 20)
    return _state["offset"]


def _deviates(make, gid, step0):
    """xi [20][n][3] by array position for the ids `gid`"""
    if gid.size and gid.min() >= GID_OFFSET:
        assert step0 == B.STEP0
        return np.ascontiguousarray(_offset(make)[:, gid - GID_OFFSET])
    return np.ascontiguousarray(_base(make, step0)[:, gid])


def _ref(make, name, n, sort, reflect, zfold=0, offset=False, refresh_after=None, step0=B.STEP0):
    """(snapshots, diag) of the CPU statement on the DEVICE's deviates for this cloud"""
    key = ("ref", name, n, sort, reflect, zfold, offset, refresh_after, step0)
    if key not in _state:
        xyz, cell0, gid = B.cloud(name, n, sort=sort)
        xi = _deviates(make, gid + (GID_OFFSET if offset else 0), step0)
        _state[key] = B.run_cpu(B.case(name), xyz, cell0, xi, reflect=reflect, zfold=zfold, refresh_after=refresh_after)
    return _state[key]


def _flags(reflect, sv, fused=True):
    return (0 if reflect else L.STEP_NO_REFLECT) | (L.STEP_STORE_VEL if sv else 0) | (L.STEP_FUSE_CYCLES if fused else 0)


def _set(ctx, opts):
    for k, v in opts:
        ctx.set_option(k, v)


def gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, opts=(), fused=True, checkpoints=B.CHECKPOINTS, refresh_after=None):
    """{k: (xyz, cell, vel | None, counters | None)} after k cycles of cpf_step_dev on device arrays, the kick's step counter
    running from B.STEP0; `expect`: the kernel name every launch must report."""
    out, done = {}, 0
    _set(ctx, (("stats", st),) + tuple(opts))
    dc = B.DeviceCloud(ctx, xyz, cell0, gid)
    try:
        for k in checkpoints:
            before = ctx.counters()
            dc.step(c.dt, c.D, B.STEP0 + done, k - done, _flags(reflect, sv, fused), store_vel=bool(sv))
            name = ctx.step_kernel_name(c.D, _flags(reflect, sv, fused))
            assert name == expect, (name, expect)
            after = ctx.counters()
            done = k
            p, cell, vel = dc.get()
            out[k] = (p, cell, vel if sv else None, {q: after[q] - before[q] for q in after} if st else None)
            if refresh_after == k:
                ctx.set_velocity(c.U2)
    finally:
        dc.close()
        if refresh_after is not None:
            ctx.set_velocity(c.U)
        _set(ctx, DEFAULTS)
    print("ran %s: %s n=%d%s" % (expect, c.name, xyz.shape[0], "" if fused else " single-cycle launches"))
    return out


def compare(ref, got, what, vel_live_at=None):
    """positions as bits, cells, stored velocities as bits, the four counters: equal, for every particle"""
    for k in got:
        p, cell, vel, cnt = got[k]
        s = ref[k]
        bad = np.nonzero(cell != s.cell)[0]
        assert bad.size == 0, (what, k, "cells differ", bad.size, bad[:5], cell[bad[:5]], s.cell[bad[:5]])
        bad = np.nonzero((_bits(p) != _bits(s.xyz)).any(1))[0]
        assert bad.size == 0, (what, k, "positions differ", bad.size, bad[:5], p[bad[:5]], s.xyz[bad[:5]])
        if vel is not None:
            m = slice(None) if vel_live_at is None else vel_live_at[k]
            bad = np.nonzero((_bits(vel[m]) != _bits(s.vel[m])).any(1))[0]
            assert bad.size == 0, (what, k, "stored velocities differ", bad.size, bad[:5], vel[m][bad[:5]], s.vel[m][bad[:5]])
        if cnt is not None:
            want = dict(cells_visited=s.stats[0], reflections=s.stats[1], lost=s.stats[2], particle_steps=s.stats[3])
            assert cnt == want, (what, k, cnt, want)


def assert_hard_paths(name, diag, ref_noreflect=None):
    """(d): the run being compared did go where the kernels are hard"""
    hp = B.hard_paths(diag)
    print("MEASURED %s | %s" % (name, hp))
    assert hp["crossing"] >= 0.10 and hp["reflecting"] >= 0.01 and hp["three_hops"] >= 1, hp
    if name in B.MESHES_THIN:
        assert hp["folded"] >= 0.20 and hp["folded_twice"] >= 1, hp
    else:
        assert hp["two_walls"] >= 1, hp
        assert (ref_noreflect[20].cell < 0).mean() >= 0.01


# ------------------------------------------------------------------------------------------------ the deviates
def test_the_two_extractors_agree_and_the_deviates_are_libms_to_2e_5(gpu_ctx_factory, oracle_libs):
    """320 000 (gid, step) pairs: gid 0 .. 5999 at steps 0 .. 19 and 1000 .. 1019 (the kernels' gid == NULL path), 5e9 .. 5e9 + 3999 at
    1000 .. 1019 (a gid array; the counter's second word).  The staged route gives the same BITS as the fused one where both apply,
    a gid array the same bits as gid == NULL, and everything is within 2e-5 of cw_normal3."""
    make = gpu_ctx_factory
    base, base0, off = _base(make, B.STEP0), _base(make, 0), _offset(make)
    staged = B.staged_deviates(_one_cell(make), N_BASE, B.STEP0, 20)
    assert np.array_equal(_bits(staged), _bits(base))
    perm = np.random.default_rng(1).permutation(N_BASE).astype(np.int64)[:4000]
    by_gid = B.fused_deviates(_one_cell(make), perm, perm.size, B.STEP0, 2)
    assert np.array_equal(_bits(by_gid), _bits(base[:2, perm]))
    worst, pairs = 0.0, 0
    for dev, gids, step0 in ((base, np.arange(N_BASE), B.STEP0), (base0, np.arange(N_BASE), 0), (off, np.arange(N_OFFSET) + GID_OFFSET, B.STEP0)):
        want = B.libm_deviates(gids, step0, 20)
        err = float(np.abs(dev - want).max())
        print("MEASURED deviates | gid %d.. step %d.. | %d pairs | max |xi_device - cw_normal3| %.3e | max |xi| %.3f"
              % (gids[0], step0, 20 * gids.size, err, np.abs(dev).max()))
        worst, pairs = max(worst, err), pairs + 20 * gids.size
        assert np.abs(dev).max() < 6.77
    assert not np.array_equal(base, base0) and not np.array_equal(base[:, :N_OFFSET], off)      # the step and the high word do count
    print("MEASURED deviates | %d pairs | max |xi_device - cw_normal3| %.3e" % (pairs, worst))
    assert pairs >= 200_000 and worst < 2e-5, worst


# ------------------------------------------------------------------------------------------------ (a)
# (mesh, cloud size, LOOKUP the launch must run, options, flag sets)
A_RUNS = [
    ("block A", 3137, 0, (), ALL8),                                 # 24 cells: n >= 128 * 24
    ("block A", 3000, 1, (), ALL8),                                 # ... below it
    ("block A", 150, 4, (), ALL8),                                  # ... below 8 * 24
    ("block A", 65, 4, (), FOUR),                                   # a tile and one lane
    ("block A", 1, 4, (), FOUR),
    ("graded box", 4000, 6, (), ALL8),
    ("graded box", 6000, 1, (("box_records", 0),), FOUR),           # (n >= 8 * 720: below it the sparse lookup takes over)
    ("refined box", 4000, 11, (), ALL8),
    ("refined box", 4000, 3, (("box_records", 0),), ALL8),
    ("refined box", 4000, 5, (("box_records", 0), ("stream_lookup", 0)), ALL8),
    ("cut corners", 4000, 2, (), ALL8),
    ("chamfered", 4000, 2, (), FOUR),
]


def test_part_a_names_are_the_64_of_the_header():
    names = {_stream(r, sv, st, lookup) for _, _, lookup, _, sets in A_RUNS for r, sv, st in sets}
    assert len(KERNELS) == 64 and names == KERNELS
    assert KERNELS == {_stream(r, sv, st, lookup) for lookup in LOOKUPS for r, sv, st in ALL8}
    assert 3137 >= 128 * 24 > 3000 >= 8 * 24 > 150 and 6000 >= 8 * 720 > 4000
    print("all 64 kicked instantiations of step_kernel_stream are asserted by name in part (a)")


@pytest.mark.parametrize("name,n,lookup,opts,flagsets", A_RUNS, ids=["%s-n%d-lookup%d" % r[:3] for r in A_RUNS])
def test_a_every_kicked_instantiation_against_the_cpu_statement(name, n, lookup, opts, flagsets, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    if name == "block A":
        assert c.mesh.n_cells == 24
    for sort in (True, False):
        xyz, cell0, gid = B.cloud(name, n, sort=sort)
        for reflect, sv, st in (flagsets if sort else AS_DRAWN):
            expect = _stream(reflect, sv, st, lookup)
            assert expect in KERNELS
            ref, _ = _ref(gpu_ctx_factory, name, n, sort, reflect)
            got = gpu_run(ctx, c, xyz, cell0, gid if sort else None, reflect, sv, st, expect, opts)
            compare(ref, got, "%s n=%d %s" % (expect, n, "by cell, gid a permutation" if sort else "as drawn, gid NULL"))
    if n >= 3000:
        assert_hard_paths(name, _ref(gpu_ctx_factory, name, n, True, 1)[1], _ref(gpu_ctx_factory, name, n, True, 0)[0])


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("lookup", [0, 1, 4])
@pytest.mark.parametrize("name", B.MESHES_THIN)
def test_b_one_cell_thick_in_z_with_and_without_the_fold(name, lookup, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    refs = {}
    for fold in (1, 0):
        ctx.set_option("z_fold", fold)
        assert ctx.mesh_flags()["z_thin"] == fold and ctx.mesh_flags()["all_hex"] == 1           # the kernels fold iff this flag is set
        ctx.set_option("z_fold", 1)
        refs[fold], diag = _ref(gpu_ctx_factory, name, n, True, 1, zfold=fold)
        if fold:
            assert_hard_paths(name, diag)
        for reflect, sv, st in ((1, 0, 0), (1, 1, 1)):
            expect = _stream(reflect, sv, st, lookup)
            got = gpu_run(ctx, c, xyz, cell0, gid, reflect, sv, st, expect, (("stream_lookup", lookup), ("z_fold", fold)))
            compare(refs[fold], got, "%s %s z_fold %d" % (expect, name, fold))
        # ... and the cloud as drawn with gid == NULL: the fold (and the wave-uniform zUnclear vote) on waves that hold up to 64 cells
        drawn, cell_drawn, _ = B.cloud(name, n, sort=False)
        expect = _stream(1, 1, 1, lookup)
        got = gpu_run(ctx, c, drawn, cell_drawn, None, 1, 1, 1, expect, (("stream_lookup", lookup), ("z_fold", fold)))
        compare(_ref(gpu_ctx_factory, name, n, False, 1, zfold=fold)[0], got, "%s %s z_fold %d, as drawn, gid NULL" % (expect, name, fold))
    # the two orders are not the same bits (so each run was held to its own statement), and a rounding apart where the cell agrees
    a, b = refs[1][1], refs[0][1]
    assert not np.array_equal(_bits(a.xyz), _bits(b.xyz))
    same = a.cell == b.cell
    assert same.mean() >= 0.999 and np.abs(a.xyz - b.xyz)[same].max() < 1e-12


# ------------------------------------------------------------------------------------------------ (c)
C_MESHES = ("graded box", "pitzDaily")


def _zfold(name):
    return 1 if name in B.MESHES_THIN else 0


def _auto_lookup(name):
    return {"graded box": 6, "pitzDaily": 4}[name]                 # 4000 particles: box records; 12 225 hexes with fewer than 8 each


@pytest.mark.parametrize("variant", [4, 3, 0])
@pytest.mark.parametrize("name", C_MESHES)
def test_c_step_variants(name, variant, gpu_ctx_factory, oracle_libs):
    """the streaming kernel, the wave-cooperative one and the generic walk: reflecting and not, velocities stored, statistics on"""
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    for reflect in (1, 0):
        expect = {4: _stream(reflect, 1, 1, _auto_lookup(name)), 3: "cpf::step_kernel_coop<true, %s, true, true>" % _TF[reflect],
                  0: "cpf::step_kernel<0, true, %s, true>" % _TF[reflect]}[variant]
        ref, _ = _ref(gpu_ctx_factory, name, n, True, reflect, zfold=_zfold(name) if reflect else 0)
        got = gpu_run(ctx, c, xyz, cell0, gid, reflect, 1, 1, expect, (("step_variant", variant),))
        compare(ref, got, "%s %s" % (expect, name))


@pytest.mark.parametrize("name", C_MESHES)
def test_c_twenty_single_cycle_launches_and_one_fused_launch(name, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    ref, _ = _ref(gpu_ctx_factory, name, n, True, 1, zfold=_zfold(name))
    end = ref[20]                            # (its counters are those since the sixth cycle: the launches here run all twenty)
    ref = {20: types.SimpleNamespace(xyz=end.xyz, cell=end.cell, vel=end.vel, stats=[sum(ref[k].stats[q] for k in B.CHECKPOINTS) for q in range(4)])}
    expect = _stream(1, 1, 1, _auto_lookup(name))
    for fused in (True, False):
        got = gpu_run(ctx, c, xyz, cell0, gid, 1, 1, 1, expect, fused=fused, checkpoints=(20,))
        compare(ref, got, "%s %s %s" % (expect, name, "one launch of 20" if fused else "20 launches of 1"))


@pytest.mark.parametrize("name", C_MESHES)
def test_c_gids_beyond_32_bits_and_a_velocity_refresh(name, gpu_ctx_factory, oracle_libs):
    c, ctx = B.case(name), _ctx(name, gpu_ctx_factory)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=True)
    expect = _stream(1, 1, 1, _auto_lookup(name))
    ref, _ = _ref(gpu_ctx_factory, name, n, True, 1, zfold=_zfold(name), offset=True)
    plain, _ = _ref(gpu_ctx_factory, name, n, True, 1, zfold=_zfold(name))
    assert not np.array_equal(ref[1].xyz, plain[1].xyz)                                          # other ids, other kicks
    got = gpu_run(ctx, c, xyz, cell0, gid + GID_OFFSET, 1, 1, 1, expect)
    compare(ref, got, "%s %s gid + 5e9" % (expect, name))
    # the field changes behind the sixth cycle (cpf_set_velocity between two launches)
    ref, _ = _ref(gpu_ctx_factory, name, n, True, 1, zfold=_zfold(name), refresh_after=6)
    assert np.array_equal(ref[6].xyz, plain[6].xyz) and not np.array_equal(ref[20].xyz, plain[20].xyz)
    got = gpu_run(ctx, c, xyz, cell0, gid, 1, 1, 1, expect, refresh_after=6)
    compare(ref, got, "%s %s velocity refresh" % (expect, name))


@pytest.mark.parametrize("how", ["sorted", "shuffled", "re-sorted on the way"])
@pytest.mark.parametrize("name", C_MESHES)
def test_c_the_contexts_own_cloud(name, how, gpu_ctx_factory, oracle_libs):
    """cpf_step on the context's own cloud: its step counter runs from 0 and its ids are the positions the particles were set with,
    whatever cpf_sort_by_cell does to the arrays -- before the first launch, never ("sort_interval" 0), or every three cycles."""
    c = B.case(name)
    n = 4000
    xyz, cell0, gid = B.cloud(name, n, sort=False)
    ref, _ = _ref(gpu_ctx_factory, name, n, False, 1, zfold=_zfold(name), step0=0)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", 3 if how == "re-sorted on the way" else 0)
    ctx.set_mesh(c.mesh); ctx.set_velocity(c.U); ctx.set_seed(B.SEED)
    ctx.set_particles(xyz, cell0)
    if how == "sorted":
        ctx.sort_by_cell()
    got, live_at, done = {}, {}, 0
    live = cell0 >= 0
    for k in B.CHECKPOINTS:
        before = ctx.counters()
        ctx.step(c.dt, c.D, k - done, L.STEP_STORE_VEL | L.STEP_FUSE_CYCLES)
        name_ran = ctx.step_kernel_name(c.D, L.STEP_STORE_VEL | L.STEP_FUSE_CYCLES)
        assert name_ran.startswith("cpf::step_kernel_stream<true, true, true, true, "), name_ran
        after = ctx.counters()
        done = k
        xyzw, cell, vel = ctx.get_particles(want_vel=True)
        assert np.array_equal(xyzw[:, 3] == 0, cell == L.CELL_FROZEN)
        got[k] = (xyzw[:, :3].copy(), cell, vel[:, :3].copy(), {q: after[q] - before[q] for q in after})
        live_at[k] = live                        # (a frame holds the velocities of the particles that launch stepped, zero for the others)
        assert not vel[~live, :3].any()
        live = cell >= 0
    ctx.close()
    compare(ref, got, "cpf_step, %s, %s" % (name, how), vel_live_at=live_at)
