"""The round of the flat walk's body without z (csrc/cpf_stream.hip, ``step_kernel_stream_flat``: its own gather walk -- four
side faces, two coordinates, on the global record --, one hook that the zero-cycle launch shares, the busy lanes carried as a wave
mask) against option ``flat_z`` 0, under which every launch runs the three-coordinate body ``step_kernel_stream<..., 8 / 9>`` that
this work does not touch, and against the CPU statement (``oracle.CellWalk``) where tests/test_gpu_flat_body.py compares with it:
the same BITS in x, y, z, the cell and the stored velocity.

What tests/test_gpu_flat_body.py leaves thin: SHUFFLED clouds of both lookups on which most rounds are gather rounds (checked on
the host: see ``_slotless``), a partial last tile and a cloud of fewer than 64 particles, clouds with fewer tiles than the grid
has waves, launches without reflection, stored velocities, and the zero-cycle launch (positions and cells come back as they went
in)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAT, STREAM = "step_kernel_stream_flat<", "step_kernel_stream<"
BIG = [(1_600_003, ", 8>"), (300_005, ", 9>")]
# small clouds around (0.05, 0) of pitzDaily, half widths in x and y: particles per occupied cell decide the lookup ("stream_lookup_by_density")
#   45 particles in 4 cells (fewer than 64: one partial tile); 5 000 in 24 cells (208 per cell: the loop lookup; 79 tiles, the last one
#   partial, far fewer than the grid's waves); 5 000 in 144 cells (35 per cell: the fixed lookup)
SMALL = [(45, 2e-4, 2e-4, ", 9>"), (5000, 2e-3, 1e-3, ", 8>"), (5000, 4e-3, 4e-3, ", 9>")]


@pytest.fixture(scope="module")
def setup(pitz, oracle_libs, gpu_ctx_factory):
    cw = oracle_libs.CellWalk()
    mesh = pitz["mesh"]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh)
    ctx.set_option("stats", 0)
    ctx.set_option("sort_interval", 0)                               # a shuffled cloud stays shuffled
    yield dict(cw=cw, mesh=mesh, tables=cw.build(mesh), ctx=ctx, pz=pitz["pz"], pitz=pitz)
    ctx.set_option("stream_lookup_by_density", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what=""):
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(p), _bits(q)), (what, k, int((_bits(p) != _bits(q)).sum()))


def _by_id(ctx, want_vel=False):
    if want_vel:
        xyzw, cell, vel = ctx.get_particles(True)
        return xyzw[:, :3].copy(), cell.copy(), vel[:, :3].copy()
    xyzw, cell = ctx.get_particles()
    return xyzw[:, :3].copy(), cell.copy()


def _reset(ctx, U, flat_z):
    ctx.set_option("step_variant", -1); ctx.set_option("stream_lookup", -1); ctx.set_option("flat_walk", 1)
    ctx.set_option("flat_z", flat_z); ctx.set_option("stats", 0)
    ctx.set_velocity(U)


def _cpu(setup, xyz, U, dt, cycles, cell=None):
    cw, t = setup["cw"], setup["tables"]
    x, y, z = (xyz[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads) if cell is None else cell.astype(np.int32).copy()
    cw.step(x, y, z, c, dt, cycles, t, U, nthreads=cw.max_threads)
    return np.stack([x, y, z], 1), c


def _slotless(cell, slots):
    """Per 64-particle tile of a cloud in storage order: the lanes left over when the ``slots`` most populated cells of the tile
    have a record slot each -- a lower bound of the lanes without a slot in the tile's first round."""
    full = (cell.size // 64) * 64
    tiles = cell[:full].reshape(-1, 64)[:4000]
    out = np.empty(tiles.shape[0], np.int64)
    for k, t in enumerate(tiles):
        cnt = np.sort(np.unique(t[t >= 0], return_counts=True)[1])[::-1]
        out[k] = (t >= 0).sum() - cnt[:slots].sum()
    return out


@pytest.mark.parametrize("n,want", BIG)
@pytest.mark.parametrize("field", ["U_uniform", "U_analytic"])
def test_shuffled_cloud_walks_by_gathers(setup, field, n, want):
    """A cloud in random order, never sorted: nearly every lane of a tile sits in a cell of its own, a round places four (fixed
    lookup: eight) records, so 32 or more lanes are without a slot in most rounds and the wave walks by per-lane gathers.  Single
    cycles, fused cycles, stored velocities; then launches without reflection."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"][field]
    xyz = pz.uniform_points(83, n, *pz.DOMAIN_BOX)
    xyz[::5, 2] = -0.0
    dt = 4e-4 if field == "U_uniform" else 2e-4
    got, vel, lost = {}, {}, {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz); ctx.locate_initial()
        _, cell0 = ctx.get_particles()
        # (nine slots at most: the fixed lookup's) at least 32 lanes without a slot in nine tiles of ten
        assert np.percentile(_slotless(cell0, 9), 10) >= 32
        ctx.step(dt, 0.0, 1, 0)                                     # streams z
        name = ctx.step_kernel_name(0.0, 0)
        assert name.endswith(want) and ((FLAT in name) if flat_z else (STREAM in name)), name
        ctx.step(dt, 0.0, 3, 0)
        ctx.step(dt, 0.0, 4, L.STEP_FUSE_CYCLES)
        ctx.step(dt, 0.0, 1, L.STEP_STORE_VEL)
        vel[flat_z] = _by_id(ctx, True)
        ctx.step(dt, 0.0, 3, L.STEP_STORE_VEL | L.STEP_FUSE_CYCLES)
        got[flat_z] = _by_id(ctx, True)
        ctx.step(3 * dt, 0.0, 2, L.STEP_NO_REFLECT)
        ctx.step(3 * dt, 0.0, 3, L.STEP_NO_REFLECT | L.STEP_FUSE_CYCLES | L.STEP_STORE_VEL)
        lost[flat_z] = _by_id(ctx, True)
    ctx.set_option("flat_z", 1)
    _same(vel[1], vel[0], "stored velocity, one cycle")
    _same(got[1], got[0], "flat_z 1 / 0")
    _same(lost[1], lost[0], "no reflection, flat_z 1 / 0")
    assert (lost[1][1] == L.CELL_LOST).sum() > 0
    _same(got[1][:2], _cpu(setup, xyz, U, dt, 12), "CPU statement")


@pytest.mark.parametrize("n,hx,hy,want", SMALL)
@pytest.mark.parametrize("shuffled", [False, True])
def test_small_clouds(setup, n, hx, hy, want, shuffled):
    """Fewer than 64 particles, a partial last tile, fewer tiles than the grid has waves (most waves find their group's counter
    exhausted and leave at once); both lookups, chosen by the particles per occupied cell that the sort counted."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"]["U_uniform"]
    zlo, zhi = pz.DOMAIN_BOX[0][2], pz.DOMAIN_BOX[1][2]
    xyz = pz.uniform_points(89, n, (0.05 - hx, -hy, zlo), (0.05 + hx, hy, zhi))
    xyz[::4, 2] = -0.0
    dt, got, lost = 4e-4, {}, {}
    ctx.set_option("stream_lookup_by_density", 1)
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell(); ctx.synchronize()
        if shuffled:                                                # the same cloud in the order it was drawn in; the sort's count stands
            ctx.set_particles(xyz); ctx.locate_initial()
        ctx.step(dt, 0.0, 1, 0)                                     # streams z
        name = ctx.step_kernel_name(0.0, 0)
        assert name.endswith(want) and ((FLAT in name) if flat_z else (STREAM in name)), name
        ctx.step(dt, 0.0, 2, 0)
        ctx.step(dt, 0.0, 5, L.STEP_FUSE_CYCLES)
        ctx.step(dt, 0.0, 2, L.STEP_STORE_VEL)
        got[flat_z] = _by_id(ctx, True)
        ctx.step(20 * dt, 0.0, 2, L.STEP_NO_REFLECT)
        ctx.step(20 * dt, 0.0, 2, L.STEP_NO_REFLECT | L.STEP_FUSE_CYCLES)
        lost[flat_z] = _by_id(ctx)
    ctx.set_option("stream_lookup_by_density", 0)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0], "flat_z 1 / 0")
    _same(lost[1], lost[0], "no reflection, flat_z 1 / 0")
    _same(got[1][:2], _cpu(setup, xyz, U, dt, 10), "CPU statement")


@pytest.mark.parametrize("n,want", BIG)
@pytest.mark.parametrize("sorted_cloud", [True, False])
def test_zero_cycle_launch_returns_what_it_loaded(setup, n, want, sorted_cloud):
    """The zero-cycle launch (loads and stores only) of the body without z: positions and cells come back bit for bit, frozen and
    lost particles included (a lost particle's cell as CPF_CELL_FROZEN, as after any launch that loads it), under either setting
    of flat_z, and the steps after it give the same bits under both."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"]["U_uniform"]
    xyz = pz.uniform_points(97, n, *pz.DOMAIN_BOX)
    dt, got = 4e-4, {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz); ctx.locate_initial()
        _, live = ctx.get_particles()
        ctx.set_particles(xyz, np.where(np.arange(n) % 11 == 0, L.CELL_FROZEN, live).astype(np.int32))
        if sorted_cloud:
            ctx.sort_by_cell()
        ctx.step(6 * dt, 0.0, 2, L.STEP_NO_REFLECT)                 # streams z, then loses particles at the walls
        name = ctx.step_kernel_name(0.0, 0)
        assert name.endswith(want) and ((FLAT in name) if flat_z else (STREAM in name)), name
        before = _by_id(ctx)
        assert (before[1] == L.CELL_LOST).sum() > 0 and (before[1] == L.CELL_FROZEN).sum() >= n // 11
        ctx.step(dt, 0.0, 0, L.STEP_FUSE_CYCLES)
        ctx.step(dt, 0.0, 0, L.STEP_FUSE_CYCLES | L.STEP_NO_REFLECT)
        name = ctx.step_kernel_name(0.0, 0)
        assert (FLAT in name) if flat_z else (STREAM in name), name  # a zero-cycle launch unsettles nothing
        # (a particle lost in one launch is stored as frozen by the next launch that loads it, whatever that launch does)
        _same(_by_id(ctx), (before[0], np.where(before[1] == L.CELL_LOST, L.CELL_FROZEN, before[1]).astype(np.int32)),
              "zero cycles, flat_z %d" % flat_z)
        ctx.step(dt, 0.0, 2, 0)
        got[flat_z] = _by_id(ctx)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0], "flat_z 1 / 0")
