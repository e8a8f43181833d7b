"""The flat walk's body without z (csrc/cpf_stream.hip, ``step_kernel_stream_flat``: what a flat launch on a cloud with settled z
runs) against option ``flat_z`` 0 -- every launch streams z through ``step_kernel_stream<..., 8 / 9>`` -- and against the CPU
statement (``oracle.CellWalk``): the same BITS in x, y, z and the cell.  pitzDaily, both fields, both lookups (cloud sizes that
give ", 8>" and ", 9>", n % 64 != 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(1_600_003, ", 8>"), (300_005, ", 9>")]
FLAT, STREAM = "step_kernel_stream_flat<", "step_kernel_stream<"


@pytest.fixture(scope="module")
def setup(pitz, oracle_libs, gpu_ctx_factory):
    cw = oracle_libs.CellWalk()
    mesh = pitz["mesh"]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh)
    ctx.set_option("stats", 0)
    return dict(cw=cw, mesh=mesh, tables=cw.build(mesh), ctx=ctx, pz=pitz["pz"], pitz=pitz)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what=""):
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(_bits(p), _bits(q)), (what, k, int((_bits(p) != _bits(q)).sum()))


def _by_id(ctx):
    xyzw, cell = ctx.get_particles()                                # (particle-id order)
    return xyzw[:, :3].copy(), cell.copy()


def _cloud(pz, n, seed):
    """Uniform over the fluid's box; z on the front / back planes and -0.0 in between (the first streaming cycle makes it +0.0)."""
    xyz = pz.uniform_points(seed, n, *pz.DOMAIN_BOX)
    zlo, zhi = pz.DOMAIN_BOX[0][2], pz.DOMAIN_BOX[1][2]
    assert zlo < 0.0 < zhi
    xyz[::7, 2] = zlo; xyz[1::7, 2] = zhi
    xyz[2::7, 2] = -0.0
    return xyz


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


@pytest.mark.parametrize("n,want", SIZES)
@pytest.mark.parametrize("field", ["U_uniform", "U_analytic"])
@pytest.mark.parametrize("sorted_cloud", [True, False])
def test_flat_body_bit_exact(setup, field, n, want, sorted_cloud):
    """Single-cycle and fused launches on a cloud kept sorted and on one that is not (the per-lane gather walk), -0.0 injected
    before the launch that streams z; then launches without reflection (flat_z 0 only: the CPU statement always reflects)."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"][field]
    xyz = _cloud(pz, n, 47)
    dt = 4e-4 if field == "U_uniform" else 2e-4
    got, lost = {}, {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz); ctx.locate_initial()
        if sorted_cloud:
            ctx.sort_by_cell()
        assert STREAM in ctx.step_kernel_name(0.0, 0)              # (the lookup goes by the most recent launch's particle count)
        ctx.step(dt, 0.0, 1, 0)                                     # streams z
        name = ctx.step_kernel_name(0.0, 0)
        assert name.endswith(want) and ((FLAT in name) if flat_z else (STREAM in name)), name
        ctx.step(dt, 0.0, 2, 0)                                     # two single-cycle launches without z
        ctx.step(dt, 0.0, 5, L.STEP_FUSE_CYCLES)                    # one fused launch
        ctx.step(dt, 0.0, 1, 0)
        got[flat_z] = _by_id(ctx)
        ctx.step(3 * dt, 0.0, 3, L.STEP_NO_REFLECT)
        ctx.step(3 * dt, 0.0, 3, L.STEP_NO_REFLECT | L.STEP_FUSE_CYCLES)
        lost[flat_z] = _by_id(ctx)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0], "flat_z 1 / 0")
    _same(lost[1], lost[0], "no reflection, flat_z 1 / 0")
    assert (lost[1][1] == L.CELL_LOST).sum() > 0
    ref = _cpu(setup, xyz, U, dt, 9)
    _same(got[1], ref, "CPU statement")
    neg0 = (xyz[:, 2] == 0.0) & np.signbit(xyz[:, 2]) & (ref[1] >= 0)
    assert neg0.sum() > 0 and not np.signbit(got[1][0][neg0, 2]).any()


@pytest.mark.parametrize("n,want", SIZES)
def test_frozen_and_lost_particles_keep_their_bytes(setup, n, want):
    """A cloud a third of which is frozen (with -0.0 in z, which a frozen particle keeps) and which loses particles at the walls on the
    way: no-reflect launches, then reflecting ones over the survivors."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"]["U_uniform"]
    xyz = _cloud(pz, n, 53)
    xyz[::3, 2] = -0.0
    dt = 4e-4
    got = {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz); ctx.locate_initial()
        _, live = ctx.get_particles()
        seeded = np.where(np.arange(n) % 3 == 0, L.CELL_FROZEN, live).astype(np.int32)
        ctx.set_particles(xyz, seeded); ctx.sort_by_cell()
        ctx.step(4 * dt, 0.0, 1, L.STEP_NO_REFLECT)                 # streams z
        ctx.step(4 * dt, 0.0, 4, L.STEP_NO_REFLECT)
        ctx.step(dt, 0.0, 3, 0)
        ctx.step(dt, 0.0, 4, L.STEP_FUSE_CYCLES)
        got[flat_z] = _by_id(ctx)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0])
    froz = np.arange(n) % 3 == 0
    assert np.array_equal(_bits(got[1][0][froz]), _bits(xyz[froz])) and (got[1][1][froz] == L.CELL_FROZEN).all()
    # (a particle lost in one launch is stored as frozen by the next one that loads it)
    assert 0 < (got[1][1] >= 0).sum() < (seeded >= 0).sum()


@pytest.mark.parametrize("n,want", SIZES)
def test_long_run_into_the_outlet_wall(setup, n, want):
    """300 cycles of the uniform field with every boundary reflecting: the whole cloud drifts into the outlet wall and bounces there
    (whole tiles reflect, up to five times a cycle; some particles are lost on the fifth bounce)."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"]["U_uniform"]
    xyz = _cloud(pz, n, 59)
    dt, got = 4e-4, {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_option("stats", 1)
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        c0 = ctx.counters()
        for k in range(10):
            ctx.step(dt, 0.0, 10, 0)
            ctx.step(dt, 0.0, 20, L.STEP_FUSE_CYCLES)
            ctx.sort_by_cell()
        c1 = ctx.counters()
        got[flat_z] = _by_id(ctx) + (np.int64(c1["reflections"] - c0["reflections"]),)
        ctx.set_option("stats", 0)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0])
    assert got[1][2] > 10 * n                                        # many reflections
    _same(got[1][:2], _cpu(setup, xyz, U, dt, 300), "CPU statement")


def test_non_finite_z_at_a_wall(setup):
    """Live particles with z of +-inf and NaN, placed to meet the outlet wall in their third and fourth cycle.  The flat walk's face
    tests do not read z, so such a particle reaches the wall; the mirror's signed distance ``dot3(plane, E) - w`` then has the term
    nz * NaN and the particle's x and y become NaN.  A launch without z cannot do that (it reflects as if z were 0): a cloud that
    holds such a particle is therefore never called settled -- the launch that streams z reports it -- and flat_z 1 runs the
    streaming kernel for it, launch after launch: the same bits as flat_z 0.  (The CPU statement walks in three dimensions: every
    one of its face tests has a NaN denominator for such a particle, which then never meets a face at all; it is compared on the
    particles with finite z only.)"""
    pz, ctx = setup["pz"], setup["ctx"]
    U = setup["pitz"]["U_uniform"]
    n, dt = 1_600_003, 4e-4
    xyz = _cloud(pz, n, 61)
    ux = float(U[0, 0])
    assert ux > 0.0
    bad = np.arange(5, n, 1009)
    xyz[bad, 0] = pz.DOMAIN_BOX[1][0] - ux * dt * (2.25 + (np.arange(bad.size) % 2))      # third / fourth cycle
    xyz[bad, 1] = 0.004 * ((np.arange(bad.size) % 5) - 2)
    finite_z = xyz[:, 2].copy()
    cells = setup["cw"].locate_initial(xyz[:, 0].copy(), xyz[:, 1].copy(), finite_z.copy(), setup["tables"], nthreads=setup["cw"].max_threads)
    assert (cells[bad] >= 0).all()
    xyz[bad[0::3], 2] = np.inf; xyz[bad[1::3], 2] = -np.inf; xyz[bad[2::3], 2] = np.nan
    got = {}
    for flat_z in (1, 0):
        _reset(ctx, U, flat_z)
        ctx.set_particles(xyz, cells); ctx.sort_by_cell()
        ctx.step(dt, 0.0, 1, 0)
        name = ctx.step_kernel_name(0.0, 0)
        assert STREAM in name and name.endswith(", 8>"), name       # not settled: a live particle's z is not finite
        ctx.step(dt, 0.0, 5, 0)
        assert STREAM in ctx.step_kernel_name(0.0, 0)
        got[flat_z] = _by_id(ctx)
    ctx.set_option("flat_z", 1)
    _same(got[1], got[0])
    p, c = got[1]
    assert np.isnan(p[bad, 2]).all()
    assert np.isnan(p[bad, 0]).all() and np.isnan(p[bad, 1]).all()  # mirrored with a NaN distance, by either setting
    ok = np.ones(n, bool); ok[bad] = False
    ref = _cpu(setup, xyz, U, dt, 6, cells)
    assert np.array_equal(_bits(p[ok]), _bits(ref[0][ok])) and np.array_equal(c[ok], ref[1][ok])
    # the same cloud without them settles as ever
    xyz[bad, 2] = finite_z[bad]
    _reset(ctx, U, 1)
    ctx.set_particles(xyz, cells); ctx.sort_by_cell(); ctx.step(dt, 0.0, 1, 0)
    assert FLAT in ctx.step_kernel_name(0.0, 0)
    ctx.step(dt, 0.0, 5, 0)
    _same(_by_id(ctx), _cpu(setup, xyz, U, dt, 6, cells))


def test_every_unsettling_event_runs_the_streaming_kernel_again(setup, gpu_ctx_factory):
    """Set, seed, revive, a launch that is not flat: the next launch runs step_kernel_stream<..., 8> again (by name, and by the bits:
    -0.0 injected with the event comes out as +0.0, as with flat_z 0), the one after it the body without z."""
    from cudaparticlesfoam_amd import _lib as L
    pz = setup["pz"]
    U = setup["pitz"]["U_uniform"]
    n, dt = 1_600_003, 4e-4
    xyz = pz.uniform_points(67, n, *pz.DOMAIN_BOX)

    def neg0(a, every, first):
        out = a.copy(); out[first::every, 2] = -0.0
        return out
    res = {}
    for flat_z in (1, 0):
        ctx = gpu_ctx_factory()
        ctx.set_option("stats", 0)
        ctx.set_mesh(setup["mesh"]); ctx.set_option("flat_z", flat_z); ctx.set_velocity(U); ctx.synchronize()
        got = []

        def settled_after(k=1):
            name = ctx.step_kernel_name(0.0, 0)
            assert STREAM in name and name.endswith(", 8>"), name
            ctx.step(dt, 0.0, k, 0)
            name = ctx.step_kernel_name(0.0, 0)
            assert ((FLAT in name) if flat_z else (STREAM in name)) and name.endswith(", 8>"), name
            ctx.step(dt, 0.0, 2, 0)
            got.append(_by_id(ctx))
        # set
        ctx.set_particles(neg0(xyz, 5, 3)); ctx.locate_initial(); ctx.sort_by_cell()
        settled_after()
        ctx.set_particles(neg0(xyz, 4, 1)); ctx.locate_initial(); ctx.sort_by_cell()
        settled_after(2)
        # seed: the cells come with the particles
        live = neg0(xyz, 6, 2)
        ctx.set_particles(live); ctx.locate_initial()
        _, cell = ctx.get_particles()
        ctx.set_particles(live, np.where(np.arange(n) % 3 == 0, L.CELL_FROZEN, cell).astype(np.int32))
        settled_after()
        # revive: the frozen third (with its -0.0) is located again
        ctx.locate_initial()
        settled_after()
        # a launch that is not flat: the kick
        ctx.step(dt, 1e-7, 1, 0)
        settled_after()
        # a sort only permutes
        ctx.sort_by_cell()
        name = ctx.step_kernel_name(0.0, 0)
        assert (FLAT in name) if flat_z else (STREAM in name), name
        res[flat_z] = got
    for a, b in zip(res[1], res[0]):
        _same(a, b)
    _same(res[1][0], _cpu(setup, neg0(xyz, 5, 3), U, dt, 3), "CPU statement")


def test_handoff_arrivals_restream_z(setup, gpu_ctx_factory):
    """A one-rank sharded cloud with the collectives forced: every hand-off's arrivals have not been through this shard's flat cycle,
    so the launch after it streams z; in between the body without z runs.  The bits of flat_z 0 and of the CPU statement."""
    import torch
    from cudaparticlesfoam_amd.parallel import ShardedCloud
    pz, mesh = setup["pz"], setup["mesh"]
    U = setup["pitz"]["U_uniform"]
    dev = torch.device("cuda", 0)
    n, dt = 1_600_003, 4e-4
    xyz = _cloud(pz, n, 71)
    out = {}
    for flat_z in (1, 0):
        ctx = gpu_ctx_factory()
        ctx.set_option("stats", 0)
        ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.synchronize()
        ctx.set_option("flat_z", flat_z)
        cloud = ShardedCloud(ctx, [0, mesh.n_cells], n + 64, None, send_fraction=1.0, exchange_interval=0)
        cloud.force_collectives = True
        cloud.rebalance_interval = 4
        cloud.sort_interval = 3
        cloud.overlap_steps = 1
        tx, ty, tz = (torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3))
        torch.cuda.synchronize()
        cloud.set_particles(tx, ty, tz, None, None)
        cloud.step(dt, 13)
        out[flat_z] = cloud.gather_to_numpy()
        assert cloud.rebalances >= 3
    _same(out[1], out[0])
    g, gx, gy, gz, gc = out[1]
    ref, c = _cpu(setup, xyz, U, dt, 13)
    assert np.array_equal(np.sort(g), np.arange(n))
    _same((gx, gy, gz, gc), (ref[g, 0], ref[g, 1], ref[g, 2], c[g]), "CPU statement")
