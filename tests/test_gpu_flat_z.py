"""Settled z on the flat walk (CPF_STEP_Z_SETTLED, csrc/cpf_walk.h "settled z"): after one flat launch that streamed z, the
flat launches after it neither load nor store z.  Results must be the same BITS as with option ``flat_z`` 0 (z streamed by
every launch) and as the CPU statement -- including particles with z == -0.0, which the first streaming cycle turns into
+0.0, and such particles injected after every event that must make the next launch stream z again."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(pitz, oracle_libs, gpu_ctx_factory):
    cw = oracle_libs.CellWalk()
    mesh = pitz["mesh"]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh)
    return dict(cw=cw, mesh=mesh, tables=cw.build(mesh), ctx=ctx, pz=pitz["pz"], pitz=pitz)


def _cloud(pz, n, seed):
    xyz = pz.uniform_points(seed, n, *pz.DOMAIN_BOX)
    zlo, zhi = pz.DOMAIN_BOX[0][2], pz.DOMAIN_BOX[1][2]
    xyz[::7, 2] = zlo; xyz[1::7, 2] = zhi                           # on the front / back planes
    xyz[2::7, 2] = -0.0 if zlo <= 0.0 <= zhi else zlo
    return xyz


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _by_id(ctx):
    xyzw, cell, vel = ctx.get_particles(want_vel=True)                 # (particle-id order)
    return xyzw[:, :3].copy(), cell.copy(), vel[:, :3].copy()


@pytest.mark.parametrize("n,want", [(1_600_003, ", 8>"), (300_005, ", 9>")])     # (n % 64 != 0: a partial last tile)
@pytest.mark.parametrize("field", ["U_uniform", "U_analytic"])
def test_settled_z_bit_exact(setup, field, n, want):
    """flat_z 1 against flat_z 0 against the CPU statement: plain, fused, stored-velocity and statistics launches, then
    launches without reflection (particles lost at the walls)."""
    from cudaparticlesfoam_amd import _lib as L
    pz, ctx, cw, t = setup["pz"], setup["ctx"], setup["cw"], setup["tables"]
    U = setup["pitz"][field]
    xyz = _cloud(pz, n, 43)
    dt = 4e-4 if field == "U_uniform" else 2e-4
    ctx.set_option("step_variant", -1); ctx.set_option("stream_lookup", -1); ctx.set_option("flat_walk", 1)
    x, y, z = (xyz[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads)
    st = np.zeros(3, np.int64)
    for k in (1, 1, 3, 2):
        st += np.asarray(cw.step(x, y, z, c, dt, k, t, U, nthreads=cw.max_threads))
    outs, lost = {}, {}
    for flat_z in (1, 0):
        ctx.set_option("flat_z", flat_z)
        ctx.set_option("stats", 0)
        ctx.set_velocity(U); ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.step(dt, 0.0, 1, 0)                                     # streams z: -0.0 -> +0.0
        assert ctx.step_kernel_name(0.0, 0).endswith(want)
        ctx.step(dt, 0.0, 1, 0)                                     # settled from here on
        ctx.step(dt, 0.0, 3, L.STEP_FUSE_CYCLES)
        ctx.set_option("stats", 1)
        c0 = ctx.counters()
        ctx.step(dt, 0.0, 2, L.STEP_STORE_VEL)
        c1 = ctx.counters()
        outs[flat_z] = _by_id(ctx)
        ctx.set_option("stats", 0)
        ctx.step(3 * dt, 0.0, 4, L.STEP_NO_REFLECT)
        ctx.step(3 * dt, 0.0, 3, L.STEP_NO_REFLECT | L.STEP_FUSE_CYCLES)
        lost[flat_z] = _by_id(ctx)
        lost[flat_z] += (c1["cells_visited"] - c0["cells_visited"],)
    ctx.set_option("flat_z", 1)
    for a, b in zip(outs[1], outs[0]):
        assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip(lost[1][:3], lost[0][:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert lost[1][3] == lost[0][3]
    assert (lost[1][1] == L.CELL_LOST).sum() > 0                    # the no-reflect launches did lose particles
    assert np.array_equal(_bits(outs[1][0]), _bits(np.stack([x, y, z], 1)))
    assert np.array_equal(outs[1][1], c)
    zi = xyz[:, 2]
    neg0 = (zi == 0.0) & np.signbit(zi) & (c >= 0)
    assert neg0.sum() > 0 and not np.signbit(outs[1][0][neg0, 2]).any()


def _neg0(xyz, every=5, first=3):
    out = xyz.copy()
    if out[:, 2].min() <= 0.0 <= out[:, 2].max():
        out[first::every, 2] = -0.0
    return out


def test_every_unsettling_event_streams_z_again(setup, gpu_ctx_factory):
    """-0.0 injected after set_particles, after a cpf_locate_initial that revives frozen particles, and in a cloud stepped
    with D > 0 and then D = 0: the next flat launch turns every live -0.0 into +0.0 -- the bits flat_z 0 gives.  (A context
    per run: the Brownian kick draws by step index.)"""
    from cudaparticlesfoam_amd import _lib as L
    pz, cw, t = setup["pz"], setup["cw"], setup["tables"]
    U = setup["pitz"]["U_uniform"]
    assert pz.DOMAIN_BOX[0][2] < 0.0 < pz.DOMAIN_BOX[1][2]
    n, dt = 400_001, 4e-4
    xyz = pz.uniform_points(7, n, *pz.DOMAIN_BOX)
    res = {}
    for flat_z in (1, 0):
        ctx = gpu_ctx_factory()
        ctx.set_mesh(setup["mesh"])
        ctx.set_option("flat_z", flat_z)
        ctx.set_velocity(U); ctx.synchronize()
        got = []
        # (1) set_particles over a settled cloud
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.step(dt, 0.0, 2, 0)
        ctx.set_particles(_neg0(xyz)); ctx.locate_initial(); ctx.sort_by_cell(); ctx.step(dt, 0.0, 1, 0)
        got.append(_by_id(ctx))
        # (2) frozen particles with -0.0, stepped while frozen (settled), then revived by cpf_locate_initial
        base = _neg0(xyz, 3, 0)                                     # the frozen third carries -0.0
        ctx.set_particles(base)
        ctx.locate_initial()
        _, live_cell = ctx.get_particles()
        seeded = np.where(np.arange(n) % 3 == 0, L.CELL_FROZEN, live_cell).astype(np.int32)
        ctx.set_particles(base, seeded)                             # a third frozen, with z == -0.0
        ctx.step(dt, 0.0, 2, 0)                                     # settled; the frozen third keeps its -0.0
        mid = _by_id(ctx)
        froz = (np.arange(n) % 3 == 0) & (live_cell >= 0)
        assert np.signbit(mid[0][froz, 2]).all()
        ctx.locate_initial()                                        # revives them
        ctx.step(dt, 0.0, 1, 0)
        got.append(_by_id(ctx))
        assert not np.signbit(got[-1][0][froz & (got[-1][1] >= 0), 2]).any()
        # (3) D > 0 then D = 0
        ctx.set_particles(_neg0(xyz)); ctx.locate_initial(); ctx.step(dt, 0.0, 1, 0)
        ctx.step(dt, 1e-7, 2, 0)
        ctx.step(dt, 0.0, 2, 0)
        got.append(_by_id(ctx))
        res[flat_z] = got
    for g1, g0 in zip(res[1], res[0]):
        for a, b in zip(g1[:2], g0[:2]):                            # (positions and cells: no launch here stores velocities)
            assert np.array_equal(_bits(a), _bits(b))
    # (1) against the CPU statement
    x, y, z = (_neg0(xyz)[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads)
    cw.step(x, y, z, c, dt, 1, t, U, nthreads=cw.max_threads)
    assert np.array_equal(_bits(res[1][0][0]), _bits(np.stack([x, y, z], 1)))
    assert np.array_equal(res[1][0][1], c)


def test_one_rank_shard_handoff_restreams_z(setup, gpu_ctx_factory):
    """The sharded cloud (what bench.py drives): one rank with the collectives forced, so that every hand-off splits,
    unpacks and replays; -0.0 in the cloud it is given, then new particles with -0.0 set into a settled shard.  Positions
    and cells as the CPU statement has them."""
    import torch
    from cudaparticlesfoam_amd.parallel import ShardedCloud
    pz, mesh, cw, t = setup["pz"], setup["mesh"], setup["cw"], setup["tables"]
    U = setup["pitz"]["U_uniform"]
    dev = torch.device("cuda", 0)
    n, dt = 300_007, 4e-4
    out = {}
    for flat_z in (1, 0):
        ctx = gpu_ctx_factory()
        ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.synchronize()
        ctx.set_option("flat_z", flat_z)
        cloud = ShardedCloud(ctx, [0, mesh.n_cells], n + 64, None, send_fraction=1.0, exchange_interval=0)
        cloud.force_collectives = True
        cloud.rebalance_interval = 3
        cloud.sort_interval = 4
        cloud.overlap_steps = 1
        xyz = _neg0(pz.uniform_points(11, n, *pz.DOMAIN_BOX))
        tx, ty, tz = (torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3))
        torch.cuda.synchronize()
        cloud.set_particles(tx, ty, tz, None, None)
        cloud.step(dt, 7)
        xyz2 = _neg0(pz.uniform_points(12, n, *pz.DOMAIN_BOX), 4, 1)
        tx, ty, tz = (torch.from_numpy(xyz2[:, k].copy()).to(dev) for k in range(3))
        torch.cuda.synchronize()
        cloud.set_particles(tx, ty, tz, None, None)
        cloud.step(dt, 5)
        out[flat_z] = cloud.gather_to_numpy()
        assert cloud.rebalances >= 3
    g, gx, gy, gz, gc = out[1]
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(_bits(a), _bits(b))
    x, y, z = (xyz2[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads)
    cw.step(x, y, z, c, dt, 5, t, U, nthreads=cw.max_threads)
    assert np.array_equal(np.sort(g), np.arange(n))
    assert np.array_equal(_bits(gx), _bits(x[g])) and np.array_equal(_bits(gy), _bits(y[g])) and np.array_equal(_bits(gz), _bits(z[g]))
    assert np.array_equal(gc, c[g])
