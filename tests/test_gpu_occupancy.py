"""GPU: per-cell occupancy accumulated on the device (include/cpf.h "per-cell occupancy"; csrc/cpf_occupancy.hip).  Expected counts
are always ``np.bincount`` over what ``get_particles()`` returns, or over the array handed in; equality is exact."""
import numpy as np
import pytest

import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases import pitzdaily as pz
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
N = 10_007                                   # a multiple of neither 64, 256 nor 1024


def _bincount(cell, n_cells):
    cell = np.asarray(cell)
    return np.bincount(cell[cell >= 0], minlength=n_cells).astype(np.uint64)


@pytest.fixture(scope="module")
def box():
    mesh = box_mesh(5, 4, 3)
    return dict(mesh=mesh, xyz=pz.uniform_points(77, N, (0.0, 0.0, 0.0), (5.0, 4.0, 3.0)))


def test_one_sample_is_the_bincount(box, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    ctx.set_mesh(box["mesh"])
    counts, ns = ctx.occupancy()                                             # before any sample: zeros and 0
    assert counts.dtype == np.uint64 and counts.shape == (60,) and not counts.any() and ns == 0
    with pytest.raises(L.CpfError) as e:                                     # no located particles yet
        ctx.occupancy_sample()
    assert e.value.status == L.CPF_ERR_STATE
    with pytest.raises(ValueError):
        ctx.concentration()
    ctx.set_particles(box["xyz"])
    assert ctx.locate_initial() == 0
    ctx.sort_by_cell()
    ctx.occupancy_sample()
    counts, ns = ctx.occupancy()
    _, cell = ctx.get_particles()
    assert ns == 1 and int(counts.sum()) == N
    assert np.array_equal(counts, _bincount(cell, 60))
    assert np.array_equal(ctx.concentration(), counts.astype(np.float64) / ctx.cell_volumes())


def test_state_errors_without_a_mesh():
    with api.Context(0) as ctx:
        for call in (ctx.occupancy_sample, lambda: ctx.occupancy_sample_dev(None, 0)):
            with pytest.raises(L.CpfError) as e:
                call()
            assert e.value.status == L.CPF_ERR_STATE


def test_accumulation_across_steps_and_resorts(box, gpu_ctx_factory):
    mesh = box["mesh"]
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory()
    ctx.set_option("sort_interval", 3)
    ctx.set_mesh(mesh); ctx.set_velocity(rng.normal(size=(mesh.n_cells, 3)) * 0.5); ctx.set_particles(box["xyz"])
    ctx.locate_initial()
    want = np.zeros(mesh.n_cells, np.uint64)
    for _ in range(7):
        ctx.step(0.05, 1e-3, 2)
        ctx.occupancy_sample()
        want += _bincount(ctx.get_particles()[1], mesh.n_cells)
    counts, ns = ctx.occupancy()
    assert ns == 7 and np.array_equal(counts, want) and int(counts.sum()) == 7 * N
    ctx.occupancy_reset()
    counts, ns = ctx.occupancy()
    assert ns == 0 and not counts.any()
    ctx.occupancy_sample()                                                   # ... and it starts again from zero
    counts, ns = ctx.occupancy()
    assert ns == 1 and np.array_equal(counts, _bincount(ctx.get_particles()[1], mesh.n_cells))


def test_lost_particles_are_not_counted(box, gpu_ctx_factory):
    mesh = box["mesh"]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(np.tile([1.0, 0.0, 0.0], (mesh.n_cells, 1))); ctx.set_particles(box["xyz"])
    ctx.locate_initial()
    before = np.zeros(mesh.n_cells, np.uint64)
    for k in range(3):
        ctx.step(0.5, 0.0, 1, L.STEP_NO_REFLECT)
        ctx.occupancy_sample()
        counts, ns = ctx.occupancy()
        _, cell = ctx.get_particles()
        assert ns == k + 1
        assert np.array_equal(counts - before, _bincount(cell, mesh.n_cells))
        assert int((counts - before).sum()) == int((cell >= 0).sum())
        before = counts
    lost = int((cell < 0).sum())                                             # x > 3.5 leaves: 30 % of 10 007, sigma 46
    assert 2000 <= lost <= 4000, lost


# ---- adversarial arrays through occupancy_sample_dev: 36 000 cells, above the 32 768 of cell_histogram's LDS path
BIG = (40, 30, 30)
N_BIG = 36_000


def _adversarial(name):
    rng = np.random.default_rng(11)
    if name == "one_cell":
        return np.full(70_001, 12_345, np.int32)
    if name == "two_alternating":
        return np.where(np.arange(4097) % 2 == 0, 7, 35_999).astype(np.int32)
    if name == "two_aliasing":                                               # far apart and in the same bin modulo 2048
        return np.where(np.arange(4097) % 2 == 0, 5, 5 + 3 * 2048 * 5).astype(np.int32)
    if name == "permutation_with_lost":
        c = rng.permutation(N_BIG).astype(np.int32)
        c[::7] = -1
        return c
    if name == "sorted_sparse":                                              # the window of a slice overflows the LDS bins
        return np.sort(rng.choice(N_BIG, size=5000, replace=False)).astype(np.int32)
    if name == "sorted_dense":                                               # several workgroups, each with a wide LDS window
        return np.sort(rng.integers(0, N_BIG, size=50_001)).astype(np.int32)
    if name == "codes_and_foreign_ids":                                      # frozen, lost, ids that are no cells of the mesh
        c = rng.integers(0, N_BIG, size=9001).astype(np.int32)
        c[::5] = -2; c[1::5] = N_BIG; c[2::5] = np.iinfo(np.int32).max; c[3::11] = np.iinfo(np.int32).min
        return c
    return rng.integers(0, N_BIG, size=int(name[1:])).astype(np.int32)       # "n<length>"


@pytest.fixture(scope="module")
def big_ctx():
    with api.Context(0) as ctx:
        ctx.set_mesh(box_mesh(*BIG))
        yield ctx


@pytest.mark.parametrize("name", ["one_cell", "two_alternating", "two_aliasing", "permutation_with_lost", "sorted_sparse", "sorted_dense",
                                  "codes_and_foreign_ids", "n0", "n1", "n63", "n64", "n65", "n4099"])
@pytest.mark.parametrize("offset", [0, 1])
def test_adversarial_arrays(big_ctx, name, offset):
    """offset 1: the array starts 4 bytes past a 16-byte boundary (the kernel's instantiation without 16-byte loads)."""
    import torch
    c = _adversarial(name)
    t = torch.from_numpy(np.concatenate([np.full(offset, 3, np.int32), c])).to(torch.device("cuda", 0))[offset:]
    assert c.size == 0 or t.data_ptr() % 16 == 4 * offset
    torch.cuda.synchronize()
    big_ctx.occupancy_reset()
    big_ctx.occupancy_sample_dev(t.data_ptr() if c.size else None, c.size)
    counts, ns = big_ctx.occupancy()
    assert ns == 1
    assert np.array_equal(counts, _bincount(np.where((c >= 0) & (c < N_BIG), c, -1), N_BIG))


def test_decomposed_cells_count_per_parent(gpu_ctx_factory):
    import torch
    mesh = W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    rng = np.random.default_rng(3)
    xyz = rng.uniform((0.05, 0.05, 0.05), (5.95, 4.95, 3.95), size=(20_000, 3))
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.5
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(xyz)
    n_derived = ctx.mesh_quality()["n_derived"]
    assert n_derived > mesh.n_cells == 120
    assert ctx.locate_initial() == 0
    ctx.step(0.05, 0.0, 5)
    ctx.occupancy_sample()
    counts, ns = ctx.occupancy()
    _, cell = ctx.get_particles()                                            # parent ids
    assert counts.size == 120 and ns == 1 and np.array_equal(counts, _bincount(cell, 120))
    # the same through caller-owned arrays, which hold DERIVED ids
    dev = torch.device("cuda", 0)
    n = xyz.shape[0]
    tx, ty, tz = (torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3))
    tc = torch.empty(n, dtype=torch.int32, device=dev)
    gid = torch.arange(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.locate_initial_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), n)
    ctx.step_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), gid.data_ptr(), None, n, 0.05, 0.0, 0, 5)
    ctx.occupancy_reset()
    ctx.occupancy_sample_dev(tc.data_ptr(), n)
    tp = torch.empty_like(tc)
    ctx.cells_to_parent_dev(tc.data_ptr(), tp.data_ptr(), n)
    counts_dev, ns = ctx.occupancy()
    derived = tc.cpu().numpy()
    assert derived.max() >= 120                                              # derived ids indeed
    assert ns == 1 and np.array_equal(counts_dev, _bincount(tp.cpu().numpy(), 120))
    assert np.array_equal(counts_dev, counts)                                # (the same particles, the same five cycles)


def test_set_mesh_drops_the_accumulators(box, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    ctx.set_mesh(box["mesh"]); ctx.set_particles(box["xyz"]); ctx.locate_initial()
    ctx.occupancy_sample()
    assert ctx.occupancy()[1] == 1
    ctx.set_mesh(box_mesh(3, 3, 2))
    counts, ns = ctx.occupancy()
    assert counts.shape == (18,) and not counts.any() and ns == 0


def test_sampling_does_not_disturb_the_run(pitz, gpu_ctx_factory):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    xyz = pz.uniform_points(9, 150_000, *pz.DOMAIN_BOX)
    out = []
    for sample in (False, True):
        ctx = gpu_ctx_factory()
        ctx.set_seed(4242)
        ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        for k in range(7):
            if k < 6:
                ctx.step(1e-4, 2e-5, 1)
            else:
                ctx.step(1e-4, 2e-5, 5, L.STEP_FUSE_CYCLES)
            if sample:
                ctx.occupancy_sample()
        out.append(ctx.get_particles())
        if sample:
            counts, ns = ctx.occupancy()
            assert ns == 7 and int(counts.sum()) <= 7 * 150_000 and counts.any()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_cuda_particles_occupancy_interval(pitz):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    dt = 2.0 ** -13                                                          # 10 * dt / dt == 10 exactly
    base = dict(numParticles=20_000, dt=dt, saveInterval=10, diffusionCoeff=1.5e-5, seedingBox=pz.DOMAIN_BOX)
    p = api.CudaParticles(mesh, U, dict(base, occupancyInterval=4))
    q = api.CudaParticles(mesh, U, base)
    try:
        for k in range(3):
            assert p.advect(k * 10 * dt, 10 * dt) == 10
            assert q.advect(k * 10 * dt, 10 * dt) == 10
        counts, ns = p.ctx.occupancy()
        assert ns == 7 and p.step == 30
        conc, V = p.concentration(), p.ctx.cell_volumes()
        total = float((conc * V).sum() * ns)
        assert abs(total - float(counts.sum())) <= 1e-12 * float(counts.sum())
        assert q.ctx.occupancy()[1] == 0
        D = base["diffusionCoeff"]
        assert q.ctx.step_kernel_name(D, L.STEP_FUSE_CYCLES) == p.ctx.step_kernel_name(D, L.STEP_FUSE_CYCLES)
        with pytest.raises(ValueError):
            q.concentration()
    finally:
        p.close(); q.close()


@pytest.mark.parametrize("which", ["pitz", "warped"])
def test_context_cell_volumes_are_the_host_ones(pitz, gpu_ctx_factory, which):
    mesh = pitz["mesh"] if which == "pitz" else W.warp_mesh(box_mesh(6, 5, 4), 0.05)
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh)
    V = ctx.cell_volumes()
    assert V.shape == (mesh.n_cells,) and np.array_equal(V, api.cell_volumes_host(mesh))      # bit for bit; parent volumes
