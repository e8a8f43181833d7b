"""GPU: meshes with warped faces (include/cpf.h, cpf_set_mesh "VALIDITY DOMAIN").  The HIP walk on the derived mesh against
the CPU cell walk on the numpy statement's derived mesh, parent ids at every boundary of the API, the refusals, and the
planar path left exactly as it was."""
import ctypes as C

import numpy as np
import pytest

import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

pytestmark = pytest.mark.gpu
TOL = L.NONPLANAR_TOL


@pytest.fixture(scope="module")
def warped_case(oracle_libs):
    mesh = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), 2e-2, seed=11)
    st = W.quality(mesh, TOL)
    centres, _ = mesh.cell_centres_volumes()
    derived, first, _ = W.derived_mesh(mesh, st["state"], centres)
    assert (st["state"] == 2).all()
    cw = oracle_libs.CellWalk()
    rng = np.random.default_rng(17)
    return dict(mesh=mesh, derived=derived, first=first, parent=W.parent_of(first), cw=cw, t=cw.build(derived),
                U=rng.normal(size=(mesh.n_cells, 3)) * 0.4, U2=rng.normal(size=(mesh.n_cells, 3)) * 0.4,
                xyz=rng.uniform(0.02, 0.98, size=(20000, 3)))


def _cpu(case, U, dt, ks, cell0=None, D=0.0, seed=0):
    cw, t, xyz = case["cw"], case["t"], case["xyz"]
    x, y, z = (xyz[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads) if cell0 is None else cell0.copy()
    out, step0 = [], 0
    for k in ks:
        cw.step(x, y, z, c, dt, k, t, U[case["parent"]], nthreads=cw.max_threads, D=D,
                gid=np.arange(x.size, dtype=np.int64), step0=step0, seed=seed)
        step0 += k
        out.append((np.stack([x, y, z], 1).copy(), c.copy()))
    return out


def _gpu(ctx, case, U, dt, ks, D=0.0, seed=0, cells=None):
    ctx.set_mesh(case["mesh"]); ctx.set_velocity(U); ctx.set_particles(case["xyz"], cells)
    if cells is None:
        assert ctx.locate_initial() == 0
    ctx.set_seed(seed)
    out = []
    for k in ks:
        ctx.step(dt, D, k)
        xyzw, cell = ctx.get_particles()
        out.append((xyzw[:, :3].copy(), cell.copy()))
    return out


def test_mesh_quality_and_derived_counts(warped_case, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    ctx.set_mesh(warped_case["mesh"])
    q = ctx.mesh_quality()
    assert q["n_cells"] == warped_case["mesh"].n_cells and q["n_flagged"] == q["n_cells"] and q["n_bad"] == 0
    assert q["n_derived"] == warped_case["derived"].n_cells == ctx.mesh_info()["n_cells"]
    off, planes, nbr = ctx.mesh_tables()
    t = warped_case["t"]
    assert np.array_equal(off, t.cell_off) and np.array_equal(nbr, t.nbr) and np.array_equal(planes, t.planes)


@pytest.mark.parametrize("D", [0.0, 1.5e-5])
def test_walk_matches_cellwalk_on_the_derived_mesh(warped_case, gpu_ctx_factory, D):
    ks, dt = (1, 8, 41), 0.01
    ref = _cpu(warped_case, warped_case["U"], dt, ks, D=D, seed=9)
    got = _gpu(gpu_ctx_factory(), warped_case, warped_case["U"], dt, ks, D=D, seed=9)
    parent = warped_case["parent"]
    for (gx, gc), (rx, rc) in zip(got, ref):
        assert (rc >= 0).all()
        if D == 0.0:
            assert np.array_equal(gx, rx) and np.array_equal(gc, parent[rc])     # bit for bit; ids are PARENT ids
    done = 0
    for k, (gx, gc), (rx, rc) in zip(ks, got, ref):
        done += k
        if D > 0.0:
            same = gc == parent[rc]                      # (the deviates' last bits differ: tests/test_gpu_brownian.py's bars)
            sigma = np.sqrt(2 * D * dt * done)
            assert same.mean() > 0.9999 and np.abs(gx - rx)[same].max() < 2e-4 * sigma


def test_new_velocity_and_parent_cells_in(warped_case, gpu_ctx_factory):
    """set_velocity of a new U mid-run, and set_particles with PARENT cells (sub-cell resolve) start where locate would."""
    cw, t, xyz = warped_case["cw"], warped_case["t"], warped_case["xyz"]
    parent = warped_case["parent"]
    cell0 = cw.locate_initial(xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), t, nthreads=cw.max_threads)
    ctx = gpu_ctx_factory()
    got = _gpu(ctx, warped_case, warped_case["U"], 0.01, (9,), cells=parent[cell0])
    ref = _cpu(warped_case, warped_case["U"], 0.01, (9,), cell0=cell0)
    assert np.array_equal(got[0][0], ref[0][0]) and np.array_equal(got[0][1], parent[ref[0][1]])
    ctx.set_velocity(warped_case["U2"])
    ctx.step(0.01, 0.0, 9)
    xyzw, cell = ctx.get_particles()
    x, y, z = (ref[0][0][:, k].copy() for k in range(3))
    c = ref[0][1].copy()
    cw.step(x, y, z, c, 0.01, 9, t, warped_case["U2"][parent], nthreads=cw.max_threads)
    assert np.array_equal(xyzw[:, 0], x) and np.array_equal(xyzw[:, 1], y) and np.array_equal(xyzw[:, 2], z)
    assert np.array_equal(cell, parent[c])


def test_device_arrays_keep_derived_ids(warped_case, gpu_ctx_factory):
    import torch
    dev = torch.device("cuda", 0)
    cw, t, xyz, parent = warped_case["cw"], warped_case["t"], warped_case["xyz"], warped_case["parent"]
    n = xyz.shape[0]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(warped_case["mesh"]); ctx.set_velocity(warped_case["U"])
    tx, ty, tz = (torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3))
    tc = torch.empty(n, dtype=torch.int32, device=dev)
    gid = torch.arange(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.locate_initial_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), n)
    ctx.step_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), gid.data_ptr(), None, n, 0.01, 0.0, 0, 7)
    tp = torch.empty_like(tc)
    ctx.cells_to_parent_dev(tc.data_ptr(), tp.data_ptr(), n)
    w = torch.zeros(warped_case["mesh"].n_cells, dtype=torch.float64, device=dev)
    ctx.cell_histogram_dev(tc.data_ptr(), n, 2.0, w.data_ptr())
    ctx.synchronize()
    ref = _cpu(warped_case, warped_case["U"], 0.01, (7,))[0]
    assert np.array_equal(tc.cpu().numpy(), ref[1])                        # derived ids in caller-owned arrays
    assert np.array_equal(tx.cpu().numpy(), ref[0][:, 0])
    assert np.array_equal(tp.cpu().numpy(), parent[ref[1]])
    assert np.array_equal(w.cpu().numpy(), 2.0 * np.bincount(parent[ref[1]], minlength=warped_case["mesh"].n_cells))


def test_vtu_frames_carry_parent_ids(warped_case, gpu_ctx_factory, tmp_path):
    ctx = gpu_ctx_factory()
    _gpu(ctx, warped_case, warped_case["U"], 0.01, (5,))
    path = str(tmp_path / "f.vtu")
    ke = C.c_double()
    assert ctx.lib.cpf_write_vtu_async(ctx.h, path.encode(), C.byref(ke)) == L.CPF_OK
    assert ctx.lib.cpf_write_vtu_wait(ctx.h) == L.CPF_OK
    text = open(path).read()
    block = text.split("Name='ConvexTetID' format='ascii'>")[1].split("</DataArray>")[0]
    ids = np.array(block.split(), dtype=np.int64)                     # frames are in particle-id order
    _, cell = ctx.get_particles()
    assert ids.size == cell.size and np.array_equal(ids, cell) and ids.max() < warped_case["mesh"].n_cells


def test_refusals(warped_case, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    ctx.set_mesh(warped_case["mesh"])
    pos, tets = warped_case["mesh"].tet_decomposition()
    r = ctx.lib.cpf_set_tets(ctx.h, pos.ctypes.data_as(C.c_void_p), pos.shape[0], tets.ctypes.data_as(C.c_void_p), tets.shape[0], 12)
    assert r != L.CPF_OK and b"warped" in ctx.lib.cpf_last_error(ctx.h)
    shard = C.c_void_p()
    r = ctx.lib.cpf_shard_create(ctx.h, None, 1024, None, C.byref(shard))
    assert r != L.CPF_OK and not shard.value and b"warped" in ctx.lib.cpf_shard_last_error(None)
    P = np.zeros((4, 4)); ids = np.zeros(4, np.int32)
    r = ctx.lib.cpf_stage_locate_initial(ctx.h, P.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), 4)
    assert r != L.CPF_OK and b"decomposed" in ctx.lib.cpf_last_error(ctx.h)


def test_split_off_keeps_the_one_plane_model(warped_case, gpu_ctx_factory, oracle_libs):
    mesh, xyz = warped_case["mesh"], warped_case["xyz"]
    cw = warped_case["cw"]
    t = cw.build(mesh)
    ctx = gpu_ctx_factory()
    ctx.set_option("split_nonplanar", 0)
    ctx.set_mesh(mesh); ctx.set_velocity(warped_case["U"]); ctx.set_particles(xyz)
    assert ctx.mesh_quality()["n_derived"] == mesh.n_cells and ctx.mesh_info()["n_cells"] == mesh.n_cells
    ctx.locate_initial(); ctx.step(0.01, 0.0, 9)
    xyzw, cell = ctx.get_particles()
    x, y, z = (xyz[:, k].copy() for k in range(3))
    c = cw.locate_initial(x, y, z, t, nthreads=cw.max_threads)
    cw.step(x, y, z, c, 0.01, 9, t, warped_case["U"], nthreads=cw.max_threads)
    assert np.array_equal(xyzw[:, 0], x) and np.array_equal(xyzw[:, 1], y) and np.array_equal(xyzw[:, 2], z)
    assert np.array_equal(cell, c)


def test_planar_mesh_path_is_unchanged(pitz, gpu_ctx_factory):
    mesh, U = pitz["mesh"], pitz["U_analytic"]
    xyz = pitz["pz"].uniform_points(5, 50000, *pitz["pz"].DOMAIN_BOX)
    res = []
    for split in (0, 1):
        ctx = gpu_ctx_factory()
        ctx.set_option("split_nonplanar", split)
        ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(xyz); ctx.locate_initial()
        assert ctx.mesh_quality()["n_flagged"] == 0
        ctx.step(1e-4, 0.0, 20)
        res.append((ctx.step_kernel_name(), ctx.mesh_flags(), ctx.get_particles()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2][0], res[1][2][0]) and np.array_equal(res[0][2][1], res[1][2][1])


def test_million_particles_on_a_warped_box(gpu_ctx_factory):
    mesh = W.warp_mesh(box_mesh(30, 28, 26, upper=(1.0, 1.0, 1.0)), 1e-2, seed=4)
    rng = np.random.default_rng(8)
    n = 1_000_000
    xyz = rng.uniform(0.0, 1.0, size=(n, 3))
    U = rng.normal(size=(mesh.n_cells, 3)) * 2.0
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(U); ctx.set_particles(xyz)
    assert ctx.locate_initial() == 0
    assert ctx.mesh_quality()["n_derived"] == 12 * mesh.n_cells
    ctx.step(2e-3, 1.5e-5, 200)
    xyzw, cell = ctx.get_particles()
    assert (cell >= 0).all() and (cell < mesh.n_cells).all() and (xyzw[:, 3] == 1).all()
    assert xyzw[:, :3].min() >= 0.0 and xyzw[:, :3].max() <= 1.0


@pytest.fixture(scope="module")
def mixed_case(oracle_libs):
    """a = 3e-11: about a third of the cells stay whole, holding face groups of the fan triangles of decomposed neighbours"""
    mesh = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), 3e-11, seed=1)
    st = W.quality(mesh, TOL)
    centres, _ = mesh.cell_centres_volumes()
    derived, first, _ = W.derived_mesh(mesh, st["state"], centres)
    whole = int((np.diff(first) == 1).sum())
    assert 0 < whole < mesh.n_cells
    cw = oracle_libs.CellWalk()
    t = cw.build(derived)
    assert t.n_groups > 0
    rng = np.random.default_rng(23)
    return dict(mesh=mesh, derived=derived, first=first, parent=W.parent_of(first), cw=cw, t=t,
                U=rng.normal(size=(mesh.n_cells, 3)) * 0.4, xyz=rng.uniform(0.02, 0.98, size=(20000, 3)))


def test_walk_matches_cellwalk_on_a_mixed_derived_mesh(mixed_case, gpu_ctx_factory):
    ks, dt = (1, 8, 41), 0.01
    ref = _cpu(mixed_case, mixed_case["U"], dt, ks)
    ctx = gpu_ctx_factory()
    got = _gpu(ctx, mixed_case, mixed_case["U"], dt, ks)
    assert ctx.mesh_quality()["n_derived"] == mixed_case["derived"].n_cells
    for (gx, gc), (rx, rc) in zip(got, ref):
        assert (rc >= 0).all() and np.array_equal(gx, rx) and np.array_equal(gc, mixed_case["parent"][rc])


def test_million_particles_on_a_warped_polyhedral_mesh(gpu_ctx_factory):
    """Extruded diamond cells (octagons and squares), warped by 1e-2 of a cell: 1e6 particles, 200 cycles with diffusion;
    every particle stays in the domain and within 1e-9 of the derived cell it claims."""
    import torch
    from cudaparticlesfoam_amd import api
    from cudaparticlesfoam_amd.cases.polygons import diamond_box
    mesh = W.warp_mesh(diamond_box(30, 30, 20)[0], 1e-2, seed=4)
    q = api.mesh_quality_host(mesh)
    assert q["n_bad"] == 0 and q["n_derived"] > 8 * mesh.n_cells
    derived, first, _ = api.build_derived_mesh_host(mesh)
    tab = api.build_mesh_tables_host(derived)
    lo, hi = mesh.points.min(0), mesh.points.max(0)
    rng = np.random.default_rng(8)
    n = 1_000_000
    xyz = rng.uniform(lo + 0.01 * (hi - lo), hi - 0.01 * (hi - lo), size=(n, 3))
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.05 * float(np.min(hi - lo))
    dev = torch.device("cuda", 0)
    ctx = gpu_ctx_factory()
    ctx.set_mesh(mesh); ctx.set_velocity(U)
    assert ctx.mesh_quality()["n_derived"] == q["n_derived"]
    tx, ty, tz = (torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3))
    tc = torch.empty(n, dtype=torch.int32, device=dev)
    gid = torch.arange(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.locate_initial_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), n)
    ctx.synchronize()
    assert (tc >= 0).all().item()
    for _ in range(4):
        ctx.step_dev(tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), tc.data_ptr(), gid.data_ptr(), None, n, 2e-3, 1.5e-5, _ * 50, 50)
    ctx.synchronize()
    X = np.stack([tx.cpu().numpy(), ty.cpu().numpy(), tz.cpu().numpy()], 1)
    cell = tc.cpu().numpy()
    assert (cell >= 0).all() and (cell < derived.n_cells).all()              # nobody lost, count conserved
    assert (X >= lo - 1e-12).all() and (X <= hi + 1e-12).all()               # nobody outside the domain
    off, planes = tab["cell_off"], tab["planes"]
    ns = np.diff(off)[cell]
    rows = np.repeat(off[cell], ns) + (np.arange(ns.sum()) - np.repeat(np.cumsum(ns) - ns, ns))
    pl = planes[rows]
    Xr = np.repeat(X, ns, axis=0)
    fd = pl[:, 3] - ((pl[:, 0] * Xr[:, 0] + pl[:, 1] * Xr[:, 1]) + pl[:, 2] * Xr[:, 2])
    assert fd.max() <= 1e-9, fd.max()                                        # inside the derived cell it claims
