"""Routes through the re-sort's tail (csrc/cpf_sort.hip, ``sort_by_cell``: census, gather, velocities) that the sort tests of
tests/test_gpu_parity.py do not take: a cloud without ids, the velocity triples of the context's own cloud under both key sorts,
and the occupied-cell census under both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [65, 4097])
def test_sort_without_ids_moves_positions_and_cells_alike(n, gpu_ctx_factory):
    """``gid`` and ``ogid`` null (include/cpf.h allows it): x, y, z and cell come out, array for array, as from the same call given
    ids -- both key sorts, in place and into a second set of arrays; a fifth of the points lie outside (the all-ones key)."""
    import torch
    from cudaparticlesfoam_amd.cases import box_mesh
    dev = torch.device("cuda", 0)
    ctx = gpu_ctx_factory(); ctx.set_mesh(box_mesh(5, 4, 3))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("sort_key_bits", 222)
    p = lambda t: t.data_ptr()   # noqa: E731
    xyz = np.random.default_rng(n).uniform([-1.25, 0, 0], [5, 4, 3], size=(n, 3))          # x < 0: outside the box
    base = [torch.from_numpy(xyz[:, k].copy()).to(dev) for k in range(3)]
    c0 = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.locate_initial_dev(p(base[0]), p(base[1]), p(base[2]), p(c0), n)
    g0 = torch.from_numpy(np.random.default_rng(n + 1).permutation(n).astype(np.int64)).to(dev)
    torch.cuda.synchronize()
    outside = int((c0 < 0).sum())
    assert 0.1 * n < outside < 0.3 * n
    for method in (0, 2):
        ctx.set_option("sort_method", method)
        got = {}
        for ids in (True, False):
            x, y, z, c = (t.clone() for t in (*base, c0))
            g = g0.clone() if ids else None
            out = [torch.zeros_like(t) for t in (x, y, z, c)] + [torch.zeros_like(g0) if ids else None]
            q = lambda t: None if t is None else t.data_ptr()   # noqa: E731
            ctx.sort_by_cell_dev_to(p(x), p(y), p(z), p(c), q(g), *(q(t) for t in out), n)
            ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), q(g), n)
            torch.cuda.synchronize()
            got[ids] = ([t.cpu().numpy() for t in out[:4]], [t.cpu().numpy() for t in (x, y, z, c)])
        for form in (0, 1):                                          # into a second set of arrays, in place
            for a, b in zip(got[True][form], got[False][form]):
                assert np.array_equal(a, b), (method, form)
        cs = got[False][1][3]
        assert (cs[:n - outside] >= 0).all() and (cs[n - outside:] < 0).all()
    ctx.use_own_stream()


def test_stored_velocities_follow_the_resort_under_both_key_sorts(gpu_ctx_factory):
    """The context's own cloud (two array sets, the velocity triples through the sort's stage): with "sort_interval" 3 the re-sort
    falls right behind the cycle that stored velocities.  Positions, cells and velocities by id equal those of a cloud that is
    never sorted, under either key sort."""
    from cudaparticlesfoam_amd import _lib as L
    from cudaparticlesfoam_amd.cases import box_mesh
    mesh = box_mesh(6, 5, 4)
    cc, _ = mesh.cell_centres_volumes()
    U = np.stack([1.0 + 0.2 * cc[:, 1], 0.6 * np.sin(2 * cc[:, 2]), 0.6 * np.cos(2 * cc[:, 0])], 1)
    n, dt = 5000, 0.05
    xyz = np.random.default_rng(7).uniform([0, 0, 0], [6, 5, 4], size=(n, 3))
    res = []
    for interval in (0, 3):
        for method in (0, 2):
            ctx = gpu_ctx_factory()
            ctx.set_option("sort_interval", interval); ctx.set_option("sort_method", method)
            ctx.set_mesh(mesh); ctx.set_velocity(U)
            ctx.set_particles(xyz); ctx.locate_initial()
            for _ in range(3):
                ctx.step(dt, 0.0, 2)
                ctx.step(dt, 0.0, 1, L.STEP_STORE_VEL)
            res.append(ctx.get_particles(want_vel=True))
            ctx.close()
    assert (res[0][2][:, :3] != 0.0).any()
    for r in res[1:]:
        for a, b in zip(r, res[0]):
            assert np.array_equal(a, b)


def test_census_decides_the_lookup_alike_under_both_key_sorts(pitz, gpu_ctx_factory):
    """"stream_lookup_by_density" 1: the lookup goes by the particles per occupied cell that the sort counted.  A dense and a sparse
    small cloud (tests/test_gpu_flat_round.py, SMALL: 5 000 particles in 24 / in 144 cells of pitzDaily) get the same step kernel
    whichever key sort fed the census, and not the same one as each other."""
    pz = pitz["pz"]
    zlo, zhi = pz.DOMAIN_BOX[0][2], pz.DOMAIN_BOX[1][2]
    ctx = gpu_ctx_factory()
    ctx.set_mesh(pitz["mesh"]); ctx.set_velocity(pitz["U_uniform"])
    ctx.set_option("sort_interval", 0); ctx.set_option("stream_lookup_by_density", 1)
    half = {"dense": (2e-3, 1e-3), "sparse": (4e-3, 4e-3)}
    names = {}
    # (every sort follows one of the OTHER cloud: a census left standing would show)
    for cloud, method in (("dense", 0), ("sparse", 2), ("dense", 2), ("sparse", 0)):
        hx, hy = half[cloud]
        ctx.set_option("sort_method", method)
        ctx.set_particles(pz.uniform_points(89, 5000, (0.05 - hx, -hy, zlo), (0.05 + hx, hy, zhi)))
        ctx.locate_initial(); ctx.sort_by_cell(); ctx.synchronize()
        names[cloud, method] = ctx.step_kernel_name(0.0, 0)
    ctx.close()
    assert names["dense", 0] == names["dense", 2] and names["sparse", 0] == names["sparse", 2], names
    assert names["dense", 0] != names["sparse", 0], names
