"""CPU: warped faces and concave cells (include/cpf.h, cpf_set_mesh "VALIDITY DOMAIN").  The library's mesh quality report and
derived mesh against the numpy statement in tests/warped.py, and the cell walk on the derived mesh against the reference's
tet walk on the fan of every cell."""
import numpy as np
import pytest

import warped as W
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh, block_mesh

from oracle.tetmesh import poly_to_tets

TOL = L.NONPLANAR_TOL
WARPS = (3e-11, 1e-8, 1e-3, 2e-2)          # 3e-11: about a third of the cells stay whole next to decomposed ones


def _repository_meshes():
    from cudaparticlesfoam_amd.cases import pitzdaily as pz, tjunction as tj
    from cudaparticlesfoam_amd.cases.refine import refined_box
    from cudaparticlesfoam_amd.cases.polygons import cut_corner_box, chamfered_box, diamond_box
    from tetcells import box_tets, tet_cell_polymesh
    yield "pitzDaily", pz.pitzdaily_mesh()
    yield "TJunction", tj.tjunction_mesh()
    yield "refined box", refined_box(6, 5, 4, (0, 0, 0), (3.0, 2.5, 2.0), ((1.0, 0.5, 0.5), (2.0, 2.0, 1.5)))[0]
    yield "tet cells", tet_cell_polymesh(*box_tets(4, 3, 2))
    yield "cut corners", cut_corner_box(6, 5, 4)[0]
    yield "chamfered", chamfered_box(6, 5, 4)[0]
    yield "diamonds", diamond_box(6, 6, 4)[0]
    rng = np.random.default_rng(3)
    for k in range(6):           # sheared, graded blocks with large coordinates (test_oracle_random, tools/fuzz_parity.py)
        lo = rng.uniform(-100.0, 100.0, 3)
        ext = rng.uniform(0.5, 3.0, 3)
        hi = lo + ext
        shear = rng.uniform(-0.25, 0.25) * ext[1]
        v = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0] + shear, hi[1], lo[2]], [lo[0] + shear, hi[1], lo[2]],
                      [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0] + shear, hi[1], hi[2]], [lo[0] + shear, hi[1], hi[2]]])
        grading = tuple(float(g) for g in rng.choice([0.3, 0.5, 1.0, 2.0, 4.0], size=3))
        yield "sheared block %d" % k, block_mesh(v, [dict(hex=range(8), n=(7, 5, 4), simple=grading)])


def test_no_repository_mesh_is_flagged():
    worst = 0.0
    for name, mesh in _repository_meshes():
        q = api.mesh_quality_host(mesh)
        assert q["n_flagged"] == 0 and q["n_derived"] == mesh.n_cells, (name, q)
        worst = max(worst, q["max_eta"], q["max_xi"])
        d, first, apex = api.build_derived_mesh_host(mesh)           # nothing flagged: the derived mesh IS the mesh
        assert np.array_equal(first, np.arange(mesh.n_cells + 1)) and apex.shape == (0, 3)
        for k in ("points", "face_offsets", "face_verts", "owner", "neighbour"):
            assert np.array_equal(getattr(d, k), getattr(mesh, k)), (name, k)
    assert worst < 0.05 * TOL                                          # rounding noise sits well below the tolerance


def test_polyhedral_mesh_is_not_flagged():
    from cudaparticlesfoam_amd.cases.polygons import chamfered_box
    mesh = chamfered_box(60, 46, 40, cuts_per_corner=1, period=3)[0]
    q = api.mesh_quality_host(mesh)
    assert q["n_flagged"] == 0 and q["max_eta"] < 0.05 * TOL and q["max_xi"] < 0.05 * TOL, q


@pytest.mark.parametrize("a", WARPS)
def test_quality_and_derived_mesh_equal_the_statement(a):
    mesh = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), a, seed=1)
    st = W.quality(mesh, TOL)
    q = api.mesh_quality_host(mesh)
    assert q["n_flagged"] == int((st["state"] > 0).sum()) > 0 and q["n_bad"] == int((st["state"] == 1).sum())
    # (the statement's sums may round differently in the last bit)
    assert abs(q["max_eta"] - st["eta"].max()) <= 1e-12 * st["eta"].max() and q["worst_face"] == int(np.argmax(st["eta"]))
    assert abs(q["max_xi"] - st["xi"].max()) <= 1e-12 * st["xi"].max() and q["worst_cell"] == int(np.argmax(st["xi"]))
    centres, _ = mesh.cell_centres_volumes()
    d, first, apex = api.build_derived_mesh_host(mesh)
    sd, sfirst, sapex = W.derived_mesh(mesh, st["state"], centres)
    assert np.array_equal(first, sfirst) and np.array_equal(apex, sapex)     # apex = OpenFOAM's cell centre, bit for bit
    assert q["n_derived"] == d.n_cells == sd.n_cells
    for k in ("points", "face_offsets", "face_verts", "owner", "neighbour"):
        assert np.array_equal(getattr(d, k), getattr(sd, k)), k
    # which cells are split: the statement's, and a split hex is its 12 tets
    split = np.diff(first) > 1
    assert np.array_equal(split, st["state"] == 2) and (np.diff(first)[split] == 12).all()
    # ... and the unsplit tolerance path: option "split_nonplanar" 0 keeps the cells
    assert api.mesh_quality_host(mesh, split=False)["n_derived"] == mesh.n_cells


@pytest.mark.parametrize("a", WARPS)
def test_tables_of_the_derived_mesh_equal_cellwalk(oracle_libs, a):
    mesh = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), a, seed=2)
    st = W.quality(mesh, TOL)
    centres, _ = mesh.cell_centres_volumes()
    sd, _, _ = W.derived_mesh(mesh, st["state"], centres)
    t = oracle_libs.CellWalk().build(sd)
    h = api.build_mesh_tables_host(sd)
    assert np.array_equal(h["cell_off"], t.cell_off) and np.array_equal(h["nbr"], t.nbr)
    assert np.array_equal(h["planes"].view(np.uint64), t.planes.view(np.uint64))
    assert np.array_equal(h["group_off"], t.group_off) and np.array_equal(h["group_nbr"], t.group_nbr[:h["group_nbr"].size])


def _outside_own_cell(t, x, y, z, cell):
    """largest plane distance of an active particle outside the derived cell it claims"""
    worst = 0.0
    for i in np.nonzero(cell >= 0)[0]:
        s0, s1 = t.cell_off[cell[i]], t.cell_off[cell[i] + 1]
        pl = t.planes[s0:s1]
        fd = pl[:, 3] - (pl[:, 0] * x[i] + pl[:, 1] * y[i] + pl[:, 2] * z[i])
        worst = max(worst, float(fd.max()))
    return worst


def _tet_of(positions, tets, cand, p):
    """the tet among `cand` that holds p best (largest smallest barycentric weight)"""
    best, bw = cand[0], -np.inf
    for t in cand:
        v = positions[tets[t]]
        T = np.stack([v[1] - v[0], v[2] - v[0], v[3] - v[0]], 1)
        w = np.linalg.solve(T, p - v[0])
        m = min(w.min(), 1.0 - w.sum())
        if m > bw:
            bw, best = m, t
    return best


@pytest.mark.parametrize("a", WARPS)
def test_cellwalk_on_derived_mesh_equals_tet_walk(oracle_libs, a):
    mesh = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), a, seed=3)
    st = W.quality(mesh, TOL)
    centres, _ = mesh.cell_centres_volumes()
    sd, first, _ = W.derived_mesh(mesh, st["state"], centres)
    parent = W.parent_of(first)
    rng = np.random.default_rng(5)
    U = rng.normal(size=(mesh.n_cells, 3)) * 0.5
    positions, tets, tet_cell, tet_u = poly_to_tets(mesh, centres, U)
    tw, cw = oracle_libs.TetWalk(), oracle_libs.CellWalk()
    m = tw.tables(positions, tets, tet_u)
    t = cw.build(sd)
    n = 1500
    xyz = rng.uniform([0.05, 0.05, 0.05], [0.95, 0.95, 0.95], size=(n, 3))
    cell0 = cw.locate_initial(xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), t, nthreads=cw.max_threads)
    assert (cell0 >= 0).all()
    tet_first = np.concatenate([[0], np.cumsum(np.bincount(tet_cell, minlength=mesh.n_cells))])
    ids = np.empty(n, np.int32)
    for i in range(n):
        c = parent[cell0[i]]
        if first[c + 1] - first[c] > 1:                  # a split cell: derived tet j of c is the reference's tet j of c
            ids[i] = tet_first[c] + (cell0[i] - first[c])
        else:
            ids[i] = _tet_of(positions, tets, np.arange(tet_first[c], tet_first[c + 1]), xyz[i])
    P = np.zeros((n, 4)); P[:, :3] = xyz; P[:, 3] = 1
    x, y, z, cc = xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), cell0.copy()
    Ud = U[parent]
    vels = np.zeros((n, 4)); disps = np.zeros((n, 4))
    L_ = float(np.sqrt(3.0))
    lo, hi = mesh.points.min(0), mesh.points.max(0)
    refs = [("tet walk", tw)] + ([("reference", oracle_libs.RefLib())] if oracle_libs.have_ref() else [])
    states = {name: (P.copy(), ids.copy(), vels.copy(), disps.copy()) for name, _ in refs}
    for k in (1, 9, 40):                                    # 50 cycles, checked after 1, 10 and 50
        cw.step(x, y, z, cc, 0.01, k, t, Ud, nthreads=cw.max_threads)
        assert (cc >= 0).all()
        xs = np.stack([x, y, z], 1)
        assert ((xs >= lo - 1e-12) & (xs <= hi + 1e-12)).all(), "particles outside the domain"
        assert _outside_own_cell(t, x, y, z, cc) <= 1e-9
        for name, walker in refs:
            Pr, idr, vr, dr = states[name]
            walker.cycles(Pr, idr, vr, dr, 0.01, k, m, nthreads=walker.max_threads)
            rel = np.sqrt(((xs - Pr[:, :3]) ** 2).sum(1)) / L_
            assert rel.max() <= 1e-10, (name, a, k, rel.max())
            assert (idr >= 0).all() and np.array_equal(parent[cc], tet_cell[idr]), (name, a, k)


def test_mesh_with_bad_cells_keeps_the_one_plane_model():
    """A warped chamfered box: flagged cells whose fan from the centre has a tet of non-positive volume (faces with runs of
    collinear vertices) cannot be decomposed, and leaving them whole next to decomposed cells would let particles leave the
    domain.  Such a mesh is walked exactly as without decomposition."""
    from cudaparticlesfoam_amd.cases.polygons import chamfered_box
    mesh = W.warp_mesh(chamfered_box(12, 10, 8, cuts_per_corner=1, period=3)[0], 1e-2, seed=4)
    st = W.quality(mesh, TOL)
    q = api.mesh_quality_host(mesh)
    assert q["n_bad"] == int((st["state"] == 1).sum()) > 0 and q["n_flagged"] == int((st["state"] > 0).sum())
    assert q["n_derived"] == mesh.n_cells
    d, first, apex = api.build_derived_mesh_host(mesh)
    assert np.array_equal(first, np.arange(mesh.n_cells + 1)) and apex.shape == (0, 3)
    for k in ("points", "face_offsets", "face_verts", "owner", "neighbour"):
        assert np.array_equal(getattr(d, k), getattr(mesh, k)), k
