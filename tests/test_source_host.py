"""CPU: the host side of the patch source (include/cpf.h "patch source"): the table builder against the numpy rule, the position
against its numpy statement on the oracle's Philox, bit for bit; that the weights do what they say; the calls ``CudaParticles``
makes; the patch faces and their fan triangles; the CPU statement of the recycled runs tests/test_gpu_source.py compares."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import recycle as R
import sourcepatch as SP
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

GIDS = np.array([0, 1, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 62 + 5], np.int64)     # test_recycle_host.py's
SEEDS = [9, 1591593751, 0xFFFFFFFF]
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 1.0, 0.25], [-0.15, 0.2, 1.0]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ulps(a, b):
    return np.abs(_bits(np.abs(a)) - _bits(np.abs(b)))


@pytest.fixture(scope="module")
def graded():
    mesh = box_mesh(10, 9, 8, upper=(1.0, 0.9, 0.8), grading=(2.0, 1.0, 0.5))
    faces = SP.boundary_faces_at_x0(mesh)
    tri, of = mesh.face_triangles(faces)
    assert faces.size == 72 and tri.shape == (144, 3, 3)
    area = SP.geometry(tri)[5]
    assert area.max() > 2.0 * area.min()                                      # unequal areas
    return dict(mesh=mesh, faces=faces, tri=tri, of=of, area=area)


def _status(call):
    with pytest.raises(L.CpfError) as e:
        call()
    return e.value.status


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("which", ["patch", "sheared"])
@pytest.mark.parametrize("weighted", [False, True])
def test_1_table_is_the_numpy_rule(graded, which, weighted):
    tri = graded["tri"] if which == "patch" else graded["tri"] @ SHEAR.T
    m = tri.shape[0]
    rng = np.random.default_rng(5)
    w = rng.uniform(0.1, 5.0, size=m) if weighted else None
    depth = np.stack([rng.uniform(0.0, 0.01, size=m), rng.uniform(0.02, 0.05, size=m)], 1)
    rec, hi = api.source_table_host(tri, w, depth)
    want, want_hi = SP.table(tri, w, depth)
    assert rec.shape == (m, 16) and hi.dtype == np.uint32
    for cols in (slice(0, 3), slice(3, 6), slice(6, 9), slice(12, 16)):      # A, e1, e2, d0 | d1 - d0 | index | 0
        assert np.array_equal(_bits(rec[:, cols]), _bits(want[:, cols])), cols
    assert np.array_equal(rec[:, 14], np.arange(m)) and (rec[:, 15] == 0.0).all()
    assert _ulps(rec[:, 9:12], want[:, 9:12]).max() <= 4
    assert np.allclose((rec[:, 9:12] ** 2).sum(1), 1.0, atol=1e-15, rtol=0)
    # the bounds: within one count of 2^32 * C_t / C in exact arithmetic on the builder's own weights
    weights = SP.geometry(tri)[5] if w is None else w
    run, total = Fraction(0), sum(Fraction(float(v)) for v in weights)
    assert (np.diff(hi.astype(np.int64)) > 0).all() and hi[-1] == 0xFFFFFFFF
    worst = 0
    for t in range(m):
        run += Fraction(float(weights[t]))
        exact = (run * 2 ** 32) // total
        worst = max(worst, abs(int(hi[t]) + 1 - int(exact)))
    assert worst <= 1, worst
    assert np.abs(hi.astype(np.int64) - want_hi.astype(np.int64)).max() <= 1
    # ... and bit for bit the rule in the builder's own arithmetic (fp64 running sums in input order)
    same, same_hi = SP.table(tri, w, depth, exact=False)
    assert np.array_equal(hi, same_hi) and np.array_equal(_bits(rec[:, :9]), _bits(same[:, :9]))
    # a scalar depth range holds for every triangle
    rec2, hi2 = api.source_table_host(tri, w, (0.25, 0.75))
    assert np.array_equal(hi2, hi) and (rec2[:, 12] == 0.25).all() and (rec2[:, 13] == 0.5).all()


def test_1_dropped_triangles(graded):
    tri = graded["tri"][:12].copy()
    w = np.linspace(1.0, 2.0, 12)
    w[3] = 0.0                                                               # a weight 0
    tri[7, 2] = tri[7, 1]                                                    # a degenerate triangle (len == 0)
    rec, hi = api.source_table_host(tri, w)
    assert np.array_equal(rec[:, 14], [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]) and hi.size == 10 and hi[-1] == 0xFFFFFFFF
    want, want_hi = SP.table(tri, w, exact=False)
    assert np.array_equal(hi, want_hi) and np.array_equal(_bits(rec[:, :9]), _bits(want[:, :9]))
    # by area, the degenerate triangle has weight 0 as well
    rec, hi = api.source_table_host(tri)
    assert np.array_equal(rec[:, 14], [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11])
    # a weight of 2^-40 of the total: its share is below 2^-32, the second rule drops it (the LAST kept triangle is the one that
    # cannot go: b_last = 2^32 by definition, so it keeps the one count its predecessor's floor leaves)
    for at in (0, 5, 10):
        w = np.ones(12)
        w[at] = 11.0 * 2.0 ** -40
        rec, hi = api.source_table_host(graded["tri"][:12], w)
        assert np.array_equal(rec[:, 14], np.delete(np.arange(12), at)) and hi[-1] == 0xFFFFFFFF and (np.diff(hi.astype(np.int64)) > 0).all()
    # one triangle
    rec, hi = api.source_table_host(graded["tri"][:1])
    assert np.array_equal(hi, [0xFFFFFFFF]) and rec.shape == (1, 16)


def test_1_argument_errors(graded):
    tri = graded["tri"][:6]
    ok = np.ones(6)
    bad_weights = [np.where(np.arange(6) == 2, v, ok) for v in (-1.0, -1e-300, np.inf, np.nan)]
    for w in bad_weights:
        assert _status(lambda: api.source_table_host(tri, w)) == L.CPF_ERR_ARG
    for depth in ((0.2, 0.1), (0.0, np.inf), (np.nan, 1.0), (-np.inf, 0.0)):
        assert _status(lambda: api.source_table_host(tri, None, depth)) == L.CPF_ERR_ARG
        per = np.tile([0.0, 0.1], (6, 1)); per[4] = depth
        assert _status(lambda: api.source_table_host(tri, None, per)) == L.CPF_ERR_ARG
    assert _status(lambda: api.source_table_host(tri, np.zeros(6))) == L.CPF_ERR_ARG                  # no triangle kept
    assert _status(lambda: api.source_table_host(np.zeros((3, 3, 3)))) == L.CPF_ERR_ARG              # ... all degenerate
    assert _status(lambda: api.source_table_host(np.zeros((0, 3, 3)))) == L.CPF_ERR_ARG              # ... none given
    nan_tri = tri.copy(); nan_tri[1, 1, 2] = np.nan
    assert _status(lambda: api.source_table_host(nan_tri)) == L.CPF_ERR_ARG                           # an area that is not finite
    # more than 2^24 triangles kept: 2^24 + 1 copies of one triangle with equal weights (2^24 are accepted)
    many = 2 ** 24 + 1
    big = np.broadcast_to(tri[0], (many, 3, 3)).copy()
    lib, k = L.load(), C.c_int64(0)
    assert lib.cpf_source_table_host(api._ptr(big), None, None, 0.0, 0.0, many, None, None, C.byref(k)) == L.CPF_ERR_ARG
    assert lib.cpf_source_table_host(api._ptr(big), None, None, 0.0, 0.0, many - 1, None, None, C.byref(k)) == L.CPF_OK
    assert k.value == 2 ** 24


def test_1_nulls_and_null_contexts():
    lib, p = L.load(), api._ptr
    tri, rec, hi, k, out = np.zeros((1, 3, 3)), np.zeros(16), np.zeros(1, np.uint32), C.c_int64(0), np.zeros(3)
    tri[0, 1, 0] = tri[0, 2, 1] = 1.0
    assert lib.cpf_source_table_host(None, None, None, 0.0, 0.0, 1, p(rec), p(hi), C.byref(k)) == L.CPF_ERR_ARG
    assert lib.cpf_source_table_host(p(tri), None, None, 0.0, 0.0, 1, p(rec), p(hi), None) == L.CPF_ERR_ARG
    assert lib.cpf_source_table_host(p(tri), None, None, 0.0, 0.0, -1, p(rec), p(hi), C.byref(k)) == L.CPF_ERR_ARG
    assert lib.cpf_source_table_host(p(tri), None, None, 0.0, 0.0, 1, p(rec), p(hi), C.byref(k)) == L.CPF_OK and k.value == 1
    assert lib.cpf_source_positions_host(1, None, 1, 0, None, p(hi), 1, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_positions_host(1, None, 1, 0, p(rec), None, 1, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_positions_host(1, None, 1, 0, p(rec), p(hi), 0, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_positions_host(1, None, 1, 0, p(rec), p(hi), 1, None) == L.CPF_ERR_ARG
    assert lib.cpf_source_positions_host(1, None, -1, 0, p(rec), p(hi), 1, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_positions_host(1, None, 1, 0, p(rec), p(hi), 1, p(out)) == L.CPF_OK
    assert lib.cpf_set_source_triangles(None, p(tri), None, None, 0.0, 0.0, 1) == L.CPF_ERR_ARG
    assert lib.cpf_get_source_table(None, None, None, C.byref(k)) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_source(None, -1) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_source_dev(None, None, None, None, None, None, 0, -1, 0) == L.CPF_ERR_ARG


# ------------------------------------------------------------------------------------------------ 2. the position
@pytest.mark.parametrize("seed", SEEDS)
def test_2_positions_are_the_numpy_statement_bit_for_bit(oracle_libs, graded, seed):
    m = graded["tri"].shape[0]
    rng = np.random.default_rng(8)
    depth = np.stack([rng.uniform(0.0, 0.01, size=m), rng.uniform(0.02, 0.05, size=m)], 1)
    pts = {}
    for tri in (graded["tri"], graded["tri"] @ SHEAR.T):
        rec, hi = api.source_table_host(tri, None, depth)
        for epoch in (0, 1, 4_000_000_000):
            got = api.source_positions_host(seed, GIDS, epoch, rec, hi)
            want, t, u1, u2, d = SP.positions(seed, GIDS, epoch, rec, hi, want_parts=True)
            assert got.shape == (GIDS.size, 3)
            assert np.array_equal(_bits(got), _bits(want)), (seed, epoch, got, want)
            v1, v2, dd = SP.recompute(got, rec, t)
            tol = 1e-12
            assert (v1 >= -tol).all() and (v2 >= -tol).all() and (v1 + v2 <= 1.0 + tol).all()
            assert (dd >= rec[t, 12] - tol).all() and (dd <= rec[t, 12] + rec[t, 13] + tol).all()
            assert np.allclose(v1, u1, atol=1e-11, rtol=0) and np.allclose(v2, u2, atol=1e-11, rtol=0)
            assert (u1 >= 0).all() and (u2 >= 0).all() and (u1 + u2 <= 1.0).all() and (d >= rec[t, 12]).all() and (d <= rec[t, 12] + rec[t, 13]).all()
            pts[(tri is graded["tri"], epoch)] = got
            for a, b in itertools.combinations(range(GIDS.size), 2):
                assert (got[a] != got[b]).any(), (a, b)
    for a, b in itertools.combinations([k for k in pts if k[0]], 2):         # different epochs: different points
        assert (pts[a] != pts[b]).any(1).all()
    rec, hi = api.source_table_host(graded["tri"], None, depth)
    assert (api.source_positions_host(seed ^ 1, GIDS, 0, rec, hi) != pts[(True, 0)]).any(1).all()   # another seed: another stream
    # gid None is the index
    assert np.array_equal(_bits(api.source_positions_host(seed, None, 3, rec, hi, n=130)),
                          _bits(SP.positions(seed, np.arange(130), 3, rec, hi)))
    assert api.source_positions_host(seed, None, 3, rec, hi, n=0).shape == (0, 3)
    # a box draw of the same (seed, gid, epoch) is another point: the key differs
    lo, up = graded["tri"].reshape(-1, 3).min(0), graded["tri"].reshape(-1, 3).max(0) + (0.05, 0.0, 0.0)
    assert (api.respawn_positions_host(seed, GIDS, 0, lo, up) != pts[(True, 0)]).any(1).all()
    w_box = np.array([R.cellwalk().philox(np.array([int(g) & 0xFFFFFFFF, (int(g) >> 32) & 0xFFFFFFFF, 0, 0], np.uint32),
                                          np.array([seed, R.KEY1], np.uint32), rounds=7) for g in GIDS])
    assert (w_box != SP.words(seed, GIDS, 0)).any(1).all() and SP.KEY1 == 0x43504633 != R.KEY1


def test_2_depth_zero_stays_in_the_plane(oracle_libs, graded):
    ids = np.arange(5000)
    for tri in (graded["tri"], graded["tri"] @ SHEAR.T):
        rec, hi = api.source_table_host(tri, None, (0.0, 0.0))
        got = api.source_positions_host(9, ids, 0, rec, hi)
        want, t, _, _, _ = SP.positions(9, ids, 0, rec, hi, want_parts=True)
        assert np.array_equal(_bits(got), _bits(want))
        size = np.sqrt(np.maximum((rec[t, 3:6] ** 2).sum(1), (rec[t, 6:9] ** 2).sum(1)))
        # the distance from the plane, in extended precision: the point's own rounding is all there is
        off = np.abs(((got.astype(np.longdouble) - rec[t, 0:3]) * rec[t, 9:12]).sum(1)).astype(np.float64)
        print("MEASURED plane distance / size: max %.3g" % (off / size).max())
        if tri is graded["tri"]:
            assert (got[:, 0] == 0.0).all()                                   # the x = 0 patch: exactly
        assert (off <= 1e-15 * size).all()


# ------------------------------------------------------------------------------------------------ 3. the weights
N_DRAWS = 200_000
WEIGHT_SEED = 9


def _outliers(counts, w):
    p = w / w.sum()
    mean, sigma = N_DRAWS * p, np.sqrt(N_DRAWS * p * (1.0 - p))
    return int((np.abs(counts - mean) > 5.0 * sigma).sum())


def test_3_weights_do_what_they_say(oracle_libs, graded):
    tri, area = graded["tri"], graded["area"]
    m = tri.shape[0]
    made_up = np.geomspace(1.0, 50.0, m)[np.random.default_rng(2).permutation(m)]          # a factor 50 between largest and smallest
    ids = np.arange(N_DRAWS)
    counts = {}
    for name, w in (("area", None), ("made up", made_up)):
        rec, hi = api.source_table_host(tri, w)
        # the triangle of every draw: the statement's pick, and -- through the library -- the triangle the point lies on
        t = SP.pick(hi, SP.words(WEIGHT_SEED, ids, 0)[:, 0])
        got = api.source_positions_host(WEIGHT_SEED, ids, 0, rec, hi)
        v1, v2, dd = SP.recompute(got, rec, t)
        assert (v1 >= -1e-12).all() and (v2 >= -1e-12).all() and (v1 + v2 <= 1 + 1e-12).all() and (np.abs(dd) <= 1e-15).all()
        counts[name] = np.bincount(rec[t, 14].astype(np.int64), minlength=m)
    print("MEASURED outliers beyond 5 sigma: area draws vs area %d, vs made up %d; made-up draws vs made up %d, vs area %d"
          % (_outliers(counts["area"], area), _outliers(counts["area"], made_up), _outliers(counts["made up"], made_up),
             _outliers(counts["made up"], area)))
    assert _outliers(counts["area"], area) == 0 and _outliers(counts["made up"], made_up) == 0
    assert _outliers(counts["area"], made_up) >= 1 and _outliers(counts["made up"], area) >= 1


# ------------------------------------------------------------------------------------------------ 4. CudaParticles
class _Recorder:
    """Stands in for ``api.Context``: records the calls ``CudaParticles`` makes (no library, no GPU)."""

    def __init__(self, device=0):
        self.calls = []

    def set_option(self, key, value): pass
    def set_mesh(self, mesh): pass
    def set_velocity(self, U): pass
    def set_sink_cells(self, cells): self.calls.append(("sink_cells", tuple(cells)))
    def set_source_triangles(self, tri, weights=None, depth=(0.0, 0.0)):
        self.calls.append(("source_triangles", np.asarray(tri).shape, None if weights is None else tuple(weights), tuple(np.ravel(depth))))
    def seed_box(self, n, lo, hi, order=1): pass
    def locate_initial(self): return 0
    def sort_by_cell(self): pass
    def step(self, dt, D, n, flags): self.calls.append(("step", n))
    def occupancy_sample(self): self.calls.append(("sample",))
    def sink_apply(self): self.calls.append(("sink",))
    def respawn_box(self, lo, hi, max_count): self.calls.append(("respawn", tuple(lo), tuple(hi), max_count))
    def respawn_source(self, max_count=-1): self.calls.append(("respawn_source", max_count))
    def close(self): pass


def test_4_advect_order_is_source_step_sink_respawn_source_sample(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    for key in ("sourceTriangles", "sourceWeights", "sourceDepth"):
        assert key not in api.DICT_DEFAULTS                                  # this library's own keys
    dt = 2.0 ** -13
    seeding = ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    tri = np.zeros((2, 3, 3))
    base = dict(dt=dt, saveInterval=10, occupancyInterval=4, recycleInterval=2, sinkCells=[3, 1], seedingBox=seeding)
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(base, sourceTriangles=tri, sourceWeights=[1.0, 2.0], sourceDepth=(0.0, 0.5)))
    assert p.advect(0.0, 6 * dt) == 6
    S, K, Rs = ("sample",), ("sink",), ("respawn_source", -1)
    T = ("source_triangles", (2, 3, 3), (1.0, 2.0), (0.0, 0.5))
    assert p.ctx.calls == [("sink_cells", (3, 1)), T, ("step", 2), K, Rs, ("step", 2), K, Rs, S, ("step", 2), K, Rs]
    # the defaults: area weights, depth 0; a source box given as well is unused
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(base, sourceTriangles=tri, sourceBox=((0, 0, 0), (0.1, 2, 3))))
    q.advect(0.0, 2 * dt)
    assert q.ctx.calls == [("sink_cells", (3, 1)), ("source_triangles", (2, 3, 3), None, (0.0, 0.0)), ("step", 2), K, Rs]
    # without the key every call is the call of today
    r = api.CudaParticles(None, np.zeros((4, 3)), dict(base, sourceWeights=[1.0, 2.0], sourceDepth=(0.0, 0.5)))
    r.advect(0.0, 6 * dt)
    Rb = ("respawn", seeding[0], seeding[1], -1)
    assert r.ctx.calls == [("sink_cells", (3, 1)), ("step", 2), K, Rb, ("step", 2), K, Rb, S, ("step", 2), K, Rb]
    # recycleInterval 0: the keys are inert
    s = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, sinkCells=[0], sourceTriangles=tri))
    s.advect(0.0, 7 * dt)
    assert s.ctx.calls == [("step", 7)]


# ------------------------------------------------------------------------------------------------ 5. patch_faces, face_triangles
def _check_fan(mesh, faces):
    tri, of = mesh.face_triangles(faces)
    fo = mesh.face_offsets.astype(np.int64)
    at = 0
    for f in faces:
        loop = mesh.face_verts[fo[f]:fo[f + 1]]
        for k in range(1, loop.size - 1):
            assert of[at] == f
            assert np.array_equal(tri[at], mesh.points[[loop[0], loop[k], loop[k + 1]]]), (f, k)
            at += 1
    assert at == tri.shape[0] == of.size and of.dtype == np.int32 and tri.dtype == np.float64
    # the triangles' area vectors add up to the faces' (OpenFOAM's faceAreas)
    vec = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    total = np.zeros((mesh.n_faces, 3)); np.add.at(total, of, vec)
    areas = mesh.face_centres_areas()[1]
    mag = np.sqrt((areas[faces] ** 2).sum(1))
    assert np.allclose(np.sqrt((total[faces] ** 2).sum(1)), mag, rtol=1e-14, atol=0)
    assert abs(np.sqrt((vec ** 2).sum(1)).sum() - mag.sum()) <= 1e-14 * mag.sum()
    return tri, of


def test_5_patch_faces_and_face_triangles_on_pitzdaily(pitz):
    mesh = pitz["mesh"]
    by = {n: (s, k) for n, _, s, k in mesh.patches}
    faces = mesh.patch_faces("inlet")
    assert faces.dtype == np.int32 and np.array_equal(faces, np.arange(by["inlet"][0], by["inlet"][0] + 30))
    tri, of = _check_fan(mesh, faces)
    assert tri.shape == (60, 3, 3) and np.array_equal(of, np.repeat(faces, 2))
    assert np.array_equal(np.unique(mesh.owner[faces]), mesh.patch_cells("inlet"))
    both = mesh.patch_faces("outlet", "inlet")                               # in the order given
    assert np.array_equal(both[-30:], faces) and both.size == 30 + by["outlet"][1]
    assert mesh.patch_faces().size == 0 and mesh.face_triangles([])[0].shape == (0, 3, 3)
    with pytest.raises(KeyError):
        mesh.patch_faces("inlet", "no such patch")
    # the inflow weights: area * max(0, -U_owner . n_out); a field that leaves through the inlet has none
    U = pitz["U_uniform"]
    w = api.inflow_weights(mesh, U, tri, of)
    n_out = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.sqrt((n_out ** 2).sum(1))
    n_out /= (2.0 * area)[:, None]
    want = area * np.maximum(0.0, -(U[mesh.owner[of]] * n_out).sum(1))
    assert np.allclose(w, want, rtol=1e-14, atol=0) and ((w > 0).all() or (w == 0).all())
    assert (api.inflow_weights(mesh, -U, tri, of) == 0.0).all() or (w == 0.0).all()
    assert (w > 0).all() or (api.inflow_weights(mesh, -U, tri, of) > 0).all()


def test_5_patch_faces_and_face_triangles_on_tjunction():
    from cudaparticlesfoam_amd.cases.tjunction import tjunction_mesh
    mesh = tjunction_mesh()
    by = {n: (s, k) for n, _, s, k in mesh.patches}
    for names in (("inlet",), ("outlet1", "outlet2")):
        faces = mesh.patch_faces(*names)
        assert faces.size == sum(by[n][1] for n in names) > 0
        tri, of = _check_fan(mesh, faces)
        assert tri.shape[0] == 2 * faces.size
    with pytest.raises(KeyError):
        mesh.patch_faces("outlet")


# ------------------------------------------------------------------------------------------------ the recycled runs' CPU statement
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_the_cpu_statement_of_the_source_runs_recycles(oracle_libs, name):
    """The runs tests/test_gpu_source.py compares bit for bit do recycle, and the patch source places every draw -- conditions on
    the CPU statement, not measurements: at least 5 % of the cloud absorbed, somebody respawned twice, drawn == placed."""
    r = SP.run(name)
    t = api.build_mesh_tables_host(r.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    cell0 = R.brute_locate(r.xyz, tables)
    assert (cell0 >= 0).all() and (r.weights > 0).all() and (r.depth[:, 1] > r.depth[:, 0]).all()
    rec, hi = api.source_table_host(r.tri, r.weights, r.depth)
    same, same_hi = SP.table(r.tri, r.weights, r.depth, exact=False)
    assert np.array_equal(hi, same_hi) and np.array_equal(_bits(rec), _bits(same))          # (axis-aligned: nIn is exact too)
    xyz, cell, absorbed, drawn, placed, times = r.cpu(tables, cell0)
    print("MEASURED %s | absorbed %d of %d | drawn %d placed %d | respawned twice or more: %d" % (name, absorbed, R.N, drawn, placed,
                                                                                                 int((times >= 2).sum())))
    assert absorbed >= 0.05 * R.N and (times >= 2).any()
    assert drawn == placed == absorbed
    assert np.isfinite(xyz).all() and (cell >= 0).all()
