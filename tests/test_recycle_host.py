"""CPU: the host side of the recycling cloud (include/cpf.h "recycling"): the respawn position against its numpy statement on the
oracle's Philox, bit for bit; the rule by which ``CudaParticles.advect`` cuts its fused launches, with recycle points; the owner
cells of a patch; argument handling without a device."""
import itertools

import numpy as np
import pytest

import recycle as R
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

GIDS = np.array([0, 1, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 62 + 5], np.int64)
BOX = ((-0.3, 0.1, -7.0), (0.7, 0.1 + 1.0 / 3.0, -6.9))            # negative and non-dyadic bounds


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("seed", [9, 1591593751, 0xFFFFFFFF])
def test_positions_are_the_numpy_statement_bit_for_bit(oracle_libs, seed):
    pts = {}
    for epoch in (0, 1, 4_000_000_000):
        got = api.respawn_positions_host(seed, GIDS, epoch, *BOX)
        want = R.positions(seed, GIDS, epoch, *BOX)
        assert got.shape == (GIDS.size, 3)
        assert np.array_equal(_bits(got), _bits(want)), (seed, epoch, got, want)
        assert (got >= np.array(BOX[0])).all() and (got <= np.array(BOX[1])).all()
        pts[epoch] = got
        # different gids: different points (all three coordinates of all nine differ pairwise)
        for a, b in itertools.combinations(range(GIDS.size), 2):
            assert (got[a] != got[b]).all(), (a, b)
    # different epochs: different points for every gid
    for a, b in itertools.combinations(pts, 2):
        assert (pts[a] != pts[b]).any(1).all()
    # another seed: another stream
    assert (api.respawn_positions_host(seed ^ 1, GIDS, 0, *BOX) != pts[0]).any(1).all()


def test_gid_none_is_the_index_and_a_flat_box_is_its_plane(oracle_libs):
    n = 130
    got = api.respawn_positions_host(9, None, 3, *BOX, n=n)
    assert np.array_equal(_bits(got), _bits(api.respawn_positions_host(9, np.arange(n), 3, *BOX)))
    assert np.array_equal(_bits(got), _bits(R.positions(9, np.arange(n), 3, *BOX)))
    flat = api.respawn_positions_host(9, None, 0, (0.0, 0.5, 0.0), (1.0, 0.5, 1.0), n=n)
    assert (flat[:, 1] == 0.5).all() and np.unique(flat[:, 0]).size == n
    assert api.respawn_positions_host(9, None, 0, *BOX, n=0).shape == (0, 3)


def test_host_entry_rejects_nulls_and_contexts_are_checked_without_a_device():
    lib = L.load()
    lo, hi = np.zeros(3), np.ones(3)
    out = np.zeros(3)
    p = api._ptr
    assert lib.cpf_respawn_positions_host(1, None, 1, 0, None, p(hi), p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_positions_host(1, None, 1, 0, p(lo), p(hi), None) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_positions_host(1, None, -1, 0, p(lo), p(hi), p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_set_sink_cells(None, None, 0) == L.CPF_ERR_ARG
    assert lib.cpf_sink_apply(None) == L.CPF_ERR_ARG
    assert lib.cpf_sink_apply_dev(None, None, 0) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_box(None, p(lo), p(hi), -1) == L.CPF_ERR_ARG
    assert lib.cpf_respawn_box_dev(None, None, None, None, None, None, 0, p(lo), p(hi), -1, 0) == L.CPF_ERR_ARG
    assert lib.cpf_get_recycle_counts(None, p(np.zeros(4, np.int64))) == L.CPF_ERR_ARG
    assert lib.cpf_recycle_reset_counts(None) == L.CPF_ERR_ARG


# ------------------------------------------------------------------------------------------------ _next_chunk
def _before(step, remaining, save_interval, occupancy_interval, has_writer, will_write):
    """``api._next_chunk`` as it stood before ``recycleInterval`` existed."""
    if will_write:
        return 1
    chunk = remaining
    if has_writer:
        chunk = min(chunk, save_interval - (step % save_interval))
    if occupancy_interval > 0:
        chunk = min(chunk, occupancy_interval - (step % occupancy_interval))
    return max(1, chunk)


def test_next_chunk_without_recycling_is_the_function_of_before():
    for step, remaining, save, writer in itertools.product(range(0, 41), range(1, 13), (1, 2, 3, 7, 10), (False, True)):
        for will_write in ((False, True) if writer else (False,)):
            for occ in (0, 4):
                want = _before(step, remaining, save, occ, writer, will_write)
                assert api._next_chunk(step, remaining, save, occ, writer, will_write) == want
                assert api._next_chunk(step, remaining, save, occ, writer, will_write, 0) == want


def test_next_chunk_ends_at_recycle_points_samples_outputs_and_call_ends():
    ends, step = [], 0
    for _ in range(3):                                   # three advect calls of 10 cycles, no writer: recycle every 3, sample every 4
        done = 0
        while done < 10:
            chunk = api._next_chunk(step, 10 - done, 10, 4, False, False, 3)
            assert chunk >= 1
            step += chunk; done += chunk
            ends.append(step)
    assert ends == [3, 4, 6, 8, 9, 10, 12, 15, 16, 18, 20, 21, 24, 27, 28, 30]
    assert api._next_chunk(8, 10, 10, 0, True, False, 6) == 2          # the output point first
    assert api._next_chunk(7, 10, 10, 0, True, False, 4) == 1          # the recycle point first
    assert api._next_chunk(12, 10, 10, 4, True, True, 3) == 1          # a cycle that writes runs alone
    assert api._next_chunk(5, 2, 10, 0, False, False, 100) == 2        # the end of the call


class _Recorder:
    """Stands in for ``api.Context``: records the calls ``CudaParticles`` makes (no library, no GPU)."""

    def __init__(self, device=0):
        self.calls = []

    def set_option(self, key, value): pass
    def set_mesh(self, mesh): pass
    def set_velocity(self, U): pass
    def set_sink_cells(self, cells): self.calls.append(("sink_cells", tuple(cells)))
    def seed_box(self, n, lo, hi, order=1): pass
    def locate_initial(self): return 0
    def sort_by_cell(self): pass
    def step(self, dt, D, n, flags): self.calls.append(("step", n))
    def occupancy_sample(self): self.calls.append(("sample",))
    def sink_apply(self): self.calls.append(("sink",))
    def respawn_box(self, lo, hi, max_count): self.calls.append(("respawn", tuple(lo), tuple(hi), max_count))
    def recycle_counts(self): return "forwarded"
    def close(self): pass


def test_advect_order_is_sink_respawn_sample(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    for key in ("recycleInterval", "sinkCells", "sourceBox"):
        assert key not in api.DICT_DEFAULTS                              # this library's own keys
    dt = 2.0 ** -13
    seeding = ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, saveInterval=10, occupancyInterval=4, recycleInterval=2, sinkCells=[3, 1],
                                                       seedingBox=seeding))
    assert p.advect(0.0, 6 * dt) == 6
    S, K, Rs = ("sample",), ("sink",), ("respawn", seeding[0], seeding[1], -1)           # sourceBox defaults to the seedingBox
    assert p.ctx.calls == [("sink_cells", (3, 1)), ("step", 2), K, Rs, ("step", 2), K, Rs, S, ("step", 2), K, Rs]
    assert p.recycle_counts() == "forwarded"
    src = ((0.0, 0.0, 0.0), (0.1, 2.0, 3.0))
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, recycleInterval=5, sinkCells=[0], sourceBox=src, seedingBox=seeding))
    q.advect(0.0, 7 * dt)
    assert q.ctx.calls == [("sink_cells", (0,)), ("step", 5), K, ("respawn", src[0], src[1], -1), ("step", 2)]
    # recycleInterval 0: the keys are inert
    r = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, sinkCells=[0], sourceBox=src))
    r.advect(0.0, 7 * dt)
    assert r.ctx.calls == [("step", 7)]


# ------------------------------------------------------------------------------------------------ patch_cells
def _direct(mesh, *names):
    by = {n: (s, k) for n, _, s, k in mesh.patches}
    return np.unique(np.concatenate([mesh.owner[by[n][0]:by[n][0] + by[n][1]] for n in names]))


def test_patch_cells_on_pitzdaily(pitz):
    mesh = pitz["mesh"]
    got = mesh.patch_cells("outlet")
    assert got.dtype == np.int32 and got.size == 57 and np.array_equal(got, _direct(mesh, "outlet"))
    assert np.array_equal(got, np.sort(got)) and np.unique(got).size == got.size
    both = mesh.patch_cells("inlet", "outlet")
    assert np.array_equal(both, _direct(mesh, "inlet", "outlet")) and both.size == 30 + 57
    assert mesh.patch_cells().size == 0
    with pytest.raises(KeyError):
        mesh.patch_cells("outlet", "no such patch")


def test_patch_cells_on_tjunction():
    from cudaparticlesfoam_amd.cases.tjunction import tjunction_mesh
    mesh = tjunction_mesh()
    for names in (("outlet1",), ("outlet2",), ("outlet1", "outlet2")):
        got = mesh.patch_cells(*names)
        assert np.array_equal(got, _direct(mesh, *names)) and got.size == 400 * len(names)
    with pytest.raises(KeyError):
        mesh.patch_cells("outlet")


# ------------------------------------------------------------------------------------------------ the recycled runs' CPU statement
@pytest.mark.parametrize("name", ["graded box", "thin box"])
def test_the_cpu_statement_of_the_recycled_runs_recycles(oracle_libs, name):
    """The runs tests/test_gpu_recycle.py compares bit for bit do recycle -- conditions on the CPU statement, not measurements: at
    least 5 % of the cloud is absorbed and somebody is respawned twice; the brute-force locate is the oracle's initial locate."""
    r = R.run(name)
    t = api.build_mesh_tables_host(r.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    cell0 = R.brute_locate(r.xyz, tables)
    cw = R.cellwalk()
    ref0 = cw.locate_initial(r.xyz[:, 0].copy(), r.xyz[:, 1].copy(), r.xyz[:, 2].copy(), cw.build(r.mesh))
    assert np.array_equal(cell0, ref0) and (cell0 >= 0).all()
    xyz, cell, absorbed, drawn, placed, times = r.cpu(tables, cell0)
    print("MEASURED %s | absorbed %d of %d | drawn %d placed %d | respawned twice or more: %d" % (name, absorbed, R.N, drawn, placed,
                                                                                                 int((times >= 2).sum())))
    assert absorbed >= 0.05 * R.N and (times >= 2).any()
    assert np.isfinite(xyz).all()
    if name == "graded box":
        assert drawn > placed                                            # the source box sticks out: some draws stay dead
    else:
        assert drawn == placed == absorbed and (r.U[:, 2] == 0.0).all() and R.N >= 8 * r.mesh.n_cells
