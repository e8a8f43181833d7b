"""CPU: the host side of the per-cell occupancy (include/cpf.h "per-cell occupancy"): cell volumes against the numpy statement of
OpenFOAM's formula, argument handling without a device, and the rule by which ``CudaParticles.advect`` cuts its fused launches."""
import itertools

import numpy as np
import pytest

import warped as W
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh
from cudaparticlesfoam_amd.cases.polygons import cut_corner_box


def _meshes(pitz):
    return dict(box=box_mesh(5, 4, 3), pitz=pitz["mesh"], prisms=cut_corner_box(6, 5, 3)[0],
                warped=W.warp_mesh(box_mesh(6, 5, 4), 0.05))


@pytest.mark.parametrize("name", ["box", "pitz", "prisms", "warped"])
def test_cell_volumes_host_matches_polymesh(pitz, name):
    """Both sides are the same fp64 formula over at most a few dozen terms per cell (rounding ~1e-15): relative 1e-12."""
    mesh = _meshes(pitz)[name]
    V = api.cell_volumes_host(mesh)
    ref = mesh.cell_centres_volumes()[1]
    assert V.shape == ref.shape == (mesh.n_cells,) and (ref > 0).all()
    rel = np.abs(V - ref) / np.abs(ref)
    print(name, "max relative difference", rel.max())
    assert rel.max() <= 1e-12
    if name == "box":
        assert np.abs(V - 1.0).max() <= 1e-12            # unit cubes


def test_cell_volumes_host_rejects_nulls_and_bad_meshes():
    lib = L.load()
    mesh = box_mesh(2, 2, 2)
    a = api._mesh_args(mesh)
    V = np.empty(mesh.n_cells)
    p = api._ptr
    assert lib.cpf_cell_volumes_host(p(a[0]), mesh.n_points, p(a[1]), p(a[2]), mesh.n_faces, p(a[3]), p(a[4]), mesh.n_internal,
                                     mesh.n_cells, None) == L.CPF_ERR_ARG
    assert lib.cpf_cell_volumes_host(None, mesh.n_points, p(a[1]), p(a[2]), mesh.n_faces, p(a[3]), p(a[4]), mesh.n_internal,
                                     mesh.n_cells, p(V)) == L.CPF_ERR_ARG
    bad = a[3].copy(); bad[0] = mesh.n_cells + 5         # an owner that is no cell
    assert lib.cpf_cell_volumes_host(p(a[0]), mesh.n_points, p(a[1]), p(a[2]), mesh.n_faces, p(bad), p(a[4]), mesh.n_internal,
                                     mesh.n_cells, p(V)) == L.CPF_ERR_MESH


def test_null_context_is_rejected_without_a_device():
    lib = L.load()
    counts = np.zeros(4, np.uint64)
    assert lib.cpf_occupancy_sample(None) == L.CPF_ERR_ARG
    assert lib.cpf_occupancy_sample_dev(None, None, 0) == L.CPF_ERR_ARG
    assert lib.cpf_occupancy_reset(None) == L.CPF_ERR_ARG
    assert lib.cpf_get_occupancy(None, api._ptr(counts), None) == L.CPF_ERR_ARG
    assert lib.cpf_get_cell_volumes(None, api._ptr(np.zeros(4))) == L.CPF_ERR_ARG
    assert not counts.any()


def _inline_rule(step, remaining, save_interval, has_writer, will_write):
    """The chunk rule as ``advect`` stated it inline before ``occupancyInterval`` existed."""
    if will_write:
        return 1
    to_next = save_interval - (step % save_interval) if has_writer else 10 ** 9
    return max(1, min(remaining, to_next))


def test_next_chunk_without_occupancy_is_the_old_rule():
    for step, remaining, save, writer in itertools.product(range(0, 41), range(1, 13), (1, 2, 3, 7, 10), (False, True)):
        for will_write in ((False, True) if writer else (False,)):
            got = api._next_chunk(step, remaining, save, 0, writer, will_write)
            assert got == _inline_rule(step, remaining, save, writer, will_write), (step, remaining, save, writer, will_write)


def test_next_chunk_ends_at_samples_outputs_and_call_ends():
    ends, step = [], 0
    for _ in range(3):                                   # three advect calls of 10 cycles, no writer
        done = 0
        while done < 10:
            chunk = api._next_chunk(step, 10 - done, 10, 4, False, False)
            assert chunk >= 1
            step += chunk; done += chunk
            ends.append(step)
    assert ends == [4, 8, 10, 12, 16, 20, 24, 28, 30]
    # with a writer the output points cut as well, and a cycle that writes runs alone
    assert api._next_chunk(8, 10, 10, 4, True, False) == 2
    assert api._next_chunk(9, 10, 6, 4, True, False) == 3
    assert api._next_chunk(12, 10, 10, 4, True, True) == 1


class _Recorder:
    """Stands in for ``api.Context``: records the calls ``CudaParticles`` makes (no library, no GPU)."""

    def __init__(self, device=0):
        self.calls = []

    def set_option(self, key, value): pass
    def set_mesh(self, mesh): pass
    def set_velocity(self, U): pass
    def seed_box(self, n, lo, hi, order=1): pass
    def locate_initial(self): return 0
    def sort_by_cell(self): pass
    def step(self, dt, D, n, flags): self.calls.append(("step", n, flags))
    def occupancy_sample(self): self.calls.append(("sample",))
    def concentration(self): return "forwarded"
    def get_particles(self, want_vel=False):
        z = np.zeros((2, 4))
        return (z, np.zeros(2, np.int32), z) if want_vel else (z, np.zeros(2, np.int32))
    def close(self): pass


def test_advect_samples_at_multiples_and_is_unchanged_without_the_key(monkeypatch):
    monkeypatch.setattr(api, "Context", _Recorder)
    assert "occupancyInterval" not in api.DICT_DEFAULTS               # this library's own key, not one of the reference's
    dt = 2.0 ** -13
    fuse = L.STEP_FUSE_CYCLES
    p = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, saveInterval=10, occupancyInterval=4))
    for k in range(3):
        assert p.advect(k * 10 * dt, 10 * dt) == 10
    S = ("sample",)
    assert p.ctx.calls == [("step", 4, fuse), S, ("step", 4, fuse), S, ("step", 2, fuse),
                           ("step", 2, fuse), S, ("step", 4, fuse), S, ("step", 4, fuse), S,
                           ("step", 4, fuse), S, ("step", 4, fuse), S, ("step", 2, fuse)]
    assert p.concentration() == "forwarded"
    # without the key: the launches of before, and no sample -- with and without a writer
    q = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, saveInterval=10))
    assert q.occupancyInterval == 0
    for k in range(3):
        q.advect(k * 10 * dt, 10 * dt)
    assert q.ctx.calls == [("step", 10, fuse)] * 3
    w = api.CudaParticles(None, np.zeros((4, 3)), dict(dt=dt, saveInterval=10), writer=lambda *a: None)
    w.ctx.calls.clear()
    w.advect(0.0, 20 * dt)
    assert w.ctx.calls == [("step", 1, L.STEP_STORE_VEL), ("step", 9, fuse)] * 2
