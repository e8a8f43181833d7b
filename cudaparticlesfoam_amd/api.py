"""Python host side above the C-ABI.

``Context`` is a thin object wrapper over ``include/cpf.h`` (numpy in / numpy out).
``CudaParticles`` mirrors the reference's two header fragments -- the only "operator
interface" the reference has for this path:

* ``CudaParticles(mesh, U, dict)``        == ``#include "initCuda.H"`` (src/initCuda.H:33-205)
* ``CudaParticles.advect(time, deltaT)``  == ``#include "advect.H"``   (src/advect.H:33-205)

with the same dictionary keys and defaults (src/initCuda.H:50-57), the same
``nCycles = max(ceil(deltaT/dt), 1)`` sub-cycling (src/advect.H:36-37) and the same
output cadence (src/advect.H:166).  All compute happens in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Optional

import numpy as np

from . import _lib as L


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# cpf_sink_record (include/cpf.h "sink log"): what ``Context.sink_log_read`` returns, 64 bytes a record, little-endian
SINK_LOG_DTYPE = np.dtype({
    "names": ["id", "apply", "cycle", "x", "y", "z", "dose", "age", "cell", "origin", "group", "zone", "fields", "reserved"],
    "formats": ["<i8", "<u4", "<u4", "<f8", "<f8", "<f8", "<f8", "<u4", "<i4", "u1", "u1", "u1", "u1", "<u4"],
    "offsets": [0, 8, 12, 16, 24, 32, 40, 48, 52, 56, 57, 58, 59, 60],
    "itemsize": 64})


class Context:
    """One GPU, one mesh, one (optional) context-owned particle cloud."""

    def __init__(self, device: int = 0):
        self.lib = L.load()
        h = C.c_void_p()
        st = self.lib.cpf_create(device, C.byref(h))
        if st != L.CPF_OK:
            raise L.CpfError(st, (self.lib.cpf_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self.n_cells = 0

    # -- plumbing
    def _ck(self, st):
        L.check(self.lib, self.h, st)

    def close(self):
        for sh in list(getattr(self, "_shards", [])):        # shards made on this context (parallel.ShardedCloud) borrow it
            sh.close()
        if getattr(self, "h", None):
            self.lib.cpf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, hip_stream: int):
        self._ck(self.lib.cpf_set_stream(self.h, C.c_void_p(hip_stream)))

    def use_own_stream(self):
        self._ck(self.lib.cpf_use_own_stream(self.h))

    def synchronize(self):
        self._ck(self.lib.cpf_synchronize(self.h))

    # -- mesh / velocity
    def set_mesh(self, mesh):
        """``mesh`` exposes points, face_offsets, face_verts, owner, neighbour, n_cells (cases.PolyMesh)."""
        lab = np.int64 if np.asarray(mesh.owner).dtype == np.int64 else np.int32
        pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
        fo = np.ascontiguousarray(mesh.face_offsets, dtype=lab)
        fv = np.ascontiguousarray(mesh.face_verts, dtype=lab)
        ow = np.ascontiguousarray(mesh.owner, dtype=lab)
        ne = np.ascontiguousarray(mesh.neighbour, dtype=lab)
        fn = self.lib.cpf_set_mesh_l64 if lab == np.int64 else self.lib.cpf_set_mesh
        self._ck(fn(self.h, _ptr(pts), pts.shape[0], _ptr(fo), _ptr(fv), ow.shape[0], _ptr(ow), _ptr(ne), ne.shape[0],
                    int(mesh.n_cells)))
        self.n_cells = int(mesh.n_cells)

    def set_mesh_parts(self, parts):
        """Rank-direct ingest: ``parts`` = the pieces of a decomposed mesh in rank order (each exposes the PolyMesh
        fields); they are stitched on the host (cpf_merge_mesh_parts) and uploaded as one mesh."""
        arr, keep = pack_mesh_parts(parts)
        r = self.lib.cpf_set_mesh_parts(self.h, arr, len(parts))
        if r == L.CPF_ERR_MESH and not self.lib.cpf_last_error(self.h):
            raise L.CpfError(r, (self.lib.cpf_merge_last_error() or b"").decode())
        self._ck(r)
        self.n_cells = int(sum(int(p.n_cells) for p in parts))

    def mesh_info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.cpf_mesh_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_cells=a.value, n_slots=b.value, device_bytes=c.value)

    def mesh_tables(self):
        info = self.mesh_info()
        off = np.empty(info["n_cells"] + 1, np.int32)
        planes = np.empty((info["n_slots"], 4), np.float64)
        nbr = np.empty(info["n_slots"], np.int32)
        self._ck(self.lib.cpf_get_mesh_tables(self.h, _ptr(off), _ptr(planes), _ptr(nbr)))
        return off, planes, nbr

    def mesh_flags(self) -> Dict[str, int]:
        """Which shortcuts of the walk the mesh layer found live: all_hex, z_layered, z_thin, mixed (include/cpf.h)."""
        v = [C.c_int32(0) for _ in range(4)]
        self._ck(self.lib.cpf_get_mesh_flags(self.h, *[C.byref(x) for x in v]))
        return dict(all_hex=v[0].value, z_layered=v[1].value, z_thin=v[2].value, mixed=v[3].value)

    def mesh_groups(self):
        """Face groups of the mesh (coplanar faces of a cell that lead to different cells share one slot): (group_off
        [n_groups + 1], group_nbr); slot neighbour id INT32_MIN + 16 + g marks group g."""
        ng, nm = C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.cpf_get_mesh_groups(self.h, C.byref(ng), C.byref(nm), None, None))
        off = np.zeros(ng.value + 1, np.int32); nbr = np.zeros(max(nm.value, 1), np.int32)
        self._ck(self.lib.cpf_get_mesh_groups(self.h, None, None, _ptr(off), _ptr(nbr)))
        return off, nbr[:nm.value]

    def set_velocity(self, U):
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim != 2 or U.shape[1] != 3:
            raise ValueError("U must be (nCells, 3)")
        self._ck(self.lib.cpf_set_velocity(self.h, _ptr(U), U.shape[0]))

    def set_tets(self, positions, tets, tets_per_cell: int = 12):
        """The tet decomposition the "VertexVelocity" advect mode needs (src/initCuda.H:86-124): positions =
        mesh.points() ++ mesh.C(), tets [nCells * tets_per_cell][4] in cell order."""
        pos = np.ascontiguousarray(positions, dtype=np.float64); t = np.ascontiguousarray(tets, dtype=np.int32)
        self._ck(self.lib.cpf_set_tets(self.h, _ptr(pos), pos.shape[0], _ptr(t), t.shape[0], int(tets_per_cell)))

    def set_vertex_velocity(self, vertex_u):
        u = np.ascontiguousarray(vertex_u, dtype=np.float64)
        self._ck(self.lib.cpf_set_vertex_velocity(self.h, _ptr(u), u.shape[0]))

    def set_velocity_dev(self, ptr: int, n_cells: int):
        self._ck(self.lib.cpf_set_velocity_dev(self.h, C.c_void_p(ptr), n_cells))

    # -- context-owned cloud
    def seed_box(self, n: int, lower, upper, order: int = 1):
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        self._ck(self.lib.cpf_seed_box(self.h, int(n), _ptr(lo), _ptr(hi), order))

    def set_particles(self, xyz, cell=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        c = None if cell is None else np.ascontiguousarray(cell, dtype=np.int32)
        self._ck(self.lib.cpf_set_particles(self.h, xyz.shape[0], _ptr(xyz), _ptr(c)))

    def locate_initial(self) -> int:
        out = C.c_int64()
        self._ck(self.lib.cpf_locate_initial(self.h, C.byref(out)))
        return out.value

    def step(self, dt: float, D: float = 0.0, n_cycles: int = 1, flags: int = 0):
        self._ck(self.lib.cpf_step(self.h, dt, D, n_cycles, flags))

    def sort_by_cell(self):
        self._ck(self.lib.cpf_sort_by_cell(self.h))

    @property
    def n(self) -> int:
        out = C.c_int64()
        self._ck(self.lib.cpf_num_particles(self.h, C.byref(out)))
        return out.value

    def get_particles(self, want_vel: bool = False):
        n = self.n
        xyzw = np.empty((n, 4)); cell = np.empty(n, np.int32)
        vel = np.empty((n, 4)) if want_vel else None
        self._ck(self.lib.cpf_get_particles(self.h, _ptr(xyzw), _ptr(cell), _ptr(vel)))
        return (xyzw, cell, vel) if want_vel else (xyzw, cell)

    def counters(self) -> Dict[str, int]:
        out = np.zeros(4, np.int64)
        self._ck(self.lib.cpf_get_counters(self.h, _ptr(out)))
        return dict(particle_steps=int(out[0]), cells_visited=int(out[1]), reflections=int(out[2]), lost=int(out[3]))

    def set_option(self, key: str, value: float):
        self._ck(self.lib.cpf_set_option(self.h, key.encode(), float(value)))

    def step_kernel_name(self, D: float = 0.0, flags: int = 0) -> str:
        buf = C.create_string_buffer(200)
        self._ck(self.lib.cpf_step_kernel_name(self.h, float(D), int(flags), buf, 200))
        return buf.value.decode()

    def set_seed(self, seed: int):
        self._ck(self.lib.cpf_set_seed(self.h, seed & 0xFFFFFFFF))

    # -- device-array level (pointers as ints, e.g. torch.Tensor.data_ptr())
    def step_dev(self, x, y, z, cell, gid, vel, n, dt, D=0.0, step0=0, n_cycles=1, flags=0):
        self._ck(self.lib.cpf_step_dev(self.h, x, y, z, cell, gid, vel, n, dt, D, step0, n_cycles, flags))

    def locate_initial_dev(self, x, y, z, cell, n):
        self._ck(self.lib.cpf_locate_initial_dev(self.h, x, y, z, cell, n))

    def seed_box_dev(self, x, y, z, first, n, lower, upper, order=1):
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        self._ck(self.lib.cpf_seed_box_dev(self.h, x, y, z, first, n, _ptr(lo), _ptr(hi), order))

    def sort_by_cell_dev(self, x, y, z, cell, gid, n):
        self._ck(self.lib.cpf_sort_by_cell_dev(self.h, x, y, z, cell, gid, n))

    def sort_by_cell_dev_to(self, x, y, z, cell, gid, ox, oy, oz, ocell, ogid, n):
        self._ck(self.lib.cpf_sort_by_cell_dev_to(self.h, x, y, z, cell, gid, ox, oy, oz, ocell, ogid, n))

    def pack_leavers_dev(self, x, y, z, cell, gid, n, cell_lo, n_ranks, my_rank, sendbuf, send_cap, counts, n_stay):
        self._ck(self.lib.cpf_pack_leavers_dev(self.h, x, y, z, cell, gid, n, cell_lo, n_ranks, my_rank, sendbuf,
                                               send_cap, counts, n_stay))

    def mesh_quality(self) -> Dict[str, float]:
        """Quality of the mesh as given (cpf_get_mesh_quality): max_eta / worst_face (face non-planarity), max_xi / worst_cell
        (cell non-convexity), n_cells, n_flagged, n_bad (flagged but left whole), n_derived (cells the walk runs on), tol."""
        q = L.MeshQuality()
        self._ck(self.lib.cpf_get_mesh_quality(self.h, C.byref(q)))
        return _quality_dict(q)

    def cells_to_parent_dev(self, cell_in, cell_out, n):
        """Derived cell ids (device int32) -> parent ids (cpf_cells_to_parent_dev); in and out may alias."""
        self._ck(self.lib.cpf_cells_to_parent_dev(self.h, cell_in, cell_out, n))

    def cell_histogram_dev(self, cell, n, scale, weights):
        self._ck(self.lib.cpf_cell_histogram_dev(self.h, cell, n, scale, weights))

    # -- per-cell occupancy: the concentration field (include/cpf.h "per-cell occupancy")
    def occupancy_sample(self):
        """One sample of the context-owned cloud: every cell's accumulator grows by the number of particles in it now."""
        self._ck(self.lib.cpf_occupancy_sample(self.h))

    def occupancy_sample_dev(self, cell_ptr, n):
        """The same from a device int32 array of DERIVED ids (what ``step_dev`` leaves in its cell array)."""
        self._ck(self.lib.cpf_occupancy_sample_dev(self.h, cell_ptr, n))

    def occupancy_reset(self):
        self._ck(self.lib.cpf_occupancy_reset(self.h))

    def occupancy(self):
        """(counts uint64 [n_cells] per parent cell, n_samples) accumulated since the last reset; synchronises."""
        counts = np.zeros(self.n_cells, np.uint64)
        ns = C.c_int64(0)
        self._ck(self.lib.cpf_get_occupancy(self.h, _ptr(counts), C.byref(ns)))
        return counts, ns.value

    def cell_volumes(self) -> np.ndarray:
        """OpenFOAM's cell volumes of the mesh as given ([n_cells], parent cells; cpf_get_cell_volumes)."""
        V = np.empty(self.n_cells, np.float64)
        self._ck(self.lib.cpf_get_cell_volumes(self.h, _ptr(V)))
        return V

    def concentration(self) -> np.ndarray:
        """Time-averaged particles per unit volume in every cell: counts / (n_samples * V)."""
        counts, ns = self.occupancy()
        if ns == 0:
            raise ValueError("concentration: no occupancy sample yet (occupancy_sample)")
        return counts.astype(np.float64) / (float(ns) * self.cell_volumes())

    # -- recycling: sink cells and a source box (include/cpf.h "recycling")
    def set_sink_cells(self, cells):
        """The sink set: cell ids of the mesh as given (an empty list clears it).  ``PolyMesh.patch_cells`` gives a patch's."""
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1)
        self._ck(self.lib.cpf_set_sink_cells(self.h, _ptr(c) if c.size else None, c.size))

    def sink_apply(self):
        """Every particle of the context-owned cloud that sits in a sink cell becomes lost (cell -1); asynchronous."""
        self._ck(self.lib.cpf_sink_apply(self.h))

    def sink_apply_dev(self, cell_ptr, n):
        """The same on a device int32 array of DERIVED ids."""
        self._ck(self.lib.cpf_sink_apply_dev(self.h, cell_ptr, n))

    def respawn_box(self, lower, upper, max_count: int = -1):
        """Up to ``max_count`` (< 0: all) dead slots of the context-owned cloud, in array order, get a fresh position in the box
        and are located; the cloud's epoch counter goes up by one."""
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        self._ck(self.lib.cpf_respawn_box(self.h, _ptr(lo), _ptr(hi), int(max_count)))

    def respawn_box_dev(self, x, y, z, cell, gid, n, lower, upper, max_count: int = -1, epoch: int = 0):
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        self._ck(self.lib.cpf_respawn_box_dev(self.h, x, y, z, cell, gid, n, _ptr(lo), _ptr(hi), int(max_count), int(epoch)))

    def recycle_counts(self) -> Dict[str, int]:
        """absorbed, drawn, placed since the last reset and the epochs of the context's own cloud; synchronises."""
        out = np.zeros(4, np.int64)
        self._ck(self.lib.cpf_get_recycle_counts(self.h, _ptr(out)))
        return dict(absorbed=int(out[0]), drawn=int(out[1]), placed=int(out[2]), epochs=int(out[3]))

    def recycle_reset_counts(self):
        self._ck(self.lib.cpf_recycle_reset_counts(self.h))

    # -- patch source: dead slots respawn on weighted triangles (include/cpf.h "patch source")
    def set_source_triangles(self, tri, weights=None, depth=(0.0, 0.0)):
        """The source: triangles [m][3][3] (``PolyMesh.face_triangles`` gives a patch's), weights [m] (None: the areas;
        ``inflow_weights`` gives the flux-weighted ones) and the depth range, (d0, d1) for all or [m][2]; no triangle clears it."""
        t, w, dep, d0, d1 = _source_args(tri, weights, depth)
        self._ck(self.lib.cpf_set_source_triangles(self.h, _ptr(t) if t.size else None, _ptr(w), _ptr(dep), d0, d1, t.shape[0]))

    def source_follow(self, cells, depth_scale: float = 0.0):
        """The source's bounds -- and, with ``depth_scale`` > 0 (seconds: dt * cycles between respawns), its slab depths -- follow
        the velocity from now on: every ``set_velocity`` / ``set_velocity_dev`` ends with a refresh on the device (include/cpf.h
        "flux table").  ``cells``: the owner cell of every triangle of ``set_source_triangles``, ``mesh.owner[face_of_tri]``."""
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1)
        self._ck(self.lib.cpf_source_follow(self.h, _ptr(c) if c.size else None, c.size, float(depth_scale)))

    def source_unfollow(self):
        """Following off: the table stays as last refreshed."""
        self._ck(self.lib.cpf_source_unfollow(self.h))

    def source_refresh(self):
        """One refresh of the followed table from the current field, asynchronous on the context's stream."""
        self._ck(self.lib.cpf_source_refresh(self.h))

    def source_follow_counts(self):
        """dict(on, refreshes, skipped): skipped counts the refreshes that found no inflow and left the table alone."""
        out = np.zeros(3, np.int64)
        self._ck(self.lib.cpf_get_source_follow(self.h, _ptr(out)))
        return dict(on=bool(out[0]), refreshes=int(out[1]), skipped=int(out[2]))

    def source_table(self):
        """(rec [k][16], hi [k] uint32) of the source (cpf_source_table_host's layout): as built, or, while it follows U, the
        device's current one; k == 0 without a source."""
        k = C.c_int64(0)
        self._ck(self.lib.cpf_get_source_table(self.h, None, None, C.byref(k)))
        rec, hi = np.empty((k.value, 16), np.float64), np.empty(k.value, np.uint32)
        if k.value:
            self._ck(self.lib.cpf_get_source_table(self.h, _ptr(rec), _ptr(hi), C.byref(k)))
        return rec, hi

    def respawn_source(self, max_count: int = -1):
        """Up to ``max_count`` (< 0: all) dead slots of the context-owned cloud, in array order, get a fresh position on the source
        and are located; the cloud's epoch counter -- ``respawn_box``'s -- goes up by one."""
        self._ck(self.lib.cpf_respawn_source(self.h, int(max_count)))

    def respawn_source_dev(self, x, y, z, cell, gid, n, max_count: int = -1, epoch: int = 0):
        self._ck(self.lib.cpf_respawn_source_dev(self.h, x, y, z, cell, gid, n, int(max_count), int(epoch)))

    # -- tracer age: residence times at the sink, the mean-age field (include/cpf.h "tracer age")
    def age_enable(self, bin_cycles: int, n_bins: int):
        """Turns age tracking of the context-owned cloud on (or starts it anew): everybody is born now; ``n_bins`` residence-time
        bins of ``bin_cycles`` cycles, the last one open-ended."""
        self._ck(self.lib.cpf_age_enable(self.h, int(bin_cycles), int(n_bins)))
        self._age_bins = (int(bin_cycles), int(n_bins))

    def age_disable(self):
        self._ck(self.lib.cpf_age_disable(self.h))

    def age_sample(self):
        """One sample of the age field: every live particle adds its age to its cell's sum and 1 to its count; asynchronous."""
        self._ck(self.lib.cpf_age_sample(self.h))

    def age_reset(self):
        """Zeroes the histogram and the field; the birth stamps stay."""
        self._ck(self.lib.cpf_age_reset(self.h))

    def age_histogram(self) -> np.ndarray:
        """uint64 [n_bins]: absorptions since the last reset by age // bin_cycles; synchronises."""
        n_bins = getattr(self, "_age_bins", (1, 1))[1]
        bins = np.zeros(n_bins, np.uint64)
        self._ck(self.lib.cpf_get_age_histogram(self.h, _ptr(bins), n_bins))
        return bins

    def age_field(self):
        """(age_sum uint64 [n_cells], count uint64 [n_cells], n_samples) per parent cell since the last reset; synchronises."""
        s, c = np.zeros(self.n_cells, np.uint64), np.zeros(self.n_cells, np.uint64)
        ns = C.c_int64(0)
        self._ck(self.lib.cpf_get_age_field(self.h, _ptr(s), _ptr(c), C.byref(ns)))
        return s, c, ns.value

    def ages(self) -> np.ndarray:
        """int64 [n] in particle-id order: age in cycles, -1 for a dead slot; synchronises."""
        a = np.empty(self.n, np.int64)
        self._ck(self.lib.cpf_get_ages(self.h, _ptr(a)))
        return a

    def age_births(self) -> np.ndarray:
        """uint32 [n] in particle-id order: the cycle count at which each particle last became live."""
        b = np.empty(self.n, np.uint32)
        self._ck(self.lib.cpf_age_get_births(self.h, _ptr(b)))
        return b

    def age_set_births(self, births):
        b = np.ascontiguousarray(births, dtype=np.uint32).reshape(-1)
        if b.size != self.n:
            raise ValueError("age_set_births: %d stamps for %d particles" % (b.size, self.n))
        self._ck(self.lib.cpf_age_set_births(self.h, _ptr(b)))

    def rtd(self, dt: float):
        """Residence-time distribution at the sink: (edges in seconds [n_bins + 1], counts uint64 [n_bins]); the last bin is
        open-ended (its upper edge is inf)."""
        counts = self.age_histogram()
        bin_cycles, n_bins = self._age_bins
        edges = np.arange(n_bins + 1, dtype=np.float64) * (bin_cycles * float(dt))
        edges[-1] = np.inf
        return edges, counts

    def mean_age(self, dt: float) -> np.ndarray:
        """Mean age in seconds of the particles found in every cell over the samples taken: age_sum / count * dt, NaN where no
        particle was found."""
        s, c, _ = self.age_field()
        out = np.full(s.size, np.nan)
        np.divide(s.astype(np.float64), c.astype(np.float64), out=out, where=c > 0)
        return out * float(dt)

    # -- tracer tags: origin per particle, grouped sinks, the transfer matrix (include/cpf.h "tracer tags")
    def tag_enable(self, n_origins: int = 1, n_sinks: int = 1):
        """Turns tagging of the context-owned cloud on (or starts it anew): everybody has origin 0, every sink cell is in group 0,
        the source and the box give origin 0; ``n_origins`` and ``n_sinks`` are each in [1, 16]."""
        self._ck(self.lib.cpf_tag_enable(self.h, int(n_origins), int(n_sinks)))
        self._tag_shape = (int(n_origins), int(n_sinks))

    def tag_disable(self):
        self._ck(self.lib.cpf_tag_disable(self.h))

    def set_sink_groups(self, cells, groups):
        """``set_sink_cells(cells)``, with cell ``cells[k]`` in sink group ``groups[k]``."""
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1)
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if c.size != g.size:
            raise ValueError("set_sink_groups: %d groups for %d cells" % (g.size, c.size))
        self._ck(self.lib.cpf_set_sink_groups(self.h, _ptr(c) if c.size else None, _ptr(g) if g.size else None, c.size))

    def set_source_origins(self, origin_of_triangle):
        """One origin per triangle of ``set_source_triangles``, in the caller's order (dropped triangles included)."""
        o = np.ascontiguousarray(origin_of_triangle, dtype=np.int32).reshape(-1)
        self._ck(self.lib.cpf_set_source_origins(self.h, _ptr(o) if o.size else None, o.size))

    def set_box_origin(self, origin: int):
        self._ck(self.lib.cpf_set_box_origin(self.h, int(origin)))

    def tag_sample(self):
        """One sample of the per-origin occupancy: every live particle adds 1 to (its cell, its origin); asynchronous."""
        self._ck(self.lib.cpf_tag_sample(self.h))

    def tag_reset(self):
        """Zeroes the transfer matrix, the field and the sample count; the origins stay."""
        self._ck(self.lib.cpf_tag_reset(self.h))

    def tag_origins(self) -> np.ndarray:
        """uint8 [n] in particle-id order: the origin of the respawn that last made each particle live (0: the initial cloud)."""
        o = np.empty(self.n, np.uint8)
        self._ck(self.lib.cpf_tag_get_origins(self.h, _ptr(o)))
        return o

    def tag_set_origins(self, origins):
        o = np.ascontiguousarray(origins, dtype=np.uint8).reshape(-1)
        if o.size != self.n:
            raise ValueError("tag_set_origins: %d origins for %d particles" % (o.size, self.n))
        self._ck(self.lib.cpf_tag_set_origins(self.h, _ptr(o)))

    def transfer(self) -> np.ndarray:
        """uint64 [n_origins][n_sinks]: absorptions since the last reset by (origin, sink group); synchronises."""
        t = np.zeros(getattr(self, "_tag_shape", (1, 1)), np.uint64)
        self._ck(self.lib.cpf_get_transfer(self.h, _ptr(t)))
        return t

    def tag_field(self):
        """(counts uint64 [n_origins][n_cells], n_samples) per parent cell since the last reset; synchronises."""
        n_origins = getattr(self, "_tag_shape", (1, 1))[0]
        c = np.zeros((self.n_cells, n_origins), np.uint64)
        ns = C.c_int64(0)
        self._ck(self.lib.cpf_get_tag_field(self.h, _ptr(c), C.byref(ns)))
        return np.ascontiguousarray(c.T), ns.value

    def origin_concentration(self) -> np.ndarray:
        """[n_origins][n_cells]: time-averaged particles of each origin per unit volume, counts / (n_samples * V)."""
        counts, ns = self.tag_field()
        if ns == 0:
            raise ValueError("origin_concentration: no tag sample yet (tag_sample)")
        return counts.astype(np.float64) / (float(ns) * self.cell_volumes()[None, :])

    def origin_fraction(self) -> np.ndarray:
        """[n_origins][n_cells]: each origin's share of the particles found in a cell over the samples taken; NaN where none was."""
        counts, _ = self.tag_field()
        c = counts.astype(np.float64)
        total = c.sum(axis=0)
        out = np.full(c.shape, np.nan)
        np.divide(c, total[None, :], out=out, where=(total > 0)[None, :])
        return out

    # -- routes: the residence time per origin and sink group (include/cpf.h "routes")
    def route_enable(self):
        """Turns routes on (or starts them anew); needs ``age_enable`` and ``tag_enable``.  ``sink_apply`` then runs one pass for
        the transfer matrix, the age histogram and the histogram per route."""
        self._ck(self.lib.cpf_route_enable(self.h))

    def route_disable(self):
        self._ck(self.lib.cpf_route_disable(self.h))

    def route_sample(self):
        """One sample of the age field per origin: every live particle adds its age and 1 to (its cell, its origin); asynchronous."""
        self._ck(self.lib.cpf_route_sample(self.h))

    def route_reset(self):
        """Zeroes the route histogram, the route field and their sample count, and nothing of age or tags."""
        self._ck(self.lib.cpf_route_reset(self.h))

    def route_histogram(self) -> np.ndarray:
        """uint64 [n_origins][n_sinks][n_bins]: absorptions since the last reset by route and age // bin_cycles; synchronises."""
        n_bins = getattr(self, "_age_bins", (1, 1))[1]
        h = np.zeros(getattr(self, "_tag_shape", (1, 1)) + (n_bins,), np.uint64)
        self._ck(self.lib.cpf_get_route_histogram(self.h, _ptr(h)))
        return h

    def route_field(self):
        """(age_sum uint64 [n_cells][n_origins], count uint64 [n_cells][n_origins], n_samples) per parent cell since the last
        reset; synchronises."""
        n_origins = getattr(self, "_tag_shape", (1, 1))[0]
        s, c = np.zeros((self.n_cells, n_origins), np.uint64), np.zeros((self.n_cells, n_origins), np.uint64)
        ns = C.c_int64(0)
        self._ck(self.lib.cpf_get_route_field(self.h, _ptr(s), _ptr(c), C.byref(ns)))
        return s, c, ns.value

    def rtd_by_route(self, dt: float):
        """Residence-time distribution per route: (edges in seconds [n_bins + 1], counts uint64 [n_origins][n_sinks][n_bins]);
        the edges are ``rtd``'s."""
        counts = self.route_histogram()
        bin_cycles, n_bins = self._age_bins
        edges = np.arange(n_bins + 1, dtype=np.float64) * (bin_cycles * float(dt))
        edges[-1] = np.inf
        return edges, counts

    def mean_age_by_origin(self, dt: float) -> np.ndarray:
        """[n_cells][n_origins]: mean age in seconds of the particles of each origin found in a cell over the samples taken, NaN
        where none was."""
        s, c, _ = self.route_field()
        out = np.full(s.shape, np.nan)
        np.divide(s.astype(np.float64), c.astype(np.float64), out=out, where=c > 0)
        return out * float(dt)

    # -- exposure: a dose per particle summed along its path, the dose histogram at the sink (include/cpf.h "exposure")
    def exposure_enable(self, bin_width: float, n_bins: int = 1):
        """Turns exposure of the context-owned cloud on (or starts it anew): every dose is 0, the rate field all zero; ``n_bins``
        dose bins of ``bin_width``, the last one open-ended, per (origin, sink group) if tagging is on at this moment."""
        self._ck(self.lib.cpf_exposure_enable(self.h, float(bin_width), int(n_bins)))
        self._dose_bins = (float(bin_width), int(n_bins), getattr(self, "_tag_shape", (1, 1)) if self._tags_on() else (1, 1))

    def _tags_on(self) -> bool:
        """Whether tagging is on in the library right now: a new cloud or mesh turns it off behind ``_tag_shape``'s back, and
        the read-back of the transfer matrix (room for 16 x 16) answers if and only if it is on."""
        t = np.zeros(256, np.uint64)
        return self.lib.cpf_get_transfer(self.h, _ptr(t)) == L.CPF_OK

    def exposure_disable(self):
        self._ck(self.lib.cpf_exposure_disable(self.h))

    def set_exposure_field(self, rate):
        """One rate per cell of the mesh as given, finite and >= 0: what a particle in that cell accumulates per unit of
        ``exposure_accumulate``'s scale."""
        r = np.ascontiguousarray(rate, dtype=np.float64).reshape(-1)
        self._ck(self.lib.cpf_set_exposure_field(self.h, _ptr(r) if r.size else None, r.size))

    def exposure_accumulate(self, scale: float):
        """dose += scale * rate[cell] for every live particle; asynchronous."""
        self._ck(self.lib.cpf_exposure_accumulate(self.h, float(scale)))

    def exposure_reset(self):
        """Zeroes the dose histogram; the doses stay."""
        self._ck(self.lib.cpf_exposure_reset(self.h))

    def dose_histogram(self) -> np.ndarray:
        """uint64 [n_origins][n_sinks][n_bins]: absorptions since the last reset by origin, sink group and dose bin; synchronises."""
        _, n_bins, shape = getattr(self, "_dose_bins", (1.0, 1, (1, 1)))
        h = np.zeros(tuple(shape) + (n_bins,), np.uint64)
        self._ck(self.lib.cpf_get_dose_histogram(self.h, _ptr(h)))
        return h

    def doses(self) -> np.ndarray:
        """float64 [n] in particle-id order: the dose, -1 for a dead slot; synchronises."""
        d = np.empty(self.n, np.float64)
        self._ck(self.lib.cpf_get_doses(self.h, _ptr(d)))
        return d

    def exposure_doses(self) -> np.ndarray:
        """float64 [n] in particle-id order: the dose table itself, dead slots included (checkpoints)."""
        d = np.empty(self.n, np.float64)
        self._ck(self.lib.cpf_exposure_get_doses(self.h, _ptr(d)))
        return d

    def exposure_set_doses(self, doses):
        d = np.ascontiguousarray(doses, dtype=np.float64).reshape(-1)
        if d.size != self.n:
            raise ValueError("exposure_set_doses: %d doses for %d particles" % (d.size, self.n))
        self._ck(self.lib.cpf_exposure_set_doses(self.h, _ptr(d)))

    def dose_distribution(self):
        """Dose distribution at the sink: (edges [n_bins + 1], counts uint64 [n_origins][n_sinks][n_bins]); the last bin is
        open-ended (its upper edge is inf)."""
        counts = self.dose_histogram()
        bin_width, n_bins, _ = self._dose_bins
        edges = np.arange(n_bins + 1, dtype=np.float64) * bin_width
        edges[-1] = np.inf
        return edges, counts

    # -- zones: the zone of every particle at the last sample, the zone-to-zone transition counts (include/cpf.h "zones")
    def zone_enable(self, n_zones: int):
        """Turns zones of the context-owned cloud on (or starts them anew): every particle is outside, the map all 0, the table
        zeroed; ``1 <= n_zones <= 63``."""
        self._ck(self.lib.cpf_zone_enable(self.h, int(n_zones)))
        self._n_zones = int(n_zones)

    def zone_disable(self):
        self._ck(self.lib.cpf_zone_disable(self.h))

    def set_zone_map(self, zone):
        """One zone in [0, n_zones) per cell of the mesh as given."""
        z = np.ascontiguousarray(zone, dtype=np.int32).reshape(-1)
        self._ck(self.lib.cpf_set_zone_map(self.h, _ptr(z) if z.size else None, z.size))

    def zone_sample(self):
        """flow[last zone][zone now] += 1 for every live particle, and the zone now becomes its last; asynchronous."""
        self._ck(self.lib.cpf_zone_sample(self.h))

    def zone_reset(self):
        """Zeroes the table and the sample count; the last zones and the map stay."""
        self._ck(self.lib.cpf_zone_reset(self.h))

    def zone_flows(self):
        """(F uint64 [n_zones + 1][n_zones + 1], n_samples) since the last reset: F[p][z] transitions from zone p at one sample
        to zone z at the next; index n_zones is "outside" (row: first seen, column: absorbed); synchronises."""
        k = getattr(self, "_n_zones", 1) + 1
        f = np.zeros((k, k), np.uint64)
        ns = C.c_int64(0)
        self._ck(self.lib.cpf_get_zone_flows(self.h, _ptr(f), C.byref(ns)))
        return f, ns.value

    def zone_last(self) -> np.ndarray:
        """uint8 [n] in particle-id order: the zone at the last sample, 0xFF for outside (checkpoints)."""
        a = np.empty(self.n, np.uint8)
        self._ck(self.lib.cpf_zone_get_last(self.h, _ptr(a)))
        return a

    def zone_set_last(self, last):
        a = np.ascontiguousarray(last, dtype=np.uint8).reshape(-1)
        if a.size != self.n:
            raise ValueError("zone_set_last: %d bytes for %d particles" % (a.size, self.n))
        self._ck(self.lib.cpf_zone_set_last(self.h, _ptr(a)))

    def zone_exchange_rates(self, sample_dt: float) -> np.ndarray:
        """[n_zones + 1][n_zones + 1] particles per second from zone p to zone z over the samples taken, ``sample_dt`` apart: the
        off-diagonal of F / (n_samples * sample_dt), the diagonal 0; NaN without a sample."""
        f, ns = self.zone_flows()
        return zone_exchange_rates(f, ns, sample_dt)

    def zone_residence(self, sample_dt: float) -> np.ndarray:
        """[n_zones] mean time of a visit to each zone in seconds: the samples found in it over the entries into it, NaN where
        nobody entered."""
        return zone_residence(self.zone_flows()[0], sample_dt)

    # -- the sink log: one record per absorbed particle, appended on the device (include/cpf.h "sink log")
    def sink_log_enable(self, capacity: int):
        """Turns the sink log of the context-owned cloud on (or starts it anew) with room for ``capacity`` records: from now on
        every ``sink_apply`` first appends one ``SINK_LOG_DTYPE`` record per particle it is about to absorb."""
        self._ck(self.lib.cpf_sink_log_enable(self.h, int(capacity)))

    def sink_log_disable(self):
        self._ck(self.lib.cpf_sink_log_disable(self.h))

    def sink_log_counts(self):
        """(stored, dropped): the records held, and the absorbed particles that found the buffer full; synchronises."""
        stored, dropped = C.c_int64(), C.c_int64()
        self._ck(self.lib.cpf_sink_log_counts(self.h, C.byref(stored), C.byref(dropped)))
        return stored.value, dropped.value

    def sink_log_read(self, max_records: Optional[int] = None) -> np.ndarray:
        """The stored records sorted by (apply, id), all of them or the first ``max_records``; the log stays as it is;
        synchronises."""
        room = self.sink_log_counts()[0] if max_records is None else int(max_records)
        rec = np.zeros(max(room, 0), SINK_LOG_DTYPE)
        got = C.c_int64()
        self._ck(self.lib.cpf_sink_log_read(self.h, _ptr(rec) if rec.size else None, room, C.byref(got)))
        return rec[:got.value]

    def sink_log_clear(self):
        """Forgets the records (and the dropped count); ``apply`` goes on counting.  Asynchronous."""
        self._ck(self.lib.cpf_sink_log_clear(self.h))

    def sink_log_drain(self) -> np.ndarray:
        """``sink_log_read()``, then ``sink_log_clear()``."""
        rec = self.sink_log_read()
        self.sink_log_clear()
        return rec

    def cell_ranges_dev(self, weights, n_ranks, cell_lo):
        self._ck(self.lib.cpf_cell_ranges_dev(self.h, weights, n_ranks, cell_lo))

    def unpack_arrivals_dev(self, x, y, z, cell, gid, n_stay, recvbuf, n_recv):
        self._ck(self.lib.cpf_unpack_arrivals_dev(self.h, x, y, z, cell, gid, n_stay, recvbuf, n_recv))

    def write_vtu(self, path: str) -> float:
        """particle_%04d.vtu in the reference's layout, synchronously; returns the total kinetic energy."""
        ke = C.c_double()
        r = self.lib.cpf_write_vtu(self.h, str(path).encode(), C.byref(ke))
        if r not in (L.CPF_OK, L.CPF_WARN_NAN):
            self._ck(r)
        return ke.value

    def write_vtu_async(self, path: str, want_ke: bool = True):
        """Same frame behind the caller's back: a device-side snapshot (one kernel), then copy, energy sum, formatting and file
        I/O on a worker thread (one frame in flight per context).  want_ke=False: returns None at once -- the step loop is not
        held up by PCIe; True: waits for the copy and returns the total kinetic energy."""
        ke = C.c_double()
        r = self.lib.cpf_write_vtu_async(self.h, str(path).encode(), C.byref(ke) if want_ke else None)
        if r not in (L.CPF_OK, L.CPF_WARN_NAN):
            self._ck(r)
        return ke.value if want_ke else None

    def write_vtu_wait(self):
        r = self.lib.cpf_write_vtu_wait(self.h)
        if r not in (L.CPF_OK, L.CPF_WARN_NAN):
            self._ck(r)

    def timing_enable(self, on: bool = True):
        self._ck(self.lib.cpf_timing_enable(self.h, int(on)))

    def timing_read(self):
        a, b = C.c_int64(), C.c_double()
        self._ck(self.lib.cpf_timing_read(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timing_poll(self):
        """Like timing_read but never waits: only launches that already finished are drained."""
        a, b = C.c_int64(), C.c_double()
        self._ck(self.lib.cpf_timing_poll(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def respawn_positions_host(seed: int, gid, epoch: int, lower, upper, n: Optional[int] = None) -> np.ndarray:
    """Where ``respawn_box`` puts the particles ``gid`` (None: 0 .. n-1) at ``epoch`` under ``seed``: [n][3], computed on the host
    alone from the kernel's own text (cpf_respawn_positions_host)."""
    lib = L.load()
    g = None if gid is None else np.ascontiguousarray(gid, dtype=np.int64).reshape(-1)
    n = int(n) if g is None else g.size
    lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
    xyz = np.empty((n, 3), np.float64)
    st = lib.cpf_respawn_positions_host(seed & 0xFFFFFFFF, _ptr(g), n, int(epoch) & 0xFFFFFFFF, _ptr(lo), _ptr(hi), _ptr(xyz))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_respawn_positions_host")
    return xyz


def _source_args(tri, weights, depth):
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and w.size != t.shape[0]:
        raise ValueError("source: %d weights for %d triangles" % (w.size, t.shape[0]))
    d = np.ascontiguousarray(depth, dtype=np.float64)
    if d.shape == (2,):
        return t, w, None, float(d[0]), float(d[1])
    if d.shape != (t.shape[0], 2):
        raise ValueError("source: depth is (d0, d1) or [m][2]")
    return t, w, d, 0.0, 0.0


def source_table_host(tri, weights=None, depth=(0.0, 0.0)):
    """The table ``Context.set_source_triangles`` would build and upload, on the host alone (cpf_source_table_host): (rec [k][16],
    hi [k] uint32) of the k triangles kept; rec[:, 14] is their index in ``tri``."""
    lib = L.load()
    t, w, dep, d0, d1 = _source_args(tri, weights, depth)
    m = t.shape[0]
    rec, hi, k = np.empty((m, 16), np.float64), np.empty(m, np.uint32), C.c_int64(0)
    st = lib.cpf_source_table_host(_ptr(t) if m else None, _ptr(w), _ptr(dep), d0, d1, m, _ptr(rec), _ptr(hi), C.byref(k))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_source_table_host")
    return rec[:k.value].copy(), hi[:k.value].copy()


def source_flux_host(rec, cells, U, depth_scale: float = 0.0):
    """The flux-table rule on the host alone (cpf_source_flux_host; include/cpf.h "flux table"): what a refresh makes of the table
    ``rec`` [k][16] under the field ``U`` [nCells][3], ``cells`` the owner cell per input triangle.  Returns (span [k], hi [k] uint32,
    q [k] uint64, empty); with ``empty`` (no inflow anywhere) a refresh changes nothing and the three arrays are all 0."""
    lib = L.load()
    r = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 16)
    c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1)
    u = np.ascontiguousarray(U, dtype=np.float64).reshape(-1, 3)
    k = r.shape[0]
    span, hi, q, empty = np.zeros(k, np.float64), np.zeros(k, np.uint32), np.zeros(k, np.uint64), C.c_int32(0)
    st = lib.cpf_source_flux_host(_ptr(r) if k else None, k, _ptr(c) if c.size else None, c.size, _ptr(u) if u.size else None,
                                  u.shape[0], float(depth_scale), _ptr(span), _ptr(hi), _ptr(q), C.byref(empty))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_source_flux_host")
    return span, hi, q, bool(empty.value)


def source_positions_host(seed: int, gid, epoch: int, rec, hi, n: Optional[int] = None) -> np.ndarray:
    """Where ``respawn_source`` puts the particles ``gid`` (None: 0 .. n-1) at ``epoch`` under ``seed`` on the table (rec, hi):
    [n][3], computed on the host alone from the kernel's own text (cpf_source_positions_host)."""
    lib = L.load()
    g = None if gid is None else np.ascontiguousarray(gid, dtype=np.int64).reshape(-1)
    n = int(n) if g is None else g.size
    r = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 16)
    h = np.ascontiguousarray(hi, dtype=np.uint32).reshape(-1)
    xyz = np.empty((n, 3), np.float64)
    st = lib.cpf_source_positions_host(seed & 0xFFFFFFFF, _ptr(g), n, int(epoch) & 0xFFFFFFFF, _ptr(r), _ptr(h), h.size, _ptr(xyz))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_source_positions_host")
    return xyz


def source_picks_host(seed: int, gid, epoch: int, hi, n: Optional[int] = None) -> np.ndarray:
    """Which kept record of the table's bounds ``hi`` ``respawn_source`` picks for the particles ``gid`` (None: 0 .. n-1) at
    ``epoch`` under ``seed``: int32 [n], computed on the host alone from the kernels' own text (cpf_source_picks_host)."""
    lib = L.load()
    g = None if gid is None else np.ascontiguousarray(gid, dtype=np.int64).reshape(-1)
    n = int(n) if g is None else g.size
    h = np.ascontiguousarray(hi, dtype=np.uint32).reshape(-1)
    pick = np.empty(n, np.int32)
    st = lib.cpf_source_picks_host(seed & 0xFFFFFFFF, _ptr(g), n, int(epoch) & 0xFFFFFFFF, _ptr(h), h.size, _ptr(pick))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_source_picks_host")
    return pick


def inflow_weights(mesh, U, tri, face_of_tri) -> np.ndarray:
    """Flux weights of the triangles of ``mesh.face_triangles``: area * max(0, -U_owner . n_out), n_out the triangle's right-hand
    unit normal (outward on a boundary face) and U_owner the velocity of the face's owner cell."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    c = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = np.sqrt((c * c).sum(1))
    n_out = c / np.where(length > 0, length, 1.0)[:, None]
    u = np.asarray(U, dtype=np.float64)[np.asarray(mesh.owner)[np.asarray(face_of_tri, dtype=np.int64)]]
    return 0.5 * length * np.maximum(0.0, -(u * n_out).sum(1))


def build_mesh_tables_host(mesh):
    """What ``Context.set_mesh(mesh)`` would build and upload, computed on the host alone (no GPU, no context): a dict with
    cell_off, planes (n_slots, 4), nbr, group_off, group_nbr -- one slot per distinct plane of a cell, face groups for the
    coplanar pieces of a split face (``include/cpf.h``: cpf_build_mesh_tables_host)."""
    lib = L.load()
    a = [np.ascontiguousarray(mesh.points, dtype=np.float64), np.ascontiguousarray(mesh.face_offsets, dtype=np.int32),
         np.ascontiguousarray(mesh.face_verts, dtype=np.int32), np.ascontiguousarray(mesh.owner, dtype=np.int32),
         np.ascontiguousarray(mesh.neighbour, dtype=np.int32)]
    ns, ng, nm = C.c_int64(0), C.c_int64(0), C.c_int64(0)

    def call(*out):
        st = lib.cpf_build_mesh_tables_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                            mesh.n_internal, mesh.n_cells, C.byref(ns), C.byref(ng), C.byref(nm), *out)
        if st != L.CPF_OK:
            raise L.CpfError(st, "cpf_build_mesh_tables_host")
    call(None, None, None, None, None)
    off = np.empty(mesh.n_cells + 1, np.int32); planes = np.empty((ns.value, 4), np.float64); nbr = np.empty(ns.value, np.int32)
    goff = np.empty(ng.value + 1, np.int32); gnbr = np.empty(max(nm.value, 1), np.int32)
    call(_ptr(off), _ptr(planes), _ptr(nbr), _ptr(goff), _ptr(gnbr))
    return dict(cell_off=off, planes=planes, nbr=nbr, group_off=goff, group_nbr=gnbr[:nm.value])


def mesh_flags_host(mesh):
    """What ``Context.mesh_flags()`` would report after ``set_mesh(mesh)``, computed on the host alone (cpf_mesh_flags_host)."""
    lib = L.load()
    a = [np.ascontiguousarray(mesh.points, dtype=np.float64), np.ascontiguousarray(mesh.face_offsets, dtype=np.int32),
         np.ascontiguousarray(mesh.face_verts, dtype=np.int32), np.ascontiguousarray(mesh.owner, dtype=np.int32),
         np.ascontiguousarray(mesh.neighbour, dtype=np.int32)]
    v = [C.c_int32(0) for _ in range(4)]
    st = lib.cpf_mesh_flags_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                 mesh.n_internal, mesh.n_cells, *[C.byref(k) for k in v])
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_mesh_flags_host")
    return dict(all_hex=v[0].value, z_layered=v[1].value, z_thin=v[2].value, mixed=v[3].value)


def mesh_box_records_host(mesh):
    """The mesh's box records ([n_cells, 16] float64; ``cpf_mesh_box_records_host``), or None if some cell is not an axis-aligned
    box.  Layout: csrc/cpf_walk.h "box records"."""
    lib = L.load()
    a = [np.ascontiguousarray(mesh.points, dtype=np.float64), np.ascontiguousarray(mesh.face_offsets, dtype=np.int32),
         np.ascontiguousarray(mesh.face_verts, dtype=np.int32), np.ascontiguousarray(mesh.owner, dtype=np.int32),
         np.ascontiguousarray(mesh.neighbour, dtype=np.int32)]
    is_box = C.c_int32(0)
    rec = np.zeros((mesh.n_cells, 16), np.float64)
    st = lib.cpf_mesh_box_records_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                       mesh.n_internal, mesh.n_cells, C.byref(is_box), _ptr(rec))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_mesh_box_records_host")
    return rec if is_box.value else None


def _quality_dict(q):
    return dict(max_eta=q.maxNonPlanarity, worst_face=q.worstFace, max_xi=q.maxNonConvexity, worst_cell=q.worstCell,
                n_cells=q.nCells, n_flagged=q.nFlaggedCells, n_bad=q.nBadCells, n_derived=q.nDerivedCells, tol=q.tol)


def _mesh_args(mesh):
    return [np.ascontiguousarray(mesh.points, dtype=np.float64), np.ascontiguousarray(mesh.face_offsets, dtype=np.int32),
            np.ascontiguousarray(mesh.face_verts, dtype=np.int32), np.ascontiguousarray(mesh.owner, dtype=np.int32),
            np.ascontiguousarray(mesh.neighbour, dtype=np.int32)]


def mesh_quality_host(mesh, tol: float = L.NONPLANAR_TOL, split: bool = True):
    """What ``Context.mesh_quality()`` would report after ``set_mesh(mesh)`` with option "nonplanar_tol" = tol (and
    "split_nonplanar" = split), on the host alone (cpf_mesh_quality_host)."""
    lib = L.load()
    a = _mesh_args(mesh)
    q = L.MeshQuality()
    st = lib.cpf_mesh_quality_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                   mesh.n_internal, mesh.n_cells, float(tol), 1 if split else 0, C.byref(q))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_mesh_quality_host")
    return _quality_dict(q)


def cell_volumes_host(mesh) -> np.ndarray:
    """What ``Context.cell_volumes()`` would return after ``set_mesh(mesh)``, on the host alone (cpf_cell_volumes_host)."""
    lib = L.load()
    a = _mesh_args(mesh)
    V = np.empty(mesh.n_cells, np.float64)
    st = lib.cpf_cell_volumes_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                   mesh.n_internal, mesh.n_cells, _ptr(V))
    if st != L.CPF_OK:
        raise L.CpfError(st, "cpf_cell_volumes_host")
    return V


def build_derived_mesh_host(mesh, tol: float = L.NONPLANAR_TOL):
    """The mesh ``Context.set_mesh(mesh)`` walks (cpf_build_derived_mesh_host): (PolyMesh of the derived mesh, first
    [n_cells + 1] -- the derived cells of parent c are first[c] .. first[c+1] --, apex points [n_decomposed][3])."""
    from .cases.polymesh import PolyMesh
    lib = L.load()
    a = _mesh_args(mesh)
    sizes = np.zeros(5, np.int64)

    def call(*out):
        st = lib.cpf_build_derived_mesh_host(_ptr(a[0]), mesh.n_points, _ptr(a[1]), _ptr(a[2]), mesh.n_faces, _ptr(a[3]), _ptr(a[4]),
                                             mesh.n_internal, mesh.n_cells, float(tol), _ptr(sizes), *out)
        if st != L.CPF_OK:
            raise L.CpfError(st, "cpf_build_derived_mesh_host")
    call(None, None, None, None, None, None)
    n_p, n_f, n_v, n_i, n_c = (int(v) for v in sizes)
    pts = np.empty((n_p, 3)); fo = np.empty(n_f + 1, np.int32); fv = np.empty(n_v, np.int32)
    ow = np.empty(n_f, np.int32); ne = np.empty(max(n_i, 1), np.int32); first = np.empty(mesh.n_cells + 1, np.int32)
    call(_ptr(pts), _ptr(fo), _ptr(fv), _ptr(ow), _ptr(ne), _ptr(first))
    derived = PolyMesh(pts, fo, fv, ow, ne[:n_i].copy(), n_c)
    return derived, first, pts[mesh.n_points:].copy()


def pack_mesh_parts(parts):
    """(ctypes array of cpf_mesh_part, the numpy arrays it points into)."""
    arr = (L.MeshPart * len(parts))()
    keep = []
    for k, m in enumerate(parts):
        lab = np.int64 if np.asarray(m.owner).dtype == np.int64 else np.int32
        pts = np.ascontiguousarray(m.points, dtype=np.float64)
        fo = np.ascontiguousarray(m.face_offsets, dtype=lab); fv = np.ascontiguousarray(m.face_verts, dtype=lab)
        ow = np.ascontiguousarray(m.owner, dtype=lab); ne = np.ascontiguousarray(m.neighbour, dtype=lab)
        keep += [pts, fo, fv, ow, ne]
        arr[k] = L.MeshPart(pts.ctypes.data, pts.shape[0], fo.ctypes.data, fv.ctypes.data, ow.shape[0], ow.ctypes.data,
                            ne.ctypes.data if ne.size else None, ne.shape[0], int(m.n_cells), 8 if lab == np.int64 else 4)
    return arr, keep


def merge_mesh_parts(parts):
    """cpf_merge_mesh_parts on the host (no GPU): the stitched global mesh as a cases.PolyMesh (64-bit labels)."""
    from .cases.polymesh import PolyMesh
    lib = L.load()
    arr, keep = pack_mesh_parts(parts)
    h = C.c_void_p()
    r = lib.cpf_merge_mesh_parts(arr, len(parts), C.byref(h))
    if r != L.CPF_OK:
        raise L.CpfError(r, (lib.cpf_merge_last_error() or b"").decode())
    try:
        n = [C.c_int64() for _ in range(5)]
        lib.cpf_merged_mesh_sizes(h, *[C.byref(v) for v in n])
        n_points, n_faces, n_fv, n_int, n_cells = (v.value for v in n)
        pts = np.empty((n_points, 3)); fo = np.empty(n_faces + 1, np.int64); fv = np.empty(n_fv, np.int64)
        ow = np.empty(n_faces, np.int64); ne = np.empty(n_int, np.int64)
        lib.cpf_merged_mesh_copy(h, _ptr(pts), _ptr(fo), _ptr(fv), _ptr(ow), _ptr(ne))
    finally:
        lib.cpf_merged_mesh_free(h)
    return PolyMesh(points=pts, face_offsets=fo, face_verts=fv, owner=ow, neighbour=ne, n_cells=int(n_cells))


# ------------------------------------------------------------------------------------------------
# the fragments' call surface
# ------------------------------------------------------------------------------------------------
DICT_DEFAULTS = dict(                       # src/initCuda.H:49-57 (getOrDefault values)
    seedingBox=((0.0, 0.0, 0.0), (30.0, 30.0, 30.0)), numParticles=1000, startTime=0.0, endTime=1e05,
    dt=1e-4, diffusionCoeff=5.7e-6, saveInterval=10)


def zone_exchange_rates(flow, n_samples: int, sample_dt: float) -> np.ndarray:
    """``Context.zone_exchange_rates`` on a table: off-diagonal flow / (n_samples * sample_dt), the diagonal 0; plain numpy."""
    f = np.asarray(flow).astype(np.float64)
    rates = f / (float(n_samples) * float(sample_dt)) if n_samples > 0 else np.full(f.shape, np.nan)
    np.fill_diagonal(rates, 0.0)
    return rates


def zone_residence(flow, sample_dt: float) -> np.ndarray:
    """``Context.zone_residence`` on a table [k + 1][k + 1]: per zone z < k, sample_dt * colsum_z / (colsum_z - flow[z][z]) -- the
    samples that found a particle in z over those that found it there for the first time of a visit --, NaN where nobody
    entered; plain numpy."""
    f = np.asarray(flow).astype(np.float64)
    k = f.shape[0] - 1
    col = f.sum(axis=0)[:k]
    entered = col - np.diagonal(f)[:k]
    out = np.full(k, np.nan)
    np.divide(float(sample_dt) * col, entered, out=out, where=entered > 0)
    return out


def _next_chunk(step: int, remaining: int, save_interval: int, occupancy_interval: int, has_writer: bool,
                will_write: bool, recycle_interval: int = 0, *, exposure_interval: int = 0, zone_interval: int = 0) -> int:
    """Cycles the next launch of ``CudaParticles.advect`` fuses: a cycle that writes a frame runs alone; otherwise everything up
    to the next output point (with a writer), the next occupancy sample (``occupancy_interval`` > 0), the next recycle point
    (``recycle_interval`` > 0), the next exposure point (``exposure_interval`` > 0), the next zone point (``zone_interval`` > 0)
    and the end of the call."""
    if will_write:
        return 1
    chunk = remaining
    if has_writer:
        chunk = min(chunk, save_interval - (step % save_interval))
    if occupancy_interval > 0:
        chunk = min(chunk, occupancy_interval - (step % occupancy_interval))
    if recycle_interval > 0:
        chunk = min(chunk, recycle_interval - (step % recycle_interval))
    if exposure_interval > 0:
        chunk = min(chunk, exposure_interval - (step % exposure_interval))
    if zone_interval > 0:
        chunk = min(chunk, zone_interval - (step % zone_interval))
    return max(1, chunk)


class CudaParticles:
    """What ``initCuda.H`` sets up and ``advect.H`` advances, for one solver process.

    ``writer(step, xyzw, vel, cell)`` is called with the cadence of
    ``writeParticles2VTU`` (frame 0 at init, then ``step % saveInterval == 0`` or at
    ``endTime``, src/initCuda.H:201, src/advect.H:166-169).

    One dictionary key is this library's own, not the reference's: ``occupancyInterval`` (cycles; default 0 = off).  When
    positive, every cycle count that is a multiple of it adds one sample to the per-cell occupancy on the device
    (``Context.occupancy_sample``), and ``concentration()`` gives the time-averaged concentration field.

    Three more are this library's own as well: ``recycleInterval`` (cycles; default 0 = off), ``sinkCells`` (an array of cell ids;
    patch names are resolved by the caller, ``mesh.patch_cells("outlet")``) and ``sourceBox`` ((lower, upper); default: the
    ``seedingBox``).  When ``recycleInterval`` is positive, at every cycle count that is a multiple of it the particles found in a
    sink cell are absorbed (``Context.sink_apply``) and every dead slot is respawned in the source box
    (``Context.respawn_box``), before the occupancy sample if one is due: an inlet and an outlet at constant particle count.

    With ``sourceTriangles`` ([m][3][3]; ``mesh.face_triangles(mesh.patch_faces("inlet"))``) the dead slots are respawned on those
    triangles instead (``Context.respawn_source``) and ``sourceBox`` is unused: ``sourceWeights`` ([m]; default: the areas,
    ``inflow_weights`` gives the flux-weighted ones) chooses the triangle and ``sourceDepth`` ((d0, d1) or [m][2]; default 0)
    is the range of depths behind it.  Those weights are fixed.  With ``sourceFollowU`` (default false; it needs
    ``recycleInterval`` > 0, ``sourceTriangles`` and ``sourceCells``, one owner cell per triangle, ``mesh.owner[face_of_tri]``, and
    excludes ``sourceWeights``) the table is built with the areas and then follows the velocity: every ``advect(U=...)`` recomputes
    the flux weights on the device (``Context.source_follow``), and with ``sourceDepthScale`` (seconds, default 0: the user's
    dt * recycleInterval) the depth behind each triangle becomes (U . n_in) * sourceDepthScale as well.

    Two more, also this library's own: ``ageBins`` (default 0 = off) and ``ageBinCycles`` (default: ``recycleInterval``, else 1).
    When ``ageBins`` is positive, age tracking (``Context.age_enable``) starts once the cloud is located: every absorption adds a
    residence time to ``rtd()``, and wherever an occupancy sample is taken the age field is sampled too, after recycling, for
    ``mean_age()``.

    Two more: ``sinkGroups`` (one int per entry of ``sinkCells``) and ``sourceOrigins`` (one int per triangle of
    ``sourceTriangles``).  Tagging (``Context.tag_enable``) is on if and only if one of them is given, with max + 1 sink groups and
    origins (1 where the key is absent), once the cloud is located: every absorption adds to ``transfer()[origin, group]``, and
    wherever an occupancy sample is taken the per-origin field is sampled too, for ``origin_fraction()``.  The initial cloud has
    origin 0, so number real sources from 1 to tell it apart.

    One more: ``routeStats`` (default false), which needs ``ageBins`` > 0 and tagging.  Routes (``Context.route_enable``) then start
    behind age tracking and tagging: every absorption also adds to ``rtd_by_route()``, and wherever the age field is sampled the
    age field per origin is sampled too, for ``mean_age_by_origin()``.

    Four more: ``exposureField`` (one rate per cell, per second, finite and >= 0; default None = off), ``exposureInterval`` (cycles;
    default 1), ``doseBins`` (default 1) and ``doseBinWidth`` (needed when ``doseBins`` > 1).  With a field, exposure
    (``Context.exposure_enable``) starts behind age tracking, tagging and routes: at every cycle count that is a multiple of
    ``exposureInterval`` every live particle adds (the time since the last such point) x (the rate of the cell it is in) to its
    dose, before the recycle point's absorption if one is due; every absorption adds to ``dose_distribution()``, and a respawned
    particle starts from 0.

    Two more: ``zoneMap`` (one non-negative int per cell; default None = off; max + 1 zones, 63 at most) and ``zoneInterval``
    (cycles; default 1).  With a map, zones (``Context.zone_enable``) start behind exposure: at every cycle count that is a
    multiple of ``zoneInterval`` every live particle adds one to ``zone_flows()[0][its zone at the last such point][its zone
    now]``, before the recycle point's absorption if one is due, so the absorbed leave from the zone they are in;
    ``zone_residence()`` is the mean time of a visit per zone.

    One more: ``sinkLog`` (a capacity in records; default 0 = off), which needs ``recycleInterval`` > 0 and ``sinkCells``.  The
    sink log (``Context.sink_log_enable``) then starts behind zones: every absorption appends one ``SINK_LOG_DTYPE`` record --
    id, cycle, exit point, age, origin, sink group, dose and zone, as far as those groups are on.  ``sink_log()`` drains it;
    nothing else does, and what finds the log full is counted as dropped.
    """

    def __init__(self, mesh, U, particle_dict: Optional[dict] = None, device: int = 0,
                 writer: Optional[Callable] = None, positions: Optional[np.ndarray] = None, seed_order: int = 1):
        d = dict(DICT_DEFAULTS)
        d.update(particle_dict or {})
        self.numParticles = int(d["numParticles"])
        self.particleStartTime = float(d["startTime"])
        self.particleEndTime = float(d["endTime"])
        self.dt = float(d["dt"])
        self.diffusionCoeff = float(d["diffusionCoeff"])
        self.saveInterval = int(d["saveInterval"])
        self.occupancyInterval = int(d.get("occupancyInterval", 0))     # this library's own key (not in DICT_DEFAULTS)
        self.seedingBox = d["seedingBox"]
        self.recycleInterval = int(d.get("recycleInterval", 0))         # this library's own keys, like occupancyInterval
        self.sinkCells = d.get("sinkCells", None)
        self.sourceBox = d.get("sourceBox", self.seedingBox)
        self.sourceTriangles = d.get("sourceTriangles", None)
        self.sourceWeights = d.get("sourceWeights", None)
        self.sourceDepth = d.get("sourceDepth", (0.0, 0.0))
        self.sourceCells = d.get("sourceCells", None)
        self.sourceFollowU = bool(d.get("sourceFollowU", False))
        self.sourceDepthScale = float(d.get("sourceDepthScale", 0.0))
        if self.sourceFollowU:
            if self.recycleInterval <= 0 or self.sourceTriangles is None or self.sourceCells is None:
                raise ValueError("sourceFollowU needs recycleInterval > 0, sourceTriangles and sourceCells")
            if self.sourceWeights is not None:
                raise ValueError("sourceFollowU computes the weights from U: it excludes sourceWeights")
        self.ageBins = int(d.get("ageBins", 0))
        self.ageBinCycles = int(d.get("ageBinCycles", self.recycleInterval if self.recycleInterval > 0 else 1))
        self.sinkGroups = d.get("sinkGroups", None)
        self.sourceOrigins = d.get("sourceOrigins", None)
        self.tags = self.sinkGroups is not None or self.sourceOrigins is not None
        if self.sinkGroups is not None and (self.recycleInterval <= 0 or self.sinkCells is None):
            raise ValueError("sinkGroups needs recycleInterval > 0 and sinkCells")
        if self.sourceOrigins is not None and (self.recycleInterval <= 0 or self.sourceTriangles is None):
            raise ValueError("sourceOrigins needs recycleInterval > 0 and sourceTriangles")
        self.routeStats = bool(d.get("routeStats", False))
        if self.routeStats and not (self.ageBins > 0 and self.tags):
            raise ValueError("routeStats needs ageBins > 0 and tagging (sinkGroups or sourceOrigins)")
        self.exposureField = d.get("exposureField", None)
        self.exposureInterval = int(d.get("exposureInterval", 1))
        self.doseBins = int(d.get("doseBins", 1))
        self.doseBinWidth = d.get("doseBinWidth", None)
        if self.exposureField is None:
            if any(k in d for k in ("exposureInterval", "doseBins", "doseBinWidth")):
                raise ValueError("exposureInterval, doseBins and doseBinWidth need exposureField")
        else:
            self.exposureField = np.ascontiguousarray(self.exposureField, dtype=np.float64).reshape(-1)
            if not (np.all(np.isfinite(self.exposureField)) and np.all(self.exposureField >= 0)):
                raise ValueError("exposureField must be finite and >= 0")
            if self.exposureInterval < 1:
                raise ValueError("exposureInterval must be >= 1")
            if self.doseBins < 1:
                raise ValueError("doseBins must be >= 1")
            if self.doseBinWidth is None and self.doseBins == 1:
                self.doseBinWidth = 1.0                                 # (one open-ended bin: any width)
            if self.doseBinWidth is None or not (math.isfinite(float(self.doseBinWidth)) and float(self.doseBinWidth) > 0):
                raise ValueError("doseBins > 1 needs a positive doseBinWidth")
            self.doseBinWidth = float(self.doseBinWidth)
        self._exposure_pending = 0.0            # time advected since the last exposure point
        self.zoneMap = d.get("zoneMap", None)
        self.zoneInterval = int(d.get("zoneInterval", 1))
        if self.zoneMap is None:
            if "zoneInterval" in d:
                raise ValueError("zoneInterval needs zoneMap")
        else:
            zone_map = np.asarray(self.zoneMap).reshape(-1)
            if zone_map.size == 0 or not np.issubdtype(zone_map.dtype, np.integer) or np.any(zone_map < 0):
                raise ValueError("zoneMap must be one non-negative int per cell")
            if int(zone_map.max()) + 1 > 63:
                raise ValueError("zoneMap has %d zones, 63 at most" % (int(zone_map.max()) + 1))
            if self.zoneInterval < 1:
                raise ValueError("zoneInterval must be >= 1")
            self.zoneMap = np.ascontiguousarray(zone_map, dtype=np.int32)
        self.sinkLog = d.get("sinkLog", 0)
        if isinstance(self.sinkLog, bool) or not isinstance(self.sinkLog, (int, np.integer)) or self.sinkLog < 0:
            raise ValueError("sinkLog must be a non-negative int, the capacity in records")
        self.sinkLog = int(self.sinkLog)
        if self.sinkLog > 0 and (self.recycleInterval <= 0 or self.sinkCells is None):
            raise ValueError("sinkLog needs recycleInterval > 0 and sinkCells")
        # hard-coded switches of the fragment (src/initCuda.H:64-72)
        self.usingAdvection = True
        self.usingBrownianMotion = True
        self.reflectWall = True
        self.step = 0
        self.writer = writer
        self.ctx = Context(device)
        if self.usingBrownianMotion and self.diffusionCoeff > 0:
            # diffusion scrambles the cell order ~5x faster than advection does (tools/sort_decay.py): shorter cadence
            self.ctx.set_option("sort_interval", 25)
        self.ctx.set_mesh(mesh)
        self.ctx.set_velocity(U)
        if self.recycleInterval > 0 and self.sinkCells is not None:
            self.ctx.set_sink_cells(self.sinkCells)
        if self.recycleInterval > 0 and self.sourceTriangles is not None:
            self.ctx.set_source_triangles(self.sourceTriangles, self.sourceWeights, self.sourceDepth)
            if self.sourceFollowU:          # (built with the areas: no triangle with inflow later is dropped now)
                self.ctx.source_follow(self.sourceCells, self.sourceDepthScale)
        if positions is not None:            # parity runs inject positions
            self.ctx.set_particles(positions)
            self.numParticles = int(np.asarray(positions).shape[0])
        else:
            lo, hi = self.seedingBox
            self.ctx.seed_box(self.numParticles, lo, hi, seed_order)
        self.outOfDomain = self.ctx.locate_initial()       # RTQuery + cudaReportParticles
        self.ctx.sort_by_cell()
        if self.ageBins > 0:
            self.ctx.age_enable(self.ageBinCycles, self.ageBins)
        if self.tags:
            n_sinks = 1 if self.sinkGroups is None else int(np.max(self.sinkGroups)) + 1
            n_origins = 1 if self.sourceOrigins is None else int(np.max(self.sourceOrigins)) + 1
            self.ctx.tag_enable(n_origins, n_sinks)
            if self.sinkGroups is not None:
                self.ctx.set_sink_groups(self.sinkCells, self.sinkGroups)
            if self.sourceOrigins is not None:
                self.ctx.set_source_origins(self.sourceOrigins)
        if self.routeStats:
            self.ctx.route_enable()
        if self.exposureField is not None:
            self.ctx.exposure_enable(self.doseBinWidth, self.doseBins)
            self.ctx.set_exposure_field(self.exposureField)
        if self.zoneMap is not None:
            self.ctx.zone_enable(int(self.zoneMap.max()) + 1)
            self.ctx.set_zone_map(self.zoneMap)
        if self.sinkLog > 0:
            self.ctx.sink_log_enable(self.sinkLog)
        if self.writer is not None:
            # frame 0 carries the velocities of one advect and out-of-domain particles as inactive, like the reference
            # (src/initCuda.H:184-201): a cycle of zero length (moves nothing, does not count as a step)
            self.ctx.step(0.0, 0.0, 1, L.STEP_STORE_VEL)
            self._write(0)

    def _flags(self, store_vel: bool) -> int:
        f = 0
        if not self.reflectWall:
            f |= L.STEP_NO_REFLECT
        if store_vel:
            f |= L.STEP_STORE_VEL
        return f

    def _write(self, frame: int):
        xyzw, cell, vel = self.ctx.get_particles(want_vel=True)
        self.writer(frame, xyzw, vel, cell)

    def advect(self, run_time_value: float, delta_t: float, U=None) -> int:
        """One ``#include "advect.H"``: returns the number of Lagrangian cycles done."""
        if not (self.particleStartTime <= run_time_value <= self.particleEndTime):     # advect.H:33
            return 0
        n_cycles = max(int(math.ceil(delta_t / self.dt)), 1)                           # advect.H:36
        cycle_dt = delta_t / n_cycles                                                  # advect.H:37
        if U is not None:                                                              # advect.H:44-57
            self.ctx.set_velocity(U)
        D = self.diffusionCoeff if self.usingBrownianMotion else 0.0
        done = 0
        while done < n_cycles:                                                         # advect.H:86
            will_write = self.writer is not None and (
                self.step % self.saveInterval == 0 or run_time_value == self.particleEndTime)
            # cycles until the next output point run inside ONE launch (U is frozen during the loop)
            chunk = _next_chunk(self.step, n_cycles - done, self.saveInterval, self.occupancyInterval,
                                self.writer is not None, will_write, self.recycleInterval,
                                exposure_interval=self.exposureInterval if self.exposureField is not None else 0,
                                zone_interval=self.zoneInterval if self.zoneMap is not None else 0)
            flags = self._flags(will_write) | (L.STEP_FUSE_CYCLES if chunk > 1 else 0)
            self.ctx.step(cycle_dt, D, chunk, flags)
            if will_write:                                                             # advect.H:166-169
                self._write(self.step + 1)
            self.step += chunk                                                         # advect.H:182
            done += chunk
            if self.exposureField is not None:
                # the time of the cycles just done goes to the cell each particle is in at the next exposure point, which comes
                # BEFORE the recycle point's absorption: the absorbed carry their last interval
                self._exposure_pending += cycle_dt * chunk
                if self.step % self.exposureInterval == 0:
                    self.ctx.exposure_accumulate(self._exposure_pending)
                    self._exposure_pending = 0.0
            if self.zoneMap is not None and self.step % self.zoneInterval == 0:
                self.ctx.zone_sample()                                                 # (BEFORE the absorption: they leave from here)
            if self.recycleInterval > 0 and self.step % self.recycleInterval == 0:
                self.ctx.sink_apply()
                if self.sourceTriangles is not None:
                    self.ctx.respawn_source(-1)
                else:
                    self.ctx.respawn_box(self.sourceBox[0], self.sourceBox[1], -1)
            if self.occupancyInterval > 0 and self.step % self.occupancyInterval == 0:
                self.ctx.occupancy_sample()
                if self.ageBins > 0:
                    self.ctx.age_sample()
                if self.tags:
                    self.ctx.tag_sample()
                if self.routeStats:
                    self.ctx.route_sample()
        return n_cycles

    def particles(self):
        return self.ctx.get_particles()

    def concentration(self):
        """Time-averaged concentration per cell from the samples ``occupancyInterval`` took (``Context.concentration``)."""
        return self.ctx.concentration()

    def recycle_counts(self):
        """absorbed, drawn, placed and epochs of the run so far (``Context.recycle_counts``)."""
        return self.ctx.recycle_counts()

    def rtd(self):
        """Residence-time distribution of the absorbed particles, (edges in seconds, counts), with ``ageBins`` set (``Context.rtd``)."""
        return self.ctx.rtd(self.dt)

    def mean_age(self):
        """Mean age in seconds per cell over the samples ``occupancyInterval`` took, with ``ageBins`` set (``Context.mean_age``)."""
        return self.ctx.mean_age(self.dt)

    def transfer(self):
        """Absorptions by (origin, sink group), with ``sinkGroups`` or ``sourceOrigins`` set (``Context.transfer``)."""
        return self.ctx.transfer()

    def origin_fraction(self):
        """Each origin's share per cell over the samples ``occupancyInterval`` took, NaN where no particle was found
        (``Context.origin_fraction``)."""
        return self.ctx.origin_fraction()

    def rtd_by_route(self):
        """Residence-time distribution per (origin, sink group), (edges in seconds, counts), with ``routeStats`` set
        (``Context.rtd_by_route``)."""
        return self.ctx.rtd_by_route(self.dt)

    def mean_age_by_origin(self):
        """Mean age in seconds per cell and origin over the samples ``occupancyInterval`` took, with ``routeStats`` set
        (``Context.mean_age_by_origin``)."""
        return self.ctx.mean_age_by_origin(self.dt)

    def dose_distribution(self):
        """Dose distribution of the absorbed particles, (edges, counts [n_origins][n_sinks][n_bins]), with ``exposureField`` set
        (``Context.dose_distribution``)."""
        return self.ctx.dose_distribution()

    def doses(self):
        """The dose of every particle in id order, -1 for a dead slot, with ``exposureField`` set (``Context.doses``)."""
        return self.ctx.doses()

    def zone_flows(self):
        """(F [n_zones + 1][n_zones + 1], n_samples): transitions between zones from one zone point to the next, with ``zoneMap``
        set (``Context.zone_flows``)."""
        return self.ctx.zone_flows()

    def zone_residence(self):
        """Mean time of a visit per zone in seconds, with ``zoneMap`` set (``Context.zone_residence``)."""
        return self.ctx.zone_residence(self.zoneInterval * self.dt)

    def sink_log(self):
        """(records, dropped) with ``sinkLog`` set: the ``SINK_LOG_DTYPE`` records of the absorbed since the last call, sorted by
        (apply, id), and how many more found the log full; the log is empty afterwards (``Context.sink_log_drain``).  Nothing else
        drains it: call often enough for the capacity."""
        dropped = self.ctx.sink_log_counts()[1]
        return self.ctx.sink_log_drain(), dropped

    def close(self):
        self.ctx.close()


class StagedCloud:
    """The reference's stage-by-stage call surface on its own array layouts (Particle = double4 AoS,
    vec4d disps / vels, int ids) -- cuda/common.h:32-77, query/ConvexQuery.h:33-46 -- over the
    ``cpf_stage_*`` entry points.  Method names are the reference wrappers' names; ids are CELL ids
    (reference: tet ids, cell = tet / 12).  Arrays live in device memory (``cpf_dev_alloc``); the
    numpy accessors copy."""

    def __init__(self, ctx: Context, n: int):
        self.ctx, self.n = ctx, int(n)
        self._bufs = {}
        for name, nbytes in (("P", 32 * n), ("vels", 32 * n), ("disps", 32 * n), ("ids", 4 * n)):
            p = C.c_void_p()
            ctx._ck(ctx.lib.cpf_dev_alloc(ctx.h, max(nbytes, 16), C.byref(p)))
            ctx._ck(ctx.lib.cpf_dev_memset(ctx.h, p, 0, max(nbytes, 16)))
            self._bufs[name] = p

    def close(self):
        for p in self._bufs.values():
            self.ctx.lib.cpf_dev_free(self.ctx.h, p)
        self._bufs = {}

    def _put(self, name, a):
        a = np.ascontiguousarray(a)
        self.ctx._ck(self.ctx.lib.cpf_copy_to_device(self.ctx.h, self._bufs[name], _ptr(a), a.nbytes))

    def _get(self, name, shape, dtype):
        a = np.empty(shape, dtype)
        self.ctx._ck(self.ctx.lib.cpf_copy_to_host(self.ctx.h, _ptr(a), self._bufs[name], a.nbytes))
        return a

    def set(self, xyzw=None, ids=None):
        if xyzw is not None:
            self._put("P", np.asarray(xyzw, np.float64).reshape(self.n, 4))
        if ids is not None:
            self._put("ids", np.asarray(ids, np.int32).reshape(self.n))

    particles = property(lambda s: s._get("P", (s.n, 4), np.float64))
    vels = property(lambda s: s._get("vels", (s.n, 4), np.float64))
    disps = property(lambda s: s._get("disps", (s.n, 4), np.float64))
    ids = property(lambda s: s._get("ids", (s.n,), np.int32))

    def cudaInitParticles(self, lower, upper, order: int = 1):            # cuda/particles.cu:100-108
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        self.ctx._ck(self.ctx.lib.cpf_stage_seed_box(self.ctx.h, self._bufs["P"], self.n, _ptr(lo), _ptr(hi), order))

    def RTQuery(self):                                                    # query/RTQuery.cu:295-310
        self.ctx._ck(self.ctx.lib.cpf_stage_locate_initial(self.ctx.h, self._bufs["P"], self._bufs["ids"], self.n))

    def cudaReportParticles(self) -> int:                                 # cuda/particles.cu:763-775
        out = C.c_int64()
        self.ctx._ck(self.ctx.lib.cpf_stage_count_outside(self.ctx.h, self._bufs["ids"], self.n, C.byref(out)))
        return out.value

    def cudaAdvect(self, dt: float, mode: str = "TetVelocity"):           # cuda/particles.cu:403-448
        b = self._bufs
        if mode == "TetVelocity":
            self.ctx._ck(self.ctx.lib.cpf_stage_advect(self.ctx.h, b["P"], b["ids"], b["vels"], b["disps"], dt, self.n))
        elif mode == "VertexVelocity":                                    # :428-437 -> particleAdvectKernel :244-313
            self.ctx._ck(self.ctx.lib.cpf_stage_advect_vertex(self.ctx.h, b["P"], b["ids"], b["vels"], b["disps"], dt, self.n))
        elif mode == "ConstantVelocity":                                  # :439-445 -> particleAdvectConstVel :376-399
            self.ctx._ck(self.ctx.lib.cpf_stage_advect_const(self.ctx.h, b["P"], b["ids"], b["vels"], b["disps"], dt, self.n))
        else:
            raise ValueError("cudaAdvect: mode must be TetVelocity, VertexVelocity or ConstantVelocity (cuda/particles.cu:417-445)")

    def cudaBrownianMotion(self, dt: float, D: float, step: int):         # cuda/particles.cu:577-599
        b = self._bufs
        self.ctx._ck(self.ctx.lib.cpf_stage_brownian(self.ctx.h, b["P"], b["disps"], dt, self.n, D, step))

    def convexTetQuery(self):                                             # query/ConvexQuery.cu:218-234
        b = self._bufs
        self.ctx._ck(self.ctx.lib.cpf_stage_locate(self.ctx.h, b["P"], b["disps"], b["ids"], self.n))

    def convexWallReflect(self):                                          # query/ConvexQuery.cu:438-458
        b = self._bufs
        self.ctx._ck(self.ctx.lib.cpf_stage_reflect(self.ctx.h, b["ids"], b["P"], b["vels"], b["disps"], self.n))

    def cudaMoveParticles(self):                                          # cuda/particles.cu:706-716
        b = self._bufs
        self.ctx._ck(self.ctx.lib.cpf_stage_move(self.ctx.h, b["P"], b["disps"], self.n))
