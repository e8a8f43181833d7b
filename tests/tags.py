"""TEST INFRASTRUCTURE ONLY.  Tracer tags (include/cpf.h "tracer tags") stated in numpy: origins as an array indexed by particle id,
the transfer matrix as one ``numpy.add.at`` over the absorbed, the per-origin field as a bincount over the virtual id
parent * nOrigins + origin, the stamp as the pick of tests/sourcepatch.py on the oracle's Philox, and the recycled runs of
tests/recycle.py with the x = 0 patch as a source of two origins and the last x layer as a sink of two groups.  Shared by
tests/test_tags_host.py (no GPU) and tests/test_gpu_tags.py."""
from __future__ import annotations

import functools

import numpy as np

import recycle as R
import sourcepatch as SP

TAG_MAX = 16                                 # origins, and sink groups, at most
FIELD_BINS = 4096                            # csrc/cpf_tags.hip, kTagFieldBins: a slice whose window of virtual ids is wider goes
                                             # through the direct-mapped cache


def transfer(origin, group_of_cell, cell, hit, n_origins, n_sinks):
    """[n_origins][n_sinks] uint64: one count per absorbed particle (hit) at (its origin, the group of its cell)"""
    T = np.zeros((n_origins, n_sinks), np.int64)
    np.add.at(T, (np.asarray(origin, np.int64)[hit], np.asarray(group_of_cell, np.int64)[np.asarray(cell)[hit]]), 1)
    return T.astype(np.uint64)


def group_of_cell(n_cells, sink_cells, groups):
    """the group of every cell: 0 outside the sink (never read there)"""
    g = np.zeros(n_cells, np.int64)
    g[np.asarray(sink_cells)] = np.asarray(groups)
    return g


def field(parent, origin, n_cells, n_origins):
    """[n_origins][n_cells] uint64 over the live particles (parent >= 0): the bincount of the virtual id, reshaped"""
    parent, origin = np.asarray(parent, np.int64), np.asarray(origin, np.int64)
    live = parent >= 0
    return (np.bincount(parent[live] * n_origins + origin[live], minlength=n_cells * n_origins)
            .reshape(n_cells, n_origins).T.astype(np.uint64))


def picks(seed, gids, epoch, hi):
    """the kept record the source picks per id: the first t with word 0 <= hi[t], on the oracle's Philox"""
    return SP.pick(hi, SP.words(seed, gids, epoch)[:, 0])


def origin_of_kept(rec, origin_of_triangle):
    """the origin of every kept record: its caller's triangle (rec[:, 14]) looked up in the caller's list"""
    return np.asarray(origin_of_triangle, np.int64)[np.asarray(rec)[:, 14].astype(np.int64)]


# ---- the adversarial id arrays of tests/test_gpu_occupancy.py and tests/test_gpu_age.py, with an origin per particle: 36 000 cells
N_BIG = 36_000


def adversarial(name, n_origins):
    """(cells int32 [n], origins uint8 [n])"""
    rng = np.random.default_rng(11)
    top = n_origins - 1
    if name == "one_cell":
        c = np.full(70_001, 12_345, np.int32)
    elif name == "two_alternating":
        c = np.where(np.arange(4097) % 2 == 0, 7, 35_999).astype(np.int32)
    elif name == "two_aliasing":                                             # far apart, and the same bin of the cache for equal origins
        c = np.where(np.arange(4097) % 2 == 0, 5, 5 + 3 * 2048 * 5).astype(np.int32)
    elif name == "permutation_with_lost":
        c = rng.permutation(N_BIG).astype(np.int32)
        c[::7] = -1
    elif name == "sorted_sparse":                                            # the window of a slice overflows the LDS bins
        c = np.sort(rng.choice(N_BIG, size=5000, replace=False)).astype(np.int32)
    elif name == "sorted_dense":                                             # several workgroups, each with a wide LDS window
        c = np.sort(rng.integers(0, N_BIG, size=50_001)).astype(np.int32)
    elif name == "window_edge":
        # windows of exactly FIELD_BINS and FIELD_BINS + 1 VIRTUAL ids, one slice each: (100, origin 0) .. (100 + w - 1, top), and
        # (9000, top) .. (9000 + w, top), with w * n_origins == FIELD_BINS
        assert FIELD_BINS % n_origins == 0
        w = FIELD_BINS // n_origins
        a = np.concatenate([[100], rng.integers(100, 100 + w, size=4094), [100 + w - 1]])
        b = np.concatenate([[9000], rng.integers(9000, 9000 + w + 1, size=4094), [9000 + w]])
        c = np.concatenate([a, b]).astype(np.int32)
        o = rng.integers(0, n_origins, size=c.size).astype(np.uint8)
        o[0], o[4095] = 0, top
        o[4096:][b == 9000] = top
        o[8191] = top
        v = c.astype(np.int64) * n_origins + o
        assert v[:4096].max() - v[:4096].min() + 1 == FIELD_BINS and v[4096:].max() - v[4096:].min() + 1 == FIELD_BINS + 1
        return c, o
    elif name == "codes_and_foreign_ids":                                    # frozen, lost, ids that are no cells of the mesh
        c = rng.integers(0, N_BIG, size=9001).astype(np.int32)
        c[::5] = -2; c[1::5] = N_BIG; c[2::5] = np.iinfo(np.int32).max; c[3::11] = np.iinfo(np.int32).min
    else:
        c = rng.integers(0, N_BIG, size=int(name[1:])).astype(np.int32)      # "n<length>"
    o = rng.integers(0, n_origins, size=c.size).astype(np.uint8)
    o[::4] = top
    return c, o


ADVERSARIAL = ["one_cell", "two_alternating", "two_aliasing", "permutation_with_lost", "sorted_sparse", "sorted_dense", "window_edge",
               "codes_and_foreign_ids", "n1", "n63", "n64", "n65", "n4099"]


# ------------------------------------------------------------------------------------------------ the whole recycled runs (D = 0)
N_ORIGINS, N_SINKS = 3, 2                    # origin 0: the initial cloud; 1, 2: the lower and the upper half of the x = 0 patch


class Run:
    """``sourcepatch.Run`` with the source split into two origins by the triangles' centroids (y below / above the patch's middle)
    and the sink (the last x layer) split into two groups by the cells' centres in the same way."""

    def __init__(self, name):
        self.base = SP.run(name)
        b = self.base
        lo, hi = b.mesh.bounds()
        mid = 0.5 * (lo[1] + hi[1])
        self.origin_of_triangle = np.where(b.tri.mean(1)[:, 1] < mid, 1, 2).astype(np.int32)
        centres = b.mesh.cell_centres_volumes()[0]
        self.groups = np.where(centres[b.sink_cells, 1] < mid, 0, 1).astype(np.int32)
        assert set(self.origin_of_triangle) == {1, 2} and set(self.groups) == {0, 1}


@functools.lru_cache(maxsize=None)
def run(name) -> Run:
    return Run(name)


def cpu_tagged_run(r: Run, tables, cell0):
    """``sourcepatch.cpu_recycled_run`` carrying the origins, the transfer matrix and the per-origin field: tagging starts with
    everybody in origin 0; a round is `cycles` cycles, the sink (the absorbed add to transfer[origin][group of the cell]), a respawn
    at epoch = round which first gives EVERY dead slot the origin of the triangle picked for (seed, id, epoch), then one sample of
    the field.  gid = index.  Returns a dict."""
    b = r.base
    cw = R.cellwalk()
    t = cw.build(b.mesh)
    rec, hi = SP.table(b.tri, b.weights, b.depth, exact=False)
    okept = origin_of_kept(rec, r.origin_of_triangle)
    group = group_of_cell(b.mesh.n_cells, b.sink_cells, r.groups)
    x, y, z = (np.ascontiguousarray(b.xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    origin = np.zeros(cell.size, np.uint8)
    T = np.zeros((N_ORIGINS, N_SINKS), np.uint64)
    F = np.zeros((N_ORIGINS, b.mesh.n_cells), np.uint64)
    occ = np.zeros(b.mesh.n_cells, np.uint64)
    absorbed = drawn = placed = 0
    for epoch in range(b.rounds):
        cw.step_given(x, y, z, cell, b.dt, b.cycles, t, b.U, 0.0, None, nthreads=cw.max_threads)
        after = R.sink(cell, b.sink_cells)
        hit = after != cell
        T += transfer(origin, group, cell, hit, N_ORIGINS, N_SINKS)
        absorbed += int(hit.sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        origin[dead] = okept[picks(R.SEED, dead, epoch, hi)]
        p = SP.positions(R.SEED, dead, epoch, rec, hi)
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
        F += field(cell, origin, b.mesh.n_cells, N_ORIGINS)
        occ += np.bincount(cell[cell >= 0], minlength=b.mesh.n_cells).astype(np.uint64)
    return dict(xyz=np.stack([x, y, z], 1), cell=cell, absorbed=absorbed, drawn=drawn, placed=placed, origin=origin, transfer=T,
                field=F, occupancy=occ, samples=b.rounds)


@functools.lru_cache(maxsize=None)
def cpu(name):
    """the tagged recycled run `name`, from its brute-force initial locate"""
    from cudaparticlesfoam_amd import api
    r = run(name)
    t = api.build_mesh_tables_host(r.base.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    return cpu_tagged_run(r, tables, R.brute_locate(r.base.xyz, tables))
