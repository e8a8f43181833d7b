"""TEST INFRASTRUCTURE ONLY.  Routes (include/cpf.h "routes") stated in numpy on top of tests/age.py and tests/tags.py: the joint
histogram [origin][sink group][bin] as one ``numpy.add.at`` over exactly the absorbed, the age field per origin as two bincounts
of the virtual id parent * nOrigins + origin, one of them weighted by the age, and the tagged recycled runs of tests/tags.py
carried through with births as tests/age.py carries its runs.  Shared by tests/test_routes_host.py (no GPU) and
tests/test_gpu_routes.py."""
from __future__ import annotations

import functools

import numpy as np

import age as A
import recycle as R
import sourcepatch as SP
import tags as T

FIELD_BINS = 2048                            # csrc/cpf_routes.hip, kRouteBins: a slice whose window of virtual ids is wider goes
                                             # through the direct-mapped cache
JOINT_WORDS = 4096                           # kRouteJointWords: a joint histogram of more words is added to in global memory


def hist(origin, group_of_cell, cell, hit, age, bin_cycles, n_bins, n_origins, n_sinks):
    """[n_origins][n_sinks][n_bins] uint64: one count per absorbed particle (hit) at (its origin, the group of its cell,
    min(age // bin_cycles, n_bins - 1)); origin, cell, hit and age are arrays over the same particles"""
    H = np.zeros((n_origins, n_sinks, n_bins), np.int64)
    o = np.asarray(origin, np.int64)[hit]
    g = np.asarray(group_of_cell, np.int64)[np.asarray(cell)[hit]]
    b = np.minimum(np.asarray(age, np.int64)[hit] // bin_cycles, n_bins - 1)
    np.add.at(H, (o, g, b), 1)
    return H.astype(np.uint64)


def field(parent, origin, age, n_cells, n_origins):
    """(age sum, count), each [n_cells][n_origins] uint64, over the live particles (parent >= 0): two bincounts of the virtual id.
    (The weighted one sums in float64: exact while a sum stays below 2^53, which every test's does.)"""
    parent, origin, age = np.asarray(parent, np.int64), np.asarray(origin, np.int64), np.asarray(age, np.int64)
    live = parent >= 0
    v = parent[live] * n_origins + origin[live]
    count = np.bincount(v, minlength=n_cells * n_origins)
    total = np.bincount(v, weights=age[live].astype(np.float64), minlength=n_cells * n_origins)
    assert total.max(initial=0.0) < 2.0 ** 53
    return (total.astype(np.uint64).reshape(n_cells, n_origins), count.astype(np.uint64).reshape(n_cells, n_origins))


def window_edge(n_origins):
    """tests/tags.py's "window_edge" for FIELD_BINS bins: (cells int32, origins uint8), two slices whose windows of virtual ids
    are exactly FIELD_BINS and FIELD_BINS + 1 wide"""
    rng = np.random.default_rng(12)
    top = n_origins - 1
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


# ------------------------------------------------------------------------------------------------ the whole recycled runs (D = 0)
BIN_CYCLES, N_BINS = A.BIN_CYCLES, A.N_BINS
LIMITED_ROUND = A.LIMITED_ROUND              # "thin box" never re-sorts: its array order is the id order


def cpu_route_run(r: T.Run, tables, cell0, limited_round=None):
    """``tags.cpu_tagged_run`` carrying the births as ``age.cpu_recycled_run`` does, the joint histogram and the age field per
    origin: a round is `cycles` cycles, the sink (the absorbed add to hist[origin][group][age bin]), a respawn at epoch = round
    which first gives EVERY dead slot the cycle count as its birth and the origin of the triangle picked for (seed, id, epoch),
    then one sample of the field.  limited_round: in that round the respawn takes only the first half of the dead slots in ARRAY
    order (id order: the caller's run must not re-sort).  Returns a dict; `rounds` holds the tables as they stand after each
    round."""
    b = r.base
    cw = R.cellwalk()
    t = cw.build(b.mesh)
    rec, hi = SP.table(b.tri, b.weights, b.depth, exact=False)
    okept = T.origin_of_kept(rec, r.origin_of_triangle)
    group = T.group_of_cell(b.mesh.n_cells, b.sink_cells, r.groups)
    nc = b.mesh.n_cells
    x, y, z = (np.ascontiguousarray(b.xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    origin = np.zeros(cell.size, np.uint8)
    births = np.zeros(cell.size, np.uint32)
    H = np.zeros((T.N_ORIGINS, T.N_SINKS, N_BINS), np.uint64)
    Fs, Fc = np.zeros((nc, T.N_ORIGINS), np.uint64), np.zeros((nc, T.N_ORIGINS), np.uint64)
    absorbed = drawn = placed = now = 0
    limited_count, rounds = None, []
    for epoch in range(b.rounds):
        cw.step_given(x, y, z, cell, b.dt, b.cycles, t, b.U, 0.0, None, nthreads=cw.max_threads)
        now += b.cycles
        after = R.sink(cell, b.sink_cells)
        hit = after != cell
        H += hist(origin, group, cell, hit, A.ages(now, births), BIN_CYCLES, N_BINS, T.N_ORIGINS, T.N_SINKS)
        absorbed += int(hit.sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        births[dead] = now
        origin[dead] = okept[T.picks(R.SEED, dead, epoch, hi)]
        if epoch == limited_round:
            limited_count = dead.size // 2
            dead = dead[:limited_count]
        p = SP.positions(R.SEED, dead, epoch, rec, hi)
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
        s, c = field(cell, origin, A.ages(now, births), nc, T.N_ORIGINS)
        Fs += s
        Fc += c
        rounds.append(dict(hist=H.copy(), field_sum=Fs.copy(), field_count=Fc.copy()))
    return dict(xyz=np.stack([x, y, z], 1), cell=cell, absorbed=absorbed, drawn=drawn, placed=placed, origin=origin, births=births,
                hist=H, field_sum=Fs, field_count=Fc, rounds=rounds, limited_count=limited_count, now=now)


@functools.lru_cache(maxsize=None)
def cpu(name):
    """the routed recycled run `name`, from its brute-force initial locate"""
    from cudaparticlesfoam_amd import api
    r = T.run(name)
    t = api.build_mesh_tables_host(r.base.mesh)
    tables = (t["cell_off"], t["planes"], t["nbr"])
    return cpu_route_run(r, tables, R.brute_locate(r.base.xyz, tables), LIMITED_ROUND[name])
