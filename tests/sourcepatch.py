"""TEST INFRASTRUCTURE ONLY.  The patch source (include/cpf.h "patch source") stated in numpy: the table rule, the position rule on
the oracle's Philox at 7 rounds -- one numpy operation per rounding --, and a whole recycled run like ``recycle.cpu_recycled_run``
with the patch source in the box's place.  Shared by tests/test_source_host.py (no GPU) and tests/test_gpu_source.py."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import recycle as R

KEY1 = 0x43504633                  # "CPF3": the source stream's second key word (the box's is ...32, the kick's ...31)
N = R.N
TWO32 = 2 ** 32


# ------------------------------------------------------------------------------------------------ the table
def geometry(tri):
    """(e1, e2, c, len, nIn, area) of tri[m][3][3], every operation rounded on its own, in the builder's order."""
    t = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    e1 = t[:, 1] - t[:, 0]
    e2 = t[:, 2] - t[:, 0]
    c = np.empty_like(e1)
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        p = e1[:, b] * e2[:, d]
        q = e1[:, d] * e2[:, b]
        c[:, a] = p - q
    sq = c * c
    s = sq[:, 0] + sq[:, 1]
    s = s + sq[:, 2]
    length = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_in = -c / length[:, None]
    return e1, e2, c, length, n_in, length / 2.0


def table(tri, weights=None, depth=(0.0, 0.0), exact=True):
    """(rec [k][16], hi [k] uint32): the table rule.  exact: the bounds come from EXACT running sums of the weights (fractions),
    so they may differ by one count from a builder that sums in fp64; not exact: the running sums, the quotient and the product
    are fp64 operations in input order, the builder's own arithmetic."""
    t = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    e1, e2, _, length, n_in, area = geometry(t)
    w = area if weights is None else np.asarray(weights, np.float64)
    keep = np.nonzero((length != 0.0) & (w != 0.0))[0]
    if exact:
        sums, run = [], Fraction(0)
        for i in keep:
            run += Fraction(float(w[i]))
            sums.append(run)
        b = [(s * TWO32) // run for s in sums]
    else:
        sums = np.cumsum(w[keep])                                       # (sequential adds)
        share = sums / sums[-1]
        b = [min(int(v), TWO32) for v in np.floor(share * 4294967296.0)]
    b[-1] = TWO32
    rows, hi, before = [], [], 0
    d = np.asarray(depth, np.float64)
    for i, bt in zip(keep, b):
        bt = int(bt)
        if bt == before:
            continue
        before = bt
        d0, d1 = (d[0], d[1]) if d.shape == (2,) else (d[i, 0], d[i, 1])
        rows.append(np.concatenate([t[i, 0], e1[i], e2[i], n_in[i], [d0, d1 - d0, float(i), 0.0]]))
        hi.append(bt - 1)
    return np.array(rows, np.float64).reshape(-1, 16), np.array(hi, np.uint32)


# ------------------------------------------------------------------------------------------------ the position
def _oracle_words(seed, gids, epoch):
    cw = R.cellwalk()
    w = np.empty((len(gids), 4), np.uint32)
    for i, g in enumerate(gids):
        g = int(g)
        w[i] = cw.philox(np.array([g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, epoch & 0xFFFFFFFF, 0], np.uint32),
                         np.array([seed & 0xFFFFFFFF, KEY1], np.uint32), rounds=7)[:4]
    return w


def _numpy_words(seed, gids, epoch):
    """Philox4x32-7 over an array of counters at once (Salmon et al., SC'11), in 64-bit numpy integers"""
    g = np.asarray(gids, np.int64).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [g & m32, (g >> np.uint64(32)) & m32, np.full(g.shape, epoch & 0xFFFFFFFF, np.uint64), np.zeros(g.shape, np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, KEY1
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def words(seed, gids, epoch):
    """[n][4] uint32: Philox4x32-7, counter (gid low, gid high, epoch, 0), key (seed, KEY1).  Up to 64 ids: the oracle's Philox,
    one call each; more: the same rounds over the whole array in numpy, checked against the oracle's on 16 of the ids."""
    gids = np.asarray(gids, np.int64).reshape(-1)
    if gids.size <= 64:
        return _oracle_words(seed, gids, epoch)
    w = _numpy_words(seed, gids, epoch)
    some = np.linspace(0, gids.size - 1, 16).astype(np.int64)
    assert np.array_equal(w[some], _oracle_words(seed, gids[some], epoch))
    return w


def pick(hi, w0):
    """the first index t with w0 <= hi[t]"""
    return np.searchsorted(np.asarray(hi, np.uint32), np.asarray(w0, np.uint32), side="left")


def fold(w):
    """(w1, w2) of the words as 64-bit integers: both mirrored where w1 + w2 > 2^32"""
    w1, w2 = w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)
    over = w1 + w2 > TWO32
    return np.where(over, TWO32 - w1, w1), np.where(over, TWO32 - w2, w2)


def positions(seed, gids, epoch, rec, hi, want_parts=False):
    """[n][3]: word 0 picks the triangle, words 1 and 2 the point, word 3 the depth; pos_k = ((A_k + u1 * e1_k) + u2 * e2_k) + d *
    nIn_k, every product and sum a numpy operation of its own."""
    w = words(seed, gids, epoch)
    t = pick(hi, w[:, 0])
    r = np.asarray(rec, np.float64)[t]
    w1, w2 = fold(w)
    u1 = w1.astype(np.float64) * 2.0 ** -32
    u2 = w2.astype(np.float64) * 2.0 ** -32
    ud = w[:, 3].astype(np.float64) * 2.0 ** -32
    dspan = ud * r[:, 13]
    d = r[:, 12] + dspan
    a1 = u1[:, None] * r[:, 3:6]
    s1 = r[:, 0:3] + a1
    a2 = u2[:, None] * r[:, 6:9]
    s2 = s1 + a2
    a3 = d[:, None] * r[:, 9:12]
    pos = s2 + a3
    return (pos, t, u1, u2, d) if want_parts else pos


def recompute(pts, rec, t):
    """(u1, u2, d) of the points from the points themselves: d along nIn, (u1, u2) by least squares in the triangle's plane"""
    r = rec[t]
    rel = pts - r[:, 0:3]
    d = (rel * r[:, 9:12]).sum(1)
    flat = rel - d[:, None] * r[:, 9:12]
    e1, e2 = r[:, 3:6], r[:, 6:9]
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    f, g = (flat * e1).sum(1), (flat * e2).sum(1)
    det = a * c - b * b
    return (c * f - b * g) / det, (a * g - b * f) / det, d


# ------------------------------------------------------------------------------------------------ a whole recycled run
def cpu_recycled_run(mesh, tables, U, xyz, cell0, dt, rounds, cycles, sink_cells, rec, hi, seed):
    """``recycle.cpu_recycled_run`` with the patch source: K rounds of `cycles` unkicked cycles, the sink, a respawn of every dead
    slot on the source at epoch = round.  Returns (xyz, cell, absorbed, drawn, placed, respawns per particle)."""
    cw = R.cellwalk()
    t = cw.build(mesh)
    x, y, z = (np.ascontiguousarray(xyz[:, k]).copy() for k in range(3))
    cell = np.array(cell0, np.int32)
    absorbed = drawn = placed = 0
    times = np.zeros(cell.size, np.int64)
    for epoch in range(rounds):
        cw.step_given(x, y, z, cell, dt, cycles, t, U, 0.0, None, nthreads=cw.max_threads)
        after = R.sink(cell, sink_cells)
        absorbed += int((after != cell).sum())
        cell = after
        dead = np.nonzero(cell < 0)[0]
        p = positions(seed, dead, epoch, rec, hi)
        where = R.brute_locate(p, tables)
        x[dead], y[dead], z[dead] = p[:, 0], p[:, 1], p[:, 2]
        cell[dead] = where
        drawn += dead.size
        placed += int((where >= 0).sum())
        times[dead[where >= 0]] += 1
    return np.stack([x, y, z], 1), cell, absorbed, drawn, placed, times


def boundary_faces_at_x0(mesh):
    """the boundary faces whose every vertex has x == 0"""
    fo = mesh.face_offsets.astype(np.int64)
    return np.array([f for f in range(mesh.n_internal, mesh.n_faces)
                     if (mesh.points[mesh.face_verts[fo[f]:fo[f + 1]], 0] == 0.0).all()], np.int32)


class Run:
    """``recycle.Run`` with the x = 0 patch as the source: the weights are the inflow's, the depth per triangle is what its owner
    cell's flow covers in one round, |U.n| * dt * cycles (plus D0, see there)."""
    D0 = 0.0

    def __init__(self, name):
        from cudaparticlesfoam_amd import api
        self.base = R.run(name)
        b = self.base
        self.name, self.mesh, self.U, self.dt, self.sort_interval = name, b.mesh, b.U, b.dt, b.sort_interval
        self.rounds, self.cycles, self.sink_cells, self.xyz = b.rounds, b.cycles, b.sink_cells, b.xyz
        self.faces = boundary_faces_at_x0(b.mesh)
        self.tri, self.face_of_tri = b.mesh.face_triangles(self.faces)
        self.weights = api.inflow_weights(b.mesh, b.U, self.tri, self.face_of_tri)
        un = np.abs(b.U[b.mesh.owner[self.face_of_tri], 0])              # n_out = (-1, 0, 0) on the x = 0 patch
        span = un * (b.dt * b.cycles)
        self.depth = np.stack([np.full(span.size, self.D0), self.D0 + span], 1)

    def cpu(self, tables, cell0):
        rec, hi = table(self.tri, self.weights, self.depth, exact=False)
        return cpu_recycled_run(self.mesh, tables, self.U, self.xyz, cell0, self.dt, self.rounds, self.cycles, self.sink_cells,
                                rec, hi, R.SEED)


@functools.lru_cache(maxsize=None)
def run(name) -> Run:
    return Run(name)
