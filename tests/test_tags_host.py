"""CPU: the host side of the tracer tags (include/cpf.h "tracer tags"): the triangle a respawn picks per particle id
(cpf_source_picks_host: the kernels' own text compiled for the host) against the numpy pick on the oracle's Philox, the origin a
kept record gets from the caller's list, also when triangles were dropped from the table, and the numpy statements of tests/tags.py
themselves on small hand-made cases."""
import numpy as np
import pytest

import sourcepatch as SP
import tags as T
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api
from cudaparticlesfoam_amd.cases.blockmesh import box_mesh

GIDS = np.array([0, 1, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 62 + 5], np.int64)     # test_recycle_host.py's
SEEDS = [9, 1591593751, 0xFFFFFFFF]
EPOCHS = [0, 1, 7, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def slab_triangles():
    mesh = box_mesh(32, 32, 2)
    tri, _ = mesh.face_triangles(np.arange(mesh.n_internal, mesh.n_faces)[:2049])
    assert tri.shape == (4098, 3, 3)
    return tri


def _table(tri, m):
    weights = 1.0 + (np.arange(m) % 7)                                       # unequal shares
    rec, hi = api.source_table_host(tri[:m], weights)
    assert hi.size == m and hi[-1] == 0xFFFFFFFF
    return rec, hi


# ------------------------------------------------------------------------------------------------ 1. the pick
@pytest.mark.parametrize("m", [1, 60, 4096, 4098])
def test_1_picks_are_the_numpy_pick_on_the_oracles_philox(slab_triangles, oracle_libs, m):
    rec, hi = _table(slab_triangles, m)
    for seed in SEEDS:
        for epoch in EPOCHS:
            got = api.source_picks_host(seed, GIDS, epoch, hi)
            want = T.picks(seed, GIDS, epoch, hi)                            # nine ids: the oracle's Philox, one call each
            assert got.dtype == np.int32 and np.array_equal(got, want), (m, seed, epoch, got, want)
    # many ids, above 2^32 among them: every part of the table is picked, its two ends included
    rng = np.random.default_rng(m)
    many = np.concatenate([np.arange(5000), 2 ** 32 + np.arange(5000), rng.integers(0, 2 ** 62, size=5000)]).astype(np.int64)
    for epoch in (0, 3):
        got = api.source_picks_host(9, many, epoch, hi)
        assert np.array_equal(got, T.picks(9, many, epoch, hi))
        assert got.min() == 0 and got.max() == m - 1 if m <= 60 else (got.min() < 8 and got.max() > m - 8)
    assert not np.array_equal(api.source_picks_host(9, many, 0, hi), api.source_picks_host(9, many, 3, hi)) or m == 1
    # gid NULL: the ids 0 .. n-1
    assert np.array_equal(api.source_picks_host(9, None, 2, hi, n=130), api.source_picks_host(9, np.arange(130), 2, hi))
    # the pick is the triangle the position lies on: cpf_source_positions_host goes through the same two functions
    pos, t, _, _, _ = SP.positions(9, GIDS, 5, rec, hi, want_parts=True)
    assert np.array_equal(api.source_picks_host(9, GIDS, 5, hi), t)


def test_1_argument_errors(slab_triangles):
    lib, p = L.load(), api._ptr
    _, hi = _table(slab_triangles, 60)
    out = np.empty(4, np.int32)
    assert lib.cpf_source_picks_host(1, None, 4, 0, p(hi), 60, p(out)) == L.CPF_OK
    assert lib.cpf_source_picks_host(1, None, 4, 0, None, 60, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_picks_host(1, None, 4, 0, p(hi), 0, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_picks_host(1, None, 4, 0, p(hi), 59, p(out)) == L.CPF_ERR_ARG          # the last bound is not 2^32 - 1
    assert lib.cpf_source_picks_host(1, None, 4, 0, p(hi), 60, None) == L.CPF_ERR_ARG
    assert lib.cpf_source_picks_host(1, None, -1, 0, p(hi), 60, p(out)) == L.CPF_ERR_ARG
    assert lib.cpf_source_picks_host(1, None, 0, 0, p(hi), 60, None) == L.CPF_OK


# ------------------------------------------------------------------------------------------------ 2. the origin of a kept record
def test_2_a_kept_record_gets_the_origin_of_its_callers_triangle(slab_triangles, oracle_libs):
    m = 60
    tri = slab_triangles[:m].copy()
    weights = 1.0 + (np.arange(m) % 7)
    weights[::5] = 0.0                                                       # dropped: weight 0
    tri[7, 2] = tri[7, 1]                                                    # dropped: degenerate
    rec, hi = api.source_table_host(tri, weights)
    dropped = np.union1d(np.arange(0, m, 5), [7])
    kept = np.setdiff1d(np.arange(m), dropped)
    assert np.array_equal(rec[:, 14], kept) and hi.size == kept.size
    origin_of_triangle = (np.arange(m) * 7 + 3) % T.TAG_MAX                  # by the CALLER's triangle, the dropped ones included
    okept = T.origin_of_kept(rec, origin_of_triangle)
    for k, i in enumerate(kept):
        assert okept[k] == origin_of_triangle[i]
    # ... so a particle's origin is the origin of the caller's triangle its position lies on
    ids = np.concatenate([GIDS, np.arange(3000)])
    pick = api.source_picks_host(9, ids, 2, hi)
    assert np.array_equal(pick, T.picks(9, ids, 2, hi))
    caller = rec[pick, 14].astype(np.int64)
    assert not np.isin(caller, dropped).any() and np.unique(caller).size == kept.size
    assert np.array_equal(okept[pick], origin_of_triangle[caller])
    # without a drop the two lists are one
    rec, hi = _table(slab_triangles, m)
    assert np.array_equal(T.origin_of_kept(rec, origin_of_triangle), origin_of_triangle)


# ------------------------------------------------------------------------------------------------ 3. the statements, by hand
def test_3_the_numpy_statements_on_a_case_counted_by_hand():
    cell = np.array([0, 2, 2, -1, 3, 2, 1], np.int32)
    origin = np.array([0, 1, 2, 2, 1, 1, 0], np.uint8)
    group = T.group_of_cell(4, [2, 3], [1, 0])
    hit = np.isin(cell, [2, 3])
    assert T.transfer(origin, group, cell, hit, 3, 2).tolist() == [[0, 0], [1, 2], [0, 1]]
    assert T.field(cell, origin, 4, 3).tolist() == [[1, 1, 0, 0], [0, 0, 2, 1], [0, 0, 1, 0]]
    for name in T.ADVERSARIAL:
        for n_origins in (1, 16):
            c, o = T.adversarial(name, n_origins)
            assert c.dtype == np.int32 and o.dtype == np.uint8 and c.shape == o.shape and o.max() == n_origins - 1


def test_3_the_tagged_runs_use_both_origins_and_both_groups(oracle_libs):
    for name in ("graded box", "thin box"):
        c = T.cpu(name)
        assert int(c["transfer"].sum()) == c["absorbed"] >= 200
        assert (c["transfer"][1:] > 0).all() and (c["transfer"][0] > 0).any()              # the initial cloud leaves too
        assert {1, 2} <= set(np.unique(c["origin"]).tolist()) <= {0, 1, 2}
        assert np.array_equal(c["field"].sum(0), c["occupancy"]) and (c["field"].sum(1) > 0).all()
