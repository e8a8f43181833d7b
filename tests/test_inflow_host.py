"""CPU: the flux table on the host (include/cpf.h "flux table"): cpf_source_flux_host against the numpy statement of
tests/inflow.py, bit for bit -- hi, span and q -- on seeded random triangle soups and velocity fields; the three properties every
search of the table relies on; that a triangle's share of the picks is its share of the quanta; the refusals."""
import ctypes as C

import numpy as np
import pytest

import inflow as IF
import sourcepatch as SP
from cudaparticlesfoam_amd import _lib as L
from cudaparticlesfoam_amd import api

SIZES = [1, 2, 3, 64, 65, 257, 4097]
DEPTH = (0.001, 0.003)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _table(seed, k, scale=1.0):
    """a table of k kept records (areas as weights), one owner cell per triangle: triangle t is owned by cell t"""
    tri = IF.soup(seed, k) * scale
    rec, hi = api.source_table_host(tri, None, DEPTH)
    assert rec.shape[0] == k
    return rec, hi, np.arange(k, dtype=np.int32)


def _field(seed, rec, mag=None):
    """U per cell == per triangle: a random field, or mag[t] * nIn_t (mag <= 0: no inflow through triangle t)"""
    k = rec.shape[0]
    if mag is None:
        return np.random.default_rng(seed).normal(size=(k, 3))
    return rec[:, 9:12] * np.asarray(mag, np.float64)[:, None]


def _same(rec, cells, U, s):
    """host entry == model, bit for bit; returns the host's (span, hi, q, empty)"""
    span, hi, q, empty = api.source_flux_host(rec, cells, U, s)
    wspan, whi, wq, wempty = IF.flux(rec, cells, U, s)
    assert empty == wempty
    if not empty:
        assert np.array_equal(q, wq)
        assert np.array_equal(hi, whi)
        assert np.array_equal(_bits(span), _bits(wspan))
    return span, hi, q, empty


def _properties(hi, seed=7):
    """non-decreasing, ends in 0xFFFFFFFF, and the host's pick of a draw is the model's lower bound"""
    assert hi.dtype == np.uint32 and int(hi[-1]) == 0xFFFFFFFF
    assert np.all(hi[1:] >= hi[:-1])
    gids = np.arange(48, dtype=np.int64)
    w0 = SP.words(seed, gids, 3)[:, 0]
    assert np.array_equal(api.source_picks_host(seed, gids, 3, hi), SP.pick(hi, w0))
    # and at the bounds themselves: a draw equal to a bound goes to the FIRST record with that bound
    first = SP.pick(hi, hi)
    assert np.array_equal(hi[first], hi) and np.all((first == 0) | (hi[np.maximum(first, 1) - 1] < hi))
    return True


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("s", [0.0, 0.0125])
def test_random_fields_match_the_model(k, s):
    rec, _, cells = _table(100 + k, k)
    some = False
    for seed in range(3):
        span, hi, q, empty = _same(rec, cells, _field(seed, rec), s)
        if not empty:
            some = True
            _properties(hi)
            assert int(q.max()) >= 2 ** 31 and int(q.max()) < 2 ** 32
            if s == 0.0:
                assert not span.any()
    assert some or k == 1                       # (a single triangle may face away from all three fields)


def test_cells_shared_between_triangles():
    """several triangles per owner cell, and cells that own none: the gather goes through column 14"""
    tri = IF.soup(11, 300)
    area = SP.geometry(tri)[5]
    weights = np.where(np.arange(300) % 7 == 3, 0.0, area)             # dropped triangles: column 14 skips them
    rec, _ = api.source_table_host(tri, weights, DEPTH)
    assert rec.shape[0] < 300
    cells = np.random.default_rng(2).integers(0, 17, size=300).astype(np.int32)
    U = np.random.default_rng(3).normal(size=(17, 3))
    span, hi, q, empty = _same(rec, cells, U, 0.5)
    assert not empty and _properties(hi)


@pytest.mark.parametrize("where", ["lead", "middle", "tail"])
@pytest.mark.parametrize("k", [3, 65, 257])
def test_triangles_without_inflow(k, where):
    rec, _, cells = _table(200 + k, k)
    mag = np.random.default_rng(k).uniform(0.5, 2.0, size=k)
    third = max(1, k // 3)
    dry = {"lead": slice(0, third), "middle": slice(third, 2 * third), "tail": slice(k - third, k)}[where]
    mag[dry] = np.where(np.arange(k)[dry] % 2 == 0, 0.0, -1.0)          # U == 0 and outward flow
    span, hi, q, empty = _same(rec, cells, _field(0, rec, mag), 0.25)
    assert not empty and _properties(hi)
    assert not q[dry].any() and not span[dry].any() and q[mag > 0].all()
    # a dry triangle is never picked: it shares its bound with its predecessor -- but for the draw w0 == 0 ahead of the first wet one
    draws = np.random.default_rng(1).integers(1, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)
    assert not np.isin(SP.pick(hi, draws), np.arange(k)[dry]).any()
    if where == "lead":
        assert SP.pick(hi, np.uint32(0)) == 0 and hi[0] == 0


def test_all_outward_flow_writes_nothing():
    rec, _, cells = _table(31, 65)
    U = _field(0, rec, -np.ones(65))
    lib = L.load()
    span, hi, q = np.full(65, 7.5), np.full(65, 77, np.uint32), np.full(65, 777, np.uint64)
    empty = C.c_int32(5)
    st = lib.cpf_source_flux_host(rec.ctypes.data, 65, cells.ctypes.data, 65, U.ctypes.data, 65, 0.5, span.ctypes.data, hi.ctypes.data,
                                  q.ctypes.data, C.byref(empty))
    assert st == L.CPF_OK and empty.value == 1
    assert (span == 7.5).all() and (hi == 77).all() and (q == 777).all()
    assert IF.flux(rec, cells, U, 0.5)[3] is True
    assert api.source_flux_host(rec, cells, np.zeros((65, 3)), 0.5)[3] is True
    # nullable outputs
    st = lib.cpf_source_flux_host(rec.ctypes.data, 65, cells.ctypes.data, 65, (-U).ctypes.data, 65, 0.5, None, None, None, C.byref(empty))
    assert st == L.CPF_OK and empty.value == 0


@pytest.mark.parametrize("bad", [(np.nan, 1.0, 1.0), (np.inf, 0.0, 0.0), (-np.inf, np.inf, 0.0), (1e308, 1e308, 1e308)])
def test_nan_and_inf_in_one_cell(bad):
    rec, _, cells = _table(41, 64)
    U = _field(0, rec, np.ones(64))
    U[20] = bad
    span, hi, q, empty = _same(rec, cells, U, 2.0)
    assert not empty and _properties(hi)
    assert np.isfinite(span).all()
    if not np.isfinite(np.dot(np.asarray(bad), rec[20, 9:12])) or np.isinf(bad[0]) or np.isnan(bad[0]):
        assert q[20] == 0 and span[20] == 0.0               # not finite: counts as 0


def test_weights_spread_over_2_to_the_45():
    rec, _, cells = _table(51, 257)
    mag = 2.0 ** (-45.0 * np.random.default_rng(4).random(257))
    span, hi, q, empty = _same(rec, cells, _field(0, rec, mag), 1.0)
    assert not empty and _properties(hi)
    assert (q == 0).any() and (q > 0).sum() > 100 and span.all()        # inflow everywhere, yet some shares are below one quantum


@pytest.mark.parametrize("scale", [1e300, 1e-300])
def test_huge_and_tiny_fields(scale):
    # triangles of edge 1e-6: areas near 1e-14, so that U * 1e-300 gives a SUBNORMAL wmax
    rec, _, cells = _table(61, 65, scale=1e-5)
    U = _field(3, rec) * scale
    span, hi, q, empty = _same(rec, cells, U, 1.0)
    assert not empty and _properties(hi)
    area = IF.lengths(rec) / 2.0
    wmax = (area * np.maximum((U * rec[:, 9:12]).sum(1), 0.0)).max()
    if scale < 1.0:
        assert 0.0 < wmax < 2.2250738585072014e-308
    else:
        assert wmax > 1e280 and np.isfinite(wmax)
    assert int(q.max()) >= 2 ** 31


def test_two_million_equal_triangles_round_the_conversions():
    """2^21 + 3 triangles of area 1/2 under un = 2 - 2^-29 - 2^-31: every q is 2^32 - 5, Q passes 2^53 with odd values, so
    (double)Q_k rounds"""
    k = 2 ** 21 + 3
    tri = np.zeros((k, 3, 3))
    tri[:, 1, 0] = 1.0
    tri[:, 2, 1] = 1.0
    rec, _ = api.source_table_host(tri, None, (0.0, 0.0))
    assert rec.shape[0] == k and (rec[:, 9:12] == [0.0, 0.0, -1.0]).all()
    cells = np.zeros(k, np.int32)
    U = np.array([[0.0, 0.0, -(2.0 - 2.0 ** -29 - 2.0 ** -31)]])
    span, hi, q, empty = _same(rec, cells, U, 0.0)
    assert not empty and (q == 2 ** 32 - 5).all()
    Q = np.cumsum(q, dtype=np.uint64)
    assert int(Q[-1]) > 2 ** 53 and (Q.astype(np.float64).astype(np.uint64) != Q).any()
    assert int(hi[-1]) == 0xFFFFFFFF and np.all(hi[1:] >= hi[:-1])


# seed 1: chosen so that the check holds on the CPU (it is deterministic: the picks are a pure function of seed, id and epoch)
SHARE_SEED = 1


def test_share_of_the_picks_is_the_share_of_the_quanta():
    rec, _, cells = _table(71, 40)
    mag = np.random.default_rng(8).uniform(0.1, 3.0, size=40)
    mag[[5, 17]] = 0.0
    _, hi, q, empty = _same(rec, cells, _field(0, rec, mag), 0.0)
    assert not empty
    n = 2 ** 20
    picks = api.source_picks_host(SHARE_SEED, None, 0, hi, n=n)
    count = np.bincount(picks, minlength=40)
    p = q.astype(np.float64) / float(q.sum())
    sd = np.sqrt(n * p * (1.0 - p))
    dev = np.abs(count - n * p)
    print("largest deviation in standard deviations:", float((dev[sd > 0] / sd[sd > 0]).max()))
    assert count[5] == 0 and count[17] == 0
    assert np.all(dev <= 5.0 * sd)


def test_refusals():
    rec, _, cells = _table(81, 5)
    U = _field(0, rec, np.ones(5))
    lib = L.load()
    empty = C.c_int32(0)

    def call(rec_=rec, k=5, cells_=cells, nt=5, U_=U, nc=5, s=0.5, e=C.byref(empty)):
        return lib.cpf_source_flux_host(None if rec_ is None else rec_.ctypes.data, k, None if cells_ is None else cells_.ctypes.data, nt,
                                        None if U_ is None else U_.ctypes.data, nc, s, None, None, None, e)

    assert call() == L.CPF_OK
    assert call(rec_=None) == L.CPF_ERR_ARG
    assert call(cells_=None) == L.CPF_ERR_ARG
    assert call(U_=None) == L.CPF_ERR_ARG
    assert call(e=None) == L.CPF_ERR_ARG
    assert call(k=0) == L.CPF_ERR_ARG and call(k=2 ** 24 + 1) == L.CPF_ERR_ARG
    assert call(nt=4) == L.CPF_ERR_ARG                                  # column 14 of the last record is 4: beyond nTriangles
    assert call(nt=0) == L.CPF_ERR_ARG and call(nc=0) == L.CPF_ERR_ARG
    assert call(nc=4) == L.CPF_ERR_ARG                                  # cell 4 is not in [0, 4)
    assert call(cells_=np.array([0, 1, -1, 3, 4], np.int32)) == L.CPF_ERR_ARG
    for s in (-1e-300, np.nan, np.inf):
        assert call(s=s) == L.CPF_ERR_ARG
    with pytest.raises(L.CpfError) as e:
        api.source_flux_host(rec, cells, U, -1.0)
    assert e.value.status == L.CPF_ERR_ARG
