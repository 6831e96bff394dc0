"""GPU: ops.search_topk (csrc/search.hip), the fused score + top-K pass of a few queries over a gallery.
(a) integer-valued inputs, where every fp32 summation order is exact, against a numpy sort of the float64 product;
(b) random floats against the project's own path, bit for bit: topk_lists(cosine_scores(Q, G)) and, roles swapped, the merged column
    lists of cosine_scores(G, Q);
(c) the seams: query counts around the instances (4 / 16 / 64), gallery sizes around the tiles, D around the chunk of 32 and the
    16-byte loads, K up to 128 and beyond the gallery, every slab count, strided and unaligned views, row0 > 0, gallery shards;
(d) worst cases for the selection: ascending scores, all rows equal, zero queries, NaN and +-inf rows;
(e) a float64 bound that does not lean on the project's GEMM.
All list comparisons are exact: indices equal, values equal as uint32 bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from topk_oracle import order_key32, topk_rows   # noqa: E402

from itr_amd import ops                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLABS = (0, 1, 2, 7, ops.SEARCH_MAX_SLABS)
ROW0 = 1000003


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def search(Qd, Gd, k, row0=0, n_slabs=0):
    idx, val, (key, val2) = ops.search_topk(Qd, Gd, k, row0=row0, n_slabs=n_slabs)
    assert val2 is val
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), key.cpu().numpy().view(np.uint64)


def expected(S, k, row0=0):
    """the lists of a score matrix S [Q, N] (any float type) -> idx int64 [Q, k] (-1 past N), val float32 [Q, k] (0 there), keys"""
    nq, n = S.shape
    idx = np.full((nq, k), -1, np.int64)
    val = np.zeros((nq, k), np.float32)
    key = np.zeros((nq, k), np.uint64)
    m = min(n, k)
    if m:
        i, v = topk_rows(S, m)
        idx[:, :m] = i + row0
        val[:, :m] = v.astype(np.float32)
        key[:, :m] = (order_key32(val[:, :m]) << np.uint64(32)) | (i.astype(np.uint64) + np.uint64(row0))
    return idx, val, key


def check(got, want, what):
    gi, gv, gk = got
    wi, wv, wk = want
    assert np.array_equal(gi.astype(np.int64), wi), what + ": indices"
    assert np.array_equal(bits(gv), bits(wv)), what + ": values"
    assert np.array_equal(gk, wk), what + ": keys"


def ints(rng, n, d, lo, hi):
    return rng.randint(lo, hi + 1, size=(n, d)).astype(np.float32)


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12).astype(np.float32)


# (Q, N, D, K): every Q, N, D and K of the seam lists at least once, K > N and K == N among them
EXACT = [(1, 1, 1, 1), (2, 15, 4, 10), (15, 16, 36, 100), (16, 17, 100, 128), (17, 63, 1023, 1), (33, 64, 1024, 10), (64, 65, 2048, 100),
         (1, 255, 36, 128), (2, 257, 4, 100), (16, 1000, 100, 128), (17, 4099, 36, 100), (64, 20011, 36, 128), (1, 20011, 1024, 10),
         (16, 4099, 2048, 1), (33, 1000, 1023, 10), (64, 100, 4, 100), (3, 128, 1, 128), (15, 10, 100, 10)]


@pytest.mark.parametrize("nq,n,d,k", EXACT)
def test_exact_integer_oracle_every_slab_count(nq, n, d, k):
    rng = np.random.RandomState(nq * 7 + n)
    Q, G = ints(rng, nq, d, -3, 3), ints(rng, n, d, -3, 3)
    want = expected(Q.astype(np.float64) @ G.astype(np.float64).T, k, ROW0)
    Qd, Gd = torch.from_numpy(Q).to(DEV), torch.from_numpy(G).to(DEV)
    for s in SLABS:
        check(search(Qd, Gd, k, ROW0, s), want, "n_slabs=%d" % s)


@pytest.mark.parametrize("nq,n,k", [(1, 257, 10), (16, 4099, 100), (64, 1000, 128), (17, 65, 100)])
def test_ties_are_the_rule(nq, n, k):
    rng = np.random.RandomState(n)
    Q, G = ints(rng, nq, 16, -1, 1), ints(rng, n, 16, -1, 1)
    want = expected(Q.astype(np.float64) @ G.astype(np.float64).T, k)
    Qd, Gd = torch.from_numpy(Q).to(DEV), torch.from_numpy(G).to(DEV)
    for s in SLABS:
        check(search(Qd, Gd, k, 0, s), want, "n_slabs=%d" % s)


FLOATS = [(1, 1000, 1024, 10), (2, 4099, 100, 100), (16, 4099, 1024, 100), (17, 257, 1023, 10), (64, 20011, 100, 128), (33, 1000, 36, 1),
          (15, 255, 2048, 128)]


@pytest.mark.parametrize("nq,n,d,k", FLOATS)
def test_bits_of_the_matrix_path(nq, n, d, k):
    rng = np.random.RandomState(n + d)
    Qd, Gd = torch.from_numpy(unit(rng, nq, d)).to(DEV), torch.from_numpy(unit(rng, n, d)).to(DEV)
    ri, rv, _ = ops.topk_lists(ops.cosine_scores(Qd, Gd), k, cols=False)
    part = ops.topk_lists(ops.cosine_scores(Gd, Qd), k, rows=False)[2]
    ci, cv = ops.topk_merge_cols([part], k)
    torch.cuda.synchronize()
    for s in (0, 1, 7):
        gi, gv, _ = search(Qd, Gd, k, 0, s)
        assert np.array_equal(gi, ri.cpu().numpy()) and np.array_equal(bits(gv), bits(rv.cpu().numpy())), "rows of cosine_scores(Q, G)"
        assert np.array_equal(gi, ci.cpu().numpy()) and np.array_equal(bits(gv), bits(cv.cpu().numpy())), "columns of cosine_scores(G, Q)"


@pytest.mark.parametrize("nq,n,d,k", [(2, 257, 36, 10), (16, 1000, 100, 100), (33, 255, 1023, 128), (64, 4099, 1024, 10)])
def test_strided_and_unaligned_views(nq, n, d, k):
    rng = np.random.RandomState(d)
    Q, G = ints(rng, nq, d, -3, 3), ints(rng, n, d, -3, 3)
    want = expected(Q.astype(np.float64) @ G.astype(np.float64).T, k)
    Qd, Gd = torch.from_numpy(Q).to(DEV), torch.from_numpy(G).to(DEV)
    # leading dimension > D (a multiple of 4: the 16-byte path where D allows, and one that is not)
    for pad in (4, 3):
        ld = (d + 3) // 4 * 4 + pad
        gb = torch.full((n, ld), 5.0, device=DEV)
        gb[:, :d] = Gd
        qb = torch.full((nq, ld + 4), -5.0, device=DEV)
        qb[:, :d] = Qd
        for s in (0, 2):
            check(search(qb[:, :d], gb[:, :d], k, 0, s), want, "ld = %d" % ld)
    # both bases one float off a 16-byte boundary
    gflat = torch.full((n * d + 1,), 5.0, device=DEV)
    qflat = torch.full((nq * d + 1,), 5.0, device=DEV)
    gflat[1:] = Gd.reshape(-1)
    qflat[1:] = Qd.reshape(-1)
    gv, qv = gflat[1:].view(n, d), qflat[1:].view(nq, d)
    assert gv.data_ptr() % 16 == 4 and qv.data_ptr() % 16 == 4
    for s in (0, 7):
        check(search(qv, gv, k, 0, s), want, "unaligned")


@pytest.mark.parametrize("nq,n,d,k", [(1, 4099, 36, 10), (17, 1000, 100, 128), (64, 20011, 36, 100), (16, 65, 4, 100)])
def test_gallery_shards_merge_to_the_whole(nq, n, d, k):
    rng = np.random.RandomState(nq)
    Qd, Gd = torch.from_numpy(unit(rng, nq, d)).to(DEV), torch.from_numpy(unit(rng, n, d)).to(DEV)
    wi, wv, _ = search(Qd, Gd, k, ROW0)
    for cuts in ((0, n // 3, n), (0, 1, n // 7, n // 2, n // 2 + 17 if n // 2 + 17 < n else n - 1, n)):
        parts = [ops.search_topk(Qd, Gd[a:b], k, row0=ROW0 + a)[2] for a, b in zip(cuts[:-1], cuts[1:])]
        mi, mv = ops.topk_merge_cols(parts, k)
        torch.cuda.synchronize()
        assert np.array_equal(mi.cpu().numpy(), wi) and np.array_equal(bits(mv.cpu().numpy()), bits(wv)), "%d shards" % len(parts)


@pytest.mark.parametrize("nq,k", [(1, 10), (16, 128), (64, 100)])
def test_worst_cases_for_the_selection(nq, k):
    n, d = 4099, 36
    rng = np.random.RandomState(k)
    # scores ascending along the gallery: every row beats the threshold (query = e_0 scaled, gallery column 0 ascending integers)
    Q = np.zeros((nq, d), np.float32)
    Q[:, 0] = np.arange(1, nq + 1)
    G = ints(rng, n, d, -3, 3)
    G[:, 0] = np.arange(n)
    cases = {"ascending": (Q, G), "all rows equal": (ints(rng, nq, d, -3, 3), np.tile(ints(rng, 1, d, -3, 3), (n, 1))),
             "zero queries": (np.zeros((nq, d), np.float32), ints(rng, n, d, -3, 3))}
    for name, (q, g) in cases.items():
        want = expected(q.astype(np.float64) @ g.astype(np.float64).T, k)
        qd, gd = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV)
        for s in (0, 1, 7):
            check(search(qd, gd, k, 0, s), want, "%s, n_slabs=%d" % (name, s))


@pytest.mark.parametrize("nq,k", [(2, 10), (17, 100)])
def test_nan_and_inf_rows_equal_the_matrix_path(nq, k):
    n, d = 1000, 100
    rng = np.random.RandomState(nq)
    Q, G = unit(rng, nq, d), unit(rng, n, d)
    G[17, 5] = np.nan
    G[500, 7] = np.inf
    G[777, 9] = -np.inf
    Qd, Gd = torch.from_numpy(Q).to(DEV), torch.from_numpy(G).to(DEV)
    ri, rv, _ = ops.topk_lists(ops.cosine_scores(Qd, Gd), k, cols=False)
    torch.cuda.synchronize()
    ri, rv = ri.cpu().numpy(), rv.cpu().numpy()
    for s in (0, 2):
        gi, gv, _ = search(Qd, Gd, k, 0, s)
        assert np.array_equal(gi, ri)
        assert np.array_equal(np.isnan(gv), np.isnan(rv))
        ok = ~np.isnan(rv)
        assert np.array_equal(bits(gv)[ok], bits(rv)[ok])
    assert np.isnan(rv).any(1).all() and (ri == 17).any(1).all()   # the NaN row is listed for every query: NaN ranks as +inf


@pytest.mark.parametrize("nq,n,d,k", [(1, 4099, 1024, 10), (16, 1000, 2048, 100), (64, 4099, 100, 128)])
def test_float64_bound_of_the_fmaf_chain(nq, n, d, k):
    rng = np.random.RandomState(n + nq)
    Q, G = unit(rng, nq, d), unit(rng, n, d)
    gi, gv, _ = search(torch.from_numpy(Q).to(DEV), torch.from_numpy(G).to(DEV), k)
    S64 = Q.astype(np.float64) @ G.astype(np.float64).T
    A64 = np.abs(Q.astype(np.float64)) @ np.abs(G.astype(np.float64)).T            # sum_k |q_k g_k|
    bound = 2.0 * d * 2.0 ** -24 * A64                                             # worst case of a length-D fp32 fmaf chain
    kth = np.sort(S64, axis=1)[:, ::-1][:, k - 1]
    got64 = np.take_along_axis(S64, gi.astype(np.int64), 1)
    b = np.take_along_axis(bound, gi.astype(np.int64), 1)
    assert (gi >= 0).all() and all(len(set(r)) == k for r in gi.tolist())
    assert (got64 >= kth[:, None] - b).all()
    assert (np.abs(gv.astype(np.float64) - got64) <= b).all()


def test_more_queries_than_the_limit_and_empty_inputs():
    G = torch.zeros(10, 8, device=DEV)
    with pytest.raises(NotImplementedError, match=str(ops.SEARCH_MAX_QUERIES)):
        ops.search_topk(torch.zeros(ops.SEARCH_MAX_QUERIES + 1, 8, device=DEV), G, 3)
    idx, val, (key, _) = ops.search_topk(torch.zeros(0, 8, device=DEV), G, 3)
    assert tuple(idx.shape) == (0, 3) and tuple(key.shape) == (0, 3)
    idx, val, (key, _) = ops.search_topk(torch.ones(5, 8, device=DEV), G[:0], 3)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -1).all() and (bits(val.cpu().numpy()) == 0).all() and (key.cpu().numpy() == 0).all()
