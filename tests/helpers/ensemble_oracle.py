"""numpy statement of ensemble reranking (itr_rerank_fuse_lists): the float64 mean of M members' scores on K-lists, and the lists in
the float64 ranker's order under it."""
import numpy as np


def fuse(idx, vals):
    """idx int [n, K] candidates in coarse order; vals float32 [M, n, K] (or a sequence of M [n, K]) member scores.
    fused = (float64(vals[0]) + float64(vals[1]) + ...) / float64(M), added in member order.  Order of a list: larger fused score
    first with -0.0 == +0.0 and NaN as +inf, the higher index on exact ties, the lower old position among equal (index, score).
    -> (idx_sorted [n, K], fused_sorted float64 [n, K], vals_sorted float32 [M, n, K], perm int32 [n, K])."""
    idx = np.asarray(idx)
    vals = np.stack([np.asarray(v, dtype=np.float32) for v in vals])
    M, n, K = vals.shape
    assert idx.shape == (n, K)
    with np.errstate(invalid='ignore'):
        acc = vals[0].astype(np.float64)
        for m in range(1, M):
            acc = acc + vals[m].astype(np.float64)
        fused = acc / np.float64(M)
        c = fused + 0.0
    c = np.where(np.isnan(c), np.inf, c)
    pos = np.arange(K)
    perm = np.empty((n, K), dtype=np.int32)
    for q in range(n):
        perm[q] = np.lexsort((pos, -idx[q].astype(np.int64), -c[q]))
    p64 = perm.astype(np.int64)
    return (np.take_along_axis(idx, p64, 1), np.take_along_axis(fused, p64, 1),
            np.take_along_axis(vals, np.broadcast_to(p64, vals.shape), 2), perm)
