"""Numpy oracle of the top-K retrieval lists (evaluation.topk, ops.topk_lists / topk_merge_cols, evalpipe.finalize_topk).

The reference's list of a query is inds = np.argsort(sims[index])[::-1] (evaluation.py:169, :209); its first K entries in the
ranker's documented order are  np.argsort(canon(x), kind='stable')[::-1][:K],  canon mapping NaN -> +inf and -0.0 -> +0.0
(a stable ascending sort reversed: among equal scores the higher index comes first)."""
import numpy as np
import torch


def canon(x):
    x = np.array(x, copy=True)
    x[np.isnan(x)] = np.inf
    return x + x.dtype.type(0.0)          # -0.0 + 0.0 = +0.0


def topk_rows(S, k):
    """-> (idx int64 [n, k], scores [n, k] with their original bits)."""
    S = np.asarray(S)
    idx = np.argsort(canon(S), axis=1, kind='stable')[:, ::-1][:, :k]
    return idx.astype(np.int64), np.take_along_axis(S, idx, 1)


def topk_cols(S, k):
    return topk_rows(np.asarray(S).T, k)


def topk_all(S, k):
    """evaluation.topk's dict."""
    ri, rv = topk_rows(S, k)
    ci, cv = topk_cols(S, k)
    return {'i2t_topk': ri, 'i2t_topk_scores': rv, 't2i_topk': ci, 't2i_topk_scores': cv}


def order_key32(v):
    """score_key of rank_key.h on the canonical float32 score, as uint64."""
    u = canon(np.asarray(v, np.float32)).view(np.uint32).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), (~u) & np.uint64(0xffffffff), u | np.uint64(0x80000000))


def topk_lists(S, k, row0=0, rows=True, cols=True):
    """Twin of ops.topk_lists on a CPU float32 tensor: row lists and this block's partial column lists
    (key = score key << 32 | global row, key 0 / score 0 past the block's rows)."""
    Sn = S.numpy() if torch.is_tensor(S) else np.asarray(S, np.float32)
    n, nc = Sn.shape
    ri = rv = part = None
    if rows:
        i, v = topk_rows(Sn, k)
        ri, rv = torch.from_numpy(i.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(v))
    if cols:
        keys = np.zeros((nc, k), np.uint64)
        vals = np.zeros((nc, k), np.float32)
        m = min(k, n)
        if n:
            i, v = topk_cols(Sn, m)
            keys[:, :m] = (order_key32(v) << np.uint64(32)) | (i.astype(np.uint64) + np.uint64(row0))
            vals[:, :m] = v
        part = (torch.from_numpy(keys.view(np.int64)), torch.from_numpy(vals))
    return ri, rv, part


def topk_merge_cols(parts, k):
    """Twin of ops.topk_merge_cols: the k largest keys over all parts of every column (-1 / 0 where fewer)."""
    keys = np.concatenate([np.asarray(p[0]).view(np.uint64) for p in parts], 1)
    vals = np.concatenate([np.asarray(p[1]) for p in parts], 1)
    order = np.argsort(keys, axis=1, kind='stable')[:, ::-1][:, :k]
    kk = np.take_along_axis(keys, order, 1)
    vv = np.take_along_axis(vals, order, 1)
    idx = np.where(kk != 0, (kk & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    vv = np.where(kk != 0, vv, np.float32(0))
    return torch.from_numpy(idx), torch.from_numpy(vv)


def topk_exact_large(S, k):
    """The same lists for a large float32 matrix by partial selection on unique 64-bit keys (score key << 32 | index):
    a full argsort of 5 000 x 25 000 would take minutes."""
    def rows(M):
        n, m = M.shape
        key = (order_key32(M) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
        part = np.partition(key, m - k, axis=1)[:, m - k:]
        top = np.sort(part, axis=1)[:, ::-1]
        idx = (top & np.uint64(0xffffffff)).astype(np.int64)
        return idx, np.take_along_axis(M, idx, 1)
    ri, rv = rows(S)
    ci, cv = rows(np.ascontiguousarray(S.T))
    return ri, rv, ci, cv
