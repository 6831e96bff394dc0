"""float64 numpy oracle of the hubness corrections (ops.hub_*, evaluation.hubness_*): the definitions, written as
they are stated.

  inverted softmax:  b[j] = (1 / beta) log sum_q exp(beta S_bank[q, j]),  a[i] = (1 / beta) log sum_q exp(beta S[i, q])
  CSLS:              b[j] = 0.5 * mean of the k largest S_bank[., j],      a[i] = 0.5 * mean of the k largest S[i, .]
                     (the k largest in the ranker's order: NaN as +inf, ties to the higher index; the mean is the float64 sum of the
                     k values, added best first one at a time, divided by k)
  adjusted matrix:   S'[i, j] = dtype((double(S[i, j]) - a[i]) - b[j])

The log-sum-exp is taken with the maximum shift in extended precision (numpy's longdouble: 64 mantissa bits on x86) and rounded
once, so it is exact to an ulp of float64; where longdouble is no wider than double the shifted terms are summed with math.fsum.
Special values as np.logaddexp.reduce gives them: -inf adds nothing, only -inf (or nothing) gives -inf, a +inf gives +inf, a NaN
gives NaN."""
import math

import numpy as np

import topk_oracle as T

_WIDE = np.finfo(np.longdouble).eps < 1e-18


def lse(x, beta):
    """(1 / beta) log sum exp(beta x) of a 1-D array, float64."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if np.isnan(x).any():
        return float('nan')
    if np.isposinf(x).any():
        return float('inf')
    if x.size == 0 or np.isneginf(x).all():
        return float('-inf')
    m = x.max()
    if _WIDE:
        d = np.longdouble(beta) * (x.astype(np.longdouble) - np.longdouble(m))
        s = np.sum(np.sort(np.exp(d)))                     # ascending: small terms first
        return float(np.longdouble(m) + np.log(s) / np.longdouble(beta))
    s = math.fsum(math.exp(beta * (float(v) - m)) if v != -np.inf else 0.0 for v in x)
    return m + math.log(s) / beta


def lse_rows(S, beta):
    return np.array([lse(r, beta) for r in np.asarray(S)], dtype=np.float64)


def lse_cols(S, beta):
    return lse_rows(np.asarray(S).T, beta)


def list_mean(vals, k):
    """0.5 * mean of the first k entries of every best-first list: an explicit float64 sum, best first, one at a time."""
    out = np.empty(len(vals), dtype=np.float64)
    for r, v in enumerate(np.asarray(vals)):
        s = np.float64(v[0])
        for x in v[1:k]:
            s = s + np.float64(x)
        out[r] = np.float64(0.5) * (s / np.float64(k))
    return out


def csls_rows(S, k):
    with np.errstate(invalid='ignore'):
        return list_mean(T.topk_rows(np.asarray(S), k)[1], k)


def csls_cols(S, k):
    return csls_rows(np.ascontiguousarray(np.asarray(S).T), k)


def vectors(S, method, k=10, beta=20.0, S_a=None, S_b=None):
    """(a, b).  Bank `self`: both from S.  External bank: a from S_a (gallery images x bank captions, row statistics), b from S_b
    (bank images x gallery captions, column statistics)."""
    S_a = S if S_a is None else S_a
    S_b = S if S_b is None else S_b
    if method == 'invsoftmax':
        return lse_rows(S_a, beta), lse_cols(S_b, beta)
    assert method == 'csls'
    return csls_rows(S_a, k), csls_cols(S_b, k)


def adjust(S, a=None, b=None):
    S = np.asarray(S)
    a = np.zeros(S.shape[0]) if a is None else np.asarray(a, dtype=np.float64)
    b = np.zeros(S.shape[1]) if b is None else np.asarray(b, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return ((S.astype(np.float64) - a[:, None]) - b[None, :]).astype(S.dtype)


def ranks(S, im_div=5):
    """Argsort ranker for both directions, the ranker's order (larger first, the higher index on ties, NaN as +inf, -0.0 == +0.0):
    -> (i2t_rank, i2t_top1, t2i_rank, t2i_top1), float64 like cal_recall's."""
    S = np.asarray(S)
    ni, nc = S.shape
    order = np.argsort(T.canon(S), axis=1, kind='stable')[:, ::-1]
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.arange(nc)[None, :].repeat(ni, 0), 1)
    i_rank = np.array([pos[i, im_div * i:im_div * (i + 1)].min() for i in range(ni)], dtype=np.float64)
    i_top = order[:, 0].astype(np.float64)
    order_t = np.argsort(T.canon(np.ascontiguousarray(S.T)), axis=1, kind='stable')[:, ::-1]
    t_rank = np.array([int(np.nonzero(order_t[j] == j // im_div)[0][0]) for j in range(nc)], dtype=np.float64)
    t_top = order_t[:, 0].astype(np.float64)
    return i_rank, i_top, t_rank, t_top


def r_at_1(rank):
    return 100.0 * float(np.mean(np.asarray(rank) < 1))


def planted_hubs(seed):
    """The planted-hub similarity matrix of the issue's recipe: 96 images x 480 captions, a tenth of the captions and of the
    images lifted by a constant along their column / row."""
    rng = np.random.default_rng(seed)
    Ni, D, Nc = 96, 16, 480
    im = rng.standard_normal((Ni, D))
    im /= np.linalg.norm(im, axis=1, keepdims=True)
    cap = np.repeat(im, 5, 0) + 0.6 * rng.standard_normal((Nc, D)) / np.sqrt(D)
    cap /= np.linalg.norm(cap, axis=1, keepdims=True)
    S0 = im @ cap.T
    col = 0.35 * np.abs(rng.standard_normal(Nc)) * (rng.random(Nc) < 0.1)
    row = 0.35 * np.abs(rng.standard_normal(Ni)) * (rng.random(Ni) < 0.1)
    return S0 + col[None, :] + row[:, None]
