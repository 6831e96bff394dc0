"""GPU: the hubness corrections (csrc/hubness.hip; ops.hub_lse_fold / hub_lse_cols / hub_list_mean / hub_adjust,
evaluation.hubness_vectors / hubness_bank_vectors / hubness_adjust) against the float64 numpy oracle of
tests/helpers/hubness_oracle.py.

Tolerance of a log-sum-exp: 1e-10 * max(1, |want|), derived, not measured: a shifted float64 sum of n <= 1e4 positive terms, with a
1-ulp exp and a rounded beta x of magnitude <= 1e4, has a relative error around 1e-12 in the sum, under 3e-12 in LSE / beta at
beta = 0.5; the bound leaves a factor of about 30.  Special values (-inf, +inf, NaN) match exactly.  List means and the adjusted
matrix are bit-exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hubness_oracle as H        # noqa: E402

from itr_amd import ops                          # noqa: E402
from itr_amd.metricmodule import evaluation      # noqa: E402

pytestmark = pytest.mark.gpu
INF = float('inf')
TOL = 1e-10


def _check_lse(got, want, what):
    """Special values exactly, finite ones within TOL * max(1, |want|) -> the largest error in units of that bound."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.isinf(got[~inf & ~np.isnan(want)]).any(), what
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    print("%s: max LSE error %.3g (bound %g)" % (what, err.max(), TOL))
    assert err.max() <= TOL, (what, err.max())
    return float(err.max())


def _matrix(seed, n, nc, scale, f64, specials):
    rng = np.random.default_rng(seed)
    S = scale * rng.uniform(-1.0, 1.0, (n, nc))
    if specials:                       # needs n, nc >= 8
        S[rng.random((n, nc)) < 0.02] = -INF           # scattered
        S[:, 5] = -INF                                 # a column and a row of only -inf
        S[3, :] = -INF
        S[1, 2] = INF
        S[n - 2, nc - 1] = np.nan
    return S.astype(np.float64 if f64 else np.float32)


def _device_view(S, pad, offset, dev):
    """S on the device inside a larger buffer: leading dimension Nc + pad, and for `offset` a view that starts one element into the
    allocation (4-byte aligned for float32)."""
    n, nc = S.shape
    ld = nc + pad
    flat = torch.full((n * ld + offset + 8,), 7.25, device=dev, dtype=torch.from_numpy(S).dtype)   # padding that would show in a sum
    view = flat[offset:offset + n * ld].view(n, ld)[:, :nc]
    view.copy_(torch.from_numpy(S))
    if offset:
        assert view.data_ptr() % 16 != 0
    return view


# n_rows, Nc, ldS - Nc, float64, beta, scale, one-element offset, special values.  Every value of the issue's table appears; the two
# VEC rows add what the 16-byte path needs (float32: ldS % 4 == 0 with full 256-column strips; float64: ldS even).
FOLD_CASES = [
    (1, 1, 0, False, 20.0, 1.0, False, False),
    (2, 3, 3, True, 0.5, 50.0, False, False),
    (63, 63, 0, False, 200.0, 50.0, False, False),
    (64, 64, 3, True, 20.0, 1.0, False, False),
    (65, 65, 0, False, 0.5, 1.0, True, False),
    (300, 257, 3, False, 200.0, 50.0, False, True),
    (300, 1031, 0, True, 20.0, 50.0, False, True),
    (63, 1031, 3, True, 200.0, 1.0, False, True),
    (65, 1031, 1, False, 20.0, 50.0, False, True),
    (64, 257, 3, False, 0.5, 1.0, True, True),
]


@pytest.mark.parametrize("n,nc,pad,f64,beta,scale,offset,specials", FOLD_CASES)
def test_fold_matches_the_oracle(dev, n, nc, pad, f64, beta, scale, offset, specials):
    S = _matrix(n * 1000 + nc, n, nc, scale, f64, specials)
    view = _device_view(S, pad, int(offset), dev)
    row_lse, state = ops.hub_lse_fold(view, beta)
    col_lse = ops.hub_lse_cols(state, beta)
    _check_lse(row_lse, H.lse_rows(S, beta), "rows %dx%d" % (n, nc))
    _check_lse(col_lse, H.lse_cols(S, beta), "cols %dx%d" % (n, nc))
    if specials:
        assert row_lse[3].item() == -INF and col_lse[5].item() == -INF and row_lse[1].item() == INF and col_lse[2].item() == INF
        assert torch.isnan(row_lse[n - 2]).item() and torch.isnan(col_lse[nc - 1]).item()
        assert state[5, 0].item() == 0.0                 # an empty column stays the empty state


@pytest.fixture(scope="module")
def part_case():
    S = _matrix(42, 300, 257, 50.0, False, True)
    return S, H.lse_rows(S, 20.0), H.lse_cols(S, 20.0)


def _fold_in_blocks(Sd, block, beta, state=None):
    rows = []
    for i0 in range(0, Sd.shape[0], block):
        r, state = ops.hub_lse_fold(Sd[i0:i0 + block], beta, state=state)
        rows.append(r)
    return torch.cat(rows), state


@pytest.mark.parametrize("block", [1, 7, 64, 300])
def test_fold_any_row_partition(dev, part_case, block):
    S, want_r, want_c = part_case
    Sd = torch.from_numpy(S).to(dev)
    rows, state = _fold_in_blocks(Sd, block, 20.0)
    _check_lse(rows, want_r, "rows, blocks of %d" % block)
    _check_lse(ops.hub_lse_cols(state, 20.0), want_c, "cols, blocks of %d" % block)


def test_fold_is_reproducible_and_starts_from_zero_bytes(dev, part_case):
    S, _, _ = part_case
    Sd = torch.from_numpy(S).to(dev)
    r1, s1 = _fold_in_blocks(Sd, 7, 20.0)
    r2, s2 = _fold_in_blocks(Sd, 7, 20.0)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    zero = torch.zeros(257 * 2 * 8, device=dev, dtype=torch.uint8).view(torch.float64).view(257, 2)
    r3, s3 = _fold_in_blocks(Sd, 7, 20.0, state=zero)
    assert s3 is zero and torch.equal(s3.view(torch.int64), s1.view(torch.int64)) and torch.equal(r3.view(torch.int64), r1.view(torch.int64))
    # "empty" is a sum of 0 whatever the second slot holds
    junk = torch.zeros(257, 2, device=dev, dtype=torch.float64)
    junk[:, 1] = 1e300
    _, s4 = _fold_in_blocks(Sd, 7, 20.0, state=junk)
    assert torch.equal(s4.view(torch.int64), s1.view(torch.int64))


def test_fold_one_direction_leaves_the_other_alone(dev, part_case):
    S, want_r, want_c = part_case
    Sd = torch.from_numpy(S).to(dev)
    _, state = ops.hub_lse_fold(Sd[:100], 20.0)
    before = state.clone()
    rows, same = ops.hub_lse_fold(Sd[100:], 20.0, state=state, cols=False)
    assert same is state and torch.equal(state.view(torch.int64), before.view(torch.int64))
    _check_lse(rows, want_r[100:], "rows only")
    none, state = ops.hub_lse_fold(Sd[100:], 20.0, state=state, rows=False)
    assert none is None
    _check_lse(ops.hub_lse_cols(state, 20.0), want_c, "cols only")
    r0, s0 = ops.hub_lse_fold(Sd, 20.0, cols=False)
    assert s0 is None and r0.shape == (300,)


def test_ops_refuse_bad_values(dev):
    S = torch.zeros(4, 8, device=dev)
    for beta in (0.0, -1.0, float('nan'), INF):
        with pytest.raises(ValueError, match="beta"):
            ops.hub_lse_fold(S, beta)
        with pytest.raises(ValueError, match="beta"):
            ops.hub_lse_cols(torch.zeros(8, 2, device=dev, dtype=torch.float64), beta)
    with pytest.raises(ValueError, match="state"):
        ops.hub_lse_fold(S, 1.0, state=torch.zeros(7, 2, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="2-D"):
        ops.hub_lse_fold(S[0], 1.0)
    with pytest.raises(ValueError):
        ops.hub_list_mean(S, 0)
    with pytest.raises(ValueError):
        ops.hub_list_mean(S, 9)
    with pytest.raises(NotImplementedError, match="ITR_TOPK_MAX"):
        ops.hub_list_mean(torch.zeros(4, 200, device=dev), 129)
    with pytest.raises(ValueError, match="a must be"):
        ops.hub_adjust(S, a=torch.zeros(5, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="b must be"):
        ops.hub_adjust(S, b=torch.zeros(8, device=dev, dtype=torch.float32))
    with pytest.raises(ValueError, match="alias"):
        big = torch.zeros(64, device=dev)
        ops.hub_adjust(big[:32].view(4, 8), out=big[4:36].view(4, 8))
    with pytest.raises(ValueError, match="larger than a side"):
        evaluation.hubness_vectors(np.zeros((4, 20)), 'csls', k=5)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("K", [1, 10, 128])
def test_list_mean_is_bit_exact(dev, f64, K):
    rng = np.random.default_rng(K + int(f64))
    S = rng.standard_normal((130, 300))
    S[rng.random(S.shape) < 0.05] = 0.5                # ties
    S[7, 9] = np.nan
    S = S.astype(np.float64 if f64 else np.float32)
    _, r_val, part = ops.topk_lists(torch.from_numpy(S).to(dev), K)
    _, c_val = ops.topk_merge_cols([part], K)
    for vals in (r_val, c_val):
        host = vals.cpu().numpy()
        for k in sorted({1, K}):
            got = ops.hub_list_mean(vals, k).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(H.list_mean(host, k))), (K, k)
            # a narrower view of the same lists: the row stride stays K
            got = ops.hub_list_mean(vals[:, :k], k).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(H.list_mean(host, k))), (K, k)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("n,nc", [(1, 1), (65, 257), (300, 1031)])
def test_adjust_is_bit_exact(dev, f64, n, nc):
    rng = np.random.default_rng(n + nc)
    S = rng.uniform(-1.0, 1.0, (n, nc))
    if n > 1:
        S[rng.random(S.shape) < 0.01] = np.nan
        S[0, 1], S[1, 0], S[2, 2] = INF, -INF, -0.0
    S = S.astype(np.float64 if f64 else np.float32)
    a, b = rng.uniform(-0.5, 0.5, n) * 1.0000001, rng.uniform(-0.5, 0.5, nc) / 3.0
    Sd, ad, bd = torch.from_numpy(S).to(dev), torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)

    def same(got, want):
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert np.array_equal(_bits(got)[fin], _bits(want)[fin])
    same(ops.hub_adjust(Sd, a=ad), H.adjust(S, a, None))
    same(ops.hub_adjust(Sd, b=bd), H.adjust(S, None, b))
    same(ops.hub_adjust(Sd, ad, bd), H.adjust(S, a, b))
    same(ops.hub_adjust(Sd), S)
    # out of place into a wider buffer (ldo != ldS); the padding is left alone
    wide = torch.full((n, nc + 5), 3.0, device=dev, dtype=Sd.dtype)
    out = ops.hub_adjust(Sd, ad, bd, out=wide[:, :nc])
    assert out.data_ptr() == wide.data_ptr() and bool((wide[:, nc:] == 3.0).all())
    same(wide[:, :nc], H.adjust(S, a, b))
    # from a strided view (ldS != ldo)
    src = torch.zeros(n, nc + 3, device=dev, dtype=Sd.dtype)
    src[:, :nc] = Sd
    same(ops.hub_adjust(src[:, :nc], ad, bd), H.adjust(S, a, b))
    # in place
    work = Sd.clone()
    assert ops.hub_adjust(work, ad, bd, out=work) is work
    same(work, H.adjust(S, a, b))


@pytest.mark.parametrize("f64", [False, True])
def test_planted_hubs_end_to_end(dev, f64):
    S = H.planted_hubs(0).astype(np.float64 if f64 else np.float32)
    raw = H.r_at_1(H.ranks(S)[0])
    assert raw <= 70.0
    for method in ("invsoftmax", "csls"):
        a, b = evaluation.hubness_vectors(S, method, k=10, beta=20.0)
        want_a, want_b = H.vectors(S, method, k=10, beta=20.0)
        _check_lse(a, want_a, "%s a" % method)
        _check_lse(b, want_b, "%s b" % method)
        adj = evaluation.hubness_adjust(S, a, b)
        want = H.adjust(S, a, b)
        assert adj.dtype == S.dtype and np.array_equal(_bits(adj), _bits(want))
        res = evaluation.cal_recall(adj)
        i_rank, i_top, t_rank, t_top = H.ranks(want)
        assert np.array_equal(res['i2t_ranks'], i_rank) and np.array_equal(res['i2t_top1'], i_top)
        assert np.array_equal(res['t2i_ranks'], t_rank) and np.array_equal(res['t2i_top1'], t_top)
        assert res['i2t_r1'] >= 90.0 and abs(res['i2t_r1'] - H.r_at_1(i_rank)) < 1e-9, (method, res['i2t_r1'])


class _Pooled(object):
    """A pooled toy model: evaluation._cal_fun finds `sim_enc`, the inner product of the embeddings on the GPU."""
    def __init__(self):
        self.config = {'name': 'VSE'}
        self.criterion = None

    @staticmethod
    def sim_enc(im, s, lens, config):
        return ops.cosine_scores(im, s)


def _dyadic_embs(seed, n_img, D=16):
    """Embeddings in multiples of 1/8: every inner product is exact in float32 whatever the order of the sum, so a block scores
    the very numbers the full matrix holds, however either is tiled.  encode_data's layout: image rows repeated per caption."""
    rng = np.random.default_rng(seed)
    img = rng.integers(-8, 9, (n_img, D)).astype(np.float32) / 8
    cap = (np.repeat(img, 5, 0) + rng.integers(-4, 5, (n_img * 5, D)).astype(np.float32) / 8) / 4
    return np.repeat(img, 5, 0), cap


@pytest.mark.parametrize("members", [1, 2])
@pytest.mark.parametrize("method", ["invsoftmax", "csls"])
def test_bank_equal_to_the_gallery_reproduces_self(dev, members, method):
    embs = [_dyadic_embs(10 + m, 96) for m in range(members)]
    models = [(_Pooled(), img, cap, None, 1 << 20) for img, cap in embs]
    sims = sum(evaluation.cal_sims(m[0], m[1][::5], m[2], shard_size=1 << 20) for m in models) / members
    want_a, want_b = evaluation.hubness_vectors(sims, method, k=10, beta=2.0)
    a, b = evaluation.hubness_bank_vectors(models, [(img, cap, None) for img, cap in embs], method, k=10, beta=2.0, block_rows=37)
    _check_lse(a, want_a, "bank a")
    _check_lse(b, want_b, "bank b")
    oa, ob = H.vectors(sims, method, k=10, beta=2.0)
    _check_lse(a, oa, "bank a vs oracle")
    _check_lse(b, ob, "bank b vs oracle")


def test_bank_is_never_materialised(dev):
    g_img, g_cap = _dyadic_embs(1, 128)                  # gallery: 128 images, 640 captions
    q_img, q_cap = _dyadic_embs(2, 4096)                 # bank: 4 096 images, 20 480 captions
    models = [(_Pooled(), g_img, g_cap, None, 1 << 20)]
    matrix_bytes = 4096 * 640 * 4                        # bank images x gallery captions (= gallery images x bank captions), fp32
    ops.cosine_scores(torch.zeros(4, 16, device=dev), torch.zeros(4, 16, device=dev))      # code objects loaded
    for method in ("invsoftmax", "csls"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a, b = evaluation.hubness_bank_vectors(models, [(q_img, q_cap, None)], method, k=10, beta=2.0, block_rows=100)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        print("%s: peak growth %d bytes, a bank-sized matrix %d" % (method, grown, matrix_bytes))
        assert grown < matrix_bytes // 2, (method, grown)
        assert a.shape == (128,) and b.shape == (640,) and np.isfinite(a).all() and np.isfinite(b).all()
        # spot check against the oracle on a slice of the (here affordable) matrices
        S_b = q_img[::5].astype(np.float64) @ g_cap[:7].astype(np.float64).T
        S_a = g_img[::5][:3].astype(np.float64) @ q_cap.astype(np.float64).T
        oa, ob = H.vectors(None, method, k=10, beta=2.0, S_a=S_a, S_b=S_b)
        _check_lse(a[:3], oa, "big bank a")
        _check_lse(b[:7], ob, "big bank b")
