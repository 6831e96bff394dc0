"""GPU: SCAN scores of candidate lists (ops.scan_candidate_scores, csrc/scan_pairs.hip), the list re-ordering
(ops.rerank_lists, csrc/rerank.hip) and evaluation.rerank, against oracle/itr_oracle.py.  Tolerance: the project's 2e-5 absolute on
scores (test_kernels_gpu.py, test_edges_gpu.py); list orders, permutations and ranks exact."""
import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops
from itr_amd.metricmodule import evaluation

pytestmark = pytest.mark.gpu

NORMS = ['clipped_l2norm', 'l2norm', 'softmax', 'no_norm', 'clipped', 'l1norm', 'clipped_l1norm']
AGGS = ['LogSumExp', 'Mean', 'Max', 'Sum']
KS = [1, 10, 37, 128]
TOL = 2e-5


def make_set(seed, Ni, lens, D, R=36):
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    lens = np.asarray(lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = O.l2norm(torch.randn(Ni, R, D), -1)
    words = torch.randn(int(lens.sum()), D) * 0.5
    L = int(lens.max())
    cap = torch.zeros(len(lens), L, D)
    for c, (o, l) in enumerate(zip(off, lens)):
        cap[c, :l] = words[o:o + l]
    return rng, img, words, cap, off, lens


def lists(rng, n_q, n_t, K):
    """random lists with repeats inside a list"""
    cand = rng.randint(0, n_t, size=(n_q, K)).astype(np.int32)
    if K > 1:
        cand[:, -1] = cand[:, 0]
    return cand


def expected(S, cand, by):
    S = S.numpy()
    q = np.arange(cand.shape[0])[:, None]
    return S[cand, q] if by == 'caption' else S[q, cand]


def maxdiff(got, want):
    return float(np.abs(got.detach().cpu().double().numpy() - np.asarray(want, np.float64)).max()) if got.numel() else 0.0


RAGGED = [1, 16, 17, 64, 5, 13, 32, 33, 48, 49, 2, 9, 11, 27, 63, 8, 12, 15, 20, 31, 7, 3, 40, 14]


@pytest.mark.parametrize("by", ['caption', 'image'])
@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
@pytest.mark.parametrize("D", [32, 1024])
def test_oracle_parity(dev, D, xa, by):
    Ni = 13                                             # not a multiple of the kernel's block of 8 images
    rng, img, words, cap, off, lens = make_set(7 + D, Ni, RAGGED, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    n_q, n_t = (Nc, Ni) if by == 'caption' else (Ni, Nc)
    worst = 0.0
    for ni, norm in enumerate(NORMS):
        for ai, agg in enumerate(AGGS):
            S = O.xattn_score(img, cap, lens, xa, norm, agg)
            for K in (KS if (ni, ai) == (0, 0) else [KS[(ni + ai) % 4]]):
                cand = lists(rng, n_q, n_t, K)
                got = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(cand).to(dev), by, cross_attn=xa,
                                                raw_feature_norm=norm, agg_func=agg)
                assert got.shape == (n_q, K)
                err = maxdiff(got, expected(S, cand, by))
                worst = max(worst, err)
                print("parity D=%d %s by=%s %s %s K=%d: max|d| = %.3g" % (D, xa, by, norm, agg, K, err))
                assert err <= TOL, (D, xa, by, norm, agg, K, err)
    print("parity worst: %.3g" % worst)


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
def test_a_pairs_score_is_its_own(dev, xa):
    """The same pair scores the same bits in a shuffled list, in a subset, with the other captions' rows removed, and through
    either list direction."""
    Ni, D, K = 21, 256, 12
    rng, img, words, cap, off, lens = make_set(11, Ni, RAGGED, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    for norm, agg in (('clipped_l2norm', 'LogSumExp'), ('softmax', 'Mean'), ('l1norm', 'Max'), ('no_norm', 'Sum')):
        kw = dict(cross_attn=xa, raw_feature_norm=norm, agg_func=agg)
        cand = lists(rng, Nc, Ni, K)
        base = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(cand).to(dev), 'caption', **kw).cpu()
        # shuffled inside every list
        perm = np.stack([rng.permutation(K) for _ in range(Nc)])
        shuf = np.take_along_axis(cand, perm, 1)
        got = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(shuf).to(dev), 'caption', **kw).cpu()
        assert torch.equal(got, torch.from_numpy(np.take_along_axis(base.numpy(), perm, 1)))
        # a subset of every list (other blocking: 5 instead of 12 pairs per caption)
        got = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(np.ascontiguousarray(cand[:, 3:8])).to(dev), 'caption', **kw).cpu()
        assert torch.equal(got, base[:, 3:8])
        # the other captions' rows removed: captions 5..10 alone, in a plan of their own
        c0, c1 = 5, 11
        r0, r1 = int(off[c0]), int(off[c1 - 1] + lens[c1 - 1])
        sub_plan = ops.ScanPlan(off[c0:c1] - r0, lens[c0:c1], r1 - r0, dev)
        got = ops.scan_candidate_scores(img_d, words_d[r0:r1].contiguous(), sub_plan, torch.from_numpy(np.ascontiguousarray(cand[c0:c1])).to(dev),
                                        'caption', **kw).cpu()
        assert torch.equal(got, base[c0:c1])
        # the same pairs listed per image
        ci = lists(rng, Ni, Nc, K)
        by_img = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(ci).to(dev), 'image', **kw).cpu()
        back = np.zeros((Nc, Ni * K), np.int32)          # per caption: the images that listed it (padded with image 0)
        src = -np.ones((Nc, Ni * K), np.int64)
        fill = np.zeros(Nc, np.int64)
        for i in range(Ni):
            for k in range(K):
                c = ci[i, k]
                back[c, fill[c]], src[c, fill[c]] = i, i * K + k
                fill[c] += 1
        W = int(fill.max())
        by_cap = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(np.ascontiguousarray(back[:, :W])).to(dev), 'caption', **kw).cpu()
        m = src[:, :W] >= 0
        assert torch.equal(by_cap[torch.from_numpy(m)], by_img.reshape(-1)[torch.from_numpy(src[:, :W][m])])


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
def test_long_captions_and_refusals(dev, xa):
    Ni, D = 11, 64
    lens = [65, 7, 82, 96, 12, 64, 1]
    rng, img, words, cap, off, lens = make_set(5, Ni, lens, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    S = O.xattn_score(img, cap, lens, xa)
    for by, K in (('caption', 10), ('image', 5), ('image', 37)):
        n_q, n_t = (Nc, Ni) if by == 'caption' else (Ni, Nc)
        cand = lists(rng, n_q, n_t, K)
        got = ops.scan_candidate_scores(img_d, words_d, plan, torch.from_numpy(cand).to(dev), by, cross_attn=xa)
        err = maxdiff(got, expected(S, cand, by))
        print("long captions %s by=%s K=%d: max|d| = %.3g" % (xa, by, K, err))
        assert err <= TOL
    cand = torch.zeros(Nc, 3, dtype=torch.int32, device=dev)
    # 97 words
    l97 = np.asarray([5, 97], np.int32)
    p97 = ops.ScanPlan(np.asarray([0, 5], np.int64), l97, 102, dev)
    with pytest.raises(NotImplementedError):
        ops.scan_candidate_scores(img_d, torch.zeros(102, D, device=dev), p97, cand[:2], 'caption', cross_attn=xa)
    with pytest.raises(NotImplementedError):
        ops.scan_candidate_scores(torch.zeros(Ni, 35, D, device=dev), words_d, plan, cand, 'caption', cross_attn=xa)
    with pytest.raises(ValueError):
        ops.scan_candidate_scores(img_d, words_d, plan, cand, 'caption', cross_attn=xa, raw_feature_norm='bogus')
    with pytest.raises(ValueError):
        ops.scan_candidate_scores(img_d, words_d, plan, cand, 'caption', cross_attn=xa, agg_func='bogus')
    with pytest.raises(ValueError):
        ops.scan_candidate_scores(img_d, words_d, plan, cand, 'caption', cross_attn='bogus')
    for bad in (-1, Ni):
        c = cand.clone()
        c[2, 1] = bad
        with pytest.raises(ValueError):
            ops.scan_candidate_scores(img_d, words_d, plan, c, 'caption', cross_attn=xa)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scan_candidate_scores(img, words_d, plan, cand, 'caption', cross_attn=xa)
    # empty shapes
    assert ops.scan_candidate_scores(img_d, words_d, plan, cand[:, :0], 'caption', cross_attn=xa).shape == (Nc, 0)
    assert ops.scan_candidate_scores(img_d[:0], words_d, plan, torch.zeros(0, 4, dtype=torch.int32, device=dev), 'image', cross_attn=xa).shape == (0, 4)
    p0 = ops.ScanPlan(np.zeros(0, np.int64), np.zeros(0, np.int32), 0, dev)
    assert ops.scan_candidate_scores(img_d, words_d[:0], p0, torch.zeros(0, 4, dtype=torch.int32, device=dev), 'caption', cross_attn=xa).shape == (0, 4)


def np_rerank_order(idx, val):
    """rank_key's order stated in numpy: canonical score (-0.0 -> +0.0, NaN -> +inf) descending, then index descending, equal
    entries in their old order (lexsort is stable)."""
    v = val.astype(np.float32) + np.float32(0.0)
    v = np.where(np.isnan(v), np.float32(np.inf), v)
    return np.stack([np.lexsort((-idx[r].astype(np.int64), -v[r].astype(np.float64))) for r in range(idx.shape[0])])


@pytest.mark.parametrize("K", [1, 2, 10, 100, 128])
def test_rerank_lists(dev, K):
    rng = np.random.RandomState(K)
    n = 37
    idx = rng.randint(0, 50, size=(n, K)).astype(np.int32)          # duplicates
    val = rng.randint(-3, 4, size=(n, K)).astype(np.float32) * 0.25   # exact ties
    val[rng.rand(n, K) < 0.1] = -0.0
    val[rng.rand(n, K) < 0.1] = 0.0
    val[3 % n, K // 2] = np.nan
    if K > 1:
        idx[5, 1], val[5, 1] = idx[5, 0], val[5, 0]                  # the same candidate with the same score twice
    io, vo, po = ops.rerank_lists(torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev))
    perm = np_rerank_order(idx, val)
    assert np.array_equal(po.cpu().numpy(), perm)
    assert np.array_equal(io.cpu().numpy(), np.take_along_axis(idx, perm, 1))
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), np.take_along_axis(val, perm, 1).view(np.uint32))


def np_reranked_ranks(coarse, fine, k, direction, im_div=5):
    """The definition: shortlist = the k best of the coarse line, in fine order, then all others in coarse order; rank = best
    position of a ground truth."""
    M_c, M_f = (coarse, fine) if direction == 'i2t' else (coarse.T, fine.T)
    ranks = np.zeros(M_c.shape[0])
    for q in range(M_c.shape[0]):
        n = M_c.shape[1]
        order_c = np.lexsort((-np.arange(n), -M_c[q]))
        short, rest = order_c[:k], order_c[k:]
        short = short[np.lexsort((-short, -M_f[q][short]))]
        ranking = np.concatenate([short, rest])
        gt = np.arange(im_div * q, im_div * q + im_div) if direction == 'i2t' else np.asarray([q // im_div])
        ranks[q] = np.nonzero(np.isin(ranking, gt))[0].min()
    return ranks


RERANK_SEED = 3            # chosen on the CPU: the smallest separation inside a shortlist is 7.2e-5


def rerank_case(seed):
    Ni, D = 40, 32
    rng = np.random.RandomState(seed)
    lens = rng.randint(8, 30, size=Ni * 5)
    _, img, words, cap, off, lens = make_set(seed, Ni, lens, D)
    coarse = (torch.randn(Ni, Ni * 5) * 0.2).float()
    kw = dict(cross_attn='t2i', raw_feature_norm='clipped_l2norm', agg_func='Sum')
    fine = O.xattn_score(img, cap, lens, 't2i', 'clipped_l2norm', 'Sum')
    return img, words, off, lens, coarse, fine, kw


def shortlists_separated(coarse, fine, k, direction):
    M_c, M_f = (coarse, fine) if direction == 'i2t' else (coarse.T, fine.T)
    worst = np.inf
    for q in range(M_c.shape[0]):
        short = np.lexsort((-np.arange(M_c.shape[1]), -M_c[q]))[:k]
        v = np.sort(M_f[q][short].astype(np.float64))
        if len(v) > 1:
            worst = min(worst, float(np.diff(v).min()))
    return worst


def test_evaluation_rerank_end_to_end(dev):
    k = 10
    img, words, off, lens, coarse, fine, kw = rerank_case(RERANK_SEED)
    c_np, f_np = coarse.numpy(), fine.numpy()
    for direction in ('i2t', 't2i'):
        sep = shortlists_separated(c_np, f_np, k, direction)
        print("shortlist separation %s: %.3g" % (direction, sep))
        assert sep > 4e-5, "oracle scores inside a %s shortlist are closer than twice the tolerance (%.3g): pick another seed" % (direction, sep)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    fn = lambda cand, by: ops.scan_candidate_scores(img_d, words_d, plan, cand, by, **kw)
    r_i, r_t, (i_ranks, t_ranks), tl = evaluation.rerank(coarse.to(dev), fn, k)
    want_i, want_t = np_reranked_ranks(c_np, f_np, k, 'i2t'), np_reranked_ranks(c_np, f_np, k, 't2i')
    assert np.array_equal(i_ranks, want_i) and np.array_equal(t_ranks, want_t)
    assert tl['i2t_topk'].shape == (40, k) and tl['t2i_topk'].shape == (200, k)
    assert tuple(r_i) == tuple(ops.recall_from_ranks(want_i)) and tuple(r_t) == tuple(ops.recall_from_ranks(want_t))
    with pytest.raises(ValueError):
        evaluation.rerank(coarse.to(dev), fn, 9)
    # k = Ni = 40 in the t2i direction: the shortlist is every image, the t2i ranks are those of the fine matrix outright
    gt = f_np[np.arange(200) // 5, np.arange(200)]
    others = np.abs(f_np - gt[None, :]) + np.where(np.arange(40)[:, None] == (np.arange(200) // 5)[None, :], np.inf, 0.0)
    assert others.min() > 4e-5, "a ground-truth score is closer than twice the tolerance to another image's: pick another seed"
    _, _, (_, t_ranks), _ = evaluation.rerank(coarse.to(dev), fn, 40)
    assert np.array_equal(t_ranks, O.rank_counts(f_np.astype(np.float64))[2])
