"""GPU: SGRAF scores of candidate lists (ops.sgraf_candidate_scores, csrc/sgraf_pairs.hip) against oracle/itr_oracle.py, the
own-score property (a pair's bits do not depend on the list, its order, K, the direction, the other captions or the chunking),
the refusals, and evaluation.rerank with the SGRAF score function.

Tolerance against the oracle: 5e-6 absolute, the bound test_kernels_gpu.py holds the dense SGRAF call to against the same oracle."""
import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops
from itr_amd.metricmodule import evaluation

pytestmark = pytest.mark.gpu

TOL = 5e-6
KS = [1, 10, 37, 128]
# test_scan_candidates_gpu.RAGGED with its 64-word caption at 63 (the fused SGRAF kernels hold 63 words + the global node)
RAGGED = [1, 16, 17, 63, 5, 13, 32, 33, 48, 49, 2, 9, 11, 27, 63, 8, 12, 15, 20, 31, 7, 3, 40, 14]
MIXED_LONG = [5, 64, 12, 70, 63, 82, 1, 30, 17]


def make_weights(D, S, steps=3, seed=5, eval_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    w = {}

    def lin(name, o, i):
        r = float(np.sqrt(6.0 / (i + o)))
        w[name + ".weight"] = (torch.rand(o, i, generator=g) * 2 - 1) * r
        w[name + ".bias"] = torch.randn(o, generator=g) * 0.02

    def bn(name, n):
        w[name + ".weight"] = torch.rand(n, generator=g) * 0.4 + 0.8
        w[name + ".bias"] = torch.randn(n, generator=g) * 0.05
        w[name + ".running_mean"] = torch.randn(n, generator=g) * 0.1
        w[name + ".running_var"] = torch.rand(n, generator=g) + 0.5

    lin("v_global_w.embedding_local.0", D, D); bn("v_global_w.embedding_local.1", 36)
    lin("v_global_w.embedding_global.0", D, D); bn("v_global_w.embedding_global.1", D)
    lin("v_global_w.embedding_common.0", 1, D)
    lin("t_global_w.embedding_local.0", D, D); lin("t_global_w.embedding_global.0", D, D); lin("t_global_w.embedding_common.0", 1, D)
    lin("sim_tranloc_w", S, D); lin("sim_tranglo_w", S, D); lin("sim_eval_w", 1, S)
    lin("SAF_module.attn_sim_w", 1, S); bn("SAF_module.bn", 1)
    for k in range(steps):
        for nm in ("graph_query_w", "graph_key_w", "sim_graph_w"):
            lin("SGR_module.sgr%d.%s" % (k, nm), S, S)
    w["sim_eval_w.weight"] = w["sim_eval_w.weight"] * eval_scale
    return w


def make_set(seed, Ni, lens, D):
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    lens = np.asarray(lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = O.l2norm(torch.randn(Ni, 36, D), -1)
    words = O.l2norm(torch.randn(int(lens.sum()), D), -1)
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


def to_dev(w, dev):
    return {k: v.to(dev) for k, v in w.items()}


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
@pytest.mark.parametrize("S", [64, 256])
@pytest.mark.parametrize("D", [32, 96, 1024])
def test_oracle_parity(dev, D, S, mod):
    Ni = 13                                             # not a multiple of 4 / 8 / 16 / 64
    rng, img, words, cap, off, lens = make_set(7 + D, Ni, RAGGED, D)
    Nc = len(lens)
    w = make_weights(D, S)
    want = O.sgraf_similarity(w, img, cap, [int(x) for x in lens], mod, 3)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d, w_d = img.to(dev), words.to(dev), to_dev(w, dev)
    worst = 0.0
    for by in ('caption', 'image'):
        n_q, n_t = (Nc, Ni) if by == 'caption' else (Ni, Nc)
        for K in KS:
            cand = lists(rng, n_q, n_t, K)
            got = ops.sgraf_candidate_scores(img_d, words_d, plan, w_d, torch.from_numpy(cand).to(dev), by, module_name=mod, sgr_step=3)
            assert got.shape == (n_q, K)
            err = maxdiff(got, expected(want, cand, by))
            worst = max(worst, err)
            print("parity %s D=%d S=%d by=%s K=%d: max|d| = %.3g" % (mod, D, S, by, K, err))
            assert err <= TOL, (mod, D, S, by, K, err)
    print("parity worst %s D=%d S=%d: %.3g" % (mod, D, S, worst))


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
@pytest.mark.parametrize("S", [64, 256])
def test_oracle_parity_with_long_captions(dev, S, mod):
    """captions of 64 / 70 / 82 words among the others: the per-caption composition scores their listed pairs"""
    Ni, D = 11, 96
    rng, img, words, cap, off, lens = make_set(3, Ni, MIXED_LONG, D)
    Nc = len(lens)
    w = make_weights(D, S)
    want = O.sgraf_similarity(w, img, cap, [int(x) for x in lens], mod, 3)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d, w_d = img.to(dev), words.to(dev), to_dev(w, dev)
    for by, K in (('caption', 10), ('image', 1), ('image', 37)):
        n_q, n_t = (Nc, Ni) if by == 'caption' else (Ni, Nc)
        cand = lists(rng, n_q, n_t, K)
        got = ops.sgraf_candidate_scores(img_d, words_d, plan, w_d, torch.from_numpy(cand).to(dev), by, module_name=mod, sgr_step=3)
        err = maxdiff(got, expected(want, cand, by))
        print("long captions %s S=%d by=%s K=%d: max|d| = %.3g" % (mod, S, by, K, err))
        assert err <= TOL, (mod, S, by, K, err)


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
@pytest.mark.parametrize("S", [64, 256])
def test_a_pairs_score_is_its_own(dev, S, mod):
    """The same pair scores the same bits in a shuffled list, in a subset, with the other captions' rows removed, through either list
    direction, under two workspace budgets that force different chunkings, and in a second run."""
    Ni, D, K = 21, 256, 12
    rng, img, words, cap, off, lens = make_set(11, Ni, RAGGED, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d, w_d = img.to(dev), words.to(dev), to_dev(make_weights(D, S), dev)
    kw = dict(module_name=mod, sgr_step=3)
    score = lambda c, by, **k2: ops.sgraf_candidate_scores(img_d, words_d, plan, w_d, torch.from_numpy(np.ascontiguousarray(c)).to(dev), by, **kw, **k2).cpu()
    cand = lists(rng, Nc, Ni, K)
    base = score(cand, 'caption')
    assert ops.SGRAF_PAIRS_LAST['chunks'] == 1
    assert not torch.isnan(base).any()
    # a second run
    assert torch.equal(score(cand, 'caption'), base)
    # shuffled inside every list
    perm = np.stack([rng.permutation(K) for _ in range(Nc)])
    got = score(np.take_along_axis(cand, perm, 1), 'caption')
    assert torch.equal(got, torch.from_numpy(np.take_along_axis(base.numpy(), perm, 1)))
    # a subset of every list (other items: 5 instead of 12 pairs per caption)
    assert torch.equal(score(cand[:, 3:8], 'caption'), base[:, 3:8])
    # two budgets that force different chunkings: a few items per chunk, and about half the list per chunk
    lib = ops._lib.load()
    m = 0 if mod == 'SAF' else 1
    seen = set()
    for n_items, n_pairs in ((3, 48), (40, 160)):
        budget = lib.itr_sgraf_pair_scores_workspace_bytes(n_pairs, n_items, D, S, m, 3)
        assert torch.equal(score(cand, 'caption', max_workspace_bytes=budget), base), (n_items, n_pairs)
        seen.add(ops.SGRAF_PAIRS_LAST['chunks'])
        assert ops.SGRAF_PAIRS_LAST['chunks'] > 1 and ops.SGRAF_PAIRS_LAST['workspace_bytes'] <= budget
    assert len(seen) == 2, "the two budgets gave the same chunking: %s" % (seen,)
    with pytest.raises(torch.cuda.OutOfMemoryError):
        score(cand, 'caption', max_workspace_bytes=1024)
    # the other captions' rows removed: captions 5..10 alone, in a plan of their own
    c0, c1 = 5, 11
    r0, r1 = int(off[c0]), int(off[c1 - 1] + lens[c1 - 1])
    sub_plan = ops.ScanPlan(off[c0:c1] - r0, lens[c0:c1], r1 - r0, dev)
    got = ops.sgraf_candidate_scores(img_d, words_d[r0:r1].contiguous(), sub_plan, w_d, torch.from_numpy(np.ascontiguousarray(cand[c0:c1])).to(dev),
                                     'caption', **kw).cpu()
    assert torch.equal(got, base[c0:c1])
    # the same pairs listed per image, with one prepared state for both directions
    state = ops.sgraf_pairs_prepare(img_d, words_d, plan, w_d, mod, 3)
    ci = lists(rng, Ni, Nc, K)
    by_img = score(ci, 'image', state=state)
    back = np.zeros((Nc, Ni * K), np.int32)          # per caption: the images that listed it (padded with image 0)
    src = -np.ones((Nc, Ni * K), np.int64)
    fill = np.zeros(Nc, np.int64)
    for i in range(Ni):
        for k in range(K):
            c = ci[i, k]
            back[c, fill[c]], src[c, fill[c]] = i, i * K + k
            fill[c] += 1
    W = int(fill.max())
    by_cap = score(back[:, :W], 'caption', state=state)
    msk = src[:, :W] >= 0
    assert torch.equal(by_cap[torch.from_numpy(msk)], by_img.reshape(-1)[torch.from_numpy(src[:, :W][msk])])
    # and equal to the dense call's entries within the project's score tolerance
    dense = ops.sgraf_scores(img_d, words_d, plan, w_d, mod, 3).cpu()
    err = maxdiff(base, expected(dense, cand, 'caption'))
    print("candidates against the dense call %s S=%d: max|d| = %.3g" % (mod, S, err))
    assert err <= 2e-5


def test_refusals(dev):
    Ni, D, S = 11, 64, 64
    rng, img, words, cap, off, lens = make_set(5, Ni, [7, 12, 3, 20, 1], D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d, w_d = img.to(dev), words.to(dev), to_dev(make_weights(D, S), dev)
    cand = torch.zeros(Nc, 3, dtype=torch.int32, device=dev)
    f = ops.sgraf_candidate_scores
    for bad in (-1, Ni):
        c = cand.clone()
        c[2, 1] = bad
        with pytest.raises(ValueError, match="out of range"):
            f(img_d, words_d, plan, w_d, c, 'caption')
    c = torch.zeros(Ni, 3, dtype=torch.int32, device=dev)
    c[0, 0] = Nc
    with pytest.raises(ValueError, match="out of range"):
        f(img_d, words_d, plan, w_d, c, 'image')
    with pytest.raises(ValueError, match="by must be"):
        f(img_d, words_d, plan, w_d, cand, 'rows')
    with pytest.raises(ValueError, match="2-D"):
        f(img_d, words_d, plan, w_d, cand.reshape(-1), 'caption')
    with pytest.raises(ValueError, match="lists"):
        f(img_d, words_d, plan, w_d, cand[:-1], 'caption')
    with pytest.raises(ValueError, match="Invalid input of config.module_name in configs.py"):
        f(img_d, words_d, plan, w_d, cand, 'caption', module_name='AVE')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(img, words_d, plan, w_d, cand, 'caption')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(img_d, words_d, plan, w_d, cand.cpu(), 'caption')
    with pytest.raises(NotImplementedError):
        f(torch.zeros(Ni, 35, D, device=dev), words_d, plan, w_d, cand, 'caption')
    # more than 191 words
    p192 = ops.ScanPlan(np.asarray([0, 5], np.int64), np.asarray([5, 192], np.int32), 197, dev)
    with pytest.raises(NotImplementedError, match="191"):
        f(img_d, torch.zeros(197, D, device=dev), p192, w_d, cand[:2], 'caption')
    # >= 2^31 pairs: refused on the shape alone (an expanded view: no memory behind it)
    huge = torch.zeros(1, 1, dtype=torch.int32, device=dev).expand(Nc, (2 ** 31) // Nc + 1)
    with pytest.raises(NotImplementedError, match="pairs"):
        f(img_d, words_d, plan, w_d, huge, 'caption')
    # empty shapes
    assert f(img_d, words_d, plan, w_d, cand[:, :0], 'caption').shape == (Nc, 0)
    assert f(img_d[:0], words_d, plan, w_d, torch.zeros(0, 4, dtype=torch.int32, device=dev), 'image').shape == (0, 4)
    p0 = ops.ScanPlan(np.zeros(0, np.int64), np.zeros(0, np.int32), 0, dev)
    assert f(img_d, words_d[:0], p0, w_d, torch.zeros(0, 4, dtype=torch.int32, device=dev), 'caption').shape == (0, 4)
    # prepared-state misuse
    state = ops.sgraf_pairs_prepare(img_d, words_d, plan, w_d, 'SAF', 3)
    f(img_d, words_d, plan, w_d, cand, 'caption', state=state)
    with pytest.raises(ValueError, match="module"):
        f(img_d, words_d, plan, w_d, cand, 'caption', module_name='SGR', state=state)
    with pytest.raises(ValueError, match="other images"):
        f(img_d.clone(), words_d, plan, w_d, cand, 'caption', state=state)
    with pytest.raises(ValueError, match="other images"):
        f(img_d, words_d, ops.ScanPlan(off, lens, words.shape[0], dev), w_d, cand, 'caption', state=state)
    w2 = dict(w_d)
    w2["sim_eval_w.weight"] = w_d["sim_eval_w.weight"].clone()
    with pytest.raises(ValueError, match="weights"):
        f(img_d, words_d, plan, w2, cand, 'caption', state=state)
    w_d["sim_eval_w.bias"].add_(1.0)                      # modified in place since
    with pytest.raises(ValueError, match="modified"):
        f(img_d, words_d, plan, w_d, cand, 'caption', state=state)
    with pytest.raises(TypeError):
        f(img_d, words_d, plan, w_d, cand, 'caption', state=object())
    sgr = ops.sgraf_pairs_prepare(img_d, words_d, plan, w_d, 'SGR', 3)
    with pytest.raises(ValueError, match="steps"):
        f(img_d, words_d, plan, w_d, cand, 'caption', module_name='SGR', sgr_step=2, state=sgr)


RERANK_SEED = {'SAF': 26, 'SGR': 26}      # chosen with the CPU oracle for well separated scores inside every shortlist; the test asserts it


def rerank_case(seed):
    Ni, D, S = 10, 32, 64
    rng = np.random.RandomState(seed)
    lens = rng.randint(3, 20, size=Ni * 5)
    _, img, words, cap, off, lens = make_set(seed, Ni, lens, D)
    # sim_eval_w scaled up: the scores spread over (0, 1) instead of crowding around 0.5
    w = make_weights(D, S, seed=seed + 100, eval_scale=40.0)
    coarse = (torch.randn(Ni, Ni * 5) * 0.2).float()
    return img, words, cap, off, lens, w, coarse


def min_gap_in_lists(idx, M):
    """smallest difference between two fine scores inside one list; idx [n, k] indexes the columns of M's rows"""
    worst = np.inf
    for q in range(idx.shape[0]):
        v = np.sort(M[q][np.unique(idx[q])].astype(np.float64))
        if len(v) > 1:
            worst = min(worst, float(np.diff(v).min()))
    return worst


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
def test_evaluation_rerank_end_to_end(dev, mod):
    """evaluation.rerank with the SGRAF score function: the reranked lists are those obtained by gathering the same entries from the
    dense sgraf_scores matrix and re-ordering them with rerank_lists, index for index."""
    k = 10
    img, words, cap, off, lens, w, coarse = rerank_case(RERANK_SEED[mod])
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d, w_d = img.to(dev), words.to(dev), to_dev(w, dev)
    state = ops.sgraf_pairs_prepare(img_d, words_d, plan, w_d, mod, 3)
    fn = lambda cand, by: ops.sgraf_candidate_scores(img_d, words_d, plan, w_d, cand, by, module_name=mod, sgr_step=3, state=state)
    coarse_d = coarse.to(dev)
    _, _, (i_ranks, t_ranks), tl = evaluation.rerank(coarse_d, fn, k)
    dense = ops.sgraf_scores(img_d, words_d, plan, w_d, mod, 3)
    r_idx, _, part = ops.topk_lists(coarse_d, k)
    c_idx, _ = ops.topk_merge_cols([part], k)
    d_np = dense.cpu().numpy()
    gap_i = min_gap_in_lists(r_idx.cpu().numpy(), d_np)
    gap_t = min_gap_in_lists(c_idx.cpu().numpy(), d_np.T)
    print("smallest fine-score gap inside a list %s: i2t %.3g, t2i %.3g" % (mod, gap_i, gap_t))
    assert min(gap_i, gap_t) > 1e-4, "fine scores inside a shortlist are closer than 1e-4: pick another seed"
    fine_i = torch.gather(dense, 1, r_idx.long())
    fine_t = torch.gather(dense.t().contiguous(), 1, c_idx.long())
    ri, _, _ = ops.rerank_lists(r_idx, fine_i)
    ci, _, _ = ops.rerank_lists(c_idx, fine_t)
    assert np.array_equal(tl['i2t_topk'], ri.cpu().numpy().astype(np.int64))
    assert np.array_equal(tl['t2i_topk'], ci.cpu().numpy().astype(np.int64))
    assert tl['i2t_topk'].shape == (10, k) and tl['t2i_topk'].shape == (50, k)
    assert maxdiff(torch.from_numpy(tl['i2t_topk_scores']), np.take_along_axis(d_np, tl['i2t_topk'], 1)) <= 2e-5
    assert len(i_ranks) == 10 and len(t_ranks) == 50
