"""GPU, full size: SGRAF candidate scores at 5 000 x 25 000, D = 1024, sim_dim 256, bench-like caption lengths.  The by-caption K = 100
lists of ALL 25 000 captions (2.5 M pairs, from a pooled-cosine top-K as tools/sgraf_cand_bench.py builds them) go through the candidate
entry: the state at Nc = 25 000, the item plan over ~500 pairs per image, and the chunking.  The reference is the dense ops.sgraf_scores
on a SAMPLED subset of 500 captions (a sub-plan of their own: the dense call does not depend on which other captions are in the call),
compared with those captions' rows of the candidate result.  Bound: 2e-5 absolute, the project's score tolerance (TOL in
test_scan_candidates_gpu.py).  Measured on an MI355X: max |cand - dense| = 5.96e-08 for SAF and for SGR."""
import numpy as np
import pytest
import torch

from itr_amd import ops
from test_sgraf_candidates_gpu import make_weights, to_dev

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.mark.parametrize("mod", ['SAF', 'SGR'])
def test_sampled_captions_against_the_dense_call(dev, mod):
    Ni, D, S, K, n_sample = 5000, 1024, 256, 100, 500
    Nc = 5 * Ni
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = ops.l2norm(torch.randn(int(lens.sum()), D, device=dev))
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    # pooled-cosine top-K images of EVERY caption
    pi = ops.l2norm(img.mean(1))
    seg = torch.repeat_interleave(torch.arange(Nc, device=dev), torch.from_numpy(lens.astype(np.int64)).to(dev))
    pc = ops.l2norm(torch.zeros(Nc, D, device=dev).index_add_(0, seg, words))
    coarse = ops.cosine_scores(pi, pc)
    _, _, part = ops.topk_lists(coarse, K)
    c_idx, _ = ops.topk_merge_cols([part], K)
    del coarse, part
    w = to_dev(make_weights(D, S), dev)
    # A budget that forces several chunks whatever the card's free memory: the workspace of a quarter of the list (2.5 M pairs in about
    # 620 000 items of 4 pairs; sized with the entry's own workspace function), about 57 GB -- so 4 to 5 chunks.
    lib = ops._lib.load()
    budget = lib.itr_sgraf_pair_scores_workspace_bytes(Nc * K // 4, Nc * K // 16, D, S, 0 if mod == 'SAF' else 1, 3)
    got = ops.sgraf_candidate_scores(img, words, plan, w, c_idx, 'caption', module_name=mod, sgr_step=3, max_workspace_bytes=budget)
    last = dict(ops.SGRAF_PAIRS_LAST)
    assert got.shape == (Nc, K) and last['pairs'] == Nc * K and last['chunks'] > 1
    assert not torch.isnan(got).any()
    # the dense reference: the sampled captions as a caption set of their own (rows gathered, a plan of their own)
    pick = np.sort(rng.choice(Nc, size=n_sample, replace=False))
    rows = np.concatenate([np.arange(off[c], off[c] + lens[c]) for c in pick])
    words_s = words[torch.from_numpy(rows).to(dev)].contiguous()
    lens_s = lens[pick]
    off_s = np.concatenate([[0], np.cumsum(lens_s)[:-1]]).astype(np.int64)
    plan_s = ops.ScanPlan(off_s, lens_s, words_s.shape[0], dev)
    dense = ops.sgraf_scores(img, words_s, plan_s, w, mod, 3)
    pick_d = torch.from_numpy(pick).to(dev)
    ref = dense.gather(0, c_idx[pick_d].to(torch.int64).t()).t()
    err = float((got[pick_d] - ref).abs().max())
    print("full size %s: %d pairs in %d items, %d chunks; %d sampled captions: max|cand - dense| = %.3g"
          % (mod, last['pairs'], last['items'], last['chunks'], n_sample, err))
    assert err <= TOL, (mod, err)
