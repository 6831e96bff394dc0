"""GPU, full size (5 000 images x 25 000 captions, D = 1024, K = 100, both list directions): SCAN candidate scores against the CPU
oracle on 256 randomly chosen listed pairs of each list direction (2e-5), and against the dense kernel's matrix on ALL listed pairs (4e-5: both are within
2e-5 of the same oracle value; the dense kernel is not code under test).  Measured: max |candidate - dense| = 1.2e-7 -- close, not
bit-identical (the dense epilogue runs its Gram product on the matrix cores, this one on the vector ALU), so the bound is asserted."""
import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
def test_candidates_fullsize(dev, xa):
    Ni, Nc, D, K = 5000, 25000, 1024, 100
    rng = np.random.RandomState(17)
    torch.manual_seed(17)
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = ops.l2norm(torch.randn(int(lens.sum()), D, device=dev))
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    # seeded pooled matrix: cosine of the mean-pooled regions and words
    seg = torch.repeat_interleave(torch.arange(Nc, device=dev), torch.from_numpy(lens.astype(np.int64)).to(dev))
    coarse = ops.cosine_scores(ops.l2norm(img.mean(1)), ops.l2norm(torch.zeros(Nc, D, device=dev).index_add_(0, seg, words)))
    r_idx, _, part = ops.topk_lists(coarse, K)
    c_idx, _ = ops.topk_merge_cols([part], K)
    del coarse
    S = ops.scan_xattn_scores(img, words, plan, cross_attn=xa)
    ws = ops.scan_pairs_prepare(img, words, plan, xa)
    img_c, words_c = img.cpu(), words.cpu()
    for by, cand in (('image', r_idx), ('caption', c_idx)):
        got = ops.scan_candidate_scores(img, words, plan, cand, by, cross_attn=xa, workspace=ws)
        c64 = cand.to(torch.int64)
        dense = S.gather(1, c64) if by == 'image' else S.gather(0, c64.t()).t()
        d_all = float((got - dense).abs().max())
        print("fullsize %s by=%s: max |candidate - dense| over %d pairs = %.3g" % (xa, by, got.numel(), d_all))
        assert d_all <= 4e-5
        got_c, cand_c = got.cpu().numpy(), cand.cpu().numpy()
        worst = 0.0
        for _ in range(256):
            q, k = rng.randint(cand_c.shape[0]), rng.randint(K)
            i, c = (q, cand_c[q, k]) if by == 'image' else (cand_c[q, k], q)
            w = words_c[off[c]:off[c] + lens[c]]
            want = float(O.xattn_score(img_c[i:i + 1], w[None], [int(lens[c])], xa)[0, 0])
            worst = max(worst, abs(float(got_c[q, k]) - want))
        print("fullsize %s by=%s: max |candidate - oracle| over 256 pairs = %.3g" % (xa, by, worst))
        assert worst <= 2e-5
