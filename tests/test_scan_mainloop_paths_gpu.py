"""The generated SCAN main-loop statement (tools/gen_scan_mainloop.py -> csrc/scan_mainloop_asm.inc), entered through each of its
paths.  The statement is prologue + a two-chunk loop body + two peeled tails (`tail_even`, `tail_odd`) + park; which of them
a call runs depends on the chunk count nk = D / 32 alone.  The other SCAN tests use D in {32, 64, 256, 1024}: nk = 1 and 2
never enter the statement, 8 and 32 are both "even trips, then tail_odd".  Here:

    D     nk   path
    96     3   straight to tail_even
    128    4   one trip, tail_odd
    160    5   two trips (one loop iteration), tail_even
    192    6   three trips: the loop's first chunk a second time, tail_odd
    224    7   four trips: both chunks a second time, tail_even

A park store or a wait that is wrong in one of the peeled copies shows up as a wrong score at that D only; a store moved ahead
of the barrier that frees its buffer shows up when workgroups share a CU and their waves drift apart (the co-residency test).

The schedule rules themselves (tools/gen_scan_mainloop.py, docstring) are checked without a GPU by the generator's own walk
of every path."""
import os
import sys

import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def maxdiff(got, want):
    got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max())


def test_every_schedule_keeps_the_rules_on_every_path():
    """CPU: the committed schedule and every legal candidate the micro-benchmark compares are walked along nk = 3 .. 11: waits
    cover what is read, stores follow the barrier that frees their buffer, reads follow the barrier that publishes it, the MFMA
    order per accumulator is the parent's, nothing is fetched past the last chunk, nothing is in flight at the end."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_scan_mainloop as G
    assert G.SCHEDULES[G.COMMITTED].legal
    for name, sc in G.SCHEDULES.items():
        if sc.legal:
            assert G.verify(sc) > 0, name


@gpu
@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
@pytest.mark.parametrize("D", [96, 128, 160, 192, 224])
def test_scan_every_entry_path_vs_oracle(dev, xa, D):
    """Ni = 5: the second image tile holds one image (the row tail that re-reads row 0); 40 captions of 2-20 words: several
    column tiles.  Inputs as in test_scan_random_vs_oracle, the same 2e-5 budget."""
    Ni, Nc = 5, 40
    rng = np.random.RandomState(Ni + Nc + D)
    torch.manual_seed(D)
    lens = [int(x) for x in rng.randint(2, 21, size=Nc)]
    img = O.l2norm(torch.randn(Ni, 36, D), -1)
    cap = torch.randn(Nc, max(lens), D) * 0.5
    want = O.xattn_score(img, cap, lens, xa)
    got = ops.scan_xattn_padded(img.to(dev), cap.to(dev), lens, cross_attn=xa)
    d = maxdiff(got, want)
    print("D=%d %s max|diff| = %.3g" % (D, xa, d))
    assert d <= 2e-5


@gpu
@pytest.mark.parametrize("D", [160, 192])
def test_scan_t2i_paths_do_not_depend_on_the_tile_packing(dev, D):
    """test_scan_t2i_scores_do_not_depend_on_the_tile_packing at an odd and an even chunk count that enter the loop: a caption
    subset scored alone equals the same columns of the full call bit for bit (clipped_l2norm / LogSumExp)."""
    rng = np.random.RandomState(3)
    torch.manual_seed(3)
    Ni, Nc = 9, 700
    lens = rng.randint(1, 30, size=Nc).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    n_rows = int(lens.sum())
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = torch.randn(n_rows, D, device=dev) * 0.3
    kw = dict(raw_feature_norm='clipped_l2norm', agg_func='LogSumExp')
    full = ops.scan_xattn_scores(img, words, ops.ScanPlan(off, lens, n_rows, dev), **kw)
    for c0, c1 in ((0, 233), (233, 466), (466, 700), (101, 118)):
        r0, r1 = int(off[c0]), int(off[c1 - 1] + lens[c1 - 1])
        sub = ops.scan_xattn_scores(img, words[r0:r1].contiguous(), ops.ScanPlan(off[c0:c1] - r0, lens[c0:c1], r1 - r0, dev), **kw)
        assert torch.equal(sub, full[:, c0:c1]), (D, c0, c1, float((sub - full[:, c0:c1]).abs().max()))


@gpu
def test_scan_coresident_workgroups_agree(dev):
    """144 images x ~1 300 words at D = 160: 36 x 21 tiles, more than two workgroups per CU, so workgroups share CUs and their
    timing differs from call to call.  Two calls on the same inputs are bit-equal, and the first 8 images match the oracle."""
    Ni, Nc, D = 144, 122, 160
    rng = np.random.RandomState(7)
    torch.manual_seed(7)
    lens = [int(x) for x in rng.randint(2, 21, size=Nc)]
    img = O.l2norm(torch.randn(Ni, 36, D), -1)
    cap = torch.randn(Nc, max(lens), D) * 0.5
    a = ops.scan_xattn_padded(img.to(dev), cap.to(dev), lens, cross_attn='t2i')
    b = ops.scan_xattn_padded(img.to(dev), cap.to(dev), lens, cross_attn='t2i')
    assert 20 * 64 < sum(lens) <= 21 * 64, sum(lens)          # 21 column tiles
    assert torch.equal(a, b)
    want = O.xattn_score(img[:8], cap, lens, 't2i')
    d = maxdiff(a[:8], want)
    print("co-resident: %d words, max|diff| of 8 images = %.3g" % (sum(lens), d))
    assert d <= 2e-5
