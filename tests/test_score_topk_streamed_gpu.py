"""GPU: evalpipe.score_topk_streamed (top-k lists and Recall ranks of a pooled scorer without the similarity matrix in memory) and
evaluation.rerank_streamed / rerank_ensemble_streamed on top of it, against the materialised matrix: finalize_topk / finalize_ranks
of the one-call matrix, the lists of the matrix concatenated from the very blocks that were streamed, and rerank / rerank_ensemble
entry for entry.  Inputs are those of tests/test_kernels_gpu.py::test_streamed_score_rank_equals_the_materialised_matrix.  All
comparisons are exact (indices equal, values equal as uint32 bit patterns)."""
import numpy as np
import pytest
import torch

from itr_amd import evalpipe, ops
from itr_amd.metricmodule import evaluation

pytestmark = pytest.mark.gpu

NI, D = 700, 64
NC = 5 * NI - 3
KINDS = ["cosine", "cosine_ties", "mvm", "pdist_cos"]
NAMES = ("i2t_idx", "i2t_val", "t2i_idx", "t2i_val")


def inputs(kind, dev):
    torch.manual_seed(5)
    if kind == "mvm":
        img = torch.randn(NI, 12, D, device=dev)
        fn = ops.mvm_scores
    else:
        img = torch.randn(NI, D, device=dev)
        fn = ops.pdist_cos if kind == "pdist_cos" else ops.cosine_scores
    cap = torch.randn(NC, D, device=dev)
    if kind == "cosine_ties":
        img, cap = torch.round(img), torch.round(cap)            # integer-valued: products are exact, scores collide by the thousand
    if kind == "pdist_cos":
        cap[17] = 0                                               # a NaN column before the epilogue zeroes it
    return img, cap, fn


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("kind", KINDS)
def test_streamed_lists_and_ranks_equal_the_materialised_matrix(dev, kind):
    img, cap, fn = inputs(kind, dev)
    S = fn(img, cap)
    comm = evalpipe.Comm()
    want_ranks = evalpipe.finalize_ranks(comm, S, 0, NI, 5)
    for k in (10, 100):
        want = evalpipe.finalize_topk(comm, S, 0, NI, k)
        for rb in (128, 256):
            seen = []

            def recording(a, b, out=None):                        # the very blocks that were streamed (full-width ones)
                r = fn(a, b, out=out)
                if b.shape[0] == NC:
                    seen.append(r.clone())
                return r
            lists, ranks = evalpipe.score_topk_streamed(img, cap, recording, k, 5, rows_per_block=rb)
            for g, w, name in zip(lists, want, NAMES):
                assert same(g, w), (kind, k, rb, name, "vs the one-call matrix")
            for g, w, name in zip(ranks, want_ranks, ("i2t_rank", "i2t_top1", "t2i_rank", "t2i_top1")):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (kind, k, rb, name)
            S_blocks = torch.cat(seen, 0)
            assert S_blocks.shape == S.shape and len(seen) == -(-NI // rb)
            for g, w, name in zip(lists, evalpipe.finalize_topk(comm, S_blocks, 0, NI, k), NAMES):
                assert same(g, w), (kind, k, rb, name, "vs the concatenated blocks")
    if kind == "cosine_ties":
        assert len(np.unique(S.cpu().numpy())) < S.numel() // 100        # (the tie case is one)


def test_directions_and_ranks_can_be_left_out(dev):
    img, cap, fn = inputs("cosine", dev)
    k = 10
    full, ranks = evalpipe.score_topk_streamed(img, cap, fn, k, rows_per_block=256)
    no_rows, r2 = evalpipe.score_topk_streamed(img, cap, fn, k, rows=False, rows_per_block=256)
    assert no_rows[0] is None and no_rows[1] is None and same(no_rows[2], full[2]) and same(no_rows[3], full[3])
    no_cols, r3 = evalpipe.score_topk_streamed(img, cap, fn, k, cols=False, rows_per_block=256)
    assert no_cols[2] is None and no_cols[3] is None and same(no_cols[0], full[0]) and same(no_cols[1], full[1])
    for r in (r2, r3):
        assert all(np.array_equal(a, b) for a, b in zip(r, ranks))
    only = evalpipe.score_topk_streamed(img, cap, fn, k, ranks=False, rows=False, rows_per_block=256)
    assert len(only) == 4 and only[0] is None and same(only[2], full[2]) and same(only[3], full[3])
    # the default block height (the 64 MB budget) is one more partition
    default, _ = evalpipe.score_topk_streamed(img, cap, fn, k)
    assert all(same(a, b) for a, b in zip(default, full))


def toy_score_fn(seed, dev):
    """a deterministic fine scorer on (query, candidate): a fixed random matrix looked up by the pair"""
    g = torch.Generator().manual_seed(seed)
    F = torch.round(torch.randn(NI, NC, generator=g) * 8).div(8).to(dev)           # coarse grid: ties inside a list

    def fn(cand, by):
        c = cand.long()
        q = torch.arange(c.shape[0], device=dev)[:, None]
        return (F[q, c] if by == 'image' else F[c, q]).contiguous()
    return fn


def assert_same_rerank(got, want, tag):
    assert got[0] == want[0] and got[1] == want[1], tag
    for a, b in zip(got[2], want[2]):
        assert np.array_equal(a, b), tag
    assert sorted(got[3]) == sorted(want[3]), tag
    for key in want[3]:
        a, b = got[3][key], want[3][key]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, key)
        assert a.tobytes() == b.tobytes(), (tag, key)


@pytest.mark.parametrize("kind", ["cosine", "cosine_ties"])
def test_rerank_streamed_equals_rerank(dev, kind):
    img, cap, fn = inputs(kind, dev)
    S = fn(img, cap)
    f1, f2 = toy_score_fn(1, dev), toy_score_fn(2, dev)
    for k in (10, 100):
        want = evaluation.rerank(S, f1, k)
        got = evaluation.rerank_streamed(img, cap, fn, f1, k)
        assert_same_rerank(got, want, (kind, k, "single"))
        want = evaluation.rerank_ensemble(S, [f1, f2], k)
        got = evaluation.rerank_ensemble_streamed(img, cap, fn, [f1, f2], k)
        assert_same_rerank(got, want, (kind, k, "ensemble"))
    with pytest.raises(ValueError):
        evaluation.rerank_streamed(img, cap, fn, f1, 9)
