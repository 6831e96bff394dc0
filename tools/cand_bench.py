#!/usr/bin/env python3
"""Timing of SCAN candidate-list scoring against the dense call, interleaved in ONE process on one device:
  dense ops.scan_xattn_scores (5 000 x 25 000, the inputs bench.py draws), ops.scan_candidate_scores for K in {10, 100} per
  direction and both, and ops.rerank_lists.  Candidates = the top-K of a seeded pooled (cosine) matrix in both directions.
Prints one line per arm: pairs, median / min ms over the rounds, pairs/s, and the executed-flop fraction (matrix-core flops the
arm executes, column padding included, over the dense call's).  Usage: python tools/cand_bench.py [--ni 5000] [--rounds 5] [--xa t2i]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
from itr_amd import ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--xa", default="both", choices=["t2i", "i2t", "both"])
    ap.add_argument("--skip-dense", action="store_true", help="candidate arms only (counter runs: the dense call is slow under them)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    Ni, Nc, D = a.ni, a.ni * 5, a.dim
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)          # bench.py's caption lengths
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = ops.l2norm(torch.randn(int(lens.sum()), D, device=dev))
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    # the pooled coarse model: cosine of mean-pooled regions and words (seeded, nothing learned: only the lists' shape matters)
    pi = ops.l2norm(img.mean(1))
    seg = torch.repeat_interleave(torch.arange(Nc, device=dev), torch.from_numpy(lens.astype(np.int64)).to(dev))
    pc = ops.l2norm(torch.zeros(Nc, D, device=dev).index_add_(0, seg, words))
    coarse = ops.cosine_scores(pi, pc)
    cols16 = float((np.ceil(lens / 16.0) * 16).sum())
    for xa in (["t2i", "i2t"] if a.xa == "both" else [a.xa]):
        ws_d = ops.scan_prepare(img, words, plan, xa)
        ws_p = ops.scan_pairs_prepare(img, words, plan, xa)
        S = torch.empty(Ni, Nc, device=dev)
        dense_flops = Ni * 36.0 * plan.n_tiles * 64
        arms = {} if a.skip_dense else {"dense": (lambda: ops.scan_xattn_scores(img, words, plan, cross_attn=xa, out=S, workspace=ws_d),
                                                  Ni * Nc, dense_flops)}
        lists = {}
        for K in (10, 100):
            r_idx, _, part = ops.topk_lists(coarse, K)
            c_idx, _ = ops.topk_merge_cols([part], K)
            lists[K] = (r_idx, c_idx)
            f_img = 48.0 * float((np.ceil(lens / 16.0) * 16)[r_idx.cpu().numpy().astype(np.int64)].sum())
            f_cap = 48.0 * K * cols16
            cs = lambda cand, by: ops.scan_candidate_scores(img, words, plan, cand, by, cross_attn=xa, workspace=ws_p)
            arms["cand K=%d by=image" % K] = ((lambda r=r_idx: cs(r, 'image')), Ni * K, f_img)
            arms["cand K=%d by=caption" % K] = ((lambda c=c_idx: cs(c, 'caption')), Nc * K, f_cap)
            arms["cand K=%d both" % K] = ((lambda r=r_idx, c=c_idx: (cs(r, 'image'), cs(c, 'caption'))), (Ni + Nc) * K, f_img + f_cap)
        fine = ops.scan_candidate_scores(img, words, plan, lists[100][1], 'caption', cross_attn=xa, workspace=ws_p)
        arms["rerank_lists K=100 (Nc lists)"] = ((lambda: ops.rerank_lists(lists[100][1], fine)), Nc * 100, 0.0)
        times = {k: [] for k in arms}
        for k in arms:
            arms[k][0]()                                             # warm-up
        torch.cuda.synchronize()
        for _ in range(a.rounds):                                    # interleaved rounds: every arm once per round
            for k in arms:
                times[k].append(timed(arms[k][0]))
        dense_ms = float(np.median(times["dense"])) if "dense" in times else float("nan")
        for k, (fn, pairs, flops) in arms.items():
            med, mn = float(np.median(times[k])), float(np.min(times[k]))
            print(json.dumps({"xa": xa, "arm": k, "pairs": int(pairs), "ms_median": round(med, 3), "ms_min": round(mn, 3),
                              "pairs_per_s": round(pairs / (med * 1e-3)), "dense_over_arm": round(dense_ms / med, 2),
                              "executed_flop_fraction": round(flops / dense_flops, 5), "device": torch.cuda.get_device_name(0)}))
        if a.skip_dense:
            continue
        # the candidate scores against the dense matrix on all listed pairs
        got = ops.scan_candidate_scores(img, words, plan, lists[100][1], 'caption', cross_attn=xa, workspace=ws_p)
        ref = S.gather(0, lists[100][1].to(torch.int64).t()).t()
        print(json.dumps({"xa": xa, "max_abs_cand_minus_dense_K100_by_caption": float((got - ref).abs().max())}))


if __name__ == "__main__":
    main()
