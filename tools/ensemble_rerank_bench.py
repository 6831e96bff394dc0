#!/usr/bin/env python3
"""Timing of ensemble reranking, interleaved medians in ONE process on one device, in two parts:
  (a) the fusion call alone: ops.rerank_fused_lists at M = 2 beside ops.rerank_lists on the same 25 000 lists of 100;
  (b) a seeded synthetic 1 000 x 5 000 problem (D = 1024, sim_dim 256, captions of 6-20 words): the SAF + SGR ensemble rerank at K in
      {10, 100} -- per member its state prepared (as evaluation.rerank_ensemble does, one member at a time), both list directions
      scored, then both directions fused -- beside the dense ensemble's GPU work on the same operands: two ops.sgraf_scores calls
      ("dense scoring"), and those plus the float64 average on the device and ops.rank_counts_f64 ("dense ensemble").  The members'
      preparation is also timed as arms of its own, so that it can be subtracted.
Candidates = the top-K of a seeded pooled (cosine) matrix in both directions.  Prints one JSON line per arm.
Usage: python tools/ensemble_rerank_bench.py [--ni 1000] [--rounds 3] [--lists 25000]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itr_amd import ops  # noqa: E402
from sgraf_cand_bench import timed, weights  # noqa: E402


def run_arms(arms, rounds):
    times = {k: [] for k in arms}
    for k in arms:
        arms[k]()                                                # warm-up
    torch.cuda.synchronize()
    for _ in range(rounds):                                      # interleaved rounds: every arm once per round
        for k in arms:
            times[k].append(timed(arms[k]))
    return {k: (float(np.median(v)), float(np.min(v)), [round(float(np.percentile(v, p)), 4) for p in (25, 75)]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ni", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lists", type=int, default=25000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    rng = np.random.RandomState(0)
    torch.manual_seed(0)

    # (a) the fusion call beside the single-score re-ordering, same lists: K = 100 distinct candidates per list, scores with ties
    n, K = a.lists, 100
    idx = torch.from_numpy(np.argsort(rng.rand(n, 4 * K), axis=1)[:, :K].astype(np.int32)).to(dev)
    vals = torch.from_numpy((rng.randint(-2000, 2001, size=(2, n, K)) / 2048.0).astype(np.float32)).to(dev)
    v0 = vals[0].contiguous()
    res = run_arms({"rerank_lists": lambda: ops.rerank_lists(idx, v0), "rerank_fused_lists M=2": lambda: ops.rerank_fused_lists(idx, vals)},
                   a.rounds)
    for k, (med, mn, quart) in res.items():
        print(json.dumps({"part": "a", "arm": k, "lists": n, "K": K, "ms_median": round(med, 4), "ms_min": round(mn, 4), "ms_p25_p75": quart,
                          "over_rerank_lists": round(med / res["rerank_lists"][0], 2), "device": name}), flush=True)
    del idx, vals, v0

    # (b) SAF + SGR ensemble rerank beside the dense ensemble
    Ni, Nc, D, S = a.ni, a.ni * 5, a.dim, 256
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = ops.l2norm(torch.randn(int(lens.sum()), D, device=dev))
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    pi = ops.l2norm(img.mean(1))
    seg = torch.repeat_interleave(torch.arange(Nc, device=dev), torch.from_numpy(lens.astype(np.int64)).to(dev))
    pc = ops.l2norm(torch.zeros(Nc, D, device=dev).index_add_(0, seg, words))
    coarse = ops.cosine_scores(pi, pc)
    w = weights(D, S, dev)
    lists = {}
    for K in (10, 100):
        r_idx, _, part = ops.topk_lists(coarse, K)
        c_idx, _ = ops.topk_merge_cols([part], K)
        lists[K] = (r_idx, c_idx)
    del coarse
    mods = ("SAF", "SGR")
    S_out = [torch.empty(Ni, Nc, device=dev) for _ in mods]
    kept = {}

    def dense_scoring():
        for mod, out in zip(mods, S_out):
            ops.sgraf_scores(img, words, plan, w, mod, 3, out=out)

    def dense_ensemble():
        dense_scoring()
        avg = (S_out[0].to(torch.float64) + S_out[1].to(torch.float64)) / 2
        kept["dense"] = (avg, ops.rank_counts_f64(avg, 5))

    def ensemble(K):
        r_idx, c_idx = lists[K]
        fine_i, fine_t = [], []
        for mod in mods:                                         # one member's state at a time
            state = ops.sgraf_pairs_prepare(img, words, plan, w, mod, 3)
            fine_i.append(ops.sgraf_candidate_scores(img, words, plan, w, r_idx, 'image', module_name=mod, sgr_step=3, state=state))
            fine_t.append(ops.sgraf_candidate_scores(img, words, plan, w, c_idx, 'caption', module_name=mod, sgr_step=3, state=state))
            del state
        kept[K] = (ops.rerank_fused_lists(r_idx, fine_i), ops.rerank_fused_lists(c_idx, fine_t))

    arms = {"dense scoring (2 x sgraf_scores)": dense_scoring, "dense ensemble (scoring + f64 average + rank_counts_f64)": dense_ensemble}
    for mod in mods:
        arms["prepare %s (inside the ensemble arms)" % mod] = lambda mod=mod: ops.sgraf_pairs_prepare(img, words, plan, w, mod, 3)
    for K in (10, 100):
        arms["ensemble rerank K=%d (2 x (prepare + both directions) + fusion)" % K] = lambda K=K: ensemble(K)
    res = run_arms(arms, a.rounds)
    scoring = res["dense scoring (2 x sgraf_scores)"][0]
    full = res["dense ensemble (scoring + f64 average + rank_counts_f64)"][0]
    for k, (med, mn, quart) in res.items():
        print(json.dumps({"part": "b", "arm": k, "images": Ni, "captions": Nc, "ms_median": round(med, 3), "ms_min": round(mn, 3), "ms_p25_p75": quart,
                          "dense_scoring_over_arm": round(scoring / med, 2), "dense_ensemble_over_arm": round(full / med, 2),
                          "device": name}), flush=True)
    # the fused list scores are the dense average's at the listed pairs (fp32 member scores from two kernels: not bit-equal)
    avg = kept["dense"][0]
    (ri, rf, _, _), (ci, cf, _, _) = kept[100]
    d_i = float((avg.gather(1, ri.to(torch.int64)) - rf).abs().max())
    d_t = float((avg.t().gather(1, ci.to(torch.int64)) - cf).abs().max())
    print(json.dumps({"part": "b", "max_abs_fused_minus_dense_average_K100": {"by_image": d_i, "by_caption": d_t}}), flush=True)


if __name__ == "__main__":
    main()
