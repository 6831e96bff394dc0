#!/usr/bin/env python3
"""Timing of SCAN attention maps for listed pairs against the score-only call on the SAME pairs, interleaved in ONE process on one
device: candidates = the top-10 of a seeded pooled (cosine) matrix at 5 000 x 25 000 (D = 1024, 6..20 words, the inputs
tools/cand_bench.py draws); for m in {1, 5, 10} and both list directions, ops.scan_candidate_attention (first m columns) and
ops.scan_candidate_scores on those m columns.  Prints one JSON line per arm: pairs, median / min ms over the rounds, and the bytes
the call writes (attn + row_sim + score, or the scores alone).  Usage: python tools/attn_bench.py [--ni 5000] [--rounds 3] [--xa both]"""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--xa", default="both", choices=["t2i", "i2t", "both"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    Ni, Nc, D = a.ni, a.ni * 5, a.dim
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = ops.l2norm(torch.randn(Ni, 36, D, device=dev))
    words = ops.l2norm(torch.randn(int(lens.sum()), D, device=dev))
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    pi = ops.l2norm(img.mean(1))
    seg = torch.repeat_interleave(torch.arange(Nc, device=dev), torch.from_numpy(lens.astype(np.int64)).to(dev))
    pc = ops.l2norm(torch.zeros(Nc, D, device=dev).index_add_(0, seg, words))
    coarse = ops.cosine_scores(pi, pc)
    r_idx, _, part = ops.topk_lists(coarse, 10)
    c_idx, _ = ops.topk_merge_cols([part], 10)
    for xa in (["t2i", "i2t"] if a.xa == "both" else [a.xa]):
        ws = ops.scan_pairs_prepare(img, words, plan, xa)
        arms = {}
        for m in (1, 5, 10):
            for by, cand in (("image", r_idx), ("caption", c_idx)):
                sub = cand[:, :m].contiguous()
                pairs = sub.numel()
                caps = sub.reshape(-1).cpu().numpy().astype(np.int64) if by == "image" else np.repeat(np.arange(Nc), m)
                n_words = int(lens[caps].sum())
                attn_bytes = 4 * (n_words * 36 + (n_words if xa == "t2i" else pairs * 36) + pairs)
                arms["attention m=%d by=%s" % (m, by)] = (
                    (lambda c=cand, b=by, m_=m: ops.scan_candidate_attention(img, words, plan, c, b, m=m_, cross_attn=xa, workspace=ws)),
                    pairs, attn_bytes)
                arms["scores m=%d by=%s" % (m, by)] = (
                    (lambda s=sub, b=by: ops.scan_candidate_scores(img, words, plan, s, b, cross_attn=xa, workspace=ws)), pairs, 4 * pairs)
        times = {k: [] for k in arms}
        for k in arms:
            arms[k][0]()                                             # warm-up
        torch.cuda.synchronize()
        for _ in range(a.rounds):                                    # interleaved rounds: every arm once per round
            for k in arms:
                times[k].append(timed(arms[k][0]))
        for k, (fn, pairs, nbytes) in arms.items():
            med, mn = float(np.median(times[k])), float(np.min(times[k]))
            line = {"xa": xa, "arm": k, "pairs": int(pairs), "ms_median": round(med, 3), "ms_min": round(mn, 3), "bytes_written": int(nbytes),
                    "device": torch.cuda.get_device_name(0)}
            if k.startswith("attention"):
                line["attention_over_scores"] = round(med / float(np.median(times[k.replace("attention", "scores")])), 2)
            print(json.dumps(line))
        # the two calls agree on the scores of the same pairs
        att = ops.scan_candidate_attention(img, words, plan, c_idx, 'caption', m=5, cross_attn=xa, workspace=ws)
        sc = ops.scan_candidate_scores(img, words, plan, c_idx[:, :5].contiguous(), 'caption', cross_attn=xa, workspace=ws)
        d = (att.score - sc.reshape(-1)).abs().max()
        print(json.dumps({"xa": xa, "max_abs_attention_score_minus_scores_m5_by_caption": float(d),
                          "bit_equal": bool(torch.equal(att.score.view(torch.int32), sc.reshape(-1).view(torch.int32)))}))


if __name__ == "__main__":
    main()
