#!/usr/bin/env python3
"""Timing of SGRAF reasoning maps for listed pairs against the score-only call on the SAME pairs, interleaved in ONE process on one
device: candidates = the top-10 of a seeded pooled (cosine) matrix at 5 000 x 25 000 (D = 1024, sim_dim 256, 6..20 words, the
inputs and weights tools/sgraf_cand_bench.py draws); for SAF and SGR, m in {1, 5, 10} and both list directions,
ops.sgraf_candidate_attention (first m columns) and ops.sgraf_candidate_scores on those m columns, with one prepared state.
Prints one JSON line per arm: pairs, items, median / min ms over the rounds, the bytes the call writes (attn + node_w or edge +
score, or the scores alone), and for the explaining arm its time over the score arm's.
Usage: python tools/sgraf_attn_bench.py [--ni 5000] [--rounds 3] [--module both]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--module", default="both", choices=["SAF", "SGR", "both"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    Ni, Nc, D, S, steps = a.ni, a.ni * 5, a.dim, 256, 3
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
    del coarse
    w = weights(D, S, dev, steps)
    for mod in (["SAF", "SGR"] if a.module == "both" else [a.module]):
        state = ops.sgraf_pairs_prepare(img, words, plan, w, mod, steps)
        kw = dict(module_name=mod, sgr_step=steps, state=state)
        arms, items = {}, {}

        def attention(cand, by, m, key):
            out = ops.sgraf_candidate_attention(img, words, plan, w, cand, by, m=m, **kw)
            items[key] = ops.SGRAF_ATTN_LAST['items']
            return out

        def scores(sub, by, key):
            out = ops.sgraf_candidate_scores(img, words, plan, w, sub, by, **kw)
            items[key] = ops.SGRAF_PAIRS_LAST['items']
            return out

        for m in (1, 5, 10):
            for by, cand in (("image", r_idx), ("caption", c_idx)):
                sub = cand[:, :m].contiguous()
                pairs = sub.numel()
                caps = sub.reshape(-1).cpu().numpy().astype(np.int64) if by == "image" else np.repeat(np.arange(Nc), m)
                n = lens[caps].astype(np.int64) + 1
                aux = int((n * n).sum()) * steps if mod == "SGR" else int(n.sum())
                nbytes = 4 * (int(lens[caps].sum()) * 36 + aux + pairs)
                ka, ks = "attention m=%d by=%s" % (m, by), "scores m=%d by=%s" % (m, by)
                arms[ka] = ((lambda c=cand, b=by, m_=m, k_=ka: attention(c, b, m_, k_)), pairs, nbytes)
                arms[ks] = ((lambda s=sub, b=by, k_=ks: scores(s, b, k_)), pairs, 4 * pairs)
        times = {k: [] for k in arms}
        for k in arms:
            arms[k][0]()                                             # warm-up
        torch.cuda.synchronize()
        for _ in range(a.rounds):                                    # interleaved rounds: every arm once per round
            for k in arms:
                times[k].append(timed(arms[k][0]))
        for k, (fn, pairs, nbytes) in arms.items():
            med, mn = float(np.median(times[k])), float(np.min(times[k]))
            line = {"module": mod, "arm": k, "pairs": int(pairs), "items": int(items[k]), "ms_median": round(med, 3), "ms_min": round(mn, 3),
                    "bytes_written": int(nbytes), "device": torch.cuda.get_device_name(0)}
            if k.startswith("attention"):
                line["attention_over_scores"] = round(med / float(np.median(times[k.replace("attention", "scores")])), 2)
            print(json.dumps(line), flush=True)
        # the two calls agree on the scores of the same pairs
        att = ops.sgraf_candidate_attention(img, words, plan, w, c_idx, 'caption', m=5, **kw)
        sc = ops.sgraf_candidate_scores(img, words, plan, w, c_idx[:, :5].contiguous(), 'caption', **kw)
        d = (att.score - sc.reshape(-1)).abs().max()
        print(json.dumps({"module": mod, "max_abs_attention_score_minus_scores_m5_by_caption": float(d),
                          "bit_equal": bool(torch.equal(att.score.view(torch.int32), sc.reshape(-1).view(torch.int32)))}), flush=True)


if __name__ == "__main__":
    main()
