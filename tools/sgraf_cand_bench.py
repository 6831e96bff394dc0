#!/usr/bin/env python3
"""Timing of SGRAF candidate-list scoring against the dense call, interleaved in ONE process on one device:
  dense ops.sgraf_scores (5 000 x 25 000, D = 1024, S = 256, bench.py's caption lengths) and ops.sgraf_candidate_scores for K in
  {10, 100} per direction and both, for SAF and SGR.  Candidates = the top-K of a seeded pooled (cosine) matrix in both directions.
Prints one JSON line per arm: pairs, items, median / min ms over the rounds, dense / arm, and the executed-flop fraction = 64-row item
tiles the arm runs through the local-node GEMM over the dense call's 64-column tiles x images (padded rows, the 16-caption limit and
partially filled last items per image included).  The once-per-call preparation is timed as an arm of its own and is NOT part of the
candidate arms (evaluation prepares once and scores both directions).
Usage: python tools/sgraf_cand_bench.py [--ni 5000] [--rounds 3] [--module SAF|SGR|both] [--skip-dense]"""
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


def weights(D, S, dev, steps=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = {}

    def lin(name, o, i):
        r = float(np.sqrt(6.0 / (i + o)))
        w[name + ".weight"] = ((torch.rand(o, i, generator=g) * 2 - 1) * r).to(dev)
        w[name + ".bias"] = (torch.randn(o, generator=g) * 0.02).to(dev)

    def bn(name, n):
        w[name + ".weight"] = (torch.rand(n, generator=g) * 0.4 + 0.8).to(dev)
        w[name + ".bias"] = (torch.randn(n, generator=g) * 0.05).to(dev)
        w[name + ".running_mean"] = (torch.randn(n, generator=g) * 0.1).to(dev)
        w[name + ".running_var"] = (torch.rand(n, generator=g) + 0.5).to(dev)

    lin("v_global_w.embedding_local.0", D, D); bn("v_global_w.embedding_local.1", 36)
    lin("v_global_w.embedding_global.0", D, D); bn("v_global_w.embedding_global.1", D)
    lin("v_global_w.embedding_common.0", 1, D)
    lin("t_global_w.embedding_local.0", D, D); lin("t_global_w.embedding_global.0", D, D); lin("t_global_w.embedding_common.0", 1, D)
    lin("sim_tranloc_w", S, D); lin("sim_tranglo_w", S, D); lin("sim_eval_w", 1, S)
    lin("SAF_module.attn_sim_w", 1, S); bn("SAF_module.bn", 1)
    for k in range(steps):
        for nm in ("graph_query_w", "graph_key_w", "sim_graph_w"):
            lin("SGR_module.sgr%d.%s" % (k, nm), S, S)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--module", default="both", choices=["SAF", "SGR", "both"])
    ap.add_argument("--skip-dense", action="store_true", help="candidate arms only (profiler runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    Ni, Nc, D, S = a.ni, a.ni * 5, a.dim, 256
    lens = rng.randint(6, 21, size=Nc).astype(np.int32)          # bench.py's caption lengths
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
    dense_tiles = float(Ni) * plan.n_tiles
    for mod in (["SAF", "SGR"] if a.module == "both" else [a.module]):
        state = ops.sgraf_pairs_prepare(img, words, plan, w, mod, 3)
        S_out = None if a.skip_dense else torch.empty(Ni, Nc, device=dev)
        items = {}

        def cs(cand, by, key):
            out = ops.sgraf_candidate_scores(img, words, plan, w, cand, by, module_name=mod, sgr_step=3, state=state)
            items[key] = ops.SGRAF_PAIRS_LAST['items']
            return out

        arms = {}
        if not a.skip_dense:
            arms["dense"] = (lambda: ops.sgraf_scores(img, words, plan, w, mod, 3, out=S_out), Ni * Nc)
        arms["prepare (once per call)"] = (lambda: ops.sgraf_pairs_prepare(img, words, plan, w, mod, 3), 0)
        for K in (10, 100):
            r_idx, c_idx = lists[K]
            arms["cand K=%d by=image" % K] = ((lambda r=r_idx, K=K: cs(r, 'image', (K, 'i'))), Ni * K)
            arms["cand K=%d by=caption" % K] = ((lambda c=c_idx, K=K: cs(c, 'caption', (K, 'c'))), Nc * K)
            arms["cand K=%d both" % K] = ((lambda r=r_idx, c=c_idx, K=K: (cs(r, 'image', (K, 'i')), cs(c, 'caption', (K, 'c')))), (Ni + Nc) * K)
        times = {k: [] for k in arms}
        for k in arms:
            arms[k][0]()                                             # warm-up
        torch.cuda.synchronize()
        for _ in range(a.rounds):                                    # interleaved rounds: every arm once per round
            for k in arms:
                times[k].append(timed(arms[k][0]))
        dense_ms = float(np.median(times["dense"])) if "dense" in times else float("nan")
        for k, (fn, pairs) in arms.items():
            med, mn = float(np.median(times[k])), float(np.min(times[k]))
            n_items = None
            if k.startswith("cand"):
                K = int(k.split("K=")[1].split()[0])
                n_items = (items[(K, 'i')] if "image" in k or "both" in k else 0) + (items[(K, 'c')] if "caption" in k or "both" in k else 0)
            print(json.dumps({"module": mod, "arm": k, "pairs": int(pairs), "items": n_items, "ms_median": round(med, 3), "ms_min": round(mn, 3),
                              "dense_over_arm": round(dense_ms / med, 2),
                              "executed_flop_fraction": None if n_items is None else round(n_items / dense_tiles, 5),
                              "chunks_last": ops.SGRAF_PAIRS_LAST.get('chunks'), "device": torch.cuda.get_device_name(0)}), flush=True)
        if a.skip_dense:
            continue
        got = cs(lists[100][1], 'caption', (100, 'c'))
        ref = S_out.gather(0, lists[100][1].to(torch.int64).t()).t()
        print(json.dumps({"module": mod, "max_abs_cand_minus_dense_K100_by_caption": float((got - ref).abs().max())}), flush=True)
        del state, S_out


if __name__ == "__main__":
    main()
