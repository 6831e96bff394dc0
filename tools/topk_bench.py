#!/usr/bin/env python3
"""Top-K retrieval lists at the headline shape: a seeded 5 000 x 25 000 fp32 similarity matrix.  One process, interleaved
rounds, warmed up; medians of HIP-event timings of
  itr_topk (ops.topk_lists + the column merge) for i2t, t2i and both, at K = 1, 10, 100;
  ops.rank_counts on the same tensor;
  torch.topk(S, K, dim=1) + torch.topk(S, K, dim=0);
and the achieved read rate against 8 TB/s (bytes of S read once per direction).  Checks its own output against torch.topk
(the score multisets of every line must be equal).  Prints one JSON line.
    python3 tools/topk_bench.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from itr_amd import ops  # noqa: E402

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--nc", type=int, default=25000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    S = torch.randn(a.ni, a.nc, device=dev, generator=g)
    nbytes = S.numel() * 4

    def topk(k, rows, cols):
        def run():
            ri, rv, part = ops.topk_lists(S, k, rows=rows, cols=cols)
            if cols:
                ops.topk_merge_cols([part], k)
        return run
    cases = {}
    for k in (1, 10, 100):
        cases["topk_i2t_k%d" % k] = (topk(k, True, False), nbytes)
        cases["topk_t2i_k%d" % k] = (topk(k, False, True), nbytes)
        cases["topk_both_k%d" % k] = (topk(k, True, True), 2 * nbytes)
        cases["torch_topk_pair_k%d" % k] = ((lambda k=k: (torch.topk(S, k, dim=1), torch.topk(S, k, dim=0))), 2 * nbytes)
    cases["rank_counts"] = ((lambda: ops.rank_counts(S)), nbytes)

    # self-check against torch.topk: equal score multisets per line (the order of equal scores is torch's own)
    ok = True
    for k in (1, 10, 100):
        ri, rv, part = ops.topk_lists(S, k)
        ci, cv = ops.topk_merge_cols([part], k)
        tr, tc = torch.topk(S, k, dim=1).values, torch.topk(S, k, dim=0).values.t()
        ok = ok and torch.equal(torch.sort(rv, 1).values, torch.sort(tr, 1).values)
        ok = ok and torch.equal(torch.sort(cv, 1).values, torch.sort(tc, 1).values)
        ok = ok and torch.equal(torch.gather(S, 1, ri.long()), rv)

    times = {name: [] for name in cases}
    for it in range(a.warmup + a.reps):
        for name, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"shape": [a.ni, a.nc], "reps": a.reps, "check_vs_torch_topk": bool(ok), "unit": "us"}
    for name, (_, b) in cases.items():
        med = float(np.median(times[name]))
        out[name] = round(med, 1)
        out[name + "_p25_p75"] = [round(float(np.percentile(times[name], p)), 1) for p in (25, 75)]
        out[name + "_TBps"] = round(b / (med * 1e-6) / 1e12, 2)
        out[name + "_frac_8TBps"] = round(b / (med * 1e-6) / HBM, 3)
    out["faster_than_torch_pair"] = {k: out["topk_both_k%d" % k] < out["torch_topk_pair_k%d" % k] for k in (1, 10, 100)}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
