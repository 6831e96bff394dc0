#!/usr/bin/env python3
"""Query-time search: ops.search_topk (csrc/search.hip, one fused pass over the gallery) beside the path the tree had before it,
ops.cosine_scores + ops.topk_lists(cols=False) (the 128 x 128 tile GEMM writes the [Q, N] matrix, one workgroup per query selects).
GPU only, seeded l2-normalised inputs, one process, warmed up, the two paths interleaved, HIP events around the ops calls, medians of
--reps with the quartiles; one JSON line per measurement on stdout (and appended to --out, by default profiles/search/bench.jsonl).

Grid: N in {5 000, 113 287, 566 435} gallery rows of D = 1 024, Q in {1, 16, 64} queries, K in {10, 100}.  Reported per cell and path:
microseconds, gallery bytes / time in TB/s, and the time the gallery takes at 6.3 TB/s (the floor: the gallery has to be read once).
Before a cell is timed the two paths' lists are compared: indices equal, score bits equal.

    python3 tools/search_bench.py [--reps 20] [--warmup 3] [--n 5000,113287,566435] [--q 1,16,64] [--k 10,100] [--dim 1024] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from itr_amd import ops  # noqa: E402

HBM_TBPS = 6.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def quartiles(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median_us": round(float(np.median(xs)), 1), "p25_us": round(float(np.percentile(xs, 25)), 1),
            "p75_us": round(float(np.percentile(xs, 75)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", default="5000,113287,566435")
    ap.add_argument("--q", default="1,16,64")
    ap.add_argument("--k", default="10,100")
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("search_bench: no GPU (a measurement does not fall back)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in [int(x) for x in a.n.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        G = torch.nn.functional.normalize(torch.randn(n, a.dim, device=dev, generator=g), dim=1)
        gbytes = G.numel() * 4
        for nq in [int(x) for x in a.q.split(",")]:
            Q = torch.nn.functional.normalize(torch.randn(nq, a.dim, device=dev, generator=g), dim=1)
            S = torch.empty(nq, n, device=dev)
            for k in [int(x) for x in a.k.split(",")]:
                fns = {"fused": lambda: ops.search_topk(Q, G, k),
                       "matrix": lambda: ops.topk_lists(ops.cosine_scores(Q, G, out=S), k, cols=False)}
                fi, fv, _ = fns["fused"]()
                mi, mv, _ = fns["matrix"]()
                torch.cuda.synchronize()
                same = bool(torch.equal(fi, mi)) and bool(torch.equal(fv.view(torch.int32), mv.view(torch.int32)))
                times = {name: [] for name in fns}
                for it in range(a.warmup + a.reps):
                    for name, fn in fns.items():
                        t = timed(fn)
                        if it >= a.warmup:
                            times[name].append(t)
                med = {}
                for name in fns:
                    st = quartiles(times[name])
                    med[name] = st["median_us"]
                    rec = {"bench": "search", "path": name, "N": n, "D": a.dim, "Q": nq, "K": k, "reps": a.reps, "gallery_bytes": gbytes,
                           **st, "gallery_TBps": round(gbytes / (st["median_us"] * 1e-6) / 1e12, 3),
                           "floor_us_at_6.3TBps": round(gbytes / (HBM_TBPS * 1e12) * 1e6, 1), "lists_equal_bitwise": same}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                print("# N=%d Q=%d K=%d: fused %.1f us, matrix %.1f us, matrix / fused = %.2f" % (n, nq, k, med["fused"], med["matrix"],
                                                                                                 med["matrix"] / med["fused"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
