#!/usr/bin/env python3
"""Hubness correction: what the statistics cost beside the one-pass readers already in the tree.  GPU only, seeded inputs, one
process, warmed up, medians of interleaved repetitions (HIP events around each op); one JSON line per measurement on stdout (and
appended to --out).

  matrix   a seeded score matrix (1 000 x 5 000 and 5 000 x 25 000), float32 and float64:
             ops.hub_lse_fold (both directions, rows only, columns only), the CSLS path (ops.topk_lists + topk_merge_cols +
             hub_list_mean twice, k = 10) and ops.hub_adjust, beside ops.rank_counts (float32) / ops.rank_counts_f64 (float64) on
             the same matrix.  Read rate = the matrix's bytes over the time; `vs_rank` = rate of the op over rate of the ranker.
             Also the largest error of the fold against a float64 torch.logsumexp of the same matrix (a check that the timed code
             computes the statistic, not the tests' oracle).
  bank     a 113 287-image bank against a 25 000-caption gallery, synthetic pooled embeddings (D = 1024), folded in 640-row blocks:
             wall time of scoring alone (ops.cosine_scores per block) and of scoring + ops.hub_lse_fold(rows=False) /
             + ops.topk_fold_cols (k = 10); host clock around work that ends in a device synchronise.

    python3 tools/hubness_bench.py matrix|bank [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from itr_amd import ops  # noqa: E402


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median_us": round(float(np.median(xs)), 1), "min_us": round(float(xs.min()), 1), "max_us": round(float(xs.max()), 1)}


def bench_matrix(a):
    dev = torch.device("cuda", 0)
    beta, k = 20.0, 10
    for ni, nc in ((1000, 5000), (5000, 25000)):
        for f64 in (False, True):
            g = torch.Generator(device=dev)
            g.manual_seed(0)
            S = torch.randn(ni, nc, device=dev, generator=g).clamp_(-4, 4).mul_(0.25)       # scores in [-1, 1]
            if f64:
                S = S.double()
            nbytes = S.numel() * S.element_size()
            state = torch.zeros(nc, 2, device=dev, dtype=torch.float64)
            out = torch.empty_like(S)
            va = torch.zeros(ni, device=dev, dtype=torch.float64)
            vb = torch.zeros(nc, device=dev, dtype=torch.float64)

            def csls():
                _, r_val, part = ops.topk_lists(S, k)
                _, c_val = ops.topk_merge_cols([part], k)
                return ops.hub_list_mean(r_val, k), ops.hub_list_mean(c_val, k)
            fns = {
                "rank": (lambda: ops.rank_counts_f64(S, 5)) if f64 else (lambda: ops.rank_counts(S, 5)),
                "hub_lse_fold": lambda: ops.hub_lse_fold(S, beta, state=state.zero_()),
                "hub_lse_fold_rows": lambda: ops.hub_lse_fold(S, beta, cols=False),
                "hub_lse_fold_cols": lambda: ops.hub_lse_fold(S, beta, state=state.zero_(), rows=False),
                "csls_k10": csls,
                "hub_adjust": lambda: ops.hub_adjust(S, va, vb, out=out),
            }
            # the timed fold against torch's float64 logsumexp
            row, st = ops.hub_lse_fold(S, beta)
            col = ops.hub_lse_cols(st, beta)
            Sd = S.double() * beta
            err = max(float((row - torch.logsumexp(Sd, 1) / beta).abs().max()), float((col - torch.logsumexp(Sd, 0) / beta).abs().max()))
            del Sd
            times = {name: [] for name in fns}
            for it in range(a.warmup + a.reps):
                for name, fn in fns.items():
                    t = timed(fn)
                    if it >= a.warmup:
                        times[name].append(t)
            rank_us = float(np.median(times["rank"]))
            for name in fns:
                st_ = stats(times[name])
                moved = nbytes * (2 if name == "hub_adjust" else 1)
                emit(a, {"bench": "matrix", "op": name, "shape": [ni, nc], "dtype": "float64" if f64 else "float32", "reps": a.reps,
                         "matrix_bytes": nbytes, **st_, "GBps": round(moved / (st_["median_us"] * 1e-6) / 1e9, 1),
                         "vs_rank": round(rank_us / st_["median_us"] * (moved / nbytes), 3),
                         "ranker": "rank_counts_f64 (+ t2i top1 pass)" if f64 else "rank_counts",
                         **({"max_abs_err_vs_torch_logsumexp": err} if name == "hub_lse_fold" else {})})
    return 0


def bench_bank(a):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    qi, nc, d, rows, k, beta = a.bank, a.nc, a.dim, a.rows, 10, 20.0
    bank = torch.nn.functional.normalize(torch.randn(qi, d, device=dev, generator=g), dim=1)
    cap = torch.nn.functional.normalize(torch.randn(nc, d, device=dev, generator=g), dim=1)
    buf = torch.empty(rows * nc, device=dev)

    def run(what):
        state = None
        for r0 in range(0, qi, rows):
            r1 = min(qi, r0 + rows)
            S = ops.cosine_scores(bank[r0:r1], cap, out=buf[:(r1 - r0) * nc].view(r1 - r0, nc))
            if what == "lse":
                _, state = ops.hub_lse_fold(S, beta, state=state, rows=False)
            elif what == "csls":
                state = ops.topk_fold_cols(S, k, r0, state)
        if what == "lse":
            return ops.hub_lse_cols(state, beta)
        if what == "csls":
            return ops.hub_list_mean(ops.topk_merge_cols([state], k)[1], k)
    for what in ("score", "lse", "csls"):       # warm-up: every shape of the timed window
        run(what)
    times = {"score": [], "lse": [], "csls": []}
    for it in range(a.bank_reps):
        for what in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(what)
            torch.cuda.synchronize()
            times[what].append(time.perf_counter() - t0)
    med = {w: float(np.median(v)) for w, v in times.items()}
    emit(a, {"bench": "bank", "bank_images": qi, "gallery_captions": nc, "dim": d, "rows_per_block": rows, "reps": a.bank_reps,
             "matrix_bytes_never_stored": qi * nc * 4, "score_only_s": round(med["score"], 4),
             "score_plus_hub_lse_fold_s": round(med["lse"], 4), "score_plus_topk_fold_cols_k10_s": round(med["csls"], 4),
             "hub_lse_fold_share_s": round(med["lse"] - med["score"], 4),
             "fold_GBps": round(qi * nc * 4 / max(med["lse"] - med["score"], 1e-9) / 1e9, 1),
             "note": "host clock around a device synchronise; the fold's share is the difference of two medians"})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["matrix", "bank"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bank", type=int, default=113287)
    ap.add_argument("--bank-reps", type=int, default=20)
    ap.add_argument("--nc", type=int, default=25000)
    ap.add_argument("--rows", type=int, default=640)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("hubness_bench: no GPU (a measurement does not fall back)", file=sys.stderr)
        return 2
    return {"matrix": bench_matrix, "bank": bench_bank}[a.what](a)


if __name__ == "__main__":
    sys.exit(main())
