#!/usr/bin/env python3
"""Top-K lists without the similarity matrix in memory: what the pieces cost.  Seeded inputs, one process, warmed up, medians of
interleaved repetitions; one JSON line per measurement on stdout (and appended to --out).

  fold      a seeded 5 000 x 25 000 fp32 matrix in 640-row blocks, K = 1, 10, 100: ops.topk_fold_cols of one block into the state of
            the blocks before it -- the first block (empty lists) and every later one (steady state) -- against what the same block
            costs today: ops.topk_lists(blk, k, rows=False) plus a two-part itr_topk_merge with the lists so far (timed separately
            and together).  HIP-event timings; the read rate is the block's bytes over the time.  Checks the folded lists against
            topk_lists + topk_merge_cols of the whole matrix, bit for bit.
  streamed  cosine, D = 1024, 5 000 x 25 000: evalpipe.score_topk_streamed against cosine_scores + finalize_topk + finalize_ranks
            of the materialised matrix (host clock around work that ends in the copies to the host).
  big       the shape that cannot be materialised: 113 287 x 566 435, D = 1024, k = 100 (coco_precomp train), once with and once
            without the row pass: wall time per stage and the peak memory of the process.  No reference exists at this size.

  kernel-times  no GPU work: reads the kernel trace (CSV) of a `rocprofv3 --kernel-trace` run of `fold` with the same --reps /
            --warmup and prints the fold kernel's own duration per K and block (the event timings above include the launch).

    python3 tools/topk_stream_bench.py fold|streamed|big [--reps 20] [--warmup 3] [--out FILE]
    python3 tools/topk_stream_bench.py kernel-times --trace KERNEL_TRACE.csv [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from itr_amd import evalpipe, ops  # noqa: E402


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
    return {"median_us": round(float(np.median(xs)), 1), "min_us": round(float(xs.min()), 1), "max_us": round(float(xs.max()), 1),
            "p25_us": round(float(np.percentile(xs, 25)), 1), "p75_us": round(float(np.percentile(xs, 75)), 1)}


def bench_fold(a):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    S = torch.randn(a.ni, a.nc, device=dev, generator=g)
    blocks = [(r0, min(a.ni, r0 + a.rows)) for r0 in range(0, a.ni, a.rows)]
    for k in (1, 10, 100):
        # the state before every block (and the self-check of the last one against the whole-matrix path)
        before, state = [], None
        for r0, r1 in blocks:
            before.append(None if state is None else (state[0].clone(), state[1].clone()))
            state = ops.topk_fold_cols(S[r0:r1], k, r0, state)
        whole = ops.topk_lists(S, k, rows=False)[2]
        ok = torch.equal(state[0], whole[0]) and torch.equal(state[1].view(torch.int32), whole[1].view(torch.int32))
        before[0] = (torch.zeros_like(state[0]), torch.zeros_like(state[1]))
        work = (torch.empty_like(state[0]), torch.empty_like(state[1]))
        t_fold = [[] for _ in blocks]
        t_cols = [[] for _ in blocks]
        t_merge = [[] for _ in blocks]
        for it in range(a.warmup + a.reps):
            for b, (r0, r1) in enumerate(blocks):
                blk = S[r0:r1]
                work[0].copy_(before[b][0])
                work[1].copy_(before[b][1])
                tf = timed(lambda: ops.topk_fold_cols(blk, k, r0, work))
                part = [None]

                def cols():
                    part[0] = ops.topk_lists(blk, k, r0, rows=False)[2]
                tc = timed(cols)
                tm = timed(lambda: ops.topk_merge_cols([before[b], part[0]], k))
                if it >= a.warmup:
                    t_fold[b].append(tf)
                    t_cols[b].append(tc)
                    t_merge[b].append(tm)
        nbytes = (blocks[0][1] - blocks[0][0]) * a.nc * 4
        steady = slice(1, len(blocks) - 1 if (blocks[-1][1] - blocks[-1][0]) != a.rows and len(blocks) > 2 else len(blocks))
        for name, sel in (("first_block", slice(0, 1)), ("steady_state_blocks", steady)):
            f = [x for xs in t_fold[sel] for x in xs]
            c = [x for xs in t_cols[sel] for x in xs]
            m = [x for xs in t_merge[sel] for x in xs]
            p = [x + y for xs, ys in zip(t_cols[sel], t_merge[sel]) for x, y in zip(xs, ys)]
            if not f:
                continue
            rec = {"bench": "fold", "which": name, "shape": [a.ni, a.nc], "rows_per_block": a.rows, "k": k, "reps": a.reps,
                   "blocks": list(range(len(blocks)))[sel], "block_bytes": nbytes, "equals_whole_matrix_lists": bool(ok),
                   "fold": stats(f), "parent_topk_cols": stats(c), "parent_merge_2_parts": stats(m), "parent_cols_plus_merge": stats(p)}
            rec["fold_TBps"] = round(nbytes / (rec["fold"]["median_us"] * 1e-6) / 1e12, 3)
            rec["parent_topk_cols_TBps"] = round(nbytes / (rec["parent_topk_cols"]["median_us"] * 1e-6) / 1e12, 3)
            rec["fold_over_parent"] = round(rec["fold"]["median_us"] / rec["parent_cols_plus_merge"]["median_us"], 3)
            emit(a, rec)
        per_block = {"bench": "fold_per_block", "k": k, "rows_per_block": a.rows, "shape": [a.ni, a.nc],
                     "fold_median_us": [round(float(np.median(x)), 1) for x in t_fold],
                     "parent_cols_plus_merge_median_us": [round(float(np.median(np.add(x, y))), 1) for x, y in zip(t_cols, t_merge)]}
        emit(a, per_block)
        if not ok:
            return 1
    return 0


def bench_streamed(a):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    img = torch.nn.functional.normalize(torch.randn(a.ni, a.dim, device=dev, generator=g), dim=1)
    cap = torch.nn.functional.normalize(torch.randn(a.nc, a.dim, device=dev, generator=g), dim=1)
    comm = evalpipe.Comm()
    for k in (10, 100):
        def materialised():
            S = ops.cosine_scores(img, cap)
            return evalpipe.finalize_topk(comm, S, 0, a.ni, k), evalpipe.finalize_ranks(comm, S, 0, a.ni, 5)

        def streamed():
            return evalpipe.score_topk_streamed(img, cap, ops.cosine_scores, k, 5)
        want, got = materialised(), streamed()
        ok = all(np.array_equal(x, y) for x, y in zip(want[0] + want[1], got[0] + got[1]))
        times = {"materialised": [], "streamed": []}
        for it in range(a.warmup + a.reps):
            for name, fn in (("materialised", materialised), ("streamed", streamed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e6)
        rec = {"bench": "streamed_vs_materialised", "scorer": "cosine", "shape": [a.ni, a.nc], "dim": a.dim, "k": k, "reps": a.reps,
               "equal_lists_and_ranks": bool(ok), "materialised": stats(times["materialised"]), "streamed": stats(times["streamed"]),
               "note": "host clock, lists and ranks copied to the host in both forms"}
        emit(a, rec)
        if not ok:
            return 1
    return 0


def bench_big(a):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    ni, nc, d, k = a.big_ni, a.big_nc, a.dim, 100
    img = torch.nn.functional.normalize(torch.randn(ni, d, device=dev, generator=g), dim=1)
    cap = torch.nn.functional.normalize(torch.randn(nc, d, device=dev, generator=g), dim=1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    # stage 0: the scoring alone, in score_topk_streamed's blocks (what every consumer's time is added to)
    rb = max(128, ((64 << 20) // (4 * nc)) // 128 * 128)
    buf = torch.empty(rb * nc, device=dev)
    t0 = time.perf_counter()
    for r0 in range(0, ni, rb):
        r1 = min(ni, r0 + rb)
        ops.cosine_scores(img[r0:r1], cap, out=buf[:(r1 - r0) * nc].view(r1 - r0, nc))
    torch.cuda.synchronize()
    emit(a, {"bench": "big", "stage": "cosine_scores of every block alone", "shape": [ni, nc], "dim": d, "rows_per_block": rb,
             "wall_s": round(time.perf_counter() - t0, 2)})
    del buf
    for rows in (False, True):
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evalpipe.score_topk_streamed(img, cap, ops.cosine_scores, k, 5, ranks=rows, rows=rows)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        lists = out[0] if rows else out
        # spot check, no reference exists at this size: the first entry of some columns is the column's maximum over all rows
        cols = [0, 1, nc // 2, nc - 1]
        best = torch.stack([ops.cosine_scores(img, cap[c:c + 1].contiguous()).view(-1).max() for c in cols]).cpu().numpy()
        rec = {"bench": "big", "shape": [ni, nc], "dim": d, "k": k, "rows": rows, "ranks": rows, "cols": True, "wall_s": round(wall, 2),
               "matrix_bytes_never_stored": ni * nc * 4, "embedding_bytes": int(base),
               "peak_device_bytes": int(torch.cuda.max_memory_allocated()),
               "peak_host_rss_bytes": int(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss) * 1024,
               "t2i_list_shape": list(lists[2].shape), "top1_is_column_max": bool((lists[3][cols, 0] == best).all()),
               "reference": "none exists at this size; correctness rests on the partition tests"}
        emit(a, rec)
        del out, lists
    return 0


def kernel_times(a):
    """bench_fold launches the fold kernel, per K: once per block (building the states), then (warmup + reps) x blocks"""
    import csv
    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {name: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
           for name in ("topk_fold_kernel", "topk_cols_kernel", "topk_merge_kernel")}
    heights = [min(a.ni, r0 + a.rows) - r0 for r0 in range(0, a.ni, a.rows)]
    nb = len(heights)
    per_k = nb + (a.warmup + a.reps) * nb
    if len(dur["topk_fold_kernel"]) != 3 * per_k:
        print("kernel-times: %d fold dispatches in the trace, %d expected for --reps %d --warmup %d"
              % (len(dur["topk_fold_kernel"]), 3 * per_k, a.reps, a.warmup), file=sys.stderr)
        return 1
    for ki, k in enumerate((1, 10, 100)):
        seg = dur["topk_fold_kernel"][ki * per_k + nb:(ki + 1) * per_k]
        for b in range(nb):
            xs = np.asarray([seg[it * nb + b] for it in range(a.warmup, a.warmup + a.reps)]) / 1e3
            med = float(np.median(xs))
            emit(a, {"bench": "fold_kernel_time", "source": "rocprofv3 --kernel-trace", "k": k, "block": b, "rows": heights[b],
                     "shape": [a.ni, a.nc], "median_us": round(med, 1), "min_us": round(float(xs.min()), 1),
                     "max_us": round(float(xs.max()), 1), "TBps": round(heights[b] * a.nc * 4 / (med * 1e-6) / 1e12, 2)})
    for name in ("topk_cols_kernel", "topk_merge_kernel"):
        xs = np.asarray(dur[name]) / 1e3
        emit(a, {"bench": "parent_kernel_time", "source": "rocprofv3 --kernel-trace", "kernel": name, "calls": len(xs),
                 "note": "all K and blocks together (and the whole-matrix self-check calls)", "median_us": round(float(np.median(xs)), 1),
                 "min_us": round(float(xs.min()), 1), "max_us": round(float(xs.max()), 1)})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fold", "streamed", "big", "kernel-times"])
    ap.add_argument("--trace", default=None, help="kernel-times: the *_kernel_trace.csv of a rocprofv3 --kernel-trace run of `fold`")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--nc", type=int, default=25000)
    ap.add_argument("--rows", type=int, default=640)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--big-ni", type=int, default=113287)
    ap.add_argument("--big-nc", type=int, default=566435)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel-times":
        return kernel_times(a)
    if not torch.cuda.is_available():
        print("topk_stream_bench: no GPU (a measurement does not fall back)", file=sys.stderr)
        return 2
    return {"fold": bench_fold, "streamed": bench_streamed, "big": bench_big}[a.what](a)


if __name__ == "__main__":
    sys.exit(main())
