#!/usr/bin/env python3
"""Positions under a general ground-truth relation (ops.rank_positions, csrc/rank_gt.hip): what they cost beside the one-threshold
ranker and beside sorting.  A seeded 5 000 x 25 000 fp32 matrix, one process, warmed up, medians of interleaved repetitions with
p25 / p75, HIP events around the ops calls; one JSON line per arm on stdout (and appended to --out).

  a  ops.rank_counts(S, 5)                         the one-threshold ranker on the same matrix
  b  ops.rank_positions, 5-captions-per-image relation
  c  ops.rank_positions, extended relation: 5 .. 40 positive captions per image (seeded; the layout pairs included)
  d  what can be done without the kernel, on the device: torch.argsort of S along both dimensions, the inverse permutations and
     the gathers that turn them into the positions of (c)'s relation

--signal X adds X to the score of every positive of (c)'s relation: 0 (default) is an untrained model, where almost every element
passes a query's smallest threshold; a few standard deviations is a trained one, where almost none does.

  kernel-times  no GPU work: reads the kernel trace (CSV) of a `rocprofv3 --kernel-trace` run of this tool and prints the duration
            of every kernel of (a), (b), (c) by name.

    python3 tools/rank_gt_bench.py run [--reps 20] [--warmup 3] [--signal 0] [--arms abcd] [--out FILE]
    python3 tools/rank_gt_bench.py kernel-times --trace KERNEL_TRACE.csv [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from itr_amd import ops  # noqa: E402

ONE_PASS_RANKER_TBPS = 4.07          # rank_fused_kernel at 5 000 x 25 000


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


def extended_pairs(ni, nc, seed):
    """5 .. 40 positive captions per image: the image's own 5 and random others."""
    rng = np.random.RandomState(seed)
    img, cap = [], []
    for i in range(ni):
        own = np.arange(5 * i, min(5 * i + 5, nc))
        more = rng.randint(0, nc, size=rng.randint(0, 36))
        c = np.unique(np.concatenate([own, more]))
        img.append(np.full(len(c), i))
        cap.append(c)
    return np.stack([np.concatenate(img), np.concatenate(cap)], 1)


def sort_positions(S, gt, entry_img, entry_cap):
    """(d): positions through two full sorts.  entry_img: the image of every image-CSR entry; entry_cap: the caption of every
    caption-CSR entry (both int64, on the device, built once outside the timing)."""
    ni, nc = S.shape
    order = torch.argsort(S, dim=1, descending=True)
    where = torch.empty_like(order)
    where.scatter_(1, order, torch.arange(nc, device=S.device).expand(ni, nc))
    i_pos = where[entry_img, gt.img_cap.long()]
    order = torch.argsort(S, dim=0, descending=True)
    where.scatter_(0, order, torch.arange(ni, device=S.device).view(ni, 1).expand(ni, nc))
    t_pos = where[gt.cap_img.long(), entry_cap]
    return i_pos, t_pos


def run(a):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    S = torch.randn(a.ni, a.nc, device=dev, generator=g)
    gt_b = ops.GroundTruth.from_layout(a.ni, a.nc, 5, dev)
    pairs = extended_pairs(a.ni, a.nc, a.seed)
    gt_c = ops.GroundTruth(pairs, a.ni, a.nc, dev)
    if a.signal:
        p = torch.from_numpy(pairs).to(dev)
        S[p[:, 0], p[:, 1]] += a.signal
    entry_img = torch.repeat_interleave(torch.arange(a.ni, device=dev), torch.from_numpy(np.diff(gt_c.img_ptr_host)).to(dev).long())
    entry_cap = torch.repeat_interleave(torch.arange(a.nc, device=dev), torch.from_numpy(np.diff(gt_c.cap_ptr_host)).to(dev).long())
    arms = {"a": ("rank_counts, im_div 5", lambda: ops.rank_counts(S, 5)),
            "b": ("rank_positions, 5-per-image relation", lambda: ops.rank_positions(S, gt_b)),
            "c": ("rank_positions, extended relation", lambda: ops.rank_positions(S, gt_c)),
            "d": ("two torch.argsort + inverse permutations + gathers, extended relation", lambda: sort_positions(S, gt_c, entry_img, entry_cap))}
    arms = {k: v for k, v in arms.items() if k in a.arms}
    # the arms agree before anything is timed
    checks, info = {}, {}
    if "c" in arms and "d" in arms:
        # (d) breaks exact ties arbitrarily, the ranker by index: seeded fp32 normals do repeat inside a line, so a few entries may
        # differ by the size of their tie group; exactness is the test suite's business (tests/test_rank_gt_gpu.py)
        got, want = arms["c"][1](), arms["d"][1]()
        diff = torch.cat([(got[0].long() - want[0]).abs(), (got[1].long() - want[1]).abs()])
        info = {"c_vs_d_entries_differing": int((diff != 0).sum()), "c_vs_d_max_position_difference": int(diff.max())}
    if "a" in arms and "b" in arms:
        i_rank, _, t_rank, _, _ = arms["a"][1]()
        i_pos, t_pos, _ = arms["b"][1]()
        checks["b_equals_a"] = bool(torch.equal(i_pos.view(a.ni, 5).min(1).values, i_rank) and torch.equal(t_pos, t_rank))
    times = {k: [] for k in arms}
    for it in range(a.warmup + a.reps):
        for k, (_, fn) in arms.items():
            t = timed(fn)
            if it >= a.warmup:
                times[k].append(t)
    nbytes = a.ni * a.nc * 4
    passes = {"a": 1, "b": 2, "c": 2}
    recs = {}
    for k, (name, _) in arms.items():
        rec = {"bench": "rank_gt", "arm": k, "what": name, "shape": [a.ni, a.nc], "seed": a.seed, "signal": a.signal, "reps": a.reps,
               "timing": "HIP events around the ops call", "matrix_bytes": nbytes}
        rec.update(stats(times[k]))
        rec["samples_us"] = [round(x, 1) for x in times[k]]
        if k in ("b", "c"):
            rec["nnz"] = (gt_b if k == "b" else gt_c).nnz
        if k in passes:
            rec["passes_over_S"] = passes[k]
            rec["read_TBps"] = round(passes[k] * nbytes / (rec["median_us"] * 1e-6) / 1e12, 3)
            rec["read_rate_over_one_pass_ranker"] = round(rec["read_TBps"] / ONE_PASS_RANKER_TBPS, 3)
        rec.update(checks)
        rec.update(info)
        recs[k] = rec
    for k in ("b", "c"):
        if k in recs and "d" in recs:
            # faster than the sort by more than the two spreads (interquartile ranges)
            spreads = (recs["d"]["p75_us"] - recs["d"]["p25_us"]) + (recs[k]["p75_us"] - recs[k]["p25_us"])
            recs[k]["d_over_this"] = round(recs["d"]["median_us"] / recs[k]["median_us"], 1)
            recs[k]["faster_than_d_beyond_spreads"] = bool(recs["d"]["median_us"] - recs[k]["median_us"] > spreads)
        if k in recs and "a" in recs:
            recs[k]["this_over_a"] = round(recs[k]["median_us"] / recs["a"]["median_us"], 2)
    for rec in recs.values():
        emit(a, rec)
    return 0 if all(checks.values()) else 1


KERNELS = ("rank_prepare_kernel", "rank_fused_kernel", "rank_rows_finish_kernel", "gt_gather_kernel", "gt_sort_kernel", "gt_rows_kernel",
           "gt_cols_kernel")


def kernel_times(a):
    import csv
    rows = list(csv.DictReader(open(a.trace)))
    nbytes = a.ni * a.nc * 4
    for name in KERNELS:
        xs = np.asarray([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]) / 1e3
        if not len(xs):
            continue
        rec = {"bench": "rank_gt_kernel_time", "source": "rocprofv3 --kernel-trace", "kernel": name, "calls": int(len(xs)),
               "shape": [a.ni, a.nc], "note": "all arms and relations that launch it together"}
        rec.update(stats(xs))
        if name in ("rank_fused_kernel", "gt_rows_kernel", "gt_cols_kernel"):
            rec["read_TBps_at_median"] = round(nbytes / (rec["median_us"] * 1e-6) / 1e12, 3)
        emit(a, rec)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["run", "kernel-times"])
    ap.add_argument("--trace", default=None, help="kernel-times: the *_kernel_trace.csv of a rocprofv3 --kernel-trace run of `run`")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ni", type=int, default=5000)
    ap.add_argument("--nc", type=int, default=25000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--signal", type=float, default=0.0)
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel-times":
        return kernel_times(a)
    if not torch.cuda.is_available():
        print("rank_gt_bench: no GPU (a measurement does not fall back)", file=sys.stderr)
        return 2
    return run(a)


if __name__ == "__main__":
    sys.exit(main())
