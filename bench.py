#!/usr/bin/env python3
"""Headline benchmark: pairs/sec scored on the MS-COCO 5k x 25k evaluation (BASELINE.json metric).

Workload (default `scan_t2i_coco5k`, BASELINE.json configs[2]): SCAN t2i LogSumExp,
5 000 images x 36 regions x 2048-d precomp features, 25 000 captions of 6..20 tokens, coco vocabulary
(11 353), word_dim 300, bi-GRU, embed 1024.  One "step" = the whole metric path on inputs already
resident in HBM:   image projection + l2norm -> embedding + bi-GRU -> [all-gather of word embeddings]
-> fused SCAN cross-attention scores (N_img x N_cap) -> Recall ranks (i2t + t2i).

    python bench.py                      # 1 GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N      # N GPUs, one rank per GPU over RCCL

The 5k x 25k score matrix is row-sharded over ranks (strong scaling: total work is fixed).
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: nothing else.  Everything else the
line can carry runs only with --full, after the timed steps: the CPU baseline and its Recall parity check, the fp16x3 study
variant, the sustained-clock probe, the short runs of the other BASELINE.json configs, the training-step timings and the
materialised re-run of --stream-scores.  Each --no-* switch drops its part of a --full run.

Exit codes: 0 clean run; 2 refused launch (--gpus / WORLD_SIZE / device count mismatch); 3 the ranks missed the initialisation
deadline and 4 Recall parity against the CPU sample failed (--full; the line is still printed); 5 --launch-check: a fabric
collective failed; 6 the primary line was printed but a SECONDARY config hung (--full, N > 1: asymmetric failure inside a
collective) -- rank 0's watchdog ended the process, the peers end by ITR_DIST_TIMEOUT_S.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "pairs/sec scored (5k img x 25k cap) + Recall@1 parity, 1/2/4/8 MI355X"
DEFAULT_WORKLOAD = "scan_t2i_coco5k"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16 / 16x16x32)
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_* peak = fp32 vector peak

WORKLOADS = {
    # name: (n_img, vocab, model)
    "scan_t2i_coco5k": dict(n_img=5000, vocab=11353, cross_attn="t2i", agg_func="LogSumExp", lambda_lse=6.0,
                            lambda_softmax=9.0, raw_feature_norm="clipped_l2norm"),
    "scan_t2i_f30k1k": dict(n_img=1000, vocab=8481, cross_attn="t2i", agg_func="LogSumExp", lambda_lse=6.0,
                            lambda_softmax=9.0, raw_feature_norm="clipped_l2norm"),
    "scan_i2t_coco5k": dict(n_img=5000, vocab=11353, cross_attn="i2t", agg_func="LogSumExp", lambda_lse=20.0,
                            lambda_softmax=4.0, raw_feature_norm="clipped_l2norm"),
    # reported SEPARATELY (STUDY_SPLIT_PRECISION.md): the same workloads with the region x word dot products on the bf16 matrix
    # core from split operands (hi.hi + hi.lo + lo.hi, fp32 accumulation); never the default, never the headline value
    "scan_t2i_coco5k_bf16x3": dict(n_img=5000, vocab=11353, cross_attn="t2i", agg_func="LogSumExp", lambda_lse=6.0,
                                   lambda_softmax=9.0, raw_feature_norm="clipped_l2norm", scan_precision="bf16x3"),
    "scan_i2t_coco5k_bf16x3": dict(n_img=5000, vocab=11353, cross_attn="i2t", agg_func="LogSumExp", lambda_lse=20.0,
                                   lambda_softmax=4.0, raw_feature_norm="clipped_l2norm", scan_precision="bf16x3"),
    "scan_t2i_coco5k_fp16x3": dict(n_img=5000, vocab=11353, cross_attn="t2i", agg_func="LogSumExp", lambda_lse=6.0,
                                   lambda_softmax=9.0, raw_feature_norm="clipped_l2norm", scan_precision="fp16x3"),
    "scan_i2t_coco5k_fp16x3": dict(n_img=5000, vocab=11353, cross_attn="i2t", agg_func="LogSumExp", lambda_lse=20.0,
                                   lambda_softmax=4.0, raw_feature_norm="clipped_l2norm", scan_precision="fp16x3"),
    # BASELINE.json configs[4]: SGRAF (EncoderSimilarity), sim_dim 256, l2-normalised bi-GRU words
    "sgraf_saf_coco5k": dict(n_img=5000, vocab=11353, sgraf="SAF"),
    "sgraf_sgr_coco5k": dict(n_img=5000, vocab=11353, sgraf="SGR"),
    "sgraf_saf_f30k1k": dict(n_img=1000, vocab=8481, sgraf="SAF"),
    "sgraf_sgr_f30k1k": dict(n_img=1000, vocab=8481, sgraf="SGR"),
    # BASELINE.json configs[1]: VSE++ f30k 1k x 5k cosine; configs[3]: SAEM / CAMERA with the BERT-base text tower
    "vsepp_f30k1k": dict(n_img=1000, vocab=8481, pooled="VSE++"),
    "vsrn_coco5k": dict(n_img=5000, vocab=11353, pooled="VSRN"),
    "vsrn_f30k1k": dict(n_img=1000, vocab=8481, pooled="VSRN"),
    "saem_coco5k": dict(n_img=5000, pooled="SAEM"),
    "camera_coco5k": dict(n_img=5000, pooled="CAMERA"),
    "camera_f30k1k": dict(n_img=1000, pooled="CAMERA"),
}


# Short runs of the other BASELINE.json configs carried by the default workload's line: (workload, timed steps, warm-up steps).
# config [1] VSE++ f30k 1k x 5k; [2] is the line itself (+ its f30k fold); [3] SAEM and CAMERA on BERT-base at coco size;
# [4] SGRAF SAF and SGR at the full 5k x 25k (the 8-GPU config) and on the 1k x 5k fold.
OTHER_CONFIGS = [("vsepp_f30k1k", 20, 5), ("scan_t2i_f30k1k", 3, 1), ("scan_i2t_coco5k", 1, 1), ("saem_coco5k", 1, 1), ("camera_coco5k", 1, 1),
                 ("sgraf_saf_f30k1k", 2, 1), ("sgraf_sgr_f30k1k", 2, 1), ("sgraf_saf_coco5k", 1, 1), ("sgraf_sgr_coco5k", 1, 1)]
BASELINE_CONFIG_OF = {"vsepp_f30k1k": 1, "scan_t2i_f30k1k": 2, "scan_i2t_coco5k": 2, "saem_coco5k": 3, "camera_coco5k": 3,
                      "sgraf_saf_f30k1k": 4, "sgraf_sgr_f30k1k": 4, "sgraf_saf_coco5k": 4, "sgraf_sgr_coco5k": 4}


def make_sgraf_weights(module_name, D=1024, S=256, sgr_step=3, seed=0):
    """EncoderSimilarity with the reference's initialisation (Xavier linears) and non-trivial BatchNorm running
    statistics (mean N(0, 0.1), var U(0.5, 1.5))."""
    from itr_amd.modalmodule import Fusionmodule
    torch.manual_seed(seed + 7)
    enc = Fusionmodule.EncoderSimilarity(D, S, module_name, sgr_step)
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return {k: v.detach().clone() for k, v in enc.state_dict().items() if "num_batches_tracked" not in k}


def make_weights(vocab, F_=2048, D=1024, E=300, seed=0):
    torch.manual_seed(seed)
    r = float(np.sqrt(6.0) / np.sqrt(F_ + D))
    wi = {"fc.weight": torch.empty(D, F_).uniform_(-r, r), "fc.bias": torch.zeros(D)}   # ImgEncoder.py:126-131
    rnn = torch.nn.GRU(E, D, 1, batch_first=True, bidirectional=True)
    wt = {"embed.weight": torch.empty(vocab, E).uniform_(-0.1, 0.1)}                      # TextEncoder.py:35-36
    wt.update({"rnn." + k: v.detach().clone() for k, v in rnn.state_dict().items()})
    return wi, wt


def make_captions(n_cap, vocab, seed=0):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(6, 21, size=n_cap)                      # randint(6, 21)
    tokens = [rng.randint(4, vocab, size=int(l)) for l in lengths]
    return lengths, tokens


def shard_captions(lengths, tokens, c0, c1, dev):
    """This rank's caption slice as the loader would hand it over: sorted by length (descending, like
    collate_fn, data_loader.py:146), packed."""
    loc_len = lengths[c0:c1]
    order = np.argsort(-loc_len, kind="stable")
    lens_sorted = loc_len[order]
    packed = np.concatenate([tokens[c0 + int(i)] for i in order]) if len(order) else np.zeros(0, np.int64)
    tok_off = np.concatenate([[0], np.cumsum(lens_sorted)[:-1]]) if len(order) else np.zeros(0, np.int64)
    return (torch.from_numpy(packed.astype(np.int64)).to(dev), torch.from_numpy(tok_off.astype(np.int64)).to(dev),
            [int(x) for x in lens_sorted], order)


RANK_NAMES = ("i2t_rank", "i2t_top1", "t2i_rank", "t2i_top1")
DUMP_SCORE_ROWS = 256
DUMP_SCORE_BYTES = 48 << 20


def dump_outputs(d, S, ranks, row0):
    """--dump-outputs: what the last timed step handed its caller.  The four rank vectors whole (float64: exact for these
    integers); of the score matrix (this rank's row block, ~0.5 GB at 5k x 25k) the full rows of a fixed, seeded sample of rows,
    with their global row indices.  At most DUMP_SCORE_BYTES + the rank vectors on disk."""
    os.makedirs(d, exist_ok=True)
    for name, r in zip(RANK_NAMES, ranks):
        np.save(os.path.join(d, name + ".npy"), np.asarray(r).astype(np.float64))
    if S is None:          # --stream-scores: the timed step kept no matrix
        return
    n_rows, n_cols = S.shape
    k = min(n_rows, DUMP_SCORE_ROWS, max(1, DUMP_SCORE_BYTES // (4 * max(1, n_cols))))
    rows = np.sort(np.random.RandomState(0).choice(n_rows, size=k, replace=False))
    sample = S.index_select(0, torch.from_numpy(rows).to(S.device)).float().cpu().numpy()
    np.save(os.path.join(d, "score_rows.npy"), sample)
    np.save(os.path.join(d, "score_row_index.npy"), (rows + row0).astype(np.float64))


def host_info():
    """What the CPU leg ran on, so that two boxes' cpu_baseline figures can be compared: logical CPUs, the CPUs this process may
    run on, physical cores (distinct (physical id, core id) pairs of /proc/cpuinfo), torch's intra-op threads and the load the
    host already carried when the leg started."""
    phys = None
    try:
        cores, pid, cid = set(), None, None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                pid = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                cid = ln.split(":")[1].strip()
            elif not ln.strip():
                if pid is not None and cid is not None:
                    cores.add((pid, cid))
                pid = cid = None
        phys = len(cores) or None
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = None
    try:
        load1 = round(os.getloadavg()[0], 2)
    except OSError:
        load1 = None
    return dict(logical_cpus=os.cpu_count(), affinity_cpus=aff, physical_cores=phys, torch_threads=torch.get_num_threads(),
                loadavg_1min_before=load1)


CPU_THREADS = None      # --cpu-threads: restrict the thread counts of the CPU leg (the 1k x 5k fold record: minutes per pass)


def time_cpu_leg(leg, repeats):
    """Run the CPU leg up to `repeats` times at torch's default thread count AND at 64 / 32 / 16 threads where the host has more (the
    160 x 800 sample does not feed 128 threads: an oversubscribed pass is 6x slower than a 32-thread one and moved the figure by 4x
    between boxes).  The MINIMUM over all passes is reported with the thread count it was reached on and the spread
    of the passes at that count.  -> (result of the last pass, stats)."""
    host = host_info()
    n_default = torch.get_num_threads()
    counts = CPU_THREADS or ([n_default] + [n for n in (64, 32, 16) if n < n_default])
    by_threads, res = {}, None
    try:
        for nt in counts:
            torch.set_num_threads(nt)
            for rep in range(max(1, repeats)):
                t0 = time.perf_counter()
                with torch.no_grad():
                    res = leg()
                by_threads.setdefault(nt, []).append(time.perf_counter() - t0)
                # a thread count that is already 1.5x behind the best pass so far is not repeated (128 threads on the 160 x 800 sample:
                # 9.0 s against 1.4 s on 32 -- r05 first run); every count is timed at least once
                if by_threads[nt][-1] > 1.5 * min(min(v) for v in by_threads.values()):
                    break
    finally:
        torch.set_num_threads(n_default)
    best_nt = min(by_threads, key=lambda k: min(by_threads[k]))
    secs = by_threads[best_nt]
    return res, dict(host, threads_used=best_nt, seconds_min=min(secs), repeats=len(secs), spread=round(max(secs) / min(secs) - 1.0, 3),
                     seconds_by_threads={str(k): [round(x, 3) for x in v] for k, v in by_threads.items()})


RECALL_TOL = 0.1      # BASELINE.json north_star: Recall@1/5/10 within +-0.1


def recall_parity(S_gpu_block, S_cpu):
    """"Recall@1 parity" of the metric, as numbers.  CPU side = the reference's own ranker restated literally (argsort of every row
    / column of the matrix the CPU path scored: /root/reference/itr/metricmodule/evaluation.py:156-222 -> oracle i2t_argsort /
    t2i_argsort); GPU side = the HIP count ranker on the matrix the HIP path scored for the SAME sample block.  Also the ranker
    alone: the HIP ranker on the CPU's matrix must reproduce the argsort rank vectors exactly (ties aside: SURVEY Q8)."""
    import itr_oracle as O
    from itr_amd import ops
    (ci, (ci_rank, _)), (ct, (ct_rank, _)) = O.i2t_argsort(S_cpu.numpy(), True), O.t2i_argsort(S_cpu.numpy(), True)
    g = ops.rank_counts(S_gpu_block.contiguous())
    gi_rank, gt_rank = g[0].cpu().numpy().astype(np.int64), g[2].cpu().numpy().astype(np.int64)
    gi, gt = ops.recall_from_ranks(gi_rank), ops.recall_from_ranks(gt_rank)
    # the ranker ALONE, on the CPU's matrix.  Where a ground-truth score occurs twice on its row / column the reference's own answer
    # is whatever numpy's unstable argsort does with the tie; the count ranker's rule is fixed (the higher index wins),
    # so the two are compared on the tie-free queries and the tied ones are counted
    h = ops.rank_counts(S_cpu.to(S_gpu_block.device).contiguous())
    Sn = S_cpu.numpy()
    ni_, nc_ = Sn.shape
    free_i = np.array([all((Sn[i] == Sn[i, c]).sum() == 1 for c in range(5 * i, min(5 * i + 5, nc_))) for i in range(ni_)])
    free_t = np.array([(Sn[:, c] == Sn[c // 5, c]).sum() == 1 for c in range(nc_)])
    hi_, ht_ = h[0].cpu().numpy().astype(np.int64), h[2].cpu().numpy().astype(np.int64)
    same_in = bool((hi_[free_i] == ci_rank.astype(np.int64)[free_i]).all() and (ht_[free_t] == ct_rank.astype(np.int64)[free_t]).all())
    n_tied = int((~free_i).sum() + (~free_t).sum())
    n_in_diff = int((hi_ != ci_rank.astype(np.int64)).sum() + (ht_ != ct_rank.astype(np.int64)).sum())
    n_diff = int((gi_rank != ci_rank.astype(np.int64)).sum() + (gt_rank != ct_rank.astype(np.int64)).sum())
    d = max(abs(a - b) for a, b in zip(tuple(gi[:3]) + tuple(gt[:3]), tuple(ci[:3]) + tuple(ct[:3])))
    return {"sample": "%d images x %d captions (the cpu_baseline sample block)" % tuple(S_cpu.shape),
            "gpu": {"i2t_r1": gi[0], "i2t_r5": gi[1], "i2t_r10": gi[2], "t2i_r1": gt[0], "t2i_r5": gt[1], "t2i_r10": gt[2]},
            "cpu": {"i2t_r1": ci[0], "i2t_r5": ci[1], "i2t_r10": ci[2], "t2i_r1": ct[0], "t2i_r5": ct[1], "t2i_r10": ct[2]},
            "max_abs_recall_diff": float(d), "tolerance": RECALL_TOL, "ok": bool(d <= RECALL_TOL),
            "rank_vectors_equal": n_diff == 0, "rank_entries_differing": n_diff, "rank_entries": int(len(gi_rank) + len(gt_rank)),
            "hip_ranker_on_cpu_scores_equals_argsort": same_in, "queries_with_tied_gt_score": n_tied,
            "hip_ranker_on_cpu_scores_entries_differing": n_in_diff,
            "note": "cpu = reference ranker (argsort) on the CPU path's scores; gpu = HIP count ranker on the HIP path's scores, same block; "
                    "run exits 4 if max_abs_recall_diff > tolerance"}


def cpu_baseline(wl, wi, wt, feats_cpu, lengths, tokens, n_img_s, repeats=3):
    """The CPU oracle (a port of the reference's algorithm, oracle/itr_oracle.py) timed on the host cores on
    a bounded sample of the same workload: the first n_img_s images and their 5*n_img_s captions.  encode + score + rank (the
    reference's argsort ranker), `repeats` passes, minimum reported."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import itr_oracle as O
    n_cap_s = 5 * n_img_s
    lens = lengths[:n_cap_s]
    order = np.argsort(-lens, kind="stable")
    L = int(lens.max())
    ids = torch.zeros(n_cap_s, L, dtype=torch.long)
    for r, i in enumerate(order):
        ids[r, :lens[i]] = torch.from_numpy(tokens[int(i)])
    lens_sorted = [int(lens[i]) for i in order]

    def leg():
        img = O.encoder_image_precomp(feats_cpu[:n_img_s], wi["fc.weight"], wi["fc.bias"])
        cap_sorted, _ = O.encoder_text(ids, lens_sorted, wt, True, True, False, None)
        cap = torch.zeros_like(cap_sorted)
        cap[torch.as_tensor(order)] = cap_sorted
        if "sgraf" in wl:
            S = O.sgraf_similarity(wl["_sim_weights"], img, O.l2norm(cap, -1), [int(x) for x in lens], wl["sgraf"], 3)
        else:
            S = O.xattn_score(img, cap, [int(x) for x in lens], wl["cross_attn"], wl["raw_feature_norm"],
                              wl["agg_func"], wl["lambda_lse"], wl["lambda_softmax"])
        O.i2t_argsort(S.numpy())
        O.t2i_argsort(S.numpy())
        return S
    S, st = time_cpu_leg(leg, repeats)
    return cpu_baseline_record(n_img_s, n_cap_s, st), S


def cpu_baseline_record(ns, ncs, st):
    # `cores` = the threads the reported pass actually used (torch's intra-op pool); the host's logical / physical counts are in `host`
    return dict(value=ns * ncs / st["seconds_min"], unit="pairs/s", cores=st["threads_used"], physical_cores=st["physical_cores"], kind="port",
                sample="first %d images x %d captions of the same synthetic workload: encode+score+rank (argsort), min of %d passes = %.2f s"
                       % (ns, ncs, st["repeats"], st["seconds_min"]),
                value_spread=st["spread"], host=st)


def scan_sustained_clock(model, feats_local, toks, tok_off, lens_sorted, order, cfg, dev):
    """Shader clock the chip sustains UNDER the SCAN kernel (MI355X is power-managed: the fp32-MFMA loop runs below the 2 400 MHz
    the peak is quoted at).  One extra, untimed launch through the library's explicit diagnostic entry point
    (itr_debug_scan_clock_probe -> ops.scan_clock_probe; no environment switch): every workgroup adds its s_memtime (shader
    cycles) and s_memrealtime (100 MHz) deltas into eight counters at the head of a scratch buffer; clock = cycles / realtime.
    (The stamps themselves cost the kernel a few percent: the launch is not the timed one.)"""
    from itr_amd import ops
    img = model.encode_images(feats_local)
    words_sorted = model.encode_captions(toks, tok_off, lens_sorted)
    lens = np.zeros(len(lens_sorted), np.int64)
    off = np.zeros(len(lens_sorted), np.int64)
    ls = np.asarray(lens_sorted, np.int64)
    lens[np.asarray(order)] = ls
    off[np.asarray(order)] = np.cumsum(ls) - ls
    plan = ops.ScanPlan(off, lens, words_sorted.shape[0], dev)
    return ops.scan_clock_probe(img, words_sorted, plan, cross_attn=cfg.get("cross_attn", "t2i"),
                                raw_feature_norm=cfg.get("raw_feature_norm", "clipped_l2norm"), agg_func=cfg.get("agg_func", "LogSumExp"),
                                lambda_lse=cfg.get("lambda_lse", 6.0), lambda_softmax=cfg.get("lambda_softmax", 9.0))


def cpu_fold_record(workload):
    """The CPU port timed ONCE on the full 1 000 x 5 000 fold of the same workload family (profiles/rNN/cpu_fold/, minutes of host
    time: too long for a default run).  Quoted next to the bounded sample the run itself times, so the speed-up is not an
    extrapolation from 160 x 800 alone.  Replayed from the committed record, labelled as such."""
    import glob
    fam = workload.replace("_coco5k", "").replace("_f30k1k", "")
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "cpu_fold", "bench_%s_f30k1k_cpu_full_fold.json" % fam)))
    if not hits:
        return None
    try:
        b = json.load(open(hits[-1]))["cpu_baseline"]
    except Exception:
        return None
    return {"fold_value": b["value"], "fold_cores": b["cores"], "fold_sample": b["sample"],
            "fold_source": "replayed: %s (not timed in this run)" % os.path.relpath(hits[-1], ROOT)}


def cpu_baseline_replayed(workload):
    """N > 1: the CPU leg is timed on rank 0 at N = 1 only (it takes the host cores of every rank's towers otherwise).  So that the
    N > 1 line parses like the N = 1 line it carries the newest COMMITTED N = 1 record of the same workload, labelled as replayed."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "bench_n1*.json")), reverse=True):
        try:
            lines = [json.loads(ln) for ln in open(f) if ln.startswith('{"metric"')]
        except Exception:
            continue
        for d in lines:
            cb = d.get("cpu_baseline")
            if d.get("config", {}).get("workload") == workload and cb and d.get("n_gpus") == 1:
                keep = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample") if k in cb}
                keep["source"] = "replayed: %s (the N = 1 run's own CPU leg; not timed in this run)" % os.path.relpath(f, ROOT)
                return keep
    return None


def pmc_traffic(workload, world):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (profiles/rNN/scan_pmc.json;
    FETCH_SIZE x2 + WRITE_SIZE, MI355X_MICROARCH.md).  bench.py cannot collect PMC counters itself (they need their own
    rocprofv3 --pmc runs), so this number is REPLAYED from the newest committed profile of the same workload, and the
    line says so: `traffic_source` = "replayed: <file> @ <commit the profile was taken at>".  null when none matches."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "**", "scan_pmc.json"), recursive=True)):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload") == workload and d.get("n_gpus") == world:
            best = (d, os.path.relpath(f, ROOT))
    if not best:
        return None, None
    return best[0]["hbm_bytes_per_launch"], "replayed: %s @ %s (not measured in this run)" % (best[1], best[0].get("commit", "unknown commit"))


# ------------------------------------------------------------------------------------------ pooled models
BERT_BASE = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 max_position_embeddings=512, type_vocab_size=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 hidden_act="gelu", initializer_range=0.02)


# the seeded BERT-base files bert_files() writes once and reuses: per user, so that a copy another account left is never in the way
BERT_DIR = os.path.join(tempfile.gettempdir(), "itr_bench_bert_%d" % os.getuid())


def bert_files(tmp):
    """bert_config.json + a seeded random pytorch_model.bin + SAEM's trans_cfg.json (pretrained weights are external
    to the reference and there is no network: SURVEY 8c)."""
    from itr_amd.modalmodule import bert
    os.makedirs(tmp, exist_ok=True)
    cfg_file, ckpt, trans = (os.path.join(tmp, n) for n in ("bert_config.json", "pytorch_model.bin", "trans_cfg.json"))
    for path, obj in ((cfg_file, BERT_BASE), (trans, dict(BERT_BASE, hidden_size=256, num_attention_heads=4, intermediate_size=1024))):
        tmp_json = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp_json, "w") as f:
            json.dump(obj, f)
        os.replace(tmp_json, path)
    if not os.path.exists(ckpt):
        # several ranks may arrive here together: everyone writes its own temporary file and renames it into place (atomic; the
        # contents are identical: seeded), nobody ever reads a half-written checkpoint
        torch.manual_seed(1)
        m = bert.BertModel(bert.BertConfig.from_dict(BERT_BASE))
        for p_ in m.parameters():
            p_.data.normal_(0, 0.02)
        tmp_ckpt = "%s.%d.tmp" % (ckpt, os.getpid())
        torch.save(m.state_dict(), tmp_ckpt)
        os.replace(tmp_ckpt, ckpt)
    return cfg_file, ckpt, trans


def pooled_inputs(n_img, n_cap, kind, dev, seed=0):
    """SURVEY 8d synthetic inputs: region features, boxes x1,y1~U(0,400), w,h~U(20,200), wh = (640, 480); BERT ids
    randint(1000, 30522) with [CLS]=101 first, mask = first `len` ones of 32, lengths randint(6, 21)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    from itr_amd import ops
    feats = ops.l2norm(torch.randn(n_img, 36, 2048, device=dev, generator=g))
    xy = torch.rand(n_img, 36, 2, device=dev, generator=g) * 400
    wh = torch.rand(n_img, 36, 2, device=dev, generator=g) * 180 + 20
    boxes = torch.cat([xy, xy + wh], -1)
    imgs_wh = torch.tensor([[640., 480.]], device=dev).repeat(n_img, 1)
    lens = rng.randint(6, 21, size=n_cap)
    ids = rng.randint(1000, 30522, size=(n_cap, 32))
    ids[:, 0] = 101
    mask = (np.arange(32)[None, :] < lens[:, None]).astype(np.int64)
    ids = ids * mask
    return feats, boxes, imgs_wh, torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), torch.zeros(n_cap, 32, dtype=torch.long, device=dev), lens


def main_pooled(args, wl, world, rank, dev, use_dist):
    from itr_amd import config as C, evalpipe, ops
    from itr_amd.modalmodule import get_model
    kind = wl["pooled"]
    n_img, n_cap = wl["n_img"], 5 * wl["n_img"]
    comm = evalpipe.Comm()
    i0, i1 = evalpipe.block_range(n_img, comm.world, comm.rank, 4)
    cap_ranges = [evalpipe.block_range(n_cap, comm.cap_world, q) for q in range(comm.cap_world)]
    c0, c1 = cap_ranges[comm.cap_rank]
    torch.manual_seed(0)
    gru_text = kind in ("VSE++", "VSRN")
    if kind == "VSE++":
        cfg = C.build_config(['with', 'VSE_PP', 'data_name=f30k_precomp', 'bi_gru=True', 'max_violation=True'])
        cfg.update(img_dim=2048, vocab_size=wl["vocab"])
    elif kind == "VSRN":
        cfg = C.build_config(['with', 'VSRN', 'data_name=%s_precomp' % ("coco" if wl["n_img"] == 5000 else "f30k")])
        cfg.update(vocab_size=wl["vocab"])
    else:
        cfg_file, ckpt, trans = bert_files(BERT_DIR)
        cfg = C.build_config(['with', kind, 'data_name=coco_precomp'])
        cfg.update(bert_config_file=cfg_file, init_checkpoint=ckpt, trans_cfg=trans, vocab_size=30522)
    torch.manual_seed(0)       # (bert_files() draws random numbers only when it has to create the checkpoint: seed AFTER it)
    model = get_model(cfg)
    if kind == "VSRN":
        # Rs_GCN initialises its BatchNorm to gamma = beta = 0 (an identity layer): trained-like statistics instead
        gbn = torch.Generator().manual_seed(1)
        for mod in model.img_enc.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=gbn) * 0.6 + 0.2)
                mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=gbn) * 0.05)
                mod.running_mean.data.copy_(torch.randn(mod.running_mean.shape, generator=gbn) * 0.1)
                mod.running_var.data.copy_(torch.rand(mod.running_var.shape, generator=gbn) + 0.5)
    model.val_start()
    if gru_text:
        # packed captions of this rank, sorted by length once (like the SCAN workload): ONE GRU call per step
        lengths, tokens = make_captions(n_cap, wl["vocab"])
        cap_ranges = evalpipe.caption_ranges(n_cap, comm.cap_world, lengths)      # near-equal token sums per owner
        c0, c1 = cap_ranges[comm.cap_rank]
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        feats = ops.l2norm(torch.randn(n_img, 36, 2048, device=dev, generator=g))
        toks, tok_off, lens_sorted, order = shard_captions(lengths, tokens, c0, c1, dev)
        order_dev = torch.from_numpy(np.ascontiguousarray(order)).to(dev)
        towers = evalpipe.GruModelEval({k: v.detach() for k, v in model.img_enc.state_dict().items()},
                                       {k: v.detach() for k, v in model.txt_enc.state_dict().items()},
                                       dict(bi_gru=kind == "VSE++", no_txtnorm=False, no_imgnorm=False), comm)
        peers = None
        if comm.virtual:
            peers = {q: shard_captions(lengths, tokens, lo, hi, dev) for q, (lo, hi) in enumerate(cap_ranges) if q != comm.cap_rank and hi > lo}
    else:
        feats, boxes, imgs_wh, ids, mask, types, lengths = pooled_inputs(n_img, n_cap, kind, dev)
    cap_counts = [hi - lo for lo, hi in cap_ranges]
    # captions per text-tower pass: 4096 x 32 tokens = 1024 row tiles, i.e. >= 4 tiles per resident workgroup for every 768-wide
    # layer, which is what the streaming GEMM asks for (ITR_POOLED_BATCH overrides)
    pe = evalpipe.PooledModelEval(model, comm, batch=int(os.environ.get('ITR_POOLED_BATCH', '4096')))
    timers = dict(scan_start=torch.cuda.Event(enable_timing=True), scan_end=torch.cuda.Event(enable_timing=True))

    def step(tm=None, keep=True):
        # --stream-scores (opt-in, one process): the timed steps keep no matrix -- one larger than 64 MB is streamed through the ranker in
        # cache-sized row blocks (evalpipe.score_rank_streamed; measured slower than writing it once: profiles/r06/NOTES.md); S is None then
        if gru_text:
            if kind == "VSRN":
                with torch.no_grad():
                    img = torch.cat([model.img_enc(feats[b0:min(b0 + 1024, i1)])[0] for b0 in range(i0, i1, 1024)], 0)
            else:
                img = ops.proj_l2norm(ops.mean_mid(feats[i0:i1]), towers.wi['fc.weight'], towers.wi['fc.bias'])
            cap_sorted = towers.encode_captions(toks, tok_off, lens_sorted, gather_last=True)
            send = torch.empty(max(cap_counts), cap_sorted.shape[1], device=dev, dtype=torch.float32)
            send[order_dev] = cap_sorted                     # back to the dataset order, in the head of the exchange's send buffer
            send[cap_sorted.shape[0]:].zero_()               # (the tail -- at most a few rows -- travels with the exchange: defined values)
            if peers is not None:
                comm.peer_blocks = {}
                for q, p in peers.items():
                    e = towers.encode_captions(p[0], p[1], p[2], gather_last=True)
                    blk = torch.empty_like(e)
                    blk[torch.from_numpy(np.ascontiguousarray(p[3])).to(dev)] = e
                    comm.peer_blocks[q] = blk
            if not keep and not comm.on and not comm.virtual and 4 * n_img * n_cap > (64 << 20):
                return None, evalpipe.score_rank_streamed(img, send[:n_cap], ops.cosine_scores, 5, timers=tm)
            S = evalpipe.exchange_score(comm, img, send, cap_ranges, n_cap, ops.cosine_scores, tm)
            return S, evalpipe.finalize_ranks(comm, S, i0, n_img, 5)
        if comm.virtual:
            comm.peer_blocks = {q: pe.encode_captions(ids[lo:hi], mask[lo:hi], types[lo:hi], [int(x) for x in lengths[lo:hi]])
                                for q, (lo, hi) in enumerate(cap_ranges) if q != comm.cap_rank and hi > lo}
        return pe.eval(feats[i0:i1], boxes[i0:i1], imgs_wh[i0:i1], ids[c0:c1], mask[c0:c1], types[c0:c1], [int(x) for x in lengths[c0:c1]],
                       n_img, n_cap, timers=tm, cap_ranges=cap_ranges, stream_scores=not keep)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(keep=not args.stream_scores)
    barrier()
    score_ms = []
    t0 = time.perf_counter()
    S = ranks = None
    for _ in range(args.steps):
        S = ranks = None          # as a validation loop would: the previous score matrix is released before the next evaluation
        S, ranks = step(timers, keep=not args.stream_scores)   # (holding it makes the caching allocator grow by 0.5 GB inside the timed region, once)
        score_ms.append(timers["scan_start"].elapsed_time(timers["scan_end"]))
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device="cpu" if os.environ.get("ITR_DIST_BACKEND") == "gloo" else dev, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    streamed = S is None
    streamed_equal = None
    if streamed and world == 1 and args.full:
        # outside the timed region: the same evaluation with the matrix kept -- the parity legs below read it, and its ranks must be
        # the streamed ones, entry for entry
        S, ranks_kept = step(None, keep=True)
        torch.cuda.synchronize()
        streamed_equal = all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(ranks, ranks_kept))
    if rank != 0:
        return None
    if getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, None if streamed else S, ranks, i0)
    from itr_amd import ops as _ops
    ms_per_step = 1e3 * dt / args.steps
    # SURVEY 8d algorithmic flop of the step on this rank
    exe_flop = None
    if kind == "VSE++":
        n_tok = float(lengths[c0:c1].sum())
        flop = (i1 - i0) * 2 * 2048 * 1024 + n_tok * 16.27e6 + float(i1 - i0) * n_cap * 2 * 1024
        # executed (round 5): VSE++ reads the bi-GRU at position len - 1 only (TextEncoder.py:57-60), where the backward direction has
        # seen ONE token: the forward recurrence (half of SURVEY 8d's 16.27 MFLOP per token) + one backward input projection per caption
        # -- and of that: the input projection once per vocabulary WORD when the shard has >= 2 tokens per word (csrc/towers.hip), and no
        # recurrence GEMM for a caption's first step (h = 0: the product is b_hh)
        n_loc = float(c1 - c0)
        in_rows = float(wl["vocab"]) if 2 * wl["vocab"] <= n_tok else n_tok
        exe_flop = ((i1 - i0) * 2 * 2048 * 1024 + in_rows * 2.0 * 3 * 1024 * 300 + (n_tok - n_loc) * 2.0 * 3 * 1024 * 1024
                    + n_loc * 2.0 * 3 * 1024 * 300 + float(i1 - i0) * n_cap * 2 * 1024)
        model_name, dims = "VSE++ bi-GRU (mean-pooled regions)", 1024
    elif kind == "VSRN":
        n_tok = float(lengths[c0:c1].sum())
        D = 2048      # per image: fc + 4 x (theta, phi, g, W convolutions + the two N x N x D relation products) + GRU over 36 regions
        flop_img = 36 * 2 * 2048 * D + 4 * (4 * 36 * 2 * D * D + 2 * 2 * 36 * 36 * D) + 36 * 2 * 3 * D * (D + D)
        flop = (i1 - i0) * float(flop_img) + n_tok * 2 * 3 * D * (300 + D) + float(i1 - i0) * n_cap * 2 * D
        model_name, dims = "VSRN (4 x Rs_GCN + region GRU image tower, uni-GRU text tower)", D
    elif kind == "SAEM":
        flop = (c1 - c0) * 5.47e9 + float(i1 - i0) * n_cap * 512
        model_name, dims = "SAEM (BERT-base + cnn head, transformer image tower)", 256
    else:
        flop = (c1 - c0) * (5.47e9 + 1.45e9) + (i1 - i0) * 1.55e9 + float(i1 - i0) * n_cap * 2 * 12 * 2048
        model_name, dims = "CAMERA (BERT-base + AGSA, 12 views x 2048)", 2048
    i2t, t2i = _ops.recall_from_ranks(ranks[0]), _ops.recall_from_ranks(ranks[2])
    out = {"metric": METRIC, "value": float(n_img) * n_cap / (dt / args.steps),
           "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": args.workload, "scorer": model_name, "n_img": n_img, "n_cap": n_cap, "regions": 36, "feat_dim": 2048,
                      "embed": dims, "parallelism": "row-shard x%d + 1 all-gather of caption embeddings" % world,
                      "step": "encode(image tower + text tower) + score + rank(i2t,t2i)"},
           "recall": {"i2t_r1": i2t[0], "i2t_r5": i2t[1], "i2t_r10": i2t[2], "t2i_r1": t2i[0], "t2i_r5": t2i[1], "t2i_r10": t2i[2]},
           "rank_checksum": [int((np.asarray(r, np.int64) * (np.arange(len(r)) % 9973 + 1)).sum()) for r in ranks],
           "roofline": {"kernel": "gemm_nt_kernel (every dense layer of the towers + the score GEMM)", "bound": "mfma",
                        "achieved": (exe_flop or flop) / (ms_per_step * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": (exe_flop or flop) / (ms_per_step * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, "traffic": None,
                        "score_kernel_ms": float(np.mean(score_ms)), "algorithmic_flop_per_step": flop,
                        "executed_flop_per_step": exe_flop or flop,
                        "algorithmic_equiv_frac": flop / (ms_per_step * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                        "note": "time = the whole step (the towers are hundreds of GEMM launches); achieved / frac = the flop EXECUTED "
                                "(= SURVEY 8d's per-unit figures, except VSE++: its last-state output needs one step of the backward GRU, "
                                "not its recurrence, the input projection runs once per vocabulary word and a caption's first step has no "
                                "recurrence product); algorithmic_equiv_frac = SURVEY 8d's flop over the same time"}}
    if streamed and world == 1:
        out["score_matrix"] = {"materialised": False, "row_block_bytes": 64 << 20,
                               "note": "timed steps stream the similarity matrix through the ranker in row blocks (evalpipe.score_rank_streamed)"}
        if streamed_equal is not None:
            out["score_matrix"]["ranks_equal_materialised_run"] = bool(streamed_equal)
            out["score_matrix"]["note"] += "; a run that keeps the matrix (after the timed region) gave the same rank vectors"
            if not streamed_equal:
                print("bench.py: the streamed ranks differ from the ranks of the materialised matrix", file=sys.stderr)
    if comm.virtual:
        out["virtual_split"] = "%d:%d" % (comm.cap_world, comm.cap_rank)
        out["config"]["parallelism"] = "1 process, caption axis split over %d virtual owners (this one: %d): TEST HOOK, time is not a result" % (
            comm.cap_world, comm.cap_rank)
    if args.full and world == 1 and not args.no_cpu_baseline:
        # CPU oracle (kind "port") on the first ns images and their 5*ns captions: encode + score + rank, and max |diff|
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import itr_oracle as O
        ns = min(args.cpu_sample_images, 40 if not gru_text else 200)
        ncs = 5 * ns
        wi = {k: v.detach().cpu() for k, v in model.img_enc.state_dict().items() if "num_batches_tracked" not in k}
        wt = {k: v.detach().cpu() for k, v in model.txt_enc.state_dict().items() if "num_batches_tracked" not in k}
        feats_c = feats[:ns].cpu()
        if gru_text:
            lens = lengths[:ncs]
            order_s = np.argsort(-lens, kind="stable")
            ids_s = torch.zeros(ncs, int(lens.max()), dtype=torch.long)
            for r, i in enumerate(order_s):
                ids_s[r, :lens[i]] = torch.from_numpy(tokens[int(i)])
        else:
            boxes_c, wh_c, ids_c, mask_c, types_c = boxes[:ns].cpu(), imgs_wh[:ns].cpu(), ids[:ncs].cpu(), mask[:ncs].cpu(), types[:ncs].cpu()

        def leg():
            if gru_text:
                if kind == "VSRN":
                    img_o, _ = O.vsrn_image(wi, feats_c, cfg["data_name"])
                else:
                    img_o = O.encoder_image_precomp(feats_c.mean(1), wi["fc.weight"], wi["fc.bias"])
                cap_sorted, _ = O.encoder_text(ids_s, [int(lens[i]) for i in order_s], wt, kind == "VSE++", False, False, "VSE++")
                cap_o = torch.zeros_like(cap_sorted)
                cap_o[torch.as_tensor(order_s)] = cap_sorted
                S_o = O.cosine_sim(img_o, cap_o)
            elif kind == "CAMERA":
                img_o, _ = O.camera_image(wi, feats_c, boxes_c, wh_c, cfg["head"])
                cap_o = O.camera_text(wt, ids_c, mask_c, types_c, 12, 12, cfg["head"])
                S_o = O.multi_view_matching(img_o, cap_o)
            else:
                img_o = O.saem_image(wi, feats_c, 4)
                cap_o = O.saem_text(wt, cfg["txt_stru"], ids_c, mask_c, types_c, 12, 12, 4)
                S_o = O.pdist_cos(img_o, cap_o)
            O.i2t_argsort(S_o.numpy())
            O.t2i_argsort(S_o.numpy())
            return S_o
        S_o, st = time_cpu_leg(leg, args.cpu_repeats)
        out["cpu_baseline"] = dict(cpu_baseline_record(ns, ncs, st), max_abs_diff_vs_gpu=float((S[:ns, :ncs].cpu() - S_o).abs().max()),
                                   recall_parity=recall_parity(S[:ns, :ncs], S_o))
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    return out


def main_from_files(args, world, rank, dev, use_dist):
    """the real-data path must not be PCIe / disk / tokeniser bound.  One step = evalpipe.evaluate_precomp on the
    files: features memory-mapped and streamed through pinned staging in row blocks under the scoring of the previous block,
    captions tokenised in one regex pass (the dataset's token cache is dropped every step, so tokenisation is inside the timed
    region), text tower, SCAN scores, ranks.  The same process then times the resident-input step on the same data."""
    from itr_amd import config as C, evalpipe, ops
    from itr_amd.datamodule import data_loader as dl
    from itr_amd.modalmodule import get_model
    name = "coco_precomp"
    cfg = C.build_config(['with', 'SCAN', 'data_name=%s' % name, 'bi_gru=True', 'max_violation=True', 'cross_attn=t2i', 'agg_func=LogSumExp',
                          'lambda_lse=6.0', 'lambda_softmax=9.0', 'raw_feature_norm=clipped_l2norm'])
    cfg.update(data_path=os.path.join(args.from_files, "data"), vocab_path=os.path.join(args.from_files, "vocab"), workers=0, word_tokenize=None)
    dset = dl.PrecompDataset(os.path.join(cfg['data_path'], name), 'test', cfg)
    cfg['vocab_size'] = len(dset.vocab)
    torch.manual_seed(0)
    model = get_model(cfg)
    comm = evalpipe.Comm()
    n_cap = len(dset)
    n_img = n_cap // 5

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def step_files():
        dset.invalidate_token_cache()             # tokenise again: part of the path being timed
        return evalpipe.evaluate_precomp(model, dset, comm)

    for _ in range(max(1, args.warmup)):          # (the first pass also pulls the feature file into the page cache)
        ranks_f = step_files()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ranks_f = step_files()
    barrier()
    dt_files = (time.perf_counter() - t0) / args.steps
    # ---- the same data resident in HBM, captions tokenised and packed beforehand
    i0, i1 = evalpipe.block_range(n_img, comm.world, comm.rank, 4)
    feats = evalpipe._features_to_device(dset.images, i0, i1, dev)
    flat_all, lens_all = dset.token_ids_range(0, n_cap)
    ranges = evalpipe.caption_ranges(n_cap, comm.world, lens_all)
    c0, c1 = ranges[comm.rank]
    offs = np.concatenate([[0], np.cumsum(lens_all)])
    tokens = [flat_all[offs[j]:offs[j + 1]] for j in range(n_cap)]
    toks, tok_off, lens_sorted, order = shard_captions(np.asarray(lens_all), tokens, c0, c1, dev)
    wi = {k: v.detach() for k, v in model.img_enc.state_dict().items()}
    wt = {k: v.detach() for k, v in model.txt_enc.state_dict().items()}
    ev = evalpipe.GruModelEval(wi, wt, dict(cfg, bi_gru=True, no_txtnorm=model.txt_enc.no_txtnorm, no_imgnorm=model.img_enc.no_imgnorm), comm)

    def step_resident():
        return ev.scan_eval(feats, toks, tok_off, lens_sorted, order, n_img, n_cap, cap_ranges=ranges, all_lengths=lens_all)[1]

    ranks_r = step_resident()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ranks_r = step_resident()
    barrier()
    dt_res = (time.perf_counter() - t0) / args.steps
    t = torch.tensor([dt_files, dt_res], device=dev if os.environ.get("ITR_DIST_BACKEND") != "gloo" else "cpu", dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt_files, dt_res = float(t[0]), float(t[1])
    if rank != 0:
        return
    same = all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(ranks_f, ranks_r))
    pairs = float(n_img) * n_cap
    out = {"metric": METRIC, "value": pairs / dt_files, "unit": "pairs/s",
           "n_gpus": world, "steps": args.steps, "warmup": max(1, args.warmup), "ms_per_step": 1e3 * dt_files, "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic precomp FILES (tools/make_synth_precomp.py)",
           "config": {"workload": "scan_t2i_coco5k_from_files", "n_img": n_img, "n_cap": n_cap, "n_words": int(np.sum(lens_all)),
                      "step": "mmap .npy -> pinned -> HBM (row blocks under the scoring) + tokenise + encode + score + rank"},
           "resident": {"value": pairs / dt_res, "ms_per_step": 1e3 * dt_res, "note": "same data already in HBM, captions packed beforehand"},
           "files_over_resident_time": dt_files / dt_res, "ranks_identical_to_resident": bool(same),
           "rank_checksum": [int((np.asarray(r, np.int64) * (np.arange(len(r)) % 9973 + 1)).sum()) for r in ranks_f]}
    print(json.dumps(out), flush=True)


def progress(stage):
    """One line per rank in $ITR_BENCH_PROGRESS_DIR (set by launch_ranks): what this rank last reached.  The launching parent reads
    it when a deadline passes, so that a start-up / first-collective hang names the rank and the stage instead of being silent."""
    d = os.environ.get("ITR_BENCH_PROGRESS_DIR")
    if not d:
        return
    try:
        tmp = os.path.join(d, ".rank%s.tmp" % os.environ.get("RANK", "0"))
        with open(tmp, "w") as f:
            f.write("%s\t%.3f\t%d\n" % (stage, time.time(), os.getpid()))
        os.replace(tmp, os.path.join(d, "rank%s" % os.environ.get("RANK", "0")))
    except OSError:
        pass


def read_progress(d, n):
    rows = []
    for r in range(n):
        try:
            stage, ts, pid = open(os.path.join(d, "rank%d" % r)).read().rstrip("\n").split("\t")
            rows.append(dict(rank=r, stage=stage, age_s=round(time.time() - float(ts), 1), pid=int(pid)))
        except (OSError, ValueError):
            rows.append(dict(rank=r, stage="(never reported: the process did not reach main())", age_s=None, pid=None))
    return rows


PG_READY_STAGES = ("pg_ready", "rank_table", "fabric_check", "workload", "done")


def launch_ranks(n, argv, init_deadline_s=420.0, total_deadline_s=2400.0):
    """`python bench.py --gpus N` started as ONE command (the reference's only multi-device notion is one process driving
    nn.DataParallel, /root/reference/itr/modalmodule/Models.py:561-562 -- one command): this parent has made NO GPU call
    (no torch.cuda.*, the HIP library is not loaded) and starts N children, one rank per GPU, through torch.distributed.run
    as a CHILD process in its own process group (never exec), relays their stdout (rank 0 prints the one JSON line) and exits
    with their code.  Two parent-side deadlines (VERDICT r4 #3b): every rank must have built the process group and finished the
    probe collective within `init_deadline_s`, and the whole run must end within `total_deadline_s`; past either the parent
    prints what every rank last reported, kills the CHILD process group (SIGTERM, then SIGKILL) and exits 124."""
    import shutil
    import signal
    import socket
    import subprocess
    import tempfile
    import threading
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    pdir = tempfile.mkdtemp(prefix="itr_bench_progress_")
    env = dict(os.environ, ITR_BENCH_LAUNCHED_BY="bench.py", ITR_BENCH_PROGRESS_DIR=pdir)
    # The platform's multi-process GPU rule (this pool's environment notes): the host driver only supports dmabuf IPC, and without
    # HSA_ENABLE_IPC_MODE_LEGACY=0 RCCL / device-memory sharing across processes fails with `hipIpcGetMemHandle: invalid argument`.
    # It is already exported on the GPU boxes; setdefault keeps an operator's own value and only fills it in when it is absent.
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    n_lines = [0]

    def relay():
        for ln in p.stdout:
            n_lines[0] += ln.startswith('{"metric"')
            sys.stdout.write(ln)
            sys.stdout.flush()
    th = threading.Thread(target=relay, daemon=True)
    th.start()
    t0 = time.time()
    ready = False
    why = None
    while p.poll() is None:
        time.sleep(0.25)
        el = time.time() - t0
        if not ready:
            ready = all(r["stage"].split(":")[0] in PG_READY_STAGES for r in read_progress(pdir, n))
            if not ready and el > init_deadline_s:
                why = "not every rank finished the process-group probe collective within %.0f s" % init_deadline_s
        if why is None and el > total_deadline_s:
            why = "the run did not end within %.0f s" % total_deadline_s
        if why:
            print("bench.py: DEADLINE: %s; last report of every rank:" % why, file=sys.stderr)
            for r in read_progress(pdir, n):
                print("bench.py:   rank %(rank)d  stage=%(stage)s  age=%(age_s)s s  pid=%(pid)s" % r, file=sys.stderr)
            sys.stderr.flush()
            for sig, wait in ((signal.SIGTERM, 10.0), (signal.SIGKILL, 10.0)):
                try:
                    os.killpg(p.pid, sig)       # the child's own process group (start_new_session): never this process
                except ProcessLookupError:
                    break
                try:
                    p.wait(timeout=wait)
                    break
                except subprocess.TimeoutExpired:
                    continue
            shutil.rmtree(pdir, ignore_errors=True)
            return 124
    rc = p.wait()
    th.join(timeout=10.0)
    if rc != 0:
        print("bench.py: the ranks exited with code %d; last report of every rank:" % rc, file=sys.stderr)
        for r in read_progress(pdir, n):
            print("bench.py:   rank %(rank)d  stage=%(stage)s  age=%(age_s)s s  pid=%(pid)s" % r, file=sys.stderr)
    shutil.rmtree(pdir, ignore_errors=True)
    if rc == 0 and n_lines[0] != 1:
        print("bench.py: %d ranks exited 0 but printed %d result lines" % (n, n_lines[0]), file=sys.stderr)
        rc = 3
    return rc


def gather_floats(vals, dev, backend, use_dist):
    """[v0, v1, ...] of THIS rank -> [[...] of rank 0, [...] of rank 1, ...] through the step's own process group."""
    t = torch.tensor([float(v) for v in vals], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    if not use_dist:
        return [t.tolist()]
    rows = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(rows, t)
    return [r.cpu().tolist() for r in rows]


def fabric_check(dev, backend, world, rank, use_dist, total_bytes, n_counts=25000, reps=3):
    """--launch-check, after the rank table (VERDICT r4 #3c): the two collectives of the evaluation's exchange on their REAL
    payloads and nothing else -- one all_gather_into_tensor of the packed word embeddings (1.33 GB in total at 5k x 25k, i.e.
    1.33 GB / N sent per rank) and the sum all-reduce of the Nc int32 partial t2i counts -- verified for content and timed per
    rank, so a fabric that fails or crawls is diagnosed apart from the kernels."""
    D = 1024
    rows = max(1, int(total_bytes // world // (4 * D)))
    on_gpu = dev.type == "cuda" and backend != "gloo"
    cdev = dev if on_gpu else torch.device("cpu")
    send = torch.full((rows, D), float(rank + 1), device=cdev, dtype=torch.float32)
    recv = torch.zeros(world * rows, D, device=cdev, dtype=torch.float32)
    counts = torch.ones(n_counts, device=cdev, dtype=torch.int32)

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
    ag_ms, ar_ms = [], []
    for it in range(reps + 1):              # (the first pass builds the channels: not timed)
        recv.zero_()
        counts.fill_(1)
        sync()
        if use_dist:
            dist.barrier()
        t0 = time.perf_counter()
        if use_dist:
            dist.all_gather_into_tensor(recv, send)
        else:
            recv.copy_(send)
        sync()
        t1 = time.perf_counter()
        if use_dist:
            dist.all_reduce(counts)
        sync()
        t2 = time.perf_counter()
        if it:
            ag_ms.append(1e3 * (t1 - t0))
            ar_ms.append(1e3 * (t2 - t1))
    ok_ag = all(bool((recv[q * rows:(q + 1) * rows] == float(q + 1)).all()) for q in range(world))
    ok_ar = bool((counts == world).all())
    per = gather_floats([min(ag_ms), min(ar_ms), float(ok_ag), float(ok_ar)], dev, "nccl" if on_gpu else "gloo", use_dist)
    sent = rows * D * 4
    recv_bytes = sent * max(1, world - 1)
    return {"all_gather_into_tensor": {"bytes_sent_per_rank": sent, "bytes_received_per_rank": recv_bytes, "bytes_total": sent * world,
                                       "ms_per_rank": [round(r[0], 3) for r in per],
                                       "gb_per_s_received_per_rank": [round(recv_bytes / (r[0] * 1e-3) / 1e9, 2) for r in per],
                                       "ok": all(r[2] == 1.0 for r in per)},
            "all_reduce_counts": {"n_int32": n_counts, "ms_per_rank": [round(r[1], 3) for r in per], "ok": all(r[3] == 1.0 for r in per)},
            "note": "min of %d timed passes per rank, barrier + synchronize around each; world 1 = a local copy" % reps}


def gather_rank_table(dev, backend, world, rank, local_rank):
    """Who took part, all-gathered THROUGH the process group the collectives of the step use (nccl = RCCL): one int64 row per rank
    = (rank, local device index, PCI domain / bus / device of that device, pid).  A 1-rank run that claims N GPUs cannot
    produce N rows with N distinct PCI ids."""
    row = [rank, local_rank, -1, -1, -1, os.getpid()]
    name = "cpu"
    if dev.type == "cuda":
        pr = torch.cuda.get_device_properties(dev)
        row[2:5] = [int(getattr(pr, "pci_domain_id", -1)), int(getattr(pr, "pci_bus_id", -1)), int(getattr(pr, "pci_device_id", -1))]
        name = pr.name
    t = torch.tensor(row, dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
    if dist.is_initialized():
        rows = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(rows, t)
    else:
        rows = [t]
    return [dict(rank=int(r[0]), device_index=int(r[1]), pci_bus_id="%04x:%02x:%02x.0" % (int(r[2]) & 0xffff, int(r[3]) & 0xff, int(r[4]) & 0xff)
                 if int(r[3]) >= 0 else None, pid=int(r[5]), device_name=name) for r in (x.cpu().tolist() for x in rows)]


class LineOnce:
    """Rank 0's ONE JSON line.  Whatever happens after the primary workload has been measured (the other BASELINE configs run after
    it), the line it earned is printed exactly once: at the normal end, from the `finally` of main(), or by the watchdog."""

    def __init__(self):
        import threading
        self.lock = threading.Lock()
        self.out = None
        self.printed = False

    def emit(self, extra=None):
        with self.lock:
            if self.printed or self.out is None:
                return False
            if extra:
                self.out.update(extra)
            print(json.dumps(self.out), flush=True)
            self.printed = True
            return True


def other_config_row(name, k, w, o, wall):
    rf = o["roofline"]
    row = {"baseline_config": BASELINE_CONFIG_OF[name], "steps": k, "warmup": w, "ms_per_step": o["ms_per_step"],
           "pairs_per_s": o["value"], "n_img": o["config"]["n_img"], "n_cap": o["config"]["n_cap"], "frac": rf["frac"],
           "achieved_tflops": rf["achieved"], "kernel_ms": rf.get("kernel_ms", rf.get("score_kernel_ms")),
           "recall": o["recall"], "rank_checksum": o["rank_checksum"], "wall_s": round(wall, 2)}
    for key in ("sgraf_block", "per_rank_step_ms"):
        if key in o:
            row[key] = o[key]
    if "algorithmic_equiv_frac" in rf:
        row["algorithmic_equiv_frac"] = rf["algorithmic_equiv_frac"]
    return row


def other_config_in_child(name, k, w, timeout_s):
    """One other BASELINE config in a FRESH child process (subprocess, never exec): a GPU fault, an abort or an out-of-memory in a
    secondary config cannot take the already-measured primary line with it, and the child starts from an empty
    memory pool like any user's process would.  -> (result dict | None, error string | None)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", name, "--steps", str(k), "--warmup", str(w)]      # a plain run
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("ITR_BENCH_PROGRESS_DIR",)}
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return None, "child process exceeded %d s and was killed" % timeout_s
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    if r.returncode != 0 or len(lines) != 1:
        tail = (r.stderr or "").strip().splitlines()
        return None, "child process exit code %d: %s" % (r.returncode, tail[-1] if tail else "no message")
    return json.loads(lines[0]), None


def train_configs_in_child(timeout_s):
    """SURVEY 8 f3, measured: one model.train_emb step of every model family at the reference's training shape (batch 128, SAEM 64;
    the reference times every training batch, /root/reference/itr/utils.py:80-102), in a fresh child process after the timed region
    (tools/train_bench.py --all --json --cpu): ms per step, forward / backward / optimizer split, pairs scored per second, the flop
    model as a fraction of the fp32 MFMA peak, and the oracle's training step on the host cores beside VSE++ / SCAN."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "--all", "--json", "--cpu", "--steps", "10", "--warmup", "3", "--budget",
           str(int(timeout_s * 0.6))]
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("ITR_BENCH_PROGRESS_DIR",)}
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"error": "child process exceeded %d s and was killed" % timeout_s}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"train_configs"')]
    if r.returncode != 0 or len(lines) != 1:
        tail = (r.stderr or "").strip().splitlines()
        return {"error": "child process exit code %d: %s" % (r.returncode, tail[-1] if tail else "no message")}
    o = json.loads(lines[0])
    o["train_configs"]["wall_s"] = o["wall_s"]
    return o["train_configs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default=DEFAULT_WORKLOAD, choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run what the headline figure does not need: the CPU baseline with its Recall parity "
                         "check (exit 4), the fp16x3 variant, the sustained-clock probe, the other BASELINE.json configs, the training-step "
                         "timings and the materialised re-run of --stream-scores (the --no-* switches drop parts of it)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and its Recall parity check")
    ap.add_argument("--no-variants", action="store_true", help="--full: skip the separately reported fp16x3 variant of the SCAN workloads")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full: skip the short runs of the other BASELINE.json configs that the default workload's line carries in "
                         "`other_configs` (and the training-step timings)")
    ap.add_argument("--stream-scores", action="store_true",
                    help="pooled workloads, one process: the timed steps stream the similarity matrix through the ranker in row blocks instead "
                         "of storing it (evalpipe.score_rank_streamed); measured slower, off by default")
    ap.add_argument("--no-train-configs", action="store_true",
                    help="--full: skip the training-step timings (model.train_emb of every family, tools/train_bench.py in a child process) "
                         "that the default workload's line carries in `train_configs`")
    ap.add_argument("--cpu-sample-images", type=int, default=160, help="--full: images of the CPU leg's sample block")
    ap.add_argument("--cpu-repeats", type=int, default=3, help="--full: passes of the CPU leg (the minimum is reported, with the spread)")
    ap.add_argument("--cpu-threads", default=None, metavar="N[,N...]",
                    help="--full: thread counts of the CPU leg (default: torch's own count and 64 / 32 / 16 where the host has more)")
    ap.add_argument("--launch-check", action="store_true",
                    help="start the ranks, build the process group, all-gather the rank table, run the exchange's two collectives on their "
                         "real payload sizes (fabric check), print the line with value = null and stop (no kernel of the path runs)")
    ap.add_argument("--launch-check-bytes", type=float, default=None,
                    help="total bytes of the fabric check's all-gather (default: 1.33e9 = the packed word embeddings of 5k x 25k on GPUs, "
                         "16 MiB on a box without one)")
    ap.add_argument("--init-deadline", type=float, default=float(os.environ.get("ITR_BENCH_INIT_DEADLINE_S", "420")),
                    help="`--gpus N` as one command: seconds the ranks have to build the process group and finish the probe collective")
    ap.add_argument("--deadline", type=float, default=float(os.environ.get("ITR_BENCH_DEADLINE_S", "2400")),
                    help="`--gpus N` as one command: seconds the whole run may take before the parent kills the ranks")
    ap.add_argument("--virtual-split", default=None, metavar="K[:V]",
                    help="TEST HOOK (1 process): treat the caption axis as owned by K ranks of which this process is owner V (default K//2): "
                         "the N>1 order of work -- asynchronous all-gather in flight on the backend's stream while the own columns are scored, "
                         "wait, the other owners' columns from the gathered buffer -- runs on one GPU (with ITR_FORCE_COLLECTIVES=1 the "
                         "gather is a real 1-rank RCCL collective).  The rank vectors must equal the plain run's; the time is not a result.")
    ap.add_argument("--from-files", default=None, metavar="DIR",
                    help="time the file -> rank path on a precomp dataset directory written by tools/make_synth_precomp.py (SCAN t2i): "
                         "memory-mapped .npy -> pinned -> HBM, tokenise, encode, score, rank; reported next to the resident-input number")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (rank 0): the four rank vectors "
                         "(float64) and a fixed, seeded sample of score-matrix rows (float32), to compare two builds output for output")
    args = ap.parse_args()
    if args.dump_outputs and (args.launch_check or args.from_files):
        ap.error("--dump-outputs applies to the resident-input workloads (not --launch-check / --from-files)")
    if args.cpu_threads:
        global CPU_THREADS
        CPU_THREADS = [int(x) for x in args.cpu_threads.split(",")]

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one command, N ranks: this process has not touched the GPU and never will
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], args.init_deadline, args.deadline))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    progress("main")
    hang = os.environ.get("ITR_BENCH_TEST_HANG")      # TEST HOOK "rank:stage" (tests/test_distributed.py): that rank stops reporting there
    if world != args.gpus:
        # never a silent 1-rank run that prints a plausible line for N GPUs (or the reverse)
        print("bench.py: --gpus %d but WORLD_SIZE=%d: start it as `python bench.py --gpus %d` (it launches the ranks itself) or as "
              "`python -m torch.distributed.run --nnodes=1 --nproc-per-node %d ... bench.py --gpus %d`" % (args.gpus, world, args.gpus, args.gpus, args.gpus),
              file=sys.stderr)
        sys.exit(2)
    # The harness translates ITS switches (flags, and the variables the tests hand to a bench child process) into explicit settings of
    # the package: itr_amd itself reads no environment variable.
    from itr_amd.settings import SETTINGS
    if args.virtual_split:
        SETTINGS.virtual_split = args.virtual_split
    SETTINGS.force_collectives = os.environ.get("ITR_FORCE_COLLECTIVES") == "1"
    if os.environ.get("ITR_SGRAF_IB"):
        SETTINGS.sgraf_image_block = int(os.environ["ITR_SGRAF_IB"])
    if os.environ.get("ITR_SGR_GROUP_ROWS") == "32":          # tools/ab_sgr.sh: the two-class node-group plan (same scores)
        SETTINGS.sgr_group_rows = 32
    backend = os.environ.get("ITR_DIST_BACKEND", "nccl")   # "gloo": several ranks on ONE GPU (tests); collectives staged through the host
    have_gpu = not args.launch_check or torch.cuda.is_available()
    if backend == "gloo":
        local_rank = local_rank % max(1, torch.cuda.device_count())
    elif have_gpu and local_rank >= torch.cuda.device_count():
        print("bench.py: rank %d wants device %d but this node exposes %d GPUs (one rank per GPU over RCCL)" % (rank, local_rank, torch.cuda.device_count()),
              file=sys.stderr)
        sys.exit(2)
    if have_gpu:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    else:
        dev = torch.device("cpu")
    # ITR_FORCE_COLLECTIVES=1: run every RCCL call of the N>1 path with a single rank (1-GPU box smoke of the
    # collectives' dtypes/ops; see tests/test_kernels_gpu.py::test_bench_collectives_single_rank)
    use_dist = world > 1 or os.environ.get("ITR_FORCE_COLLECTIVES") == "1"
    if use_dist:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # An explicit, short collective timeout instead of the process group's 10-minute default (VERDICT r4 #3b): the longest
        # stretch a rank legitimately waits for a peer is one step of the slowest config (SGR: 18 s / N) -- a first collective that
        # has not completed after three minutes is a dead fabric, and the error names the collective
        pg_timeout = datetime.timedelta(seconds=float(os.environ.get("ITR_DIST_TIMEOUT_S", "180")))
        progress("pg_init")
        if hang == "%d:pg_init" % rank:
            time.sleep(3600)
        if backend == "gloo":
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=pg_timeout)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=pg_timeout)
        # build the communicator now (RCCL creates it lazily on the first collective): never inside the timed region,
        # whatever --warmup is
        progress("pg_probe_collective")
        _probe = torch.zeros(1, device=dev if backend != "gloo" else "cpu")
        dist.all_reduce(_probe)
        dist.barrier()
        assert dist.get_world_size() == args.gpus
    progress("pg_ready")
    launch = {"ranks": gather_rank_table(dev, backend if use_dist else "none", world, rank, local_rank),
              "rccl_world": dist.get_world_size() if use_dist else 1,
              "dist_backend": (dist.get_backend() if use_dist else "none"),
              "launched_by": os.environ.get("ITR_BENCH_LAUNCHED_BY", "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "direct")}
    progress("rank_table")
    # one rank per GPU: the local device indices are distinct by construction (LOCAL_RANK, checked against device_count above) and RCCL
    # itself refuses two ranks on one device; the PCI ids are evidence for the reader of the line, not a gate (a virtualised node may
    # not expose them)
    launch["distinct_devices"] = len(set((r["device_index"], r["pci_bus_id"]) for r in launch["ranks"]))
    if backend == "nccl" and world > 1 and len(set(r["device_index"] for r in launch["ranks"])) != world:
        print("bench.py: %d ranks on %d distinct devices" % (world, len(set(r["device_index"] for r in launch["ranks"]))), file=sys.stderr)
        sys.exit(2)
    if args.launch_check:
        progress("fabric_check")
        nbytes = args.launch_check_bytes if args.launch_check_bytes is not None else (1.33e9 if dev.type == "cuda" else float(16 << 20))
        fabric = fabric_check(dev, backend if use_dist else "none", world, rank, use_dist, nbytes)
        if rank == 0:
            print(json.dumps(dict({"metric": METRIC, "value": None, "unit": "pairs/s", "n_gpus": world, "launch_check": True, "fabric": fabric},
                                  **launch)), flush=True)
        progress("done")
        if use_dist:
            dist.destroy_process_group()
        if not (fabric["all_gather_into_tensor"]["ok"] and fabric["all_reduce_counts"]["ok"]):
            sys.exit(5)
        return

    if args.from_files:
        progress("workload:from_files")
        main_from_files(args, world, rank, dev, use_dist)
        progress("done")
        if use_dist:
            dist.destroy_process_group()
        return
    line = LineOnce()
    rc = 0
    try:
        progress("workload:%s" % args.workload)
        out = run_workload(args, world, rank, dev, use_dist, backend)
        if rank == 0:
            out.update(launch)
            line.out = out
            rp = (out.get("cpu_baseline") or {}).get("recall_parity")
            if rp is not None and not rp["ok"]:
                print("bench.py: Recall parity FAILED: |dR@K| = %.3f > %.1f on the CPU sample block" % (rp["max_abs_recall_diff"], RECALL_TOL), file=sys.stderr)
                rc = 4
        if args.full and args.workload == DEFAULT_WORKLOAD and not args.no_other_configs and not args.virtual_split:
            other_configs(args, world, rank, dev, use_dist, backend, line)
        if (args.full and args.workload == DEFAULT_WORKLOAD and not args.no_train_configs and not args.no_other_configs and not args.virtual_split
                and world == 1 and not use_dist and dev.type == "cuda" and os.environ.get("ITR_BENCH_OTHER") != "small"):
            progress("train_configs")
            line.out["train_configs"] = train_configs_in_child(240)
    finally:
        # the primary workload's line, whatever the secondary runs did (an exception on this rank lands here too)
        if rank == 0:
            line.emit()
    progress("done")
    if use_dist:
        dist.destroy_process_group()
    if rc:
        sys.exit(rc)


def other_configs(args, world, rank, dev, use_dist, backend, line):
    """A driver-observed number for EVERY BASELINE.json config, after (never inside) the timed region of the line's own workload: the
    same step function, the same barrier / max-over-ranks timing, fewer steps.  cal_sims is the one scorer loop of all the model
    families (/root/reference/itr/metricmodule/evaluation.py:124-153).  Never at the price of the line itself:
      * one process (N = 1): every config runs in a fresh CHILD process with a time limit -- a fault, abort or out-of-memory there
        is recorded as that config's error;
      * N ranks: in this process group (the configs are sharded like the primary).  A config that raises on every rank is recorded
        and skipped (the ranks agree through one tiny all-reduce); an ASYMMETRIC failure (one rank raises while its peers wait in
        a collective) cannot be agreed on -- rank 0's watchdog then prints the primary line with what has finished and ends the
        process, and the collective timeout (ITR_DIST_TIMEOUT_S) ends the peers;
      * nothing more is started once these runs have taken five minutes."""
    import threading
    others = {}
    if rank == 0:
        line.out["other_configs"] = others
    small = os.environ.get("ITR_BENCH_OTHER") == "small"      # tests: the 1k x 5k forms only
    in_child = world == 1 and not use_dist
    t_other = time.perf_counter()
    wd = None
    if rank == 0 and not in_child:
        def bark():
            if line.emit({"other_configs_error": "watchdog: the other configs did not finish within 420 s (asymmetric failure or hang); "
                                                 "the configs listed are those that had finished"}):
                sys.stderr.write("bench.py: watchdog: other_configs hung; primary line printed, exiting with code 6\n")
                sys.stderr.flush()
                os._exit(6)       # "primary line OK, secondary configs hung": not a clean run (the peers end by ITR_DIST_TIMEOUT_S)
        wd = threading.Timer(420.0, bark)
        wd.daemon = True
        wd.start()
    try:
        for name, k, w in OTHER_CONFIGS:
            if small and not name.endswith("f30k1k"):
                continue
            progress("workload:%s" % name)
            ok, err, o = 1, None, None
            t0 = time.perf_counter()
            if in_child:
                o, err = other_config_in_child(name, k, w, 240)
                ok = int(o is not None)
            else:
                a2 = argparse.Namespace(**dict(vars(args), workload=name, steps=k, warmup=w, full=False, dump_outputs=None))
                try:
                    o = run_workload(a2, world, rank, dev, use_dist, backend)
                except Exception as e:      # noqa: BLE001
                    ok, err = 0, "%s: %s" % (type(e).__name__, e)
            flag = torch.tensor([ok, int(time.perf_counter() - t_other < 300.0)], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
            if use_dist:
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if rank == 0:
                if int(flag[0]) and o is not None:
                    others[name] = other_config_row(name, k, w, o, time.perf_counter() - t0)
                    if in_child:
                        others[name]["process"] = "child"
                else:
                    others[name] = {"baseline_config": BASELINE_CONFIG_OF[name], "error": err or "failed on another rank"}
            if not int(flag[1]):
                break
    finally:
        if wd is not None:
            wd.cancel()


def run_workload(args, world, rank, dev, use_dist, backend):
    """One workload, timed as the contract says (W untimed steps, barrier + synchronize, K steps, barrier + synchronize, MAX over
    ranks).  Returns the result dict on rank 0 and None elsewhere.  Without args.full: no CPU leg, no study variant, no clock probe."""
    import gc
    try:
        if "pooled" in WORKLOADS[args.workload]:
            return main_pooled(args, WORKLOADS[args.workload], world, rank, dev, use_dist)
        return main_words(args, world, rank, dev, use_dist, backend)
    finally:
        gc.collect()
        torch.cuda.empty_cache()      # the next workload starts from an empty pool, like a fresh process would


def main_words(args, world, rank, dev, use_dist, backend):
    """The word-level scorers: SCAN (t2i / i2t) and SGRAF (SAF / SGR) on bi-GRU word embeddings."""
    from itr_amd import evalpipe, ops
    wl = WORKLOADS[args.workload]
    n_img, n_cap = wl["n_img"], 5 * wl["n_img"]
    F_, D, R = 2048, 1024, 36
    is_sgraf = "sgraf" in wl
    cfg = dict(wl, bi_gru=True, no_txtnorm=not is_sgraf, no_imgnorm=False)
    sim_w = None
    if is_sgraf:
        cfg.update(module_name=wl["sgraf"], sgr_step=3)
        sim_w_cpu = make_sgraf_weights(wl["sgraf"])
        sim_w = {k: v.to(dev) for k, v in sim_w_cpu.items()}
        wl = dict(wl, _sim_weights=sim_w_cpu)

    # ---- synthetic inputs (seeded; identical on every rank, each rank keeps its shard in HBM)
    wi, wt = make_weights(wl["vocab"])
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    feats = torch.randn(n_img, R, F_, device=dev, generator=g)
    feats = ops.l2norm(feats)                                       # precomp features are l2-normalised
    lengths, tokens = make_captions(n_cap, wl["vocab"])
    comm = evalpipe.Comm()
    i0, i1 = evalpipe.block_range(n_img, comm.world, comm.rank, 4)
    cap_ranges = evalpipe.caption_ranges(n_cap, comm.cap_world, lengths)      # near-equal TOKEN sums per owner
    c0, c1 = cap_ranges[comm.cap_rank]
    feats_local = feats[i0:i1].contiguous()
    feats_head = feats[:args.cpu_sample_images].cpu() if args.full and rank == 0 else None
    del feats
    toks, tok_off, lens_sorted, order = shard_captions(lengths, tokens, c0, c1, dev)
    model = evalpipe.GruModelEval({k: v.to(dev) for k, v in wi.items()}, {k: v.to(dev) for k, v in wt.items()}, cfg, comm)
    torch.cuda.synchronize()

    timers = dict(scan_start=torch.cuda.Event(enable_timing=True), scan_end=torch.cuda.Event(enable_timing=True))

    peers = None
    if comm.virtual:       # the other virtual owners' packed token shards (their word embeddings are produced inside step())
        peers = {q: shard_captions(lengths, tokens, lo, hi, dev) for q, (lo, hi) in enumerate(cap_ranges) if q != comm.cap_rank and hi > lo}

    def step(tm=None):
        if peers is not None:
            comm.peer_blocks = {q: model.encode_captions(p[0], p[1], p[2]) for q, p in peers.items()}
        # every rank generated all the captions: their lengths are known everywhere, no metadata exchange (all_lengths)
        return model.scan_eval(feats_local, toks, tok_off, lens_sorted, order, n_img, n_cap, timers=tm, sgraf_weights=sim_w,
                               cap_ranges=cap_ranges, all_lengths=lengths)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    scan_ms, step_ms = [], []
    t0 = time.perf_counter()
    S = ranks = plan = None
    for _ in range(args.steps):
        ts = time.perf_counter()
        # As a validation loop would: the previous 0.5 GB score matrix is released before the next evaluation.  (Holding it made
        # the second timed step allocate a second one -- a hipMalloc of 60 ms, 350 ms in the first process on a fresh machine.)
        S = ranks = plan = None
        S, ranks, plan = step(timers)
        # the step already synchronised the stream when it copied the ranks to the host; with several ranks the row block is
        # scored in up to three launches (own captions while the exchange is in flight, then the others): their sum
        scan_ms.append(sum(a.elapsed_time(b) for a, b in timers["segments"]))
        step_ms.append(1e3 * (time.perf_counter() - ts))
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device=dev if backend != "gloo" else "cpu", dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    # every rank's own step times and how long its scoring stream still waited for the all-gather (VERDICT r4 #3d): a slow rank
    # or an exposed exchange shows up in the line, not only in the max-over-ranks total
    wait_ms = timers["exchange_wait"][0].elapsed_time(timers["exchange_wait"][1]) if "exchange_wait" in timers else 0.0
    per_rank = gather_floats([min(step_ms), max(step_ms), float(np.mean(step_ms)), float(np.mean(scan_ms)), wait_ms], dev, backend, use_dist)

    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, S, ranks, i0)
        ms_per_step = 1e3 * dt / args.steps
        pairs = float(n_img) * n_cap
        n_words = int(lengths.sum())
        # SCAN K7 = (4*36+6) * W * D flop per (image, caption) pair, summed over the pairs this rank scored
        alg_flop = float(i1 - i0) * n_words * (4 * 36 + 6) * D
        # executed by this design: raw dot products only (2*36*W*D) + the 36x36 quadratic form per (image, word)
        exe_flop = float(i1 - i0) * n_words * (2 * 36 * D + 36 * 37)
        k_ms = float(np.mean(scan_ms))
        model_name = "SCAN %s %s bi-GRU" % (wl.get("cross_attn"), wl.get("agg_func"))
        kernel_name, note = "scan_xattn_kernel", ("achieved/frac count the flop the kernel executes (2*36*W*D dot products + the 36x36 quadratic "
                                                  "form per word); SURVEY 8d's algorithmic (4*36+6)*W*D flop/pair, about twice that because the "
                                                  "context bmm is replaced by the Gram identity (DESIGN.md 4.3), is in algorithmic_equiv_*")
        if is_sgraf:
            # 4*36*W*D + 2*W*D*s + 2*D*s + T*(6*(W+1)*s^2 + 4*(W+1)^2*s) + 2s per pair (T = 0 for SAF)
            s_, T_ = 256, (3 if wl["sgraf"] == "SGR" else 0)
            W_ = lengths.astype(np.float64)
            per_img = (4 * 36 * W_ * D + 2 * W_ * D * s_ + 2 * D * s_ + T_ * (6 * (W_ + 1) * s_ ** 2 + 4 * (W_ + 1) ** 2 * s_) + 2 * s_).sum()
            alg_flop = float(i1 - i0) * per_img
            # executed: (i) the key projection of every graph step is folded into the query weight (softmax_j(q_i.k_j) =
            # softmax_j((W_k^T q_i).x_j)), so two of K8's three s x s projections per node and step are run;
            # (ii) the LAST step only produces node 0 (Fusionmodule.py:443 reads sim_emb[:, 0]): its query and graph projections
            # run for the global node only (2 x 2 W s^2 less) and its attention for one query row (4 (W+1) s instead of 4 (W+1)^2 s).
            # (Rounds 1-2 subtracted (i) only: their "executed" fractions counted ~8 % of flop that was never run.)
            exe_flop = alg_flop
            if T_:
                exe_flop -= float(i1 - i0) * (T_ * 2 * (W_ + 1) * s_ ** 2 + 4 * W_ * s_ ** 2 + 4 * (W_ + 1) * W_ * s_).sum()
            model_name = "SGRAF-%s bi-GRU" % wl["sgraf"]
            kernel_name = ("sgraf pair stage (scan_xattn_kernel emit + sgraf_loc_kernel + " +
                           ("sgr_fused_kernel: all graph steps of a caption group in one workgroup)" if wl["sgraf"] == "SGR" else "saf_pair_kernel)"))
            note = ("time = the whole itr_sgraf_scores call (global nodes + the pair stage in image blocks); algorithmic_* = SURVEY 8d K8; "
                    "achieved/frac = the flop executed: K8 minus the folded key projection of the SGR steps and minus the last step's work on "
                    "nodes other than node 0, which nothing reads (nothing is subtracted for SAF)")
        dtype, peak = "f32", FP32_MFMA_PEAK_TFLOPS
        if wl.get("scan_precision") in ("bf16x3", "fp16x3"):
            half = "bf16" if wl["scan_precision"] == "bf16x3" else "fp16"
            dtype, peak = "f32 inputs split into %s hi+lo planes, 3 %s MFMA products, f32 accumulate (%s)" % (half, half, wl["scan_precision"]), BF16_MFMA_PEAK_TFLOPS
            exe_flop = float(i1 - i0) * n_words * (3 * 2 * 36 * D + 36 * 37)
            note = ("STUDY VARIANT, reported separately: region x word dot products as hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_%s "
                    "(peak = dense bf16 / fp16 MFMA); the fp32 epilogue is unchanged.  " % ("bf16" if half == "bf16" else "f16") + note)
        from itr_amd import ops as _ops
        i2t = _ops.recall_from_ranks(ranks[0])
        t2i = _ops.recall_from_ranks(ranks[2])
        traffic, traffic_src = pmc_traffic(args.workload, world)
        out = {
            "metric": METRIC,
            "value": pairs / (dt / args.steps), "unit": "pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "step_ms": [round(x, 2) for x in step_ms],
            "step_ms_drift": round(step_ms[-1] - step_ms[0], 2) if len(step_ms) > 1 else 0.0,      # > 0: the chip clocks down as it warms up
            "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": args.workload, "scorer": model_name,
                       "n_img": n_img, "n_cap": n_cap, "regions": R, "feat_dim": F_, "embed": D,
                       "n_words": n_words, "parallelism": "row-shard x%d + 1 all-gather" % world,
                       "step": "encode(img proj + bi-GRU) + score + rank(i2t,t2i)"},
            "recall": {"i2t_r1": i2t[0], "i2t_r5": i2t[1], "i2t_r10": i2t[2], "t2i_r1": t2i[0], "t2i_r5": t2i[1],
                       "t2i_r10": t2i[2]},
            # order-sensitive checksums of the four rank vectors: equal across GPU counts iff the sharded result is identical
            "rank_checksum": [int((np.asarray(r, np.int64) * (np.arange(len(r)) % 9973 + 1)).sum()) for r in ranks],
            # achieved / frac = what the matrix core EXECUTES per launch / HIP-event kernel time (a hardware fraction, <= 1);
            # SURVEY 8d's algorithmic flop (which includes the context bmm this design never runs) is reported next to it
            "roofline": {"kernel": kernel_name, "bound": "mfma", "achieved": exe_flop / (k_ms * 1e-3) / 1e12,
                         "peak": peak, "unit": "TFLOP/s",
                         "frac": exe_flop / (k_ms * 1e-3) / 1e12 / peak,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "kernel_ms": k_ms, "executed_flop_per_launch": exe_flop,
                         "algorithmic_flop_per_launch": alg_flop,
                         "algorithmic_equiv_tflops": alg_flop / (k_ms * 1e-3) / 1e12,
                         "algorithmic_equiv_frac": alg_flop / (k_ms * 1e-3) / 1e12 / peak,
                         "note": note},
        }
        out["per_rank_step_ms"] = [dict(rank=q, min=round(r[0], 2), max=round(r[1], 2), mean=round(r[2], 2), score_kernels=round(r[3], 2),
                                        exchange_wait_after_own_launch=round(r[4], 3)) for q, r in enumerate(per_rank)]
        if is_sgraf:
            out["sgraf_block"] = dict(_ops.SGRAF_LAST_BLOCK)      # the image block the free memory admitted, and its workspace
        if "exchange_wait" in timers:
            # N > 1 (or the virtual split): time the scoring stream still had to wait for the all-gather after its own-column launch
            out["exchange"] = {"bytes_gathered": timers["exchange_bytes"], "own_launch_ms": timers["segments"][0][0].elapsed_time(timers["segments"][0][1]),
                               "wait_after_own_launch_ms": timers["exchange_wait"][0].elapsed_time(timers["exchange_wait"][1]),
                               "note": "last timed step, rank 0; ~0 = the collective ran under the own-column launch"}
        if comm.virtual:
            out["virtual_split"] = "%d:%d" % (comm.cap_world, comm.cap_rank)
            out["config"]["parallelism"] = "1 process, caption axis split over %d virtual owners (this one: %d): TEST HOOK, time is not a result" % (
                comm.cap_world, comm.cap_rank)
        if args.full and world == 1 and not is_sgraf and "scan_precision" not in wl and not comm.virtual:
            # the peak is quoted at 2 400 MHz; the chip sustains less under this kernel (power management): measured in-kernel
            try:
                mhz = scan_sustained_clock(model, feats_local, toks, tok_off, lens_sorted, order, cfg, dev)
            except Exception as e:          # a failed probe must not cost the line the timed run has already earned
                mhz = None
                out["roofline"]["clock_note"] = "clock probe failed: %r" % (e,)
            if mhz:
                out["roofline"]["sustained_clock_mhz"] = mhz
                out["roofline"]["frac_of_sustained_clock_peak"] = out["roofline"]["frac"] * 2400.0 / mhz
                out["roofline"]["clock_note"] = ("s_memtime / s_memrealtime summed over every workgroup of one extra instrumented launch; "
                                                 "frac uses the 2 400 MHz peak, frac_of_sustained_clock_peak the clock the chip actually ran at")
        if args.full and world == 1 and not is_sgraf and "scan_precision" not in wl and not args.no_variants and not comm.virtual:
            # Reported NEXT TO the exact-fp32 metric, never instead of it (STUDY_SPLIT_PRECISION.md): the same step with the region x word dot
            # products from split fp16 operands (hi.hi + hi.lo' + lo'.hi, fp32 accumulation) -- outside the timed region above
            vmodel = evalpipe.GruModelEval(model.wi, model.wt, dict(cfg, scan_precision="fp16x3"), comm)
            vt = dict(scan_start=torch.cuda.Event(enable_timing=True), scan_end=torch.cuda.Event(enable_timing=True))
            vstep = lambda tm=None: vmodel.scan_eval(feats_local, toks, tok_off, lens_sorted, order, n_img, n_cap, timers=tm, cap_ranges=cap_ranges,
                                                     all_lengths=lengths)
            vstep()
            torch.cuda.synchronize()
            tv = time.perf_counter()
            vk = []
            for _ in range(2):
                Sv, ranks_v, _ = vstep(vt)
                vk.append(sum(a.elapsed_time(b) for a, b in vt["segments"]))
            torch.cuda.synchronize()
            dtv = (time.perf_counter() - tv) / 2
            iv, tvv = _ops.recall_from_ranks(ranks_v[0]), _ops.recall_from_ranks(ranks_v[2])
            out["variant_fp16x3"] = {
                "value": pairs / dtv, "unit": "pairs/s", "ms_per_step": 1e3 * dtv, "kernel_ms": float(np.mean(vk)),
                "max_abs_diff_vs_fp32_scores": float((Sv - S).abs().max()), "mean_abs_diff_vs_fp32_scores": float((Sv - S).abs().mean()),
                "recall": {"i2t_r1": iv[0], "i2t_r5": iv[1], "i2t_r10": iv[2], "t2i_r1": tvv[0], "t2i_r5": tvv[1], "t2i_r10": tvv[2]},
                "note": "opt-in study variant, reported separately: fp32 inputs split into scaled fp16 hi + lo planes, 3 fp16 MFMA products, "
                        "fp32 accumulate; against a float64 oracle it is not further from the truth than the fp32 kernel (STUDY_SPLIT_PRECISION.md)"}
            del Sv
        if args.full and world == 1 and not args.no_cpu_baseline:
            base, S_cpu = cpu_baseline(wl, wi, wt, feats_head, lengths, tokens, args.cpu_sample_images, args.cpu_repeats)
            ns, ncs = args.cpu_sample_images, 5 * args.cpu_sample_images
            base["max_abs_diff_vs_gpu"] = float((S[:ns, :ncs].cpu() - S_cpu).abs().max())
            base["recall_parity"] = recall_parity(S[:ns, :ncs], S_cpu)
            base.update(cpu_fold_record(args.workload) or {})
            out["cpu_baseline"] = base
            out["speedup_vs_cpu_baseline"] = out["value"] / base["value"]
            # which CPU figure the ratio stands on: the bounded sample THIS run timed; the full 1k x 5k fold (a committed
            # record, minutes of host time) gives the other ratio, labelled as replayed
            out["speedup_vs_cpu_baseline_basis"] = "cpu_baseline.value: %s, timed in this run" % base["sample"]
            if base.get("fold_value"):
                out["speedup_vs_cpu_fold"] = out["value"] / base["fold_value"]
                out["speedup_vs_cpu_fold_basis"] = base["fold_source"]
        elif args.full and world > 1 and not args.no_cpu_baseline:
            rec = cpu_baseline_replayed(args.workload)
            if rec is not None:
                out["cpu_baseline"] = rec
                out["speedup_vs_cpu_baseline"] = out["value"] / rec["value"]
                out["speedup_vs_cpu_baseline_basis"] = "cpu_baseline.value: " + rec["source"]
        return out
    return None


if __name__ == "__main__":
    main()
