#!/usr/bin/env python3
"""Evaluate checkpoints like the reference's test.py:  python test.py MODEL_PATH [MODEL_PATH_2] [--data-path P]
[--split test|testall|dev] [--fold5] [--topk K] [--gt FILE.npz] [--hubness csls|invsoftmax [--hub-k K] [--hub-beta B] [--querybank SPLIT]] [--rerank K [--stream-coarse] [--explain M | --explain-sgraf M]]  ->  <run dir>/<data_name>[_5fold]_{single,ensemble}_result.yaml
(and with --topk K the top-K retrieval lists of every query in <data_name>[_5fold]_{single,ensemble}_top<K>.npz).
With --gt FILE.npz (`pairs` [nnz, 2] of (image, caption), optionally n_images / n_captions): a ground-truth relation with any number of
positives per query  ->  also <data_name>_{single,ensemble}_gt_result.yaml (R@K, medr, meanr, R-Precision, mAP@R of both directions)
and <data_name>_{single,ensemble}_gt_positions.npz (the position of every positive in its query's ranked list)
With --hubness csls|invsoftmax: besides everything above, the matrix is corrected for hubs before ranking (S - a - b: CSLS with the mean of
the --hub-k nearest, or the inverted softmax at --hub-beta; statistics of the evaluated matrix itself, or of the split --querybank names)
->  also <data_name>[_5fold]_{single,ensemble}_hub_<method>_result.yaml and ..._hub_<method>.npz (the vectors a and b)
python test.py COARSE_PATH FINE_PATH --rerank K: coarse-to-fine retrieval, the first model shortlists K candidates per query and the
second (SCAN or SGRAF) scores only those  ->  <data_name>[_5fold]_rerank<K>_result.yaml and <data_name>[_5fold]_rerank<K>.npz
With --explain M (SCAN fine model): also the word-by-region attention maps, per-word / per-region similarities and scores of the
best M results of every query  ->  <data_name>_rerank<K>_explain<M>.npz
With --explain-sgraf M (SGRAF fine model): the word-by-region attention, SAF's filtration weights or SGR's graph edges of every
step, and the scores of the best M results of every query  ->  <data_name>_rerank<K>_explain<M>_sgraf.npz
python test.py COARSE_PATH FINE_1 FINE_2 [FINE_3 [FINE_4]] --rerank K: ensemble reranking, every fine model (SCAN or SGRAF, any mix; SAF + SGR
is the published SGRAF, SCAN t2i + i2t the published SCAN) scores the shortlists and they are re-ordered by the float64 mean of the
members' scores  ->  <data_name>[_5fold]_rerank<K>_ensemble_result.yaml and <data_name>[_5fold]_rerank<K>_ensemble.npz; with --explain M /
--explain-sgraf M every SCAN / SGRAF member explains the fused best M  ->  <data_name>_rerank<K>_ensemble_explain<M>_member<j>[_sgraf].npz"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from itr_amd.metricmodule import evaluation     # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("model_path", nargs="+")
    ap.add_argument("--data-path", default=None)
    ap.add_argument("--split", default="test")
    ap.add_argument("--fold5", action="store_true")
    ap.add_argument("--fast", action="store_true",
                    help="sharded device-resident evaluation (evalpipe.evaluate_precomp); run under torch.distributed.run for >1 GPU")
    ap.add_argument("--topk", type=int, default=0, metavar="K",
                    help="also write the top-K retrieved items of every query (indices and scores) to <data_name>..._top<K>.npz")
    ap.add_argument("--gt", default=None, metavar="FILE.npz",
                    help="a ground-truth relation over the gallery (`pairs` [nnz, 2] of (image, caption)): also write R@K, R-Precision and "
                         "mAP@R under it to <data_name>_..._gt_result.yaml and every positive's position to ..._gt_positions.npz")
    ap.add_argument("--rerank", type=int, default=0, metavar="K",
                    help="two checkpoints COARSE FINE: FINE (SCAN or SGRAF) re-scores only COARSE's top-K candidates of every query; "
                         "three to five checkpoints COARSE FINE_1 FINE_2 [FINE_3 [FINE_4]]: the fine models' scores of those candidates "
                         "are averaged in float64 (ensemble reranking)")
    ap.add_argument("--explain", type=int, default=None, metavar="M",
                    help="with --rerank K and a SCAN fine model: also write the attention maps of the best M <= K results of every query")
    ap.add_argument("--explain-sgraf", type=int, default=None, metavar="M",
                    help="with --rerank K and an SGRAF fine model: also write the attention, filtration weights (SAF) or graph edges (SGR) "
                         "of the best M <= K results of every query")
    ap.add_argument("--stream-coarse", action="store_true",
                    help="with --rerank K and a pooled coarse model: the coarse similarity matrix is streamed in row blocks and never "
                         "stored (a gallery whose matrix does not fit); same files")
    ap.add_argument("--hubness", choices=("csls", "invsoftmax"), default=None,
                    help="also rank the hubness-corrected matrix S - a - b and write <data_name>_..._hub_<method>_result.yaml and "
                         "..._hub_<method>.npz (the vectors); the plain results are written as without the flag")
    ap.add_argument("--hub-k", type=int, default=None, metavar="K", help="with --hubness csls: neighbours in the mean (default 10)")
    ap.add_argument("--hub-beta", type=float, default=None, metavar="B",
                    help="with --hubness invsoftmax: the inverse temperature (default 20)")
    ap.add_argument("--querybank", default=None, metavar="SPLIT",
                    help="with --hubness: the split (dev, train) whose queries define the correction, encoded with the same loader; "
                         "default: the evaluated split itself (transductive)")
    a = ap.parse_args()
    if a.hubness is None and (a.hub_k is not None or a.hub_beta is not None or a.querybank is not None):
        ap.error("--hub-k / --hub-beta / --querybank need --hubness csls|invsoftmax")
    if a.hubness is not None and a.fast:
        ap.error("--hubness does not combine with --fast: the sharded evaluation never holds a matrix to adjust")
    if a.hubness is not None and a.rerank:
        ap.error("--hubness does not combine with --rerank: the scores of coarse and fine lists are not comparable after a correction")
    hub_kw = {} if a.hubness is None else {'hubness': a.hubness, 'hub_k': 10 if a.hub_k is None else a.hub_k,
                                           'hub_beta': 20.0 if a.hub_beta is None else a.hub_beta,
                                           'querybank': 'self' if a.querybank is None else a.querybank}
    if a.stream_coarse and not a.rerank:
        ap.error("--stream-coarse needs --rerank K")
    if a.explain is not None and not a.rerank:
        ap.error("--explain needs --rerank K")
    if a.explain_sgraf is not None and not a.rerank:
        ap.error("--explain-sgraf needs --rerank K")
    if a.gt is not None and a.rerank:
        ap.error("--gt does not combine with --rerank: metrics of reranked lists under a general relation are not implemented")
    if a.gt is not None and a.fast:
        ap.error("--gt does not combine with --fast: the sharded evaluation ranks the 5-captions-per-image layout only")
    if a.gt is not None and a.fold5:
        ap.error("--gt does not combine with --fold5: a relation indexes one gallery")
    gt_kw = {} if a.gt is None else {'gt': a.gt}
    if a.rerank:
        if not 2 <= len(a.model_path) <= 5:
            ap.error("--rerank needs two checkpoints, COARSE FINE, or for an ensemble up to five: COARSE FINE_1 FINE_2 [FINE_3 [FINE_4]]")
        if a.fast or a.topk:
            ap.error("--rerank does not combine with --fast or --topk (the reranked lists are written to ..._rerank<K>.npz)")
        if len(a.model_path) == 2:
            evaluation.evalrank_rerank(a.model_path[0], a.model_path[1], a.rerank, data_path=a.data_path, split=a.split, fold5=a.fold5,
                                       explain=a.explain, explain_sgraf=a.explain_sgraf, stream_coarse=a.stream_coarse)
        else:
            evaluation.evalrank_rerank_ensemble(a.model_path[0], a.model_path[1:], a.rerank, data_path=a.data_path, split=a.split,
                                                fold5=a.fold5, explain=a.explain, explain_sgraf=a.explain_sgraf, stream_coarse=a.stream_coarse)
    elif a.fast:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl")
        evaluation.evalrank_fast(a.model_path[0], data_path=a.data_path, split=a.split, fold5=a.fold5, topk=a.topk)
        if dist.is_initialized():
            dist.destroy_process_group()
    elif len(a.model_path) == 1:
        evaluation.evalrank_single(a.model_path[0], data_path=a.data_path, split=a.split, fold5=a.fold5, topk=a.topk, **gt_kw, **hub_kw)
    else:
        evaluation.evalrank_ensemble(a.model_path[0], a.model_path[1], data_path=a.data_path, split=a.split, fold5=a.fold5,
                                     topk=a.topk, **gt_kw, **hub_kw)
