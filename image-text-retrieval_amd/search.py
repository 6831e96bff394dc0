#!/usr/bin/env python3
"""Answer queries against an encoded gallery:

    python search.py COARSE.pth.tar [FINE.pth.tar] --split test [--data-path P] [--index FILE.npz]
           (--query "a man riding a horse" ... | --queries FILE.txt | --query-images FILE.npy) [-k 10] [--rerank K] [--out FILE.npz]

COARSE (VSE++ with measure=cosine, or VSRN) shortlists; FINE (SCAN or SGRAF), with --rerank K, re-scores the K shortlisted items of
every query.  Sentences are answered with the split's distinct images, images ([n, 36, F] region features in a .npy file) with its
captions.  --index FILE.npz: the encoded gallery is loaded from the file if it exists, else built and saved there.  One line per
result is printed: query, rank, index, score -- for image queries also the caption's text.  --out FILE.npz: the result arrays (idx,
scores, coarse_idx, coarse_scores) and the query strings."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description="top-k search of sentences or images against the encoded gallery of a split")
    ap.add_argument("model_path", nargs="+", metavar="CHECKPOINT", help="COARSE.pth.tar [FINE.pth.tar]")
    ap.add_argument("--data-path", default=None)
    ap.add_argument("--split", default="test")
    ap.add_argument("--index", default=None, metavar="FILE.npz", help="load the encoded gallery from this file if it exists, else build and save it")
    ap.add_argument("--query", action="append", default=None, metavar="SENTENCE", help="a sentence to search images for (repeatable)")
    ap.add_argument("--queries", default=None, metavar="FILE.txt", help="sentences, one per line")
    ap.add_argument("--query-images", default=None, metavar="FILE.npy", help="region features [n, 36, F] to search captions for")
    ap.add_argument("-k", type=int, default=10, help="results per query (default 10)")
    ap.add_argument("--rerank", type=int, default=None, metavar="K", help="FINE re-scores the K >= k shortlisted items of every query")
    ap.add_argument("--out", default=None, metavar="FILE.npz", help="write the result arrays and the query strings")
    a = ap.parse_args(argv)
    if len(a.model_path) > 2:
        ap.error("one or two checkpoints: COARSE [FINE]")
    if sum(x is not None for x in (a.query, a.queries, a.query_images)) != 1:
        ap.error("give exactly one of --query, --queries, --query-images")
    if a.rerank is not None and len(a.model_path) != 2:
        ap.error("--rerank K needs a FINE checkpoint")

    import numpy as np
    from itr_amd.search import GalleryIndex
    coarse, fine = a.model_path[0], a.model_path[1] if len(a.model_path) == 2 else None
    if a.index is not None and os.path.exists(a.index):
        index = GalleryIndex.load(a.index, coarse, fine, data_path=a.data_path)
        print("index loaded from %s" % a.index)
    else:
        index = GalleryIndex.build(coarse, fine, data_path=a.data_path, split=a.split)
        if a.index is not None:
            index.save(a.index)
            print("index saved to %s" % a.index)
    if a.query_images is not None:
        feats = np.load(a.query_images)
        names = ["image %d" % i for i in range(len(feats))]
        res = index.search_images(feats, a.k, rerank=a.rerank)
    else:
        if a.queries is not None:
            with open(a.queries, 'rb') as f:
                names = [line.strip().decode('utf-8', 'ignore') for line in f if line.strip()]
        else:
            names = list(a.query)
        res = index.search_text(names, a.k, rerank=a.rerank)
    for qi, name in enumerate(names):
        print("query %d: %s" % (qi, name))
        for r in range(res.idx.shape[1]):
            i = int(res.idx[qi, r])
            text = ""
            if a.query_images is not None and i >= 0 and index.dataset is not None:
                text = "  " + index.dataset.caption_text(index.dataset.captions[i])
            print("  %3d  %8d  %.6f%s" % (r + 1, i, float(res.scores[qi, r]), text))
    if a.out is not None:
        with open(a.out, 'wb') as f:
            np.savez(f, queries=np.asarray(names), direction=np.asarray(res.direction), **res.arrays())


if __name__ == "__main__":
    main()
