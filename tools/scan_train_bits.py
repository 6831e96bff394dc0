#!/usr/bin/env python3
"""Bit fingerprint of the SCAN training kernels: one sha256 per case of tests/helpers/scan_train_cases.py and tensor (S, d_images,
d_words), from a forward and backward through ag.scan_t2i_scores / ag.scan_i2t_scores on the seeded inputs the float64 sweep uses.

    python tools/scan_train_bits.py > new.txt                          this tree
    python tools/scan_train_bits.py --tree tools/ab/parent > old.txt   a side-by-side build (tools/ab_checkout.sh <commit> parent)

Run each tree in a process of its own on the GPU box and diff the listings: a refactor that keeps every summation order leaves them
equal.  The cases and their inputs always come from THIS tree's table, so the two listings fingerprint the same inputs."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="root of the build whose library runs (default: this tree)")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    for p in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "oracle"), os.path.join(tree, "image-text-retrieval_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from itr_amd import autograd as ag
    import scan_train_cases as S
    assert os.path.abspath(ag.__file__).startswith(tree + os.sep), ag.__file__
    dev = torch.device("cuda", 0)
    for c in S.CASES:
        x = c.inputs()
        img = x['images'].to(dev)
        if c.unaligned:                      # as the sweep: a contiguous view one float into its buffer
            buf = torch.zeros(img.numel() + 8, device=dev, dtype=torch.float32)
            buf[1:1 + img.numel()].view_as(img).copy_(img)
            img = buf[1:1 + img.numel()].view_as(img)
        img = img.detach().requires_grad_(True)
        words = x['words'].to(dev).requires_grad_(True)
        off = np.concatenate([[0], np.cumsum(c.lens)[:-1]]).astype(np.int64)
        fn = ag.scan_t2i_scores if c.xa == 't2i' else ag.scan_i2t_scores
        Sd = fn(img, words, off, list(c.lens), c.norm, c.agg, S.LAMBDA_LSE, S.LAMBDA_SOFTMAX)
        out = {'S': Sd.detach()}
        if c.backward:
            (Sd * x['g_S'].to(dev)).sum().backward()
            out['d_images'], out['d_words'] = img.grad, words.grad
        for name, t in out.items():
            print("%s %s %s" % (c.name, name, hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
