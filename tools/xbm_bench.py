#!/usr/bin/env python3
"""Time the four cross-batch-memory loss entry points (csrc/xbm_loss.hip) with HIP events, DESIGN 4.5.2's protocol (that of
profiles/infonce): each entry called through the C ABI on preallocated buffers, `--calls` calls between two events, `--windows`
windows after `--warm` warm-up calls; median, min and max microseconds per call beside the bytes the pass must move and the
bandwidth that makes (a cached figure: the operands fit the Infinity Cache).

    python tools/xbm_bench.py --json out.json [--shapes 128x4096,128x16384]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from itr_amd import _lib
    from itr_amd.ops import _p, _stream
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x4096,128x16384")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    out = {}
    for shape in a.shapes.split(","):
        B, n = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(B + n)
        S, R, C = (torch.rand(s, generator=g).to(dev) for s in ((B, B), (B, n), (n, B)))
        group = torch.arange(B, dtype=torch.int32, device=dev) // 5                    # the batch of tools/train_bench.py
        bank = (torch.arange(n, dtype=torch.int32, device=dev) % B) // 5               # ... pushed n / B times
        loss, grad = torch.empty(1, device=dev), torch.ones(1, device=dev)
        ra, ca = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        rl, cl = torch.empty(B, device=dev), torch.empty(B, device=dev)
        dS, dR, dC = torch.empty_like(S), torch.empty_like(R), torch.empty_like(C)
        ws = torch.empty(int(lib.itr_xbm_workspace_bytes(B, n)), dtype=torch.uint8, device=dev)
        head = (_p(S), B, _p(R), n, _p(C), B, _p(group), _p(bank), B, n, 0)
        read = 4 * B * (B + 2 * n)
        entries = {
            "hinge_fwd": (lambda: lib.itr_xbm_hinge_fwd(*head, 0.2, 1, _p(loss), _p(ra), _p(ca), _p(ws), _stream()), 2 * 4 * B * B + read - 4 * B * B),
            "hinge_bwd": (lambda: lib.itr_xbm_hinge_bwd(*head, 0.2, 1, _p(ra), _p(ca), _p(grad), _p(dS), B, _p(dR), n, _p(dC), B, _stream()), 2 * read),
            "infonce_fwd": (lambda: lib.itr_xbm_infonce_fwd(*head, 20.0, _p(loss), _p(rl), _p(cl), _p(ws), _stream()), 2 * 4 * B * B + read - 4 * B * B),
            "infonce_bwd": (lambda: lib.itr_xbm_infonce_bwd(*head, 20.0, _p(rl), _p(cl), _p(grad), _p(dS), B, _p(dR), n, _p(dC), B, _stream()), 2 * read),
        }
        for name, (call, nbytes) in entries.items():
            for _ in range(a.warm):
                _lib.check(call())
            us = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            med = float(np.median(us))
            out["B%d n%d %s" % (B, n, name)] = dict(us_median=round(med, 2), us_min=round(min(us), 2), us_max=round(max(us), 2), bytes=nbytes,
                                                    gb_per_s=round(nbytes / med / 1e3, 1), workspace_bytes=int(ws.numel()))
            print("B=%d n=%d %-12s %8.2f us (min %.2f max %.2f)  %d bytes  %.1f GB/s" % (B, n, name, med, min(us), max(us), nbytes, nbytes / med / 1e3))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
