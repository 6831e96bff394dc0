#!/usr/bin/env python3
"""Time the score-distillation entry points (csrc/distill.hip) with HIP events, DESIGN 4.5.3's protocol (that of profiles/infonce):
each entry called through the C ABI on preallocated buffers, `--calls` calls between two events, `--windows` windows after `--warm`
warm-up calls; median, min and max microseconds per call beside the bytes the pass must move.  The InfoNCE entries (no groups) are
timed beside them at the same B.

    python tools/distill_bench.py --json out.json [--sizes 128,1024]"""
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
    ap.add_argument("--sizes", default="128,1024")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    out = {}
    for B in (int(x) for x in a.sizes.split(",")):
        g = torch.Generator().manual_seed(B)
        S, T = torch.rand(B, B, generator=g).to(dev), torch.rand(B, B, generator=g).to(dev)
        loss, grad = torch.empty(1, device=dev), torch.ones(1, device=dev)
        v = [torch.empty(B, device=dev) for _ in range(4)]
        dS = torch.empty_like(S)
        ws_d = torch.empty(int(lib.itr_distill_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        ws_n = torch.empty(int(lib.itr_infonce_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        mat = 4 * B * B
        entries = {
            "distill_fwd": (lambda: lib.itr_distill_fwd(_p(S), _p(T), B, B, B, 20.0, 20.0, _p(loss), _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]),
                                                        _p(ws_d), _stream()), 4 * mat, int(ws_d.numel())),
            "distill_bwd": (lambda: lib.itr_distill_bwd(_p(S), _p(T), B, B, B, 20.0, 20.0, _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), _p(grad),
                                                        _p(dS), B, _stream()), 3 * mat, 0),
            "infonce_fwd": (lambda: lib.itr_infonce_fwd(_p(S), None, B, B, 20.0, _p(loss), _p(v[0]), _p(v[1]), _p(ws_n), _stream()), 2 * mat,
                            int(ws_n.numel())),
            "infonce_bwd": (lambda: lib.itr_infonce_bwd(_p(S), None, B, B, 20.0, _p(v[0]), _p(v[1]), _p(grad), _p(dS), B, _stream()), 2 * mat, 0),
        }
        for name, (call, nbytes, ws_bytes) in entries.items():
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
            out["B%d %s" % (B, name)] = dict(us_median=round(med, 2), us_min=round(min(us), 2), us_max=round(max(us), 2), bytes=nbytes,
                                             gb_per_s=round(nbytes / med / 1e3, 1), workspace_bytes=ws_bytes)
            print("B=%d %-12s %8.2f us (min %.2f max %.2f)  %d bytes  %.1f GB/s" % (B, name, med, min(us), max(us), nbytes, nbytes / med / 1e3))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
