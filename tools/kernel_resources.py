#!/usr/bin/env python3
"""Register, scratch and occupancy table of the kernels of HIP sources, from hipcc's own remarks (no GPU needed):

    python tools/kernel_resources.py [-I dir ...] [--match scan_train] file.hip [file.hip ...]

One line per kernel: demangled name, VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, static LDS bytes (dynamic LDS is not in it)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-text-retrieval_amd", "csrc")
FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "waves"),
          ("LDS Size [bytes/block]", "lds"))


def table(path, includes, arch):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=" + arch, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", path, "-o", os.devnull]
    for inc in includes:
        cmd += ["-I", inc]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True, check=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z ]+(?: \[[^\]]+\])?): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = {"name": m.group(1)}
            rows.append(cur)
        elif cur is not None:
            for label, key in FIELDS:
                if m.group(2).strip() == label:
                    cur[key] = int(m.group(3))
    names = subprocess.run(["c++filt"] + [r["name"] for r in rows], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()
    for r, n in zip(rows, names):
        r["name"] = re.sub(r"^void |\(.*\)$", "", n)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("-I", dest="includes", action="append", default=[CSRC, os.path.join(ROOT, "include")])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--match", default="", help="only kernels whose name matches this regular expression")
    a = ap.parse_args()
    print("%-72s %5s %5s %8s %6s %7s" % ("kernel", "VGPR", "SGPR", "scratch", "waves", "LDS"))
    for path in a.files:
        for r in sorted(table(path, a.includes, a.arch), key=lambda r: r["name"]):
            if re.search(a.match, r["name"]):
                print("%-72s %5d %5d %8d %6d %7d" % (r["name"], r.get("vgpr", -1), r.get("sgpr", -1), r.get("scratch", -1), r.get("waves", -1),
                                                    r.get("lds", -1)))


if __name__ == "__main__":
    sys.exit(main())
