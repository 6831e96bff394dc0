#!/usr/bin/env python3
"""Time the training LOOP a user runs (`train.py` -> utils.train_step over get_loaders' train loader), not train_emb on batches that
already lie in HBM (tools/train_bench.py): per model family two arms on one synthetic coco_precomp-shaped train split,

    loader     the reference's path: DataLoader, workers=8, Python collate_fn, blocking host -> device copy in the step
    resident   resident_data=True: the split uploaded once, every batch gathered from HBM (datamodule/resident.py)

each arm in a fresh child process under its own time limit, the arms of a family back to back, the pair repeated --reps times.
Per child one JSON line: loop_ms_per_step (wall clock between two device synchronisations, the first --drop steps left out),
data_ms (the loop's own data_time meter over the same steps: what the host waits for a batch), upload_s and hbm_bytes of the
resident tables.  `--kernel` times itr_collate_batch alone with HIP events.  The parent appends every line to --out and prints
the table: median and min..max per arm, beside tools/train_bench.py's device-resident ms_per_step.

    python tools/train_loop_bench.py --out profiles/train_loop/loop.jsonl                  every family, 3 repeats
    python tools/train_loop_bench.py --families SCAN VSRN --reps 1 --out ...
    python tools/train_loop_bench.py --kernel --out profiles/train_loop/kernel.jsonl

Run on the GPU box.  Worker pools: the loader arm's 8 workers are the reference's `workers` default; nothing is sized by
os.cpu_count()."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "image-text-retrieval_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

FAMILIES = {"VSE_PP": ("VSE_PP", None, 128), "SCAN": ("SCAN", None, 128), "SGRAF-SAF": ("SGRAF", "SAF", 128), "SGRAF-SGR": ("SGRAF", "SGR", 128),
            "CAMERA": ("CAMERA", None, 128), "SAEM": ("SAEM", None, 64), "VSRN": ("VSRN", None, 128)}
NAME = "coco_precomp"
V_COCO = 11353


def make_split(out, n_img, seed=0):
    """<out>/data/coco_precomp/{train,dev}_{ims,boxes,img_sizes}.npy + _caps.txt, <out>/vocab/coco_precomp_vocab.json and
    <out>/bert/vocab.txt: l2-normalised random region rows, 5 captions of 4..18 random words per image (6..20 GRU tokens)."""
    import torch
    d = os.path.join(out, "data", NAME)
    for sub in (d, os.path.join(out, "vocab"), os.path.join(out, "bert")):
        os.makedirs(sub, exist_ok=True)
    rng = np.random.RandomState(seed)
    for split, n in (("train", n_img), ("dev", 8)):
        ims = np.lib.format.open_memmap(os.path.join(d, "%s_ims.npy" % split), mode="w+", dtype=np.float32, shape=(n, 36, 2048))
        for r0 in range(0, n, 512):
            r1 = min(n, r0 + 512)
            dev = "cuda" if torch.cuda.is_available() else "cpu"
            g = torch.Generator(device=dev)
            g.manual_seed(seed * 100003 + r0)
            x = torch.randn(r1 - r0, 36, 2048, device=dev, generator=g)
            ims[r0:r1] = (x / (x.pow(2).sum(-1, keepdim=True).sqrt() + 1e-8)).cpu().numpy()
        ims.flush()
        del ims
        wh = rng.randint(300, 640, size=(n, 2)).astype(np.float32)
        xy = np.sort(rng.rand(n, 36, 2, 2).astype(np.float32), axis=2)
        np.save(os.path.join(d, "%s_boxes.npy" % split), np.concatenate([xy[:, :, 0], xy[:, :, 1]], -1) * np.tile(wh, 2)[:, None, :])
        np.save(os.path.join(d, "%s_img_sizes.npy" % split), wh)
        with open(os.path.join(d, "%s_caps.txt" % split), "w") as f:
            for k in rng.randint(4, 19, size=5 * n):
                f.write(" ".join("w%d" % t for t in rng.randint(4, V_COCO, size=int(k))) + "\n")
    words = ["<pad>", "<start>", "<end>", "<unk>"] + ["w%d" % i for i in range(4, V_COCO)]
    json.dump({"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": {str(i): w for i, w in enumerate(words)}, "idx": len(words)},
              open(os.path.join(out, "vocab", "%s_vocab.json" % NAME), "w"))
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + ["[unused%d]" % i for i in range(995)] + ["w%d" % i for i in range(4, V_COCO)]
    open(os.path.join(out, "bert", "vocab.txt"), "w").write("\n".join(pieces) + "\n")


class _Limited(object):
    """The first `steps` batches of a loader; the clock starts (after a device synchronisation) when batch `drop` is asked for
    and stops (after another) when the loop asks for batch `steps`."""

    def __init__(self, loader, steps, drop):
        self.loader, self.steps, self.drop = loader, steps, drop
        self.dataset = getattr(loader, "dataset", None)
        self.t0 = self.t1 = None

    def __len__(self):
        return self.steps

    def __iter__(self):
        import torch
        it = iter(self.loader)
        for k in range(self.steps):
            if k == self.drop:
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
            yield next(it)
        torch.cuda.synchronize()
        self.t1 = time.perf_counter()
        del it


def child(a):
    """one arm of one family -> one JSON line on stdout"""
    import torch
    from itr_amd import config as C, utils
    from itr_amd.datamodule import data_loader as dl
    from itr_amd.metricmodule import evaluation
    from itr_amd.modalmodule import get_model
    model_name, module, batch = FAMILIES[a.family]
    over = ['with', model_name, 'data_name=' + NAME, 'data_path=' + os.path.join(a.data, "data"), 'vocab_path=' + os.path.join(a.data, "vocab"),
            'vocab_type=json', 'bi_gru=True', 'max_violation=True', 'img_dim=2048', 'batch_size=%d' % batch, 'workers=%d' % a.workers,
            'val_step=1000000000', 'log_step=1000000000', 'resident_data=%s' % (a.arm == 'resident'), 'bert_path=' + os.path.join(a.data, "bert")]
    if module:
        over.append('module_name=' + module)
    cfg = C.build_config(over)
    if model_name in ('SAEM', 'CAMERA'):
        import bench
        cfg_file, ckpt, trans = bench.bert_files(bench.BERT_DIR)
        cfg.update(bert_config_file=cfg_file, init_checkpoint=ckpt, trans_cfg=trans)
    utils.setup_seed(cfg['seed'])
    torch.cuda.set_device(0)
    torch.cuda.init()
    t_load = time.perf_counter()
    train_loader, val_loader, cfg['vocab_size'] = dl.get_loaders(cfg['data_name'], cfg['batch_size'], cfg['workers'], cfg)
    t_load = time.perf_counter() - t_load
    if model_name in ('SAEM', 'CAMERA'):
        cfg['vocab_size'] = 30522
    model = get_model(cfg).cuda()
    meters = []

    class Recording(evaluation.AverageMeter):          # train_step's own batch_time / data_time meters, value by value
        def __init__(self):
            super().__init__()
            self.vals = []
            meters.append(self)

        def update(self, val, n=0):
            if isinstance(val, float):                 # (the loss meters of the step hold device scalars: never read them here)
                self.vals.append(val)
            super().update(val, n)
    utils.eval.AverageMeter = Recording
    limited = _Limited(train_loader, a.steps, a.drop)
    if len(train_loader) < a.steps:
        raise SystemExit("the train split gives %d steps at batch %d, %d asked for" % (len(train_loader), batch, a.steps))
    utils.train_step(cfg, limited, model, 0, val_loader)
    batch_time, data_time = meters[0], meters[1]
    timed = a.steps - a.drop
    rs = getattr(train_loader, "resident_set", None)
    row = {"family": a.family, "arm": a.arm, "batch": batch, "steps": a.steps, "dropped": a.drop, "workers": a.workers if a.arm == 'loader' else 0,
           "loop_ms_per_step": round((limited.t1 - limited.t0) / timed * 1e3, 3),
           "data_ms": round(float(np.mean(data_time.vals[a.drop:])) * 1e3, 3),
           "data_ms_all_steps_avg": round(data_time.avg * 1e3, 3),
           "host_iter_ms": round(float(np.mean(batch_time.vals[a.drop:])) * 1e3, 3),
           "upload_s": round(rs.upload_seconds, 3) if rs is not None else 0.0, "hbm_bytes": int(rs.bytes_held) if rs is not None else 0,
           "get_loaders_s": round(t_load, 3), "max_memory_allocated": int(torch.cuda.max_memory_allocated()),
           "train_captions": len(train_loader.dataset), "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter between device synchronisations (loop), train_step's data_time meter (data)"}
    print("LOOPROW " + json.dumps(row), flush=True)


def kernel(a):
    """itr_collate_batch alone at B = 128, 36 x 2048: HIP events over --launches launches -> us per launch, TB/s of read + written bytes"""
    import torch
    from itr_amd import ops
    dev = torch.device("cuda", 0)
    rows = []
    for n_img, label in ((a.kernel_rows, "%d-row table" % a.kernel_rows),):
        feat = torch.randn(n_img, 36, 2048, device=dev)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        rng = np.random.RandomState(0)
        idxs = [torch.from_numpy(rng.randint(0, n_img, size=128).astype(np.int64)).to(dev) for _ in range(8)]
        for _ in range(10):
            ops.collate_batch(feat, idxs[0], bad_flag=flag)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = []
        for rep in range(3):
            e0.record()
            for k in range(a.launches):
                ops.collate_batch(feat, idxs[k % 8], bad_flag=flag)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / a.launches * 1e3)
        moved = 2 * 128 * 36 * 2048 * 4
        us = float(np.median(per))
        rows.append({"kernel": "itr_collate_batch", "B": 128, "row_elems": 36 * 2048, "table": label, "launches": a.launches, "us_per_launch": round(us, 2),
                     "us_min_max": [round(min(per), 2), round(max(per), 2)], "bytes_read_plus_written": moved, "TB_per_s": round(moved / us / 1e6, 3),
                     "includes": "the output allocation and launch of ops.collate_batch; back-to-back launches on one stream",
                     "device": torch.cuda.get_device_name(0), "clock": "HIP events around %d launches, median of 3" % a.launches})
    return rows


def run_child(cmd, limit):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"error": "time limit of %d s" % limit}
    for line in r.stdout.splitlines():
        if line.startswith("LOOPROW "):
            return json.loads(line[8:])
    return {"error": "exit %d: %s" % (r.returncode, (r.stderr or r.stdout)[-600:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="jsonl file the raw lines are appended to")
    ap.add_argument("--families", nargs="*", default=list(FAMILIES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--drop", type=int, default=20)
    ap.add_argument("--workers", type=int, default=8, help="the loader arm's DataLoader workers (the reference's default)")
    ap.add_argument("--n-img", type=int, default=7808, help="images of the synthetic train split (5 captions each): 7808 -> 305 steps of 128")
    ap.add_argument("--data", default=None, help="directory of the synthetic split (made when missing)")
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--no-train-bench", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--kernel-rows", type=int, default=7808)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--arm", default=None, choices=["loader", "resident"], help="(child) run one arm of --family and print its line")
    ap.add_argument("--family", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    if a.kernel:
        for row in kernel(a):
            emit(row)
        return
    data = a.data or os.path.join(tempfile.gettempdir(), "itr_train_loop_%d" % os.getuid())
    if not os.path.exists(os.path.join(data, "bert", "vocab.txt")):
        t0 = time.perf_counter()
        make_split(data, a.n_img)
        print("made %s: %d train images (%.2f GB) in %.0f s" % (data, a.n_img, a.n_img * 36 * 2048 * 4 / 1e9, time.perf_counter() - t0), flush=True)
    table = {}
    for fam in a.families:
        model_name, module, batch = FAMILIES[fam]
        for rep in range(a.reps):
            for arm in ("loader", "resident"):
                row = run_child([sys.executable, os.path.abspath(__file__), "--arm", arm, "--family", fam, "--data", data, "--steps", str(a.steps),
                                 "--drop", str(a.drop), "--workers", str(a.workers)], a.limit)
                row.update(family=fam, arm=arm, rep=rep)
                emit(row)
                if "error" in row:
                    # a child that failed may have left the device in a bad state: nothing more is started on it
                    raise SystemExit("%s / %s failed: %s" % (fam, arm, row["error"]))
                table.setdefault((fam, arm), []).append(row)
        if not a.no_train_bench:
            cmd = [sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "--model", model_name, "--json", "--steps", "20", "--warmup", "5"]
            if module:
                cmd += ["--module", module]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                tb = json.loads(r.stdout.strip().splitlines()[-1])["train_configs"][fam]
                row = {"family": fam, "arm": "train_emb on resident batches (tools/train_bench.py)", "ms_per_step": tb.get("ms_per_step"), "error": tb.get("error")}
            except Exception as e:      # noqa: BLE001
                row = {"family": fam, "arm": "train_emb on resident batches (tools/train_bench.py)", "error": "%s: %s" % (type(e).__name__, e)}
            emit(row)
            table[(fam, "emb")] = row.get("ms_per_step")
    print("\n%-10s | %-30s | %-30s | %-9s | %-20s | %s" % ("family", "loader loop ms (min..max)", "resident loop ms (min..max)", "train_emb", "data ms loader/resid.",
                                                            "upload s, HBM GB"))
    for fam in a.families:
        cell = {}
        for arm in ("loader", "resident"):
            rows = table.get((fam, arm), [])
            v = [r["loop_ms_per_step"] for r in rows]
            cell[arm] = ("%.2f (%.2f..%.2f, n=%d)" % (np.median(v), min(v), max(v), len(v))) if v else "-"
            cell[arm + "_d"] = ("%.2f" % np.median([r["data_ms"] for r in rows])) if rows else "-"
        res = table.get((fam, "resident"), [])
        print("%-10s | %-30s | %-30s | %-9s | %-20s | %s" % (fam, cell["loader"], cell["resident"], table.get((fam, "emb"), "-"),
                                                             cell["loader_d"] + " / " + cell["resident_d"],
                                                             ("%.1f, %.2f" % (np.median([r["upload_s"] for r in res]), res[0]["hbm_bytes"] / 1e9)) if res else "-"))


if __name__ == "__main__":
    main()
