"""CPU, world_size 2 over gloo: the collective logic of the row-sharded evaluation (evalpipe.finalize_ranks,
Comm.all_gather_rows) must reproduce the single-process ranks exactly.  The HIP rank kernels are replaced by
their oracle here (injected callables) -- what is under test is the exchange: max-reduce of GT scores,
sum-reduce of partial t2i counts, sign-flipped max-reduce of the top-1 keys, ragged row all-gather."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _order_key(v):
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)


def cpu_gather_gt(S, im_div, row0, s_gt):
    n, nc = S.shape
    for j in range(nc):
        g = j // im_div - row0
        if 0 <= g < n:
            s_gt[j] = S[g, j]
    return s_gt


def cpu_rank_counts(S, im_div, row0, s_gt, t_rank, t_best):
    """Oracle twin of itr_rank_counts for a row block (partial t2i counts accumulate in place)."""
    Sn, gt = S.numpy(), s_gt.numpy()
    n, nc = Sn.shape
    i_rank = np.zeros(n, np.int32)
    i_top = np.zeros(n, np.int32)
    cidx = np.arange(nc)
    for r in range(n):
        gi = row0 + r
        best = None
        for g in range(im_div * gi, im_div * gi + im_div):
            c = int((Sn[r] > Sn[r, g]).sum() + ((Sn[r] == Sn[r, g]) & (cidx > g)).sum())
            best = c if best is None else min(best, c)
        i_rank[r] = best
        i_top[r] = nc - 1 - int(np.argmax(Sn[r][::-1]))
    rows = row0 + np.arange(n)
    for j in range(nc):
        col = Sn[:, j]
        t_rank[j] += int((col > gt[j]).sum() + ((col == gt[j]) & (rows > j // im_div)).sum())
        key = (_order_key(col) << np.uint64(32)) | rows.astype(np.uint64)
        t_best[j] = max(int(t_best[j]) & 0xffffffffffffffff, int(key.max())) - (1 << 64 if max(int(t_best[j]) & 0xffffffffffffffff, int(key.max())) >= (1 << 63) else 0)
    return torch.from_numpy(i_rank), torch.from_numpy(i_top), t_rank, t_best, s_gt


def _worker(rank, world, port, ni, tmp):
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from itr_amd import evalpipe
    import itr_oracle as O
    rng = np.random.RandomState(0)
    sims = rng.randn(ni, 5 * ni).astype(np.float32)
    sims[:, ::7] = np.round(sims[:, ::7])          # some exact ties
    comm = evalpipe.Comm()
    assert comm.world == world and comm.on
    i0, i1 = evalpipe.block_range(ni, world, rank, 4)
    S_local = torch.from_numpy(sims[i0:i1].copy())
    got = evalpipe.finalize_ranks(comm, S_local, i0, ni, 5, rank_fn=cpu_rank_counts, gather_fn=cpu_gather_gt)
    want = O.rank_counts(sims)
    ok = all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got, want))
    # ragged all-gather
    counts = [3 + 2 * q for q in range(world)]
    local = torch.full((counts[rank], 4), float(rank))
    buf, maxrows = comm.all_gather_rows(local, counts)
    for q in range(world):
        ok = ok and bool((buf[q * maxrows:q * maxrows + counts[q]] == q).all())
    # the pooled models' exchange: own columns first, then the other owners' (exchange_score), unequal blocks
    n_cap, D = 23, 6
    emb = torch.from_numpy(rng.randn(n_cap, D).astype(np.float32))
    img = torch.from_numpy(rng.randn(5, D).astype(np.float32))
    ranges = [(0, 9), (9, 23)]
    counts = [hi - lo for lo, hi in ranges]
    send = torch.zeros(max(counts), D)
    send[:counts[rank]] = emb[ranges[rank][0]:ranges[rank][1]]

    def score(im, cap, out):
        out.copy_(im @ cap.t())
        return out
    S = evalpipe.exchange_score(comm, img, send, ranges, n_cap, score)
    ok = ok and bool(torch.allclose(S, img @ emb.t(), rtol=0, atol=1e-6))
    # the same exchange as point-to-point sends / receives (SETTINGS.exchange = "p2p")
    from itr_amd.settings import SETTINGS
    SETTINGS.exchange = "p2p"
    S2 = evalpipe.exchange_score(comm, img, send, ranges, n_cap, score)
    SETTINGS.exchange = "all_gather"
    ok = ok and bool(torch.equal(S2, S))
    open(os.path.join(tmp, "ok_%d" % rank), "w").write("1" if ok else "0")
    dist.destroy_process_group()


@pytest.mark.parametrize("ni", [8, 22])
def test_sharded_ranks_equal_single_process(tmp_path, ni):
    world = 2
    port = 29500 + (os.getpid() % 2000) + ni
    mp.spawn(_worker, args=(world, port, ni, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert open(os.path.join(str(tmp_path), "ok_%d" % r)).read() == "1"


def test_block_range_partition():
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
    from itr_amd import evalpipe
    for n in (0, 1, 7, 1000, 5000):
        for world in (1, 2, 4, 8):
            for align in (1, 4):
                spans = [evalpipe.block_range(n, world, r, align) for r in range(world)]
                assert spans[0][0] == 0 and spans[-1][1] == n
                for (a0, a1), (b0, b1) in zip(spans[:-1], spans[1:]):
                    assert a1 == b0 and a0 <= a1
                assert all(lo % align == 0 or lo == n for lo, _ in spans)


def test_caption_ranges_balance_tokens():
    """caption shards are balanced by token count.  Ranges are contiguous, cover every caption once, and no
    rank's token sum exceeds the mean by more than one caption's length."""
    from itr_amd import evalpipe
    rng = np.random.RandomState(0)
    for n_cap, world in ((25000, 8), (5000, 3), (7, 4), (3, 8), (0, 2)):
        lens = rng.randint(6, 21, size=n_cap)
        lens[: n_cap // 3] = np.sort(lens[: n_cap // 3])[::-1]            # a skewed head: count-balanced shards would be unequal
        r = evalpipe.caption_ranges(n_cap, world, lens)
        assert len(r) == world and r[0][0] == 0 and r[-1][1] == n_cap
        assert all(r[q][1] == r[q + 1][0] and r[q][0] <= r[q][1] for q in range(world - 1))
        sums = [int(lens[lo:hi].sum()) for lo, hi in r]
        assert sum(sums) == int(lens.sum())
        if n_cap >= world * 4:
            assert max(sums) <= lens.sum() / world + 20 and min(sums) >= lens.sum() / world - 20
    assert evalpipe.caption_ranges(10, 1, np.ones(10)) == [(0, 10)]
    assert evalpipe.caption_ranges(10, 2) == [(0, 5), (5, 10)]
    with pytest.raises(ValueError):
        evalpipe.caption_ranges(10, 2, np.ones(9))


def test_caption_ranges_never_leave_an_owner_empty():
    """A few very long captions (or as many owners as captions) must not produce an empty range: that owner's text tower
    would have nothing to encode while the others wait for it in the all-gather."""
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
    from itr_amd import evalpipe
    for w, world in (([1000, 1, 1, 1, 1, 1, 1, 1], 4), ([1, 1, 1, 1, 1, 1, 1, 1000], 4), ([5, 5, 5, 5], 4), ([3, 900, 2, 2, 800, 1], 5)):
        r = evalpipe.caption_ranges(len(w), world, w)
        assert r[0][0] == 0 and r[-1][1] == len(w)
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(hi > lo for lo, hi in r), (w, world, r)
    r = evalpipe.caption_ranges(2, 4, [7, 7])          # fewer captions than owners: the first owners get one each
    assert [hi - lo for lo, hi in r] == [1, 1, 0, 0]


def test_virtual_caption_split_scores_like_one_owner():
    """Comm(virtual_split="k:v") on one process: exchange_score takes the several-owner order of work (own columns, wait,
    the other owners' columns from the gathered buffer) and must fill the same matrix as the plain single-owner call."""
    sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))
    from itr_amd import evalpipe
    rng = np.random.RandomState(3)
    n_cap, D = 31, 5
    emb = torch.from_numpy(rng.randn(n_cap, D).astype(np.float32))
    img = torch.from_numpy(rng.randn(7, D).astype(np.float32))
    calls = []

    def score(im, cap, out):
        calls.append(cap.shape[0])
        out.copy_(im @ cap.t())
        return out
    want = img @ emb.t()
    for k, v, ranges in ((3, 1, [(0, 11), (11, 22), (22, 31)]), (4, 0, [(0, 2), (2, 12), (12, 22), (22, 31)]),
                         (4, 3, [(0, 8), (8, 16), (16, 24), (24, 31)]), (3, 1, [(0, 10), (10, 10), (10, 31)])):
        comm = evalpipe.Comm(virtual_split="%d:%d" % (k, v))
        assert comm.virtual and comm.world == 1 and (comm.cap_world, comm.cap_rank) == (k, v)
        counts = [hi - lo for lo, hi in ranges]
        send = torch.full((max(counts), D), float("nan"))
        send[:counts[v]] = emb[ranges[v][0]:ranges[v][1]]
        comm.peer_blocks = {q: emb[lo:hi].clone() for q, (lo, hi) in enumerate(ranges) if q != v and hi > lo}
        del calls[:]
        S = evalpipe.exchange_score(comm, img, send, ranges, n_cap, score)
        assert torch.allclose(S, want, rtol=0, atol=1e-6), (k, v)
        assert sum(calls) == n_cap and (counts[v] == 0 or calls[0] == counts[v])      # own block first, every caption exactly once
    with pytest.raises(ValueError):
        evalpipe.Comm(virtual_split="3:3")


def _run_bench(args, env_extra=None, drop=()):
    import subprocess
    env = dict(os.environ, **(env_extra or {}))
    for k in drop:
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)


def test_bench_gpus_n_starts_n_ranks_itself():
    """`python bench.py --gpus 2` as ONE command: the parent makes no GPU call, starts two ranks through
    torch.distributed.run as a child process, and rank 0's line carries n_gpus = 2, the process group's world size and a rank
    table with two distinct processes that was all-gathered through that group."""
    import json
    r = _run_bench(["--gpus", "2", "--launch-check"], dict(ITR_DIST_BACKEND="gloo"), drop=("WORLD_SIZE", "RANK", "LOCAL_RANK"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_world"] == 2 and out["launched_by"] == "bench.py"
    assert [x["rank"] for x in out["ranks"]] == [0, 1] and len({x["pid"] for x in out["ranks"]}) == 2
    # VERDICT r4 #3c: after the rank table the launch check runs the exchange's two collectives on a real payload, checks what
    # arrived and reports a rate per rank (16 MiB here; 1.33 GB on GPUs)
    fab = out["fabric"]
    assert fab["all_gather_into_tensor"]["ok"] and fab["all_reduce_counts"]["ok"]
    assert fab["all_gather_into_tensor"]["bytes_total"] == 16 << 20 and len(fab["all_gather_into_tensor"]["gb_per_s_received_per_rank"]) == 2
    assert all(v > 0 for v in fab["all_gather_into_tensor"]["ms_per_rank"] + fab["all_reduce_counts"]["ms_per_rank"])


def test_bench_launch_deadline_kills_the_ranks_and_names_the_stuck_one():
    """VERDICT r4 #3b: a rank that never gets through process-group start-up must not hang the command silently.  Rank 1 stops at
    `pg_init` (test hook); the parent's init deadline passes, it prints what every rank last reported, kills the CHILD process
    group and exits 124 with no result line -- and none of the ranks survives."""
    import time
    t0 = time.time()
    r = _run_bench(["--gpus", "2", "--launch-check", "--init-deadline", "30"], dict(ITR_DIST_BACKEND="gloo", ITR_BENCH_TEST_HANG="1:pg_init",
                                                                                  ITR_DIST_TIMEOUT_S="600"),
                   drop=("WORLD_SIZE", "RANK", "LOCAL_RANK"))
    assert r.returncode == 124, (r.returncode, r.stderr[-2000:])
    assert time.time() - t0 < 120
    assert '{"metric"' not in r.stdout
    assert "DEADLINE" in r.stderr and "rank 1  stage=pg_init" in r.stderr, r.stderr[-2000:]
    pids = [int(ln.split("pid=")[1]) for ln in r.stderr.splitlines() if "pid=" in ln and "pid=None" not in ln]
    assert pids
    time.sleep(1.0)
    for pid in pids:
        assert not os.path.exists("/proc/%d" % pid) or open("/proc/%d/stat" % pid).read().split()[2] == "Z", pid


def test_bench_line_survives_failing_other_configs(monkeypatch, capsys):
    """the primary workload's line is printed exactly once whatever the secondary configs do -- a config that
    raises is recorded as its error, an exception that escapes still leaves the line (main()'s finally), and the watchdog's emit
    and the normal emit cannot both print."""
    import importlib
    import json
    import types
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    line = bench.LineOnce()
    line.out = {"metric": bench.METRIC, "value": 1.0}
    calls = []

    def fake(a2, *rest, **kw):
        calls.append(a2.workload)
        if a2.workload == "scan_i2t_coco5k":
            raise RuntimeError("boom")
        return {"ms_per_step": 1.0, "value": 2.0, "config": {"n_img": 1, "n_cap": 5}, "recall": {}, "rank_checksum": [0],
                "roofline": {"frac": 0.5, "achieved": 1.0, "kernel_ms": 1.0}}
    monkeypatch.setattr(bench, "run_workload", fake)
    args = types.SimpleNamespace(workload=bench.DEFAULT_WORKLOAD, steps=1, warmup=0)
    bench.other_configs(args, 2, 0, torch.device("cpu"), False, "gloo", line)      # world 2: the in-process form
    assert calls == [n for n, _, _ in bench.OTHER_CONFIGS]
    oc = line.out["other_configs"]
    assert "boom" in oc["scan_i2t_coco5k"]["error"] and oc["vsepp_f30k1k"]["frac"] == 0.5
    assert line.emit() and not line.emit() and not line.emit({"other_configs_error": "late watchdog"})
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{"metric"')]
    assert len(printed) == 1 and "other_configs_error" not in json.loads(printed[0])


def test_bench_refuses_a_world_that_is_not_gpus():
    """A 1-rank process asked for 2 GPUs (or 2 ranks asked for 1) exits non-zero and prints no result line."""
    r = _run_bench(["--gpus", "2", "--launch-check"], dict(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and '{"metric"' not in r.stdout
    r = _run_bench(["--gpus", "1", "--launch-check"], dict(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and '{"metric"' not in r.stdout


def test_bench_parent_makes_no_gpu_call_before_launching():
    """The launching parent must not initialise the GPU (a re-launch from a process that has is what takes this pool's machines
    down): between the top of main() and launch_ranks() there is no torch.cuda / HIP-library call."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    seen_launch = False
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and getattr(node.func, "id", "") == "launch_ranks":
            seen_launch = True
            launch_line = node.lineno
    assert seen_launch
    head = "\n".join(src.splitlines()[fn.lineno - 1:launch_line])
    assert "torch.cuda" not in head and "_lib" not in head and "itr_amd" not in head
    lr = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "launch_ranks"][0]
    body = "\n".join(src.splitlines()[lr.body[1].lineno - 1:lr.end_lineno])      # (past the docstring)
    assert "torch.cuda" not in body and "os.exec" not in body and "execv" not in body


def test_bench_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """--dump-outputs: the four rank vectors whole (float64, exact), a seeded sample of full score rows (float32) with their global
    row indices, the same sample every time, and at most 64 MB in all."""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    n_rows, n_cols, row0 = 1000, 25000, 40
    S = torch.randn(n_rows, n_cols, generator=torch.Generator().manual_seed(0))
    rng = np.random.RandomState(1)
    ranks = tuple(rng.randint(0, 5000, size=n).astype(np.int64) for n in (n_rows, n_rows, n_cols, n_cols))
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(d, S, ranks, row0)
    files = sorted(os.listdir(dirs[0]))
    assert files == sorted([n + ".npy" for n in bench.RANK_NAMES] + ["score_rows.npy", "score_row_index.npy"])
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in files) <= 64 << 20
    for name, r in zip(bench.RANK_NAMES, ranks):
        a = np.load(os.path.join(dirs[0], name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, r)
    rows, idx = np.load(os.path.join(dirs[0], "score_rows.npy")), np.load(os.path.join(dirs[0], "score_row_index.npy"))
    assert rows.dtype == np.float32 and rows.shape == (bench.DUMP_SCORE_ROWS, n_cols) and idx.dtype == np.float64
    assert np.array_equal(rows, S.numpy()[idx.astype(np.int64) - row0])
    for f in files:
        assert np.array_equal(np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f)))
    bench.dump_outputs(str(tmp_path / "c"), None, ranks, row0)          # --stream-scores: no matrix was kept
    assert sorted(os.listdir(str(tmp_path / "c"))) == sorted(n + ".npy" for n in bench.RANK_NAMES)
