"""GPU: the reference's Python seams (get_model / forward_emb / forward_loss / encode_data / cal_sims / i2t / t2i)
re-implemented on the HIP kernels, checked against golden vectors captured from the reference."""
import os

import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import config as C
from itr_amd.modalmodule import get_model
from itr_amd.metricmodule import evaluation

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.asarray(a))


class FakeLoader:
    """The collate_fn 8-tuple (data_loader.py:178), batches sorted by caption length."""

    def __init__(self, images, token_ids, lengths, batch):
        n = len(lengths)
        self.dataset = list(range(n))
        self.batches = []
        for b0 in range(0, n, batch):
            idx = sorted(range(b0, min(b0 + batch, n)), key=lambda i: -lengths[i])
            lens = [lengths[i] for i in idx]
            tok = torch.zeros(len(idx), max(lens), dtype=torch.long)
            for r, i in enumerate(idx):
                tok[r, :lengths[i]] = token_ids[i][:lengths[i]]
            self.batches.append((images[idx], None, None, tok, lens, idx, None, None))

    def __iter__(self):
        return iter(self.batches)


def scan_model_from_golden(g):
    cfg = C.build_config(['with', 'SCAN', 'bi_gru=True', 'data_name=coco_precomp'])
    cfg.update(img_dim=48, embed_size=32, word_dim=16, vocab_size=50)
    model = get_model(cfg)
    wi = {k[5:]: T(g[k]) for k in g.files if k.startswith("wimg_")}
    wt = {k[5:]: T(g[k]) for k in g.files if k.startswith("wtxt_")}
    model.load_state_dict([wi, wt])
    return model


def test_scan_harness_golden(golden, dev):
    g = golden("g11_harness_scan")
    model = scan_model_from_golden(g)
    feats = T(g["features"])
    lengths = [int(x) for x in g["lengths"]]
    loader = FakeLoader(feats.repeat_interleave(5, 0), T(g["token_ids"]), lengths, 32)
    img_embs, cap_embs, cap_lens = evaluation.encode_data(model, loader, islength=True)
    assert img_embs.shape == (200, 36, 32) and cap_embs.shape == g["cap_embs"].shape
    assert np.abs(img_embs[::5] - g["img_embs"]).max() <= 2e-6
    assert np.abs(cap_embs - g["cap_embs"]).max() <= 5e-6
    assert (cap_lens == g["cap_lens"]).all()
    img_u = img_embs[::5]
    sims = evaluation.cal_sims(model, img_u, cap_embs, cap_lens, shard_size=10 ** 9)
    assert sims.dtype == np.float64 and np.abs(sims - g["sims"]).max() <= 2e-5
    sims_sh = evaluation.cal_sims(model, img_u, cap_embs, cap_lens, shard_size=100)       # sliced lengths
    assert np.abs(sims_sh - g["sims"]).max() <= 2e-5
    sims_q1 = evaluation.cal_sims(model, img_u, cap_embs, cap_lens, shard_size=100, ref_quirk_unsliced_lengths=True)
    assert np.abs(sims_q1 - g["sims_q1_shard100"]).max() <= 2e-5
    # ranks on the reference's own matrix: bit-exact
    (ri, (ranks_i, top_i)) = evaluation.i2t(g["sims"], True)
    (rt, (ranks_t, top_t)) = evaluation.t2i(g["sims"], True)
    assert ri == pytest.approx(tuple(g["i2t"])) and rt == pytest.approx(tuple(g["t2i"]))
    assert (ranks_i == g["i2t_ranks"]).all() and (ranks_t == g["t2i_ranks"]).all()
    assert (top_i == g["i2t_top1"]).all() and (top_t == g["t2i_top1"]).all()
    # Recall@K of the HIP-scored matrix within +-0.1 of the reference (north_star)
    res = evaluation.cal_recall(sims)
    for k, want in zip(("i2t_r1", "i2t_r5", "i2t_r10"), g["i2t"][:3]):
        assert abs(res[k] - want) <= 0.1 + 1e-9
    for k, want in zip(("t2i_r1", "t2i_r5", "t2i_r10"), g["t2i"][:3]):
        assert abs(res[k] - want) <= 0.1 + 1e-9


def test_scan_forward_loss_vs_oracle(golden, dev):
    g = golden("g11_harness_scan")
    model = scan_model_from_golden(g)
    model.val_start()
    lengths = [int(x) for x in g["lengths"]]
    idx = sorted(range(24), key=lambda i: -lengths[i])
    lens = [lengths[i] for i in idx]
    tok = torch.zeros(24, max(lens), dtype=torch.long)
    for r, i in enumerate(idx):
        tok[r, :lengths[i]] = T(g["token_ids"])[i][:lengths[i]]
    feats = T(g["features"])[:24]
    img_emb, cap_emb, cap_lens = model.forward_emb(feats, tok, lens)
    loss = model.forward_loss(img_emb, cap_emb, cap_lens)
    wi = {k[5:]: T(g[k]) for k in g.files if k.startswith("wimg_")}
    wt = {k[5:]: T(g[k]) for k in g.files if k.startswith("wtxt_")}
    o_img = O.encoder_image_precomp(feats, wi["fc.weight"], wi["fc.bias"])
    o_cap, _ = O.encoder_text(tok, lens, wt, True, True, False, None)
    o_S = O.xattn_score(o_img, o_cap, lens)
    o_loss = O.hinge_loss(o_S, 0.2, False)
    assert abs(float(loss.detach()) - float(o_loss)) <= 1e-4 * max(1.0, float(o_loss))


def test_vsepp_cfg1_toy_batch(golden, dev):
    """BASELINE config 1 shape: 128-pair batch, bi-GRU text, pooled precomp regions, hinge with hardest negatives."""
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    cfg = C.build_config(['with', 'VSE_PP', 'data_name=coco_precomp', 'max_violation=True', 'bi_gru=True'])
    cfg.update(img_dim=256, embed_size=128, word_dim=32, vocab_size=300)
    model = get_model(cfg)
    model.val_start()
    B = 128
    lens = sorted([int(x) for x in rng.randint(3, 15, size=B)], reverse=True)
    tok = torch.zeros(B, max(lens), dtype=torch.long)
    for r, l in enumerate(lens):
        tok[r, :l] = torch.from_numpy(rng.randint(4, 300, size=l))
    feats = O.l2norm(torch.randn(B, 36, 256), -1)
    img_emb, cap_emb = model.forward_emb(feats, tok, lens)
    assert img_emb.shape == (B, 128) and cap_emb.shape == (B, 128)
    loss = model.forward_loss(img_emb, cap_emb)
    wi = {k: v.detach().cpu() for k, v in model.img_enc.state_dict().items()}
    wt = {k: v.detach().cpu() for k, v in model.txt_enc.state_dict().items()}
    o_img = O.encoder_image_precomp(feats.mean(1), wi["fc.weight"], wi["fc.bias"])
    o_cap, _ = O.encoder_text(tok, lens, wt, True, False, False, 'VSE++')
    assert float((img_emb.cpu() - o_img).abs().max()) <= 2e-6
    assert float((cap_emb.cpu() - o_cap).abs().max()) <= 5e-6
    o_loss = O.hinge_loss(O.cosine_sim(o_img, o_cap), 0.2, True)
    assert abs(float(loss.detach()) - float(o_loss)) <= 1e-4


def test_get_model_errors(dev):
    with pytest.raises(KeyError):
        get_model({'name': 'nope'})
    with pytest.raises(NotImplementedError):          # raw-image towers (torchvision CNNs) are out of scope
        get_model(dict(C.build_config(['with', 'VSRN']), data_name='coco', vocab_size=10))


def test_state_dict_round_trip(golden, dev):
    g = golden("g11_harness_scan")
    m1 = scan_model_from_golden(g)
    sd = m1.state_dict()
    assert isinstance(sd, list) and len(sd) == 2 and 'fc.weight' in sd[0] and 'rnn.weight_ih_l0_reverse' in sd[1]
    m2 = scan_model_from_golden(g)
    m2.load_state_dict(sd)
    assert torch.equal(m2.img_enc.fc.weight, m1.img_enc.fc.weight)


@pytest.mark.parametrize("mod", ["SAF", "SGR"])
def test_sgraf_model_wrapper(golden, dev, mod):
    """get_model('SGRAF'): forward_emb -> sim_enc -> forward_loss, checkpoint-style state_dict round trip."""
    g = golden("g6_sgraf")
    cfg = C.build_config(['with', 'SGRAF', 'module_name=%s' % mod, 'max_violation=True'])
    cfg.update(img_dim=48, embed_size=64, word_dim=16, vocab_size=50, sim_dim=32)
    model = get_model(cfg)
    pre = "w_%s_" % mod
    w = {k[len(pre):]: T(g[k]) for k in g.files if k.startswith(pre)}
    sd = model.sim_enc.state_dict()
    sd.update(w)
    model.sim_enc.load_state_dict(sd)
    model.val_start()
    sims = model.sim_enc(T(g["images"]).to(dev), T(g["captions"]).to(dev), [int(x) for x in g["cap_lens"]])
    assert float((sims.cpu() - T(g["sim_" + mod])).abs().max()) <= 5e-6
    loss = model.forward_loss(sims[:, :8].contiguous())
    want = O.hinge_loss(T(g["sim_" + mod])[:, :8], 0.2, True)
    assert abs(float(loss.detach()) - float(want)) <= 1e-4
    full = model.state_dict()
    assert len(full) == 3 and 'sim_tranloc_w.weight' in full[2]
    model.load_state_dict(full)
    # eval pipeline entry point used by cal_sims
    from itr_amd.metricmodule import evaluation
    d = evaluation.cal_sims(model, g["images"], g["captions"], g["cap_lens"], shard_size=10 ** 9)
    assert np.abs(d - g["sim_" + mod]).max() <= 5e-6


_BENCH_LINES = {}


def _bench_line(args, env=None, launcher=None, timeout=900):
    """One bench.py run -> its JSON line.  Plain single-process lines are cached per argument list (several tests compare
    against the same one)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    key = tuple(args)
    if env is None and launcher is None and key in _BENCH_LINES:
        return _BENCH_LINES[key]
    cmd = [sys.executable] + (launcher or []) + [os.path.join(root, "bench.py")] + list(args)
    r = subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]   # RCCL prints a version banner too
    assert len(line) == 1, r.stdout[-2000:]
    out = json.loads(line[0])
    if env is None and launcher is None:
        _BENCH_LINES[key] = out
    return out


def _base_args(workload):
    return ["--workload", workload, "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-variants", "--no-other-configs"]


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["scan_t2i_f30k1k", "sgraf_sgr_f30k1k", "sgraf_saf_f30k1k", "vsepp_f30k1k", "camera_f30k1k"])
def test_bench_collectives_single_rank(workload):
    """Every RCCL call of the N>1 path (asynchronous all-gather of the packed words / of the pooled caption vectors, fp32
    max / int32 sum / sign-flipped int64 max all-reduces, the ragged rank gather) executed with a 1-rank nccl group on the
    1-GPU box, for the word-level (SCAN, SGRAF) and the pooled (VSE++, CAMERA with its BERT tower) workloads: same rank
    vectors as the no-collective run."""
    plain = _bench_line(_base_args(workload))
    forced = _bench_line(_base_args(workload), env=dict(ITR_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541"))
    assert plain["recall"] == forced["recall"] and plain["rank_checksum"] == forced["rank_checksum"]
    assert forced["n_gpus"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("workload,split", [("scan_t2i_f30k1k", "3:1"), ("scan_t2i_f30k1k", "8:0"), ("scan_i2t_coco5k", "8:7"),
                                            ("sgraf_saf_f30k1k", "3:1"), ("sgraf_sgr_f30k1k", "4:3"), ("vsepp_f30k1k", "3:1"),
                                            ("vsrn_f30k1k", "2:0"), ("camera_f30k1k", "4:2"), ("saem_coco5k", "8:3")])
def test_virtual_split_runs_the_multi_rank_branch_on_one_gpu(workload, split):
    """The branch a multi-GPU run takes and a 1-GPU box otherwise never executes: with ONE process, the
    caption axis is treated as owned by k ranks (bench.py --virtual-split k:v, evalpipe.Comm).  The exchange is a real
    asynchronous collective on RCCL's stream (1-rank nccl group, ITR_FORCE_COLLECTIVES=1) -- and, in a second run, a copy on a
    side stream without any process group -- in flight while the own columns are scored on the current stream; wait(); the
    left / right launches read the gathered buffer.  The rank vectors must equal the plain single-launch run's for the
    word-level scorers (SCAN t2i / i2t, SGRAF SAF / SGR) and the pooled ones (VSE++, VSRN, CAMERA, SAEM)."""
    plain = _bench_line(_base_args(workload))
    # the exchange as a 1-rank RCCL collective for every workload; as a side-stream copy without a process group for two of them
    for force in (("1", "0") if (workload, split) in (("scan_t2i_f30k1k", "3:1"), ("vsepp_f30k1k", "3:1")) else ("1",)):
        virt = _bench_line(_base_args(workload) + ["--virtual-split", split],
                           env=dict(ITR_FORCE_COLLECTIVES=force, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543"))
        assert virt["virtual_split"] == split and virt["n_gpus"] == 1
        assert virt["rank_checksum"] == plain["rank_checksum"], (force, virt["rank_checksum"], plain["rank_checksum"])
        assert virt["recall"] == plain["recall"]


# ranks of one test that may share a single GPU: each holds its own context and workspaces, and the test process holds one too
RANKS_SHARING_ONE_GPU = 4


@pytest.mark.gpu
@pytest.mark.parametrize("workload,world", [("scan_t2i_f30k1k", 2), ("scan_t2i_f30k1k", 3), ("sgraf_saf_f30k1k", 2), ("sgraf_sgr_f30k1k", 3),
                                            ("vsepp_f30k1k", 2), ("vsrn_f30k1k", 2), ("camera_f30k1k", 2),
                                            ("scan_t2i_coco5k", 8), ("sgraf_saf_coco5k", 8)])
def test_sharded_eval_equals_single_process_on_one_gpu(workload, world):
    """The WHOLE sharded pipeline (row-sharded images, caption slices, packed all-gather, max / sum / key reductions,
    ragged rank gather) with real kernels: `world` ranks share this box's one GPU through the gloo backend (RCCL refuses
    two ranks per device) and must reproduce the single-process rank vectors exactly.  The two world-8 cases are the REAL
    partition of BASELINE configs[2] / [4]: 5 000 images in row blocks of 628 / ... / 604, 25 000 captions in token-balanced
    ranges (VERDICT r2 #2b).  Up to RANKS_SHARING_ONE_GPU ranks share one device; a larger world needs a GPU per rank (with gloo,
    rank r runs on device r % device_count)."""
    import torch
    n_dev = torch.cuda.device_count()
    if world > RANKS_SHARING_ONE_GPU and n_dev < world:
        pytest.skip("needs %d GPUs, found %d" % (world, n_dev))
    single = _bench_line(_base_args(workload))
    # (world 8 on ONE GPU: eight SGRAF workspaces side by side -- the smaller image block of rounds 1-3; scores do not depend on it)
    multi = _bench_line(["--gpus", str(world)] + _base_args(workload), env=dict(ITR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", ITR_SGRAF_IB="16"),
                        launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                                  "--master-port", str(29560 + world)], timeout=1500)
    assert multi["n_gpus"] == world
    assert multi["rank_checksum"] == single["rank_checksum"]
    assert multi["recall"] == single["recall"]


@pytest.mark.gpu
def test_bench_gpus_2_as_one_command_on_one_gpu():
    """`python bench.py --gpus 2` with NO launcher in front: bench.py starts the two ranks itself (gloo: they share
    this box's one GPU), the line says n_gpus = 2, carries the process group's world size and the all-gathered rank table, and the
    rank vectors equal the 1-rank line's.  `--gpus 1` is unchanged: one process, no group."""
    single = _bench_line(_base_args("scan_t2i_f30k1k"))
    assert single["n_gpus"] == 1 and single["rccl_world"] == 1 and len(single["ranks"]) == 1 and single["launched_by"] == "direct"
    assert single["ranks"][0]["pci_bus_id"] is not None
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + _base_args("scan_t2i_f30k1k"),
                       env=dict(env, ITR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1
    multi = json.loads(lines[0])
    assert multi["n_gpus"] == 2 and multi["rccl_world"] == 2 and multi["launched_by"] == "bench.py"
    assert [x["rank"] for x in multi["ranks"]] == [0, 1] and len({x["pid"] for x in multi["ranks"]}) == 2
    assert multi["rank_checksum"] == single["rank_checksum"] and multi["recall"] == single["recall"]
    # two nccl ranks on ONE device is refused loudly, not run as something else
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--launch-check"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and '{"metric"' not in r.stdout


@pytest.mark.gpu
def test_other_configs_ride_along_with_the_default_line():
    """the default workload's line carries a timed figure for every other BASELINE.json config.  Run here on the
    small default (ITR_BENCH_OTHER=small keeps the 1k x 5k forms only, so the test stays short)."""
    out = _bench_line(["--full", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-variants"], env=dict(ITR_BENCH_OTHER="small"),
                      timeout=1500)
    oc = out["other_configs"]
    assert set(oc) >= {"vsepp_f30k1k", "scan_t2i_f30k1k", "sgraf_saf_f30k1k", "sgraf_sgr_f30k1k"}
    for name, o in oc.items():
        assert o["ms_per_step"] > 0 and o["pairs_per_s"] > 0 and 0 < o["frac"] < 1 and len(o["rank_checksum"]) == 4, name
    assert oc["scan_t2i_f30k1k"]["rank_checksum"] == _bench_line(_base_args("scan_t2i_f30k1k"))["rank_checksum"]
    # one process: every other config ran in its own child process (a fault there cannot take the primary line with it)
    assert all(o["process"] == "child" for o in oc.values())
    # the same with two ranks (started by bench.py itself; gloo: they share the GPU): every config runs sharded, same rank vectors
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--full", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline", "--no-variants"], env=dict(env, ITR_DIST_BACKEND="gloo", ITR_BENCH_OTHER="small"), capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    two = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][0])
    assert two["n_gpus"] == 2 and two["rank_checksum"] == out["rank_checksum"]
    for name, o in two["other_configs"].items():
        assert "error" not in o, (name, o)
        assert o["rank_checksum"] == oc[name]["rank_checksum"], name


@pytest.mark.gpu
def test_plain_run_measures_only_the_headline():
    """Without --full the default workload's run stops after its timed steps: the line carries the headline figure and what the
    steps themselves gave, and none of the CPU leg, the fp16x3 variant, the clock probe, the other configs or the training timings."""
    out = _bench_line(["--steps", "1", "--warmup", "0"])
    assert out["config"]["workload"] == "scan_t2i_coco5k" and out["steps"] == 1 and out["ms_per_step"] > 0 and len(out["rank_checksum"]) == 4
    for key in ("cpu_baseline", "speedup_vs_cpu_baseline", "variant_fp16x3", "other_configs", "train_configs"):
        assert key not in out, key
    assert "sustained_clock_mhz" not in out["roofline"] and out["roofline"]["frac"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["scan_t2i_f30k1k", "vsepp_f30k1k", "sgraf_saf_f30k1k"])
def test_bench_line_carries_recall_parity_and_a_repeatable_cpu_baseline(workload):
    """the metric is "pairs/sec + Recall@1 parity" -- the line's cpu_baseline carries Recall@1/5/10 of the
    reference's argsort ranker on the CPU path's scores next to the HIP ranker's on the HIP path's scores for the same sample
    block (|dR@K| <= 0.1 or the run exits 4), the HIP ranker alone reproduces the argsort rank vectors on the CPU's matrix, and the
    CPU leg is timed more than once with the host it ran on recorded."""
    out = _bench_line(["--full", "--workload", workload, "--steps", "1", "--warmup", "0", "--no-variants", "--no-other-configs",
                       "--cpu-sample-images", "40", "--cpu-repeats", "2"])
    cb = out["cpu_baseline"]
    rp = cb["recall_parity"]
    assert rp["ok"] and rp["max_abs_recall_diff"] <= 0.1 and rp["hip_ranker_on_cpu_scores_equals_argsort"], rp
    assert set(rp["gpu"]) == set(rp["cpu"]) == {"i2t_r1", "i2t_r5", "i2t_r10", "t2i_r1", "t2i_r5", "t2i_r10"}
    assert rp["rank_entries"] == 40 + 200 and rp["rank_entries_differing"] <= 2
    h = cb["host"]
    assert h["repeats"] >= 2 and h["logical_cpus"] >= 1 and h["threads_used"] == cb["cores"] and cb["value"] > 0
    assert str(cb["cores"]) in h["seconds_by_threads"] and cb["max_abs_diff_vs_gpu"] <= 2e-5


@pytest.mark.gpu
def test_launch_check_runs_the_exchange_collectives_over_rccl():
    """VERDICT r4 #3c, the form a 1-GPU box can run: `--launch-check` with a 1-rank RCCL group moves the REAL payloads -- the
    1.33 GB packed-word all_gather_into_tensor and the 25 000-int32 sum all-reduce -- checks the contents and reports a rate."""
    out = _bench_line(["--launch-check"], env=dict(ITR_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547"))
    assert out["launch_check"] and out["value"] is None and out["dist_backend"] == "nccl"
    fab = out["fabric"]
    assert fab["all_gather_into_tensor"]["ok"] and fab["all_reduce_counts"]["ok"]
    assert fab["all_gather_into_tensor"]["bytes_total"] >= 1.3e9 and fab["all_gather_into_tensor"]["gb_per_s_received_per_rank"][0] > 50


@pytest.mark.gpu
def test_fp16x3_variant_rides_along_with_the_single_gpu_line():
    """The separately reported split-fp16 variant of the SCAN workloads: fp32-level scores, same Recall@K, reported next to
    (never instead of) the fp32 line."""
    single = _bench_line(["--full", "--workload", "scan_t2i_f30k1k", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
    v = single["variant_fp16x3"]
    assert v["max_abs_diff_vs_fp32_scores"] <= 1e-5 and v["recall"] == single["recall"]


@pytest.mark.gpu
def test_from_files_path_single_and_two_ranks(tmp_path):
    """bench.py --from-files on a small synthetic precomp directory (tools/make_synth_precomp.py): the file -> rank path
    (memory-mapped features streamed in row blocks, one-pass tokenisation, token-balanced caption ranges) gives the rank vectors
    of the resident-input step, with one process and with two ranks (gloo, sharing the GPU)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path / "synth")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "make_synth_precomp.py"), d, "--n-img", "1300", "--vocab", "500"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    base = [os.path.join(root, "bench.py"), "--from-files", d, "--steps", "1", "--warmup", "1"]

    def run(cmd, env):
        rr = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert rr.returncode == 0, rr.stderr[-3000:]
        line = [ln for ln in rr.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(line) == 1, rr.stdout[-2000:]
        return json.loads(line[0])

    single = run([sys.executable] + base, dict(os.environ))
    assert single["ranks_identical_to_resident"] and single["config"]["n_img"] == 1300 and single["config"]["n_cap"] == 6500
    env = dict(os.environ, ITR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    multi = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                 "--master-port", "29577", base[0], "--gpus", "2"] + base[1:], env)
    assert multi["n_gpus"] == 2 and multi["ranks_identical_to_resident"]
    assert multi["rank_checksum"] == single["rank_checksum"]


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["scan_t2i_f30k1k", "vsepp_f30k1k"])
def test_bench_dump_outputs_are_the_last_timed_step(workload, tmp_path):
    """bench.py --dump-outputs DIR: --steps timed steps ran, and DIR holds the rank vectors of the line (same checksums, float64)
    and float32 score rows that rank like the line's i2t vector on the sampled rows; a second run writes the same ranks."""
    import numpy as np
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    dumps = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        out = _bench_line(["--workload", workload, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-variants", "--no-other-configs",
                           "--dump-outputs", d])
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        dumps.append({n: np.load(os.path.join(d, n + ".npy")) for n in bench.RANK_NAMES + ("score_rows", "score_row_index")})
    a, b = dumps
    ranks = [a[n] for n in bench.RANK_NAMES]
    assert all(r.dtype == np.float64 for r in ranks)
    assert [int((r.astype(np.int64) * (np.arange(len(r)) % 9973 + 1)).sum()) for r in ranks] == out["rank_checksum"]
    assert a["score_rows"].dtype == np.float32 and a["score_rows"].shape[1] == 5 * out["config"]["n_img"]
    rows = a["score_row_index"].astype(np.int64)
    top1 = a["score_rows"].shape[1] - 1 - np.argmax(a["score_rows"][:, ::-1], axis=1)
    assert np.array_equal(top1, a["i2t_top1"][rows].astype(np.int64))
    for n in bench.RANK_NAMES + ("score_row_index",):
        assert np.array_equal(a[n], b[n]), n
