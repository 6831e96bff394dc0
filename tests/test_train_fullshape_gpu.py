"""GPU: model.train_emb at the benchmarked training shapes (tools/train_bench.py: batch 128, 36 x 2048 regions, the COCO vocabulary,
word_dim 300, embed 1024, bi-GRU, sim_dim 256, max_violation) against the oracle's float64 step from the same weights and batch.
The toy-shape parity tests (G15 / G20) never reach the code this step runs: the 128-row split-K recurrence GEMMs, the skinny and
k-sliced dense layers, the split reduction of gemm_tn, the batched SGRAF kernels at B = C = 128 and S = 256, the dense SCAN backward,
and the multi-tensor clip + Adam over ~50 tensors and up to ~19 M parameters.  VSRN (batch 128, embed 2048, 61-id captions, the
captioning model with dim_hidden 512 over the 11 353-word vocabulary) adds the 4 608 x 2 048 GCN layers with training-mode BatchNorms,
the D = 2 048 region and text GRUs, the captioning decoder's 59 teacher-forced steps, and a clip + Adam over ~125 M parameters.

Per (config, batch): loss (and VSRN's Loss_caption / Loss_retrieval), pre-clip gradient norm, every parameter's clipped gradient by
name, and the BatchNorm running statistics of SGRAF and of VSRN's four GCNs (replayed from the oracle's batch statistics,
AttentionFiltration's once per caption).  Batch A is train_bench's shape;
batch B adds a dozen 33..64-word captions and two of 70 and 82 words (SCAN's MAXW = 64 / ST_MAXW kernels; SGRAF's batched path
with an 82-word Wmax).  Every error is bounded by the float32 oracle's own error on the host:

    err(GPU vs float64) <= K * err(host float32 vs float64) + FLOOR          (K = 8, FLOOR = 1e-6, relative)

Gradient errors are relative Frobenius errors; a parameter whose float64 gradient norm is below TINY x the largest one is measured
against TINY x the largest instead (an absolute bound).  The biases whose exact gradient is 0 (ZERO_GRAD) have a bound of their own.

The optimizer at full size (SCAN t2i, SGRAF-SGR and VSRN, batch A): the step's own clip + Adam against clip_grad_norm_ + torch.optim.Adam
in float64 (and float32 for the bound), all fed the GPU's fp32 gradients: every tensor's update, exp_avg and exp_avg_sq.

Precondition: the max-violation hinge follows one hardest negative per row and column; the smallest distance of the float64 score
matrix from a discrete change (top-2 gap of the negatives, or the hinge's kink) must be >= 10 x the GPU's and the host float32's
max |S - S64|, or the seed is unsuitable.  Seeds (one seed for the weights and the batch) and that distance, float64, on the host:

    VSEPP-A 15: 9.7e-5    SCAN-t2i-A 0: 4.9e-5    SCAN-t2i-B 1: 6.3e-5    SCAN-i2t-A 1: 1.1e-5
    SGRAF-SAF-A 10: 1.2e-5    SGRAF-SAF-B 12: 8.8e-6    SGRAF-SGR-A 19: 2.4e-6    VSRN-A 0: 5.4e-3 (the first seed tried)

VSRN reads every caption's state after its 61 ids, so the 128 caption vectors coincide (float64: to 3e-10) and each row's hardest
negative is a tie between interchangeable captions: for VSRN the rows' top-2 gaps are left out, and the tie itself is asserted
(F.caption_spread <= 1e-8).

Measured on one MI355X (the test prints these): worst err / bound, and worst err / max(err fp32, FLOOR / K), per configuration:

    VSEPP-A       0.10  1.0  scores
    SCAN-t2i-A    0.25  2.0  txt.rnn.bias_hh_l0_reverse
    SCAN-t2i-B    0.27  2.6  txt.rnn.weight_hh_l0_reverse; scores
    SCAN-i2t-A    0.19  2.1  scores
    SGRAF-SAF-A   0.40  3.2  sim.SAF_module.bn.weight
    SGRAF-SAF-B   0.32  2.6  sim.sim_eval_w.bias
    SGRAF-SGR-A   0.42  3.4  sim.sim_eval_w.bias
    VSRN-A        0.44  3.8  scores
    Adam, SCAN-t2i-A    0.25  2.1  txt.embed.weight exp_avg_sq
    Adam, SGRAF-SGR-A   0.69  5.8  sim.v_global_w.embedding_local.1.bias exp_avg_sq
    Adam, VSRN-A        0.13  1.0  img.Rs_GCN_1.g.bias update

VSRN's host float32 step clips with a pre-clip norm 9e-5 from float64 (torch's fp32 norm over 4 M-element tensors), so its clipped
gradients' float32 yardstick is about 1e-4: a silent error smaller than ~7e-4 of a VSRN gradient can pass.

The whole file takes about 90 s there with 16 CPUs, the float64 and float32 oracle steps included (VSRN's: 17 s and 5 s; each
case prints its own).
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fullshape as F  # noqa: E402
from itr_amd import ops  # noqa: E402
from itr_amd.metricmodule.evaluation import LogCollector  # noqa: E402
from itr_amd.modalmodule import get_model  # noqa: E402

pytestmark = pytest.mark.gpu

K, FLOOR, TINY = 8.0, 1e-6, 1e-4
SEEDS = {('VSEPP', 'A'): 15, ('SCAN-t2i', 'A'): 0, ('SCAN-t2i', 'B'): 1, ('SCAN-i2t', 'A'): 1, ('SGRAF-SAF', 'A'): 10, ('SGRAF-SAF', 'B'): 12,
         ('SGRAF-SGR', 'A'): 19, ('VSRN', 'A'): 0}
# biases whose exact gradient is 0: in front of a softmax over the axis they are broadcast along (VisualSA / TextSA weights), or of a
# BatchNorm whose statistics run over everything the bias is added to (VisualSA's global embedding, AttentionFiltration's BatchNorm1d(1)).
# What either side computes for them is the residue of a cancelling sum, scaled by 1 / sigma behind a BatchNorm; its size depends on
# the summation order, which varies from run to run on the GPU: 5e-10 .. 4e-8 of the largest gradient there, 1e-15 on the host (fp32).
# So they get a bound of their own, in units of ZERO_TOL x the largest gradient: K x the host fp32's residue + ZERO_TOL.  VSRN's GCN
# convolution W.0 sits in front of the GCN's BatchNorm (statistics over all 36 x 128 region rows); behind the first GCN the residue is
# amplified by 1 / sigma of a narrow W.0 output, 6e-7 of the largest gradient on the host in fp32.
ZERO_GRAD = {'sim.v_global_w.embedding_common.0.bias', 'sim.t_global_w.embedding_common.0.bias', 'sim.v_global_w.embedding_global.0.bias',
             'sim.SAF_module.attn_sim_w.bias'} | {'img.Rs_GCN_%d.W.0.bias' % i for i in (1, 2, 3, 4)}
ZERO_TOL = 1e-6
OPT_CASES = [('SCAN-t2i', 'A'), ('SGRAF-SGR', 'A'), ('VSRN', 'A')]   # the optimizer at full size: a GRU model, SGR, and the largest one
PREFIXES = {'SGRAF': ('img.', 'txt.', 'sim.'), 'VSRN': ('img.', 'txt.', 'cap.')}   # of the state dicts F.make_weights returns
BN_MODULE = {'SGRAF': 2, 'VSRN': 0}                                                  # which of them holds the BatchNorm buffers


def _threads():
    """The CPUs this process may use (the environment's allowance), never more than 16 -- not os.cpu_count()."""
    n = os.environ.get('OMP_NUM_THREADS')
    return max(1, min(16, int(n) if n and n.isdigit() else len(os.sched_getaffinity(0))))


def _named(model):
    out = [('txt.' + n, p) for n, p in model.txt_enc.named_parameters()] + [('img.' + n, p) for n, p in model.img_enc.named_parameters()]
    if getattr(model, 'sim_enc', None) is not None:
        out += [('sim.' + n, p) for n, p in model.sim_enc.named_parameters()]
    if getattr(model, 'caption_model', None) is not None:
        out += [('cap.' + n, p) for n, p in model.caption_model.named_parameters()]
    return out


def _gpu_step(cfg, weights, batch, keep_optimizer):
    feats, ids, lens = batch[:3]
    model = get_model(cfg)
    if cfg['name'] == 'VSRN':           # the captioning model is not part of VSRN's checkpoints (load_state_dict)
        model.img_enc.load_state_dict(weights[0])
        model.txt_enc.load_state_dict(weights[1])
        model.caption_model.load_state_dict(weights[2])
    else:
        model.load_state_dict(weights)
    model.txt_enc.dropout_p = 0.0
    if getattr(model, 'sim_enc', None) is not None:
        for m in model.sim_enc.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    model.train_start()
    model.logger = LogCollector()
    seen, hinge = [], ops.hinge_loss

    def spy(scores, *a, **k):             # the score matrix the step's own hinge reads
        seen.append(scores.detach().double().cpu())
        return hinge(scores, *a, **k)
    ops.hinge_loss = spy
    try:
        model.train_emb((feats, None, None, ids, lens, list(range(len(lens))), batch[3] if len(batch) > 3 else None, None))
    finally:
        ops.hinge_loss = hinge
    torch.cuda.synchronize()
    assert len(seen) == 1
    r = dict(loss=float(model.logger.meters['Loss'].val), grad_norm=float(model.optimizer.last_grad_norm[0]), scores=seen[0],
             grads={n: (p.grad.detach().cpu() if p.grad is not None else None) for n, p in _named(model)},
             terms={k: float(model.logger.meters[k].val) for k in ('Loss_caption', 'Loss_retrieval') if k in model.logger.meters})
    bn_mod = {'SGRAF': getattr(model, 'sim_enc', None), 'VSRN': model.img_enc}.get(cfg['name'])
    if bn_mod is not None:
        r['buffers'] = {k: v.detach().cpu() for k, v in bn_mod.state_dict().items() if 'running_' in k or 'num_batches' in k}
    if keep_optimizer:
        st = model.optimizer.state
        r['after'] = {n: (p.detach().cpu(), st[p]['exp_avg'].cpu(), st[p]['exp_avg_sq'].cpu()) for n, p in _named(model) if p in st}
    del model
    torch.cuda.empty_cache()
    return r


@pytest.fixture(scope="module")
def steps(dev):
    """(config, batch) -> the GPU step and the host oracle's float64 and float32 steps, each computed once."""
    cache = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(_threads())

    def get(case):
        if case not in cache:
            name, kind = case
            cfg = F.config(name)
            weights = F.make_weights(cfg, SEEDS[case])
            batch = F.make_batch('VSRN' if name == 'VSRN' else kind, SEEDS[case])
            gpu = _gpu_step(cfg, weights, batch, case in OPT_CASES)
            t0 = time.perf_counter()
            o64 = F.oracle_step(cfg, weights, batch, torch.float64)
            t1 = time.perf_counter()
            o32 = F.oracle_step(cfg, weights, batch, torch.float32)
            print("\n%s-%s: host oracle steps float64 %.1f s, float32 %.1f s (%d threads)" % (name, kind, t1 - t0, time.perf_counter() - t1,
                                                                                         torch.get_num_threads()))
            cache[case] = dict(cfg=cfg, weights=weights, gpu=gpu, o64=o64, o32=o32)
        return cache[case]
    yield get
    torch.set_num_threads(threads)


def _rel(x, ref, denom=None):
    d = float((x.double() - ref.double()).norm())
    return d / (denom if denom is not None else max(float(ref.double().norm()), 1e-300))


def _judge(case, rows):
    """rows: (what, err GPU, err host fp32).  Prints the worst ratios, then fails on every row over its bound, by name."""
    bound = lambda e32: K * e32 + FLOOR
    worst_bound = max(rows, key=lambda r: r[1] / bound(r[2]))
    worst_fp32 = max(rows, key=lambda r: r[1] / max(r[2], FLOOR / K))
    print("\n%s-%s: %d quantities; worst err / bound %.3f (%s: %.2e vs fp32 %.2e); worst err / max(err fp32, FLOOR/K) %.2f (%s)" % (
        case[0], case[1], len(rows), worst_bound[1] / bound(worst_bound[2]), worst_bound[0], worst_bound[1], worst_bound[2],
        worst_fp32[1] / max(worst_fp32[2], FLOOR / K), worst_fp32[0]))
    print("  absolute bound: %s" % [w for w, _, _ in rows if w.endswith(')')])
    bad = [(w, "err %.3e > bound %.3e (fp32 %.3e)" % (e, bound(e32), e32)) for w, e, e32 in rows if not e <= bound(e32)]
    assert not bad, "%s-%s: %s" % (case[0], case[1], bad)


@pytest.mark.parametrize("case", list(SEEDS), ids=["%s-%s" % c for c in SEEDS])
def test_train_emb_step_vs_float64(steps, case):
    r = steps(case)
    gpu, o64, o32 = r['gpu'], r['o64'], r['o32']
    S64 = o64['scores']
    # VSRN reads its captions' state after all 61 ids (the loader's layout): 40+ steps of padding wash the words out, and the 128
    # caption vectors coincide (float64: to 3e-10).  A row's hardest negative is then a tie between interchangeable captions: a flip
    # moves the row's gradient from one caption's tower to another's, identical to the same order.  That tie is checked, not skipped.
    ties = r['cfg']['name'] == 'VSRN'
    if ties:
        assert F.caption_spread(S64) <= 1e-8, F.caption_spread(S64)
    flip = F.flip_margin(S64, row_gaps=not ties)
    e_s, e_s32 = float((gpu['scores'] - S64).abs().max()), float((o32['scores'].double() - S64).abs().max())
    s_max = float(S64.abs().max())
    if e_s / s_max <= K * e_s32 / s_max + FLOOR:        # scores out of bounds are a finding of their own, reported with the rest below
        assert flip >= 10 * max(e_s, e_s32), "seed %d unsuitable for %s-%s: the hinge is %.2e from a discrete change, max|S_gpu - S64| = " \
            "%.2e, max|S_fp32 - S64| = %.2e" % (SEEDS[case], case[0], case[1], flip, e_s, e_s32)
    rows = [('scores', e_s / s_max, e_s32 / s_max),
            ('loss', abs(gpu['loss'] - o64['loss']) / abs(o64['loss']), abs(o32['loss'] - o64['loss']) / abs(o64['loss'])),
            ('grad_norm', abs(gpu['grad_norm'] - o64['grad_norm']) / o64['grad_norm'], abs(o32['grad_norm'] - o64['grad_norm']) / o64['grad_norm'])]
    assert set(gpu['terms']) == set(o64['terms'])
    for k, v64 in o64['terms'].items():
        rows.append((k, abs(gpu['terms'][k] - v64) / abs(v64), abs(o32['terms'][k] - v64) / abs(v64)))
    coef = min(1.0, r['cfg']['grad_clip'] / (gpu['grad_norm'] + 1e-6))
    assert set(gpu['grads']) == set(o64['grads'])
    big = max(float(g.norm()) for g in o64['grads'].values())
    for n, g64 in o64['grads'].items():
        g = gpu['grads'][n]
        g = torch.zeros_like(g64) if g is None else g.double() * coef
        if n in ZERO_GRAD:
            assert float(g64.norm()) <= 1e-12 * big, (n, float(g64.norm()), big)
            rows.append((n + ' (zero)', float(g.norm()) / big * FLOOR / ZERO_TOL, float(o32['grads'][n].double().norm()) / big * FLOOR / ZERO_TOL))
            continue
        denom = max(float(g64.norm()), TINY * big)
        rows.append((n if denom == float(g64.norm()) else n + ' (absolute)', _rel(g, g64, denom), _rel(o32['grads'][n], g64, denom)))
    if 'buffers' in gpu:
        model = r['cfg']['name']
        ws, prefix = r['weights'][BN_MODULE[model]], PREFIXES[model][BN_MODULE[model]]
        buffers = {k: v for k, v in ws.items() if 'running_' in k or 'num_batches' in k}
        want64, want32 = F.replay_bn(buffers, o64['bn_stats']), F.replay_bn(buffers, o32['bn_stats'])
        assert sorted(want64) == sorted(gpu['buffers'])
        for k, v in gpu['buffers'].items():
            if k.endswith('num_batches_tracked'):
                assert int(v) == want64[k], (k, int(v), want64[k])
                continue
            rows.append((prefix + k, _rel(v, want64[k]), _rel(want32[k], want64[k])))
        if model == 'VSRN':
            assert all(want64['Rs_GCN_%d.W.1.num_batches_tracked' % i] == 1 for i in (1, 2, 3, 4))
        else:
            assert want64['SAF_module.bn.num_batches_tracked' if r['cfg']['module_name'] == 'SAF' else
                          'v_global_w.embedding_global.1.num_batches_tracked'] == (F.BATCH if r['cfg']['module_name'] == 'SAF' else 1)
    _judge(case, rows)


def _adam(params0, grads, dtype, cfg):
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params0]
    for p, g in zip(ps, grads):
        p.grad = g.to(dtype).clone()
    torch.nn.utils.clip_grad_norm_(ps, cfg['grad_clip'])
    opt = torch.optim.Adam(ps, lr=cfg['learning_rate'])
    opt.step()
    return [(p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']) for p in ps]


@pytest.mark.parametrize("case", OPT_CASES, ids=["%s-%s" % c for c in OPT_CASES])
def test_clip_adam_full_size(steps, case):
    """The step's own ag.Adam (clip + Adam, multi-tensor) against clip_grad_norm_ + torch.optim.Adam in float64, both fed the GPU's
    fp32 gradients: the updates p1 - p0, m and v of every tensor."""
    r = steps(case)
    gpu, cfg = r['gpu'], r['cfg']
    p0 = {}
    for prefix, w in zip(PREFIXES.get(cfg['name'], ('img.', 'txt.')), r['weights']):
        p0.update({prefix + k: v for k, v in w.items()})
    names = list(gpu['after'])
    assert len(names) == len([g for g in gpu['grads'].values() if g is not None]) and len(names) >= 9
    grads = [gpu['grads'][n] for n in names]
    ref64 = _adam([p0[n] for n in names], grads, torch.float64, cfg)
    ref32 = _adam([p0[n] for n in names], grads, torch.float32, cfg)
    rows = []
    for i, n in enumerate(names):
        start = p0[n].double()
        (p1, m1, v1), (p64, m64, v64), (p32, m32, v32) = gpu['after'][n], ref64[i], ref32[i]
        rows.append((n + ' update', _rel(p1.double() - start, p64 - start), _rel(p32.double() - start, p64 - start)))
        rows.append((n + ' exp_avg', _rel(m1, m64), _rel(m32, m64)))
        rows.append((n + ' exp_avg_sq', _rel(v1, v64), _rel(v32, v64)))
    _judge(case + ('adam',), rows)
