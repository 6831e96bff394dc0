"""GPU: every small kernel behind itr_amd/autograd.py (csrc/train.hip, train_bert.hip, train_camera.hip, train_vsrn.hip) swept over
the edges of its launch geometry -- 256-thread workgroups, waves of 64, four rows per workgroup, BatchNorm's 64-column blocks and row
slices, float4 paths, grid-stride loops, the optimizer's block tables -- forward and backward, against the same operation written
with plain torch ops in float64 (tests/helpers/train_prim_cases.py).

Bound of every compared tensor: 16 * max(e32, 2^-24 * max|want|), e32 = the error of the float64 reference's own float32 run on
the CPU; exact ops (transpose, relu + max-pool, group max, row gather, dropout) are compared bit for bit.  No bound is taken from
what the kernels give; tests/test_train_primitive_cases.py proves on the CPU that each bound sees one dropped element.

ITR_TRAIN_PRIM_REPORT=<file> writes (case, tensor, err, e32, tol, rule) of everything compared (a module finaliser
writes it); one run is kept as profiles/train_primitives/measured.txt.  Worst err / tol per op family in that run:
    flat elementwise 0.12    column kernels 0.22    wave per row 0.22    log-softmax / NLL 0.72    BatchNorm 0.29
    summarize 0.11    attention 0.07    batched products 0.17    rows and columns 0.15    optimizer 0.07
The sweep's one finding: the Adam kernels formed 1 - beta2 as 1.f - 0.999f = 0.99998713e-3, so every element of exp_avg_sq was a
relative 1.3e-5 off torch's (err / tol 17 in test_adam_with_clipping); csrc/train.hip now takes 1 - beta and the bias corrections
from the decimal the float beta stands for, as torch does from its double.  (The embedding scatter behind gather_rows' backward adds a
token's rows in row order, without atomics, so that a training step can be replayed bit for bit:
test_embedding_scatter_repeats_bit_for_bit; 161 us at 7808 tokens x 300 columns, 32 us at 1527, 106 us for a 7808-row permutation
of 1024 columns on the MI355X.)
"""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import train_prim_cases as T        # noqa: E402

from itr_amd import autograd as ag      # noqa: E402

pytestmark = pytest.mark.gpu

RECORD = []          # (family, case, tensor, err, e32, tol, rule)


def _bits(t):
    return (t.float() + 0.0).contiguous().view(torch.int32)


def _compare(family, label, name, got, want, e32, tol, rule):
    got = got.detach().cpu()
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    err = float((got.double() - want).abs().max()) if want.numel() else 0.0
    ok = bool((_bits(got) == _bits(want)).all()) if rule == 'exact' else err <= tol
    RECORD.append((family, label, name, err, e32, tol, rule))
    print("%-44s %-14s err %.3e  e32 %.3e  tol %.3e  %s%s" % (label, name, err, e32, tol, rule, "" if ok else "   <-- MISS"))
    return ok


def _dev_inputs(case, dev):
    x = {}
    for k, v in case.inputs().items():
        if torch.is_tensor(v):
            v = v.to(dev)
            if k in case.grads:
                v.requires_grad_(True)
        x[k] = v
    return x


def _sweep(family, case, dev, run):
    x = _dev_inputs(case, dev)
    out = run(case, x)
    got = {k: v for k, v in out.items()}
    if case.grads:
        loss = sum((out[k] * x['g_' + k]).sum() for k in out if out[k].requires_grad)
        for k, g in zip(case.grads, torch.autograd.grad(loss, [x[k] for k in case.grads])):
            got['d_' + k] = g
    ref = case.reference()
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    misses = []
    for name in sorted(ref):
        want, e32, tol, rule = ref[name]
        assert torch.isfinite(got[name]).all(), (case, name)
        if not _compare(family, case.name, name, case.mask(name, got[name].detach()), want, e32, tol, rule):
            misses.append(name)
    assert not misses, "%s: %s outside the bound" % (case, misses)


def _param(*ops):
    return pytest.mark.parametrize("case", T.cases(*ops), ids=repr)


# ---------------------------------------------------------------------------------------------------------------------
def _run_gru(case, x):
    rnn = types.SimpleNamespace(weight_ih_l0=x['w_ih'], weight_hh_l0=x['w_hh'], bias_ih_l0=x['b_ih'], bias_hh_l0=x['b_hh'])
    return {'hn': ag.gru_cell(x['x'], x['h'], rnn)}


_FLAT = {
    'mul': lambda c, x: {'y': ag.mul(x['a'], x['b'])},
    'act': lambda c, x: {'y': ag.act(x['x'], c.extra)},
    'gelu': lambda c, x: {'y': ag.gelu(x['x'])},
    'gate_apply': lambda c, x: dict(zip(('qo', 'ko'), ag.gate_apply(x['q'], x['k'], x['M']))),
    'gru_cell': _run_gru,
}


@_param(*_FLAT)
def test_flat_elementwise(case, dev):
    _sweep('flat elementwise', case, dev, _FLAT[case.op])


_COL = {
    'add_bcast_mid_act': lambda c, x: {'y': ag.add_bcast_mid_act(x['x'], x['v'], c.extra)},
    'l2norm_mid': lambda c, x: {'z': ag.l2norm_mid(x['x'])},
    'relu_maxpool': lambda c, x: {'y': ag.relu_maxpool(x['x'])},
    'mean_mid': lambda c, x: {'y': ag.mean_mid(x['x'])},
    'group_max': lambda c, x: {'S': ag._GroupMax.apply(x['T'], c.extra)},
    'mvm_scores': lambda c, x: {'S': ag.mvm_scores(x['img'], x['cap'])},
}


@_param(*_COL)
def test_thread_per_column(case, dev):
    _sweep('column kernels', case, dev, _COL[case.op])


_ROW = {
    'add_layernorm': lambda c, x: {'y': ag.add_layernorm(x['x'], x.get('res'), x['gamma'], x['beta'], 1e-12)},
    'addattn_score': lambda c, x: {'e': ag.addattn_score(x['x'], x['v'], x['w'])},
    'l2norm_rows': lambda c, x: {'z': ag.l2norm_rows(x['x'])},
}


@_param(*_ROW)
def test_wave_per_row(case, dev):
    _sweep('wave per row', case, dev, _ROW[case.op])


@_param('nll_logsoftmax')
def test_nll_logsoftmax(case, dev):
    _sweep('log-softmax / NLL', case, dev, lambda c, x: {'loss': ag.nll_logsoftmax(x['logits'], x['target'], x['mask'])})


def _run_bn(case, x):
    bn = types.SimpleNamespace(weight=x['gamma'], bias=x['beta'], eps=T.BN_EPS, momentum=T.BN_MOM, running_mean=x['rm'].clone(),
                               running_var=x['rv'].clone(), num_batches_tracked=torch.zeros((), dtype=torch.int64, device=x['x'].device))
    y = ag.batch_norm_train(x['x'], bn)
    assert int(bn.num_batches_tracked) == 1
    return {'y': y, 'running_mean': bn.running_mean, 'running_var': bn.running_var}


@_param('batch_norm_train')
def test_batch_norm_train(case, dev):
    _sweep('BatchNorm', case, dev, _run_bn)


@_param('summarize')
def test_summarize(case, dev):
    _sweep('summarize', case, dev, lambda c, x: {'out': ag.summarize(x['smry'], x['x'])})


@pytest.mark.parametrize("R,K", [(T.SMRY_LIMIT + 1, 4), (4, T.SMRY_LIMIT + 1)])
def test_summarize_refuses_more_than_its_limit(R, K, dev):
    with pytest.raises((ValueError, NotImplementedError)):
        ag.summarize(torch.zeros(1, R, K, device=dev), torch.zeros(1, R, 8, device=dev))


@_param('mha')
def test_mha(case, dev):
    B, L, heads, dk = case.extra
    _sweep('attention', case, dev, lambda c, x: {'out': ag.mha(x['qkv'], x.get('mask'), B, L, heads, 0.0, 0)})


@pytest.mark.parametrize("L,dk", [(T.MHA_LIMIT + 1, 4), (4, T.MHA_LIMIT + 1)])
def test_mha_refuses_more_than_its_limit(L, dk, dev):
    with pytest.raises((ValueError, NotImplementedError)):
        ag.mha(torch.zeros(L, 3 * dk, device=dev), None, 1, L, 1, 0.0, 0)


@_param('bmm_nn', 'bmm_nt')
def test_small_batched_products(case, dev):
    fn = ag.bmm_nt if case.op == 'bmm_nt' else ag.bmm_nn
    _sweep('batched products', case, dev, lambda c, x: {'C': fn(x['A'], x['B'])})


_RC = {
    'transpose2d': lambda c, x: {'y': ag.transpose2d(x['x'])},
    'colsum': lambda c, x: {'y': ag.colsum(x['x'], out=x['out0'].clone(), accumulate=True) if 'out0' in x else ag.colsum(x['x'])},
    'gather_rows': lambda c, x: {'y': ag.gather_rows(x['x'], x['idx'])},
}


@_param(*_RC)
def test_rows_and_columns(case, dev):
    _sweep('rows and columns', case, dev, _RC[case.op])


@_param('gather_rows')
def test_embedding_scatter_repeats_bit_for_bit(case, dev):
    """The backward of gather_rows (the embedding scatter) adds the rows of an index in row order: three runs on the same inputs -- one
    row is the sum of 400 -- give the same bits."""
    x = _dev_inputs(case, dev)
    runs = []
    for _ in range(3):
        y = ag.gather_rows(x['x'], x['idx'])
        runs.append(torch.autograd.grad((y * x['g_y']).sum(), x['x'])[0])
    assert (_bits(runs[0].cpu()) == _bits(runs[1].cpu())).all() and (_bits(runs[0].cpu()) == _bits(runs[2].cpu())).all()


# ---------------------------------------------------------------------------------------------------------------------
def test_adam_with_clipping(dev):
    """ag.Adam.step(max_norm) == clip_grad_norm_ + torch.optim.Adam in float64 over three steps: every parameter tensor, both of its
    moment buffers, and the gradient norm, each under its own bound; the set of tensors with a gradient changes after the first step
    (the block tables are rebuilt).  tests/test_train_primitive_cases.py shows that an update skipped for a tensor's last element
    moves all three by at least 10 x these bounds."""
    params, grads = T.adam_problem()
    w64, w32 = T.adam_reference(torch.float64), T.adam_reference(torch.float32)
    ps = [torch.nn.Parameter(p.to(dev)) for p in params]
    opt = ag.Adam(ps, lr=T.ADAM_LR)
    misses = []
    for s, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(dev)
        opt.step(max_norm=T.ADAM_MAX_NORM)
        zeros = [torch.zeros_like(p.data) for p in ps]
        got = ([p.data for p in ps], [opt.state[p]['exp_avg'] if p in opt.state else z for p, z in zip(ps, zeros)],
               [opt.state[p]['exp_avg_sq'] if p in opt.state else z for p, z in zip(ps, zeros)])
        for kind, gt, a, b in zip(('param', 'exp_avg', 'exp_avg_sq'), got, w64[s], w32[s]):
            for i, (g_, a_, b_) in enumerate(zip(gt, a, b)):
                e32, tol = T.tolerance(a_, b_)
                if not _compare('optimizer', 'adam-step%d-tensor%d-n%d' % (s + 1, i, a_.numel()), kind, g_, a_, e32, tol, 'primary'):
                    misses.append((s + 1, kind, i))
        e32, tol = T.tolerance(w64[s][3], w32[s][3])
        if not _compare('optimizer', 'adam-step%d' % (s + 1), 'grad_norm', opt.last_grad_norm, w64[s][3], e32, tol, 'primary'):
            misses.append((s + 1, 'grad_norm'))
    assert not misses, misses


def _inv_keep(p):
    one = torch.ones((), dtype=torch.float32)
    return one / (one - torch.tensor(p, dtype=torch.float32))


@pytest.mark.parametrize("p", T.DROPOUT_P)
@pytest.mark.parametrize("n", T.DROPOUT_N)
def test_dropout_is_exact(n, p, dev):
    """Every output is 0 or bit-equal to x * (1 / (1 - p)) in float32; the backward of dy = 1 is the same mask times the same scale
    (== y / x bit for bit where that quotient is exact: inputs that are powers of two); the same seed gives the same bits."""
    g = torch.Generator().manual_seed(1000 * n + int(100 * p))
    s = _inv_keep(p)
    pow2 = torch.pow(2.0, torch.randint(-3, 4, (n,), generator=g).float()) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    for x in (torch.randn(n, generator=g), pow2):
        seeds = ag.DropoutSeeds()
        torch.manual_seed(n)
        seeds.new_step()
        gx = x.to(dev).requires_grad_(True)
        y = ag.dropout(gx, p, seeds)
        y.backward(torch.ones_like(y))
        yc, dx = y.detach().cpu(), gx.grad.cpu()
        kept = yc != 0
        assert (_bits(yc) == _bits(torch.where(kept, x * s, torch.zeros_like(x)))).all()
        assert (_bits(dx) == _bits(torch.where(kept, s, torch.zeros(())).expand_as(dx))).all()
        if x is pow2:
            assert (_bits(dx) == _bits(yc / x)).all()
        seeds2 = ag.DropoutSeeds()
        torch.manual_seed(n)
        seeds2.new_step()
        assert (_bits(ag.dropout(x.to(dev), p, seeds2).cpu()) == _bits(yc)).all()
    RECORD.append(('flat elementwise', 'dropout-n%d-p%s' % (n, p), 'y, dx', 0.0, 0.0, 0.0, 'exact'))


@pytest.mark.parametrize("p", T.DROPOUT_P)
def test_dropout_sites_of_one_step_differ(p, dev):
    n = T.DROPOUT_N[-1]
    x = torch.ones(n, device=dev)
    seeds = ag.DropoutSeeds()
    torch.manual_seed(3)
    seeds.new_step()
    a, b = ag.dropout(x, p, seeds), ag.dropout(x, p, seeds)
    assert not torch.equal(a, b)
    for y in (a, b):            # both sites drop about p of the elements: within 5 sigma of a binomial
        dropped = float((y == 0).sum())
        assert abs(dropped - n * p) <= 5.0 * (n * p * (1 - p)) ** 0.5


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's last test: the table of everything compared, when ITR_TRAIN_PRIM_REPORT names a file."""
    yield
    path = os.environ.get("ITR_TRAIN_PRIM_REPORT")
    if not path or not RECORD:
        return
    worst = {}
    with open(path, "w") as f:
        f.write("# family | case | tensor | err | e32 | tol | rule\n")
        for fam, case, name, err, e32, tol, rule in RECORD:
            f.write("%s | %s | %s | %.3e | %.3e | %.3e | %s\n" % (fam, case, name, err, e32, tol, rule))
            if tol > 0:
                worst[fam] = max(worst.get(fam, 0.0), err / tol)
        f.write("# worst err / tol per family\n")
        for fam in sorted(worst):
            f.write("# %-20s %.3f\n" % (fam, worst[fam]))
