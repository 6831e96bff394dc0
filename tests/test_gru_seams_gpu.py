"""GPU: the text GRU kernels at every case of tests/helpers/gru_cases.py against the float64 reference -- the training path
(csrc/gru_train.hip through ag.gru_sequence: the WHOLE of out, d_embed and every weight and bias gradient of sum(out * g_out)) and the
evaluation path (csrc/towers.hip through ops.gru_encode: EVERY row of the sequence output and of the last state, in the default and
the batch-invariant form).

Tolerance per compared tensor: 16 * max(e32, 2^-24 max|want|) (tests/helpers/gru_cases.py; tests/test_gru_case_table.py proves on the
CPU that it is tight -- at most 2^-12 of the tensor's largest value -- and that it sees a hidden unit or a K slice left out of the
recurrence product, forward or backward, a caption that keeps its old state, a carry lost where the prefix grows, a token row lost
from d_embed and a missing reverse direction).  Every training case also checks that out has exactly n_tok rows, that everything is
finite, and that a second forward and backward on fresh tensors give the same bits (the header of gru_train.hip promises a fixed
summation order; the bi cases run the reverse direction on the side stream).  profiles/gru_seams/measured.txt is the record of one
run (ITR_GRU_SEAMS_RECORD=<file> appends one line per case and test)."""
import os
import sys

import pytest
import torch

from itr_amd import autograd as ag
from itr_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gru_cases as G        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_GRU_SEAMS_RECORD")


def _routes(c):
    return "fwd %s bwd %s" % ("+".join(sorted(c.fwd_routes)), "+".join(sorted(c.bwd_routes)) or "none")


def _compare(c, ref, got, again=None):
    """-> ({tensor: err / tol}, [failure])."""
    ratios, fails = {}, []
    for name, val in got.items():
        want, e32, _, tol = ref[name.split('@')[0]]
        if tuple(val.shape) != tuple(want.shape):
            fails.append("%s has shape %s, not %s" % (name, tuple(val.shape), tuple(want.shape)))
            continue
        if not bool(torch.isfinite(val).all()):
            fails.append("%s is not finite" % name)
        err = float(torch.nan_to_num((val.double().cpu() - want).abs(), nan=float('inf')).max())
        ratios[name] = err / tol if tol > 0 else (0.0 if err == 0 else float('inf'))
        print("%s %s: max err %.3e e32 %.3e tol %.3e ratio %.3f" % (c.name, name, err, e32, tol, ratios[name]))
        if not err <= tol:
            fails.append("%s: max err %.3e is %.3f x tol %.3e" % (name, err, ratios[name], tol))
        if again is not None and not torch.equal(val, again[name]):
            fails.append("%s: a second run gives other bits" % name)
    return ratios, fails


def _record(c, what, ref, ratios, tail):
    if RECORD:
        cols = " ".join("%s: e32 %.3e tol %.3e ratio %.3f" % (k, ref[k.split('@')[0]][1], ref[k.split('@')[0]][3], r) for k, r in ratios.items())
        with open(RECORD, "a") as f:
            f.write("%s %s %s %s | %s | %s\n" % (what, c.name, _routes(c), 'fallback' if c.name in G.FALLBACK else 'primary', cols, tail))


def _device_inputs(c, dev):
    x = c.inputs()
    tokens = x['tokens'].to(dev)
    off = torch.tensor(c.off, dtype=torch.int64, device=dev)
    return x, tokens, off


def train(c, dev):
    """One forward and backward of the case on fresh device tensors -> {tensor: value}."""
    x, tokens, off = _device_inputs(c, dev)
    embed = x['embed'].to(dev).requires_grad_(True)
    w = {n: x[n].to(dev).requires_grad_(True) for n in c.weight_names}
    with torch.enable_grad():
        out = ag.gru_sequence(tokens, off, list(c.lens), embed, w, c.bi)
        loss = (out * x['g_out'].to(dev)).sum()
    loss.backward()
    res = {'out': out.detach(), 'd_embed': embed.grad}
    for n in c.weight_names:
        res['d_' + n] = w[n].grad
    return res


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_gru_train_seams_vs_float64(dev, case):
    c, ref = case, case.reference()
    got, again = train(c, dev), train(c, dev)
    assert set(got) == set(c.tensors), c
    ratios, fails = _compare(c, ref, got, again)
    if got['out'].shape[0] != c.n_tok:
        fails.append("out has %d rows, not %d" % (got['out'].shape[0], c.n_tok))
    _record(c, "train", ref, ratios, "repeat %s" % ('DIFFERENT' if any('other bits' in m for m in fails) else 'equal'))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_gru_eval_seams_vs_float64(dev, case):
    c, ref = case, case.reference()
    x, tokens, off = _device_inputs(c, dev)
    weights = {'embed.weight': x['embed'].to(dev)}
    weights.update({'rnn.' + n: x[n].to(dev) for n in c.weight_names})
    got = {}
    for inv in (False, True):
        for last in (False, True):
            name = ('last' if last else 'out') + ('@batch_invariant' if inv else '@default')
            got[name] = ops.gru_encode(tokens, off, list(c.lens), weights, c.bi, no_txtnorm=True, gather_last=last, batch_invariant=inv)
    ratios, fails = _compare(c, ref, got)
    _record(c, "eval", ref, ratios, "input projection %s" % c.eval_projection)
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))
