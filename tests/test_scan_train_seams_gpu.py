"""GPU: the SCAN training similarity kernels (csrc/scan_train.hip, csrc/scan_train_i2t.hip, through ag.scan_t2i_scores and
ag.scan_i2t_scores) at every case of tests/helpers/scan_train_cases.py against the float64 oracle under autograd -- the WHOLE of S,
d_images and d_words.

Tolerance per compared tensor: 16 * max(e32_oracle, e32_mirror, 2^-24 max|want|) (tests/helpers/scan_train_cases.py;
tests/test_scan_train_case_table.py proves on the CPU that it is tight -- at most 2^-10 of the tensor's largest value -- and that it
sees a zeroed feature, a dropped region, a dropped word, a dropped caption's share of d_images and a dropped image's share of
d_words).  Every case also checks that d_words has exactly n_tok rows, that everything is finite, and that a second forward and
backward give the same bits (the kernels' headers promise disjoint writes and no atomics).  An unaligned case hands the library a
contiguous view one float into its buffer and asserts that the pointer is not 16-byte aligned.  The cases whose backward the library
rejects (more than 36 regions with a caption of more than 64 words, t2i) check the forward and the NotImplementedError.
profiles/scan_train_seams/measured.txt is the record of one run (ITR_SCAN_SEAMS_RECORD=<file> appends one line per case)."""
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import autograd as ag

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scan_train_cases as S        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_SCAN_SEAMS_RECORD")


def run(c, dev):
    """One forward and backward of the case on fresh device tensors -> {tensor: value}."""
    x = c.inputs()
    if c.unaligned:
        n = c.Bi * c.R * c.D
        buf = torch.zeros(n + 8, device=dev, dtype=torch.float32)
        img = buf[1:1 + n].view(c.Bi, c.R, c.D)
        img.copy_(x['images'])
        assert buf.data_ptr() % 16 == 0 and img.data_ptr() % 16 != 0 and img.is_contiguous()
    else:
        img = x['images'].to(dev)
        assert img.data_ptr() % 16 == 0
    img = img.detach().requires_grad_(True)
    assert img.data_ptr() % 16 == (4 if c.unaligned else 0)
    words = x['words'].to(dev).requires_grad_(True)
    gS = x['g_S'].to(dev)
    off = np.concatenate([[0], np.cumsum(c.lens)[:-1]]).astype(np.int64)
    fn = ag.scan_t2i_scores if c.xa == 't2i' else ag.scan_i2t_scores
    with torch.enable_grad():
        Sd = fn(img, words, off, list(c.lens), c.norm, c.agg, S.LAMBDA_LSE, S.LAMBDA_SOFTMAX)
        loss = (Sd * gS).sum()
    out = {'S': Sd.detach()}
    if not c.backward:
        with pytest.raises(NotImplementedError):
            loss.backward()
        return out
    loss.backward()
    out['d_images'], out['d_words'] = img.grad, words.grad
    return out


def check(c, dev):
    ref = c.reference()
    got, again = run(c, dev), run(c, dev)
    assert set(got) == set(ref), c
    ratios, fails = {}, []
    for name, (want, e_oracle, e_mirror, tol, _) in ref.items():
        val = got[name]
        if tuple(val.shape) != tuple(want.shape):
            fails.append("%s has shape %s, not %s" % (name, tuple(val.shape), tuple(want.shape)))
            continue
        if not bool(torch.isfinite(val).all()):
            fails.append("%s is not finite" % name)
        err = float(torch.nan_to_num((val.double().cpu() - want).abs(), nan=float('inf')).max())
        ratios[name] = err / tol
        print("%s %s: max err %.3e e32_oracle %.3e e32_mirror %.3e tol %.3e ratio %.3f" % (c.name, name, err, e_oracle, e_mirror, tol, err / tol))
        if not err <= tol:
            fails.append("%s: max err %.3e is %.3f x tol %.3e" % (name, err, err / tol, tol))
        if not torch.equal(val, again[name]):
            fails.append("%s: a second run gives other bits" % name)
    if c.backward and got['d_words'].shape[0] != c.n_tok:
        fails.append("d_words has %d rows, not %d" % (got['d_words'].shape[0], c.n_tok))
    if RECORD:
        tols = " ".join("%s: e32_oracle %.3e e32_mirror %.3e tol %.3e ratio %.3f" % ((k,) + ref[k][1:4] + (ratios.get(k, float('inf')),)) for k in ref)
        with open(RECORD, "a") as f:
            f.write("%s fwd %s bwd %s | %s | repeat %s\n" % (c.name, c.fwd_route, c.bwd_route, tols,
                                                           'DIFFERENT' if any('other bits' in m for m in fails) else 'equal'))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


@pytest.mark.parametrize("case", S.cases('t2i'), ids=lambda c: c.name)
def test_scan_t2i_train_seams_vs_float64(dev, case):
    check(case, dev)


@pytest.mark.parametrize("case", S.cases('i2t'), ids=lambda c: c.name)
def test_scan_i2t_train_seams_vs_float64(dev, case):
    check(case, dev)
