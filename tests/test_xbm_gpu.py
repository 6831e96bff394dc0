"""GPU: the losses on batch u memory (csrc/xbm_loss.hip: itr_xbm_*; ops.xbm_hinge_loss / ops.xbm_infonce_loss) and the memory itself
(itr_amd/membank.py) against the float64 helper (tests/helpers/xbm_oracle.py) over the helper's case table: 17 (B, n) pairs on the
seams the helper names, the hinge in both forms and InfoNCE at two amplitudes, each with the in-batch mask on and off.

Tolerance of the loss, the log-sum-exps and the InfoNCE gradients: the primary rule of tests/helpers/train_prim_cases.py,
FACTOR * max(e32, U * max|want|), e32 the float32 helper's own error.  The hinge's gradients are small integer multiples of the
upstream gradient and every case keeps each hinge decision further than fp32 rounding from a flip (tests/test_xbm_cpu.py), so they
are compared exactly."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import autograd as ag
from itr_amd import ops
from itr_amd.membank import MemoryBank

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hinge_groups_oracle as HG  # noqa: E402
import xbm_oracle as X  # noqa: E402

pytestmark = pytest.mark.gpu

T = X.TEMPERATURE
IDS = [X.case_id(*c) for c in X.SWEEP]


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def loss_fn(kind, s, r, c, groups, bank_groups, mask_batch):
    if kind == "infonce":
        return ops.xbm_infonce_loss(s, r, c, groups, bank_groups, T, mask_batch=mask_batch)
    return ops.xbm_hinge_loss(s, r, c, groups, bank_groups, X.MARGIN, kind == "hinge_max", mask_batch=mask_batch)


def run(kind, ref, mask_batch, dev, upstream=X.UPSTREAM):
    s, r, c = (ref[k].to(dev).requires_grad_(True) for k in ("S", "R", "C"))
    loss = loss_fn(kind, s, r, c, ref["groups"], ref["bank_groups"], mask_batch)
    (loss * upstream).backward()
    return loss.detach(), s.grad, r.grad, c.grad


def dropped(ref, mask_batch):
    return [~k for k in X.kept(ref["groups"], ref["bank_groups"], mask_batch)]


@pytest.mark.parametrize("B,n,kind,amp,mask_batch", X.SWEEP, ids=IDS)
def test_sweep_vs_float64(dev, B, n, kind, amp, mask_batch):
    ref = X.reference(B, n, kind, amp, mask_batch)
    got = dict(zip(("loss", "dS", "dR", "dC"), run(kind, ref, mask_batch, dev)))
    assert got["loss"].dtype == torch.float32 and got["loss"].dim() == 0
    assert got["dS"].shape == (B, B) and got["dR"].shape == (B, n) and got["dC"].shape == (n, B)
    failures = []
    for name in ("loss", "dS", "dR", "dC"):
        want, e32, tol = ref[name]
        g = got[name].cpu().double()
        err = float((g - want).abs().max())
        print("\n%s %s: got %.9g want %.9g (max|want| %.6g) err %.3g e32 %.3g tol %.3g" % (
            X.case_id(B, n, kind, amp, mask_batch), name, float(g.reshape(-1)[0]), float(want.reshape(-1)[0]), float(want.abs().max()), err, e32, tol))
        if name != "loss" and kind != "infonce":
            if not torch.equal(got[name].cpu(), want.float()):          # exactly float32(3 * d64)
                failures.append((name, "not exact", err))
        elif not (torch.isfinite(g).all() and err <= tol):
            failures.append((name, err, tol))
    assert not failures, failures
    for name, off in zip(("dS", "dR", "dC"), dropped(ref, mask_batch)):
        assert torch.equal(bits(got[name])[off], torch.zeros(int(off.sum()), dtype=torch.int32)), name          # bit-zero, not -0.0
    if B >= 2 and n >= 2:
        assert all(int(off.sum()) >= 2 for off in dropped(ref, True))


@pytest.mark.parametrize("B,n", [(2, 63), (65, 255), (128, 4099), (257, 1000)])
@pytest.mark.parametrize("mask_batch", [False, True])
def test_saved_vectors(dev, B, n, mask_batch):
    """row_lse / col_lse, the max form's arg vectors and the sum form's violator counts are the helper's"""
    ref = X.reference(B, n, "infonce", 30.0, mask_batch)
    S, R, C = (ref[k].to(dev) for k in ("S", "R", "C"))
    _, rl, cl = ops.xbm_infonce_fwd(S, R, C, ref["groups"], ref["bank_groups"], T, mask_batch)
    _, w_rl, w_cl = X.infonce_parts(ref["S"], ref["R"], ref["C"], ref["groups"], ref["bank_groups"], X.scale_of(T), mask_batch)
    _, f_rl, f_cl = X.infonce_parts(ref["S"], ref["R"], ref["C"], ref["groups"], ref["bank_groups"], X.scale_of(T), mask_batch, torch.float32)
    for got, want, w32 in ((rl, w_rl, f_rl), (cl, w_cl, f_cl)):
        tol = X.FACTOR * max(float((w32.double() - want).abs().max()), X.U * float(want.abs().max()))
        assert float((got.cpu().double() - want).abs().max()) <= tol
    ref = X.reference(B, n, "hinge_max", 1.0, mask_batch)
    S, R, C = (ref[k].to(dev) for k in ("S", "R", "C"))
    _, ra, ca = ops.xbm_hinge_fwd(S, R, C, ref["groups"], ref["bank_groups"], X.MARGIN, True, mask_batch)
    w_ra, w_ca = X.hinge_args(ref["S"], ref["R"], ref["C"], ref["groups"], ref["bank_groups"], X.MARGIN, mask_batch)
    assert HG.args_agree(ra, w_ra) and HG.args_agree(ca, w_ca)
    assert int(ra.min()) >= 0 and int(ra.max()) < B + n and int(ca.min()) >= 0 and int(ca.max()) < B + n
    ref = X.reference(B, n, "hinge_sum", 1.0, mask_batch)
    S, R, C = (ref[k].to(dev) for k in ("S", "R", "C"))
    _, rc, cc = ops.xbm_hinge_fwd(S, R, C, ref["groups"], ref["bank_groups"], X.MARGIN, False, mask_batch)
    w_rc, w_cc = X.hinge_counts(ref["S"], ref["R"], ref["C"], ref["groups"], ref["bank_groups"], X.MARGIN, mask_batch)
    assert torch.equal(rc.cpu().long(), w_rc) and torch.equal(cc.cpu().long(), w_cc)


@pytest.mark.parametrize("B,n,kind,amp", [(1, 1, "hinge_max", 1.0), (65, 255, "hinge_sum", 1.0), (128, 4099, "hinge_max", 1.0),
                                           (128, 4099, "infonce", 30.0), (257, 1000, "infonce", 1.0)])
def test_same_bits_run_to_run(dev, B, n, kind, amp):
    ref = X.reference(B, n, kind, amp, True)
    a, b = run(kind, ref, True, dev), run(kind, ref, True, dev)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [1, 65, 128])
@pytest.mark.parametrize("mask_batch", [False, True])
def test_empty_memory_has_the_bits_of_the_in_batch_ops(dev, B, mask_batch):
    ref = X.reference(B, {1: 1, 65: 63, 128: 64}[B], "hinge_max", 1.0, mask_batch)          # S and the groups of a case of the table
    S, groups = ref["S"], ref["groups"]
    R, C, none = torch.zeros(B, 0), torch.zeros(0, B), np.zeros(0, dtype=np.int64)
    for kind in ("hinge_sum", "hinge_max", "infonce"):
        s, r, c = (t.to(dev).requires_grad_(True) for t in (S, R, C))
        loss = loss_fn(kind, s, r, c, groups, none, mask_batch)
        (loss * X.UPSTREAM).backward()
        s2 = S.to(dev).requires_grad_(True)
        g2 = groups if mask_batch else None
        loss2 = ops.infonce_loss(s2, T, groups=g2) if kind == "infonce" else ops.hinge_loss(s2, X.MARGIN, kind == "hinge_max", groups=g2)
        (loss2 * X.UPSTREAM).backward()
        assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(s.grad), bits(s2.grad)), kind


@pytest.mark.parametrize("kind,amp", X.KINDS)
@pytest.mark.parametrize("mask_batch", [False, True])
def test_a_memory_of_the_queries_own_images_changes_nothing(dev, kind, amp, mask_batch):
    """all groups equal: every memory entry is dropped, the loss is the in-batch loss of S alone and dR, dC are all zero"""
    ref = X.reference(65, 255, kind, amp, mask_batch)
    B, n = 65, 255
    one = np.full(B, 7, dtype=np.int64)
    case = dict(ref, groups=one, bank_groups=np.full(n, 7, dtype=np.int64))
    loss, dS, dR, dC = run(kind, case, False, dev)
    none = np.zeros(0, dtype=np.int64)
    w64 = X.loss_and_grads(kind, ref["S"], ref["R"][:, :0], ref["C"][:0], one, none, False, torch.float64)
    w32 = X.loss_and_grads(kind, ref["S"], ref["R"][:, :0], ref["C"][:0], one, none, False, torch.float32)
    for got, a, b in ((loss, w64[0], w32[0]), (dS, w64[1], w32[1])):
        tol = X.FACTOR * max(float((b.double() - a).abs().max()), X.U * float(a.abs().max()))
        assert float((got.cpu().double() - a).abs().max()) <= tol
    assert not bits(dR).any() and not bits(dC).any()
    if mask_batch:          # ... and with the in-batch mask on nothing at all is left
        loss, dS, dR, dC = run(kind, case, True, dev)
        assert float(loss) == 0.0 and float(dS.abs().max()) == 0.0 and not bits(dR).any() and not bits(dC).any()


def test_ties(dev):
    """equal scores in S and R: the in-batch candidate wins; equal scores in two slots: the lower slot wins"""
    S = torch.tensor([[0.5, 0.7], [0.1, 0.6]])
    R = torch.tensor([[0.7, 0.9, 0.9], [0.2, 0.3, 0.3]])
    C = torch.tensor([[0.1, 0.2], [0.1, 0.9], [0.1, 0.9]])
    for Rk, Ck, bank, row0, col1 in ((R, C, [3, 4, 5], 3, 3), (R[:, :1].contiguous(), C[:1], [3], 1, 0)):
        s, r, c = (t.to(dev).requires_grad_(True) for t in (S, Rk, Ck))
        _, ra, ca = ops.xbm_hinge_fwd(s.detach(), r.detach(), c.detach(), [1, 2], bank, X.MARGIN, True)
        assert int(ra[0]) == row0 and int(ca[1]) == col1
        w_ra, w_ca = X.hinge_args(S, Rk, Ck, [1, 2], bank)
        assert HG.args_agree(ra, w_ra) and HG.args_agree(ca, w_ca)
        ops.xbm_hinge_loss(s, r, c, [1, 2], bank, X.MARGIN, True).backward()
        want = X.loss_and_grads("hinge_max", S, Rk, Ck, [1, 2], bank, False, upstream=1.0)
        for got, w in zip((s.grad, r.grad, c.grad), want[1:]):
            assert torch.equal(got.cpu(), w.float())
        assert int((r.grad != 0).sum(1).max()) <= 1 and int((c.grad != 0).sum(0).max()) <= 1


@pytest.mark.parametrize("max_violation", [False, True])
def test_backward_checks_the_mask_again(dev, max_violation):
    """the arg vectors of an UNMASKED forward (all groups distinct) name entries that the groups of the backward drop"""
    ref = X.reference(65, 255, "hinge_max" if max_violation else "hinge_sum", 1.0, True)
    B, n = 65, 255
    S, R, C = (ref[k].to(dev) for k in ("S", "R", "C"))
    _, ra, ca = ops.xbm_hinge_fwd(S, R, C, np.arange(B), 1000 + np.arange(n), X.MARGIN, max_violation, False)
    g = torch.full((1,), X.UPSTREAM, device=dev)
    # a batch whose hardest negatives all share the query's image
    groups = np.arange(B)
    bank_groups = 1000 + np.arange(n)
    hard_r, hard_c = ra.cpu().numpy(), ca.cpu().numpy()
    if max_violation:
        for i in range(0, B, 2):
            if hard_r[i] >= B:
                bank_groups[hard_r[i] - B] = groups[i]
    else:
        bank_groups[::3] = groups[np.arange(len(bank_groups[::3])) % B]
    dS, dR, dC = ops.xbm_hinge_bwd(S, R, C, groups, bank_groups, X.MARGIN, max_violation, ra, ca, g, True)
    off_s, off_r, off_c = [~k for k in X.kept(groups, bank_groups, True)]
    assert int(off_r.sum()) >= 2
    for got, off in ((dS, off_s), (dR, off_r), (dC, off_c)):
        assert torch.equal(bits(got)[off], torch.zeros(int(off.sum()), dtype=torch.int32))


def test_ring(dev):
    """M = 10, pushes of 4, 4, 4, 3 rows against a host deque"""
    M, D = 10, 6
    bank = MemoryBank(M, dev)
    with pytest.raises(ValueError):
        bank.view()
    slots = [None] * M
    head, at = 0, 0
    rng = np.random.RandomState(3)
    fifo = collections.deque(maxlen=M)
    for count in (4, 4, 4, 3):
        img = torch.from_numpy(rng.randn(count, 2, D).astype(np.float32))
        cap = torch.from_numpy(rng.randn(count, D).astype(np.float32))
        groups = rng.randint(0, 1000, size=count)
        bank.push(img.to(dev).requires_grad_(True), cap.to(dev), groups)
        for r in range(count):
            slots[(head + r) % M] = (img[r], cap[r], int(groups[r]))
            fifo.append(int(groups[r]))
        head, at = (head + count) % M, at + count
        n = min(at, M)
        v_img, v_cap, v_group = bank.view()
        assert len(bank) == n and v_img.shape == (n, 2, D) and v_cap.shape == (n, D) and v_group.dtype == torch.int32
        assert not v_img.requires_grad
        assert torch.equal(v_img.cpu(), torch.stack([s[0] for s in slots[:n]]))
        assert torch.equal(v_cap.cpu(), torch.stack([s[1] for s in slots[:n]]))
        assert v_group.cpu().tolist() == [s[2] for s in slots[:n]]
        assert sorted(v_group.cpu().tolist()) == sorted(fifo)          # the last min(pushed, M) rows, whatever their slots
    with pytest.raises(ValueError, match="do not fit"):
        bank.push(torch.zeros(M + 1, 2, D, device=dev), torch.zeros(M + 1, D, device=dev), np.zeros(M + 1, dtype=np.int64))
    bank.reset()
    assert len(bank) == 0 and bank.view()[0].shape[0] == 0


@pytest.mark.parametrize("measure", ["cosine", "order"])
@pytest.mark.parametrize("kind", ["hinge_max", "infonce"])
def test_embedding_gradients_through_the_three_matrices(dev, measure, kind):
    """d loss / d img and d cap through S = pair(img, cap), R = pair(img, memory captions), C = pair(memory images, cap); the
    memory carries no gradient"""
    B, n, D = 12, 20, 32
    rng = np.random.RandomState(5)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    img, cap, b_img, b_cap = (torch.from_numpy(unit(rng.randn(k, D)).astype(np.float32)) for k in (B, B, n, n))
    groups = rng.randint(0, 8, size=B)
    bank_groups = rng.randint(0, 16, size=n)
    pair = ag.order_scores if measure == "order" else ag.cosine_scores

    def pair_ref(a, b):
        if measure == "cosine":
            return a @ b.t()
        return -(b[None, :, :] - a[:, None, :]).clamp(min=0).pow(2).sum(2).sqrt()

    grads = {}
    for dtype in (torch.float64, torch.float32):
        a, b = img.clone().to(dtype).requires_grad_(True), cap.clone().to(dtype).requires_grad_(True)
        loss = X.loss_of(kind, pair_ref(a, b), pair_ref(a, b_cap.to(dtype)), pair_ref(b_img.to(dtype), b), groups, bank_groups, True, dtype)
        (loss * X.UPSTREAM).backward()
        grads[dtype] = (loss.detach(), a.grad, b.grad)
    a, b = img.to(dev).requires_grad_(True), cap.to(dev).requires_grad_(True)
    mem_img, mem_cap = b_img.to(dev), b_cap.to(dev)
    loss = loss_fn(kind, pair(a, b), pair(a, mem_cap), pair(mem_img, b), groups, bank_groups, True)
    (loss * X.UPSTREAM).backward()
    assert mem_img.grad is None and mem_cap.grad is None
    for got, w64, w32 in zip((loss.detach(), a.grad, b.grad), grads[torch.float64], grads[torch.float32]):
        tol = X.FACTOR * max(float((w32.double() - w64).abs().max()), X.U * float(w64.abs().max()))
        err = float((got.cpu().double() - w64).abs().max())
        print("\n%s %s: err %.3g tol %.3g" % (measure, kind, err, tol))
        assert err <= tol, (err, tol)


def test_refused_inputs(dev):
    S, R, C = torch.rand(6, 6), torch.rand(6, 9), torch.rand(9, 6)
    g, b = np.arange(6), np.arange(9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.xbm_hinge_loss(S, R, C, g, b, 0.2, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.xbm_infonce_loss(S, R, C, g, b, T)
    S, R, C = S.to(dev), R.to(dev), C.to(dev)
    with pytest.raises(ValueError, match="square"):
        ops.xbm_hinge_loss(R, R, C, g, b, 0.2, True)
    for bad_r, bad_c in ((C, C), (R, R), (R[:, :8], C), (R[:5], C)):
        with pytest.raises(ValueError, match=r"needs R \[6, n\] and C \[n, 6\]"):
            ops.xbm_infonce_loss(S, bad_r, bad_c, g, b, T)
    with pytest.raises(ValueError, match="length 6"):
        ops.xbm_hinge_loss(S, R, C, b, b, 0.2, True)
    with pytest.raises(ValueError, match="length 9"):
        ops.xbm_hinge_loss(S, R, C, g, g, 0.2, True)
    with pytest.raises(ValueError, match="groups"):
        ops.xbm_hinge_loss(S, R, C, None, b, 0.2, True)
    with pytest.raises(TypeError):
        ops.xbm_hinge_loss(S, R, C, g.astype(np.float32), b, 0.2, True)
    with pytest.raises(TypeError):
        ops.xbm_infonce_loss(S.double(), R, C, g, b, T)
    with pytest.raises(ValueError, match="temperature"):
        ops.xbm_infonce_loss(S, R, C, g, b, 0.0)
