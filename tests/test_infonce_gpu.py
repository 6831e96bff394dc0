"""GPU: the InfoNCE loss (csrc/infonce.hip: itr_infonce_fwd / _bwd; ops.infonce_loss) against the float64 helper
(tests/helpers/infonce_oracle.py) over the helper's case table.

Sizes: 1, 2, the wave (64) and workgroup (256) strides of the kernels and their neighbours, 300, and one global-batch size (1024: 16
column blocks x 16 row slices).  Amplitudes at temperature 0.05: S = rand (z within 20) and S = 30 * rand (z up to ~750: exp without
its maximum subtracted overflows fp32), each plus a quarter of the amplitude on the last row and column, so that an index dropped
at the end moves the loss by thousands of tolerances (tests/test_infonce_cpu.py proves it for every case).  Groups: none, and the
clustered draw of test_hinge_groups_gpu.py.  Upstream gradient 3.0.

Tolerance, for the loss and for dS: the primary rule of tests/helpers/train_prim_cases.py, FACTOR * max(e32, U * max|want|), e32 the
float32 helper's own error against float64."""
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import infonce_oracle as N  # noqa: E402

pytestmark = pytest.mark.gpu

T = N.TEMPERATURE


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def run(S, groups, dev, temperature=T, upstream=N.UPSTREAM):
    s = S.to(dev).requires_grad_(True)
    loss = ops.infonce_loss(s, temperature, groups=groups)
    (loss * upstream).backward()
    return loss.detach(), s.grad


@pytest.mark.parametrize("B,amp,grouped", N.CASES, ids=["B%d-amp%g-%s" % (b, a, "groups" if g else "plain") for b, a, g in N.CASES])
def test_sweep_vs_float64(dev, B, amp, grouped):
    ref = N.reference(B, amp, grouped)
    loss, grad = run(ref["S"], ref["groups"], dev)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == (B, B)
    failures = []
    for name, got in (("loss", loss.cpu().double()), ("dS", grad.cpu().double())):
        want, e32, tol = ref[name]
        err = float((got - want).abs().max())
        print("\nB=%d amp=%g groups=%s %s: got %.9g want %.9g (max|want| %.6g) err %.3g e32 %.3g tol %.3g" % (
            B, amp, grouped, name, float(got.reshape(-1)[0]), float(want.reshape(-1)[0]), float(want.abs().max()), err, e32, tol))
        if not (torch.isfinite(got).all() and err <= tol):
            failures.append((name, err, tol))
    assert not failures, failures
    masked = ~N.allowed(ref["groups"], B)
    if grouped and B >= 2:
        assert int(masked.sum()) >= 2
    assert torch.equal(bits(grad)[masked], torch.zeros(int(masked.sum()), dtype=torch.int32))       # bit-zero, not -0.0


@pytest.mark.parametrize("B,amp", [(1, 1.0), (65, 1.0), (300, 30.0), (1024, 1.0), (1024, 30.0)])
def test_same_bits_run_to_run(dev, B, amp):
    ref = N.reference(B, amp, True)
    l0, g0 = run(ref["S"], ref["groups"], dev)
    l1, g1 = run(ref["S"], ref["groups"], dev)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(g0), bits(g1))


@pytest.mark.parametrize("B,amp", [(1, 1.0), (2, 30.0), (65, 1.0), (257, 30.0), (300, 1.0), (1024, 30.0)])
def test_distinct_groups_have_the_bits_of_no_groups(dev, B, amp):
    S = N.reference(B, amp, False)["S"].to(dev)
    groups = np.random.RandomState(B).permutation(B) * 5 - 7
    l0, r0, c0 = ops.infonce_fwd(S, T)
    l1, r1, c1 = ops.infonce_fwd(S, T, groups=groups)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(r0), bits(r1)) and torch.equal(bits(c0), bits(c1))
    g = torch.full((1,), N.UPSTREAM, device=dev)
    assert torch.equal(bits(ops.infonce_bwd(S, T, r0, c0, g)), bits(ops.infonce_bwd(S, T, r1, c1, g, groups=groups)))
    a, b = run(S.cpu(), None, dev), run(S.cpu(), groups, dev)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_saved_log_sum_exps(dev):
    """row_lse / col_lse, the forward's saved vectors, are the helper's: torch.logsumexp over the kept entries"""
    ref = N.reference(300, 1.0, True)
    z = ref["S"].double() * ref["scale"]
    keep = N.allowed(ref["groups"], 300)
    _, r, c = ops.infonce_fwd(ref["S"].to(dev), T, groups=ref["groups"])
    for got, want in ((r, N._lse(z, keep, 1)), (c, N._lse(z, keep, 0))):
        assert float((got.cpu().double() - want).abs().max()) <= N.FACTOR * N.U * float(want.abs().max()) + N.FACTOR * N.U * float(z.abs().max())


@pytest.mark.parametrize("B", [1, 5, 300])
@pytest.mark.parametrize("amp", N.AMPLITUDES)
def test_one_group_batch_is_zero(dev, B, amp):
    S = N.reference(300, amp, False)["S"][:B, :B].contiguous()
    loss, grad = run(S, [7] * B, dev)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_batch_of_one_is_zero(dev):
    for value in (0.3, -40.0, 35.0):
        loss, grad = run(torch.full((1, 1), value), None, dev)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0 and grad.shape == (1, 1)


def test_rows_without_negatives_contribute_nothing(dev):
    """rows 1 and 2 of a batch of 3 share a group: each keeps row 0 as its only negative (the primary rule holds on this matrix
    too); the two alone have no negative left, and the loss and its gradient are exactly 0"""
    S = torch.tensor([[0.5, 0.9, 0.1], [0.2, 0.4, 0.8], [0.7, 0.3, 0.6]])
    loss, grad = run(S, [1, 2, 2], dev)
    l64, d64 = N.infonce_loss_and_grad(S, [1, 2, 2], N.scale_of(T), upstream=N.UPSTREAM)
    l32, d32 = N.infonce_loss_and_grad(S, [1, 2, 2], N.scale_of(T), torch.float32, N.UPSTREAM)
    for got, w64, w32 in ((loss.cpu().double(), l64, l32), (grad.cpu().double(), d64, d32)):
        assert float((got - w64).abs().max()) <= N.FACTOR * max(float((w32.double() - w64).abs().max()), N.U * float(w64.abs().max()))
    assert float(grad[1, 2]) == 0.0 and float(grad[2, 1]) == 0.0
    loss, grad = run(S[1:, 1:].contiguous(), [2, 2], dev)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_temperature_and_group_input_kinds(dev):
    ref = N.reference(65, 1.0, True)
    S, groups = ref["S"], ref["groups"]
    want_l, want_g = run(S, groups, dev)
    for kind in (torch.from_numpy(groups), torch.from_numpy(groups).to(dev), groups.astype(np.int32), [int(x) for x in groups]):
        loss, grad = run(S, kind, dev)
        assert torch.equal(bits(loss), bits(want_l)) and torch.equal(bits(grad), bits(want_g))
    for temperature in (0.07, 1.0):
        loss, grad = run(S, groups, dev, temperature=temperature)
        l64, d64 = N.infonce_loss_and_grad(S, groups, N.scale_of(temperature), upstream=N.UPSTREAM)
        l32, d32 = N.infonce_loss_and_grad(S, groups, N.scale_of(temperature), torch.float32, N.UPSTREAM)
        for got, w64, w32 in ((loss.cpu().double(), l64, l32), (grad.cpu().double(), d64, d32)):
            tol = N.FACTOR * max(float((w32.double() - w64).abs().max()), N.U * float(w64.abs().max()))
            assert float((got - w64).abs().max()) <= tol, (temperature, float((got - w64).abs().max()), tol)
    # a non-contiguous view is taken as the matrix it shows
    wide = torch.zeros(65, 80)
    wide[:, :65] = S
    s = wide.to(dev)[:, :65].requires_grad_(True)
    (ops.infonce_loss(s, T, groups=groups) * N.UPSTREAM).backward()
    assert torch.equal(bits(s.grad), bits(want_g))


def test_refused_inputs(dev):
    S = torch.rand(6, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infonce_loss(S, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.infonce_fwd(S, T)
    for bad in (torch.rand(6, 5), torch.rand(6), torch.rand(2, 6, 6)):
        with pytest.raises(ValueError, match="square"):
            ops.infonce_loss(bad.to(dev), T)
    for bad in ([1] * 5, [1] * 7, np.zeros((6, 1), dtype=np.int64), torch.zeros(7, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="length 6"):
            ops.infonce_loss(S.to(dev), T, groups=bad)
    with pytest.raises(TypeError):
        ops.infonce_loss(S.to(dev), T, groups=np.zeros(6, dtype=np.float32))
    for bad in (0.0, -0.05, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            ops.infonce_loss(S.to(dev), bad)
        with pytest.raises(ValueError, match="temperature"):
            ops.infonce_fwd(S.to(dev), bad)
    with pytest.raises(TypeError):
        ops.infonce_loss(S.double().to(dev), T)
