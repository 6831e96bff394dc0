"""CPU: the float64 helper of the InfoNCE tests (tests/helpers/infonce_oracle.py) is the loss the header states -- against
torch's cross entropy without groups, against an explicit double loop over A(i) with groups, its closed-form dS against float64
autograd -- and the GPU table's inputs make a kernel that stops one index early visible at the table's tolerance."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import infonce_oracle as N  # noqa: E402

SCALE = N.scale_of(N.TEMPERATURE)


def test_scale_is_the_float32_reciprocal():
    assert SCALE == float(np.float32(1.0 / 0.05)) == 20.0
    assert N.scale_of(0.07) == float(np.float32(1.0 / 0.07)) != 1.0 / 0.07


@pytest.mark.parametrize("B", [1, 2, 7, 65])
@pytest.mark.parametrize("amp", N.AMPLITUDES)
def test_without_groups_is_the_symmetric_cross_entropy(B, amp):
    S, _ = N.make_case(B, amp, False)
    z = S.double() * SCALE
    t = torch.arange(B)
    want = 0.5 * (F.cross_entropy(z, t) + F.cross_entropy(z.t(), t))
    got, _ = N.infonce_loss_and_grad(S, None, SCALE)
    assert float(got) == pytest.approx(float(want), rel=1e-13, abs=1e-13)
    assert float(N.infonce_loss(S, None, SCALE)) == pytest.approx(float(want), rel=1e-13, abs=1e-13)
    # all groups distinct: nothing is masked
    assert float(N.infonce_loss(S, np.arange(B) * 7 - 3, SCALE)) == float(N.infonce_loss(S, None, SCALE))


@pytest.mark.parametrize("B", [2, 7, 23])
@pytest.mark.parametrize("amp", N.AMPLITUDES)
def test_with_groups_is_the_double_loop(B, amp):
    S, groups = N.make_case(B, amp, True)
    if B == 23:
        groups[[0, 5, 22]] = 99                     # the last row and column take part in a cluster as well
    z = (S.double() * SCALE).tolist()
    total = 0.0
    for i in range(B):
        A = [j for j in range(B) if j == i or groups[j] != groups[i]]
        mr = max(z[i][j] for j in A)
        mc = max(z[j][i] for j in A)
        row = mr + math.log(sum(math.exp(z[i][j] - mr) for j in A))
        col = mc + math.log(sum(math.exp(z[j][i] - mc) for j in A))
        total += (row - z[i][i]) + (col - z[i][i])
    want = total / (2 * B)
    got, _ = N.infonce_loss_and_grad(S, groups, SCALE)
    assert float(got) == pytest.approx(want, rel=1e-12, abs=1e-12)
    assert float(N.infonce_loss(S, groups, SCALE)) == pytest.approx(want, rel=1e-12, abs=1e-12)
    n_masked = int((~N.allowed(groups, B)).sum())
    assert n_masked >= 2
    if amp == 1.0:          # (at amplitude 30 a left-out entry can lie 100 below its row's maximum: below float64's last bit)
        assert float(got) != float(N.infonce_loss(S, None, SCALE))


@pytest.mark.parametrize("B", [1, 2, 7, 65, 130])
@pytest.mark.parametrize("amp", N.AMPLITUDES)
@pytest.mark.parametrize("grouped", [False, True])
def test_closed_form_gradient_is_autograd(B, amp, grouped):
    S, groups = N.make_case(B, amp, grouped)
    x = S.double().requires_grad_(True)
    (N.infonce_loss(x, groups, SCALE) * N.UPSTREAM).backward()
    _, dS = N.infonce_loss_and_grad(S, groups, SCALE, upstream=N.UPSTREAM)
    assert torch.isfinite(x.grad).all()
    assert float((dS - x.grad).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max()))
    masked = ~N.allowed(groups, B)
    if grouped and B >= 2:
        assert int(masked.sum()) >= 2
    assert float(dS[masked].abs().max() if masked.any() else 0.0) == 0.0
    assert float(x.grad[masked].abs().max() if masked.any() else 0.0) == 0.0
    # the same in float32: exact zeros as well
    _, d32 = N.infonce_loss_and_grad(S, groups, SCALE, torch.float32, N.UPSTREAM)
    assert d32.dtype == torch.float32 and float(d32[masked].abs().max() if masked.any() else 0.0) == 0.0


def test_edge_cases():
    S = torch.rand(5, 5)
    loss, dS = N.infonce_loss_and_grad(S, [4] * 5, SCALE, upstream=N.UPSTREAM)         # every negative masked
    assert float(loss) == 0.0 and float(dS.abs().max()) == 0.0
    loss, dS = N.infonce_loss_and_grad(S[:1, :1], None, SCALE, upstream=N.UPSTREAM)    # B = 1
    assert float(loss) == 0.0 and float(dS.abs().max()) == 0.0
    groups = [1, 2, 2, 2, 3]
    full, _ = N.infonce_loss_and_grad(S, groups, SCALE)
    keep = N.allowed(groups, 5)
    assert keep.tolist() == keep.t().tolist() and int((~keep).sum()) == 6 and bool(torch.diagonal(keep).all())


@pytest.mark.parametrize("B,amp,grouped", N.CASES, ids=["B%d-amp%g-%s" % (b, a, "groups" if g else "plain") for b, a, g in N.CASES])
def test_table_sees_a_dropped_last_index(B, amp, grouped):
    """Every case of the GPU table: row sums without column B - 1 and column sums without row B - 1 move the loss by at least
    SENSITIVITY x the tolerance the GPU test applies to it."""
    ref = N.reference(B, amp, grouped)
    want, e32, tol = ref["loss"]
    defect = N.infonce_loss(ref["S"], ref["groups"], ref["scale"], drop_last=True)
    moved = abs(float(defect) - float(want))
    print("\nB=%d amp=%g groups=%s: loss %.9g, e32 %.3g, tol %.3g, defect moves it by %.3g (%.3g x tol)" % (
        B, amp, grouped, float(want), e32, tol, moved, moved / tol if tol > 0 else float('inf')))
    assert tol >= 0.0 and moved > 0.0 and moved >= N.SENSITIVITY * tol
    assert tol <= 1e-4 * max(1.0, abs(float(want)))          # and the rule is no looser than the sibling tests' bound for a loss
