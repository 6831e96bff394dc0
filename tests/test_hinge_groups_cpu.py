"""CPU: the float64 helper the masked-hinge GPU tests compare against (tests/helpers/hinge_groups_oracle.py) is itself checked --
with all groups distinct it is the oracle's hinge, it masks what it should, and its arg-max takes the lower index on ties."""
import os
import sys

import numpy as np
import pytest
import torch

import itr_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hinge_groups_oracle as H  # noqa: E402


@pytest.mark.parametrize("mv", [False, True])
@pytest.mark.parametrize("B", [1, 2, 7, 65, 130])
def test_distinct_groups_equal_the_oracle(mv, B):
    torch.manual_seed(B)
    sc = torch.rand(B, B).double()
    want_l, want_g = O.hinge_loss_and_grad(sc, 0.2, mv)
    for groups in (np.arange(B), np.arange(B)[::-1] * 7 - 3):
        got_l, got_g = H.hinge_groups_loss_and_grad(sc, groups, 0.2, mv)
        assert got_l.dtype == torch.float64 and got_g.dtype == torch.float64
        assert float(got_l) == pytest.approx(float(want_l), rel=1e-14, abs=1e-14)
        assert torch.equal(got_g, want_g)


@pytest.mark.parametrize("mv", [False, True])
def test_masked_entries_cost_nothing(mv):
    torch.manual_seed(3)
    B = 9
    sc = torch.rand(B, B).double()
    groups = [0, 1, 0, 2, 3, 0, 4, 3, 5]
    masked = H.same_group(groups) & ~torch.eye(B, dtype=torch.bool)
    assert int(masked.sum()) == 8
    loss, g = H.hinge_groups_loss_and_grad(sc, groups, 0.2, mv)
    assert float(g[masked].abs().max()) == 0.0
    # the masked scores do not enter the loss at all: any value gives the same loss and the same gradient
    other = sc.clone()
    other[masked] += 5.0
    loss2, g2 = H.hinge_groups_loss_and_grad(other, groups, 0.2, mv)
    assert float(loss2) == float(loss) and torch.equal(g, g2)
    assert float(O.hinge_loss(other, 0.2, mv)) > float(loss) + 1.0          # ... unlike the reference's loss
    # brute force
    want = 0.0
    for i in range(B):
        rs = [max(0.0, 0.2 + float(sc[i, j]) - float(sc[i, i])) for j in range(B) if j != i and groups[i] != groups[j]]
        cs = [max(0.0, 0.2 + float(sc[j, i]) - float(sc[i, i])) for j in range(B) if j != i and groups[i] != groups[j]]
        want += (max(rs) + max(cs)) if mv else (sum(rs) + sum(cs))
    assert float(loss) == pytest.approx(want, rel=1e-13)


def test_lower_index_wins_ties():
    S = torch.zeros(4, 4, dtype=torch.float64)
    S.fill_diagonal_(1.0)
    S[0, 1] = S[0, 3] = 0.95          # row 0: columns 1 and 3 tie
    S[1, 2] = S[3, 2] = 0.97          # column 2: rows 1 and 3 tie
    groups = [0, 1, 2, 3]
    ra, ca = H.hinge_groups_args(S, groups, 0.2)
    assert int(ra[0]) == 1 and int(ca[2]) == 1
    _, g = H.hinge_groups_loss_and_grad(S, groups, 0.2, True)
    # each of these entries is also the only violator of its own column (0, 1), (0, 3) or row (1, 2), (3, 2): +1 from there
    assert float(g[0, 1]) == 2.0 and float(g[0, 3]) == 1.0
    assert float(g[1, 2]) == 2.0 and float(g[3, 2]) == 1.0
    # with the lower-index one masked, the tie goes to the unmasked higher index
    ra, ca = H.hinge_groups_args(S, [0, 0, 2, 3], 0.2)
    assert int(ra[0]) == 3
    _, g = H.hinge_groups_loss_and_grad(S, [0, 0, 2, 3], 0.2, True)
    assert float(g[0, 1]) == 0.0 and float(g[0, 3]) == 2.0


def test_flip_distance():
    S = torch.tensor([[1.0, 0.9, 0.3], [0.2, 1.0, 0.85], [0.1, 0.7, 1.0]], dtype=torch.float64)
    g = [0, 1, 2]
    assert H.flip_distance(S, g, 0.2, False) == pytest.approx(0.05, abs=1e-12)       # 0.2 + 0.85 - 1 = 0.05 from its kink
    assert H.flip_distance(S, g, 0.2, True) == pytest.approx(0.05, abs=1e-12)
    S[0, 2] = 0.9 - 1e-9                                                              # a near tie in row 0
    assert H.flip_distance(S, g, 0.2, True) == pytest.approx(1e-9, rel=1e-3)
    S[0, 2] = 0.9                                                                     # an exact tie is no hazard
    assert H.flip_distance(S, g, 0.2, True) == pytest.approx(0.05, abs=1e-12)
