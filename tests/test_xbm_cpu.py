"""CPU: the float64 helper of the cross-batch-memory losses (tests/helpers/xbm_oracle.py) is what it says, and its case table can
tell a wrong kernel from a right one.  Runs without the library."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hinge_groups_oracle as HG  # noqa: E402
import xbm_oracle as X  # noqa: E402

IDS = [X.case_id(*c) for c in X.SWEEP]


def plain_losses(S, R, C, groups, bank_groups, margin, scale, mask_batch):
    """(hinge sum, hinge max, InfoNCE) by a double loop over Python floats"""
    S, R, C = S.double().tolist(), R.double().tolist(), C.double().tolist()
    B, n = len(S), len(C)
    total_sum = total_max = nce = 0.0
    for q in range(B):
        for side in ("row", "col"):
            costs, zs = [0.0], [scale * S[q][q]]          # the diagonal: cost 0, and a term of the softmax
            for t in range(B + n):
                if t == q:
                    continue
                if t < B:
                    if mask_batch and groups[t] == groups[q]:
                        continue
                    s = S[q][t] if side == "row" else S[t][q]
                else:
                    if bank_groups[t - B] == groups[q]:
                        continue
                    s = R[q][t - B] if side == "row" else C[t - B][q]
                costs.append(max(0.0, (margin + s) - S[q][q]))
                zs.append(scale * s)
            total_sum += sum(costs)
            total_max += max(costs)
            top = max(zs)
            nce += top + math.log(sum(math.exp(z - top) for z in zs)) - scale * S[q][q]
    return total_sum, total_max, nce / (2 * B)


@pytest.mark.parametrize("B,n", [(1, 1), (4, 3), (6, 9)])
@pytest.mark.parametrize("mask_batch", [False, True])
def test_helper_equals_a_double_loop(B, n, mask_batch):
    S, R, C, _, _ = X.make_case(B, n, 1.0)
    groups = np.asarray([5, 5, 9, 5, 2, 9][:B])
    bank_groups = np.asarray([9, 40, 5, 41, 42, 2, 43, 5, 44][:n])
    scale = X.scale_of(X.TEMPERATURE)
    want = plain_losses(S, R, C, groups, bank_groups, X.MARGIN, scale, mask_batch)
    got = (X.hinge_loss(S, R, C, groups, bank_groups, X.MARGIN, False, mask_batch),
           X.hinge_loss(S, R, C, groups, bank_groups, X.MARGIN, True, mask_batch),
           X.infonce_parts(S, R, C, groups, bank_groups, scale, mask_batch)[0])
    for g, w in zip(got, want):
        assert abs(float(g) - w) <= 1e-12 * max(1.0, abs(w)), (float(g), w)


def test_first_maximum_and_counts():
    """a tie between an in-batch candidate and a memory slot goes to the in-batch one; between two slots to the lower slot"""
    S = torch.tensor([[0.5, 0.7], [0.1, 0.6]])
    R = torch.tensor([[0.7, 0.9, 0.9], [0.2, 0.3, 0.3]])
    C = torch.tensor([[0.1, 0.2], [0.1, 0.9], [0.1, 0.9]])
    row, col = X.hinge_args(S, R, C, [1, 2], [3, 4, 5])
    assert row.tolist() == [3, -1] and col.tolist() == [-1, 3]
    row, col = X.hinge_args(S, R[:, :1], C[:1], [1, 2], [3])
    assert row.tolist() == [1, -1] and col.tolist() == [-1, 0]
    rc, cc = X.hinge_counts(S, R, C, [1, 2], [3, 4, 5])
    assert rc.tolist() == [4, 0] and cc.tolist() == [0, 3]


def test_case_table_covers_the_seams():
    Bs, ns = {b for b, _ in X.CASES}, {n for _, n in X.CASES}
    assert Bs == {1, 2, 63, 64, 65, 128, 257} and ns == {1, 63, 64, 65, 255, 257, 1000, 4099}
    assert 14 <= len(X.CASES) <= 18 and len(set(X.CASES)) == len(X.CASES)
    for values in X.SEAMS.values():
        for v in values:
            if isinstance(v, tuple):
                assert v in X.CASES, v


@pytest.mark.parametrize("B,n", X.CASES)
def test_groups_drop_entries_everywhere(B, n):
    _, _, _, groups, bank_groups = X.make_case(B, n, 1.0)
    keep_s, keep_r, keep_c = X.kept(groups, bank_groups, True)
    assert bool(X.kept(groups, bank_groups, False)[0].all())
    if B >= 2 and n >= 2:
        assert int((~keep_s).sum()) >= 2 and int((~keep_r).sum()) >= 2 and int((~keep_c).sum()) >= 2
        assert bool(keep_r[:, -1].all()) and bool(keep_c[-1, :].all())          # the last slot is nobody's own image


@pytest.mark.parametrize("B,n,kind,amp,mask_batch", X.SWEEP, ids=IDS)
def test_last_slot_is_decisive_and_no_decision_is_close(B, n, kind, amp, mask_batch):
    ref = X.reference(B, n, kind, amp, mask_batch)
    want, _, tol = ref["loss"]
    moved = X.last_slot_move(ref, kind, mask_batch)
    print("\n%s: seed %d, loss %.9g, tol %.3g, moves by %.3g without the last slot, flip distance %.3g" % (
        X.case_id(B, n, kind, amp, mask_batch), ref["seed"], float(want), tol, moved, ref["flip"]))
    assert moved > X.SENSITIVITY * tol, (moved, float(want), tol)
    if kind != "infonce":
        assert ref["flip"] > HG.FP32_COST_ERR, ref["flip"]
