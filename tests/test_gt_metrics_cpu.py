"""CPU: metrics under a general ground-truth relation (evaluation.metrics_from_positions) against a brute force, the host CSR
construction of ops.GroundTruth and its refusals, and the argument checks of the new C entry points (nothing is launched)."""
import numpy as np
import pytest

from itr_amd import _lib, ops
from itr_amd.metricmodule import evaluation


def brute(ptr, pos, ks=(1, 5, 10)):
    """The definitions, query by query, in float64."""
    best, rp, ap = [], [], []
    none = 0
    for q in range(len(ptr) - 1):
        p = sorted(int(x) for x in pos[ptr[q]:ptr[q + 1]])
        if not p:
            none += 1
            continue
        R = len(p)
        best.append(p[0])
        rp.append(sum(1 for x in p if x < R) / R)
        ap.append(sum((j + 1) / (x + 1) for j, x in enumerate(p) if x < R) / R)
    n = len(best)
    out = {'r@%d' % k: 100.0 * sum(1 for b in best if b < k) / n for k in ks}
    out.update(medr=float(np.floor(np.median(best)) + 1), meanr=float(np.mean(best)) + 1, rprecision=100.0 * float(np.mean(rp)),
               map_at_r=100.0 * float(np.mean(ap)), n_queries=n, n_without_positives=none)
    return out


def test_worked_example():
    """Positives at positions {0, 2, 5}: R@1 = 1, R-Precision = 2/3, AP@R = (1/1 + 2/3) / 3 = 5/9."""
    m = evaluation.metrics_from_positions([0, 3], [5, 0, 2])
    assert m['r@1'] == 100.0 and m['r@5'] == 100.0 and m['medr'] == 1.0 and m['meanr'] == 1.0
    assert m['rprecision'] == pytest.approx(100.0 * 2 / 3, abs=1e-12)
    assert m['map_at_r'] == pytest.approx(100.0 * 5 / 9, abs=1e-12)
    assert m['n_queries'] == 1 and m['n_without_positives'] == 0
    assert m['best'].tolist() == [0] and m['rprecision_q'][0] == pytest.approx(2 / 3, abs=1e-15) and m['ap_q'][0] == pytest.approx(5 / 9, abs=1e-15)


def test_query_without_positives_is_left_out_of_the_means():
    m = evaluation.metrics_from_positions([0, 1, 1, 3], [4, 0, 7])
    assert m['n_queries'] == 2 and m['n_without_positives'] == 1
    assert m['best'].tolist() == [4, -1, 0] and np.isnan(m['rprecision_q'][1]) and np.isnan(m['ap_q'][1])
    assert m['r@1'] == 50.0 and m['r@5'] == 100.0 and m['medr'] == 3.0 and m['meanr'] == 3.0
    assert m['rprecision'] == pytest.approx(100.0 * (0 + 0.5) / 2, abs=1e-12)
    assert m['map_at_r'] == pytest.approx(100.0 * (0 + 0.5 * 1.0) / 2, abs=1e-12)
    empty = evaluation.metrics_from_positions([0, 0], [])
    assert empty['n_queries'] == 0 and empty['n_without_positives'] == 1 and np.isnan(empty['r@1']) and np.isnan(empty['map_at_r'])
    with pytest.raises(ValueError):
        evaluation.metrics_from_positions([0, 2], [1])


def test_random_positions_against_brute_force():
    rng = np.random.RandomState(0)
    for n_q, n_gallery, max_r in ((1, 10, 3), (50, 200, 40), (333, 1000, 12)):
        R = rng.randint(0, max_r + 1, size=n_q)
        ptr = np.concatenate([[0], np.cumsum(R)])
        pos = np.concatenate([rng.choice(n_gallery, size=r, replace=False) for r in R] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        if R.sum() == 0:
            continue
        got, want = evaluation.metrics_from_positions(ptr, pos, ks=(1, 5, 10, 50)), brute(ptr, pos, ks=(1, 5, 10, 50))
        for k, v in want.items():
            assert got[k] == pytest.approx(v, abs=1e-12), k


def test_ground_truth_host_csr():
    pairs = np.array([[2, 3], [0, 1], [2, 0], [0, 4], [1, 4]])
    ip, ic, cp, ci = ops.ground_truth_csr(pairs, 4, 5)
    assert ip.tolist() == [0, 2, 3, 5, 5] and ic.tolist() == [1, 4, 4, 0, 3]          # image 3 has none
    assert cp.tolist() == [0, 1, 2, 2, 3, 5] and ci.tolist() == [2, 0, 2, 0, 1]       # caption 2 has none
    assert all(a.dtype == np.int32 for a in (ip, ic, cp, ci))
    ip, ic, cp, ci = ops.ground_truth_csr(np.zeros((0, 2), dtype=np.int64), 2, 3)
    assert ip.tolist() == [0, 0, 0] and cp.tolist() == [0, 0, 0, 0] and len(ic) == len(ci) == 0
    import torch
    ip2 = ops.ground_truth_csr(torch.from_numpy(pairs), 4, 5)[0]
    assert ip2.tolist() == [0, 2, 3, 5, 5]


def test_ground_truth_refusals():
    with pytest.raises(ValueError, match=r"pair 1 = \(image 4, caption 0\)"):
        ops.ground_truth_csr([[0, 0], [4, 0]], 4, 5)
    with pytest.raises(ValueError, match=r"pair 0 = \(image 0, caption 5\)"):
        ops.ground_truth_csr([[0, 5]], 4, 5)
    with pytest.raises(ValueError, match="out of range"):
        ops.ground_truth_csr([[-1, 0]], 4, 5)
    with pytest.raises(ValueError, match=r"pair 2 = \(image 1, caption 2\) is given more than once"):
        ops.ground_truth_csr([[1, 2], [0, 0], [1, 2]], 4, 5)
    with pytest.raises(ValueError, match="shape"):
        ops.ground_truth_csr([[1, 2, 3]], 4, 5)
    with pytest.raises(TypeError):
        ops.ground_truth_csr(np.array([[0.0, 1.0]]), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.GroundTruth([[0, 0]], 1, 1, 'cpu')


def test_new_entry_points_check_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.itr_rank_gt_workspace_bytes(0, 0) < lib.itr_rank_gt_workspace_bytes(1000, 0) < lib.itr_rank_gt_workspace_bytes(1000, 1)
    #                               S   ldS row0 n Nc Ni nnz
    assert lib.itr_rank_gt_gather(None, 4, 0, 2, 4, 2, 3, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.itr_last_error()
    assert lib.itr_rank_gt_count(None, 4, 0, 2, 4, 2, 3, None, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.itr_rank_gt_count(None, 3, 0, 2, 4, 2, 3, None, None, None, None, None, None, 0, None, 0, None) == -1      # ldS < Nc
    assert b"bad shape" in lib.itr_last_error()
    assert lib.itr_rank_gt_count(None, 4, 1, 2, 4, 2, 3, None, None, None, None, None, None, 0, None, 0, None) == -1      # rows past Ni
    assert lib.itr_rank_gt_count(None, 4, 0, 2, 4, 2, 3, None, None, None, None, None, None, 2, None, 0, None) == -1      # unknown flag
    assert lib.itr_rank_gt_count(None, 4, 0, 2, 4, 2, 2 ** 31, None, None, None, None, None, None, 0, None, 0, None) == -2
    assert b"2^31" in lib.itr_last_error()
    assert lib.itr_rank_gt_positions_f64(None, 4, 2, 4, 3, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.itr_rank_gt_count(None, 4, 0, 2, 4, 2, 0, None, None, None, None, None, None, 0, None, 0, None) == 0       # nnz == 0: nothing to do
