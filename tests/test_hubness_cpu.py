"""CPU: the numpy oracle of the hubness corrections (tests/helpers/hubness_oracle.py) against hand-computed cases, the identity that
lets one adjusted matrix serve both directions, and the planted-hub property the GPU tests rely on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hubness_oracle as H        # noqa: E402

INF, NAN = float('inf'), float('nan')
LN2 = math.log(2.0)


def test_lse_hand_cases():
    S = np.array([[0.0, 0.0, -INF, -INF],          # two ones: ln 2
                  [-INF, -INF, -INF, -INF],        # nothing: -inf
                  [1000.0, 1000.0, 1000.0, 1000.0]])   # needs the shift: 1000 + ln 4
    got = H.lse_rows(S, 1.0)
    assert abs(got[0] - LN2) <= 1e-15 and got[1] == -INF and abs(got[2] - (1000.0 + 2 * LN2)) <= 2e-13
    # beta scales inside and out: (1 / 2) ln(4 e^0) = ln 2;  beta = 10, scores up to 1000: beta S = 1e4
    assert abs(H.lse(np.zeros(4), 2.0) - LN2) <= 1e-15
    assert abs(H.lse([1000.0, 1000.0, -1000.0, -INF], 10.0) - (1000.0 + LN2 / 10.0)) <= 2e-13
    # columns of the same matrix, beta = 1: [1000, 1000, 1000, 1000] (the other entries vanish beside e^1000)
    assert np.allclose(H.lse_cols(S, 1.0), 1000.0, rtol=0, atol=1e-12)
    # special values: np.logaddexp.reduce's results
    T = np.array([[0.0, INF, -INF, 1.0], [0.0, NAN, INF, 1.0], [-INF, -INF, 5.0, -INF]])
    got = H.lse_rows(T, 20.0)
    assert got[0] == INF and math.isnan(got[1]) and got[2] == 5.0
    with np.errstate(invalid='ignore'):
        want = [np.logaddexp.reduce(20.0 * r) / 20.0 for r in T]
    assert got[0] == want[0] and math.isnan(want[1]) and got[2] == want[2]
    c = H.lse_cols(T, 20.0)
    assert c[0] == 0.0 + math.log(2.0) / 20.0 and math.isnan(c[1]) and c[2] == INF and abs(c[3] - (1.0 + LN2 / 20.0)) <= 1e-15


def test_csls_hand_cases():
    S = np.array([[3.0, 1.0, 3.0, 2.0],            # a tie at the top: both 3s are taken, (3 + 3) / 2 / 2
                  [NAN, 1.0, 2.0, 0.0],            # NaN ranks as +inf: it is the first entry of the list
                  [-0.0, 0.0, -1.0, -2.0]])        # -0.0 == +0.0: the higher index, +0.0, is first
    a2 = H.csls_rows(S, 2)
    assert a2[0] == 1.5 and math.isnan(a2[1]) and a2[2] == 0.0
    a1 = H.csls_rows(S, 1)
    assert a1[0] == 1.5 and math.isnan(a1[1]) and a1[2] == 0.0 and not np.signbit(a1[2])
    # the tie goes to the higher index: with the zeros swapped the list starts with -0.0
    z = H.csls_rows(np.array([[0.0, -0.0, -1.0, -2.0]]), 1)
    assert z[0] == 0.0 and np.signbit(z[0])
    # k = 4: ((3 + 3) + 2) + 1, best first
    assert H.csls_rows(S[:1], 4)[0] == 0.5 * (9.0 / 4.0)
    # columns: of [3, nan, -0], [1, 1, 0], [3, 2, -1], [2, 0, -2] with k = 2
    b = H.csls_cols(S, 2)
    assert math.isnan(b[0]) and b[1] == 0.5 and b[2] == 1.25 and b[3] == 0.5
    # best first matters in float64: 1e16 + 1 + 1 is 1e16 when the small terms are added one at a time
    assert H.list_mean(np.array([[1e16, 1.0, 1.0]]), 3)[0] == 0.5 * (1e16 / 3.0)
    # float32 lists are widened, not summed in float32
    v = np.array([[16777216.0, 1.0]], dtype=np.float32)
    assert H.list_mean(v, 2)[0] == 0.5 * (16777217.0 / 2.0)


def test_adjust_hand_cases():
    S = np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32)
    out = H.adjust(S, np.array([0.5, 1.0]), np.array([0.25, 0.0]))
    assert out.dtype == np.float32 and np.array_equal(out, np.array([[0.25, 1.5], [1.75, 3.0]], dtype=np.float32))
    # two subtractions, each rounded on its own: with u = 2^-53, 1 - 0.6 u rounds to 1 - u and (1 - u) - 0.6 u to 1 - 2 u;
    # subtracting the sum 1.2 u at once would give 1 - u
    u = 2.0 ** -53
    one = H.adjust(np.array([[1.0]]), np.array([0.6 * u]), np.array([0.6 * u]))
    assert one[0, 0] == 1.0 - 2 * u and 1.0 - (0.6 * u + 0.6 * u) == 1.0 - u
    # None means zeros, and zeros change nothing, signed zeros and special values included
    Z = np.array([[-0.0, 0.0, NAN, -INF]])
    assert np.array_equal(H.adjust(Z).view(np.uint64), Z.view(np.uint64))
    assert np.array_equal(H.adjust(Z, None, np.zeros(4)).view(np.uint64), Z.view(np.uint64))
    # inf - inf is NaN, as numpy gives it
    assert math.isnan(H.adjust(np.array([[INF]]), np.array([INF]), None)[0, 0])
    # the cast comes last: 16777216 - 0.5 - 0.25 = 16777215.25 exactly in float64, and float32 keeps 16777215
    big = H.adjust(np.array([[16777216.0]], dtype=np.float32), np.array([0.5]), np.array([0.25]))
    assert big.dtype == np.float32 and big[0, 0] == np.float32(16777215.0)


def test_ranks_oracle_on_a_tiny_matrix():
    # 2 images x 10 captions; image 0 owns captions 0-4
    S = np.zeros((2, 10))
    S[0, 7] = 3.0
    S[0, 2] = 2.0
    S[1, 9] = 1.0
    i_rank, i_top, t_rank, t_top = H.ranks(S)
    assert i_rank.tolist() == [1.0, 0.0] and i_top.tolist() == [7.0, 9.0]
    # column 0 is all zeros: the tie goes to the higher index, image 1 first, so caption 0's image (0) is at position 1
    assert t_rank[0] == 1.0 and t_top[0] == 1.0 and t_rank[7] == 1.0 and t_rank[2] == 0.0 and t_rank[9] == 0.0


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("method", ["invsoftmax", "csls"])
def test_one_matrix_serves_both_directions(seed, method):
    S = H.planted_hubs(seed)
    a, b = H.vectors(S, method, k=10, beta=20.0)
    both = H.ranks(H.adjust(S, a, b))
    only_b, only_a = H.ranks(H.adjust(S, None, b)), H.ranks(H.adjust(S, a, None))
    assert np.array_equal(both[0], only_b[0]) and np.array_equal(both[1], only_b[1])      # i2t: b does the work
    assert np.array_equal(both[2], only_a[2]) and np.array_equal(both[3], only_a[3])      # t2i: a does the work


@pytest.mark.parametrize("seed", range(6))
def test_planted_hubs_are_corrected(seed):
    S = H.planted_hubs(seed)
    raw = H.r_at_1(H.ranks(S)[0])
    assert raw <= 70.0, raw
    for method in ("invsoftmax", "csls"):
        a, b = H.vectors(S, method, k=10, beta=20.0)
        fixed = H.r_at_1(H.ranks(H.adjust(S, a, b))[0])
        assert fixed >= 90.0, (method, raw, fixed)
