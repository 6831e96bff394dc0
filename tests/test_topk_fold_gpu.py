"""GPU: running top-K column lists (ops.topk_fold_cols, csrc/topk_fold.hip).  Every partition of a matrix into row blocks, folded in
any order from an empty state or from topk_lists' part of the first block, gives the whole-matrix lists -- those of a numpy sort
written out here (canonical score: NaN -> +inf, -0.0 -> +0.0; score descending, then index descending; -1 where a column has fewer
than K rows) and those of the existing whole-matrix path (ops.topk_lists + ops.topk_merge_cols).  All comparisons are exact: indices
equal, values equal as uint32 bit patterns."""
import numpy as np
import pytest
import torch

from itr_amd import ops

pytestmark = pytest.mark.gpu

STRIP = 32                       # TF_COLS of csrc/topk_fold.hip: columns owned by one workgroup
KS = (1, 10, 100, 128)
ROW0 = 1000003
SHAPES = [(1, 1), (7, 5), (130, 37), (300, 1030), (257, 4099), (70, STRIP - 1), (70, STRIP), (70, STRIP + 1)]


def expected(S, k, row0=0):
    """-> (idx int64 [Nc, k] global rows, -1 past the column's rows; val float32 [Nc, k], 0 there)"""
    n, nc = S.shape
    c = np.array(S, copy=True)
    c[np.isnan(c)] = np.inf
    c = c + np.float32(0.0)
    order = np.argsort(c.T, axis=1, kind='stable')[:, ::-1][:, :k]           # ascending and stable, reversed: the higher index first
    idx = np.full((nc, k), -1, np.int64)
    val = np.zeros((nc, k), np.float32)
    m = min(n, k)
    idx[:, :m] = order + row0
    val[:, :m] = np.take_along_axis(S.T, order, 1)
    return idx, val


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def partitions(n):
    """name -> list of (r0, r1) covering 0 .. n, in folding order"""
    def cut(heights):
        out, r, i = [], 0, 0
        while r < n:
            h = heights[i] if i < len(heights) else n
            out.append((r, min(n, r + h)))
            r, i = out[-1][1], i + 1
        return out
    uneven = cut([3, 64, 1])
    cyc = cut([63, 64, 65] * (n // 63 + 1))
    shuffled = [uneven[i] for i in np.random.RandomState(n).permutation(len(uneven))] if len(uneven) > 1 else None
    rev = list(reversed(cyc))
    p = {"one": [(0, n)], "rows": [(r, r + 1) for r in range(n)], "uneven": uneven, "63_64_65": cyc, "63_64_65_reversed": rev}
    if shuffled:
        p["uneven_shuffled"] = shuffled
    return p


def on_device(S, dev, padded):
    """the matrix on the device: dense, or as the head of rows of a buffer whose leading dimension is a multiple of 4 (16-byte loads)"""
    n, nc = S.shape
    if not padded:
        return torch.from_numpy(S).to(dev)
    buf = torch.full((n, (nc + 3) // 4 * 4 + 4), 7.0, device=dev)
    buf[:, :nc] = torch.from_numpy(S).to(dev)
    return buf[:, :nc]


def fold(Sd, k, blocks, row0, start):
    state = None
    if start == "part":                # topk_lists' column part of the first block is a valid starting state
        r0, r1 = blocks[0]
        state = ops.topk_lists(Sd[r0:r1], k, row0 + r0, rows=False)[2]
        blocks = blocks[1:]
    elif start == "zeros":
        nc = Sd.shape[1]
        state = (torch.zeros(nc, k, device=Sd.device, dtype=torch.int64), torch.zeros(nc, k, device=Sd.device, dtype=torch.float32))
    for r0, r1 in blocks:
        out = ops.topk_fold_cols(Sd[r0:r1], k, row0 + r0, state)
        if state is not None:
            assert out[0] is state[0] and out[1] is state[1]            # updated in place and returned
        state = out
    return state


def finish(state, k):
    idx, val = ops.topk_merge_cols([state], k)
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy()


def check(state, k, want, whole, tag):
    idx, val = finish(state, k)
    assert np.array_equal(idx, want[0]), (tag, "idx vs numpy", int((idx != want[0]).sum()))
    assert np.array_equal(bits(val), bits(want[1])), (tag, "val vs numpy", int((bits(val) != bits(want[1])).sum()))
    # the state itself equals the whole-matrix part: keys and values, bit for bit
    assert torch.equal(state[0], whole[0]), (tag, "keys vs topk_lists")
    assert torch.equal(state[1].view(torch.int32), whole[1].view(torch.int32)), (tag, "vals vs topk_lists")


def matrix(n, nc, seed, kind="randn"):
    rng = np.random.RandomState(seed)
    if kind == "randn":
        S = rng.randn(n, nc).astype(np.float32)
        S[:, ::3] = np.round(S[:, ::3])                                   # exact ties in every third column
        return S
    # ties and special values; the second NaN has its sign bit set (bits must survive)
    pool = np.array([0xff800000, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000, 0x7f800000, 0x7fc00000, 0xffc00001], np.uint32).view(np.float32)
    return pool[rng.randint(0, len(pool), size=(n, nc))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_partition_gives_the_whole_matrix_lists(dev, shape):
    n, nc = shape
    S = matrix(n, nc, 11 * n + nc)
    parts = partitions(n)
    wants = {(k, row0): expected(S, k, row0) for k in KS for row0 in (0, ROW0)}       # computed once, shared by both layouts
    for padded in (True, False):
        Sd = on_device(S, dev, padded)
        for k in KS:
            for row0 in (0, ROW0):
                want = wants[k, row0]
                whole = ops.topk_lists(Sd, k, row0, rows=False)[2]
                w_idx, w_val = finish(whole, k)
                assert np.array_equal(w_idx, want[0]) and np.array_equal(bits(w_val), bits(want[1]))      # the existing path
                for name, blocks in parts.items():
                    if not padded and name not in ("uneven", "one"):
                        continue                                          # the dense layout: two partitions are enough
                    if row0 and name == "rows":
                        continue
                    for start in ("empty", "zeros", "part"):
                        if start == "zeros" and name != "uneven":
                            continue
                        state = fold(Sd, k, blocks, row0, start)
                        check(state, k, want, whole, (shape, padded, k, row0, name, start))


@pytest.mark.parametrize("shape", [(130, 37), (200, 1030)], ids=lambda s: "%dx%d" % s)
def test_ties_and_special_values_keep_their_bits(dev, shape):
    n, nc = shape
    S = matrix(n, nc, 5, "special")
    assert np.isnan(S).any() and (bits(S) == 0x80000000).any() and (bits(S) == 0xffc00001).any()
    for padded in (True, False):
        Sd = on_device(S, dev, padded)
        for k in KS:
            want = expected(S, k)
            whole = ops.topk_lists(Sd, k, 0, rows=False)[2]
            for name, blocks in partitions(n).items():
                if name == "rows" and k not in (1, 128):
                    continue
                for start in ("empty", "part"):
                    check(fold(Sd, k, blocks, 0, start), k, want, whole, (shape, padded, k, name, start))


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_worst_cases(dev, order):
    """ascending in row order: every element of every block passes the threshold (the kernel only merges more often); descending:
    nothing passes after the first K rows.  Nc = 1030, K = 128, blocks of 64 rows."""
    n, nc, k = 448, 1030, 128
    r = np.arange(n, dtype=np.float32)[:, None] + np.zeros((1, nc), np.float32)
    r[:, 1::2] += 0.5 * (np.arange(nc)[1::2] % 3)[None, :]             # not every column the same
    S = np.ascontiguousarray(r if order == "ascending" else -r)
    want = expected(S, k)
    for padded in (True, False):
        Sd = on_device(S, dev, padded)
        whole = ops.topk_lists(Sd, k, 0, rows=False)[2]
        blocks = [(r0, min(n, r0 + 64)) for r0 in range(0, n, 64)]
        for start in ("empty", "part"):
            check(fold(Sd, k, blocks, 0, start), k, want, whole, (order, padded, start))
        check(fold(Sd, k, [(0, n)], 0, "empty"), k, want, whole, (order, padded, "one block"))


def test_alignment(dev):
    """S[:, 1:] of a wider buffer (rows start 4 bytes off a 16-byte boundary) and an odd leading dimension, against the aligned copy"""
    n, nc, k = 200, 517, 100
    S = matrix(n, nc + 1, 9)
    wide = torch.from_numpy(S).to(dev)
    aligned = on_device(np.ascontiguousarray(S[:, 1:]), dev, True)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) % 4 == 0
    want = expected(S[:, 1:], k)
    blocks = partitions(n)["uneven"]
    ref = fold(aligned, k, blocks, 0, "empty")
    check(ref, k, want, ref, "aligned")
    shifted = wide[:, 1:]
    assert shifted.data_ptr() % 16 == 4 and shifted.stride(0) == nc + 1
    check(fold(shifted, k, blocks, 0, "empty"), k, want, ref, "S[:, 1:]")
    odd = torch.empty(n, nc + 2, device=dev)[:, :nc]
    assert odd.stride(0) % 2 == 1
    odd.copy_(aligned)
    check(fold(odd, k, blocks, 0, "empty"), k, want, ref, "odd ldS")
    # an aligned base with an even leading dimension that is no multiple of 4
    even = torch.empty(n, nc + 1, device=dev)[:, :nc]
    assert even.stride(0) % 4 == 2
    even.copy_(aligned)
    check(fold(even, k, blocks, 0, "empty"), k, want, ref, "ldS % 4 == 2")


def test_refusals_and_no_ops(dev):
    S = torch.randn(20, 40, device=dev)
    for k in (0, 129):
        with pytest.raises((ValueError, NotImplementedError)):
            ops.topk_fold_cols(S, k)
    k = 5
    good = ops.topk_fold_cols(S, k)
    assert good[0].shape == (40, k) and good[0].dtype == torch.int64 and good[1].dtype == torch.float32
    bad_states = [
        (good[0][:39], good[1][:39]),                                     # shape: a column short
        (good[0][:, :4].contiguous(), good[1][:, :4].contiguous()),       # shape: another k
        (good[0].to(torch.int32), good[1]),                               # dtype
        (good[0], good[1].to(torch.float64)),
        (good[0].cpu(), good[1].cpu()),                                   # device
        (good[0],),
    ]
    for st in bad_states:
        with pytest.raises(ValueError):
            ops.topk_fold_cols(S, k, 20, st)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_fold_cols(S.cpu(), k)
    with pytest.raises(TypeError):
        ops.topk_fold_cols(S.double(), k)
    # a zero-row block is a no-op on a state; Nc = 0 is a no-op
    before = (good[0].clone(), good[1].clone())
    out = ops.topk_fold_cols(S[:0], k, 20, good)
    assert out[0] is good[0] and torch.equal(good[0], before[0]) and torch.equal(good[1], before[1])
    empty = ops.topk_fold_cols(S[:0], k)
    assert empty[0].shape == (40, k) and not empty[0].any() and not empty[1].any()
    none = ops.topk_fold_cols(S[:, :0], k)
    assert none[0].shape == (0, k) and none[1].shape == (0, k)
    torch.cuda.synchronize()
