"""GPU: ops.rerank_fused_lists / itr_rerank_fuse_lists (csrc/rerank_fuse.hip) against tests/helpers/ensemble_oracle.py, bit for bit:
idx, perm, the fused float64 scores as uint64 and the permuted member scores as uint32.  Scores come from a small set (multiples
of 0.25 in [-1, 1]) and indices repeat, so most lists hold exact fused ties and duplicate candidates; +-inf, NaN and -0.0 are
sprinkled in, and +inf meets -inf in one slot (the fused NaN sorts first and comes out as NaN).

One statement about NaN bits.  IEEE 754 fixes neither the sign nor the payload of a NaN an operation produces (inf - inf, or a NaN
operand passed through + and /): x86 gives the negative default NaN, other hardware a positive one.  So where the oracle's fused
score is a NaN the kernel's must be a NaN, at the same position; every other double, and every member score including NaNs (they are
moved, not computed), is compared by its bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ensemble_oracle                                                               # noqa: E402
from itr_amd import _lib, ops                                                        # noqa: E402

pytestmark = pytest.mark.gpu

ALL_K = [1, 2, 3, 10, 63, 64, 65, 100, 127, 128]
CASES = sorted(set([(2, K) for K in ALL_K] + [(M, K) for M in (1, 2, 3, 4) for K in (3, 65, 128)]))


def make_lists(seed, M, n, K):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, max(2, (3 * K) // 4), size=(n, K)).astype(np.int32)          # fewer names than slots: repeats
    vals = (rng.randint(-4, 5, size=(M, n, K)) * 0.25).astype(np.float32)
    special = np.asarray([np.inf, -np.inf, np.nan, -0.0], dtype=np.float32)
    hit = rng.rand(M, n, K) < 0.06
    vals[hit] = special[rng.randint(0, 4, size=int(hit.sum()))]
    if M >= 2:                                                                          # +inf and -inf in one slot: a fused NaN
        vals[0, :, K // 2] = np.inf
        vals[1, :, K // 2] = -np.inf
    return idx, vals


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def assert_same(got, want, what=""):
    gi, gf, gv, gp = [t.cpu().numpy() for t in got]
    wi, wf, wv, wp = want
    assert gi.dtype == np.int32 and gf.dtype == np.float64 and gv.dtype == np.float32 and gp.dtype == np.int32
    assert np.array_equal(gp, wp), what
    assert np.array_equal(gi, wi), what
    nan = np.isnan(wf)
    assert np.array_equal(np.isnan(gf), nan), what
    assert np.array_equal(gf.view(np.uint64)[~nan], wf.view(np.uint64)[~nan]), what
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), what
    return bool(np.array_equal(gf.view(np.uint64), wf.view(np.uint64)))


@pytest.mark.parametrize("M,K", CASES)
def test_fused_lists_equal_the_oracle(dev, M, K):
    raw = []
    for n in (1, 3, 257):
        idx, vals = make_lists(1000 * M + K, M, n, K)
        want = ensemble_oracle.fuse(idx, vals)
        got = ops.rerank_fused_lists(torch.from_numpy(idx).to(dev), torch.from_numpy(vals).to(dev))
        raw.append(assert_same(got, want, (M, n, K)))
        if M >= 2:
            # the slot where +inf met -inf: its fused NaN stands in the leading group (NaN sorts as +inf) and is still a NaN
            f, p = got[1].cpu().numpy(), got[3].cpu().numpy()
            for q in range(n):
                at = int(np.nonzero(p[q] == K // 2)[0][0])
                assert np.isnan(f[q, at]), (q, at)
                assert all(np.isnan(x) or x == np.inf for x in f[q, :at]), (q, at)
        # a sequence of members is the same call
        got2 = ops.rerank_fused_lists(torch.from_numpy(idx).to(dev), [torch.from_numpy(v).to(dev) for v in vals])
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, got2))
    print("M = %d, K = %d: NaN bit patterns equal numpy's too: %s" % (M, K, raw))


def test_only_float64_separates_these(dev):
    """members (1.0, 2^-30) against (1.0, 0.0): 1 + 2^-30 rounds to 1 in fp32, so an fp32 accumulator ties the two entries and the
    higher index would lead; in float64 the lower index has the larger score"""
    idx = torch.tensor([[4, 9]], dtype=torch.int32, device=dev)
    vals = torch.tensor([[[1.0, 1.0]], [[2.0 ** -30, 0.0]]], dtype=torch.float32, device=dev)
    assert float(np.float32(1.0) + np.float32(2.0 ** -30)) == 1.0
    io, fo, vo, po = ops.rerank_fused_lists(idx, vals)
    assert io.cpu().tolist() == [[4, 9]] and po.cpu().tolist() == [[0, 1]]
    assert fo.cpu().tolist() == [[(1.0 + 2.0 ** -30) / 2.0, 0.5]]
    assert_same((io, fo, vo, po), ensemble_oracle.fuse(idx.cpu().numpy(), vals.cpu().numpy()))


def test_division_by_three_is_a_division(dev):
    """(0.25 + 0.25 + 0.75) / 3.0 = 0x1.aaaaaaaaaaaabp-2, while 1.25 * (1.0 / 3.0) = 0x1.aaaaaaaaaaaaap-2 (found by search on the
    host): a reciprocal multiply shows in the last bit"""
    assert 1.25 / 3.0 == float.fromhex('0x1.aaaaaaaaaaaabp-2') and 1.25 * (1.0 / 3.0) == float.fromhex('0x1.aaaaaaaaaaaaap-2')
    idx = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    vals = torch.tensor([[[0.25, 0.5, 0.0]], [[0.25, 0.5, 0.0]], [[0.75, 0.5, 0.0]]], dtype=torch.float32, device=dev)
    io, fo, vo, po = ops.rerank_fused_lists(idx, vals)
    assert io.cpu().tolist() == [[1, 0, 2]]
    assert fo.cpu().numpy().view(np.uint64).tolist() == [np.asarray([0.5, float.fromhex('0x1.aaaaaaaaaaaabp-2'), 0.0]).view(np.uint64).tolist()]
    assert_same((io, fo, vo, po), ensemble_oracle.fuse(idx.cpu().numpy(), vals.cpu().numpy()))


@pytest.mark.parametrize("K", [3, 65, 128])
def test_one_member_is_rerank_lists(dev, K):
    idx, vals = make_lists(7 + K, 1, 257, K)
    d_idx, d_val = torch.from_numpy(idx).to(dev), torch.from_numpy(vals).to(dev)
    ri, rv, rp = ops.rerank_lists(d_idx, d_val[0].contiguous())
    io, fo, vo, po = ops.rerank_fused_lists(d_idx, d_val)
    assert torch.equal(io, ri) and torch.equal(po, rp)
    assert torch.equal(vo[0].view(torch.int32), rv.view(torch.int32))
    # float64 of an fp32 score, exactly (NaN: position only)
    f, r = fo.cpu().numpy(), rv.cpu().numpy().astype(np.float64)
    nan = np.isnan(r)
    assert np.array_equal(np.isnan(f), nan) and np.array_equal(f.view(np.uint64)[~nan], r.view(np.uint64)[~nan])


@pytest.mark.parametrize("K", [2, 65, 128])
def test_swapping_two_members_changes_nothing(dev, K):
    idx, vals = make_lists(11 + K, 2, 257, K)
    d_idx, d_val = torch.from_numpy(idx).to(dev), torch.from_numpy(vals).to(dev)
    a = ops.rerank_fused_lists(d_idx, d_val)
    b = ops.rerank_fused_lists(d_idx, d_val.flip(0).contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))                  # fused bits, NaNs included: one device
    assert torch.equal(a[2].view(torch.int32), b[2].flip(0).view(torch.int32))


def test_raw_abi_without_member_output(dev):
    lib = _lib.load()
    M, n, K = 3, 5, 65
    idx, vals = make_lists(5, M, n, K)
    d_idx, d_val = torch.from_numpy(idx).to(dev), torch.from_numpy(vals).to(dev)
    want = ops.rerank_fused_lists(d_idx, d_val)
    io, po = torch.full_like(d_idx, -7), torch.full_like(d_idx, -7)
    fo = torch.full((n, K), -7.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    rc = lib.itr_rerank_fuse_lists(p(d_idx), p(d_val), M, n, K, p(io), p(fo), None, p(po), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.itr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(io, want[0]) and torch.equal(po, want[3]) and torch.equal(fo.view(torch.int64), want[1].view(torch.int64))


def test_host_side_refusals(dev):
    idx = torch.zeros((2, 4), dtype=torch.int32, device=dev)
    val = torch.zeros((2, 2, 4), dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rerank_fused_lists(idx.cpu(), val)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rerank_fused_lists(idx, [val[0].cpu(), val[1]])
    with pytest.raises(TypeError):
        ops.rerank_fused_lists(idx.long(), val)
    with pytest.raises(TypeError):
        ops.rerank_fused_lists(idx, val.double())
    with pytest.raises(ValueError):
        ops.rerank_fused_lists(idx, val[:, :, :3].contiguous())
    with pytest.raises(ValueError):
        ops.rerank_fused_lists(idx, [val[0], val[1][:1]])
    with pytest.raises(ValueError):
        ops.rerank_fused_lists(idx, val[0])
    with pytest.raises(NotImplementedError):
        ops.rerank_fused_lists(torch.zeros((2, 129), dtype=torch.int32, device=dev), torch.zeros((2, 2, 129), dtype=torch.float32, device=dev))
    with pytest.raises(NotImplementedError):
        ops.rerank_fused_lists(idx, torch.zeros((5, 2, 4), dtype=torch.float32, device=dev))
    io, fo, vo, po = ops.rerank_fused_lists(idx[:0], val[:, :0])
    assert io.shape == (0, 4) and fo.shape == (0, 4) and fo.dtype == torch.float64 and vo.shape == (2, 0, 4) and po.shape == (0, 4)
