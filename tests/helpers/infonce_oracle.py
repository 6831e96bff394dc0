"""Float64 restatement of the InfoNCE loss of csrc/infonce.hip (include/itr_hip.h: itr_infonce_fwd / _bwd), plain torch on the CPU,
and the case table its CPU and GPU tests share.  Nothing here imports the library.

    z = scale * S,  scale = float(np.float32(1 / temperature)) -- the factor the op hands to the kernels
    A(i) = {i} u {j : group[j] != group[i]}            (an off-diagonal entry of one group is masked: left out, not set to -inf)
    row_lse[i] = log sum_{j in A(i)} exp z[i,j]        col_lse[j] = log sum_{i in A(j)} exp z[i,j]
    loss = (sum_i (row_lse[i] - z[i,i]) + sum_j (col_lse[j] - z[j,j])) / (2 B)
    dS[i,j] = g scale / (2 B) (exp(z[i,j] - row_lse[i]) + exp(z[i,j] - col_lse[j]) - 2 [i == j]) on A, 0 at masked entries

Run in float32 (dtype=torch.float32) the same statements give the reference's own rounding error e32; the tolerance of a compared
tensor is the primary rule of tests/helpers/train_prim_cases.py: FACTOR * max(e32, U * max|want|)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_prim_cases import FACTOR, SENSITIVITY, U  # noqa: E402,F401

TEMPERATURE = 0.05
UPSTREAM = 3.0
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1024]      # wave and workgroup strides, their neighbours, one global-batch size
AMPLITUDES = [1.0, 30.0]                                  # z within 20; z up to ~750, where exp without its maximum overflows fp32
CASES = [(B, amp, grouped) for B in SIZES for amp in AMPLITUDES for grouped in (False, True)]


def scale_of(temperature):
    return float(np.float32(1.0 / float(temperature)))


def allowed(groups, B):
    """bool [B, B]: True where (i, j) is in the sums -- the diagonal and every entry of two different groups."""
    if groups is None:
        return torch.ones(B, B, dtype=torch.bool)
    g = torch.as_tensor(np.asarray(groups, dtype=np.int64))
    assert g.shape == (B,)
    return (g[:, None] != g[None, :]) | torch.eye(B, dtype=torch.bool)


def _lse(z, keep, dim):
    """log sum exp over the kept entries along `dim`, relative to their maximum; an empty set gives -inf"""
    floor = z.min() if z.numel() else z.new_zeros(())
    m = torch.where(keep, z, floor).max(dim, keepdim=True).values
    zk = torch.where(keep, z, m.expand_as(z))              # a left-out entry never reaches exp (it may lie far above the kept maximum)
    s = torch.where(keep, torch.exp(zk - m), torch.zeros_like(z)).sum(dim, keepdim=True)
    return (m + torch.log(s)).squeeze(dim)


def infonce_loss(S, groups, scale, dtype=torch.float64, drop_last=False):
    """The loss (0-dim tensor of `dtype`), differentiable w.r.t. S.  drop_last: the row sums lose column B - 1 and the column sums
    lose row B - 1 -- the defect of a kernel that stops one index early."""
    B = S.shape[0]
    z = S.to(dtype) * torch.tensor(scale, dtype=dtype)
    keep = allowed(groups, B)
    keep_r, keep_c = keep, keep
    if drop_last:
        keep_r, keep_c = keep.clone(), keep.clone()
        keep_r[:, B - 1] = False
        keep_c[B - 1, :] = False
    d = torch.diagonal(z)
    return ((_lse(z, keep_r, 1) - d).sum() + (_lse(z, keep_c, 0) - d).sum()) / (2 * B)


def infonce_loss_and_grad(S, groups, scale, dtype=torch.float64, upstream=1.0):
    """-> (loss, dS = upstream * dloss/dS) by the closed form above, in `dtype`."""
    B = S.shape[0]
    z = S.to(dtype) * torch.tensor(scale, dtype=dtype)
    keep = allowed(groups, B)
    rl, cl = _lse(z, keep, 1), _lse(z, keep, 0)
    d = torch.diagonal(z)
    loss = ((rl - d).sum() + (cl - d).sum()) / (2 * B)
    coef = torch.tensor(upstream, dtype=dtype) * (torch.tensor(scale, dtype=dtype) / (2 * B))
    p = torch.exp(z - rl[:, None]) + torch.exp(z - cl[None, :]) - 2.0 * torch.eye(B, dtype=dtype)
    return loss, torch.where(keep, coef * p, torch.zeros_like(p))


def draw_groups(B, rng):
    """tests/test_hinge_groups_gpu.py::draw_groups: about a tenth of the rows (at least two) share their group with another row, in
    clusters of 3, 2, 4, 2, ... rows at random positions; every other row is alone.  Group values are arbitrary integers."""
    groups = rng.permutation(B).astype(np.int64) * 3 + 11
    shared = rng.permutation(B)[:min(B, max(2, int(round(B / 10.0))))] if B >= 2 else []
    at, k = 0, 0
    while at < len(shared):
        size = (3, 2, 4, 2)[k % 4]
        if len(shared) - at - size == 1:          # nobody is left alone
            size += 1
        groups[shared[at:at + size]] = -(k + 1)
        at, k = at + size, k + 1
    return groups


def make_case(B, amp, grouped):
    """-> (S float32 [B, B], groups or None).  S = amp * rand, plus 0.25 * amp on the last row and the last column, so that the last
    index carries weight in every row sum and every column sum."""
    g = torch.Generator().manual_seed(1000 * B + int(amp))
    S = torch.rand(B, B, generator=g) * amp
    S[-1, :] += 0.25 * amp
    S[:, -1] += 0.25 * amp
    return S, (draw_groups(B, np.random.RandomState(B)) if grouped else None)


_REF = {}


def reference(B, amp, grouped):
    """-> dict(S, groups, scale, loss=(want64, e32, tol), dS=(want64, e32, tol)); computed once per case and shared."""
    key = (B, amp, grouped)
    if key not in _REF:
        S, groups = make_case(B, amp, grouped)
        scale = scale_of(TEMPERATURE)
        l64, d64 = infonce_loss_and_grad(S, groups, scale, torch.float64, UPSTREAM)
        l32, d32 = infonce_loss_and_grad(S, groups, scale, torch.float32, UPSTREAM)
        out = dict(S=S, groups=groups, scale=scale)
        for name, w64, w32 in (("loss", l64, l32), ("dS", d64, d32)):
            e32 = float((w32.double() - w64).abs().max())
            out[name] = (w64, e32, FACTOR * max(e32, U * float(w64.abs().max())))
        _REF[key] = out
    return _REF[key]
