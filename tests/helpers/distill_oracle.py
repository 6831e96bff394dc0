"""Float64 restatement of the score-distillation loss of csrc/distill.hip (include/itr_hip.h: itr_distill_fwd / _bwd), plain torch on
the CPU, and the case table its CPU and GPU tests share.  Nothing here imports the library.

    z_s = scale_s * S, z_t = scale_t * T,  scale = float(np.float32(1 / temperature)) -- the factors the op hands to the kernels
    p_row[i,:] = softmax_j z_t[i,:]     q_row[i,:] = softmax_j z_s[i,:]     p_col[:,j] = softmax_i z_t[:,j]     q_col[:,j] = softmax_i z_s[:,j]
    KL_row[i] = sum_j p_row[i,j] (z_t[i,j] - z_s[i,j]) - (lse_t_row[i] - lse_s_row[i])         (KL_col[j] alike, over i)
    loss = (sum_i KL_row[i] + sum_j KL_col[j]) / (2 B)
    dS[i,j] = g scale_s / (2 B) ((q_row - p_row)[i,j] + (q_col - p_col)[i,j])

The decomposition is the kernel's -- cross term minus the difference of the two log-sum-exps, not sum p log(p / q) -- so that the same
statements run in float32 (dtype=torch.float32) give the rounding error e32 of that arithmetic.  Tolerances, the primary rule of
tests/helpers/train_prim_cases.py:
    dS and the four log-sum-exp vectors    FACTOR * max(e32, U * max|want|)
    loss                                   FACTOR * max(e32, U * (max|z_s| + max|z_t|))
The loss is a difference of three terms of size up to max|z_s| + max|z_t| (the cross term and the two log-sum-exps), so its floor is
the rounding of that size, not of the small difference that is left."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_prim_cases import FACTOR, U  # noqa: E402,F401

TEMPERATURE = 0.05
UPSTREAM = 3.0
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1024]      # wave and workgroup strides, their neighbours, one global-batch size
AMPLITUDES = [1.0, 30.0]                                  # z within 25; z up to ~750, where exp without its maximum overflows fp32
CASES = [(B, amp_s, amp_t) for B in SIZES for amp_s in AMPLITUDES for amp_t in AMPLITUDES]
VECTORS = ("row_lse_s", "col_lse_s", "row_lse_t", "col_lse_t")


def scale_of(temperature):
    return float(np.float32(1.0 / float(temperature)))


def _keeps(B, drop_last):
    """(rows' kept entries, columns' kept entries), bool [B, B].  drop_last: the row sums lose column B - 1 and the column sums lose
    row B - 1 -- the defect of a kernel that stops one index early."""
    keep_r, keep_c = torch.ones(B, B, dtype=torch.bool), torch.ones(B, B, dtype=torch.bool)
    if drop_last:
        keep_r[:, B - 1] = False
        keep_c[B - 1, :] = False
    return keep_r, keep_c


def _lse(z, keep, dim):
    """log sum exp over the kept entries along `dim`, relative to their maximum"""
    m = torch.where(keep, z, z.min().expand_as(z)).max(dim, keepdim=True).values
    s = torch.where(keep, torch.exp(torch.where(keep, z, m.expand_as(z)) - m), torch.zeros_like(z)).sum(dim, keepdim=True)
    return (m + torch.log(s)).squeeze(dim)


def _side(zs, zt, keep, dim):
    """One direction -> (KL [B], lse_s [B], lse_t [B], q - p [B, B], zero at left-out entries)."""
    ls, lt = _lse(zs, keep, dim), _lse(zt, keep, dim)
    zero = torch.zeros_like(zs)
    p = torch.where(keep, torch.exp(zt - lt.unsqueeze(dim)), zero)
    q = torch.where(keep, torch.exp(zs - ls.unsqueeze(dim)), zero)
    cross = (p * (zt - zs)).sum(dim)
    return cross - (lt - ls), ls, lt, q - p


def distill_parts(S, T, scale_s, scale_t, dtype=torch.float64, upstream=1.0, drop_last=False):
    """-> dict(loss, dS = upstream * dloss/dS by the closed form, row_lse_s, col_lse_s, row_lse_t, col_lse_t), all in `dtype`.
    The loss is built from differentiable torch operations on S."""
    B = S.shape[0]
    zs = S.to(dtype) * torch.tensor(scale_s, dtype=dtype)
    zt = T.detach().to(dtype) * torch.tensor(scale_t, dtype=dtype)
    keep_r, keep_c = _keeps(B, drop_last)
    kl_r, rls, rlt, d_r = _side(zs, zt, keep_r, 1)
    kl_c, cls, clt, d_c = _side(zs, zt, keep_c, 0)
    loss = (kl_r.sum() + kl_c.sum()) / (2 * B)
    coef = torch.tensor(upstream, dtype=dtype) * (torch.tensor(scale_s, dtype=dtype) / (2 * B))
    return dict(loss=loss, dS=(coef * (d_r + d_c)).detach(), row_lse_s=rls.detach(), col_lse_s=cls.detach(), row_lse_t=rlt.detach(),
                col_lse_t=clt.detach())


def distill_loss(S, T, scale_s, scale_t, dtype=torch.float64, drop_last=False):
    """The loss (0-dim tensor of `dtype`), differentiable w.r.t. S."""
    return distill_parts(S, T, scale_s, scale_t, dtype, 1.0, drop_last)["loss"]


def distill_loss_and_grad(S, T, scale_s, scale_t, dtype=torch.float64, upstream=1.0, drop_last=False):
    """-> (loss, dS = upstream * dloss/dS) by the closed forms above, in `dtype`."""
    parts = distill_parts(S, T, scale_s, scale_t, dtype, upstream, drop_last)
    return parts["loss"].detach(), parts["dS"]


def loss_tolerance(e32, S, T, scale_s, scale_t):
    size = float(S.abs().max()) * scale_s + float(T.abs().max()) * scale_t
    return FACTOR * max(e32, U * size)


def make_case(B, amp_s, amp_t):
    """-> (S, T) float32 [B, B]: independent amp * rand draws, each plus 0.25 * amp on the last row and the last column, so that the
    last index carries weight in every row sum and every column sum of both matrices."""
    out = []
    for k, amp in enumerate((amp_s, amp_t)):
        g = torch.Generator().manual_seed(1000 * B + int(amp) + 500000 * k)
        X = torch.rand(B, B, generator=g) * amp
        X[-1, :] += 0.25 * amp
        X[:, -1] += 0.25 * amp
        out.append(X)
    return out[0], out[1]


def tolerances(S, T, scale_s, scale_t, upstream=UPSTREAM, drop_last=False):
    """-> dict name -> (want64, e32, tol) for loss, dS and the four saved vectors."""
    p64 = distill_parts(S, T, scale_s, scale_t, torch.float64, upstream, drop_last)
    p32 = distill_parts(S, T, scale_s, scale_t, torch.float32, upstream, drop_last)
    out = {}
    for name in ("loss", "dS") + VECTORS:
        w64 = p64[name].detach()
        e32 = float((p32[name].detach().double() - w64).abs().max())
        tol = loss_tolerance(e32, S, T, scale_s, scale_t) if name == "loss" else FACTOR * max(e32, U * float(w64.abs().max()))
        out[name] = (w64, e32, tol)
    return out


_REF = {}


def reference(B, amp_s, amp_t):
    """-> dict(S, T, scale_s, scale_t, loss=(want64, e32, tol), dS=..., row_lse_s=..., ...); computed once per case and shared."""
    key = (B, amp_s, amp_t)
    if key not in _REF:
        S, T = make_case(B, amp_s, amp_t)
        scale = scale_of(TEMPERATURE)
        out = dict(S=S, T=T, scale_s=scale, scale_t=scale)
        out.update(tolerances(S, T, scale, scale))
        _REF[key] = out
    return _REF[key]
