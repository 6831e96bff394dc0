"""Float64 restatement of the two losses on batch u memory (csrc/xbm_loss.hip; include/itr_hip.h: itr_xbm_*), torch autograd on the
CPU, and the case table their CPU and GPU tests share.  Nothing here imports the library or follows the kernels' structure: the
candidates are concatenated, dropped entries are masked, the first maximum is spelled out (hinge_groups_oracle._first_max) and the
log-sum-exp is torch.logsumexp over the kept entries.

    S [B, B] image i vs caption j;  R [B, n] image i vs memory caption k;  C [n, B] memory image k vs caption j
    row i's candidates: S[i, :] then R[i, :];  column j's: S[:, j] then C[:, j]
    dropped: S (i, j), i != j, iff mask_batch and groups[i] == groups[j];  R (i, k) iff groups[i] == bank_groups[k];
             C (k, j) iff bank_groups[k] == groups[j]

Run in float32 (dtype=torch.float32) the same statements give the reference's own rounding error e32; the tolerance of a compared
tensor is the primary rule of tests/helpers/train_prim_cases.py: FACTOR * max(e32, U * max|want|)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_groups_oracle as HG  # noqa: E402
from infonce_oracle import draw_groups, scale_of  # noqa: E402
from train_prim_cases import FACTOR, SENSITIVITY, U  # noqa: E402,F401

TEMPERATURE = 0.05
MARGIN = 0.2
UPSTREAM = 3.0
AMPLITUDES = [1.0, 30.0]          # InfoNCE: z within 25; z up to ~750, where exp without its maximum overflows fp32
MAX_SEEDS = 8

# the seams of the geometry that is built (csrc/xbm_loss.hip), T = B + n the candidates of a row / column:
SEAMS = {
    "B: one lane, one wave of a column group (64) and its neighbours, two groups, five groups": [1, 2, 63, 64, 65, 128, 257],
    "n: memory of one slot; T around the wave stride of the row pass (64, 128) and its unroll (512)": [1, 63, 64, 65, 255, 257],
    "T < 16: one slice; 16 <= T < 2048: ceil(T / 16) slices; T >= 2048: 128 slices (B <= 256) or ceil(512 / 5) = 103 (B = 257)": [(2, 1), (63, 64), (128, 4099), (257, 4099)],
    "slice boundary inside S, on the S / C border (B a multiple of the slice rows) and inside C": [(65, 63), (64, 1000), (2, 257)],
    "backward: B (B + n) and n B below, around and far above one block of 1024 entries": [(2, 63), (63, 1), (65, 255), (257, 4099)],
}
CASES = [(1, 1), (1, 4099), (2, 1), (2, 63), (2, 257), (63, 1), (63, 64), (64, 65), (64, 1000), (65, 63), (65, 255), (128, 64),
         (128, 1000), (128, 4099), (257, 257), (257, 1000), (257, 4099)]
KINDS = [("hinge_sum", 1.0), ("hinge_max", 1.0), ("infonce", 1.0), ("infonce", 30.0)]


def kept(groups, bank_groups, mask_batch):
    """-> bool (keepS [B, B] with the diagonal True, keepR [B, n], keepC [n, B])"""
    g = torch.as_tensor(np.asarray(groups, dtype=np.int64))
    b = torch.as_tensor(np.asarray(bank_groups, dtype=np.int64))
    B = g.shape[0]
    eye = torch.eye(B, dtype=torch.bool)
    keep_s = ((g[:, None] != g[None, :]) | eye) if mask_batch else torch.ones(B, B, dtype=torch.bool)
    keep_r = g[:, None] != b[None, :]
    return keep_s, keep_r, keep_r.t().clone()


def _hinge_costs(S, R, C, groups, bank_groups, margin, mask_batch):
    """-> (raw_row [B, B + n], raw_col [B + n, B], off_row, off_col): raw hinges (margin + s) - d and where they cost nothing"""
    B = S.shape[0]
    keep_s, keep_r, keep_c = kept(groups, bank_groups, mask_batch)
    eye = torch.eye(B, dtype=torch.bool)
    d = torch.diagonal(S)
    raw_row = (margin + torch.cat([S, R], 1)) - d[:, None]
    raw_col = (margin + torch.cat([S, C], 0)) - d[None, :]
    return raw_row, raw_col, torch.cat([~keep_s | eye, ~keep_r], 1), torch.cat([~keep_s | eye, ~keep_c], 0)


def hinge_loss(S, R, C, groups, bank_groups, margin=MARGIN, max_violation=False, mask_batch=False, dtype=torch.float64):
    """0-dim loss of `dtype`, differentiable w.r.t. S, R and C (used as they are when they already have `dtype`)."""
    S, R, C = S.to(dtype), R.to(dtype), C.to(dtype)
    raw_row, raw_col, off_row, off_col = _hinge_costs(S, R, C, groups, bank_groups, margin, mask_batch)
    cost_row = raw_row.clamp(min=0).masked_fill(off_row, 0)
    cost_col = raw_col.clamp(min=0).masked_fill(off_col, 0)
    if max_violation:
        return HG._first_max(cost_row, 1)[0] + HG._first_max(cost_col, 0)[0]
    return cost_row.sum() + cost_col.sum()


def hinge_args(S, R, C, groups, bank_groups, margin=MARGIN, mask_batch=False):
    """(row_arg, col_arg) of the max form in [0, B + n); -1 where the row / column has no violator."""
    raw_row, raw_col, off_row, off_col = _hinge_costs(S.double(), R.double(), C.double(), groups, bank_groups, margin, mask_batch)
    cost_row = raw_row.clamp(min=0).masked_fill(off_row, 0)
    cost_col = raw_col.clamp(min=0).masked_fill(off_col, 0)
    none = torch.full((S.shape[0],), -1, dtype=torch.int64)
    return (torch.where(cost_row.max(1)[0] > 0, HG._first_max(cost_row, 1)[1], none),
            torch.where(cost_col.max(0)[0] > 0, HG._first_max(cost_col, 0)[1], none))


def hinge_counts(S, R, C, groups, bank_groups, margin=MARGIN, mask_batch=False):
    """(violators of every row, of every column): what the sum form's forward leaves in row_arg / col_arg"""
    raw_row, raw_col, off_row, off_col = _hinge_costs(S.double(), R.double(), C.double(), groups, bank_groups, margin, mask_batch)
    return ((raw_row > 0) & ~off_row).sum(1), ((raw_col > 0) & ~off_col).sum(0)


def flip_distance(S, R, C, groups, bank_groups, margin=MARGIN, max_violation=False, mask_batch=False):
    """hinge_groups_oracle.flip_distance for the three matrices: the smallest change of one cost (float64) that changes a gradient.
    Sum form: the distance of any kept raw hinge from 0.  Max form: per row / column, the gap between the largest cost and the next
    different one, and the distance of the largest raw hinge from 0."""
    raw_row, raw_col, off_row, off_col = _hinge_costs(S.double(), R.double(), C.double(), groups, bank_groups, margin, mask_batch)
    best = float('inf')
    for raw, off, dim in ((raw_row, off_row, 1), (raw_col, off_col, 0)):
        if not max_violation:
            r = raw.abs().masked_fill(off, float('inf'))
            if r.numel():
                best = min(best, float(r.min()))
            continue
        r = raw.masked_fill(off, -float('inf'))
        top = r.max(dim, keepdim=True)[0]
        live = torch.isfinite(top)
        if not bool(live.any()):
            continue
        best = min(best, float(top[live].abs().min()))
        c = r.clamp(min=0)
        ctop = c.max(dim, keepdim=True)[0]
        lower = c.masked_fill(c == ctop, -float('inf')).max(dim, keepdim=True)[0]
        gap = (ctop - lower)[torch.isfinite(lower) & live]
        if gap.numel():
            best = min(best, float(gap.min()))
    return best


def infonce_parts(S, R, C, groups, bank_groups, scale, mask_batch=False, dtype=torch.float64):
    """-> (loss, row_lse, col_lse) of `dtype`, differentiable w.r.t. S, R and C."""
    B = S.shape[0]
    sc = torch.tensor(scale, dtype=dtype)
    zs, zr, zc = S.to(dtype) * sc, R.to(dtype) * sc, C.to(dtype) * sc
    keep_s, keep_r, keep_c = kept(groups, bank_groups, mask_batch)
    ninf = -float('inf')
    row_lse = torch.logsumexp(torch.cat([zs.masked_fill(~keep_s, ninf), zr.masked_fill(~keep_r, ninf)], 1), 1)
    col_lse = torch.logsumexp(torch.cat([zs.masked_fill(~keep_s, ninf), zc.masked_fill(~keep_c, ninf)], 0), 0)
    d = torch.diagonal(zs)
    return ((row_lse - d).sum() + (col_lse - d).sum()) / (2 * B), row_lse, col_lse


def loss_of(kind, S, R, C, groups, bank_groups, mask_batch, dtype=torch.float64):
    if kind == "infonce":
        return infonce_parts(S, R, C, groups, bank_groups, scale_of(TEMPERATURE), mask_batch, dtype)[0]
    return hinge_loss(S, R, C, groups, bank_groups, MARGIN, kind == "hinge_max", mask_batch, dtype)


def loss_and_grads(kind, S, R, C, groups, bank_groups, mask_batch, dtype=torch.float64, upstream=UPSTREAM):
    """-> (loss, dS, dR, dC) of `dtype` by autograd, the gradients times `upstream`."""
    with torch.enable_grad():
        leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (S, R, C)]
        loss = loss_of(kind, leaves[0], leaves[1], leaves[2], groups, bank_groups, mask_batch, dtype)
        (loss * upstream).backward()
    return (loss.detach(),) + tuple(t.grad.detach() for t in leaves)


def draw_bank_groups(B, n, groups, rng):
    """Every slot an image of its own, then about a tenth of the slots (at least two when n >= 2; never the last slot when n >= 2)
    hold captions of images that are in the batch too -- the clustered ones first, so that one batch group meets several slots."""
    bank = 1000003 + 7 * rng.permutation(n).astype(np.int64)
    if n >= 2:
        slots = rng.permutation(n - 1)[:min(n - 1, max(2, int(round(n / 10.0))))]
        order = np.argsort(groups, kind='stable')          # clustered batch groups are negative: they come first
        for q, k in enumerate(slots):
            bank[k] = groups[order[q % B]]
    return bank


def make_case(B, n, amp, seed=0):
    """-> (S, R, C float32, groups [B], bank_groups [n]).  Scores are amp * rand; a quarter of the amplitude is added to the last row
    and column of S, to the last slot's column of R and to its row of C, so that the last index carries weight everywhere."""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * B + n + int(amp))
    S, R, C = torch.rand(B, B, generator=g) * amp, torch.rand(B, n, generator=g) * amp, torch.rand(n, B, generator=g) * amp
    S[-1, :] += 0.25 * amp
    S[:, -1] += 0.25 * amp
    R[:, -1] += 0.25 * amp
    C[-1, :] += 0.25 * amp
    rng = np.random.RandomState(17 * B + n)
    groups = draw_groups(B, rng)
    return S, R, C, groups, draw_bank_groups(B, n, groups, rng)


_REF = {}


def _measure(S, R, C, groups, bank_groups, kind, mask_batch):
    """-> dict(loss / dS / dR / dC = (want64, e32, tol)) of one draw"""
    w64 = loss_and_grads(kind, S, R, C, groups, bank_groups, mask_batch, torch.float64)
    w32 = loss_and_grads(kind, S, R, C, groups, bank_groups, mask_batch, torch.float32)
    out = {}
    for name, a, b in zip(("loss", "dS", "dR", "dC"), w64, w32):
        e32 = float((b.double() - a).abs().max()) if a.numel() else 0.0
        out[name] = (a, e32, FACTOR * max(e32, U * (float(a.abs().max()) if a.numel() else 0.0)))
    return out


def last_slot_move(ref, kind, mask_batch):
    """how far the float64 loss moves when the last memory slot is left out"""
    n = ref["R"].shape[1]
    short = loss_of(kind, ref["S"], ref["R"][:, :n - 1], ref["C"][:n - 1], ref["groups"], ref["bank_groups"][:n - 1], mask_batch)
    return abs(float(short) - float(ref["loss"][0]))


def reference(B, n, kind, amp, mask_batch):
    """-> dict(S, R, C, groups, bank_groups, flip, seed, loss / dS / dR / dC = (want64, e32, tol)); computed once and shared.
    The draw is make_case at the first of MAX_SEEDS seeds that can tell a wrong kernel from a right one: every hinge decision lies
    further than fp32 rounding from a flip, and the loss moves by more than SENSITIVITY tolerances when the last memory slot is left
    out (at B = 1 the positive carries both quarters of the amplitude, and at amplitude 30 a softmax is decided by its largest term:
    not every draw gives the last slot weight).  Both conditions look at the inputs and the float64 / float32 helper only."""
    key = (B, n, kind, amp, bool(mask_batch))
    if key not in _REF:
        for seed in range(MAX_SEEDS):
            S, R, C, groups, bank_groups = make_case(B, n, amp, seed)
            flip = float('inf') if kind == "infonce" else flip_distance(S, R, C, groups, bank_groups, MARGIN, kind == "hinge_max", mask_batch)
            out = dict(S=S, R=R, C=C, groups=groups, bank_groups=bank_groups, flip=flip, seed=seed)
            if flip <= HG.FP32_COST_ERR:
                continue
            out.update(_measure(S, R, C, groups, bank_groups, kind, mask_batch))
            if last_slot_move(out, kind, mask_batch) > SENSITIVITY * out["loss"][2]:
                break
        if "loss" not in out:
            out.update(_measure(S, R, C, groups, bank_groups, kind, mask_batch))
        _REF[key] = out
    return _REF[key]


def case_id(B, n, kind, amp, mask_batch):
    return "B%d-n%d-%s-amp%g-%s" % (B, n, kind, amp, "mask" if mask_batch else "nomask")


SWEEP = [(B, n, kind, amp, mask) for (B, n) in CASES for (kind, amp) in KINDS for mask in (False, True)]
