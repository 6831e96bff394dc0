"""float64 restatement of the bidirectional hinge with same-group entries masked (ops.hinge_loss(groups=...)), torch autograd on
the CPU.  Both cost matrices of the reference's loss (Objectives.py:93-115) get masked_fill(diagonal OR same group, 0), then max or
sum.  The max is taken at the FIRST index of the largest cost (the reference's torch.max on the CPU returns the first too; it is
spelled out here so the tie rule does not depend on the torch build).

flip_distance() is the test's precondition: how far the float64 loss is from a discrete change (a hinge at its kink, a change of
a row's or column's arg-max), to be compared with what fp32 rounding can move a cost by."""
import numpy as np
import torch

# what fp32 evaluation of (margin + s) - d can differ from the exact value by, for |margin + s| < 2 and |result| < 2:
# the two roundings (half an ulp of a value in [1, 2) each: 2^-24) and the fp32 margin (|0.2f - 0.2| < 2^-28)
FP32_COST_ERR = 2.0 ** -23 + 2.0 ** -28


def same_group(groups):
    g = torch.as_tensor(np.asarray(groups, dtype=np.int64))
    return g.view(-1, 1) == g.view(1, -1)            # includes the diagonal


def _first_max(cost, dim):
    """sum over the other dim of cost at the first index of its maximum along `dim`; the gradient follows that index alone."""
    top = cost.max(dim, keepdim=True)[0]
    is_top = cost == top
    first = is_top & (is_top.to(torch.int64).cumsum(dim) == 1)
    idx = first.to(torch.int64).argmax(dim, keepdim=True)       # exactly one True per line
    return cost.gather(dim, idx).sum(), idx.squeeze(dim)


def costs(scores, groups, margin):
    n = scores.shape[0]
    s = scores.double()
    diag = s.diag().view(n, 1)
    masked = same_group(groups)
    cost_s = (margin + s - diag).clamp(min=0).masked_fill(masked, 0)
    cost_im = (margin + s - diag.t()).clamp(min=0).masked_fill(masked, 0)
    return cost_s, cost_im


def hinge_groups_loss(scores, groups, margin=0.2, max_violation=False):
    cost_s, cost_im = costs(scores, groups, margin)
    if max_violation:
        return _first_max(cost_s, 1)[0] + _first_max(cost_im, 0)[0]
    return cost_s.sum() + cost_im.sum()


def hinge_groups_loss_and_grad(scores, groups, margin=0.2, max_violation=False):
    """-> (loss, dS), float64."""
    with torch.enable_grad():
        s = scores.detach().double().clone().requires_grad_(True)
        loss = hinge_groups_loss(s, groups, margin, max_violation)
        loss.backward()
    return loss.detach(), s.grad.detach()


def hinge_groups_args(scores, groups, margin=0.2):
    """(row_arg, col_arg) of the max form: first index of the largest cost of every row / column after masking; -1 for a row / column
    without a violator (all costs 0: which index stands there carries no meaning, as long as it is not a masked one)."""
    cost_s, cost_im = costs(scores.detach(), groups, margin)
    none = torch.full((scores.shape[0],), -1, dtype=torch.int64)
    return (torch.where(cost_s.max(1)[0] > 0, _first_max(cost_s, 1)[1], none),
            torch.where(cost_im.max(0)[0] > 0, _first_max(cost_im, 0)[1], none))


def args_agree(got, want):
    """got: the kernel's arg vector; want: hinge_groups_args'.  Equal wherever there is a violator."""
    got = got.detach().cpu().to(torch.int64)
    return bool(((got == want) | (want < 0)).all())


def flip_distance(scores, groups, margin=0.2, max_violation=False):
    """Smallest change of a single cost (float64) that changes dS: sum form -- the distance of any unmasked raw hinge from 0;
    max form -- per row / column, the gap between the largest cost and the next DIFFERENT cost (entries that tie exactly tie in
    every precision: equal scores), and the distance of the largest raw hinge from 0."""
    n = scores.shape[0]
    s = scores.detach().double()
    diag = s.diag().view(n, 1)
    masked = same_group(groups)
    best = float('inf')
    for raw, dim in ((margin + s - diag, 1), (margin + s - diag.t(), 0)):
        if not max_violation:
            r = raw.abs().masked_fill(masked, float('inf'))
            best = min(best, float(r.min()))
            continue
        r = raw.masked_fill(masked, -float('inf'))
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
