"""GPU: the hinge with same-group entries masked (csrc/hinge.hip: itr_hinge_groups_fwd / _bwd; ops.hinge_loss(groups=...)) against
the float64 helper (tests/helpers/hinge_groups_oracle.py).

Bounds.  Loss: 1e-4 * max(1, loss64), the bound of test_kernels_gpu.py::test_hinge_random for the unmasked kernel on the same kind of
input.  dS: exactly the helper's (every entry is a small integer times the upstream gradient 3.0).

Precondition of the exact comparison.  The kernel evaluates (margin + s) - d in fp32, the helper in float64, so a cost differs by up to
H.FP32_COST_ERR (two roundings of values below 2, and the fp32 margin); dS can only differ where the float64 loss is closer than that
to a discrete change -- a hinge at its kink, or two different costs of a row / column closer than twice that competing for the
arg-max.  H.flip_distance measures that distance on the float64 side alone; a seed whose matrix comes closer than 2 x FP32_COST_ERR is
unsuitable, and the test says so instead of comparing.  SEEDS holds, per size, the first seed from B upwards that is suitable for
both forms (B = 1024, sum form: two million hinges with a density of ~0.8 per unit near the kink, so about every other seed is).

Sizes: 1, 2, the wave (64) and workgroup (256) strides of the kernels' loops and their neighbours, 300, and one global-batch size."""
import os
import sys

import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hinge_groups_oracle as H  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 0.2
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1024]
SEEDS = {1: 1, 2: 2, 63: 63, 64: 64, 65: 65, 255: 255, 256: 256, 257: 257, 300: 300, 1024: 1024}


def draw_groups(B, rng):
    """About a tenth of the rows (at least two) share their group with another row: clusters of 3, 2, 4, 2, 3, ... rows at random
    positions; every other row is alone in its group.  Group values are arbitrary integers, not 0 .. B-1."""
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


def make_case(B, seed):
    torch.manual_seed(seed)
    sc = torch.rand(B, B)
    return sc, draw_groups(B, np.random.RandomState(seed))


@pytest.fixture(scope="module")
def cases():
    """B -> (scores, groups, {mv: (loss64, dS64, flip distance)}), each computed once."""
    cache = {}

    def get(B):
        if B not in cache:
            sc, groups = make_case(B, SEEDS[B])
            ref = {mv: H.hinge_groups_loss_and_grad(sc, groups, MARGIN, mv) + (H.flip_distance(sc, groups, MARGIN, mv),) for mv in (False, True)}
            cache[B] = (sc, groups, ref)
        return cache[B]
    return get


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def run(sc, groups, mv, dev, upstream=3.0):
    s = sc.to(dev).requires_grad_(True)
    loss = ops.hinge_loss(s, MARGIN, mv, groups=groups)
    (loss * upstream).backward()
    return loss.detach(), s.grad


def check(sc, groups, mv, dev, ref=None, what=""):
    want_l, want_g, flip = ref if ref is not None else H.hinge_groups_loss_and_grad(sc, groups, MARGIN, mv) + (H.flip_distance(sc, groups, MARGIN, mv),)
    assert flip > 2 * H.FP32_COST_ERR, "%s: unsuitable input, the float64 loss is %.2e from a discrete change" % (what, flip)
    loss, grad = run(sc, groups, mv, dev)
    err = abs(float(loss) - float(want_l))
    print("\n%s mv=%s: loss %.6f vs %.6f (err %.2e, bound %.2e), flip distance %.2e" % (what, mv, float(loss), float(want_l), err,
                                                                                     1e-4 * max(1.0, float(want_l)), flip))
    assert err <= 1e-4 * max(1.0, float(want_l))
    assert torch.equal(grad.cpu().double(), want_g * 3.0), "%s: dS differs at %d entries" % (what, int((grad.cpu().double() != want_g * 3.0).sum()))
    return loss, grad


# ------------------------------------------------------------------------------------------ the size sweep
def test_groups_are_drawn_as_described():
    for B in SIZES[2:]:
        g = draw_groups(B, np.random.RandomState(SEEDS[B]))
        _, counts = np.unique(g, return_counts=True)
        n_shared = int(counts[counts > 1].sum())
        assert abs(n_shared - B / 10.0) <= 1.0 and counts.max() >= (3 if B >= 63 else 2) and (counts == 1).sum() == B - n_shared, (B, counts)


@pytest.mark.parametrize("mv", [False, True])
@pytest.mark.parametrize("B", SIZES)
def test_sweep_vs_float64(cases, dev, B, mv):
    sc, groups, ref = cases(B)
    _, grad = check(sc, groups, mv, dev, ref[mv], "B=%d" % B)
    masked = H.same_group(groups) & ~torch.eye(B, dtype=torch.bool)
    assert B < 3 or int(masked.sum()) >= 2
    assert float(grad.cpu()[masked].abs().max() if masked.any() else 0.0) == 0.0


# ------------------------------------------------------------------------------------------ (a) bit identity without collisions
@pytest.mark.parametrize("mv", [False, True])
@pytest.mark.parametrize("B", [1, 2, 65, 257, 300])
def test_distinct_groups_are_bit_identical_to_the_unmasked_kernels(dev, B, mv):
    torch.manual_seed(B)
    s = torch.rand(B, B).to(dev)
    if B > 2:
        d = float(s[3, 3])
        s[3] = d - 0.5               # a row without violators: the arg falls to index 0 on both sides
        s[3, 3] = d
    groups = np.random.RandomState(B).permutation(B) * 5 - 7
    l0, ra0, ca0 = ops.hinge_fwd(s, MARGIN, mv)
    l1, ra1, ca1 = ops.hinge_fwd(s, MARGIN, mv, groups=groups)
    assert torch.equal(bits(l0), bits(l1))
    if mv:
        assert torch.equal(ra0, ra1) and torch.equal(ca0, ca1)
    g = torch.full((1,), 3.0, device=dev)
    d0 = ops.hinge_bwd(s, MARGIN, mv, ra0, ca0, g)
    d1 = ops.hinge_bwd(s, MARGIN, mv, ra1, ca1, g, groups=groups)
    assert torch.equal(bits(d0), bits(d1))
    # and through autograd
    a, b = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
    (ops.hinge_loss(a, MARGIN, mv) * 3.0).backward()
    (ops.hinge_loss(b, MARGIN, mv, groups=groups) * 3.0).backward()
    assert torch.equal(bits(a.grad), bits(b.grad))


# ------------------------------------------------------------------------------------------ (b) the hardest entries are the masked ones
@pytest.mark.parametrize("mv", [False, True])
def test_hardest_entries_masked(dev, mv):
    """Same-group pairs whose entries are the largest of their rows and columns (raw score + 1), at index 0, at index B - 1 and next
    to the diagonal: the arg-max skips them, the loss is the helper's -- and not the unmasked loss of the same matrix."""
    B = 70
    torch.manual_seed(70)
    sc = torch.rand(B, B)
    groups = np.arange(B) + 100
    pairs = [(7, 0), (20, B - 1), (30, 31), (65, 64)]
    for i, j in pairs:
        groups[j] = groups[i]
        sc[i, j] += 1.0
        sc[j, i] += 1.0
    for i, j in pairs + [(j, i) for i, j in pairs]:
        assert float(sc[i, j]) == float(sc[i].max()) == float(sc[:, j].max())
    loss, _ = check(sc, groups, mv, dev, what="hardest masked")
    _, ra, ca = ops.hinge_fwd(sc.to(dev), MARGIN, True, groups=groups)
    want_ra, want_ca = H.hinge_groups_args(sc, groups, MARGIN)
    assert H.args_agree(ra, want_ra) and H.args_agree(ca, want_ca)
    assert int((want_ra >= 0).sum()) >= 4 and int((want_ca >= 0).sum()) >= 4
    for i, j in pairs + [(j, i) for i, j in pairs]:
        assert int(ra[i]) != j and int(ca[j]) != i
    gt = torch.as_tensor(groups)
    idx = torch.arange(B)
    for arg in (ra.cpu().long(), ca.cpu().long()):
        assert bool(((gt[arg] != gt) | (arg == idx)).all())          # never a masked index
    # the reference's loss on the same matrix mines exactly these entries
    unmasked = ops.hinge_loss(sc.to(dev), MARGIN, mv)
    want_unmasked = float(O.hinge_loss(sc.double(), MARGIN, mv))
    assert abs(float(unmasked) - want_unmasked) <= 1e-4 * max(1.0, want_unmasked)
    assert float(unmasked) - float(loss) > 1.0
    _, ra_u, _ = ops.hinge_fwd(sc.to(dev), MARGIN, True)
    assert [int(ra_u[i]) for i, _ in pairs] == [j for _, j in pairs]


# ------------------------------------------------------------------------------------------ (c) only the masked entries violate
@pytest.mark.parametrize("mv", [False, True])
def test_only_violators_masked(dev, mv):
    """Row 9 and column 9 violate the margin only at their entries with pair 0, which shares their group: they contribute nothing,
    and the backward does not invent a gradient from the forward's fall-back arg (the lowest index, which here is the masked one)."""
    B = 66
    torch.manual_seed(66)
    sc = torch.rand(B, B) * 0.5
    sc.fill_diagonal_(1.0)
    sc[9, 0] = sc[0, 9] = 1.5                      # raw hinge 0.7 for row 9 / column 0 and for row 0 / column 9
    sc[20, 40] = 0.95                              # one real violation elsewhere, so the loss is not 0
    groups = np.arange(B)
    groups[9] = groups[0]
    loss, grad = check(sc, groups, mv, dev, what="only violators masked")
    assert float(loss) == pytest.approx(2 * 0.15, abs=1e-6)
    g = grad.cpu()
    for r in (0, 9):
        assert float(g[r].abs().max()) == 0.0 and float(g[:, r].abs().max()) == 0.0
    assert float(ops.hinge_loss(sc.to(dev), MARGIN, mv)) > float(loss) + 2.0      # the unmasked loss counts them
    # the backward checks the mask itself: arg vectors that name the masked entries (as a forward without the mask writes them)
    s = sc.to(dev)
    _, ra_u, ca_u = ops.hinge_fwd(s, MARGIN, True)
    assert int(ra_u[9]) == 0 and int(ca_u[9]) == 0 and int(ra_u[0]) == 9 and int(ca_u[0]) == 9
    dS = ops.hinge_bwd(s, MARGIN, True, ra_u, ca_u, torch.ones(1, device=dev), groups=groups).cpu()
    for r in (0, 9):
        assert float(dS[r].abs().max()) == 0.0 and float(dS[:, r].abs().max()) == 0.0


@pytest.mark.parametrize("mv", [False, True])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_one_group_batch_is_zero(dev, B, mv):
    torch.manual_seed(B)
    sc = torch.rand(B, B)
    loss, grad = run(sc, [7] * B, mv, dev)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ (d) ties, group values, input kinds
def test_ties(dev):
    B = 130
    torch.manual_seed(130)
    sc = torch.rand(B, B) * 0.5
    sc.fill_diagonal_(1.0)
    groups = np.arange(B)
    sc[0, 1] = sc[0, 129] = 0.95                   # row 0: the masked lower index ties with an unmasked higher one (another wave)
    groups[1] = groups[0]
    sc[5, 70] = sc[5, 128] = 0.9                   # row 5: two unmasked entries tie -> the lower index
    sc[3, 10] = sc[100, 10] = 0.93                 # column 10: masked row 3 ties with unmasked row 100
    groups[10] = groups[3]
    sc[64, 20] = sc[90, 20] = 0.92                 # column 20: two unmasked rows tie -> the lower index
    s = sc.to(dev)
    _, ra, ca = ops.hinge_fwd(s, MARGIN, True, groups=groups)
    assert int(ra[0]) == 129 and int(ra[5]) == 70 and int(ca[10]) == 100 and int(ca[20]) == 64
    want_ra, want_ca = H.hinge_groups_args(sc, groups, MARGIN)
    assert H.args_agree(ra, want_ra) and H.args_agree(ca, want_ca)
    assert int((want_ra >= 0).sum()) >= 4 and int((want_ca >= 0).sum()) >= 4
    gt, idx = torch.as_tensor(groups), torch.arange(B)
    for arg in (ra.cpu().long(), ca.cpu().long()):
        assert bool(((gt[arg] != gt) | (arg == idx)).all())          # never a masked index, rows without a violator included (row 1)
    _, ra_u, ca_u = ops.hinge_fwd(s, MARGIN, True)
    assert int(ra_u[0]) == 1 and int(ca_u[10]) == 3                              # what the mask changed
    for mv in (False, True):
        check(sc, groups, mv, dev, what="ties")


@pytest.mark.parametrize("mv", [False, True])
def test_group_values_and_input_kinds(dev, mv):
    B = 67
    torch.manual_seed(67)
    sc = torch.rand(B, B)
    rng = np.random.RandomState(67)
    groups = rng.randint(-2 ** 31, 2 ** 31 - 1, size=B).astype(np.int64)
    groups[[2, 40, 66]] = 2 ** 31 - 1
    groups[[0, 65]] = -2 ** 31
    groups[[10, 11]] = -5
    groups[[20, 50]] = 0
    want_l, want_g = check(sc, groups, mv, dev, what="group values")
    for kind in (torch.from_numpy(groups), torch.from_numpy(groups).to(dev), groups.astype(np.int32), torch.from_numpy(groups.astype(np.int32)).to(dev),
                 [int(x) for x in groups]):
        loss, grad = run(sc, kind, mv, dev)
        assert torch.equal(bits(loss), bits(want_l)) and torch.equal(bits(grad), bits(want_g))
    s = sc.to(dev).requires_grad_(True)
    gdev = torch.from_numpy(groups).to(dev)
    ops.hinge_loss(s, MARGIN, mv, groups=gdev).backward()
    assert gdev.grad is None and s.grad is not None
    for bad in (groups[:-1], list(groups) + [1], torch.zeros(B, 1, dtype=torch.long), torch.zeros(B + 1, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            ops.hinge_loss(sc.to(dev), MARGIN, mv, groups=bad)
    for bad in ([2 ** 31] + [0] * (B - 1), np.full(B, -2 ** 31 - 1, dtype=np.int64), torch.full((B,), 2 ** 31, dtype=torch.int64, device=dev)):
        with pytest.raises(ValueError):
            ops.hinge_loss(sc.to(dev), MARGIN, mv, groups=bad)
    with pytest.raises(TypeError):
        ops.hinge_loss(sc.to(dev), MARGIN, mv, groups=np.zeros(B, dtype=np.float32))


# ------------------------------------------------------------------------------------------ (e) repeatability
@pytest.mark.parametrize("mv", [False, True])
@pytest.mark.parametrize("B", [300, 1024])
def test_same_bits_run_to_run(cases, dev, B, mv):
    sc, groups, _ = cases(B)
    l0, g0 = run(sc, groups, mv, dev)
    l1, g1 = run(sc, groups, mv, dev)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(g0), bits(g1))
