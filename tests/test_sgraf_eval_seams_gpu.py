"""GPU: the dense SGRAF evaluation scorer (ops.sgraf_scores -> itr_sgraf_scores: csrc/sgraf.hip, sgraf_loc.hip, sgr_fused.hip, the SCAN
kernel in emit mode) at every case of tests/helpers/sgraf_eval_cases.py against the float64 oracle -- the WHOLE of S.

Tolerance per case: 16 * max(e32_oracle, e32_mirror, 2^-24 max|want|) (tests/helpers/sgraf_eval_cases.py;
tests/test_sgraf_eval_case_table.py proves on the CPU that it is never looser than the flat 5e-6 of the older tests and that it sees
each claimed defect at 10 x).  Every case writes into columns 1 .. Nc of a NaN-filled (Ni, Nc + 3) buffer and checks that every score
is finite, that the guard columns are still NaN, that a second call on fresh tensors gives the same bits, that the node-group plan the
library built (plan.node_groups() read back) is the planner mirror's and that ops.SGRAF_LAST_BLOCK["image_block"] is the mirror's.

Bit identities (identical rank vectors for every row partition of the sharded evaluation):
    image rows: images [i0, i1) scored alone have the bits of those rows of the full call -- one image, the tail image, a range across
        a 4-image boundary, a range across the 64-image block boundary; SAF, SGR fused, the SGR chain;
    caption subsets scored alone have the bits of their columns (some caption changes its column tile and its node group);
    every image_block in {4, 8, 16, 32, 64}, the persistent and the non-persistent walk, sgr_group_rows 32 and 64 give the same bits;
    fused and chain at sim_dim 256 are each within tol of float64.
The persistent-walk cases are built for 256 compute units and are skipped with a message on another device.
profiles/sgraf_eval_seams/measured.txt is the record of one run (ITR_SGRAF_EVAL_SEAMS_RECORD=<file> appends one line per case)."""
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import ops
from itr_amd.settings import SETTINGS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sgraf_eval_cases as G        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_SGRAF_EVAL_SEAMS_RECORD")
_WEIGHTS = {}


def device_weights(c, dev):
    key = (c.mod, c.D, c.S, c.steps)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = {k: v.to(dev) for k, v in c.weights.items()}
    return _WEIGHTS[key]


def scores(c, dev, images=None, caps=None, guard=False, **over):
    """S of the case on fresh tensors; `images` = (i0, i1) keeps those images, `caps` keeps those captions (re-packed); over: variant,
    pinned, group_rows in place of the case's.  -> (S, plan), with guard (S as a view, the NaN-filled buffer around it, plan)."""
    x = c.inputs()
    img, words, lens = x['images'], x['words'], list(c.lens)
    if images is not None:
        img = img[images[0]:images[1]]
    if caps is not None:
        off = G._offsets(c.lens)
        words = torch.cat([words[off[k]:off[k] + c.lens[k]] for k in caps], 0)
        lens = [c.lens[k] for k in caps]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img, words = img.contiguous().to(dev), words.contiguous().to(dev)
    old = SETTINGS.sgr_group_rows
    SETTINGS.sgr_group_rows = over.get('group_rows', c.group_rows)
    try:
        plan = ops.ScanPlan(off, lens, int(sum(lens)), dev, max_kernel_len=ops.SGRAF_MAX_WORDS)
        args = dict(module_name=c.mod, sgr_step=c.steps, image_block=over.get('pinned', c.pinned), variant=over.get('variant', c.variant))
        if not guard:
            out = torch.empty(img.shape[0], plan.Nc, device=dev, dtype=torch.float32) if c.out_given else None
            return ops.sgraf_scores(img, words, plan, device_weights(c, dev), out=out, **args), plan
        buf = torch.full((img.shape[0], plan.Nc + 3), float('nan'), device=dev, dtype=torch.float32)
        out = buf[:, 1:1 + plan.Nc]
        got = ops.sgraf_scores(img, words, plan, device_weights(c, dev), out=out, **args)
        assert got.data_ptr() == out.data_ptr() and out.stride(0) == plan.Nc + 3
        groups = plan.node_groups() if plan.Nc_kernel else None
        return got, buf, plan, groups
    finally:
        SETTINGS.sgr_group_rows = old


def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def needs_256_cus(c, dev):
    if c.group == 'walk' and cus(dev) != G.WALK_CUS:
        pytest.skip("the persistent-walk cases are built for %d compute units, this device has %d" % (G.WALK_CUS, cus(dev)))


def check(c, dev):
    needs_256_cus(c, dev)
    want, e_oracle, e_mirror, tol, _, _ = c.reference()
    got, buf, plan, groups = scores(c, dev, guard=True)
    block = ops.SGRAF_LAST_BLOCK.get("image_block")
    again, _ = scores(c, dev)
    fails = []
    assert tuple(got.shape) == tuple(want.shape) == (c.Ni, c.Nc), c
    if not bool(torch.isfinite(got).all()):
        fails.append("S is not finite")
    err = float(torch.nan_to_num((got.double().cpu() - want).abs(), nan=float('inf')).max())
    print("%s: max err %.3e e32_oracle %.3e e32_mirror %.3e tol %.3e ratio %.3f" % (c.name, err, e_oracle, e_mirror, tol, err / tol))
    if not err <= tol:
        fails.append("max err %.3e is %.3f x tol %.3e" % (err, err / tol, tol))
    if not (bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, 1 + c.Nc:]).all())):
        fails.append("a guard column was written")
    same = torch.equal(got, again)
    if not same:
        fails.append("a second run gives other bits")
    # the plans the library built are the mirror's
    p = c.plan
    if (plan.Nc_kernel, plan.n_tiles) != (p.Nc_kernel, p.n_tiles):
        fails.append("the library plans %d captions into %d tiles, the mirror %d into %d" % (plan.Nc_kernel, plan.n_tiles, p.Nc_kernel, p.n_tiles))
    if (plan.long_idx is None) != (not p.long_idx) or (p.long_idx and plan.long_idx.tolist() != p.long_idx):
        fails.append("the library's long captions are not the mirror's")
    if p.Nc_kernel:
        if groups is None or groups[2] != p.n_groups:
            fails.append("the library plans %s node groups, the mirror %d" % (groups and groups[2], p.n_groups))
        elif groups[0].cpu().tolist() != p.group_begin or groups[1].cpu().tolist() != p.group_order:
            fails.append("the library's group_begin / group_order are not the mirror's")
    if block != p.last_block:
        fails.append("the library ran with image_block %s, the mirror says %d" % (block, p.last_block))
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("%s | %s | e32_oracle %.3e e32_mirror %.3e tol %.3e%s err %.3e ratio %.3f | repeat %s\n" % (
                c.name, p.describe(), e_oracle, e_mirror, tol, " (fallback)" if c.name in G.FALLBACK else "", err, err / tol,
                'equal' if same else 'DIFFERENT'))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


@pytest.mark.parametrize("case", G.cases(mod='SAF'), ids=lambda c: c.name)
def test_saf_eval_seams_vs_float64(dev, case):
    check(case, dev)


@pytest.mark.parametrize("case", G.cases(mod='SGR'), ids=lambda c: c.name)
def test_sgr_eval_seams_vs_float64(dev, case):
    check(case, dev)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities
def differ(a, b):
    return "differ by up to %.3e" % float((a - b).abs().max())


ROW_CASES = [c for c in G.CASES if (c.group == 'Ni' and c.Ni == 65) or (c.group == 'route' and c.route_name() in
                                                                        ('saf256', 'saf_generic', 'sgr_fused', 'sgr_chain256', 'sgr_chain'))]


def row_ranges(Ni):
    """One image, the tail image, a range across a 4-image boundary, a range across the 64-image block boundary."""
    return sorted(set([(2, 3), (Ni - 1, Ni), (3, min(Ni, 7))] + ([(62, 65)] if Ni >= 65 else [])))


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c.name)
def test_image_rows_scored_alone_have_the_bits_of_the_full_call(dev, case):
    c = case
    full, _ = scores(c, dev)
    assert c.Ni >= 5 and any(i0 < 4 < i1 for i0, i1 in row_ranges(c.Ni))
    for i0, i1 in row_ranges(c.Ni):
        part, _ = scores(c, dev, images=(i0, i1))
        assert part.shape == (i1 - i0, c.Nc)
        assert torch.equal(part, full[i0:i1]), "%s: images [%d, %d) alone %s" % (c.name, i0, i1, differ(part, full[i0:i1]))


SUBSET_CASES = [c for c in G.CASES if c.group == 'groups' or (c.group == 'route' and c.route_name() in ('saf256', 'saf_generic', 'sgr_fused', 'sgr_chain256', 'sgr_chain'))
                or (c.group == 'tiles' and c.tag == 'sixteen4')]


def caption_subsets(c):
    """Every other caption; the set without its two longest captions; the captions in the second half and the first one."""
    n = c.Nc
    longest = sorted(range(n), key=lambda k: -c.lens[k])[:2]
    return [s for s in (list(range(0, n, 2)), [k for k in range(n) if k not in longest], [0] + list(range(n // 2 + 1, n))) if s]


@pytest.mark.parametrize("case", SUBSET_CASES, ids=lambda c: c.name)
def test_caption_subsets_scored_alone_have_the_bits_of_their_columns(dev, case):
    c = case
    full, _ = scores(c, dev)
    moved_col = moved_group = 0
    for caps in caption_subsets(c):
        part, _ = scores(c, dev, caps=caps)
        assert part.shape == (c.Ni, len(caps))
        assert torch.equal(part, full[:, caps]), "%s: captions %s alone %s" % (c.name, caps, differ(part, full[:, caps]))
        sub = G.Plan(c.mod, c.Ni, c.D, c.S, [c.lens[k] for k in caps], c.variant, c.group_rows, c.pinned)
        moved_col += sum(1 for j, k in enumerate(caps) if sub.cols.cap_col[j] != c.plan.cols.cap_col[k])
        where_full = {k: (gi, s) for gi, g in enumerate(c.plan.groups) for s, k in enumerate(g)}
        where_sub = {j: (gi, s) for gi, g in enumerate(sub.groups) for s, j in enumerate(g)}
        moved_group += sum(1 for j, k in enumerate(caps) if where_sub[j] != where_full[k])
    assert moved_col and moved_group, c         # the subsets are packed differently: some caption changed its column and its group


BLOCK_CASES = [c for c in G.CASES if c.group == 'Ni' and c.Ni == 65]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: c.name)
def test_every_image_block_gives_the_same_bits(dev, case):
    c = case
    full, _ = scores(c, dev)
    for ib in (4, 8, 16, 32, 64):
        got, _ = scores(c, dev, pinned=ib)
        assert ops.SGRAF_LAST_BLOCK["image_block"] == ib
        assert torch.equal(got, full), "%s: image_block %d %s" % (c.name, ib, differ(got, full))


WALK_CASES = [c for c in G.CASES if c.plan.route == 'sgr_fused' and c.plan.persistent and
              (c.group in ('walk', 'groups', 'route') or (c.group == 'ngroups' and c.Nc in (257, 1030)))]


@pytest.mark.parametrize("case", WALK_CASES, ids=lambda c: c.name)
def test_persistent_and_non_persistent_walks_give_the_same_bits(dev, case):
    c = case
    needs_256_cus(c, dev)
    full, _ = scores(c, dev)
    got, _ = scores(c, dev, variant=c.variant + ('non_persistent',))
    assert torch.equal(got, full), "%s: one workgroup per item %s" % (c.name, differ(got, full))


ROWS_CASES = [c for c in G.CASES if c.plan.route == 'sgr_fused' and c.plan.persistent and
              (c.group in ('groups', 'route') or (c.group == 'words' and c.tag in ('max15', 'max16', 'max31', 'max32', 'max63')))]


@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: c.name)
def test_group_rows_32_and_64_give_the_same_bits(dev, case):
    c = case
    a, _ = scores(c, dev, group_rows=64)
    b, _ = scores(c, dev, group_rows=32)
    assert G.Plan(c.mod, c.Ni, c.D, c.S, c.lens, c.variant, 32).groups != G.Plan(c.mod, c.Ni, c.D, c.S, c.lens, c.variant, 64).groups
    assert torch.equal(a, b), "%s: sgr_group_rows 32 and 64 %s" % (c.name, differ(a, b))


CHAIN_TWINS = [(c, G._BY_NAME[c.name + "-unfused_steps"]) for c in G.cases(mod='SGR') if c.name + "-unfused_steps" in G._BY_NAME]


@pytest.mark.parametrize("pair", CHAIN_TWINS, ids=lambda p: p[0].name)
def test_fused_and_chain_are_each_within_tol_of_float64(dev, pair):
    """The twins share shape and weights, not the seed (it comes from the name): each is held to its own reference; and on ONE input
    the two forms agree to the sum of the two bounds."""
    fused, chain = pair
    assert len(CHAIN_TWINS) >= 10 and fused.plan.route == 'sgr_fused' and chain.plan.route == 'sgr_chain256'
    want, _, _, tol, _, _ = fused.reference()
    a, _ = scores(fused, dev)
    b, _ = scores(fused, dev, variant=('unfused_steps',))
    ea, eb = float((a.double().cpu() - want).abs().max()), float((b.double().cpu() - want).abs().max())
    print("%s: fused err %.3e chain err %.3e tol %.3e" % (fused.name, ea, eb, tol))
    assert ea <= tol and eb <= tol, (fused.name, ea, eb, tol)


# ---------------------------------------------------------------------------------------------------------------------
# error edges: refused before any kernel of the pair stage runs
@pytest.mark.parametrize("what,mod,D,S,steps", [("sim_dim 1040", 'SAF', 32, 1040, 3), ("D = 48", 'SAF', 48, 256, 3), ("SGR sim_dim 40", 'SGR', 32, 40, 3),
                                                ("sgr_step 0", 'SGR', 32, 256, 0), ("sgr_step 9", 'SGR', 32, 256, 9)])
def test_unsupported_shapes_raise_what_the_header_documents(dev, what, mod, D, S, steps):
    g = torch.Generator().manual_seed(3)
    img, words = torch.randn(2, 36, D, generator=g).to(dev), torch.randn(5, D, generator=g).to(dev)
    plan = ops.ScanPlan(np.array([0, 3], dtype=np.int64), [3, 2], 5, dev)
    w = {k: v.to(dev) for k, v in G.sgraf_weights.make(D, S, max(steps, 1)).items()}
    with pytest.raises(NotImplementedError):
        ops.sgraf_scores(img, words, plan, w, mod, steps)
    torch.cuda.synchronize()
