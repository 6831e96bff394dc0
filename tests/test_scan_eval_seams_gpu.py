"""GPU: the fused SCAN evaluation scorer (csrc/scan_xattn.hip through ops.scan_xattn_scores, 36 regions) at every case of
tests/helpers/scan_eval_cases.py against the float64 oracle -- the WHOLE of S.

Tolerance per case: 16 * max(e32_oracle, e32_mirror, 2^-24 max|want|) (tests/helpers/scan_eval_cases.py;
tests/test_scan_eval_case_table.py proves on the CPU that it is at most 2^-10 of the largest score and never looser than the flat
2e-5 of the older tests, and that it sees each claimed defect at 10 x).  Every case writes into columns 1 .. Nc of a NaN-filled
(Ni, Nc + 3) buffer -- an output stride that is not Nc, rows that are not 16-byte aligned -- and checks that every score is finite,
that the guard columns are still NaN, that the plan the library built (tile_begin, cap_order read back from the device) is the planner
mirror's, and that a second call on fresh tensors gives the same bits.

Bit identities (identical rank vectors for every row partition of the sharded evaluation):
    image rows, both directions: images [i0, i1) scored alone have the bits of those rows of the full call -- one image, the tail
        image, a range across a 4-image boundary;
    caption subsets, t2i (i2t sums over a caption's words in an order that follows its column in the tile: exempt): the
        tile-composition cases' captions scored in other company have the bits of their columns;
    workspace: one scan_prepare workspace reused across (norm, aggregation) settings gives the bits of fresh calls.
profiles/scan_eval_seams/measured.txt is the record of one run (ITR_SCAN_EVAL_SEAMS_RECORD=<file> appends one line per case)."""
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scan_eval_cases as E        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_SCAN_EVAL_SEAMS_RECORD")


def device_inputs(c, dev, images=None, caps=None):
    """Fresh device tensors and a fresh plan of the case: (images, packed words, ScanPlan); `images` = (i0, i1) keeps those images,
    `caps` keeps those captions (re-packed)."""
    x = c.inputs()
    img, words, lens = x['images'], x['words'], list(c.lens)
    if images is not None:
        img = img[images[0]:images[1]]
    if caps is not None:
        off = E._offsets(c.lens)
        words = torch.cat([words[off[k]:off[k] + c.lens[k]] for k in caps], 0)
        lens = [c.lens[k] for k in caps]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    plan = ops.ScanPlan(off, lens, int(sum(lens)), dev)
    return img.contiguous().to(dev), words.contiguous().to(dev), plan


def scores(c, dev, norm=None, agg=None, guard=False, **kw):
    """S of the case on fresh tensors -> (S, plan) or, with guard, (S as a view, the NaN-filled buffer around it, plan)."""
    img, words, plan = device_inputs(c, dev, **kw)
    args = dict(cross_attn=c.xa, raw_feature_norm=norm or c.norm, agg_func=agg or c.agg, lambda_lse=E.LAMBDA_LSE, lambda_softmax=c.ls)
    if not guard:
        return ops.scan_xattn_scores(img, words, plan, **args), plan
    buf = torch.full((img.shape[0], plan.Nc + 3), float('nan'), device=dev, dtype=torch.float32)
    out = buf[:, 1:1 + plan.Nc]
    assert out.stride(0) == plan.Nc + 3 and out.data_ptr() % 16 != 0
    got = ops.scan_xattn_scores(img, words, plan, out=out, **args)
    assert got.data_ptr() == out.data_ptr()
    return got, buf, plan


def check(c, dev):
    want, e_oracle, e_mirror, tol, _ = c.reference()
    got, buf, plan = scores(c, dev, guard=True)
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
    # the plan the library built is the mirror's
    p = c.plan
    if (plan.Nc_kernel, plan.n_tiles) != (p.Nc_kernel, p.n_tiles):
        fails.append("the library plans %d captions into %d tiles, the mirror %d into %d" % (plan.Nc_kernel, plan.n_tiles, p.Nc_kernel, p.n_tiles))
    elif plan.tile_begin.cpu().tolist() != p.tile_begin or plan.cap_order.cpu().tolist()[:p.Nc_kernel] != p.cap_order:
        fails.append("the library's tile_begin / cap_order are not the mirror's")
    if (plan.long_idx is None) != (not p.long_idx) or (p.long_idx and plan.long_idx.tolist() != p.long_idx):
        fails.append("the library's long captions are not the mirror's")
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("%s | %s | e32_oracle %.3e e32_mirror %.3e tol %.3e%s err %.3e ratio %.3f | repeat %s\n" % (
                c.name, p.describe(), e_oracle, e_mirror, tol, " (fallback)" if c.name in E.FALLBACK else "", err, err / tol,
                'equal' if same else 'DIFFERENT'))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


@pytest.mark.parametrize("case", E.cases('t2i'), ids=lambda c: c.name)
def test_scan_t2i_eval_seams_vs_float64(dev, case):
    check(case, dev)


@pytest.mark.parametrize("case", E.cases('i2t'), ids=lambda c: c.name)
def test_scan_i2t_eval_seams_vs_float64(dev, case):
    check(case, dev)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities
ROW_CASES = [c for c in E.CASES if (c.group == 'Ni' and c.Ni >= 5) or (c.group == 'norm' and c.agg == 'LogSumExp') or
             (c.group == 'gate' and c.norm == 'l2norm')]


def row_ranges(Ni):
    """One image, the tail image, a range across a 4-image boundary."""
    return sorted(set([(2, 3), (Ni - 1, Ni), (3, min(Ni, 7))]))


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c.name)
def test_image_rows_scored_alone_have_the_bits_of_the_full_call(dev, case):
    c = case
    full, _ = scores(c, dev)
    assert c.Ni >= 5 and any(i0 < 4 < i1 for i0, i1 in row_ranges(c.Ni))
    for i0, i1 in row_ranges(c.Ni):
        part, _ = scores(c, dev, images=(i0, i1))
        assert part.shape == (i1 - i0, c.Nc)
        assert torch.equal(part, full[i0:i1]), "%s: images [%d, %d) alone differ from their rows by up to %.3e" % (
            c.name, i0, i1, float((part - full[i0:i1]).abs().max()))


SUBSET_CASES = [c for c in E.cases('t2i') if c.group in ('tile', 'ends')]


def caption_subsets(c):
    """Every other caption; the set without its two companions; the captions in the second half and the first one."""
    n = c.Nc
    comp = [k for k, w in enumerate(c.lens) if w in E.COMPANIONS][:2]
    return [s for s in (list(range(0, n, 2)), [k for k in range(n) if k not in comp], [0] + list(range(n // 2 + 1, n))) if s]


@pytest.mark.parametrize("case", SUBSET_CASES, ids=lambda c: c.name)
def test_t2i_caption_subsets_scored_alone_have_the_bits_of_their_columns(dev, case):
    c = case
    full, _ = scores(c, dev)
    moved = 0
    for caps in caption_subsets(c):
        part, _ = scores(c, dev, caps=caps)
        assert part.shape == (c.Ni, len(caps))
        assert torch.equal(part, full[:, caps]), "%s: captions %s alone differ from their columns by up to %.3e" % (
            c.name, caps, float((part - full[:, caps]).abs().max()))
        # the subset is packed differently: some caption sits in another column of its tile than in the full call
        col_full = E.Plan(c.Ni, c.D, c.lens, c.xa, c.norm, c.ls).cap_col
        col_sub = E.Plan(c.Ni, c.D, [c.lens[k] for k in caps], c.xa, c.norm, c.ls).cap_col
        moved += sum(1 for j, k in enumerate(caps) if col_sub[j][1] != col_full[k][1])
    assert moved or c.tag in ('one64',), c


WS_CASES = [c for c in E.CASES if c.group == 'norm' and c.norm == E.DEFAULT and c.agg == 'LogSumExp'] + \
           [c for c in E.CASES if c.group == 'long' and c.tag == 'first.middle']


@pytest.mark.parametrize("case", WS_CASES, ids=lambda c: c.name)
def test_one_workspace_serves_every_norm_and_aggregation(dev, case):
    c = case
    img, words, plan = device_inputs(c, dev)
    ws = ops.scan_prepare(img, words, plan, c.xa)
    settings = (('clipped_l2norm', 'LogSumExp'), ('no_norm', 'Sum'), ('softmax', 'Max'), ('clipped_l2norm', 'LogSumExp'))
    for norm, agg in settings:
        got = ops.scan_xattn_scores(img, words, plan, cross_attn=c.xa, raw_feature_norm=norm, agg_func=agg, lambda_lse=E.LAMBDA_LSE,
                                    lambda_softmax=c.ls, workspace=ws)
        fresh, _ = scores(c, dev, norm=norm, agg=agg)
        assert torch.equal(got, fresh), "%s %s %s: the reused workspace gives other bits (up to %.3e)" % (
            c.name, norm, agg, float((got - fresh).abs().max()))
