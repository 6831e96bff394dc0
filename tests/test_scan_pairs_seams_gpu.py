"""GPU: the SCAN candidate-list kernels (csrc/scan_pairs.hip through ops.scan_candidate_scores, csrc/scan_attn.hip through
ops.scan_pair_attention) at every case of tests/helpers/scan_pairs_cases.py against the float64 oracle -- every score of every list, and
for the attention entry the whole of `attn`, `row_sim` and `score`.

Tolerance per case and tensor: 16 * max(e32_oracle, e32_mirror, 2^-24 max|want|) (tests/helpers/scan_pairs_cases.py;
tests/test_scan_pairs_case_table.py proves on the CPU that it is at most 2^-10 of the tensor's largest value, for scores and cosines never
looser than the flat 2e-5 of the older tests, and that it sees each claimed defect at 10 x).  Every output is finite, a second call on
fresh tensors gives the same bits, the number of compared elements is the number produced, and t2i rows / i2t columns of every attention
matrix sum to 1.  The direct-call cases hand the C entry points lists that ops never makes (slots descending inside a caption, output
slots with gaps) and NaN-filled buffers longer than declared: what no pair names stays NaN, and the block offsets the library left in
its workspace are the planning mirror's.

Bit identities the code claims (scan_pairs.hip, scan_attn.hip headers): a pair's bits are the same in another list, in another block
position, through the other `by`, and with a scan_pairs_prepare workspace reused across norms and aggregations -- on the seam cases.
The attention entry's score against scan_candidate_scores on the same pairs is held to the bound, and to bit equality for captions of up
to 64 words.

Index guards, only where a broken guard gives a wrong number inside memory the test owns: an output slot >= out_len inside the longer
buffer stays NaN; a caption declared with length 0 or 65 (its word rows exist) scores NaN; an image index >= the declared Ni (the image
tensor and the workspace hold that image) scores NaN.
profiles/scan_pairs_seams/measured.txt is the record of one run (ITR_SCAN_PAIRS_SEAMS_RECORD=<file> appends one line per case)."""
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import scan_pairs_cases as C        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_SCAN_PAIRS_SEAMS_RECORD")
NAN = float('nan')


def device_inputs(c, dev):
    """Fresh device tensors and a fresh plan of the case: (images, packed words, ScanPlan)."""
    x = c.inputs()
    plan = ops.ScanPlan(np.asarray(c.off, np.int64), np.asarray(c.lens, np.int32), c.n_tok, dev)
    return x['images'].contiguous().to(dev), x['words'].contiguous().to(dev), plan


def settings(c, norm=None, agg=None):
    return dict(cross_attn=c.xa, raw_feature_norm=norm or c.norm, agg_func=agg or c.agg, lambda_lse=C.LAMBDA_LSE, lambda_softmax=c.ls)


def i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.int32))).to(dev)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def list_scores(c, dev, cand=None, by=None, **kw):
    """ops.scan_candidate_scores on fresh tensors -> [n_q, K]"""
    img, words, plan = device_inputs(c, dev)
    return ops.scan_candidate_scores(img, words, plan, i32(c.cand if cand is None else cand, dev), by or c.by, **settings(c, **kw))


def direct_scores(c, dev, slot_of=None, out_len=None, buf_len=None, Ni=None, call_len=None):
    """itr_scan_pairs_prepare + itr_scan_pair_scores on the plan's caption-major list.  slot_of: pair (in the case's order) -> output
    slot; Ni: the image count declared to both entry points (the tensor and the workspace hold c.Ni); call_len: {caption: the length
    declared to the scores entry}.  -> (the NaN-filled buffer after the call, blk_ptr as the library left it)."""
    lib, p = _lib.load(), c.plan
    x = c.inputs()
    img, words = x['images'].contiguous().to(dev), x['words'].contiguous().to(dev)
    mode, Ni = (0 if c.xa == 't2i' else 1), (c.Ni if Ni is None else Ni)
    off = torch.as_tensor(np.asarray(c.off, np.int64)).to(dev)
    klen = list(p.klen)
    prep_len = i32([0 if call_len and k in call_len else w for k, w in enumerate(klen)], dev)      # as ops does for what the kernel does not take
    for k, w in (call_len or {}).items():
        assert c.off[k] + max(w, 1) <= c.n_tok          # the declared rows exist
        klen[k] = w
    wsb = lib.itr_scan_pairs_workspace_bytes(c.Ni, C.SC_R, c.n_tok, c.Nc, mode)
    ws = torch.zeros(wsb, device=dev, dtype=torch.uint8)
    _lib.check(lib.itr_scan_pairs_prepare(ops._p(img), ops._p(words), ops._p(off), ops._p(prep_len), Ni, c.Nc, c.n_tok, C.SC_R, c.D, mode,
                                          ops._p(ws), wsb, ops._stream()))
    slot_of = slot_of or (lambda s: s)
    out_len = c.P if out_len is None else out_len
    buf = torch.full((buf_len or out_len,), NAN, device=dev, dtype=torch.float32)
    pair_out = [slot_of(s) for s in p.pair_out]
    assert all(0 <= s < buf.numel() for s in pair_out)                  # a refused slot still lies inside the buffer the test owns
    assert all(0 <= i < c.Ni for i in p.pair_img)                       # ... and a refused image inside the tensor
    klen_d, cap_ptr_d, pair_img_d, pair_out_d = i32(klen, dev), i32(p.cap_ptr, dev), i32(p.pair_img, dev), i32(pair_out, dev)      # (held until the call is over)
    _lib.check(lib.itr_scan_pair_scores(
        ops._p(img), ops._p(words), ops._p(off), ops._p(klen_d), ops._p(cap_ptr_d), ops._p(pair_img_d),
        ops._p(pair_out_d), p.P, Ni, c.Nc, c.n_tok, C.SC_R, c.D, mode, ops._NORMS[c.norm], ops._AGGS[c.agg], c.ls, C.LAMBDA_LSE,
        ops._p(buf), out_len, ops._p(ws), wsb, ops._stream()))
    torch.cuda.synchronize()
    return buf.cpu(), ws[:4 * (c.Nc + 1)].cpu().view(torch.int32).tolist()


GUARD = 5           # NaN floats before and after each flat buffer of the direct attention call


def attention(c, dev, direct=False, **kw):
    """-> {tensor: flat float32 on the host}, and for the direct call the guard floats' state"""
    img, words, plan = device_inputs(c, dev)
    pairs = i32(c.pairs, dev).view(-1, 2)
    if not direct:
        got = ops.scan_pair_attention(img, words, plan, pairs, **settings(c, **kw))
        assert len(got) == c.P and got.cap_len.cpu().tolist() == [c.lens[k] for _, k in c.pairs]
        return {'attn': got.attn.cpu(), 'row_sim': got.row_sim.cpu(), 'score': got.score.cpu()}, True
    lib = _lib.load()
    mode = 0 if c.xa == 't2i' else 1
    ws = ops.scan_pairs_prepare(img, words, plan, c.xa).buf
    off, lens = torch.as_tensor(np.asarray(c.off, np.int64)).to(dev), i32(c.lens, dev)
    w = [c.lens[k] for _, k in c.pairs]
    row_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(w)]).astype(np.int64)).to(dev)
    attn_ptr = row_ptr * C.SC_R
    n = {'attn': sum(w) * C.SC_R, 'row_sim': sum(w) if mode == 0 else c.P * C.SC_R, 'score': c.P}
    buf = {k: torch.full((GUARD + v + GUARD,), NAN, device=dev, dtype=torch.float32) for k, v in n.items()}
    view = {k: buf[k][GUARD:GUARD + v] for k, v in n.items()}
    pair_img, pair_cap = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    _lib.check(lib.itr_scan_pair_attention(
        ops._p(img), ops._p(words), ops._p(off), ops._p(lens), ops._p(pair_img), ops._p(pair_cap), c.P, c.Ni,
        c.Nc, c.n_tok, C.SC_R, c.D, mode, ops._NORMS[c.norm], ops._AGGS[c.agg], c.ls, C.LAMBDA_LSE, ops._p(view['attn']), ops._p(attn_ptr), n['attn'],
        ops._p(view['row_sim']), ops._p(row_ptr), n['row_sim'], ops._p(view['score']), ops._p(ws), ws.numel(), ops._stream()))
    torch.cuda.synchronize()
    guards = all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()) for b in buf.values())
    return {k: v.cpu() for k, v in view.items()}, guards


def compare(c, got, fails):
    """got {tensor: flat float32} against the case's references -> the record's figures per tensor"""
    ref, figures = c.reference(), []
    for t in C.TENSORS[c.kernel]:
        want, e_oracle, e_mirror, tol, _ = ref[t]
        if tuple(got[t].shape) != tuple(want.shape):
            fails.append("%s holds %d elements, the reference %d" % (t, got[t].numel(), want.numel()))
            continue
        if not bool(torch.isfinite(got[t]).all()):
            fails.append("%s is not finite" % t)
        err = float(torch.nan_to_num((got[t].double() - want).abs(), nan=float('inf')).max())
        if not err <= tol:
            fails.append("%s: max err %.3e is %.3f x tol %.3e" % (t, err, err / tol, tol))
        figures.append((t, e_oracle, e_mirror, tol, err))
    return figures


def record(c, figures, same, extra=""):
    line = "; ".join("%s e32_oracle %.3e e32_mirror %.3e tol %.3e%s err %.3e ratio %.3f" % (
        t, eo, em, tol, " (fallback)" if t in C.FALLBACK.get(c.name, {}) else "", err, err / tol) for t, eo, em, tol, err in figures)
    print("%s: %s%s" % (c.name, line, extra))
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("%s | %s | %s | repeat %s%s\n" % (c.name, c.describe(), line, 'equal' if same else 'DIFFERENT', extra))


ABI_GAP = 2         # the direct scores call writes pair s to slot 2 s: every odd slot is named by nobody
ABI_TAIL = 7


def check_scores(c, dev):
    fails = []
    if not c.abi:
        out = list_scores(c, dev)
        assert out.shape == (len(c.cand), len(c.cand[0]))
        got, again = out.reshape(-1).cpu(), list_scores(c, dev).reshape(-1).cpu()
    else:
        slot_of = lambda s: ABI_GAP * s
        run = lambda: direct_scores(c, dev, slot_of, out_len=ABI_GAP * c.P, buf_len=ABI_GAP * c.P + ABI_TAIL)
        (buf, blk_ptr), (buf2, _) = run(), run()
        got, again = buf[0:ABI_GAP * c.P:ABI_GAP], buf2[0:ABI_GAP * c.P:ABI_GAP]
        if not (bool(torch.isnan(buf[1:ABI_GAP * c.P:ABI_GAP]).all()) and bool(torch.isnan(buf[ABI_GAP * c.P:]).all())):
            fails.append("a slot that no pair names, or the tail behind out_len, was written")
        if blk_ptr != c.plan.blk_ptr:
            fails.append("the library's blk_ptr %s is not the mirror's %s" % (blk_ptr, c.plan.blk_ptr))
    figures = compare(c, {'score': got}, fails)
    same = torch.equal(bits(got), bits(again))
    if not same:
        fails.append("a second run gives other bits")
    record(c, figures, same)
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


# the attention entry's score against scan_candidate_scores on the same pairs, over the whole table: case -> (largest difference,
# captions of <= 64 words bit-equal)
VS_SCORES = {}


def lists_for(c, by):
    """The case's pairs as lists of the given direction, padded with the first pair's entry -> (cand [n_q, K], flat position of pair p)."""
    n_q = c.Nc if by == 'caption' else c.Ni
    per, where = [[] for _ in range(n_q)], []
    for i, k in c.pairs:
        q, e = (k, i) if by == 'caption' else (i, k)
        where.append((q, len(per[q])))
        per[q].append(e)
    K = max(len(v) for v in per)
    pad = c.pairs[0][0] if by == 'caption' else c.pairs[0][1]
    cand = np.asarray([v + [pad] * (K - len(v)) for v in per], np.int32)
    return cand, np.asarray([q * K + j for q, j in where], np.int64)


def check_attention(c, dev):
    fails = []
    got, guards = attention(c, dev, direct=c.abi)
    again, _ = attention(c, dev, direct=c.abi)
    if not guards:
        fails.append("a guard float around a flat buffer was written")
    figures = compare(c, got, fails)
    ref = c.reference()
    # t2i rows and i2t columns of every matrix sum to 1: n terms, each within the bound; never looser than the older test's 1e-5
    tol_attn, o, e_sum, n_attn = ref['attn'][3], 0, 0.0, 0
    if got['attn'].numel() == ref['attn'][0].numel():
        for _, k in c.pairs:
            A = got['attn'][o:o + c.lens[k] * C.SC_R].view(-1, C.SC_R).double()
            sums = A.sum(1 if c.xa == 't2i' else 0)
            bound = min((C.SC_R if c.xa == 't2i' else c.lens[k]) * tol_attn, 1e-5)
            e = float(torch.nan_to_num((sums - 1.0).abs(), nan=float('inf')).max())
            if not e <= bound:
                fails.append("an attention matrix of %d words sums to 1 +- %.3e (bound %.3e)" % (c.lens[k], e, bound))
            e_sum = max(e_sum, e)
            o += A.numel()
            n_attn += A.numel()
        assert n_attn == got['attn'].numel()
    same = all(torch.equal(bits(got[t]), bits(again[t])) for t in got)
    if not same:
        fails.append("a second run gives other bits")
    # the score-only path on the same pairs
    cand, pos = lists_for(c, 'caption' if c.Nc < 1000 else 'image')
    sc = list_scores(c, dev, cand, 'caption' if c.Nc < 1000 else 'image').reshape(-1).cpu()[torch.from_numpy(pos)]
    short = torch.tensor([c.lens[k] <= C.SP_MAXW for _, k in c.pairs])
    d = float(torch.nan_to_num((sc.double() - got['score'].double()).abs(), nan=float('inf')).max())
    eq = torch.equal(bits(sc[short]), bits(got['score'][short]))
    VS_SCORES[c.name] = (d, eq)
    if not d <= ref['score'][3]:
        fails.append("the score differs from scan_candidate_scores' by %.3e, tol %.3e" % (d, ref['score'][3]))
    if not eq:          # (measured over the whole table before it was asserted: profiles/scan_pairs_seams/README.md)
        fails.append("the scores of captions of <= 64 words are not the bits of scan_candidate_scores")
    record(c, figures, same, " | sums-1 %.3e | vs scores %.3e (<= 64 words bit-equal: %s)" % (e_sum, d, eq))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


@pytest.mark.parametrize("case", C.cases('scores', 't2i'), ids=lambda c: c.name)
def test_scan_pairs_t2i_seams_vs_float64(dev, case):
    check_scores(case, dev)


@pytest.mark.parametrize("case", C.cases('scores', 'i2t'), ids=lambda c: c.name)
def test_scan_pairs_i2t_seams_vs_float64(dev, case):
    check_scores(case, dev)


@pytest.mark.parametrize("case", C.cases('attention', 't2i'), ids=lambda c: c.name)
def test_scan_attn_t2i_seams_vs_float64(dev, case):
    check_attention(case, dev)


@pytest.mark.parametrize("case", C.cases('attention', 'i2t'), ids=lambda c: c.name)
def test_scan_attn_i2t_seams_vs_float64(dev, case):
    check_attention(case, dev)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities, on the seam cases
IDENT_CASES = [c for c in C.CASES if c.kernel == 'scores' and not c.abi and
               (c.group in ('count', 'long', 'zero', 'ls', 'D') or (c.group == 'Nc' and c.Nc in (1, 2, 1025)) or (c.group == 'norm' and c.agg == 'LogSumExp'))]


@pytest.mark.parametrize("case", IDENT_CASES, ids=lambda c: c.name)
def test_a_pairs_bits_are_its_own_in_any_list(dev, case):
    """Every list rotated by three places (another slot of the block; with more than 8 entries another block), only the second half
    of every list (another blocking), and the same pairs through the other `by` (other company: padding entries)."""
    c = case
    base = list_scores(c, dev).cpu()
    cand = np.asarray(c.cand, np.int32)
    K = cand.shape[1]
    rolled = list_scores(c, dev, np.roll(cand, 3, 1)).cpu()
    assert torch.equal(bits(rolled), bits(torch.roll(base, 3, 1))), "%s: lists rotated by 3 give other bits (up to %.3e)" % (
        c.name, float((rolled - torch.roll(base, 3, 1)).abs().max()))
    if K > 1:
        half = list_scores(c, dev, cand[:, K // 2:]).cpu()
        assert torch.equal(bits(half), bits(base[:, K // 2:])), "%s: the lists' second halves alone give other bits" % c.name
    other = 'image' if c.by == 'caption' else 'caption'
    cand_o, pos = lists_for(c, other)
    through = list_scores(c, dev, cand_o, other).reshape(-1).cpu()[torch.from_numpy(pos)]
    assert through.numel() == c.P
    assert torch.equal(bits(through), bits(base.reshape(-1))), "%s: by=%r gives other bits (up to %.3e)" % (
        c.name, other, float((through - base.reshape(-1)).abs().max()))


WS_CASES = [c for c in C.CASES if c.kernel == 'scores' and not c.abi and
            ((c.group == 'norm' and c.norm == C.DEFAULT and c.agg == 'LogSumExp') or (c.group == 'long' and c.tag == 'first.middle') or
             (c.group == 'count' and c.tag in ('K9', 'empty.run')))]


@pytest.mark.parametrize("case", WS_CASES, ids=lambda c: c.name)
def test_one_workspace_serves_every_norm_and_aggregation(dev, case):
    c = case
    img, words, plan = device_inputs(c, dev)
    ws = ops.scan_pairs_prepare(img, words, plan, c.xa)
    for norm, agg in (('clipped_l2norm', 'LogSumExp'), ('no_norm', 'Sum'), ('softmax', 'Max'), ('l1norm', 'Mean'), ('clipped_l2norm', 'LogSumExp')):
        got = ops.scan_candidate_scores(img, words, plan, i32(c.cand, dev), c.by, workspace=ws, **settings(c, norm, agg))
        fresh = list_scores(c, dev, norm=norm, agg=agg)
        assert torch.equal(bits(got), bits(fresh)), "%s %s %s: the reused workspace gives other bits (up to %.3e)" % (
            c.name, norm, agg, float((got - fresh).abs().max()))
        a = ops.scan_pair_attention(img, words, plan, i32(c.pairs, dev).view(-1, 2), workspace=ws, **settings(c, norm, agg))
        b = ops.scan_pair_attention(img, words, plan, i32(c.pairs, dev).view(-1, 2), **settings(c, norm, agg))
        assert all(torch.equal(bits(getattr(a, t)), bits(getattr(b, t))) for t in ('attn', 'row_sim', 'score')), (c.name, norm, agg)


def test_attention_scores_are_the_score_kernels_bits(dev):
    """scan_attn.hip: "so that scores agree".  Over the whole table, for every pair whose caption has at most 64 words."""
    missing = [c for c in C.CASES if c.kernel == 'attention' and c.name not in VS_SCORES]
    for c in missing:           # (run alone: measure here)
        try:
            check_attention(c, dev)
        except AssertionError:
            pass
    print("attention score vs scan_candidate_scores: %d cases, largest difference %.3e, bit-equal for <= 64 words in %d" % (
        len(VS_SCORES), max(d for d, _ in VS_SCORES.values()), sum(eq for _, eq in VS_SCORES.values())))
    assert len(VS_SCORES) == len([c for c in C.CASES if c.kernel == 'attention'])
    assert all(eq for _, eq in VS_SCORES.values()), sorted(k for k, (_, eq) in VS_SCORES.items() if not eq)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own index guards: a refused pair stays NaN, every other pair is right
def guard_case(xa):
    c, = C.cases('scores', xa, 'abi')
    return c


def refused_and_others(c, buf, refused):
    want, _, _, tol, _ = c.reference()['score']
    got = buf[:c.P]
    assert refused and bool(torch.isnan(got[refused]).all()), "%s: a refused pair was scored: %s" % (c.name, got[refused].tolist())
    keep = [s for s in range(c.P) if s not in refused]
    err = float(torch.nan_to_num((got[keep].double() - want[keep]).abs(), nan=float('inf')).max())
    assert keep and err <= tol, "%s: beside refused pairs, max err %.3e, tol %.3e" % (c.name, err, tol)


@pytest.mark.parametrize("xa", C.DIRECTIONS)
def test_an_output_slot_behind_out_len_stays_nan(dev, xa):
    c = guard_case(xa)
    moved = [s for s in range(c.P) if s % 5 == 2]            # these pairs name slots P .. P + len(moved) - 1, inside the longer buffer
    slot_of = lambda s: c.P + moved.index(s) if s in moved else s
    buf, _ = direct_scores(c, dev, slot_of, out_len=c.P, buf_len=c.P + len(moved) + ABI_TAIL)
    assert bool(torch.isnan(buf[c.P:]).all()), "a slot >= out_len was written: %s" % buf[c.P:].tolist()
    refused_and_others(c, buf, moved)


@pytest.mark.parametrize("declared", [0, 65])
@pytest.mark.parametrize("xa", C.DIRECTIONS)
def test_a_caption_declared_outside_1_to_64_words_scores_nan(dev, xa, declared):
    c = guard_case(xa)
    k = 1                                                      # 17 words, 9 pairs (two blocks), 65 rows exist behind its first
    assert c.plan.counts[k] == 9 and c.off[k] + 65 <= c.n_tok
    buf, _ = direct_scores(c, dev, call_len={k: declared}, buf_len=c.P + ABI_TAIL)
    assert bool(torch.isnan(buf[c.P:]).all())
    refused_and_others(c, buf, [s for s, (_, kk) in enumerate(c.pairs) if kk == k])


@pytest.mark.parametrize("xa", C.DIRECTIONS)
def test_an_image_index_behind_the_declared_count_scores_nan(dev, xa):
    c = guard_case(xa)
    refused = [s for s, (i, _) in enumerate(c.pairs) if i == c.Ni - 1]
    buf, _ = direct_scores(c, dev, Ni=c.Ni - 1, buf_len=c.P + ABI_TAIL)
    assert bool(torch.isnan(buf[c.P:]).all())
    refused_and_others(c, buf, refused)
