"""GPU: the SGRAF candidate-list kernels (csrc/sgraf_pairs.hip through ops.sgraf_candidate_scores, csrc/sgraf_attn.hip through
ops.sgraf_pair_attention) at every case of tests/helpers/sgraf_pairs_cases.py against the float64 oracle -- every score of every list,
and for the attention entry the whole of `attn`, `node_w` / `edge` and `score`.

Tolerance per case and tensor: 16 * max(e32_oracle, e32_mirror, 2^-24 max|want|) (tests/helpers/sgraf_pairs_cases.py;
tests/test_sgraf_pairs_case_table.py proves on the CPU that it is never looser than the flat bounds of the older tests and that it sees
each claimed defect at 10 x), or the older flat bound where that is smaller: the float32 references are matrix products and their
rounding depends on the BLAS that runs them.  Every output is finite, a second call on fresh tensors gives the same bits, a run under
the case's workspace budget gives the bits of the one-chunk run in as many chunks, and with as many workspace bytes, as the Python mirror counts.
The device plan (pair_len, pair_col, pair_capok, item_begin, item_img, n_items through ops._sgraf_item_plan) is the mirror's, element
for element.  Row sums: every row of `attn`, `node_w` and `edge` sums to 1 within the tensor's bound + n x 2^-24 (the kernel divides
the row by its own n-term float32 sum) + |s - 1|, s the float64 row's sum (1, or 1 - 1e-8 / sum for AttentionFiltration's l1norm); never
looser than the older tests' 1e-5.  The explained scores
are held to the score bound against sgraf_candidate_scores (not bit-equal, other summation orders).

The direct calls hand itr_sgraf_pairs_plan, itr_sgraf_pair_scores and itr_sgraf_pair_attention CSR input that ops never makes, built
so that a broken guard reads and writes only memory the test owns (Nc, out_len and aux_len are DECLARED smaller than the tensors):
  caption index -1 / >= Nc, rows behind n_rows    sgraf_pairs.hip:55-58, before cap_len[c] / cap_off[c]; the pair becomes a one-word slot
                                                  with pair_capok -1, which :138, :201 and :248 test before any read through it
  a pair_out slot outside out_len                 sgraf_pairs.hip:260 / sgraf_attn.hip:63, before the store / before attn_ptr[o]
  an edge / node_w block outside aux_len          sgraf_attn.hip:66-69 (reason_out_ok), called at :147 and :335 before any block access
A refused pair's score is NaN where its slot is valid, and nothing else of it is written.
profiles/sgraf_pairs_seams/measured.txt is the record of one run (ITR_SGRAF_PAIRS_SEAMS_RECORD=<file> appends one line per case)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from itr_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sgraf_pairs_cases as C        # noqa: E402

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("ITR_SGRAF_PAIRS_SEAMS_RECORD")
NAN = float('nan')
_WEIGHTS = {}


def i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.int32))).to(dev)


def i64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.int64))).to(dev)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def device_inputs(c, dev):
    """Fresh device tensors and a fresh plan of the case: (images, packed words, ScanPlan, weights)."""
    x = c.inputs()
    plan = ops.ScanPlan(np.asarray(c.off, np.int64), np.asarray(c.lens, np.int32), c.n_tok, dev)
    key = id(c.weights)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = {k: v.contiguous().to(dev) for k, v in c.weights.items()}
    return x['images'].contiguous().to(dev), x['words'].contiguous().to(dev), plan, _WEIGHTS[key]


def list_scores(c, dev, budget=None):
    """ops.sgraf_candidate_scores on fresh tensors -> (flat scores on the host, ops.SGRAF_PAIRS_LAST of the call)"""
    img, words, plan, w = device_inputs(c, dev)
    out = ops.sgraf_candidate_scores(img, words, plan, w, i32(c.cand, dev), c.by, module_name=c.mod, sgr_step=c.steps, max_workspace_bytes=budget)
    assert out.shape == (len(c.cand), c.K)
    return out.reshape(-1).cpu(), dict(ops.SGRAF_PAIRS_LAST)


def pair_attention(c, dev, budget=None):
    """ops.sgraf_pair_attention on fresh tensors -> ({tensor: flat float32 on the host}, the result, ops.SGRAF_ATTN_LAST of the call)"""
    img, words, plan, w = device_inputs(c, dev)
    a = ops.sgraf_pair_attention(img, words, plan, w, i32(c.pairs, dev).view(-1, 2), module_name=c.mod, sgr_step=c.steps, max_workspace_bytes=budget)
    aux = a.node_w if c.mod == 'SAF' else a.edge
    assert (a.edge if c.mod == 'SAF' else a.node_w) is None and len(a) == c.P
    return {'attn': a.attn.cpu(), c.aux: aux.cpu(), 'score': a.score.cpu()}, a, dict(ops.SGRAF_ATTN_LAST)


def compare(c, got, fails):
    ref, figures = c.reference(), []
    for t in c.tensors:
        want, e_oracle, e_mirror, tol, _ = ref[t]
        tol = min(tol, C.OLD[t])             # the float32 references' error moves with the host's BLAS: never looser than the older tests
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


def record(c, figures, extra):
    line = "; ".join("%s e32_oracle %.3e e32_mirror %.3e tol %.3e err %.3e ratio %.3f" % (t, eo, em, tol, err, err / tol) for t, eo, em, tol, err in figures)
    print("%s: %s | %s" % (c.name, line, extra))
    if RECORD:
        with open(RECORD, "a") as f:
            f.write("%s | %s | %s | %s\n" % (c.name, c.describe(), line, extra))


def check_device_plan(c, dev, fails):
    """itr_sgraf_pairs_plan on the image-major list the mirror made of the case's pairs"""
    p = c.plan
    (pair_len, pair_col, pair_capok, item_begin, item_img), n_items, ib = ops._sgraf_item_plan(
        _lib.load(), i32(p.img_ptr, dev), i32(p.pair_cap, dev), i64(c.off, dev), i32(p.klen, dev), p.P, c.Ni, c.Nc, c.n_tok, dev)
    if n_items != p.n_items:
        fails.append("the device plans %d items, the mirror %d" % (n_items, p.n_items))
        return
    for name, dev_t, mine in (('pair_len', pair_len, p.pair_len), ('pair_col', pair_col, p.pair_col), ('pair_capok', pair_capok, p.pair_capok),
                              ('item_begin', item_begin[:n_items + 1], p.item_begin), ('item_img', item_img[:n_items], p.item_img)):
        if dev_t.cpu().tolist() != list(mine):
            fails.append("the device plan's %s is not the mirror's" % name)
    if ib.tolist() != list(p.item_begin):
        fails.append("the item bounds read back are not the mirror's")


def chunk_facts(c, last, fails):
    p = c.plan
    if last['chunks'] != len(p.chunks) or last['items'] != p.n_items or last['pairs'] != p.P:
        fails.append("the library ran %d chunks of %d items, %d pairs; the mirror counts %d, %d, %d" % (
            last['chunks'], last['items'], last['pairs'], len(p.chunks), p.n_items, p.P))
    if last['workspace_bytes'] != max(p.need(a, b) for a, b in p.chunks):
        fails.append("the workspace has %d bytes, the mirror counts %d" % (last['workspace_bytes'], max(p.need(a, b) for a, b in p.chunks)))


def check_scores(c, dev):
    fails = []
    got, last = list_scores(c, dev, c.plan.budget)
    chunk_facts(c, last, fails)
    figures = compare(c, {'score': got}, fails)
    again, _ = list_scores(c, dev, c.plan.budget)
    same = torch.equal(bits(got), bits(again))
    if not same:
        fails.append("a second run gives other bits")
    if c.plan.budget:
        whole, last1 = list_scores(c, dev)
        if last1['chunks'] != 1:
            fails.append("the unbudgeted run took %d chunks" % last1['chunks'])
        if not torch.equal(bits(whole), bits(got)):
            fails.append("%d chunks give other bits than one (up to %.3e)" % (last['chunks'], float((whole - got).abs().max())))
    check_device_plan(c, dev, fails)
    record(c, figures, "repeat %s | chunks %d" % ('equal' if same else 'DIFFERENT', last['chunks']))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


def row_sums(c, got, a, fails):
    """-> the largest |row sum - 1| over attn (per word), node_w (per pair) and edge (per querying node)"""
    ref = c.reference()
    worst = 0.0

    def check(name, rows, want_rows, n):
        nonlocal worst
        # the tensor's bound, + n * 2^-24 for the kernel's own denominator (an n-term float32 sum that the row is divided by),
        # + what the float64 row itself misses 1 by (AttentionFiltration's l1norm: 1e-8 / sum); never looser than the older 1e-5
        bound = min(min(ref[name][3], C.OLD[name]) + n * C.U + float((want_rows.sum(1) - 1.0).abs().max()), C.OLD_SUM)
        e = float(torch.nan_to_num((rows.double().sum(1) - 1.0).abs(), nan=float('inf')).max())
        worst = max(worst, e)
        if not e <= bound:
            fails.append("%s rows of %d terms sum to 1 +- %.3e (bound %.3e)" % (name, n, e, bound))

    if got['attn'].numel() == ref['attn'][0].numel():
        check('attn', got['attn'].view(-1, C.SC_R), ref['attn'][0].view(-1, C.SC_R), C.SC_R)
    if got[c.aux].numel() == ref[c.aux][0].numel():
        o = 0
        for s, (_, k) in enumerate(c.pairs):
            if c.short(s):
                n = c.lens[k] + 1
                m = n if c.mod == 'SAF' else c.steps * n * n
                check(c.aux, got[c.aux][o:o + m].view(-1, n), ref[c.aux][0][o:o + m].view(-1, n), n)
                o += m
    return worst


def check_attention(c, dev):
    fails = []
    got, a, last = pair_attention(c, dev, c.plan.budget)
    chunk_facts(c, last, fails)
    short = [c.short(s) for s in range(c.P)]
    W = [c.lens[k] if ok else 0 for ok, (_, k) in zip(short, c.pairs)]
    if a.explained.cpu().tolist() != short or a.cap_len.cpu().tolist() != [c.lens[k] for _, k in c.pairs]:
        fails.append("explained / cap_len are not the list's")
    if a.attn_ptr.cpu().tolist() != np.concatenate([[0], np.cumsum(np.asarray(W, np.int64) * C.SC_R)]).tolist():
        fails.append("attn_ptr is not the prefix of W x 36 (0 for a caption of more than 63 words)")
    aux_n = [0 if not w else (w + 1 if c.mod == 'SAF' else c.steps * (w + 1) ** 2) for w in W]
    if (a.node_ptr if c.mod == 'SAF' else a.edge_ptr).cpu().tolist() != np.concatenate([[0], np.cumsum(np.asarray(aux_n, np.int64))]).tolist():
        fails.append("%s_ptr is not the prefix of the blocks" % c.aux[:4])
    figures = compare(c, got, fails)
    e_sum = row_sums(c, got, a, fails)
    again, _, _ = pair_attention(c, dev, c.plan.budget)
    same = all(torch.equal(bits(got[t]), bits(again[t])) for t in got)
    if not same:
        fails.append("a second run gives other bits")
    if c.plan.budget:
        whole, _, last1 = pair_attention(c, dev)
        if last1['chunks'] != 1:
            fails.append("the unbudgeted run took %d chunks" % last1['chunks'])
        for t in got:
            if not torch.equal(bits(whole[t]), bits(got[t])):
                fails.append("%s: %d chunks give other bits than one" % (t, last['chunks']))
    # the score-only path on the same pairs (documented as not bit-equal)
    sc, _ = list_scores(c, dev)
    d = float(torch.nan_to_num((sc.double() - got['score'].double()).abs(), nan=float('inf')).max())
    tol_score = min(c.reference()['score'][3], C.OLD['score'])
    if not d <= tol_score:
        fails.append("the score differs from sgraf_candidate_scores' by %.3e, tol %.3e" % (d, tol_score))
    check_device_plan(c, dev, fails)
    record(c, figures, "repeat %s | chunks %d | sums-1 %.3e | vs scores %.3e" % ('equal' if same else 'DIFFERENT', last['chunks'], e_sum, d))
    assert not fails, "%s: %s" % (c.name, "; ".join(fails))


GROUPS = sorted(set((c.kernel, c.group, c.mod) for c in C.CASES))


@pytest.mark.parametrize("kernel,group,mod", GROUPS, ids=lambda v: str(v))
def test_sgraf_pairs_seams_vs_float64(dev, kernel, group, mod):
    cs = C.cases(kernel, group, mod)
    assert cs
    failed = []
    for c in cs:
        try:
            (check_scores if kernel == 'scores' else check_attention)(c, dev)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------------------
# direct calls of the C entry points
def behind(t):
    """The same values as a view that starts one element behind its allocation's first: index -1 of a broken guard stays inside it."""
    return torch.cat([t[:1], t])[1:]


def base_case(kernel, mod):
    c, = [c for c in C.cases(kernel, 'lists', mod) if c.by == 'image' and c.K == 10]
    return c


NC_DECLARED = 7             # of the base case's 9 captions: indices 7 and 8 lie inside the tensors and outside the declared count


def hand_made_csr(c):
    """Four images, the second one with no pairs; the entries name captions -1, 7 and 8 beside valid ones -> (img_ptr, pair_img, pair_cap)"""
    assert c.Nc == 9 and c.Ni >= 4 and max(c.lens) <= C.GP_MAXW
    per_img = [[0, -1, 3, 7, 2, 5], [], [6, 8, 1, 1, 4], [5, 0, 6]]
    img_ptr = [0]
    for v in per_img:
        img_ptr.append(img_ptr[-1] + len(v))
    return img_ptr, [i for i, v in enumerate(per_img) for _ in v], [k for v in per_img for k in v]


@pytest.mark.parametrize("mod", C.MODS)
def test_plan_entry_on_hand_made_csr(dev, mod):
    """itr_sgraf_pairs_plan alone: an empty image range, caption indices -1 and >= the declared Nc, and -- with n_rows declared one row
    short of the last declared caption's end -- rows behind n_rows.  The offset and length tensors hold all 9 captions."""
    c = base_case('scores', mod)
    img_ptr, pair_img, pair_cap = hand_made_csr(c)
    for n_rows in (c.n_tok, c.off[NC_DECLARED - 1] + c.lens[NC_DECLARED - 1] - 1):
        want = C.item_plan(img_ptr, pair_cap, c.off, c.plan.klen, NC_DECLARED, n_rows)
        refused = [q for q, k in enumerate(pair_cap) if not 0 <= k < NC_DECLARED or c.off[k] + c.lens[k] > n_rows]
        assert [q for q, k in enumerate(want[2]) if k < 0] == refused and len(refused) == (3 if n_rows == c.n_tok else 5)
        (pair_len, pair_col, pair_capok, item_begin, item_img), n_items, ib = ops._sgraf_item_plan(
            _lib.load(), i32(img_ptr, dev), i32(pair_cap, dev), behind(i64(c.off, dev)), behind(i32(c.plan.klen, dev)), len(pair_cap), 4, NC_DECLARED,
            n_rows, dev)
        got = (pair_len.cpu().tolist(), pair_col.cpu().tolist(), pair_capok.cpu().tolist(), item_begin[:n_items + 1].cpu().tolist(),
               item_img[:n_items].cpu().tolist(), n_items)
        assert got == want, (n_rows, got, want)
        assert 1 not in want[4]                                     # the image with no pairs has no item


def direct_setup(c, dev):
    """The hand-made list planned on the device with Nc declared 7, and a state prepared for the first 7 captions (the state is ONE buffer:
    a global vector read for caption 7 or 8 through a broken guard lies in the Gram matrices behind cap_glo, inside it)."""
    lib = _lib.load()
    img, words, _, w = device_inputs(c, dev)
    plan7 = ops.ScanPlan(np.asarray(c.off[:NC_DECLARED], np.int64), np.asarray(c.lens[:NC_DECLARED], np.int32), c.n_tok, dev)
    state = ops.sgraf_pairs_prepare(img, words, plan7, w, c.mod, c.steps)
    img_ptr, pair_img, pair_cap = hand_made_csr(c)
    off = behind(i64(c.off, dev))
    plan_t, n_items, ib = ops._sgraf_item_plan(lib, i32(img_ptr, dev), i32(pair_cap, dev), off, behind(i32(c.plan.klen, dev)), len(pair_cap), 4,
                                               NC_DECLARED, c.n_tok, dev)
    return lib, img, words, w, state, off, i32(pair_img, dev), pair_cap, plan_t, n_items


def reference_of(c, pair_img, pair_cap):
    """float64 scores of the hand-made pairs from a case over the same inputs, all images x all captions"""
    full = C.PairCase('scores', c.group, c.tag, c.mod, c.Ni, c.D, c.S, c.lens, [list(range(c.Nc))] * c.Ni, 'image', steps=c.steps)
    full.name = c.name                                               # the same seed: the same inputs
    ref = full.reference()['score']
    S = ref[0].view(c.Ni, c.Nc)
    return [float(S[i, k]) if 0 <= k < NC_DECLARED else NAN for i, k in zip(pair_img, pair_cap)], ref[3]


@pytest.mark.parametrize("mod", C.MODS)
def test_scores_entry_guards_leave_nan_and_touch_nothing_else(dev, mod):
    c = base_case('scores', mod)
    lib, img, words, w, state, off, pair_img, pair_cap, (pair_len, pair_col, pair_capok, item_begin, item_img), n_items = direct_setup(c, dev)
    P = len(pair_cap)
    want, tol = reference_of(c, pair_img.cpu().tolist(), pair_cap)
    TAIL = 8
    moved = 4                                                         # this pair names slot P + 3: inside the buffer, outside out_len
    slots = [P + 3 if q == moved else q for q in range(P)]
    buf = torch.full((P + TAIL,), NAN, device=dev, dtype=torch.float32)
    m = 0 if mod == 'SAF' else 1
    wsb = lib.itr_sgraf_pair_scores_workspace_bytes(P, n_items, c.D, c.S, m, c.steps)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    pair_out = i32(slots, dev)
    _lib.check(lib.itr_sgraf_pair_scores(ops._p(img), ops._p(words), ops._p(off), ops._p(pair_img), ops._p(pair_capok), ops._p(pair_len), ops._p(pair_col),
                                         ops._p(pair_out), ops._p(item_begin), ops._p(item_img), 0, P, 0, n_items, c.Ni, NC_DECLARED, c.n_tok, C.SC_R, c.D,
                                         c.S, m, c.steps, ctypes.byref(state.struct), ops._p(state.buf), state.buf.numel(), ops._p(buf), P,
                                         ops._p(ws), wsb, ops._stream()))
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[P:]).all()), "a slot >= out_len was written: %s" % got[P:].tolist()
    for q in range(P):
        if q == moved or want[q] != want[q]:
            assert got[q] != got[q], "pair %d (caption %d) was refused and yet scored %r" % (q, pair_cap[q], float(got[q]))
        else:
            assert abs(float(got[q]) - want[q]) <= tol, "beside refused pairs, pair %d is %.3e off (tol %.3e)" % (q, abs(float(got[q]) - want[q]), tol)


@pytest.mark.parametrize("mod", C.MODS)
def test_attention_entry_unaligned_blocks_and_guards(dev, mod):
    """itr_sgraf_pair_attention on the hand-made list: `attn` handed over one float behind a 16-byte boundary (the scalar branch of
    sgraf_attn_scatter_kernel) gives the bits of the aligned call; a slot outside out_len and a node_w / edge block that does not fit
    the declared aux_len leave NaN and touch nothing else."""
    c = base_case('attention', mod)
    lib, img, words, w, state, off, pair_img, pair_cap, (pair_len, pair_col, pair_capok, item_begin, item_img), n_items = direct_setup(c, dev)
    P = len(pair_cap)
    want, tol = reference_of(c, pair_img.cpu().tolist(), pair_cap)
    ok = [0 <= k < NC_DECLARED for k in pair_cap]
    Wq = [c.lens[k] if good else 0 for good, k in zip(ok, pair_cap)]
    blk = [0 if not n else (n + 1 if mod == 'SAF' else c.steps * (n + 1) ** 2) for n in Wq]
    attn_ptr = np.concatenate([[0], np.cumsum(np.asarray(Wq, np.int64) * C.SC_R)])
    aux_ptr = np.concatenate([[0], np.cumsum(np.asarray(blk, np.int64))])
    moved, TAIL = 4, 8
    slots = [P + 3 if q == moved else q for q in range(P)]            # pair q writes slot q: the pointers are indexed by slot
    last = max(q for q in range(P) if ok[q])                          # the last valid pair's aux block ends at aux_ptr[-1]
    assert aux_ptr[last + 1] == aux_ptr[-1] and last != moved
    m = 0 if mod == 'SAF' else 1
    wsb = lib.itr_sgraf_pair_attention_workspace_bytes(P, n_items, c.D, c.S, m, c.steps)
    # (the pointer tensors run on behind slot P with their last value: a broken slot guard would still read inside them)
    pair_out, attn_ptr_d, aux_ptr_d = i32(slots, dev), i64(list(attn_ptr) + [attn_ptr[-1]] * TAIL, dev), i64(list(aux_ptr) + [aux_ptr[-1]] * TAIL, dev)

    def call(shift, aux_len):
        attn = torch.full((shift + int(attn_ptr[-1]) + TAIL,), NAN, device=dev, dtype=torch.float32)
        aux = torch.full((int(aux_ptr[-1]) + TAIL,), NAN, device=dev, dtype=torch.float32)
        score = torch.full((P + TAIL,), NAN, device=dev, dtype=torch.float32)
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        view = attn[shift:]
        assert view.data_ptr() % 16 == 4 * shift
        node_args = (ops._p(aux), ops._p(aux_ptr_d), aux_len, None, None, 0) if mod == 'SAF' else (None, None, 0, ops._p(aux), ops._p(aux_ptr_d), aux_len)
        _lib.check(lib.itr_sgraf_pair_attention(
            ops._p(img), ops._p(words), ops._p(off), ops._p(pair_img), ops._p(pair_capok), ops._p(pair_len), ops._p(pair_col), ops._p(pair_out),
            ops._p(item_begin), ops._p(item_img), 0, P, 0, n_items, c.Ni, NC_DECLARED, c.n_tok, C.SC_R, c.D, c.S, m, c.steps, ctypes.byref(state.struct),
            ops._p(state.buf), state.buf.numel(), ops._p(view), ops._p(attn_ptr_d), int(attn_ptr[-1]), *node_args, ops._p(score), P, ops._p(ws), wsb,
            ops._stream()))
        torch.cuda.synchronize()
        return attn.cpu(), aux.cpu(), score.cpu()

    attn0, aux0, score0 = call(0, int(aux_ptr[-1]))
    attn1, aux1, score1 = call(1, int(aux_ptr[-1]))
    assert bool(torch.isnan(attn1[:1]).all()) and torch.equal(bits(attn1[1:]), bits(attn0)), "the unaligned scatter gives other bits"
    assert torch.equal(bits(aux1), bits(aux0)) and torch.equal(bits(score1), bits(score0))
    # refused: captions -1 / 7 / 8 (by the plan), the moved slot; everything else is written and right
    for buf_, n in ((attn0, int(attn_ptr[-1])), (aux0, int(aux_ptr[-1])), (score0, P)):
        assert bool(torch.isnan(buf_[n:]).all()), "floats behind the declared length were written"
    for q in range(P):
        a_blk, x_blk = attn0[attn_ptr[q]:attn_ptr[q + 1]], aux0[aux_ptr[q]:aux_ptr[q + 1]]
        if q == moved or not ok[q]:
            assert score0[q] != score0[q] and bool(torch.isnan(a_blk).all()) and bool(torch.isnan(x_blk).all()), q
        else:
            assert abs(float(score0[q]) - want[q]) <= tol and bool(torch.isfinite(a_blk).all()) and bool(torch.isfinite(x_blk).all()), q
    # aux_len one float short of the last valid pair's block: that pair alone is refused as well
    attn2, aux2, score2 = call(0, int(aux_ptr[-1]) - 1)
    keep = [q for q in range(P) if q != last]
    assert score2[last] != score2[last] and bool(torch.isnan(attn2[attn_ptr[last]:attn_ptr[last + 1]]).all())
    assert bool(torch.isnan(aux2[aux_ptr[last]:]).all())
    assert torch.equal(bits(score2[keep]), bits(score0[keep])) and torch.equal(bits(aux2[:aux_ptr[last]]), bits(aux0[:aux_ptr[last]]))
    assert torch.equal(bits(attn2[:attn_ptr[last]]), bits(attn0[:attn_ptr[last]])) and torch.equal(bits(attn2[attn_ptr[last + 1]:]), bits(attn0[attn_ptr[last + 1]:]))
