"""Case table of the SGRAF candidate-list kernels (csrc/sgraf_pairs.hip + sgraf_pairs.h behind ops.sgraf_candidate_scores,
csrc/sgraf_attn.hip behind ops.sgraf_pair_attention) and their float64 references.

One entry per (kernel, module, images, D, sim_dim, caption lengths, pair list, graph steps, workspace budget).  `kernel` is 'scores' (the
list arrives as `cand` + `by`) or 'attention' (the same lists flattened to [P, 2] pairs).  Inputs by sgraf_eval_cases.SgrafCase._make,
seeded from the case's name; the weights are sgraf_eval_cases.weights (the SHARPENED ones), never the plain Xavier ones.

REFERENCES, on the listed images and captions only (a pair's score depends on its own operands; VisualSA's BatchNorm runs on running
statistics), every tensor flat in the caller's order:
    oracle   scores: sgraf_eval_cases.oracle.  attention: sgraf_explain_oracle.sgraf_similarity_explained (`attn`, `node_w` | `edge`,
             `score`).  float64 = want, float32 -> e32_oracle
    mirror   sgraf_eval_cases.mirror up to the node rows (folded query, Gram-form ||ctx||, ...); scores: its own SAF / SGR stage;
             attention: `reason` below, sgraf_reason_kernel's algebra -- the folded query, ALL nodes at every step, SAF as normalised
             weights, then the aggregate, then l2norm.  float32 -> e32_mirror, float64 == oracle to MIRROR_AGREES
Tolerance per tensor: FACTOR * max(e32_oracle, e32_mirror, U * max|want|), proved by tests/test_sgraf_pairs_case_table.py to be at most
the older flat bounds (scores 5e-6; attn / node_w / edge 2e-5).

The planning is mirrored in plain Python, each function marked with the source lines it copies: the greedy item planner, the prefix
kernel's per-thread ranges, the chunk workspace's byte count, ops._chunks_within, per item the node rows, row tiles and fused-group class.

Defects, all float64, numbered as the CPU test restates them (PairCase.claims says which a case claims):
     1  a pair reads the columns of the next pair of its item (wrong pair_col)                       node rows re-gathered
     2  an item of a later chunk scored against the image of item t - it0 (item_img not rebased)     want, re-gathered
     3  cap_col not rebased by it0 * 64 in a later chunk: the columns of item t + it0                node rows re-gathered
     4  the global node of pair j of a later chunk taken from pair j - p0                            node rows re-gathered
     5  the items of images >= 1024 numbered from zero (prefix stride)                               node rows re-gathered
     6  the last node counted twice in the SAF weights / the edge softmax (tail mask)                mirror
     7  the last word of every caption of more than one word dropped                                 oracle on changed inputs
     8  Gram-form ||ctx|| with the off-diagonal terms counted once                                   mirror
     9  region 35 zeroed; 90: the last feature zeroed (D <= 96 only: sgraf_eval_cases, defect a)     oracle on changed inputs
    10  the results rotated by one inside each list (pair_out)                                       want, re-laid
    11  a caption of more than 63 words truncated to 63                                              oracle on changed inputs
    12  attention, SGR: a caption's softmax rows include the first node of the item's next caption   mirror
    13  attention, SAF: the weights normalised over the item instead of the caption                  mirror
    14  attention, SGR: step k's edges written into step k - 1's block                               want, re-laid
1 .. 9 go through the stages both entries share (sgraf_pairs_nodes) and are claimed by both kernels; an attention case shows them on
its score.  The cases of more than 300 pairs or 1000 images claim only what their size is there for (5, 10).  SAF at sim_dim != 256
through the scores entry walks one node per trip: no 6 there.  Nothing here imports the library."""
import torch

import sgraf_eval_cases as E
import sgraf_explain_oracle as X
from scan_pairs_cases import lists_by_caption
from sgraf_eval_cases import MIRROR_AGREES, FALLBACK_SHARE, MIN_SHARP, MIN_SPAN, OLD_BOUND, ceil_div, _offsets      # noqa: F401
from train_prim_cases import Case, U, FACTOR, SENSITIVITY      # noqa: F401

OLD_ATTN = 2e-5             # tests/test_sgraf_attention_gpu.py TOL_ATTN: attn, node_w, edge
OLD_SUM = 1e-5              # ... TOL_SUM: every softmax / l1 row sum
OLD = {'score': OLD_BOUND, 'attn': OLD_ATTN, 'node_w': OLD_ATTN, 'edge': OLD_ATTN}

# geometry (pinned to csrc/ and ops.py by tests/test_sgraf_pairs_case_table.py)
SC_R = E.SC_R
GP_PAIRS, GP_MAXW, GP_ITEM, GP_MAXCAP = 8, 63, 64, 16                 # sgraf_pairs.h:11-15
GR_WAVES, GR_MAXS, GR_LDE = 4, 256, 68                                # sgraf_attn.hip:42-45
PREFIX_THREADS, PLAN_THREADS, INDEX_THREADS = 1024, 256, 256          # sgraf_pairs.hip:77, :40, :101
PER_WG = 4                                                            # pairs / columns per workgroup: colsrc, gather (sgraf_pairs.hip:196, :206), scatter (sgraf_attn.hip:330)
GROUP_META_BYTES = 512                                                # sgr_fused.hip: sizeof(SgrGroupMeta)
MAX_COMPOSED = 191                                                    # ops.py SGRAF_COMPOSED_MAX_WORDS

KERNELS = ('scores', 'attention')
SEAMS = {}          # kernel -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule and that are judged by a derived a-priori bound instead:
# name -> {tensor: bound}, the derivation in a comment next to the entry.  No case needs it (profiles/sgraf_pairs_seams/measured.txt).
FALLBACK = {}


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the planning
def prefix_ranges(n):
    """sgraf_pairs.hip:81-82 (sgraf_pairs_prefix_kernel): (per, [(b, e) of thread t])."""
    per = (n + PREFIX_THREADS - 1) // PREFIX_THREADS
    out = []
    for t in range(PREFIX_THREADS):
        b = t * per if t * per < n else n
        out.append((b, b + per if b + per < n else n))
    return per, out


def prefix_items(counts):
    """sgraf_pairs.hip:77-97, thread by thread: per-thread partial sums, their exclusive scan by thread 0, the running offsets.
    -> (first item of every image, total)."""
    n = len(counts)
    _, ranges = prefix_ranges(n)
    part = [sum(counts[b:e]) for b, e in ranges]
    run, starts = 0, []
    for v in part:
        starts.append(run)
        run += v
    out = [0] * n
    for (b, e), r in zip(ranges, starts):
        for i in range(b, e):
            out[i] = r
            r += counts[i]
    return out, run


def item_plan(img_ptr, pair_cap, cap_off, cap_len, Nc, n_rows):
    """sgraf_pairs.hip:46-73 (sgraf_pairs_plan_kernel, pass 0 and pass 1 around the prefix kernel): one walk per image in list order; a
    caption opens a new item when the current one has 16 captions or rows + len + 1 > 64.
    -> (pair_len, pair_col, pair_capok, item_begin[n_items + 1], item_img, n_items)."""
    Ni, P = len(img_ptr) - 1, len(pair_cap)
    pair_len, pair_col, pair_capok = [0] * P, [0] * P, [0] * P
    for PASS in (0, 1):
        if PASS:
            base, n_items = prefix_items(img_items)
            item_begin, item_img = [0] * (n_items + 1), [0] * n_items
            item_begin[n_items] = P                                        # :91
        else:
            img_items = [0] * Ni
        for i in range(Ni):
            b = min(max(img_ptr[i], 0), P)                                 # :48-50
            e = min(max(img_ptr[i + 1], b), P)
            item = base[i] if PASS else 0
            ncap = rows = n = 0
            for p in range(b, e):
                c = pair_cap[p]
                ln = cap_len[c] if 0 <= c < Nc else 0                      # :55
                ok = 1 <= ln <= GP_MAXW
                if ok:
                    ok = cap_off[c] >= 0 and cap_off[c] + ln <= n_rows      # :57
                if not ok:
                    ln = 1
                if n == 0 or ncap == GP_MAXCAP or rows + ln + 1 > GP_ITEM:  # :59
                    if n:
                        item += 1
                    n += 1
                    ncap = rows = 0
                    if PASS:
                        item_begin[item], item_img[item] = p, i
                if PASS:
                    pair_len[p], pair_col[p], pair_capok[p] = ln, item * GP_ITEM + (rows - ncap), (c if ok else -1)      # :66-68
                ncap += 1
                rows += ln + 1
            if not PASS:
                img_items[i] = n
    return pair_len, pair_col, pair_capok, item_begin, item_img, n_items


def align256(v):
    return (v + 255) & ~255


def fused_ws_bytes(n_groups, n_caps):
    """sgr_fused.hip:913-926 (sgr_carve) at sgr_step 0: the group records only."""
    return sum(align256(v) for v in (n_groups * GROUP_META_BYTES, n_groups, 2 * n_groups * 4, 256, n_caps * 4, 0, 256))


def chunk_bytes(n_pairs, n_items, D, S, sgr, with_steps=True):
    """sgraf_pairs.h:45-70 (gp_chunk): the workspace of a chunk; with_steps False: itr_sgraf_pair_attention's."""
    ncols = n_items * GP_ITEM
    fused = sgr and S == 256
    take = [ncols * D * 4, ncols * SC_R * 4, ncols * 4, ncols * S * 4]
    if S != 256:
        take.append(ncols * D * 4)
    take += [n_pairs * D * 4, n_pairs * S * 4]
    if sgr and with_steps:
        take.append(n_pairs * S * 4)
        take += [fused_ws_bytes(n_items, n_pairs), 256] if fused else [ncols * S * 4, ncols * S * 4, n_pairs * S * 4]
    take += [n_pairs * 4, ncols * 8, n_pairs * 4, n_pairs * 4, (n_items + 1) * 4]
    return sum(align256(v) for v in take)


def chunks_within(need, n_items, budget):
    """ops.py:1739-1755 (_chunks_within): the fewest chunks of whole items, every chunk as long as fits."""
    chunks, it0 = [], 0
    while it0 < n_items:
        assert need(it0, it0 + 1) <= budget, "one item does not fit the budget"
        lo, hi = it0 + 1, n_items
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if need(it0, mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        chunks.append((it0, lo))
        it0 = lo
    return chunks


class ListPlan(object):
    """What ops.sgraf_candidate_scores / sgraf_pair_attention and itr_sgraf_pairs_plan make of a pair list (pairs in the caller's order)."""

    def __init__(self, kernel, sgr, Ni, D, S, lens, pairs, budget_items=None):
        self.klen = [w if w <= GP_MAXW else 0 for w in lens]                              # ops._caption_tables(plan, dev, SGRAF_MAX_WORDS)
        self.long_slots = [s for s, (i, c) in enumerate(pairs) if self.klen[c] == 0]      # ops._long_caption_pairs
        per_img = [[] for _ in range(Ni)]
        for s, (i, c) in enumerate(pairs):                                                # ops._group_pairs: stable by image
            if self.klen[c]:
                per_img[i].append((c, s))
        self.img_ptr = [0]
        for v in per_img:
            self.img_ptr.append(self.img_ptr[-1] + len(v))
        self.pair_img = [i for i, v in enumerate(per_img) for _ in v]
        self.pair_cap = [c for v in per_img for c, _ in v]
        self.pair_out = [s for v in per_img for _, s in v]
        self.P = len(self.pair_cap)
        off = _offsets(lens)
        self.pair_len, self.pair_col, self.pair_capok, self.item_begin, self.item_img, self.n_items = item_plan(
            self.img_ptr, self.pair_cap, off, self.klen, len(lens), sum(lens))
        assert self.pair_capok == self.pair_cap
        self.items = [list(range(self.item_begin[t], self.item_begin[t + 1])) for t in range(self.n_items)]
        self.item_of = [t for t, v in enumerate(self.items) for _ in v]
        self.rows = [sum(self.pair_len[p] + 1 for p in v) for v in self.items]
        self.na = [ceil_div(r, 16) for r in self.rows]                                    # sgraf_attn.hip:163
        self.rbase, self.T = [0] * self.P, [0] * self.P
        for v in self.items:
            r = 0
            for p in v:
                self.rbase[p], self.T[p] = r, ceil_div(self.pair_len[p] + 1, 16)          # sgraf_attn.hip:150, :284
                r += self.pair_len[p] + 1
        # an item as a group of the fused graph steps (sgr_fused.hip sgr_group_meta_kernel): class 0 = small, 1 = large
        self.cls = [E.group_meta(list(range(len(v))), [self.pair_len[p] for p in v])[3] for v in self.items]
        self.per = prefix_ranges(Ni)[0]
        # chunks: budget = what the first `budget_items` items need
        ib = self.item_begin
        self.need = lambda a, b: chunk_bytes(ib[b] - ib[a], b - a, D, S, sgr, with_steps=kernel == 'scores')
        self.budget = self.need(0, budget_items) if budget_items and self.n_items else None
        self.chunks = chunks_within(self.need, self.n_items, self.budget) if self.budget else ([(0, self.n_items)] if self.n_items else [])

    def chunk_of(self, t):
        return next(k for k, (a, b) in enumerate(self.chunks) if a <= t < b)

    def describe(self):
        rows = sorted(set(self.rows))
        return "pairs %d (long %d) items %d rows %s na %s classes %d+%d caps/item %s per %d chunks %d [pairs %s items %s]" % (
            self.P, len(self.long_slots), self.n_items, rows if len(rows) <= 8 else "%d..%d" % (rows[0], rows[-1]), sorted(set(self.na)),
            self.cls.count(0), self.cls.count(1), sorted(set(len(v) for v in self.items)), self.per, len(self.chunks),
            sorted(set(self.item_begin[b] - self.item_begin[a] for a, b in self.chunks)), sorted(set(b - a for a, b in self.chunks)))


# ---------------------------------------------------------------------------------------------------------------------
# the mirror of sgraf_reason_kernel (dtype-generic)
def reason(w, x, mod, steps, extra=None, denom=None):
    """sgraf_attn.hip:172-324 on node rows x [B, n, S] (node 0 = the global node) -> (score [B], node_w [B, n] | edge [B, steps, n, n]).
    SAF (:174-219): sigmoid of the BatchNorm'd logit as 1 / (1 + exp(-z)), l1norm, the aggregate of the NORMALISED weights, l2norm.
    SGR (:224-324): per step Q' = X Wfold^T + vfold for ALL rows, the maximum taken out of the softmax, Y = E X, X' = relu(Y Wg^T + b).
    extra: 'last' (defect 6: the last node a second time) or a [B, 1, S] row (defect 12) joins the weights / the keys; its column is
    cut from what is returned.  denom: [B, 1] replaces the l1 norm's sum (defect 13)."""
    one = torch.ones((), dtype=x.dtype)
    n = x.shape[1]
    if mod == 'SAF':
        pb = 'SAF_module.bn'
        bscale = w[pb + '.weight'][0] / torch.sqrt(w[pb + '.running_var'][0] + 1e-5)
        xs = x if extra is None else torch.cat([x, x[:, -1:] if isinstance(extra, str) else extra], 1)
        s = xs @ w['SAF_module.attn_sim_w.weight'][0] + w['SAF_module.attn_sim_w.bias'][0]
        a = one / (one + torch.exp(-((s - w[pb + '.running_mean'][0]) * bscale + w[pb + '.bias'][0])))
        an = a / ((a.abs().sum(1, keepdim=True) if denom is None else denom) + 1e-8)
        vec = (an[:, :, None] * xs).sum(1)
        sc = (vec * w['sim_eval_w.weight'][0]).sum(1) / ((vec * vec).sum(1).sqrt() + 1e-8) + w['sim_eval_w.bias'][0]
        return one / (one + torch.exp(-sc)), an[:, :n]
    edges = []
    for k in range(steps):
        pre = 'SGR_module.sgr%d.' % k
        Wq, bq, Wk = w[pre + 'graph_query_w.weight'], w[pre + 'graph_query_w.bias'], w[pre + 'graph_key_w.weight']
        keys = x if extra is None else torch.cat([x, x[:, -1:] if isinstance(extra, str) else extra], 1)
        e = (x @ (Wk.t() @ Wq).t() + bq @ Wk) @ keys.transpose(1, 2)                 # sgraf.hip sgraf_fold_weights
        e = torch.exp(e - e.max(2, keepdim=True)[0])
        edge = e * (one / e.sum(2, keepdim=True))
        edges.append(edge[:, :, :n])
        x = torch.relu(E._lin(edge @ keys, w, pre + 'sim_graph_w'))
    sc = (x[:, 0] * w['sim_eval_w.weight'][0]).sum(1) + w['sim_eval_w.bias'][0]
    return one / (one + torch.exp(-sc)), torch.stack(edges, 1)


def _padded(words, lens):
    L = max(lens)
    return torch.stack([torch.nn.functional.pad(words[o:o + n], (0, 0, 0, L - n)) for o, n in zip(_offsets(lens), lens)], 0)


# ---------------------------------------------------------------------------------------------------------------------
class PairCase(Case):
    """train_prim_cases.Case with two references (oracle and mirror), the plan and the defects."""

    def __init__(self, kernel, group, tag, mod, Ni, D, S, lens, cand, by, steps=3, budget_items=None, seed=0):
        self.kernel, self.group, self.tag, self.mod, self.Ni, self.D, self.S = kernel, group, tag, mod, Ni, D, S
        self.lens = tuple(int(n) for n in lens)
        self.Nc, self.n_tok, self.steps, self.zero = len(self.lens), sum(self.lens), steps, None
        self.cand, self.by, self.budget_items = [list(r) for r in cand], by, budget_items
        assert kernel in KERNELS and mod in ('SAF', 'SGR') and by in ('caption', 'image') and D % 32 == 0
        assert all(1 <= n <= MAX_COMPOSED for n in self.lens) and (kernel == 'scores' or (S <= GR_MAXS and S % 16 == 0))
        self.K = len(cand[0])
        assert len(cand) == (self.Nc if by == 'caption' else Ni) and all(len(r) == self.K for r in cand)
        self.pairs = [((e, q) if by == 'caption' else (q, e)) for q, row in enumerate(cand) for e in row]
        assert all(0 <= i < Ni and 0 <= c < self.Nc for i, c in self.pairs)
        self.P = len(self.pairs)
        self.LI, self.LC = sorted(set(i for i, _ in self.pairs)), sorted(set(c for _, c in self.pairs))
        self.li, self.lc = {i: k for k, i in enumerate(self.LI)}, {c: k for k, c in enumerate(self.LC)}
        self.sub_lens = tuple(self.lens[c] for c in self.LC)
        self.off = _offsets(self.lens)
        self.plan = ListPlan(kernel, mod == 'SGR', Ni, D, S, self.lens, self.pairs, budget_items)
        self.aux = 'node_w' if mod == 'SAF' else 'edge'
        self.tensors = ('score',) if kernel == 'scores' else ('attn', self.aux, 'score')
        Case.__init__(self, mod, {}, lambda g: E.SgrafCase._make(self, g), None)
        self.name = "%s-%s-%s-%s-Ni%d-D%d-S%d-Nc%d-by%s-K%d%s%s%s" % (
            kernel, mod, group, tag, Ni, D, S, self.Nc, by, self.K, "-steps%d" % steps if mod == 'SGR' else "",
            "-budget%d" % budget_items if budget_items else "", "-seed%d" % seed if seed else "")

    @property
    def weights(self):
        return E.weights(self.mod, self.D, self.S, self.steps if self.mod == 'SGR' else 3)

    @property
    def big(self):
        return self.P > 300 or self.Ni > 1000

    def short(self, s):
        return self.lens[self.pairs[s][1]] <= GP_MAXW

    # ---- what the case covers -------------------------------------------------------------------------------------
    def route_name(self):
        if self.kernel == 'attention':
            return 'reason_' + self.mod.lower()
        if self.mod == 'SAF':
            return 'saf256' if self.S == 256 else 'saf_generic'
        return 'sgr_fused' if self.S == 256 else 'sgr_chain'

    def seams(self):
        """{parameter: set of values} this case puts into the coverage of SEAMS[kernel]."""
        p = self.plan
        W = set(p.pair_len)
        s = {'route': {self.route_name()}, 'S_' + self.mod.lower(): {self.S}, 'D': {self.D}, 'Ni': {self.Ni}, 'W': W, 'by': {self.by}, 'K': {self.K},
             'ncb': set(ceil_div(w, 16) for w in W), 'long': set(self.lens[c] for c in self.LC if self.lens[c] > GP_MAXW),
             'long_at': set(('first' if c == 0 else ('last' if c == self.Nc - 1 else 'middle')) for c in self.LC if self.lens[c] > GP_MAXW),
             'rows': set(p.rows), 'na': set(p.na), 'class': set('sl'[k] for k in p.cls), 'caps_per_item': set(len(v) for v in p.items),
             'T': set(p.T), 'per': {p.per}, 'chunks': {'one' if len(p.chunks) == 1 else 'several'},
             'pairs_per_chunk': set(p.item_begin[b] - p.item_begin[a] for a, b in p.chunks)}
        if self.mod == 'SGR':
            s['sgr_step'] = {self.steps}
            if self.S == 256:
                s['items_per_chunk'] = set(b - a for a, b in p.chunks)
                if self.kernel == 'scores':          # sgr_fused.hip:1001-1008 with nb = 1: the fullest chunk's items of a class against the resident workgroups
                    for k, rows in ((0, E.SF_SMALL), (1, E.SF_ROWS)):
                        n = max(p.cls[a:b].count(k) for a, b in p.chunks)
                        res = E.WALK_CUS * E.WG_PER_CU[rows]
                        if n:
                            s['walk%d' % rows] = {'below' if n < res else ('equal' if n == res else ('above' if n <= 2 * res else 'twice'))}
        if self.kernel == 'attention':
            s['out_tiles'] = {self.S // 16}
            s['vec_trips'] = {ceil_div(self.S, 64)}
        shape = set()
        for t, v in enumerate(p.items):
            ws = [p.pair_len[q] for q in v]
            last_of_image = t + 1 == p.n_items or p.item_img[t + 1] != p.item_img[t]
            if len(v) == GP_MAXCAP and p.rows[t] < GP_ITEM and not last_of_image:
                shape.add('closed_by_16_captions')
            if ws == [1] * 16:
                shape.add('16x1word')
            if p.rows[t] == GP_ITEM:
                shape.add('exact_fill')
            if not last_of_image and p.rows[t] + p.pair_len[p.item_begin[t + 1]] + 1 == GP_ITEM + 1:
                shape.add('one_over')
            if ws == [GP_MAXW]:
                shape.add('63_alone' + ('_then_another' if not last_of_image else ''))
            if any(p.rbase[q] % 16 and p.rbase[q] // 16 != (p.rbase[q] + p.pair_len[q]) // 16 for q in v):
                shape.add('straddles_row_tile')
        if self.P == 1:
            shape.add('one_pair')
        if self.by == 'caption' and any(a < i < b for a, b in zip(self.LI[:-1], self.LI[1:]) for i in range(a + 1, b)):
            shape.add('unlisted_image_between')
        if any(len(set(r)) < len(r) for r in self.cand):
            shape.add('pair_twice_in_a_list')
        s['item_shape'] = shape
        s['image'] = set(i for i in self.LI if i in (0, 254, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, self.Ni - 1))
        cuts = set()
        for a, b in p.chunks[1:]:
            cuts.add('after_first_item' if a == 1 else 'later')
            if p.item_img[a - 1] == p.item_img[a]:
                cuts.add('inside_an_image')
        if len(p.chunks) > 1 and p.chunks[-1][1] - p.chunks[-1][0] == 1:
            cuts.add('last_chunk_one_item')
        s['cut'] = cuts
        return s

    def describe(self):
        return "%s by %s K %d %s" % (self.route_name(), self.by, self.K, self.plan.describe())

    @property
    def claims(self):
        """The defects this case claims to see (module docstring)."""
        p = self.plan
        out = []
        if p.P == 0:
            return [11]
        several = any(len(v) > 1 for v in p.items)
        if not self.big:
            out += [1] if any(p.pair_cap[q] != p.pair_cap[q + 1] for v in p.items for q in v[:-1]) else []
            if len(p.chunks) > 1:
                out += [3, 4]
                if any(p.item_img[t - a] != p.item_img[t] for a, b in p.chunks[1:] for t in range(a, b)):
                    out.append(2)
            if self.kernel == 'attention' or self.mod == 'SGR' or (self.S == 256 and any((n + 1) % 4 for n in p.pair_len)):
                out.append(6)
            out += ([7] if max(p.pair_len) > 1 else []) + [8, 9] + ([90] if self.D <= 96 else [])
            if self.kernel == 'scores' and p.long_slots:
                out.append(11)
            if self.kernel == 'attention':
                out += ([12] if several and self.mod == 'SGR' else []) + ([13] if several and self.mod == 'SAF' else [])
                out += [14] if self.mod == 'SGR' and self.steps > 1 else []
        if any(i >= PREFIX_THREADS for i in p.pair_img):
            out.append(5)
        if self.kernel == 'scores' and any(a != b for r in self.cand for a, b in zip(r, r[1:] + r[:1])):
            out.append(10)
        return out

    # ---- references ---------------------------------------------------------------------------------------------
    def _sub(self, dtype):
        """The listed images and captions alone, re-packed: (weights, images, words, lengths)."""
        x = self.inputs()
        words = torch.cat([x['words'][self.off[c]:self.off[c] + self.lens[c]] for c in self.LC], 0)
        return {k: v.to(dtype) for k, v in self.weights.items()}, x['images'][self.LI].to(dtype).clone(), words.to(dtype).clone(), self.sub_lens

    def _flat(self, score_of, blocks=None):
        """score_of(image k, caption k) and blocks {tensor: fn(image k, caption k) -> block} over the listed set -> the flat tensors."""
        ks = [(self.li[i], self.lc[c]) for i, c in self.pairs]
        out = {'score': torch.stack([score_of(a, b) for a, b in ks])}
        for t, fn in (blocks or {}).items():
            out[t] = torch.cat([fn(a, b).reshape(-1) for s, (a, b) in enumerate(ks) if self.short(s)])
        return out

    def oracle(self, dtype, change=None):
        w, img, words, lens = self._sub(dtype)
        if change is not None:
            img, words, lens = change(img, words, lens)
        if self.kernel == 'scores' or change is not None:
            S = E.oracle(w, img, words, lens, self.mod, self.steps)
            return self._flat(lambda a, b: S[a, b])
        S, parts = X.sgraf_similarity_explained(w, img, _padded(words, lens), list(lens), self.mod, self.steps)
        aux = (lambda a, b: parts[b]['node_w'][a]) if self.mod == 'SAF' else (lambda a, b: parts[b]['edge'][:, a])
        return self._flat(lambda a, b: S[a, b], {'attn': lambda a, b: parts[b]['attn'][a], self.aux: aux})

    def nodes(self, dtype, **kw):
        """sgraf_eval_cases.mirror up to the node rows: {listed caption k: (x [listed images, n + 1, S], attn [.., n, 36])}."""
        w, img, words, lens = self._sub(dtype)
        got = {}

        def collect(c, x, attn):
            got[c] = (x, attn)
            return torch.zeros(x.shape[0], dtype=x.dtype)
        E.mirror(w, img, words, lens, self.mod, self.steps, tail=collect, **kw)
        return w, got

    def mirror(self, dtype, dup_last=False, gram=None, stats=None):
        w, img, words, lens = self._sub(dtype)
        if self.kernel == 'scores':
            S = E.mirror(w, img, words, lens, self.mod, self.steps, dup_last=dup_last, gram=gram, stats=stats)
            return self._flat(lambda a, b: S[a, b])
        w, got = self.nodes(dtype, gram=gram)
        res = {b: reason(w, x, self.mod, self.steps, extra='last' if dup_last else None) for b, (x, _) in got.items()}
        return self._flat(lambda a, b: res[b][0][a], {'attn': lambda a, b: got[b][1][a], self.aux: lambda a, b: res[b][1][a]})

    def reference(self):
        """{tensor: (want float64, e32_oracle, e32_mirror, tol, max |mirror float64 - want|)} and 'sharp'; computed once and shared."""
        if 'ref' not in self._cache:
            stats = {}
            w64, w32 = self.oracle(torch.float64), self.oracle(torch.float32)
            m64, m32 = self.mirror(torch.float64, stats=stats if self.kernel == 'scores' else None), self.mirror(torch.float32)
            if self.kernel == 'attention':
                w, img, words, lens = self._sub(torch.float64)
                E.mirror(w, img, words, lens, self.mod, self.steps, stats=stats)
            out = {'sharp': stats['sharp']}
            for k in self.tensors:
                want = w64[k]
                eo, em = float((w32[k].double() - want).abs().max()), float((m32[k].double() - want).abs().max())
                tol = FALLBACK.get(self.name, {}).get(k, FACTOR * max(eo, em, U * float(want.abs().max())))
                out[k] = (want, eo, em, tol, float((m64[k] - want).abs().max()))
            self._cache['ref'] = out
        return self._cache['ref']

    def defects(self):
        """{number: {tensor: float64 value with the defect}} for every claimed defect (only tensors that keep their shape)."""
        p, claims = self.plan, self.claims
        want = {k: self.reference()[k][0] for k in self.tensors}
        out = {}

        def regroup(words, lens, rows):
            return words[[r for v in rows for r in v]].clone(), tuple(len(v) for v in rows)

        rows0 = [list(range(o, o + n)) for o, n in zip(_offsets(self.sub_lens), self.sub_lens)]

        def drop_last(img, words, lens):
            return (img,) + regroup(words, lens, [r[:-1] if len(r) > 1 else r for r in rows0])

        def truncate_long(img, words, lens):
            return (img,) + regroup(words, lens, [r[:GP_MAXW] for r in rows0])

        def zero_region(img, words, lens):
            img[:, SC_R - 1] = 0.0
            return img, words, lens

        def zero_feature(img, words, lens):
            img[..., -1] = 0.0
            words[..., -1] = 0.0
            return img, words, lens

        for n, change in ((7, drop_last), (11, truncate_long), (9, zero_region), (90, zero_feature)):
            if n in claims:
                out[n] = {'score': self.oracle(torch.float64, change)['score']}
        if 6 in claims:
            res = self.mirror(torch.float64, dup_last=True)
            out[6] = {k: v for k, v in res.items() if k != 'attn'}
        if 8 in claims:
            once = lambda G: torch.triu(G, 1) + torch.diag_embed(torch.diagonal(G, dim1=1, dim2=2))      # the kernel's form is diag + 2 x upper (scan_pairs_cases.py mirror_caption_t2i)
            out[8] = {'score': self.mirror(torch.float64, gram=once)['score']}
        if 10 in claims:
            out[10] = {'score': torch.roll(want['score'].view(-1, self.K), -1, 1).reshape(-1)}
        if 14 in claims:
            edge, o = want['edge'].clone(), 0
            for s, (i, c) in enumerate(self.pairs):
                if self.short(s):
                    nn = (self.lens[c] + 1) ** 2 * self.steps
                    edge[o:o + nn] = torch.roll(edge[o:o + nn].view(self.steps, -1), -1, 0).reshape(-1)
                    o += nn
            out[14] = {'edge': edge}
        node_level = [n for n in (1, 2, 3, 4, 5, 12, 13) if n in claims]
        if node_level:
            w, got = self.nodes(torch.float64)
            S_dim = self.S
            img_k = [self.li[i] for i in p.pair_img]
            cap_k = [self.lc[c] for c in p.pair_cap]
            rows_of = lambda q: got[cap_k[q]][0][img_k[q]]                                  # [n + 1, S] of image-major pair q
            stream = {}

            def item_stream(t):
                """the local node rows of item t as the chunk buffer holds them: [64, S], zeros where no caption owns the column"""
                if t not in stream:
                    buf = torch.zeros(GP_ITEM, S_dim, dtype=torch.float64)
                    for q in (p.items[t] if 0 <= t < p.n_items else []):
                        o = p.pair_col[q] - t * GP_ITEM
                        buf[o:o + p.pair_len[q]] = rows_of(q)[1:]
                    stream[t] = buf
                return stream[t]

            def rescore(n, changed):
                """changed: {image-major pair: node rows} -> the flat scores with these pairs' scores replaced"""
                score = want['score'].clone()
                for q, x in list(changed.items())[:64]:
                    score[p.pair_out[q]] = reason(w, x[None], self.mod, self.steps)[0][0]
                out[n] = {'score': score}

            first_chunk = {q: (a, b) for a, b in p.chunks for t in range(a, b) for q in p.items[t]}
            if 1 in claims:
                ch = {}
                for v in p.items:
                    for q, nxt in zip(v[:-1], v[1:]):
                        t, o = p.item_of[q], p.pair_col[nxt] % GP_ITEM
                        loc = torch.cat([item_stream(t), torch.zeros(GP_ITEM, S_dim, dtype=torch.float64)])[o:o + p.pair_len[q]]
                        ch[q] = torch.cat([rows_of(q)[:1], loc])
                rescore(1, ch)
            if 3 in claims:
                ch = {}
                for q in range(p.P):
                    a, b = first_chunk[q]
                    if a:
                        t, o = p.item_of[q], p.pair_col[q] % GP_ITEM
                        src = item_stream(t + a) if t + a < b else torch.zeros(GP_ITEM, S_dim, dtype=torch.float64)
                        ch[q] = torch.cat([rows_of(q)[:1], src[o:o + p.pair_len[q]]])
                rescore(3, ch)
            if 4 in claims:
                ch = {}
                for q in range(p.P):
                    p0 = p.item_begin[first_chunk[q][0]]
                    if p0 and (img_k[q - p0], cap_k[q - p0]) != (img_k[q], cap_k[q]):
                        ch[q] = torch.cat([rows_of(q - p0)[:1], rows_of(q)[1:]])
                rescore(4, ch)
            if 5 in claims:
                base = min(t for t in range(p.n_items) if p.item_img[t] >= PREFIX_THREADS)
                ch = {}
                for q in range(p.P):
                    if p.pair_img[q] >= PREFIX_THREADS and base:
                        o = p.pair_col[q] % GP_ITEM
                        ch[q] = torch.cat([rows_of(q)[:1], item_stream(p.item_of[q] - base)[o:o + p.pair_len[q]]])
                rescore(5, ch)
            if 2 in claims:
                score = want['score'].clone()
                S = E.oracle(*self._sub(torch.float64), self.mod, self.steps)
                for a, b in p.chunks[1:]:
                    for t in range(a, b):
                        for q in p.items[t]:
                            score[p.pair_out[q]] = S[self.li[p.item_img[t - a]], cap_k[q]]
                out[2] = {'score': score}
            if 12 in claims or 13 in claims:
                n = 12 if 12 in claims else 13
                score, aux, o = want['score'].clone(), want[self.aux].clone(), {}
                at = 0
                for s, (i, c) in enumerate(self.pairs):          # where pair s's block of `aux` starts
                    if self.short(s):
                        o[s] = at
                        at += (self.lens[c] + 1) if self.mod == 'SAF' else self.steps * (self.lens[c] + 1) ** 2
                for v in p.items:
                    if n == 13:
                        tot = sum(reason(w, rows_of(q)[None], 'SAF', 0, denom=torch.ones(1, 1, dtype=torch.float64) - 1e-8)[1].abs().sum() for q in v)
                    for k, q in enumerate(v):
                        if len(v) == 1 or (n == 12 and k + 1 == len(v)):
                            continue
                        if n == 12:
                            sc, ax = reason(w, rows_of(q)[None], self.mod, self.steps, extra=rows_of(v[k + 1])[None, :1])
                        else:
                            sc, ax = reason(w, rows_of(q)[None], self.mod, self.steps, denom=tot.reshape(1, 1))
                        s = p.pair_out[q]
                        score[s] = sc[0]
                        aux[o[s]:o[s] + ax.numel()] = ax.reshape(-1)
                out[n] = {'score': score, self.aux: aux}
        return out


# The inputs are seeded from the case's name.  A case whose seed fails a condition takes another seed here; the seam stays.  The float32
# references are matrix products, so their rounding error depends on the BLAS that runs them; the GPU sweep therefore applies
# min(tol, older bound), never the wider of the two.
RESEED = {
    'scores-SAF-route-allW-Ni5-D32-S16-Nc16-bycaption-K3': 1,                        # score tol 5.44e-06
    'scores-SGR-steps-allW-Ni5-D32-S64-Nc16-bycaption-K3-steps8': 1,                 # span 0.038
    'attention-SGR-route-allW-Ni5-D32-S64-Nc16-bycaption-K3-steps3': 1,              # attn tol 2.33e-05
    'attention-SGR-steps-allW-Ni5-D32-S256-Nc16-bycaption-K3-steps1': 1,             # score tol 5.14e-06
    'attention-SGR-steps-allW-Ni5-D32-S256-Nc16-bycaption-K3-steps2': 1,             # edge tol 2.37e-05
    'attention-SGR-items-cap16-Ni3-D32-S256-Nc19-byimage-K19-steps3': 3,             # edge tol 2.02e-05 (seed 1: 1.77e-05)
    'attention-SAF-items-fill64-Ni3-D32-S256-Nc5-byimage-K3': 1,                     # span 0.040
    'attention-SAF-items-percap-Ni3-D32-S256-Nc48-byimage-K16': 1,                   # sharpness 1.75
    'scores-SAF-perchunk-K1-Ni3-D32-S256-Nc1-byimage-K1-budget1': 1,                 # sharpness 1.48
    'attention-SAF-perchunk-K4-Ni3-D32-S256-Nc4-byimage-K4-budget1': 1,              # sharpness 1.84
    'attention-SGR-perchunk-P256-Ni21-D32-S256-Nc4-bycaption-K64-steps3': 2,         # edge tol 2.34e-05 (seed 1: 1.58e-05)
    'scores-SAF-cut-items9-Ni3-D32-S64-Nc5-byimage-K3-budget1': 1,                   # span 0.020
    'attention-SAF-cut-items9-Ni3-D32-S256-Nc5-byimage-K3-budget1': 2,               # span 0.041
    'scores-SAF-cut-items9-Ni3-D32-S256-Nc5-byimage-K3-budget2': 6,                  # span 0.040
    'scores-SAF-cut-items9-Ni3-D32-S64-Nc5-byimage-K3-budget2': 3,                   # span 0.041
    'scores-SAF-cut-items9-Ni3-D32-S256-Nc5-byimage-K3-budget4': 1,                  # span 0.037
    'scores-SAF-cut-items9-Ni3-D32-S64-Nc5-byimage-K3-budget4': 5,                   # span 0.041
    'attention-SAF-cut-items9-Ni3-D32-S256-Nc5-byimage-K3-budget4': 4,               # span 0.047
    'attention-SGR-cut-items9-Ni3-D32-S256-Nc5-byimage-K3-steps3-budget1': 1,        # edge tol 2.17e-05
    'attention-SGR-cut-mixed-Ni5-D32-S256-Nc16-byimage-K8-steps3-budget2': 1,        # attn tol 2.10e-05
    'scores-SAF-Ni-edges-Ni1-D32-S256-Nc4-bycaption-K6': 6,                          # sharpness 1.52, span 0.039 (four scores)
    'scores-SAF-Ni-edges-Ni255-D32-S256-Nc4-bycaption-K6': 1,                        # sharpness 1.29
    'scores-SAF-Ni-edges-Ni256-D32-S256-Nc4-bycaption-K6': 1,                        # sharpness 1.83
    'scores-SGR-D-short-Ni5-D1024-S256-Nc9-bycaption-K3-steps3': 1,                  # span 0.040
    'attention-SAF-D-short-Ni5-D1024-S256-Nc9-bycaption-K3': 1,                      # attn tol 2.03e-05
    'scores-SGR-D-short-Ni5-D1024-S64-Nc9-bycaption-K3-steps3': 3,                   # span 0.034
    # inside the older cap, but by less than a quarter of it
    'attention-SGR-route-allW-Ni5-D32-S128-Nc16-bycaption-K3-steps3': 1,             # edge tol 1.85e-05
    'attention-SGR-route-allW-Ni5-D32-S192-Nc16-bycaption-K3-steps3': 1,             # edge tol 1.62e-05
    'attention-SAF-lists-short-Ni13-D32-S256-Nc9-byimage-K10': 1,                    # attn tol 1.76e-05
    'attention-SGR-lists-short-Ni13-D32-S256-Nc9-byimage-K10-steps3': 11,            # edge tol 1.67e-05
    'attention-SGR-items-percap-Ni3-D32-S256-Nc48-byimage-K16-steps3': 1,            # edge tol 1.99e-05
    'attention-SGR-perchunk-K5-Ni3-D32-S256-Nc5-byimage-K5-steps3-budget1': 1,       # attn tol 1.85e-05
    'attention-SGR-Ni-edges-Ni257-D32-S256-Nc4-bycaption-K6-steps3': 1,              # edge tol 1.54e-05
    'attention-SGR-D-short-Ni5-D288-S256-Nc9-bycaption-K3-steps3': 9,                # attn tol 1.73e-05
    'attention-SGR-D-short-Ni5-D64-S256-Nc9-bycaption-K3-steps3': 3,                 # edge tol 1.64e-05
    'attention-SGR-D-short-Ni5-D96-S256-Nc9-bycaption-K3-steps3': 9,                 # attn tol 1.54e-05
    'attention-SGR-D-short-Ni5-D256-S256-Nc9-bycaption-K3-steps3': 9,                # attn tol 1.76e-05, edge tol 2.06e-05
}


def _add(kernel, group, tag, mod, Ni, D, S, lens, cand, by, **kw):
    c = PairCase(kernel, group, tag, mod, Ni, D, S, lens, cand, by, **kw)
    if c.name in RESEED:
        c = PairCase(kernel, group, tag, mod, Ni, D, S, lens, cand, by, seed=RESEED[c.name], **kw)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(kernel=None, group=None, mod=None):
    return [c for c in CASES if (kernel is None or c.kernel == kernel) and (group is None or c.group == group) and (mod is None or c.mod == mod)]


def _seam(kernels, **params):
    for k in kernels:
        for name, v in params.items():
            SEAMS.setdefault(k, {})[name] = sorted(set(SEAMS.get(k, {}).get(name, [])) | set(v), key=str)


def image_lists(Ni, Nc, K):
    """cand [Ni, K] of caption indices for by='image': list i walks the captions from i in steps of 2."""
    return [[(i + 2 * k) % Nc for k in range(K)] for i in range(Ni)]


BOTH = KERNELS
MODS = ('SAF', 'SGR')
ALL_W = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)        # every seam of the words per caption; 16 captions
NI = 5
SHORT = (5, 9, 3, 14, 2, 7, 11, 20, 1)

# every route on every word count: three images per caption (Ni = 5: every image, the last one too)
_W3 = lists_by_caption(len(ALL_W), NI, 3)
for _S in (256, 16, 64, 512, 1024):
    _add('scores', 'route', 'allW', 'SAF', NI, 32, _S, ALL_W, _W3, 'caption')
    _add('scores', 'route', 'allW', 'SGR', NI, 32, _S, ALL_W, _W3, 'caption')
for _k in (1, 2, 8):
    _add('scores', 'steps', 'allW', 'SGR', NI, 32, 256, ALL_W, _W3, 'caption', steps=_k)
    _add('scores', 'steps', 'allW', 'SGR', NI, 32, 64, ALL_W, _W3, 'caption', steps=_k)
_seam(('scores',), route=('saf256', 'saf_generic', 'sgr_fused', 'sgr_chain'), S_saf=(16, 64, 256, 512, 1024), S_sgr=(16, 64, 256, 512, 1024))
# the attention entry: sim_dim / 16 = 1 / 3 / 4 / 5 / 8 / 12 / 16 output tiles on four waves, SAF vec[u] trips 1 .. 4 (192: the third)
for _S in (16, 48, 64, 80, 128, 192, 256):
    _add('attention', 'route', 'allW', 'SAF', NI, 32, _S, ALL_W, _W3, 'caption')
    _add('attention', 'route', 'allW', 'SGR', NI, 32, _S, ALL_W, _W3, 'caption')
for _k in (1, 2, 8):
    _add('attention', 'steps', 'allW', 'SGR', NI, 32, 256, ALL_W, _W3, 'caption', steps=_k)
_seam(('attention',), route=('reason_saf', 'reason_sgr'), S_saf=(16, 48, 64, 80, 128, 192, 256), S_sgr=(16, 48, 64, 80, 128, 192, 256),
      out_tiles=(1, 3, 4, 5, 8, 12, 16), vec_trips=(1, 2, 3, 4))
_seam(BOTH, W=ALL_W, ncb=(1, 2, 3, 4), sgr_step=(1, 2, 3, 8), T=(1, 2, 3, 4))

# both list directions, K = 1 | 10 | 37 (K above the targets: the same pair several times in one list; list q holds the pairs of query
# q alone, so no pair stands in two lists of one direction -- the attention entry's [P, 2] form is these lists flattened)
for _mod in MODS:
    for _K in (1, 10, 37):
        for _kernel in BOTH:
            if _kernel == 'scores' or _K == 10:
                _add(_kernel, 'lists', 'short', _mod, 13, 32, 256, SHORT, lists_by_caption(len(SHORT), 13, _K), 'caption')
                _add(_kernel, 'lists', 'short', _mod, 13, 32, 256, SHORT, image_lists(13, len(SHORT), _K), 'image')
_seam(('scores',), K=(1, 10, 37))
_seam(BOTH, by=('caption', 'image'))

# items.  by='image': an image's list is its row of cand, in order
ITEM_SETS = {
    # 17 one-word captions: an item closed by the 16-caption limit at 32 rows, and a 17th caption; two companions for the sharpness
    'cap16': ((1,) * 17 + (40, 22), [list(range(17)) + [17, 18]] * 3),
    # 31 + 31 words = 64 rows exactly | 31 + 32: one over
    'fill64': ((31, 31, 32, 20, 9), [[0, 1, 3], [0, 2, 4], [1, 0, 2]]),
    # a 63-word caption alone in its item, followed by another
    'w63': ((63, 5, 63, 9), [[0, 1, 2], [2, 0, 3], [1, 3, 0]]),
    # node rows 16 | 17 | 32 | 33 | 48 | 49 | 64 of an item: na = 1 .. 4, the small / large class; (7, 8) and the like straddle a row tile
    'rows': ((7, 7, 7, 8, 15, 15, 15, 16, 23, 23, 23, 24, 31, 31), [[2 * i, 2 * i + 1] for i in range(7)]),
    # 16 | 4 | 5 (and 1) captions per item: the wave-per-caption loops
    'percap': ((1,) * 16 + (12,) * 16 + (11,) * 16, [list(range(16)), list(range(16, 32)), list(range(32, 48))]),
}
for _tag, (_lens, _cand) in ITEM_SETS.items():
    for _mod in MODS:
        for _kernel in BOTH:
            _add(_kernel, 'items', _tag, _mod, len(_cand), 32, 256, _lens, _cand, 'image')
    _add('scores', 'items', _tag, 'SGR', len(_cand), 32, 64, _lens, _cand, 'image')
# one pair; an image listed by nobody between listed ones
for _mod in MODS:
    for _kernel in BOTH:
        _add(_kernel, 'items', 'one', _mod, 3, 32, 256, (9,), [[1]], 'caption')
        _add(_kernel, 'items', 'unlisted', _mod, 7, 32, 256, SHORT[:4], [[0, 3, 6], [3, 0, 5], [6, 6, 0], [5, 3, 0]], 'caption')
_seam(BOTH, item_shape=('closed_by_16_captions', '16x1word', 'exact_fill', 'one_over', '63_alone_then_another', 'straddles_row_tile', 'one_pair',
                        'unlisted_image_between', 'pair_twice_in_a_list'),
      rows=(16, 17, 32, 33, 48, 49, 64), na=(1, 2, 3, 4), caps_per_item=(1, 4, 5, 16), **{'class': ('s', 'l')})

# pairs per chunk: three images x K short captions, one item per image and the budget of the first item (K = 17: items of 16 and 1
# captions and the budget of the first two)
PER_CHUNK = (1, 3, 4, 5, 7, 8, 9, 16, 17)
for _j, _K in enumerate(PER_CHUNK):
    _lens = tuple((k * 5) % 3 + (5 if _K <= 9 else 1) for k in range(_K))          # K <= 9: 5 .. 7 words, at most 63 rows; else 1 .. 3
    for _kernel in BOTH:
        _add(_kernel, 'perchunk', 'K%d' % _K, MODS[_j % 2], 3, 32, 256, _lens, [list(range(_K))] * 3, 'image', budget_items=1 + _K // 17)
    _add('scores', 'perchunk', 'K%d' % _K, MODS[(_j + 1) % 2], 3, 32, 64, _lens, [list(range(_K))] * 3, 'image', budget_items=1 + _K // 17)
# ... and 255 | 256 | 257 pairs in one chunk (the 256-thread index and scatter kernels): 21 images, lists with repeats
for _j, (_Nc, _K) in enumerate(((5, 51), (4, 64), (1, 257))):
    for _kernel in BOTH:
        _add(_kernel, 'perchunk', 'P%d' % (_Nc * _K), MODS[_j % 2], 21, 32, 256, SHORT[:_Nc], lists_by_caption(_Nc, 21, _K), 'caption')
_seam(BOTH, pairs_per_chunk=PER_CHUNK + (255, 256, 257))

# chunk cuts: every caption of more than 31 words is an item of its own; 9 items; budgets of the first 1 | 2 | 4 items: a cut after the
# first item, cuts inside an image's items, a last chunk of one item; and items of several pairs (p0 != it0)
CUT_LENS = (40, 35, 50, 33, 45)
for _mod in MODS:
    for _b in (1, 2, 4):
        _add('scores', 'cut', 'items9', _mod, 3, 32, 256, CUT_LENS, image_lists(3, 5, 3), 'image', budget_items=_b)
        _add('scores', 'cut', 'items9', _mod, 3, 32, 64, CUT_LENS, image_lists(3, 5, 3), 'image', budget_items=_b)
        _add('attention', 'cut', 'items9', _mod, 3, 32, 256, CUT_LENS, image_lists(3, 5, 3), 'image', budget_items=_b)
    for _kernel in BOTH:
        _add(_kernel, 'cut', 'mixed', _mod, 5, 32, 256, ALL_W, image_lists(5, len(ALL_W), 8), 'image', budget_items=2)
_seam(BOTH, cut=('after_first_item', 'inside_an_image', 'last_chunk_one_item', 'later'), chunks=('one', 'several'))

# images: the planner's 256-thread block, the prefix kernel's 1 024-thread stride (per = 1 | 2 | 3).  Four captions list images on both
# sides of each edge, image 0 and the last one
BIG_NI = (1, 255, 256, 257, 1024, 1025, 2049)
for _Ni in BIG_NI:
    _edge = sorted(set(i for i in (0, 254, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, _Ni - 1) if i < _Ni))
    _cand = [[_edge[(3 * c + k) % len(_edge)] for k in range(6)] for c in range(4)]
    for _mod in MODS:
        _add('scores', 'Ni', 'edges', _mod, _Ni, 32, 256, SHORT[:4], _cand, 'caption')
    _add('attention', 'Ni', 'edges', MODS[_Ni % 2], _Ni, 32, 256, SHORT[:4], _cand, 'caption')
_seam(BOTH, Ni=BIG_NI, per=(1, 2, 3), image=(0, 255, 256, 1023, 1024, 2048))

# items per chunk through sgr_fused_plan_groups: one pair per image, every item in the 32-row class (two workgroups per CU: 512 resident
# on 256 CUs, so 1 025 items are three for some workgroup of the persistent walk)
for _n in (256, 257, 1024, 1025):
    _lens = (1, 1, 30, 22, 1)
    _add('scores', 'nitems', 'n%d' % _n, 'SGR', _n, 32, 256, _lens, [[i % 5] for i in range(_n)], 'image')
_seam(('scores',), items_per_chunk=(1, 2, 256, 257, 1024, 1025), walk32=('below', 'above', 'twice'), walk64=('below',))

# D: the gather's 64 lanes x float4 (D = 256: one trip exactly, 288: a second), the 256-thread loops of the ctx and glo kernels
for _D in (64, 96, 256, 288, 1024):
    for _mod in MODS:
        _add('scores', 'D', 'short', _mod, NI, _D, 256, SHORT, lists_by_caption(len(SHORT), NI, 3), 'caption')
        if _D <= 256:
            _add('attention', 'D', 'short', _mod, NI, _D, 256, SHORT, lists_by_caption(len(SHORT), NI, 3), 'caption')
# The attention entry sees D only through the stages it shares with the scores entry (sgraf_pairs_nodes).  SGR at D = 1024 is left to
# the scores entry: there the float32 oracle's own attn / edge error (1.6e-6 / 2.0e-6 at every seed tried) x 16 is above the older 2e-5.
for _D in (288, 1024):
    for _mod in MODS:
        _add('scores', 'D', 'short', _mod, NI, _D, 64, SHORT, lists_by_caption(len(SHORT), NI, 3), 'caption')
        if (_D, _mod) != (1024, 'SGR'):
            _add('attention', 'D', 'short', _mod, NI, _D, 256, SHORT, lists_by_caption(len(SHORT), NI, 3), 'caption')
_seam(('scores',), D=(32, 64, 96, 256, 288, 1024))
_seam(('attention',), D=(32, 64, 96, 256, 288, 1024))

# captions of 64 | 82 | 191 words, first / middle / last: the composed path (scores), explained == False with empty blocks (attention)
LONG = (64, 5, 9, 82, 12, 3, 191)
for _mod in MODS:
    for _kernel in BOTH:
        _add(_kernel, 'long', 'first.middle.last', _mod, NI, 32, 256, LONG, lists_by_caption(len(LONG), NI, 3), 'caption')
    _add('scores', 'long', 'first.middle.last', _mod, NI, 32, 64, LONG, image_lists(NI, len(LONG), 4), 'image')
_seam(BOTH, long=(64, 82, 191), long_at=('first', 'middle', 'last'))

assert all(k + '-seed%d' % v in _BY_NAME for k, v in RESEED.items())
