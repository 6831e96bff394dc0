"""Case table of the fused SCAN evaluation scorer (csrc/scan_xattn.hip with scan_mainloop.inc / scan_mainloop_asm.inc, reached through
ops.scan_xattn_scores with 36 regions per image) and its float64 references.

One entry per (direction, images, D, caption lengths, first norm, aggregation, lambda_softmax): seeded CPU inputs by the recipe of
tests/helpers/scan_train_cases.py (l2-normalised regions, words = 0.6 * randn, packed, seeded from the case's name, the same tie under
Max; lambda_lse = 6), the REFERENCE -- itr_oracle.xattn_score in float64 and again in float32 for its own rounding error e32_oracle --
and the MIRROR, a plain-torch function per direction that follows this kernel's algebra where it differs from the literal evaluation
order (A = V E^T from one matrix product, the statistics of the l2 / l1 first norms stored as reciprocals multiplied by
lambda_softmax * log2 e, the attention weights as exp2 without a maximum shift where the first norm bounds the logit, q = e^T G e / den^2
through the Gram matrix and clamped at 0, the cosine clamp at 1e-8), run in float32 for e32_mirror and in float64 to prove that it is
the oracle's function.  The oracle call and the aggregation are scan_train_cases.oracle and _aggregate; the training table's mirrors
(softmax of lambda * _first_norm) are a third writing of each pair that the CPU test holds this one against; nothing here reads the code
under test.

Tolerance on the whole of S (tests/test_scan_eval_seams_gpu.py applies it, tests/test_scan_eval_case_table.py proves it):
    tol = 16 * max(e32_oracle, e32_mirror, u * max|want|),  u = 2^-24              (FACTOR, U: tests/helpers/train_prim_cases.py)
with tol <= 2^-10 max|want| (CAP) and tol <= 2e-5 (x the longest caption's words under t2i Sum, x 36 under i2t Sum), the flat bound
the older tests hold the kernel to (OLD_BOUND).

The host-side planning is mirrored below in plain Python, each function marked with the source lines it copies: the bin planner of
pack_plan.h, the column layout of scan_pack_kernel, the patch walk of the kernel, the epilogue route of the i2t kernel.  Every case
derives its plan from them (Plan) and SEAMS[direction] lists the values that must appear in the table.

Defects, all float64 (Case.claims says which a case claims and why not the others):
    a  the last feature of images and words zeroed                                     oracle on changed inputs
    b  the last region dropped                                                         oracle on changed inputs
    c  the last word of every caption of more than one word dropped                    oracle on changed inputs
    p  a zero word appended to the shortest caption: a padding column counted          oracle on changed inputs
    s  the last word of caption k of a tile given to caption k + 1 of that tile: a segment boundary off by one
                                                                                       oracle on changed inputs
    m  Mean (t2i) divided by the tile's used columns instead of the caption's words    oracle, columns rescaled
    f  i2t, matrix-core route, tiles with `far`: the caption Gram zeroed where the two words' 16-column blocks of the tile differ by
       two or more                                                                     mirror
    t  Ni % 4 != 0: the last image scored with image 0's Gram matrix (t2i) or region norms (i2t)     mirror
    o  i2t, more than 1024 captions: caption c >= 1024 read with the Gram offset of caption c - 1024  mirror
Under Max, b (i2t) and c (t2i) are decisive only where the dropped element carries the maximum: the tie of scan_train_cases.py.
p under t2i Sum and Max adds a term 0 (the cosine of a zero word is 0), which neither moves: claimed for LogSumExp and Mean only.
p under i2t moves nothing at all: a zero word adds nothing to a region's context vector and only scales the other words' weights, and
the cosine does not see a scale -- a counted padding column is harmless there, and no i2t case claims it.
t for i2t needs region norms that differ between images; the recipe's regions have norm 1, so only the cases with an all-zero region
in image 0 can claim it.
Nothing here imports the library: the table is checked on a machine without a GPU."""
import torch

import itr_oracle as O
import scan_train_cases as T
from scan_train_cases import NORMS, AGGS, LAMBDA_LSE, CAP, MIRROR_AGREES, FALLBACK_SHARE, ceil_div, _aggregate, _offsets      # noqa: F401
from train_prim_cases import Case, U, FACTOR, SENSITIVITY        # noqa: F401  (re-exported)

LAMBDA_SOFTMAX = 9.0
OLD_BOUND = 2e-5
LOG2E = 1.44269504088896341

# geometry of the kernel (pinned to csrc/ by tests/test_scan_eval_case_table.py)
SC_R, SC_IMGS, SC_NT, SC_MAXCAP, SC_BK = 36, 4, 64, 16, 32          # scan_common.h:7-15
PACK_MAXN = 16                                                      # pack_plan.h:21
TPW = 2                                                             # scan_xattn.hip:1088
PATCH = 8                                                           # scan_xattn.hip:165-174: 8 x 8 patches, one per XCD
PIPELINE_NK = 3                                                     # scan_mainloop.inc:63
I2T_MFMA_LS = 30.0                                                  # scan_xattn.hip:434-438
PREFIX_THREADS = 1024                                               # scan_xattn.hip:780-784
GRAM_ACC = 16                                                       # scan_xattn.hip:663: pairs per thread of gram_kernel
MFMA_NORMS = ('clipped_l2norm', 'l2norm', 'softmax', 'l1norm', 'clipped_l1norm')      # scan_xattn.hip:438: norms 0, 1, 2, 5, 6

SEAMS = {}          # direction -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule and that are judged by a derived a-priori bound instead: name -> bound, the
# derivation in a comment next to the entry.  No case needs it (profiles/scan_eval_seams/measured.txt).
FALLBACK = {}


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the host-side planning
def pack_exact_fill(by_size, cap, maxn):
    """pack_plan.h:28-90 (pack_exact_fill): the largest remaining item opens a bin, a bounded subset sum over the remaining size
    histogram finds the fewest items that fill the rest exactly (or the fullest reachable sum), the pattern repeats while the
    histogram holds it.  by_size[w] = ids of the items of size w -> list of bins (lists of ids, largest first)."""
    maxn = min(maxn, PACK_MAXN)
    INF = 255
    avail = [0] + [len(by_size[w]) for w in range(1, cap + 1)]
    head = [0] * (cap + 1)
    remaining = sum(avail)
    bins, hi = [], cap
    while remaining > 0:
        while avail[hi] == 0:
            hi -= 1
        L, rem = hi, cap - hi
        avail[L] -= 1
        best = [INF] * (cap + 1)
        best[0] = 0
        stages = []
        for w in range(min(L, rem), 0, -1):
            if avail[w] == 0:
                continue
            ch, nb = [0] * (cap + 1), list(best)
            for s in range(0, rem - w + 1):
                if best[s] == INF:
                    continue
                k = 1
                while k <= avail[w] and s + k * w <= rem and best[s] + k <= maxn - 1:
                    if best[s] + k < nb[s + k * w]:
                        nb[s + k * w] = best[s] + k
                        ch[s + k * w] = k
                    k += 1
            best = nb
            stages.append((w, ch))
        s = rem
        while best[s] == INF:
            s -= 1
        cnt = [0] * (cap + 1)
        for w, ch in reversed(stages):
            k = ch[s]
            cnt[w] += k
            s -= k * w
        avail[L] += 1
        cnt[L] += 1
        reps = remaining
        for w in range(1, L + 1):
            if cnt[w] and avail[w] // cnt[w] < reps:
                reps = avail[w] // cnt[w]
        reps = max(reps, 1)
        for _ in range(reps):
            b = []
            for w in range(L, 0, -1):
                for _k in range(cnt[w]):
                    b.append(by_size[w][head[w]])
                    head[w] += 1
            bins.append(b)
        for w in range(1, L + 1):
            avail[w] -= reps * cnt[w]
            remaining -= reps * cnt[w]
    return bins


def pack_best_fit_decreasing(by_size, cap, maxn):
    """pack_plan.h:93-116 (pack_best_fit_decreasing): items by decreasing size into the open bin with the least room that still
    takes them (the last one opened among equals), a new bin otherwise."""
    maxn = min(maxn, PACK_MAXN)
    bins, open_ = [], [[] for _ in range(cap + 1)]
    for w in range(cap, 0, -1):
        for c in by_size[w]:
            r = w
            while r <= cap and not open_[r]:
                r += 1
            if r <= cap:
                t = open_[r].pop()
            else:
                t = len(bins)
                bins.append([])
                r = cap
            bins[t].append(c)
            if len(bins[t]) < maxn and r - w > 0:
                open_[r - w].append(t)
    return bins


def pack_bins(lens, cap=SC_NT, maxn=SC_MAXCAP):
    """pack_plan.h:120-126 (pack_bins) behind scan_xattn.hip:933-950 (itr_scan_plan_tiles): exact fill unless best fit decreasing
    needs fewer bins.  lens[c] = words of caption c -> tiles as lists of caption ids."""
    by_size = [[] for _ in range(cap + 1)]
    for c, w in enumerate(lens):
        assert 1 <= w <= cap
        by_size[w].append(c)
    a, b = pack_exact_fill(by_size, cap, maxn), pack_best_fit_decreasing(by_size, cap, maxn)
    return b if len(b) < len(a) else a


def tile_layout(tile, lens):
    """scan_xattn.hip:825-846 (scan_pack_kernel): (cap_start[ncap + 1], col_cap[64], far) of one tile, captions in the planner's
    order (largest first)."""
    pos, far, cap_start, col_cap = 0, 0, [], [-1] * SC_NT
    for k, c in enumerate(tile):
        w = lens[c]
        cap_start.append(pos)
        assert pos + w <= SC_NT
        if ((pos + w - 1) >> 4) - (pos >> 4) >= 2:
            far = 1
        for j in range(w):
            col_cap[pos + j] = k
        pos += w
    return cap_start + [pos], col_cap, far


def patch_walk(Ni, n_tiles):
    """scan_xattn.hip:164-175 (the kernel) and :1075-1089 (the launch): (img_tiles, PI, PJ, grid, the `rep` values and the `pgroup`
    values that own a patch, (image tile, column tile) pairs visited -- each exactly once, asserted)."""
    img_tiles = ceil_div(Ni, SC_IMGS)
    PI, PJ = ceil_div(img_tiles, PATCH), ceil_div(n_tiles, PATCH)
    grid = ceil_div(ceil_div(PI * PJ, 8), TPW) * 64 * 8
    reps, pgroups, seen = set(), set(), set()
    for b in range(grid):
        xcd, slot = b & 7, b >> 3
        pgroup, within = slot >> 6, slot & 63
        for rep in range(TPW):
            patch = (pgroup * TPW + rep) * 8 + xcd
            if patch >= PI * PJ:
                break
            it, ct = (patch // PJ) * 8 + (within & 7), (patch % PJ) * 8 + (within >> 3)
            if it >= img_tiles or ct >= n_tiles:
                continue
            assert (it, ct) not in seen
            seen.add((it, ct))
            reps.add(rep)
            pgroups.add(pgroup)
    assert len(seen) == img_tiles * n_tiles
    return img_tiles, PI, PJ, grid, reps, pgroups


def i2t_route(norm, ls):
    """scan_xattn.hip:434-438: the i2t epilogue on the matrix cores, or one lane per region row."""
    return 'mfma' if norm in MFMA_NORMS and abs(ls) <= I2T_MFMA_LS else 'scalar'


class Plan(object):
    """What ops.ScanPlan and the launch make of a caption set: captions of more than 64 words leave for the pair kernels
    (ops.py: ScanPlan.__init__), the others are planned into tiles."""

    def __init__(self, Ni, D, lens, xa, norm, ls):
        self.short_idx = [c for c, w in enumerate(lens) if w <= SC_NT]
        self.long_idx = [c for c, w in enumerate(lens) if w > SC_NT]
        self.k_len = [lens[c] for c in self.short_idx]
        self.Nc_kernel = len(self.k_len)
        self.tiles = pack_bins(self.k_len) if self.k_len else []
        self.n_tiles = len(self.tiles)
        self.tile_begin, self.cap_order = [0], []
        for t in self.tiles:
            self.cap_order += t
            self.tile_begin.append(len(self.cap_order))
        self.layout = [tile_layout(t, self.k_len) for t in self.tiles]
        self.summary = [(len(t), lay[0][-1], lay[2]) for t, lay in zip(self.tiles, self.layout)]        # (ncap, used columns, far)
        self.cap_col = {}           # caption (index into lens) -> (tile, first column)
        for ti, (t, lay) in enumerate(zip(self.tiles, self.layout)):
            for k, c in enumerate(t):
                self.cap_col[self.short_idx[c]] = (ti, lay[0][k])
        self.nk = D // SC_BK
        self.mainloop = 'pipelined' if self.nk >= PIPELINE_NK else 'simple'
        self.route = i2t_route(norm, ls) if xa == 'i2t' else 't2i'
        self.per = ceil_div(self.Nc_kernel, PREFIX_THREADS)
        if self.n_tiles:
            self.img_tiles, self.PI, self.PJ, self.grid, self.reps, self.pgroups = patch_walk(Ni, self.n_tiles)
        else:
            self.img_tiles, self.PI, self.PJ, self.grid, self.reps, self.pgroups = ceil_div(Ni, SC_IMGS), 0, 0, 0, set(), set()

    def far_from(self):
        """{'first', 'later'}: the position inside its tile of the captions that set `far`."""
        out = set()
        for t, (cs, _, _) in zip(self.tiles, self.layout):
            for k in range(len(t)):
                if ((cs[k + 1] - 1) >> 4) - (cs[k] >> 4) >= 2:
                    out.add('first' if k == 0 else 'later')
        return out

    def describe(self):
        tiles = ",".join("%dx%d%s" % (n, used, "far" if far else "") for n, used, far in self.summary[:6]) + ("..." if self.n_tiles > 6 else "")
        return "tiles %d [%s] long %d img_tiles %d PIxPJ %dx%d reps %s pgroups %s nk %d %s route %s per %d" % (
            self.n_tiles, tiles, len(self.long_idx), self.img_tiles, self.PI, self.PJ, sorted(self.reps), sorted(self.pgroups), self.nk,
            self.mainloop, self.route, self.per)


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors, dtype-generic
def _leaky(a, norm):
    return torch.where(a > 0, a, 0.1 * a) if norm in ('clipped_l2norm', 'clipped', 'clipped_l1norm') else a


def _weights(a, norm, ls, stat_dim, ctx_dim, shifted):
    """Un-normalised attention weights e of the raw products a: the first norm along stat_dim, the softmax that follows along ctx_dim.
    scan_xattn.hip:239-266, :300-329 (t2i), :441-468, :515-516 (i2t, matrix cores): the l2 / l1 statistics are stored as
    1 / (norm + eps) * (lambda_softmax * log2 e) and the weight is exp2(f(a) * stat); softmax: b = exp(a - max) * (1 / sum) and
    e = exp(b * lambda_softmax); neither takes a maximum out.  no_norm and clipped (:318-322), and every norm on the scalar i2t route
    (:583-593), shift by the maximum: `shifted`."""
    b = _leaky(a, norm)
    if norm in ('clipped', 'no_norm'):
        x = b * ls
        return torch.exp2((x - x.max(ctx_dim, keepdim=True)[0]) * LOG2E)
    if norm == 'softmax':
        ex = torch.exp(a - a.max(stat_dim, keepdim=True)[0])
        u = ex * (1.0 / ex.sum(stat_dim, keepdim=True))
    else:
        nrm = (b * b).sum(stat_dim, keepdim=True).sqrt() if norm in ('clipped_l2norm', 'l2norm') else b.abs().sum(stat_dim, keepdim=True)
        rcp = 1.0 / (nrm + 1e-8)
        if not shifted:
            return torch.exp2(b * (rcp * (ls * LOG2E)))
        u = b * rcp
    x = u * ls
    if shifted:
        return torch.exp(x - x.max(ctx_dim, keepdim=True)[0])
    return torch.exp2(x * LOG2E)


def mirror_t2i(x, lens, norm, agg, ls=LAMBDA_SOFTMAX, gram=None):
    """scan_xattn.hip:17-26 (header) and :204-425: A = V E^T for all pairs, G_i = V_i V_i^T, ||e_w||; per pair the weights e over the
    regions (first norm along the caption's words per region), num_w = sum_r e a / den, q_w = e^T G e / den^2 clamped at 0 (:388-400),
    s_w = num_w / max(||e_w|| sqrt(q_w), 1e-8) (:401).  gram: a change to G (defect t)."""
    V, E = x['images'], x['words']
    Ni, R, D = V.shape
    A = (V.reshape(Ni * R, D) @ E.t()).view(Ni, R, -1)
    G = V @ V.transpose(1, 2)                                          # scan_xattn.hip:704-746 (gram_mfma_kernel)
    if gram is not None:
        G = gram(G)
    enorm = (E * E).sum(1).sqrt()                                      # scan_xattn.hip:864-867 (scan_pack_kernel)
    cols = []
    for o, W in zip(_offsets(lens), lens):
        a = A[:, :, o:o + W]
        e = _weights(a, norm, ls, 2, 1, False)
        rden = 1.0 / e.sum(1)
        num = (e * a).sum(1) * rden
        q = ((e * (G @ e)).sum(1) * rden * rden).clamp_min(0.0)
        s = num / (enorm[o:o + W] * q.sqrt()).clamp_min(1e-8)
        cols.append(_aggregate(s, agg))
    return {'S': torch.stack(cols, 1)}


def mirror_i2t(x, lens, norm, agg, ls=LAMBDA_SOFTMAX, vnorm=None, cgram=None):
    """scan_xattn.hip:430-638: A = V E^T, H_c = E_c E_c^T (gram_kernel), ||v_r|| (rownorm_kernel); per pair the weights e over the
    caption's words (first norm along the 36 regions per word), num_r = sum_w e a / den, q_r = e^T H_c e clamped at 0,
    s_r = num_r / max(||v_r|| sqrt(q_r) / den, 1e-8) (:552-558, :595-604).  vnorm: a change to the region norms (defect t);
    cgram(c, H): a change to caption c's Gram matrix (defects f, o)."""
    V, E = x['images'], x['words']
    Ni, R, D = V.shape
    A = (V.reshape(Ni * R, D) @ E.t()).view(Ni, R, -1)
    vn = (V * V).sum(2).sqrt()
    if vnorm is not None:
        vn = vnorm(vn)
    shifted = i2t_route(norm, ls) == 'scalar'
    cols = []
    for c, (o, W) in enumerate(zip(_offsets(lens), lens)):
        Ec = E[o:o + W]
        H = Ec @ Ec.t()
        if cgram is not None:
            H = cgram(c, H)
        a = A[:, :, o:o + W]
        e = _weights(a, norm, ls, 1, 2, shifted)
        rden = 1.0 / e.sum(2)
        num = (e * a).sum(2) * rden
        w2 = (e * (e @ H)).sum(2).clamp_min(0.0).sqrt() * rden
        s = num / (vn * w2).clamp_min(1e-8)
        cols.append(_aggregate(s, agg))
    return {'S': torch.stack(cols, 1)}


# ---------------------------------------------------------------------------------------------------------------------
class EvalCase(Case):
    """train_prim_cases.Case with two references (oracle and mirror), the plan and the defects."""

    def __init__(self, group, tag, xa, Ni, D, lens, norm, agg, ls=LAMBDA_SOFTMAX, zero=None, seed=0):
        self.group, self.tag, self.xa, self.Ni, self.D, self.lens = group, tag, xa, Ni, D, tuple(int(w) for w in lens)
        self.Bi, self.R = Ni, SC_R
        self.norm, self.agg, self.ls, self.zero = norm, agg, float(ls), zero
        assert all(w >= 1 for w in self.lens) and D % SC_BK == 0
        self.Nc, self.max_len, self.min_len, self.n_tok = len(self.lens), max(self.lens), min(self.lens), sum(self.lens)
        self.plan = Plan(Ni, D, self.lens, xa, norm, self.ls)
        Case.__init__(self, xa, {}, self._make, None)
        self.name = "%s-%s-%s-Ni%d-D%d-%s-%s%s%s" % (xa, group, tag, Ni, D, norm, agg, "" if self.ls == LAMBDA_SOFTMAX else "-ls%g" % self.ls,
                                                   "-seed%d" % seed if seed else "")
        fn = mirror_t2i if xa == 't2i' else mirror_i2t
        self.mirror = lambda x, **kw: fn(x, self.lens, norm, agg, self.ls, **kw)

    # ---- what the case covers -------------------------------------------------------------------------------------
    @property
    def tied(self):
        """(region row of image 0, word row) that a Max case ties together, else None (scan_train_cases.ScanCase.tied)."""
        if self.agg != 'Max':
            return None
        c = next((k for k, w in enumerate(self.lens) if w > 1), 0)
        return self.R - 1, _offsets(self.lens)[c] + self.lens[c] - 1

    @property
    def big(self):
        """More than 1000 captions: the references walk the captions one by one, so only the defects this size is there for."""
        return self.Nc > 1000

    def _segment_pair(self):
        """(caption that loses its last word, caption of the same tile right behind it that gains it), or None."""
        p = self.plan
        for t in p.tiles:
            for k in range(len(t) - 1):
                if p.k_len[t[k]] > 1:
                    return p.short_idx[t[k]], p.short_idx[t[k + 1]]
        return None

    @property
    def claims(self):
        """The defects this case claims to see (module docstring)."""
        p = self.plan
        out = 'a'
        if not self.big:
            out += 'b' + ('c' if self.max_len > 1 else '')
            if self.xa == 't2i' and self.agg in ('LogSumExp', 'Mean'):
                out += 'p'
            if self._segment_pair() is not None:
                out += 's'
        if self.xa == 't2i' and self.agg == 'Mean' and any(n > 1 for n, _, _ in p.summary):
            out += 'm'
        if self.xa == 'i2t' and p.route == 'mfma' and any(far for _, _, far in p.summary):
            out += 'f'
        if self.Ni % SC_IMGS and self.Ni > 1 and p.n_tiles and (self.xa == 't2i' or self.zero is not None):
            out += 't'
        if self.xa == 'i2t' and p.Nc_kernel > PREFIX_THREADS:
            out += 'o'
        return out

    def seams(self):
        """{parameter: set of values} this case puts into the coverage of SEAMS[direction]."""
        p = self.plan
        ends = set()
        for cs, _, _ in p.layout:
            ends |= set(e - 1 for e in cs[1:] if e > 0)
        s = {'Ni': {self.Ni}, 'Ni%4': {self.Ni % 4}, 'D': {self.D}, 'nk': {p.nk}, 'mainloop': {p.mainloop}, 'n_tiles': {p.n_tiles},
             'img_tiles': {p.img_tiles}, 'PIxPJ': {(p.PI, p.PJ)}, 'PI*PJ': {p.PI * p.PJ}, 'rep': set(p.reps), 'pgroup': set(p.pgroups),
             'tile': set(p.summary), 'ncap': set(n for n, _, _ in p.summary), 'used': set(u for _, u, _ in p.summary),
             'far': set(f for _, _, f in p.summary), 'far_from': p.far_from(), 'cap_end': ends, 'W': set(p.k_len),
             'norm,agg': {(self.norm, self.agg)}, 'Nc_kernel': {p.Nc_kernel}, 'long': set(w for w in self.lens if w > SC_NT),
             'long_at': set(('first' if c == 0 else ('last' if c == self.Nc - 1 else 'middle')) for c in p.long_idx),
             'zero': {self.zero or 'none'}}
        # the tiles that hold W = 1 .. 9 together (E1's four-way unrolled loop and its remainder in one walk)
        s['unroll_tile'] = set(1 for t in p.tiles if set(p.k_len[c] for c in t) >= set(range(1, 10)))
        if self.xa == 'i2t':
            s['route'] = {p.route}
            s['route,norm,ls'] = {(p.route, self.norm, self.ls)}
            s['per'] = {p.per}
            s['W*W'] = set(w * w for w in p.k_len)
            if p.route == 'scalar':
                s['scalar_tile'] = set(x for n, u, far in p.summary for x in (('ncap16',) if n == SC_MAXCAP else ()) + (('far',) if far else ()) +
                                       (('W64',) if n == 1 and u == SC_NT else ()))
        return s

    # ---- inputs and references ----------------------------------------------------------------------------------
    def _make(self, g):
        img = O.l2norm(torch.randn(self.Ni, self.R, self.D, generator=g), -1)
        words = 0.6 * torch.randn(self.n_tok, self.D, generator=g)
        if self.tied:
            r, w = self.tied
            if self.xa == 't2i':
                words[w] = 3.0 * img[0, r]
            else:
                img[0, r] = O.l2norm(words[w:w + 1], -1)[0]
        if self.zero:
            (zi, zr), zw = self.zero
            img[zi, zr] = 0.0
            words[zw] = 0.0
        return {'images': img, 'words': words}

    def evaluate(self, dtype, fn=None, change=None, **kw):
        """S of `fn` (default: the oracle) in `dtype` on the inputs (after `change`, a function of the input dict and the lengths)."""
        x = {k: v.to(dtype).clone() for k, v in self.inputs().items()}
        lens = self.lens
        if change is not None:
            x, lens = change(x, lens)
        if fn is None:
            return T.oracle(x, self.xa, lens, self.norm, self.agg, self.ls)['S']
        assert change is None
        return fn(x, **kw)['S']

    def old_bound(self):
        """What tests/test_kernels_gpu.py holds the fused kernel to on a whole score matrix: 2e-5, x the longest caption's words under t2i
        Sum (test_scan_golden: 9), x 36 under i2t Sum."""
        if self.agg != 'Sum':
            return OLD_BOUND
        return OLD_BOUND * (self.max_len if self.xa == 't2i' else SC_R)

    def reference(self):
        """(want float64, e32_oracle, e32_mirror, tol, max |mirror float64 - want|); computed once and shared."""
        if 'ref' not in self._cache:
            want, w32 = self.evaluate(torch.float64), self.evaluate(torch.float32)
            m64, m32 = self.evaluate(torch.float64, self.mirror), self.evaluate(torch.float32, self.mirror)
            eo, em = float((w32.double() - want).abs().max()), float((m32.double() - want).abs().max())
            tol = FALLBACK.get(self.name, FACTOR * max(eo, em, U * float(want.abs().max())))
            self._cache['ref'] = (want, eo, em, tol, float((m64 - want).abs().max()))
        return self._cache['ref']

    def defects(self):
        """{letter: float64 S with the defect} for every claimed defect."""
        lens0, p = self.lens, self.plan
        off0 = _offsets(lens0)

        def zero_last_feature(x, lens):
            x['images'][..., -1] = 0.0
            x['words'][..., -1] = 0.0
            return x, lens

        def drop_last_region(x, lens):
            x['images'] = x['images'][:, :-1].clone()
            return x, lens

        def regroup(x, new_rows):
            """words re-packed: new_rows[c] = the rows of the old packed array (or -1: a zero word) of caption c"""
            z = torch.zeros(1, x['words'].shape[1], dtype=x['words'].dtype)
            src = torch.cat([x['words'], z], 0)
            idx = [r if r >= 0 else x['words'].shape[0] for rows in new_rows for r in rows]
            x['words'] = src[idx].clone()
            return x, tuple(len(rows) for rows in new_rows)

        rows0 = [list(range(o, o + w)) for o, w in zip(off0, lens0)]

        def drop_last_words(x, lens):
            return regroup(x, [r[:-1] if len(r) > 1 else r for r in rows0])

        def pad_counted(x, lens):
            c = lens0.index(self.min_len)
            return regroup(x, [r + [-1] if k == c else r for k, r in enumerate(rows0)])

        def boundary_off_by_one(x, lens):
            k0, k1 = self._segment_pair()
            return regroup(x, [r[:-1] if k == k0 else ([rows0[k0][-1]] + r if k == k1 else r) for k, r in enumerate(rows0)])

        def far_blocks_skipped(c, H):
            if c not in p.cap_col:
                return H
            col = torch.arange(H.shape[0]) + p.cap_col[c][1]
            blk = col >> 4
            return torch.where((blk[:, None] - blk[None, :]).abs() >= 2, torch.zeros_like(H), H)

        out = {}
        for letter in self.claims:
            if letter in 'abcps':
                change = {'a': zero_last_feature, 'b': drop_last_region, 'c': drop_last_words, 'p': pad_counted, 's': boundary_off_by_one}[letter]
                out[letter] = self.evaluate(torch.float64, change=change)
            elif letter == 'm':
                scale = torch.ones(self.Nc, dtype=torch.float64)
                for c, (ti, _) in p.cap_col.items():
                    scale[c] = lens0[c] / float(p.summary[ti][1])
                out[letter] = self.reference()[0] * scale
            elif letter == 'f':
                out[letter] = self.evaluate(torch.float64, self.mirror, cgram=far_blocks_skipped)
            elif letter == 't':
                def first_for_last(v):
                    v = v.clone()
                    v[-1] = v[0]
                    return v
                out[letter] = self.evaluate(torch.float64, self.mirror, **({'gram': first_for_last} if self.xa == 't2i' else {'vnorm': first_for_last}))
            else:
                assert letter == 'o' and not p.long_idx
                x64 = self.inputs()['words'].double()
                flat = torch.cat([(x64[o:o + w] @ x64[o:o + w].t()).reshape(-1) for o, w in zip(off0, lens0)])
                goff = _offsets([w * w for w in lens0])                 # scan_xattn.hip:780-797 (sq_prefix_kernel)

                def wrapped_offset(c, H):
                    if c < PREFIX_THREADS:
                        return H
                    W = H.shape[0]
                    return flat[goff[c - PREFIX_THREADS]:goff[c - PREFIX_THREADS] + W * W].view(W, W)
                out[letter] = self.evaluate(torch.float64, self.mirror, cgram=wrapped_offset)
        return out


# The inputs are seeded from the case's name.  A case whose seed fails the conditioning cap takes another seed here; the seam stays.
RESEED = {}


def _add(group, tag, xa, Ni, D, lens, norm, agg, ls=LAMBDA_SOFTMAX, zero=None):
    c = EvalCase(group, tag, xa, Ni, D, lens, norm, agg, ls, zero)
    if c.name in RESEED:
        c = EvalCase(group, tag, xa, Ni, D, lens, norm, agg, ls, zero, seed=RESEED[c.name])
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(xa, group=None):
    return [c for c in CASES if c.xa == xa and (group is None or c.group == group)]


def _seam(xa, **params):
    SEAMS.setdefault(xa, {}).update({k: sorted(set(v), key=str) for k, v in params.items()})


_count = {'t2i': 0, 'i2t': 0}


def _agg(xa):
    """The next aggregation of a direction's rotation."""
    _count[xa] += 1
    return AGGS[(_count[xa] - 1) % 4]


DIRECTIONS = ('t2i', 'i2t')
DEFAULT = 'clipped_l2norm'
LENS16 = (1, 2, 15, 16, 17, 31, 33, 5, 9, 12, 3, 7, 64, 48, 49, 63)

# every first norm x every aggregation: Ni = 5 (one full workgroup of images and a tail of one), D = 96 (the pipelined main loop's
# shortest trip), captions across every 16-column block seam with a full-tile caption
for _xa in DIRECTIONS:
    for _n in NORMS:
        for _a in AGGS:
            _add('norm', 'lens16', _xa, 5, 96, LENS16, _n, _a)
    _seam(_xa, **{'norm,agg': [(n, a) for n in NORMS for a in AGGS]})

# the main loop: D / 32 = 1, 2 (the plain loop), 3 (prologue and peeled tail only), 4 .. 8 (every length of the steady state up to five
# trips), 32 (the headline's D = 1024)
MAINLOOP_D = (32, 64, 96, 128, 160, 192, 224, 256, 1024)
for _xa in DIRECTIONS:
    for _D in MAINLOOP_D:
        _add('D', 'lens16', _xa, 5, _D, LENS16, DEFAULT, 'LogSumExp')
    _seam(_xa, D=MAINLOOP_D, nk=[d // 32 for d in MAINLOOP_D], mainloop=('simple', 'pipelined'))

# the image tail (waves whose image does not exist, tail rows that re-read row 0) and the image tiles on 8 | 9 (Ni 32 | 33: PI 1 | 2),
# with two column tiles
TAIL_NI = (1, 2, 3, 4, 5, 8, 31, 32, 33)
TWO_TILES = (40, 20, 30, 25, 4, 9)
for _xa in DIRECTIONS:
    for _Ni in TAIL_NI:
        _add('Ni', 'twotiles', _xa, _Ni, 96, TWO_TILES, DEFAULT, _agg(_xa))
    _seam(_xa, Ni=TAIL_NI + (65,), img_tiles=(1, 2, 8, 9, 17), **{'Ni%4': (0, 1, 2, 3)})

# column tiles on 8 | 9 (PJ 1 | 2) and 16 | 17 (PJ 2 | 3), and 1 and 7, with Ni = 5: tiles of (40, 24) words
GRID_TILES = (1, 7, 8, 9, 16, 17)
for _xa in DIRECTIONS:
    for _nt in GRID_TILES:
        _add('tiles', '%dx40.24' % _nt, _xa, 5, 96, (40, 24) * _nt, DEFAULT, _agg(_xa))
    # PI * PJ = 9 as 3 x 3 (patches 8 is the second `rep` of pgroup 0); 16 | 17 as 1 x 16 | 1 x 17 (patch 16: the second pgroup)
    _add('patch', '3x3', _xa, 65, 32, (64,) * 17, DEFAULT, _agg(_xa))
    _add('patch', '1x16', _xa, 3, 32, (64,) * 128, DEFAULT, _agg(_xa))
    _add('patch', '1x17', _xa, 3, 32, (64,) * 129, DEFAULT, _agg(_xa))
    _seam(_xa, n_tiles=GRID_TILES + (128, 129), PIxPJ=((1, 1), (1, 2), (1, 3), (2, 1), (3, 3), (1, 16), (1, 17)), rep=(0, 1), pgroup=(0, 1),
          **{'PI*PJ': (1, 2, 3, 9, 16, 17)})

# tile composition.  Each set is scored together with a caption of 57 words and one of 7: they fill a tile between themselves, so several
# tiles exist and the planner leaves the set's tile as the row says (captions of 7 words alone would be packed INTO the set's tile
# and e.g. break up the sixteen one-word captions).
COMPANIONS = (57, 7)
COMPOSITION = {
    'one64': ((64,), (1, 64, 1)),                                           # a full tile of one caption
    'sixteen4': ((4,) * 16, (16, 64, 0)),                                   # a full tile of SC_MAXCAP captions
    'sixteen1': ((1,) * 16, (16, 16, 0)),                                   # 48 padding columns
    'seventeen1': ((1,) * 17, (1, 1, 0)),                                   # ... and a second tile that holds one caption of one word
    'blockseams': ((15, 16, 17, 31, 32, 33, 47, 48, 49, 63), (2, 64, 1)),   # one caption each on, before and behind the block seams
    '32.32': ((32, 32), (2, 64, 0)),                                        # `far` = 0 in a full tile
    '33.31': ((33, 31), (2, 64, 1)),                                        # `far` from the first caption
    '31.18.15': ((31, 18, 15), (3, 64, 1)),                                 # `far` from the second caption (columns 31 .. 48)
    'one2nine': (tuple(range(1, 10)), (9, 45, 0)),                          # E1's unrolled loop and its remainder, W = 1 .. 9
}
for _xa in DIRECTIONS:
    for _tag, (_set, _tile) in COMPOSITION.items():
        for _n in (DEFAULT, 'softmax') + (('no_norm',) if _xa == 'i2t' else ()):
            _c = _add('tile', _tag, _xa, 5, 96, _set[:len(_set) // 2] + COMPANIONS + _set[len(_set) // 2:], _n, _agg(_xa))
            assert _tile in _c.plan.summary and _c.plan.n_tiles >= 2, (_c, _c.plan.summary)
    _seam(_xa, tile=[t for _, t in COMPOSITION.values()], ncap=(1, 2, 3, 9, 16), used=(1, 16, 45, 64), far=(0, 1), far_from=('first', 'later'),
          W=tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64), unroll_tile=(1,))

# t2i: E3's segmented scan with a caption ending on every lane.  The rows above leave 16 lanes out; a tile lays its captions out largest
# first, so these four descending sets put their running sums on them (18 19 | 25 27 | 23 37 46 54 59 | 22 34 43 51 58 61 62)
ENDS = {'18.1': (18, 1), '25.2': (25, 2), '23to5': (23, 14, 9, 8, 5), '22to1': (22, 12, 9, 8, 7, 3, 1)}
for _tag, _set in ENDS.items():
    _add('ends', _tag, 't2i', 5, 96, _set[:1] + COMPANIONS + _set[1:], DEFAULT, _agg('t2i'))
_seam('t2i', cap_end=range(64))

# the i2t preparation: sq_prefix_kernel's items per thread (Nc on 1023 | 1024 | 1025 and 2049: per = 1 | 1 | 2 | 3), gram_kernel's
# pairs per thread (W * W on 256 | 289 and 4096, the whole register array), scan_hblk_kernel behind both
for _Nc in (1023, 1024, 1025, 2049):
    _add('prep', 'Nc%d' % _Nc, 'i2t', 1, 32, [(k * 7 + 2) % 2 + 1 for k in range(_Nc)], DEFAULT, 'LogSumExp')
_add('prep', 'W16.17.64', 'i2t', 1, 32, (16, 17, 64), DEFAULT, 'LogSumExp')
_seam('i2t', Nc_kernel=(1023, 1024, 1025, 2049), per=(1, 2, 3), **{'W*W': (256, 289, 4096)})

# the i2t route gate on both sides for the first norms that can take the matrix cores; and the scalar route (behind the gate, and
# no_norm / clipped at any lambda) on what it has never met: a tile of 16 captions, a `far` tile, a caption of 64 words.
# The gate stood at |lambda_softmax| <= 60 when this table was written, and its cases at 60 | 60.5 found it wrong: the matrix-core
# route takes no maximum out, so q = e^T H e holds exp(2 lambda b) for normalised logits |b| <= 1 -- exp(120) at the gate, beyond
# float32 (inf for b > 0.74, which clipped_l2norm reaches on this recipe's inputs; 0 for a caption whose largest logit is below
# -0.73).  It now stands at 30, where exp(+-60) leaves e^28 of float32's range to W * max|H| above and to ||word||^2 below.  Both
# pairs stay: 60 | 60.5 (both scalar now) and 30 | 30.5, the latter with every aggregation (the tie under Max puts b ~ 0.85 there).
GATE_LENS = (33, 64) + (4,) * 16 + (31,)
GATE_NORMS = ('clipped_l2norm', 'l2norm', 'softmax', 'l1norm')
for _n in GATE_NORMS:
    for _ls in (60.0, 60.5):
        _add('gate', 'mixed', 'i2t', 5, 96, GATE_LENS, _n, 'LogSumExp', ls=_ls)
for _j, _n in enumerate(GATE_NORMS):
    for _ls in (I2T_MFMA_LS, I2T_MFMA_LS + 0.5):
        _add('gate', 'mixed', 'i2t', 5, 96, GATE_LENS, _n, AGGS[_j], ls=_ls)
for _n in ('no_norm', 'clipped'):
    for _a in ('LogSumExp', 'Mean'):
        _add('gate', 'mixed', 'i2t', 5, 96, GATE_LENS, _n, _a)
_seam('i2t', route=('mfma', 'scalar'), scalar_tile=('ncap16', 'far', 'W64'),
      **{'route,norm,ls': [(r, n, l) for n in GATE_NORMS for r, l in (('mfma', 30.0), ('scalar', 30.5), ('scalar', 60.0), ('scalar', 60.5))] +
         [('scalar', 'no_norm', 9.0), ('scalar', 'clipped', 9.0)]})

# captions of more than 64 words leave the fused kernel for the pair kernels (ops._scan_scores_with_long_captions): a caption of 65
# and one of 96 words at the first, a middle and the last caption index, and a set without any caption for the fused kernel
SHORT = (5, 9, 12, 3, 7, 20)
LONG_SETS = {'first.middle': (65,) + SHORT[:3] + (96,) + SHORT[3:], 'middle.last': SHORT[:2] + (96,) + SHORT[2:] + (65,),
             'last.first': (96,) + SHORT + (65,), 'all': (65, 96, 70)}
for _xa in DIRECTIONS:
    for _j, (_tag, _ls_) in enumerate(LONG_SETS.items()):
        _add('long', _tag, _xa, 5, 96, _ls_, NORMS[(2 * _j) % 7] if _j else DEFAULT, _agg(_xa))
    _seam(_xa, long=(65, 96), long_at=('first', 'middle', 'last'), Nc_kernel=SEAMS[_xa].get('Nc_kernel', []) + [0])

# degenerate rows: an all-zero word inside a caption and an all-zero region (image 0, so that the last image read with image 0's
# region norms is seen: defect t of i2t)
for _xa in DIRECTIONS:
    for _n in (DEFAULT, 'softmax'):
        _add('zero', 'word.region', _xa, 5, 96, (5, 9, 12, 3), _n, 'LogSumExp', zero=((0, 7), 8))
    _seam(_xa, zero=('none', ((0, 7), 8)))

assert all(k + '-seed%d' % v in _BY_NAME for k, v in RESEED.items())
