"""Case table of the SCAN candidate-list kernels (csrc/scan_pairs.hip and csrc/scan_attn.hip over pair_mainloop.h / pair_epilogue.h,
reached through ops.scan_candidate_scores and ops.scan_pair_attention) and their float64 references.

One entry per (kernel, direction, images, D, caption lengths, pair list, first norm, aggregation, lambda_softmax).  `kernel` is
'scores' (the list arrives as `cand` + `by`, or -- direct ABI -- as a caption-major list of the case's own making) or 'attention'
(a [P, 2] pair list).  Inputs by the recipe of scan_eval_cases.EvalCase._make: l2-normalised regions, words = 0.6 * randn, packed,
seeded from the case's name, the Max tie put on the first listed pair.

REFERENCES, per compared tensor (scores: `score`; attention: `attn`, `row_sim`, `score`; every tensor flat, in pair order):
    oracle   scores: scan_train_cases.oracle on the listed captions only, re-packed.  attention: itr_oracle.func_attention and the
             cosine of Objectives.py:10-15, as tests/test_scan_attention_gpu.py:oracle_pairs.  float64 = want, float32 -> e32_oracle
    mirror   plain torch per direction after the pair kernels' algebra where it differs from the literal order: the raw block from one
             product, the first-norm statistics as reciprocals, the maximum always taken out of the softmax, q = e^T G e through the
             Gram matrix (upper-triangular for t2i), clamped at 0, the cosine clamp at 1e-8; i2t attention above 64 words sums
             ||ctx||^2 over D directly.  Captions of 65..96 words of a `scores` case leave for the training path
             (ops._long_caption_pairs): their mirror is the training table's.  float32 -> e32_mirror, float64 == oracle to MIRROR_AGREES

Tolerance per tensor (tests/test_scan_pairs_seams_gpu.py applies it, tests/test_scan_pairs_case_table.py proves it):
    tol = FACTOR * max(e32_oracle, e32_mirror, U * max|want|)
with tol <= CAP * max|want| and, for scores and cosines, tol <= 2e-5 (the score under Sum: x the longest listed caption's words (t2i), x 36 (i2t)).

The planning is mirrored in plain Python, each function marked with the source lines it copies.  SEAMS[kernel, direction] lists the
values that must appear in the table; PairCase.seams() reports what a case contributes.

Defects, all float64 (PairCase.claims says which a case claims and why not the others):
    a  the last feature of images and words zeroed                                                 oracle on changed inputs
    b  the last region dropped                                                                     oracle on changed inputs
    c  the last word of every caption of more than one word dropped                                oracle on changed inputs
    r  the last word of every caption counted twice: what the main loop's column clamp (columns past the caption re-read its last
       word) would give if the epilogue read one column too far                                    oracle on changed inputs
    n  a pair scored with the image of the neighbouring slot (slot ^ 1) of its workgroup           want, re-gathered
    k  scores: the pairs 9.. of a caption scored with the next listed caption's words -- the bisection over blk_ptr off by one
       across equal neighbours                                                                     want, re-gathered
    g  i2t: the Gram matrix of the previously listed caption (its flat W' x W' floats read as W x W)   mirror
    o  i2t: caption c >= 1024 read with the Gram offset of caption c - 1024                        mirror
    t  t2i: the last image scored with image 0's Gram matrix                                       mirror
    2  attention: the second main-loop pass lost, the raw block of words 64.. is zero              mirror
    l  attention, t2i: the second round of lanes missing from the aggregate                        want, re-aggregated
    T  attention: the block stored as [36, W]                                                      want, re-laid
    d  attention: the weights not divided by den                                                   mirror
Exemptions, those of scan_eval_cases: under Max, b (i2t) and c (t2i) are decisive only where the dropped element carries the
maximum -- the tie, which sits on a listed pair.  r under t2i adds a second copy of a term: Max does not move, nor does Mean of a
one-word caption, and with no_norm / clipped (no statistics along the words) the other terms do not move either; r under i2t moves
nothing for a one-word caption (its context vector is that word at any weight).  l under Max needs the maximum among words 64..:
not claimed.  Nothing here imports the library: the table is checked on a machine without a GPU."""
import torch

import itr_oracle as O
import scan_train_cases as T
from scan_train_cases import NORMS, AGGS, LAMBDA_LSE, CAP, MIRROR_AGREES, FALLBACK_SHARE, ceil_div, _offsets      # noqa: F401
from train_prim_cases import Case, U, FACTOR, SENSITIVITY        # noqa: F401  (re-exported)

LAMBDA_SOFTMAX = 9.0
OLD_BOUND = 2e-5
SC_R = 36                                                           # scan_common.h:7

# geometry of the kernels (pinned to csrc/ by tests/test_scan_pairs_case_table.py)
SP_IMGS = 8                                                         # scan_pairs.hip:44: pairs (= waves) per workgroup
SP_BK = 16                                                          # pair_mainloop.h:9
SP_LDP = 37                                                         # pair_mainloop.h:8
SP_MAXW = 64                                                        # pair_epilogue.h:13
SA_WAVES = 4                                                        # scan_attn.hip:34
SA_MAXW = 96                                                        # scan_attn.hip:36
PREFIX_THREADS = 1024                                               # scan_pairs.hip:248 (pairs_blkptr_kernel), scan_xattn.hip:780 (sq_prefix_kernel)
STAGE_THREADS = SP_IMGS * 64                                        # scan_pairs.hip:45, :187: the threads that stage W^2 Gram floats

KERNELS = ('scores', 'attention')
DIRECTIONS = ('t2i', 'i2t')
TENSORS = {'scores': ('score',), 'attention': ('attn', 'row_sim', 'score')}
SEAMS = {}          # (kernel, direction) -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule and that are judged by a derived a-priori bound instead:
# name -> {tensor: bound}, the derivation in a comment next to the entry.  No case needs it (profiles/scan_pairs_seams/measured.txt).
FALLBACK = {}


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the planning
def ncb(W):
    """scan_pairs.hip:121, scan_attn.hip:111: 16-column word tiles of the main loop (1..4 per pass; 5, 6: a second pass of 1, 2)."""
    return (W + 15) >> 4


def chunks(D):
    """pair_mainloop.h:39-40: trips of the K loop; the last one prefetches its own chunk again (kn = k0)."""
    return D // SP_BK


def blocks_of(n):
    """scan_pairs.hip:253-256 (pairs_blkptr_kernel: blocks): workgroups of a caption that n pairs list."""
    return (n + SP_IMGS - 1) // SP_IMGS if n > 0 else 0


def prefix_per(n):
    """scan_pairs.hip:251 (pairs_blkptr_kernel) and scan_xattn.hip:784 (sq_prefix_kernel): captions per thread of the one workgroup."""
    return (n + PREFIX_THREADS - 1) // PREFIX_THREADS


def blk_ptr_of(counts):
    """scan_pairs.hip:248-269 (pairs_blkptr_kernel), thread by thread: per-thread partial sums over `per` captions, their exclusive
    scan, the running offsets.  -> blk_ptr[Nc + 1]."""
    n = len(counts)
    per = prefix_per(n)
    part, out = [], [0] * (n + 1)
    for t in range(PREFIX_THREADS):
        b = min(t * per, n)
        e = b + per if b + per < n else n
        part.append(sum(blocks_of(counts[i]) for i in range(b, e)))
    run, starts = 0, []
    for v in part:
        starts.append(run)
        run += v
    out[n] = run
    for t in range(PREFIX_THREADS):
        b = min(t * per, n)
        e = b + per if b + per < n else n
        r = starts[t]
        for i in range(b, e):
            out[i] = r
            r += blocks_of(counts[i])
    return out


def bisect_caption(blk_ptr, b, Nc):
    """scan_pairs.hip:97-102: the caption workgroup b lands on, blk_ptr[lo] <= b < blk_ptr[hi]."""
    lo, hi = 0, Nc
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if blk_ptr[mid] <= b:
            lo = mid
        else:
            hi = mid
    return lo


def grid_bound(P, Nc):
    """scan_pairs.hip:332: the grid of scan_pairs_kernel, a bound on sum_c ceil(n_c / 8)."""
    return P // SP_IMGS + min(Nc, P) + 1


def sq_offsets(klen):
    """scan_xattn.hip:780-797 (sq_prefix_kernel) on the lengths the pair kernels are given (0 for a long caption): the Gram offsets."""
    return _offsets([w * w for w in klen])


def attn_unit(p, W):
    """scan_attn.hip:86 and :141: (workgroup, wave) of pair p and its rounds of lane = word."""
    return p // SA_WAVES, p % SA_WAVES, ceil_div(W, 64)


class ScoresPlan(object):
    """What ops.scan_candidate_scores (or a direct call) hands to itr_scan_pair_scores and what the kernel makes of it."""

    def __init__(self, Ni, lens, pairs, reverse=False):
        Nc = len(lens)
        self.klen = [w if w <= SP_MAXW else 0 for w in lens]                    # ops.py: _caption_tables(plan, dev, SCAN_NT)
        self.long_pairs = [s for s, (i, c) in enumerate(pairs) if self.klen[c] == 0]      # ops.py: _long_caption_pairs
        per_cap = [[] for _ in range(Nc)]
        for s, (i, c) in enumerate(pairs):                                       # ops.py: _group_pairs (stable by caption)
            if self.klen[c]:
                per_cap[c].append((i, s))
        if reverse:
            per_cap = [list(reversed(v)) for v in per_cap]
        self.per_cap = per_cap
        self.counts = [len(v) for v in per_cap]
        self.P = sum(self.counts)
        self.cap_ptr = [0]
        for n in self.counts:
            self.cap_ptr.append(self.cap_ptr[-1] + n)
        self.pair_img = [i for v in per_cap for i, _ in v]
        self.pair_out = [s for v in per_cap for _, s in v]
        self.blk_ptr = blk_ptr_of(self.counts)
        self.n_blocks = self.blk_ptr[Nc]
        self.grid = grid_bound(self.P, Nc) if self.P else 0
        assert self.n_blocks <= self.grid
        # every workgroup finds the caption that owns it
        self.blocks, owner = [], [c for c in range(Nc) for _ in range(blocks_of(self.counts[c]))]
        for b in range(self.n_blocks):
            c = bisect_caption(self.blk_ptr, b, Nc)
            assert c == owner[b], (b, c, owner[b])
            k = b - self.blk_ptr[c]
            self.blocks.append((c, per_cap[c][k * SP_IMGS:(k + 1) * SP_IMGS]))
        self.per = prefix_per(Nc)

    def describe(self):
        nz = [n for n in self.counts if n]
        return "pairs %d (long %d) captions listed %d of %d counts %s blocks %d grid %d per %d" % (
            self.P, len(self.long_pairs), len(nz), len(self.counts), sorted(set(nz)), self.n_blocks, self.grid, self.per)


# ---------------------------------------------------------------------------------------------------------------------
# the references, dtype-generic; every function -> (attn [Ni, W, R], sims [Ni, W | R], score [Ni]) of one caption and all images
def _cosine(x1, x2, eps=1e-8):
    """cosine_similarity, Objectives.py:10-15"""
    w12 = torch.sum(x1 * x2, -1)
    return w12 / (torch.norm(x1, 2, -1) * torch.norm(x2, 2, -1)).clamp(min=eps)


def oracle_caption(V, Ec, xa, norm, agg, ls):
    """tests/test_scan_attention_gpu.py:oracle_pairs for one caption."""
    e = Ec.unsqueeze(0).expand(V.shape[0], Ec.shape[0], -1)
    if xa == 't2i':
        ctx, a = O.func_attention(e, V, norm, ls)
        sims = _cosine(e, ctx)
    else:
        ctx, a = O.func_attention(V, e, norm, ls)
        a = a.transpose(1, 2)
        sims = _cosine(V, ctx)
    return a.contiguous(), sims, O._aggregate(sims, agg, LAMBDA_LSE)


def _leaky(a):
    return torch.where(a > 0, a, 0.1 * a)


def _apply(a, norm, dim):
    """pair_epilogue.h:16-40 (PairNorm): the first norm along `dim`, its statistics stored as reciprocals."""
    b = _leaky(a) if norm in ('clipped_l2norm', 'clipped', 'clipped_l1norm') else a
    if norm in ('clipped_l2norm', 'l2norm'):
        return b * (1.0 / ((b * b).sum(dim, keepdim=True).sqrt() + 1e-8))
    if norm in ('l1norm', 'clipped_l1norm'):
        return b * (1.0 / (b.abs().sum(dim, keepdim=True) + 1e-8))
    if norm == 'softmax':
        ex = torch.exp(a - a.max(dim, keepdim=True)[0])
        return ex * (1.0 / ex.sum(dim, keepdim=True))
    assert norm in ('clipped', 'no_norm'), norm
    return b


def _pair_aggregate(s, agg):
    """scan_pairs.hip:75-85 (pair_aggregate), scan_attn.hip:65-78 (AttnAgg): no maximum is taken out of the LSE."""
    if agg == 'LogSumExp':
        return torch.log(torch.exp(s * LAMBDA_LSE).sum(1)) / LAMBDA_LSE
    if agg == 'Max':
        return s.max(1)[0]
    return s.sum(1) if agg == 'Sum' else s.sum(1) / s.shape[1]


def mirror_caption_t2i(V, Ec, norm, agg, ls, gram=None, araw=None, keep_den=False):
    """scan_pairs.hip:130-181, scan_attn.hip:126-180: a = V E_c^T; statistics along the caption's words per region; per word
    e = exp(x - max_r x), den, num = sum e a, q = e^T G' e with G' the upper-triangular form (scan_xattn.hip:652), w2 = sqrt(max(q, 0)) / den,
    sim = (num / den) / max(||e_w|| w2, 1e-8); the word's attention is e / den.  gram / araw: changes to G and to the raw block
    (defects t, 2); keep_den: defect d."""
    a = V @ Ec.t()                                                       # (Ni, R, W)
    if araw is not None:
        a = araw(a)
    G = V @ V.transpose(1, 2)
    G = torch.triu(G, 1) * 2.0 + torch.diag_embed(torch.diagonal(G, dim1=1, dim2=2))
    if gram is not None:
        G = gram(G)
    x = _apply(a, norm, 2) * ls
    e = torch.exp(x - x.max(1, keepdim=True)[0])
    rden = 1.0 / e.sum(1)                                                # (Ni, W)
    num = (e * a).sum(1)
    q = (e * (G @ e)).sum(1)
    w1 = (Ec * Ec).sum(1).sqrt()
    w2 = q.clamp_min(0.0).sqrt() * rden
    sims = (num * rden) / (w1 * w2).clamp_min(1e-8)
    attn = (e if keep_den else e * rden.unsqueeze(1)).transpose(1, 2)
    return attn.contiguous(), sims, _pair_aggregate(sims, agg)


def mirror_caption_i2t(V, Ec, norm, agg, ls, direct=False, cgram=None, araw=None, keep_den=False):
    """scan_pairs.hip:190-241, scan_attn.hip:182-253: statistics along the 36 regions per word; per region e = exp(x - max_w x), den,
    num = sum e a, q = e^T H_c e (direct: ||sum_w e_w E_w||^2 summed over D, scan_attn.hip:229-243), w2 = sqrt(max(q, 0)) / den,
    sim = (num / den) / max(||v_r|| w2, 1e-8); the region's attention is e / den.  cgram / araw: changes to H_c and to the raw block
    (defects g, o, 2); keep_den: defect d."""
    a = V @ Ec.t()                                                       # (Ni, R, W)
    if araw is not None:
        a = araw(a)
    x = _apply(a, norm, 1) * ls
    e = torch.exp(x - x.max(2, keepdim=True)[0])
    rden = 1.0 / e.sum(2)                                                # (Ni, R)
    num = (e * a).sum(2)
    if direct:
        ctx = e @ Ec
        q = (ctx * ctx).sum(2)
    else:
        H = Ec @ Ec.t()
        if cgram is not None:
            H = cgram(H)
        q = (e * (e @ H)).sum(2)
    w1 = (V * V).sum(2).sqrt()
    w2 = q.clamp_min(0.0).sqrt() * rden
    sims = (num * rden) / (w1 * w2).clamp_min(1e-8)
    attn = (e if keep_den else e * rden.unsqueeze(2)).transpose(1, 2)
    return attn.contiguous(), sims, _pair_aggregate(sims, agg)


# ---------------------------------------------------------------------------------------------------------------------
class PairCase(Case):
    """train_prim_cases.Case with two references (oracle and mirror), the plan and the defects."""

    def __init__(self, kernel, group, tag, xa, Ni, D, lens, norm, agg, cand=None, by=None, pairs=None, abi=False, ls=LAMBDA_SOFTMAX,
                 zero=None, seed=0):
        self.kernel, self.group, self.tag, self.xa, self.Ni, self.D = kernel, group, tag, xa, Ni, D
        self.lens = tuple(int(w) for w in lens)
        self.R, self.Nc, self.n_tok = SC_R, len(self.lens), sum(self.lens)
        self.norm, self.agg, self.ls, self.zero, self.abi = norm, agg, float(ls), zero, bool(abi)
        self.cand, self.by = cand, by
        assert kernel in KERNELS and all(1 <= w <= SA_MAXW for w in self.lens) and D % SP_BK == 0
        if cand is not None:
            assert kernel == 'scores' and pairs is None and by in ('caption', 'image')
            K = len(cand[0])
            assert len(cand) == (self.Nc if by == 'caption' else Ni) and all(len(r) == K for r in cand)
            pairs = [((e, q) if by == 'caption' else (q, e)) for q, row in enumerate(cand) for e in row]
        self.pairs = [(int(i), int(c)) for i, c in pairs]
        assert all(0 <= i < Ni and 0 <= c < self.Nc for i, c in self.pairs)
        self.P = len(self.pairs)
        self.listed = sorted(set(c for _, c in self.pairs))
        self.listed_lens = [self.lens[c] for c in self.listed]
        self.off = _offsets(self.lens)
        if kernel == 'scores':
            self.plan = ScoresPlan(Ni, self.lens, self.pairs, reverse=self.abi)
            assert not (self.abi and self.plan.long_pairs)
        else:
            self.plan = None
        Case.__init__(self, xa, {}, self._make, None)
        self.name = "%s-%s-%s-%s-Ni%d-D%d-%s-%s%s%s" % (kernel, xa, group, tag, Ni, D, norm, agg, "" if self.ls == LAMBDA_SOFTMAX else "-ls%g" % self.ls,
                                                      "-seed%d" % seed if seed else "")

    # ---- what the case covers -------------------------------------------------------------------------------------
    @property
    def tied(self):
        """(image, region row, word row) that a Max case ties together -- on its first listed pair whose caption has more than one
        word (else on its first pair) -- else None (scan_train_cases.ScanCase.tied)."""
        if self.agg != 'Max':
            return None
        i, c = next(((i, c) for i, c in self.pairs if self.lens[c] > 1), self.pairs[0])
        return i, self.R - 1, self.off[c] + self.lens[c] - 1

    def taken(self, c):
        """Whether the kernel under test scores caption c itself (a `scores` case hands 65..96 words to the training path)."""
        return self.kernel == 'attention' or self.lens[c] <= SP_MAXW

    def units(self):
        """The kernel's groups of pairs that share a workgroup, as lists of pair indices in wave order."""
        if self.kernel == 'scores':
            return [[s for _, s in blk] for _, blk in self.plan.blocks]
        return [list(range(p, min(p + SA_WAVES, self.P))) for p in range(0, self.P, SA_WAVES)]

    def _neighbour(self):
        """pair -> the pair in slot ^ 1 of its workgroup (or itself)."""
        out = list(range(self.P))
        for u in self.units():
            for j, p in enumerate(u):
                if (j ^ 1) < len(u):
                    out[p] = u[j ^ 1]
        return out

    def _next_caption(self):
        """scores: pair -> the next listed caption the kernel takes, for the pairs 9.. of a caption (else None)."""
        out, nz = {}, [c for c, n in enumerate(self.plan.counts) if n]
        for k, c in enumerate(nz[:-1]):
            for _, s in self.plan.per_cap[c][SP_IMGS:]:
                out[s] = nz[k + 1]
        return out

    @property
    def claims(self):
        """The defects this case claims to see (module docstring)."""
        L = [self.lens[c] for c in self.listed]
        K = [self.lens[c] for c in self.listed if self.taken(c)]
        out = 'ab'
        if max(L) > 1:
            out += 'c'
        stats = self.norm not in ('no_norm', 'clipped')
        if self.xa == 't2i':
            if self.agg in ('LogSumExp', 'Sum') or (self.agg == 'Mean' and max(L) > 1) or (self.agg == 'Max' and stats and max(L) > 1):
                out += 'r'
        elif max(L) > 1:
            out += 'r'
        nb = self._neighbour()
        if any(self.pairs[p][0] != self.pairs[q][0] and self.taken(self.pairs[p][1]) for p, q in enumerate(nb)):
            out += 'n'
        if self.kernel == 'scores' and self._next_caption():
            out += 'k'
        short = [c for c in self.listed if self.lens[c] <= SP_MAXW]
        if self.xa == 'i2t' and len(short) >= 2:
            out += 'g'
        if self.xa == 'i2t' and any(c >= PREFIX_THREADS for c in short):
            out += 'o'
        if self.xa == 't2i' and self.Ni > 1 and any(i == self.Ni - 1 and self.taken(c) for i, c in self.pairs):
            out += 't'
        if self.kernel == 'attention':
            if max(L) > SP_MAXW:
                out += '2' + ('l' if self.xa == 't2i' and self.agg != 'Max' else '')
            out += ('T' if max(L) > 1 else '') + 'd'
        assert K or self.kernel == 'scores'
        return out

    def seams(self):
        """{parameter: set of values} this case puts into the coverage of SEAMS[kernel, direction]."""
        K = [self.lens[c] for c in self.listed if self.taken(c)]
        s = {'D': {self.D}, 'chunks': {chunks(self.D)}, 'W': set(K), 'ncb': set(ncb(w) for w in K), 'Nc': {self.Nc}, 'Ni': {self.Ni},
             'norm,agg': {(self.norm, self.agg)}, 'ls': {self.ls}, 'zero': {self.zero or 'none'}, 'abi': {int(self.abi)},
             'long_at': set(('first' if c == 0 else ('last' if c == self.Nc - 1 else 'middle')) for c in self.listed if self.lens[c] > SP_MAXW),
             'only_long': {int(all(self.lens[c] > SP_MAXW for c in self.listed))},
             'image': set(['last'] if any(i == self.Ni - 1 for i, _ in self.pairs) else [])}
        if self.xa == 'i2t':
            s['W*W'] = set(w * w for w in K if w <= SP_MAXW)
            s['stage'] = set(('<=' if w * w <= STAGE_THREADS else '>') + '512' for w in K if w <= SP_MAXW)
            s['per'] = {prefix_per(self.Nc)}
        if self.kernel == 'scores':
            p = self.plan
            s['by'] = {self.by or 'abi'}
            s['n_c'] = set(p.counts)
            s['blocks'] = set(blocks_of(n) for n in p.counts)
            s['per'] = {p.per}
            s['surplus'] = {p.grid - p.n_blocks}
            nz = [c for c, n in enumerate(p.counts) if n]
            if nz:
                gaps = [b - a - 1 for a, b in zip(nz[:-1], nz[1:])]
                s['empty_at'] = set((['first'] if nz[0] > 0 else []) + (['last'] if nz[-1] < self.Nc - 1 else []) +
                                    (['run'] if any(g >= 2 for g in gaps) else []) + (['all_but_one'] if len(nz) == 1 and self.Nc > 2 else []))
                s['listed_at'] = set(c for c in nz if c in (0, 1023, 1024, self.Nc - 1))
            if any(len(blk) == SP_IMGS and len(set(i for i, _ in blk)) == 1 for _, blk in p.blocks):
                s['image'].add('block_of_one')
        else:
            s['P'] = {self.P}
            s['rounds'] = set(attn_unit(0, w)[2] for w in K)
            s['direct'] = set(int(w > SP_MAXW) for w in K)
            if any(len(set(self.lens[self.pairs[p][1]] > SP_MAXW for p in u)) == 2 for u in self.units()):
                s['mixed_wg'] = {1}
            s['listed_at'] = set(c for c in self.listed if c in (0, 1023, 1024, self.Nc - 1))
        return s

    def describe(self):
        if self.kernel == 'scores':
            return "by %s %s chunks %d" % (self.by or 'abi', self.plan.describe(), chunks(self.D))
        K = sorted(set(self.listed_lens))
        return "pairs %d workgroups %d captions listed %d of %d W %s rounds %s chunks %d" % (
            self.P, ceil_div(self.P, SA_WAVES), len(self.listed), self.Nc, K if len(K) <= 8 else "%d..%d" % (K[0], K[-1]),
            sorted(set(attn_unit(0, w)[2] for w in K)), chunks(self.D))

    # ---- inputs and references ----------------------------------------------------------------------------------
    def _make(self, g):
        img = O.l2norm(torch.randn(self.Ni, self.R, self.D, generator=g), -1)
        words = 0.6 * torch.randn(self.n_tok, self.D, generator=g)
        if self.tied:
            i, r, w = self.tied
            if self.xa == 't2i':
                words[w] = 3.0 * img[i, r]
            else:
                img[i, r] = O.l2norm(words[w:w + 1], -1)[0]
        if self.zero:
            (zi, zr), zw = self.zero
            img[zi, zr] = 0.0
            words[zw] = 0.0
        return {'images': img, 'words': words}

    def _gather(self, parts, flip=None, image_of=None, caption_of=None):
        """Per-caption results {c: (attn, sims, score)} -> the case's flat tensors in pair order."""
        attn, sims, score = [], [], []
        for p, (i, c) in enumerate(self.pairs):
            if image_of is not None:
                i = image_of[p]
            if caption_of is not None:
                c = caption_of.get(p, c)
            a, s, sc = parts[c]
            score.append(sc[i])
            if self.kernel == 'attention':
                attn.append((a[i].t() if flip else a[i]).reshape(-1))
                sims.append(s[i])
        out = {'score': torch.stack(score)}
        if self.kernel == 'attention':
            out['attn'], out['row_sim'] = torch.cat(attn), torch.cat(sims)
        return out

    def _rows(self, x, lens, c):
        o = _offsets(lens)[c]
        return x['words'][o:o + lens[c]]

    def oracle_parts(self, x, lens):
        V = x['images']
        if self.kernel == 'attention':
            return {c: oracle_caption(V, self._rows(x, lens, c), self.xa, self.norm, self.agg, self.ls) for c in self.listed}
        # scores: scan_train_cases.oracle on the listed captions, re-packed
        sub = {'images': V, 'words': torch.cat([self._rows(x, lens, c) for c in self.listed], 0)}
        S = T.oracle(sub, self.xa, [lens[c] for c in self.listed], self.norm, self.agg, self.ls)['S']
        return {c: (None, None, S[:, k]) for k, c in enumerate(self.listed)}

    def mirror_parts(self, x, hooks=None):
        """hooks: {caption: keyword arguments of its mirror} (the defects)."""
        V, out = x['images'], {}
        for c in self.listed:
            Ec, kw = self._rows(x, self.lens, c), dict((hooks or {}).get(c, {}))
            if not self.taken(c):                      # ops._scan_long_caption_col: the training path's forward
                fn = T.mirror_t2i if self.xa == 't2i' else T.mirror_i2t
                out[c] = (None, None, fn({'images': V, 'words': Ec}, (self.lens[c],), self.norm, self.agg, self.ls)['S'][:, 0])
            elif self.xa == 't2i':
                out[c] = mirror_caption_t2i(V, Ec, self.norm, self.agg, self.ls, **kw)
            else:
                out[c] = mirror_caption_i2t(V, Ec, self.norm, self.agg, self.ls, direct=self.lens[c] > SP_MAXW, **kw)
        return out

    def evaluate(self, dtype, which='oracle', change=None, hooks=None):
        """{tensor: flat value} of the oracle (after `change`, a function of the input dict and the lengths) or the mirror in `dtype`."""
        x = {k: v.to(dtype).clone() for k, v in self.inputs().items()}
        if which == 'mirror':
            assert change is None
            return self._gather(self.mirror_parts(x, hooks))
        lens = self.lens
        if change is not None:
            x, lens = change(x, lens)
        return self._gather(self.oracle_parts(x, lens))

    def old_bound(self, tensor):
        """What the older tests hold scores and cosines to: 2e-5; the score under Sum scaled as scan_eval_cases.EvalCase.old_bound (x the
        longest listed caption's words under t2i, x 36 under i2t).  The attention weights answer to CAP alone (None): under no_norm and
        clipped the float32 oracle's own softmax of 9 x the raw products is 1.9e-6 off, and 16 x that is above 2e-5."""
        if tensor == 'attn':
            return None
        if tensor != 'score' or self.agg != 'Sum':
            return OLD_BOUND
        return OLD_BOUND * (max(self.listed_lens) if self.xa == 't2i' else SC_R)

    def reference(self):
        """{tensor: (want float64, e32_oracle, e32_mirror, tol, max |mirror float64 - want|)}; computed once and shared."""
        if 'ref' not in self._cache:
            w64, w32 = self.evaluate(torch.float64), self.evaluate(torch.float32)
            m64, m32 = self.evaluate(torch.float64, 'mirror'), self.evaluate(torch.float32, 'mirror')
            out = {}
            for k in TENSORS[self.kernel]:
                want = w64[k]
                eo, em = float((w32[k].double() - want).abs().max()), float((m32[k].double() - want).abs().max())
                tol = FACTOR * max(eo, em, U * float(want.abs().max()))
                tol = FALLBACK.get(self.name, {}).get(k, tol)
                out[k] = (want, eo, em, tol, float((m64[k] - want).abs().max()))
            self._cache['ref'] = out
        return self._cache['ref']

    def defects(self):
        """{letter: {tensor: float64 value with the defect}} for every claimed defect (only tensors that keep their shape)."""
        lens0, off0 = self.lens, self.off
        rows0 = [list(range(o, o + w)) for o, w in zip(off0, lens0)]

        def zero_last_feature(x, lens):
            x['images'][..., -1] = 0.0
            x['words'][..., -1] = 0.0
            return x, lens

        def drop_last_region(x, lens):
            x['images'] = x['images'][:, :-1].clone()
            return x, lens

        def regroup(x, new_rows):
            x['words'] = x['words'][[r for rows in new_rows for r in rows]].clone()
            return x, tuple(len(rows) for rows in new_rows)

        def drop_last_words(x, lens):
            return regroup(x, [r[:-1] if len(r) > 1 else r for r in rows0])

        def repeat_last_words(x, lens):
            return regroup(x, [r + r[-1:] for r in rows0])

        want = {k: v[0] for k, v in self.reference().items()}
        x64 = {k: v.double() for k, v in self.inputs().items()}
        out = {}
        for letter in self.claims:
            if letter in 'abcr':
                change = {'a': zero_last_feature, 'b': drop_last_region, 'c': drop_last_words, 'r': repeat_last_words}[letter]
                res = self.evaluate(torch.float64, change=change)
                out[letter] = {k: v for k, v in res.items() if v.shape == want[k].shape and (letter == 'a' or k == 'score')}
            elif letter in 'nk':
                # every image of every listed caption is in the per-caption results: re-gather
                parts = self.oracle_parts({k: v.clone() for k, v in x64.items()}, lens0)
                if letter == 'n':
                    nb = self._neighbour()
                    img = [self.pairs[nb[p]][0] if self.taken(self.pairs[p][1]) else self.pairs[p][0] for p in range(self.P)]
                    out[letter] = self._gather(parts, image_of=img)
                else:
                    out[letter] = self._gather(parts, caption_of=self._next_caption())
            elif letter in 'go':
                short = [c for c in self.listed if lens0[c] <= SP_MAXW]
                hooks = {}
                if letter == 'g':
                    for prev, c in zip(short[:-1], short[1:]):
                        Hp = (x64['words'][rows0[prev]] @ x64['words'][rows0[prev]].t()).reshape(-1)
                        W = lens0[c]
                        flat = torch.cat([Hp, torch.zeros(max(0, W * W - Hp.numel()), dtype=torch.float64)])[:W * W]
                        hooks[c] = {'cgram': lambda H, f=flat: f.view(H.shape)}
                else:
                    klen = [w if w <= SP_MAXW else 0 for w in lens0]
                    goff = sq_offsets(klen)
                    flat = torch.cat([(x64['words'][rows0[c]] @ x64['words'][rows0[c]].t()).reshape(-1) for c in range(self.Nc) if klen[c]] +
                                     [torch.zeros(SP_MAXW * SP_MAXW, dtype=torch.float64)])
                    for c in short:
                        if c >= PREFIX_THREADS:
                            o, W = goff[c - PREFIX_THREADS], lens0[c]
                            hooks[c] = {'cgram': lambda H, f=flat[o:o + W * W]: f.view(H.shape)}
                out[letter] = self.evaluate(torch.float64, 'mirror', hooks=hooks)
            elif letter == 't':
                def first_for_last(G):
                    G = G.clone()
                    G[-1] = G[0]
                    return G
                out[letter] = self.evaluate(torch.float64, 'mirror', hooks={c: {'gram': first_for_last} for c in self.listed if self.taken(c)})
            elif letter == '2':
                def no_second_pass(a):
                    a = a.clone()
                    a[:, :, 64:] = 0.0
                    return a
                out[letter] = self.evaluate(torch.float64, 'mirror', hooks={c: {'araw': no_second_pass} for c in self.listed if lens0[c] > SP_MAXW})
            elif letter == 'l':
                score, o = want['score'].clone(), 0
                for p, (i, c) in enumerate(self.pairs):
                    W = lens0[c]
                    if W > 64:
                        s = want['row_sim'][o:o + 64].unsqueeze(0)
                        score[p] = (_pair_aggregate(s, self.agg) * (64.0 / W if self.agg == 'Mean' else 1.0))[0]
                    o += W
                out[letter] = {'score': score}
            elif letter == 'T':
                parts = self.oracle_parts({k: v.clone() for k, v in x64.items()}, lens0)
                out[letter] = {'attn': self._gather(parts, flip=True)['attn']}
            else:
                assert letter == 'd'
                out[letter] = {'attn': self.evaluate(torch.float64, 'mirror', hooks={c: {'keep_den': True} for c in self.listed})['attn']}
        return out


# The inputs are seeded from the case's name.  A case whose seed fails a cap takes another seed here; the seam stays.
RESEED = {}


def _add(kernel, group, tag, xa, Ni, D, lens, norm, agg, **kw):
    c = PairCase(kernel, group, tag, xa, Ni, D, lens, norm, agg, **kw)
    if c.name in RESEED:
        c = PairCase(kernel, group, tag, xa, Ni, D, lens, norm, agg, seed=RESEED[c.name], **kw)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(kernel, xa, group=None):
    return [c for c in CASES if c.kernel == kernel and c.xa == xa and (group is None or c.group == group)]


def _seam(kernel, xa, **params):
    SEAMS.setdefault((kernel, xa), {}).update({k: sorted(set(v), key=str) for k, v in params.items()})


_count = {}


def _agg(key):
    """The next aggregation of a (kernel, direction)'s rotation."""
    _count[key] = _count.get(key, 0) + 1
    return AGGS[(_count[key] - 1) % 4]


# ---------------------------------------------------------------------------------------------------------------------
# pair lists
def lists_by_caption(Nc, Ni, K, shift=0):
    """cand [Nc, K] of image indices: list c walks the images from c + shift in steps of 2 (Ni odd: every image, the last one too)."""
    return [[(c + shift + 2 * k) % Ni for k in range(K)] for c in range(Nc)]


def lists_by_image(counts, Ni):
    """cand [Ni, K] of caption indices in which caption c is listed counts[c] times: entry t of the captions' run-length list goes to
    image t % Ni, so a caption's pairs walk the images in turn."""
    flat = [c for c, n in enumerate(counts) for _ in range(n)]
    assert flat and len(flat) % Ni == 0, (len(flat), Ni)
    K = len(flat) // Ni
    return [[flat[k * Ni + i] for k in range(K)] for i in range(Ni)]


def pairs_of_counts(counts, Ni):
    """A caption-major pair list for the direct call: caption c with counts[c] images, walking the images from c."""
    return [((c + j) % Ni, c) for c, n in enumerate(counts) for j in range(n)]


def pairs_round_robin(P, Nc, Ni):
    """An attention list: pair p is (image 4 p + 1 mod Ni, caption p mod Nc) -- neighbours differ in both."""
    return [((4 * p + 1) % Ni, p % Nc) for p in range(P)]


DEFAULT = 'clipped_l2norm'
NI = 9
# one caption on, before and behind every 16-column tile seam, W^2 on either side of the 512 staging threads (22, 23), one and two words
MIXED = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 22, 23)
W_SHORT = MIXED
W_LONG = (65, 79, 80, 81, 95, 96)
MAINLOOP_D = (16, 32, 48, 64, 272)
SMALL = (5, 17, 33, 2, 20, 9, 12, 3)

# every first norm x every aggregation on the mixed set, D = 48 (an odd chunk count): scores through both `by` in turn (three images
# per caption | 45 entries spread 3 per caption), attention on two images per caption and a caption of 80 words
for _xa in DIRECTIONS:
    for _j, (_n, _a) in enumerate((n, a) for n in NORMS for a in AGGS):
        if _j % 2 == 0:
            _add('scores', 'norm', 'mixed', _xa, NI, 48, MIXED, _n, _a, cand=lists_by_caption(len(MIXED), NI, 3, _j), by='caption')
        else:
            _add('scores', 'norm', 'mixed', _xa, NI, 48, MIXED, _n, _a, cand=lists_by_image((3,) * len(MIXED), NI), by='image')
        _add('attention', 'norm', 'mixed', _xa, NI, 48, MIXED + (80,), _n, _a, pairs=pairs_round_robin(2 * (len(MIXED) + 1), len(MIXED) + 1, NI))
    for _k in KERNELS:
        _seam(_k, _xa, **{'norm,agg': [(n, a) for n in NORMS for a in AGGS], 'W': W_SHORT, 'ncb': (1, 2, 3, 4), 'image': ('last',)})
    _seam('attention', _xa, rounds=(1, 2))

# the main loop: D / 16 = 1 (the loop runs once, on its own re-read), 2, 3 (odd), 4, 17
for _xa in DIRECTIONS:
    for _D in MAINLOOP_D:
        _add('scores', 'D', 'mixed', _xa, NI, _D, MIXED, DEFAULT, 'LogSumExp', cand=lists_by_caption(len(MIXED), NI, 2), by='caption')
        _add('attention', 'D', 'mixed', _xa, NI, _D, MIXED + (65, 96), DEFAULT, 'LogSumExp', pairs=pairs_round_robin(len(MIXED) + 2, len(MIXED) + 2, NI))
    for _k in KERNELS:
        _seam(_k, _xa, D=MAINLOOP_D, chunks=(1, 2, 3, 4, 17))

# i2t: the W^2 Gram floats staged by 512 threads: 484 | 529 on either side of one round, 4096 eight rounds
for _k in KERNELS:
    _seam(_k, 'i2t', stage=('<=512', '>512'), **{'W*W': (484, 529, 4096)})

# scores: pairs per caption.  by='caption' gives every caption K pairs (K on 7 | 8 | 9 and 16 | 17: one block, one block and a tail of
# one, two blocks and a tail); 'oneimage' lists the last image in all 8 slots of a block
for _xa in DIRECTIONS:
    for _K in (1, 7, 8, 9, 16, 17):
        _add('scores', 'count', 'K%d' % _K, _xa, NI, 48, SMALL[:4], DEFAULT, _agg(('scores', _xa)), cand=lists_by_caption(4, NI, _K), by='caption')
    _add('scores', 'count', 'oneimage', _xa, NI, 48, SMALL[:3], DEFAULT, _agg(('scores', _xa)),
         cand=[[NI - 1] * 8, [(3 * k) % NI for k in range(8)], [0] * 8], by='caption')
    # by='image': captions listed 0 times first, last, several in a row between two listed ones, and everywhere but one caption
    for _tag, _counts in (('empty.first', (0, 9, 8, 1)), ('empty.last', (7, 10, 1, 0)), ('empty.run', (9, 0, 0, 0, 17, 1)),
                          ('empty.allbutone', (0, 0, 0, 18, 0, 0)), ('empty.16', (16, 0, 2))):
        _add('scores', 'count', _tag, _xa, NI, 48, SMALL[:len(_counts)], DEFAULT, _agg(('scores', _xa)), cand=lists_by_image(_counts, NI), by='image')
    _seam('scores', _xa, n_c=(0, 1, 7, 8, 9, 16, 17), blocks=(0, 1, 2, 3), empty_at=('first', 'last', 'run', 'all_but_one'),
          image=('last', 'block_of_one'), by=('caption', 'image', 'abi'))

# the caption count: Nc = 1 and 2; and 1023 | 1024 | 1025 and 2049 (`per` of the two 1024-thread prefix kernels 1 | 1 | 2 | 3) with
# captions of one to four words and a dozen listed ones spread over the first, the 1024th, the 1025th and the last; Ni = 1 and 9
BIG_NC = (1023, 1024, 1025, 2049)


def big_lens(Nc):
    return [(k * 7 + 2) % 4 + 1 for k in range(Nc)]


def big_listed(Nc):
    return sorted(set(c for c in (0, 1, 5, 511, 512, 1022, 1023, 1024, 1030, 2047, Nc - 2, Nc - 1) if 0 <= c < Nc))


for _xa in DIRECTIONS:
    _add('scores', 'Nc', 'Nc1', _xa, NI, 48, (17,), DEFAULT, _agg(('scores', _xa)), cand=[[8, 0, 4]], by='caption')
    _add('scores', 'Nc', 'Nc1.Ni1', _xa, 1, 48, (33,), DEFAULT, _agg(('scores', _xa)), cand=[[0] * 9], by='image')
    _add('scores', 'Nc', 'Nc2', _xa, NI, 48, (5, 64), DEFAULT, _agg(('scores', _xa)), cand=lists_by_image((17, 1), NI), by='image')
    _add('attention', 'Nc', 'Nc1', _xa, NI, 48, (17,), DEFAULT, _agg(('attention', _xa)), pairs=[(8, 0), (0, 0), (4, 0)])
    _add('attention', 'Nc', 'Nc1.Ni1', _xa, 1, 48, (80,), DEFAULT, _agg(('attention', _xa)), pairs=[(0, 0)])
    _add('attention', 'Nc', 'Nc2', _xa, NI, 48, (5, 64), DEFAULT, _agg(('attention', _xa)), pairs=pairs_round_robin(5, 2, NI))
    for _Nc in BIG_NC:
        _l = big_listed(_Nc)
        _counts = [0] * _Nc
        for _j, _c in enumerate(_l):
            _counts[_c] = (1, 9, 2, 8, 3, 17)[_j % 6]
        _Ni = 1 if _Nc == 1024 else NI
        _counts[_l[-1]] += -sum(_counts) % _Ni
        _add('scores', 'Nc', 'Nc%d' % _Nc, _xa, _Ni, 16, big_lens(_Nc), DEFAULT, 'LogSumExp', cand=lists_by_image(_counts, _Ni), by='image')
        _add('attention', 'Nc', 'Nc%d' % _Nc, _xa, _Ni, 16, big_lens(_Nc), DEFAULT, 'LogSumExp', pairs=[((3 * j) % _Ni, c) for j, c in enumerate(_l)])
    for _k in KERNELS:
        _seam(_k, _xa, Nc=(1, 2) + BIG_NC, Ni=(1, NI), listed_at=(0, 1022, 1023, 1024, 2048))
    _seam('scores', _xa, per=(1, 2, 3))
_seam('attention', 'i2t', per=(1, 2, 3))

# attention: the pair count on 3 | 4 | 5 and 8 | 9 (one workgroup, its tail, two workgroups and a tail) and 1, with captions of more
# and of fewer than 64 words inside one workgroup; and every length of the second main-loop pass
ATT_MIX = (80, 5, 64, 96, 17)
for _xa in DIRECTIONS:
    for _P in (1, 3, 4, 5, 8, 9):
        _add('attention', 'P', 'P%d' % _P, _xa, NI, 48, ATT_MIX, DEFAULT, _agg(('attention', _xa)), pairs=pairs_round_robin(_P, len(ATT_MIX), NI))
    for _n in (DEFAULT, 'softmax', 'no_norm'):
        _add('attention', 'W', 'long', _xa, NI, 48, W_LONG + (64, 5), _n, _agg(('attention', _xa)), pairs=pairs_round_robin(16, len(W_LONG) + 2, NI))
    _seam('attention', _xa, P=(1, 3, 4, 5, 8, 9), mixed_wg=(1,), W=W_SHORT + W_LONG, ncb=(1, 2, 3, 4, 5, 6), direct=(0, 1))

# captions of 65..96 words in the plan of a scores case: the kernel and sq_prefix_kernel see length 0, their pairs go through
# ops._long_caption_pairs.  One at the first, a middle and the last index; a list made of long captions only; both `by`
LONG_SETS = {'first.middle': (65,) + SMALL[:3] + (96,) + SMALL[3:6], 'middle.last': SMALL[:2] + (96,) + SMALL[2:6] + (65,),
             'last.first': (96,) + SMALL[:6] + (65,), 'all': (65, 96, 70)}
for _xa in DIRECTIONS:
    for _j, (_tag, _ls_) in enumerate(LONG_SETS.items()):
        _n = NORMS[(2 * _j) % 7] if _j else DEFAULT
        if _j % 2 == 0:
            _add('scores', 'long', _tag, _xa, NI, 48, _ls_, _n, _agg(('scores', _xa)), cand=lists_by_caption(len(_ls_), NI, 9), by='caption')
        else:
            _add('scores', 'long', _tag, _xa, NI, 48, _ls_, _n, _agg(('scores', _xa)), cand=lists_by_image((3 + -3 * len(_ls_) % NI,) + (3,) * (len(_ls_) - 1), NI), by='image')
    _add('scores', 'long', 'all.image', _xa, NI, 48, LONG_SETS['all'], DEFAULT, _agg(('scores', _xa)), cand=lists_by_image((3, 3, 3), NI), by='image')
    _seam('scores', _xa, long_at=('first', 'middle', 'last'), only_long=(0, 1))

# lambda_softmax = 4, the reference's other setting, once per direction and kernel; an all-zero word inside a caption and an all-zero
# region (the cosine clamp decides); the direct call: caption-major lists no `by` produces (descending slots inside a caption)
ZERO = ((0, 7), 8)
ABI_COUNTS = (0, 9, 0, 0, 17, 8, 1, 0)
for _xa in DIRECTIONS:
    _add('scores', 'ls', 'mixed', _xa, NI, 48, MIXED, DEFAULT, 'LogSumExp', cand=lists_by_caption(len(MIXED), NI, 3), by='caption', ls=4.0)
    _add('attention', 'ls', 'mixed', _xa, NI, 48, MIXED + (80,), DEFAULT, 'LogSumExp', pairs=pairs_round_robin(len(MIXED) + 1, len(MIXED) + 1, NI), ls=4.0)
    for _n in (DEFAULT, 'softmax'):
        _add('scores', 'zero', 'word.region', _xa, NI, 48, (5, 9, 12, 3), _n, 'LogSumExp', cand=lists_by_caption(4, NI, 9), by='caption', zero=ZERO)
        _add('attention', 'zero', 'word.region', _xa, NI, 48, (5, 9, 12, 3), _n, 'LogSumExp', pairs=pairs_round_robin(9, 4, NI), zero=ZERO)
    _add('scores', 'abi', 'reversed', _xa, NI, 48, SMALL, DEFAULT, _agg(('scores', _xa)), pairs=pairs_of_counts(ABI_COUNTS, NI), abi=True)
    _add('attention', 'abi', 'guards', _xa, NI, 48, ATT_MIX, DEFAULT, _agg(('attention', _xa)), pairs=pairs_round_robin(6, len(ATT_MIX), NI), abi=True)
    for _k in KERNELS:
        _seam(_k, _xa, ls=(4.0, 9.0), zero=('none', ZERO), abi=(0, 1))

assert all(k + '-seed%d' % v in _BY_NAME for k, v in RESEED.items())
