"""Case table of the SCAN training similarity kernels (csrc/scan_train.hip: t2i, csrc/scan_train_i2t.hip: i2t, reached through
ag.scan_t2i_scores / ag.scan_i2t_scores) and their float64 references.

One entry per (direction, shape, first norm, aggregation): seeded CPU inputs (l2-normalised regions, words = 0.6 * randn, packed,
gS = randn; lambda_lse = 6 and lambda_softmax = 9, the reference's values), the REFERENCE -- itr_oracle.xattn_score under autograd, in
float64 for S, d_images and d_words of sum(S * gS) and again in float32 for its own rounding error e32_oracle -- and the MIRROR, a
plain-torch function per direction that follows the kernels' algebra (A = V E^T from one matrix product, q through the Gram matrix,
the cosine clamp at 1e-8), run under autograd in float32 for e32_mirror and in float64 to prove that it is the same function as the
oracle.  Shapes sit on both sides of every seam of the launch code (SEAMS lists them); the host-side routing is mirrored below, each
function marked with the source lines it copies, and tests/test_scan_train_case_table.py pins the constants to the source text.

Tolerance of a compared tensor (tests/test_scan_train_seams_gpu.py applies it, tests/test_scan_train_case_table.py proves that it
sees every claimed defect at SENSITIVITY x):
    tol = 16 * max(e32_oracle, e32_mirror, u * max|want|),  u = 2^-24              (FACTOR, U: tests/helpers/train_prim_cases.py)
e32_mirror is there because the kernels take q = p^T G p from the Gram matrix, which rounds differently from the oracle's
||sum_r p_r v_r||; both terms come from reference code, neither from the code under test.  Conditioning cap: every compared tensor
has tol <= 2^-10 max|want|, so a loose bound cannot hide a wrong kernel.  D = 1 is the one exception and only for the gradients: the
cosine of two collinear vectors is the constant +-1, so d_images and d_words are zero in exact arithmetic (CAP_EXEMPT_D); they are
still compared under tol, but no cap and no gradient defect can be claimed for them, and S, a pattern of +-1, moves under defect a
only (the D = 1 cases are there for the zero-filled slice of caption_gram_kernel and the lane loops, which S and defect a see).

Defects, all float64 and all computed by the oracle on changed inputs (Case.claims says which a case claims):
    a  the last feature of images and words zeroed            -> S
    b  the last region dropped (R > 1)                        -> S
    c  the last word of every caption of more than one word dropped -> S
    d  the last column of gS zeroed (Bc > 1)                  -> d_images
    e  the last row of gS zeroed (Bi > 1)                     -> d_words
Under Max, b (i2t) and c (t2i) are decisive only if the dropped element carries the maximum: every Max case ties the last region
of image 0 to the last word of the first caption of more than one word (t2i: the word is 3 x that region; i2t: the region is that
word's direction), which puts the maximum of that pair there.
Nothing here imports the library: the table is checked on a machine without a GPU."""
import torch

import itr_oracle as O
from train_prim_cases import Case, U, FACTOR, SENSITIVITY        # noqa: F401  (re-exported)

NORMS = ('clipped_l2norm', 'l2norm', 'no_norm', 'clipped', 'softmax', 'l1norm', 'clipped_l1norm')     # as tests/test_train_gpu.py: NORMS
AGGS = ('LogSumExp', 'Mean', 'Sum', 'Max')
LAMBDA_LSE, LAMBDA_SOFTMAX = 6.0, 9.0
CAP = 2.0 ** -10
MIRROR_AGREES = 1e-11
CAP_EXEMPT_D = 1              # see the module docstring
FALLBACK_SHARE = 0.02

# geometry of the kernels (pinned to csrc/ by tests/test_scan_train_case_table.py)
ST_RMAX, ST_MAXW = 100, 96                  # scan_train_pair.h:26-27 (both directions)
SC_R = 36                                   # scan_common.h:7
GRAM_MFMA_RMAX = 48                         # scan_train.hip:224
DG_UNROLL = 16                              # scan_train.hip:128
CGRAM_SLICE = 32                            # scan_train_i2t.hip:124
NTP_ROUND = 32                              # autograd.py: _scan_pair_dots (_ScanT2I.forward and _ScanI2T.forward)

SEAMS = {}          # direction -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule and that are judged by a derived a-priori bound instead:
# name -> {tensor: bound}, the derivation in a comment next to the entry.  No case needs it (profiles/scan_train_seams/measured.txt).
FALLBACK = {}


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the host-side routing
def t2i_pair_route(R, max_len, backward):
    """scan_train_pair.h:251-252 (check_train_args), scan_train.hip:246-257 (itr_scan_train_fwd), :268-279 (itr_scan_train_bwd): the
    pair kernel's instantiation (MAXW, RMAX, FIXED), or 'rejected'."""
    if R < 1 or R > ST_RMAX or max_len > ST_MAXW:
        return 'rejected'
    if backward and R > SC_R and max_len > 64:
        return 'rejected'
    if R == SC_R and max_len <= 32:
        return (32, SC_R, True)
    maxw = 64 if max_len <= 64 else ST_MAXW
    if R == SC_R:
        return (maxw, SC_R, True)
    if R < SC_R:
        return (maxw, SC_R, False)
    return (maxw, ST_RMAX, False)


def i2t_pair_route(R, max_len=1):
    """scan_train_pair.h:251-252 (check_train_args), scan_train_i2t.hip:177-179 (itr_scan_train_i2t_fwd), :193-195
    (itr_scan_train_i2t_bwd): (RMAX, FIXED), forward and backward alike, or 'rejected'."""
    if R < 1 or R > ST_RMAX or max_len > ST_MAXW:
        return 'rejected'
    if R == SC_R:
        return (SC_R, True)
    return (SC_R, False) if R < SC_R else (ST_RMAX, False)


def gram_route(R, D, aligned):
    """scan_train.hip:224-230 (itr_scan_train_prepare): the kernel that computes G = V V^T."""
    if R <= GRAM_MFMA_RMAX and D % 4 == 0 and aligned:
        return 'mfma'
    return 'gram36' if R == SC_R else 'train_gram'


def dg_reduce_blocks(R):
    """scan_train.hip:290 (itr_scan_train_finish): workgroups per image of scan_train_dg_reduce_kernel."""
    return ceil_div(R * R, 256)


def ntp(n_tok):
    """autograd.py: _scan_pair_dots (_ScanT2I.forward and _ScanI2T.forward): the padded word count."""
    return (n_tok + NTP_ROUND - 1) // NTP_ROUND * NTP_ROUND


# ---------------------------------------------------------------------------------------------------------------------
# the oracle and the mirrors, dtype-generic
def _offsets(lens):
    off, o = [], 0
    for w in lens:
        off.append(o)
        o += w
    return off


def oracle(x, xa, lens, norm, agg, lambda_softmax=LAMBDA_SOFTMAX):
    """itr_oracle.xattn_score on the packed words (padded per caption; the oracle reads captions[c, :len] only)."""
    words, L = x['words'], max(lens)
    cap = torch.stack([torch.nn.functional.pad(words[o:o + w], (0, 0, 0, L - w)) for o, w in zip(_offsets(lens), lens)], 0)
    return {'S': O.xattn_score(x['images'], cap, list(lens), xa, norm, agg, LAMBDA_LSE, lambda_softmax)}


def _first_norm(a, norm, dim):
    """scan_train_pair.h:66-88 (pair_forward, both directions): b = leaky(a) | a; u = b / (||b|| + eps) | b / (sum |b| + eps) | softmax(a) | b."""
    b = torch.where(a > 0, a, 0.1 * a) if norm in ('clipped_l2norm', 'clipped', 'clipped_l1norm') else a
    if norm in ('clipped_l2norm', 'l2norm'):
        return b / ((b * b).sum(dim, keepdim=True).sqrt() + 1e-8)
    if norm in ('l1norm', 'clipped_l1norm'):
        return b / (b.abs().sum(dim, keepdim=True) + 1e-8)
    if norm == 'softmax':
        return torch.softmax(a, dim)
    assert norm in ('clipped', 'no_norm'), norm
    return b


def _aggregate(s, agg):
    """scan_train_pair.h:137-154 (pair_aggregate, both directions; the LSE with its maximum taken out first)."""
    if agg == 'LogSumExp':
        return torch.logsumexp(s * LAMBDA_LSE, 1) / LAMBDA_LSE
    if agg == 'Max':
        return s.max(1)[0]
    return s.sum(1) if agg == 'Sum' else s.mean(1)


def mirror_t2i(x, lens, norm, agg, lambda_softmax=LAMBDA_SOFTMAX):
    """scan_train.hip:5-14 (header), :73-79 (t2i_pair_forward) and scan_train_pair.h:63-134 (pair_forward with context = regions,
    query = words): A = V E^T for all pairs from one product, G_i = V_i V_i^T, ||e_w||; per pair u = first norm over the caption's
    words per region, p = softmax_r(lambda_s u), num_w = sum_r p a, q_w = p^T G p (clamped at 0, scan_train_pair.h:129),
    s_w = num_w / max(||e_w|| sqrt(q_w), 1e-8) (:131)."""
    V, E = x['images'], x['words']
    Bi, R, D = V.shape
    A = (V.reshape(Bi * R, D) @ E.t()).view(Bi, R, -1)               # autograd.py: _scan_pair_dots: A = _gemm_nt(V2, Ep)
    G = V @ V.transpose(1, 2)                                          # scan_train.hip:224-230
    enorm = (E * E).sum(1).sqrt()                                      # scan_train.hip:180-188 (rownorm_train_kernel)
    cols = []
    for o, W in zip(_offsets(lens), lens):
        a = A[:, :, o:o + W]
        p = torch.softmax(lambda_softmax * _first_norm(a, norm, 2), 1)
        num = (p * a).sum(1)
        q = (p * (G @ p)).sum(1).clamp_min(0.0)
        s = num / (enorm[o:o + W] * q.sqrt()).clamp_min(1e-8)
        cols.append(_aggregate(s, agg))
    return {'S': torch.stack(cols, 1)}


def mirror_i2t(x, lens, norm, agg, lambda_softmax=LAMBDA_SOFTMAX):
    """scan_train_i2t.hip:3-9 (header), :52-59 (i2t_pair_forward) and scan_train_pair.h:63-134 (pair_forward with context = words,
    query = regions): A = V E^T, H_c = E_c E_c^T, ||v_r||; per pair u = first norm over the regions per word,
    p = softmax_w(lambda_s u), num_r = sum_w p a, q_r = p_r^T H_c p_r (clamped at 0, scan_train_pair.h:129),
    s_r = num_r / max(||v_r|| sqrt(q_r), 1e-8) (:131)."""
    V, E = x['images'], x['words']
    Bi, R, D = V.shape
    A = (V.reshape(Bi * R, D) @ E.t()).view(Bi, R, -1)               # autograd.py: _scan_pair_dots
    vnorm = (V * V).sum(2).sqrt()                                      # scan_train.hip:180-188 (rownorm_train_kernel)
    cols = []
    for o, W in zip(_offsets(lens), lens):
        Ec = E[o:o + W]
        H = Ec @ Ec.t()                                                # scan_train_i2t.hip:113-149
        a = A[:, :, o:o + W]
        p = torch.softmax(lambda_softmax * _first_norm(a, norm, 1), 2)
        num = (p * a).sum(2)
        q = (p * (p @ H)).sum(2).clamp_min(0.0)
        s = num / (vnorm * q.sqrt()).clamp_min(1e-8)
        cols.append(_aggregate(s, agg))
    return {'S': torch.stack(cols, 1)}


# ---------------------------------------------------------------------------------------------------------------------
class ScanCase(Case):
    """train_prim_cases.Case with two references (oracle and mirror) and the oracle's defects."""

    def __init__(self, group, xa, Bi, R, D, lens, norm, agg, unaligned=False, seed=0):
        self.group, self.xa, self.Bi, self.R, self.D, self.lens = group, xa, Bi, R, D, tuple(int(w) for w in lens)
        self.norm, self.agg, self.unaligned = norm, agg, bool(unaligned)
        assert all(w >= 1 for w in self.lens)
        self.Bc, self.max_len, self.n_tok = len(self.lens), max(self.lens), sum(self.lens)
        if xa == 't2i':
            self.fwd_route, self.bwd_route = t2i_pair_route(R, self.max_len, False), t2i_pair_route(R, self.max_len, True)
        else:
            self.fwd_route = self.bwd_route = i2t_pair_route(R, self.max_len)
        assert self.fwd_route != 'rejected'
        self.backward = self.bwd_route != 'rejected'
        shape = {'Bi': Bi, 'R': R, 'D': D, 'lens': ".".join(str(w) for w in self.lens) if self.Bc <= 4 else
                 "%dcaptions.%dwords.longest%d" % (self.Bc, self.n_tok, self.max_len)}
        Case.__init__(self, xa, shape, self._make, lambda x: oracle(x, xa, self.lens, norm, agg),
                      grads=('images', 'words') if self.backward else ())
        self.name = "%s-%s-%s-%s-%s%s%s" % (xa, group, self.name[len(xa) + 1:], norm, agg, "-unaligned" if self.unaligned else "",
                                            "-seed%d" % seed if seed else "")
        self.mirror = (lambda x: mirror_t2i(x, self.lens, norm, agg)) if xa == 't2i' else (lambda x: mirror_i2t(x, self.lens, norm, agg))

    # ---- what the case covers -------------------------------------------------------------------------------------
    @property
    def tied(self):
        """(region row of image 0, word row) that a Max case ties together, else None."""
        if self.agg != 'Max':
            return None
        c = next((k for k, w in enumerate(self.lens) if w > 1), 0)
        return self.R - 1, _offsets(self.lens)[c] + self.lens[c] - 1

    @property
    def claims(self):
        """The defects this case claims to see (module docstring)."""
        out = 'a'
        if self.D <= CAP_EXEMPT_D:          # S is a sign pattern: only the zeroed feature moves it
            return out
        if self.R > 1:
            out += 'b'
        if self.max_len > 1:
            out += 'c'
        if self.backward:
            out += ('d' if self.Bc > 1 else '') + ('e' if self.Bi > 1 else '')
        return out

    def capped(self, tensor):
        return tensor == 'S' or self.D > CAP_EXEMPT_D

    def seams(self):
        """{parameter: set of values} this case puts into the coverage of SEAMS[direction]."""
        s = {'R': {self.R}, 'D': {self.D}, 'Bc': {self.Bc}, 'Bi': {self.Bi}, 'n_tok': {self.n_tok}, 'unaligned': {int(self.unaligned)},
             'n_tok%4': {self.n_tok % 4}, 'Bi*R%4': {self.Bi * self.R % 4}, 'fwd_route': {self.fwd_route}, 'bwd_route': {self.bwd_route},
             'ntp': {ntp(self.n_tok)}}
        if self.xa == 't2i':
            where = 'R=36' if self.R == SC_R else ('R<36' if self.R < SC_R else ('R>36,backward' if self.backward else 'R>36,forward only'))
            s['max_len@' + where] = {self.max_len}
            s['R*W'] = set('<256' if self.R * w < 256 else ('=256' if self.R * w == 256 else '>256') for w in self.lens)
            s['gram_route'] = {gram_route(self.R, self.D, not self.unaligned)}
            s['gram_route@R,D%4,aligned'] = {(self.R, int(self.D % 4 == 0), int(not self.unaligned))}
            s['dg_reduce_blocks'] = {dg_reduce_blocks(self.R)}
            s['R*R'] = {self.R * self.R}
        else:
            s['W'] = set(self.lens)
            s['W*W'] = set(w * w for w in self.lens)
            s['R,W'] = set((self.R, w) for w in self.lens)
        return s

    # ---- inputs and references ----------------------------------------------------------------------------------
    def _make(self, g):
        img = O.l2norm(torch.randn(self.Bi, self.R, self.D, generator=g), -1)
        words = 0.6 * torch.randn(self.n_tok, self.D, generator=g)
        gS = torch.randn(self.Bi, self.Bc, generator=g)
        if self.tied:
            r, w = self.tied
            if self.xa == 't2i':
                words[w] = 3.0 * img[0, r]
            else:
                img[0, r] = O.l2norm(words[w:w + 1], -1)[0]
        return {'images': img, 'words': words, 'g_S': gS}

    def evaluate(self, dtype, fn=None, change=None, grads=None):
        """{tensor: value} of `fn` (default: the oracle) in `dtype` on the inputs (after `change`, a function of the float64 / float32
        input dict): S and, for a case with a backward, d_images and d_words of sum(S * gS)."""
        x = {k: v.to(dtype).clone() for k, v in self.inputs().items()}
        lens = self.lens
        if change is not None:
            x, lens = change(x, lens)
        grads = self.grads if grads is None else grads
        for k in grads:
            x[k].requires_grad_(True)
        if fn is None:
            out = oracle(x, self.xa, lens, self.norm, self.agg)
        else:
            assert change is None
            out = fn(x)
        res = {'S': out['S'].detach()}
        if grads:
            for k, gr in zip(grads, torch.autograd.grad((out['S'] * x['g_S']).sum(), [x[k] for k in grads])):
                res['d_' + k] = gr
        return res

    def reference(self):
        """{tensor: (want float64, e32_oracle, e32_mirror, tol, mirror float64 - want)}; computed once and shared."""
        if 'ref' in self._cache:
            return self._cache['ref']
        w64, w32 = self.evaluate(torch.float64), self.evaluate(torch.float32)
        m64, m32 = self.evaluate(torch.float64, self.mirror), self.evaluate(torch.float32, self.mirror)
        out = {}
        for k, want in w64.items():
            eo, em = float((w32[k].double() - want).abs().max()), float((m32[k].double() - want).abs().max())
            tol = FACTOR * max(eo, em, U * float(want.abs().max()))
            if self.name in FALLBACK and k in FALLBACK[self.name]:
                tol = FALLBACK[self.name][k]
            out[k] = (want, eo, em, tol, float((m64[k] - want).abs().max()))
        self._cache['ref'] = out
        return out

    def defects(self):
        """{letter: (tensor, float64 value of the oracle on the changed inputs)} for every claimed defect."""
        def zero_last_feature(x, lens):
            x['images'][..., -1] = 0.0
            x['words'][..., -1] = 0.0
            return x, lens

        def drop_last_region(x, lens):
            x['images'] = x['images'][:, :-1].clone()
            return x, lens

        def drop_last_words(x, lens):
            keep, o = [], 0
            for w in lens:
                keep += list(range(o, o + (w - 1 if w > 1 else w)))
                o += w
            x['words'] = x['words'][keep].clone()
            return x, tuple(w - 1 if w > 1 else w for w in lens)

        def zero_last_column(x, lens):
            x['g_S'][:, -1] = 0.0
            return x, lens

        def zero_last_row(x, lens):
            x['g_S'][-1] = 0.0
            return x, lens

        how = {'a': ('S', zero_last_feature, ()), 'b': ('S', drop_last_region, ()), 'c': ('S', drop_last_words, ()),
               'd': ('d_images', zero_last_column, ('images',)), 'e': ('d_words', zero_last_row, ('words',))}
        out = {}
        for letter in self.claims:
            tensor, change, grads = how[letter]
            out[letter] = (tensor, self.evaluate(torch.float64, change=change, grads=grads)[tensor])
        return out


# The inputs are seeded from the case's name.  A case whose seed fails the conditioning cap, or comes within a quarter of it (a region
# whose product with a one-word caption is nearly zero makes the l2 norm's derivative there a difference of close numbers), takes
# another seed here; the seam stays.  (First seeds: 1.44, 0.84 and 0.79 of the cap; now at most 0.43 over the whole table.)
RESEED = {'t2i-pair-Bi2-R36-D18-lens2.33.1-clipped_l2norm-Mean': 2, 't2i-pair-Bi2-R36-D24-lens1.1.1-clipped_l2norm-LogSumExp': 3,
          't2i-pair-Bi2-R35-D18-lens2.96.1-l2norm-Mean': 2}


def _add(group, xa, Bi, R, D, lens, norm, agg, unaligned=False):
    c = ScanCase(group, xa, Bi, R, D, lens, norm, agg, unaligned)
    if c.name in RESEED:
        c = ScanCase(group, xa, Bi, R, D, lens, norm, agg, unaligned, seed=RESEED[c.name])
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(xa, group=None):
    return [c for c in CASES if c.xa == xa and (group is None or c.group == group)]


def _seam(xa, **params):
    SEAMS.setdefault(xa, {}).update({k: sorted(set(v), key=str) for k, v in params.items()})


def _lens(max_len):
    """A caption of max_len words between captions of 2 and 1 words (not sorted)."""
    return (2, max_len, 1) if max_len > 2 else ((1, 2, 1) if max_len == 2 else (1, 1, 1))


_count = {'t2i': 0, 'i2t': 0}


def _rot(xa):
    """The next (norm, agg) of a direction's rotation, in which every norm meets every aggregation (7 and 4 are coprime)."""
    n = _count[xa]
    _count[xa] += 1
    return NORMS[n % 7], AGGS[n % 4]


# ---------------------------------------------------------------------------------------------------------------------
# t2i pair kernels: every instantiation x every first norm (the aggregations rotate), (R, max_len) on both sides of the gates
# 32|33 (R == 36 only), 64|65, 96 and of R < 36 | == 36 | > 36; D alternates between the matrix-core Gram route (D % 4 == 0) and
# the others.  (96, 100, False) exists as a forward only: the backward of those cases is rejected.
T2I_ROUTES = {
    (32, SC_R, True): ((36, 1), (36, 32), (36, 5), (36, 32), (36, 2), (36, 17), (36, 31)),
    (64, SC_R, True): ((36, 33), (36, 64), (36, 48), (36, 33), (36, 64), (36, 63), (36, 34)),
    (ST_MAXW, SC_R, True): ((36, 65), (36, 96), (36, 80), (36, 65), (36, 96), (36, 95), (36, 66)),
    (64, SC_R, False): ((1, 64), (16, 12), (17, 64), (35, 33), (1, 3), (35, 64), (16, 64)),
    (ST_MAXW, SC_R, False): ((1, 65), (35, 96), (16, 65), (17, 96), (35, 65), (1, 96), (17, 65)),
    (64, ST_RMAX, False): ((37, 64), (48, 7), (49, 64), (100, 64), (37, 5), (100, 33), (48, 64)),
    (ST_MAXW, ST_RMAX, False): ((37, 65), (100, 96), (48, 65), (49, 96), (100, 65), (37, 96), (49, 65)),
}
for _i, (_route, _shapes) in enumerate(T2I_ROUTES.items()):
    for _j, (_R, _W) in enumerate(_shapes):
        assert t2i_pair_route(_R, _W, False) == _route
        _add('pair', 't2i', 2, _R, (24, 18)[(_i + _j) % 2], _lens(_W), NORMS[_j], AGGS[(_i + _j) % 4])
_seam('t2i', R=(1, 16, 17, 35, 36, 37, 48, 49, 100),
      **{'max_len@R=36': (1, 32, 33, 64, 65, 96), 'max_len@R<36': (64, 65, 96), 'max_len@R>36,backward': (64,),
         'max_len@R>36,forward only': (65, 96), 'fwd_route': list(T2I_ROUTES), 'bwd_route': [r for r in T2I_ROUTES if r != (ST_MAXW, ST_RMAX, False)] +
         ['rejected']})

# R * W on both sides of one 256-thread pass over the pair's block (16 x 16, 32 x 8)
for _R, _Ws in ((16, (15, 16, 17)), (32, (7, 8, 9))):
    for _ in range(2):
        _add('block', 't2i', 2, _R, 20, _Ws, *_rot('t2i'))
_seam('t2i', **{'R*W': ('<256', '=256', '>256')})

# i2t pair kernels: every instantiation x every first norm; W on both sides of the caption Gram's 256-pair pass (16 | 17) and of
# 64 | 65, and 96; R = 100 with W = 96 fills the largest LDS block, forward and backward
I2T_ROUTES = {
    (SC_R, True): ((36, 1), (36, 2), (36, 16), (36, 17), (36, 64), (36, 65), (36, 96)),
    (SC_R, False): ((1, 96), (35, 1), (1, 2), (35, 16), (16, 17), (35, 64), (1, 65)),
    (ST_RMAX, False): ((37, 1), (100, 96), (37, 2), (100, 16), (49, 17), (37, 64), (100, 65)),
}
for _i, (_route, _shapes) in enumerate(I2T_ROUTES.items()):
    for _j, (_R, _W) in enumerate(_shapes):
        assert i2t_pair_route(_R, _W) == _route
        _add('pair', 'i2t', 2, _R, (24, 18)[(_i + _j) % 2], _lens(_W), NORMS[_j], AGGS[(_i + _j) % 4])
_seam('i2t', R=(1, 35, 36, 37, 100), W=(1, 2, 16, 17, 64, 65, 96), fwd_route=list(I2T_ROUTES), bwd_route=list(I2T_ROUTES),
      **{'R,W': ((100, 96),), 'W*W': (256, 289)})

# the feature axis: 32-wide slices of caption_gram_kernel (zero-filled tail), the rownorm kernel's lane stride of 64, the 256-wide
# grids of scan_train_gram_bwd_kernel / rownorm_bwd_kernel (both directions) and i2t_gram_bwd_kernel's stride of 256; the three
# region classes of the Gram backward at D > 256; Bi <= 2
SCAN_D = (1, 31, 32, 33, 62, 63, 64, 65, 255, 256, 257, 513)
for _xa, _ls in (('t2i', (3, 1, 6)), ('i2t', (17, 16, 2))):
    for _j, _D in enumerate(SCAN_D):
        _add('D', _xa, 2, (36, 5, 37)[_j % 3], _D, _ls, *_rot(_xa))
    for _D in (257, 513):
        for _R in (36, 5, 37):
            if not any(c.D == _D and c.R == _R for c in cases(_xa, 'D')):
                _add('D', _xa, 1 if _R == 5 else 2, _R, _D, _ls, *_rot(_xa))
    _seam(_xa, D=SCAN_D)

# captions per batch: the 16-way unrolled sum of scan_train_dg_reduce_kernel with its scalar tail (t2i; R = 16 | 17: one | two
# workgroups per image), the column sums over captions / images of the i2t partials
SCAN_BC = (1, 15, 16, 17, 33)
for _Bc in SCAN_BC:
    _ls = [(k * 7 + 2) % 4 + 1 for k in range(_Bc)]
    for _R in (16, 17):
        _add('Bc', 't2i', 2, _R, 12, _ls, *_rot('t2i'))
    _add('Bc', 'i2t', 2, 5, 12, _ls, *_rot('i2t'))
_seam('t2i', Bc=SCAN_BC, dg_reduce_blocks=(1, 2), **{'R*R': (256, 289)})
_seam('i2t', Bc=SCAN_BC)

# images per batch; region rows Bi * R that are no multiple of the rownorm kernel's four rows per workgroup (i2t)
SCAN_BI = (1, 2, 5)
for _Bi in SCAN_BI:
    _add('Bi', 't2i', _Bi, 36, 20, (3, 1, 4), *_rot('t2i'))
    _add('Bi', 'i2t', _Bi, 35, 20, (3, 1, 4), *_rot('i2t'))
_seam('t2i', Bi=SCAN_BI)
_seam('i2t', Bi=SCAN_BI, **{'Bi*R%4': (2, 3)})

# the padded word axis: n_tok on both sides of a multiple of 32
SCAN_NTOK = {31: (10, 1, 20), 32: (10, 2, 20), 33: (11, 2, 20)}
for _n, _ls in SCAN_NTOK.items():
    _add('n_tok', 't2i', 2, 36, 16, _ls, *_rot('t2i'))
    _add('n_tok', 'i2t', 2, 5, 16, _ls, *_rot('i2t'))
for _xa in ('t2i', 'i2t'):
    _seam(_xa, n_tok=list(SCAN_NTOK), ntp=(32, 64), **{'n_tok%4': (1, 3)})

# the three Gram routes of itr_scan_train_prepare: matrix cores (R <= 48, D % 4 == 0, 16-byte aligned), the evaluation's gram_kernel
# (R == 36 otherwise), scan_train_gram_kernel (the rest); unaligned = a contiguous view one float into its buffer
GRAM_CASES = ((36, 16, 0), (36, 18, 0), (36, 16, 1), (48, 16, 0), (49, 16, 0), (48, 18, 0), (48, 16, 1), (1, 16, 0), (100, 16, 1), (36, 18, 1))
for _R, _D, _u in GRAM_CASES:
    _add('gram', 't2i', 2, _R, _D, (4, 1, 2), *_rot('t2i'), unaligned=bool(_u))
_add('gram', 't2i', 5, 36, 32, (4, 1, 2), *_rot('t2i'), unaligned=True)           # 180 region rows: the GEMMs leave the <= 128-row routes
_add('gram', 'i2t', 2, 36, 16, (4, 1, 2), *_rot('i2t'), unaligned=True)
_add('gram', 'i2t', 2, 5, 17, (4, 1, 2), *_rot('i2t'), unaligned=True)
_add('gram', 'i2t', 5, 37, 32, (4, 1, 2), *_rot('i2t'), unaligned=True)
_seam('t2i', gram_route=('mfma', 'gram36', 'train_gram'), unaligned=(0, 1),
      **{'gram_route@R,D%4,aligned': ((36, 1, 1), (36, 0, 1), (36, 1, 0), (48, 1, 1), (49, 1, 1), (48, 0, 1), (48, 1, 0))})
_seam('i2t', unaligned=(0, 1))

DIRECTIONS = ('t2i', 'i2t')
assert all(k + '-seed%d' % v in _BY_NAME for k, v in RESEED.items())
