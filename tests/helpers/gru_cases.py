"""Case table of the text GRU kernels -- training (csrc/gru_train.hip through ag.gru_sequence) and evaluation (csrc/towers.hip through
ops.gru_encode) -- and their float64 reference.

One entry per (lengths, D, E, direction, token kind): seeded CPU inputs (packed token ids, the embedding table and the nn.GRU-named
weights at the reference's initial scales: embed ~ U(-0.1, 0.1), weights and biases ~ U(-1 / sqrt(D), 1 / sqrt(D)); g_out = randn)
and the REFERENCE, the GRU written with plain torch ops on the packed layout (gate order r, z, n; h' = (1 - z) n + z h; a bi-GRU's
output is (fwd + bwd) / 2), run under autograd in float64 for out, d_embed and every weight and bias gradient of sum(out * g_out), and
again in float32 for its own rounding error e32.  torch.nn.GRU is not used: the defects below need a hook inside the recurrence.

The per-step recurrence products change kernel with D and with the ACTIVE PREFIX n_act of the step (captions are sorted by length,
descending; the captions alive at step t are the prefix [0, n_act)).  The host-side planning is mirrored below (splitk_choice,
gru_step_routes; gemm_cases.skinny_ok / skinny_plan / nt_kernel are reused), each function marked with the source lines it copies;
tests/test_gru_case_table.py pins them to the source text.  Every case carries the routes it reaches (fwd_routes, bwd_routes):
    direct_fast | direct_aligned | direct_scalar     one slice: the 128 x 128 tile kernel (persistent, float4 or scalar loader) adds b_hh itself
    tile_aligned | tile_scalar                        K slices of the tile kernel, summed by the gate kernels
    skinny16 | skinny32 | skinny64                    K slices of the skinny kernel (n_act <= 128, K % 4 == 0), summed by the gate kernels

Tolerance of a compared tensor (tests/test_gru_seams_gpu.py applies it, tests/test_gru_case_table.py proves that it is tight and that
it sees every defect):
    primary    tol = 16 * max(e32, u * max|want|),  u = 2^-24                          (FACTOR, U: tests/helpers/train_prim_cases.py)
    fallback   tol = 16 * max(e32, e32_mirror, u * max|want|)  for the cases named in FALLBACK: e32_mirror is the error of the same
               float32 reference with the recurrence products summed in the kernels' slices (gru_step_routes gives them)
    condition  tol <= 2^-12 * max|want| for every tensor of every case (CAP)

Defects, all float64 (Case.claims says which a case claims; each is what a plausible kernel bug would compute):
    a   the last hidden unit j = D - 1 is left out of the recurrence product (Lmax > 1)
    bf  the last K slice of the planned split is left out of every sliced forward product
    bb  the last K slice of the planned split is left out of every sliced BPTT product (the forward is right)
    c   the last active caption of every step keeps its old state
    d   the carry's product share from step t + 1 is not added for row prev_n - 1, at the steps where the prefix grows
    e   the last token row's contribution to d_embed is dropped
    f   the reverse direction is missing from the average (bi)
Nothing here imports the library: the table is checked on a machine without a GPU."""
import zlib

import torch

from gemm_cases import BK, BM, BN, ceil_div, nt_kernel, skinny_ok, skinny_plan
from train_prim_cases import U, FACTOR, SENSITIVITY        # noqa: F401  (re-exported)

CAP = 2.0 ** -12
SPLITK_MIN_K, SPLITK_TARGET, SPLITK_MAX, SPLITK_MIN_SLICE = 256, 256, 16, 128        # gemm_f32.hip:373-379 (gemm_splitk_choice)
PARTIALS_MAX_SLICES = 16                    # gemm_f32.hip:449 (the scratch of gru_train_ws holds 16 slices of B x 3D)
GATE_BLOCK = 256                            # gru_train.hip: both gate kernels launch ceil(D / 256) column blocks
TRANSPOSE_TILE = 64                         # gru_train.hip: transpose_kernel
GATHER_THREADS = 128                        # gru_train.hip: embed_gather_train_kernel strides E by 128 threads

FWD_ROUTES = ('direct_fast', 'direct_aligned', 'direct_scalar', 'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32', 'skinny64')
BWD_ROUTES = ('direct_fast', 'direct_aligned', 'direct_scalar', 'tile_scalar', 'tile_aligned', 'skinny16', 'skinny32')
WEIGHTS = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
TOKEN_KINDS = ('random', 'repeated', 'dense')
DEFECTS = ('a', 'bf', 'bb', 'c', 'd', 'e', 'f')

SEAMS = {}          # parameter -> values that must appear in the table, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose measured error exceeds the primary rule because the kernels sum the recurrence products in slice order: they add the
# e32_mirror term (module docstring).  No case needs it (profiles/gru_seams/measured.txt).
FALLBACK = set()


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the host-side planning
def splitk_choice(M, N, K):
    """gemm_f32.hip:373-379 (gemm_splitk_choice)."""
    tiles = ceil_div(M, BM) * ceil_div(N, BN)
    if tiles >= 128 or K < SPLITK_MIN_K:
        return 1
    s = SPLITK_TARGET // tiles
    while s > 1 and K // s < SPLITK_MIN_SLICE:
        s -= 1
    return 1 if s < 1 else min(s, SPLITK_MAX)


def product_route(splits, M, N, K):
    """gru_train.hip:246-247 and :319-322 (which entry a step calls), gemm_f32.hip:441-463 (gemm_nt_splitk_partials) and :393-399
    (gemm_nt_splitk with one slice): (route, slices, k per slice) of one recurrence product of M active rows.  Both operands are
    dense rows of K floats in 16-byte aligned buffers."""
    if splits <= 1:
        return 'direct_' + nt_kernel(M, N, K, K, K), 1, K
    if skinny_ok(M, N, K, K, K):
        nc, kslice, ns, _ = skinny_plan(M, N, K, PARTIALS_MAX_SLICES)
        return 'skinny%d' % (16 * nc), ns, kslice
    ksplit = ceil_div(ceil_div(K, splits), BK) * BK
    return 'tile_' + ('aligned' if K % 4 == 0 else 'scalar'), ceil_div(K, ksplit), ksplit


def prefixes(lens):
    """n_act of every time step."""
    return [sum(1 for w in lens if w > t) for t in range(max(lens))]


def gru_step_routes(case):
    """{'fwd': [(t, n_act, route, slices, k per slice)] for t = 0 .. Lmax - 1 (h W_hh^T: N = 3D, K = D; gru_train.hip:223, :243-247),
    'bwd': the same for t = Lmax - 1 .. 1 in the order the BPTT runs them (dgh W_hh: N = D, K = 3D; gru_train.hip:284, :310-322)}.
    The two directions of a bi-GRU have the same prefix at every step, so the list holds for each of them."""
    B, D, n = case.B, case.D, prefixes(case.lens)
    sh, sc = splitk_choice(B, 3 * D, D), splitk_choice(B, D, 3 * D)
    return {'fwd': [(t, n[t]) + product_route(sh, n[t], 3 * D, D) for t in range(len(n))],
            'bwd': [(t, n[t]) + product_route(sc, n[t], D, 3 * D) for t in range(len(n) - 1, 0, -1)]}


# ---------------------------------------------------------------------------------------------------------------------
class _SlicedProduct(torch.autograd.Function):
    """h W^T summed slice by slice over K (forward) and dg W summed slice by slice over the 3D gate columns (backward): the order in
    which the gate kernels add the recurrence products' slices."""

    @staticmethod
    def forward(ctx, h, W, kf, kb):
        ctx.save_for_backward(h, W)
        ctx.kb = kb
        out = None
        for k0 in range(0, h.shape[1], kf):
            p = h[:, k0:k0 + kf] @ W[:, k0:k0 + kf].t()
            out = p if out is None else out + p
        return out

    @staticmethod
    def backward(ctx, dg):
        h, W = ctx.saved_tensors
        dh = None
        for k0 in range(0, W.shape[0], ctx.kb):
            p = dg[:, k0:k0 + ctx.kb] @ W[k0:k0 + ctx.kb]
            dh = p if dh is None else dh + p
        return dh, dg.t() @ h, None, None


class GruCase(object):
    def __init__(self, group, lens, D, E, bi, tokens, scale=1.0):
        self.group, self.lens, self.D, self.E, self.bi, self.tokens = group, tuple(int(w) for w in lens), D, E, bool(bi), tokens
        self.scale = scale
        assert list(self.lens) == sorted(self.lens, reverse=True) and self.lens[-1] >= 1 and tokens in TOKEN_KINDS
        self.B, self.Lmax, self.n_tok = len(self.lens), self.lens[0], sum(self.lens)
        self.V = {'random': self.n_tok + 7, 'repeated': 3, 'dense': self.n_tok}[tokens]
        self.off = [sum(self.lens[:b]) for b in range(self.B)]
        self.prefix = prefixes(self.lens)
        shape = ".".join(str(w) for w in self.lens) if self.B <= 5 else "%dcaptions.prefix%s" % (self.B, ".".join(str(n) for n in self.prefix))
        self.name = "%s-D%d-E%d-lens%s-%s-%s" % (group, D, E, shape, 'bi' if bi else 'uni', tokens)
        self.steps = gru_step_routes(self)
        self.fwd_routes = set(s[2] for s in self.steps['fwd'])
        self.bwd_routes = set(s[2] for s in self.steps['bwd'])
        self._cache = {}

    def __repr__(self):
        return self.name

    # ---- what the case covers -------------------------------------------------------------------------------------
    @property
    def eval_projection(self):
        """towers.hip (itr_gru_fwd): `const bool table = 2 * V <= n_tok && !want_per_token;`"""
        return 'vocabulary_table' if 2 * self.V <= self.n_tok else 'per_token'

    @property
    def weight_names(self):
        return WEIGHTS + (tuple(n + '_reverse' for n in WEIGHTS) if self.bi else ())

    @property
    def tensors(self):
        return ('out', 'd_embed') + tuple('d_' + n for n in self.weight_names)

    def route_changes(self, which):
        r = [s[2] for s in self.steps[which]]
        return any(a != b for a, b in zip(r, r[1:]))

    @property
    def grow_steps(self):
        """Steps t + 1 >= 1 whose prefix is shorter than that of step t: the backward pass meets a longer prefix right after them."""
        return [t + 1 for t in range(self.Lmax - 1) if self.prefix[t] > self.prefix[t + 1]]

    @property
    def claims(self):
        out = ['c', 'e']
        if self.Lmax > 1:
            out.append('a')
            if any(s[3] > 1 for s in self.steps['fwd'][1:]):        # (step 0 multiplies h = 0)
                out.append('bf')
            if any(s[3] > 1 for s in self.steps['bwd']):
                out.append('bb')
            if self.grow_steps:
                out.append('d')
        if self.bi:
            out.append('f')
        return tuple(sorted(out))

    def seams(self):
        p = self.prefix
        kinds = set()
        if self.B == 1:
            kinds.add('B=1')
        if self.Lmax == 1:
            kinds.add('all lengths 1')
        if self.B > 1 and self.Lmax > 1 and len(set(self.lens)) == 1:
            kinds.add('all lengths equal')
        if self.B > 1 and self.Lmax > 2 and set(self.lens[1:]) == {1}:
            kinds.add('one long caption, the others of length 1')
        if self.B > 128 and min(p) > 128:
            kinds.add('never leaves the tile kernel')
        return {'D': {self.D}, 'E': {self.E}, 'tokens': {self.tokens}, 'bi': {int(self.bi)}, 'lengths': kinds, 'prefix': set(p), 'B': {self.B},
                'eval_projection': {self.eval_projection}, 'fwd_route': self.fwd_routes, 'bwd_route': self.bwd_routes,
                'fwd_route@bi': set((r, int(self.bi)) for r in self.fwd_routes), 'bwd_route@bi': set((r, int(self.bi)) for r in self.bwd_routes),
                'prefix@D256': set(p) if self.D == 256 else set()}

    # ---- inputs and references ----------------------------------------------------------------------------------
    def inputs(self):
        """Seeded CPU tensors: tokens (int64, packed), embed [V, E], the nn.GRU-named weights, g_out [n_tok, D]."""
        if 'inp' in self._cache:
            return self._cache['inp']
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))

        def uni(k, *shape):
            return (torch.rand(*shape, generator=g) * 2 - 1) * k

        x = {}
        if self.tokens == 'dense':
            x['tokens'] = torch.randperm(self.n_tok, generator=g)
        else:
            x['tokens'] = torch.randint(0, self.V, (self.n_tok,), generator=g)
        x['embed'] = uni(0.1 * self.scale, self.V, self.E)
        k = self.scale / self.D ** 0.5
        for n in self.weight_names:
            x[n] = uni(k, *((3 * self.D,) if 'bias' in n else (3 * self.D, self.E if '_ih_' in n else self.D)))
        x['g_out'] = torch.randn(self.n_tok, self.D, generator=g)
        self._cache['inp'] = x
        return x

    def _rows(self, t, n_act, reverse):
        return [self.off[b] + (self.lens[b] - 1 - t if reverse else t) for b in range(n_act)]

    def forward(self, x, defect=None, sliced=False):
        """(out [n_tok, D], gathered embeddings [n_tok, E]) of the GRU on the packed layout with plain torch ops."""
        D = self.D
        emb = x['embed'][x['tokens']]
        fwd, bwd = {s[0]: s for s in self.steps['fwd']}, {s[0]: s for s in self.steps['bwd']}
        outs = []
        for reverse in ((False, True) if self.bi else (False,)):
            suf = '_reverse' if reverse else ''
            w_ih, w_hh, b_ih, b_hh = (x[n + suf] for n in WEIGHTS)
            gi = emb @ w_ih.t() + b_ih
            h = emb.new_zeros(self.B, D)
            rows_all, vals = [], []
            for t, n_act in enumerate(self.prefix):
                rows = self._rows(t, n_act, reverse)
                hp = h[:n_act]
                _, _, _, ns, kslice = fwd[t]
                if defect == 'a':
                    gh = hp[:, :D - 1] @ w_hh[:, :D - 1].t()
                elif defect == 'bf' and ns > 1:
                    k1 = (ns - 1) * kslice
                    gh = hp[:, :k1] @ w_hh[:, :k1].t()
                elif defect == 'bb' and t in bwd and bwd[t][3] > 1:
                    # the value is right; of the gate columns' gradients only those of the slices before the last reach h
                    k1 = (bwd[t][3] - 1) * bwd[t][4]
                    keep = torch.zeros(3 * D, dtype=hp.dtype)
                    keep[:k1] = 1
                    through_h = hp @ w_hh.detach().t()
                    gh = hp.detach() @ w_hh.t() + (through_h - through_h.detach()) * keep
                elif defect == 'd' and t in self.grow_steps:
                    # the last active row's product sends nothing back to its state (W_hh still receives the row's share)
                    gh = torch.cat([hp[:n_act - 1], hp[n_act - 1:].detach()], 0) @ w_hh.t()
                elif sliced and t > 0:
                    gh = _SlicedProduct.apply(hp, w_hh, kslice, bwd[t][4] if t in bwd else 3 * D)
                else:
                    gh = hp @ w_hh.t()
                gh = gh + b_hh
                g = gi[rows]
                r = torch.sigmoid(g[:, :D] + gh[:, :D])
                z = torch.sigmoid(g[:, D:2 * D] + gh[:, D:2 * D])
                n = torch.tanh(g[:, 2 * D:] + r * gh[:, 2 * D:])
                hn = (1 - z) * n + z * hp
                if defect == 'c':
                    hn = torch.cat([hn[:n_act - 1], hp[n_act - 1:]], 0)
                h = torch.cat([hn, h[n_act:]], 0)
                rows_all += rows
                vals.append(hn)
            outs.append(emb.new_zeros(self.n_tok, D).index_put((torch.tensor(rows_all),), torch.cat(vals, 0)))
        if not self.bi:
            return outs[0], emb
        return (outs[0] + (0 if defect == 'f' else outs[1])) / 2, emb

    def evaluate(self, dtype, defect=None, sliced=False):
        """{tensor: value} in `dtype`: out, last (the rows at len - 1: what gather_last returns), d_embed and every weight gradient."""
        x = {k: (v.to(dtype).clone() if v.is_floating_point() else v) for k, v in self.inputs().items()}
        leaves = ('embed',) + self.weight_names
        for k in leaves:
            x[k].requires_grad_(True)
        out, emb = self.forward(x, defect, sliced)
        wrt = [x[k] for k in leaves] + [emb]
        grads = torch.autograd.grad((out * x['g_out']).sum(), wrt, allow_unused=True)         # (defect a at D = 1 leaves W_hh unused)
        grads = [torch.zeros_like(v) if gr is None else gr for v, gr in zip(wrt, grads)]
        res = {'out': out.detach(), 'last': out.detach()[[o + w - 1 for o, w in zip(self.off, self.lens)]]}
        for k, gr in zip(leaves, grads):
            res['d_' + k] = gr
        if defect == 'e':
            last = int(x['tokens'][-1])
            res['d_embed'] = res['d_embed'].clone()
            res['d_embed'][last] -= grads[-1][-1]
        return res

    def reference(self):
        """{tensor: (want float64, e32, e32_mirror or None, tol)}; computed once and shared."""
        if 'ref' in self._cache:
            return self._cache['ref']
        w64, w32 = self.evaluate(torch.float64), self.evaluate(torch.float32)
        m32 = self.evaluate(torch.float32, sliced=True) if self.name in FALLBACK else None
        out = {}
        for k, want in w64.items():
            e32 = float((w32[k].double() - want).abs().max())
            em = float((m32[k].double() - want).abs().max()) if m32 is not None else None
            out[k] = (want, e32, em, FACTOR * max(e32, em or 0.0, U * float(want.abs().max())))
        self._cache['ref'] = out
        return out

    def defects(self):
        """{letter: {tensor: float64 value}} for every claimed defect."""
        return {d: self.evaluate(torch.float64, defect=d) for d in self.claims}


def _add(group, lens, D, E, bi, tokens, **kw):
    c = GruCase(group, lens, D, E, bi, tokens, **kw)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def _seam(**params):
    SEAMS.update({k: sorted(set(v), key=str) for k, v in params.items()})


# ---------------------------------------------------------------------------------------------------------------------
# D over the split-K thresholds (K = D and K = 3D against 256: D = 85 | 86, 255 | 256), the 256-column gate block, D % 4, the skinny
# strip widths (N = 3D across 1024 and 4096: D = 340 | 344, 1364 | 1368; N = D across 1024: D = 1020 | 1024) and the transpose's
# 64-tile edge; a short batch whose prefix shrinks at every kind of step (4, 3, 3, 1).  E and the token kind rotate; every D runs
# as a uni- and as a bi-GRU where it is the carrier of a route.  B <= 5 and Lmax <= 4 from D = 1020 upward.
SHORT = (4, 3, 3, 1)
GRU_D = (1, 32, 36, 84, 85, 86, 255, 256, 257, 258, 260, 340, 344, 1020, 1024, 1364, 1368)
GRU_E = (1, 5, 127, 128, 129, 300)
for _lens, _D, _E, _bi, _tok in (
        (SHORT, 1, 5, 0, 'random'), (SHORT, 1, 1, 1, 'repeated'),
        (SHORT, 32, 128, 0, 'dense'), (SHORT, 32, 129, 1, 'random'),
        (SHORT, 84, 129, 0, 'repeated'), (SHORT, 36, 127, 1, 'dense'),          # K % 4 == 0, K % 32 != 0, one slice: the float4 loader
        (SHORT, 85, 127, 0, 'random'), (SHORT, 85, 5, 1, 'dense'),
        (SHORT, 86, 300, 0, 'repeated'), (SHORT, 86, 128, 1, 'random'),
        (SHORT, 255, 5, 0, 'dense'), (SHORT, 255, 129, 1, 'repeated'),
        (SHORT, 256, 300, 0, 'random'), (SHORT, 256, 127, 1, 'dense'),
        (SHORT, 257, 128, 0, 'repeated'), (SHORT, 257, 1, 1, 'random'),
        (SHORT, 258, 5, 0, 'random'), (SHORT, 258, 127, 1, 'dense'),
        (SHORT, 260, 300, 0, 'dense'),
        (SHORT, 340, 129, 0, 'random'), (SHORT, 340, 128, 1, 'repeated'),
        (SHORT, 344, 127, 0, 'dense'), (SHORT, 344, 5, 1, 'random'),
        ((3, 2, 2, 1, 1), 1020, 129, 0, 'repeated'),
        (SHORT, 1024, 128, 0, 'random'), ((3, 2, 1), 1024, 300, 1, 'dense'),
        ((3, 2, 1), 1364, 5, 0, 'random'),
        ((4, 2, 2, 1, 1), 1368, 127, 0, 'dense'), ((3, 2, 1), 1368, 128, 1, 'repeated')):
    _add('D', _lens, _D, _E, _bi, _tok)
_seam(D=GRU_D, E=GRU_E, tokens=TOKEN_KINDS, bi=(0, 1), eval_projection=('vocabulary_table', 'per_token'),
      fwd_route=FWD_ROUTES, bwd_route=BWD_ROUTES, **{'fwd_route@bi': [(r, b) for r in FWD_ROUTES for b in (0, 1)],
                                                      'bwd_route@bi': [(r, b) for r in BWD_ROUTES for b in (0, 1)]})

# lengths: one caption; all lengths 1 (no BPTT product at all); a constant prefix; prefix B -> 1 after the first step
for _lens, _D, _E, _bi, _tok in (
        ((3,), 256, 128, 0, 'dense'), ((3,), 32, 5, 1, 'random'),
        ((1, 1, 1), 256, 129, 1, 'random'), ((1, 1, 1), 32, 300, 0, 'dense'),
        ((3, 3, 3), 257, 127, 0, 'random'), ((3, 3, 3), 256, 1, 1, 'repeated'),
        ((4, 1, 1, 1, 1), 256, 5, 0, 'repeated'), ((4, 1, 1, 1, 1), 86, 129, 1, 'dense')):
    _add('lengths', _lens, _D, _E, _bi, _tok)
_seam(lengths=('B=1', 'all lengths 1', 'all lengths equal', 'one long caption, the others of length 1', 'never leaves the tile kernel'))


def _lens_for(prefix):
    """The lengths (sorted, descending) whose active prefix at step t is prefix[t]."""
    out = []
    for t in range(len(prefix) - 1, -1, -1):
        out += [t + 1] * (prefix[t] - len(out))
    return tuple(out)


# prefixes: a D = 256 batch that leaves the tile kernel's partials for the skinny kernel (130, 129 | 128) and ends on 2 rows; the
# skinny kernel's 16-row tiles and its one-tile / two-tile wave split (65, 64 | 17, 16 | 15), once with a short last K slice
# (D = 260); 257 captions that never leave the tile kernel
P130, P65, P257 = (130, 129, 128, 2), (65, 64, 17, 16, 15), (257, 200)
for _p, _D, _E, _bi, _tok in ((P130, 256, 128, 0, 'random'), (P130, 256, 5, 1, 'repeated'), (P65, 260, 129, 0, 'repeated'), (P65, 256, 127, 1, 'dense'),
                              (P257, 256, 300, 0, 'dense'), (P257, 256, 1, 1, 'random')):
    assert prefixes(_lens_for(_p)) == list(_p)
    _add('prefix', _lens_for(_p), _D, _E, _bi, _tok)
_seam(prefix=set(P130 + P65 + P257 + (1,)), B=(1, 130, 257), **{'prefix@D256': P130})
