"""Case table of the glue kernels of the evaluation towers (BERT / SAEM / CAMERA / VSRN: csrc/transformer.hip, agsa_gate.hip,
eltwise.hip, vsrn.hip, norm.hip, reached through itr_amd/ops.py only) and their float64 references.

One entry per (family, shape): seeded CPU inputs, `ref` -- the operation in plain torch ops, run in float64 for `want` and again in
float32 for the reference's own rounding error e32 --, `named`, float64 results that are wrong in one specific way (what a plausible
kernel bug would compute), and the route the library must take.  The dispatch code is mirrored in plain Python (mha_route, norm_route,
agsa_passes, chunks), each function marked with the source lines it copies; tests/test_tower_case_table.py pins the constants to the
source text.  Shapes are the smallest that reach each seam of the launch geometry.

Tolerance of a compared tensor (tests/test_tower_seams_gpu.py applies it, tests/test_tower_case_table.py proves that it is tight and
that it sees every named defect):
    primary    tol = 16 * max(e32, u * max|want|),  u = 2^-24                  (FACTOR, U: tests/helpers/train_prim_cases.py)
    fallback   tol = max(primary, prior)  for the cases named in FALLBACK: `prior` is the a-priori bound of the operation's own
               sequential fp32 sums, (terms + 2) * u * (the sum of the terms' absolute values), derived next to the family (Case.prior)
    condition  tol <= 2^-12 * max|want| for every tensor of every case (CAP)
NaN in `want` (x / ||x|| of an all-zero row) is compared by position: max_err is infinite when the positions differ.
Nothing here imports the library: the table is checked on a machine without a GPU."""
import torch

from train_prim_cases import Case, U, FACTOR, SENSITIVITY, tolerance        # noqa: F401  (re-exported)

CAP = 2.0 ** -12
LN_MAXV, LN_ROWS = 16, 4                    # transformer.hip: float4 per lane (H <= 4096), rows (waves) per workgroup
NORM_MAXV, NORM_WAVES = 16, 4               # norm.hip
GCN_MAXN, GCN_KC = 36, 64                   # vsrn.hip
AGSA_GRID_CAP, AGSA_WAVES, AGSA_TILE = 256 * 8, 4, 16          # agsa_gate.hip: workgroups at most, waves per workgroup, rows per wave pass
MHA_MAXL, MHA_DKS = 64, (16, 32, 64)
MHA_REG_WAVES = 4                           # transformer.hip: mha_reg_kernel
MHA_LDS_WAVES = {1: 4, 2: 4, 3: 2, 4: 2}    # transformer.hip: dispatch_mha_mfma, waves per workgroup by NT
SUMMARIZE_MAXR, SUMMARIZE_THREADS = 64, 256
CHUNK = 65535                               # ops.relu_maxpool / ops.mean_mid: groups per call (grid y)
ACTS = ('none', 'relu', 'tanh', 'sigmoid', 'gelu', 'leaky_relu')          # the codes itr_affine_cols accepts (0 .. 5)
NORM_EPS = {0: 1e-8, 1: 1e-8, 2: 1e-12, 3: 0.0}       # ops.l2norm, ops.l1norm, ops.normalize, ops.pdist_cos

FAMILIES = ('attention', 'add_layernorm', 'bert_embed_ln', 'relu_maxpool', 'mean_mid', 'agsa_gate', 'gcn_relation', 'camera_summarize',
            'camera_posenc', 'affine_cols', 'mul_rows', 'norm')
SEAMS = {}          # 'family.parameter' -> values that must appear in the table, filled next to the cases
CASES = []
_BY_NAME = {}

# Cases whose kernel is honestly outside the primary rule (an accumulation order the float32 torch reference does not share): they
# are judged by their family's a-priori bound (module docstring).  No case needs it (profiles/tower_seams/measured.txt).
FALLBACK = set()

# What each entry point refuses (tests/test_tower_seams_gpu.py makes the calls): NotImplementedError or RuntimeError.
REFUSALS = ('mha L=65', 'mha dk=8', 'layernorm H=4100', 'agsa dk=64', 'gcn N=37', 'summarize R=65')


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the dispatch code
def ceil_div(a, b):
    return -(-a // b)


def mha_route(q_off, k_off, v_off, ldq, ldk, ldv, out_off, ldo, L):
    """transformer.hip (itr_mha_small: `const bool al = ...`; dispatch_mha_mfma) -> (route, NT, waves per workgroup).  Offsets are in
    floats from a 16-byte aligned address, strides in floats.  'valu' is mha_small_kernel: one wave per workgroup, no key tiles."""
    if any(s % 4 for s in (ldq, ldk, ldv)) or any(o % 4 for o in (q_off, k_off, v_off)):
        return 'valu', 0, 1
    nt = ceil_div(L, 16)
    if ldo % 4 == 0 and out_off % 4 == 0:
        return 'reg', nt, MHA_REG_WAVES
    return 'lds', nt, MHA_LDS_WAVES[nt]


def norm_route(dim, aligned):
    """norm.hip (norm_rows: `const bool vec = ...`)."""
    return 'vec' if dim % 4 == 0 and dim <= 64 * 4 * NORM_MAXV and aligned else 'scalar'


def agsa_passes(rows):
    """agsa_gate.hip (itr_agsa_gate's grid; `for (int64_t t = wave0; t < ntiles; t += nwaves)`): the passes of the busiest wave."""
    ntiles = ceil_div(rows, AGSA_TILE)
    grid = min(ceil_div(ntiles, AGSA_WAVES), AGSA_GRID_CAP)
    return ceil_div(ntiles, grid * AGSA_WAVES)


def chunks(B):
    """ops.relu_maxpool / ops.mean_mid: `for b0 in range(0, B, 65535)`."""
    return ceil_div(B, CHUNK)


def max_err(got, want):
    """max |got - want| (float64) over the positions where `want` is a number; infinite when the NaN positions differ or a compared
    value is not finite."""
    got = got.double()
    gn, wn = torch.isnan(got), torch.isnan(want)
    if tuple(got.shape) != tuple(want.shape) or not torch.equal(gn, wn):
        return float('inf')
    if want.numel() == 0:
        return 0.0
    return float(torch.where(wn, torch.zeros_like(want), (got - want).abs()).max())


def max_abs(want):
    return float(torch.nan_to_num(want, nan=0.0).abs().max()) if want.numel() else 0.0


class TowerCase(Case):
    """train_prim_cases.Case plus named defects, the route, the seam values the case carries and the fallback term."""

    def __init__(self, family, shape, make, ref, named, route=None, seams=None, extra=None, prior=None):
        Case.__init__(self, family, shape, make, ref, extra=extra)
        self.family, self.named, self.route, self.prior = family, dict(named), route, prior
        self._seams = {family + '.' + k: set(v if isinstance(v, (set, list)) else [v]) for k, v in (seams or {}).items()}

    def seams(self):
        return self._seams

    def x64(self):
        return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in self.inputs().items()}

    def reference(self):
        """{tensor: (want float64, e32, tol, rule)}; computed once and shared."""
        if 'ref' in self._cache:
            return self._cache['ref']
        w64, w32 = self.evaluate(torch.float64), self.evaluate(torch.float32)
        fb = self.name in FALLBACK
        prior = self.prior(self.x64()) if fb else {}
        out = {}
        for k, want in w64.items():
            e32 = max_err(w32[k], want)
            out[k] = (want, e32, max(FACTOR * max(e32, U * max_abs(want)), prior.get(k, 0.0)), 'fallback' if fb else 'primary')
        self._cache['ref'] = out
        return out

    def defects(self):
        """{defect name: {tensor: float64 value}} for every defect the case claims."""
        x = self.x64()
        return {name: fn(x) for name, fn in self.named.items()}


def _add(family, shape, make, ref, named, **kw):
    c = TowerCase(family, shape, make, ref, named, **kw)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(*families):
    return [c for c in CASES if c.family in families]


def _seam(family, **params):
    for k, v in params.items():
        SEAMS[family + '.' + k] = sorted(set(v), key=str)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g)


def _zero_last(name):
    """A flat kernel whose last element is never written."""
    def defect(x, want):
        d = want[name].clone()
        d.view(-1)[-1] = 0.0
        return {name: d}
    return defect


# ---------------------------------------------------------------------------------------------------------------------
# attention (ops.mha_small): matrix-core kernels in registers ('reg': 16-byte aligned output rows, four waves per workgroup) or with
# LDS staging ('lds': any other output; four waves, two from NT = 3), NT = ceil(L / 16) key / query tiles; the VALU kernel ('valu',
# one wave per workgroup) for q, k or v that are not 16-byte aligned or have a row stride that is no multiple of 4.
MHA_L = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
VALU_L = (1, 33, 64)
MHA_LAYOUTS = ('fused', 'camera', 'fused+1', 'stride3A+1')
PAIR_SHAPES = {1: (1, 1), 2: (2, 1), 3: (1, 3), 4: (2, 2), 5: (5, 1), 9: (3, 3)}          # B * heads -> (B, heads)
# pair counts of the nine (L, dk) cases of one (route, NT): below, at and one above the waves per workgroup (4; 2; 1)
PAIR_COUNTS = {4: (1, 4, 5, 3, 9, 4, 5, 3, 9), 2: (1, 2, 3, 4, 5, 9, 2, 3, 1), 1: (1, 2, 3, 4, 5, 9, 1, 2, 3)}


def mha_placement(layout, out_kind, A):
    """-> (buffers {name: (floats skipped in front, row stride)}, operands {'q' | 'k' | 'v' | 'out': (buffer, first column)}).  The
    GPU test builds NaN-filled buffers from this; an operand absent from the second dict ('out') is the library's own tensor.
        fused        one [rows, 3A] buffer, q | k | v column slices (BERT, SAEM)
        camera       q and k contiguous, v the second half of the columns of a [rows, 2A] buffer (CAMERA)
        fused+1      the fused buffer one float into its allocation: q, k and v are 4 bytes off a 16-byte boundary
        stride3A+1   the fused slices in a buffer whose row stride is 3A + 1
    out_kind 'block+1': the output is the column block [1, 1 + A) of a [rows, A + 2] buffer."""
    if layout == 'camera':
        bufs, ops = {'q': (0, A), 'k': (0, A), 'xv': (0, 2 * A)}, {'q': ('q', 0), 'k': ('k', 0), 'v': ('xv', A)}
    else:
        bufs = {'qkv': {'fused': (0, 3 * A), 'fused+1': (1, 3 * A), 'stride3A+1': (0, 3 * A + 1)}[layout]}
        ops = {'q': ('qkv', 0), 'k': ('qkv', A), 'v': ('qkv', 2 * A)}
    if out_kind == 'block+1':
        bufs['out'], ops['out'] = (0, A + 2), ('out', 1)
    return bufs, ops


def mha_case_route(layout, out_kind, A, L):
    bufs, ops = mha_placement(layout, out_kind, A)
    off = {n: bufs[b][0] + col for n, (b, col) in ops.items()}
    ld = {n: bufs[b][1] for n, (b, col) in ops.items()}
    return mha_route(off['q'], off['k'], off['v'], ld['q'], ld['k'], ld['v'], off.get('out', 0), ld.get('out', A), L)


def _mha_mask(g, B, L, first):
    """(B, L) of 0 / 1 and the kinds used: sequences alternate between a ragged tail (the last key is masked) and holes inside the
    sequence (the last key is kept); every sequence keeps a key."""
    m, kinds = torch.ones(B, L), set()
    for b in range(B):
        kind = ('ragged', 'holes')[(b + first) % 2]
        if L == 1:
            continue
        kinds.add(kind)
        if kind == 'ragged':
            m[b, 1 + int(torch.randint(0, L - 1, (1,), generator=g)):] = 0.0
        elif L == 2:
            m[b, 0] = 0.0
        else:
            m[b] = (torch.rand(L, generator=g) < 0.6).float()
            m[b, L // 2], m[b, -1] = 0.0, 1.0
    return m, kinds


def _mha_make(B, L, heads, dk, masked, first):
    def make(g):
        A = heads * dk
        d = {n: _rn(g, B * L, A) for n in 'qkv'}
        # the value row of key L - 1 stands out (2 .. 2.5, another value per column): the row the matrix-core kernels re-read for padding keys
        d['v'].view(B, L, A)[:, -1] = 2.0 + 0.5 * torch.rand(B, A, generator=g)
        if masked:
            d['mask'] = _mha_mask(g, B, L, first)[0]
        return d
    return make


def mha_ref(x, B, L, heads, dk, defect=None):
    q, k, v = (x[n].reshape(B, L, heads, dk).permute(0, 2, 1, 3) for n in 'qkv')
    if defect == 'neighbour head':
        v = v.roll(-1, 1)
    s = q @ k.transpose(2, 3) / dk ** 0.5
    if 'mask' in x and defect != 'mask ignored':
        s = s + (1.0 - x['mask'])[:, None, None, :] * -10000.0
    if defect == 'padding key counted':
        s = torch.cat([s, q @ k[:, :, L - 1:].transpose(2, 3) / dk ** 0.5], -1)
        v = torch.cat([v, v[:, :, L - 1:]], 2)
    P = torch.softmax(s, -1)
    if defect == 'last key dropped':
        P, v = P[..., :L - 1], v[:, :, :L - 1]
    return {'out': (P @ v).permute(0, 2, 1, 3).reshape(B * L, heads * dk)}


def _mha_add(i, route_want, layout, out_kind, L, dk, pairs):
    B, heads = PAIR_SHAPES[pairs]
    A = heads * dk
    route = mha_case_route(layout, out_kind, A, L)
    assert route[0] == route_want, (route, route_want, layout, out_kind, L, dk)
    for masked in (0, 1):
        shape = {'route': route[0], 'L': L, 'dk': dk, 'B': B, 'heads': heads, 'layout': layout, 'mask': masked}
        c_args = (B, L, heads, dk)
        make = _mha_make(B, L, heads, dk, masked, i)
        last_kept, kinds = True, set()
        if masked:
            c0 = TowerCase('attention', shape, make, None, {})
            m = c0.inputs()['mask']
            last_kept = bool((m[:, -1] == 1).any())
            kinds = _mha_mask(torch.Generator().manual_seed(0), B, L, i)[1]
        named = {}
        if last_kept:
            named['last key dropped'] = (lambda a: lambda x: mha_ref(x, *a, defect='last key dropped'))(c_args)
        if route[0] != 'valu' and L % 16 and L > 1:          # (L = 1: the padding key is the only key over again)
            named['padding key counted'] = (lambda a: lambda x: mha_ref(x, *a, defect='padding key counted'))(c_args)
        if masked and L > 1:
            named['mask ignored'] = (lambda a: lambda x: mha_ref(x, *a, defect='mask ignored'))(c_args)
        if heads > 1:
            named['neighbour head'] = (lambda a: lambda x: mha_ref(x, *a, defect='neighbour head'))(c_args)
        w = route[2]
        count = 'below' if pairs < w else 'equal' if pairs == w else 'above' if pairs == w + 1 else 'more'
        _add('attention', shape, make, (lambda a: lambda x: mha_ref(x, *a))(c_args), named, route=route,
             seams={'L': L, 'dk': dk, 'mask': masked, 'layout': layout, 'pairs': pairs, 'route_nt_dk': [(route[0], route[1], dk)],
                    'route_nt_count': [(route[0], route[1], count)], 'mask_kind': kinds,
                    'last_key': ['kept' if last_kept else 'masked'] if masked and L > 1 else []},
             extra={'B': B, 'L': L, 'heads': heads, 'dk': dk, 'layout': layout, 'out': out_kind})


for _ri, (_route, _out) in enumerate((('reg', 'own'), ('lds', 'block+1'))):
    for _li, _L in enumerate(MHA_L):
        for _di, _dk in enumerate(MHA_DKS):
            _nt = ceil_div(_L, 16)
            _w = MHA_REG_WAVES if _route == 'reg' else MHA_LDS_WAVES[_nt]
            _i = 3 * (_li % 3) + _di
            _mha_add(_i + _ri, _route, ('fused', 'camera')[(_i + _ri) % 2], _out, _L, _dk, PAIR_COUNTS[_w][_i])
for _yi, _layout in enumerate(('fused+1', 'stride3A+1')):
    for _li, _L in enumerate(VALU_L):
        for _di, _dk in enumerate(MHA_DKS):
            _i = 3 * _li + _di
            _mha_add(_i + _yi, 'valu', _layout, 'own', _L, _dk, PAIR_COUNTS[1][(_i + 4 * _yi) % 9])
_seam('attention', L=MHA_L, dk=MHA_DKS, mask=(0, 1), layout=MHA_LAYOUTS, pairs=(1, 3, 4, 5, 9), mask_kind=('ragged', 'holes'),
      last_key=('kept', 'masked'),
      route_nt_dk=[(r, nt, dk) for r in ('reg', 'lds') for nt in (1, 2, 3, 4) for dk in MHA_DKS] + [('valu', 0, dk) for dk in MHA_DKS],
      route_nt_count=[(r, nt, c) for r in ('reg', 'lds') for nt in (1, 2, 3, 4) for c in ('below', 'equal', 'above')] +
                     [('valu', 0, 'equal'), ('valu', 0, 'above')])


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm(x + residual) and the embedding sum + LayerNorm: one wave per row, four rows per workgroup, lane + 64 i float4 per lane
LN_ROW_COUNTS = (1, 3, 4, 5, 9)
LN_H = (4, 252, 256, 260, 768, 4096)
LN_EPS = 1e-12


def _ln_tail(z, gamma, beta, drop4):
    H = z.shape[-1]
    n = H - 4 if drop4 else H
    u = z[..., :n].sum(-1, keepdim=True) / H
    q = ((z - u) ** 2)[..., :n].sum(-1, keepdim=True) / H
    return gamma * ((z - u) / torch.sqrt(q + LN_EPS)) + beta


def _ln_make(rows, H, res):
    def make(g):
        d = {'x': _rn(g, rows, H), 'gamma': torch.rand(H, generator=g) + 0.5, 'beta': _rn(g, H) * 0.1}
        d['x'][:, -4:] += 3.0                       # the last float4 of every row is an outlier
        if res:
            d['res'] = _rn(g, rows, H)
        return d
    return make


def add_ln_ref(x, defect=None):
    z = x['x'] + x['res'] if 'res' in x and defect != 'residual dropped' else x['x']
    return {'y': _ln_tail(z, x['gamma'], x['beta'], defect == 'last float4 out of the mean')}


for _res in (1, 0):
    for _r in LN_ROW_COUNTS:
        for _h in LN_H:
            _named = {'last float4 out of the mean': lambda x: add_ln_ref(x, 'last float4 out of the mean')}
            if _res:
                _named['residual dropped'] = lambda x: add_ln_ref(x, 'residual dropped')
            _add('add_layernorm', {'res': _res, 'rows': _r, 'H': _h}, _ln_make(_r, _h, _res), add_ln_ref, _named,
                 seams={'rows': _r, 'H': _h, 'res': _res})
_seam('add_layernorm', rows=LN_ROW_COUNTS, H=LN_H, res=(0, 1))

EMB_ROWS = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 9: (3, 3)}            # rows -> (B, L)
EMB_V, EMB_TV = 11, 2


def _emb_make(B, L, H, P, typed):
    def make(g):
        d = {'ids': torch.randint(0, EMB_V, (B, L), generator=g), 'word': _rn(g, EMB_V, H), 'pos': _rn(g, P, H), 'type': _rn(g, EMB_TV, H),
             'gamma': torch.rand(H, generator=g) + 0.5, 'beta': _rn(g, H) * 0.1}
        d['word'][:, -4:] += 3.0
        if typed:
            d['type_ids'] = torch.randint(0, EMB_TV, (B, L), generator=g)
            d['type_ids'][:, -1] = 1
        return d
    return make


def embed_ln_ref(x, defect=None):
    B, L = x['ids'].shape
    t = torch.arange(L)
    if defect == 'position t - 1':
        t = (t - 1) % L
    ty = x['type_ids'] if 'type_ids' in x and defect != 'type embedding ignored' else torch.zeros_like(x['ids'])
    z = x['word'][x['ids']] + x['pos'][t][None] + x['type'][ty]
    return {'y': _ln_tail(z, x['gamma'], x['beta'], defect == 'last float4 out of the mean')}


for _hi, _h in enumerate(LN_H):
    for _ri, _r in enumerate(LN_ROW_COUNTS):
        _B, _L = EMB_ROWS[_r]
        _typed, _full = (_hi + _ri) % 2, ((_hi + _ri) // 2) % 2
        _named = {'last float4 out of the mean': lambda x: embed_ln_ref(x, 'last float4 out of the mean')}
        if _L > 1:
            _named['position t - 1'] = lambda x: embed_ln_ref(x, 'position t - 1')
        if _typed:
            _named['type embedding ignored'] = lambda x: embed_ln_ref(x, 'type embedding ignored')
        _add('bert_embed_ln', {'B': _B, 'L': _L, 'H': _h, 'P': _L if _full else _L + 3, 'types': _typed},
             _emb_make(_B, _L, _h, _L if _full else _L + 3, _typed), embed_ln_ref, _named,
             seams={'rows': _r, 'H': _h, 'types': _typed, 'L_vs_max_pos': 'equal' if _full else 'below'})
_seam('bert_embed_ln', rows=LN_ROW_COUNTS, H=LN_H, types=(0, 1), L_vs_max_pos=('below', 'equal'))


# ---------------------------------------------------------------------------------------------------------------------
# relu + max over the first `valid` positions (evaluation form): one thread per channel, 256 per workgroup, grid y = the batch item,
# at most 65535 per call
RMP_C = (1, 255, 256, 257)
RMP_L = 5


def _rmp_make(B, L, C, valid):
    def make(g):
        x = _rn(g, B, L, C).clamp(-2.5, 2.5)
        x[:, valid - 1, :] = 3.0 + torch.rand(B, C, generator=g)      # the decisive maximum is the last valid position
        if valid < L:
            x[:, valid, :] = 6.0                                      # ... and the first position that must not be seen is larger
        if C > 1:
            x[:, :, 0] = -x[:, :, 0].abs() - 0.1                      # an all-negative channel: 0
        return {'x': x}
    return make


def rmp_ref(x, valid, shift=0, lose_from=None):
    t = torch.relu(x['x'])[:, :valid + shift]
    y = t.max(1).values if t.shape[1] else torch.zeros(t.shape[0], t.shape[2], dtype=t.dtype)
    if lose_from is not None:
        y = y.clone()
        y[lose_from:] = 0.0
    return {'y': y}


def _rmp_add(B, L, C, valid):
    named = {'valid one too small': lambda x: rmp_ref(x, valid, -1)}
    if valid < L:
        named['valid one too large'] = lambda x: rmp_ref(x, valid, 1)
    if chunks(B) > 1:
        named['second chunk lost'] = lambda x: rmp_ref(x, valid, lose_from=CHUNK)
    _add('relu_maxpool', {'B': B, 'L': L, 'C': C, 'valid': valid}, _rmp_make(B, L, C, valid), lambda x: rmp_ref(x, valid), named,
         seams={'C': C, 'valid': {1: ['1'], L - 1: ['L-1'], L: ['L']}.get(valid, []) if L == RMP_L else [], 'chunks': chunks(B)},
         extra={'valid': valid})


for _c in RMP_C:
    for _v in (1, RMP_L - 1, RMP_L):
        _rmp_add(3, RMP_L, _c, _v)
_rmp_add(CHUNK + 1, 2, 3, 1)
_seam('relu_maxpool', C=RMP_C, valid=('1', 'L-1', 'L'), chunks=(1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# mean over the middle axis: one thread per four features (float4 when F % 4 == 0), grid y = the group, at most 65535 per call.
# A-priori term of the sequential sum of R terms and the division: (R + 1) u mean_r |x|.
MM_F = (1, 3, 4, 5, 1023, 1024, 1028)
MM_R = (1, 36)


def _mm_make(B, R, F):
    def make(g):
        x = _rn(g, B, R, F) + 1.5
        x[:, -1, :] = 3.0
        return {'x': x}
    return make


def mm_ref(x, lose_from=None):
    y = x['x'].mean(1)
    if lose_from is not None:
        y = y.clone()
        y[lose_from:] = 0.0
    return {'y': y}


def _mm_add(B, R, F):
    named = {'last group lost': lambda x: mm_ref(x, B - 1)}
    if chunks(B) > 1:
        named['second chunk lost'] = lambda x: mm_ref(x, CHUNK)
    _add('mean_mid', {'B': B, 'R': R, 'F': F}, _mm_make(B, R, F), mm_ref, named, seams={'F': F, 'R': R, 'chunks': chunks(B), 'chunks_F': [(chunks(B), F)]},
         prior=lambda x: {'y': (R + 1) * U * float(x['x'].abs().mean(1).max())})


for _f in MM_F:
    for _r in MM_R:
        _mm_add(3, _r, _f)
_mm_add(CHUNK + 1, 2, 4)
_mm_add(CHUNK + 1, 2, 5)                # the second chunk starts 12 bytes off a 16-byte boundary
_seam('mean_mid', F=MM_F, R=MM_R, chunks=(1, 2), chunks_F=((2, 4), (2, 5)))


# ---------------------------------------------------------------------------------------------------------------------
# CAMERA's query / key gate: one wave per 16 rows, four waves per workgroup, at most 256 * 8 workgroups (persistent loop above)
AGSA_ROWS = (1, 15, 16, 17, 63, 64, 65, AGSA_TILE * AGSA_WAVES * AGSA_GRID_CAP, AGSA_TILE * AGSA_WAVES * AGSA_GRID_CAP + 16 + 5)
AGSA_DK = (16, 32)


def _agsa_make(rows, dk):
    def make(g):
        s = dk ** -0.5
        return {'q': _rn(g, rows, dk), 'k': _rn(g, rows, dk), 'Wq': _rn(g, dk, dk) * s, 'bq': _rn(g, dk) * 0.1, 'Wk': _rn(g, dk, dk) * s,
                'bk': _rn(g, dk) * 0.1, 'Wg': _rn(g, 2 * dk, dk) * s, 'bg': _rn(g, 2 * dk) * 0.1}
    return make


def agsa_ref(x, defect=None):
    dk = x['q'].shape[1]
    G = (x['q'] @ x['Wq'].t() + x['bq']) * (x['k'] @ x['Wk'].t() + x['bk'])
    M = torch.sigmoid(G @ x['Wg'].t() + x['bg'])
    mq, mk = (M[:, dk:], M[:, :dk]) if defect == 'gate halves swapped' else (M[:, :dk], M[:, dk:])
    qo, ko = x['q'] * mq, x['k'] * mk
    if defect == 'second-pass tile unwritten':
        first = AGSA_TILE * AGSA_WAVES * AGSA_GRID_CAP
        qo = qo.clone()
        qo[first:first + AGSA_TILE] = 0.0
    return {'qo': qo, 'ko': ko}


for _dk in AGSA_DK:
    for _r in AGSA_ROWS:
        _named = {'gate halves swapped': lambda x: agsa_ref(x, 'gate halves swapped')}
        if agsa_passes(_r) > 1:
            _named['second-pass tile unwritten'] = lambda x: agsa_ref(x, 'second-pass tile unwritten')
        _add('agsa_gate', {'dk': _dk, 'rows': _r}, _agsa_make(_r, _dk), agsa_ref, _named, route=agsa_passes(_r),
             seams={'dk': _dk, 'rows': _r, 'passes_dk': [(agsa_passes(_r), _dk)]})
_seam('agsa_gate', dk=AGSA_DK, rows=AGSA_ROWS, passes_dk=[(p, d) for p in (1, 2) for d in AGSA_DK])


# ---------------------------------------------------------------------------------------------------------------------
# VSRN's region affinity y = (theta phi^T / N) g: one workgroup per image, theta / phi through LDS in 64-column chunks, 3 x 3 register
# tiles of R on 12 x 12 threads, then one thread per output column.  A-priori bound of the two sequential fmaf chains (D products, the
# division, then N products): ((D + 2) + (N + 2)) u (|theta| |phi|^T / N) |g|, its largest element.  theta and phi have mean 1 and
# deviation 1 (times D^-1/4): signed, but theta . phi does not cancel.  With a zero mean, sum |theta| |phi| is 30 x |R| at D = 2048: the
# output is then the small remainder of a cancelling sum, the error of the kernel's ONE chain of 2048 fmaf (a random walk of about
# sqrt(D / 3) u / sqrt(12) = 8 u of the partial sums) is measured against that remainder (N = 1, where nothing is averaged behind it:
# 26 u max|want|, 0.8 x the primary bound with one host's e32 and 1.6 x with another's), and no a-priori bound of a sum, all in terms
# of sum |theta| |phi|, stays under the 2^-12 cap either.  Without the cancellation the same chain is at 6 u max|want|.
GCN_N = (1, 2, 3, 35, 36)
GCN_D = (4, 60, 64, 68, 260, 2048)


def _gcn_make(n_img, N, D):
    def make(g):
        t = _rn(g, n_img * N, 3 * D)
        t[:, :2 * D] = (t[:, :2 * D] + 1.0) * D ** -0.25
        return {'tpg': t}
    return make


def gcn_ref(x, n_img, N, D, defect=None):
    th, ph, g = (x['tpg'].view(n_img, N, 3, D)[:, :, i] for i in range(3))
    if defect == 'partial last chunk dropped':
        keep = D - D % GCN_KC
        th, ph = th[..., :keep], ph[..., :keep]
    R = th @ ph.transpose(1, 2) / (GCN_MAXN if defect == 'divisor 36' else N)
    if defect == 'region N - 1 dropped':
        R, g = R[:, :, :N - 1], g[:, :N - 1]
    return {'y': (R @ g).reshape(n_img * N, D)}


def _gcn_prior(n_img, N, D):
    def prior(x):
        a = {'tpg': x['tpg'].abs()}
        return {'y': (D + N + 4) * U * float(gcn_ref(a, n_img, N, D)['y'].max())}
    return prior


def _gcn_add(n_img, N, D, pad=0):
    a = (n_img, N, D)
    named = {'region N - 1 dropped': lambda x: gcn_ref(x, *a, defect='region N - 1 dropped')}
    if D % GCN_KC:
        named['partial last chunk dropped'] = lambda x: gcn_ref(x, *a, defect='partial last chunk dropped')
    if N < GCN_MAXN:
        named['divisor 36'] = lambda x: gcn_ref(x, *a, defect='divisor 36')
    shape = {'n_img': n_img, 'N': N, 'D': D}
    if pad:
        shape['ld'] = 3 * D + pad
    _add('gcn_relation', shape, _gcn_make(*a), lambda x: gcn_ref(x, *a), named, seams={'N': N, 'D': D, 'n_img': n_img, 'ld': ['3D+4' if pad else '3D']},
         extra={'n_img': n_img, 'N': N, 'D': D, 'ld': 3 * D + pad, 'ldy': D + pad}, prior=_gcn_prior(*a))


for _ni, _n in enumerate(GCN_N):
    for _di, _d in enumerate(GCN_D):
        _gcn_add((1, 3)[(_ni + _di) % 2], _n, _d)
_gcn_add(3, 35, 68, pad=4)
_seam('gcn_relation', N=GCN_N, D=GCN_D, n_img=(1, 3), ld=('3D', '3D+4'))


# ---------------------------------------------------------------------------------------------------------------------
# CAMERA's multi-view summary: one workgroup per (image, view), softmax over R <= 64 regions by one thread, D strided by 256 threads, the
# norm reduced over four waves.  A-priori term of the sequential sum over R and of the norm: (R + 4) u max|out|.
SMRY_R = (1, 36, 63, 64)
SMRY_K = (1, 12)
SMRY_D = (1, 255, 256, 257, 2048)


def _smry_make(B, R, k, D):
    def make(g):
        d = {'smry': _rn(g, B, R, k), 'X': _rn(g, B, R, D)}
        d['smry'][:, -1, :] = 3.0                   # the last region holds a large share of every view
        d['X'][:, :, -1] = 2.0                      # ... and the last column a large share of every norm
        return d
    return make


def smry_ref(x, defect=None):
    L, X = torch.softmax(x['smry'], 1), x['X']
    if defect == 'last region dropped':
        L, X = L[:, :-1], X[:, :-1]
    s = L.transpose(1, 2) @ X
    n = (s[..., :SUMMARIZE_THREADS] if defect == 'norm over the first 256 columns' else s).pow(2).sum(-1, keepdim=True).sqrt()
    return {'out': s / torch.clamp(n, min=1e-12)}


for _ri, _r in enumerate(SMRY_R):
    for _di, _d in enumerate(SMRY_D):
        _k = SMRY_K[(_ri + _di) % 2]
        _named = {}
        if _d > 1 or _r == 1:                       # (D = 1: the summary is +-1 whatever the weights are)
            _named['last region dropped'] = lambda x: smry_ref(x, 'last region dropped')
        if _d > SUMMARIZE_THREADS:
            _named['norm over the first 256 columns'] = lambda x: smry_ref(x, 'norm over the first 256 columns')
        _add('camera_summarize', {'B': 2, 'R': _r, 'k': _k, 'D': _d}, _smry_make(2, _r, _k, _d), smry_ref, _named,
             seams={'R': _r, 'k': _k, 'D': _d}, prior=(lambda R: lambda x: {'out': (R + 4) * U})(_r))
_seam('camera_summarize', R=SMRY_R, k=SMRY_K, D=SMRY_D)

# box position features: one thread per box, 256 per workgroup
POSENC_SHAPES = ((1, 1), (5, 51), (4, 64), (1, 257))


def _posenc_make(B, R):
    def make(g):
        xy = torch.rand(B, R, 2, generator=g) * 100.0
        return {'boxes': torch.cat([xy, xy + torch.rand(B, R, 2, generator=g) * 100.0 + 1.0], -1), 'wh': torch.rand(B, 2, generator=g) * 500.0 + 100.0}
    return make


def posenc_ref(x):
    b, W, H = x['boxes'], x['wh'][:, None, 0], x['wh'][:, None, 1]
    px, py, w, h = b[..., 0], b[..., 1], b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    return {'out': torch.stack([px / W, py / H, w / W, h / H, w / h, (w * h) / (W * H)], -1)}


for _b, _r in POSENC_SHAPES:
    _add('camera_posenc', {'B': _b, 'R': _r}, _posenc_make(_b, _r), posenc_ref,
         {'last box unwritten': (lambda z: lambda x: z(x, posenc_ref(x)))(_zero_last('out'))}, seams={'boxes': _b * _r})
_seam('camera_posenc', boxes=[b * r for b, r in POSENC_SHAPES])


# ---------------------------------------------------------------------------------------------------------------------
# act(x * scale[c] + shift[c]) + residual and a[r, c] * b[r * ldb + c]: one thread per element, 256 per workgroup
ELT_SHAPES = ((1, 1), (85, 3), (256, 1), (1, 257))            # (R, C): R * C = 1, 255, 256, 257; C = 1, 3, 257
ACT_FN = {'none': lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid,
          'gelu': lambda t: t * 0.5 * (1.0 + torch.erf(t / 2.0 ** 0.5)), 'leaky_relu': lambda t: torch.where(t > 0, t, 0.1 * t)}


def _aff_make(R, C, scaled, res):
    def make(g):
        d = {'x': _rn(g, R, C)}
        d['x'][-1, -1] = -1.0 if res else 1.25      # the last element: act(-1) + 2 is far from act(-1 + 2) for every activation
        if scaled:
            d['scale'], d['shift'] = torch.rand(C, generator=g) + 0.5, _rn(g, C) * 0.3
            d['scale'][-1], d['shift'][-1] = 1.0, 0.0
        if res:
            d['res'] = _rn(g, R, C)
            d['res'][-1, -1] = 2.0
        return d
    return make


def aff_ref(x, act, defect=None):
    v = x['x'] * x['scale'] + x['shift'] if 'scale' in x else x['x']
    if defect == 'activation after the residual':
        return {'y': ACT_FN[act](v + x['res'])}
    v = ACT_FN[act](v)
    return {'y': v + x['res'] if 'res' in x else v}


for _act in ACTS:
    for _scaled in (0, 1):
        for _res in (0, 1):
            for _r, _c in ELT_SHAPES:
                _named = {'last element unwritten': (lambda z, a: lambda x: z(x, aff_ref(x, a)))(_zero_last('y'), _act)}
                if _res and _act != 'none':
                    _named['activation after the residual'] = (lambda a: lambda x: aff_ref(x, a, 'activation after the residual'))(_act)
                _add('affine_cols', {'act': _act, 'scale': _scaled, 'res': _res, 'R': _r, 'C': _c}, _aff_make(_r, _c, _scaled, _res),
                     (lambda a: lambda x: aff_ref(x, a))(_act), _named, extra={'act': _act},
                     seams={'act': _act, 'scale': _scaled, 'res': _res, 'n': _r * _c, 'C': _c, 'act_scale_res': [(_act, _scaled, _res)]})
_seam('affine_cols', act=ACTS, scale=(0, 1), res=(0, 1), n=(1, 255, 256, 257), C=(1, 3, 257),
      act_scale_res=[(a, s, r) for a in ACTS for s in (0, 1) for r in (0, 1)])

MULROWS_SHAPES = ((85, 3), (4, 64), (257, 1))
MULROWS_PAD, MULROWS_COL = 5, 2


def _mr_make(R, C):
    def make(g):
        return {'a': _rn(g, R, C) + 2.0, 'bbuf': _rn(g, R, C + MULROWS_PAD)}
    return make


def mr_ref(x, defect=None):
    R, C = x['a'].shape
    b = x['bbuf'][:, MULROWS_COL:MULROWS_COL + C]
    if defect == 'ldb ignored':
        b = x['bbuf'].reshape(-1)[MULROWS_COL:MULROWS_COL + R * C].view(R, C)
    return {'y': x['a'] * b}


for _r, _c in MULROWS_SHAPES:
    _add('mul_rows', {'R': _r, 'C': _c, 'ldb': _c + MULROWS_PAD}, _mr_make(_r, _c), mr_ref, {'ldb ignored': lambda x: mr_ref(x, 'ldb ignored')},
         seams={'n': _r * _c})
_seam('mul_rows', n=[r * c for r, c in MULROWS_SHAPES])


# ---------------------------------------------------------------------------------------------------------------------
# row norms (ops._norm): one wave per row, four rows per workgroup; rows of at most 4096 floats stay in registers as float4 when the
# row length is a multiple of 4 and both pointers are 16-byte aligned ('vec'), else two scalar passes ('scalar').
# kinds: 0 x / (||x||_2 + eps)   1 x / (||x||_1 + eps)   2 x / max(||x||_2, eps)   3 x / ||x||_2 (0 / 0 = NaN kept)
NORM_DIM = (1, 3, 4, 252, 256, 260, 4096, 4100)
NORM_ROW_COUNTS = (1, 3, 4, 5)
SMALL_ROW, ZERO_ROW = 1, 2              # with three rows or more: row 1 has scale 1e-7 (where eps sits decides it), row 2 is all zero


def _norm_make(rows, dim):
    def make(g):
        x = _rn(g, rows, dim)
        x[:, -1] = 3.0
        if rows > ZERO_ROW:
            x[SMALL_ROW] *= 1e-7
            x[ZERO_ROW] = 0.0
        return {'x': x}
    return make


def norm_ref(x, kind, take_abs, defect=None):
    t, eps = x['x'], NORM_EPS[kind]
    l1 = (kind == 1) != (defect == 'l1 and l2 exchanged')
    n = t.abs().sum(-1, keepdim=True) if l1 else (t * t).sum(-1, keepdim=True).sqrt()
    if kind in (0, 1):
        d = torch.sqrt((t * t).sum(-1, keepdim=True) + eps) if defect == 'eps inside the sqrt' else n + eps
    elif kind == 2:
        d = torch.clamp(n, min=eps)
    else:
        d = n
    y = t / d
    return {'y': y.abs() if take_abs else y}


def _norm_add(kind, take_abs, rows, dim, lead=0):
    a = (kind, take_abs)
    named = {}
    if dim > 1:
        named['l1 and l2 exchanged'] = lambda x: norm_ref(x, *a, defect='l1 and l2 exchanged')
    if kind == 0 and rows > ZERO_ROW:
        named['eps inside the sqrt'] = lambda x: norm_ref(x, *a, defect='eps inside the sqrt')
    route = norm_route(dim, lead % 4 == 0)
    shape = {'kind': kind, 'abs': take_abs, 'rows': rows, 'dim': dim}
    if lead:
        shape['lead'] = lead
    _add('norm', shape, _norm_make(rows, dim), lambda x: norm_ref(x, *a), named, route=route,
         seams={'kind_abs': [(kind, take_abs)], 'dim': dim, 'rows': rows, 'route_kind': [(route, kind)],
                'route_dim': [(route, 'dim%4==0' if dim % 4 == 0 and dim <= 4096 else 'other')],
                'special_rows': [(kind, 'small and zero row')] if rows > ZERO_ROW else []},
         extra={'kind': kind, 'abs': take_abs, 'lead': lead})


for _kind in (0, 1, 2, 3):
    for _abs in (0, 1):
        for _di, _d in enumerate(NORM_DIM):
            _norm_add(_kind, _abs, NORM_ROW_COUNTS[(_di + _kind + 2 * _abs) % 4], _d)
    _norm_add(_kind, _kind % 2, 5, 256, lead=1)             # through ctypes: a view one float into its buffer
_seam('norm', kind_abs=[(k, a) for k in (0, 1, 2, 3) for a in (0, 1)], dim=NORM_DIM, rows=NORM_ROW_COUNTS,
      route_kind=[(r, k) for r in ('vec', 'scalar') for k in (0, 1, 2, 3)], route_dim=(('vec', 'dim%4==0'), ('scalar', 'dim%4==0'), ('scalar', 'other')),
      special_rows=[(k, 'small and zero row') for k in (0, 1, 2, 3)])
