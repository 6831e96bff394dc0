"""Case table of the training primitives (itr_amd/autograd.py over csrc/train*.hip) and their float64 references.

One entry per (op, shape): seeded CPU inputs, `ref` -- the operation written with plain torch ops, run under autograd in float64 for
the values and every input gradient and again in float32 for the reference's own rounding error e32 -- and `defect`, the float64
result with the LAST index of the reduced / tiled axis left out (sums lose their last term and keep their divisor; flat kernels lose
their last element).  Shapes sit on both sides of every seam of the launch geometry (256 threads, waves of 64, four rows per
workgroup, 64-column x 32-row BatchNorm blocks, float4 paths, grid-stride loops, optimizer block tables), and the inputs make the
last element decisive: a dropped one moves the result by far more than the bound.

Tolerance of a compared tensor (tests/test_train_primitives_gpu.py applies it, tests/test_train_primitive_cases.py proves that it
sees a one-element defect):
    primary    tol = 16 * max(e32, u * max|want|),  u = 2^-24
    exact      bit equality
(No case needs the issue's fallback, the a-priori bound n * u * S of a sequential sum: every sum here is within the primary rule.)
Nothing here imports the library: the table is checked on a machine without a GPU.
"""
import zlib

import torch

U = 2.0 ** -24
FACTOR = 16
SENSITIVITY = 10

SEAMS = {}          # op -> {parameter: values that must appear in the table}, filled next to the cases
CASES = []
_BY_NAME = {}


class Case(object):
    def __init__(self, op, shape, make, ref, grads=(), defect=None, exact=(), ignore=None, extra=None):
        self.op, self.shape, self.make, self.ref, self.grads = op, dict(shape), make, ref, tuple(grads)
        self.defect, self.exact, self.ignore, self.extra = defect, tuple(exact), dict(ignore or {}), extra
        self.name = op + "-" + "-".join("%s%s" % (k, v) for k, v in shape.items())
        self._cache = {}

    def __repr__(self):
        return self.name

    def inputs(self):
        if 'inp' not in self._cache:
            g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
            self._cache['inp'] = self.make(g)
        return self._cache['inp']

    def evaluate(self, dtype, fn=None):
        """{tensor: value} of `fn` (default: ref) in `dtype`: outputs and, for every name in grads, d_<name> of sum(out * g_<out>)."""
        x = {}
        for k, v in self.inputs().items():
            if torch.is_tensor(v) and v.is_floating_point():
                v = v.to(dtype).clone()
                if k in self.grads:
                    v.requires_grad_(True)
            x[k] = v
        out = (fn or self.ref)(x)
        res = {k: v.detach() for k, v in out.items()}
        if self.grads:
            loss = sum((out[k] * x['g_' + k]).sum() for k in out if out[k].requires_grad)
            for k, g in zip(self.grads, torch.autograd.grad(loss, [x[k] for k in self.grads])):
                res['d_' + k] = g
        return res

    def _masked(self, res):
        res = dict(res)
        for k, fn in self.ignore.items():
            if k in res:
                res[k] = torch.where(fn(self.inputs()), torch.zeros_like(res[k]), res[k])
        return res

    def mask(self, name, t):
        """`t` with the entries of tensor `name` that the case leaves out of the comparison set to zero."""
        if name in self.ignore:
            m = self.ignore[name](self.inputs())
            return torch.where(m.to(t.device), torch.zeros_like(t), t)
        return t

    def reference(self):
        """{tensor: (want float64, e32, tol, rule)}; computed once and shared."""
        if 'ref' in self._cache:
            return self._cache['ref']
        w64 = self._masked(self.evaluate(torch.float64))
        w32 = self._masked(self.evaluate(torch.float32))
        out = {}
        for k, want in w64.items():
            e32 = float((w32[k].double() - want).abs().max()) if want.numel() else 0.0
            if k in self.exact:
                out[k] = (want, e32, 0.0, 'exact')
            else:
                out[k] = (want, e32, FACTOR * max(e32, U * float(want.abs().max())), 'primary')
        self._cache['ref'] = out
        return out

    def defects(self):
        """{tensor: float64 result with the last index of the reduced / tiled axis left out}."""
        if self.defect is None:
            return {}
        x64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in self.inputs().items()}
        want = {k: v[0] for k, v in self.reference().items()}
        return self._masked(self.defect(self, x64, want))


def _add(op, shape, make, ref, **kw):
    c = Case(op, shape, make, ref, **kw)
    assert c.name not in _BY_NAME, c.name
    CASES.append(c)
    _BY_NAME[c.name] = c
    return c


def cases(*ops):
    return [c for c in CASES if c.op in ops]


def _rn(g, *shape):
    return torch.randn(*shape, generator=g)


def _seam(op, **params):
    SEAMS.setdefault(op, {}).update({k: sorted(set(v)) for k, v in params.items()})


def _zero_last(names):
    """Flat kernels: the last element of the last block is never written."""
    def defect(case, x, want):
        out = {}
        for k in names:
            d = want[k].clone()
            d.view(-1)[-1] = 0.0
            out[k] = d
        return out
    return defect


# --------------------------------------------------------------------------------------------------------------------
# flat elementwise kernels: one thread per element, 256 per workgroup
FLAT_N = (1, 255, 256, 257, 513)
_ACT_FN = {
    'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid,
    'leaky_relu': lambda t: torch.where(t > 0, t, 0.1 * t), None: lambda t: t,
}


def _flat_make(names, n):
    def make(g):
        d = {k: _rn(g, n) for k in names}
        for k in names:
            d[k][-1] = 1.25 if not k.startswith('g_') else -1.5          # the last element is far from zero in every output
        return d
    return make


for _n in FLAT_N:
    _add('mul', {'n': _n}, _flat_make(('a', 'b', 'g_y'), _n), lambda x: {'y': x['a'] * x['b']}, grads=('a', 'b'),
         defect=_zero_last(('y', 'd_a', 'd_b')))
    for _kind in ('relu', 'tanh', 'sigmoid', 'leaky_relu'):
        _add('act', {'kind': _kind, 'n': _n}, _flat_make(('x', 'g_y'), _n), (lambda fn: lambda x: {'y': fn(x['x'])})(_ACT_FN[_kind]),
             grads=('x',), defect=_zero_last(('y', 'd_x')), extra=_kind)
    _add('gelu', {'n': _n}, _flat_make(('x', 'g_y'), _n),
         lambda x: {'y': x['x'] * 0.5 * (1.0 + torch.erf(x['x'] / 2.0 ** 0.5))}, grads=('x',), defect=_zero_last(('y', 'd_x')))
_seam('mul', n=FLAT_N)
_seam('act', n=FLAT_N, kind=('relu', 'tanh', 'sigmoid', 'leaky_relu'))
_seam('gelu', n=FLAT_N)


def _gate_make(rows, dk):
    def make(g):
        d = {'q': _rn(g, rows, dk), 'k': _rn(g, rows, dk), 'M': torch.rand(rows, 2 * dk, generator=g) + 0.25,
             'g_qo': _rn(g, rows, dk), 'g_ko': _rn(g, rows, dk)}
        for k in ('q', 'k', 'g_qo', 'g_ko'):
            d[k][-1, -1] = 1.25
        return d
    return make


def _gate_ref(x):
    dk = x['q'].shape[1]
    return {'qo': x['q'] * x['M'][:, :dk], 'ko': x['k'] * x['M'][:, dk:]}


GATE_SHAPES = ((1, 1), (3, 85), (8, 32), (257, 1), (5, 33), (19, 27))
for _r, _d in GATE_SHAPES:
    _add('gate_apply', {'rows': _r, 'dk': _d}, _gate_make(_r, _d), _gate_ref, grads=('q', 'k', 'M'),
         defect=_zero_last(('qo', 'ko', 'd_q', 'd_k', 'd_M')))
_seam('gate_apply', n=[r * d for r, d in GATE_SHAPES])
assert set(r * d for r, d in GATE_SHAPES) >= set(FLAT_N)


GRU_E = 5


def _gru_make(B, H):
    def make(g):
        d = {'x': _rn(g, B, GRU_E), 'h': _rn(g, B, H), 'w_ih': _rn(g, 3 * H, GRU_E) * 0.4, 'w_hh': _rn(g, 3 * H, H) * (0.4 / H ** 0.5),
             'b_ih': _rn(g, 3 * H) * 0.2, 'b_hh': _rn(g, 3 * H) * 0.2, 'g_hn': _rn(g, B, H)}
        d['h'][-1, -1], d['g_hn'][-1, -1] = 1.5, -1.5
        return d
    return make


def _gru_ref(x):
    H = x['h'].shape[1]
    gi = x['x'] @ x['w_ih'].t() + x['b_ih']
    gh = x['h'] @ x['w_hh'].t() + x['b_hh']
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return {'hn': (1.0 - z) * n + z * x['h']}


GRU_SHAPES = ((1, 1), (4, 64), (3, 86), (7, 37))
for _b, _h in GRU_SHAPES:
    _add('gru_cell', {'B': _b, 'H': _h}, _gru_make(_b, _h), _gru_ref, grads=('x', 'h', 'w_ih', 'w_hh', 'b_ih', 'b_hh'),
         defect=_zero_last(('hn',)))
_seam('gru_cell', n=[b * h for b, h in GRU_SHAPES])

DROPOUT_N = (1, 255, 256, 257)
DROPOUT_P = (0.1, 0.5)


# --------------------------------------------------------------------------------------------------------------------
# one thread per column (256 per workgroup), blockIdx.y per batch item, a loop over the middle axis
COL_W = (1, 255, 256, 257, 513)
COL_MID = (1, 2, 37)
COL_B = (1, 3)
COL_SHAPES = [(3, 37, w) for w in COL_W] + [(b, m, 257) for b in COL_B for m in COL_MID if (b, m) != (3, 37)]


def _sum_mid_wo_last(t):
    return t[:, :-1].sum(1)


def _abm_make(B, N, H):
    def make(g):
        d = {'x': _rn(g, B, N, H), 'v': _rn(g, B, H), 'g_y': _rn(g, B, N, H)}
        d['x'][:, -1, :] = 0.75                 # the last middle index carries weight in dv for every activation
        d['v'][:] = d['v'].abs() * 0.5
        d['g_y'][:, -1, :] = 2.0
        return d
    return make


def _abm_defect(case, x, want):
    return {'d_v': _sum_mid_wo_last(want['d_x'])}


for _kind in (None, 'relu', 'tanh', 'sigmoid'):
    for _b, _m, _w in COL_SHAPES:
        _add('add_bcast_mid_act', {'kind': _kind, 'B': _b, 'N': _m, 'H': _w}, _abm_make(_b, _m, _w),
             (lambda fn: lambda x: {'y': fn(x['x'] + x['v'][:, None, :])})(_ACT_FN[_kind]), grads=('x', 'v'), defect=_abm_defect,
             extra=_kind)
_seam('add_bcast_mid_act', H=COL_W, N=COL_MID, B=COL_B, kind=('None', 'relu', 'tanh', 'sigmoid'))


# additive attention score: the forward is one wave per (b, n) row with a float4 path for H % 4 == 0, the backward one thread per column
ROW_ROWS = (1, 3, 4, 5)
ROW_H = (1, 63, 64, 65, 130, 257, 260)
_ROWS_AS_BN = {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5)}


def _aas_make(B, N, H):
    def make(g):
        d = {'x': _rn(g, B, N, H), 'v': _rn(g, B, H), 'w': _rn(g, H), 'g_e': _rn(g, B, N)}
        d['x'][:, :, -1], d['v'][:, -1], d['w'][-1] = 0.5, 0.5, 3.0          # the last column: w tanh(1) = 2.3 in every score
        d['g_e'][:, -1] = 2.0
        return d
    return make


def _aas_ref(x):
    return {'e': (torch.tanh(x['x'] + x['v'][:, None, :]) * x['w']).sum(-1)}


def _aas_defect(case, x, want):
    p = torch.tanh(x['x'] + x['v'][:, None, :])
    return {'e': (p * x['w'])[..., :-1].sum(-1), 'd_v': _sum_mid_wo_last(want['d_x']),
            'd_w': (x['g_e'][..., None] * p).sum(1)[:-1].sum(0)}


_AAS_SHAPES = list(COL_SHAPES) + [_ROWS_AS_BN[r] + (h,) for r in ROW_ROWS for h in ROW_H]
for _b, _m, _w in sorted(set(_AAS_SHAPES)):
    _add('addattn_score', {'B': _b, 'N': _m, 'H': _w}, _aas_make(_b, _m, _w), _aas_ref, grads=('x', 'v', 'w'), defect=_aas_defect)
_seam('addattn_score', H=COL_W + ROW_H, N=COL_MID, B=COL_B, rows=ROW_ROWS)


def _l2m_make(B, R, D):
    def make(g):
        d = {'x': _rn(g, B, R, D), 'g_z': _rn(g, B, R, D)}
        d['x'][:, -1, :] = 2.5
        if D > 1:
            d['x'][0, :, 0] = 0.0                   # a zero column: z = 0, finite gradient, left out of the gradient comparison
        return d
    return make


def _l2m_ref(x, drop=0):
    t = x['x']
    s = (t * t)[:, :t.shape[1] - drop].sum(1, keepdim=True)
    return {'z': t / (s.sqrt() + 1e-8)}


def _l2m_zero_col(inp):
    return ((inp['x'] * inp['x']).sum(1, keepdim=True) == 0).expand_as(inp['x'])


for _b, _m, _w in COL_SHAPES:
    _add('l2norm_mid', {'B': _b, 'R': _m, 'D': _w}, _l2m_make(_b, _m, _w), _l2m_ref, grads=('x',),
         defect=lambda case, x, want: {'z': _l2m_ref(x, 1)['z']}, ignore={'d_x': _l2m_zero_col})
_seam('l2norm_mid', D=COL_W, R=COL_MID, B=COL_B)


def _rmp_make(B, P, C):
    def make(g):
        d = {'x': _rn(g, B, P, C), 'g_y': _rn(g, B, C)}
        d['x'][-1, :, -1] = -d['x'][-1, :, -1].abs() - 0.1
        d['x'][-1, -1, -1] = 3.0                    # the winner of the last channel is the last position
        if C > 1:
            d['x'][:, :, 0] = -d['x'][:, :, 0].abs() - 0.1      # an all-negative channel: output 0, gradient 0
        d['g_y'][-1, -1] = 1.5
        return d
    return make


def _rmp_ref(x, drop=0):
    t = torch.relu(x['x'])
    t = t[:, :t.shape[1] - drop]
    if t.shape[1] == 0:
        return {'y': torch.zeros(t.shape[0], t.shape[2], dtype=t.dtype)}
    return {'y': t.max(1).values}


for _b, _m, _w in COL_SHAPES:
    _add('relu_maxpool', {'B': _b, 'npos': _m, 'C': _w}, _rmp_make(_b, _m, _w), _rmp_ref, grads=('x',),
         defect=lambda case, x, want: {'y': _rmp_ref(x, 1)['y']}, exact=('y', 'd_x'))
_seam('relu_maxpool', C=COL_W, npos=COL_MID, B=COL_B)


def _mm_make(B, R, F):
    def make(g):
        d = {'x': _rn(g, B, R, F), 'g_y': _rn(g, B, F)}
        d['x'][:, -1, :] = 3.0
        return d
    return make


for _b, _m, _w in COL_SHAPES:
    _add('mean_mid', {'B': _b, 'R': _m, 'F': _w}, _mm_make(_b, _m, _w), lambda x: {'y': x['x'].mean(1)}, grads=('x',),
         defect=lambda case, x, want: {'y': x['x'][:, :-1].sum(1) / x['x'].shape[1]})
_seam('mean_mid', F=COL_W, R=COL_MID, B=COL_B)


def _gm_make(Ni, k, Nc):
    def make(g):
        d = {'T': _rn(g, Ni * k, Nc), 'g_S': _rn(g, Ni, Nc)}
        d['T'][-1, -1] = 6.0                        # the last view wins the last column of the last image
        return d
    return make


def _gm_ref(x, k, drop=0):
    T = x['T'].view(-1, k, x['T'].shape[1])[:, :k - drop]
    if T.shape[1] == 0:
        return {'S': torch.full((T.shape[0], T.shape[2]), float('-inf'), dtype=T.dtype)}
    return {'S': T.max(1).values}


for _b, _m, _w in COL_SHAPES:
    _add('group_max', {'Ni': _b, 'k': _m, 'Nc': _w}, _gm_make(_b, _m, _w), (lambda k: lambda x: _gm_ref(x, k))(_m), grads=('T',),
         defect=(lambda k: lambda case, x, want: {'S': _gm_ref(x, k, 1)['S']})(_m), exact=('S', 'd_T'), extra=_m)
_seam('group_max', Nc=COL_W, k=COL_MID, Ni=COL_B)

MVM_D = 8


def _mvm_make(Ni, k, Nc):
    def make(g):
        d = {'img': _rn(g, Ni, k, MVM_D), 'cap': _rn(g, Nc, MVM_D), 'g_S': _rn(g, Ni, Nc)}
        d['img'][-1, -1], d['cap'][-1] = 1.5, 1.5   # the last view of the last image wins the last caption by a wide margin
        return d
    return make


def _mvm_ref(x, drop=0):
    Ni, k, D = x['img'].shape
    T = (x['img'].reshape(Ni * k, D) @ x['cap'].t()).view(Ni, k, -1)
    return {'S': T[:, :k - drop].max(1).values}


for _b, _m, _w in ((3, 2, 257), (1, 37, 255)):
    _add('mvm_scores', {'Ni': _b, 'k': _m, 'Nc': _w}, _mvm_make(_b, _m, _w), _mvm_ref, grads=('img', 'cap'),
         defect=lambda case, x, want: {'S': _mvm_ref(x, 1)['S']})


# --------------------------------------------------------------------------------------------------------------------
# one wave per row, four rows per workgroup
def _ln_make(rows, H, res):
    def make(g):
        d = {'x': _rn(g, rows, H), 'gamma': torch.rand(H, generator=g) + 0.5, 'beta': _rn(g, H) * 0.1, 'g_y': _rn(g, rows, H)}
        if res:
            d['res'] = _rn(g, rows, H)
            d['res'][:, -1] = 1.0
        d['x'][:, -1] = 4.0                         # the last column is an outlier of every row
        return d
    return make


def _ln_ref(x, drop=0):
    z = x['x'] + x['res'] if 'res' in x else x['x']
    H = z.shape[1]
    u = z[:, :H - drop].sum(1, keepdim=True) / H
    q = ((z - u) ** 2)[:, :H - drop].sum(1, keepdim=True) / H
    return {'y': x['gamma'] * ((z - u) / torch.sqrt(q + 1e-12)) + x['beta']}


for _res in (True, False):
    for _r in ROW_ROWS:
        for _h in ROW_H:
            _gr = (('x', 'res') if _res else ('x',)) + ('gamma', 'beta')
            _add('add_layernorm', {'res': int(_res), 'rows': _r, 'H': _h}, _ln_make(_r, _h, _res), _ln_ref,
                 grads=_gr if _h > 1 else (),        # H = 1: the variance is 0 -- values only
                 defect=lambda case, x, want: {'y': _ln_ref(x, 1)['y']})
_seam('add_layernorm', rows=ROW_ROWS, H=ROW_H, res=(0, 1))


def _l2r_make(rows, dim):
    def make(g):
        d = {'x': _rn(g, rows, dim), 'g_z': _rn(g, rows, dim)}
        d['x'][:, -1] = 3.0
        return d
    return make


def _l2r_ref(x, drop=0):
    t = x['x']
    return {'z': t / ((t * t)[:, :t.shape[1] - drop].sum(1, keepdim=True).sqrt() + 1e-8)}


L2R_DIM = (1, 63, 64, 65, 257, 1025)
for _d in L2R_DIM:
    _add('l2norm_rows', {'rows': 5, 'dim': _d}, _l2r_make(5, _d), _l2r_ref, grads=('x',),
         defect=lambda case, x, want: {'z': _l2r_ref(x, 1)['z']})
_seam('l2norm_rows', dim=L2R_DIM)


# --------------------------------------------------------------------------------------------------------------------
# one workgroup per row: log-softmax + masked NLL
NLL_V = (1, 63, 64, 65, 255, 256, 257, 513)
NLL_B = (1, 7)


def _nll_make(B, V):
    def make(g):
        lg = _rn(g, B, V) * 3.0
        tgt = torch.randint(0, V, (B,), generator=g)
        mask = torch.ones(B)
        lg[0, -1] = lg[0].max() + 2.0               # row 0: the row maximum is the last column
        tgt[0] = V - 1
        if B > 2:
            tgt[0] = 0
            tgt[1] = V - 1                          # row 1: the target is the last column
            sign = torch.where(torch.rand(V, generator=g) < 0.5, -1.0, 1.0)
            lg[2] = 80.0 * sign                     # row 2: without the row maximum subtracted exp() overflows in float32
            lg[2, -1] = 80.0
            mask[3], mask[B - 1] = 0.0, 0.0
        d = {'logits': lg, 'target': tgt, 'mask': mask, 'g_loss': _rn(g, B)}
        d['g_loss'][:3] = 1.5
        return d
    return make


def _nll_ref(x, drop=0):
    lg = x['logits']
    V = lg.shape[1]
    part = lg[:, :V - drop]
    if part.shape[1] == 0:
        lse = torch.full((lg.shape[0],), float('-inf'), dtype=lg.dtype)
    else:
        m = part.max(1).values
        lse = m + torch.log(torch.exp(part - m[:, None]).sum(1))
    picked = lg.gather(1, x['target'][:, None])[:, 0]
    return {'loss': torch.where(x['mask'] != 0, -(picked - lse) * x['mask'], torch.zeros_like(lse))}


for _b in NLL_B:
    for _v in NLL_V:
        _add('nll_logsoftmax', {'B': _b, 'V': _v}, _nll_make(_b, _v), _nll_ref, grads=('logits',),
             defect=lambda case, x, want: {'loss': _nll_ref(x, 1)['loss']})
_seam('nll_logsoftmax', V=NLL_V, B=NLL_B)


# --------------------------------------------------------------------------------------------------------------------
# BatchNorm1d, training mode: 64-column blocks x row slices, 32-row unrolled loop + remainder, two-stage reduction over the slices
BN_MAXSLICES = 64


def bn_slices(N, C):
    """The row slices the library cuts N rows into (csrc/train_camera.hip: bn_slices) and the rows of each."""
    col_blocks = -(-C // 64)
    s = min(-(-1024 // col_blocks), -(-N // 256), BN_MAXSLICES)
    s = max(s, 1)
    per = -(-N // s)
    return s, [max(0, min(N, (i + 1) * per) - i * per) for i in range(s)]


BN_EPS, BN_MOM = 1e-5, 0.1
BN_SHAPES = ((2, 1), (31, 64), (32, 65), (33, 63), (257, 65), (513, 3), (16385, 2))


def _bn_make(N, C):
    def make(g):
        d = {'x': _rn(g, N, C) * 2.0 + 0.5, 'gamma': torch.rand(C, generator=g) + 0.5, 'beta': _rn(g, C) * 0.1,
             'rm': _rn(g, C) * 0.1, 'rv': torch.rand(C, generator=g) + 0.5, 'g_y': _rn(g, N, C)}
        if N > 2:
            body = d['x'][:-1]
            d['x'][-1] = body.mean(0) + 3.0 * body.std(0)          # the last row: an outlier of 3 sigma in every column
        d['g_y'][-1] = 3.0
        return d
    return make


def _bn_ref(x, drop=0):
    t = x['x']
    N = t.shape[0]
    mean = t[:N - drop].sum(0) / N
    var = ((t - mean) ** 2)[:N - drop].sum(0) / N
    y = (t - mean) / torch.sqrt(var + BN_EPS) * x['gamma'] + x['beta']
    return {'y': y, 'running_mean': ((1 - BN_MOM) * x['rm'] + BN_MOM * mean).detach(),
            'running_var': ((1 - BN_MOM) * x['rv'] + BN_MOM * var * (N / max(N - 1, 1))).detach()}


def _bn_defect(case, x, want):
    d = _bn_ref(x, 1)
    xhat = (x['x'] - x['x'].mean(0)) / torch.sqrt(x['x'].var(0, unbiased=False) + BN_EPS)
    return {'y': d['y'], 'running_mean': d['running_mean'], 'running_var': d['running_var'],
            'd_beta': x['g_y'][:-1].sum(0), 'd_gamma': (x['g_y'] * xhat)[:-1].sum(0)}


for _n, _c in BN_SHAPES:
    _add('batch_norm_train', {'N': _n, 'C': _c}, _bn_make(_n, _c), _bn_ref, grads=('x', 'gamma', 'beta'), defect=_bn_defect)
_seam('batch_norm_train', N=[n for n, _ in BN_SHAPES], C=[c for _, c in BN_SHAPES])


# --------------------------------------------------------------------------------------------------------------------
# multi-view summary: softmax over the regions in LDS (at most 192 x 192), one thread per feature column
SMRY_SHAPES = ((1, 1, 1, 1), (2, 36, 12, 257), (2, 37, 65, 64), (1, 96, 96, 70), (1, 192, 192, 8),
               (1, 5, 3, 255), (3, 2, 5, 256), (1, 5, 3, 513))          # the last three: the feature axis of dx at the column kernels' widths
SMRY_LIMIT = 192


def _smry_make(B, R, K, D):
    def make(g):
        d = {'smry': _rn(g, B, R, K), 'x': _rn(g, B, R, D), 'g_out': _rn(g, B, K, D)}
        d['smry'][:, -1, :] = 3.0                   # the last region holds a large share of every view
        d['x'][:, -1, :] = 2.0
        d['g_out'][:, -1, :] = 1.5
        return d
    return make


def _smry_ref(x, drop=0):
    L = torch.softmax(x['smry'], 1)
    R = L.shape[1]
    return {'out': L[:, :R - drop].transpose(1, 2) @ x['x'][:, :R - drop]}


def _smry_defect(case, x, want):
    L = torch.softmax(x['smry'], 1)
    return {'out': _smry_ref(x, 1)['out'], 'd_x': L[:, :, :-1] @ x['g_out'][:, :-1]}


for _s in SMRY_SHAPES:
    _add('summarize', dict(zip('BRKD', _s)), _smry_make(*_s), _smry_ref, grads=('smry', 'x'), defect=_smry_defect)
_seam('summarize', R=[s[1] for s in SMRY_SHAPES], K=[s[2] for s in SMRY_SHAPES], D=[s[3] for s in SMRY_SHAPES])


# --------------------------------------------------------------------------------------------------------------------
# short-sequence attention: one workgroup per (sequence, head), at most 64 positions and a head size of at most 64
MHA_SHAPES = ((1, 1, 1, 1), (2, 63, 3, 5), (1, 64, 2, 64), (3, 17, 1, 33))
MHA_LIMIT = 64


def _mha_make(B, L, heads, dk, masked):
    def make(g):
        A = heads * dk
        d = {'qkv': _rn(g, B * L, 3 * A), 'g_out': _rn(g, B * L, A)}
        d['qkv'][:, 2 * A:].view(B, L, A)[:, -1] = 2.0           # the last key's value row stands out
        if masked:
            m = (torch.rand(B, L, generator=g) < 0.7).float()
            m[:, 0], m[:, -1] = 1.0, 1.0
            if B > 1:
                m[0] = 0.0
                m[0, 0] = 1.0                                       # one sequence keeps only position 0
            d['mask'] = m
        return d
    return make


def _mha_ref(x, heads, drop=0):
    A = x['qkv'].shape[1] // 3
    B = x['mask'].shape[0] if 'mask' in x else x['B']
    L, dk = x['qkv'].shape[0] // B, A // heads
    q, k, v = (x['qkv'][:, i * A:(i + 1) * A].reshape(B, L, heads, dk).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(2, 3) / dk ** 0.5
    if 'mask' in x:
        s = s + (1.0 - x['mask'])[:, None, None, :] * -10000.0
    P = torch.softmax(s, -1)
    out = P[..., :L - drop] @ v[:, :, :L - drop]
    return {'out': out.permute(0, 2, 1, 3).reshape(B * L, A)}


for _s in MHA_SHAPES:
    for _masked in (0, 1):
        _mk = _mha_make(*_s, masked=_masked)
        _add('mha', dict(zip(('B', 'L', 'heads', 'dk'), _s), mask=_masked),
             (lambda mk, B: lambda g: dict(mk(g), B=B))(_mk, _s[0]),
             (lambda h: lambda x: _mha_ref(x, h))(_s[2]), grads=('qkv',),
             defect=(lambda h: lambda case, x, want: {'out': _mha_ref(x, h, 1)['out']})(_s[2]), extra=_s)
_seam('mha', L=[s[1] for s in MHA_SHAPES], dk=[s[3] for s in MHA_SHAPES], mask=(0, 1))


# --------------------------------------------------------------------------------------------------------------------
# small batched products; (1, 129, 128, 3) has more outputs than the 64 x 256 threads of the thread-per-output kernel's largest grid, so
# that its grid-stride loop takes a second pass (bmm_nt with more than 64 output columns runs on that kernel)
BMM_SHAPES = ((1, 1, 1, 1), (3, 9, 11, 14), (2, 16, 17, 257), (1, 65, 65, 3), (1, 129, 128, 3))
BMM_SMALL_MAX_GRID = 64 * 256


def _bmm_make(Bn, M, N, K, nt):
    def make(g):
        d = {'A': _rn(g, Bn, M, K), 'B': _rn(g, Bn, N, K) if nt else _rn(g, Bn, K, N), 'g_C': _rn(g, Bn, M, N)}
        d['A'][:, :, -1] = 2.0
        if nt:
            d['B'][:, :, -1] = 2.0
        else:
            d['B'][:, -1, :] = 2.0
        return d
    return make


def _bmm_ref(x, nt, drop=0):
    K = x['A'].shape[2]
    A = x['A'][:, :, :K - drop]
    Bm = x['B'][:, :, :K - drop].transpose(1, 2) if nt else x['B'][:, :K - drop]
    return {'C': A @ Bm}


for _nt in (0, 1):
    for _s in BMM_SHAPES:
        _add('bmm_nt' if _nt else 'bmm_nn', dict(zip(('batch', 'M', 'N', 'K'), _s)), _bmm_make(*_s, nt=_nt),
             (lambda nt: lambda x: _bmm_ref(x, nt))(_nt), grads=('A', 'B'),
             defect=(lambda nt: lambda case, x, want: {'C': _bmm_ref(x, nt, 1)['C']})(_nt))
    _seam('bmm_nt' if _nt else 'bmm_nn', K=[s[3] for s in BMM_SHAPES], M=[s[1] for s in BMM_SHAPES])


# --------------------------------------------------------------------------------------------------------------------
# rows and columns: 64 x 64 transpose tiles, column sums over 32-row partials (16 loads in flight), row gather / embedding scatter
RC = (1, 31, 32, 33, 63, 64, 65, 257)


def _t2d_make(r, c):
    return lambda g: {'x': _rn(g, r, c)}


for _r in RC:
    for _c in RC:
        _add('transpose2d', {'rows': _r, 'cols': _c}, _t2d_make(_r, _c), lambda x: {'y': x['x'].t().contiguous()}, exact=('y',))
_seam('transpose2d', rows=RC, cols=RC)


def _cs_make(r, c, acc):
    def make(g):
        d = {'x': _rn(g, r, c)}
        d['x'][-1] = 3.0
        if acc:
            d['out0'] = _rn(g, c)
        return d
    return make


def _cs_ref(x, drop=0):
    s = x['x'][:x['x'].shape[0] - drop].sum(0)
    return {'y': s + x['out0'] if 'out0' in x else s}


COLSUM_SHAPES = [(r, c, 0) for r in RC for c in RC] + [(513, 33, 0), (4097, 33, 0), (4097, 257, 1), (33, 65, 1)]
for _r, _c, _acc in COLSUM_SHAPES:
    _add('colsum', {'rows': _r, 'cols': _c, 'acc': _acc}, _cs_make(_r, _c, _acc), _cs_ref,
         defect=lambda case, x, want: {'y': _cs_ref(x, 1)['y']})
_seam('colsum', rows=RC + (4097,), cols=RC, acc=(0, 1))

GATHER_E = (1, 127, 128, 129, 300)
GATHER_ROWS, GATHER_N, GATHER_DUP = 40, 513, 400


def _gr_make(E):
    def make(g):
        idx = torch.randint(0, GATHER_ROWS, (GATHER_N,), generator=g)
        pos = torch.randperm(GATHER_N, generator=g)[:GATHER_DUP]
        idx[pos] = 7                                # one row 400 times: its gradient is the sum of 400 rows
        idx[-1] = 7
        d = {'x': _rn(g, GATHER_ROWS, E), 'idx': idx, 'g_y': _rn(g, GATHER_N, E)}
        d['g_y'][-1] = 4.0
        return d
    return make


def _gr_defect(case, x, want):
    d = want['d_x'].clone()
    d[x['idx'][-1]] -= x['g_y'][-1]                 # the last index entry never scattered
    return {'d_x': d}


for _e in GATHER_E:
    _add('gather_rows', {'E': _e}, _gr_make(_e), lambda x: {'y': x['x'][x['idx']]}, grads=('x',), defect=_gr_defect, exact=('y',))
_seam('gather_rows', E=GATHER_E)


# --------------------------------------------------------------------------------------------------------------------
# optimizer: clip_grad_norm_ + Adam over a list of tensors (block tables of the two multi-tensor launches)
SQ_SUM_ELEMS_PER_BLOCK = 256 * 8            # itr_sq_sum_blocks(n) = min(ceil(n / 2048), 1024): 2048 -> 1 block, 2049 -> 2
ADAM_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, SQ_SUM_ELEMS_PER_BLOCK, SQ_SUM_ELEMS_PER_BLOCK + 1, 65537)
ADAM_ONES = 40
ADAM_STEPS, ADAM_MAX_NORM, ADAM_LR = 3, 2.0, 1e-3
ADAM_MIN_G = 2.0 ** -6                       # exact in float32, >= 0.01


def adam_problem():
    """Parameters and per-step gradients.  The list: the sizes above but the largest, a tensor that never gets a gradient, forty
    one-element tensors, the 65537-element tensor.  Every gradient element has |g| >= 0.01.  Step 1 has a norm far above max_norm
    (clipped).  With |g| >= 0.01 the 65537 elements alone have a norm of 2.56 > max_norm, so in steps 2 and 3 -- which are not
    clipped -- the largest tensor has no gradient (the block tables are rebuilt for the smaller set; torch skips it likewise).  The
    last gradient element of every tensor is decisive: 1.5 in step 1 and 0.05 later, with one sign per tensor over the steps, so that
    an update skipped for it moves the parameter and both moments by far more than their bounds; the very last element of a step is
    large enough to show in the norm.  (ag.Adam counts one step for all tensors where torch counts per parameter; no tensor here gets
    its first gradient after step 1, so the two counts agree.)"""
    g = torch.Generator().manual_seed(20260)
    sizes = list(ADAM_SIZES[:-1]) + [33] + [1] * ADAM_ONES + [ADAM_SIZES[-1]]
    no_grad = len(ADAM_SIZES) - 1
    params = [_rn(g, n) for n in sizes]
    signs = torch.where(torch.rand(len(sizes), generator=g) < 0.5, -1.0, 1.0)
    grads = []
    for step in range(ADAM_STEPS):
        gs = []
        for i, n in enumerate(sizes):
            if i == no_grad or (step > 0 and i == len(sizes) - 1):
                gs.append(None)
                continue
            t = _rn(g, n) * (1.0 if step == 0 else 0.012)
            t = torch.where(t.abs() < ADAM_MIN_G, torch.where(t < 0, -ADAM_MIN_G, ADAM_MIN_G), t)
            t[-1] = signs[i] * (1.5 if step == 0 else 0.05)
            gs.append(t)
        last = [t for t in gs if t is not None][-1]
        last[-1] = 6.0 if step == 0 else 0.5
        grads.append(gs)
    return params, grads


def adam_reference(dtype, drop_last=False, skip_last=False):
    """Three steps of clip_grad_norm_(max_norm) + torch.optim.Adam on the CPU in `dtype` -> per step (params, exp_avg, exp_avg_sq, norm).
    drop_last: the norm of every step misses the last element of the last tensor.  skip_last: the update of every step skips the last
    element of every tensor (the last thread of its last block): parameter and moments keep their values there."""
    params, grads = adam_problem()
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = torch.optim.Adam(ps, lr=ADAM_LR)
    steps = []
    for gs in grads:
        for p, gr in zip(ps, gs):
            p.grad = None if gr is None else gr.to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, ADAM_MAX_NORM)
        if drop_last:
            have = [gr.to(dtype) for gr in gs if gr is not None]
            norm = torch.sqrt(sum((gr ** 2).sum() for gr in have) - have[-1][-1] ** 2)
        keep = [(p, p.data[-1].clone(), [opt.state[p][k][-1].clone() if k in opt.state[p] else None for k in ('exp_avg', 'exp_avg_sq')])
                for p in ps if p.grad is not None]
        opt.step()
        if skip_last:
            for p, p_last, (m_last, v_last) in keep:
                p.data[-1] = p_last
                opt.state[p]['exp_avg'][-1] = 0.0 if m_last is None else m_last
                opt.state[p]['exp_avg_sq'][-1] = 0.0 if v_last is None else v_last
        zeros = [torch.zeros_like(p.data) for p in ps]
        steps.append(([p.data.clone() for p in ps],
                      [opt.state[p]['exp_avg'].clone() if p in opt.state and 'exp_avg' in opt.state[p] else z for p, z in zip(ps, zeros)],
                      [opt.state[p]['exp_avg_sq'].clone() if p in opt.state and 'exp_avg_sq' in opt.state[p] else z for p, z in zip(ps, zeros)],
                      norm.detach().reshape(1).clone()))
    return steps


def tolerance(want64, got32):
    """The primary rule for tensors outside the table (the optimizer): (e32, tol)."""
    e32 = float((got32.double() - want64).abs().max())
    return e32, FACTOR * max(e32, U * float(want64.abs().max()))
